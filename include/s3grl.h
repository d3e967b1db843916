/*
 * s3grl.h — C ABI of libs3grl_hip.so, the MI355X (gfx950) S3GRL operator-precompute engine.
 *
 * This is the drop-in boundary for ONE path of venomouscyanide/S3GRL: the per-link PoS /
 * PoS Plus / SoP operator precompute that `utils.extract_enclosing_subgraphs`
 * (reference utils.py:446-554) dispatches to
 *     OptimizedSignOperations.get_PoS_prepped_ds       (reference tuned_SIGN.py:137-189)
 *     OptimizedSignOperations.get_PoS_Plus_prepped_ds  (reference tuned_SIGN.py:192-262)
 *     OptimizedSignOperations.get_SoP_prepped_ds       (reference tuned_SIGN.py:49-134)
 * including the k-hop extraction they call (reference utils.py:33-85) and, for SoP, the global
 * operator setup of `SEALDataset.process` (reference sgrl_link_pred.py:161-178).
 *
 * The reference is pure Python and has no FFI of its own; a maintainer binds these entry
 * points with ctypes from `tuned_SIGN.py` (stub in INTEGRATION.md).  All pointers are plain
 * DEVICE pointers unless a parameter says "host"; no torch / PyG types cross this boundary.
 * Every function returns an s3grl_status; nothing is printed, nothing throws.
 *
 * Output contract (what reference models.py:372 `torch.cat(xs, dim=-1)` feeds the MLP):
 *     rows     fp32 [total_rows, sign_k+1, 1+F]   operator 0 is x itself, column 0 the label
 *                                                  column z (1 for src/dst rows, else 0)
 *     row_ptr  int64 [L+1]                         rows of link l are row_ptr[l]..row_ptr[l+1];
 *                                                  first two are src, dst; PoS Plus appends the
 *                                                  common-neighbour rows in ascending node id
 * Thread-compatibility: one context per host thread / stream; contexts share nothing.
 */
#ifndef S3GRL_H_
#define S3GRL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S3GRL_ABI_VERSION 6

typedef enum s3grl_status {
  S3GRL_OK = 0,
  S3GRL_ERR_INVALID_ARGUMENT = 1, /* null pointer, negative size, sign_k < 1, link id out of range,
                                     malformed CSR (indptr not monotone, column id outside
                                     [0,N), a row not strictly ascending) */
  S3GRL_ERR_NOT_IMPLEMENTED = 2,  /* maps to the reference's NotImplementedError:
                                     k_node_set_strategy other than "intersection"
                                     (tuned_SIGN.py:235; "union" is unusable as shipped),
                                     SoP on a directed graph */
  S3GRL_ERR_NO_FEATURES = 3,      /* X == NULL: the reference's `assert subgraph_features is not
                                     None` (tuned_SIGN.py:166,221) */
  S3GRL_ERR_OUT_OF_MEMORY = 4,
  S3GRL_ERR_HIP = 5,              /* a HIP runtime call failed; see s3grl_last_error() */
  S3GRL_ERR_NO_DEVICE = 6,        /* no gfx950 device visible */
  S3GRL_ERR_GRAPH_TOO_LARGE = 7,  /* nnz or num_nodes >= 2^31, nothing else.  No plan has a node limit: beyond
                                     ~327 680 nodes the N-bit bitmaps of the sizing pass, of the overflow class
                                     and of the SoP scalar kernel live in HBM slices instead of LDS.  A SoP ball
                                     has no size limit either: one that does not fit LDS is formed in an HBM
                                     workspace (S3GRL_ERR_OUT_OF_MEMORY when not even one ball's slice can be
                                     allocated) */
  S3GRL_ERR_SELF_LINK = 8         /* src == dst: the reference duplicates the node; unsupported */
} s3grl_status;

typedef enum s3grl_mode {
  S3GRL_MODE_POS = 0,      /* get_PoS_prepped_ds       : rows {src,dst} */
  S3GRL_MODE_POS_PLUS = 1, /* get_PoS_Plus_prepped_ds  : rows {src,dst} + N(src) ∩ N(dst) */
  S3GRL_MODE_SOP = 2,      /* get_SoP_prepped_ds       : global operators, rows {src,dst} */
  S3GRL_MODE_SOP_RESTRICTED = 3 /* NOT a reference flow (its SoP ignores num_hops, tuned_SIGN.py:49-134): the SoP rows
                              with every operator row restricted to the num_hops-ball of {src,dst} — the optional
                              twin BASELINE config 3 ("2-hop subgraphs") and SURVEY §8(d) name, reported separately.
                              x_i[s] = [Â^i[s,s] | Σ_{w in ball, w != d} Â^i[s,w] X[w]] with the GLOBAL Â; through
                              s3grl_plan_create / s3grl_run like PoS; needs sign_k - 1 <= num_hops */
} s3grl_mode;

typedef enum s3grl_strategy {
  S3GRL_STRATEGY_INTERSECTION = 0, /* sign_kwargs['k_node_set_strategy'] == 'intersection' */
  S3GRL_STRATEGY_UNION = 1         /* accepted by the reference's parser, broken in its code */
} s3grl_strategy;

/* s3grl_cfg.flags */
#define S3GRL_FLAG_FULL_STATS 1u /* per-link diagnostics: exact total_sub_edges even when
                                    sign_k < num_hops, subgraph export for every link (turns
                                    the folding of reversed duplicates off) */
#define S3GRL_FLAG_NO_FOLD 2u    /* do not serve (d,s) from the extraction of (s,d) */
#define S3GRL_FLAG_COUNT_ONLY 4u /* sizing pass only: the plan holds the subgraph sizes (node_ptr of
                                    s3grl_plan_export_subgraphs, total_nodes / max_nodes / total_rows
                                    of the stats) and nothing else; it cannot be run.  Used to
                                    balance the shards of a multi-GPU job by exact subgraph size.
                                    Reversed duplicates are folded like in a full plan (size 0 for
                                    the folded link) unless S3GRL_FLAG_NO_FOLD is set too */

/* sign_kwargs / call arguments of the reference operators (tuned_SIGN.py:137-138,145,200,229) */
typedef struct s3grl_cfg {
  int32_t mode;      /* s3grl_mode */
  int32_t num_hops;  /* k of the k-hop enclosing subgraph (ignored for SoP, like the reference) */
  int32_t sign_k;    /* number of operators K >= 1 */
  int32_t strategy;  /* s3grl_strategy, PoS Plus only */
  int32_t directed;  /* 1 iff the graph was made by s3grl_graph_create_directed (A and A_csc) */
  uint32_t flags;    /* S3GRL_FLAG_* */
  int32_t rw_m;      /* ScaLed subgraphs (reference utils.py:86-150, rw_kwargs): rw_M random walks */
  int32_t rw_M;      /*   of length rw_m per node, drawn by the engine, replace the BFS (num_hops is
                          then ignored, like in the reference); 0 = k-hop BFS.  Walk node sets cached
                          by the caller: s3grl_plan_create_sets */
  uint32_t seed;     /* seed of the engine's own counter-based generator (walks, hop sampling) */
  int32_t max_nodes_per_hop; /* utils.py:68-70: keep at most this many nodes of every hop;
                                0 = no cap (None) */
  double ratio_per_hop;      /* utils.py:66-67: keep int(ratio * |fringe|) nodes of every hop
                                (before the cap), uniformly; >= 1.0 = keep all (every paper
                                config).  A double, like the Python float whose product is
                                truncated.  Offset 40. */
  int32_t reserved[4];       /* must be 0 */
} s3grl_cfg;

/* sizes a plan measured while extracting; the benchmark's algorithmic-bytes figure
 * (B_link = 8n + 4 vol(S) + 4 n F + 4 R (K+1)(1+F)) is computed from these. */
typedef struct s3grl_plan_stats {
  int64_t num_links;
  int64_t total_rows;       /* ΣR */
  int64_t total_nodes;      /* Σ n        subgraph nodes over all links */
  int64_t total_volume;     /* Σ vol(S)   global degrees of those nodes */
  int64_t total_sub_edges;  /* Σ e        directed entries of the masked induced sub-CSRs */
  int64_t total_support;    /* Σ over row pairs of nodes with a non-zero operator coefficient */
  int64_t num_row_pairs;    /* gather jobs */
  int64_t max_nodes;        /* max n */
  int64_t workspace_bytes;  /* device bytes held by the plan + context arena */
  int64_t folded_links;     /* links (d,s) served by the extraction of their reversed duplicate
                               (s,d) earlier in the list: same subgraph, rows swapped.  The
                               totals above count them like any other link (algorithmic). */
  int64_t extracted_nodes;  /* Σ n over the links actually extracted */
  int64_t oriented_entries; /* one-hop plans on big graphs: Σ over the extracted links of the degree-oriented
                               row entries of their subgraph's nodes, hub_links excepted (what link_full_kernel probes: the
                               physical counterpart of total_volume); 0 for other plans */
  int64_t hub_links;        /* ... of which: links served from a cached hub neighbourhood (link_hub_kernel:
                               the induced adjacency of a hub's neighbours is built once per graph and
                               shared by all of the hub's links); their oriented rows are NOT probed */
  int64_t hub_read_bytes;   /* bytes those links requested: the two endpoint rows, the rows of the nodes
                               only the non-hub endpoint brings (bounds + entries), the cached rows staged */
  int64_t hub_endpoint_entries; /* Σ deg(src) + deg(dst) over those links (their share of the endpoint rows) */
  int64_t hub_nodes;        /* Σ n over those links (their share of extracted_nodes) */
} s3grl_plan_stats;

typedef struct s3grl_context s3grl_context; /* device, stream, workspace arena */
typedef struct s3grl_graph s3grl_graph;     /* structure of the train graph A (values ignored,
                                               exactly as ssp.find -> SparseTensor(row, col)
                                               ignores them, tuned_SIGN.py:153-156) */
typedef struct s3grl_plan s3grl_plan;       /* extraction + operator coefficients of one call */
typedef struct s3grl_sop s3grl_sop;         /* SoP global state: Â, Y_i = Â^i X */
typedef struct s3grl_features s3grl_features; /* X prepared for the gather (dense or sparse rows) */

int32_t s3grl_abi_version(void);
const char* s3grl_status_string(s3grl_status s);
/* message of the last failing call on this host thread (HIP error text), never NULL */
const char* s3grl_last_error(void);

/* `stream` is a hipStream_t passed as void* (NULL = the legacy default stream). */
s3grl_status s3grl_context_create(int32_t device, void* stream, s3grl_context** out);
s3grl_status s3grl_context_destroy(s3grl_context* ctx);
/* Loads the library's GPU code now instead of at the first launch of each kernel family (HIP loads a code
 * object lazily: ~16 ms of a process's first s3grl_graph_create and ~7-20 ms of its first plan + run are that,
 * whatever the size of the graph).  units: bit 0 = what every PoS / PoS Plus call at sign_k 3 or 4 needs, bit 1 =
 * the link kernels of the other sign_k, bit 2 = SoP and the pooling; ms (host double [16], may be NULL) =
 * milliseconds per unit.  Optional — nothing depends on it; a host thread can call it while the caller still
 * loads its dataset (s3grl_amd.tuned_SIGN does at import). */
s3grl_status s3grl_context_preload(s3grl_context* ctx, uint32_t units, double* ms);

/* CSR of A as scipy holds it (reference sgrl_link_pred.py:111-114): indptr [N+1], indices
 * [nnz] strictly ascending within a row (canonical format: sorted, duplicates summed); the
 * matrix must be structurally symmetric (undirected train graph).  The arrays are copied; the
 * caller may free them afterwards.  The structure is validated on the device (indptr[0] == 0,
 * indptr monotone and ending at nnz, ids in [0,N), rows strictly ascending):
 * S3GRL_ERR_INVALID_ARGUMENT otherwise.  Symmetry is the caller's promise (the Python binding
 * checks it). */
s3grl_status s3grl_graph_create(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr,
                                const int32_t* indices, int64_t nnz, s3grl_graph** out);
/* A DIRECTED graph, as the reference holds it when `directed` is set (sgrl_link_pred.py:107-119: A from the
 * directed edge_index, A_csc = A.tocsc(); only ogbl-citation2 of the reference's datasets): both forms
 * of the same nnz arcs — csr_* the successors of every node, csc_* the predecessors (scipy's CSC arrays
 * as they are: indptr over columns, row ids ascending).  Plans on such a graph need s3grl_cfg.directed
 * = 1: the BFS follows successors and predecessors (utils.py:58-63), the induced matrix keeps the
 * directions, D = out-degrees (tuned_SIGN.py:158-161).  That the two forms describe the same arcs is
 * the caller's promise.  SoP is not available on directed graphs (S3GRL_ERR_NOT_IMPLEMENTED). */
s3grl_status s3grl_graph_create_directed(s3grl_context* ctx, int64_t num_nodes, const int64_t* csr_indptr,
                                         const int32_t* csr_indices, const int64_t* csc_indptr,
                                         const int32_t* csc_indices, int64_t nnz, s3grl_graph** out);
s3grl_status s3grl_graph_destroy(s3grl_graph* g);

/* PoS / PoS Plus, feature-independent half: BFS to num_hops from {src,dst} on the unmasked
 * graph, induced sub-CSR with the target link removed, D^-1/2 A D^-1/2, and rows {src,dst}
 * (+ common neighbours) of Â^1..Â^K by row propagation.  `links` is int64 [L,2] (the
 * reference iterates link_index.t().tolist(), tuned_SIGN.py:147). */
s3grl_status s3grl_plan_create(s3grl_context* ctx, const s3grl_graph* g, const int64_t* links,
                               int64_t num_links, const s3grl_cfg* cfg, s3grl_plan** out);

/* ScaLed subgraphs from node sets the CALLER cached (reference utils.py:94-108: with rw_kwargs the
 * subgraph of (src,dst) is torch.unique(cat(cache[src], cache[dst])) of rw_kwargs['cached_pos_rws'] /
 * ['cached_neg_rws'] — dict node -> unique nodes of its walks, built by utils.create_rw_cache,
 * utils.py:425-443, sgrl_link_pred.py:123-128 — or rw_kwargs['unique_nodes'][(src,dst)]; src and dst
 * first, utils.py:134-135).  A CSR of sets on the device:
 *   per_link == 0: num_sets == the graph's num_nodes, set i belongs to NODE i (empty for nodes the
 *                  cache does not hold); subgraph of (s,d) = {s,d} ∪ set[s] ∪ set[d];
 *   per_link == 1: num_sets == num_links, set l belongs to LINK l; subgraph = {s,d} ∪ set[l].
 * Nodes beyond {src,dst} form "hop 1" (dists 0,0,1,1,..., utils.py:145-146); num_hops, rw_m, rw_M and
 * the per-hop sampling fields of the cfg play no part (rw_m / rw_M must be 0).  The arrays are read
 * while the plan is created, not afterwards.  S3GRL_ERR_INVALID_ARGUMENT for a malformed set_ptr
 * or an id outside [0, num_nodes). */
typedef struct s3grl_node_sets {
  const int64_t* set_ptr;   /* device int64 [num_sets + 1], monotone from 0 to num_set_nodes */
  const int32_t* set_nodes; /* device int32 [num_set_nodes] (duplicates and src / dst themselves allowed) */
  int64_t num_sets;
  int64_t num_set_nodes;
  int32_t per_link;         /* 0 or 1 */
  int32_t reserved;         /* must be 0 */
} s3grl_node_sets;
s3grl_status s3grl_plan_create_sets(s3grl_context* ctx, const s3grl_graph* g, const int64_t* links,
                                    int64_t num_links, const s3grl_cfg* cfg, const s3grl_node_sets* sets,
                                    s3grl_plan** out);
/* The producer of such a cache, in place of reference utils.create_rw_cache (utils.py:425-443:
 * torch_cluster random_walk from every start node repeated rw_M times, walk length rw_m, unique per
 * start): for start i the ascending unique nodes of its rw_M uniform walks of length rw_m, the start
 * itself included, in set_nodes[set_ptr[i] .. set_ptr[i+1]).  starts: device int64 [num_starts];
 * set_ptr: device int64 [num_starts + 1] out; set_nodes: device int32 out with room for
 * num_starts * (rw_m * rw_M + 1) entries.  The walks are those a plan with the same cfg.rw_m / rw_M /
 * seed draws by itself (counter-based generator keyed by seed, node, walk, step): same distribution
 * as torch_cluster's, other random numbers.  rw_m * rw_M + 1 <= 8192. */
s3grl_status s3grl_walk_sets(s3grl_context* ctx, const s3grl_graph* g, const int64_t* starts,
                             int64_t num_starts, int32_t rw_m, int32_t rw_M, uint32_t seed,
                             int64_t* set_ptr, int32_t* set_nodes);

s3grl_status s3grl_plan_destroy(s3grl_plan* p);
/* host struct out.  Plan creation does not wait for its last kernels (the gather of s3grl_run* is
 * queued right behind them): total_sub_edges / total_support / total_volume are read back here, i.e.
 * this call waits for the context's stream when it is the first to ask. */
s3grl_status s3grl_plan_get_stats(const s3grl_plan* p, s3grl_plan_stats* out);
/* ΣR alone (host int64 out): what the caller sizes `rows` by; never waits */
s3grl_status s3grl_plan_total_rows(const s3grl_plan* p, int64_t* total_rows);
/* what the host knows of a plan the moment it exists (host int64 [4] out; never waits): [0] links,
 * [1] total rows ΣR, [2] links folded into their reversed duplicate, [3] row pairs (gather jobs) */
s3grl_status s3grl_plan_counts(const s3grl_plan* p, int64_t* what);
/* device int64 [L+1] out */
s3grl_status s3grl_plan_row_ptr(const s3grl_plan* p, int64_t* row_ptr);
/* device int64 [total_rows] out: global node id of every output row */
s3grl_status s3grl_plan_row_nodes(const s3grl_plan* p, int64_t* row_nodes);
/* parity hook: node_ptr int64 [L+1] (always), then, when non-NULL, nodes int32 [Σn] per link in
 * hop-major order, ascending id inside a hop, and dists int8 [Σn] (hop distance from
 * {src,dst}) — the quantities reference utils.k_hop_subgraph returns as `nodes`, `dists`
 * (utils.py:53-54,73-74; its order inside a hop is CPython set order). */
s3grl_status s3grl_plan_export_subgraphs(const s3grl_plan* p, int64_t* node_ptr, int32_t* nodes,
                                         int8_t* dists);

/* Relative cost of every link (device fp32 [L] out), in arbitrary units, from the sizes the plan
 * measured — what a multi-GPU caller balances its shards by (a count-only plan is enough).  The
 * model follows the kernels and was fitted on MI355X: multi-hop plans  pairs * n + 400  (gather and
 * row walks grow with the subgraph and with the row pairs of PoS Plus, ~400 nodes' worth of fixed
 * work per link); one-hop plans on big graphs  e_bound + 220 + (pairs - 1) * n  with e_bound the
 * bound of the induced entries the sizing pass derives from the degree-oriented rows (a hub-rich
 * positive costs several times a random negative of the collab-scale workload; node counts alone
 * say 1.5x) — except for the links served from a cached hub neighbourhood (plan statistics: hub_links),
 * whose oriented rows are not probed:  12.1 * n + 1380 + (pairs - 1) * n  (both fitted with
 * tools/cost_fit_onehop.py: the two kinds of links timed apart, two size buckets each; round 4, after
 * link_tiny_kernel and gather_narrow_kernel: profiles/r04_cost_fit_onehop.txt).  A reversed duplicate (d,s) that the plan folds into its primary (s,d) costs 250: its two
 * output rows and bookkeeping (least squares over the shards of 2-, 4- and 8-way splits of PubMed:
 * 410 / 290 at sign_k = 3, 310 / 260 at sign_k = 5) — so the cost of a pair is what ONE rank pays for it when both directions are kept
 * together (s3grl_amd.parallel.shard_assignment); with S3GRL_FLAG_NO_FOLD every link is priced in full. */
s3grl_status s3grl_plan_link_cost(const s3grl_plan* p, float* cost);

/* PoS / PoS Plus, feature half: rows[r, i, :] = [z | Σ_w Â^i[row r, w] X[w, :]].
 * X fp32 [N, F] row-major with leading dimension ldx (elements); rows fp32
 * [total_rows, K+1, 1+F] dense.  Asynchronous on the context's stream. */
s3grl_status s3grl_run(s3grl_context* ctx, const s3grl_plan* p, const float* X, int64_t ldx,
                       int64_t num_features, float* rows);

/* The feature operand x of the reference operators (dense fp32 [N,F], utils.py:83), prepared
 * once: 16-byte aligned rows (borrowed when X already is: keep X alive and unchanged while the
 * handle is in use).  flags: 0 = let the engine choose: when at most half of X's 16-byte
 * chunks hold a non-zero (bag-of-words / TF-IDF / one-hot rows) it also keeps a packed copy —
 * per row a bit mask of the non-zero chunks + those chunks — and the gather fetches only them;
 * same sums bit for bit.  1 = dense rows only; 4 = packed rows whatever the density;
 * 2 = (column, value)-pair rows accumulated in LDS (kept for comparison: slower than both).
 * Beside packed rows the engine keeps per row its (column, value) element rows, which the gather
 * reads for the list rows that feed only the last operator (same sums bit for bit); adding 8 to
 * flags 0 or 4 leaves them out (comparison runs). */
s3grl_status s3grl_features_create(s3grl_context* ctx, const float* X, int64_t ldx,
                                   int64_t num_nodes, int64_t num_features, int32_t flags,
                                   s3grl_features** out);
s3grl_status s3grl_features_destroy(s3grl_features* f);
/* host outs (either may be NULL): stored non-zeros (0 when never counted), sparse rows in use */
s3grl_status s3grl_features_info(const s3grl_features* f, int64_t* nnz, int32_t* is_sparse);
/* same contract as s3grl_run, with a prepared operand */
s3grl_status s3grl_run_features(s3grl_context* ctx, const s3grl_plan* p, const s3grl_features* f,
                                float* rows);

/* SoP: one-off global setup (reference sgrl_link_pred.py:161-178 recomputes it per split):
 * Â = D^-1/2 A D^-1/2 of the whole graph and Y_i = Â^i X, i = 1..K. */
s3grl_status s3grl_sop_create(s3grl_context* ctx, const s3grl_graph* g, const float* X,
                              int64_t ldx, int64_t num_features, int32_t sign_k, s3grl_sop** out);
/* The same on a MULTIGRAPH: the reference builds its global operator from the uncoalesced edge_index
 * (sgrl_link_pred.py:161-172: `SparseTensor(row, col)`, degree = entries per row), so a pair that
 * occurs m times counts m times in the degree and weighs m in every product, while the CSR of A
 * holds it once (scipy sums duplicates).  multiplicity: device fp32 [nnz], aligned with the graph's
 * `indices` as handed to s3grl_graph_create (NULL = all 1 = s3grl_sop_create); copied.
 * A_hat = D^-1/2 M D^-1/2 with D = row sums of M.  Every paper dataset is coalesced (m = 1). */
s3grl_status s3grl_sop_create_weighted(s3grl_context* ctx, const s3grl_graph* g, const float* X,
                                       int64_t ldx, int64_t num_features, int32_t sign_k,
                                       const float* multiplicity, s3grl_sop** out);
s3grl_status s3grl_sop_destroy(s3grl_sop* s);
/* the global SIGN features themselves, out fp32 [K, N, F]: out[i-1] = Â^i X.  This is what the
 * reference's non-optimised twin `TunedSIGN.__call__` (tuned_SIGN.py:18-23, PyG SIGN(K)) computes
 * for the graph it is handed. */
s3grl_status s3grl_sop_features(s3grl_context* ctx, const s3grl_sop* s, float* out);
/* rows fp32 [2L, K+1, 1+F]: x_i[src] = [Â^i[s,s] | Σ_{w != d} Â^i[s,w] X[w]] and the mirror
 * image for dst (reference tuned_SIGN.py:71-78,92-113,119-132).
 * The three scalars per operator are formed inside the ball of {src,dst} of radius ceil(K/2) (one less for
 * odd K).  A ball has no size limit: the links are binned by what their ball (4 + 16·ceil(K/2) bytes per
 * node) needs into three LDS classes, and class 3 — balls beyond a CU's LDS, up to the whole graph — keeps
 * its node list and propagated rows in an HBM workspace slice per workgroup, sized per link and launched in
 * chunks under a byte cap (1 GiB; one link at least per chunk).  Same arithmetic in the same order: a link's
 * rows do not depend on where its ball lived.  S3GRL_ERR_OUT_OF_MEMORY when one slice cannot be allocated.
 * Comparison hooks (environment, results identical): S3GRL_SOP_FORCE_HBM_BALLS = every ball in HBM,
 * S3GRL_SOP_BALL_WORKSPACE_BYTES = the cap. */
s3grl_status s3grl_sop_run(s3grl_context* ctx, const s3grl_sop* s, const int64_t* links,
                           int64_t num_links, float* rows);
/* Without a GPU: how s3grl_sop_run lays a ball out on a graph of num_nodes nodes at sign_k.  out (host
 * int32 [8]): [0] = radius of the ball, [1] = bytes per ball node, [2] = 1 when the N-bit bitmaps live in HBM
 * slices (num_nodes > ~327 680), [3..5] = the most ball nodes LDS classes 0, 1, 2 take ([5]: a larger ball is
 * class 3), [6] = LDS bytes next to the ball, [7] = 0. */
s3grl_status s3grl_sop_layout(int64_t num_nodes, int32_t sign_k, int32_t* out);
/* out (host int64 [4]): links per class of the context's last s3grl_sop_run; [3] = balls formed in HBM
 * (all of them under S3GRL_SOP_FORCE_HBM_BALLS).  Reversed duplicates folded into their primary count nowhere. */
s3grl_status s3grl_sop_class_links(const s3grl_context* ctx, int64_t* out);

/* Consumer-side centre / common-neighbour pooling, reference SIGNNet._centre_pool_helper
 * (models.py:339-369) on the engine's layout: h fp32 [total_rows, H] (the output of
 * operator_diff), rows of link b = row_ptr[b]..row_ptr[b+1], the first two being src, dst.
 * mode 0 (k_heuristic == 0): out [B, H] = h[src] * h[dst];  mode 1 / 2 (k_pool_strategy 'mean' /
 * 'sum'): out [B, 2H] = [h[src] * h[dst] | mean or sum of the remaining rows], zeros when a link
 * has none (the reference's `size=B`).  'concat' (models.py:363-367) is mode 0 plus a strided
 * view of the k rows, done by the Python binding (s3grl_amd/pool.py).  No host sync (the
 * reference does np.unique on the CPU per batch, models.py:341).  backward: grad_h [total_rows,
 * H] is fully overwritten. */
s3grl_status s3grl_centre_pool_forward(s3grl_context* ctx, const float* h, const int64_t* row_ptr,
                                       int64_t num_links, int64_t hidden, int32_t mode, float* out);
s3grl_status s3grl_centre_pool_backward(s3grl_context* ctx, const float* h, const int64_t* row_ptr,
                                        int64_t num_links, int64_t hidden, int32_t mode,
                                        const float* grad_out, float* grad_h);

/* Per-phase device time accumulated since profiling was last switched on, in milliseconds,
 * from HIP events recorded on the context's stream around the kernels themselves:
 * what[0]=structure (count+scan+build+jobs), [1]=propagate, [2]=gather (the dominant kernel),
 * [3]=sop setup, [4]=sop run, [5]=number of gather launches in [2], [6]=number of plans in
 * [0],[1], [7]=number of sop runs in [4], [8]=sop_rows_kernel alone (part of [4]),
 * [9]=the spmm_norm_kernel launches alone (part of [3]), [10]=number of sop setups in [3],
 * [11]=the SoP scalar launches over balls in HBM alone, their slice sizing included (part of [4]),
 * [12..15] reserved (0).  Host array of 16 doubles. */
s3grl_status s3grl_context_timings(s3grl_context* ctx, double* what);
/* switch the HIP-event timing on/off and zero the accumulators (off by default) */
s3grl_status s3grl_context_set_profiling(s3grl_context* ctx, int32_t enabled);

/* Gives the workspace blocks the context caches between calls (plans, stashes, scratch: several
 * GB after a PubMed-scale plan) back to the HIP allocator; blocks of live handles stay.  Call it
 * when the precompute phase is over and the training step needs the memory. *released (host,
 * may be NULL) = bytes freed. */
s3grl_status s3grl_context_trim(s3grl_context* ctx, int64_t* released);

/* Measurement: the bytes the gather launch of `p` on operand `f` REQUESTS, computed exactly from
 * the plan (no timing, no sampling): what[0] = node-id bytes (4 per list entry and column tile),
 * [1] = packed-row header bytes (32 per entry and tile; 0 for a dense operand), [2] = feature
 * bytes (packed: 16 per non-zero chunk of every gathered row, or, where the last operator's rows
 * beyond the prefix are read as element rows, 8 per entry of the row-tile; the phase-B launch of
 * a two-launch plan fetches a row of up to 64 entries as 16-byte pairs: the count rounded up to
 * even, the padding entry of an odd row included; dense: the 16-byte lane loads that fall inside
 * the row), [3] = coefficient bytes (8 per entry, operator and tile actually read:
 * the packed kernel reads only the last operator beyond the prefix the others can reach),
 * [4] = output bytes written (folded reversed duplicates included), [5] = operator-0 rows of X
 * read for the output, [6] = per-job metadata bytes, [7] = wavefronts launched.
 * Host array of 8 int64.  Synchronises the context's stream. */
s3grl_status s3grl_plan_gather_traffic(s3grl_context* ctx, const s3grl_plan* p,
                                       const s3grl_features* f, int64_t* what);

/* Measurement aid, not on the product path: reads a KNOWN number of bytes of `buf` (device, `bytes`
 * long) in one of the engine's access shapes, so that rocprofv3's FETCH_SIZE can be calibrated on
 * gfx950 for that shape (tools/pmc_calibrate.py).  pattern 0 / 1 / 2: one coalesced pass with 16 /
 * 8 / 4 bytes per lane; 3: `rows` rows of `row_bytes` (multiple of 16) at pseudo-random places, one
 * wavefront per row, 16 bytes per lane.  *requested_bytes (host) = the bytes the loads asked for. */
s3grl_status s3grl_calibration_read(s3grl_context* ctx, const void* buf, int64_t bytes, int32_t pattern,
                                    int64_t rows, int32_t row_bytes, int64_t* requested_bytes);

/* ---- Labelled enclosing subgraphs (the SEAL baselines) ---------------------------------------------------
 * Reference utils.py:556-573: per link k_hop_subgraph (utils.py:47-85) followed by construct_pyg_graph
 * (utils.py:277-316) with a node-labelling trick, without sign_pyg_kwargs.  Per link (s, d):
 *   nodes   the k-hop extraction of a PoS plan with the same settings: s, d, then hop-major, ascending id
 *           inside a hop (the reference: CPython set order there); dists its hop distances
 *   edges   every non-zero entry of A[nodes][:, nodes] except the target link's two, in local ids: rows in
 *           list order, ascending local column inside a row; weight = A's value (the `values` array)
 *           — ssp.find after subgraph[0, 1] = subgraph[1, 0] = 0.  A directed graph keeps its arcs.
 *   z       by label, distances unweighted on the UNDIRECTED subgraph:
 *           DRNL     [n]    1 + min(ds, dd) + (D/2)(D/2 + D%2 - 1), D = ds + dd, ds from s with d removed and dd
 *                           from d with s removed; s, d: 1; a node either endpoint does not reach: 0
 *           DE       [n, 2] distance to s, to d, nothing removed and the target link counted as an edge (scipy
 *                           keeps the explicit zeros), clamped at 3 (unreached: 3)
 *           DE_PLUS  [n, 2] ds, dd as for DRNL, the removed endpoint's own entry 0, clamped at 100 (unreached: 100)
 *           HOP      [n]    dists;   ZO [n]  dists == 0
 *           DEGREE   [n]    column sums of the subgraph's values (in-weights), as integers, capped at 100
 *           anything else   [n] zeros
 * Outputs are integers and bit-exact.  Every link is served whatever its size: a link whose list, distances
 * and edges fit the LDS budget is labelled on-chip, any other one (more than 65 535 nodes included) with
 * HBM workspace; the choice depends on the link alone. */
typedef enum s3grl_label {
  S3GRL_LABEL_DRNL = 0,
  S3GRL_LABEL_DE = 1,
  S3GRL_LABEL_DE_PLUS = 2,
  S3GRL_LABEL_HOP = 3,
  S3GRL_LABEL_ZO = 4,
  S3GRL_LABEL_DEGREE = 5,
  S3GRL_LABEL_ZEROS = 6
} s3grl_label;

typedef struct s3grl_subgraph_cfg {
  int32_t num_hops;          /* k of the k-hop enclosing subgraph */
  uint32_t seed;             /* per-hop sampling: the keyed generator of s3grl_cfg.seed */
  int32_t max_nodes_per_hop; /* as s3grl_cfg: 0 = no cap */
  int32_t lds_budget;        /* bytes of LDS a link may use (0 = 64 KiB, at most 159 KiB); beyond, the HBM
                                flavour.  1 sends every link to the HBM flavour */
  double ratio_per_hop;      /* as s3grl_cfg: >= 1.0 = keep all */
  int32_t reserved[4];       /* must be 0 */
} s3grl_subgraph_cfg;

typedef struct s3grl_subgraphs s3grl_subgraphs; /* the labelled subgraphs of one call, on the device */

/* links int64 [L, 2] device; values device fp32 [nnz] aligned with the graph's CSR indices (the successor
 * CSR of a directed graph), or NULL for ones; label an s3grl_label.  A directed graph is labelled as such
 * (its plan follows out- and in-arcs).  S3GRL_ERR_INVALID_ARGUMENT for a link endpoint outside [0, N) or
 * src == dst.  Waits for its kernels: the workspace goes back to the context's arena on return. */
s3grl_status s3grl_subgraphs_create(s3grl_context* ctx, const s3grl_graph* g, const float* values,
                                    const int64_t* links, int64_t num_links, const s3grl_subgraph_cfg* cfg,
                                    int32_t label, s3grl_subgraphs** out);
/* host int64 [4] out: [0] links L, [1] Σn nodes, [2] Σe edges, [3] columns of z (2 for DE / DE_PLUS, else 1) */
s3grl_status s3grl_subgraphs_counts(const s3grl_subgraphs* s, int64_t* what);
/* device outs, each may be NULL: node_ptr int64 [L+1], nodes int32 [Σn], dists int8 [Σn], edge_ptr int64 [L+1],
 * src / dst int32 [Σe] (local ids of the link), weight fp32 [Σe], z int32 [Σn, columns].  Asynchronous on the
 * context's stream. */
s3grl_status s3grl_subgraphs_export(const s3grl_subgraphs* s, int64_t* node_ptr, int32_t* nodes, int8_t* dists,
                                    int64_t* edge_ptr, int32_t* src, int32_t* dst, float* weight, int32_t* z);
s3grl_status s3grl_subgraphs_destroy(s3grl_subgraphs* s);

/* The graph operators of the SEAL baselines' models on a batch of labelled enclosing subgraphs (reference
 * models.py:12-76 GCN and :139-222 DGCNN, which use PyG GCNConv and global_sort_pool), kernels in
 * csrc/s3grl_propagate.hip (gcn_norm, gcn_propagate) and csrc/s3grl_seal_nn.hip (sort_pool).  All are
 * deterministic (no float atomics; bit-identical between runs) and asynchronous on the context's stream.  S3GRL_ERR_INVALID_ARGUMENT for a null pointer or a size out of range.
 *
 * gcn_norm (PyG gcn_norm, add_remaining_self_loops): ptr int64 [N+1] groups a split's edges by destination,
 * self-loops included; weight fp32 [E] in that order, or NULL for ones.  dinv fp32 [N] = deg^-1/2 with
 * deg[i] the weight sum of the edges into i, summed in CSR order; 0 where deg == 0. */
s3grl_status s3grl_gcn_norm(s3grl_context* ctx, int64_t num_nodes, const int64_t* ptr, const float* weight,
                            float* dinv);
/* GCNConv propagation after its linear: out [R, hidden] = Σ_e coef[e] · h[row of nbr[e]] (+ bias [hidden], may
 * be NULL) over the CSR entries ptr[rows[r]] .. ptr[rows[r]+1] of every batch row r, in CSR order.  rows int64
 * [R]: the split node of each batch row (a batch holds whole subgraphs back to back); loc int32 [N]: a split
 * node's position in its subgraph; nbr int32 [E]: the neighbour's position in the same subgraph, so its batch
 * row is r - loc[rows[r]] + nbr[e].  With the CSR grouped by destination this is the forward; grouped by source
 * (the same coef, transposed) and bias NULL it is the backward with respect to h. */
s3grl_status s3grl_gcn_propagate(s3grl_context* ctx, int64_t num_rows, int64_t hidden, const int64_t* rows,
                                 const int32_t* loc, const int64_t* ptr, const int32_t* nbr, const float* coef,
                                 const float* h, const float* bias, float* out);
/* global_sort_pool(x, batch, k): x fp32 [R, width], graph g = rows node_ptr[g] .. node_ptr[g+1] (device int64
 * [G+1]).  out fp32 [G, k·width]: each graph's rows by the last channel descending (ties by ascending row,
 * -0.0 == +0.0), the first k, zero rows past its size; index int32 [G, k]: the source row of every output row,
 * -1 for padding.  max_nodes (host) bounds every graph's size; a graph whose sort does not fit lds_budget bytes
 * of LDS (0: 64 KiB, at most 159 KiB) sorts in workspace (device uint64 [2·R]), which may be NULL only when
 * the power of two >= max_nodes fits.  S3GRL_ERR_INVALID_ARGUMENT when it does not. */
s3grl_status s3grl_sort_pool_forward(s3grl_context* ctx, const float* x, const int64_t* node_ptr,
                                     int64_t num_graphs, int64_t width, int64_t k, int64_t max_nodes,
                                     int64_t lds_budget, uint64_t* workspace, float* out, int32_t* index);
/* grad_x fp32 [num_rows, width] is fully overwritten: the row index[g, j] gets grad_out[g, j], all others zero. */
s3grl_status s3grl_sort_pool_backward(s3grl_context* ctx, int64_t num_graphs, int64_t width, int64_t k,
                                      const int32_t* index, const float* grad_out, int64_t num_rows,
                                      float* grad_x);

/* Message passing on the RAW edge list, for the SEAL baselines' SAGE and GIN models (reference models.py:78-135,
 * :225-298) and the MPGNN rows (baselines/gnn_link_pred.py), which use PyG SAGEConv, GINConv and global_mean_pool;
 * kernels in csrc/s3grl_propagate.hip (nbr_aggregate: gcn_propagate's kernel with another weight source) and
 * csrc/s3grl_mpnn.hip (segment_mean).  Deterministic (no float atomics; bit-identical between runs) and asynchronous
 * on the context's stream.  S3GRL_ERR_INVALID_ARGUMENT for a null pointer or a size out of range.
 *
 * nbr_aggregate: out [R, hidden] = self_coef · h[r] + Σ_e s(e) · h[row of nbr[e]] over the CSR entries
 * ptr[rows[r]] .. ptr[rows[r]+1] of every batch row r, summed in CSR order, the self term added last (and not read
 * when self_coef == 0).  rows / loc / ptr / nbr are gcn_propagate's batch convention, but the edge list is the
 * subgraph's own: an input (i, i) entry is an edge, a duplicated arc counts twice, nothing is added, and no per-edge
 * coefficient is read.  scale fp32 [N] over the split's nodes (for the mean: 1 / max(indeg, 1), so a node without
 * in-arcs gets a zero row) with scale_side:
 *   S3GRL_SCALE_NONE       scale must be NULL; s(e) = 1: the sum, forward (CSR by destination) and backward (by source)
 *   S3GRL_SCALE_OWN        s(e) = scale[rows[r]], applied once to the finished sum: the mean's forward
 *   S3GRL_SCALE_NEIGHBOUR  s(e) = scale[split node of nbr[e]]: the mean's backward over the CSR by source, where the
 *                          weight of an arc belongs to its destination
 * OWN / NEIGHBOUR with scale NULL, or NONE with a scale, is S3GRL_ERR_INVALID_ARGUMENT.  nbr may be NULL when the
 * split has no edge at all. */
#define S3GRL_SCALE_NONE 0
#define S3GRL_SCALE_OWN 1
#define S3GRL_SCALE_NEIGHBOUR 2
s3grl_status s3grl_nbr_aggregate(s3grl_context* ctx, int64_t num_rows, int64_t hidden, const int64_t* rows,
                                 const int32_t* loc, const int64_t* ptr, const int32_t* nbr, const float* scale,
                                 int32_t scale_side, float self_coef, const float* h, float* out);
/* global_mean_pool: x fp32 [R, width], graph g = rows node_ptr[g] .. node_ptr[g+1] (device int64 [G+1]); out fp32
 * [G, width] = Σ rows / max(n_g, 1), a zero row for an empty graph.  Rows are summed in 2048-row chunks, inside a
 * chunk by fixed slices joined by a fixed butterfly, the chunks in order.  max_nodes (host) bounds every graph's
 * size; partial: device fp32 [G · ceil(max_nodes / 2048) · width] of scratch, may be NULL when max_nodes <= 2048. */
s3grl_status s3grl_segment_mean_forward(s3grl_context* ctx, const float* x, const int64_t* node_ptr,
                                        int64_t num_graphs, int64_t width, int64_t max_nodes, float* partial,
                                        float* out);
/* grad_x fp32 [R, width] is fully overwritten: grad_x[r] = grad_out[graph of r] / max(n_g, 1). */
s3grl_status s3grl_segment_mean_backward(s3grl_context* ctx, const int64_t* node_ptr, int64_t num_graphs,
                                         int64_t width, int64_t max_nodes, const float* grad_out, float* grad_x);

/* Graph InfoClust (reference Software/GIC: layers/cluster.py, layers/discriminator.py:Discriminator_cluster), kernels
 * in csrc/s3grl_gic.hip.  All device fp32, row-major; N nodes, d channels, K clusters with 1 <= N < 2^31, 1 <= d <=
 * S3GRL_GIC_MAX_DIM, 1 <= K <= S3GRL_GIC_MAX_CLUSTERS (S3GRL_ERR_INVALID_ARGUMENT outside).  Deterministic (no float
 * atomics: nodes are taken in chunks of 64, a chunk's sums run in node order and the chunks are added in order) and
 * asynchronous on the context's stream.  Non-finite values follow IEEE: a cluster whose total responsibility is 0 gives
 * inf / nan, as in the reference.  ld* are row strides in floats (>= d) of inputs that may be column slices. */
#define S3GRL_GIC_MAX_DIM 4096
#define S3GRL_GIC_MAX_CLUSTERS 256
/* out [rows, d] = x[r] / (‖x[r]‖ + 1e-6); nrm [rows] = ‖x[r]‖, may be NULL. */
s3grl_status s3grl_gic_normalise(s3grl_context* ctx, int64_t rows, int64_t d, const float* x, int64_t ldx, float* out,
                                 float* nrm);
/* cluster(data, K, 1, num_iter, init, beta) on row-normalised data [N, d] (s3grl_gic_normalise): num_iter >= 1 times
 * mu <- mu / (‖mu‖ + 1e-6); r = softmax(beta · data · muᵀ); cluster_r = Σ_n r; mu = (1 / cluster_r) · (rᵀ · data).
 * Outputs: mu [K, d], r [N, K] and cluster_r [K] of the LAST iteration (r is computed from the previous mu) and
 * mun_last [K, d], the normalised table that iteration read.  Scratch: mun_tmp [K, d] (may be NULL when num_iter ==
 * 1), partial [ceil(N / 64) · (K + K·d)].  Two launches per iteration, plus one. */
s3grl_status s3grl_gic_cluster_forward(s3grl_context* ctx, int64_t N, int64_t d, int64_t K, float beta,
                                       int32_t num_iter, const float* data, const float* init, float* mun_last,
                                       float* mun_tmp, float* partial, float* mu, float* cluster_r, float* r);
/* The backward of ONE iteration (num_iter == 1, init detached) into h, data = h / (‖h‖ + 1e-6): g_h [N, d] from gZ
 * [K, d] and gS [N, K], given that call's data, mun_last, r, Z = mu, cluster_r and the normalise call's nrm.
 * Scratch: table_ws [K·d + K]. */
s3grl_status s3grl_gic_cluster_backward(s3grl_context* ctx, int64_t N, int64_t d, int64_t K, float beta,
                                        const float* data, const float* h, int64_t ldh, const float* nrm,
                                        const float* mun, const float* r, const float* Z, const float* cluster_r,
                                        const float* gZ, const float* gS, float* table_ws, float* g_h);
/* logits [2N]: logits[n] = h1[n] · c2[n], logits[N + n] = h2[n] · c2[n] with c2[n] = sigmoid(Σ_k S[n, k] · Z[k]),
 * never written to memory.  h1 and h2 share the row stride ldh. */
s3grl_status s3grl_gic_disc_forward(s3grl_context* ctx, int64_t N, int64_t d, int64_t K, const float* S,
                                    const float* Z, const float* h1, const float* h2, int64_t ldh, float* logits);
/* Its backward from grad_logits [2N]: g_h1, g_h2 (row stride ldg), gS [N, K] and gZ [K, d].  Scratch: g_pre [N, d],
 * partial [ceil(N / 64) · K·d]. */
s3grl_status s3grl_gic_disc_backward(s3grl_context* ctx, int64_t N, int64_t d, int64_t K, const float* S,
                                     const float* Z, const float* h1, const float* h2, int64_t ldh,
                                     const float* grad_logits, float* g_h1, float* g_h2, int64_t ldg, float* g_pre,
                                     float* partial, float* gS, float* gZ);

/* node2vec pretraining (reference n2v_prep.node_2_vec_pretrain: PyG Node2Vec with p = q = 1, sparse=True, trained
 * by torch.optim.SparseAdam), kernels in csrc/s3grl_node2vec.hip.  One trainer holds the embedding, SparseAdam's
 * two moment tables and its step count, all fp32 [N, dim] on the device.  Every draw (epoch permutation, walks,
 * negatives, the N(0, 1) initial table) comes from the engine's counter-based generator keyed by (seed, epoch,
 * step, position): the same algorithm and distributions as PyG, not its random streams.  Deterministic: no float
 * atomics; two trainers with one seed are bit-identical.  Asynchronous on the context's stream unless a call
 * says otherwise. */
typedef struct s3grl_skipgram_cfg {
  int32_t dim;                  /* embedding_dim, 1 .. 16384 */
  int32_t walk_length;          /* steps per walk (the walk holds walk_length + 1 nodes), >= context_size */
  int32_t context_size;         /* nodes per window, >= 2 */
  int32_t walks_per_node;
  int32_t num_negative_samples;
  uint32_t seed;
  double p, q;                  /* must be 1.0: S3GRL_ERR_NOT_IMPLEMENTED otherwise */
  int32_t reserved[4];          /* must be 0 */
} s3grl_skipgram_cfg;

typedef struct s3grl_skipgram s3grl_skipgram;

/* indptr int64 [N+1] / indices int32 [nnz] device: the CSR of the caller's edge_index (rows = sources, duplicates
 * kept), checked on the host.  init fp32 [N, dim] device, or NULL for N(0, 1) from the seed.  Waits for the
 * device. */
s3grl_status s3grl_skipgram_create(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                                   int64_t num_entries, const s3grl_skipgram_cfg* cfg, const float* init,
                                   s3grl_skipgram** out);
/* One pass over a permutation of range(N) in batches of batch_size (the last one short), one SparseAdam step
 * (betas 0.9 / 0.999, eps 1e-8) per batch.  step_loss device fp32 [ceil(N / batch_size)] or NULL: every step's
 * loss, written on the device (no host sync). */
s3grl_status s3grl_skipgram_epoch(s3grl_skipgram* t, int64_t epoch, int64_t batch_size, float lr, float* step_loss);
/* One step on the caller's windows: pos int32 [num_pos, context_size], neg int32 [num_neg, context_size] device,
 * checked on the host (a node outside [0, N): S3GRL_ERR_INVALID_ARGUMENT).  loss device fp32 [1] or NULL.  Waits
 * for the device.  The test and oracle hook: it runs the kernels an epoch step runs. */
s3grl_status s3grl_skipgram_step_windows(s3grl_skipgram* t, const int32_t* pos, int64_t num_pos, const int32_t* neg,
                                         int64_t num_neg, float lr, float* loss);
/* The windows step `step` of epoch `epoch` draws, B = min(batch_size, N - step · batch_size) starts: pos int32
 * [W·B·walks_per_node, context_size], neg int32 [W·B·walks_per_node·num_negative_samples, context_size], W =
 * walk_length + 2 - context_size, window-index-major.  Changes no training state. */
s3grl_status s3grl_skipgram_export_windows(s3grl_skipgram* t, int64_t epoch, int64_t step, int64_t batch_size,
                                           int32_t* pos, int32_t* neg);
/* device outs fp32 [N, dim], each may be NULL; steps (host) the SparseAdam step count */
s3grl_status s3grl_skipgram_state(const s3grl_skipgram* t, float* emb, float* exp_avg, float* exp_avg_sq,
                                  int64_t* steps);
/* *emb = the live table, device fp32 [N, dim]: no copy.  It is the trainer's: valid until destroy, and what a later
 * step on the context's stream writes a later read on that stream sees. */
s3grl_status s3grl_skipgram_weight(const s3grl_skipgram* t, const float** emb);
s3grl_status s3grl_skipgram_destroy(s3grl_skipgram* t);

/* Matrix factorisation link prediction (reference baselines/mf.py train_mf: nn.Embedding(N, hidden), a LinkPredictor
 * of num_layers Linear layers over the Hadamard product of the endpoint rows, dense torch.optim.Adam over both),
 * kernels in csrc/s3grl_mf.hip.  One trainer holds the table [N, hidden], the predictor as one flat array (per layer
 * its weight [out, hidden] in torch's layout, then its bias [out]; P = (num_layers - 1)(hidden² + hidden) + hidden + 1
 * values), both Adam moment sets and the step count, all fp32 on the device.  A step takes B positive pairs and B
 * negative ones and is two launches: no float atomics, no host round trip.  Every draw (epoch permutation, negative
 * pairs, dropout masks, initial parameters) comes from the engine's counter-based generator keyed by (seed, epoch,
 * step, index): torch's algorithm and distributions, not its random streams.  Two trainers with one seed are
 * bit-identical.  Asynchronous on the context's stream unless a call says otherwise.  S3GRL_ERR_NOT_IMPLEMENTED
 * outside hidden <= 128, num_layers <= 4, batch_size <= 1024. */
typedef struct s3grl_mf_cfg {
  int32_t hidden;               /* 1 .. 128 */
  int32_t num_layers;           /* Linear layers of the predictor, 2 .. 4 */
  double dropout;               /* p in [0, 1): after every hidden layer's relu, kept values scaled by 1 / (1 - p) */
  uint32_t seed;
  int32_t reserved[3];          /* must be 0 */
} s3grl_mf_cfg;

typedef struct s3grl_mf s3grl_mf;

/* The lane layout of the step kernels, a pure host function: out[0] channels per lane, out[1] lanes per pair (and per
 * table row), out[2] pairs per tile, out[3] tiles of a step of batch_size positives. */
s3grl_status s3grl_mf_layout(int32_t hidden, int32_t num_layers, int64_t batch_size, int32_t* out);
/* init_table fp32 [N, hidden] / init_pred fp32 [P] device, or NULL for N(0, 1) / torch's Linear default (uniform in
 * ±1 / sqrt(hidden)) from the seed.  Waits for the device. */
s3grl_status s3grl_mf_create(s3grl_context* ctx, int64_t num_nodes, const s3grl_mf_cfg* cfg, const float* init_table,
                             const float* init_pred, s3grl_mf** out);
/* One pass over a permutation of the train links (int32 [num_train, 2] device, checked on the host: one wait per
 * epoch) in batches of batch_size, the last one short; per batch as many uniform random negative pairs and one Adam
 * step (betas 0.9 / 0.999, eps 1e-8).  step_loss device fp32 [ceil(num_train / batch_size)] or NULL. */
s3grl_status s3grl_mf_epoch(s3grl_mf* t, int64_t epoch, const int32_t* train, int64_t num_train, int64_t batch_size,
                            double lr, float* step_loss);
/* One step on the caller's pairs int32 [2·batch, 2] device (positives, then negatives), checked on the host (waits
 * for the device).  masks uint8 [2·batch, num_layers - 1, hidden] device (non-zero: kept), or NULL for the engine's
 * own draw.  loss device fp32 [1] or NULL.  The test and oracle hook: it runs the kernels an epoch step runs. */
s3grl_status s3grl_mf_step_pairs(s3grl_mf* t, const int32_t* pairs, int64_t batch, const uint8_t* masks, double lr,
                                 float* loss);
/* What step `step` of epoch `epoch` over num_train links draws, B = min(batch_size, num_train - step · batch_size):
 * pos_idx int32 [B] (positions in the train list), neg int32 [B, 2], masks uint8 [2B, num_layers - 1, hidden].
 * Changes no training state. */
s3grl_status s3grl_mf_export_draws(s3grl_mf* t, int64_t epoch, int64_t step, int64_t num_train, int64_t batch_size,
                                   int32_t* pos_idx, int32_t* neg, uint8_t* masks);
/* out fp32 [num_pairs] device = sigmoid(predictor(x[a] ⊙ x[b])) in eval mode (no dropout); pairs int32 [num_pairs, 2]
 * device, checked on the host (waits for the device). */
s3grl_status s3grl_mf_score(s3grl_mf* t, const int32_t* pairs, int64_t num_pairs, float* out);
/* device outs, each may be NULL: the table and its moments fp32 [N, hidden], the predictor and its moments fp32 [P];
 * steps (host) Adam's step count */
s3grl_status s3grl_mf_state(const s3grl_mf* t, float* table, float* table_avg, float* table_avg_sq, float* pred,
                            float* pred_avg, float* pred_avg_sq, int64_t* steps);
s3grl_status s3grl_mf_destroy(s3grl_mf* t);

/* SIGNNet, the model that consumes the engine's rows (reference models.py:301-383; twin: harness.SIGNNetTwin):
 * operator_diff = Linear(in_width -> hidden), ELU, BatchNorm1d, dropout over the rows of a mini-batch of links, centre
 * pooling (none / mean / sum, as s3grl_centre_pool_forward), link_pred_mlp = Linear(ch·hidden -> hidden), ReLU,
 * BatchNorm1d, dropout, Linear(hidden -> 1), BCE with logits, dense torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8) over
 * the ten tensors; kernels in csrc/s3grl_signnet.hip.  `rows` fp32 [num_rows, in_width] and `row_ptr` int64
 * [num_links + 1] are the engine's output on the device; a link's rows are read in place.  A step is four launches: no
 * float atomics, no host round trip.  Every draw (initial values, the epoch's permutation, both dropout masks) is a
 * counter-based hash of (seed, epoch, step, stream, index).  Asynchronous on the context's stream unless a call says
 * otherwise.  S3GRL_ERR_NOT_IMPLEMENTED outside hidden <= 256, in_width <= 2^20, batch_size <= 64. */
typedef struct s3grl_signnet_cfg {
  int32_t in_width;             /* (sign_k + 1)(1 + F): one collated row */
  int32_t hidden;               /* 1 .. 256 */
  int32_t pool_mode;            /* 0: no common-neighbour rows pooled; 1: their mean; 2: their sum (ch = 2) */
  uint32_t seed;
  double dropout;               /* p in [0, 1) of both dropouts; kept values scaled by 1 / (1 - p) */
  int32_t reserved[4];          /* must be 0 */
} s3grl_signnet_cfg;

typedef struct s3grl_signnet s3grl_signnet;

/* The layout of the step kernels, a pure host function: out[0] hidden columns per workgroup, out[1] workgroups per
 * launch, out[2] rows a wavefront carries per pass over k, out[3] floats per load along in_width (4 when in_width is a
 * multiple of 4, else 1), out[4] the inner tile along in_width (64 · out[3]), out[5] floats per load along the head's
 * input (4 when ch · hidden is a multiple of 4; pooled != 0: ch = 2), out[6] rows per tile of the dW1 pass, out[7] links
 * per score tile. */
s3grl_status s3grl_signnet_layout(int32_t hidden, int64_t in_width, int32_t batch, int32_t pooled, int32_t* out);
/* Initial values from the seed: torch's Linear default (uniform in ±1 / sqrt(fan_in)), γ = 1, β = 0, running mean 0 and
 * var 1.  Waits for the device. */
s3grl_status s3grl_signnet_create(s3grl_context* ctx, const s3grl_signnet_cfg* cfg, s3grl_signnet** out);
/* One pass over a permutation of the links in batches of batch_size (2 .. 64; a last batch of one link is skipped), one
 * Adam step each.  y fp32 [num_links] device.  row_ptr is checked on the host (one wait per epoch).  step_loss device
 * fp32 [ceil((num_links - 1) / batch_size)] or NULL. */
s3grl_status s3grl_signnet_fit_epoch(s3grl_signnet* t, int64_t epoch, const float* rows, int64_t num_rows,
                                     const int64_t* row_ptr, const float* y, int64_t num_links, int64_t batch_size,
                                     double lr, float* step_loss);
/* fit_epoch for num_members (1 .. 16) handles at once, every step of the epoch four launches for the whole group: the
 * step kernels get a second grid dimension, the member.  Each member keeps its own parameters, Adam state and count,
 * BatchNorm statistics, permutation and masks, and ends bit-identical to what s3grl_signnet_fit_epoch(members[r], epoch,
 * .., lr[r], ..) alone computes; every other call keeps working on a member before and after.  lr host [num_members];
 * step_loss device fp32 [num_members, steps] or NULL.  row_ptr is checked once (one wait per epoch).  Members may differ
 * in seed, dropout, lr and Adam's step count.  S3GRL_ERR_INVALID_ARGUMENT when they differ in context, hidden, in_width
 * or pool mode or a handle appears twice; S3GRL_ERR_NOT_IMPLEMENTED above 16 members. */
s3grl_status s3grl_signnetruns_fit_epoch(s3grl_signnet* const* members, int32_t num_members, int64_t epoch,
                                           const float* rows, int64_t num_rows, const int64_t* row_ptr, const float* y,
                                           int64_t num_links, int64_t batch_size, const double* lr, float* step_loss);
/* What step `step` of epoch `epoch` over num_links links draws, B = min(batch_size, num_links - step · batch_size);
 * each out may be NULL: link_ids int32 [B], mask1 uint8 [mask1_rows, hidden] (the rows of the batch in batch order),
 * mask2 uint8 [B, hidden].  Changes no training state. */
s3grl_status s3grl_signnet_draws(s3grl_signnet* t, int64_t epoch, int64_t step, int64_t num_links, int64_t batch_size,
                                 int32_t* link_ids, uint8_t* mask1, int64_t mask1_rows, uint8_t* mask2);
/* One step on the caller's links int32 [batch] device, checked on the host with row_ptr (waits for the device).  mask1
 * uint8 [ΣR_b, hidden] / mask2 uint8 [batch, hidden] device (non-zero: kept), or NULL for the engine's own draw.  loss
 * device fp32 [1] or NULL.  The test hook: it runs the kernels an epoch step runs. */
s3grl_status s3grl_signnet_step(s3grl_signnet* t, const float* rows, int64_t num_rows, const int64_t* row_ptr,
                                const float* y, int64_t num_links, const int32_t* link_ids, int64_t batch,
                                const uint8_t* mask1, const uint8_t* mask2, double lr, float* loss);
/* out fp32 [num_links] device = the logit of every link in eval mode (running statistics, no dropout).  row_ptr is
 * checked on the host (waits for the device). */
s3grl_status s3grl_signnet_score(s3grl_signnet* t, const float* rows, int64_t num_rows, const int64_t* row_ptr,
                                 int64_t num_links, float* out);
/* which 0 / 1 / 2: the parameters / exp_avg / exp_avg_sq, packed W1 [hidden, in_width], b1, γ1, β1, W2 [hidden,
 * ch·hidden], b2, γ2, β2, W3 [hidden], b3 [1]; which 3: the running mean and var of BN1, then of BN2 [4, hidden].  Device
 * arrays, may be NULL.  counters (host, may be NULL) [3]: Adam's step count, num_batches_tracked of BN1 and of BN2. */
s3grl_status s3grl_signnet_read_state(s3grl_signnet* t, int32_t which, float* out, int64_t* counters);
s3grl_status s3grl_signnet_write_state(s3grl_signnet* t, int32_t which, const float* in, const int64_t* counters);
s3grl_status s3grl_signnet_destroy(s3grl_signnet* t);

/* The link classifier of the N2V row (reference baselines/n2v.py: sklearn's default LogisticRegression over the Hadamard
 * features emb[src] ⊙ emb[dst]); kernels in csrc/s3grl_linkclf.hip.  It computes the minimiser over θ = (w [dim], b) of
 *   f(θ) = ½ w·w + C Σ_i [ log(1 + exp(z_i)) − y_i z_i ],  z_i = (emb[src_i] ⊙ emb[dst_i])·w + b
 * (the intercept is not penalised) by damped Newton in fp64: the step is θ − t H⁻¹g with the first t of 1, ½, … 2⁻¹⁵ for
 * which f(θ − t d) <= f(θ) − 1e-4 t gᵀd + 2⁻³² |f(θ)|.  `emb` fp32 [num_nodes, dim] device is read in place through
 * `pairs` int32 [num_pairs, 2] device; `labels` uint8 [num_pairs] device (non-zero: class 1).  Pairs and labels are
 * checked on the host before the first launch (one wait); the launches that follow are asynchronous on the context's
 * stream: four per iteration, no float atomics, no kernel that waits for another.  Two fits of one input are
 * bit-identical.  dim is 1 .. 128. */
typedef struct s3grl_linkclf s3grl_linkclf;

/* The lane layout of the row kernels, a pure host function: out[0] channels per lane, out[1] lanes per row, out[2] rows
 * per tile (a block's share of the rows up to out[3] tiles), out[3] the most blocks of a row pass: past it a block
 * takes several tiles, one after the other. */
s3grl_status s3grl_linkclf_layout(int32_t dim, int32_t* out);
/* C > 0 the inverse ridge strength, tol >= 0 on max|∇f|, max_iter the Newton iterations of a fit. */
s3grl_status s3grl_linkclf_create(s3grl_context* ctx, int32_t dim, double C, double tol, int32_t max_iter,
                                  s3grl_linkclf** out);
/* max_iter iterations from init_theta (host fp64 [dim + 1], the intercept last) or from 0 when NULL.  Once max|∇f| <=
 * tol at the current θ the `done` flag on the device is raised and every later launch returns at once.
 * S3GRL_ERR_INVALID_ARGUMENT when the labels hold one class only. */
s3grl_status s3grl_linkclf_fit(s3grl_linkclf* t, const float* emb, int64_t num_nodes, const int32_t* pairs,
                               const uint8_t* labels, int64_t num_pairs, const double* init_theta);
/* One iteration from the current θ, whatever `done` said before.  The test hook: it runs the launches a fit runs. */
s3grl_status s3grl_linkclf_newton_step(s3grl_linkclf* t, const float* emb, int64_t num_nodes, const int32_t* pairs,
                                       const uint8_t* labels, int64_t num_pairs);
/* Host outs, each may be NULL; waits for the device.  theta and grad fp64 [dim + 1]: the current θ, and ∇f where the
 * last iteration began, as is loss = f there; step_t the t it took (0: none); n_iter the steps taken; done 0: not yet,
 * 1: max|∇f| <= tol at θ, 2: no t of the ladder was accepted, 3: the Hessian was not positive definite or not finite. */
s3grl_status s3grl_linkclf_state(s3grl_linkclf* t, double* theta, double* grad, double* loss, double* step_t,
                                 int32_t* n_iter, int32_t* done);
/* pred uint8 [num_pairs] device = z > 0; decision fp32 [num_pairs] device = z, or NULL; with labels, counts int64 [4]
 * device = (true positives, false positives, false negatives, true negatives), or NULL.  Pairs are checked on the host
 * (waits for the device). */
s3grl_status s3grl_linkclf_predict(s3grl_linkclf* t, const float* emb, int64_t num_nodes, const int32_t* pairs,
                                   int64_t num_pairs, const uint8_t* labels, uint8_t* pred, float* decision,
                                   int64_t* counts);
s3grl_status s3grl_linkclf_destroy(s3grl_linkclf* t);

/* Link-ranking metrics (reference utils.py evaluate_auc / evaluate_hits / evaluate_mrr / evaluate_ogb_rocauc) on scores
 * that stay on the device; kernels in csrc/s3grl_metrics.hip.  The handle owns the workspace (keys, the sort's temporary,
 * per-tile partials, a pinned result record) and grows it on demand.  All work goes on the context's stream; every call
 * below that takes a handle waits for the device once, at its end.  No float atomics: a call repeated gives the same
 * bits. */
typedef struct s3grl_metrics s3grl_metrics;

/* A pure host function.  out[0] sorted scores per workgroup of the scan passes; for rows of num_neg negatives (1 ..
 * 2^31 − 1): out[1] rows per wavefront of the MRR kernel, out[2] lanes per row (out[1] · out[2] = 64), out[5] rows per
 * workgroup; out[3] floats per vector load; out[4] the most K values of one ranked call. */
s3grl_status s3grl_metrics_layout(int64_t num_neg, int32_t* out);
s3grl_status s3grl_metrics_create(s3grl_context* ctx, s3grl_metrics** out);
/* One sort of scores fp32 [n] device, 1 <= n < 2^31.  labels uint8 [n] device (1: positive, 0: negative, anything
 * else is counted as bad), or NULL: the first n_pos scores are the positives.  ks (host) [num_k <= out[4] of the
 * layout], each >= 1.  Host outs: counts [6] = positives P, negatives N, distinct thresholds (−0.0 and +0.0 are one;
 * ±inf are values), NaN scores, bad labels, Σ over the thresholds of fp_g (2 tp_b + tp_g) = 2·P·N·AUC as an exact
 * integer; *ap = Σ (tp_g / P) tp / (tp + fp) in fp64 (sklearn's average precision; NaN when P = 0); hits [num_k]: the
 * positives strictly above the K-th largest negative, or −1 when there are fewer than K negatives.  With a NaN among the
 * scores the other outs mean nothing. */
s3grl_status s3grl_metrics_ranked(s3grl_metrics* m, const float* scores, const uint8_t* labels, int64_t n, int64_t n_pos,
                                  const int64_t* ks, int32_t num_k, int64_t* counts, double* ap, int64_t* hits);
/* pos fp32 [num_pos] and neg fp32 [num_pos, num_neg] (row-major, row stride num_neg) device.  Per row rank =
 * (#{neg > pos} + #{neg >= pos}) / 2 + 1 and mrr_list [num_pos] (device fp32) = 1 / rank, an fp32 division.  Host
 * outs: *sum = Σ mrr_list in fp64, counts [4] = rows of rank <= 1, <= 3, <= 10, and the NaNs among pos and neg. */
s3grl_status s3grl_metrics_mrr(s3grl_metrics* m, const float* pos, const float* neg, int64_t num_pos, int64_t num_neg,
                               float* mrr_list, double* sum, int64_t* counts);
s3grl_status s3grl_metrics_destroy(s3grl_metrics* m);

/* Link heuristics of the reference's use_heuristic branch (utils.py CN, AA, PPR; PPR as fast_pagerank 0.0.4
 * pagerank_power), kernels in csrc/s3grl_heuristics.hip.  One object holds a graph A (CSR, fp64 values) with its
 * transpose, fp64 row sums, column sums and Adamic-Adar weights 1 / ln(column sum) (±inf -> 0).  Deterministic: no
 * float atomics; every score is summed in fp64 in a fixed order and written as fp32. */
#define S3GRL_HEURISTIC_CN 0    /* sum_k A[s,k] A[d,k] */
#define S3GRL_HEURISTIC_AA 1    /* sum_k A[s,k] (A[d,k] w_k); NaN when row d holds a key of NaN weight (a negative
                                 * column sum), common or not: the reference's sparse product keeps 0 * NaN */
/* Four indices the reference does not have (DESIGN.md section 23 is their specification).  r: row sums, c: column
 * sums, deg: stored entries of a row. */
#define S3GRL_HEURISTIC_RA 2        /* resource allocation: sum_k A[s,k] (A[d,k] v_k), v_k = 1 / c_k, 0 where c_k == 0 */
#define S3GRL_HEURISTIC_JACCARD 3   /* structural: |keys(s) & keys(d)| / (deg(s) + deg(d) - |&|), 0 when that is 0 */
#define S3GRL_HEURISTIC_PA 4        /* preferential attachment: r_s r_d */
#define S3GRL_KATZ_MAX_LEN 64

typedef struct s3grl_heuristics s3grl_heuristics;

/* indptr int64 [N+1] / indices int32 [nnz] device, every row strictly ascending; values fp64 [nnz] device or NULL
 * for ones.  Checked and transposed on the host.  Waits for the device. */
s3grl_status s3grl_heuristics_create(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr,
                                     const int32_t* indices, const double* values, int64_t num_entries,
                                     s3grl_heuristics** out);
/* kind: one of the five S3GRL_HEURISTIC_* above (any other: S3GRL_ERR_INVALID_ARGUMENT); links int32 [2, L] device
 * (sources, then destinations), checked on the host (an id outside [0, N): S3GRL_ERR_INVALID_ARGUMENT); out fp32
 * [L] device. */
s3grl_status s3grl_heuristics_pairs(s3grl_heuristics* h, int32_t kind, const int32_t* links, int64_t num_links,
                                    float* out);
/* Personalised PageRank of each source, solved once: fp64 power iteration with a stop per source once
 * ||x_new - x_old||_2 <= tol on the unnormalised iterate, or after max_iter iterations.  sources int32 [S] device,
 * distinct; links int32 [2, L] device, every source among sources; out fp32 [L] device: x[d] / sum(x) of the
 * link's source; iterations int32 [S] device or NULL.  block_width: sources per block, a multiple of 64 in
 * [64, 1024], or 0 for the default (both iterates within about 128 MiB, 64 .. 256); results do not depend on it.
 * Waits for the device. */
s3grl_status s3grl_heuristics_ppr(s3grl_heuristics* h, const int32_t* sources, int64_t num_sources,
                                  const int32_t* links, int64_t num_links, double p, double tol, int32_t max_iter,
                                  int32_t block_width, float* out, int32_t* iterations);
/* Truncated Katz index sum_{l=1..max_len} beta^l (A^l)[s, d] of each source, solved once, by Horner's rule in fp64
 * on the CSR of the transpose: x_0 = 0, x_l[j] = beta * sum_i A[i,j] (x_{l-1}[i] + [i == s]) with column j's entries
 * added in ascending i; out fp32 [L] device: x_max_len[d] of the link's source (an overflow of fp32 gives +-inf).
 * beta finite and 1 <= max_len <= S3GRL_KATZ_MAX_LEN, else S3GRL_ERR_INVALID_ARGUMENT.  sources, links and
 * block_width as for s3grl_heuristics_ppr; results do not depend on block_width.  Waits for the device. */
s3grl_status s3grl_heuristics_katz(s3grl_heuristics* h, const int32_t* sources, int64_t num_sources,
                                   const int32_t* links, int64_t num_links, double beta, int32_t max_len,
                                   int32_t block_width, float* out);
s3grl_status s3grl_heuristics_destroy(s3grl_heuristics* h);

/* Subgraph sketching (ELPH / BUDDY), kernels in csrc/s3grl_sketch.hip; DESIGN.md section 24 is the specification.
 * Per node and hop i in 0..hops a MinHash row of num_perm uint32 and a HyperLogLog row of m = 2^hll_p uint8
 * registers: hop 0 from the hash H(v, s) = fmix32(v * 0x9E3779B1 + fmix32(seed + s * 0x27D4EB2F)) (slots
 * 0..num_perm-1: MinHash, slot num_perm: HLL), hop i the elementwise min / max of hop i-1 over a row's stored keys
 * and the row itself.  Integer min / max / compare / popcount only, no atomics: every output is a function of its
 * inputs alone.  Envelope: 1 <= N <= 2^24, nnz < 2^31, 1 <= hops <= 4, num_perm a multiple of 64 in [64, 512],
 * 7 <= hll_p <= 10; outside it S3GRL_ERR_INVALID_ARGUMENT.  The calls are asynchronous on the context's stream after
 * their host checks. */
#define S3GRL_SKETCH_MAX_HOPS 4
#define S3GRL_SKETCH_MAX_NODES (1 << 24)

/* indptr int64 [N+1] / indices int32 [nnz] device (used structurally; checked on the host: a column outside [0, N)
 * is S3GRL_ERR_INVALID_ARGUMENT).  Fills minhash uint32 [hops+1, N, num_perm] and hll uint8 [hops+1, N, m], both
 * device and 8-byte aligned. */
s3grl_status s3grl_sketch_build(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                                int64_t num_entries, int32_t hops, int32_t num_perm, int32_t hll_p, uint32_t seed,
                                uint32_t* minhash, uint8_t* hll);
/* The cardinality of num_rows register rows (uint8 [num_rows, m] device) as fp32 [num_rows]: T = sum 2^(33-p-reg),
 * z = zero registers, E = c / T in fp64, replaced by lc[z] when E <= 2.5 m and z > 0.  lc: fp64 [m+1] device, the
 * host's table m ln(m / z); c = alpha m^2 2^(33-p) from the host. */
s3grl_status s3grl_sketch_cardinality(s3grl_context* ctx, int32_t hll_p, const double* lc, double c,
                                      const uint8_t* registers, int64_t num_rows, float* out);
/* Per link (u, v) of links int32 [2, L] device (checked on the host; u == v is legal) and i, j in 0..hops:
 * match_ij = #{s: MH_i[u,s] == MH_j[v,s]}, T_ij and z_ij of max(HL_i[u], HL_j[v]), I_ij = (match_ij E_ij) /
 * num_perm; features [L, hops^2 + 2 hops] = [A_11 .. A_kk | Bu_1 .. Bu_k | Bv_1 .. Bv_k] by inclusion-exclusion in
 * fp64, in the order DESIGN.md section 24 fixes.  Outputs are device arrays, each may be NULL: match int32, t int64,
 * z int32 and intersections fp32, all [L, hops+1, hops+1]; features fp32. */
s3grl_status s3grl_sketch_pairs(s3grl_context* ctx, int64_t num_nodes, int32_t hops, int32_t num_perm, int32_t hll_p,
                                const uint32_t* minhash, const uint8_t* hll, const double* lc, double c,
                                const int32_t* links, int64_t num_links, int32_t* match, int64_t* t, int32_t* z,
                                float* intersections, float* features);
/* The pairs call above on the graph without each link's own entries: the outputs of link
 * (u, v) are, to the byte, those of the same tables built on the CSR without the stored entries (u, v) and (v, u),
 * formed per link from the unmasked tables by a walk over the two endpoint rows; a link neither of whose entries is
 * stored gets the unmasked outputs.  indptr int64 [N+1] / indices int32 [nnz] device: the CSR the tables were built
 * from, rows ascending and distinct (the caller's promise; the build call checked it).  Exact for hops <= 2 only:
 * S3GRL_ERR_NOT_IMPLEMENTED for hops 3 and 4.  Links are checked on the host; every output may be NULL. */
s3grl_status s3grl_masked_sketch_pairs(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr,
                                       const int32_t* indices, int64_t num_entries, int32_t hops, int32_t num_perm,
                                       int32_t hll_p, const uint32_t* minhash, const uint8_t* hll, const double* lc,
                                       double c, const int32_t* links, int64_t num_links, int32_t* match, int64_t* t,
                                       int32_t* z, float* intersections, float* features);

/* Neural Common Neighbour (NCN), kernels in csrc/s3grl_ncn.hip; DESIGN.md section 26 is the specification.  The
 * graph: indptr int64 [N+1] / indices int32 [nnz] device, rows ascending and distinct with every column in [0, N)
 * (the caller's promise), used structurally: N(x) is the stored keys of row x, nothing is symmetrised.  links int32
 * [2, L] device; u == v and repeated links are legal.  The host checks 1 <= N < 2^31, nnz < 2^31, L < 2^31 and every
 * link id before any GPU work (S3GRL_ERR_INVALID_ARGUMENT), which waits for the device; the launches are asynchronous
 * on the context's stream.  No atomics: every output is a function of its inputs alone.
 *
 * The list of link l is N(u) ∩ N(v) in ascending id, less u and v themselves when exclude_endpoints is 1 (0 or 1,
 * anything else is refused).  The count call writes counts int64 [L] (device); the caller scans them into cn_ptr
 * int64 [L+1] (device) with total = cn_ptr[L], and the fill call writes cn_idx int32 [total] (device) at cn_ptr[l] +
 * rank.  The fill writes nothing outside [0, total). */
s3grl_status s3grl_cn_count(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                            int64_t num_entries, const int32_t* links, int64_t num_links, int32_t exclude_endpoints,
                            int64_t* counts);
s3grl_status s3grl_cn_fill(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                           int64_t num_entries, const int32_t* links, int64_t num_links, int32_t exclude_endpoints,
                           const int64_t* cn_ptr, int64_t total, int32_t* cn_idx);
/* The rectangular segment sum out[r, :] = sum over j in [ptr[r], ptr[r+1]) of h[idx[j], :]: h fp32 [M, dim], ptr
 * int64 [R+1] rising from 0, idx int32 [ptr[R]] with every entry in [0, M) (the caller's promise), out fp32 [R, dim],
 * all device; 0 <= M < 2^31, 1 <= dim <= 65536, 0 <= R < 2^31.  The order of the fp32 additions is fixed: a row is
 * cut into chunks of 64 consecutive entries, a chunk's partial is the sequential sum of its entries in ascending j
 * starting from its first entry, the row is the sequential sum of the partials in chunk order starting from the first
 * partial, and an empty row is +0.0.  Rows are read as 16-byte words where dim % 4 == 0 and h and out are 16-byte
 * aligned, as scalars otherwise; the result does not depend on it.  Asynchronous on the context's stream. */
s3grl_status s3grl_segment_sum(s3grl_context* ctx, const float* h, int64_t num_source_rows, int64_t dim,
                               const int64_t* ptr, const int32_t* idx, int64_t num_rows, float* out);

/* NCNC's completion step, same unit; DESIGN.md section 27 is the specification.  Graph, links, flag and host checks
 * as for s3grl_cn_count / s3grl_cn_fill.  The list of link l = (u, v) is three sections, each in ascending id, one
 * after the other: S0 = N(u) ∩ N(v), S1 = N(u) \ N(v), S2 = N(v) \ N(u); with exclude_endpoints 1 the keys u and v
 * are dropped from all three.  u == v gives S0 = N(u) and empty S1, S2.  S0 is what s3grl_cn_fill writes for the same
 * link and flag.  The count call writes counts int64 [3, L] (device; row s holds |Ss|); the caller scans the sum of
 * the three rows into ptr int64 [L+1] (device) with total = ptr[L], and the fill call reads counts and ptr and writes
 * idx int32 [total] and side int32 [total] (0, 1 or 2: the entry's section), nothing outside [0, total). */
s3grl_status s3grl_cn_split_count(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                                  int64_t num_entries, const int32_t* links, int64_t num_links,
                                  int32_t exclude_endpoints, int64_t* counts);
s3grl_status s3grl_cn_split_fill(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                                 int64_t num_entries, const int32_t* links, int64_t num_links,
                                 int32_t exclude_endpoints, const int64_t* counts, const int64_t* ptr, int64_t total,
                                 int32_t* idx, int32_t* side);
/* The weighted segment sum out[r, :] = sum over j in [ptr[r], ptr[r+1]) of w[j]·h[idx[j], :], w fp32 [ptr[R]] device,
 * everything else as s3grl_segment_sum.  Every term is the fp32 product rounded once (never fused into the addition)
 * and the terms are added in s3grl_segment_sum's order, so unit weights give its bits. */
s3grl_status s3grl_segment_wsum(s3grl_context* ctx, const float* h, int64_t num_source_rows, int64_t dim,
                                const int64_t* ptr, const int32_t* idx, const float* w, int64_t num_rows, float* out);
/* The gradient of that sum in the weights: out_w[j] = sum over c of g[r(j), c]·h[idx[j], c], r(j) the list that holds
 * entry j; g fp32 [R, dim], h fp32 [M, dim], out_w fp32 [ptr[R]], all device; sizes as s3grl_segment_sum.  The order
 * is fixed and independent of alignment and launch shape: slot t of 64 owns the columns c with (c mod 256) / 4 == t
 * and adds its rounded products in ascending c from its first product (+0.0 without a column); the slots are combined
 * by the halving tree s = 32, 16, .., 1 (slot t < s becomes slot t + slot t+s); the result is slot 0. */
s3grl_status s3grl_segment_dot(s3grl_context* ctx, const float* g, int64_t num_rows, const float* h,
                               int64_t num_source_rows, int64_t dim, const int64_t* ptr, const int32_t* idx,
                               float* out_w);

/* Graph autoencoders (reference baselines/vgae.py run_vgae: PyG GAE / VGAE / ARGVA), kernels in csrc/s3grl_gae.hip:
 * the pair keys and PyG's sparse negative sampling, the inner-product decoder with recon_loss's per-pair gradient
 * and loss, and the pair backward over node-major incidence lists.  Deterministic (no float atomics; two runs with
 * one seed are bit-identical), asynchronous on the context's stream except where a count comes back; workspace
 * from the context's arena.  Pair lists are int32 device arrays of sources and destinations, every id in [0, N)
 * (checked by s3grl_gae_keys, the caller's promise elsewhere).  S3GRL_ERR_INVALID_ARGUMENT for a null pointer or
 * a size out of range (N outside [1, 2^31), more than 2^30 pairs, count < 0, dim outside [1, 65536]).
 *
 * keys: key(i, j) = i·(N−1) + j − [j > i] of every pair i != j, sorted ascending into keys [P] (device uint64);
 * self-loops sort last as UINT64_MAX.  *num_keys (host) = the pairs that are not self-loops, duplicates counted
 * (PyG's idx.numel()).  Waits for the device. */
s3grl_status s3grl_gae_keys(s3grl_context* ctx, int64_t num_nodes, const int32_t* src, const int32_t* dst,
                            int64_t num_pairs, uint64_t* keys, int64_t* num_keys);
/* PyG negative_sampling(method='sparse') against the first num_keys of pos_keys (sorted, from s3grl_gae_keys):
 * distinct, uniformly random ordered pairs i != j that are not positives, at most count of them, written to
 * src / dst [count] (device int32) in key order; *num_out (host) how many.  Candidates come from a counter-based
 * generator keyed by (seed, epoch, round, index).  Waits for the device. */
s3grl_status s3grl_gae_negatives(s3grl_context* ctx, int64_t num_nodes, const uint64_t* pos_keys, int64_t num_keys,
                                 int64_t count, uint32_t seed, int64_t epoch, int32_t* src, int32_t* dst,
                                 int64_t* num_out);
/* Node-major incidence of P pairs: slot [2P] (device int32) holds 2·pair + side (side 0: the node is the pair's
 * source), grouped by node, pairs ascending inside a node; ptr [N+1] (device int64) the node's range. */
s3grl_status s3grl_gae_incidence(s3grl_context* ctx, int64_t num_nodes, const int32_t* src, const int32_t* dst,
                                 int64_t num_pairs, int64_t* ptr, int32_t* slot);
/* logits [P+Q] (device fp32) = z[u]·z[v] of the positive pairs, then the negative ones; z fp32 [N, dim].  With coef
 * [P+Q] and loss [1] (both or neither): PyG recon_loss = -log(sigmoid + 1e-15).mean() over the positives
 * + -log(1 - sigmoid + 1e-15).mean() over the negatives, summed in fp64 in a fixed order, and each pair's
 * d loss / d logit in fp32. */
s3grl_status s3grl_gae_decode(s3grl_context* ctx, int64_t dim, const float* z, const int32_t* pos_src,
                              const int32_t* pos_dst, int64_t num_pos, const int32_t* neg_src, const int32_t* neg_dst,
                              int64_t num_neg, float* logits, float* coef, float* loss);
/* grad_z [N, dim] (device fp32, every row written) = scale · Σ coef[p] · z[other end of p] over each node's
 * incidence entries (s3grl_gae_incidence) of the positive list, then of the negative list (neg_* all NULL: none).
 * scale: device fp32 [1] or NULL for 1. */
s3grl_status s3grl_gae_backward(s3grl_context* ctx, int64_t num_nodes, int64_t dim, const float* z, const float* scale,
                                const int64_t* pos_ptr, const int32_t* pos_slot, const int32_t* pos_src,
                                const int32_t* pos_dst, const float* pos_coef, const int64_t* neg_ptr,
                                const int32_t* neg_slot, const int32_t* neg_src, const int32_t* neg_dst,
                                const float* neg_coef, float* grad_z);

/* WalkPool's own operator (reference Software/WalkPooling/src/model.py:74-219), kernels in csrc/s3grl_walkpool.hip:
 * the attention weights of every arc of a batch of enclosing subgraphs and the walk profile of the two stochastic
 * matrices they make.  Deterministic (no float atomics, every sum in a fixed order: two runs are bit-identical in
 * values and gradients) and asynchronous on the context's stream.  S3GRL_ERR_INVALID_ARGUMENT for a null pointer
 * or a size out of range (heads 1 .. 64, hidden 1 .. 4096, walk_len 1 .. 16).
 *
 * The batch: num_links subgraphs back to back, link g owning the batch nodes node_ptr[g] .. node_ptr[g+1]; its local
 * nodes 0 and 1 are the candidate link.  The arcs are those of E+ = E- with i -> j and j -> i added, in two orders:
 * grouped by target node (in_ptr [n+1] over the batch nodes; in_nbr the source and in_dst the target as positions
 * in the own subgraph; in_flag 1 on the two candidate arcs) and grouped by source node (out_ptr, out_nbr the
 * target, out_arc the arc's position in the in-order).  Every per-arc array of the calls below is [e, heads] in
 * the in-order.  All pointers are device memory; max_nodes / max_arcs bound every link's nodes and arcs (the
 * host's promise: a link outside it gets zeros). */
typedef struct s3grl_wp_batch {
  const int64_t* node_ptr;   /* [num_links + 1] */
  const int32_t* link;       /* [num_nodes] the link of every batch node */
  const int64_t* in_ptr;     /* [num_nodes + 1] */
  const int32_t* in_nbr;     /* [num_arcs] */
  const int32_t* in_dst;     /* [num_arcs] */
  const uint8_t* in_flag;    /* [num_arcs] */
  const int64_t* out_ptr;    /* [num_nodes + 1] */
  const int32_t* out_nbr;    /* [num_arcs] */
  const int64_t* out_arc;    /* [num_arcs] */
  int64_t num_links, num_nodes, num_arcs, max_nodes, max_arcs;
} s3grl_wp_batch;

/* A pure host function: how the walk kernels run a batch whose largest link has n_max nodes and e_max arcs.
 * out int64 [8], forward then backward, four each: the column block W (4, 8, 16 or 32), the workgroups per
 * (link, head, sign), the flavour (0: the block's arrays in LDS; 1: in the workspace) and the workspace bytes per
 * link.  A workgroup holds 2 (forward) or walk_len + 2 (backward) arrays of n_max x W floats; W is the widest that
 * fits lds_budget bytes (0: 80 KiB, so that two workgroups share a CU; at most 159 KiB) and is below 2·n_max;
 * flavour 1 (W = 4) when W = 4 does not fit, or with lds_budget = 1.  S3GRL_ERR_NOT_IMPLEMENTED above 4096 nodes. */
s3grl_status s3grl_wp_layout(int64_t n_max, int64_t e_max, int32_t heads, int32_t walk_len, int64_t lds_budget,
                             int64_t* out);
/* q, k fp32 [n, heads, hidden].  w[e, h] = <q[r, h], k[c, h]> / sqrt(hidden) of the arc r -> c; weights_p its softmax
 * over the arcs of E+ into c; weights_m = (1 - flag) exp(w - max over E+ into c) / (sum over E- into c + 1e-16);
 * omega fp32 [num_links, heads] = sigmoid(w[i -> j]) + sigmoid(w[j -> i]). */
s3grl_status s3grl_wp_attention_forward(s3grl_context* ctx, const s3grl_wp_batch* batch, int32_t heads,
                                        int32_t hidden, const float* q, const float* k, float* w, float* weights_p,
                                        float* weights_m, float* omega);
/* grad_q, grad_k [n, heads, hidden] (every element written) from the gradients of weights_p, weights_m and omega;
 * w, weights_p, weights_m as the forward wrote them; grad_w [e, heads] is scratch.  grad_k sums over the arcs into
 * a node, grad_q over the arcs out of it, both in CSR order. */
s3grl_status s3grl_wp_attention_backward(s3grl_context* ctx, const s3grl_wp_batch* batch, int32_t heads,
                                         int32_t hidden, const float* q, const float* k, const float* w,
                                         const float* weights_p, const float* weights_m, const float* grad_p,
                                         const float* grad_m, const float* grad_omega, float* grad_w, float* grad_q,
                                         float* grad_k);
/* out fp32 [num_links, heads, walk_len, 5]: for tau = t + 2 and X = P^tau, P[c, r] the weight of r -> c:
 * tr(X+) - tr(X-), X+[i,i] + X+[j,j], the same of X-, X+[i,j] + X+[j,i], the same of X-.  workspace: at least
 * num_links x the layout's forward bytes per link, 16-byte aligned.  S3GRL_ERR_NOT_IMPLEMENTED when max_nodes > 4096. */
s3grl_status s3grl_wp_walk_forward(s3grl_context* ctx, const s3grl_wp_batch* batch, int32_t heads, int32_t walk_len,
                                   int64_t lds_budget, const float* weights_p, const float* weights_m,
                                   void* workspace, int64_t workspace_bytes, float* out);
/* grad_p, grad_m [e, heads] (every element written) from grad_out [num_links, heads, walk_len, 5]; workspace: at
 * least num_links x the layout's backward bytes per link. */
s3grl_status s3grl_wp_walk_backward(s3grl_context* ctx, const s3grl_wp_batch* batch, int32_t heads,
                                    int32_t walk_len, int64_t lds_budget, const float* weights_p,
                                    const float* weights_m, const float* grad_out, void* workspace,
                                    int64_t workspace_bytes, float* grad_p, float* grad_m);

/* Top-K link recommendation: which new links does a node most likely have?  Kernels in csrc/s3grl_recommend.hip.
 * Candidate enumeration lists, per source, every node at graph distance 2 .. hops; the caller scores the pairs
 * (the precompute and a trained SIGNNet, or a heuristic) and the segment top-K ranks them per source.  No float
 * arithmetic and no atomics on any output: a call repeated gives the same bytes.
 *
 * Candidates.  g: an undirected graph (S3GRL_ERR_NOT_IMPLEMENTED for a directed one); sources int32 [num_sources]
 * device, each in [0, N), repeats allowed: every occurrence is a segment of its own; 2 <= hops <= 8;
 * exclude_keys uint64 [num_exclude] device or NULL: sorted, unique keys min(u, v) * N + max(u, v).  Segment i holds,
 * in ascending node id, every v with 2 <= dist(sources[i], v) <= hops on the graph as given, less the v whose pair
 * with the source is among the keys.  One workgroup per source walks the graph level by level over two N-bit
 * bitmaps: in LDS up to 524 288 nodes, beyond in an HBM workspace of one slice per resident workgroup.  The count
 * call writes seg_ptr int64 [num_sources + 1] (device) and *total (host) = seg_ptr[num_sources], and waits for the
 * device once.  The fill call repeats the walk and writes cand int32 [total] (device) at the offsets of seg_ptr, which
 * must be what the count call wrote for the same arguments; a segment whose length does not match is not written
 * and the call returns S3GRL_ERR_INVALID_ARGUMENT, as both do for a source outside [0, N).  Both wait. */
s3grl_status s3grl_candidates_count(s3grl_context* ctx, const s3grl_graph* g, const int32_t* sources,
                                    int64_t num_sources, int32_t hops, const uint64_t* exclude_keys,
                                    int64_t num_exclude, int64_t* seg_ptr, int64_t* total);
s3grl_status s3grl_candidates_fill(s3grl_context* ctx, const s3grl_graph* g, const int32_t* sources,
                                   int64_t num_sources, int32_t hops, const uint64_t* exclude_keys,
                                   int64_t num_exclude, const int64_t* seg_ptr, int32_t* cand);
/* Without a GPU: how the two calls above lay a source's walk out on a graph of num_nodes nodes.  out (host int64
 * [8]): [0] = 1 when the bitmaps live in HBM slices (num_nodes > 524 288), else 0 (LDS); [1] = words of one bitmap;
 * [2] = threads per workgroup; [3] = LDS bytes of the bitmaps per workgroup; [4] = workspace bytes per resident
 * workgroup; [5] = the most resident workgroups of the HBM flavour (0: one workgroup per source); [6] = the node
 * bound of the LDS flavour; [7] = 0. */
s3grl_status s3grl_candidates_layout(int64_t num_nodes, int32_t hops, int64_t* out);
/* Segment top-K.  scores fp32 [num_pairs], cand int32 [num_pairs], seg_ptr int64 [num_segments + 1] rising from
 * >= 0 to <= num_pairs, all device; 1 <= k <= 1024 (beyond: S3GRL_ERR_NOT_IMPLEMENTED).  Per segment the k best
 * entries, score descending, then position in the segment ascending (candidates are in ascending id, so ties go to
 * the lower id); -0.0 counts as +0.0 and a NaN ranks below -inf.  top_nodes int32 [num_segments, k] = cand of the
 * entries, padded with -1; top_scores fp32 [num_segments, k] = their scores as given, padded with -inf; top_count
 * int32 [num_segments] = min(k, segment length).  One workgroup per segment of any length: up to 2 048 entries are
 * sorted whole in LDS, longer segments by a radix select of the k-th key and a sort of the survivors.  Waits for the
 * device once; a bad seg_ptr is S3GRL_ERR_INVALID_ARGUMENT (no entry of scores or cand outside [0, num_pairs) is
 * read). */
s3grl_status s3grl_segment_topk(s3grl_context* ctx, const float* scores, const int64_t* seg_ptr, const int32_t* cand,
                                int64_t num_pairs, int64_t num_segments, int32_t k, int32_t* top_nodes,
                                float* top_scores, int32_t* top_count);

#ifdef __cplusplus
}
#endif
#endif /* S3GRL_H_ */
