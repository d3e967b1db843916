// Link kernels of the PoS / PoS Plus path and their launchers, gfx950.  Included by the four link units
// s3grl_links_k12.hip, _k34, _k56 and _k78 only: each instantiates launch_links_k for its two sign_k values,
// so that the instantiations (per sign_k, thread count, lanes per row and flavour: most of the engine's
// compile time) build in parallel.
//
//   link_kernel       ONE workgroup per link, everything on-chip: BFS (N-bit LDS bitmaps),
//                     local ids = popcount rank, degrees of the masked induced subgraph,
//                     D^-1/2, common neighbours, and rows {a,b} of Â^1..Â^K by K pull steps
//                     r_i = r_{i-1}·Â over the GLOBAL CSR rows filtered through the bitmap.
//                     No induced sub-CSR is ever materialised, nothing but the final
//                     (node id, coefficient) lists leaves the CU.
//   link_full_kernel  the full-reach one-hop case on big graphs, see there.
//
// Restates (not translates) reference tuned_SIGN.py:151-175 / :206-240: the reference materialises
// Â², …, Â^K of the whole n×n subgraph by SpGEMM and keeps R rows; here only those R rows are ever formed.
#include "s3grl_internal.hpp"
#include "s3grl_device.hpp"
#include "s3grl_link_classes.hpp"

#include <type_traits>

namespace s3grl {
namespace {

// ---------------------------------------------------------------------------------------
// The fused per-link kernel.  LDS layout (dynamic, 16-byte aligned base), n = |S|, p = |P|:
//   rec[W][3]              one record per 32 global ids, what a neighbour visit reads at ONE address:
//     inP                    P as a bitmap (the BFS's next-frontier bitmap until the BFS is done)
//     wpreP                  word-level popcount prefix of inP: local id of u ∈ P = rank in P
//     vis                    S as a bitmap
//                          (the helpers of s3grl_device.hpp take the stride between words, kSetRec)
//   cn[cn_cap] lvl_end[kMaxLevels] zbuf[4K] sh[32] hub[kHubWords]   (link_tail_words; hub[] only where the
//                          hub path is armed: a graph without hub rows pays no LDS for it)
//   list[n]                S in hop-major order, ascending id inside a hop (global ids)
//   dinvP[p]               D^-1/2 of the masked induced subgraph for the nodes of P
//   cur[p], nxs[p]         float2 propagation state s_i = dinv·r_i (rows a, b of the pair); bitmap flavour: one
//                          readable entry behind each, where a visit lands with the rank of a non-member of P
// P = the hop-major prefix of S that r_{K-1} can reach; only the LAST operator touches the
// rest of S, and it needs no state there: its degree and its sum come out of the same pass.
// GS = true: list / dinvP / state live in a per-workgroup HBM scratch slice instead of LDS (links
// whose subgraph does not fit what the bitmaps leave of 160 KiB); same code, slower memory.
// HS = true: the visited set is a hash table sized by the subgraph (keys/vals of C = pow2 >= 2n
// slots) instead of three N-bit bitmaps, local id = position in the hop-major list: for graphs
// whose bitmaps alone would take tens of KB of LDS per workgroup.  Same node lists, rows and
// statistics bit for bit; the sums agree to fp32 round-off (small fully-reached subgraphs are
// propagated through an LDS adjacency bit matrix in this flavour: another summation order).
// DM = true (with HS): the visited set is a direct map, one uint16 per node of the GRAPH holding the
// node's position in the hop-major list (0xFFFF = not in S): a neighbour visit is one LDS read instead
// of two bitmap words + a rank prefix + a popcount.  For graphs whose map (2N bytes) leaves most of
// the LDS free; the list comes from count_kernel's stash (the host sends no other link here).  Rows
// are walked in the same order by the same lanes as in the bitmap flavour: same sums bit for bit.
// DIRECTED (bitmap flavour only): the BFS above ran on the union of successors and predecessors
// (utils.py:60-63); the operator is D^-1/2 A D^-1/2 of the directed induced matrix with D = OUT-degrees
// (row counts, tuned_SIGN.py:158-161), so r_i = r_{i-1} A_hat pulls over a node's PREDECESSORS (dg.in_*)
// and the degrees are counted over its successors (dg.out_*), for every node of S (p == n).
// one wave per SIMD at least: eight spill here (headline link phase 3.87 -> 4.53 ms)
constexpr int kLinkMinWaves = 1;
template <int T, int K, int G, bool GS, bool HS, bool DM = false, bool DIRECTED = false>
__global__ __launch_bounds__(T, kLinkMinWaves) void link_kernel(
    const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices, int W,
    const int64_t* __restrict__ links, const int32_t* __restrict__ class_list, int hops, int plus,
    int cn_cap, int full_stats, int hubs, const WalkSets ws,
    const int32_t* __restrict__ p_nodes, const int64_t* __restrict__ node_off, const int64_t* __restrict__ row_ptr,
    const int64_t* __restrict__ job_off, const int64_t* __restrict__ coef_off,
    const int32_t* __restrict__ mirror_of, int32_t* __restrict__ c_ids, float* __restrict__ c_coef,
    Job* __restrict__ jobs, float* __restrict__ job_z, int32_t* __restrict__ job_lim,
    int64_t* __restrict__ row_nodes, int32_t* __restrict__ lvl, unsigned long long* __restrict__ tot_edges,
    unsigned long long* __restrict__ tot_support, unsigned long long* __restrict__ tot_vol,
    const int32_t* __restrict__ old_of_new, int split_t, int seg_shift,
    char* __restrict__ scratch, int64_t scratch_stride, int bm_ext_words, unsigned long long* __restrict__ dbg,
    HopSampling smp, const int32_t* __restrict__ stash, int slot,
    const int32_t* __restrict__ new_of_old, int lo_id, const DirGraph dg, int sop2) {
  static_assert(!DIRECTED || (!HS && !DM), "directed plans run on the bitmap flavour");
  // The LinkOut the output helpers take, built here from __restrict__ parameters: its members as a by-value
  // kernel parameter carry no noalias, which cost this kernel 2-20 VGPRs (and spills) per instantiation.
  const LinkOut out{node_off, row_ptr, job_off, coef_off, mirror_of, c_ids, c_coef, jobs, job_z, job_lim,
                    row_nodes, lvl, tot_edges, tot_support, tot_vol, old_of_new, split_t, seg_shift};
  // sop2 (S3GRL_MODE_SOP_RESTRICTED): the rows of the GLOBAL operator restricted to the subgraph — D^-1/2 from
  // the global degrees, the target link NOT removed, the partner's column zeroed in the features and the
  // label column = the diagonal entry (reference tuned_SIGN.py:71-78,102-113 on the ball instead of all of V)
  extern __shared__ uint32_t smem[];
  // rows walked by the operator passes (pull), by the degree count and by the common-neighbour test
  const int32_t* __restrict__ w_indptr = DIRECTED ? dg.in_indptr : indptr;
  const int32_t* __restrict__ w_indices = DIRECTED ? dg.in_indices : indices;
  const int32_t* __restrict__ o_indptr = DIRECTED ? dg.out_indptr : indptr;
  const int32_t* __restrict__ o_indices = DIRECTED ? dg.out_indices : indices;
  unsigned long long t_prev = dbg ? __builtin_amdgcn_s_memtime() : 0ull;   // phase_stamp
  const int tid = threadIdx.x;
  const int l = class_list[blockIdx.x];
  const int64_t noff = out.node_off[l];
  const int n_alloc = (int)(out.node_off[l + 1] - noff);
  const int p_alloc = p_nodes[l];
  const int mirror = out.mirror_of ? out.mirror_of[l] : -1;          // reversed duplicate folded into l
  const int64_t mrp = mirror >= 0 ? out.row_ptr[mirror] : -1;

  // visited set: three bitmaps of W words, or (HS) keys + vals of C words each
  uint32_t hmask = 0;
  int set_words = 3 * W;
  if constexpr (DM) {
    set_words = 16 * W;   // 32 W uint16 entries
  } else if constexpr (HS) {
    int C = 64;
    while (C < 2 * n_alloc) C <<= 1;
    hmask = (uint32_t)(C - 1);
    set_words = 2 * C;
  }
  // GS on a graph whose three N-bit bitmaps do not fit LDS (num_nodes > ~327 680): they sit at the head
  // of the workgroup's HBM slice (bm_ext_words > 0) and LDS holds the small fixed part only
  const bool bm_ext = GS && bm_ext_words > 0;
  if (bm_ext) set_words = 0;
  uint16_t* dmap = reinterpret_cast<uint16_t*>(smem);
  // (bitmap flavour: word w of inP / wpreP / vis is entry 0 / 1 / 2 of record w, RS words apart: a visit
  // fetches the two that make up a rank with one LDS read)
  constexpr int RS = HS ? 1 : kSetRec;
  uint32_t* rec0 = smem;
  int32_t* hkeys = reinterpret_cast<int32_t*>(smem);
  int32_t* hvals = hkeys + (hmask + 1);
  int32_t* cn = reinterpret_cast<int32_t*>(smem + set_words);
  int* lvl_end = cn + cn_cap;
  float* zbuf = reinterpret_cast<float*>(lvl_end + kMaxLevels);  // [2 (src,dst)][K][2 (rows)]
  int* sh = reinterpret_cast<int*>(zbuf + 4 * K);
  int* hub = hubs ? sh + 32 : nullptr;
  int32_t* list;
  float* dinvP;
  float2* cur;
  if constexpr (GS) {
    char* base = scratch + (int64_t)blockIdx.x * scratch_stride;   // 256-byte aligned slices
    if (bm_ext) {
      rec0 = reinterpret_cast<uint32_t*>(base);
      base += (size_t)bm_ext_words * 4;
    }
    list = reinterpret_cast<int32_t*>(base);
    dinvP = reinterpret_cast<float*>(list + n_alloc);
    cur = reinterpret_cast<float2*>(base + (((size_t)(n_alloc + p_alloc) * 4 + 7) & ~(size_t)7));
  } else {
    const int fixed_words = set_words + link_tail_words(cn_cap, K, hubs != 0);
    list = reinterpret_cast<int32_t*>(smem + fixed_words);
    dinvP = reinterpret_cast<float*>(list + n_alloc);
    cur = reinterpret_cast<float2*>(smem + ((fixed_words + n_alloc + p_alloc + 1) & ~1));
  }
  float2* nxs = cur + p_alloc;
  uint32_t* inP = rec0;
  uint32_t* wpreP = rec0 + 1;
  uint32_t* vis = rec0 + 2;

  const int src = (int)links[2 * (int64_t)l], dst = (int)links[2 * (int64_t)l + 1];
  const int msrc = sop2 ? -2 : src, mdst = sop2 ? -3 : dst;   // the endpoints as far as the MASKING is concerned
  auto gdinv = [&](int v) -> float {                          // sop2: D^-1/2 of the global degree
    const int d = indptr[v + 1] - indptr[v];
    return d > 0 ? 1.0f / sqrtf((float)d) : 0.0f;
  };

  // ---- BFS on the unmasked graph (reference utils.py:53-74) --------------------------------
  int nlev;
  int n;
  if (DM || (stash && n_alloc - 2 <= slot)) {
    // count_kernel left this link's node list (hop-major, ascending id inside a hop) and its
    // level ends in HBM: rebuild the LDS state from them instead of walking the graph again
    const int32_t* __restrict__ st = stash + (int64_t)l * slot;
    const int32_t* lv = out.lvl + (int64_t)l * kMaxLevels;   // rewritten below, after the barriers
    if constexpr (DM) {
      for (int t = tid; t < 16 * W; t += T) smem[t] = 0xffffffffu;
    } else if constexpr (HS) {
      for (uint32_t t = tid; t <= hmask; t += T) hkeys[t] = -1;
    } else {
      for (int t = tid; t < W; t += T) {
        vis[RS * t] = 0;
        inP[RS * t] = 0;
      }
    }
    nlev = lv[kMaxLevels - 1];
    if (tid < nlev) lvl_end[tid] = lv[tid];
    if (tid == 0) {
      list[0] = min(src, dst);
      list[1] = max(src, dst);
    }
    hub_rows_clear<T>(hub);
    __syncthreads();
    for (int t = tid; t < n_alloc; t += T) {
      const int v = t < 2 ? list[t] : st[t - 2];
      if (t >= 2) list[t] = v;
      if constexpr (DM) {
        dmap[v] = (uint16_t)t;
      } else if constexpr (HS) {
        hs_insert(hkeys, hmask, v);
        hvals[hs_find(hkeys, hmask, v)] = t;
      } else {
        atomicOr(&vis[RS * (v >> 5)], 1u << (v & 31));
      }
    }
    __syncthreads();
    n = n_alloc;
  } else if constexpr (HS) {
    n = bfs_hash<T, G>(indptr, indices, src, dst, hops, hkeys, hvals, hmask, list, n_alloc, lvl_end, sh + 31,
                       hub, nlev, ws, l);
  } else {
    n = bfs_list<T, G, RS>(indptr, indices, W, src, dst, hops, vis, inP, list, n_alloc, lvl_end, sh, hub, nlev,
                       ws, l, smp);
  }
  // set queries of the passes below: membership in S; index into the P-state arrays (+ is it in P);
  // the P-state index of list entry t (= node v)
  auto in_s = [&](int u) -> bool {
    if constexpr (DM) return dmap[u] != 0xffffu;
    else if constexpr (HS) return hs_find(hkeys, hmask, u) >= 0;
    else return test_bit<RS>(vis, u);
  };
  auto p_index_of_row = [&](int t, int v) -> int {
    if constexpr (HS) { (void)v; return t; }
    else { (void)t; return rank_of<RS>(inP, wpreP, v); }
  };

  phase_stamp(dbg, 0, t_prev);
  // ---- rows of this link ----------------------------------------------------------------
  const int64_t rp = out.row_ptr[l];
  const int R = (int)(out.row_ptr[l + 1] - rp);
  const LinkSlot ls{l, src, dst, mirror, noff, rp, mrp};
  const int max_row_hop = R > 2 ? 1 : 0;  // common neighbours sit at hop 1
  const int p = DIRECTED ? n : lvl_end[min(K - 1 + max_row_hop, nlev - 1)];

  // ---- P as bitmap + rank prefix; node list out -------------------------------------------
  if constexpr (!HS) {
    for (int t = tid; t < p; t += T) {
      const int v = list[t];
      atomicOr(&inP[RS * (v >> 5)], 1u << (v & 31));
    }
  }
  int vol_local = 0;   // vol(S) = Σ global degrees, the 4·vol(S) term of the algorithmic bytes
  for (int t = tid; t < n; t += T) {
    const int v = list[t];
    out.c_ids[noff + t] = ext_id(out, v);
    vol_local += indptr[v + 1] - indptr[v];
  }
  if (plus && wave_id() == 0) {
    const int c = common_neighbours(o_indptr, o_indices, in_s, src, dst, cn);
    sort_caller_order(cn, c, out.old_of_new, lane_id());
  }
  __syncthreads();
  if constexpr (!HS) rank_prefix<T, RS>(inP, wpreP, W, sh);
  __syncthreads();
  if (tid == 0)
    for (int d = 0; d < kMaxLevels; ++d) export_level(out, l, d, nlev, lvl_end[d], n);
  for (int r = tid; r < R; r += T) write_row_node(out, ls, r, row_node(r, src, dst, cn));

  phase_stamp(dbg, 1, t_prev);
  // ---- D^-1/2 on P (inf -> 0) -------------------------------------------------------------
  // reference tuned_SIGN.py:153-161: structure only, target link removed, no self-loops added
  // Only for the hops the row nodes themselves sit in (src/dst; the common neighbours at hop 1):
  // every later pass derives the D^-1/2 of the list rows it reaches for the first time from its
  // own walk of those rows (dinv_rows = how far that has got), so no row of P is walked for its
  // degree alone.
  int edges_local = 0;
  int edges_exact = -1;   // set when a pass of pair 0 walked every row of S
  int dinv_rows = DIRECTED ? n : lvl_end[min(max_row_hop, nlev - 1)];
  if (sop2) {
    for (int t = tid; t < dinv_rows; t += T) {
      const int v = list[t];
      dinvP[p_index_of_row(t, v)] = gdinv(v);
      edges_local += indptr[v + 1] - indptr[v];
    }
  } else if (!DIRECTED && !walks_on(ws) && !sampling_on(smp) && hops > max_row_hop) {
    // A plain BFS to `hops` holds every neighbour of a node that sits below hop `hops`: the
    // subgraph degree of such a row is its global degree, minus the masked target link at src and
    // dst (utils.py:79-80).  No walk.
    for (int t = tid; t < dinv_rows; t += T) {
      const int v = list[t];
      const int b = indptr[v], e = indptr[v + 1];
      int d = e - b;
      if (v == src || v == dst) d -= sorted_contains(indices + b, d, v == src ? dst : src) ? 1 : 0;
      dinvP[p_index_of_row(t, v)] = d > 0 ? 1.0f / sqrtf((float)d) : 0.0f;
      edges_local += d;
    }
  } else {
    walk_rows<T, G, 2>(
        0, dinv_rows, list, o_indptr, o_indices, hub,
        [&](RowAcc& a, int v, int u, bool valid) {
          // the target link is masked (utils.py:79-80): one compare per neighbour against the
          // row's partner (-1 for every row but src and dst; hoisted out of the neighbour loop)
          const int mp = v == msrc ? dst : (v == mdst ? src : -1);
          a.n += (valid && in_s(u) && u != mp) ? 1 : 0;
        },
        [&](RowAcc& a, int t, int v) {
          dinvP[p_index_of_row(t, v)] = a.n > 0 ? 1.0f / sqrtf((float)a.n) : 0.0f;
          edges_local += a.n;
        });
  }
  __syncthreads();

  phase_stamp(dbg, 2, t_prev);
  // ---- per row pair: K pull steps --------------------------------------------------------
  // State s_i[u] = dinv[u]·r_i[u] for u ∈ P (float2: rows a and b of the pair):
  //   r_i[w] = dinv[w] · Σ_{u ∈ N_S(w)} s_{i-1}[u]            (Â symmetric: pull == r_{i-1}·Â)
  // Each r_i[w] is summed in the stored order of w's row and reduced over G lanes by a fixed
  // xor tree: bit-reproducible.  All terms are >= 0: no cancellation.  A walk of length i
  // from a row at hop h_r stays within hop h_r + i, so step i only visits that list prefix;
  // the last step visits everything it can reach and derives dinv[w] from the same pass.
  // Small subgraphs that every operator reaches entirely (p == n: sign_k - 1 >= the BFS depth):
  // the first pass over all rows also records the masked induced adjacency as an n x n bit matrix
  // in LDS (row = list position, column = list position), and every later full pass — the
  // remaining operators, the last one, the passes of the common-neighbour pairs — sums over the
  // set bits of a row instead of walking its global CSR row through the bitmaps / the hash
  // (a 1-hop subgraph of a power-law graph has a few hundred induced edges and ~13 000 stored
  // neighbours).  Columns are list positions in both flavours of the visited set, so both sum in
  // the same order.
  const int WB = (n + 31) >> 5;
  // Hash flavour only (big graphs, where a visit costs a hash probe).  In the bitmap flavour it
  // measured a loss: USAir's 1-hop subgraphs are nearly as dense as their global rows (+20 % on
  // the link kernel), and on PubMed K=5 the matrix of a 300-500-node subgraph pushes the link
  // into a bigger LDS class (+10 %); the collab-scale config gains 12 %.
  const bool use_bm = HS && !DM && !GS && K >= 2 && p == n && p_alloc == n_alloc && n <= kBmMaxNodes && !sop2;
  uint32_t* bm = reinterpret_cast<uint32_t*>(nxs + p_alloc);              // [n][WB]
  uint16_t* pos_of_rank = reinterpret_cast<uint16_t*>(bm + (use_bm ? n * WB : 0));   // bitmap flavour
  uint16_t* rank_of_pos = pos_of_rank + n;
  bool bm_ready = false;
  if (use_bm) {
    for (int i = tid; i < n * WB; i += T) bm[i] = 0;
    if constexpr (!HS) {
      for (int t = tid; t < n; t += T) {
        const int r = rank_of<RS>(inP, wpreP, list[t]);
        pos_of_rank[r] = (uint16_t)t;
        rank_of_pos[t] = (uint16_t)r;
      }
    }
    __syncthreads();
  }
  // The graph is walked in descending degree order (lo_id >= 0: ids >= lo_id have at most two stored
  // neighbours), so the rows of a hop are sorted by length and its leaves form its tail.  The tail of
  // the LAST hop — a fifth of a PubMed subgraph's rows — is walked with one lane per row (both
  // neighbours in the lane's two slots, no tail loop) instead of G; two terms add up to the same
  // bits either way.
  int lo_begin = n;
  if (lo_id >= 0 && nlev >= 2 && !walks_on(ws)) {
    int lo = lvl_end[nlev - 2], hi = n;   // ascending ids inside the hop
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (list[mid] < lo_id) lo = mid + 1; else hi = mid;
    }
    lo_begin = lo;
  }
  // Only list rows 0 and 1 (src and dst) have a masked partner: the bitmap flavour walks every wavefront's slice
  // that holds neither with visit_plain, the same visit less the compare against the partner (-1 there).
  auto walk_split = [&](int limit, auto visit, auto visit_plain, auto commit) __attribute__((always_inline)) {
    const int a_end = min(limit, lo_begin);
    if constexpr (HS) {
      walk_rows<T, G, 2>(0, a_end, list, w_indptr, w_indices, hub, visit, commit);
      if (limit > a_end) walk_rows<T, 1, 2>(a_end, limit, list, w_indptr, w_indices, nullptr, visit, commit);
    } else {
      walk_rows_impl<T, G, 2, true>(0, a_end, list, w_indptr, w_indices, hub, visit, visit_plain, 2, commit);
      // (lo_begin lies in the last hop of a list of two hops at least: beyond rows 0 and 1)
      if (limit > a_end) walk_rows<T, 1, 2>(a_end, limit, list, w_indptr, w_indices, nullptr, visit_plain, commit);
    }
  };
  // Bitmap flavour: what a visit reads of u.  One record address; the bits of u in S and in P; and u's state at
  // its rank in P.  A non-member of P ranks anywhere in 0..p, and entry p of a state array is readable (the
  // spare entry below), so the rank needs no clamp; the visit adds the state only where u is in P.
  auto probe = [&](const float2* s, int u, uint32_t& in_set, uint32_t& in_p) -> float2 {
    // (bitmaps in LDS have far fewer than 2^24 words: the full-rate 24-bit multiply; 64-bit pointers otherwise)
    const uint32_t* rec = rec0 + (GS ? kSetRec * (u >> 5) : (int)__umul24((uint32_t)u >> 5, (uint32_t)kSetRec));
    const uint32_t wp = rec[0], pre = rec[1], wv = rec[2];
    // (bit-field extracts: the hardware takes offset and width from the low five bits of u by itself)
    int r = (int)pre + __popc(__builtin_amdgcn_ubfe(wp, 0u, (uint32_t)u));
    // (kept whole: popcount-and-add, then shift-and-add onto the array's base; the optimiser otherwise scales
    // the two terms separately, two instructions more)
    asm("" : "+v"(r));
    in_set = __builtin_amdgcn_ubfe(wv, (uint32_t)u, 1u);
    in_p = __builtin_amdgcn_ubfe(wp, (uint32_t)u, 1u);
    return s[r];
  };
  typedef std::integral_constant<bool, true> Masked;
  typedef std::integral_constant<bool, false> Plain;
  const int npairs = (R + 1) / 2;
  for (int pr = 0; pr < npairs; ++pr) {
    const int64_t jid = out.job_off[l] + pr;
    // PoS: one pair per link, its list sits at the link's node offset; PoS Plus: per-pair offsets
    const int64_t coff = out.coef_off ? out.coef_off[jid] : noff;
    int node_a, node_b;
    pair_rows(pr, R, src, dst, cn, node_a, node_b);
    const int row_hop = pr == 0 ? 0 : 1;
    const int support = lvl_end[min(K + row_hop, nlev - 1)];
    // the middle operators' zeros end here (the last of them reaches lvl_end[K - 1 + row_hop])
    const int zero_end = coef_zero_end(lvl_end[min(K - 1 + row_hop, nlev - 1)], support);
    // with full_stats the last pass also walks the rows beyond its reach, to count edges
    const int last_rows = (pr == 0 && full_stats) ? n : support;

    // Bitmap flavour: one entry more, the spare entry a visit reads at rank p (probe above).  cur's is nxs[0]
    // where p fills the array; nxs's lies in the 16 bytes link_lds_need keeps behind the arrays, of which the
    // alignment of cur takes 4 at most.
    for (int w = tid; w < p + (HS ? 0 : 1); w += T) {
      cur[w] = make_float2(0.f, 0.f);
      nxs[w] = make_float2(0.f, 0.f);
    }
    if (tid < 4 * K) zbuf[tid] = 0.f;
    __syncthreads();
    if (tid == 0) {
      auto p_index = [&](int v) -> int {
        if constexpr (DM) return (int)dmap[v];
        else if constexpr (HS) return hvals[hs_find(hkeys, hmask, v)];
        else return rank_of<RS>(inP, wpreP, v);
      };
      const int la = p_index(node_a);
      cur[la].x = dinvP[la];
      if (node_b >= 0) {
        const int lb = p_index(node_b);
        cur[lb].y = dinvP[lb];
      }
    }
    __syncthreads();

    float2* s_in = cur;
    float2* s_out = nxs;
    float2* coef = reinterpret_cast<float2*>(out.c_coef) + coff * K;  // [K][support] float2
    // A list longer than split_t entries is cut into pieces that the gather treats as jobs of their
    // own (s3grl_internal.hpp, kSplitThreshold, coef_index)
    const bool split = split_list(out, support);
    auto cidx = [&](int i, int t) -> int64_t { return coef_index(i, t, support, K, split, out.seg_shift); };
    // one operator step over ALL rows through the bit matrix: WL lanes per row (one word of the
    // row each, WL = the row's word count rounded up to a power of two, at most 16), the set
    // bits of a word in ascending position, then a fixed xor tree over the WL lanes:
    // bit-reproducible, and the same order in both flavours of the visited set
    int edges_bm = 0;
    const int wl_shift = WB <= 1 ? 0 : (WB <= 2 ? 1 : (WB <= 4 ? 2 : (WB <= 8 ? 3 : 4)));
    auto bm_pass = [&](int i, bool last) {
      const int WL = 1 << wl_shift;
      const int j0 = tid & (WL - 1);
      for (int base = 0; base < n; base += T >> wl_shift) {
        const int t = base + (tid >> wl_shift);
        float ax = 0.f, ay = 0.f;
        int deg = 0;
        if (t < n) {
          for (int j = j0; j < WB; j += WL) {
            uint32_t w32 = bm[t * WB + j];
            deg += __popc(w32);
            while (w32) {
              const int c = j * 32 + __ffs(w32) - 1;
              w32 &= w32 - 1;
              int idx = c;
              if constexpr (!HS) idx = rank_of_pos[c];
              const float2 sv = s_in[idx];
              ax += sv.x;
              ay += sv.y;
            }
          }
        }
        for (int o = WL >> 1; o > 0; o >>= 1) {   // WL divides 64: the partners are in this wave
          ax += __shfl_xor(ax, o);
          ay += __shfl_xor(ay, o);
          deg += __shfl_xor(deg, o);
        }
        if (t < n && j0 == 0) {
          edges_bm += deg;
          const int v = list[t];
          int w = t;
          if constexpr (!HS) w = rank_of_pos[t];
          const float dw = dinvP[w];
          const float rx = dw * ax, ry = dw * ay;
          if (!last) s_out[w] = make_float2(dw * rx, dw * ry);
          coef[cidx(i, t)] = make_float2(rx, ry);
          if (v == src) { zbuf[(0 * K + i) * 2] = rx; zbuf[(0 * K + i) * 2 + 1] = ry; }
          if (v == dst) { zbuf[(1 * K + i) * 2] = rx; zbuf[(1 * K + i) * 2 + 1] = ry; }
        }
      }
    };
#pragma unroll 1
    for (int i = 0; i < K - 1; ++i) {
      const int limit = lvl_end[min(i + 1 + row_hop, nlev - 1)];  // <= p
      if (bm_ready && limit == n) {
        bm_pass(i, false);
        __syncthreads();
        float2* tmp = s_in;
        s_in = s_out;
        s_out = tmp;
        continue;
      }
      const bool build_bm = use_bm && !bm_ready && limit == n;   // first pass over all rows
      auto mid_visit = [&](auto masked, RowAcc& a, int v, int u, bool valid) __attribute__((always_inline)) {
            bool on;
            float2 sv;
            bool member;
            int col = 0;   // list position of u (meaningful for members; hash flavour only)
            if constexpr (DM) {
              const int r = dmap[u];   // list position; 0xFFFF (>= p) = not in S
              sv = s_in[min(r, p - 1)];
              member = valid && r != 0xffff;
              on = valid && r < p;
              col = r;
            } else if constexpr (HS) {
              const int slot = hs_find(hkeys, hmask, u);
              const int r = hvals[max(slot, 0)];
              sv = s_in[min(max(r, 0), p - 1)];
              member = valid && slot >= 0;
              on = member && r < p;
              col = r;
            } else {
              // all LDS reads unconditional, count and contribution selected afterwards (P is a subset of S:
              // the bit of P alone says whether the state counts)
              uint32_t in_set, in_p;
              sv = probe(s_in, u, in_set, in_p);
              member = valid && in_set;
              on = valid && in_p;
            }
            if constexpr (decltype(masked)::value) {
              const int mp = v == msrc ? dst : (v == mdst ? src : -1);
              member = member && u != mp;
              on = on && u != mp;
            }
            if (build_bm && member) {
              if constexpr (!HS) col = pos_of_rank[min(col, n - 1)];
              atomicOr(&bm[a.row * WB + (col >> 5)], 1u << (col & 31));
            }
            a.n += member ? 1 : 0;
            a.x += on ? sv.x : 0.f;
            a.y += on ? sv.y : 0.f;
          };
      walk_split(
          limit,
          [&](RowAcc& a, int v, int u, bool valid) { mid_visit(Masked{}, a, v, u, valid); },
          [&](RowAcc& a, int v, int u, bool valid) { mid_visit(Plain{}, a, v, u, valid); },
          [&](RowAcc& a, int t, int v) {
            const int w = p_index_of_row(t, v);
            float dw;
            if (t >= dinv_rows) {   // first pass to reach this row: its degree comes from this walk
              dw = sop2 ? gdinv(v) : (a.n > 0 ? 1.0f / sqrtf((float)a.n) : 0.0f);
              dinvP[w] = dw;
              edges_local += a.n;
            } else {
              dw = dinvP[w];
            }
            const float rx = dw * a.x, ry = dw * a.y;
            s_out[w] = make_float2(dw * rx, dw * ry);
            // (sop2: the partner's column is zeroed in the product with X — tuned_SIGN.py:73-76)
            coef[cidx(i, t)] = make_float2((sop2 && v == dst) ? 0.f : rx, (sop2 && v == src) ? 0.f : ry);
            // label column of operator i+1: Σ_w r[w] z_w = r[src] + r[dst]  (tuned_SIGN.py:177-185)
            if (v == src) { zbuf[(0 * K + i) * 2] = rx; zbuf[(0 * K + i) * 2 + 1] = ry; }
            if (v == dst) { zbuf[(1 * K + i) * 2] = rx; zbuf[(1 * K + i) * 2 + 1] = ry; }
          });
      // zeros only where a reader multiplies without asking for the limit (coef_zero_end); the rest of the
      // list — on a deep plan most of it — is left unwritten for this operator
      for (int t = limit + tid; t < zero_end; t += T) coef[cidx(i, t)] = make_float2(0.f, 0.f);
      dinv_rows = max(dinv_rows, limit);
      if (build_bm) bm_ready = true;
      __syncthreads();
      float2* tmp = s_in;
      s_in = s_out;
      s_out = tmp;
    }
    phase_stamp(dbg, 3, t_prev);
    if (bm_ready && last_rows == n && support == n) {   // last operator through the bit matrix
      edges_bm = 0;
      bm_pass(K - 1, true);
      if (pr == 0) edges_exact = edges_bm;
      __syncthreads();
    } else {  // last operator: degree and sum of every reachable row in one pass over its CSR row
      const int i = K - 1;
      int edges_pass = 0;
      auto last_visit = [&](auto masked, RowAcc& a, int v, int u, bool valid) __attribute__((always_inline)) {
            bool member, on;
            float2 sv;
            if constexpr (DM) {
              const int r = dmap[u];
              sv = s_in[min(r, p - 1)];
              member = valid && r != 0xffff;
              on = valid && r < p;
            } else if constexpr (HS) {
              const int slot = hs_find(hkeys, hmask, u);
              const int r = hvals[max(slot, 0)];
              sv = s_in[min(max(r, 0), p - 1)];
              member = valid && slot >= 0;
              on = member && r < p;
            } else {
              // all LDS reads unconditional, count and contribution selected afterwards (see mid_visit)
              uint32_t in_set, in_p;
              sv = probe(s_in, u, in_set, in_p);
              member = valid && in_set;
              on = valid && in_p;
            }
            if constexpr (decltype(masked)::value) {
              const int mp = v == msrc ? dst : (v == mdst ? src : -1);
              member = member && u != mp;
              on = on && u != mp;
            }
            a.n += member ? 1 : 0;
            a.x += on ? sv.x : 0.f;
            a.y += on ? sv.y : 0.f;
          };
      walk_split(
          last_rows,
          [&](RowAcc& a, int v, int u, bool valid) { last_visit(Masked{}, a, v, u, valid); },
          [&](RowAcc& a, int v, int u, bool valid) { last_visit(Plain{}, a, v, u, valid); },
          [&](RowAcc& a, int t, int v) {
            edges_pass += a.n;
            if (t < support) {
              // (directed: a.n counted predecessors; D^-1/2 is the out-degree's, known for all of S)
              const float dw = DIRECTED ? dinvP[p_index_of_row(t, v)]
                                        : (sop2 ? gdinv(v) : (a.n > 0 ? 1.0f / sqrtf((float)a.n) : 0.0f));
              const float rx = dw * a.x, ry = dw * a.y;
              coef[cidx(i, t)] = make_float2((sop2 && v == dst) ? 0.f : rx, (sop2 && v == src) ? 0.f : ry);
              if (v == src) { zbuf[(0 * K + i) * 2] = rx; zbuf[(0 * K + i) * 2 + 1] = ry; }
              if (v == dst) { zbuf[(1 * K + i) * 2] = rx; zbuf[(1 * K + i) * 2 + 1] = ry; }
            }
          });
      if (pr == 0 && last_rows == n) edges_exact = edges_pass;
      __syncthreads();
    }
    phase_stamp(dbg, 4, t_prev);
    if (tid < 2 * K) {
      const int i = tid >> 1, r = tid & 1;
      // label column of operator i+1: r[src] + r[dst]; sop2: the diagonal entry — r_a[src] for row a, r_b[dst] for b
      out.job_z[(jid * K + i) * 2 + r] = sop2 ? zbuf[(r * K + i) * 2 + r]
                                          : zbuf[(0 * K + i) * 2 + r] + zbuf[(1 * K + i) * 2 + r];
    }
    // operator i+1 reaches the list prefix within i+1 hops of the row (the limits of the passes
    // above): the gather skips its multiply-adds beyond that
    end_pair(out, ls, tid, K, pr, jid, coff, support, node_a, node_b, split,
             [&](int i) { return i == K - 1 ? support : lvl_end[min(i + 1 + row_hop, nlev - 1)]; });
    __syncthreads();
  }
  // edges of the masked induced subgraph: exact when the last pass of pair 0 covered all of S
  // (always with full_stats; otherwise whenever K >= num_hops), else the edges of P's rows
  phase_stamp(dbg, 5, t_prev);
  edges_local = block_sum<T>(edges_exact >= 0 ? edges_exact : edges_local, sh);
  vol_local = block_sum<T>(vol_local, sh);
  if (tid == 0) commit_link_stats(out, mirror, edges_local, vol_local);
}

// ---------------------------------------------------------------------------------------
// One-hop plans on big graphs.
//
// The reference's own answer to large graphs is num_hops = 1 (reference utils.py:57-74 with
// num_hops = 1: S = {src,dst} ∪ N(src) ∪ N(dst)).  On a power-law graph such a subgraph has a few
// hundred induced edges but its nodes store ~10^4 neighbours (hubs), and with sign_k - 1 >= 1 every
// operator reaches all of S.  Walking the global rows through a hash of S for every operator
// (link_kernel, HS flavour) costs vol(S) probes per pass.  Here instead:
//
//   count1_kernel     n = |S|, R, and a bound of the induced entries — by intersecting the two
//                     sorted rows (binary searches), one wavefront per link, no bitmaps: no limit
//                     on the number of nodes of the graph (s3grl_structure.hip).
//   link_full_kernel  S by a rank merge of the two sorted rows (canonical order: ascending id),
//                     the masked induced adjacency ONCE as an n x n bit matrix through the
//                     degree-ORIENTED rows (`fwd`: only the neighbours of higher (degree, id); a
//                     hub's oriented row is short, Σ over S is ~10x smaller than vol(S)), from it a
//                     CSR of local ids in LDS, and every operator as a pull over that CSR.
//
// Same rows, same coefficients as link_kernel up to the summation order (ascending local id here,
// stored order of the global row there).

// ---- the fused per-link kernel of the full-reach one-hop case ------------------------------------
// LDS (dynamic): [hkeys C | hvals C]  (aliased by the float2 state arrays cur[n], nxs[n] once the
// probes are done: 8C >= 16n)  cn[cn_cap] cnpos[cn_cap] lvl_end[2] zbuf[4K] sh[32]
// list[n] dinv[n] off[n+1] cols[ecap] (uint16 local ids) bm[n][WB]
// (BMG, the class of the biggest subgraphs: no matrix; cols and the list of found edges in a
// per-workgroup HBM slice, four per-wave sort bitmaps of WB words behind off[])
template <int T, int K, bool BMG>
__global__ __launch_bounds__(T, (T <= 256 ? 8 : 1)) void link_full_kernel(
    const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const int32_t* __restrict__ fwd_indptr, const int32_t* __restrict__ fwd_indices,
    const int64_t* __restrict__ links, const int32_t* __restrict__ class_list, int count, int plus,
    int cn_cap, const int32_t* __restrict__ e_cap, const int64_t* __restrict__ node_off, const int64_t* __restrict__ row_ptr,
    const int64_t* __restrict__ job_off, const int64_t* __restrict__ coef_off,
    const int32_t* __restrict__ mirror_of, int32_t* __restrict__ c_ids, float* __restrict__ c_coef,
    Job* __restrict__ jobs, float* __restrict__ job_z, int32_t* __restrict__ job_lim,
    int64_t* __restrict__ row_nodes, int32_t* __restrict__ lvl, unsigned long long* __restrict__ tot_edges,
    unsigned long long* __restrict__ tot_support, unsigned long long* __restrict__ tot_vol,
    const int32_t* __restrict__ old_of_new, int split_t, int seg_shift,
    uint32_t* __restrict__ bm_scratch, int64_t bm_stride_words, int lds_bytes, unsigned long long* __restrict__ dbg) {
  extern __shared__ uint32_t smem[];
  const int tid = threadIdx.x;
  constexpr int G = 4;
  // The LinkOut the output helpers take, built here from __restrict__ parameters: its members as a by-value
  // kernel parameter carry no noalias, which cost this kernel up to 10 VGPRs (and spills) per instantiation.
  const LinkOut out{node_off, row_ptr, job_off, coef_off, mirror_of, c_ids, c_coef, jobs, job_z, job_lim,
                    row_nodes, lvl, tot_edges, tot_support, tot_vol, old_of_new, split_t, seg_shift};
  // diagnostic only (S3GRL_DEBUG_STAMPS): phase_stamp into slots 8..15
  unsigned long long t_prev = dbg ? __builtin_amdgcn_s_memtime() : 0ull;
  // BMG: a persistent grid, every workgroup owns one bit-matrix slice and strides over the class
  for (int item = blockIdx.x; item < count; item += gridDim.x) {
    const int l = class_list[item];
    const int64_t noff = out.node_off[l];
    const int n = (int)(out.node_off[l + 1] - noff);
    const int ecap = (e_cap[l] + 1) & ~1;
    const int mirror = out.mirror_of ? out.mirror_of[l] : -1;
    const int64_t mrp = mirror >= 0 ? out.row_ptr[mirror] : -1;
    const int C = full_hash_slots(n);
    const uint32_t hmask = (uint32_t)(C - 1);
    const int WB = (n + 31) >> 5;
    int32_t* hkeys = reinterpret_cast<int32_t*>(smem);
    int32_t* hvals = hkeys + C;
    float2* cur = reinterpret_cast<float2*>(smem);          // aliases the hash (used after the probes)
    float2* nxs = cur + n;
    int32_t* cn = reinterpret_cast<int32_t*>(smem + 2 * C);
    int32_t* cnpos = cn + cn_cap;
    int* lvl_end = cnpos + cn_cap;                           // [2]
    float* zbuf = reinterpret_cast<float*>(lvl_end + 2);     // [2][K][2]
    int* sh = reinterpret_cast<int*>(zbuf + 4 * K);          // [32]
    uint16_t* longrows = reinterpret_cast<uint16_t*>(sh + 32);   // [kLongCap]
    int32_t* list = sh + 32 + kLongCap / 2;
    float* dinv = reinterpret_cast<float*>(list + n);
    int32_t* off = reinterpret_cast<int32_t*>(dinv + n);     // [n+1]
    // On-chip classes: CSR columns and an n x n bit matrix in LDS.  Big class (BMG): the columns
    // and a list of the found edges sit in this workgroup's HBM slice and there is no matrix — the
    // CSR is built from the edge list (degree count, scan, scatter) and every row is then sorted,
    // so that the sums run in ascending local id like in the on-chip classes.
    uint16_t* cols_l = reinterpret_cast<uint16_t*>(off + n + 1 + ((n + 1) & 1));
    uint32_t* bm_l = reinterpret_cast<uint32_t*>(cols_l + ecap);
    uint32_t* elist = bm_scratch + (int64_t)blockIdx.x * bm_stride_words;              // [ecap / 2]
    uint16_t* cols_g = reinterpret_cast<uint16_t*>(elist + ((ecap / 2 + 1) & ~1));         // [ecap]
    uint32_t* sortbm = reinterpret_cast<uint32_t*>(off + n + 1);                         // [T/64][WB] (BMG)
    // BMG: the columns stay on chip after all when the EXACT entry count (known once the degrees
    // are) fits what the class's LDS leaves — the bound the class was chosen by is loose
    uint16_t* cols_b = reinterpret_cast<uint16_t*>(sortbm + (T / 64) * WB);
    const int cols_b_cap = (lds_bytes - (int)(reinterpret_cast<char*>(cols_b) - reinterpret_cast<char*>(smem))) / 2;
    bool big_on_chip = false;
    auto cols_ld = [&](int k) -> int {
      if constexpr (BMG) return big_on_chip ? cols_b[k] : cols_g[k]; else return cols_l[k];
    };
    auto cols_st = [&](int k, int v) {
      if constexpr (BMG) {
        if (big_on_chip) cols_b[k] = (uint16_t)v; else cols_g[k] = (uint16_t)v;
      } else {
        cols_l[k] = (uint16_t)v;
      }
    };

    const int src = (int)links[2 * (int64_t)l], dst = (int)links[2 * (int64_t)l + 1];
    const int32_t* __restrict__ rs = indices + indptr[src];
    const int32_t* __restrict__ rd = indices + indptr[dst];
    const int cs = indptr[src + 1] - indptr[src], cd = indptr[dst + 1] - indptr[dst];

    // ---- S in canonical order: {min,max}, then N(src) ∪ N(dst) \ {src,dst} ascending ------------
    // rank merge of the two sorted rows: element x of one row lands at (its index among the row's
    // own members) + (members of the other row below x) - (common members below x).  Phase 1 keeps
    // (lower bound in the other row, common?, member?) per element in `tmp` (the hash's space:
    // 4(cs+cd) <= 8n <= 4C... the two tables together hold 2C >= 4n words); phase 2 turns the
    // per-row prefix counts of "common" into positions.
    // both rows are staged in LDS first (the hash's space holds 2C >= 4n >= 2(cs + cd) words):
    // the searches then cost LDS latency instead of a dozen dependent trips to L2 each
    int32_t* rows_l = reinterpret_cast<int32_t*>(smem);   // [cs + cd]: row src, then row dst
    uint32_t* tmp = smem + (cs + cd);                     // [cs + cd]
    for (int e = tid; e < cs + cd; e += T) rows_l[e] = e < cs ? rs[e] : rd[e - cs];
    if (tid == 0) {
      list[0] = min(src, dst);
      list[1] = max(src, dst);
      lvl_end[0] = 2;
      lvl_end[1] = n;
      sh[29] = 0;   // long rows registered
    }
    __syncthreads();
    const int32_t* rs_l = rows_l;
    const int32_t* rd_l = rows_l + cs;
    const bool s_has_s = sorted_contains(rs_l, cs, src), s_has_d = sorted_contains(rs_l, cs, dst);
    const bool d_has_s = sorted_contains(rd_l, cd, src), d_has_d = sorted_contains(rd_l, cd, dst);
    for (int e = tid; e < cs + cd; e += T) {
      const bool from_s = e < cs;
      const int x = rows_l[e];
      const bool member = x != src && x != dst;
      const int lb = from_s ? row_lower_bound(rd_l, cd, x) : row_lower_bound(rs_l, cs, x);
      const bool dup = member && (from_s ? (lb < cd && rd_l[lb] == x) : (lb < cs && rs_l[lb] == x));
      tmp[e] = ((uint32_t)lb << 2) | (dup ? 2u : 0u) | (member ? 1u : 0u);
    }
    __syncthreads();
    for (int side = 0; side < 2; ++side) {
      const int base = side == 0 ? 0 : cs, len = side == 0 ? cs : cd;
      const int32_t* row = rows_l + base;
      const int per = (len + T - 1) / T;
      const int e0 = min(tid * per, len), e1 = min(e0 + per, len);
      int dups = 0;
      for (int e = e0; e < e1; ++e) dups += (tmp[base + e] >> 1) & 1u;
      int total;
      int c = block_excl_scan<T>(dups, sh, total);
      // excluded entries (src, dst themselves) below x, in this row and in the other one
      const bool own_s = side == 0 ? s_has_s : d_has_s, own_d = side == 0 ? s_has_d : d_has_d;
      const bool oth_s = side == 0 ? d_has_s : s_has_s, oth_d = side == 0 ? d_has_d : s_has_d;
      for (int e = e0; e < e1; ++e) {
        const uint32_t w = tmp[base + e];
        const bool dup = (w >> 1) & 1u;
        if ((w & 1u) && !(side == 1 && dup)) {       // common members are emitted from row src only
          const int x = row[e];
          const int own = e - ((own_s && src < x) ? 1 : 0) - ((own_d && dst < x) ? 1 : 0);
          const int oth = (int)(w >> 2) - ((oth_s && src < x) ? 1 : 0) - ((oth_d && dst < x) ? 1 : 0);
          const int pos = 2 + own + oth - c;
          if (pos < n) list[pos] = x;
        }
        c += dup ? 1 : 0;
      }
    }
    __syncthreads();   // list complete, tmp dead
    phase_stamp(dbg, 8 + 0, t_prev);

    // ---- hash of S (probe structure), node list out, bit matrix zeroed --------------------------
    for (uint32_t t = tid; t <= hmask; t += T) hkeys[t] = -1;
    if constexpr (BMG) {
      for (int t = tid; t <= n; t += T) off[t] = 0;            // degree counters
      if (tid == 0) sh[30] = 0;                                // edges found
    } else {
      for (int i = tid; i < n * WB; i += T) bm_l[i] = 0;
    }
    __syncthreads();
    int vol_local = 0;
    // (on-chip classes: the bounds of the oriented rows are fetched here, with the other per-node loads —
    // the probes below then start from LDS.  They sit in dinv's / off's space, unused until the CSR is built.)
    int32_t* qstart = reinterpret_cast<int32_t*>(dinv);   // [n] first entry of node t's oriented row
    int32_t* qoff = off;                                    // [n + 1] running offsets of those rows
    for (int t = tid; t < n; t += T) {
      const int v = list[t];
      hs_insert(hkeys, hmask, v);
      hvals[hs_find(hkeys, hmask, v)] = t;
      out.c_ids[noff + t] = ext_id(out, v);
      vol_local += indptr[v + 1] - indptr[v];
      if constexpr (!BMG) {
        const int fb = fwd_indptr[v];
        qstart[t] = fb;
        qoff[t] = fwd_indptr[v + 1] - fb;
      }
    }
    const int64_t rp = out.row_ptr[l];
    const int R = (int)(out.row_ptr[l + 1] - rp);
    const LinkSlot ls{l, src, dst, mirror, noff, rp, mrp};
    __syncthreads();
    if (plus && tid < 64) {
      const int c =
          common_neighbours(indptr, indices, [&](int x) { return hs_find(hkeys, hmask, x) >= 0; }, src, dst, cn);
      sort_caller_order(cn, c, out.old_of_new, tid);
    }
    if (tid == 0)
      for (int dd = 0; dd < kMaxLevels; ++dd) export_level(out, l, dd, 1, 2, n);
    __syncthreads();
    for (int r = tid; r < R; r += T) {
      const int node = row_node(r, src, dst, cn);
      write_row_node(out, ls, r, node);
      if (r >= 2) cnpos[r - 2] = hvals[hs_find(hkeys, hmask, node)];
    }
    const int pos_src = src < dst ? 0 : 1, pos_dst = 1 - pos_src;
    phase_stamp(dbg, 8 + 1, t_prev);

    // ---- masked induced adjacency through the oriented rows (reference utils.py:76-80) ----------
    if constexpr (!BMG) {
      // The oriented rows are walked FLAT: entry e of their concatenation by thread e mod T — a subgraph of
      // 25 nodes has ~40 oriented entries, and a walk with four lanes per row paid two dependent global
      // round trips (bounds, then entries) for rows of one or two entries; here the bounds are in LDS.
      {
        const int per = (n + T - 1) / T;
        const int t0 = min(tid * per, n), t1 = min(t0 + per, n);
        int mine = 0;
        for (int t = t0; t < t1; ++t) mine += qoff[t];
        int total;
        int run = block_excl_scan<T>(mine, sh, total);
        for (int t = t0; t < t1; ++t) {
          const int len = qoff[t];
          qoff[t] = run;
          run += len;
        }
        if (tid == 0) qoff[n] = total;
      }
      __syncthreads();
      const int walk_total = qoff[n];
      for (int e = tid; e < walk_total; e += T) {
        int ra = 0, rb = n;   // the row holding entry e: last r with qoff[r] <= e
        while (rb - ra > 1) {
          const int mid = (ra + rb) >> 1;
          if (qoff[mid] <= e) ra = mid; else rb = mid;
        }
        const int u = fwd_indices[qstart[ra] + (e - qoff[ra])];
        const int v = list[ra];
        const int slot = hs_find(hkeys, hmask, u);
        const bool target = (v == src && u == dst) || (v == dst && u == src);
        if (slot >= 0 && !target) {
          const int i = ra, j = hvals[slot];
          atomicOr(&bm_l[i * WB + (j >> 5)], 1u << (j & 31));
          if (i != j) atomicOr(&bm_l[j * WB + (i >> 5)], 1u << (i & 31));
        }
      }
    } else {
    walk_rows<T, G, 2>(
        0, n, list, fwd_indptr, fwd_indices, nullptr,
        [&](RowAcc& a, int v, int u, bool valid) {
          const int slot = hs_find(hkeys, hmask, u);
          const int j = hvals[max(slot, 0)];
          const int i = a.row;
          const bool target = (v == src && u == dst) || (v == dst && u == src);
          const bool found = valid && slot >= 0 && !target;
          if constexpr (BMG) {
            // one LDS atomic per wavefront for the list position (the visit is called by all lanes)
            const unsigned long long fm = __ballot(found);
            int base = 0;
            if (fm) {
              const int leader = __ffsll((long long)fm) - 1;
              if ((tid & 63) == leader) base = atomicAdd(&sh[30], __popcll(fm));
              base = __shfl(base, leader);
            }
            if (found) {
              const int k = base + __popcll(fm & ((1ull << (tid & 63)) - 1ull));
              if (2 * k < ecap) elist[k] = ((uint32_t)i << 16) | (uint32_t)j;
              atomicAdd(&off[i], 1);
              if (i != j) atomicAdd(&off[j], 1);
            }
          } else if (found) {
            atomicOr(&bm_l[i * WB + (j >> 5)], 1u << (j & 31));
            if (i != j) atomicOr(&bm_l[j * WB + (i >> 5)], 1u << (i & 31));
          }
        },
        [](RowAcc&, int, int) {});
    }
    if constexpr (BMG) __threadfence();   // the edge list is read back by other waves (through L2)
    __syncthreads();
    phase_stamp(dbg, 8 + 2, t_prev);

    // ---- degrees, D^-1/2 (inf -> 0), CSR of local ids (ascending) --------------------------------
    if constexpr (BMG) {
      int32_t* cursor = hvals;              // the hash values are dead: positions were copied out
      const int per = (n + T - 1) / T;
      const int t0 = min(tid * per, n), t1 = min(t0 + per, n);
      int mine = 0;
      for (int t = t0; t < t1; ++t) mine += off[t];
      int total;
      int run = block_excl_scan<T>(mine, sh, total);
      for (int t = t0; t < t1; ++t) {
        const int dg = off[t];
        dinv[t] = dg > 0 ? 1.0f / sqrtf((float)dg) : 0.0f;
        off[t] = run;
        cursor[t] = run;
        run += dg;
      }
      if (tid == 0) off[n] = total;
      big_on_chip = total <= cols_b_cap;
      if (dbg && tid == 0) {   // diagnostic: links of the class / whose columns had to stay in the HBM slice
        atomicAdd(&dbg[8 + 6], 1ull);
        if (!big_on_chip) atomicAdd(&dbg[8 + 7], 1ull);
      }
      __syncthreads();
      const int found = min(sh[30], ecap / 2);
      for (int k = tid; k < found; k += T) {
        const uint32_t w = elist[k];
        const int i = (int)(w >> 16), j = (int)(w & 0xffffu);
        cols_st(atomicAdd(&cursor[i], 1), j);
        if (i != j) cols_st(atomicAdd(&cursor[j], 1), i);
      }
      if (!big_on_chip) __threadfence();
      __syncthreads();
      // every row ascending: one wavefront per row.  Short rows by rank (each lane counts the
      // smaller entries), long ones through a per-wave bitmap of the n local ids.
      const int lane = tid & 63, wv = tid >> 6;
      uint32_t* wbm = sortbm + wv * WB;
      // (a) rows of at most 16 entries — nearly all of them — four at a time per wavefront
      {
        const int sub = lane >> 4, sl = lane & 15;
        for (int r0 = wv * 4; r0 < n; r0 += (T / 64) * 4) {
          const int r = min(r0 + sub, n - 1);
          const int b = off[r], len = off[r + 1] - b;
          const bool mine = r0 + sub < n && len > 1 && len <= 16;
          const int x = mine && sl < len ? cols_ld(b + sl) : 0x7fffffff;
          int rank = 0;
#pragma unroll
          for (int k = 0; k < 16; ++k) rank += __shfl(x, (lane & 48) + k) < x ? 1 : 0;
          if (mine && sl < len) cols_st(b + rank, x);
        }
      }
      // (b) longer rows, one wavefront each: by rank up to 64 entries, through a bitmap beyond
      for (int r = wv; r < n; r += T / 64) {
        const int b = off[r], len = off[r + 1] - b;
        if (len <= 16) continue;
        if (len <= 64) {
          const int x = lane < len ? cols_ld(b + lane) : 0x7fffffff;
          int rank = 0;
          for (int k = 0; k < len; ++k) rank += __shfl(x, k) < x ? 1 : 0;
          if (lane < len) cols_st(b + rank, x);
        } else {
          for (int w = lane; w < WB; w += 64) wbm[w] = 0;
          for (int k = lane; k < len; k += 64) {
            const int c = cols_ld(b + k);
            atomicOr(&wbm[c >> 5], 1u << (c & 31));
          }
          int base = b;
          for (int w0 = 0; w0 < WB; w0 += 64) {
            uint32_t word = w0 + lane < WB ? wbm[w0 + lane] : 0u;
            const int cnt = __popc(word);
            int inc = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
              const int t = __shfl_up(inc, o);
              if (lane >= o) inc += t;
            }
            int k = base + inc - cnt;
            while (word) {
              const int bit = __ffs(word) - 1;
              word &= word - 1;
              cols_st(k++, (w0 + lane) * 32 + bit);
            }
            base += __shfl(inc, 63);
          }
        }
      }
      if (!big_on_chip) __threadfence();
    } else {
      const int per = (n + T - 1) / T;
      const int t0 = min(tid * per, n), t1 = min(t0 + per, n);
      int mine = 0;
      for (int t = t0; t < t1; ++t) {
        int dg = 0;
        for (int j = 0; j < WB; ++j) dg += __popc(bm_l[t * WB + j]);
        mine += dg;
      }
      int total;
      int run = block_excl_scan<T>(mine, sh, total);
      for (int t = t0; t < t1; ++t) {
        off[t] = run;
        int k = run;
        for (int j = 0; j < WB; ++j) {
          uint32_t w = bm_l[t * WB + j];
          while (w) {
            const int b = __ffs(w) - 1;
            w &= w - 1;
            if (k < ecap) cols_l[k] = (uint16_t)(j * 32 + b);
            ++k;
          }
        }
        const int dg = k - run;
        dinv[t] = dg > 0 ? 1.0f / sqrtf((float)dg) : 0.0f;
        run = k;
      }
      if (tid == 0) off[n] = total;
    }
    __syncthreads();   // hash dead from here: cur / nxs take its space
    phase_stamp(dbg, 8 + 3, t_prev);
    const int edges_total = off[n];
    // Long rows (src and dst are adjacent to about half of a one-hop subgraph each, a hub inside
    // it to more): four lanes would stride such a row for hundreds of trips while the rest of the
    // workgroup waits at the barrier of the pass.  They are registered here (sign bit of their
    // D^-1/2 as the per-row flag) and summed by a whole wavefront each, after the short rows.
    // (the first kLongCap of them in row order — a block scan, not the order of an atomic: which rows
    // get a wavefront decides the last bit of their sums)
    int nlong;
    {
      const int per = (n + T - 1) / T;
      const int t0 = min(tid * per, n), t1 = min(t0 + per, n);
      int mine = 0;
      for (int t = t0; t < t1; ++t) mine += off[t + 1] - off[t] > kLongRow ? 1 : 0;
      int total;
      int q = block_excl_scan<T>(mine, sh, total);
      for (int t = t0; t < t1; ++t) {
        if (off[t + 1] - off[t] > kLongRow) {
          if (q < kLongCap) {
            longrows[q] = (uint16_t)t;
            dinv[t] = -dinv[t];
          }
          ++q;
        }
      }
      nlong = min(total, kLongCap);
    }
    __syncthreads();

    // ---- per row pair: K pulls over the CSR ------------------------------------------------------
    const int npairs = (R + 1) / 2;
    for (int pr = 0; pr < npairs; ++pr) {
      const int64_t jid = out.job_off[l] + pr;
      const int64_t coff = out.coef_off ? out.coef_off[jid] : noff;
      int node_a, node_b, la, lb;
      pair_rows(pr, R, src, dst, cn, node_a, node_b);
      pair_rows(pr, R, pos_src, pos_dst, cnpos, la, lb);
      for (int w = tid; w < n; w += T) {
        cur[w] = make_float2(w == la ? fabsf(dinv[w]) : 0.f, w == lb ? fabsf(dinv[w]) : 0.f);
      }
      if (tid < 4 * K) zbuf[tid] = 0.f;
      __syncthreads();
      float2* s_in = cur;
      float2* s_out = nxs;
      float2* coef = reinterpret_cast<float2*>(out.c_coef) + coff * K;   // [K][n] float2
      const bool split = split_list(out, n);
      auto cidx = [&](int i, int t) -> int64_t { return coef_index(i, t, n, K, split, out.seg_shift); };
#pragma unroll 1
      for (int i = 0; i < K; ++i) {
        const int g = tid & (G - 1);
        auto commit = [&](int t, float ax, float ay) {
          const float dw = fabsf(dinv[t]);
          const float rx = dw * ax, ry = dw * ay;
          s_out[t] = make_float2(dw * rx, dw * ry);
          coef[cidx(i, t)] = make_float2(rx, ry);
          // label column of operator i+1: r[src] + r[dst]  (tuned_SIGN.py:177-185)
          if (t == pos_src) { zbuf[(0 * K + i) * 2] = rx; zbuf[(0 * K + i) * 2 + 1] = ry; }
          if (t == pos_dst) { zbuf[(1 * K + i) * 2] = rx; zbuf[(1 * K + i) * 2 + 1] = ry; }
        };
        for (int base = 0; base < n; base += T / G) {
          const int t = base + tid / G;
          float ax = 0.f, ay = 0.f;
          const bool mine = t < n && !(dinv[min(t, n - 1)] < 0.f);   // short row of this lane group
          if (mine) {
            const int k1 = off[t + 1];
            for (int k = off[t] + g; k < k1; k += G) {
              const float2 sv = s_in[cols_ld(k)];
              ax += sv.x;
              ay += sv.y;
            }
          }
#pragma unroll
          for (int o = G / 2; o > 0; o >>= 1) {
            ax += __shfl_xor(ax, o);
            ay += __shfl_xor(ay, o);
          }
          if (mine && g == 0) commit(t, ax, ay);
        }
        for (int q = tid >> 6; q < nlong; q += T / 64) {   // one wavefront per long row
          const int t = longrows[q];
          const int k1 = off[t + 1];
          float ax = 0.f, ay = 0.f;
          for (int k = off[t] + (tid & 63); k < k1; k += 64) {
            const float2 sv = s_in[cols_ld(k)];
            ax += sv.x;
            ay += sv.y;
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            ax += __shfl_xor(ax, o);
            ay += __shfl_xor(ay, o);
          }
          if ((tid & 63) == 0) commit(t, ax, ay);
        }
        __syncthreads();
        float2* tmp2 = s_in;
        s_in = s_out;
        s_out = tmp2;
      }
      write_label_column(out, tid, K, jid, zbuf);
      // operator i+1 reaches the list prefix within i+1 hops of the row; with one hop that is the
      // whole list from the first operator on (from the second for nothing: n == support)
      end_pair(out, ls, tid, K, pr, jid, coff, n, node_a, node_b, split, [&](int) { return n; });
      __syncthreads();
    }
    phase_stamp(dbg, 8 + 4, t_prev);
    vol_local = block_sum<T>(vol_local, sh);
    if (tid == 0) commit_link_stats(out, mirror, edges_total, vol_local);
    __syncthreads();   // LDS is reused by the next item of a persistent workgroup
  }
}

// a LinkOut as the __restrict__ output parameters of link_kernel and link_full_kernel (see there), in member order
#define S3GRL_LINK_OUT_ARGS(o)                                                                                 \
  (o).node_off, (o).row_ptr, (o).job_off, (o).coef_off, (o).mirror_of, (o).c_ids, (o).c_coef, (o).jobs, (o).job_z, \
      (o).job_lim, (o).row_nodes, (o).lvl, (o).tot_edges, (o).tot_support, (o).tot_vol, (o).old_of_new, (o).split_t, \
      (o).seg_shift

// One-hop full-reach classes (link_full_kernel).  Small classes run one wavefront per link (no
// cross-wave barriers to pay for 25-node subgraphs), the others four; the class whose bit matrix
// lives in HBM runs a persistent grid, one matrix slice per resident workgroup.
template <int T, int K, bool BMG>
s3grl_status launch_full_class(s3grl_context* ctx, const LinkArgs& a, int64_t L, int cls, int count,
                               hipStream_t stream, uint32_t* bm_scratch, int64_t bm_stride_words, int grid) {
  const ClassBounds fb = class_bounds_full(a.cn_cap, K);
  const size_t lds = (size_t)4 * full_fixed_words(a.cn_cap, K) +
                     (size_t)(cls == kFullBig ? a.big_need : fb.b[cls - kFullBase]);
  auto kern = link_full_kernel<T, K, BMG>;
  S3GRL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(T), lds, stream, a.g->indptr, a.g->indices,
                     a.g->fwd_indptr, a.g->fwd_indices, a.links, a.class_list + (int64_t)cls * L, count,
                     a.plus, a.cn_cap, a.e_cap, S3GRL_LINK_OUT_ARGS(a.out), bm_scratch, bm_stride_words,
                     getenv("S3GRL_BIG_COLS_HBM") ? 0 : (int)lds,   // test hook: big class, columns in HBM
                     (BMG && a.dbg) ? a.dbg : nullptr);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

template <int T, int K, int G, bool GS, bool HS, bool DM = false, bool DIRECTED = false>
s3grl_status launch_link_class_g(s3grl_context* ctx, const LinkArgs& a, int64_t L, int cls, int count,
                                 hipStream_t stream) {
  const int W = words_for(a.g->num_nodes);
  size_t lds;
  if (DM)
    lds = (size_t)4 * link_fixed_words_dm(a.g, a.cn_cap, K) + class_bounds_dm(a.g, a.cn_cap, K).b[cls - kSparseBase];
  else if (HS)
    lds = (size_t)4 * link_fixed_words_sparse(a.g, a.cn_cap, K) +
          class_bounds_sparse(a.g, a.cn_cap, K).b[cls - kSparseBase];
  else if (GS && a.bm_ext_words > 0)
    lds = (size_t)4 * link_fixed_words_sparse(a.g, a.cn_cap, K);
  else
    lds = (size_t)4 * link_fixed_words(a.g, a.cn_cap, K) + (GS ? 0 : (size_t)class_bounds(a.g, a.cn_cap, K).b[cls]);
  // (S3GRL_DEBUG: the LDS of the launch and how many of its workgroups a CU holds)
  if (getenv("S3GRL_DEBUG"))
    fprintf(stderr, "[s3grl] link class %d: %d links, %d threads, %zu B of LDS, %d resident per CU\n", cls, count, T,
            lds, std::min(lds_resident(lds), 32 / (T / 64)));
  auto kern = link_kernel<T, K, G, GS, HS, DM, DIRECTED>;
  S3GRL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)count), dim3(T), lds, stream, a.g->indptr,
                     a.g->indices, W, a.links, a.class_list + (int64_t)cls * L + a.list_offset, a.hops, a.plus,
                     a.cn_cap, a.full_stats, hub_armed(a.g) ? 1 : 0, a.ws,
                     a.p_nodes, S3GRL_LINK_OUT_ARGS(a.out), a.scratch, a.scratch_stride, GS ? a.bm_ext_words : 0, a.dbg, a.smp,
                     a.stash, a.slot, a.new_of_old, a.lo_id, a.dg, a.sop2);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

// lanes per CSR row: 4 for sparse graphs (PubMed/Cora: mean degree ~4), 8 otherwise
template <int T, int K>
s3grl_status launch_link_class(s3grl_context* ctx, const LinkArgs& a, int64_t L, int cls, int count,
                               hipStream_t stream) {
  const double mean_deg = (double)a.g->nnz / (double)std::max<int64_t>(a.g->num_nodes, 1);
  const int gsel = mean_deg <= 6.0 ? 4 : 8;
  if (a.dg.out_indptr) {   // directed plans: bitmap flavour, four lanes per row (two instantiations per sign_k)
    if (cls == kNumClasses) return launch_link_class_g<1024, K, 4, true, false, false, true>(ctx, a, L, cls, count, stream);
    return launch_link_class_g<256, K, 4, false, false, false, true>(ctx, a, L, cls, count, stream);
  }
  if (cls == kNumClasses) {   // HBM-scratch overflow class
    if (gsel <= 4) return launch_link_class_g<1024, K, 4, true, false>(ctx, a, L, cls, count, stream);
    return launch_link_class_g<1024, K, 8, true, false>(ctx, a, L, cls, count, stream);
  }
  if (cls >= kSparseBase && dm_mode_for(a.g)) {   // direct-map flavour
    if (gsel <= 4) return launch_link_class_g<T, K, 4, false, true, true>(ctx, a, L, cls, count, stream);
    return launch_link_class_g<T, K, 8, false, true, true>(ctx, a, L, cls, count, stream);
  }
  if (cls >= kSparseBase) {   // hash flavour
    if (gsel <= 4) return launch_link_class_g<256, K, 4, false, true>(ctx, a, L, cls, count, stream);
    return launch_link_class_g<256, K, 8, false, true>(ctx, a, L, cls, count, stream);
  }
  if (gsel <= 4) return launch_link_class_g<T, K, 4, false, false>(ctx, a, L, cls, count, stream);
  return launch_link_class_g<T, K, 8, false, false>(ctx, a, L, cls, count, stream);
}

}  // namespace

// The launches of the LDS classes do not depend on each other: they go round-robin onto the
// context's stream and its side streams (forked and joined with events), so that the tail of one
// class overlaps the start of the next instead of draining the chip five times per plan.
template <int K>
s3grl_status launch_links_k(s3grl_context* ctx, const LinkArgs& a, int64_t L,
                            const int32_t* class_count_in) {
  static const bool serial = getenv("S3GRL_SERIAL_CLASSES") != nullptr;
  const int32_t* class_count_host = class_count_in;
  int launches = 0;
  for (int c = 0; c <= kTinyList + 1; ++c) launches += class_count_host[c] > 0 && c != kNumClasses + 1;
  for (int c = kCsrBase; c < kNumListsAll; ++c) launches += class_count_host[c] > 0;
  const bool fork = !serial && launches > 1;
  // the side streams rejoin the context's stream on EVERY way out: a launch that fails half-way must not leave
  // kernels of this plan running beside whatever the caller queues next (its buffers go back to the arena)
  struct SideJoin {
    s3grl_context* ctx;
    bool armed = false;
    hipError_t join() {
      hipError_t first = hipSuccess;
      if (armed)
        for (int i = 0; i < s3grl_context::kSide; ++i) {
          hipError_t e = hipEventRecord(ctx->side_ev[i], ctx->side[i]);
          if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->side_ev[i], 0);
          if (e != hipSuccess && first == hipSuccess) first = e;
        }
      armed = false;
      return first;
    }
    ~SideJoin() { (void)join(); }
  } side_join{ctx};
  if (fork) {
    S3GRL_TRY(ensure_side_streams(ctx));
    S3GRL_HIP_TRY(hipEventRecord(ctx->side_ev[s3grl_context::kSide], ctx->stream));
    side_join.armed = true;
    for (int i = 0; i < s3grl_context::kSide; ++i)
      S3GRL_HIP_TRY(hipStreamWaitEvent(ctx->side[i], ctx->side_ev[s3grl_context::kSide], 0));
  }
  int turn = 0;
  auto next_stream = [&]() -> hipStream_t {
    if (!fork) return ctx->stream;
    const int k = turn++ % (s3grl_context::kSide + 1);
    return k == 0 ? ctx->stream : ctx->side[k - 1];
  };
  // largest subgraphs first: they are the long poles of the tail
  if (class_count_host[kNumClasses] > 0) {
    if (a.bm_ext_words > 0) {   // bounded number of slices: the class runs in chunks, one after the other
      hipStream_t st = next_stream();
      for (int off = 0; off < class_count_host[kNumClasses]; off += a.gs_chunk) {
        LinkArgs b = a;
        b.list_offset = off;
        S3GRL_TRY((launch_link_class<1024, K>(ctx, b, L, kNumClasses,
                                               std::min(a.gs_chunk, class_count_host[kNumClasses] - off), st)));
      }
    } else {
      S3GRL_TRY((launch_link_class<1024, K>(ctx, a, L, kNumClasses, class_count_host[kNumClasses], next_stream())));
    }
  }
  for (int c = kNumListsAll - 1; c >= kCsrBase; --c) {   // full-reach links on their induced LDS CSR (s3grl_csr.hip)
    if (class_count_host[c] == 0) continue;
    CsrLinkArgs h{a.g->indptr, a.g->indices, words_for(a.g->num_nodes), a.hops,
                  a.g->balls.bits + (int64_t)(a.hops - 1) * a.g->balls.level_stride, a.links, a.plus, a.cn_cap,
                  a.csr_cnt, a.csr_e, a.out, a.stash, a.slot, a.dbg};
    S3GRL_TRY(launch_csr_class(ctx, h, K, c - kCsrBase, a.class_list + (int64_t)c * L, class_count_host[c],
                               next_stream()));
  }
  if (class_count_host[kFullBig] > 0)
    S3GRL_TRY((launch_full_class<1024, K, true>(ctx, a, L, kFullBig, class_count_host[kFullBig], next_stream(),
                                                  a.bm_scratch, a.bm_stride_words, a.bm_grid)));
  unsigned long long* hub_rows = a.out.tot_vol + 2 * (size_t)kStatShards * kStatStride;   // rows 4..8 of d_stats
  for (int c = kHubBase + kHubClasses; c >= kHubBase; --c) {   // cached hub neighbourhoods (s3grl_hub.hip)
    if (class_count_host[c] == 0) continue;
    HubLinkArgs h{a.g->indptr, a.g->indices, a.g->hub, a.links, a.plus, a.cn_cap, a.x_cap, a.out,
                  hub_rows, hub_rows + kStatShards * kStatStride, hub_rows + 2 * kStatShards * kStatStride,
                  hub_rows + 3 * kStatShards * kStatStride, hub_rows + 4 * kStatShards * kStatStride,
                  a.e_cap, a.dbg, a.hub_slices, a.hub_slice_words, a.hub_slice_grid};
    S3GRL_TRY(launch_hub_class(ctx, h, K, c - kHubBase, a.class_list + (int64_t)c * L, class_count_host[c],
                               next_stream()));
  }
  for (int w = 0; w < 2; ++w) {   // the smallest one-hop links, half a wavefront / a wavefront each (s3grl_hub.hip)
    if (class_count_host[kTinyList + w] == 0) continue;
    TinyLinkArgs t{a.g->indptr, a.g->indices, a.g->fwd_indptr, a.g->fwd_indices, a.links, a.out};
    S3GRL_TRY(launch_tiny_class(ctx, t, K, w == 0 ? 32 : 64, a.class_list + (int64_t)(kTinyList + w) * L,
                                class_count_host[kTinyList + w], next_stream()));
  }
  for (int c = kFullBig - 1; c >= kFullBase; --c) {
    const int count = class_count_host[c];
    if (count == 0) continue;
    // threads per link by class: a wavefront for the smallest subgraphs; the classes whose LDS
    // leaves one or two workgroups per CU get 1024 / 512 threads (their probing trips are chains
    // of dependent loads: more rows per trip, more loads in flight)
    const int fc = c - kFullBase;
    // (class 2 at 128 threads since the links of at most 64 nodes left for link_tiny_kernel: 16.55 -> 16.3 ms on
    // config 5; 64: 16.75, 256: 16.55, 512: 18.2)
    const int t = fc <= 1 ? 64 : (fc == 2 ? 128 : (fc == 3 ? 256 : (fc == 4 ? 512 : 1024)));
    if (t <= 64)
      S3GRL_TRY((launch_full_class<64, K, false>(ctx, a, L, c, count, next_stream(), nullptr, 0, count)));
    else if (t <= 128)
      S3GRL_TRY((launch_full_class<128, K, false>(ctx, a, L, c, count, next_stream(), nullptr, 0, count)));
    else if (t <= 256)
      S3GRL_TRY((launch_full_class<256, K, false>(ctx, a, L, c, count, next_stream(), nullptr, 0, count)));
    else if (t <= 512)
      S3GRL_TRY((launch_full_class<512, K, false>(ctx, a, L, c, count, next_stream(), nullptr, 0, count)));
    else
      S3GRL_TRY((launch_full_class<1024, K, false>(ctx, a, L, c, count, next_stream(), nullptr, 0, count)));
  }
  for (int c = kFullBase - 1; c >= kSparseBase; --c) {
    if (class_count_host[c] == 0) continue;
    if (dm_mode_for(a.g)) {
      const size_t lds = (size_t)4 * link_fixed_words_dm(a.g, a.cn_cap, K) +
                         class_bounds_dm(a.g, a.cn_cap, K).b[c - kSparseBase];
      const int t = threads_for_class(lds, c - kSparseBase);
      if (t <= 128) S3GRL_TRY((launch_link_class<128, K>(ctx, a, L, c, class_count_host[c], next_stream())));
      else if (t <= 256) S3GRL_TRY((launch_link_class<256, K>(ctx, a, L, c, class_count_host[c], next_stream())));
      else if (t <= 512) S3GRL_TRY((launch_link_class<512, K>(ctx, a, L, c, class_count_host[c], next_stream())));
      else S3GRL_TRY((launch_link_class<1024, K>(ctx, a, L, c, class_count_host[c], next_stream())));
    } else {
      S3GRL_TRY((launch_link_class<256, K>(ctx, a, L, c, class_count_host[c], next_stream())));
    }
  }
  for (int c = kNumClasses - 1; c >= 0; --c) {
    const int count = class_count_host[c];
    if (count == 0) continue;
    // Fewer workgroups fit a CU as the LDS per workgroup grows (bigger subgraph class, or a big
    // graph whose three N-bit bitmaps alone take tens of KB): give each more waves then.
    const size_t lds = (size_t)4 * link_fixed_words(a.g, a.cn_cap, K) + class_bounds(a.g, a.cn_cap, K).b[c];
    const int t = threads_for_class(lds, c);
    if (t <= 128) S3GRL_TRY((launch_link_class<128, K>(ctx, a, L, c, count, next_stream())));
    else if (t <= 256) S3GRL_TRY((launch_link_class<256, K>(ctx, a, L, c, count, next_stream())));
    else if (t <= 512) S3GRL_TRY((launch_link_class<512, K>(ctx, a, L, c, count, next_stream())));
    else S3GRL_TRY((launch_link_class<1024, K>(ctx, a, L, c, count, next_stream())));
  }
  S3GRL_HIP_TRY(side_join.join());
  return S3GRL_OK;
}

}  // namespace s3grl
