// Labelled enclosing subgraphs for the SEAL baselines (reference utils.py:47-85 k_hop_subgraph, followed by
// construct_pyg_graph with a node-labelling trick, utils.py:211-316): per link the node list of the k-hop
// extraction, the edges of the induced matrix without the target link in local ids, and z.
//
// The node lists come from a plan (the same BFS, sampling and directed handling as PoS): hop-major, ascending
// id inside a hop.  A list is therefore a sequence of sorted segments — {src}, {dst}, hop 1, hop 2, ... — and
// the position of a global id is a binary search in each segment; ascending position inside a segment is
// ascending id.  Three passes:
//   seal_count_kernel   one workgroup per link, one wavefront per row: induced entries per list position
//   (scan)              row offsets of the whole output, edge_ptr[l] = row_off[node_ptr[l]]
//   seal_link_kernel    one workgroup per link: the edges (rows in list order, inside a row the segments in
//                       order, ascending id inside a segment = ascending position), then the label passes
// seal_link_kernel has two flavours chosen by the link's OWN size: the list, both distance arrays and the
// packed edges on-chip (LDS) when they fit the budget, else the distance arrays in an HBM slice of the link's
// own and the edges read back from the output.  Both run the same code on different pointers.
// Everything is integer: results are bit-exact and independent of the launch order.
#include "s3grl_internal.hpp"

#include <algorithm>

namespace s3grl {
namespace {

constexpr int kSealBlock = 256;
constexpr int kSealWaves = kSealBlock / 64;
constexpr int kSegMax = kMaxLevels + 2;            // {src}, {dst}, hops 1 .. kMaxLevels
constexpr int32_t kInf = 0x3fffffff;               // not reached
constexpr int32_t kBlocked = -1;                   // the masked endpoint (never expands, never reached)
constexpr int64_t kDefaultLdsBudget = 64 << 10;
constexpr int64_t kMaxLdsBudget = 159 << 10;   // 160 KiB per CU, less the static part

// segment k of a link's list is positions [lo[k], lo[k+1]); lo[0] = 0, lo[1] = 1, lo[2] = 2, ..., lo[nseg] = n
struct Segs {
  int32_t nseg;
  int32_t lo[kSegMax + 1];
};

// hop distances are non-decreasing along a list: hop h starts at the first position whose distance is >= h
__device__ void seal_segments(const int8_t* dists, int32_t n, Segs& sg) {
  const int hmax = n > 2 ? dists[n - 1] : 0;
  sg.lo[0] = 0;
  sg.lo[1] = 1;
  sg.lo[2] = 2;
  for (int h = 2; h <= hmax; ++h) {
    int a = sg.lo[h], b = n;
    while (a < b) {
      const int m = (a + b) >> 1;
      if (dists[m] < h) a = m + 1; else b = m;
    }
    sg.lo[h + 1] = a;
  }
  sg.nseg = hmax + 2;
  sg.lo[sg.nseg] = n;
}

// position of v in segment k of `ids` (the link's list), or -1
__device__ __forceinline__ int32_t seg_find(const int32_t* ids, const Segs& sg, int k, int32_t v) {
  int32_t a = sg.lo[k], b = sg.lo[k + 1];
  while (a < b) {
    const int32_t m = (a + b) >> 1;
    if (ids[m] < v) a = m + 1; else b = m;
  }
  return (a < sg.lo[k + 1] && ids[a] == v) ? a : -1;
}

// the target link's two entries are not edges (subgraph[0, 1] = subgraph[1, 0] = 0, dropped by ssp.find)
__device__ __forceinline__ bool is_target(int32_t row, int32_t col) {
  return (row == 0 && col == 1) || (row == 1 && col == 0);
}

__global__ void __launch_bounds__(kSealBlock)
seal_count_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                  const int64_t* __restrict__ node_ptr, const int32_t* __restrict__ nodes,
                  const int8_t* __restrict__ dists, int32_t* __restrict__ row_cnt) {
  __shared__ Segs sg;
  const int64_t l = blockIdx.x;
  const int64_t base = node_ptr[l];
  const int32_t n = (int32_t)(node_ptr[l + 1] - base);
  const int32_t* ids = nodes + base;
  if (threadIdx.x == 0) seal_segments(dists + base, n, sg);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int32_t i = threadIdx.x >> 6; i < n; i += kSealWaves) {
    const int32_t u = ids[i];
    const int32_t r0 = indptr[u], r1 = indptr[u + 1];
    int32_t cnt = 0;
    for (int32_t k = r0 + lane; k < r1; k += 64) {
      const int32_t v = indices[k];
      int32_t p = -1;
      for (int s = 0; s < sg.nseg && p < 0; ++s) p = seg_find(ids, sg, s, v);
      cnt += (p >= 0 && !is_target(i, p)) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) row_cnt[base + i] = cnt;
  }
}

// the export orders hop 0 like any other hop (ascending id): put src, dst back in front
__global__ void seal_endpoints_kernel(const int64_t* __restrict__ links, const int64_t* __restrict__ node_ptr,
                                      int64_t L, int32_t* __restrict__ nodes) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  nodes[node_ptr[l]] = (int32_t)links[2 * l];
  nodes[node_ptr[l] + 1] = (int32_t)links[2 * l + 1];
}

__host__ __device__ inline int64_t seal_lds_need(int64_t n, int64_t e) {
  return 12 * n + 4 * e;   // ids, two distance arrays, packed (row << 16 | col) edges
}

// per link: its edge offset, and the HBM slice its distance arrays need (0 for the on-chip flavour)
__global__ void seal_classify_kernel(const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ row_off,
                                     int64_t L, int64_t budget, int64_t* __restrict__ edge_ptr,
                                     int32_t* __restrict__ hbm_n, unsigned long long* __restrict__ max_lds) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l > L) return;
  edge_ptr[l] = row_off[node_ptr[l]];
  if (l == L) return;
  const int64_t n = node_ptr[l + 1] - node_ptr[l];
  const int64_t need = seal_lds_need(n, row_off[node_ptr[l + 1]] - row_off[node_ptr[l]]);
  const bool lds = need <= budget && n <= 65535;
  hbm_n[l] = lds ? 0 : (int32_t)n;
  if (lds) atomicMax(max_lds, (unsigned long long)need);
}

struct LinkArgs {
  const int32_t* indptr;
  const int32_t* indices;
  const float* values;        // [nnz] aligned with indices, or null (ones)
  const int64_t* node_ptr;
  const int32_t* nodes;
  const int8_t* dists;
  const int64_t* row_off;     // [Σn + 1] first output edge of every list position
  const int64_t* ws_off;      // [L] first HBM workspace node of a link of the HBM flavour
  int32_t* ws;                // [2 Σ n over those links]
  int64_t budget;
  int32_t label;
  int32_t zw;                 // z columns
  int32_t* src;
  int32_t* dst;
  float* weight;
  int32_t* z;                 // [Σn, zw], zeroed
};

// one level-synchronous BFS step from both endpoints at once over the (symmetrised) edge list: a node at
// level `lev` reaches its unreached neighbours.  Races only ever write the same value.
template <bool kLds>
__device__ __forceinline__ bool bfs_level(const uint32_t* ledges, const int32_t* gsrc, const int32_t* gdst, int32_t e,
                                          int32_t* da, int32_t* db, int32_t lev) {
  bool any = false;
  for (int32_t k = threadIdx.x; k < e; k += kSealBlock) {
    int32_t u, v;
    if (kLds) {
      const uint32_t w = ledges[k];
      u = (int32_t)(w >> 16);
      v = (int32_t)(w & 0xffff);
    } else {
      u = gsrc[k];
      v = gdst[k];
    }
    const int32_t au = da[u], av = da[v], bu = db[u], bv = db[v];
    if (au == lev && av == kInf) { da[v] = lev + 1; any = true; }
    if (av == lev && au == kInf) { da[u] = lev + 1; any = true; }
    if (bu == lev && bv == kInf) { db[v] = lev + 1; any = true; }
    if (bv == lev && bu == kInf) { db[u] = lev + 1; any = true; }
  }
  return any;
}

template <bool kLds>
__global__ void __launch_bounds__(kSealBlock) seal_link_kernel(LinkArgs a) {
  extern __shared__ int32_t lds[];
  __shared__ Segs sg;
  __shared__ int32_t chg[3];
  const int64_t l = blockIdx.x;
  const int64_t base = a.node_ptr[l];
  const int32_t n = (int32_t)(a.node_ptr[l + 1] - base);
  const int64_t e0 = a.row_off[base];
  const int32_t e = (int32_t)(a.row_off[base + n] - e0);
  const bool fits = seal_lds_need(n, e) <= a.budget && n <= 65535;
  if (fits != kLds) return;   // the other flavour's link (uniform over the workgroup)

  const int32_t* ids = a.nodes + base;
  int32_t *da, *db;
  uint32_t* ledges = nullptr;
  if (kLds) {
    int32_t* lids = lds;
    for (int32_t i = threadIdx.x; i < n; i += kSealBlock) lids[i] = ids[i];
    ids = lids;
    da = lds + n;
    db = lds + 2 * n;
    ledges = reinterpret_cast<uint32_t*>(lds + 3 * n);
  } else {
    da = a.ws + 2 * a.ws_off[l];
    db = da + n;
  }
  if (threadIdx.x == 0) {
    seal_segments(a.dists + base, n, sg);
    chg[0] = chg[1] = chg[2] = 0;
  }
  __syncthreads();

  // ---- edges: row i by one wavefront; per segment a stable compaction of the row's hits --------------
  const int lane = threadIdx.x & 63;
  const bool degree = a.label == S3GRL_LABEL_DEGREE;
  for (int32_t i = threadIdx.x >> 6; i < n; i += kSealWaves) {
    const int32_t u = ids[i];
    const int32_t r0 = a.indptr[u], r1 = a.indptr[u + 1];
    int64_t out = a.row_off[base + i];
    const int64_t row_end = a.row_off[base + i + 1];   // what the count pass found: never written beyond
    for (int s = 0; s < sg.nseg; ++s) {
      for (int32_t k0 = r0; k0 < r1; k0 += 64) {
        const int32_t k = k0 + lane;
        int32_t p = -1;
        if (k < r1) p = seg_find(ids, sg, s, a.indices[k]);
        const bool hit = p >= 0 && !is_target(i, p);
        const unsigned long long bal = __ballot(hit);
        const int64_t o = out + __popcll(bal & ((1ull << lane) - 1));
        if (hit && o < row_end) {
          const float w = a.values ? a.values[k] : 1.0f;
          a.src[o] = i;
          a.dst[o] = p;
          a.weight[o] = w;
          if (kLds) ledges[o - e0] = ((uint32_t)i << 16) | (uint32_t)p;
          if (degree) atomicAdd(&a.z[base + p], (int32_t)w);   // column sums: in-weights
        }
        out += __popcll(bal);
      }
    }
  }

  // ---- labels -----------------------------------------------------------------------------------------
  const int label = a.label;
  int32_t* z = a.z + base * a.zw;
  if (label == S3GRL_LABEL_HOP || label == S3GRL_LABEL_ZO) {
    for (int32_t i = threadIdx.x; i < n; i += kSealBlock) {
      const int32_t d = a.dists[base + i];
      z[i] = label == S3GRL_LABEL_HOP ? d : (d == 0 ? 1 : 0);
    }
    return;
  }
  if (degree) {
    __syncthreads();
    for (int32_t i = threadIdx.x; i < n; i += kSealBlock) z[i] = min(z[i], 100);
    return;
  }
  if (label != S3GRL_LABEL_DRNL && label != S3GRL_LABEL_DE && label != S3GRL_LABEL_DE_PLUS) return;   // zeros

  // distances on the UNDIRECTED subgraph (shortest_path(directed=False)): da from src, db from dst.
  // drnl / de+: the other endpoint removed; de: nothing removed and the target link counted as an edge
  // (scipy keeps the explicit zeros of subgraph[0, 1] = 0 and csgraph follows them)
  const bool masked = label != S3GRL_LABEL_DE;
  for (int32_t i = threadIdx.x; i < n; i += kSealBlock) {
    da[i] = i == 0 ? 0 : (i == 1 ? (masked ? kBlocked : 1) : kInf);
    db[i] = i == 1 ? 0 : (i == 0 ? (masked ? kBlocked : 1) : kInf);
  }
  __syncthreads();
  const int32_t* gsrc = a.src + e0;
  const int32_t* gdst = a.dst + e0;
  for (int32_t lev = 0;; ++lev) {
    if (threadIdx.x == 0) chg[(lev + 1) % 3] = 0;   // every thread read that flag before the last barrier
    if (bfs_level<kLds>(ledges, gsrc, gdst, e, da, db, lev)) chg[lev % 3] = 1;
    __syncthreads();
    if (!chg[lev % 3]) break;
  }
  for (int32_t i = threadIdx.x; i < n; i += kSealBlock) {
    int32_t ds = da[i], dd = db[i];
    if (label == S3GRL_LABEL_DRNL) {
      int32_t v;
      if (i < 2) {
        v = 1;
      } else if (ds >= kInf || dd >= kInf) {
        v = 0;   // inf -> NaN -> 0
      } else {
        const int32_t D = ds + dd, h = D / 2;
        v = 1 + min(ds, dd) + h * (h + D % 2 - 1);
      }
      z[i] = v;
    } else if (label == S3GRL_LABEL_DE) {
      z[2 * i] = min(ds, 3);        // inf is clamped too: 4 never occurs
      z[2 * i + 1] = min(dd, 3);
    } else {                          // de+: the removed endpoint's own entry is 0
      if (ds == kBlocked) ds = 0;
      if (dd == kBlocked) dd = 0;
      z[2 * i] = min(ds, 100);
      z[2 * i + 1] = min(dd, 100);
    }
  }
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

struct s3grl_subgraphs {
  s3grl_context* ctx = nullptr;
  int64_t L = 0, total_nodes = 0, total_edges = 0;
  int32_t label = 0, zw = 1;
  int64_t* node_ptr = nullptr;   // [L+1]
  int32_t* nodes = nullptr;      // [Σn]
  int8_t* dists = nullptr;       // [Σn]
  int64_t* edge_ptr = nullptr;   // [L+1]
  int32_t* src = nullptr;        // [Σe] local row
  int32_t* dst = nullptr;        // [Σe] local column
  float* weight = nullptr;       // [Σe]
  int32_t* z = nullptr;          // [Σn, zw]
  std::vector<void*> owned;
};

namespace {

template <typename T>
s3grl_status seal_alloc(s3grl_context* ctx, int64_t count, T** out, std::vector<void*>& keep) {
  void* p = nullptr;
  S3GRL_TRY(ctx->arena.alloc((size_t)std::max<int64_t>(count, 1) * sizeof(T), &p));
  keep.push_back(p);
  *out = static_cast<T*>(p);
  return S3GRL_OK;
}

int32_t label_width(int32_t label) {
  return (label == S3GRL_LABEL_DE || label == S3GRL_LABEL_DE_PLUS) ? 2 : 1;
}

s3grl_status build(s3grl_context* ctx, const s3grl_graph* g, const float* values, const int64_t* links,
                   int64_t L, const s3grl_subgraph_cfg* cfg, s3grl_subgraphs* sub) {
  hipStream_t st = ctx->stream;
  std::vector<void*>& own = sub->owned;
  Transient tmp{ctx, {}};
  S3GRL_TRY(seal_alloc(ctx, L + 1, &sub->node_ptr, own));
  S3GRL_TRY(seal_alloc(ctx, L + 1, &sub->edge_ptr, own));
  if (L == 0) {
    S3GRL_HIP_TRY(hipMemsetAsync(sub->node_ptr, 0, 8, st));
    S3GRL_HIP_TRY(hipMemsetAsync(sub->edge_ptr, 0, 8, st));
    return S3GRL_OK;
  }
  // the node lists: a PoS plan's extraction (same BFS, sampling and directed rules), every link in full
  s3grl_cfg pc{};
  pc.mode = S3GRL_MODE_POS;
  pc.num_hops = cfg->num_hops;
  pc.sign_k = 1;
  pc.strategy = S3GRL_STRATEGY_INTERSECTION;
  pc.directed = g->directed ? 1 : 0;
  pc.flags = S3GRL_FLAG_FULL_STATS | S3GRL_FLAG_NO_FOLD;
  pc.seed = cfg->seed;
  pc.max_nodes_per_hop = cfg->max_nodes_per_hop;
  pc.ratio_per_hop = cfg->ratio_per_hop;
  s3grl_plan* plan = nullptr;
  s3grl_status s = s3grl_plan_create(ctx, g, links, L, &pc, &plan);
  if (s == S3GRL_ERR_SELF_LINK) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_TRY(s);
  s3grl_plan_stats ps{};
  s = s3grl_plan_get_stats(plan, &ps);
  const int64_t tn = ps.extracted_nodes;
  if (s == S3GRL_OK) s = seal_alloc(ctx, tn, &sub->nodes, own);
  if (s == S3GRL_OK) s = seal_alloc(ctx, tn, &sub->dists, own);
  if (s == S3GRL_OK) s = s3grl_plan_export_subgraphs(plan, sub->node_ptr, sub->nodes, sub->dists);
  s3grl_plan_destroy(plan);   // stream-ordered: the export copies are queued before its blocks are reused
  S3GRL_TRY(s);
  sub->total_nodes = tn;
  hipLaunchKernelGGL(seal_endpoints_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, st, links,
                     sub->node_ptr, L, sub->nodes);
  S3GRL_HIP_TRY(hipGetLastError());

  const int32_t* indptr = g->directed ? g->out_indptr : g->indptr;
  const int32_t* indices = g->directed ? g->out_indices : g->indices;
  int32_t* row_cnt;
  int64_t *row_off, *scan_ws;
  S3GRL_TRY(seal_alloc(ctx, tn, &row_cnt, tmp.ptrs));
  S3GRL_TRY(seal_alloc(ctx, tn + 1, &row_off, tmp.ptrs));
  S3GRL_TRY(seal_alloc(ctx, scan_workspace_elems(tn), &scan_ws, tmp.ptrs));
  hipLaunchKernelGGL(seal_count_kernel, dim3((unsigned)L), dim3(kSealBlock), 0, st, indptr, indices, sub->node_ptr,
                     sub->nodes, sub->dists, row_cnt);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(launch_scan_i32_to_i64(ctx, row_cnt, tn, row_off, scan_ws));

  int64_t budget = cfg->lds_budget > 0 ? std::min<int64_t>(cfg->lds_budget, kMaxLdsBudget) : kDefaultLdsBudget;
  int32_t* hbm_n;
  int64_t* ws_off;
  S3GRL_TRY(seal_alloc(ctx, L, &hbm_n, tmp.ptrs));
  S3GRL_TRY(seal_alloc(ctx, L + 1, &ws_off, tmp.ptrs));
  int64_t* ds = ctx->d_scalars;
  S3GRL_HIP_TRY(hipMemsetAsync(ds, 0, 8, st));
  hipLaunchKernelGGL(seal_classify_kernel, dim3((unsigned)((L + 256) / 256)), dim3(256), 0, st, sub->node_ptr, row_off,
                     L, budget, sub->edge_ptr, hbm_n, reinterpret_cast<unsigned long long*>(ds));
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(launch_scan_i32_to_i64(ctx, hbm_n, L, ws_off, scan_ws));   // (L <= Σn: the workspace is big enough)
  S3GRL_HIP_TRY(hipMemcpyAsync(ctx->h_scalars, ds, 8, hipMemcpyDeviceToHost, st));
  S3GRL_HIP_TRY(hipMemcpyAsync(ctx->h_scalars + 1, row_off + tn, 8, hipMemcpyDeviceToHost, st));
  S3GRL_HIP_TRY(hipMemcpyAsync(ctx->h_scalars + 2, ws_off + L, 8, hipMemcpyDeviceToHost, st));
  S3GRL_HIP_TRY(hipStreamSynchronize(st));
  const int64_t max_lds = ctx->h_scalars[0], te = ctx->h_scalars[1], hbm_nodes = ctx->h_scalars[2];
  sub->total_edges = te;

  S3GRL_TRY(seal_alloc(ctx, te, &sub->src, own));
  S3GRL_TRY(seal_alloc(ctx, te, &sub->dst, own));
  S3GRL_TRY(seal_alloc(ctx, te, &sub->weight, own));
  S3GRL_TRY(seal_alloc(ctx, tn * sub->zw, &sub->z, own));
  S3GRL_HIP_TRY(hipMemsetAsync(sub->z, 0, (size_t)std::max<int64_t>(tn * sub->zw, 1) * 4, st));
  int32_t* ws = nullptr;
  if (hbm_nodes > 0) S3GRL_TRY(seal_alloc(ctx, 2 * hbm_nodes, &ws, tmp.ptrs));

  LinkArgs a{indptr, indices, values, sub->node_ptr, sub->nodes, sub->dists, row_off, ws_off, ws, budget,
             sub->label, sub->zw, sub->src, sub->dst, sub->weight, sub->z};
  const bool any_lds = hbm_nodes < tn;   // some link of the on-chip flavour (max_lds may be 0 for none at all)
  if (any_lds) {
    const unsigned dyn = (unsigned)((std::max<int64_t>(max_lds, 4) + 15) & ~(int64_t)15);
    if (dyn > (48u << 10))
      S3GRL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(seal_link_kernel<true>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    hipLaunchKernelGGL(seal_link_kernel<true>, dim3((unsigned)L), dim3(kSealBlock), dyn, st, a);
    S3GRL_HIP_TRY(hipGetLastError());
  }
  if (hbm_nodes > 0) {
    hipLaunchKernelGGL(seal_link_kernel<false>, dim3((unsigned)L), dim3(kSealBlock), 0, st, a);
    S3GRL_HIP_TRY(hipGetLastError());
  }
  S3GRL_HIP_TRY(hipStreamSynchronize(st));   // the transient workspace is released on return
  return S3GRL_OK;
}

}  // namespace

extern "C" {

s3grl_status s3grl_subgraphs_create(s3grl_context* ctx, const s3grl_graph* g, const float* values,
                                    const int64_t* links, int64_t num_links, const s3grl_subgraph_cfg* cfg,
                                    int32_t label, s3grl_subgraphs** out) {
  if (!ctx || !g || !cfg || !out || num_links < 0 || (num_links > 0 && !links)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (cfg->num_hops < 0 || cfg->num_hops > kMaxLevels - 2 || cfg->lds_budget < 0 || cfg->max_nodes_per_hop < 0) {
    set_last_error("num_hops outside [0, 30], or a negative lds_budget / max_nodes_per_hop");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  for (int r : cfg->reserved)
    if (r != 0) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_links > 0x7fffffff) {
    set_last_error("more than 2^31 - 1 links in one call");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  auto* sub = new (std::nothrow) s3grl_subgraphs();
  if (!sub) return S3GRL_ERR_OUT_OF_MEMORY;
  sub->ctx = ctx;
  sub->L = num_links;
  sub->label = label;
  sub->zw = label_width(label);
  const s3grl_status s = build(ctx, g, values, links, num_links, cfg, sub);
  if (s != S3GRL_OK) {
    s3grl_subgraphs_destroy(sub);
    return s;
  }
  *out = sub;
  return S3GRL_OK;
}

s3grl_status s3grl_subgraphs_counts(const s3grl_subgraphs* s, int64_t* what) {
  if (!s || !what) return S3GRL_ERR_INVALID_ARGUMENT;
  what[0] = s->L;
  what[1] = s->total_nodes;
  what[2] = s->total_edges;
  what[3] = s->zw;
  return S3GRL_OK;
}

s3grl_status s3grl_subgraphs_export(const s3grl_subgraphs* s, int64_t* node_ptr, int32_t* nodes, int8_t* dists,
                                    int64_t* edge_ptr, int32_t* src, int32_t* dst, float* weight, int32_t* z) {
  if (!s) return S3GRL_ERR_INVALID_ARGUMENT;
  hipStream_t st = s->ctx->stream;
  const size_t L1 = (size_t)s->L + 1, n = (size_t)s->total_nodes, e = (size_t)s->total_edges;
  auto copy = [&](void* to, const void* from, size_t bytes) -> s3grl_status {
    if (to && bytes) S3GRL_HIP_TRY(hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, st));
    return S3GRL_OK;
  };
  S3GRL_TRY(copy(node_ptr, s->node_ptr, L1 * 8));
  S3GRL_TRY(copy(nodes, s->nodes, n * 4));
  S3GRL_TRY(copy(dists, s->dists, n));
  S3GRL_TRY(copy(edge_ptr, s->edge_ptr, L1 * 8));
  S3GRL_TRY(copy(src, s->src, e * 4));
  S3GRL_TRY(copy(dst, s->dst, e * 4));
  S3GRL_TRY(copy(weight, s->weight, e * 4));
  S3GRL_TRY(copy(z, s->z, n * s->zw * 4));
  return S3GRL_OK;
}

s3grl_status s3grl_subgraphs_destroy(s3grl_subgraphs* s) {
  if (!s) return S3GRL_ERR_INVALID_ARGUMENT;
  for (void* p : s->owned) s->ctx->arena.release(p);
  delete s;
  return S3GRL_OK;
}

}  // extern "C"
