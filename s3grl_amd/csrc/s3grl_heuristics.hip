// Classic link heuristics of the reference's `--use_heuristic` branch (utils.py CN / AA / PPR) on gfx950.
//
//   prepare_kernel    once per graph, one thread per node: fp64 row sums r, column sums c (over the CSR of Aᵀ, so
//                     in ascending row order, as scipy's A.sum(axis=0) adds them) and the Adamic-Adar weights
//                     w = 1 / ln(c), ±inf -> 0
//   nan_rows_kernel   once per graph, one thread per node: whether the row holds a key of NaN weight (a negative
//                     column sum).  The reference's sparse A[s].multiply(A_[d]) keeps 0·NaN for the entries of
//                     row d that row s lacks, so its AA(s, d) is NaN for every s; pairs_kernel does the same
//   pairs_kernel<KIND> one wavefront per link, one instantiation per local index.  The lanes walk the shorter of the
//                     two sorted rows and binary-search the longer one (s3grl_rows.hpp); a_s·a_d (CN),
//                     a_s·(a_d·w_k) (AA) or a_s·(a_d·v_k) (RA) summed in fp64, lane-sequential, then a fixed xor
//                     butterfly; an integer count of the common keys for Jaccard, divided once by
//                     deg(s) + deg(d) − count; PA is r_s·r_d without a walk; written as fp32
//   ppr_coef_kernel   per call (p is an argument): W's entries (p·a_ji)·(1/r_j) laid out as the CSR of Aᵀ, and z
//   ppr_spmm_kernel   one iteration x_new = W·x_old + s·t for a block of B distinct sources.  X is node-major
//                     [N, B] fp64, so a neighbour is one contiguous row load per 64 columns.  A workgroup owns a
//                     tile of kTile nodes and 64 columns; wave w takes the tile's nodes w, w + 4, ... in order and
//                     the four waves' partials are added ((0 + 1) + (2 + 3)).  Per tile and column it writes the
//                     partials of Σ(x_new − x_old)², Σ z·x_new and Σ x_new to a slab, [3][B][tiles]
//   ppr_reduce_kernel one wavefront per column: the slab's tiles in a fixed order and butterfly; sets t for the next
//                     iteration, counts the iteration, and freezes the column once ‖x_new − x_old‖ <= tol or
//                     max_iter iterations have run (fast_pagerank's pagerank_power loop)
//   ppr_finish_kernel x[d] / Σx for every link whose source is in the block, and the block's iteration counts
//
// Four indices the reference does not have (DESIGN.md §23 is their specification): RA, Jaccard and PA are
// instantiations of pairs_kernel, and
//
//   ra_weights_kernel   once per graph, one thread per node: the resource-allocation weights v = 1 / c, 0 where c = 0
//   katz_spmm_kernel    one level x_new = β·Aᵀ·(x_old + e_s) of Horner's rule for Σ_{l=1..max_len} β^l·A^l, for a
//                       block of B distinct sources: ppr_spmm_kernel's tiles, wave split and entry order, with the
//                       source's 1 added to the operand.  No norm, no slab: the level count is fixed
//   katz_finish_kernel  x[d] for every link whose source is in the block, from the buffer the last level wrote
//
// Determinism: no float atomics.  A column's arithmetic depends on its own source only: the node tiles, the wave
// split inside a tile and the reduction over tiles are fixed, whatever B is and whichever sources share the
// block.  A frozen column is no longer written; its result lives in the buffer its last iteration wrote
// (iteration k writes buffer k & 1).
#include "s3grl_internal.hpp"
#include "s3grl_rows.hpp"
#include "s3grl_train.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace s3grl {
namespace {

constexpr int kHBlock = 256;
constexpr int kTile = 16;            // nodes per SpMM workgroup: fixes the reduction tree of every column
constexpr int kWaves = kHBlock / 64;
constexpr int kCheckEvery = 8;       // iterations between host reads of the active flags (early exit only)
constexpr int64_t kBudgetBytes = int64_t(128) << 20;   // both iterate buffers: about the Infinity Cache
constexpr int kMinWidth = 64, kMaxWidth = 1024, kDefaultMaxWidth = 256;


__global__ __launch_bounds__(kHBlock) void prepare_kernel(int64_t n, const int64_t* __restrict__ ptr,
                                                          const double* __restrict__ val,
                                                          const int64_t* __restrict__ tptr,
                                                          const double* __restrict__ tval, double* __restrict__ r,
                                                          double* __restrict__ c, double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (i >= n) return;
  double rs = 0.0, cs = 0.0;
  for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) rs += val[e];
  for (int64_t e = tptr[i]; e < tptr[i + 1]; ++e) cs += tval[e];
  r[i] = rs;
  c[i] = cs;
  const double wk = 1.0 / log(cs);
  w[i] = isinf(wk) ? 0.0 : wk;   // c = 1; c = 0 gives -0.0 and 0 < c < 1 a negative weight, both kept
}

__global__ __launch_bounds__(kHBlock) void nan_rows_kernel(int64_t n, const int64_t* __restrict__ ptr,
                                                           const int32_t* __restrict__ idx,
                                                           const double* __restrict__ w,
                                                           int32_t* __restrict__ nan_row) {
  const int64_t i = (int64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (i >= n) return;
  int32_t f = 0;
  for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) f |= isnan(w[idx[e]]) ? 1 : 0;
  nan_row[i] = f;
}

// KIND: one of the five S3GRL_HEURISTIC_*.  wk: the keys' weights, w for AA and v for RA (the others do not read it)
template <int KIND>
__global__ __launch_bounds__(kHBlock) void pairs_kernel(int64_t L, const int32_t* __restrict__ links,
                                                        const int64_t* __restrict__ ptr,
                                                        const int32_t* __restrict__ idx,
                                                        const double* __restrict__ val,
                                                        const double* __restrict__ wk,
                                                        const double* __restrict__ r,
                                                        const int32_t* __restrict__ nan_row,
                                                        float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t l = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (l >= L) return;   // wave-uniform
  const int32_t s = links[l], d = links[L + l];
  if constexpr (KIND == S3GRL_HEURISTIC_PA) {
    if (lane == 0) out[l] = (float)(r[s] * r[d]);
    return;
  }
  const int64_t s0 = ptr[s], s1 = ptr[s + 1], d0 = ptr[d], d1 = ptr[d + 1];
  const RowWalk<int64_t> rows = pick_walk(s0, s1, d0, d1, s, d);
  double acc = 0.0;
  int32_t common = 0;
  if (rows.o1 > rows.o0) {
    for (int64_t e = rows.w0 + lane; e < rows.w1; e += 64) {
      const int32_t k = idx[e];
      const int64_t f = find_sorted(idx, rows.o0, rows.o1, k);
      if (f < 0) continue;
      if constexpr (KIND == S3GRL_HEURISTIC_JACCARD) {
        ++common;
      } else {
        const double as = rows.first ? val[e] : val[f], ad = rows.first ? val[f] : val[e];
        if constexpr (KIND == S3GRL_HEURISTIC_CN) acc += as * ad;
        else acc += as * (ad * wk[k]);
      }
    }
  }
  if constexpr (KIND == S3GRL_HEURISTIC_JACCARD) {
    for (int o = 32; o > 0; o >>= 1) common += __shfl_xor(common, o);
    const int64_t either = (s1 - s0) + (d1 - d0) - common;
    if (lane == 0) out[l] = either > 0 ? (float)((double)common / (double)either) : 0.0f;
  } else {
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0)   // AA: see nan_rows_kernel
      out[l] = (KIND == S3GRL_HEURISTIC_AA && nan_row[d]) ? __builtin_nanf("") : (float)acc;
  }
}

// W = (p·Aᵀ)·diag(1/r) entry by entry (scipy evaluates `p * A.T @ D_1` left to right), and
// z = ((1-p)·[r != 0] + [r == 0]) / n
__global__ __launch_bounds__(kHBlock) void ppr_coef_kernel(int64_t n, const int64_t* __restrict__ tptr,
                                                           const int32_t* __restrict__ tidx,
                                                           const double* __restrict__ tval,
                                                           const double* __restrict__ r, double p,
                                                           double* __restrict__ coef, double* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (i >= n) return;
  for (int64_t e = tptr[i]; e < tptr[i + 1]; ++e) {
    const double rj = r[tidx[e]];
    coef[e] = rj != 0.0 ? (p * tval[e]) * (1.0 / rj) : 0.0;
  }
  z[i] = ((r[i] != 0.0 ? 1.0 - p : 0.0) + (r[i] == 0.0 ? 1.0 : 0.0)) / (double)n;
}

// a block's columns: x0 = s (n at the source; the buffer is zeroed before), t = zᵀs, no iteration yet
__global__ void ppr_init_kernel(int B, int ncols, int64_t b0, const int32_t* __restrict__ sources,
                                const double* __restrict__ z, double nn, int32_t* __restrict__ src,
                                int32_t* __restrict__ active, int32_t* __restrict__ iters, double* __restrict__ tz,
                                double* __restrict__ total, double* __restrict__ x0) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= B) return;
  const int32_t s = c < ncols ? sources[b0 + c] : -1;
  src[c] = s;
  active[c] = s >= 0;
  iters[c] = 0;
  tz[c] = s >= 0 ? z[s] * nn : 0.0;
  total[c] = 1.0;
  if (s >= 0) x0[(int64_t)s * B + c] = nn;
}

__global__ __launch_bounds__(kHBlock) void ppr_spmm_kernel(int64_t n, const int64_t* __restrict__ tptr,
                                                           const int32_t* __restrict__ tidx,
                                                           const double* __restrict__ coef,
                                                           const double* __restrict__ z, int B,
                                                           const int32_t* __restrict__ src,
                                                           const int32_t* __restrict__ active,
                                                           const double* __restrict__ tz, double nn,
                                                           const double* __restrict__ xo, double* __restrict__ xn,
                                                           double* __restrict__ slab) {
  __shared__ double part[3][kWaves][64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.y * 64 + lane;
  const bool act = active[c] != 0;
  if (!__any(act)) return;   // every wave of the workgroup sees the same 64 columns: uniform
  const int32_t s = src[c];
  const double add = act ? nn * tz[c] : 0.0;
  double dd = 0.0, zd = 0.0, sx = 0.0;
  const int64_t i_end = min(n, (int64_t)(blockIdx.x + 1) * kTile);
  if (act) {
    for (int64_t i = (int64_t)blockIdx.x * kTile + w; i < i_end; i += kWaves) {
      double acc = 0.0;
      const int64_t e1 = tptr[i + 1];
      int64_t e = tptr[i];
      for (; e + 4 <= e1; e += 4) {   // four rows in flight, added in entry order
        const double v0 = xo[(int64_t)tidx[e] * B + c], v1 = xo[(int64_t)tidx[e + 1] * B + c];
        const double v2 = xo[(int64_t)tidx[e + 2] * B + c], v3 = xo[(int64_t)tidx[e + 3] * B + c];
        acc += coef[e] * v0;
        acc += coef[e + 1] * v1;
        acc += coef[e + 2] * v2;
        acc += coef[e + 3] * v3;
      }
      for (; e < e1; ++e) acc += coef[e] * xo[(int64_t)tidx[e] * B + c];
      if (i == s) acc += add;
      const double dx = acc - xo[i * B + c];
      xn[i * B + c] = acc;
      dd += dx * dx;
      zd += z[i] * acc;
      sx += acc;
    }
  }
  part[0][w][lane] = dd;
  part[1][w][lane] = zd;
  part[2][w][lane] = sx;
  __syncthreads();
  if (w < 3 && act)
    slab[((int64_t)w * B + c) * gridDim.x + blockIdx.x] =
        (part[w][0][lane] + part[w][1][lane]) + (part[w][2][lane] + part[w][3][lane]);
}

__global__ __launch_bounds__(kHBlock) void ppr_reduce_kernel(int B, int64_t tiles, const double* __restrict__ slab,
                                                             double tol, int max_iter, int32_t* __restrict__ active,
                                                             int32_t* __restrict__ iters, double* __restrict__ tz,
                                                             double* __restrict__ total) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (c >= B || !active[c]) return;   // wave-uniform
  double v[3] = {0.0, 0.0, 0.0};
  for (int64_t t = lane; t < tiles; t += 64)
    for (int q = 0; q < 3; ++q) v[q] += slab[((int64_t)q * B + c) * tiles + t];
  for (int q = 0; q < 3; ++q)
    for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o);
  if (lane == 0) {
    const int k = iters[c] + 1;
    iters[c] = k;
    tz[c] = v[1];
    total[c] = v[2];
    if (!(sqrt(v[0]) > tol) || k >= max_iter) active[c] = 0;
  }
}

__global__ __launch_bounds__(kHBlock) void ppr_finish_kernel(int64_t L, const int32_t* __restrict__ links,
                                                             const int32_t* __restrict__ link_col, int64_t b0,
                                                             int ncols, int B, const double* __restrict__ x0,
                                                             const double* __restrict__ x1,
                                                             const int32_t* __restrict__ iters,
                                                             const double* __restrict__ total,
                                                             float* __restrict__ out, int32_t* __restrict__ it_out) {
  const int64_t t = (int64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (it_out && t < ncols) it_out[b0 + t] = iters[t];
  if (t >= L) return;
  const int64_t g = (int64_t)link_col[t] - b0;
  if (g < 0 || g >= ncols) return;
  const double* x = (iters[g] & 1) ? x1 : x0;
  out[t] = (float)(x[(int64_t)links[L + t] * B + g] / total[g]);
}

// ---- RA's weights and Katz ------------------------------------------------------------------------------------

__global__ __launch_bounds__(kHBlock) void ra_weights_kernel(int64_t n, const double* __restrict__ c,
                                                             double* __restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (i >= n) return;
  v[i] = c[i] != 0.0 ? 1.0 / c[i] : 0.0;   // a negative or fractional column sum: a finite weight, kept
}

// One Horner level for the block's columns: xn[j] = β·Σ_i A[i, j]·(xo[i] + [i = s]), column j's entries in ascending
// i (row j of Aᵀ in CSR order).  Tiles, wave split and loads in flight as in ppr_spmm_kernel; the block's padding
// columns (c >= ncols) never run and are never read.
__global__ __launch_bounds__(kHBlock) void katz_spmm_kernel(int64_t n, const int64_t* __restrict__ tptr,
                                                            const int32_t* __restrict__ tidx,
                                                            const double* __restrict__ tval, int B, int ncols,
                                                            const int32_t* __restrict__ src, double beta,
                                                            const double* __restrict__ xo, double* __restrict__ xn) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.y * 64 + lane;
  if (c >= ncols) return;
  const int32_t s = src[c];
  const int64_t i_end = min(n, (int64_t)(blockIdx.x + 1) * kTile);
  for (int64_t i = (int64_t)blockIdx.x * kTile + w; i < i_end; i += kWaves) {
    double acc = 0.0;
    const int64_t e1 = tptr[i + 1];
    int64_t e = tptr[i];
    for (; e + 4 <= e1; e += 4) {   // four rows in flight, added in entry order
      const int32_t j0 = tidx[e], j1 = tidx[e + 1], j2 = tidx[e + 2], j3 = tidx[e + 3];
      const double v0 = xo[(int64_t)j0 * B + c], v1 = xo[(int64_t)j1 * B + c];
      const double v2 = xo[(int64_t)j2 * B + c], v3 = xo[(int64_t)j3 * B + c];
      acc += tval[e] * (v0 + (j0 == s ? 1.0 : 0.0));
      acc += tval[e + 1] * (v1 + (j1 == s ? 1.0 : 0.0));
      acc += tval[e + 2] * (v2 + (j2 == s ? 1.0 : 0.0));
      acc += tval[e + 3] * (v3 + (j3 == s ? 1.0 : 0.0));
    }
    for (; e < e1; ++e) {
      const int32_t j = tidx[e];
      acc += tval[e] * (xo[(int64_t)j * B + c] + (j == s ? 1.0 : 0.0));
    }
    xn[i * B + c] = beta * acc;
  }
}

__global__ __launch_bounds__(kHBlock) void katz_finish_kernel(int64_t L, const int32_t* __restrict__ links,
                                                              const int32_t* __restrict__ link_col, int64_t b0,
                                                              int ncols, int B, const double* __restrict__ x,
                                                              float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (t >= L) return;
  const int64_t g = (int64_t)link_col[t] - b0;
  if (g < 0 || g >= ncols) return;
  out[t] = (float)x[(int64_t)links[L + t] * B + g];
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

struct s3grl_heuristics {
  s3grl_context* ctx = nullptr;
  int64_t N = 0, nnz = 0;
  int64_t *ptr = nullptr, *tptr = nullptr;
  int32_t *idx = nullptr, *tidx = nullptr;
  double *val = nullptr, *tval = nullptr;
  double *r = nullptr, *c = nullptr, *w = nullptr;
  double* v = nullptr;   // RA weights 1 / c
  int32_t* nan_row = nullptr;
  // PPR work buffers, grown on demand
  double *coef = nullptr, *z = nullptr;
  size_t cap_x = 0, cap_slab = 0, cap_links = 0, cap_src = 0;
  double *x0 = nullptr, *x1 = nullptr, *slab = nullptr;
  int32_t *col_src = nullptr, *active = nullptr, *iters = nullptr;   // [kMaxWidth]
  double *tz = nullptr, *total = nullptr;                              // [kMaxWidth]
  int32_t *link_col = nullptr, *sources = nullptr;
};

namespace {

void h_free(s3grl_heuristics* h) {
  for (void* p : {(void*)h->ptr, (void*)h->tptr, (void*)h->idx, (void*)h->tidx, (void*)h->val, (void*)h->tval,
                  (void*)h->r, (void*)h->c, (void*)h->w, (void*)h->v, (void*)h->nan_row, (void*)h->coef, (void*)h->z,
                  (void*)h->x0, (void*)h->x1,
                  (void*)h->slab, (void*)h->col_src, (void*)h->active, (void*)h->iters, (void*)h->tz,
                  (void*)h->total, (void*)h->link_col, (void*)h->sources})
    if (p) (void)hipFree(p);
}

template <typename T>
s3grl_status h_grow(T** p, size_t* cap, size_t count) {
  if (count <= *cap && *p) return S3GRL_OK;
  S3GRL_TRY(regrow(p, count));
  *cap = count;
  return S3GRL_OK;
}

// links [2, L] device: every id checked against [0, N) on the host; `host` (may be null) receives the copy
s3grl_status check_links(s3grl_heuristics* h, const int32_t* links, int64_t L, std::vector<int32_t>* host = nullptr) {
  return check_ids(h->ctx, links, 2 * L, h->N, "heuristics: a link endpoint outside [0, N)", host);
}

// The per-source solvers' lists: `sources` must be distinct ids in [0, N) and every link's source one of them.  Leaves
// the sources in h->sources and each link's column (its source's position) in h->link_col.  Waits for the device.
s3grl_status stage_sources(s3grl_heuristics* h, const char* who, const int32_t* sources, int64_t num_sources,
                           const int32_t* links, int64_t num_links) {
  hipStream_t st = h->ctx->stream;
  std::vector<int32_t> src((size_t)num_sources), lk;
  if (num_sources)
    S3GRL_HIP_TRY(hipMemcpyAsync(src.data(), sources, src.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  S3GRL_TRY(check_links(h, links, num_links, &lk));   // its wait completes the copy of the sources too
  std::vector<int32_t> col_of((size_t)h->N, -1), link_col((size_t)num_links);
  for (int64_t k = 0; k < num_sources; ++k) {
    const int32_t v = src[(size_t)k];
    if (v < 0 || v >= h->N || col_of[(size_t)v] >= 0) {
      set_last_error(std::string(who) + ": sources must be distinct ids in [0, N)");
      return S3GRL_ERR_INVALID_ARGUMENT;
    }
    col_of[(size_t)v] = (int32_t)k;
  }
  for (int64_t l = 0; l < num_links; ++l) {
    link_col[(size_t)l] = col_of[(size_t)lk[(size_t)l]];
    if (link_col[(size_t)l] < 0) {
      set_last_error(std::string(who) + ": a link whose source is not in sources");
      return S3GRL_ERR_INVALID_ARGUMENT;
    }
  }
  S3GRL_TRY(h_grow(&h->sources, &h->cap_src, (size_t)num_sources));
  S3GRL_TRY(h_grow(&h->link_col, &h->cap_links, (size_t)num_links));
  if (num_sources)
    S3GRL_HIP_TRY(hipMemcpyAsync(h->sources, src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (num_links)
    S3GRL_HIP_TRY(hipMemcpyAsync(h->link_col, link_col.data(), link_col.size() * sizeof(int32_t),
                                 hipMemcpyHostToDevice, st));
  S3GRL_HIP_TRY(hipStreamSynchronize(st));   // the host vectors go out of scope
  return S3GRL_OK;
}

// both iterate buffers, [N, width] fp64 each
s3grl_status grow_iterates(s3grl_heuristics* h, size_t count) {
  if (count <= h->cap_x) return S3GRL_OK;
  h->cap_x = 0;
  S3GRL_TRY(regrow(&h->x0, count));
  S3GRL_TRY(regrow(&h->x1, count));
  h->cap_x = count;
  return S3GRL_OK;
}

bool bad_width(int32_t block_width) {
  return block_width != 0 && (block_width < kMinWidth || block_width > kMaxWidth || block_width % 64);
}

int default_width(int64_t n) {
  int64_t b = kBudgetBytes / (2 * 8 * std::max<int64_t>(n, 1));
  b = std::min<int64_t>(std::max<int64_t>(b / 64 * 64, kMinWidth), kDefaultMaxWidth);
  return (int)b;
}

}  // namespace

extern "C" {

s3grl_status s3grl_heuristics_create(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr,
                                     const int32_t* indices, const double* values, int64_t num_entries,
                                     s3grl_heuristics** out) {
  if (!ctx || !out || !indptr || num_nodes < 1 || num_entries < 0 || (num_entries > 0 && !indices))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_nodes >= (int64_t(1) << 31) || num_entries >= (int64_t(1) << 31)) return S3GRL_ERR_GRAPH_TOO_LARGE;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  // the CSR is checked and transposed on the host once: input preparation, the kernels trust it
  const size_t n = (size_t)num_nodes, m = (size_t)num_entries;
  std::vector<int64_t> ip;
  std::vector<int32_t> ix;
  std::vector<double> vx(m, 1.0);
  if (m && values)   // check_csr's wait completes this copy too
    S3GRL_HIP_TRY(hipMemcpyAsync(vx.data(), values, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  S3GRL_TRY(check_csr(ctx, num_nodes, indptr, indices, num_entries, /*ascending=*/true,
                      "heuristics: malformed CSR (indptr not monotone from 0 to nnz, a column outside [0, N), or a "
                      "row not strictly ascending)",
                      &ip, &ix));
  // Aᵀ by a stable counting sort: row k of Aᵀ lists the rows j with A[j, k] != 0 in ascending order
  std::vector<int64_t> tp(n + 1, 0);
  std::vector<int32_t> tx(m);
  std::vector<double> tv(m);
  for (size_t e = 0; e < m; ++e) ++tp[(size_t)ix[e] + 1];
  for (size_t i = 0; i < n; ++i) tp[i + 1] += tp[i];
  {
    std::vector<int64_t> fill(tp.begin(), tp.end() - 1);
    for (size_t j = 0; j < n; ++j)
      for (int64_t e = ip[j]; e < ip[j + 1]; ++e) {
        const int64_t at = fill[(size_t)ix[e]]++;
        tx[at] = (int32_t)j;
        tv[at] = vx[e];
      }
  }
  auto* h = new s3grl_heuristics();
  h->ctx = ctx;
  h->N = num_nodes;
  h->nnz = num_entries;
  s3grl_status s = S3GRL_OK;
  if ((s = regrow(&h->ptr, n + 1)) || (s = regrow(&h->tptr, n + 1)) || (s = regrow(&h->idx, m)) ||
      (s = regrow(&h->tidx, m)) || (s = regrow(&h->val, m)) || (s = regrow(&h->tval, m)) ||
      (s = regrow(&h->r, n)) || (s = regrow(&h->c, n)) || (s = regrow(&h->w, n)) || (s = regrow(&h->v, n)) ||
      (s = regrow(&h->nan_row, n)) || (s = regrow(&h->coef, m)) ||
      (s = regrow(&h->z, n)) || (s = regrow(&h->col_src, kMaxWidth)) || (s = regrow(&h->active, kMaxWidth)) ||
      (s = regrow(&h->iters, kMaxWidth)) || (s = regrow(&h->tz, kMaxWidth)) ||
      (s = regrow(&h->total, kMaxWidth))) {
    h_free(h);
    delete h;
    return s;
  }
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(h->ptr, ip.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h->tptr, tp.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && m) e = hipMemcpyAsync(h->idx, ix.data(), m * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && m) e = hipMemcpyAsync(h->tidx, tx.data(), m * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && m) e = hipMemcpyAsync(h->val, vx.data(), m * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && m) e = hipMemcpyAsync(h->tval, tv.data(), m * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(prepare_kernel, dim3(grid_of(num_nodes, kHBlock)), dim3(kHBlock), 0, st, num_nodes, h->ptr,
                       h->val, h->tptr, h->tval, h->r, h->c, h->w);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(nan_rows_kernel, dim3(grid_of(num_nodes, kHBlock)), dim3(kHBlock), 0, st, num_nodes, h->ptr,
                       h->idx, h->w, h->nan_row);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(ra_weights_kernel, dim3(grid_of(num_nodes, kHBlock)), dim3(kHBlock), 0, st, num_nodes, h->c,
                       h->v);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);   // the host vectors go out of scope
  if (e != hipSuccess) {
    set_last_error(std::string("heuristics create: ") + hipGetErrorString(e));
    h_free(h);
    delete h;
    return e == hipErrorOutOfMemory ? S3GRL_ERR_OUT_OF_MEMORY : S3GRL_ERR_HIP;
  }
  *out = h;
  return S3GRL_OK;
}

s3grl_status s3grl_heuristics_pairs(s3grl_heuristics* h, int32_t kind, const int32_t* links, int64_t num_links,
                                    float* out) {
  if (!h || num_links < 0 || (num_links > 0 && (!links || !out)) || kind < S3GRL_HEURISTIC_CN ||
      kind > S3GRL_HEURISTIC_PA)
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_links == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(h->ctx->device));
  S3GRL_TRY(check_links(h, links, num_links));
  auto* pairs = kind == S3GRL_HEURISTIC_CN        ? pairs_kernel<S3GRL_HEURISTIC_CN>
                : kind == S3GRL_HEURISTIC_AA      ? pairs_kernel<S3GRL_HEURISTIC_AA>
                : kind == S3GRL_HEURISTIC_RA      ? pairs_kernel<S3GRL_HEURISTIC_RA>
                : kind == S3GRL_HEURISTIC_JACCARD ? pairs_kernel<S3GRL_HEURISTIC_JACCARD>
                                                  : pairs_kernel<S3GRL_HEURISTIC_PA>;
  hipLaunchKernelGGL(pairs, dim3(grid_of(num_links, kWaves)), dim3(kHBlock), 0, h->ctx->stream, num_links, links,
                     h->ptr, h->idx, h->val, kind == S3GRL_HEURISTIC_AA ? h->w : h->v, h->r, h->nan_row, out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_heuristics_ppr(s3grl_heuristics* h, const int32_t* sources, int64_t num_sources,
                                  const int32_t* links, int64_t num_links, double p, double tol, int32_t max_iter,
                                  int32_t block_width, float* out, int32_t* iterations) {
  if (!h || num_sources < 0 || num_links < 0 || (num_sources > 0 && !sources) ||
      (num_links > 0 && (!links || !out)) || !(p >= 0.0 && p <= 1.0) || !(tol >= 0.0) || max_iter < 1 ||
      bad_width(block_width))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_sources == 0 && num_links == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(h->ctx->device));
  hipStream_t st = h->ctx->stream;
  S3GRL_TRY(stage_sources(h, "heuristics ppr", sources, num_sources, links, num_links));
  const int64_t N = h->N, tiles = (N + kTile - 1) / kTile;
  const int B = block_width ? block_width : default_width(N);
  const int Bmax = (int)std::min<int64_t>(B, (num_sources + 63) / 64 * 64);
  S3GRL_TRY(grow_iterates(h, (size_t)N * Bmax));
  S3GRL_TRY(h_grow(&h->slab, &h->cap_slab, (size_t)tiles * 3 * Bmax));
  hipLaunchKernelGGL(ppr_coef_kernel, dim3(grid_of(N, kHBlock)), dim3(kHBlock), 0, st, N, h->tptr, h->tidx, h->tval,
                     h->r, p, h->coef, h->z);
  S3GRL_HIP_TRY(hipGetLastError());
  const double nn = (double)N;
  std::vector<int32_t> flags(kMaxWidth);
  for (int64_t b0 = 0; b0 < num_sources; b0 += B) {
    const int ncols = (int)std::min<int64_t>(B, num_sources - b0);
    const int Bc = (ncols + 63) / 64 * 64;   // the block's row stride; padding columns never run
    S3GRL_HIP_TRY(hipMemsetAsync(h->x0, 0, (size_t)N * Bc * sizeof(double), st));
    hipLaunchKernelGGL(ppr_init_kernel, dim3(grid_of(Bc, 64)), dim3(64), 0, st, Bc, ncols, b0, h->sources, h->z, nn,
                       h->col_src, h->active, h->iters, h->tz, h->total, h->x0);
    S3GRL_HIP_TRY(hipGetLastError());
    for (int it = 1; it <= max_iter; ++it) {
      const double* xo = (it & 1) ? h->x0 : h->x1;
      double* xn = (it & 1) ? h->x1 : h->x0;
      hipLaunchKernelGGL(ppr_spmm_kernel, dim3((unsigned)tiles, (unsigned)(Bc / 64)), dim3(kHBlock), 0, st, N,
                         h->tptr, h->tidx, h->coef, h->z, Bc, h->col_src, h->active, h->tz, nn, xo, xn, h->slab);
      S3GRL_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(ppr_reduce_kernel, dim3(grid_of(Bc, kWaves)), dim3(kHBlock), 0, st, Bc, tiles, h->slab, tol,
                         (int)max_iter, h->active, h->iters, h->tz, h->total);
      S3GRL_HIP_TRY(hipGetLastError());
      if (it % kCheckEvery == 0 && it < max_iter) {   // early exit once every column is frozen; no effect on values
        S3GRL_HIP_TRY(hipMemcpyAsync(flags.data(), h->active, (size_t)Bc * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        S3GRL_HIP_TRY(hipStreamSynchronize(st));
        if (std::all_of(flags.begin(), flags.begin() + Bc, [](int32_t f) { return f == 0; })) break;
      }
    }
    hipLaunchKernelGGL(ppr_finish_kernel, dim3(grid_of(std::max<int64_t>(num_links, ncols), kHBlock)),
                       dim3(kHBlock), 0, st, num_links, links, h->link_col, b0, ncols, Bc, h->x0, h->x1, h->iters,
                       h->total, out, iterations);
    S3GRL_HIP_TRY(hipGetLastError());
  }
  S3GRL_HIP_TRY(hipStreamSynchronize(st));
  return S3GRL_OK;
}

s3grl_status s3grl_heuristics_katz(s3grl_heuristics* h, const int32_t* sources, int64_t num_sources,
                                   const int32_t* links, int64_t num_links, double beta, int32_t max_len,
                                   int32_t block_width, float* out) {
  if (!h || num_sources < 0 || num_links < 0 || (num_sources > 0 && !sources) ||
      (num_links > 0 && (!links || !out)) || !std::isfinite(beta) || max_len < 1 || max_len > S3GRL_KATZ_MAX_LEN ||
      bad_width(block_width))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_sources == 0 && num_links == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(h->ctx->device));
  hipStream_t st = h->ctx->stream;
  S3GRL_TRY(stage_sources(h, "heuristics katz", sources, num_sources, links, num_links));
  const int64_t N = h->N, tiles = (N + kTile - 1) / kTile;
  const int B = block_width ? block_width : default_width(N);
  const int Bmax = (int)std::min<int64_t>(B, (num_sources + 63) / 64 * 64);
  S3GRL_TRY(grow_iterates(h, (size_t)N * Bmax));
  for (int64_t b0 = 0; b0 < num_sources; b0 += B) {
    const int ncols = (int)std::min<int64_t>(B, num_sources - b0);
    const int Bc = (ncols + 63) / 64 * 64;   // the block's row stride; padding columns never run
    S3GRL_HIP_TRY(hipMemsetAsync(h->x0, 0, (size_t)N * Bc * sizeof(double), st));   // x_0 = 0
    for (int level = 1; level <= max_len; ++level) {   // level l reads buffer (l - 1) & 1 and writes buffer l & 1
      const double* xo = (level & 1) ? h->x0 : h->x1;
      double* xn = (level & 1) ? h->x1 : h->x0;
      hipLaunchKernelGGL(katz_spmm_kernel, dim3((unsigned)tiles, (unsigned)(Bc / 64)), dim3(kHBlock), 0, st, N,
                         h->tptr, h->tidx, h->tval, Bc, ncols, h->sources + b0, beta, xo, xn);
      S3GRL_HIP_TRY(hipGetLastError());
    }
    if (num_links) {
      hipLaunchKernelGGL(katz_finish_kernel, dim3(grid_of(num_links, kHBlock)), dim3(kHBlock), 0, st, num_links,
                         links, h->link_col, b0, ncols, Bc, (max_len & 1) ? h->x1 : h->x0, out);
      S3GRL_HIP_TRY(hipGetLastError());
    }
  }
  S3GRL_HIP_TRY(hipStreamSynchronize(st));
  return S3GRL_OK;
}

s3grl_status s3grl_heuristics_destroy(s3grl_heuristics* h) {
  if (!h) return S3GRL_OK;
  (void)hipSetDevice(h->ctx->device);
  (void)hipStreamSynchronize(h->ctx->stream);
  h_free(h);
  delete h;
  return S3GRL_OK;
}

}  // extern "C"
