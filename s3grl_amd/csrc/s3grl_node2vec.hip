// node2vec pretraining (PyG Node2Vec with p = q = 1, sparse=True, trained by torch.optim.SparseAdam; reference
// n2v_prep.py) on gfx950.  One optimiser step over a batch of B start nodes is the radix sort plus five launches, all stream-ordered:
//
//   windows_kernel   one thread per walk row: the B·R positive walks (uniform over the CSR entries of the node,
//                    a node without entries stays put) and the B·R·Q negative rows (start, then uniform draws
//                    from [0, N)), written straight into their C-node windows, window-index-major
//   dots_kernel      one group of LPD lanes per dot <h[w0], h[wi]>: the dot, its loss term, the loss derivative
//                    g (the EPS form PyG's loss has) and two sort keys, (row << ib | 2·dot + side), one for each
//                    row the dot's gradient lands on
//   radix sort       rocPRIM, keys only, ib + rb bits: the contributions of every touched row, in index order
//   bounds_kernel    one thread per sorted key: the key range [first, last) of every row the step touches
//   row_grad_kernel  one wavefront per touched row: Σ g · h[other] over the row's keys, in key order within each
//                    of 64 / LPD fixed slices, the slices added by a fixed butterfly, into the row's gradient
//   adam_kernel      one group of LPD lanes per touched row: SparseAdam's row update of the embedding and both
//                    moment tables
//
// Determinism: no float atomics.  Every draw is a counter-based hash of (seed, epoch, step, stream, row,
// position), the generator of s3grl_train.hpp with a 2-bit stream field; the sort keys are unique, so the sorted
// order is fixed; each row's gradient is summed in that order by a fixed slice assignment and a fixed reduction
// tree.  Two runs with one seed are bit-identical.  Lane layout: VEC channels
// per lane (float4 when D % 4 == 0), LPD lanes per dot / row, the smallest power of two covering D / VEC (up to
// 64): D = 16 is four lanes per dot, sixteen dots per wavefront; D = 256 a wavefront per dot.
#include "s3grl_internal.hpp"
#include "s3grl_device.hpp"
#include "s3grl_train.hpp"

#include <algorithm>
#include <cmath>

namespace s3grl {
namespace {

constexpr int kSgBlock = 256;
constexpr int64_t kMaxDim = 1 << 14;
enum Stream : uint32_t { kPosWalk = 0, kNegDraw = 1, kPermute = 2, kInit = 3 };

int bits_for(uint64_t v) {   // bits to hold every value in [0, v]
  int b = 1;
  while (b < 64 && (v >> b)) ++b;
  return b;
}

// ---- windows -----------------------------------------------------------------------------------------------
// rows [0, B·R): positive walks of batch[r % B] (batch.repeat(R)); rows [B·R, B·R·(1+Q)): negative rows.  Node s
// of a row is column s - j of every window j in [max(0, s-C+1), min(s, W-1)], window j of row r at j·rows + r.
__global__ __launch_bounds__(kSgBlock) void windows_kernel(const int32_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices, int32_t n,
                                                           const int32_t* __restrict__ batch, int B, int R, int Q,
                                                           int L, int C, uint64_t kpos, uint64_t kneg,
                                                           int32_t* __restrict__ pos, int32_t* __restrict__ neg) {
  const int64_t t = (int64_t)blockIdx.x * kSgBlock + threadIdx.x;
  const int64_t rp = (int64_t)B * R, rn = rp * Q;
  if (t >= rp + rn) return;
  const bool is_pos = t < rp;
  const int64_t r = is_pos ? t : t - rp;
  const int64_t rows = is_pos ? rp : rn;
  int32_t* __restrict__ out = is_pos ? pos : neg;
  const int W = L + 2 - C;
  int cur = batch[r % B];
  for (int s = 0; s <= L; ++s) {
    if (s > 0) {
      if (is_pos) {
        const int b = indptr[cur], deg = indptr[cur + 1] - b;
        if (deg > 0) cur = indices[b + below(draw(kpos, (uint64_t)r, (uint64_t)s), (uint32_t)deg)];
      } else {
        cur = (int)below(draw(kneg, (uint64_t)r, (uint64_t)s), (uint32_t)n);
      }
    }
    const int j0 = max(0, s - C + 1), j1 = min(s, W - 1);
    for (int j = j0; j <= j1; ++j) out[((int64_t)j * rows + r) * C + (s - j)] = cur;
  }
}

// ---- dots --------------------------------------------------------------------------------------------------
// dot d = window d / (C-1), column 1 + d % (C-1); windows [0, npos_w) are positive.  PyG's loss:
//   pos  -log(sigmoid(out) + EPS).mean()      d/dout = -s(1-s) / (s + EPS) / n_pos
//   neg  -log(1 - sigmoid(out) + EPS).mean()  d/dout =  s(1-s) / (1 - s + EPS) / n_neg
// partial[2b], [2b+1]: block b's Σ of positive and negative terms
template <int VEC, int LPD>
__global__ __launch_bounds__(kSgBlock) void dots_kernel(int64_t ndots, int64_t npos_w, int C, int D,
                                                        const int32_t* __restrict__ win, const float* __restrict__ h,
                                                        float inv_pos, float inv_neg, int ib, float* __restrict__ gdot,
                                                        uint64_t* __restrict__ keys, double* __restrict__ partial) {
  typedef Vec<VEC> V;
  __shared__ double sh[kSgBlock / 64];
  const int q = threadIdx.x % LPD;
  const int64_t d = (int64_t)blockIdx.x * (kSgBlock / LPD) + threadIdx.x / LPD;
  double tp = 0.0, tn = 0.0;
  if (d < ndots) {
    const int64_t k = d / (C - 1);
    const int i = 1 + (int)(d - k * (C - 1));
    const int64_t a = win[k * C], b = win[k * C + i];
    float acc = 0.f;
    for (int c = q * VEC; c < D; c += LPD * VEC) acc += V::sum(V::load(h + a * D + c) * V::load(h + b * D + c));
    for (int o = LPD / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);   // the group's lanes, fixed butterfly
    if (q == 0) {
      const float s = 1.f / (1.f + expf(-acc));
      float g;
      if (k < npos_w) {
        tp = -logf(s + 1e-15f);
        g = -(s * (1.f - s)) / (s + 1e-15f) * inv_pos;
      } else {
        tn = -logf(1.f - s + 1e-15f);
        g = (s * (1.f - s)) / (1.f - s + 1e-15f) * inv_neg;
      }
      gdot[d] = g;
      keys[2 * d] = ((uint64_t)a << ib) | (uint64_t)(2 * d);           // row w0 gets g · h[wi]
      keys[2 * d + 1] = ((uint64_t)b << ib) | (uint64_t)(2 * d + 1);   // row wi gets g · h[w0]
    }
  }
  const double sp = block_sum_f64<kSgBlock>(tp, sh);
  const double sn = block_sum_f64<kSgBlock>(tn, sh);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = sp;
    partial[2 * blockIdx.x + 1] = sn;
  }
}

// ---- gradient ----------------------------------------------------------------------------------------------
// first[u], last[u]: the sorted keys of row u are [first, last); stamp[u] = the step that wrote them (rows the step
// does not touch keep an older stamp).  Block 0 also folds the dots' loss partials, in block order, into loss_out.
__global__ __launch_bounds__(kSgBlock) void bounds_kernel(int64_t nc, int ib, const uint64_t* __restrict__ keys,
                                                          int32_t* __restrict__ first, int32_t* __restrict__ last,
                                                          int64_t* __restrict__ stamp, int64_t step_id,
                                                          const double* __restrict__ partial, int64_t nparts,
                                                          double inv_pos, double inv_neg, float* __restrict__ loss_out) {
  if (blockIdx.x == 0 && loss_out) {
    __shared__ double sh[kSgBlock / 64];
    double sp = 0.0, sn = 0.0;
    for (int64_t j = threadIdx.x; j < nparts; j += kSgBlock) {
      sp += partial[2 * j];
      sn += partial[2 * j + 1];
    }
    sp = block_sum_f64<kSgBlock>(sp, sh);
    sn = block_sum_f64<kSgBlock>(sn, sh);
    if (threadIdx.x == 0) loss_out[0] = (float)(sp * inv_pos + sn * inv_neg);
  }
  const int64_t p = (int64_t)blockIdx.x * kSgBlock + threadIdx.x;
  if (p >= nc) return;
  const int64_t u = (int64_t)(keys[p] >> ib);
  if (p == 0 || (int64_t)(keys[p - 1] >> ib) != u) {
    first[u] = (int32_t)p;
    stamp[u] = step_id;
  }
  if (p == nc - 1 || (int64_t)(keys[p + 1] >> ib) != u) last[u] = (int32_t)(p + 1);
}

// One wavefront per row: S = 64 / LPD slices of LPD lanes; slice s sums the row's keys first + s, first + s + S, ...
// in order, then the slices are added by a fixed butterfly.  grad[u] = Σ g · h[other] over the row's keys.
template <int VEC, int LPD>
__global__ __launch_bounds__(kSgBlock) void row_grad_kernel(int64_t N, int64_t step_id, const int64_t* __restrict__ stamp,
                                                            const int32_t* __restrict__ first,
                                                            const int32_t* __restrict__ last, int ib, int C, int D,
                                                            const uint64_t* __restrict__ keys,
                                                            const int32_t* __restrict__ win,
                                                            const float* __restrict__ gdot, const float* __restrict__ h,
                                                            float* __restrict__ grad) {
  typedef Vec<VEC> V;
  typedef typename V::T T;
  constexpr int S = 64 / LPD;
  const int64_t u = (int64_t)blockIdx.x * (kSgBlock / 64) + (threadIdx.x >> 6);
  if (u >= N || stamp[u] != step_id) return;
  const int lane = threadIdx.x & 63, q = lane % LPD, sl = lane / LPD;
  const int64_t p0 = first[u], p1 = last[u];
  const uint64_t mask = (1ull << ib) - 1;
  for (int c = q * VEC; c < D; c += LPD * VEC) {
    T acc = (T)(0.f);
#pragma unroll 4
    for (int64_t p = p0 + sl; p < p1; p += S) {
      const int64_t key = (int64_t)(keys[p] & mask), d = key >> 1, k = d / (C - 1);
      const int64_t other = (key & 1) ? win[k * C] : win[k * C + 1 + (d - k * (C - 1))];
      acc += gdot[d] * V::load(h + other * D + c);
    }
#pragma unroll
    for (int o = S / 2; o > 0; o >>= 1) {   // slice s + o into slice s, the same tree in every lane
#pragma unroll
      for (int i = 0; i < VEC; ++i) V::set(acc, i, V::at(acc, i) + __shfl_xor(V::at(acc, i), o * LPD, 64));
    }
    if (sl == 0) V::store(grad + u * D + c, acc);
  }
}

// ---- SparseAdam --------------------------------------------------------------------------------------------
// torch.optim.SparseAdam on the coalesced rows, in its own operation order:
//   m' = m + (g - m)(1 - b1);  v' = v + (g² - v)(1 - b2);  h' = h + (-step_size) · (m' / (sqrt(v') + eps))
// One group of LPD lanes per row; rows the step did not touch are left alone.
template <int VEC, int LPD>
__global__ __launch_bounds__(kSgBlock) void adam_kernel(int64_t N, int64_t step_id, const int64_t* __restrict__ stamp,
                                                        int D, const float* __restrict__ grad, float* __restrict__ h,
                                                        float* __restrict__ m, float* __restrict__ v, float neg_step,
                                                        float b1c, float b2c, float eps) {
  typedef Vec<VEC> V;
  typedef typename V::T T;
  const int q = threadIdx.x % LPD;
  const int64_t u = (int64_t)blockIdx.x * (kSgBlock / LPD) + threadIdx.x / LPD;
  if (u >= N || stamp[u] != step_id) return;
  for (int c = q * VEC; c < D; c += LPD * VEC) {
    const T g = V::load(grad + u * D + c);
    T mm = V::load(m + u * D + c), vv = V::load(v + u * D + c), hh = V::load(h + u * D + c);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float gi = V::at(g, i), mo = V::at(mm, i), vo = V::at(vv, i);
      const float mn = mo + (gi - mo) * b1c;
      const float vn = vo + (gi * gi - vo) * b2c;
      V::set(mm, i, mn);
      V::set(vv, i, vn);
      V::set(hh, i, V::at(hh, i) + neg_step * (mn / (sqrtf(vn) + eps)));
    }
    V::store(m + u * D + c, mm);
    V::store(v + u * D + c, vv);
    V::store(h + u * D + c, hh);
  }
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

struct s3grl_skipgram {
  s3grl_context* ctx = nullptr;
  int64_t N = 0;
  int D = 0, L = 0, C = 0, R = 0, Q = 0;
  uint32_t seed = 0;
  int vec = 1, lpd = 1;
  int64_t steps = 0;                // SparseAdam's step count
  int32_t *indptr = nullptr, *indices = nullptr;
  float *emb = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr;
  int32_t *first = nullptr, *last = nullptr;   // [N] sorted-key range of every touched row
  int64_t* stamp = nullptr;         // [N] the step that last touched a row (-1: none yet)
  int32_t* perm = nullptr;          // [N] permutation of perm_epoch
  int64_t perm_epoch = -1;
  // per-step buffers, sized for cap_w windows (grown on demand)
  int64_t cap_w = 0, cap_keys = 0;
  int32_t* win = nullptr;           // [cap_w, C] positive windows, then negative
  float* gdot = nullptr;            // [cap_w (C-1)]
  uint64_t *keys_a = nullptr, *keys_b = nullptr;   // [cap_keys]
  double* partial = nullptr;        // [2 · blocks of dots_kernel]
  SortScratch sort;
};

namespace {

// four streams, a 2-bit stream field: the width is part of every draw (s3grl_train.hpp)
uint64_t key_of(const s3grl_skipgram* t, int64_t epoch, int64_t step, Stream stream) {
  return stream_key<2>(t->seed, epoch, step, stream);
}

void sg_free(s3grl_skipgram* t) {
  for (void* p : {(void*)t->indptr, (void*)t->indices, (void*)t->emb, (void*)t->m, (void*)t->v, (void*)t->grad,
                  (void*)t->first, (void*)t->last, (void*)t->stamp, (void*)t->perm, (void*)t->win, (void*)t->gdot,
                  (void*)t->keys_a, (void*)t->keys_b, (void*)t->partial, t->sort.tmp})
    if (p) (void)hipFree(p);
}

int64_t per_block(const s3grl_skipgram* t) { return kSgBlock / t->lpd; }

s3grl_status ensure_windows(s3grl_skipgram* t, int64_t nw) {
  const int64_t keys_needed = std::max<int64_t>(2 * nw * (t->C - 1), t->N);
  if (nw > t->cap_w || keys_needed > t->cap_keys) {
    S3GRL_HIP_TRY(hipStreamSynchronize(t->ctx->stream));   // the old buffers may still be in use
    const int64_t w = std::max(nw, t->cap_w);
    const int64_t dots = w * (t->C - 1);
    const int64_t keys = std::max<int64_t>(2 * dots, t->N);
    S3GRL_TRY(regrow(&t->win, (size_t)(w * t->C)));
    S3GRL_TRY(regrow(&t->gdot, (size_t)dots));
    S3GRL_TRY(regrow(&t->keys_a, (size_t)keys));
    S3GRL_TRY(regrow(&t->keys_b, (size_t)keys));
    S3GRL_TRY(regrow(&t->partial, (size_t)(2 * ((dots + per_block(t) - 1) / per_block(t)))));
    t->cap_w = w;
    t->cap_keys = keys;
  }
  return S3GRL_OK;
}

s3grl_status sort_keys(s3grl_skipgram* t, int64_t n, int end_bit) {
  return sort_keys_u64(t->ctx, t->sort, t->keys_a, t->keys_b, (size_t)n, end_bit);
}

s3grl_status ensure_perm(s3grl_skipgram* t, int64_t epoch) {
  if (t->perm_epoch == epoch) return S3GRL_OK;
  S3GRL_TRY(ensure_windows(t, 0));
  S3GRL_TRY(launch_epoch_perm(t->ctx, key_of(t, epoch, 0, kPermute), t->N, t->keys_a, t->keys_b,
                              t->sort, t->perm));
  t->perm_epoch = epoch;
  return S3GRL_OK;
}

int64_t batch_of(const s3grl_skipgram* t, int64_t step, int64_t bs) { return std::min(bs, t->N - step * bs); }
int64_t windows_per_row(const s3grl_skipgram* t) { return t->L + 2 - t->C; }

s3grl_status launch_windows(s3grl_skipgram* t, int64_t epoch, int64_t step, int64_t bs, int32_t* pos, int32_t* neg) {
  const int64_t B = batch_of(t, step, bs);
  const int64_t rows = B * t->R * (1 + t->Q);
  hipLaunchKernelGGL(windows_kernel, dim3(grid_of(rows, kSgBlock)), dim3(kSgBlock), 0, t->ctx->stream, t->indptr,
                     t->indices, (int32_t)t->N, t->perm + step * bs, (int)B, t->R, t->Q, t->L, t->C,
                     key_of(t, epoch, step, kPosWalk),
                     key_of(t, epoch, step, kNegDraw), pos, neg);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

template <int VEC, int LPD>
s3grl_status launch_step_kernels(s3grl_skipgram* t, int64_t npw, int64_t nnw, float lr, float* loss_out) {
  hipStream_t st = t->ctx->stream;
  const int64_t ndots = (npw + nnw) * (t->C - 1), nc = 2 * ndots;
  const int ib = bits_for((uint64_t)(nc - 1)), rb = bits_for((uint64_t)(t->N - 1));
  const int64_t per = kSgBlock / LPD;
  const unsigned dot_blocks = grid_of(ndots, per);
  const double n_pos = (double)npw * (t->C - 1), n_neg = (double)nnw * (t->C - 1);
  hipLaunchKernelGGL((dots_kernel<VEC, LPD>), dim3(dot_blocks), dim3(kSgBlock), 0, st, ndots, npw, t->C, t->D,
                     t->win, t->emb, (float)(1.0 / n_pos), (float)(1.0 / n_neg), ib, t->gdot, t->keys_a, t->partial);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(sort_keys(t, nc, ib + rb));
  const int64_t step_id = t->steps;   // before this step's increment: a row touched by it carries this stamp
  hipLaunchKernelGGL(bounds_kernel, dim3(grid_of(nc, kSgBlock)), dim3(kSgBlock), 0, st, nc, ib, t->keys_b, t->first,
                     t->last, t->stamp, step_id, t->partial, (int64_t)dot_blocks, 1.0 / n_pos, 1.0 / n_neg, loss_out);
  S3GRL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL((row_grad_kernel<VEC, LPD>), dim3(grid_of(t->N, kSgBlock / 64)), dim3(kSgBlock), 0, st, t->N,
                     step_id, t->stamp, t->first, t->last, ib, t->C, t->D, t->keys_b, t->win, t->gdot, t->emb, t->grad);
  S3GRL_HIP_TRY(hipGetLastError());
  t->steps += 1;
  const double bc1 = 1.0 - std::pow(kAdamBeta1, (double)t->steps), bc2 = 1.0 - std::pow(kAdamBeta2, (double)t->steps);
  const double step_size = (double)lr * std::sqrt(bc2) / bc1;
  hipLaunchKernelGGL((adam_kernel<VEC, LPD>), dim3(grid_of(t->N, per)), dim3(kSgBlock), 0, st, t->N, step_id, t->stamp,
                     t->D, t->grad, t->emb, t->m, t->v, (float)(-step_size), (float)(1.0 - kAdamBeta1),
                     (float)(1.0 - kAdamBeta2), (float)kAdamEps);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

template <int VEC>
s3grl_status dispatch_lpd(s3grl_skipgram* t, int64_t npw, int64_t nnw, float lr, float* loss_out) {
  switch (t->lpd) {
    case 1: return launch_step_kernels<VEC, 1>(t, npw, nnw, lr, loss_out);
    case 2: return launch_step_kernels<VEC, 2>(t, npw, nnw, lr, loss_out);
    case 4: return launch_step_kernels<VEC, 4>(t, npw, nnw, lr, loss_out);
    case 8: return launch_step_kernels<VEC, 8>(t, npw, nnw, lr, loss_out);
    case 16: return launch_step_kernels<VEC, 16>(t, npw, nnw, lr, loss_out);
    case 32: return launch_step_kernels<VEC, 32>(t, npw, nnw, lr, loss_out);
    default: return launch_step_kernels<VEC, 64>(t, npw, nnw, lr, loss_out);
  }
}

// the windows are in t->win: npw positive, then nnw negative
s3grl_status run_step(s3grl_skipgram* t, int64_t npw, int64_t nnw, float lr, float* loss_out) {
  if (2 * (npw + nnw) * (t->C - 1) >= (int64_t(1) << 31)) {   // key positions are int32
    set_last_error("node2vec: more than 2^30 dots in one step");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  return t->vec == 4 ? dispatch_lpd<4>(t, npw, nnw, lr, loss_out) : dispatch_lpd<1>(t, npw, nnw, lr, loss_out);
}

}  // namespace

extern "C" {

s3grl_status s3grl_skipgram_create(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                                   int64_t num_entries, const s3grl_skipgram_cfg* cfg, const float* init,
                                   s3grl_skipgram** out) {
  if (!ctx || !cfg || !out || num_nodes < 1 || num_nodes >= (int64_t(1) << 31) || num_entries < 0 ||
      num_entries >= (int64_t(1) << 31) || !indptr || (num_entries > 0 && !indices))
    return S3GRL_ERR_INVALID_ARGUMENT;
  for (int32_t r : cfg->reserved)
    if (r) return S3GRL_ERR_INVALID_ARGUMENT;
  if (cfg->dim < 1 || cfg->dim > kMaxDim || cfg->context_size < 2 || cfg->walk_length < cfg->context_size ||
      cfg->walk_length > 4096 || cfg->walks_per_node < 1 || cfg->num_negative_samples < 1) {
    set_last_error("node2vec: need 1 <= dim <= 16384, 2 <= context_size <= walk_length <= 4096, "
                   "walks_per_node >= 1, num_negative_samples >= 1");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (cfg->p != 1.0 || cfg->q != 1.0) {
    set_last_error("node2vec: only p = q = 1 (every reference config)");
    return S3GRL_ERR_NOT_IMPLEMENTED;
  }
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  // the CSR is checked on the host once: the walk kernel trusts it
  std::vector<int64_t> ip;
  std::vector<int32_t> ix;
  S3GRL_TRY(check_csr(ctx, num_nodes, indptr, indices, num_entries, /*ascending=*/false,
                      "node2vec: malformed CSR (indptr not monotone from 0 to nnz, or a column outside [0, N))", &ip,
                      &ix));
  std::vector<int32_t> ip32(ip.begin(), ip.end());
  auto* t = new s3grl_skipgram();
  t->ctx = ctx;
  t->N = num_nodes;
  t->D = cfg->dim;
  t->L = cfg->walk_length;
  t->C = cfg->context_size;
  t->R = cfg->walks_per_node;
  t->Q = cfg->num_negative_samples;
  t->seed = cfg->seed;
  t->vec = t->D % 4 == 0 ? 4 : 1;
  while (t->lpd < t->D / t->vec && t->lpd < 64) t->lpd <<= 1;
  const size_t table = (size_t)num_nodes * t->D;
  s3grl_status s = S3GRL_OK;
  auto fail = [&](s3grl_status st) {
    sg_free(t);
    delete t;
    return st;
  };
  if ((s = regrow(&t->indptr, ip32.size())) || (s = regrow(&t->indices, ix.size())) || (s = regrow(&t->emb, table)) ||
      (s = regrow(&t->m, table)) || (s = regrow(&t->v, table)) || (s = regrow(&t->grad, table)) ||
      (s = regrow(&t->first, (size_t)num_nodes)) || (s = regrow(&t->last, (size_t)num_nodes)) ||
      (s = regrow(&t->stamp, (size_t)num_nodes)) || (s = regrow(&t->perm, (size_t)num_nodes)))
    return fail(s);
  hipError_t e = hipMemcpyAsync(t->indptr, ip32.data(), ip32.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                ctx->stream);
  if (e == hipSuccess && num_entries)
    e = hipMemcpyAsync(t->indices, ix.data(), ix.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->m, 0, table * sizeof(float), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->v, 0, table * sizeof(float), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->stamp, 0xff, (size_t)num_nodes * sizeof(int64_t), ctx->stream);
  if (e == hipSuccess && init)
    e = hipMemcpyAsync(t->emb, init, table * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess && !init &&
      (s = launch_init_normal(ctx, key_of(t, 0, 0, kInit), (int64_t)table, t->emb)))
    return fail(s);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // the host vectors go out of scope
  if (e != hipSuccess) {
    set_last_error(std::string("node2vec create: ") + hipGetErrorString(e));
    return fail(e == hipErrorOutOfMemory ? S3GRL_ERR_OUT_OF_MEMORY : S3GRL_ERR_HIP);
  }
  *out = t;
  return S3GRL_OK;
}

s3grl_status s3grl_skipgram_epoch(s3grl_skipgram* t, int64_t epoch, int64_t batch_size, float lr, float* step_loss) {
  if (!t || epoch < 0 || batch_size < 1 || bad_lr(lr)) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  const int64_t W = windows_per_row(t);
  S3GRL_TRY(ensure_windows(t, W * std::min(batch_size, t->N) * t->R * (1 + t->Q)));
  S3GRL_TRY(ensure_perm(t, epoch));
  const int64_t steps = (t->N + batch_size - 1) / batch_size;
  for (int64_t s = 0; s < steps; ++s) {
    const int64_t npw = W * batch_of(t, s, batch_size) * t->R;
    S3GRL_TRY(launch_windows(t, epoch, s, batch_size, t->win, t->win + npw * t->C));
    S3GRL_TRY(run_step(t, npw, npw * t->Q, lr, step_loss ? step_loss + s : nullptr));
  }
  return S3GRL_OK;
}

s3grl_status s3grl_skipgram_step_windows(s3grl_skipgram* t, const int32_t* pos, int64_t num_pos, const int32_t* neg,
                                         int64_t num_neg, float lr, float* loss) {
  if (!t || !pos || !neg || num_pos < 1 || num_neg < 1 || num_pos + num_neg >= (int64_t(1) << 28) || bad_lr(lr))
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(ensure_windows(t, num_pos + num_neg));
  // a test and oracle hook: the caller's windows are gathered into t->win, positives first, and checked on the host
  // before any kernel reads them
  const int64_t np = num_pos * t->C, nn = num_neg * t->C;
  S3GRL_HIP_TRY(hipMemcpyAsync(t->win, pos, (size_t)np * sizeof(int32_t), hipMemcpyDeviceToDevice, t->ctx->stream));
  S3GRL_HIP_TRY(hipMemcpyAsync(t->win + np, neg, (size_t)nn * sizeof(int32_t), hipMemcpyDeviceToDevice,
                               t->ctx->stream));
  S3GRL_TRY(check_ids(t->ctx, t->win, np + nn, t->N, "node2vec step: a window node outside [0, N)"));
  return run_step(t, num_pos, num_neg, lr, loss);
}

s3grl_status s3grl_skipgram_export_windows(s3grl_skipgram* t, int64_t epoch, int64_t step, int64_t batch_size,
                                           int32_t* pos, int32_t* neg) {
  if (!t || !pos || !neg || epoch < 0 || batch_size < 1 || step < 0 || step * batch_size >= t->N)
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(ensure_perm(t, epoch));
  return launch_windows(t, epoch, step, batch_size, pos, neg);
}

s3grl_status s3grl_skipgram_state(const s3grl_skipgram* t, float* emb, float* exp_avg, float* exp_avg_sq,
                                  int64_t* steps) {
  if (!t) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  const size_t bytes = (size_t)t->N * t->D * sizeof(float);
  if (emb) S3GRL_HIP_TRY(hipMemcpyAsync(emb, t->emb, bytes, hipMemcpyDeviceToDevice, t->ctx->stream));
  if (exp_avg) S3GRL_HIP_TRY(hipMemcpyAsync(exp_avg, t->m, bytes, hipMemcpyDeviceToDevice, t->ctx->stream));
  if (exp_avg_sq) S3GRL_HIP_TRY(hipMemcpyAsync(exp_avg_sq, t->v, bytes, hipMemcpyDeviceToDevice, t->ctx->stream));
  if (steps) *steps = t->steps;
  return S3GRL_OK;
}

s3grl_status s3grl_skipgram_weight(const s3grl_skipgram* t, const float** emb) {
  if (!t || !emb) return S3GRL_ERR_INVALID_ARGUMENT;
  *emb = t->emb;
  return S3GRL_OK;
}

s3grl_status s3grl_skipgram_destroy(s3grl_skipgram* t) {
  if (!t) return S3GRL_OK;
  (void)hipSetDevice(t->ctx->device);
  (void)hipStreamSynchronize(t->ctx->stream);
  sg_free(t);
  delete t;
  return S3GRL_OK;
}

}  // extern "C"
