// Graph autoencoders (PyG GAE / VGAE / ARGVA as reference baselines/vgae.py:run_vgae trains them) on gfx950: the
// pieces of a training step that are not dense linears or GCN propagation (s3grl_seal_nn.hip).
//
//   pair keys        key(i, j) = i·(N−1) + j − [j > i] over the N(N−1) ordered pairs i != j (PyG
//                    edge_index_to_vector); a graph's positive keys are sorted once
//   negatives        PyG negative_sampling(method='sparse'): T candidate draws — 3 rounds of S = int(1.1·count/prob)
//                    draws, or every key in key order when S >= N(N−1) (PyG's `sample` then returns arange) —
//                    are sorted by (key, draw); a draw survives when it is the earliest draw of its key and not a
//                    positive (binary search); the first `count` survivors in draw order are kept and written out
//                    in key order.  Equal to PyG's rounds: a later round only matters when the earlier ones fell
//                    short, and then its survivors follow theirs.
//   incidence        node-major lists of a pair list: (node, 2·pair + side) sorted by node, pairs ascending inside
//                    a node, and ptr [N + 1] by binary search
//   decode           one group of LPD lanes per pair, VEC channels per lane (float4 when D % 4 == 0): the logit
//                    z_u·z_v, and for a loss PyG recon_loss's per-pair dL/dlogit and fixed-order block partials
//   backward         one wavefront per node: grad_z[i] = Σ coef · z[other] over i's incidence entries (positives',
//                    then negatives'), 64 / LPD slices in entry order, the slices added by a fixed butterfly
//
// Determinism: no float atomics; every draw is a counter-based hash of (seed, epoch, round, index), a key derivation
// of its own over mix64 of s3grl_train.hpp; every sort has unique (key, value) pairs, so every order is fixed.  Two
// runs with one seed are bit-identical.  The two radix sorts are the (u64 key, i32 value) sort instantiated once, in s3grl_relabel.hip.
#include "s3grl_internal.hpp"
#include "s3grl_device.hpp"
#include "s3grl_train.hpp"

#include <algorithm>
#include <cmath>

namespace s3grl {
namespace {

constexpr int kGaeBlock = 256;
constexpr uint64_t kNoKey = ~0ull;

__device__ __forceinline__ uint64_t pair_key(int64_t i, int64_t j, int64_t n) {
  return (uint64_t)(i * (n - 1) + j - (j > i ? 1 : 0));
}

// ---- keys --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGaeBlock) void keys_kernel(int64_t P, int64_t n, const int32_t* __restrict__ src,
                                                        const int32_t* __restrict__ dst, uint64_t* __restrict__ keys,
                                                        int32_t* __restrict__ vals,
                                                        unsigned long long* __restrict__ bad) {
  const int64_t p = (int64_t)blockIdx.x * kGaeBlock + threadIdx.x;
  if (p >= P) return;
  const int64_t i = src[p], j = dst[p];
  if (i < 0 || i >= n || j < 0 || j >= n) {   // bad[0]: ids out of range, bad[1]: self-loops
    atomicAdd(bad, 1ull);
    keys[p] = kNoKey;
  } else if (i == j) {
    atomicAdd(bad + 1, 1ull);
    keys[p] = kNoKey;
  } else {
    keys[p] = pair_key(i, j, n);
  }
  vals[p] = (int32_t)p;
}

// ---- negatives ---------------------------------------------------------------------------------------------
// candidate t: enumerate mode, key t; else round t / S, draw t % S, mapped to [0, pop) by a 64 x 64 -> 128-bit
// multiply (bias below pop / 2^64)
__global__ __launch_bounds__(kGaeBlock) void cand_kernel(int64_t T, int64_t S, uint64_t pop, int enumerate,
                                                        uint64_t key, uint64_t* __restrict__ keys,
                                                        int32_t* __restrict__ vals) {
  const int64_t t = (int64_t)blockIdx.x * kGaeBlock + threadIdx.x;
  if (t >= T) return;
  uint64_t k;
  if (enumerate) {
    k = (uint64_t)t;
  } else {
    const uint64_t round = (uint64_t)(t / S), i = (uint64_t)(t - (int64_t)round * S);
    k = __umul64hi(mix64(key ^ mix64((round << 40) ^ i)), pop);
  }
  keys[t] = k;
  vals[t] = (int32_t)t;
}

__device__ __forceinline__ bool is_positive(const uint64_t* __restrict__ pos, int64_t M, uint64_t k) {
  int64_t lo = 0, hi = M;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (pos[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo < M && pos[lo] == k;
}

// flag[draw] = 1 when the sorted entry q is the earliest draw of its key and not a positive
__global__ __launch_bounds__(kGaeBlock) void survive_kernel(int64_t T, const uint64_t* __restrict__ keys,
                                                           const int32_t* __restrict__ vals,
                                                           const uint64_t* __restrict__ pos, int64_t M,
                                                           int32_t* __restrict__ flag) {
  const int64_t q = (int64_t)blockIdx.x * kGaeBlock + threadIdx.x;
  if (q >= T) return;
  const uint64_t k = keys[q];
  flag[vals[q]] = (q == 0 || keys[q - 1] != k) && !is_positive(pos, M, k) ? 1 : 0;
}

// keep[q] = the sorted entry q survives and is among the first `count` survivors in draw order
__global__ __launch_bounds__(kGaeBlock) void keep_kernel(int64_t T, const int32_t* __restrict__ vals,
                                                        const int32_t* __restrict__ flag,
                                                        const int64_t* __restrict__ rank, int64_t count,
                                                        int32_t* __restrict__ keep) {
  const int64_t q = (int64_t)blockIdx.x * kGaeBlock + threadIdx.x;
  if (q >= T) return;
  const int32_t d = vals[q];
  keep[q] = flag[d] && rank[d] < count ? 1 : 0;
}

__global__ __launch_bounds__(kGaeBlock) void compact_kernel(int64_t T, int64_t n, const uint64_t* __restrict__ keys,
                                                           const int32_t* __restrict__ keep,
                                                           const int64_t* __restrict__ at, int64_t cap,
                                                           int32_t* __restrict__ src, int32_t* __restrict__ dst) {
  const int64_t q = (int64_t)blockIdx.x * kGaeBlock + threadIdx.x;
  if (q >= T || !keep[q]) return;
  const int64_t o = at[q];
  if (o >= cap) return;
  const uint64_t k = keys[q];
  const int64_t i = (int64_t)(k / (uint64_t)(n - 1));
  int64_t j = (int64_t)(k - (uint64_t)i * (uint64_t)(n - 1));
  if (j >= i) ++j;
  src[o] = (int32_t)i;
  dst[o] = (int32_t)j;
}

// ---- incidence ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGaeBlock) void inc_keys_kernel(int64_t P, const int32_t* __restrict__ src,
                                                            const int32_t* __restrict__ dst,
                                                            uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int64_t e = (int64_t)blockIdx.x * kGaeBlock + threadIdx.x;
  if (e >= 2 * P) return;
  const int64_t p = e >> 1;
  keys[e] = (uint64_t)(uint32_t)((e & 1) ? dst[p] : src[p]);
  vals[e] = (int32_t)e;
}

__global__ __launch_bounds__(kGaeBlock) void inc_ptr_kernel(int64_t n, int64_t E, const uint64_t* __restrict__ keys,
                                                           int64_t* __restrict__ ptr) {
  const int64_t i = (int64_t)blockIdx.x * kGaeBlock + threadIdx.x;
  if (i > n) return;
  int64_t lo = 0, hi = E;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < (uint64_t)i) lo = mid + 1; else hi = mid;
  }
  ptr[i] = lo;
}

// ---- decode ------------------------------------------------------------------------------------------------
// pairs [0, Pa) of list a, [Pa, Pa + Pb) of list b.  With coef (a loss), PyG recon_loss in fp32, as autograd chains it:
//   a  -log(sigmoid(x) + EPS).mean()       coef = (-1/Pa) / (s + EPS) · (1 − s) · s
//   b  -log(1 − sigmoid(x) + EPS).mean()   coef = ( 1/Pb) / (1 − s + EPS) · (1 − s) · s
// partial[2·block], [2·block + 1]: the block's Σ of a and b terms
template <int VEC, int LPD>
__global__ __launch_bounds__(kGaeBlock) void decode_kernel(int D, const float* __restrict__ z, int64_t Pa,
                                                          const int32_t* __restrict__ sa, const int32_t* __restrict__ da,
                                                          int64_t Pb, const int32_t* __restrict__ sb,
                                                          const int32_t* __restrict__ db, float inv_a, float inv_b,
                                                          float* __restrict__ logits, float* __restrict__ coef,
                                                          double* __restrict__ partial) {
  typedef Vec<VEC> V;
  __shared__ double sh[kGaeBlock / 64];
  const int q = threadIdx.x % LPD;
  const int64_t p = (int64_t)blockIdx.x * (kGaeBlock / LPD) + threadIdx.x / LPD;
  double ta = 0.0, tb = 0.0;
  if (p < Pa + Pb) {
    const bool in_a = p < Pa;
    const int64_t u = in_a ? sa[p] : sb[p - Pa], v = in_a ? da[p] : db[p - Pa];
    float acc = 0.f;
    for (int c = q * VEC; c < D; c += LPD * VEC) acc += V::sum(V::load(z + u * D + c) * V::load(z + v * D + c));
    for (int o = LPD / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);   // the group's lanes, fixed butterfly
    if (q == 0) {
      logits[p] = acc;
      if (coef) {
        const float s = 1.f / (1.f + expf(-acc));
        if (in_a) {
          ta = -logf(s + 1e-15f);
          coef[p] = (-inv_a) / (s + 1e-15f) * (1.f - s) * s;
        } else {
          tb = -logf(1.f - s + 1e-15f);
          coef[p] = inv_b / (1.f - s + 1e-15f) * (1.f - s) * s;
        }
      }
    }
  }
  if (!partial) return;
  const double sa_ = block_sum_f64<kGaeBlock>(ta, sh);
  const double sb_ = block_sum_f64<kGaeBlock>(tb, sh);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = sa_;
    partial[2 * blockIdx.x + 1] = sb_;
  }
}

// one block: the partials in block order -> loss = mean(a terms) + mean(b terms)
__global__ __launch_bounds__(kGaeBlock) void loss_kernel(const double* __restrict__ partial, int64_t nparts,
                                                        double inv_a, double inv_b, float* __restrict__ loss) {
  __shared__ double sh[kGaeBlock / 64];
  double sa = 0.0, sb = 0.0;
  for (int64_t j = threadIdx.x; j < nparts; j += kGaeBlock) {
    sa += partial[2 * j];
    sb += partial[2 * j + 1];
  }
  sa = block_sum_f64<kGaeBlock>(sa, sh);
  sb = block_sum_f64<kGaeBlock>(sb, sh);
  if (threadIdx.x == 0) loss[0] = (float)(sa * inv_a) + (float)(sb * inv_b);
}

// ---- backward ----------------------------------------------------------------------------------------------
struct IncList {
  const int64_t* ptr;     // [N + 1]
  const int32_t* slot;    // 2·pair + side; side 0: the node is the pair's source, so the other end is its target
  const int32_t *src, *dst;
  const float* coef;
};

__device__ __forceinline__ int64_t other_end(const IncList& l, int32_t s, float* c) {
  const int64_t p = s >> 1;
  *c = l.coef[p];
  return (s & 1) ? l.src[p] : l.dst[p];
}

// one wavefront per node u: S = 64 / LPD slices; slice s sums entries s, s + S, ... of u's list a entries followed
// by its list b entries, then the slices are added by a fixed butterfly.  grad[u] = scale · Σ coef · z[other].
template <int VEC, int LPD>
__global__ __launch_bounds__(kGaeBlock) void backward_kernel(int64_t N, int D, const float* __restrict__ z,
                                                            IncList a, IncList b, int has_b,
                                                            const float* __restrict__ scale, float* __restrict__ grad) {
  typedef Vec<VEC> V;
  typedef typename V::T T;
  constexpr int S = 64 / LPD;
  const int64_t u = (int64_t)blockIdx.x * (kGaeBlock / 64) + (threadIdx.x >> 6);
  if (u >= N) return;
  const int lane = threadIdx.x & 63, q = lane % LPD, sl = lane / LPD;
  const int64_t a0 = a.ptr[u], na = a.ptr[u + 1] - a0;
  const int64_t b0 = has_b ? b.ptr[u] : 0, nb = has_b ? b.ptr[u + 1] - b0 : 0;
  const float sc = scale ? scale[0] : 1.f;
  for (int c = q * VEC; c < D; c += LPD * VEC) {
    T acc = (T)(0.f);
    for (int64_t j = sl; j < na + nb; j += S) {
      float cf;
      const int64_t o = j < na ? other_end(a, a.slot[a0 + j], &cf) : other_end(b, b.slot[b0 + j - na], &cf);
      acc += (cf * sc) * V::load(z + o * D + c);
    }
#pragma unroll
    for (int o = S / 2; o > 0; o >>= 1) {   // slice s + o into slice s, the same tree in every lane
#pragma unroll
      for (int i = 0; i < VEC; ++i) V::set(acc, i, V::at(acc, i) + __shfl_xor(V::at(acc, i), o * LPD, 64));
    }
    if (sl == 0) V::store(grad + u * D + c, acc);
  }
}

// ---- host helpers ------------------------------------------------------------------------------------------
template <typename T>
s3grl_status take(s3grl_context* ctx, Transient& tr, size_t count, T** out) {
  void* p = nullptr;
  S3GRL_TRY(ctx->arena.alloc(std::max<size_t>(count, 1) * sizeof(T), &p));
  tr.ptrs.push_back(p);
  *out = static_cast<T*>(p);
  return S3GRL_OK;
}

// (u64 key, i32 value) pairs sorted by key, stable: keys_out / vals_out
s3grl_status sort_pairs(s3grl_context* ctx, Transient& tr, uint64_t* keys_in, uint64_t* keys_out, int32_t* vals_in,
                        int32_t* vals_out, size_t n) {
  size_t bytes = 0;
  S3GRL_TRY(sort_pairs_u64_i32_bytes(ctx, n, &bytes));
  char* tmp = nullptr;
  S3GRL_TRY(take(ctx, tr, bytes, &tmp));
  return sort_pairs_u64_i32(ctx, tmp, bytes, keys_in, keys_out, vals_in, vals_out, n);
}

int lanes_for(int D, int vec) {
  int lpd = 1;
  while (lpd < D / vec && lpd < 64) lpd <<= 1;
  return lpd;
}

template <int VEC, int LPD>
s3grl_status launch_decode(s3grl_context* ctx, int D, const float* z, int64_t Pa, const int32_t* sa, const int32_t* da,
                           int64_t Pb, const int32_t* sb, const int32_t* db, float* logits, float* coef, float* loss,
                           double* partial) {
  const unsigned blocks = grid_of(Pa + Pb, kGaeBlock / LPD);
  const double ia = Pa ? 1.0 / (double)Pa : 0.0, ib = Pb ? 1.0 / (double)Pb : 0.0;
  hipLaunchKernelGGL((decode_kernel<VEC, LPD>), dim3(blocks), dim3(kGaeBlock), 0, ctx->stream, D, z, Pa, sa, da, Pb,
                     sb, db, (float)ia, (float)ib, logits, coef, loss ? partial : nullptr);
  S3GRL_HIP_TRY(hipGetLastError());
  if (loss) {
    // PyG: the mean of an empty list is NaN; 0 · NaN stays NaN
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(kGaeBlock), 0, ctx->stream, partial, (int64_t)blocks,
                       Pa ? ia : NAN, Pb ? ib : NAN, loss);
    S3GRL_HIP_TRY(hipGetLastError());
  }
  return S3GRL_OK;
}

template <int VEC, int LPD>
s3grl_status launch_backward(s3grl_context* ctx, int64_t N, int D, const float* z, const IncList& a, const IncList& b,
                             int has_b, const float* scale, float* grad) {
  hipLaunchKernelGGL((backward_kernel<VEC, LPD>), dim3(grid_of(N, kGaeBlock / 64)), dim3(kGaeBlock), 0, ctx->stream,
                     N, D, z, a, b, has_b, scale, grad);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

// F(VEC, LPD) for the lane layout of D
#define S3GRL_GAE_DISPATCH(D, F)                                        \
  do {                                                                  \
    const int vec_ = (D) % 4 == 0 ? 4 : 1;                              \
    const int lpd_ = lanes_for((D), vec_);                              \
    if (vec_ == 4) {                                                    \
      switch (lpd_) {                                                   \
        case 1: return F(4, 1);                                         \
        case 2: return F(4, 2);                                         \
        case 4: return F(4, 4);                                         \
        case 8: return F(4, 8);                                         \
        case 16: return F(4, 16);                                       \
        case 32: return F(4, 32);                                       \
        default: return F(4, 64);                                       \
      }                                                                 \
    }                                                                   \
    switch (lpd_) {                                                     \
      case 1: return F(1, 1);                                           \
      case 2: return F(1, 2);                                           \
      case 4: return F(1, 4);                                           \
      case 8: return F(1, 8);                                           \
      case 16: return F(1, 16);                                         \
      case 32: return F(1, 32);                                         \
      default: return F(1, 64);                                         \
    }                                                                   \
  } while (0)

constexpr int64_t kMaxNodes = int64_t(1) << 31;
constexpr int64_t kMaxPairs = int64_t(1) << 30;   // 2·pairs incidence entries and draw indices are int32
constexpr int kMaxDim = 1 << 16;

}  // namespace
}  // namespace s3grl

using namespace s3grl;

extern "C" {

s3grl_status s3grl_gae_keys(s3grl_context* ctx, int64_t num_nodes, const int32_t* src, const int32_t* dst,
                            int64_t num_pairs, uint64_t* keys, int64_t* num_keys) {
  if (!ctx || !num_keys || num_nodes < 1 || num_nodes >= kMaxNodes || num_pairs < 0 || num_pairs > kMaxPairs ||
      (num_pairs > 0 && (!src || !dst || !keys)))
    return S3GRL_ERR_INVALID_ARGUMENT;
  *num_keys = 0;
  if (num_pairs == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  Transient tr{ctx, {}};
  uint64_t* k0;
  int32_t *v0, *v1;
  unsigned long long* bad;
  S3GRL_TRY(take(ctx, tr, (size_t)num_pairs, &k0));
  S3GRL_TRY(take(ctx, tr, (size_t)num_pairs, &v0));
  S3GRL_TRY(take(ctx, tr, (size_t)num_pairs, &v1));
  S3GRL_TRY(take(ctx, tr, 2, &bad));
  S3GRL_HIP_TRY(hipMemsetAsync(bad, 0, 2 * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(keys_kernel, dim3(grid_of(num_pairs, kGaeBlock)), dim3(kGaeBlock), 0, ctx->stream, num_pairs,
                     num_nodes, src, dst, k0, v0, bad);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(sort_pairs(ctx, tr, k0, keys, v0, v1, (size_t)num_pairs));
  unsigned long long h[2];
  S3GRL_HIP_TRY(hipMemcpyAsync(h, bad, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));   // the count comes back
  if (h[0]) {
    set_last_error("gae keys: a node id outside [0, N)");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  *num_keys = num_pairs - (int64_t)h[1];
  return S3GRL_OK;
}

s3grl_status s3grl_gae_negatives(s3grl_context* ctx, int64_t num_nodes, const uint64_t* pos_keys, int64_t num_keys,
                                 int64_t count, uint32_t seed, int64_t epoch, int32_t* src, int32_t* dst,
                                 int64_t* num_out) {
  if (!ctx || !num_out || num_nodes < 1 || num_nodes >= kMaxNodes || num_keys < 0 || (num_keys > 0 && !pos_keys) ||
      count < 0 || count > kMaxPairs || epoch < 0 || (count > 0 && (!src || !dst)))
    return S3GRL_ERR_INVALID_ARGUMENT;
  *num_out = 0;
  const uint64_t pop = (uint64_t)num_nodes * (uint64_t)(num_nodes - 1);
  if ((uint64_t)num_keys >= pop || count == 0) return S3GRL_OK;   // PyG: no room for a negative
  // PyG: prob = 1 - idx.numel() / population; sample_size = int(1.1 * num_neg_samples / prob)
  const double prob = 1.0 - (double)num_keys / (double)pop;
  const double s_real = 1.1 * (double)count / prob;
  const bool enumerate = s_real >= (double)pop;
  const int64_t S = enumerate ? (int64_t)pop : (int64_t)s_real;
  const int64_t T = enumerate ? S : 3 * S;
  if (S < 1 || T >= (int64_t(1) << 31)) {
    set_last_error("gae negatives: more than 2^31 candidate draws");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  Transient tr{ctx, {}};
  uint64_t *k0, *k1;
  int32_t *v0, *v1, *flag, *keep;
  int64_t *rank, *at, *ws;
  const int64_t wsn = scan_workspace_elems(T);
  S3GRL_TRY(take(ctx, tr, (size_t)T, &k0));
  S3GRL_TRY(take(ctx, tr, (size_t)T, &k1));
  S3GRL_TRY(take(ctx, tr, (size_t)T, &v0));
  S3GRL_TRY(take(ctx, tr, (size_t)T, &v1));
  S3GRL_TRY(take(ctx, tr, (size_t)T, &flag));
  S3GRL_TRY(take(ctx, tr, (size_t)T, &keep));
  S3GRL_TRY(take(ctx, tr, (size_t)T + 1, &rank));
  S3GRL_TRY(take(ctx, tr, (size_t)T + 1, &at));
  S3GRL_TRY(take(ctx, tr, (size_t)wsn, &ws));
  const uint64_t key = mix64(mix64(mix64(seed) ^ (uint64_t)epoch) ^ 0x6761655f6e6567ull);   // "gae_neg"
  const unsigned g = grid_of(T, kGaeBlock);
  hipLaunchKernelGGL(cand_kernel, dim3(g), dim3(kGaeBlock), 0, ctx->stream, T, S, pop, (int)enumerate, key, k0, v0);
  S3GRL_HIP_TRY(hipGetLastError());
  if (enumerate) {   // already in key order
    k1 = k0;
    v1 = v0;
  } else {
    S3GRL_TRY(sort_pairs(ctx, tr, k0, k1, v0, v1, (size_t)T));
  }
  hipLaunchKernelGGL(survive_kernel, dim3(g), dim3(kGaeBlock), 0, ctx->stream, T, k1, v1, pos_keys, num_keys, flag);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(launch_scan_i32_to_i64(ctx, flag, T, rank, ws));
  hipLaunchKernelGGL(keep_kernel, dim3(g), dim3(kGaeBlock), 0, ctx->stream, T, v1, flag, rank, count, keep);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(launch_scan_i32_to_i64(ctx, keep, T, at, ws));
  hipLaunchKernelGGL(compact_kernel, dim3(g), dim3(kGaeBlock), 0, ctx->stream, T, num_nodes, k1, keep, at, count, src,
                     dst);
  S3GRL_HIP_TRY(hipGetLastError());
  int64_t k = 0;
  S3GRL_HIP_TRY(hipMemcpyAsync(&k, at + T, sizeof(k), hipMemcpyDeviceToHost, ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));   // the count comes back
  *num_out = std::min(k, count);
  return S3GRL_OK;
}

s3grl_status s3grl_gae_incidence(s3grl_context* ctx, int64_t num_nodes, const int32_t* src, const int32_t* dst,
                                 int64_t num_pairs, int64_t* ptr, int32_t* slot) {
  if (!ctx || !ptr || num_nodes < 1 || num_nodes >= kMaxNodes || num_pairs < 0 || num_pairs > kMaxPairs ||
      (num_pairs > 0 && (!src || !dst || !slot)))
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  if (num_pairs == 0) {
    S3GRL_HIP_TRY(hipMemsetAsync(ptr, 0, (size_t)(num_nodes + 1) * sizeof(int64_t), ctx->stream));
    return S3GRL_OK;
  }
  const int64_t E = 2 * num_pairs;
  Transient tr{ctx, {}};
  uint64_t *k0, *k1;
  int32_t* v0;
  S3GRL_TRY(take(ctx, tr, (size_t)E, &k0));
  S3GRL_TRY(take(ctx, tr, (size_t)E, &k1));
  S3GRL_TRY(take(ctx, tr, (size_t)E, &v0));
  hipLaunchKernelGGL(inc_keys_kernel, dim3(grid_of(E, kGaeBlock)), dim3(kGaeBlock), 0, ctx->stream, num_pairs, src,
                     dst, k0, v0);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(sort_pairs(ctx, tr, k0, k1, v0, slot, (size_t)E));
  hipLaunchKernelGGL(inc_ptr_kernel, dim3(grid_of(num_nodes + 1, kGaeBlock)), dim3(kGaeBlock), 0, ctx->stream,
                     num_nodes, E, k1, ptr);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_gae_decode(s3grl_context* ctx, int64_t dim, const float* z, const int32_t* pos_src,
                              const int32_t* pos_dst, int64_t num_pos, const int32_t* neg_src, const int32_t* neg_dst,
                              int64_t num_neg, float* logits, float* coef, float* loss) {
  if (!ctx || !z || !logits || dim < 1 || dim > kMaxDim || num_pos < 0 || num_neg < 0 ||
      num_pos + num_neg > kMaxPairs || (num_pos > 0 && (!pos_src || !pos_dst)) ||
      (num_neg > 0 && (!neg_src || !neg_dst)) || (!coef) != (!loss))
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  if (num_pos + num_neg == 0) {
    if (loss) {
      const float nan = NAN;
      S3GRL_HIP_TRY(hipMemcpyAsync(loss, &nan, sizeof(float), hipMemcpyHostToDevice, ctx->stream));
      S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return S3GRL_OK;
  }
  Transient tr{ctx, {}};
  double* partial = nullptr;
  if (loss) S3GRL_TRY(take(ctx, tr, (size_t)2 * grid_of(num_pos + num_neg, kGaeBlock / 64), &partial));   // LPD <= 64
  const int D = (int)dim;
#define S3GRL_GAE_DECODE(V, L) \
  launch_decode<V, L>(ctx, D, z, num_pos, pos_src, pos_dst, num_neg, neg_src, neg_dst, logits, coef, loss, partial)
  S3GRL_GAE_DISPATCH(D, S3GRL_GAE_DECODE);
#undef S3GRL_GAE_DECODE
}

s3grl_status s3grl_gae_backward(s3grl_context* ctx, int64_t num_nodes, int64_t dim, const float* z, const float* scale,
                                const int64_t* pos_ptr, const int32_t* pos_slot, const int32_t* pos_src,
                                const int32_t* pos_dst, const float* pos_coef, const int64_t* neg_ptr,
                                const int32_t* neg_slot, const int32_t* neg_src, const int32_t* neg_dst,
                                const float* neg_coef, float* grad_z) {
  if (!ctx || !z || !grad_z || !pos_ptr || !pos_slot || !pos_src || !pos_dst || !pos_coef || num_nodes < 1 ||
      num_nodes >= kMaxNodes || dim < 1 || dim > kMaxDim)
    return S3GRL_ERR_INVALID_ARGUMENT;
  const int has_b = neg_ptr != nullptr;
  if (has_b && (!neg_slot || !neg_src || !neg_dst || !neg_coef)) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const IncList a{pos_ptr, pos_slot, pos_src, pos_dst, pos_coef};
  const IncList b = has_b ? IncList{neg_ptr, neg_slot, neg_src, neg_dst, neg_coef} : a;
  const int D = (int)dim;
#define S3GRL_GAE_BACKWARD(V, L) launch_backward<V, L>(ctx, num_nodes, D, z, a, b, has_b, scale, grad_z)
  S3GRL_GAE_DISPATCH(D, S3GRL_GAE_BACKWARD);
#undef S3GRL_GAE_BACKWARD
}

}  // extern "C"
