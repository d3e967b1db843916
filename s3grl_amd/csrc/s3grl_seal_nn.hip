// The two graph operators of the SEAL baselines' models (reference models.py:12-76 GCN, :139-222 DGCNN), on a
// batch of labelled enclosing subgraphs, gfx950.  Both are deterministic: no float atomics, every output
// element is summed or copied in a fixed order, two runs are bit-identical.
//
// GCN propagation (PyG GCNConv message passing after its linear, with gcn_norm and add_remaining_self_loops):
//   out[i] = Σ_{j -> i, self-loop included} coef_ji · h[j]  (+ bias),   coef_ji = dinv[j] · w_ji · dinv[i]
// The operator's structure is a property of the split, not of the batch: the caller builds once per split a
// CSR over the split's nodes (ptr / nbr / coef, nbr a link-local id) grouped by destination for the forward and
// by source for the backward (the transposed operator), and dinv with gcn_norm_kernel.  A batch is a set of
// whole links laid out back to back; `rows` names the split node of every batch row, `loc` that node's local id
// in its link, so the batch row of neighbour nbr is  r - loc[rows[r]] + nbr.  One group of LPN lanes per
// node, VEC channels per lane (float4 when H % 4 == 0): H = 256 is a wavefront per node, H = 32 eight nodes per
// wavefront, H = 1 one node per lane.  The neighbours of a node are walked in CSR order.
//
// SortPooling (PyG global_sort_pool): per graph, nodes ordered by the last channel descending, ties by
// ascending position, ±0 equal; the first k rows of all D channels, zero rows past n.  One workgroup per graph
// bitonic-sorts 64-bit keys (order-preserving key bits, inverted, above the position) of a power-of-two
// length P >= n: in LDS when P keys fit the budget, else in the graph's own HBM slice [2·first, 2·first + P)
// of the caller's workspace (P <= 2n, so slices never overlap).  The forward saves the batch row of every
// output row (-1 for padding); the backward zero-fills and copies each output row's gradient back.
#include "s3grl_internal.hpp"

#include <algorithm>

namespace s3grl {
namespace {

typedef float float4_t __attribute__((ext_vector_type(4)));

constexpr int kNnBlock = 256;
constexpr int kNnWaves = kNnBlock / 64;
constexpr int64_t kDefaultSortLdsBudget = 64 << 10;
constexpr int64_t kMaxSortLdsBudget = 159 << 10;   // 160 KiB per CU, less the static part

// deg[i] = Σ in-weights of i (loop included) in CSR order; dinv = deg^-1/2, 0 where deg == 0 (PyG: inf -> 0)
__global__ __launch_bounds__(kNnBlock) void gcn_norm_kernel(int64_t n, const int64_t* __restrict__ ptr,
                                                           const float* __restrict__ w, float* __restrict__ dinv) {
  const int64_t i = (int64_t)blockIdx.x * kNnBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t a = ptr[i], b = ptr[i + 1];
  float deg = 0.f;
  if (w) {
    for (int64_t e = a; e < b; ++e) deg += w[e];
  } else {
    deg = (float)(b - a);
  }
  const float d = 1.0f / sqrtf(deg);
  dinv[i] = isinf(d) ? 0.f : d;
}

template <int VEC>
struct Vec;
template <>
struct Vec<4> {
  typedef float4_t T;
  static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const float4_t*>(p); }
  static __device__ __forceinline__ void store(float* p, T v) { *reinterpret_cast<float4_t*>(p) = v; }
};
template <>
struct Vec<1> {
  typedef float T;
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
};

// LPN lanes per node (a power of two dividing 64), VEC channels per lane
template <int VEC, int LPN>
__global__ __launch_bounds__(kNnBlock) void gcn_prop_kernel(int64_t n_rows, int H, const int64_t* __restrict__ rows,
                                                           const int32_t* __restrict__ loc,
                                                           const int64_t* __restrict__ ptr,
                                                           const int32_t* __restrict__ nbr,
                                                           const float* __restrict__ coef,
                                                           const float* __restrict__ h,
                                                           const float* __restrict__ bias, float* __restrict__ out) {
  typedef Vec<VEC> V;
  typedef typename V::T T;
  constexpr int kNodesPerWave = 64 / LPN;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPN;
  const int64_t r = ((int64_t)blockIdx.x * kNnWaves + (threadIdx.x >> 6)) * kNodesPerWave + lane / LPN;
  if (r >= n_rows) return;
  const int64_t g = rows[r];
  const int64_t base = r - loc[g];
  const int64_t e0 = ptr[g], e1 = ptr[g + 1];
  for (int c = q * VEC; c < H; c += LPN * VEC) {
    const float* __restrict__ hc = h + c;
    T acc = (T)(0.f);
    int64_t e = e0;
    for (; e + 4 <= e1; e += 4) {   // four loads in flight, summed in CSR order
      const float w0 = coef[e], w1 = coef[e + 1], w2 = coef[e + 2], w3 = coef[e + 3];
      const T v0 = V::load(hc + (base + nbr[e]) * H);
      const T v1 = V::load(hc + (base + nbr[e + 1]) * H);
      const T v2 = V::load(hc + (base + nbr[e + 2]) * H);
      const T v3 = V::load(hc + (base + nbr[e + 3]) * H);
      acc += w0 * v0;
      acc += w1 * v1;
      acc += w2 * v2;
      acc += w3 * v3;
    }
    for (; e < e1; ++e) acc += coef[e] * V::load(hc + (base + nbr[e]) * H);
    if (bias) acc += V::load(bias + c);
    V::store(out + r * H + c, acc);
  }
}

template <int VEC>
s3grl_status launch_prop(hipStream_t st, int64_t n_rows, int H, const int64_t* rows, const int32_t* loc,
                         const int64_t* ptr, const int32_t* nbr, const float* coef, const float* h,
                         const float* bias, float* out) {
  const int cols = H / VEC;
  int lpn = 1;
  while (lpn < cols && lpn < 64) lpn <<= 1;
  const int64_t per_block = (int64_t)kNnWaves * (64 / lpn);
  const dim3 grid((unsigned)((n_rows + per_block - 1) / per_block)), block(kNnBlock);
#define PROP_CASE(L)                                                                                       \
  case L:                                                                                                   \
    hipLaunchKernelGGL((gcn_prop_kernel<VEC, L>), grid, block, 0, st, n_rows, H, rows, loc, ptr, nbr, coef, \
                       h, bias, out);                                                                       \
    break;
  switch (lpn) {
    PROP_CASE(1)
    PROP_CASE(2)
    PROP_CASE(4)
    PROP_CASE(8)
    PROP_CASE(16)
    PROP_CASE(32)
    PROP_CASE(64)
  }
#undef PROP_CASE
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

// order-preserving key: ascending uint64 = last channel descending (±0 equal), then position ascending
__device__ __forceinline__ uint64_t sort_key(float v, int64_t pos) {
  uint32_t u = __float_as_uint(v);
  if ((u << 1) == 0) u = 0;
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)(~asc) << 32) | (uint32_t)pos;
}

__global__ __launch_bounds__(kNnBlock) void sortpool_fwd_kernel(const float* __restrict__ x,
                                                               const int64_t* __restrict__ node_ptr, int D, int k,
                                                               int64_t lds_keys, uint64_t* __restrict__ ws,
                                                               float* __restrict__ out,
                                                               int32_t* __restrict__ index) {
  extern __shared__ uint64_t s_keys[];
  const int64_t b = blockIdx.x;
  const int64_t r0 = node_ptr[b];
  int64_t n = node_ptr[b + 1] - r0;
  int64_t P = 1;
  while (P < n) P <<= 1;
  uint64_t* keys = P <= lds_keys ? s_keys : (ws ? ws + 2 * r0 : nullptr);
  if (!keys) n = 0;   // larger than the caller's max_nodes promised: zero rows, index -1
  if (n > 0) {
    for (int64_t i = threadIdx.x; i < P; i += kNnBlock)
      keys[i] = i < n ? sort_key(x[(r0 + i) * D + D - 1], i) : ~(uint64_t)0;
    __syncthreads();
    for (int64_t size = 2; size <= P; size <<= 1) {
      for (int64_t stride = size >> 1; stride > 0; stride >>= 1) {
        for (int64_t t = threadIdx.x; t < (P >> 1); t += kNnBlock) {
          const int64_t i = 2 * stride * (t / stride) + (t % stride), j = i + stride;
          const uint64_t a = keys[i], c = keys[j];
          if ((a > c) == ((i & size) == 0)) {
            keys[i] = c;
            keys[j] = a;
          }
        }
        __syncthreads();
      }
    }
  }
  const int lane = threadIdx.x & 63;
  for (int j = threadIdx.x >> 6; j < k; j += kNnWaves) {
    const int64_t pos = j < n ? (int64_t)(uint32_t)(keys[j] & 0xffffffffu) : -1;
    float* __restrict__ o = out + (b * k + j) * (int64_t)D;
    if (lane == 0) index[b * k + j] = pos >= 0 ? (int32_t)(r0 + pos) : -1;
    if (pos < 0) {
      for (int c = lane; c < D; c += 64) o[c] = 0.f;
    } else if ((D & 3) == 0) {
      const float* __restrict__ s = x + (r0 + pos) * D;
      for (int c = lane * 4; c < D; c += 256)
        *reinterpret_cast<float4_t*>(o + c) = *reinterpret_cast<const float4_t*>(s + c);
    } else {   // rows not 16-byte aligned: dword copy
      const float* __restrict__ s = x + (r0 + pos) * D;
      for (int c = lane; c < D; c += 64) o[c] = s[c];
    }
  }
}

// one wavefront per output row: grad_x[index[b, j]] = grad_out[b, j]; the rest was zero-filled
__global__ __launch_bounds__(kNnBlock) void sortpool_bwd_kernel(int64_t rows, int D,
                                                               const int32_t* __restrict__ index,
                                                               const float* __restrict__ gout,
                                                               float* __restrict__ gx) {
  const int64_t o = (int64_t)blockIdx.x * kNnWaves + (threadIdx.x >> 6);
  if (o >= rows) return;
  const int32_t r = index[o];
  if (r < 0) return;
  const int lane = threadIdx.x & 63;
  const float* __restrict__ s = gout + o * D;
  float* __restrict__ d = gx + (int64_t)r * D;
  if ((D & 3) == 0) {
    for (int c = lane * 4; c < D; c += 256)
      *reinterpret_cast<float4_t*>(d + c) = *reinterpret_cast<const float4_t*>(s + c);
  } else {
    for (int c = lane; c < D; c += 64) d[c] = s[c];
  }
}

int64_t sort_lds_keys(int64_t lds_budget) {
  const int64_t budget = lds_budget > 0 ? std::min(lds_budget, kMaxSortLdsBudget) : kDefaultSortLdsBudget;
  int64_t keys = 1;
  while (keys * 2 * 8 <= budget) keys <<= 1;
  return keys * 8 <= budget ? keys : 0;
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

extern "C" {

s3grl_status s3grl_gcn_norm(s3grl_context* ctx, int64_t num_nodes, const int64_t* ptr, const float* weight,
                            float* dinv) {
  if (!ctx || num_nodes < 0 || (num_nodes > 0 && (!ptr || !dinv))) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_nodes == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(gcn_norm_kernel, dim3((unsigned)((num_nodes + kNnBlock - 1) / kNnBlock)), dim3(kNnBlock), 0,
                     ctx->stream, num_nodes, ptr, weight, dinv);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_gcn_propagate(s3grl_context* ctx, int64_t num_rows, int64_t hidden, const int64_t* rows,
                                 const int32_t* loc, const int64_t* ptr, const int32_t* nbr, const float* coef,
                                 const float* h, const float* bias, float* out) {
  if (!ctx || num_rows < 0 || hidden <= 0 || hidden > (1 << 20)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_rows > 0 && (!rows || !loc || !ptr || !nbr || !coef || !h || !out)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_rows == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  if (hidden % 4 == 0)
    return launch_prop<4>(ctx->stream, num_rows, (int)hidden, rows, loc, ptr, nbr, coef, h, bias, out);
  return launch_prop<1>(ctx->stream, num_rows, (int)hidden, rows, loc, ptr, nbr, coef, h, bias, out);
}

s3grl_status s3grl_sort_pool_forward(s3grl_context* ctx, const float* x, const int64_t* node_ptr,
                                     int64_t num_graphs, int64_t width, int64_t k, int64_t max_nodes,
                                     int64_t lds_budget, uint64_t* workspace, float* out, int32_t* index) {
  if (!ctx || num_graphs < 0 || width <= 0 || width > (1 << 20) || k < 1 || k > (1 << 24) || max_nodes < 0 ||
      max_nodes >= (int64_t(1) << 31) || lds_budget < 0)
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_graphs > 0 && (!x || !node_ptr || !out || !index)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_graphs == 0) return S3GRL_OK;
  const int64_t lds_keys = sort_lds_keys(lds_budget);
  int64_t p_max = 1;
  while (p_max < max_nodes) p_max <<= 1;
  if (p_max > lds_keys && !workspace) {
    set_last_error("sort pool: a graph of max_nodes does not fit the LDS budget and no workspace was given");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  const int64_t dyn_keys = std::min(p_max, lds_keys);
  const unsigned dyn = (unsigned)(std::max<int64_t>(dyn_keys, 1) * 8);
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  if (dyn > (48u << 10))
    S3GRL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(sortpool_fwd_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  hipLaunchKernelGGL(sortpool_fwd_kernel, dim3((unsigned)num_graphs), dim3(kNnBlock), dyn, ctx->stream, x, node_ptr,
                     (int)width, (int)k, dyn_keys, workspace, out, index);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_sort_pool_backward(s3grl_context* ctx, int64_t num_graphs, int64_t width, int64_t k,
                                      const int32_t* index, const float* grad_out, int64_t num_rows,
                                      float* grad_x) {
  if (!ctx || num_graphs < 0 || width <= 0 || width > (1 << 20) || k < 1 || num_rows < 0)
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_rows > 0 && !grad_x) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_graphs > 0 && (!index || !grad_out)) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  if (num_rows > 0)
    S3GRL_HIP_TRY(hipMemsetAsync(grad_x, 0, (size_t)(num_rows * width) * sizeof(float), ctx->stream));
  const int64_t out_rows = num_graphs * k;
  if (out_rows == 0) return S3GRL_OK;
  hipLaunchKernelGGL(sortpool_bwd_kernel, dim3((unsigned)((out_rows + kNnWaves - 1) / kNnWaves)), dim3(kNnBlock), 0,
                     ctx->stream, out_rows, (int)width, index, grad_out, grad_x);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

}  // extern "C"
