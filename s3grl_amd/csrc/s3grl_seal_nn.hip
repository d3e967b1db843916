// SortPooling, the pooling operator of the SEAL baselines' DGCNN (reference models.py:139-222), on a batch of labelled
// enclosing subgraphs, gfx950.  Deterministic: every output element is copied in a fixed order, two runs are
// bit-identical.  (GCN propagation, the model's other graph operator, is in s3grl_propagate.hip.)
//
// SortPooling (PyG global_sort_pool): per graph, nodes ordered by the last channel descending, ties by
// ascending position, ±0 equal; the first k rows of all D channels, zero rows past n.  One workgroup per graph
// bitonic-sorts 64-bit keys (order-preserving key bits, inverted, above the position) of a power-of-two
// length P >= n: in LDS when P keys fit the budget, else in the graph's own HBM slice [2·first, 2·first + P)
// of the caller's workspace (P <= 2n, so slices never overlap).  The forward saves the batch row of every
// output row (-1 for padding); the backward zero-fills and copies each output row's gradient back.
#include "s3grl_internal.hpp"
#include "s3grl_device.hpp"

#include <algorithm>

namespace s3grl {
namespace {

constexpr int kNnBlock = 256;
constexpr int kNnWaves = kNnBlock / 64;
constexpr int64_t kDefaultSortLdsBudget = 64 << 10;
constexpr int64_t kMaxSortLdsBudget = 159 << 10;   // 160 KiB per CU, less the static part

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
