// The kernels every trainer launches alike on the draw generator of s3grl_train.hpp: the epoch's permutation and the
// initial values, one thread per element.  An element's value depends on (key, index) alone, not on the launch shape.
#include "s3grl_internal.hpp"
#include "s3grl_train.hpp"

namespace s3grl {
namespace {

constexpr int kTrainBlock = 256;

// the epoch's permutation of range(n): sort (hash(i) << 32 | i), keep the low half
__global__ __launch_bounds__(kTrainBlock) void epoch_perm_keys_kernel(int64_t n, uint64_t key,
                                                                      uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kTrainBlock + threadIdx.x;
  if (i < n) out[i] = ((uint64_t)draw(key, 0, (uint64_t)i) << 32) | (uint64_t)i;
}
__global__ __launch_bounds__(kTrainBlock) void epoch_perm_take_kernel(int64_t n, const uint64_t* __restrict__ sorted,
                                                                      int32_t* __restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * kTrainBlock + threadIdx.x;
  if (i < n) perm[i] = (int32_t)(sorted[i] & 0xffffffffu);
}

__global__ __launch_bounds__(kTrainBlock) void init_normal_kernel(int64_t n, uint64_t key,
                                                                  float* __restrict__ out) {   // N(0, 1), Box-Muller
  const int64_t e = (int64_t)blockIdx.x * kTrainBlock + threadIdx.x;
  if (e >= n) return;
  const float u1 = ((float)draw(key, (uint64_t)e >> 32, 2 * (uint32_t)e) + 0.5f) * 2.3283064365386963e-10f;
  const float u2 = (float)draw(key, (uint64_t)e >> 32, 2 * (uint32_t)e + 1) * 2.3283064365386963e-10f;
  out[e] = sqrtf(-2.f * logf(u1)) * cosf(6.2831853071795865f * u2);
}
__global__ __launch_bounds__(kTrainBlock) void init_uniform_kernel(int64_t n, uint64_t key, float bound,
                                                                   float* __restrict__ out) {   // U(-b, b)
  const int64_t e = (int64_t)blockIdx.x * kTrainBlock + threadIdx.x;
  if (e >= n) return;
  const float u = ((float)(draw(key, 0, (uint64_t)e) >> 8) + 0.5f) * 5.9604644775390625e-8f;   // (0, 1), 24 bits
  out[e] = (2.f * u - 1.f) * bound;
}
__global__ __launch_bounds__(kTrainBlock) void fill_kernel(int64_t n, float value, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kTrainBlock + threadIdx.x;
  if (e < n) out[e] = value;
}

}  // namespace

s3grl_status launch_epoch_perm(s3grl_context* ctx, uint64_t key, int64_t n, uint64_t* keys_a, uint64_t* keys_b,
                               SortScratch& scratch, int32_t* perm) {
  const dim3 grid(grid_of(n, kTrainBlock)), block(kTrainBlock);
  hipLaunchKernelGGL(epoch_perm_keys_kernel, grid, block, 0, ctx->stream, n, key, keys_a);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(sort_keys_u64(ctx, scratch, keys_a, keys_b, (size_t)n, 64));
  hipLaunchKernelGGL(epoch_perm_take_kernel, grid, block, 0, ctx->stream, n, keys_b, perm);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_init_normal(s3grl_context* ctx, uint64_t key, int64_t n, float* out) {
  hipLaunchKernelGGL(init_normal_kernel, dim3(grid_of(n, kTrainBlock)), dim3(kTrainBlock), 0, ctx->stream, n, key, out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_init_uniform(s3grl_context* ctx, uint64_t key, float bound, int64_t n, float* out) {
  hipLaunchKernelGGL(init_uniform_kernel, dim3(grid_of(n, kTrainBlock)), dim3(kTrainBlock), 0, ctx->stream, n, key,
                     bound, out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_fill(s3grl_context* ctx, float value, int64_t n, float* out) {
  hipLaunchKernelGGL(fill_kernel, dim3(grid_of(n, kTrainBlock)), dim3(kTrainBlock), 0, ctx->stream, n, value, out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

}  // namespace s3grl
