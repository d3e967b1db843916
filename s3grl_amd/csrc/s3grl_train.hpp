// What the baseline trainers (node2vec, MF, SIGNNet, GAE) share: the counter-based draw generator, the dropout mask
// rule, dense Adam, a fixed-order fp64 block sum and a few host helpers.  The kernels built on the generator that
// need no trainer of their own (epoch permutation, initial values) are s3grl_train.hip.
//
// The wave reductions are NOT here: GIC's wave_sum / wave_max butterfly with offsets 1 -> 32, WalkPool's and SoP's
// 32 -> 1, and a float sum rounds differently in the other order.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "s3grl_internal.hpp"

namespace s3grl {
namespace {

// ---- the draw generator --------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {   // splitmix64 finaliser (a bijection)
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
// The key of one stream of draws at (seed, epoch, step).  The stream number sits under the step in a field of
// StreamBits bits, and the width is part of every draw: node2vec has four streams and packs step << 2, MF and SIGNNet
// pack step << 3.  Each trainer keeps its own stream enum (the values are part of the draw as well).
template <int StreamBits>
uint64_t stream_key(uint32_t seed, int64_t epoch, int64_t step, uint32_t stream) {
  static_assert(StreamBits == 2 || StreamBits == 3, "a width no trainer draws with");
  return mix64(mix64(mix64(seed) ^ (uint64_t)epoch) ^ (((uint64_t)step << StreamBits) | stream));
}
// 32 random bits for (row < 2^31, position < 2^32) of one stream
__device__ __forceinline__ uint32_t draw(uint64_t key, uint64_t row, uint64_t pos) {
  return (uint32_t)(mix64(key ^ mix64((row << 32) ^ pos)) >> 32);
}
__device__ __forceinline__ uint32_t below(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }

// dropout of one element: the caller's uint8 mask or the hash.  How an element indexes `given` and the draw is the
// trainer's (keeps in s3grl_mf.hip, sn_keeps in s3grl_signnet.hip: their layouts differ).
struct DropMask {
  const uint8_t* given;
  uint64_t key;
  uint32_t drop_below;   // an element is dropped when its draw is below this: p · 2^32
  float scale;           // 1 / (1 - p)
};
DropMask drop_mask(double dropout, const uint8_t* given, uint64_t key) {
  const double thr = dropout * 4294967296.0;
  return DropMask{given, key, (uint32_t)std::min(thr, 4294967295.0), (float)(1.0 / (1.0 - dropout))};
}

// ---- dense Adam ----------------------------------------------------------------------------------------------
// torch.optim.Adam and SparseAdam defaults.  node2vec's SparseAdam (s3grl_node2vec.hip) shares these three only: its
// operation order differs.
constexpr double kAdamBeta1 = 0.9, kAdamBeta2 = 0.999, kAdamEps = 1e-8;

// torch.optim.Adam (no weight decay, no amsgrad) in its own operation order:
//   m' = m + (g - m)(1 - b1);  v' = v b2 + (1 - b2) g g;  w' = w - step_size · m' / (sqrt(v') / sqrt(bc2) + eps)
struct AdamStep {
  float b1c, b2, b2c, step_size, bc2_sqrt, eps;
};
AdamStep adam_step(double lr, int64_t steps) {   // steps: the count this update brings Adam to
  const double bc1 = 1.0 - std::pow(kAdamBeta1, (double)steps), bc2 = 1.0 - std::pow(kAdamBeta2, (double)steps);
  return AdamStep{(float)(1.0 - kAdamBeta1), (float)kAdamBeta2, (float)(1.0 - kAdamBeta2), (float)(lr / bc1),
                  (float)std::sqrt(bc2), (float)kAdamEps};
}
__device__ __forceinline__ void adam_update(const AdamStep& k, float g, float* w, float* m, float* v) {
  const float mn = *m + (g - *m) * k.b1c;
  const float vn = *v * k.b2 + k.b2c * g * g;
  *m = mn;
  *v = vn;
  *w = *w - k.step_size * (mn / (sqrtf(vn) / k.bc2_sqrt + k.eps));
}

// ---- device helpers ------------------------------------------------------------------------------------------
// fixed-order sum of one double per thread over a block of Block threads; the result is valid in thread 0.
// sh: Block / 64 doubles of LDS
template <int Block>
__device__ __forceinline__ double block_sum_f64(double x, double* sh) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < Block / 64; ++w) s += sh[w];
  __syncthreads();
  return s;
}

__device__ __forceinline__ float sigmoid32(float x) { return 1.f / (1.f + expf(-x)); }

// ---- host helpers --------------------------------------------------------------------------------------------
bool bad_lr(double lr) { return !(lr > 0.0) || !std::isfinite(lr); }

// *p -> a fresh block of at least one T and `count` of them; the caller has made sure the old one is idle
template <typename T>
s3grl_status regrow(T** p, size_t count) {
  if (*p) S3GRL_HIP_TRY(hipFree(*p));
  *p = nullptr;
  S3GRL_HIP_TRY(hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(T)));
  return S3GRL_OK;
}

}  // namespace
}  // namespace s3grl
