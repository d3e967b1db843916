// The link classifier of the N2V row (reference baselines/n2v.py: sklearn's default LogisticRegression over the Hadamard
// features emb[src] ⊙ emb[dst]) on gfx950: the minimiser of
//
//   f(θ) = ½ w·w + C Σ_i [ log(1 + exp(z_i)) − y_i z_i ],   z_i = x_i·w + b,   θ = (w, b),   x_i = emb[src_i] ⊙ emb[dst_i]
//
// by damped Newton in fp64.  The rows of the [N, D] fp32 table are read in place through the pair list; no [M, D] feature
// matrix exists.  One iteration is four launches on the context's stream, every cross-block dependency a launch boundary:
//
//   lc_grad_kernel    rows in tiles of 64 over the blocks; a tile's x̃ = (x, 1) rows sit in LDS as fp64.  Per row z, p, the
//                     loss term, p − y and p(1 − p); then thread j sums column j of the gradient and every thread sums its
//                     entries of the packed upper triangle of Σ p(1 − p) x̃ x̃ᵀ, both in row order.  One partial (loss, g,
//                     triangle) per block
//   lc_solve_kernel   one block: folds the partials in block order, adds the ridge, writes g, f and max|g|.  At
//                     max|g| <= tol it raises `done`.  Otherwise Cholesky H = UᵀU in LDS (one owner thread per entry), the
//                     two triangular solves for d = H⁻¹ g, and gᵀd
//   lc_ladder_kernel  per row z and s = x̃·d once, then the loss term at z − t s for the whole ladder t = 1, ½, … 2⁻¹⁵,
//                     the rungs dealt over the row's lanes; one partial of 16 sums per block
//   lc_accept_kernel  one block: folds the ladder partials (16 chunks of blocks, then the chunks), adds the ridge term
//                     of every rung, takes the first t with f(θ − t d) <= f(θ) − c₁ t gᵀd + slack and moves θ; no
//                     such rung raises `done` = 2
//
// No kernel waits for another: no flag is polled, there is no grid barrier, and with `done` set every kernel returns at
// once, so a fit is max_iter × 4 launches without a host round trip.  Determinism: no float atomics; every sum has one
// owner thread and a fixed order; the butterfly over a row's lanes has a fixed shape.  Lane layout (lc_shape): LPR lanes
// per row, the smallest power of two >= D up to 64, each lane ceil(D / LPR) <= 2 channels; 256 / LPR rows at a time.
#include "s3grl_internal.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace s3grl {
namespace {

constexpr int kLcBlock = 256;
constexpr int kLcMaxDim = 128;
constexpr int kLcTile = 64;          // rows per tile: 64 · 129 fp64 of x̃ is 66 KB of LDS at D = 128
constexpr int kLcMaxBlocks = 256;    // of the two row passes, one per CU: past 256 tiles a block takes several, one
                                     // after the other, and the one block that folds the partials reads 256 of them
constexpr int kLcRungs = 16;         // t = 2^0 .. 2^-15
constexpr double kLcArmijo = 1e-4;
constexpr double kLcSlack = 0x1p-32;   // · |f(θ)|: what rounding may add to a ladder loss, far below any real increase
enum LcDone : int32_t { kRunning = 0, kConverged = 1, kNoRung = 2, kNotPositive = 3 };

// the device state: doubles [loss, gTd, step_t, gmax, θ (n), g (n), d (n)], then int32 [done, n_iter]
constexpr int kLcLoss = 0, kLcGtd = 1, kLcStepT = 2, kLcGmax = 3, kLcTheta = 4;

struct LcShape {
  int D, n, T, LPR, XS, P;   // n = D + 1; T = n (n + 1) / 2; XS the LDS row stride (odd); P doubles per partial
};
LcShape lc_shape(int D) {
  LcShape s;
  s.D = D;
  s.n = D + 1;
  s.T = s.n * (s.n + 1) / 2;
  s.LPR = 1;
  while (s.LPR < D && s.LPR < 64) s.LPR <<= 1;
  s.XS = s.n | 1;
  s.P = 1 + s.n + s.T;
  return s;
}
size_t grad_lds(const LcShape& s) { return ((size_t)kLcTile * s.XS + 3 * kLcTile) * sizeof(double); }
size_t solve_lds(const LcShape& s) { return ((size_t)s.T + 2 * s.n + 4) * sizeof(double); }

__host__ __device__ __forceinline__ int tri_off(int n, int i) { return i * n - i * (i - 1) / 2; }   // of entry (i, i)
// entry e of the packed upper triangle (row-major, n columns) -> its row; the column is i + e - tri_off(i)
__host__ __device__ __forceinline__ int tri_row(int n, int e) {
  const double b = 2.0 * n + 1.0;
  int i = (int)((b - sqrt(b * b - 8.0 * (double)e)) * 0.5);
  i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  if (tri_off(n, i) > e) --i;
  else if (i + 1 < n && tri_off(n, i + 1) <= e) ++i;
  return i;
}

// softplus(z) = log(1 + exp(z)) without overflow
__device__ __forceinline__ double softplus(double z) { return fmax(z, 0.0) + log1p(exp(-fabs(z))); }

struct LcRows {
  const float* __restrict__ emb;       // [N, D]
  const int32_t* __restrict__ pairs;   // [M, 2]
  const uint8_t* __restrict__ labels;  // [M] or null
  int64_t M;
  int tiles, tiles_per_block;
};

// The lanes of a row (q = their rank among LPR) form x̃ of row `row` and its dot products with u and (SECOND) v, both
// [n] fp64 with the intercept's entry last.  Every lane of the wave calls it; an inactive row gives zeros.  xs: the
// row's LDS image or null.
template <bool SECOND>
__device__ __forceinline__ void row_dots(const LcShape& s, const LcRows& r, int64_t row, bool active, int q,
                                         const double* __restrict__ u, const double* __restrict__ v, double* xs,
                                         double& du, double& dv) {
  double a = 0.0, b = 0.0;
  if (active) {
    const float* ea = r.emb + (int64_t)r.pairs[2 * row] * s.D;
    const float* eb = r.emb + (int64_t)r.pairs[2 * row + 1] * s.D;
    for (int k = q; k < s.D; k += s.LPR) {
      const double x = (double)ea[k] * (double)eb[k];   // exact: two fp32 factors
      if (xs) xs[k] = x;
      a = fma(x, u[k], a);
      if (SECOND) b = fma(x, v[k], b);
    }
  }
  for (int o = s.LPR / 2; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    if (SECOND) b += __shfl_xor(b, o, 64);
  }
  du = a + u[s.D];
  dv = SECOND ? b + v[s.D] : 0.0;
  if (xs && active && q == 0) xs[s.D] = 1.0;
}

// ---- pass 1: loss, gradient and Hessian partials -----------------------------------------------------------------
__global__ __launch_bounds__(kLcBlock) void lc_grad_kernel(LcShape s, LcRows r, const double* __restrict__ st,
                                                           const int32_t* __restrict__ flags,
                                                           double* __restrict__ partial) {
  if (flags[0] != kRunning) return;
  extern __shared__ double lc_lds[];
  double* xs = lc_lds;                    // [kLcTile][XS]
  double* rs = xs + kLcTile * s.XS;       // p − y
  double* ws = rs + kLcTile;              // p (1 − p)
  double* ls = ws + kLcTile;              // the loss term
  const int tid = threadIdx.x, G = kLcBlock / s.LPR, g = tid / s.LPR, q = tid % s.LPR;
  const double* theta = st + kLcTheta;
  double* part = partial + (int64_t)blockIdx.x * s.P;
  const int t0 = blockIdx.x * r.tiles_per_block;
  for (int ti = 0; ti < r.tiles_per_block; ++ti) {
    const int tile = t0 + ti;
    if (tile >= r.tiles) break;           // uniform over the block
    const int64_t p0 = (int64_t)tile * kLcTile;
    const int np = (int)min((int64_t)kLcTile, r.M - p0);
    for (int pb = 0; pb < kLcTile; pb += G) {
      const int p = pb + g;
      const bool active = p < np;
      double z, unused;
      row_dots<false>(s, r, p0 + p, active, q, theta, nullptr, active ? xs + p * s.XS : nullptr, z, unused);
      if (active && q == 0) {
        const double y = r.labels[p0 + p] ? 1.0 : 0.0;
        const double e = exp(-fabs(z)), big = 1.0 / (1.0 + e), small = e * big;
        rs[p] = (z >= 0.0 ? big : small) - y;
        ws[p] = big * small;
        ls[p] = softplus(z) - y * z;
      }
    }
    __syncthreads();
    if (tid < s.n) {                      // column tid of the gradient, rows in order
      double acc = 0.0;
      for (int p = 0; p < np; ++p) acc = fma(rs[p], xs[p * s.XS + tid], acc);
      part[1 + tid] = ti ? part[1 + tid] + acc : acc;
    } else if (tid == s.n) {
      double acc = 0.0;
      for (int p = 0; p < np; ++p) acc += ls[p];
      part[0] = ti ? part[0] + acc : acc;
    }
    for (int e = tid; e < s.T; e += kLcBlock) {
      const int i = tri_row(s.n, e), j = i + e - tri_off(s.n, i);
      double acc = 0.0;
      for (int p = 0; p < np; ++p) acc = fma(ws[p] * xs[p * s.XS + i], xs[p * s.XS + j], acc);
      part[1 + s.n + e] = ti ? part[1 + s.n + e] + acc : acc;
    }
    __syncthreads();
  }
}

// Σ over blocks [b0, b1) of p[b · stride], added in block order; eight loads in flight at a time
__device__ __forceinline__ double fold_blocks(const double* __restrict__ p, int stride, int b0, int b1) {
  double acc = 0.0;
  int b = b0;
  for (; b + 8 <= b1; b += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(b + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; b < b1; ++b) acc += p[(int64_t)b * stride];
  return acc;
}

// ---- pass 2: fold, factorise, solve ------------------------------------------------------------------------------
__global__ __launch_bounds__(kLcBlock) void lc_solve_kernel(LcShape s, int blocks, double C, double tol,
                                                            const double* __restrict__ partial, double* __restrict__ st,
                                                            int32_t* __restrict__ flags) {
  if (flags[0] != kRunning) return;
  extern __shared__ double lc_lds[];
  const int n = s.n, T = s.T, tid = threadIdx.x;
  double* H = lc_lds;        // [T] packed upper triangle, becomes U
  double* gv = H + T;        // [n] g, then y of Uᵀ y = g, then d
  double* g0 = gv + n;       // [n] g kept for gᵀd
  double* sc = g0 + n;       // [4] loss sum, verdict, pivot
  const double* theta = st + kLcTheta;
  for (int e = tid; e < s.P; e += kLcBlock) {
    const double acc = fold_blocks(partial + e, s.P, 0, blocks);
    if (e == 0) {
      sc[0] = acc;
    } else if (e <= n) {
      const int j = e - 1;
      const double gj = C * acc + (j < s.D ? theta[j] : 0.0);   // the intercept is not penalised
      gv[j] = g0[j] = gj;
    } else {
      const int t = e - 1 - n, i = tri_row(n, t), j = i + t - tri_off(n, i);
      H[t] = C * acc + (i == j && i < s.D ? 1.0 : 0.0);
    }
  }
  __syncthreads();
  if (tid == 0) {
    double ww = 0.0, gmax = 0.0;
    for (int j = 0; j < s.D; ++j) ww = fma(theta[j], theta[j], ww);
    for (int j = 0; j < n; ++j) gmax = fmax(gmax, fabs(gv[j]));
    st[kLcLoss] = 0.5 * ww + C * sc[0];
    st[kLcGmax] = gmax;
    sc[1] = gmax <= tol ? 1.0 : 0.0;    // NaN compares false: the factorisation below then stops the fit
  }
  if (tid < n) st[kLcTheta + n + tid] = gv[tid];
  __syncthreads();
  if (sc[1] != 0.0) {
    if (tid == 0) flags[0] = kConverged;
    return;
  }
  // H = UᵀU, right-looking; row k of U is H[tri_off(k) ..]
  for (int k = 0; k < n; ++k) {
    const int rk = tri_off(n, k);
    if (tid == 0) sc[2] = H[rk];
    __syncthreads();
    const double piv = sc[2];
    if (!(piv > 0.0) || !(piv < HUGE_VAL)) {   // uniform: every thread read the same value
      if (tid == 0) flags[0] = kNotPositive;
      return;
    }
    const double root = sqrt(piv);
    for (int j = k + tid; j < n; j += kLcBlock) H[rk + j - k] = j == k ? root : H[rk + j - k] / root;
    __syncthreads();
    const int m = n - k - 1;                   // the trailing triangle: entries (k+1+a, k+1+b), a <= b < m
    for (int e = tid; e < m * (m + 1) / 2; e += kLcBlock) {
      const int a = tri_row(m, e), b = a + e - tri_off(m, a);
      const int i = k + 1 + a, j = k + 1 + b;
      H[tri_off(n, i) + j - i] = fma(-H[rk + i - k], H[rk + j - k], H[tri_off(n, i) + j - i]);
    }
    __syncthreads();
  }
  for (int k = 0; k < n; ++k) {                // Uᵀ y = g: column k of Uᵀ is row k of U
    const int rk = tri_off(n, k);
    if (tid == 0) gv[k] = gv[k] / H[rk];
    __syncthreads();
    const int j = k + 1 + tid;
    if (j < n) gv[j] = fma(-H[rk + j - k], gv[k], gv[j]);
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {           // U d = y: column k of U above the diagonal
    if (tid == 0) gv[k] = gv[k] / H[tri_off(n, k)];
    __syncthreads();
    if (tid < k) gv[tid] = fma(-H[tri_off(n, tid) + k - tid], gv[k], gv[tid]);
    __syncthreads();
  }
  if (tid < n) st[kLcTheta + 2 * n + tid] = gv[tid];
  if (tid == 0) {
    double gtd = 0.0;
    for (int j = 0; j < n; ++j) gtd = fma(g0[j], gv[j], gtd);
    st[kLcGtd] = gtd;
  }
}

// ---- pass 3: the ladder's losses ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kLcBlock) void lc_ladder_kernel(LcShape s, LcRows r, const double* __restrict__ st,
                                                             const int32_t* __restrict__ flags,
                                                             double* __restrict__ partial) {
  if (flags[0] != kRunning) return;
  __shared__ double term[kLcTile][kLcRungs + 1];
  const int tid = threadIdx.x, G = kLcBlock / s.LPR, g = tid / s.LPR, q = tid % s.LPR;
  const double* theta = st + kLcTheta;
  const double* d = st + kLcTheta + 2 * s.n;
  const int t0 = blockIdx.x * r.tiles_per_block;
  double total = 0.0;                     // of rung tid, tid < kLcRungs
  for (int ti = 0; ti < r.tiles_per_block; ++ti) {
    const int tile = t0 + ti;
    if (tile >= r.tiles) break;
    const int64_t p0 = (int64_t)tile * kLcTile;
    const int np = (int)min((int64_t)kLcTile, r.M - p0);
    for (int pb = 0; pb < kLcTile; pb += G) {
      const int p = pb + g;
      const bool active = p < np;
      double z, sd;
      row_dots<true>(s, r, p0 + p, active, q, theta, d, nullptr, z, sd);
      if (active) {                        // the butterfly left z and sd on every lane of the row: a rung each
        const double y = r.labels[p0 + p] ? 1.0 : 0.0;
        for (int k = q; k < kLcRungs; k += s.LPR) {
          const double zt = z - ldexp(1.0, -k) * sd;
          term[p][k] = softplus(zt) - y * zt;
        }
      }
    }
    __syncthreads();
    if (tid < kLcRungs)
      for (int p = 0; p < np; ++p) total += term[p][tid];
    __syncthreads();
  }
  if (tid < kLcRungs) partial[(int64_t)blockIdx.x * kLcRungs + tid] = total;
}

// ---- pass 4: Armijo and the move ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kLcBlock) void lc_accept_kernel(LcShape s, int blocks, double C,
                                                             const double* __restrict__ partial, double* __restrict__ st,
                                                             int32_t* __restrict__ flags) {
  if (flags[0] != kRunning) return;
  __shared__ double f[kLcRungs];
  __shared__ double seg[kLcBlock / kLcRungs][kLcRungs];
  __shared__ int pick;
  const int n = s.n, tid = threadIdx.x;
  double* theta = st + kLcTheta;
  const double* d = st + kLcTheta + 2 * n;
  {   // thread (c, k) folds chunk c of the blocks for rung k; the chunks are then added in order
    const int k = tid % kLcRungs, c = tid / kLcRungs, chunks = kLcBlock / kLcRungs;
    const int per = (blocks + chunks - 1) / chunks;
    seg[c][k] = fold_blocks(partial + k, kLcRungs, min(c * per, blocks), min((c + 1) * per, blocks));
  }
  __syncthreads();
  if (tid < kLcRungs) {
    double acc = 0.0;
    for (int c = 0; c < kLcBlock / kLcRungs; ++c) acc += seg[c][tid];
    const double t = ldexp(1.0, -tid);
    double ww = 0.0;
    for (int j = 0; j < s.D; ++j) {
      const double w = theta[j] - t * d[j];
      ww = fma(w, w, ww);
    }
    f[tid] = 0.5 * ww + C * acc;
  }
  __syncthreads();
  if (tid == 0) {
    const double f0 = st[kLcLoss], gtd = st[kLcGtd], slack = kLcSlack * fabs(f0);
    int k = 0;
    while (k < kLcRungs && !(f[k] <= f0 - kLcArmijo * ldexp(1.0, -k) * gtd + slack)) ++k;   // NaN: rejected
    pick = k;
    if (k == kLcRungs) {
      st[kLcStepT] = 0.0;
      flags[0] = kNoRung;
    } else {
      st[kLcStepT] = ldexp(1.0, -k);
      flags[1] += 1;
    }
  }
  __syncthreads();
  if (pick < kLcRungs && tid < n) theta[tid] -= ldexp(1.0, -pick) * d[tid];
}

// ---- predict ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLcBlock) void lc_predict_kernel(LcShape s, LcRows r, const double* __restrict__ st,
                                                              uint8_t* __restrict__ pred, float* __restrict__ decision,
                                                              unsigned long long* __restrict__ counts) {
  __shared__ unsigned int cnt[4];         // tp, fp, fn, tn
  const int tid = threadIdx.x, G = kLcBlock / s.LPR, g = tid / s.LPR, q = tid % s.LPR;
  if (tid < 4) cnt[tid] = 0;
  __syncthreads();
  const int64_t p0 = (int64_t)blockIdx.x * kLcTile;
  const int np = (int)min((int64_t)kLcTile, r.M - p0);
  for (int pb = 0; pb < kLcTile; pb += G) {
    const int p = pb + g;
    const bool active = p < np;
    double z, unused;
    row_dots<false>(s, r, p0 + p, active, q, st + kLcTheta, nullptr, nullptr, z, unused);
    if (active && q == 0) {
      const bool hit = z > 0.0;
      pred[p0 + p] = hit ? 1 : 0;
      if (decision) decision[p0 + p] = (float)z;
      if (counts) atomicAdd(&cnt[r.labels[p0 + p] ? (hit ? 0 : 2) : (hit ? 1 : 3)], 1u);
    }
  }
  __syncthreads();
  if (counts && tid < 4 && cnt[tid]) atomicAdd(&counts[tid], (unsigned long long)cnt[tid]);
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

struct s3grl_linkclf {
  s3grl_context* ctx = nullptr;
  LcShape shape{};
  double C = 1.0, tol = 1e-8;
  int max_iter = 50;
  double* st = nullptr;        // the device state (see kLcTheta), flags behind it
  int32_t* flags = nullptr;
  double* partial = nullptr;   // [cap_blocks, P]
  double* ladder = nullptr;    // [cap_blocks, kLcRungs]
  int64_t cap_blocks = 0;
};

namespace {

size_t st_doubles(const LcShape& s) { return (size_t)kLcTheta + 3 * s.n; }
size_t st_bytes(const LcShape& s) { return st_doubles(s) * sizeof(double) + 2 * sizeof(int32_t); }

void lc_free(s3grl_linkclf* t) {
  for (void* p : {(void*)t->st, (void*)t->partial, (void*)t->ladder})
    if (p) (void)hipFree(p);
}

// pairs int32 [M, 2] and labels uint8 [M] (or null), both device -> checked on the host: ids in [0, N), both classes
s3grl_status lc_check(const s3grl_linkclf* t, int64_t N, const int32_t* pairs, const uint8_t* labels, int64_t M,
                      bool both_classes, const char* what) {
  std::vector<uint8_t> y(labels ? (size_t)M : 0);
  if (labels) S3GRL_HIP_TRY(hipMemcpyAsync(y.data(), labels, y.size(), hipMemcpyDeviceToHost, t->ctx->stream));
  S3GRL_TRY(check_ids(t->ctx, pairs, 2 * M, N, std::string(what) + ": a node outside [0, N)"));   // waits for y too
  if (both_classes) {
    size_t ones = 0;
    for (uint8_t v : y) ones += v != 0;
    if (ones == 0 || ones == y.size()) {
      set_last_error(std::string(what) + ": the labels hold one class only");
      return S3GRL_ERR_INVALID_ARGUMENT;
    }
  }
  return S3GRL_OK;
}

LcRows rows_of(const float* emb, const int32_t* pairs, const uint8_t* labels, int64_t M) {
  LcRows r;
  r.emb = emb;
  r.pairs = pairs;
  r.labels = labels;
  r.M = M;
  r.tiles = (int)((M + kLcTile - 1) / kLcTile);
  r.tiles_per_block = (r.tiles + kLcMaxBlocks - 1) / kLcMaxBlocks;
  return r;
}
int blocks_of(const LcRows& r) { return (r.tiles + r.tiles_per_block - 1) / r.tiles_per_block; }

s3grl_status ensure_partials(s3grl_linkclf* t, int64_t blocks) {
  if (blocks <= t->cap_blocks) return S3GRL_OK;
  S3GRL_HIP_TRY(hipStreamSynchronize(t->ctx->stream));   // the old buffers may still be in use
  for (double** p : {&t->partial, &t->ladder}) {
    if (*p) S3GRL_HIP_TRY(hipFree(*p));
    *p = nullptr;
  }
  t->cap_blocks = 0;
  S3GRL_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->partial), (size_t)blocks * t->shape.P * sizeof(double)));
  S3GRL_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->ladder), (size_t)blocks * kLcRungs * sizeof(double)));
  t->cap_blocks = blocks;
  return S3GRL_OK;
}

// `iters` Newton iterations from the current θ, four launches each
s3grl_status lc_iterate(s3grl_linkclf* t, const float* emb, const int32_t* pairs, const uint8_t* labels, int64_t M,
                        int iters) {
  const LcShape& s = t->shape;
  const LcRows r = rows_of(emb, pairs, labels, M);
  const int blocks = blocks_of(r);
  S3GRL_TRY(ensure_partials(t, blocks));
  hipStream_t st = t->ctx->stream;
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(lc_grad_kernel, dim3(blocks), dim3(kLcBlock), grad_lds(s), st, s, r, t->st, t->flags, t->partial);
    hipLaunchKernelGGL(lc_solve_kernel, dim3(1), dim3(kLcBlock), solve_lds(s), st, s, blocks, t->C, t->tol, t->partial,
                       t->st, t->flags);
    hipLaunchKernelGGL(lc_ladder_kernel, dim3(blocks), dim3(kLcBlock), 0, st, s, r, t->st, t->flags, t->ladder);
    hipLaunchKernelGGL(lc_accept_kernel, dim3(1), dim3(kLcBlock), 0, st, s, blocks, t->C, t->ladder, t->st, t->flags);
    S3GRL_HIP_TRY(hipGetLastError());
  }
  return S3GRL_OK;
}

bool lc_bad_rows(const s3grl_linkclf* t, const float* emb, int64_t N, const int32_t* pairs, int64_t M) {
  return !t || !emb || !pairs || N < 1 || N >= (int64_t(1) << 31) || M < 1 || M >= (int64_t(1) << 31);
}

}  // namespace

extern "C" {

s3grl_status s3grl_linkclf_layout(int32_t dim, int32_t* out) {
  if (!out || dim < 1 || dim > kLcMaxDim) return S3GRL_ERR_INVALID_ARGUMENT;
  const LcShape s = lc_shape(dim);
  out[0] = (s.D + s.LPR - 1) / s.LPR;
  out[1] = s.LPR;
  out[2] = kLcTile;
  out[3] = kLcMaxBlocks;
  return S3GRL_OK;
}

s3grl_status s3grl_linkclf_create(s3grl_context* ctx, int32_t dim, double C, double tol, int32_t max_iter,
                                  s3grl_linkclf** out) {
  if (!ctx || !out || dim < 1 || dim > kLcMaxDim || !(C > 0.0) || !std::isfinite(C) || !(tol >= 0.0) || max_iter < 0 ||
      max_iter > 10000)
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  auto* t = new s3grl_linkclf();
  t->ctx = ctx;
  t->shape = lc_shape(dim);
  t->C = C;
  t->tol = tol;
  t->max_iter = max_iter;
  auto fail = [&](hipError_t e) {
    set_last_error(std::string("linkclf create: ") + hipGetErrorString(e));
    lc_free(t);
    delete t;
    return e == hipErrorOutOfMemory ? S3GRL_ERR_OUT_OF_MEMORY : S3GRL_ERR_HIP;
  };
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&t->st), st_bytes(t->shape));
  if (e == hipSuccess) {
    t->flags = reinterpret_cast<int32_t*>(t->st + st_doubles(t->shape));
    e = hipMemsetAsync(t->st, 0, st_bytes(t->shape), ctx->stream);
  }
  // the two kernels with more than 64 KB of LDS at D = 128
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(lc_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)grad_lds(lc_shape(kLcMaxDim)));
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(lc_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)solve_lds(lc_shape(kLcMaxDim)));
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(e);
  *out = t;
  return S3GRL_OK;
}

s3grl_status s3grl_linkclf_fit(s3grl_linkclf* t, const float* emb, int64_t num_nodes, const int32_t* pairs,
                               const uint8_t* labels, int64_t num_pairs, const double* init_theta) {
  if (lc_bad_rows(t, emb, num_nodes, pairs, num_pairs) || !labels) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(lc_check(t, num_nodes, pairs, labels, num_pairs, true, "linkclf fit"));
  const LcShape& s = t->shape;
  std::vector<double> h(st_doubles(s) + 1, 0.0);   // + the two flags, both 0
  if (init_theta) std::copy(init_theta, init_theta + s.n, h.begin() + kLcTheta);
  S3GRL_HIP_TRY(hipMemcpyAsync(t->st, h.data(), st_bytes(s), hipMemcpyHostToDevice, t->ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(t->ctx->stream));   // h leaves scope
  return lc_iterate(t, emb, pairs, labels, num_pairs, t->max_iter);
}

s3grl_status s3grl_linkclf_newton_step(s3grl_linkclf* t, const float* emb, int64_t num_nodes, const int32_t* pairs,
                                       const uint8_t* labels, int64_t num_pairs) {
  if (lc_bad_rows(t, emb, num_nodes, pairs, num_pairs) || !labels) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(lc_check(t, num_nodes, pairs, labels, num_pairs, true, "linkclf newton_step"));
  S3GRL_HIP_TRY(hipMemsetAsync(t->flags, 0, sizeof(int32_t), t->ctx->stream));   // done: an earlier verdict does not bind
  return lc_iterate(t, emb, pairs, labels, num_pairs, 1);
}

s3grl_status s3grl_linkclf_state(s3grl_linkclf* t, double* theta, double* grad, double* loss, double* step_t,
                                 int32_t* n_iter, int32_t* done) {
  if (!t) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  const LcShape& s = t->shape;
  std::vector<double> h(st_doubles(s) + 1);
  S3GRL_HIP_TRY(hipMemcpyAsync(h.data(), t->st, st_bytes(s), hipMemcpyDeviceToHost, t->ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  int32_t fl[2];
  std::memcpy(fl, h.data() + st_doubles(s), sizeof(fl));
  if (theta) std::copy(h.begin() + kLcTheta, h.begin() + kLcTheta + s.n, theta);
  if (grad) std::copy(h.begin() + kLcTheta + s.n, h.begin() + kLcTheta + 2 * s.n, grad);
  if (loss) *loss = h[kLcLoss];
  if (step_t) *step_t = h[kLcStepT];
  if (n_iter) *n_iter = fl[1];
  if (done) *done = fl[0];
  return S3GRL_OK;
}

s3grl_status s3grl_linkclf_predict(s3grl_linkclf* t, const float* emb, int64_t num_nodes, const int32_t* pairs,
                                   int64_t num_pairs, const uint8_t* labels, uint8_t* pred, float* decision,
                                   int64_t* counts) {
  if (!t || num_pairs < 0) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  if (counts) S3GRL_HIP_TRY(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), t->ctx->stream));
  if (num_pairs == 0) return S3GRL_OK;
  if (lc_bad_rows(t, emb, num_nodes, pairs, num_pairs) || !pred || (counts && !labels))
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_TRY(lc_check(t, num_nodes, pairs, nullptr, num_pairs, false, "linkclf predict"));
  LcRows r = rows_of(emb, pairs, labels, num_pairs);
  hipLaunchKernelGGL(lc_predict_kernel, dim3((unsigned)r.tiles), dim3(kLcBlock), 0, t->ctx->stream, t->shape, r, t->st,
                     pred, decision, reinterpret_cast<unsigned long long*>(counts));
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_linkclf_destroy(s3grl_linkclf* t) {
  if (!t) return S3GRL_OK;
  (void)hipSetDevice(t->ctx->device);
  (void)hipStreamSynchronize(t->ctx->stream);
  lc_free(t);
  delete t;
  return S3GRL_OK;
}

}  // extern "C"
