// Graph InfoClust's per-epoch hot path, gfx950: the soft k-means "Clusterator" (forward and the backward of its one
// differentiable iteration) and the fused cluster discriminator (forward and backward).  Deterministic: no float
// atomics, every sum runs in a fixed order, two runs are bit-identical.  fp32 in, fp32 out, asynchronous on the
// context's stream.
//
// All four are per-node work against a small K x d table plus one K x d reduction over the nodes, so they share one
// shape: a workgroup of 256 threads owns a chunk of kGicChunk = 64 nodes and keeps its [64, K] matrix (responsibilities,
// S, or their gradients) in LDS.  Three tile products, each thread a 4 x 4 register block, the table streamed through
// one 16.5 KiB LDS tile (so the table itself is read through L2, never held whole):
//   dot_rows    q[n][k]    = Σ_c X[n][c] · T[k][c]      the chunk's rows against every table row
//   mix_rows    out[n][c] += Σ_k a[n][k] · T[k][c]      the chunk's [64, K] matrix times the table
//   outer_rows  part[k][c] = Σ_n a[n][k] · X[n][c]      the chunk's K x d partial, n ascending
// The K x d (and K) partials of the chunks are added in chunk order by a second launch.
#include "s3grl_internal.hpp"
#include "s3grl_train.hpp"

#include <algorithm>
#include <atomic>

namespace s3grl {
namespace {

constexpr int kGicBlock = 256;
constexpr int kGicChunk = 64;            // nodes per workgroup
constexpr int kGicTile = 64;             // K tile and d tile of the products
constexpr int kGicDotTile = 32;          // reduction tile of dot_rows
constexpr int kGicTileFloats = 2 * kGicChunk * (kGicDotTile + 1);   // >= 64 · 65
constexpr float kGicEps = 1e-6f;

__host__ __device__ inline int gic_lda(int K) { return (K + kGicTile - 1) / kGicTile * kGicTile + 1; }

__device__ inline float wave_sum(float v) {
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline float wave_max(float v) {
  for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// q[nn][k] = Σ_c X[n0 + nn][c] · T[k][c] for the chunk's 64 rows and every k < K; rows past N read as zero.
// Ends with a barrier.
__device__ void dot_rows(const float* __restrict__ X, int64_t ldx, int64_t n0, int64_t N, const float* __restrict__ T,
                         int K, int d, float* __restrict__ q, int ldq, float* __restrict__ tile) {
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  float* __restrict__ Xs = tile;
  float* __restrict__ Ts = tile + kGicChunk * (kGicDotTile + 1);
  for (int k0 = 0; k0 < K; k0 += kGicTile) {
    float acc[4][4] = {};
    for (int c0 = 0; c0 < d; c0 += kGicDotTile) {
      for (int e = t; e < kGicChunk * kGicDotTile; e += kGicBlock) {
        const int row = e / kGicDotTile, col = e % kGicDotTile;
        const int c = c0 + col;
        const int64_t n = n0 + row;
        const int k = k0 + row;
        Xs[row * (kGicDotTile + 1) + col] = (n < N && c < d) ? X[n * ldx + c] : 0.f;
        Ts[row * (kGicDotTile + 1) + col] = (k < K && c < d) ? T[(int64_t)k * d + c] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int c = 0; c < kGicDotTile; ++c) {
        float a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = Xs[(ty * 4 + i) * (kGicDotTile + 1) + c];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = Ts[(tx + 16 * j) * (kGicDotTile + 1) + c];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + tx + 16 * j;
        if (k < K) q[(ty * 4 + i) * ldq + k] = acc[i][j];
      }
  }
  __syncthreads();
}

// acc[i][j] += Σ_k a[ty·4 + i][k] · T[k][c0 + tx + 16·j]; columns past d read as zero.  Ends with a barrier.
__device__ void mix_rows(const float* __restrict__ a, int lda, const float* __restrict__ T, int K, int d, int c0,
                         float* __restrict__ tile, float (&acc)[4][4]) {
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  for (int k0 = 0; k0 < K; k0 += kGicTile) {
    for (int e = t; e < kGicTile * kGicTile; e += kGicBlock) {
      const int row = e / kGicTile, col = e % kGicTile;
      const int k = k0 + row, c = c0 + col;
      tile[row * (kGicTile + 1) + col] = (k < K && c < d) ? T[(int64_t)k * d + c] : 0.f;
    }
    __syncthreads();
    const int kn = min(kGicTile, K - k0);
    for (int k = 0; k < kn; ++k) {
      float av[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = a[(ty * 4 + i) * lda + k0 + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = tile[k * (kGicTile + 1) + tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * b[j];
    }
    __syncthreads();
  }
}

// part[k][c] = Σ_nn a[nn][k] · X[n0 + nn][c], nn ascending, for k < K, c < d.  a's columns K .. lda-2 and its rows
// past N must hold zeros.  Ends with a barrier.
__device__ void outer_rows(const float* __restrict__ a, int lda, const float* __restrict__ X, int64_t ldx, int64_t n0,
                           int64_t N, int K, int d, float* __restrict__ part, float* __restrict__ tile) {
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  for (int c0 = 0; c0 < d; c0 += kGicTile) {
    for (int e = t; e < kGicChunk * kGicTile; e += kGicBlock) {
      const int row = e / kGicTile, col = e % kGicTile;
      const int64_t n = n0 + row;
      const int c = c0 + col;
      tile[row * (kGicTile + 1) + col] = (n < N && c < d) ? X[n * ldx + c] : 0.f;
    }
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += kGicTile) {
      float acc[4][4] = {};
#pragma unroll 4
      for (int nn = 0; nn < kGicChunk; ++nn) {
        float av[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = a[nn * lda + k0 + ty * 4 + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = tile[nn * (kGicTile + 1) + tx + 16 * j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * b[j];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + ty * 4 + i, c = c0 + tx + 16 * j;
          if (k < K && c < d) part[(int64_t)k * d + c] = acc[i][j];
        }
    }
    __syncthreads();
  }
}

// out[r] = x[r] / (‖x[r]‖ + 1e-6), nrm[r] = ‖x[r]‖ (nrm may be null); a wavefront per row
__global__ __launch_bounds__(kGicBlock) void gic_normalise_kernel(const float* __restrict__ x, int64_t ldx,
                                                                 int64_t rows, int d, float* __restrict__ out,
                                                                 float* __restrict__ nrm) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (kGicBlock / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  float ss = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = x[r * ldx + c];
    ss += v * v;
  }
  const float norm = sqrtf(wave_sum(ss));
  const float den = norm + kGicEps;
  for (int c = lane; c < d; c += 64) out[r * d + c] = x[r * ldx + c] / den;
  if (nrm && lane == 0) nrm[r] = norm;
}

// One k-means assignment of a chunk: r = softmax(beta · data · munᵀ) (written out when r_out is given), and the
// chunk's partials cr_part[chunk][k] = Σ_n r[n][k], cm_part[chunk][k][:] = Σ_n r[n][k] · data[n].
__global__ __launch_bounds__(kGicBlock) void gic_assign_kernel(const float* __restrict__ data,
                                                              const float* __restrict__ mun, int64_t N, int K, int d,
                                                              float beta, float* __restrict__ r_out,
                                                              float* __restrict__ cr_part,
                                                              float* __restrict__ cm_part) {
  extern __shared__ float gic_dyn[];
  __shared__ float tile[kGicTileFloats];
  float* __restrict__ q = gic_dyn;
  const int lda = gic_lda(K);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t n0 = (int64_t)blockIdx.x * kGicChunk;
  for (int e = t; e < kGicChunk * lda; e += kGicBlock) q[e] = 0.f;
  __syncthreads();
  dot_rows(data, d, n0, N, mun, K, d, q, lda, tile);
  for (int nn = wave * 16; nn < wave * 16 + 16; ++nn) {
    const int64_t n = n0 + nn;
    float* __restrict__ row = q + nn * lda;
    if (n < N) {
      float m = -INFINITY;
      for (int k = lane; k < K; k += 64) m = fmaxf(m, beta * row[k]);
      m = wave_max(m);
      float s = 0.f;
      for (int k = lane; k < K; k += 64) {
        const float e = expf(beta * row[k] - m);
        row[k] = e;
        s += e;
      }
      s = wave_sum(s);
      for (int k = lane; k < K; k += 64) {
        const float rv = row[k] / s;
        row[k] = rv;
        if (r_out) r_out[n * K + k] = rv;
      }
    } else {
      for (int k = lane; k < K; k += 64) row[k] = 0.f;
    }
  }
  __syncthreads();
  for (int k = t; k < K; k += kGicBlock) {
    float s = 0.f;
    for (int nn = 0; nn < kGicChunk; ++nn) s += q[nn * lda + k];
    cr_part[(int64_t)blockIdx.x * K + k] = s;
  }
  outer_rows(q, lda, data, d, n0, N, K, d, cm_part + (int64_t)blockIdx.x * K * d, tile);
}

// Workgroup k: cluster_r[k] and cluster_mean[k] from the chunk partials in chunk order, mu[k] = (1 / cluster_r) ·
// cluster_mean, and (when mun is given) the next iteration's mu[k] / (‖mu[k]‖ + 1e-6).
__global__ __launch_bounds__(kGicBlock) void gic_update_kernel(const float* __restrict__ cr_part,
                                                              const float* __restrict__ cm_part, int64_t chunks,
                                                              int K, int d, float* __restrict__ mu,
                                                              float* __restrict__ cr_out, float* __restrict__ mun) {
  __shared__ float s_w[kGicBlock / 64];
  const int k = blockIdx.x, t = threadIdx.x;
  float cr = 0.f;
  for (int64_t z = 0; z < chunks; ++z) cr += cr_part[z * K + k];
  const float inv = 1.f / cr;
  float ss = 0.f;
  for (int c = t; c < d; c += kGicBlock) {
    float s = 0.f;
    for (int64_t z = 0; z < chunks; ++z) s += cm_part[(z * K + k) * d + c];
    const float m = inv * s;
    mu[(int64_t)k * d + c] = m;
    ss += m * m;
  }
  if (t == 0) cr_out[k] = cr;
  if (!mun) return;
  ss = wave_sum(ss);
  if ((t & 63) == 0) s_w[t >> 6] = ss;
  __syncthreads();
  float tot = s_w[0];
  for (int w = 1; w < kGicBlock / 64; ++w) tot += s_w[w];
  const float den = sqrtf(tot) + kGicEps;
  for (int c = t; c < d; c += kGicBlock) mun[(int64_t)k * d + c] = mu[(int64_t)k * d + c] / den;
}

// Workgroup k: gM[k] = gZ[k] / cluster_r[k], g_cr[k] = -Σ_c gZ[k][c] · Z[k][c] / cluster_r[k]
__global__ __launch_bounds__(kGicBlock) void gic_gm_kernel(const float* __restrict__ gZ, const float* __restrict__ Z,
                                                          const float* __restrict__ cr, int d,
                                                          float* __restrict__ gM, float* __restrict__ g_cr) {
  __shared__ float s_w[kGicBlock / 64];
  const int k = blockIdx.x, t = threadIdx.x;
  const float c_r = cr[k];
  float s = 0.f;
  for (int c = t; c < d; c += kGicBlock) {
    const float g = gZ[(int64_t)k * d + c];
    gM[(int64_t)k * d + c] = g / c_r;
    s += g * Z[(int64_t)k * d + c];
  }
  s = wave_sum(s);
  if ((t & 63) == 0) s_w[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    float tot = s_w[0];
    for (int w = 1; w < kGicBlock / 64; ++w) tot += s_w[w];
    g_cr[k] = -tot / c_r;
  }
}

// The backward of one k-means iteration for a chunk (mu detached): g_r = gS + g_cr + data · gMᵀ, the softmax backward
// times beta against mun, the rᵀ · data term, and back through h / (‖h‖ + 1e-6).
__global__ __launch_bounds__(kGicBlock) void gic_cluster_bwd_kernel(
    const float* __restrict__ data, const float* __restrict__ h, int64_t ldh, const float* __restrict__ nrm,
    const float* __restrict__ mun, const float* __restrict__ r, const float* __restrict__ gM,
    const float* __restrict__ g_cr, const float* __restrict__ gS, int64_t N, int K, int d, float beta,
    float* __restrict__ g_h) {
  extern __shared__ float gic_dyn[];
  __shared__ float tile[kGicTileFloats];
  const int lda = gic_lda(K);
  float* __restrict__ a = gic_dyn;                      // r
  float* __restrict__ b = gic_dyn + kGicChunk * lda;    // data · gMᵀ, then the gradient of dist
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, tx = t & 15, ty = t >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * kGicChunk;
  for (int e = t; e < 2 * kGicChunk * lda; e += kGicBlock) gic_dyn[e] = 0.f;
  __syncthreads();
  dot_rows(data, d, n0, N, gM, K, d, b, lda, tile);
  for (int nn = wave * 16; nn < wave * 16 + 16; ++nn) {
    const int64_t n = n0 + nn;
    if (n >= N) continue;                  // a and b stay zero (dot_rows read the row as zero)
    float dotp = 0.f;
    for (int k = lane; k < K; k += 64) {
      const float rv = r[n * K + k];
      const float gr = gS[n * K + k] + g_cr[k] + b[nn * lda + k];
      a[nn * lda + k] = rv;
      b[nn * lda + k] = gr;
      dotp += rv * gr;
    }
    dotp = wave_sum(dotp);
    for (int k = lane; k < K; k += 64) b[nn * lda + k] = beta * a[nn * lda + k] * (b[nn * lda + k] - dotp);
  }
  __syncthreads();
  for (int c0 = 0; c0 < d; c0 += kGicTile) {
    float acc[4][4] = {};
    mix_rows(a, lda, gM, K, d, c0, tile, acc);
    mix_rows(b, lda, mun, K, d, c0, tile, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t n = n0 + ty * 4 + i;
        const int c = c0 + tx + 16 * j;
        if (n < N && c < d) g_h[n * d + c] = acc[i][j];
      }
  }
  __threadfence_block();
  __syncthreads();
  for (int nn = wave * 16; nn < wave * 16 + 16; ++nn) {
    const int64_t n = n0 + nn;
    if (n >= N) continue;
    float dp = 0.f;
    for (int c = lane; c < d; c += 64) dp += g_h[n * d + c] * h[n * ldh + c];
    dp = wave_sum(dp);
    const float norm = nrm[n];
    const float s = 1.f / (norm + kGicEps);
    const float coef = norm > 0.f ? dp * s * s / norm : 0.f;
    for (int c = lane; c < d; c += 64) g_h[n * d + c] = s * g_h[n * d + c] - h[n * ldh + c] * coef;
  }
}


// logits[n] = h1[n] · c2[n], logits[N + n] = h2[n] · c2[n], c2[n] = sigmoid(Σ_k S[n][k] · Z[k]) kept in registers
__global__ __launch_bounds__(kGicBlock) void gic_disc_fwd_kernel(const float* __restrict__ S,
                                                                const float* __restrict__ Z,
                                                                const float* __restrict__ h1,
                                                                const float* __restrict__ h2, int64_t ldh, int64_t N,
                                                                int K, int d, float* __restrict__ logits) {
  extern __shared__ float gic_dyn[];
  __shared__ float tile[kGicTileFloats];
  const int lda = gic_lda(K);
  float* __restrict__ a = gic_dyn;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * kGicChunk;
  for (int e = t; e < kGicChunk * lda; e += kGicBlock) {
    const int row = e / lda, k = e % lda;
    a[e] = (n0 + row < N && k < K) ? S[(n0 + row) * K + k] : 0.f;
  }
  __syncthreads();
  float p1[4] = {}, p2[4] = {};
  for (int c0 = 0; c0 < d; c0 += kGicTile) {
    float acc[4][4] = {};
    mix_rows(a, lda, Z, K, d, c0, tile, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t n = n0 + ty * 4 + i;
        const int c = c0 + tx + 16 * j;
        if (n < N && c < d) {
          const float c2 = sigmoid32(acc[i][j]);
          p1[i] += h1[n * ldh + c] * c2;
          p2[i] += h2[n * ldh + c] * c2;
        }
      }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    for (int o = 1; o < 16; o <<= 1) {      // the 16 lanes of one ty sit side by side in a wavefront
      p1[i] += __shfl_xor(p1[i], o, 64);
      p2[i] += __shfl_xor(p2[i], o, 64);
    }
    const int64_t n = n0 + ty * 4 + i;
    if (tx == 0 && n < N) {
      logits[n] = p1[i];
      logits[N + n] = p2[i];
    }
  }
}

// The discriminator's backward for a chunk: g_h1 = g1 · c2, g_h2 = g2 · c2, g_pre = (g1 · h1 + g2 · h2) · c2(1 - c2)
// (written to g_pre for the two products), gS = g_pre · Zᵀ and the chunk's partial of gZ = Sᵀ · g_pre.
__global__ __launch_bounds__(kGicBlock) void gic_disc_bwd_kernel(
    const float* __restrict__ S, const float* __restrict__ Z, const float* __restrict__ h1,
    const float* __restrict__ h2, int64_t ldh, const float* __restrict__ g, int64_t N, int K, int d,
    float* __restrict__ g_h1, float* __restrict__ g_h2, int64_t ldg, float* __restrict__ g_pre,
    float* __restrict__ gS, float* __restrict__ gZ_part) {
  extern __shared__ float gic_dyn[];
  __shared__ float tile[kGicTileFloats];
  const int lda = gic_lda(K);
  float* __restrict__ a = gic_dyn;
  float* __restrict__ b = gic_dyn + kGicChunk * lda;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * kGicChunk;
  for (int e = t; e < kGicChunk * lda; e += kGicBlock) {
    const int row = e / lda, k = e % lda;
    a[e] = (n0 + row < N && k < K) ? S[(n0 + row) * K + k] : 0.f;
    b[e] = 0.f;
  }
  __syncthreads();
  for (int c0 = 0; c0 < d; c0 += kGicTile) {
    float acc[4][4] = {};
    mix_rows(a, lda, Z, K, d, c0, tile, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t n = n0 + ty * 4 + i;
        const int c = c0 + tx + 16 * j;
        if (n < N && c < d) {
          const float c2 = sigmoid32(acc[i][j]);
          const float g1 = g[n], g2 = g[N + n];
          g_h1[n * ldg + c] = g1 * c2;
          g_h2[n * ldg + c] = g2 * c2;
          g_pre[n * d + c] = (g1 * h1[n * ldh + c] + g2 * h2[n * ldh + c]) * (c2 * (1.f - c2));
        }
      }
  }
  __threadfence_block();
  __syncthreads();
  dot_rows(g_pre, d, n0, N, Z, K, d, b, lda, tile);
  for (int e = t; e < kGicChunk * K; e += kGicBlock) {
    const int row = e / K, k = e % K;
    if (n0 + row < N) gS[(n0 + row) * K + k] = b[row * lda + k];
  }
  outer_rows(a, lda, g_pre, d, n0, N, K, d, gZ_part + (int64_t)blockIdx.x * K * d, tile);
}

// out[i] = Σ_z part[z][i] in chunk order
__global__ __launch_bounds__(kGicBlock) void gic_sum_parts_kernel(const float* __restrict__ part, int64_t chunks,
                                                                 int64_t M, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kGicBlock + threadIdx.x;
  if (i >= M) return;
  float s = 0.f;
  for (int64_t z = 0; z < chunks; ++z) s += part[z * M + i];
  out[i] = s;
}

bool gic_shape_ok(int64_t N, int64_t d, int64_t K) {
  if (N < 1 || N >= (int64_t(1) << 31) || d < 1 || d > S3GRL_GIC_MAX_DIM || K < 1 || K > S3GRL_GIC_MAX_CLUSTERS) {
    set_last_error("gic: need 1 <= N < 2^31, 1 <= d <= " + std::to_string(S3GRL_GIC_MAX_DIM) +
                   " and 1 <= K <= " + std::to_string(S3GRL_GIC_MAX_CLUSTERS));
    return false;
  }
  return true;
}

int64_t gic_chunks(int64_t N) { return (N + kGicChunk - 1) / kGicChunk; }

// Raises a kernel's dynamic-LDS limit to `lds` bytes on the context's device, once per size: `have` (one per kernel)
// keeps the largest size set so far per device, so that the steady state of an epoch makes no runtime call here.
constexpr int kGicMaxDevices = 64;
struct GicLdsSet {
  std::atomic<int> bytes[kGicMaxDevices];
};

template <typename Kern>
s3grl_status gic_set_lds(Kern kern, size_t lds, int device, GicLdsSet& have) {
  const bool cached = device >= 0 && device < kGicMaxDevices;
  if (cached && have.bytes[device].load(std::memory_order_relaxed) >= (int)lds) return S3GRL_OK;
  S3GRL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
  if (cached) have.bytes[device].store((int)lds, std::memory_order_relaxed);
  return S3GRL_OK;
}

GicLdsSet g_assign_lds, g_cluster_bwd_lds, g_disc_fwd_lds, g_disc_bwd_lds;

}  // namespace
}  // namespace s3grl

using namespace s3grl;

extern "C" {

s3grl_status s3grl_gic_normalise(s3grl_context* ctx, int64_t rows, int64_t d, const float* x, int64_t ldx, float* out,
                                 float* nrm) {
  if (!ctx || !x || !out || ldx < d) return S3GRL_ERR_INVALID_ARGUMENT;
  if (!gic_shape_ok(rows, d, 1)) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const int per = kGicBlock / 64;
  hipLaunchKernelGGL(gic_normalise_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(kGicBlock), 0, ctx->stream, x,
                     ldx, rows, (int)d, out, nrm);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_gic_cluster_forward(s3grl_context* ctx, int64_t N, int64_t d, int64_t K, float beta,
                                       int32_t num_iter, const float* data, const float* init, float* mun_last,
                                       float* mun_tmp, float* partial, float* mu, float* cluster_r, float* r) {
  if (!ctx || !data || !init || !mun_last || !partial || !mu || !cluster_r || !r || num_iter < 1 ||
      (num_iter > 1 && !mun_tmp))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (!gic_shape_ok(N, d, K)) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t chunks = gic_chunks(N);
  float* cr_part = partial;
  float* cm_part = partial + chunks * K;
  const size_t lds = sizeof(float) * kGicChunk * gic_lda((int)K);
  if (s3grl_status st = gic_set_lds(gic_assign_kernel, lds, ctx->device, g_assign_lds)) return st;
  // the iterations alternate between the two tables so that the last one reads mun_last
  float* cur = (num_iter - 1) % 2 == 0 ? mun_last : mun_tmp;
  float* nxt = cur == mun_last ? mun_tmp : mun_last;
  const int per = kGicBlock / 64;
  hipLaunchKernelGGL(gic_normalise_kernel, dim3((unsigned)((K + per - 1) / per)), dim3(kGicBlock), 0, ctx->stream, init,
                     d, K, (int)d, cur, (float*)nullptr);
  S3GRL_HIP_TRY(hipGetLastError());
  for (int32_t it = 0; it < num_iter; ++it) {
    const bool last = it == num_iter - 1;
    hipLaunchKernelGGL(gic_assign_kernel, dim3((unsigned)chunks), dim3(kGicBlock), lds, ctx->stream, data, cur, N,
                       (int)K, (int)d, beta, last ? r : (float*)nullptr, cr_part, cm_part);
    S3GRL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gic_update_kernel, dim3((unsigned)K), dim3(kGicBlock), 0, ctx->stream, cr_part, cm_part, chunks,
                       (int)K, (int)d, mu, cluster_r, last ? (float*)nullptr : nxt);
    S3GRL_HIP_TRY(hipGetLastError());
    std::swap(cur, nxt);
  }
  return S3GRL_OK;
}

s3grl_status s3grl_gic_cluster_backward(s3grl_context* ctx, int64_t N, int64_t d, int64_t K, float beta,
                                        const float* data, const float* h, int64_t ldh, const float* nrm,
                                        const float* mun, const float* r, const float* Z, const float* cluster_r,
                                        const float* gZ, const float* gS, float* table_ws, float* g_h) {
  if (!ctx || !data || !h || !nrm || !mun || !r || !Z || !cluster_r || !gZ || !gS || !table_ws || !g_h || ldh < d)
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (!gic_shape_ok(N, d, K)) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  float* gM = table_ws;
  float* g_cr = table_ws + K * d;
  hipLaunchKernelGGL(gic_gm_kernel, dim3((unsigned)K), dim3(kGicBlock), 0, ctx->stream, gZ, Z, cluster_r, (int)d, gM,
                     g_cr);
  S3GRL_HIP_TRY(hipGetLastError());
  const size_t lds = sizeof(float) * 2 * kGicChunk * gic_lda((int)K);
  if (s3grl_status st = gic_set_lds(gic_cluster_bwd_kernel, lds, ctx->device, g_cluster_bwd_lds)) return st;
  hipLaunchKernelGGL(gic_cluster_bwd_kernel, dim3((unsigned)gic_chunks(N)), dim3(kGicBlock), lds, ctx->stream, data, h,
                     ldh, nrm, mun, r, gM, g_cr, gS, N, (int)K, (int)d, beta, g_h);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_gic_disc_forward(s3grl_context* ctx, int64_t N, int64_t d, int64_t K, const float* S,
                                    const float* Z, const float* h1, const float* h2, int64_t ldh, float* logits) {
  if (!ctx || !S || !Z || !h1 || !h2 || !logits || ldh < d) return S3GRL_ERR_INVALID_ARGUMENT;
  if (!gic_shape_ok(N, d, K)) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const size_t lds = sizeof(float) * kGicChunk * gic_lda((int)K);
  if (s3grl_status st = gic_set_lds(gic_disc_fwd_kernel, lds, ctx->device, g_disc_fwd_lds)) return st;
  hipLaunchKernelGGL(gic_disc_fwd_kernel, dim3((unsigned)gic_chunks(N)), dim3(kGicBlock), lds, ctx->stream, S, Z, h1,
                     h2, ldh, N, (int)K, (int)d, logits);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_gic_disc_backward(s3grl_context* ctx, int64_t N, int64_t d, int64_t K, const float* S,
                                     const float* Z, const float* h1, const float* h2, int64_t ldh,
                                     const float* grad_logits, float* g_h1, float* g_h2, int64_t ldg, float* g_pre,
                                     float* partial, float* gS, float* gZ) {
  if (!ctx || !S || !Z || !h1 || !h2 || !grad_logits || !g_h1 || !g_h2 || !g_pre || !partial || !gS || !gZ ||
      ldh < d || ldg < d)
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (!gic_shape_ok(N, d, K)) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t chunks = gic_chunks(N);
  const size_t lds = sizeof(float) * 2 * kGicChunk * gic_lda((int)K);
  if (s3grl_status st = gic_set_lds(gic_disc_bwd_kernel, lds, ctx->device, g_disc_bwd_lds)) return st;
  hipLaunchKernelGGL(gic_disc_bwd_kernel, dim3((unsigned)chunks), dim3(kGicBlock), lds, ctx->stream, S, Z, h1, h2, ldh,
                     grad_logits, N, (int)K, (int)d, g_h1, g_h2, ldg, g_pre, gS, partial);
  S3GRL_HIP_TRY(hipGetLastError());
  const int64_t M = K * d;
  hipLaunchKernelGGL(gic_sum_parts_kernel, dim3((unsigned)((M + kGicBlock - 1) / kGicBlock)), dim3(kGicBlock), 0,
                     ctx->stream, partial, chunks, M, gZ);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

}  // extern "C"
