// SIGNNet, the consumer of the engine's rows (reference models.py:301-383, twin harness.SIGNNetTwin), trained on gfx950:
//   operator_diff  h = dropout(BN1(ELU(x·W1ᵀ + b1))) over the ΣR_b rows of a mini-batch of B links, read IN PLACE from
//                  the engine's row store [ΣR_all, in_width] through row_ptr (no gathered copy)
//   centre pool    z = h[first] ⊙ h[first + 1] (| mean or sum of the link's remaining rows), as s3grl_pool.hip
//   link_pred_mlp  Linear(ch·H -> H), ReLU, BN2 over the B links, dropout, Linear(H -> 1); BCE with logits, mean over B
//   dense torch.optim.Adam over W1 b1 γ1 β1 W2 b2 γ2 β2 W3 b3
// One optimiser step is four launches, stream-ordered, every one a grid of column slices of kTC hidden columns:
//
//   signnet_front_kernel     its columns of x·W1ᵀ + b1 for every row of the batch (kept: `pre`), BN1's batch statistics
//                            and running-stat update, ELU, BN1, hashed dropout (kept: `h`), and its columns of the
//                            pooled z: all of it is local to a hidden column
//   signnet_head_kernel      its columns of z·W2ᵀ + b2 (kept: `pre2`), ReLU, BN2's statistics and running-stat update,
//                            dropout (kept: `d2`), and its partial of every link's logit Σ_j W3[j]·d2[b, j]
//   signnet_head_back_kernel folds the logit partials in slice order, BCE and d loss / d logit; for its columns the
//                            dropout, BN2 and ReLU backward (kept: `dpre2`) and Adam on b2, γ2, β2, W3 (b3: slice 0)
//   signnet_back_kernel      for its columns k of h: dz[:, k] = dpre2·W2[:, k], then dW2[:, k] = dpre2ᵀ·z[:, k] and Adam
//                            on that column of W2 (no other workgroup reads it); the pool's adjoint, dropout, BN1 and
//                            ELU backward for its columns of every row; dW1[k, :] = dAᵀ·x and Adam on W1[k, :], b1, γ1, β1
//
// The logit needs every column of the head (a grid-wide dependency), so the head is two launches and not one; a head in
// ONE workgroup would run its three B × ch·H × H products on one CU.  dx is never formed.  No float atomics, no host
// round trip; every sum has a fixed order: a lane's stride over k then a butterfly, a thread's stride over rows then
// a tree in LDS, partials in slice order.  Draws (initial values, the epoch's permutation, both dropout masks) are
// counter-based hashes of (seed, epoch, step, stream, index), the generator of s3grl_train.hpp with a 3-bit stream field.
// signnet_score_front_kernel / signnet_score_kernel are the same forward through the same device functions in eval
// mode (running statistics, no dropout) over tiles of 64 links.
// signnet_{front,head,head_back,back}_runs_kernel are the four step kernels with a second grid dimension, the run: up to
// 16 trainers of one shape take a step in the same four launches (s3grl_signnetruns_fit_epoch), each through the
// device functions of the lone kernels and therefore bit-identical to a lone run of its seed.
#include "s3grl_internal.hpp"
#include "s3grl_train.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

namespace s3grl {
namespace {

constexpr int kSnBlock = 1024;             // 16 wavefronts: a launch is only ⌈H / kTC⌉ workgroups, one per CU
constexpr int kTC = 4;                  // hidden columns per workgroup
constexpr int kNQ = kSnBlock / kTC;     // threads per column in the column-local passes
constexpr int kRW = 4;                  // rows a wavefront carries per pass over k
constexpr int kSnLoads = 8;             // independent loads a thread keeps in flight in the backward's row loops
constexpr int kSnTile = 64;             // links per score tile; rows per tile of the dW1 pass; the largest batch
constexpr int kSnMaxHidden = 256, kSnMaxBatch = kSnTile, kSnMaxWidth = 1 << 20;
constexpr float kBnEps = 1e-5f, kBnMomentum = 0.1f;                     // nn.BatchNorm1d defaults
static_assert(kRW * kTC <= 64 && kSnBlock % kTC == 0 && (kNQ & (kNQ - 1)) == 0 && kSnTile % kSnLoads == 0 &&
                  kSnMaxHidden % 64 == 0,
              "column slice layout");
enum SnStream : uint32_t { kSnMask1 = 0, kSnMask2 = 1, kSnPermute = 2, kSnInit = 3 };

// The ten tensors live in one array, each at an offset that is a multiple of 4 floats (float4 loads of W1 and W2 rows).
struct SnShape {
  int H, IW, CH, ZW, mode;   // hidden, in_width, 1 or 2 pooled blocks, ZW = CH·H the head's input width, pool mode
  int oW1, ob1, og1, obe1, oW2, ob2, og2, obe2, oW3, ob3, P;
};
enum { kPoolNone = 0, kPoolMean = 1, kPoolSum = 2 };

SnShape sn_shape_of(int H, int IW, int mode) {
  SnShape s{};
  s.H = H;
  s.IW = IW;
  s.mode = mode;
  s.CH = mode == kPoolNone ? 1 : 2;
  s.ZW = s.CH * H;
  int o = 0;
  auto take = [&](int n) {
    const int at = o;
    o = (o + n + 3) & ~3;
    return at;
  };
  s.oW1 = take(H * IW);
  s.ob1 = take(H);
  s.og1 = take(H);
  s.obe1 = take(H);
  s.oW2 = take(H * s.ZW);
  s.ob2 = take(H);
  s.og2 = take(H);
  s.obe2 = take(H);
  s.oW3 = take(H);
  s.ob3 = take(1);
  s.P = o;
  return s;
}

// the links of a step: ids[b] (the caller's list or a slice of the epoch's permutation), or the consecutive ids of a
// score tile
struct SnBatch {
  const int64_t* row_ptr;
  const int32_t* ids;   // null: id0 + b
  int64_t id0, total;   // score: the first link of tile 0 and the number of links
  int B;
};

// dropout of element (row, column): the caller's mask uint8 [rows, H] or the hash
__device__ __forceinline__ bool sn_keeps(const DropMask& m, int H, int64_t row, int col) {
  return m.given ? m.given[row * H + col] != 0 : draw(m.key, (uint64_t)row, (uint64_t)col) >= m.drop_below;
}

__device__ __forceinline__ float sn_elu(float x) { return x > 0.f ? x : expm1f(x); }

// what a step draws, for the teacher-forcing hook: ids [B], mask1 uint8 [R, H], mask2 uint8 [B, H]; each may be null
__global__ void sn_export_kernel(int H, int B, int64_t R, const int32_t* __restrict__ perm, DropMask m1, DropMask m2,
                                 int32_t* __restrict__ ids, uint8_t* __restrict__ mask1, uint8_t* __restrict__ mask2) {
  const int64_t t = (int64_t)blockIdx.x * kSnBlock + threadIdx.x;
  if (ids && t < B) ids[t] = perm[t];
  if (mask1 && t < R * H) mask1[t] = sn_keeps(m1, H, t / H, (int)(t % H)) ? 1 : 0;
  if (mask2 && t < (int64_t)B * H) mask2[t] = sn_keeps(m2, H, t / H, (int)(t % H)) ? 1 : 0;
}

// ---- shared device functions -------------------------------------------------------------------------------
// lptr[b] = the batch-local index of link b's first row (lptr[B] = ΣR_b), start[b] its row in the store.
__device__ __forceinline__ void sn_load_batch(const SnBatch& bt, int* lptr, int64_t* start) {
  const int t = threadIdx.x;
  if (t < bt.B) {
    const int64_t id = bt.ids ? (int64_t)bt.ids[t] : bt.id0 + t;
    const int64_t s = bt.row_ptr[id];
    start[t] = s;
    lptr[t + 1] = (int)(bt.row_ptr[id + 1] - s);
  }
  __syncthreads();
  if (t == 0) {
    lptr[0] = 0;
    for (int b = 0; b < bt.B; ++b) lptr[b + 1] += lptr[b];
  }
  __syncthreads();
}
__device__ __forceinline__ int sn_link_of(const int* lptr, int B, int r) {   // the last b with lptr[b] <= r
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lptr[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ int64_t sn_store_row(const int* lptr, const int64_t* start, int B, int r) {
  const int b = sn_link_of(lptr, B, r);
  return start[b] + (r - lptr[b]);
}

template <int V>
struct SnVec;
template <>
struct SnVec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
};
template <>
struct SnVec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  }
};

// out[r · ldo + c] = bias[c] + Σ_k row(r)[k] · W[c · K + k] for r < R, c < ncols <= kTC: the columns of one slice of
// an x·Wᵀ product whose both operands are contiguous in k.  A wavefront carries kRW rows at a time; its lanes stride
// over k (V floats per load), each with kRW · kTC accumulators, then a butterfly.  K % V == 0 and 16-byte aligned
// rows when V = 4.  `row(r)` gives the address of row r.
template <int V, typename Row>
__device__ __forceinline__ void sn_gemm_nt(int R, int K, Row row, const float* __restrict__ W, int ncols,
                                           const float* __restrict__ bias, float* out, int64_t ldo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* wp[kTC];
#pragma unroll
  for (int c = 0; c < kTC; ++c) wp[c] = W + (int64_t)min(c, ncols - 1) * K;
  for (int g = wave; g * kRW < R; g += kSnBlock / 64) {
    const float* xp[kRW];
#pragma unroll
    for (int i = 0; i < kRW; ++i) xp[i] = row(min(g * kRW + i, R - 1));
    float acc[kRW][kTC];
#pragma unroll
    for (int i = 0; i < kRW; ++i)
#pragma unroll
      for (int c = 0; c < kTC; ++c) acc[i][c] = 0.f;
    for (int k = lane * V; k < K; k += 64 * V) {
      SnVec<V> xv[kRW], wv[kTC];
#pragma unroll
      for (int i = 0; i < kRW; ++i) xv[i].load(xp[i] + k);
#pragma unroll
      for (int c = 0; c < kTC; ++c) wv[c].load(wp[c] + k);
#pragma unroll
      for (int i = 0; i < kRW; ++i)
#pragma unroll
        for (int c = 0; c < kTC; ++c)
#pragma unroll
          for (int v = 0; v < V; ++v) acc[i][c] = fmaf(xv[i].v[v], wv[c].v[v], acc[i][c]);
    }
    float mine = 0.f;
#pragma unroll
    for (int i = 0; i < kRW; ++i)
#pragma unroll
      for (int c = 0; c < kTC; ++c) {
        float a = acc[i][c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == i * kTC + c) mine = a;
      }
    const int i = lane / kTC, c = lane % kTC, r = g * kRW + i;
    if (lane < kRW * kTC && r < R && c < ncols) out[(int64_t)r * ldo + c] = mine + bias[c];
  }
}

// the sums over the kNQ threads of a column (thread t: column t % kTC, rank t / kTC) of N values at once, in a fixed
// tree order; every thread of the column gets them in v.  red: kSnRed floats of LDS.
constexpr int kSnSums = 3, kSnRed = kSnSums * kSnBlock;
template <int N>
__device__ __forceinline__ void sn_col_sums(float (&v)[N], float* red) {
  static_assert(N <= kSnSums, "red holds kSnSums values per thread");
  const int t = threadIdx.x, c = t % kTC, q = t / kTC;
#pragma unroll
  for (int i = 0; i < N; ++i) red[i * kSnBlock + t] = v[i];
  __syncthreads();
  for (int s = kNQ / 2; s > 0; s >>= 1) {
    if (q < s)
#pragma unroll
      for (int i = 0; i < N; ++i) red[i * kSnBlock + t] += red[i * kSnBlock + t + s * kTC];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = red[i * kSnBlock + c];
  __syncthreads();
}
__device__ __forceinline__ float sn_col_sum(float v, float* red) {
  float a[1] = {v};
  sn_col_sums(a, red);
  return a[0];
}

// ---- forward -----------------------------------------------------------------------------------------------
// Columns c0 .. c0 + kTC of operator_diff and of the pool for the links of `bt`.  TRAIN: batch statistics over the
// batch's rows, running-stat update, dropout; pre [R, H], h [R, H], z [B, ZW] are the step's buffers.  Eval: the
// running statistics, h indexed by the store's rows (pre is not kept), z by link id.
template <int V, bool TRAIN>
__device__ __forceinline__ void sn_front(const SnShape& s, SnBatch bt, const float* __restrict__ x,
                                         const float* __restrict__ P, float* __restrict__ rstats, const DropMask& mk,
                                         float* __restrict__ pre, float* __restrict__ h, float* __restrict__ z,
                                         float* __restrict__ save) {
  __shared__ int lptr[kSnMaxBatch + 1];
  __shared__ int64_t start[kSnMaxBatch];
  __shared__ float red[kSnRed];
  sn_load_batch(bt, lptr, start);
  const int B = bt.B, H = s.H, R = lptr[B];
  const int c0 = blockIdx.x * kTC, ncols = min(kTC, H - c0);
  const int64_t base = TRAIN ? 0 : start[0];   // the links of a score tile are consecutive in the store
  float* preb = (TRAIN ? pre : h) + base * H;
  float* hb = h + base * H;
  const int IW = s.IW;
  sn_gemm_nt<V>(R, IW, [&](int r) { return x + sn_store_row(lptr, start, B, r) * IW; }, P + s.oW1 + (int64_t)c0 * IW,
                ncols, P + s.ob1 + c0, preb + c0, H);
  __syncthreads();
  const int c = threadIdx.x % kTC, q = threadIdx.x / kTC, col = c0 + c;
  const bool ok = c < ncols;
  float mean, invstd;
  if (TRAIN) {
    float sum = 0.f;
    if (ok)
      for (int r = q; r < R; r += kNQ) sum += sn_elu(preb[(int64_t)r * H + col]);
    mean = sn_col_sum(sum, red) / (float)R;
    float ss = 0.f;
    if (ok)
      for (int r = q; r < R; r += kNQ) {
        const float d = sn_elu(preb[(int64_t)r * H + col]) - mean;
        ss = fmaf(d, d, ss);
      }
    const float var = sn_col_sum(ss, red) / (float)R;
    invstd = 1.f / sqrtf(var + kBnEps);
    if (ok && q == 0) {
      save[col] = mean;
      save[H + col] = invstd;
      rstats[col] = (1.f - kBnMomentum) * rstats[col] + kBnMomentum * mean;
      rstats[H + col] = (1.f - kBnMomentum) * rstats[H + col] + kBnMomentum * (var * ((float)R / (float)(R - 1)));
    }
  } else {
    mean = ok ? rstats[col] : 0.f;
    invstd = ok ? 1.f / sqrtf(rstats[H + col] + kBnEps) : 0.f;
  }
  if (ok) {
    const float gamma = P[s.og1 + col], beta = P[s.obe1 + col];
    for (int r = q; r < R; r += kNQ) {
      float v = (sn_elu(preb[(int64_t)r * H + col]) - mean) * invstd * gamma + beta;
      if (TRAIN) v = sn_keeps(mk, H, r, col) ? v * mk.scale : 0.f;
      hb[(int64_t)r * H + col] = v;
    }
  }
  __syncthreads();
  if (ok) {   // the pool of s3grl_pool.hip, one column at a time
    const int64_t zbase = TRAIN ? 0 : bt.id0;
    for (int b = q; b < B; b += kNQ) {
      const float* hs = hb + (int64_t)lptr[b] * H + col;
      float* zo = z + (zbase + b) * s.ZW + col;
      zo[0] = hs[0] * hs[H];
      if (s.CH == 2) {
        const int extra = lptr[b + 1] - lptr[b] - 2;
        const float scale = (s.mode == kPoolMean && extra > 0) ? 1.0f / (float)extra : 1.0f;
        float acc = 0.f;
        for (int e = 0; e < extra; ++e) acc += hs[(int64_t)(2 + e) * H];
        zo[H] = acc * scale;
      }
    }
  }
}

// Columns c0 .. of link_pred_mlp up to its dropout for B links whose pooled rows are zr [B, ZW]: tile [kSnTile, kTC]
// (LDS) gets d2; thread t < B returns its link's partial logit Σ_c W3[c0 + c] · d2[t, c].  Ends with a barrier
// between the last read of `tile` and the return.
template <int V, bool TRAIN>
__device__ __forceinline__ float sn_head_cols(const SnShape& s, int B, const float* __restrict__ zr,
                                              const float* __restrict__ P, float* __restrict__ rstats,
                                              const DropMask& mk, int c0, float* tile, float* red,
                                              float* __restrict__ pre2, float* __restrict__ d2,
                                              float* __restrict__ save) {
  const int H = s.H, ZW = s.ZW, ncols = min(kTC, H - c0);
  sn_gemm_nt<V>(B, ZW, [&](int r) { return zr + (int64_t)r * ZW; }, P + s.oW2 + (int64_t)c0 * ZW, ncols,
                P + s.ob2 + c0, tile, kTC);
  __syncthreads();
  const int c = threadIdx.x % kTC, q = threadIdx.x / kTC, col = c0 + c;
  const bool ok = c < ncols;
  float mean, invstd;
  if (TRAIN) {
    float sum = 0.f;
    if (ok)
      for (int b = q; b < B; b += kNQ) sum += fmaxf(tile[b * kTC + c], 0.f);
    mean = sn_col_sum(sum, red) / (float)B;
    float ss = 0.f;
    if (ok)
      for (int b = q; b < B; b += kNQ) {
        const float d = fmaxf(tile[b * kTC + c], 0.f) - mean;
        ss = fmaf(d, d, ss);
      }
    const float var = sn_col_sum(ss, red) / (float)B;
    invstd = 1.f / sqrtf(var + kBnEps);
    if (ok && q == 0) {
      save[2 * H + col] = mean;
      save[3 * H + col] = invstd;
      float* rs = rstats + 2 * H;
      rs[col] = (1.f - kBnMomentum) * rs[col] + kBnMomentum * mean;
      rs[H + col] = (1.f - kBnMomentum) * rs[H + col] + kBnMomentum * (var * ((float)B / (float)(B - 1)));
    }
  } else {
    mean = ok ? rstats[2 * H + col] : 0.f;
    invstd = ok ? 1.f / sqrtf(rstats[3 * H + col] + kBnEps) : 0.f;
  }
  if (ok) {
    const float gamma = P[s.og2 + col], beta = P[s.obe2 + col];
    for (int b = q; b < B; b += kNQ) {
      const float p2 = tile[b * kTC + c];
      float v = (fmaxf(p2, 0.f) - mean) * invstd * gamma + beta;
      if (TRAIN) {
        v = sn_keeps(mk, H, b, col) ? v * mk.scale : 0.f;
        pre2[b * H + col] = p2;
        d2[b * H + col] = v;
      }
      tile[b * kTC + c] = v;
    }
  }
  __syncthreads();
  float part = 0.f;
  if ((int)threadIdx.x < B)
    for (int cc = 0; cc < ncols; ++cc) part = fmaf(P[s.oW3 + c0 + cc], tile[threadIdx.x * kTC + cc], part);
  __syncthreads();
  return part;
}

template <int V>
__global__ __launch_bounds__(kSnBlock) void signnet_front_kernel(SnShape s, SnBatch bt, const float* __restrict__ x,
                                                                 const float* __restrict__ P,
                                                                 float* __restrict__ rstats, DropMask mk,
                                                                 float* __restrict__ pre, float* __restrict__ h,
                                                                 float* __restrict__ z, float* __restrict__ save) {
  sn_front<V, true>(s, bt, x, P, rstats, mk, pre, h, z, save);
}

// grid (column slices, link tiles): tile y takes the links id0 + 64·y ..
template <int V>
__global__ __launch_bounds__(kSnBlock) void signnet_score_front_kernel(SnShape s, SnBatch bt,
                                                                       const float* __restrict__ x,
                                                                       const float* __restrict__ P,
                                                                       float* __restrict__ rstats,
                                                                       float* __restrict__ h, float* __restrict__ z) {
  bt.id0 += (int64_t)blockIdx.y * kSnTile;
  bt.B = (int)min((int64_t)kSnTile, bt.total - bt.id0);
  sn_front<V, false>(s, bt, x, P, rstats, DropMask{nullptr, 0, 0, 1.f}, nullptr, h, z, nullptr);
}

// plog [slices, kSnTile]: slice 0's partial carries b3, so that folding in slice order gives the logit
template <int V>
__global__ __launch_bounds__(kSnBlock) void signnet_head_kernel(SnShape s, int B, const float* __restrict__ z,
                                                                const float* __restrict__ P,
                                                                float* __restrict__ rstats, DropMask mk,
                                                                float* __restrict__ pre2, float* __restrict__ d2,
                                                                float* __restrict__ save, float* __restrict__ plog) {
  __shared__ float tile[kSnTile * kTC];
  __shared__ float red[kSnRed];
  const float part = sn_head_cols<V, true>(s, B, z, P, rstats, mk, blockIdx.x * kTC, tile, red, pre2, d2, save);
  if ((int)threadIdx.x < B) plog[blockIdx.x * kSnTile + threadIdx.x] = blockIdx.x == 0 ? P[s.ob3] + part : part;
}

// one workgroup per tile of 64 links walks every column slice; the same fold order as training
template <int V>
__global__ __launch_bounds__(kSnBlock) void signnet_score_kernel(SnShape s, int64_t id0, int64_t total,
                                                                 const float* __restrict__ z,
                                                                 const float* __restrict__ P,
                                                                 float* __restrict__ rstats, float* __restrict__ out) {
  __shared__ float tile[kSnTile * kTC];
  __shared__ float red[kSnRed];
  const int64_t first = id0 + (int64_t)blockIdx.x * kSnTile;
  const int B = (int)min((int64_t)kSnTile, total - first);
  float logit = 0.f;
  for (int c0 = 0; c0 < s.H; c0 += kTC) {
    const float part = sn_head_cols<V, false>(s, B, z + first * s.ZW, P, rstats, DropMask{nullptr, 0, 0, 1.f}, c0, tile,
                                              red, nullptr, nullptr, nullptr);
    logit = c0 == 0 ? P[s.ob3] + part : logit + part;
  }
  if ((int)threadIdx.x < B) out[first + threadIdx.x] = logit;
}

// ---- backward ----------------------------------------------------------------------------------------------
// BCE with logits, mean over B: max(o, 0) - o·y + log1p(exp(-|o|)); d / d o = (sigmoid(o) - y) / B
__device__ __forceinline__ void sn_head_back(const SnShape& s, int B, const int32_t* __restrict__ ids,
                                             const float* __restrict__ y, int nslices,
                                             const float* __restrict__ plog, const float* __restrict__ pre2,
                                             const float* __restrict__ d2, const float* __restrict__ save,
                                             const DropMask& mk, const AdamStep& k, float* __restrict__ P,
                                             float* __restrict__ M, float* __restrict__ Vv,
                                             float* __restrict__ dpre2, float* __restrict__ loss_out) {
  __shared__ float dl[kSnTile];
  __shared__ double lterm[kSnTile];
  __shared__ float red[kSnRed];
  __shared__ float pl[(kSnMaxHidden + kTC - 1) / kTC * kSnTile];
  const int t = threadIdx.x, H = s.H;
  for (int e = t; e < nslices * kSnTile; e += kSnBlock) pl[e] = (e % kSnTile) < B ? plog[e] : 0.f;
  __syncthreads();
  if (t < B) {
    float o = pl[t];
    for (int sl = 1; sl < nslices; ++sl) o += pl[sl * kSnTile + t];
    const float yb = y[ids[t]];
    lterm[t] = (double)(fmaxf(o, 0.f) - o * yb + log1pf(expf(-fabsf(o))));
    dl[t] = (1.f / (1.f + expf(-o)) - yb) / (float)B;
  }
  __syncthreads();
  if (blockIdx.x == 0 && t == 0) {
    double sum = 0.0;
    float db3 = 0.f;
    for (int b = 0; b < B; ++b) {
      sum += lterm[b];
      db3 += dl[b];
    }
    if (loss_out) loss_out[0] = (float)(sum / (double)B);
    adam_update(k, db3, P + s.ob3, M + s.ob3, Vv + s.ob3);   // b3 was read by the head kernel alone
  }
  const int c0 = blockIdx.x * kTC, ncols = min(kTC, H - c0);
  const int c = t % kTC, q = t / kTC, col = c0 + c;
  const bool ok = c < ncols;
  const float mean = ok ? save[2 * H + col] : 0.f, invstd = ok ? save[3 * H + col] : 0.f;
  const float w3 = ok ? P[s.oW3 + col] : 0.f, gamma = ok ? P[s.og2 + col] : 0.f;
  float sb = 0.f, sg = 0.f, sw = 0.f;
  if (ok)
    for (int b = q; b < B; b += kNQ) {
      const float dbn = sn_keeps(mk, H, b, col) ? dl[b] * w3 * mk.scale : 0.f;
      const float xhat = (fmaxf(pre2[b * H + col], 0.f) - mean) * invstd;
      sb += dbn;
      sg = fmaf(dbn, xhat, sg);
      sw = fmaf(dl[b], d2[b * H + col], sw);
    }
  float sums[3] = {sb, sg, sw};
  sn_col_sums(sums, red);
  const float dbeta = sums[0], dgamma = sums[1], dw3 = sums[2];
  float sp = 0.f;
  if (ok)
    for (int b = q; b < B; b += kNQ) {
      const float p2 = pre2[b * H + col];
      const float dbn = sn_keeps(mk, H, b, col) ? dl[b] * w3 * mk.scale : 0.f;
      const float xhat = (fmaxf(p2, 0.f) - mean) * invstd;
      const float dr = gamma * invstd * (dbn - dbeta / (float)B - xhat * (dgamma / (float)B));
      const float dp = p2 > 0.f ? dr : 0.f;
      dpre2[b * H + col] = dp;
      sp += dp;
    }
  const float db2 = sn_col_sum(sp, red);
  if (ok && q == 0) {   // every read of these four by this workgroup lies before sn_col_sum's barriers
    adam_update(k, db2, P + s.ob2 + col, M + s.ob2 + col, Vv + s.ob2 + col);
    adam_update(k, dgamma, P + s.og2 + col, M + s.og2 + col, Vv + s.og2 + col);
    adam_update(k, dbeta, P + s.obe2 + col, M + s.obe2 + col, Vv + s.obe2 + col);
    adam_update(k, dw3, P + s.oW3 + col, M + s.oW3 + col, Vv + s.oW3 + col);
  }
}

__global__ __launch_bounds__(kSnBlock) void signnet_head_back_kernel(SnShape s, int B, const int32_t* __restrict__ ids,
                                                                     const float* __restrict__ y, int nslices,
                                                                     const float* __restrict__ plog,
                                                                     const float* __restrict__ pre2,
                                                                     const float* __restrict__ d2,
                                                                     const float* __restrict__ save, DropMask mk,
                                                                     AdamStep k, float* __restrict__ P,
                                                                     float* __restrict__ M, float* __restrict__ Vv,
                                                                     float* __restrict__ dpre2,
                                                                     float* __restrict__ loss_out) {
  sn_head_back(s, B, ids, y, nslices, plog, pre2, d2, save, mk, k, P, M, Vv, dpre2, loss_out);
}

// `pre` [R, H] comes in as operator_diff's pre-activations and leaves as dA = d loss / d them (column by column, in
// place: an element is read and written by one thread).
template <int V>
__device__ __forceinline__ void sn_back(const SnShape& s, SnBatch bt, const float* __restrict__ x, const DropMask& mk,
                                        const AdamStep& k, float* __restrict__ P, float* __restrict__ M,
                                        float* __restrict__ Vv, float* __restrict__ pre, const float* __restrict__ h,
                                        const float* __restrict__ z, const float* __restrict__ dpre2,
                                        const float* __restrict__ save) {
  __shared__ int lptr[kSnMaxBatch + 1];
  __shared__ int64_t start[kSnMaxBatch];
  __shared__ int64_t rowbase[kSnTile];
  __shared__ float red[kSnRed];
  __shared__ float dzs[2][kSnTile * kTC], zs[2][kSnTile * kTC];
  __shared__ float das[kSnTile * kTC];
  sn_load_batch(bt, lptr, start);
  const int t = threadIdx.x, B = bt.B, H = s.H, ZW = s.ZW, IW = s.IW, R = lptr[B];
  const int c0 = blockIdx.x * kTC, ncols = min(kTC, H - c0);
  const int c = t % kTC, q = t / kTC, col = c0 + c;
  const bool ok = c < ncols;
  // dz[:, col (+ H)] = dpre2 · W2[:, col (+ H)]: a wavefront per link; lane l holds the rows j = l, l + 64, .. of
  // this slice of W2 in registers, sums its j ascending, then a butterfly
  {
    constexpr int kJ = kSnMaxHidden / 64;
    const int lane = t & 63, wave = t >> 6;
    float w2[2][kJ][kTC];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
      for (int i = 0; i < kJ; ++i)
#pragma unroll
        for (int cc = 0; cc < kTC; ++cc) {
          const int j = lane + 64 * i;
          w2[ch][i][cc] = (ch < s.CH && j < H && cc < ncols) ? P[s.oW2 + (int64_t)j * ZW + ch * H + c0 + cc] : 0.f;
        }
    for (int b = wave; b < B; b += kSnBlock / 64) {
      float d[kJ];
#pragma unroll
      for (int i = 0; i < kJ; ++i) d[i] = lane + 64 * i < H ? dpre2[b * H + lane + 64 * i] : 0.f;
#pragma unroll
      for (int ch = 0; ch < 2; ++ch)
#pragma unroll
        for (int cc = 0; cc < kTC; ++cc) {
          float acc = 0.f;
#pragma unroll
          for (int i = 0; i < kJ; ++i) acc = fmaf(d[i], w2[ch][i][cc], acc);
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
          if (lane == 0) dzs[ch][b * kTC + cc] = acc;
        }
    }
    for (int e = t; e < kSnTile * kTC; e += kSnBlock) {   // zero past B, past the slice and without a pooled block
      const int b = e / kTC, cc = e % kTC;
      for (int ch = 0; ch < 2; ++ch)
        zs[ch][e] = (ch < s.CH && b < B && cc < ncols) ? z[(int64_t)b * ZW + ch * H + c0 + cc] : 0.f;
    }
  }
  __syncthreads();
  // dW2[:, col (+ H)] = dpre2ᵀ · z[:, col (+ H)], b ascending; these columns of W2 are this workgroup's alone
  if (ok)
    for (int j = q; j < H; j += kNQ) {
      float g[2] = {0.f, 0.f};
      for (int b0 = 0; b0 < B; b0 += kSnLoads) {   // kSnLoads loads in flight
        float d[kSnLoads];
#pragma unroll
        for (int u = 0; u < kSnLoads; ++u) d[u] = b0 + u < B ? dpre2[(b0 + u) * H + j] : 0.f;
#pragma unroll
        for (int u = 0; u < kSnLoads; ++u) {
          g[0] = fmaf(d[u], zs[0][(b0 + u) * kTC + c], g[0]);
          g[1] = fmaf(d[u], zs[1][(b0 + u) * kTC + c], g[1]);
        }
      }
      for (int ch = 0; ch < s.CH; ++ch) {
        const int64_t at = s.oW2 + (int64_t)j * ZW + ch * H + col;
        adam_update(k, g[ch], P + at, M + at, Vv + at);
      }
    }
  // the pool's adjoint (s3grl_pool.hip), dropout, BN1 and ELU backward for this column of every row
  const float mean = ok ? save[col] : 0.f, invstd = ok ? save[H + col] : 0.f, gamma = ok ? P[s.og1 + col] : 0.f;
  auto dbn_of = [&](int r) {
    const int b = sn_link_of(lptr, B, r), off = r - lptr[b];
    float dh;
    if (off == 0) {
      dh = dzs[0][b * kTC + c] * h[(int64_t)(r + 1) * H + col];
    } else if (off == 1) {
      dh = dzs[0][b * kTC + c] * h[(int64_t)(r - 1) * H + col];
    } else if (s.CH == 2) {
      const int extra = lptr[b + 1] - lptr[b] - 2;
      dh = dzs[1][b * kTC + c] * (s.mode == kPoolMean ? 1.0f / (float)extra : 1.0f);
    } else {
      dh = 0.f;
    }
    return sn_keeps(mk, H, r, col) ? dh * mk.scale : 0.f;
  };
  float sb = 0.f, sg = 0.f;
  if (ok)
    for (int r = q; r < R; r += kNQ) {
      const float dbn = dbn_of(r);
      const float xhat = (sn_elu(pre[(int64_t)r * H + col]) - mean) * invstd;
      sb += dbn;
      sg = fmaf(dbn, xhat, sg);
    }
  float sums[2] = {sb, sg};
  sn_col_sums(sums, red);
  const float dbeta = sums[0], dgamma = sums[1];
  float sp = 0.f;
  if (ok)
    for (int r = q; r < R; r += kNQ) {
      const float p = pre[(int64_t)r * H + col];
      const float xhat = (sn_elu(p) - mean) * invstd;
      const float da = gamma * invstd * (dbn_of(r) - dbeta / (float)R - xhat * (dgamma / (float)R));
      const float dp = p > 0.f ? da : da * expf(p);
      pre[(int64_t)r * H + col] = dp;
      sp += dp;
    }
  const float db1 = sn_col_sum(sp, red);   // (its barriers also publish dA to the workgroup)
  if (ok && q == 0) {
    adam_update(k, db1, P + s.ob1 + col, M + s.ob1 + col, Vv + s.ob1 + col);
    adam_update(k, dgamma, P + s.og1 + col, M + s.og1 + col, Vv + s.og1 + col);
    adam_update(k, dbeta, P + s.obe1 + col, M + s.obe1 + col, Vv + s.obe1 + col);
  }
  // dW1[col, :] = Σ_r dA[r, col] · x[r, :], r ascending: threads own V consecutive k, rows come in tiles of 64
  for (int k0 = 0; k0 < IW; k0 += kSnBlock * V) {
    const int kk = k0 + t * V;
    const bool active = kk < IW;
    float acc[kTC][V];
#pragma unroll
    for (int cc = 0; cc < kTC; ++cc)
#pragma unroll
      for (int v = 0; v < V; ++v) acc[cc][v] = 0.f;
    for (int r0 = 0; r0 < R; r0 += kSnTile) {
      __syncthreads();
      const int nr = min(kSnTile, R - r0);
      if (t < nr) rowbase[t] = sn_store_row(lptr, start, B, r0 + t) * IW;
      for (int e = t; e < kSnTile * kTC; e += kSnBlock) {
        const int rr = e / kTC, cc = e % kTC;
        das[e] = (rr < nr && cc < ncols) ? pre[(int64_t)(r0 + rr) * H + c0 + cc] : 0.f;
      }
      __syncthreads();
      if (active)
        for (int rr = 0; rr < nr; rr += kSnLoads) {   // das is 0 past nr; a row past it re-reads the tile's first
          SnVec<V> xv[kSnLoads];
#pragma unroll
          for (int u = 0; u < kSnLoads; ++u) xv[u].load(x + rowbase[rr + u < nr ? rr + u : 0] + kk);
#pragma unroll
          for (int u = 0; u < kSnLoads; ++u)
#pragma unroll
            for (int cc = 0; cc < kTC; ++cc)
#pragma unroll
              for (int v = 0; v < V; ++v) acc[cc][v] = fmaf(das[(rr + u) * kTC + cc], xv[u].v[v], acc[cc][v]);
        }
    }
    if (active)
#pragma unroll
      for (int cc = 0; cc < kTC; ++cc)
        if (cc < ncols)
#pragma unroll
          for (int v = 0; v < V; ++v) {
            const int64_t at = s.oW1 + (int64_t)(c0 + cc) * IW + kk + v;
            adam_update(k, acc[cc][v], P + at, M + at, Vv + at);
          }
  }
}

template <int V>
__global__ __launch_bounds__(kSnBlock) void signnet_back_kernel(SnShape s, SnBatch bt, const float* __restrict__ x,
                                                                DropMask mk, AdamStep k, float* __restrict__ P,
                                                                float* __restrict__ M, float* __restrict__ Vv,
                                                                float* __restrict__ pre, const float* __restrict__ h,
                                                                const float* __restrict__ z,
                                                                const float* __restrict__ dpre2,
                                                                const float* __restrict__ save) {
  sn_back<V>(s, bt, x, mk, k, P, M, Vv, pre, h, z, dpre2, save);
}

// ---- a group of runs ---------------------------------------------------------------------------------------
// The four step kernels with a second grid dimension, the run: workgroup (x, y) does for member y of the group exactly
// what workgroup x of the lone kernel does for a lone trainer, through the same device functions, so every member stays
// bit-identical to a lone run of its seed.  The runs share the store, the step's offset into the permutation and the
// batch size; nothing is reduced across runs.
constexpr int kSnMaxRuns = 16;
// what stays put for the life of a group: a row per member in device memory, rewritten when a buffer regrows
struct SnRunTable {
  float *P, *M, *V, *rstats, *save, *pre, *h, *z, *pre2, *d2, *dpre2, *plog;
  const int32_t* perm;    // the epoch's permutation; a step's ids start at perm + step · batch_size
  uint32_t drop_below;    // DropMask's two constants of the member's dropout
  float scale;
};
// what changes with every step, by value in the kernel arguments: 40 bytes a run, 640 in all
struct SnRunsStep {
  uint64_t key1[kSnMaxRuns], key2[kSnMaxRuns];   // the mask keys of operator_diff and of link_pred_mlp
  AdamStep k[kSnMaxRuns];
};
static_assert(sizeof(SnRunTable) == 13 * sizeof(void*) + 8, "a row without padding: the host compares rows as bytes");
static_assert(sizeof(SnRunsStep) == 40 * kSnMaxRuns && sizeof(SnRunsStep) + sizeof(SnShape) + 128 <= 1024,
              "the argument block stays well under 4 KB");

template <int V>
__global__ __launch_bounds__(kSnBlock) void signnet_front_runs_kernel(SnShape s, const int64_t* __restrict__ row_ptr,
                                                                      int64_t at, int B, const float* __restrict__ x,
                                                                      const SnRunTable* __restrict__ table,
                                                                      SnRunsStep step) {
  const SnRunTable g = table[blockIdx.y];
  const DropMask mk{nullptr, step.key1[blockIdx.y], g.drop_below, g.scale};
  sn_front<V, true>(s, SnBatch{row_ptr, g.perm + at, 0, 0, B}, x, g.P, g.rstats, mk, g.pre, g.h, g.z, g.save);
}

template <int V>
__global__ __launch_bounds__(kSnBlock) void signnet_head_runs_kernel(SnShape s, int B,
                                                                     const SnRunTable* __restrict__ table,
                                                                     SnRunsStep step) {
  __shared__ float tile[kSnTile * kTC];
  __shared__ float red[kSnRed];
  const SnRunTable g = table[blockIdx.y];
  const DropMask mk{nullptr, step.key2[blockIdx.y], g.drop_below, g.scale};
  const float part =
      sn_head_cols<V, true>(s, B, g.z, g.P, g.rstats, mk, blockIdx.x * kTC, tile, red, g.pre2, g.d2, g.save);
  if ((int)threadIdx.x < B) g.plog[blockIdx.x * kSnTile + threadIdx.x] = blockIdx.x == 0 ? g.P[s.ob3] + part : part;
}

// loss_out [runs, loss_stride]: run y writes loss_out[y · loss_stride]
__global__ __launch_bounds__(kSnBlock) void signnet_head_back_runs_kernel(SnShape s, int B, int64_t at,
                                                                          const float* __restrict__ y, int nslices,
                                                                          const SnRunTable* __restrict__ table,
                                                                          SnRunsStep step, float* __restrict__ loss_out,
                                                                          int64_t loss_stride) {
  const SnRunTable g = table[blockIdx.y];
  const DropMask mk{nullptr, step.key2[blockIdx.y], g.drop_below, g.scale};
  const AdamStep k = step.k[blockIdx.y];
  sn_head_back(s, B, g.perm + at, y, nslices, g.plog, g.pre2, g.d2, g.save, mk, k, g.P, g.M, g.V, g.dpre2,
               loss_out ? loss_out + (int64_t)blockIdx.y * loss_stride : nullptr);
}

template <int V>
__global__ __launch_bounds__(kSnBlock) void signnet_back_runs_kernel(SnShape s, const int64_t* __restrict__ row_ptr,
                                                                     int64_t at, int B, const float* __restrict__ x,
                                                                     const SnRunTable* __restrict__ table,
                                                                     SnRunsStep step) {
  const SnRunTable g = table[blockIdx.y];
  const DropMask mk{nullptr, step.key1[blockIdx.y], g.drop_below, g.scale};
  const AdamStep k = step.k[blockIdx.y];
  sn_back<V>(s, SnBatch{row_ptr, g.perm + at, 0, 0, B}, x, mk, k, g.P, g.M, g.V, g.pre, g.h, g.z, g.dpre2, g.save);
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

struct s3grl_signnet {
  s3grl_context* ctx = nullptr;
  SnShape shape{};
  double dropout = 0.0;
  uint32_t seed = 0;
  int64_t steps = 0;             // Adam's step count
  int64_t tracked[2] = {0, 0};   // num_batches_tracked of BN1 and BN2
  float *P = nullptr, *M = nullptr, *V = nullptr;   // [shape.P] parameters and Adam's moments
  float* rstats = nullptr;       // [4, H] running mean and var of BN1, then of BN2
  float* save = nullptr;         // [4, H] a step's batch mean and 1 / std of BN1, then of BN2
  // per-step buffers
  int64_t cap_rows = 0;
  float *pre = nullptr, *h = nullptr;   // [cap_rows, H]
  uint8_t* given_mask1 = nullptr;       // [cap_rows, H] a teacher-forced step's masks
  uint8_t* given_mask2 = nullptr;       // [kSnMaxBatch, H]
  int32_t* given_ids = nullptr;         // [kSnMaxBatch]
  float *z = nullptr, *pre2 = nullptr, *d2 = nullptr, *dpre2 = nullptr, *plog = nullptr;
  // score buffers (grown on demand)
  int64_t cap_score_rows = 0, cap_score_links = 0;
  float *sh = nullptr, *sz = nullptr;
  // the epoch's permutation
  int64_t cap_perm = 0, perm_epoch = -1, perm_size = -1;
  int32_t* perm = nullptr;
  uint64_t *keys_a = nullptr, *keys_b = nullptr;
  SortScratch sort;
  std::vector<int64_t> host_ptr;   // the last checked row_ptr
  // the operand table of the groups this handle has led as member 0 (s3grl_signnetruns_fit_epoch)
  SnRunTable* group_table = nullptr;     // [kSnMaxRuns] device
  std::vector<SnRunTable> group_rows;    // what group_table holds
};

namespace {

void sn_free(s3grl_signnet* t) {
  for (void* p : {(void*)t->P, (void*)t->M, (void*)t->V, (void*)t->rstats, (void*)t->save, (void*)t->pre, (void*)t->h,
                  (void*)t->given_mask1, (void*)t->given_mask2, (void*)t->given_ids, (void*)t->z, (void*)t->pre2,
                  (void*)t->d2, (void*)t->dpre2, (void*)t->plog, (void*)t->sh, (void*)t->sz, (void*)t->perm,
                  (void*)t->keys_a, (void*)t->keys_b, (void*)t->group_table, t->sort.tmp})
    if (p) (void)hipFree(p);
}

// four streams, a 3-bit stream field: the width is part of every draw (s3grl_train.hpp)
uint64_t sn_key(const s3grl_signnet* t, int64_t epoch, int64_t step, SnStream stream) {
  return stream_key<3>(t->seed, epoch, step, stream);
}

int sn_slices(int H) { return (H + kTC - 1) / kTC; }

DropMask sn_mask_of(const s3grl_signnet* t, const uint8_t* given, uint64_t key) {
  return drop_mask(t->dropout, given, key);
}

s3grl_status sn_not_implemented(const char* what) {
  set_last_error(what);
  return S3GRL_ERR_NOT_IMPLEMENTED;
}

s3grl_status sn_check_shape(int64_t hidden, int64_t in_width, int64_t batch) {
  if (hidden < 1 || in_width < 1 || batch < 1) return S3GRL_ERR_INVALID_ARGUMENT;
  if (hidden > kSnMaxHidden) return sn_not_implemented("signnet: hidden above 256");
  if (in_width > kSnMaxWidth) return sn_not_implemented("signnet: in_width above 1048576");
  if (batch > kSnMaxBatch) return sn_not_implemented("signnet: batch_size above 64");
  return S3GRL_OK;
}

// float4 loads along k need rows of a multiple of 4 floats on a 16-byte boundary
int sn_vec(int64_t width, const void* base) { return width % 4 == 0 && ((uintptr_t)base & 15) == 0 ? 4 : 1; }

// row_ptr int64 [L + 1] device -> t->host_ptr, checked: non-decreasing from >= 0, every link two rows or more (its
// two centre rows), the last entry inside the store.  Waits for the device.
s3grl_status sn_check_row_ptr(s3grl_signnet* t, const int64_t* row_ptr, int64_t L, int64_t num_rows, const char* what) {
  t->host_ptr.resize((size_t)L + 1);
  S3GRL_HIP_TRY(hipMemcpyAsync(t->host_ptr.data(), row_ptr, t->host_ptr.size() * sizeof(int64_t),
                               hipMemcpyDeviceToHost, t->ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
  const std::vector<int64_t>& p = t->host_ptr;
  bool good = p[0] >= 0 && p[(size_t)L] <= num_rows;
  for (int64_t i = 0; good && i < L; ++i) good = p[(size_t)i + 1] - p[(size_t)i] >= 2;
  if (!good) {
    set_last_error(std::string(what) + ": row_ptr must start at >= 0, give every link at least its two centre rows "
                                       "and end inside rows");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  return S3GRL_OK;
}

// no batch of an epoch has more rows than the batch_size largest links together
int64_t sn_batch_rows_cap(const std::vector<int64_t>& ptr, int64_t num_links, int64_t batch_size) {
  std::vector<int64_t> cnt((size_t)num_links);
  for (int64_t i = 0; i < num_links; ++i) cnt[(size_t)i] = ptr[(size_t)i + 1] - ptr[(size_t)i];
  const size_t top = (size_t)std::min(batch_size, num_links);
  std::partial_sort(cnt.begin(), cnt.begin() + top, cnt.end(), std::greater<int64_t>());
  int64_t cap = 0;
  for (size_t i = 0; i < top; ++i) cap += cnt[i];
  return cap;
}

s3grl_status sn_ensure_rows(s3grl_signnet* t, int64_t rows) {
  if (rows <= t->cap_rows) return S3GRL_OK;
  if (rows >= (int64_t(1) << 31)) return sn_not_implemented("signnet: 2^31 or more rows in one batch");
  S3GRL_HIP_TRY(hipStreamSynchronize(t->ctx->stream));   // the old buffers may still be in use
  const size_t n = (size_t)rows * t->shape.H;
  S3GRL_TRY(regrow(&t->pre, n));
  S3GRL_TRY(regrow(&t->h, n));
  S3GRL_TRY(regrow(&t->given_mask1, n));
  t->cap_rows = rows;
  return S3GRL_OK;
}

s3grl_status sn_ensure_perm(s3grl_signnet* t, int64_t epoch, int64_t L) {
  if (t->perm_epoch == epoch && t->perm_size == L) return S3GRL_OK;
  hipStream_t st = t->ctx->stream;
  if (L > t->cap_perm) {
    S3GRL_HIP_TRY(hipStreamSynchronize(st));
    S3GRL_TRY(regrow(&t->perm, (size_t)L));
    S3GRL_TRY(regrow(&t->keys_a, (size_t)L));
    S3GRL_TRY(regrow(&t->keys_b, (size_t)L));
    t->cap_perm = L;
  }
  t->perm_epoch = t->perm_size = -1;
  S3GRL_TRY(launch_epoch_perm(t->ctx, sn_key(t, epoch, 0, kSnPermute), L, t->keys_a, t->keys_b, t->sort, t->perm));
  t->perm_epoch = epoch;
  t->perm_size = L;
  return S3GRL_OK;
}

template <int V1, int V2>
s3grl_status sn_launch_step(s3grl_signnet* t, const SnBatch& bt, const float* x, const float* y, const DropMask& m1,
                            const DropMask& m2, const AdamStep& k, float* loss_out) {
  hipStream_t st = t->ctx->stream;
  const SnShape& s = t->shape;
  const int slices = sn_slices(s.H);
  hipLaunchKernelGGL(signnet_front_kernel<V1>, dim3(slices), dim3(kSnBlock), 0, st, s, bt, x, t->P, t->rstats, m1,
                     t->pre, t->h, t->z, t->save);
  S3GRL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(signnet_head_kernel<V2>, dim3(slices), dim3(kSnBlock), 0, st, s, bt.B, t->z, t->P, t->rstats, m2,
                     t->pre2, t->d2, t->save, t->plog);
  S3GRL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(signnet_head_back_kernel, dim3(slices), dim3(kSnBlock), 0, st, s, bt.B, bt.ids, y, slices,
                     t->plog, t->pre2, t->d2, t->save, m2, k, t->P, t->M, t->V, t->dpre2, loss_out);
  S3GRL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(signnet_back_kernel<V1>, dim3(slices), dim3(kSnBlock), 0, st, s, bt, x, m1, k, t->P, t->M, t->V,
                     t->pre, t->h, t->z, t->dpre2, t->save);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

// one optimiser step on the links ids[0 .. B) (device), every id and row_ptr already checked
s3grl_status sn_run_step(s3grl_signnet* t, const float* x, const int64_t* row_ptr, const float* y, const int32_t* ids,
                         int64_t B, const DropMask& m1, const DropMask& m2, double lr, float* loss_out) {
  t->steps += 1;
  t->tracked[0] += 1;
  t->tracked[1] += 1;
  const AdamStep k = adam_step(lr, t->steps);
  const SnBatch bt{row_ptr, ids, 0, 0, (int)B};
  const int v1 = sn_vec(t->shape.IW, x), v2 = sn_vec(t->shape.ZW, nullptr);
  if (v1 == 4) return v2 == 4 ? sn_launch_step<4, 4>(t, bt, x, y, m1, m2, k, loss_out)
                              : sn_launch_step<4, 1>(t, bt, x, y, m1, m2, k, loss_out);
  return v2 == 4 ? sn_launch_step<1, 4>(t, bt, x, y, m1, m2, k, loss_out)
                 : sn_launch_step<1, 1>(t, bt, x, y, m1, m2, k, loss_out);
}

template <int V1, int V2>
s3grl_status sn_launch_runs_step(s3grl_signnet* lead, int R, const int64_t* row_ptr, int64_t at, int B, const float* x,
                                 const float* y, const SnRunsStep& step, float* loss_out, int64_t loss_stride) {
  hipStream_t st = lead->ctx->stream;
  const SnShape& s = lead->shape;
  const int slices = sn_slices(s.H);
  const dim3 grid(slices, R), block(kSnBlock);
  const SnRunTable* table = lead->group_table;
  hipLaunchKernelGGL(signnet_front_runs_kernel<V1>, grid, block, 0, st, s, row_ptr, at, B, x, table, step);
  S3GRL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(signnet_head_runs_kernel<V2>, grid, block, 0, st, s, B, table, step);
  S3GRL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(signnet_head_back_runs_kernel, grid, block, 0, st, s, B, at, y, slices, table, step, loss_out,
                     loss_stride);
  S3GRL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(signnet_back_runs_kernel<V1>, grid, block, 0, st, s, row_ptr, at, B, x, table, step);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

// The lead's device table <- a row per member; copied (and waited for) only when a row differs from what it holds.
s3grl_status sn_ensure_group_table(s3grl_signnet* lead, s3grl_signnet* const* members, int R) {
  std::vector<SnRunTable> rows((size_t)R);
  for (int r = 0; r < R; ++r) {
    const s3grl_signnet* m = members[r];
    const DropMask d = sn_mask_of(m, nullptr, 0);
    rows[(size_t)r] = SnRunTable{m->P,  m->M,    m->V,     m->rstats, m->save,      m->pre,  m->h, m->z,
                                 m->pre2, m->d2, m->dpre2, m->plog,   m->perm, d.drop_below, d.scale};
  }
  if (lead->group_table && lead->group_rows.size() == rows.size() &&
      std::memcmp(rows.data(), lead->group_rows.data(), rows.size() * sizeof(SnRunTable)) == 0)   // (no padding)
    return S3GRL_OK;
  hipStream_t st = lead->ctx->stream;
  lead->group_rows.clear();
  if (!lead->group_table) S3GRL_TRY(regrow(&lead->group_table, (size_t)kSnMaxRuns));
  S3GRL_HIP_TRY(hipMemcpyAsync(lead->group_table, rows.data(), rows.size() * sizeof(SnRunTable), hipMemcpyHostToDevice,
                               st));
  S3GRL_HIP_TRY(hipStreamSynchronize(st));   // `rows` goes out of scope
  lead->group_rows = std::move(rows);
  return S3GRL_OK;
}

s3grl_status sn_check_batch(int64_t B) {
  if (B < 2) {
    set_last_error("signnet: a training batch needs two links or more (BatchNorm)");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (B > kSnMaxBatch) return sn_not_implemented("signnet: batch_size above 64");
  return S3GRL_OK;
}

// the ten tensors in state order: (offset in the padded array, count)
void sn_tensors(const SnShape& s, int off[10], int cnt[10]) {
  const int o[10] = {s.oW1, s.ob1, s.og1, s.obe1, s.oW2, s.ob2, s.og2, s.obe2, s.oW3, s.ob3};
  const int n[10] = {s.H * s.IW, s.H, s.H, s.H, s.H * s.ZW, s.H, s.H, s.H, s.H, 1};
  for (int i = 0; i < 10; ++i) off[i] = o[i], cnt[i] = n[i];
}

}  // namespace

extern "C" {

s3grl_status s3grl_signnet_layout(int32_t hidden, int64_t in_width, int32_t batch, int32_t pooled, int32_t* out) {
  if (!out) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_TRY(sn_check_shape(hidden, in_width, batch));
  out[0] = kTC;
  out[1] = sn_slices(hidden);
  out[2] = kRW;
  out[3] = in_width % 4 == 0 ? 4 : 1;
  out[4] = 64 * out[3];
  out[5] = ((pooled ? 2 : 1) * hidden) % 4 == 0 ? 4 : 1;
  out[6] = kSnTile;
  out[7] = kSnTile;
  return S3GRL_OK;
}

s3grl_status s3grl_signnet_create(s3grl_context* ctx, const s3grl_signnet_cfg* cfg, s3grl_signnet** out) {
  if (!ctx || !cfg || !out || !(cfg->dropout >= 0.0) || !(cfg->dropout < 1.0) || cfg->pool_mode < 0)
    return S3GRL_ERR_INVALID_ARGUMENT;
  for (int32_t r : cfg->reserved)
    if (r) return S3GRL_ERR_INVALID_ARGUMENT;
  if (cfg->pool_mode > kPoolSum) return sn_not_implemented("signnet: only the pools none / mean / sum are fused");
  S3GRL_TRY(sn_check_shape(cfg->hidden, cfg->in_width, 2));
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  auto* t = new s3grl_signnet();
  t->ctx = ctx;
  t->shape = sn_shape_of(cfg->hidden, (int)cfg->in_width, cfg->pool_mode);
  t->dropout = cfg->dropout;
  t->seed = cfg->seed;
  const SnShape& s = t->shape;
  const size_t P = (size_t)s.P, BH = (size_t)kSnMaxBatch * s.H;
  auto fail = [&](s3grl_status st) {
    sn_free(t);
    delete t;
    return st;
  };
  s3grl_status r = S3GRL_OK;
  if ((r = regrow(&t->P, P)) || (r = regrow(&t->M, P)) || (r = regrow(&t->V, P)) ||
      (r = regrow(&t->rstats, (size_t)4 * s.H)) || (r = regrow(&t->save, (size_t)4 * s.H)) ||
      (r = regrow(&t->given_mask2, BH)) || (r = regrow(&t->given_ids, (size_t)kSnMaxBatch)) ||
      (r = regrow(&t->z, (size_t)kSnMaxBatch * s.ZW)) || (r = regrow(&t->pre2, BH)) ||
      (r = regrow(&t->d2, BH)) || (r = regrow(&t->dpre2, BH)) ||
      (r = regrow(&t->plog, (size_t)sn_slices(s.H) * kSnTile)))
    return fail(r);
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemsetAsync(t->P, 0, P * sizeof(float), st);
  if (e == hipSuccess) e = hipMemsetAsync(t->M, 0, P * sizeof(float), st);
  if (e == hipSuccess) e = hipMemsetAsync(t->V, 0, P * sizeof(float), st);
  if (e == hipSuccess) e = hipMemsetAsync(t->rstats, 0, (size_t)4 * s.H * sizeof(float), st);
  if (e == hipSuccess) {   // torch's defaults: Linear uniform in ±1/sqrt(fan_in) (weight and bias), γ = 1, β = 0,
                           // running mean 0 and var 1
    int off[10], cnt[10];
    sn_tensors(s, off, cnt);
    const double fan[10] = {(double)s.IW, (double)s.IW, 0, 0, (double)s.ZW, (double)s.ZW, 0, 0, (double)s.H, (double)s.H};
    for (int i = 0; i < 10 && r == S3GRL_OK; ++i) {
      if (i == 2 || i == 6)
        r = launch_fill(ctx, 1.f, cnt[i], t->P + off[i]);
      else if (fan[i] > 0)
        r = launch_init_uniform(ctx, sn_key(t, 0, i, kSnInit), (float)(1.0 / std::sqrt(fan[i])), cnt[i], t->P + off[i]);
    }
    for (int b = 0; b < 2 && r == S3GRL_OK; ++b) r = launch_fill(ctx, 1.f, s.H, t->rstats + (2 * b + 1) * s.H);
    if (r != S3GRL_OK) return fail(r);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    set_last_error(std::string("signnet create: ") + hipGetErrorString(e));
    return fail(e == hipErrorOutOfMemory ? S3GRL_ERR_OUT_OF_MEMORY : S3GRL_ERR_HIP);
  }
  *out = t;
  return S3GRL_OK;
}

s3grl_status s3grl_signnet_fit_epoch(s3grl_signnet* t, int64_t epoch, const float* rows, int64_t num_rows,
                                     const int64_t* row_ptr, const float* y, int64_t num_links, int64_t batch_size,
                                     double lr, float* step_loss) {
  if (!t || !rows || !row_ptr || !y || epoch < 0 || num_links < 2 || num_links >= (int64_t(1) << 31) || num_rows < 0 ||
      bad_lr(lr))
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_TRY(sn_check_batch(batch_size));
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(sn_check_row_ptr(t, row_ptr, num_links, num_rows, "signnet fit_epoch"));
  S3GRL_TRY(sn_ensure_rows(t, sn_batch_rows_cap(t->host_ptr, num_links, batch_size)));
  S3GRL_TRY(sn_ensure_perm(t, epoch, num_links));
  // harness.train_and_evaluate's batching: range(0, L - 1, batch_size), so a last batch of one link is skipped
  const int64_t steps = (num_links - 1 + batch_size - 1) / batch_size;
  for (int64_t i = 0; i < steps; ++i) {
    const int64_t B = std::min(batch_size, num_links - i * batch_size);
    S3GRL_TRY(sn_run_step(t, rows, row_ptr, y, t->perm + i * batch_size, B,
                          sn_mask_of(t, nullptr, sn_key(t, epoch, i, kSnMask1)),
                          sn_mask_of(t, nullptr, sn_key(t, epoch, i, kSnMask2)), lr,
                          step_loss ? step_loss + i : nullptr));
  }
  return S3GRL_OK;
}

s3grl_status s3grl_signnetruns_fit_epoch(s3grl_signnet* const* members, int32_t num_members, int64_t epoch,
                                           const float* rows, int64_t num_rows, const int64_t* row_ptr, const float* y,
                                           int64_t num_links, int64_t batch_size, const double* lr,
                                           float* step_loss) {
  if (!members || num_members < 1 || !lr) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_members > kSnMaxRuns) return sn_not_implemented("signnet: a group of more than 16 members");
  if (!rows || !row_ptr || !y || epoch < 0 || num_links < 2 || num_links >= (int64_t(1) << 31) || num_rows < 0)
    return S3GRL_ERR_INVALID_ARGUMENT;
  const int R = num_members;
  for (int r = 0; r < R; ++r) {
    if (!members[r] || bad_lr(lr[r])) return S3GRL_ERR_INVALID_ARGUMENT;
    const SnShape &a = members[0]->shape, &b = members[r]->shape;
    if (members[r]->ctx != members[0]->ctx || a.H != b.H || a.IW != b.IW || a.mode != b.mode) {
      set_last_error("signnet group: members must share the context, hidden, in_width and the pool mode");
      return S3GRL_ERR_INVALID_ARGUMENT;
    }
    for (int q = 0; q < r; ++q)
      if (members[q] == members[r]) {
        set_last_error("signnet group: the same handle appears twice");
        return S3GRL_ERR_INVALID_ARGUMENT;
      }
  }
  S3GRL_TRY(sn_check_batch(batch_size));
  s3grl_signnet* lead = members[0];
  S3GRL_HIP_TRY(hipSetDevice(lead->ctx->device));
  S3GRL_TRY(sn_check_row_ptr(lead, row_ptr, num_links, num_rows, "signnet fit_epoch_group"));   // once for the group
  const int64_t cap = sn_batch_rows_cap(lead->host_ptr, num_links, batch_size);
  for (int r = 0; r < R; ++r) S3GRL_TRY(sn_ensure_rows(members[r], cap));
  for (int r = 0; r < R; ++r) S3GRL_TRY(sn_ensure_perm(members[r], epoch, num_links));
  S3GRL_TRY(sn_ensure_group_table(lead, members, R));
  const int64_t steps = (num_links - 1 + batch_size - 1) / batch_size;
  const int v1 = sn_vec(lead->shape.IW, rows), v2 = sn_vec(lead->shape.ZW, nullptr);
  for (int64_t i = 0; i < steps; ++i) {
    const int B = (int)std::min(batch_size, num_links - i * batch_size);
    SnRunsStep step{};
    for (int r = 0; r < R; ++r) {   // the counters advance as in sn_run_step
      s3grl_signnet* m = members[r];
      m->steps += 1;
      m->tracked[0] += 1;
      m->tracked[1] += 1;
      step.key1[r] = sn_key(m, epoch, i, kSnMask1);
      step.key2[r] = sn_key(m, epoch, i, kSnMask2);
      step.k[r] = adam_step(lr[r], m->steps);
    }
    const int64_t at = i * batch_size;
    float* loss = step_loss ? step_loss + i : nullptr;
    s3grl_status st;
    if (v1 == 4)
      st = v2 == 4 ? sn_launch_runs_step<4, 4>(lead, R, row_ptr, at, B, rows, y, step, loss, steps)
                   : sn_launch_runs_step<4, 1>(lead, R, row_ptr, at, B, rows, y, step, loss, steps);
    else
      st = v2 == 4 ? sn_launch_runs_step<1, 4>(lead, R, row_ptr, at, B, rows, y, step, loss, steps)
                   : sn_launch_runs_step<1, 1>(lead, R, row_ptr, at, B, rows, y, step, loss, steps);
    S3GRL_TRY(st);
  }
  return S3GRL_OK;
}

s3grl_status s3grl_signnet_draws(s3grl_signnet* t, int64_t epoch, int64_t step, int64_t num_links, int64_t batch_size,
                                 int32_t* link_ids, uint8_t* mask1, int64_t mask1_rows, uint8_t* mask2) {
  if (!t || epoch < 0 || step < 0 || num_links < 2 || num_links >= (int64_t(1) << 31) || mask1_rows < 0 ||
      (mask1_rows >= (int64_t(1) << 31)))
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_TRY(sn_check_batch(batch_size));
  if (step * batch_size >= num_links - 1) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(sn_ensure_perm(t, epoch, num_links));
  const int64_t B = std::min(batch_size, num_links - step * batch_size);
  const int H = t->shape.H;
  const int64_t threads = std::max<int64_t>(std::max<int64_t>(B, mask1 ? mask1_rows : 0) * H, 1);
  hipLaunchKernelGGL(sn_export_kernel, dim3(grid_of(threads, kSnBlock)), dim3(kSnBlock), 0, t->ctx->stream, H, (int)B,
                     mask1_rows, t->perm + step * batch_size,
                     sn_mask_of(t, nullptr, sn_key(t, epoch, step, kSnMask1)),
                     sn_mask_of(t, nullptr, sn_key(t, epoch, step, kSnMask2)), link_ids, mask1, mask2);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_signnet_step(s3grl_signnet* t, const float* rows, int64_t num_rows, const int64_t* row_ptr,
                                const float* y, int64_t num_links, const int32_t* link_ids, int64_t batch,
                                const uint8_t* mask1, const uint8_t* mask2, double lr, float* loss) {
  if (!t || !rows || !row_ptr || !y || !link_ids || num_links < 2 || num_links >= (int64_t(1) << 31) || num_rows < 0 ||
      bad_lr(lr))
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_TRY(sn_check_batch(batch));
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  hipStream_t st = t->ctx->stream;
  int32_t ids[kSnMaxBatch];
  S3GRL_HIP_TRY(hipMemcpyAsync(ids, link_ids, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  S3GRL_TRY(sn_check_row_ptr(t, row_ptr, num_links, num_rows, "signnet step"));   // (waits for the ids too)
  int64_t R = 0;
  for (int64_t b = 0; b < batch; ++b) {
    if (ids[b] < 0 || ids[b] >= num_links) {
      set_last_error("signnet step: a link id outside [0, L)");
      return S3GRL_ERR_INVALID_ARGUMENT;
    }
    R += t->host_ptr[(size_t)ids[b] + 1] - t->host_ptr[(size_t)ids[b]];
  }
  S3GRL_TRY(sn_ensure_rows(t, R));
  const size_t H = (size_t)t->shape.H;
  S3GRL_HIP_TRY(hipMemcpyAsync(t->given_ids, link_ids, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  if (mask1) S3GRL_HIP_TRY(hipMemcpyAsync(t->given_mask1, mask1, (size_t)R * H, hipMemcpyDeviceToDevice, st));
  if (mask2) S3GRL_HIP_TRY(hipMemcpyAsync(t->given_mask2, mask2, (size_t)batch * H, hipMemcpyDeviceToDevice, st));
  // without masks the step draws its own, keyed by Adam's step count in an epoch no fit_epoch reaches
  const int64_t free_epoch = (int64_t(1) << 40) + t->steps;
  return sn_run_step(t, rows, row_ptr, y, t->given_ids, batch,
                     sn_mask_of(t, mask1 ? t->given_mask1 : nullptr, sn_key(t, free_epoch, 0, kSnMask1)),
                     sn_mask_of(t, mask2 ? t->given_mask2 : nullptr, sn_key(t, free_epoch, 0, kSnMask2)),
                     lr, loss);
}

s3grl_status s3grl_signnet_score(s3grl_signnet* t, const float* rows, int64_t num_rows, const int64_t* row_ptr,
                                 int64_t num_links, float* out) {
  if (!t || num_links < 0 || num_links >= (int64_t(1) << 31) || num_rows < 0 ||
      (num_links > 0 && (!rows || !row_ptr || !out)))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_links == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(sn_check_row_ptr(t, row_ptr, num_links, num_rows, "signnet score"));
  hipStream_t st = t->ctx->stream;
  const SnShape& s = t->shape;
  if (num_rows > t->cap_score_rows) {   // h of every row of the store, indexed as the store is
    S3GRL_TRY(regrow(&t->sh, (size_t)num_rows * s.H));
    t->cap_score_rows = num_rows;
  }
  if (num_links > t->cap_score_links) {
    S3GRL_TRY(regrow(&t->sz, (size_t)num_links * s.ZW));
    t->cap_score_links = num_links;
  }
  const int slices = sn_slices(s.H), v1 = sn_vec(s.IW, rows), v2 = sn_vec(s.ZW, nullptr);
  const int64_t tiles = (num_links + kSnTile - 1) / kSnTile;
  for (int64_t t0 = 0; t0 < tiles; t0 += 32768) {   // (a grid's second dimension ends at 65535)
    const unsigned nt = (unsigned)std::min<int64_t>(32768, tiles - t0);
    const SnBatch bt{row_ptr, nullptr, t0 * kSnTile, num_links, 0};
    if (v1 == 4)
      hipLaunchKernelGGL(signnet_score_front_kernel<4>, dim3(slices, nt), dim3(kSnBlock), 0, st, s, bt, rows, t->P,
                         t->rstats, t->sh, t->sz);
    else
      hipLaunchKernelGGL(signnet_score_front_kernel<1>, dim3(slices, nt), dim3(kSnBlock), 0, st, s, bt, rows, t->P,
                         t->rstats, t->sh, t->sz);
    S3GRL_HIP_TRY(hipGetLastError());
    if (v2 == 4)
      hipLaunchKernelGGL(signnet_score_kernel<4>, dim3(nt), dim3(kSnBlock), 0, st, s, t0 * kSnTile, num_links, t->sz,
                         t->P, t->rstats, out);
    else
      hipLaunchKernelGGL(signnet_score_kernel<1>, dim3(nt), dim3(kSnBlock), 0, st, s, t0 * kSnTile, num_links, t->sz,
                         t->P, t->rstats, out);
    S3GRL_HIP_TRY(hipGetLastError());
  }
  return S3GRL_OK;
}

static s3grl_status sn_state_array(s3grl_signnet* t, int32_t which, float** base, bool* packed) {
  *packed = which < 3;
  switch (which) {
    case 0: *base = t->P; return S3GRL_OK;
    case 1: *base = t->M; return S3GRL_OK;
    case 2: *base = t->V; return S3GRL_OK;
    case 3: *base = t->rstats; return S3GRL_OK;
    default: return S3GRL_ERR_INVALID_ARGUMENT;
  }
}

static s3grl_status sn_state_copy(s3grl_signnet* t, int32_t which, float* user, bool read) {
  float* base = nullptr;
  bool tensors = false;
  S3GRL_TRY(sn_state_array(t, which, &base, &tensors));
  hipStream_t st = t->ctx->stream;
  if (!tensors) {
    const size_t n = (size_t)4 * t->shape.H * sizeof(float);
    S3GRL_HIP_TRY(hipMemcpyAsync(read ? user : base, read ? base : user, n, hipMemcpyDeviceToDevice, st));
    return S3GRL_OK;
  }
  int off[10], cnt[10];
  sn_tensors(t->shape, off, cnt);
  size_t at = 0;
  for (int i = 0; i < 10; ++i) {
    float* mine = base + off[i];
    float* theirs = user + at;
    S3GRL_HIP_TRY(hipMemcpyAsync(read ? theirs : mine, read ? mine : theirs, (size_t)cnt[i] * sizeof(float),
                                 hipMemcpyDeviceToDevice, st));
    at += (size_t)cnt[i];
  }
  return S3GRL_OK;
}

s3grl_status s3grl_signnet_read_state(s3grl_signnet* t, int32_t which, float* out, int64_t* counters) {
  if (!t) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  if (out) S3GRL_TRY(sn_state_copy(t, which, out, true));
  if (counters) counters[0] = t->steps, counters[1] = t->tracked[0], counters[2] = t->tracked[1];
  return S3GRL_OK;
}

s3grl_status s3grl_signnet_write_state(s3grl_signnet* t, int32_t which, const float* in, const int64_t* counters) {
  if (!t) return S3GRL_ERR_INVALID_ARGUMENT;
  if (counters && (counters[0] < 0 || counters[1] < 0 || counters[2] < 0)) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  if (in) S3GRL_TRY(sn_state_copy(t, which, const_cast<float*>(in), false));
  if (counters) t->steps = counters[0], t->tracked[0] = counters[1], t->tracked[1] = counters[2];
  return S3GRL_OK;
}

s3grl_status s3grl_signnet_destroy(s3grl_signnet* t) {
  if (!t) return S3GRL_OK;
  (void)hipSetDevice(t->ctx->device);
  (void)hipStreamSynchronize(t->ctx->stream);
  sn_free(t);
  delete t;
  return S3GRL_OK;
}

}  // extern "C"
