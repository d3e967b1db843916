// Matrix factorisation link prediction (reference baselines/mf.py: a learnable nn.Embedding(N, H), a LinkPredictor MLP
// of L Linear layers over the Hadamard product of the two endpoint rows, dense torch.optim.Adam over both, batches
// of B positive links and B uniform random pairs) on gfx950.  One optimiser step is two launches, stream-ordered:
//
//   mf_pair_kernel    one workgroup per tile of T of the step's 2·B pairs (positives, then negatives): gathers the two
//                     rows, h0 = x[a] ⊙ x[b], the MLP forward with hashed dropout, sigmoid and the loss term in fp32,
//                     the MLP backward.  A tile's activations and the two gradient buffers live in LDS; the predictor
//                     is read through L2.  It writes the step's endpoint list (2·pair + side), the two FINISHED table
//                     terms of every pair (dh0 ⊙ x[b] for endpoint a, dh0 ⊙ x[a] for endpoint b: the update never
//                     reads a table row another workgroup may already have moved), the tile's partial sum of every
//                     predictor gradient and its fp64 loss partials
//   mf_update_kernel  dense Adam.  Table blocks: LPP lanes per row walk the 4·B endpoint list (staged in LDS) in list
//                     order and add the terms of their row, so duplicates and self-pairs add in a fixed order without
//                     a sort; every row gets the Adam update, touched or not.  Predictor blocks: one thread per
//                     parameter folds the tile partials in tile order; one thread folds the loss.
//
// Determinism: no float atomics; every draw (epoch permutation, negative pairs, dropout masks, initial parameters) is
// a counter-based hash of (seed, epoch, step, stream, index), the generator of s3grl_train.hpp with a 3-bit stream
// field.  Lane layout (mf_layout): LPP lanes per pair / table row, the smallest power of two >= H up to 64, each lane
// ceil(H / LPP) <= 2 channels; T = max(256 / LPP, 16) pairs per tile.  LDS rows are padded to an odd stride, so the
// pairs of one wavefront sit on different banks.
#include "s3grl_internal.hpp"
#include "s3grl_train.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace s3grl {
namespace {

constexpr int kMfBlock = 256;
constexpr int kMfMaxHidden = 128, kMfMinLayers = 2, kMfMaxLayers = 4, kMfMaxBatch = 1024;
constexpr int kMfMaxCpl = 2;   // channels per lane: ceil(128 / 64)
enum MfStream : uint32_t { kNegPair = 0, kMask = 1, kPermute = 2, kInitTable = 3, kInitPred = 4, kFreeMask = 5 };

// H channels, L layers; the predictor is one flat array: per layer its weight [out, H] (torch's layout), then its
// bias [out]; out = H but for the last layer's 1.  LPP lanes per pair, T pairs per tile, HS the LDS row stride.
struct MfShape {
  int H, L, LPP, T, HS, P;
};
__host__ __device__ __forceinline__ int w_off(const MfShape& s, int l) { return l * (s.H * s.H + s.H); }
__host__ __device__ __forceinline__ int b_off(const MfShape& s, int l) {
  return w_off(s, l) + (l == s.L - 1 ? s.H : s.H * s.H);
}

MfShape shape_of(int H, int L) {
  MfShape s;
  s.H = H;
  s.L = L;
  s.LPP = 1;
  while (s.LPP < H && s.LPP < 64) s.LPP <<= 1;
  s.T = std::max(kMfBlock / s.LPP, 16);
  s.HS = H | 1;
  s.P = (L - 1) * (H * H + H) + H + 1;
  return s;
}
size_t pair_lds_floats(const MfShape& s, bool train) {
  return (size_t)(s.L + (train ? 2 : 0)) * s.T * s.HS + 5 * (size_t)s.T;
}

// where a step's 2·B pairs come from: the caller's list, or the epoch's permutation of the train links and the hash
struct MfPairs {
  const int32_t* given;   // [2B, 2] or null
  const int32_t* train;   // [E, 2]
  const int32_t* perm;    // the step's B positions in train
  uint64_t kneg;
  int32_t N;
};
__device__ __forceinline__ void pair_of(const MfPairs& s, int i, int B, int& a, int& b) {
  if (s.given) {
    a = s.given[2 * i];
    b = s.given[2 * i + 1];
  } else if (i < B) {
    const int e = s.perm[i];
    a = s.train[2 * e];
    b = s.train[2 * e + 1];
  } else {
    a = (int)below(draw(s.kneg, (uint64_t)(i - B), 0), (uint32_t)s.N);
    b = (int)below(draw(s.kneg, (uint64_t)(i - B), 1), (uint32_t)s.N);
  }
}

// dropout of hidden layer l, channel j of pair i (of the step's 2·B): the caller's mask uint8 [2B, L-1, H] or the hash
__device__ __forceinline__ bool keeps(const DropMask& m, const MfShape& s, int i, int l, int j) {
  const int64_t e = ((int64_t)i * (s.L - 1) + l) * s.H + j;
  return m.given ? m.given[e] != 0 : draw(m.key, (uint64_t)i, (uint64_t)(l * s.H + j)) >= m.drop_below;
}

// what a step draws, for the teacher-forcing hook: pos_idx [B], neg [B, 2], masks uint8 [2B, L-1, H]
__global__ void mf_export_kernel(MfShape s, int B, MfPairs src, DropMask mk, int32_t* __restrict__ pos_idx,
                                 int32_t* __restrict__ neg, uint8_t* __restrict__ masks) {
  const int64_t t = (int64_t)blockIdx.x * kMfBlock + threadIdx.x;
  if (t < B) {
    pos_idx[t] = src.perm[t];
    int a, b;
    pair_of(src, B + (int)t, B, a, b);
    neg[2 * t] = a;
    neg[2 * t + 1] = b;
  }
  const int per = (s.L - 1) * s.H;
  if (t < (int64_t)2 * B * per) {
    const int i = (int)(t / per), r = (int)(t - (int64_t)i * per);
    masks[t] = keeps(mk, s, i, r / s.H, r % s.H) ? 1 : 0;
  }
}

// ---- the predictor forward over one tile -------------------------------------------------------------------
// act [L][T][HS] in LDS: act[0] = x[a] ⊙ x[b], act[l] the output of hidden layer l - 1 (relu, dropout); outv [T] the
// last layer's output.  Pair p of the tile is pair p0 + p of the step; LPP lanes (q = their rank) per pair, G pairs
// at a time.  Ends with a barrier.
template <bool TRAIN>
__device__ __forceinline__ void mf_forward(const MfShape& s, int p0, int np, const float* __restrict__ x,
                                           const float* __restrict__ pred, const int* ia, const int* ib,
                                           const DropMask& mk, float* act, float* outv) {
  const int H = s.H, HS = s.HS, TH = s.T * s.HS;
  const int G = kMfBlock / s.LPP, g = threadIdx.x / s.LPP, q = threadIdx.x % s.LPP;
  for (int p = g; p < np; p += G) {
    const float* xa = x + (int64_t)ia[p] * H;
    const float* xb = x + (int64_t)ib[p] * H;
    for (int k = q; k < H; k += s.LPP) act[p * HS + k] = xa[k] * xb[k];
  }
  __syncthreads();
  for (int l = 0; l < s.L - 1; ++l) {
    const float* __restrict__ W = pred + w_off(s, l);
    const float* __restrict__ bias = pred + b_off(s, l);
    const float* in = act + l * TH;
    float* out = act + (l + 1) * TH;
    for (int p = g; p < np; p += G) {
      for (int j = q; j < H; j += s.LPP) {
        float acc = bias[j];
        for (int k = 0; k < H; ++k) acc = fmaf(W[j * H + k], in[p * HS + k], acc);
        float a = fmaxf(acc, 0.f);
        if (TRAIN) a = keeps(mk, s, p0 + p, l, j) ? a * mk.scale : 0.f;
        out[p * HS + j] = a;
      }
    }
    __syncthreads();
  }
  const float* __restrict__ w = pred + w_off(s, s.L - 1);
  const float* in = act + (s.L - 1) * TH;
  for (int p = g; p < np; p += G) {   // uniform over a pair's lanes: the butterfly stays inside the group
    float acc = 0.f;
    for (int k = q; k < H; k += s.LPP) acc = fmaf(w[k], in[p * HS + k], acc);
    for (int o = s.LPP / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (q == 0) outv[p] = acc + pred[b_off(s, s.L - 1)];
  }
  __syncthreads();
}

// The tile's LDS: lterm double [T] | act [L][T][HS] | (train: da, db [T][HS]) | outv [T] | ia, ib [T]
__global__ __launch_bounds__(kMfBlock) void mf_score_kernel(MfShape s, int64_t npairs, const int32_t* __restrict__ pairs,
                                                            const float* __restrict__ x, const float* __restrict__ pred,
                                                            float* __restrict__ out) {
  extern __shared__ double mf_lds[];
  float* act = reinterpret_cast<float*>(mf_lds) + 2 * s.T;
  float* outv = act + s.L * s.T * s.HS;
  int* ia = reinterpret_cast<int*>(outv + s.T);
  int* ib = ia + s.T;
  const int64_t p0 = (int64_t)blockIdx.x * s.T;
  const int np = (int)min((int64_t)s.T, npairs - p0);
  for (int p = threadIdx.x; p < np; p += kMfBlock) {
    ia[p] = pairs[2 * (p0 + p)];
    ib[p] = pairs[2 * (p0 + p) + 1];
  }
  __syncthreads();
  mf_forward<false>(s, 0, np, x, pred, ia, ib, DropMask{nullptr, 0, 0, 1.f}, act, outv);
  for (int p = threadIdx.x; p < np; p += kMfBlock) out[p0 + p] = sigmoid32(outv[p]);
}

// loss (reference mf.py:53-59): pos -log(s + 1e-15).mean(), d/dout = -s(1-s) / (s + EPS) / B
//                               neg -log(1 - s + 1e-15).mean(), d/dout = s(1-s) / (1 - s + EPS) / B
__global__ __launch_bounds__(kMfBlock) void mf_pair_kernel(MfShape s, int B, MfPairs src, DropMask mk,
                                                           const float* __restrict__ x, const float* __restrict__ pred,
                                                           int32_t* __restrict__ ends, float* __restrict__ terms,
                                                           float* __restrict__ partial, double* __restrict__ lpart) {
  extern __shared__ double mf_lds[];
  const int H = s.H, HS = s.HS, TH = s.T * s.HS, tid = threadIdx.x;
  double* lterm = mf_lds;
  float* act = reinterpret_cast<float*>(mf_lds) + 2 * s.T;
  float* dcur = act + s.L * TH;
  float* dnext = dcur + TH;
  float* gout = dnext + TH;
  int* ia = reinterpret_cast<int*>(gout + s.T);
  int* ib = ia + s.T;
  const int p0 = blockIdx.x * s.T;
  const int np = min(s.T, 2 * B - p0);
  for (int p = tid; p < np; p += kMfBlock) {
    int a, b;
    pair_of(src, p0 + p, B, a, b);
    ia[p] = a;
    ib[p] = b;
    ends[2 * (p0 + p)] = a;
    ends[2 * (p0 + p) + 1] = b;
  }
  __syncthreads();
  mf_forward<true>(s, p0, np, x, pred, ia, ib, mk, act, gout);
  const float inv_b = 1.f / (float)B;
  for (int p = tid; p < np; p += kMfBlock) {
    const float sg = sigmoid32(gout[p]);
    if (p0 + p < B) {
      lterm[p] = (double)-logf(sg + 1e-15f);
      gout[p] = -(sg * (1.f - sg)) / (sg + 1e-15f) * inv_b;
    } else {
      lterm[p] = (double)-logf(1.f - sg + 1e-15f);
      gout[p] = (sg * (1.f - sg)) / (1.f - sg + 1e-15f) * inv_b;
    }
  }
  __syncthreads();
  if (tid == 0) {   // the tile's loss, in pair order
    double sp = 0.0, sn = 0.0;
    for (int p = 0; p < np; ++p) {
      if (p0 + p < B) sp += lterm[p]; else sn += lterm[p];
    }
    lpart[2 * blockIdx.x] = sp;
    lpart[2 * blockIdx.x + 1] = sn;
  }
  float* __restrict__ part = partial + (int64_t)blockIdx.x * s.P;
  const int G = kMfBlock / s.LPP, g = tid / s.LPP, q = tid % s.LPP;
  {   // the last layer [1, H]: its gradient, and d pre of the hidden layer below it
    const int l = s.L - 1;
    const float* in = act + l * TH;
    for (int k = tid; k < H; k += kMfBlock) {
      float acc = 0.f;
      for (int p = 0; p < np; ++p) acc = fmaf(gout[p], in[p * HS + k], acc);
      part[w_off(s, l) + k] = acc;
    }
    if (tid == 0) {
      float acc = 0.f;
      for (int p = 0; p < np; ++p) acc += gout[p];
      part[b_off(s, l)] = acc;
    }
    const float* __restrict__ w = pred + w_off(s, l);
    for (int p = g; p < np; p += G)
      for (int k = q; k < H; k += s.LPP) dcur[p * HS + k] = in[p * HS + k] > 0.f ? w[k] * gout[p] * mk.scale : 0.f;
  }
  __syncthreads();
  for (int l = s.L - 2; l >= 0; --l) {   // dcur = d loss / d pre of layer l, whose input is act[l]
    const float* in = act + l * TH;
    for (int e = tid; e < H * H; e += kMfBlock) {
      const int j = e / H, k = e - j * H;
      float acc = 0.f;
      for (int p = 0; p < np; ++p) acc = fmaf(dcur[p * HS + j], in[p * HS + k], acc);
      part[w_off(s, l) + e] = acc;
    }
    for (int j = tid; j < H; j += kMfBlock) {
      float acc = 0.f;
      for (int p = 0; p < np; ++p) acc += dcur[p * HS + j];
      part[b_off(s, l) + j] = acc;
    }
    const float* __restrict__ W = pred + w_off(s, l);
    for (int p = g; p < np; p += G) {
      for (int k = q; k < H; k += s.LPP) {
        float acc = 0.f;
        for (int j = 0; j < H; ++j) acc = fmaf(W[j * H + k], dcur[p * HS + j], acc);
        if (l > 0) {
          dnext[p * HS + k] = in[p * HS + k] > 0.f ? acc * mk.scale : 0.f;
        } else {   // the finished table terms: endpoint a gets dh0 ⊙ x[b], endpoint b gets dh0 ⊙ x[a]
          const int64_t t0 = (int64_t)2 * (p0 + p) * H + k;
          terms[t0] = acc * x[(int64_t)ib[p] * H + k];
          terms[t0 + H] = acc * x[(int64_t)ia[p] * H + k];
        }
      }
    }
    __syncthreads();
    float* t = dcur;
    dcur = dnext;
    dnext = t;
  }
}

// ---- dense Adam --------------------------------------------------------------------------------------------
// torch.optim.Adam over the table and the predictor: adam_update of s3grl_train.hpp
__global__ __launch_bounds__(kMfBlock) void mf_update_kernel(MfShape s, int64_t N, int nends, int ntiles,
                                                             unsigned tblocks, const int32_t* __restrict__ ends,
                                                             const float* __restrict__ terms,
                                                             const float* __restrict__ partial,
                                                             const double* __restrict__ lpart, double inv_b, AdamStep k,
                                                             float* __restrict__ x, float* __restrict__ xm,
                                                             float* __restrict__ xv, float* __restrict__ pred,
                                                             float* __restrict__ pm, float* __restrict__ pv,
                                                             float* __restrict__ loss_out) {
  extern __shared__ int32_t mf_ends[];
  const int tid = threadIdx.x;
  if (blockIdx.x < tblocks) {
    for (int i = tid; i < nends; i += kMfBlock) mf_ends[i] = ends[i];
    __syncthreads();
    const int q = tid % s.LPP;
    const int64_t u = (int64_t)blockIdx.x * (kMfBlock / s.LPP) + tid / s.LPP;
    if (u >= N) return;
    float acc[kMfMaxCpl] = {0.f, 0.f};
    for (int e = 0; e < nends; ++e) {   // list order: positives then negatives, endpoint a then b
      if (mf_ends[e] != (int32_t)u) continue;
#pragma unroll
      for (int i = 0; i < kMfMaxCpl; ++i) {
        const int c = q + i * s.LPP;
        if (c < s.H) acc[i] += terms[(int64_t)e * s.H + c];
      }
    }
#pragma unroll
    for (int i = 0; i < kMfMaxCpl; ++i) {
      const int c = q + i * s.LPP;
      if (c < s.H) adam_update(k, acc[i], x + u * s.H + c, xm + u * s.H + c, xv + u * s.H + c);
    }
    return;
  }
  const int idx = (int)(blockIdx.x - tblocks) * kMfBlock + tid;
  if (idx < s.P) {
    float g = 0.f;
    for (int t = 0; t < ntiles; ++t) g += partial[(int64_t)t * s.P + idx];
    adam_update(k, g, pred + idx, pm + idx, pv + idx);
  }
  if (blockIdx.x == tblocks && tid == 0 && loss_out) {
    double sp = 0.0, sn = 0.0;
    for (int t = 0; t < ntiles; ++t) {
      sp += lpart[2 * t];
      sn += lpart[2 * t + 1];
    }
    loss_out[0] = (float)(sp * inv_b + sn * inv_b);
  }
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

struct s3grl_mf {
  s3grl_context* ctx = nullptr;
  int64_t N = 0;
  MfShape shape{};
  double dropout = 0.0;
  uint32_t seed = 0;
  int64_t steps = 0;                // Adam's step count
  float *x = nullptr, *xm = nullptr, *xv = nullptr;         // [N, H]
  float *pred = nullptr, *pm = nullptr, *pv = nullptr;      // [P]
  // per-step buffers, sized for the largest batch
  int32_t* ends = nullptr;          // [4 · kMfMaxBatch]
  float* terms = nullptr;           // [4 · kMfMaxBatch, H]
  float* partial = nullptr;         // [tiles, P]
  double* lpart = nullptr;          // [2 · tiles]
  int32_t* given = nullptr;         // [2 · kMfMaxBatch, 2] a teacher-forced step's pairs
  uint8_t* given_masks = nullptr;   // [2 · kMfMaxBatch, L-1, H]
  // the epoch's train links and their permutation (grown on demand)
  int64_t cap_train = 0, num_train = 0;
  int32_t *train = nullptr, *perm = nullptr;
  uint64_t *keys_a = nullptr, *keys_b = nullptr;
  int64_t perm_epoch = -1, perm_size = -1;
  SortScratch sort;
};

namespace {

// six streams, a 3-bit stream field: the width is part of every draw (s3grl_train.hpp)
uint64_t key_of(const s3grl_mf* t, int64_t epoch, int64_t step, MfStream stream) {
  return stream_key<3>(t->seed, epoch, step, stream);
}

void mf_free(s3grl_mf* t) {
  for (void* p : {(void*)t->x, (void*)t->xm, (void*)t->xv, (void*)t->pred, (void*)t->pm, (void*)t->pv, (void*)t->ends,
                  (void*)t->terms, (void*)t->partial, (void*)t->lpart, (void*)t->given, (void*)t->given_masks,
                  (void*)t->train, (void*)t->perm, (void*)t->keys_a, (void*)t->keys_b, t->sort.tmp})
    if (p) (void)hipFree(p);
}

int mf_tiles(const MfShape& s, int64_t B) { return (int)((2 * B + s.T - 1) / s.T); }
size_t mask_count(const MfShape& s, int64_t B) { return (size_t)(2 * B) * (s.L - 1) * s.H; }

DropMask mask_of(const s3grl_mf* t, const uint8_t* given, uint64_t key) { return drop_mask(t->dropout, given, key); }

s3grl_status ensure_train(s3grl_mf* t, int64_t E) {
  if (E > t->cap_train) {
    S3GRL_HIP_TRY(hipStreamSynchronize(t->ctx->stream));   // the old buffers may still be in use
    S3GRL_TRY(regrow(&t->train, (size_t)(2 * E)));
    S3GRL_TRY(regrow(&t->perm, (size_t)E));
    S3GRL_TRY(regrow(&t->keys_a, (size_t)E));
    S3GRL_TRY(regrow(&t->keys_b, (size_t)E));
    t->cap_train = E;
    t->perm_epoch = t->perm_size = -1;
  }
  return S3GRL_OK;
}

s3grl_status ensure_perm(s3grl_mf* t, int64_t epoch, int64_t E) {
  if (t->perm_epoch == epoch && t->perm_size == E) return S3GRL_OK;
  S3GRL_TRY(ensure_train(t, E));
  S3GRL_TRY(launch_epoch_perm(t->ctx, key_of(t, epoch, 0, kPermute), E, t->keys_a, t->keys_b,
                              t->sort, t->perm));
  t->perm_epoch = epoch;
  t->perm_size = E;
  return S3GRL_OK;
}

// pairs int32 [count, 2] device -> checked on the host, every id in [0, N)
s3grl_status check_pairs(const s3grl_mf* t, const int32_t* pairs, int64_t count, const char* what) {
  return check_ids(t->ctx, pairs, 2 * count, t->N, std::string(what) + ": a node outside [0, N)");
}

s3grl_status run_step(s3grl_mf* t, int64_t B, const MfPairs& src, const DropMask& mk, double lr, float* loss_out) {
  hipStream_t st = t->ctx->stream;
  const MfShape& s = t->shape;
  const int tiles = mf_tiles(s, B);
  hipLaunchKernelGGL(mf_pair_kernel, dim3(tiles), dim3(kMfBlock), pair_lds_floats(s, true) * sizeof(float), st, s,
                     (int)B, src, mk, t->x, t->pred, t->ends, t->terms, t->partial, t->lpart);
  S3GRL_HIP_TRY(hipGetLastError());
  t->steps += 1;
  const AdamStep k = adam_step(lr, t->steps);
  const unsigned tblocks = grid_of(t->N, kMfBlock / s.LPP);
  hipLaunchKernelGGL(mf_update_kernel, dim3(tblocks + grid_of(s.P, kMfBlock)), dim3(kMfBlock),
                     (size_t)(4 * B) * sizeof(int32_t), st, s, t->N, (int)(4 * B), tiles, tblocks, t->ends, t->terms,
                     t->partial, t->lpart, 1.0 / (double)B, k, t->x, t->xm, t->xv, t->pred, t->pm, t->pv, loss_out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status check_batch(int64_t B) {
  if (B < 1) return S3GRL_ERR_INVALID_ARGUMENT;
  if (B > kMfMaxBatch) {
    set_last_error("mf: batch_size above 1024");
    return S3GRL_ERR_NOT_IMPLEMENTED;
  }
  return S3GRL_OK;
}

}  // namespace

extern "C" {

s3grl_status s3grl_mf_layout(int32_t hidden, int32_t num_layers, int64_t batch_size, int32_t* out) {
  if (!out || hidden < 1 || num_layers < kMfMinLayers || batch_size < 1) return S3GRL_ERR_INVALID_ARGUMENT;
  if (hidden > kMfMaxHidden || num_layers > kMfMaxLayers || batch_size > kMfMaxBatch) {
    set_last_error("mf: hidden above 128, num_layers above 4 or batch_size above 1024");
    return S3GRL_ERR_NOT_IMPLEMENTED;
  }
  const MfShape s = shape_of(hidden, num_layers);
  out[0] = (s.H + s.LPP - 1) / s.LPP;
  out[1] = s.LPP;
  out[2] = s.T;
  out[3] = mf_tiles(s, batch_size);
  return S3GRL_OK;
}

s3grl_status s3grl_mf_create(s3grl_context* ctx, int64_t num_nodes, const s3grl_mf_cfg* cfg, const float* init_table,
                             const float* init_pred, s3grl_mf** out) {
  if (!ctx || !cfg || !out || num_nodes < 1 || num_nodes >= (int64_t(1) << 31) || cfg->hidden < 1 ||
      cfg->num_layers < kMfMinLayers || !(cfg->dropout >= 0.0) || !(cfg->dropout < 1.0))
    return S3GRL_ERR_INVALID_ARGUMENT;
  for (int32_t r : cfg->reserved)
    if (r) return S3GRL_ERR_INVALID_ARGUMENT;
  if (cfg->hidden > kMfMaxHidden || cfg->num_layers > kMfMaxLayers) {
    set_last_error("mf: hidden above 128 or num_layers above 4");
    return S3GRL_ERR_NOT_IMPLEMENTED;
  }
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  auto* t = new s3grl_mf();
  t->ctx = ctx;
  t->N = num_nodes;
  t->shape = shape_of(cfg->hidden, cfg->num_layers);
  t->dropout = cfg->dropout;
  t->seed = cfg->seed;
  const MfShape& s = t->shape;
  const size_t table = (size_t)num_nodes * s.H, P = (size_t)s.P;
  const size_t tiles = (size_t)mf_tiles(s, kMfMaxBatch);
  auto fail = [&](s3grl_status st) {
    mf_free(t);
    delete t;
    return st;
  };
  s3grl_status r = S3GRL_OK;
  if ((r = regrow(&t->x, table)) || (r = regrow(&t->xm, table)) || (r = regrow(&t->xv, table)) ||
      (r = regrow(&t->pred, P)) || (r = regrow(&t->pm, P)) || (r = regrow(&t->pv, P)) ||
      (r = regrow(&t->ends, (size_t)4 * kMfMaxBatch)) || (r = regrow(&t->terms, (size_t)4 * kMfMaxBatch * s.H)) ||
      (r = regrow(&t->partial, tiles * P)) || (r = regrow(&t->lpart, 2 * tiles)) ||
      (r = regrow(&t->given, (size_t)4 * kMfMaxBatch)) ||
      (r = regrow(&t->given_masks, mask_count(s, kMfMaxBatch))))
    return fail(r);
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemsetAsync(t->xm, 0, table * sizeof(float), st);
  if (e == hipSuccess) e = hipMemsetAsync(t->xv, 0, table * sizeof(float), st);
  if (e == hipSuccess) e = hipMemsetAsync(t->pm, 0, P * sizeof(float), st);
  if (e == hipSuccess) e = hipMemsetAsync(t->pv, 0, P * sizeof(float), st);
  if (e == hipSuccess && init_table)
    e = hipMemcpyAsync(t->x, init_table, table * sizeof(float), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && init_pred)
    e = hipMemcpyAsync(t->pred, init_pred, P * sizeof(float), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && !init_table &&
      (r = launch_init_normal(ctx, key_of(t, 0, 0, kInitTable), (int64_t)table, t->x)))
    return fail(r);
  // torch's Linear.reset_parameters: weight and bias uniform in ±1/sqrt(fan_in), fan_in = H everywhere
  if (e == hipSuccess && !init_pred &&
      (r = launch_init_uniform(ctx, key_of(t, 0, 0, kInitPred),
                               (float)(1.0 / std::sqrt((double)s.H)), (int64_t)P, t->pred)))
    return fail(r);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    set_last_error(std::string("mf create: ") + hipGetErrorString(e));
    return fail(e == hipErrorOutOfMemory ? S3GRL_ERR_OUT_OF_MEMORY : S3GRL_ERR_HIP);
  }
  *out = t;
  return S3GRL_OK;
}

s3grl_status s3grl_mf_epoch(s3grl_mf* t, int64_t epoch, const int32_t* train, int64_t num_train, int64_t batch_size,
                            double lr, float* step_loss) {
  if (!t || !train || epoch < 0 || num_train < 1 || num_train >= (int64_t(1) << 31) || bad_lr(lr))
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_TRY(check_batch(batch_size));
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(check_pairs(t, train, num_train, "mf epoch"));
  S3GRL_TRY(ensure_train(t, num_train));
  S3GRL_HIP_TRY(hipMemcpyAsync(t->train, train, (size_t)(2 * num_train) * sizeof(int32_t), hipMemcpyDeviceToDevice,
                               t->ctx->stream));
  S3GRL_TRY(ensure_perm(t, epoch, num_train));
  const int64_t steps = (num_train + batch_size - 1) / batch_size;
  for (int64_t i = 0; i < steps; ++i) {
    const int64_t B = std::min(batch_size, num_train - i * batch_size);
    const MfPairs src{nullptr, t->train, t->perm + i * batch_size, key_of(t, epoch, i, kNegPair),
                      (int32_t)t->N};
    S3GRL_TRY(run_step(t, B, src, mask_of(t, nullptr, key_of(t, epoch, i, kMask)), lr,
                       step_loss ? step_loss + i : nullptr));
  }
  return S3GRL_OK;
}

s3grl_status s3grl_mf_step_pairs(s3grl_mf* t, const int32_t* pairs, int64_t batch, const uint8_t* masks, double lr,
                                 float* loss) {
  if (!t || !pairs || bad_lr(lr)) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_TRY(check_batch(batch));
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(check_pairs(t, pairs, 2 * batch, "mf step"));
  hipStream_t st = t->ctx->stream;
  S3GRL_HIP_TRY(hipMemcpyAsync(t->given, pairs, (size_t)(4 * batch) * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  if (masks)
    S3GRL_HIP_TRY(hipMemcpyAsync(t->given_masks, masks, mask_count(t->shape, batch), hipMemcpyDeviceToDevice, st));
  const MfPairs src{t->given, nullptr, nullptr, 0, (int32_t)t->N};
  return run_step(t, batch, src, mask_of(t, masks ? t->given_masks : nullptr, key_of(t, t->steps, 0, kFreeMask)),
                  lr, loss);
}

s3grl_status s3grl_mf_export_draws(s3grl_mf* t, int64_t epoch, int64_t step, int64_t num_train, int64_t batch_size,
                                   int32_t* pos_idx, int32_t* neg, uint8_t* masks) {
  if (!t || !pos_idx || !neg || !masks || epoch < 0 || step < 0 || num_train < 1 || num_train >= (int64_t(1) << 31))
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_TRY(check_batch(batch_size));
  if (step * batch_size >= num_train) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(ensure_perm(t, epoch, num_train));
  const int64_t B = std::min(batch_size, num_train - step * batch_size);
  const MfPairs src{nullptr, nullptr, t->perm + step * batch_size, key_of(t, epoch, step, kNegPair),
                    (int32_t)t->N};
  const int64_t threads = std::max<int64_t>(B, (int64_t)mask_count(t->shape, B));
  hipLaunchKernelGGL(mf_export_kernel, dim3(grid_of(threads, kMfBlock)), dim3(kMfBlock), 0, t->ctx->stream, t->shape,
                     (int)B, src, mask_of(t, nullptr, key_of(t, epoch, step, kMask)), pos_idx, neg, masks);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_mf_score(s3grl_mf* t, const int32_t* pairs, int64_t num_pairs, float* out) {
  if (!t || num_pairs < 0 || num_pairs >= (int64_t(1) << 30) || (num_pairs > 0 && (!pairs || !out)))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_pairs == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  S3GRL_TRY(check_pairs(t, pairs, num_pairs, "mf score"));
  const MfShape& s = t->shape;
  hipLaunchKernelGGL(mf_score_kernel, dim3(grid_of(num_pairs, s.T)), dim3(kMfBlock),
                     pair_lds_floats(s, false) * sizeof(float), t->ctx->stream, s, num_pairs, pairs, t->x, t->pred, out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_mf_state(const s3grl_mf* t, float* table, float* table_avg, float* table_avg_sq, float* pred,
                            float* pred_avg, float* pred_avg_sq, int64_t* steps) {
  if (!t) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(t->ctx->device));
  const size_t tb = (size_t)t->N * t->shape.H * sizeof(float), pb = (size_t)t->shape.P * sizeof(float);
  hipStream_t st = t->ctx->stream;
  if (table) S3GRL_HIP_TRY(hipMemcpyAsync(table, t->x, tb, hipMemcpyDeviceToDevice, st));
  if (table_avg) S3GRL_HIP_TRY(hipMemcpyAsync(table_avg, t->xm, tb, hipMemcpyDeviceToDevice, st));
  if (table_avg_sq) S3GRL_HIP_TRY(hipMemcpyAsync(table_avg_sq, t->xv, tb, hipMemcpyDeviceToDevice, st));
  if (pred) S3GRL_HIP_TRY(hipMemcpyAsync(pred, t->pred, pb, hipMemcpyDeviceToDevice, st));
  if (pred_avg) S3GRL_HIP_TRY(hipMemcpyAsync(pred_avg, t->pm, pb, hipMemcpyDeviceToDevice, st));
  if (pred_avg_sq) S3GRL_HIP_TRY(hipMemcpyAsync(pred_avg_sq, t->pv, pb, hipMemcpyDeviceToDevice, st));
  if (steps) *steps = t->steps;
  return S3GRL_OK;
}

s3grl_status s3grl_mf_destroy(s3grl_mf* t) {
  if (!t) return S3GRL_OK;
  (void)hipSetDevice(t->ctx->device);
  (void)hipStreamSynchronize(t->ctx->stream);
  mf_free(t);
  delete t;
  return S3GRL_OK;
}

}  // extern "C"
