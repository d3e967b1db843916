// Link-ranking metrics on gfx950: what the reference's four --eval_metric values report (utils.py evaluate_auc,
// evaluate_hits, evaluate_mrr, evaluate_ogb_rocauc), from scores that never leave the device.
//
// Ranked metrics (AUC, AP, Hits@K from ONE sort of n scores).  Launches, all on the context's stream:
//
//   mt_key_kernel      score -> 33-bit key: the fp32 bits under the order-preserving DESCENDING transform (−0.0 folded
//                      into +0.0 first: one threshold, as sklearn has it; ±inf ordinary values), shifted left by one,
//                      the label in bit 0.  NaNs and labels outside {0, 1} are counted: one integer add per block
//   sort_keys_u64 (rocPRIM's radix sort) over bits [0, 33): ascending keys = descending scores, a tie group contiguous
//   mt_partial_kernel  per tile of kMtTile sorted keys: its positives, and its LAST group start (a key whose score
//                      differs from its predecessor's) with the tile's positives in front of that start
//   mt_scan_kernel     one workgroup: exclusive sum of the positives and exclusive "last start" (a max: both the start's
//                      index and the positives in front of it grow with the index) over the tiles, 1024 at a time
//   mt_emit_kernel     per tile again, now with tp and the group start known at every element although a tie group may
//                      span any number of tiles.  At a group end e (start b, tp_b = tp[b−1], tp_g = tp[e] − tp_b, fp_g
//                      alike): the integer AUC term fp_g (2 tp_b + tp_g), the fp64 AP term (tp_g / P) tp[e] / (e + 1)
//                      and one threshold.  The element that is the K-th negative stores tp_b of its group: the
//                      positives strictly above the K-th largest negative.  One partial per tile
//   mt_fold_kernel     one workgroup: the partials in a fixed order -> the result record
//
// then one copy of the record to pinned memory and the call's one wait.  Σ of the AUC terms is 2·P·N·AUC, an exact
// integer below 2^61 for n < 2^31; the caller divides once.  No kernel waits for another workgroup, there are no float
// atomics, and every fp64 sum has a fixed shape (a thread's terms in index order, a butterfly over the wave, the waves
// in order, the tiles strided over 1024 threads in order, the same tree again): a call repeated gives the same bits.
//
// MRR (mt_mrr_kernel): positives [P], negatives [P, M] row-major.  Per row optimistic = #{neg > pos}, pessimistic =
// #{neg >= pos}, rank = (optimistic + pessimistic) / 2 + 1, mrr = 1 / rank in fp32, hits@J = rank <= J.  LPR lanes per
// row, the smallest power of two >= ceil(M / 4) up to 64, so 64 / LPR rows per wavefront; the negatives are read once,
// 16 bytes per lane, with the up to three elements in front of a row's first 16-byte boundary and behind its last peeled
// off (a row base is only 4-byte aligned when M % 4 != 0).  The kernel does nothing but read HBM and compare.
#include "s3grl_internal.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

namespace s3grl {
namespace {

constexpr int kMtBlock = 256;
constexpr int kMtIpt = 8;                       // consecutive sorted keys per thread
constexpr int kMtTile = kMtBlock * kMtIpt;      // keys per workgroup of the two tile passes
constexpr int kMtFold = 1024;                   // threads of the two one-workgroup kernels
constexpr int kMtMaxK = 16;                     // K values per call
constexpr int kMtKeyBits = 33;
constexpr int kMtVec = 4;                       // floats per 16-byte load
constexpr uint64_t kMtNone = ~0ull;             // no key: beyond either end of the list (a key has 33 bits)

// the device record, uint64 each; the MRR call uses the first five as Σ mrr (fp64 bits), hits@1, @3, @10, NaNs
enum : int { kRecP = 0, kRecThr = 1, kRecAuc = 2, kRecAp = 3, kRecNan = 4, kRecBad = 5, kRecHits = 8 };
constexpr int kRecWords = kRecHits + kMtMaxK;

struct KList {
  int32_t n;
  uint32_t k[kMtMaxK];
};

struct TilePart {   // of one tile
  uint64_t loc;     // (index of its last group start + 1) << 32 | the tile's positives in front of it; 0: no start
  uint32_t pos;     // its positives
  uint32_t pad;
};
struct TileBase {   // in front of one tile
  uint64_t carry;   // (index of the last group start + 1) << 32 | ALL positives in front of that start
  uint32_t tp;      // positives
  uint32_t pad;
};

// ---- workgroup primitives: a scan over the wave by shuffles, the waves through LDS ------------------------------------
struct OpAdd {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// exclusive scan of v over the workgroup's threads (identity 0), `total` on every thread; lds: blockDim.x / 64 + 1 T
template <typename T, typename Op>
__device__ __forceinline__ T block_excl_scan(T v, T* lds, T& total, Op op) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  T x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o, 64);
    if (lane >= o) x = op(x, y);
  }
  __syncthreads();                      // lds may still be read from an earlier call
  if (lane == 63) lds[wave] = x;
  __syncthreads();
  T before = 0, all = 0;
  for (int w = 0; w < waves; ++w) {
    const T s = lds[w];
    if (w < wave) before = op(before, s);
    all = op(all, s);
  }
  total = all;
  T excl = __shfl_up(x, 1, 64);
  if (lane == 0) excl = 0;
  return op(before, excl);
}

// Σ v over the workgroup, on every thread: a butterfly over the wave, then the waves in order
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* lds) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  T acc = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) acc += lds[w];
  return acc;
}

// ---- keys ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t score_key(float s, uint32_t label, uint32_t& nan) {
  uint32_t b = __float_as_uint(s);
  nan += (b & 0x7fffffffu) > 0x7f800000u;
  if (b == 0x80000000u) b = 0;                                   // −0.0 is +0.0
  const uint32_t asc = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
  return ((uint64_t)(~asc) << 1) | (label & 1u);
}

// labels [n] (1: positive; anything above 1 is counted as bad) or null: the first n_pos entries are the positives
__global__ __launch_bounds__(kMtBlock) void mt_key_kernel(const float* __restrict__ scores,
                                                          const uint8_t* __restrict__ labels, int64_t n, int64_t n_pos,
                                                          uint64_t* __restrict__ keys, unsigned long long* __restrict__ rec) {
  __shared__ uint32_t lds[kMtBlock / 64];
  const int64_t i0 = ((int64_t)blockIdx.x * kMtBlock + threadIdx.x) * kMtVec;
  uint32_t nan = 0, bad = 0;
  if (i0 < n) {
    float s[kMtVec];
    uint32_t y[kMtVec];
    const int cnt = (int)min((int64_t)kMtVec, n - i0);
    if (cnt == kMtVec && ((uintptr_t)scores & 15) == 0) {
      const float4 v = *reinterpret_cast<const float4*>(scores + i0);
      s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
    } else {
      for (int j = 0; j < kMtVec; ++j) s[j] = j < cnt ? scores[i0 + j] : 0.f;
    }
    if (!labels) {
      for (int j = 0; j < kMtVec; ++j) y[j] = i0 + j < n_pos;
    } else if (cnt == kMtVec && ((uintptr_t)labels & 3) == 0) {
      const uchar4 v = *reinterpret_cast<const uchar4*>(labels + i0);
      y[0] = v.x, y[1] = v.y, y[2] = v.z, y[3] = v.w;
    } else {
      for (int j = 0; j < kMtVec; ++j) y[j] = j < cnt ? labels[i0 + j] : 0;
    }
    uint64_t k[kMtVec];
    for (int j = 0; j < kMtVec; ++j) {
      uint32_t dummy = 0;
      k[j] = score_key(s[j], y[j], j < cnt ? nan : dummy);
      bad += j < cnt && y[j] > 1;
    }
    if (cnt == kMtVec) {                                          // keys + i0: 32-byte aligned
      ulonglong2* o = reinterpret_cast<ulonglong2*>(keys + i0);
      o[0] = make_ulonglong2(k[0], k[1]);
      o[1] = make_ulonglong2(k[2], k[3]);
    } else {
      for (int j = 0; j < cnt; ++j) keys[i0 + j] = k[j];
    }
  }
  const uint32_t both = block_sum(nan | (bad << 16), lds);       // at most 1024 of either per block
  if (threadIdx.x == 0 && both) {
    if (both & 0xffffu) atomicAdd(&rec[kRecNan], (unsigned long long)(both & 0xffffu));
    if (both >> 16) atomicAdd(&rec[kRecBad], (unsigned long long)(both >> 16));
  }
}

// ---- the tile passes ----------------------------------------------------------------------------------------------------
// LDS position of tile slot p (slot 0: the key in front of the tile, 1 .. kMtTile: its keys, kMtTile + 1: the key
// behind it): one slot of padding per eight, so that the 64-byte runs of a wave's lanes start on different banks
__device__ __forceinline__ int mt_slot(int p) { return p + (p >> 3); }
constexpr int kMtTileLds = kMtTile + 2 + ((kMtTile + 2) >> 3) + 1;

// keys [base, base + kMtTile) of the sorted list come in 16 bytes per lane, coalesced; a thread leaves with its
// kMtIpt consecutive keys, the one in front and the one behind (kMtNone beyond either end of the list)
__device__ __forceinline__ void load_tile(const uint64_t* __restrict__ keys, int64_t n, int64_t base, uint64_t* lds,
                                          uint64_t (&k)[kMtIpt], uint64_t& prev, uint64_t& next) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < kMtIpt / 2; ++j) {
    const int p = (j * kMtBlock + t) * 2;
    const int64_t i = base + p;
    ulonglong2 v = make_ulonglong2(kMtNone, kMtNone);
    if (i + 1 < n) v = *reinterpret_cast<const ulonglong2*>(keys + i);   // base and p even, keys 256-byte aligned
    else if (i < n) v.x = keys[i];
    lds[mt_slot(p + 1)] = v.x;
    lds[mt_slot(p + 2)] = v.y;
  }
  if (t == 0) {
    lds[mt_slot(0)] = base > 0 ? keys[base - 1] : kMtNone;
    lds[mt_slot(kMtTile + 1)] = base + kMtTile < n ? keys[base + kMtTile] : kMtNone;
  }
  __syncthreads();
  prev = lds[mt_slot(t * kMtIpt)];
#pragma unroll
  for (int j = 0; j < kMtIpt; ++j) k[j] = lds[mt_slot(t * kMtIpt + 1 + j)];
  next = lds[mt_slot(t * kMtIpt + kMtIpt + 1)];
}

// a thread's positives and its last group start as TilePart::loc with the THREAD's positives in front of it
__device__ __forceinline__ void thread_part(const uint64_t (&k)[kMtIpt], uint64_t prev, int64_t i0, int64_t n,
                                            uint32_t& pos, uint64_t& loc) {
  pos = 0;
  loc = 0;
  uint64_t sp = prev >> 1;
#pragma unroll
  for (int j = 0; j < kMtIpt; ++j) {
    if (i0 + j < n) {
      const uint64_t s = k[j] >> 1;
      if (s != sp) loc = ((uint64_t)(i0 + j + 1) << 32) | pos;
      pos += (uint32_t)(k[j] & 1);
      sp = s;
    }
  }
}

__global__ __launch_bounds__(kMtBlock) void mt_partial_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                              TilePart* __restrict__ parts) {
  __shared__ uint64_t tile[kMtTileLds];
  __shared__ uint64_t sc[kMtBlock / 64 + 1];
  const int64_t base = (int64_t)blockIdx.x * kMtTile;
  uint64_t k[kMtIpt], prev, next;
  load_tile(keys, n, base, tile, k, prev, next);
  uint32_t pos;
  uint64_t loc;
  thread_part(k, prev, base + (int64_t)threadIdx.x * kMtIpt, n, pos, loc);
  uint64_t total, top;
  const uint64_t excl = block_excl_scan<uint64_t>(pos, sc, total, OpAdd());
  block_excl_scan<uint64_t>(loc ? loc + excl : 0, sc, top, OpMax());
  if (threadIdx.x == 0) parts[blockIdx.x] = TilePart{top, (uint32_t)total, 0};
}

__global__ __launch_bounds__(kMtFold) void mt_scan_kernel(const TilePart* __restrict__ parts, int64_t tiles,
                                                          TileBase* __restrict__ bases,
                                                          unsigned long long* __restrict__ rec) {
  __shared__ uint64_t sc[kMtFold / 64 + 1];
  uint64_t carry_tp = 0, carry_loc = 0;
  for (int64_t c0 = 0; c0 < tiles; c0 += kMtFold) {
    const int64_t b = c0 + threadIdx.x;
    TilePart p{0, 0, 0};
    if (b < tiles) p = parts[b];
    uint64_t total, top;
    const uint64_t tp = carry_tp + block_excl_scan<uint64_t>(p.pos, sc, total, OpAdd());
    uint64_t before = block_excl_scan<uint64_t>(p.loc ? p.loc + tp : 0, sc, top, OpMax());
    if (before < carry_loc) before = carry_loc;
    if (b < tiles) bases[b] = TileBase{before, (uint32_t)tp, 0};
    carry_tp += total;
    if (top > carry_loc) carry_loc = top;
  }
  if (threadIdx.x == 0) rec[kRecP] = carry_tp;
}

__global__ __launch_bounds__(kMtBlock) void mt_emit_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                           const TileBase* __restrict__ bases, KList ks,
                                                           unsigned long long* __restrict__ rec,
                                                           double* __restrict__ part_ap,
                                                           unsigned long long* __restrict__ part_auc,
                                                           unsigned long long* __restrict__ part_thr) {
  __shared__ uint64_t tile[kMtTileLds];
  __shared__ uint64_t sc[kMtBlock / 64 + 1];
  __shared__ double scd[kMtBlock / 64];
  const int64_t base = (int64_t)blockIdx.x * kMtTile, i0 = base + (int64_t)threadIdx.x * kMtIpt;
  uint64_t k[kMtIpt], prev, next;
  load_tile(keys, n, base, tile, k, prev, next);
  uint32_t pos;
  uint64_t loc;
  thread_part(k, prev, i0, n, pos, loc);
  const TileBase tb = bases[blockIdx.x];
  uint64_t unused;
  const uint64_t tp0 = tb.tp + block_excl_scan<uint64_t>(pos, sc, unused, OpAdd());
  uint64_t cur = block_excl_scan<uint64_t>(loc ? loc + tp0 : 0, sc, unused, OpMax());
  if (cur < tb.carry) cur = tb.carry;
  const double P = (double)rec[kRecP];                  // mt_scan_kernel's, a launch ago
  // the walk: tp the positives so far, (gs, gtp) the current group's start and the positives in front of it
  uint64_t tp = tp0, gs = (cur >> 32) - 1, gtp = cur & 0xffffffffu;
  uint64_t auc = 0, thr = 0;
  double ap = 0.0;
  uint64_t sp = prev >> 1;
#pragma unroll
  for (int j = 0; j < kMtIpt; ++j) {
    const uint64_t i = (uint64_t)(i0 + j);
    if ((int64_t)i < n) {
      const uint64_t s = k[j] >> 1, lab = k[j] & 1, sn = (j + 1 < kMtIpt ? k[j + 1] : next) >> 1;
      if (s != sp) gs = i, gtp = tp;
      tp += lab;
      if (!lab) {
        const uint64_t negs = i + 1 - tp;                 // this is the negs-th negative
        for (int q = 0; q < ks.n; ++q)
          if (negs == ks.k[q]) rec[kRecHits + q] = gtp;
      }
      if (s != sn) {                                      // a group end
        const uint64_t tp_g = tp - gtp, fp_g = (i + 1 - tp) - (gs - gtp);
        auc += fp_g * (2 * gtp + tp_g);
        ap += ((double)tp_g / P) * (double)tp / (double)(i + 1);
        ++thr;
      }
      sp = s;
    }
  }
  const double ap_b = block_sum(ap, scd);
  const uint64_t auc_b = block_sum(auc, sc), thr_b = block_sum(thr, sc);
  if (threadIdx.x == 0) {
    part_ap[blockIdx.x] = ap_b;
    part_auc[blockIdx.x] = auc_b;
    part_thr[blockIdx.x] = thr_b;
  }
}

// rec[slot_d] = Σ d (fp64 bits) and rec[slot_u[c]] = Σ u[c], c < 4 (null: skipped), over `count` partials: thread t adds
// partials t, t + 1024, … in order, then block_sum's tree
struct FoldArgs {
  const double* d;
  const unsigned long long* u[4];
  int slot_d, slot_u[4];
};
__global__ __launch_bounds__(kMtFold) void mt_fold_kernel(FoldArgs a, int64_t count, unsigned long long* __restrict__ rec) {
  __shared__ uint64_t sc[kMtFold / 64];
  __shared__ double scd[kMtFold / 64];
  double d = 0.0;
  for (int64_t b = threadIdx.x; b < count; b += kMtFold) d += a.d[b];
  d = block_sum(d, scd);
  if (threadIdx.x == 0) rec[a.slot_d] = (unsigned long long)__double_as_longlong(d);
  for (int c = 0; c < 4; ++c) {
    if (!a.u[c]) continue;
    uint64_t u = 0;
    for (int64_t b = threadIdx.x; b < count; b += kMtFold) u += a.u[c][b];
    u = block_sum(u, sc);
    if (threadIdx.x == 0) rec[a.slot_u[c]] = u;
  }
}

// ---- MRR ----------------------------------------------------------------------------------------------------------------
int mrr_lanes_per_row(int64_t M) {
  const int64_t v = (M + kMtVec - 1) / kMtVec;
  int lpr = 1;
  while (lpr < v && lpr < 64) lpr <<= 1;
  return lpr;
}

__device__ __forceinline__ void mrr_count(float v, float pv, uint32_t& gt, uint32_t& ge, uint32_t& nan) {
  gt += v > pv;
  ge += v >= pv;
  nan += v != v;
}
__device__ __forceinline__ void mrr_count4(float4 v, float pv, uint32_t& gt, uint32_t& ge, uint32_t& nan) {
  mrr_count(v.x, pv, gt, ge, nan);
  mrr_count(v.y, pv, gt, ge, nan);
  mrr_count(v.z, pv, gt, ge, nan);
  mrr_count(v.w, pv, gt, ge, nan);
}
constexpr int kMrrBatch = 4;   // 16-byte loads a lane has in flight on a long row

__global__ __launch_bounds__(kMtBlock) void mt_mrr_kernel(const float* __restrict__ pos, const float* __restrict__ neg,
                                                          int64_t P, int64_t M, int lpr, float* __restrict__ mrr_list,
                                                          double* __restrict__ part_sum,
                                                          unsigned long long* __restrict__ part_h1,
                                                          unsigned long long* __restrict__ part_h3,
                                                          unsigned long long* __restrict__ part_h10,
                                                          unsigned long long* __restrict__ part_nan) {
  __shared__ uint64_t sc[kMtBlock / 64];
  __shared__ double scd[kMtBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rpw = 64 / lpr, g = lane / lpr, q = lane % lpr;
  const int64_t row = ((int64_t)blockIdx.x * (kMtBlock / 64) + wave) * rpw + g;
  uint32_t gt = 0, ge = 0, nan = 0;
  if (row < P) {
    const float pv = pos[row];
    if (q == 0) nan += pv != pv;
    const float* __restrict__ r = neg + row * M;
    // head: up to the row's first 16-byte boundary; body: whole float4; tail: what is left
    const int64_t head = min(M, (int64_t)((0 - ((uintptr_t)r >> 2)) & 3));
    const int64_t nv = (M - head) / kMtVec, t0 = head + nv * kMtVec;
    for (int64_t x = q; x < head; x += lpr) mrr_count(r[x], pv, gt, ge, nan);
    const float4* __restrict__ body = reinterpret_cast<const float4*>(r + head);
    if (nv <= lpr) {                                      // a short row: one load per lane covers it
      if (q < nv) mrr_count4(body[q], pv, gt, ge, nan);
    } else {
      // kMrrBatch loads of a lane are issued before the first is used (a load beyond the row re-reads its last vector
      // and is not counted): a wavefront keeps 4 KB in flight, not 1 KB
      for (int64_t x0 = q; x0 < nv; x0 += (int64_t)kMrrBatch * lpr) {
        float4 v[kMrrBatch];
#pragma unroll
        for (int u = 0; u < kMrrBatch; ++u) v[u] = body[min(x0 + (int64_t)u * lpr, nv - 1)];
#pragma unroll
        for (int u = 0; u < kMrrBatch; ++u)
          if (x0 + (int64_t)u * lpr < nv) mrr_count4(v[u], pv, gt, ge, nan);
      }
    }
    for (int64_t x = t0 + q; x < M; x += lpr) mrr_count(r[x], pv, gt, ge, nan);
  }
  for (int o = lpr >> 1; o > 0; o >>= 1) {               // the lanes of a row are lpr consecutive lanes
    gt += __shfl_xor(gt, o, 64);
    ge += __shfl_xor(ge, o, 64);
  }
  double m = 0.0;
  uint64_t hits = 0;                                      // hits@1 | hits@3 << 16 | hits@10 << 32: at most 256 each
  if (row < P && q == 0) {
    const float rank = (float)(0.5 * (double)((uint64_t)gt + ge) + 1.0);
    const float mr = __fdiv_rn(1.0f, rank);
    mrr_list[row] = mr;
    m = (double)mr;
    hits = (uint64_t)(rank <= 1.f) | ((uint64_t)(rank <= 3.f) << 16) | ((uint64_t)(rank <= 10.f) << 32);
  }
  m = block_sum(m, scd);
  hits = block_sum(hits, sc);
  const uint64_t nans = block_sum((uint64_t)nan, sc);
  if (threadIdx.x == 0) {
    part_sum[blockIdx.x] = m;
    part_h1[blockIdx.x] = hits & 0xffffu;
    part_h3[blockIdx.x] = (hits >> 16) & 0xffffu;
    part_h10[blockIdx.x] = (hits >> 32) & 0xffffu;
    part_nan[blockIdx.x] = nans;
  }
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

struct s3grl_metrics {
  s3grl_context* ctx = nullptr;
  uint64_t* keys = nullptr;        // [2, cap_n]: the keys, then the sorted keys
  int64_t cap_n = 0;
  SortScratch sort;
  TilePart* parts = nullptr;       // [cap_tiles]
  TileBase* bases = nullptr;       // [cap_tiles]
  int64_t cap_tiles = 0;
  unsigned long long* red = nullptr;   // [5, cap_red] partials of the emitting pass / the MRR kernel
  int64_t cap_red = 0;
  unsigned long long* rec = nullptr;   // [kRecWords] device
  unsigned long long* h_rec = nullptr; // pinned
};

namespace {

void mt_free(s3grl_metrics* m) {
  for (void* p : {(void*)m->keys, m->sort.tmp, (void*)m->parts, (void*)m->bases, (void*)m->red, (void*)m->rec})
    if (p) (void)hipFree(p);
  if (m->h_rec) (void)hipHostFree(m->h_rec);
}

// *p -> at least `bytes`; the old block may still be in use on the stream
s3grl_status mt_grow(s3grl_metrics* m, void** p, size_t bytes) {
  S3GRL_HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  if (*p) S3GRL_HIP_TRY(hipFree(*p));
  *p = nullptr;
  S3GRL_HIP_TRY(hipMalloc(p, bytes));
  return S3GRL_OK;
}

s3grl_status ensure_red(s3grl_metrics* m, int64_t blocks) {
  if (blocks <= m->cap_red) return S3GRL_OK;
  m->cap_red = 0;
  S3GRL_TRY(mt_grow(m, reinterpret_cast<void**>(&m->red), (size_t)blocks * 5 * sizeof(unsigned long long)));
  m->cap_red = blocks;
  return S3GRL_OK;
}

s3grl_status read_record(s3grl_metrics* m) {
  hipStream_t st = m->ctx->stream;
  S3GRL_HIP_TRY(hipMemcpyAsync(m->h_rec, m->rec, kRecWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  S3GRL_HIP_TRY(hipStreamSynchronize(st));
  return S3GRL_OK;
}

}  // namespace

extern "C" {

s3grl_status s3grl_metrics_layout(int64_t num_neg, int32_t* out) {
  if (!out || num_neg < 1 || num_neg >= (int64_t(1) << 31)) return S3GRL_ERR_INVALID_ARGUMENT;
  const int lpr = mrr_lanes_per_row(num_neg);
  out[0] = kMtTile;
  out[1] = 64 / lpr;
  out[2] = lpr;
  out[3] = kMtVec;
  out[4] = kMtMaxK;
  out[5] = (kMtBlock / 64) * (64 / lpr);
  return S3GRL_OK;
}

s3grl_status s3grl_metrics_create(s3grl_context* ctx, s3grl_metrics** out) {
  if (!ctx || !out) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  auto* m = new s3grl_metrics();
  m->ctx = ctx;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->rec), kRecWords * sizeof(unsigned long long));
  if (e == hipSuccess)
    e = hipHostMalloc(reinterpret_cast<void**>(&m->h_rec), kRecWords * sizeof(unsigned long long), hipHostMallocDefault);
  if (e != hipSuccess) {
    set_last_error(std::string("metrics create: ") + hipGetErrorString(e));
    mt_free(m);
    delete m;
    return e == hipErrorOutOfMemory ? S3GRL_ERR_OUT_OF_MEMORY : S3GRL_ERR_HIP;
  }
  *out = m;
  return S3GRL_OK;
}

s3grl_status s3grl_metrics_ranked(s3grl_metrics* m, const float* scores, const uint8_t* labels, int64_t n, int64_t n_pos,
                                  const int64_t* ks, int32_t num_k, int64_t* counts, double* ap, int64_t* hits) {
  if (!m || !scores || !counts || !ap || n < 1 || n >= (int64_t(1) << 31) || num_k < 0 || num_k > kMtMaxK ||
      (num_k && (!ks || !hits)) || (!labels && (n_pos < 0 || n_pos > n)))
    return S3GRL_ERR_INVALID_ARGUMENT;
  KList kl{};
  kl.n = num_k;
  for (int q = 0; q < num_k; ++q) {
    if (ks[q] < 1) {
      set_last_error("metrics ranked: K must be at least 1");
      return S3GRL_ERR_INVALID_ARGUMENT;
    }
    kl.k[q] = (uint32_t)std::min<int64_t>(ks[q], 0xffffffffll);   // beyond n: no element is the K-th negative
  }
  S3GRL_HIP_TRY(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  const int64_t tiles = (n + kMtTile - 1) / kMtTile;
  if (n > m->cap_n) {
    const int64_t cap = (n + 31) & ~(int64_t)31;   // the second half starts 256-byte aligned too
    m->cap_n = 0;
    S3GRL_TRY(mt_grow(m, reinterpret_cast<void**>(&m->keys), (size_t)cap * 2 * sizeof(uint64_t)));
    m->cap_n = cap;
  }
  if (tiles > m->cap_tiles) {
    m->cap_tiles = 0;
    S3GRL_TRY(mt_grow(m, reinterpret_cast<void**>(&m->parts), (size_t)tiles * sizeof(TilePart)));
    S3GRL_TRY(mt_grow(m, reinterpret_cast<void**>(&m->bases), (size_t)tiles * sizeof(TileBase)));
    m->cap_tiles = tiles;
  }
  S3GRL_TRY(ensure_red(m, tiles));
  uint64_t* keys_in = m->keys;
  uint64_t* keys_out = m->keys + m->cap_n;
  S3GRL_HIP_TRY(hipMemsetAsync(m->rec, 0, kRecHits * sizeof(unsigned long long), st));
  S3GRL_HIP_TRY(hipMemsetAsync(m->rec + kRecHits, 0xff, kMtMaxK * sizeof(unsigned long long), st));   // -1: no K-th negative
  const int64_t key_blocks = (n + (int64_t)kMtBlock * kMtVec - 1) / ((int64_t)kMtBlock * kMtVec);
  hipLaunchKernelGGL(mt_key_kernel, dim3((unsigned)key_blocks), dim3(kMtBlock), 0, st, scores, labels, n, n_pos, keys_in,
                     m->rec);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(sort_keys_u64(m->ctx, m->sort, keys_in, keys_out, (size_t)n, kMtKeyBits));
  double* part_ap = reinterpret_cast<double*>(m->red);
  unsigned long long* part_auc = m->red + m->cap_red;
  unsigned long long* part_thr = m->red + 2 * m->cap_red;
  hipLaunchKernelGGL(mt_partial_kernel, dim3((unsigned)tiles), dim3(kMtBlock), 0, st, keys_out, n, m->parts);
  hipLaunchKernelGGL(mt_scan_kernel, dim3(1), dim3(kMtFold), 0, st, m->parts, tiles, m->bases, m->rec);
  hipLaunchKernelGGL(mt_emit_kernel, dim3((unsigned)tiles), dim3(kMtBlock), 0, st, keys_out, n, m->bases, kl, m->rec,
                     part_ap, part_auc, part_thr);
  FoldArgs fa{part_ap, {part_auc, part_thr, nullptr, nullptr}, kRecAp, {kRecAuc, kRecThr, 0, 0}};
  hipLaunchKernelGGL(mt_fold_kernel, dim3(1), dim3(kMtFold), 0, st, fa, tiles, m->rec);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(read_record(m));
  const unsigned long long* r = m->h_rec;
  counts[0] = (int64_t)r[kRecP];
  counts[1] = n - (int64_t)r[kRecP];
  counts[2] = (int64_t)r[kRecThr];
  counts[3] = (int64_t)r[kRecNan];
  counts[4] = (int64_t)r[kRecBad];
  counts[5] = (int64_t)r[kRecAuc];
  std::memcpy(ap, &r[kRecAp], sizeof(double));
  for (int q = 0; q < num_k; ++q) hits[q] = (int64_t)r[kRecHits + q];
  return S3GRL_OK;
}

s3grl_status s3grl_metrics_mrr(s3grl_metrics* m, const float* pos, const float* neg, int64_t num_pos, int64_t num_neg,
                               float* mrr_list, double* sum, int64_t* counts) {
  if (!m || !pos || !neg || !mrr_list || !sum || !counts || num_pos < 1 || num_neg < 1 ||
      num_pos >= (int64_t(1) << 31) || num_neg >= (int64_t(1) << 31))
    return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  const int lpr = mrr_lanes_per_row(num_neg);
  const int64_t rows_per_block = (kMtBlock / 64) * (64 / lpr);
  const int64_t blocks = (num_pos + rows_per_block - 1) / rows_per_block;
  S3GRL_TRY(ensure_red(m, blocks));
  double* part_sum = reinterpret_cast<double*>(m->red);
  unsigned long long* u[4];
  for (int c = 0; c < 4; ++c) u[c] = m->red + (c + 1) * m->cap_red;
  hipLaunchKernelGGL(mt_mrr_kernel, dim3((unsigned)blocks), dim3(kMtBlock), 0, st, pos, neg, num_pos, num_neg, lpr,
                     mrr_list, part_sum, u[0], u[1], u[2], u[3]);
  FoldArgs fa{part_sum, {u[0], u[1], u[2], u[3]}, 0, {1, 2, 3, 4}};
  hipLaunchKernelGGL(mt_fold_kernel, dim3(1), dim3(kMtFold), 0, st, fa, blocks, m->rec);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(read_record(m));
  std::memcpy(sum, &m->h_rec[0], sizeof(double));
  for (int c = 0; c < 4; ++c) counts[c] = (int64_t)m->h_rec[1 + c];
  return S3GRL_OK;
}

s3grl_status s3grl_metrics_destroy(s3grl_metrics* m) {
  if (!m) return S3GRL_OK;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  mt_free(m);
  delete m;
  return S3GRL_OK;
}

}  // extern "C"
