// Subgraph sketching (ELPH / BUDDY, Chamberlain et al., ICLR 2023): a MinHash and a HyperLogLog sketch of every
// node's 0..k-hop ball, and per link the estimated intersections of the two endpoints' balls with the structure counts
// that follow from them by inclusion-exclusion.  DESIGN.md section 24 is the specification; tests/sketch_reference.py
// restates it in numpy, and every output here equals that restatement to the bit.
//
//   sketch_init_kernel        hop 0 of both tables: MH_0[v, s] = H(v, s), HL_0[v] one register of rank(H(v, P))
//   sketch_propagate_kernel   hop i from hop i-1: elementwise min (MinHash) / max (HLL) over a row's stored keys and
//                             the row itself.  A wavefront owns a row; lanes run over columns (8-byte MinHash words,
//                             4 register bytes per HLL word).  A row of more than kSplitKeys keys is split over the
//                             four wavefronts of its workgroup and combined through LDS.  min / max are associative,
//                             commutative and idempotent: any split gives the same bits, and there are no atomics.
//   sketch_cardinality_kernel E(row) of register rows, a wavefront per row (ball sizes)
//   sketch_pairs_kernel       a wavefront per link: the 2 (hops + 1) rows of both endpoints are read once into
//                             registers; match by ballot + popcount, T and z by one packed integer wave reduction per
//                             pair; then lane k does pair k's fp64 tail (one division per lane, not (hops + 1)^2 in
//                             lane 0) and lanes share the intersections through LDS for the inclusion-exclusion.
//
// Everything up to the fp64 tail is integer min / max / compare / popcount; the tail is single IEEE operations in the
// order of the specification (no reciprocal, nothing -ffp-contract could fuse), and the device evaluates no logarithm:
// the linear-counting table LC[z] comes from the host.
#include "s3grl_internal.hpp"

#include <algorithm>
#include <vector>

namespace s3grl {
namespace {

constexpr int kSkBlock = 256, kSkWaves = 4;
constexpr int kSplitKeys = 64;       // a row with more keys than this is split over the workgroup's wavefronts
constexpr int kBatch = 4;            // neighbour rows a wavefront loads before it reduces them
// columns per lane (NC below): num_perm / 2 <= 256 MinHash words and m / 4 <= 256 HLL words, so 1, 2 or 4

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ uint32_t sketch_hash(uint32_t v, uint32_t slot, uint32_t seed) {
  return fmix32(v * 0x9E3779B1u + fmix32(seed + slot * 0x27D4EB2Fu));
}

// the larger of each of the four bytes
__device__ __forceinline__ uint32_t max_u8x4(uint32_t a, uint32_t b) {
  return max(a & 0x000000FFu, b & 0x000000FFu) | max(a & 0x0000FF00u, b & 0x0000FF00u) |
         max(a & 0x00FF0000u, b & 0x00FF0000u) | max(a & 0xFF000000u, b & 0xFF000000u);
}

__device__ __forceinline__ uint2 min_u32x2(uint2 a, uint2 b) { return make_uint2(min(a.x, b.x), min(a.y, b.y)); }

__device__ __forceinline__ int wave_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

// mh [N, P] uint32, hl [N, m / 4] words of four registers (byte k of a word is register 4 w + k)
__global__ __launch_bounds__(kSkBlock) void sketch_init_kernel(int64_t n, int P, int p, uint32_t seed,
                                                               uint32_t* __restrict__ mh, uint32_t* __restrict__ hl) {
  const int64_t stride = (int64_t)gridDim.x * kSkBlock, first = (int64_t)blockIdx.x * kSkBlock + threadIdx.x;
  for (int64_t at = first; at < n * P; at += stride)
    mh[at] = sketch_hash((uint32_t)(at / P), (uint32_t)(at % P), seed);
  const int words = (1 << p) / 4;
  for (int64_t at = first; at < n * words; at += stride) {
    const uint32_t h = sketch_hash((uint32_t)(at / words), (uint32_t)P, seed);
    const uint32_t reg = h >> (32 - p), field = h & ((1u << (32 - p)) - 1u);
    const uint32_t rank = field ? (uint32_t)__clz((int)field) - (uint32_t)p + 1u : (uint32_t)(33 - p);
    hl[at] = (int)(reg >> 2) == (int)(at % words) ? rank << (8 * (reg & 3u)) : 0u;
  }
}

// One wavefront's share of a row: the row itself and keys [begin, end) of idx, reduced into acc.  Lanes hold columns
// lane, lane + 64, ...; the keys are loaded 64 at a time and handed round by readlane.
template <int NC>
__device__ __forceinline__ void reduce_keys(int lane, int64_t self, int begin, int end, const int32_t* __restrict__ idx,
                                            int P2, int M4, const uint2* __restrict__ mh,
                                            const uint32_t* __restrict__ hl, uint2 (&am)[NC], uint32_t (&ah)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = c * 64 + lane;
    am[c] = col < P2 ? mh[self * P2 + col] : make_uint2(0u, 0u);
    ah[c] = col < M4 ? hl[self * M4 + col] : 0u;
  }
  for (int e0 = begin; e0 < end; e0 += 64) {
    const int mine = e0 + lane < end ? idx[e0 + lane] : 0;
    const int count = min(64, end - e0);
    int j = 0;
    for (; j + kBatch <= count; j += kBatch) {   // kBatch rows in flight: the loads do not wait for each other
      uint2 tm[kBatch][NC];
      uint32_t th[kBatch][NC];
#pragma unroll
      for (int q = 0; q < kBatch; ++q) {
        const int64_t w = __builtin_amdgcn_readlane(mine, j + q);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int col = c * 64 + lane;
          tm[q][c] = col < P2 ? mh[w * P2 + col] : make_uint2(0u, 0u);
          th[q][c] = col < M4 ? hl[w * M4 + col] : 0u;
        }
      }
#pragma unroll
      for (int q = 0; q < kBatch; ++q)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int col = c * 64 + lane;
          if (col < P2) am[c] = min_u32x2(am[c], tm[q][c]);
          if (col < M4) ah[c] = max_u8x4(ah[c], th[q][c]);
        }
    }
    for (; j < count; ++j) {
      const int64_t w = __builtin_amdgcn_readlane(mine, j);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = c * 64 + lane;
        if (col < P2) am[c] = min_u32x2(am[c], mh[w * P2 + col]);
        if (col < M4) ah[c] = max_u8x4(ah[c], hl[w * M4 + col]);
      }
    }
  }
}

// Hop i from hop i - 1.  A workgroup takes four consecutive rows.  Rows of at most kSplitKeys keys: one per wavefront.
// Longer rows: one after the other, each wavefront a quarter of the keys, the four partial rows combined through LDS.
template <int NC>
__global__ __launch_bounds__(kSkBlock) void sketch_propagate_kernel(int64_t n, const int64_t* __restrict__ ptr,
                                                                    const int32_t* __restrict__ idx, int P2, int M4,
                                                                    const uint2* __restrict__ mh_prev,
                                                                    const uint32_t* __restrict__ hl_prev,
                                                                    uint2* __restrict__ mh_next,
                                                                    uint32_t* __restrict__ hl_next) {
  __shared__ uint2 part_m[kSkWaves][64 * NC];
  __shared__ uint32_t part_h[kSkWaves][64 * NC];
  const int wave = wave_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t base = (int64_t)blockIdx.x * kSkWaves;
  uint2 am[NC];
  uint32_t ah[NC];
  {
    const int64_t r = base + wave;
    if (r < n) {
      const int begin = wave_uniform((int)ptr[r]), end = wave_uniform((int)ptr[r + 1]);
      if (end - begin <= kSplitKeys) {
        reduce_keys<NC>(lane, r, begin, end, idx, P2, M4, mh_prev, hl_prev, am, ah);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int col = c * 64 + lane;
          if (col < P2) mh_next[r * P2 + col] = am[c];
          if (col < M4) hl_next[r * M4 + col] = ah[c];
        }
      }
    }
  }
  for (int q = 0; q < kSkWaves; ++q) {   // every wavefront of the workgroup takes the same path from here on
    const int64_t r = base + q;
    if (r >= n) break;
    const int begin = wave_uniform((int)ptr[r]), end = wave_uniform((int)ptr[r + 1]);
    if (end - begin <= kSplitKeys) continue;
    const int share = (end - begin + kSkWaves - 1) / kSkWaves;
    const int b = min(end, begin + wave * share), e = min(end, b + share);
    reduce_keys<NC>(lane, r, b, e, idx, P2, M4, mh_prev, hl_prev, am, ah);   // each partial starts from the row itself
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      part_m[wave][c * 64 + lane] = am[c];
      part_h[wave][c * 64 + lane] = ah[c];
    }
    __syncthreads();
    for (int col = threadIdx.x; col < 64 * NC; col += kSkBlock) {
      uint2 m = part_m[0][col];
      uint32_t h = part_h[0][col];
#pragma unroll
      for (int w = 1; w < kSkWaves; ++w) {
        m = min_u32x2(m, part_m[w][col]);
        h = max_u8x4(h, part_h[w][col]);
      }
      if (col < P2) mh_next[r * P2 + col] = m;
      if (col < M4) hl_next[r * M4 + col] = h;
    }
    __syncthreads();
  }
}

// A lane's share of T = sum 2^(R - reg) and of z = the zero registers, over the four registers of a word.  A lane
// holds at most 16 registers, so its T stays below 2^(R + 4) <= 2^30 and fits 32 bits.
__device__ __forceinline__ void word_tz(uint32_t w, int R, uint32_t& t, uint32_t& z) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t reg = (w >> (8 * k)) & 0xFFu;
    t += 1u << (R - (int)reg);
    z += reg == 0u;
  }
}

// T in the low 40 bits, z from bit 40: T <= m 2^R = 2^33 and z <= m <= 2^10, so one 64-bit sum carries both
__device__ __forceinline__ uint64_t pack_tz(uint32_t t, uint32_t z) { return (uint64_t)t | ((uint64_t)z << 40); }

template <int CTRL>
__device__ __forceinline__ uint64_t dpp_add(uint64_t x) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), CTRL, 0xF, 0xF, false);
  return x + (((uint64_t)hi << 32) | lo);
}

// The sum over the 64 lanes, in every lane; all lanes active.  Within a row of 16 lanes by data-parallel moves (lane
// ^ 1, lane ^ 2, the mirror of 8, the mirror of 16), no LDS; the four rows by readlane.
__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
  x = dpp_add<0xB1>(x);    // quad_perm [1, 0, 3, 2]
  x = dpp_add<0x4E>(x);    // quad_perm [2, 3, 0, 1]
  x = dpp_add<0x141>(x);   // row_half_mirror
  x = dpp_add<0x140>(x);   // row_mirror
  uint64_t total = 0;
#pragma unroll
  for (int row = 0; row < 64; row += 16)
    total += ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), row) << 32) |
             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, row);
  return total;
}

// the cardinality of a register row from its T and z: E_raw = C / T, the linear-counting table below 2.5 m
__device__ __forceinline__ double cardinality(int64_t T, int z, int m, double C, const double* __restrict__ lc) {
  const double raw = C / (double)T;
  return (raw <= 2.5 * (double)m && z > 0) ? lc[z] : raw;
}

__global__ __launch_bounds__(kSkBlock) void sketch_cardinality_kernel(int64_t rows, int p, double C,
                                                                      const double* __restrict__ lc,
                                                                      const uint32_t* __restrict__ hl,
                                                                      float* __restrict__ out) {
  const int wave = wave_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kSkWaves + wave;
  if (r >= rows) return;
  const int M4 = (1 << p) / 4, R = 33 - p;
  uint32_t t = 0, z = 0;
  for (int col = lane; col < M4; col += 64) word_tz(hl[r * M4 + col], R, t, z);
  const uint64_t acc = wave_sum(pack_tz(t, z));
  if (lane == 0)
    out[r] = (float)cardinality((int64_t)(acc & ((uint64_t(1) << 40) - 1)), (int)(acc >> 40), 1 << p, C, lc);
}

// The per-link tail, shared by sketch_pairs_kernel and sketch_masked_pairs_kernel, in two steps.  pair_estimates, by a
// wavefront that has a link, on the 2 (H + 1) endpoint rows it holds in registers: match, T, z and I_ij (each output
// may be null; int32, int64, int32, fp32, all [L, H+1, H+1]), with I_ij and the endpoints' own E left in LDS.
template <int H, int NC>
__device__ __forceinline__ void pair_estimates(int wave, int lane, int64_t l, int P, int p, double C,
                                               const double* __restrict__ lc, const uint2 (&mu)[H + 1][NC],
                                               const uint2 (&mv)[H + 1][NC], const uint32_t (&hu)[H + 1][NC],
                                               const uint32_t (&hv)[H + 1][NC],
                                               double (&s_i)[kSkWaves][(H + 1) * (H + 1)],
                                               double (&s_e)[kSkWaves][2 * (H + 1)], int32_t* __restrict__ out_match,
                                               int64_t* __restrict__ out_t, int32_t* __restrict__ out_z,
                                               float* __restrict__ out_inter) {
  constexpr int K = H + 1, NP = K * K;
  static_assert(NP + 2 * K <= 64 && H * H + 2 * H <= 64, "one lane per pair and per endpoint row");
  const int P2 = P / 2, m = 1 << p, M4 = m / 4, R = 33 - p;
  {
    int my_match = 0, my_z = 0;
    int64_t my_t = 1;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int j = 0; j < K; ++j) {
        int match = 0;
        uint32_t t = 0, z = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int col = c * 64 + lane;
          const bool in_m = col < P2;
          match += __popcll(__ballot(in_m && mu[i][c].x == mv[j][c].x)) +
                   __popcll(__ballot(in_m && mu[i][c].y == mv[j][c].y));
          if (col < M4) word_tz(max_u8x4(hu[i][c], hv[j][c]), R, t, z);
        }
        const uint64_t acc = wave_sum(pack_tz(t, z));
        if (lane == i * K + j) {
          my_match = match;
          my_t = (int64_t)(acc & ((uint64_t(1) << 40) - 1));
          my_z = (int)(acc >> 40);
        }
      }
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
      for (int i = 0; i < K; ++i) {
        uint32_t t = 0, z = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c * 64 + lane < M4) word_tz(side ? hv[i][c] : hu[i][c], R, t, z);
        const uint64_t acc = wave_sum(pack_tz(t, z));
        if (lane == NP + side * K + i) {
          my_t = (int64_t)(acc & ((uint64_t(1) << 40) - 1));
          my_z = (int)(acc >> 40);
        }
      }
    // lane k < NP: pair k; lanes NP .. NP + 2K - 1: the endpoints' own rows
    const double card = cardinality(my_t, my_z, m, C, lc);
    if (lane < NP) {
      const double inter = ((double)my_match * card) / (double)P;
      s_i[wave][lane] = inter;
      if (out_match) out_match[l * NP + lane] = my_match;
      if (out_t) out_t[l * NP + lane] = my_t;
      if (out_z) out_z[l * NP + lane] = my_z;
      if (out_inter) out_inter[l * NP + lane] = (float)inter;
    } else if (lane < NP + 2 * K) {
      s_e[wave][lane - NP] = card;
    }
  }
}

// pair_features, by every wavefront of the workgroup, with a link or not (it holds the barrier of the LDS hand-over):
// feat fp32 [L, H*H + 2 H] = [A_11 .. A_HH | Bu_1 .. Bu_H | Bv_1 .. Bv_H], may be null.
template <int H>
__device__ __forceinline__ void pair_features(bool live, int wave, int lane, int64_t l,
                                              const double (&s_i)[kSkWaves][(H + 1) * (H + 1)],
                                              const double (&s_e)[kSkWaves][2 * (H + 1)],
                                              float* __restrict__ out_feat) {
  constexpr int K = H + 1;
  __syncthreads();
  if (!live || !out_feat) return;
  const double* I = s_i[wave];
  // A_ij = ((I_ij - I_{i-1,j}) - I_{i,j-1}) + I_{i-1,j-1} with I = 0 at index -1, for i, j in 0..H
  auto at = [&](int i, int j) { return (i < 0 || j < 0) ? 0.0 : I[i * K + j]; };
  auto A = [&](int i, int j) { return ((at(i, j) - at(i - 1, j)) - at(i, j - 1)) + at(i - 1, j - 1); };
  constexpr int F = H * H + 2 * H;
  if (lane < H * H) {
    out_feat[l * F + lane] = (float)A(lane / H + 1, lane % H + 1);
  } else if (lane < F) {
    const int t = lane - H * H, side = t / H, i = t % H + 1;   // side 0: Bu_i, side 1: Bv_i
    double sum = 0.0;
    for (int j = 0; j <= H; ++j) sum += side ? A(j, i) : A(i, j);
    const double* E = s_e[wave] + side * K;
    out_feat[l * F + lane] = (float)((E[i] - E[i - 1]) - sum);
  }
}

// links [2, L]; the outputs are pair_estimates' and pair_features'
template <int H, int NC>
__global__ __launch_bounds__(kSkBlock) void sketch_pairs_kernel(int64_t L, const int32_t* __restrict__ links, int64_t n,
                                                                int P, int p, double C, const double* __restrict__ lc,
                                                                const uint2* __restrict__ mh,
                                                                const uint32_t* __restrict__ hl,
                                                                int32_t* __restrict__ out_match,
                                                                int64_t* __restrict__ out_t, int32_t* __restrict__ out_z,
                                                                float* __restrict__ out_inter,
                                                                float* __restrict__ out_feat) {
  constexpr int K = H + 1, NP = K * K;
  __shared__ double s_i[kSkWaves][NP];        // I_ij
  __shared__ double s_e[kSkWaves][2 * K];     // E(HL_i[u]), then E(HL_j[v])
  const int wave = wave_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t l = (int64_t)blockIdx.x * kSkWaves + wave;
  const bool live = l < L;                    // wave-uniform; a wavefront without a link still meets the barrier
  const int P2 = P / 2, M4 = (1 << p) / 4;
  if (live) {
    const int64_t u = wave_uniform(links[l]), v = wave_uniform(links[L + l]);
    uint2 mu[K][NC], mv[K][NC];
    uint32_t hu[K][NC], hv[K][NC];
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = c * 64 + lane;
        const bool in_m = col < P2, in_h = col < M4;
        mu[i][c] = in_m ? mh[((int64_t)i * n + u) * P2 + col] : make_uint2(0u, 0u);
        mv[i][c] = in_m ? mh[((int64_t)i * n + v) * P2 + col] : make_uint2(0u, 0u);
        hu[i][c] = in_h ? hl[((int64_t)i * n + u) * M4 + col] : 0u;
        hv[i][c] = in_h ? hl[((int64_t)i * n + v) * M4 + col] : 0u;
      }
    pair_estimates<H, NC>(wave, lane, l, P, p, C, lc, mu, mv, hu, hv, s_i, s_e, out_match, out_t, out_z, out_inter);
  }
  pair_features<H>(live, wave, lane, l, s_i, s_e, out_feat);
}

// Whether the ascending, distinct keys idx[begin, end) hold `key`, decided by the whole wavefront: 64 evenly spaced
// probes narrow the range 64-fold per trip (the lanes whose probe is <= key are a prefix), the last trip compares 64
// consecutive keys.  A row of at most 64 keys is one load.  The answer is the same in every lane.
__device__ __forceinline__ bool row_holds(int lane, const int32_t* __restrict__ idx, int begin, int end, int key) {
  int64_t lo = begin, hi = end;
  while (hi - lo > 64) {
    const int64_t step = (hi - lo + 63) / 64, pos = lo + lane * step;
    const int below = __popcll(__ballot(pos < hi && idx[pos] <= key));
    if (below == 0) return false;
    lo += (below - 1) * step;
    hi = min(hi, lo + step);
  }
  return __ballot(lo + lane < hi && idx[lo + lane] == key) != 0;
}

// neighbours a wavefront loads before it reduces them in the masked walk: kBatch, fewer where a neighbour is more
// than two (MinHash, HLL) column loads per lane, so that at most eight such pairs are in flight and held in registers
template <int H, int NC>
constexpr int masked_batch() { return H * NC <= 2 ? kBatch : H * NC >= 8 ? 1 : 8 / (H * NC); }

// One wavefront's share of a masked endpoint x: keys [begin, end) of row x except x itself and the partner y.  Hop h
// (h < H) of every key kept is reduced into am[h] / ah[h], which the caller starts at the identities: MH_0 / HL_0 and,
// for H = 2, MH_1 / HL_1 of a neighbour in the same trip.  The keys are loaded 64 at a time; the ballot of the keys
// kept is walked bit by bit and each key handed round by readlane, so a skipped key costs no load and no batch slot.
template <int H, int NC>
__device__ __forceinline__ void masked_reduce_keys(int lane, int x, int y, int begin, int end,
                                                   const int32_t* __restrict__ idx, int64_t n, int P2, int M4,
                                                   const uint2* __restrict__ mh, const uint32_t* __restrict__ hl,
                                                   uint2 (&am)[H][NC], uint32_t (&ah)[H][NC]) {
  constexpr int NB = masked_batch<H, NC>();
  for (int e0 = begin; e0 < end; e0 += 64) {
    const bool have = e0 + lane < end;
    const int mine = have ? idx[e0 + lane] : 0;
    uint64_t keep = __ballot(have && mine != x && mine != y);
    while (__popcll(keep) >= NB) {             // NB neighbours in flight: the loads do not wait for each other
      uint2 tm[NB][H][NC];
      uint32_t th[NB][H][NC];
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        const int64_t w = __builtin_amdgcn_readlane(mine, __builtin_ctzll(keep));
        keep &= keep - 1;
#pragma unroll
        for (int h = 0; h < H; ++h)
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const int col = c * 64 + lane;
            tm[q][h][c] = col < P2 ? mh[((int64_t)h * n + w) * P2 + col] : make_uint2(0u, 0u);
            th[q][h][c] = col < M4 ? hl[((int64_t)h * n + w) * M4 + col] : 0u;
          }
      }
#pragma unroll
      for (int q = 0; q < NB; ++q)
#pragma unroll
        for (int h = 0; h < H; ++h)
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const int col = c * 64 + lane;
            if (col < P2) am[h][c] = min_u32x2(am[h][c], tm[q][h][c]);
            if (col < M4) ah[h][c] = max_u8x4(ah[h][c], th[q][h][c]);
          }
    }
    while (keep) {
      const int64_t w = __builtin_amdgcn_readlane(mine, __builtin_ctzll(keep));
      keep &= keep - 1;
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int col = c * 64 + lane;
          if (col < P2) am[h][c] = min_u32x2(am[h][c], mh[((int64_t)h * n + w) * P2 + col]);
          if (col < M4) ah[h][c] = max_u8x4(ah[h][c], hl[((int64_t)h * n + w) * M4 + col]);
        }
    }
  }
}

template <int H, int NC>
__device__ __forceinline__ void masked_identity(uint2 (&am)[H][NC], uint32_t (&ah)[H][NC]) {
#pragma unroll
  for (int h = 0; h < H; ++h)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      am[h][c] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
      ah[h][c] = 0u;
    }
}

// rows 1..H of a masked endpoint from its hop 0 and the walk's reductions: MH'_1 = min(MH_0, am[0]),
// MH'_2 = min(MH'_1, am[1]); HL' the same with max
template <int H, int NC>
__device__ __forceinline__ void masked_rows(uint2 (&m)[H + 1][NC], uint32_t (&h)[H + 1][NC], const uint2 (&am)[H][NC],
                                            const uint32_t (&ah)[H][NC]) {
#pragma unroll
  for (int i = 1; i <= H; ++i)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      m[i][c] = min_u32x2(m[i - 1][c], am[i - 1][c]);
      h[i][c] = max_u8x4(h[i - 1][c], ah[i - 1][c]);
    }
}

// sketch_pairs_kernel on the graph without the link's own entries, H <= 2.  ptr / idx: the CSR
// the tables were built from, rows ascending and distinct.  Per link and endpoint x with partner y, wave-uniform:
//   (x, y) not stored               rows 0..H from the tables, as sketch_pairs_kernel loads them
//   stored, at most kSplitKeys keys the wavefront walks row x itself
//   stored, a longer row            the workgroup's four wavefronts walk a quarter of the keys each and the link's own
//                                   wavefront combines the partial rows from LDS
// Which long rows there are goes through LDS, so every wavefront takes the same trips through the barriers whatever
// its own link is.  min / max are idempotent: any split gives the same bits, and there are no atomics.
template <int H, int NC>
__global__ __launch_bounds__(kSkBlock) void sketch_masked_pairs_kernel(
    int64_t L, const int32_t* __restrict__ links, int64_t n, const int64_t* __restrict__ ptr,
    const int32_t* __restrict__ idx, int P, int p, double C, const double* __restrict__ lc,
    const uint2* __restrict__ mh, const uint32_t* __restrict__ hl, int32_t* __restrict__ out_match,
    int64_t* __restrict__ out_t, int32_t* __restrict__ out_z, float* __restrict__ out_inter,
    float* __restrict__ out_feat) {
  static_assert(H <= 2, "beyond hops 2 the rows of an endpoint's neighbours change too");
  constexpr int K = H + 1, NP = K * K;
  __shared__ double s_i[kSkWaves][NP];
  __shared__ double s_e[kSkWaves][2 * K];
  __shared__ int s_long[kSkWaves];            // bit `side` of a wavefront's word: that endpoint's walk is the workgroup's
  __shared__ uint2 part_m[kSkWaves][H][64 * NC];
  __shared__ uint32_t part_h[kSkWaves][H][64 * NC];
  const int wave = wave_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t l = (int64_t)blockIdx.x * kSkWaves + wave;
  const bool live = l < L;
  const int P2 = P / 2, M4 = (1 << p) / 4;
  uint2 rm[2][K][NC];                         // [0]: u's rows, [1]: v's
  uint32_t rh[2][K][NC];
  int deferred = 0;
  if (live) {
    const int u = wave_uniform(links[l]), v = wave_uniform(links[L + l]);
    int first[2], last[2];
    bool held[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {    // both searches before any row load, so that neither waits for rows
      const int x = side ? v : u;
      first[side] = wave_uniform((int)ptr[x]);
      last[side] = wave_uniform((int)ptr[x + 1]);
      held[side] = row_holds(lane, idx, first[side], last[side], side ? u : v);
    }
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int x = side ? v : u, y = side ? u : v, begin = first[side], end = last[side];
      const bool stored = held[side];
      const int top = stored ? 0 : H;         // the table rows this endpoint keeps
#pragma unroll
      for (int i = 0; i < K; ++i)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int col = c * 64 + lane;
          rm[side][i][c] = i <= top && col < P2 ? mh[((int64_t)i * n + x) * P2 + col] : make_uint2(0u, 0u);
          rh[side][i][c] = i <= top && col < M4 ? hl[((int64_t)i * n + x) * M4 + col] : 0u;
        }
      if (stored && end - begin <= kSplitKeys) {
        uint2 am[H][NC];
        uint32_t ah[H][NC];
        masked_identity<H, NC>(am, ah);
        masked_reduce_keys<H, NC>(lane, x, y, begin, end, idx, n, P2, M4, mh, hl, am, ah);
        masked_rows<H, NC>(rm[side], rh[side], am, ah);
      } else if (stored) {
        deferred |= 1 << side;
      }
    }
  }
  if (lane == 0) s_long[wave] = deferred;
  __syncthreads();
  for (int q = 0; q < kSkWaves; ++q) {        // every wavefront of the workgroup takes the same path from here on
    const int todo = wave_uniform(s_long[q]);
    if (!todo) continue;
    const int64_t lq = (int64_t)blockIdx.x * kSkWaves + q;
    const int u = wave_uniform(links[lq]), v = wave_uniform(links[L + lq]);
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      if (!(todo >> side & 1)) continue;
      const int x = side ? v : u, y = side ? u : v;
      const int begin = wave_uniform((int)ptr[x]), end = wave_uniform((int)ptr[x + 1]);
      const int share = (end - begin + kSkWaves - 1) / kSkWaves;
      const int b = min(end, begin + wave * share), e = min(end, b + share);
      uint2 am[H][NC];
      uint32_t ah[H][NC];
      masked_identity<H, NC>(am, ah);
      masked_reduce_keys<H, NC>(lane, x, y, b, e, idx, n, P2, M4, mh, hl, am, ah);
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          part_m[wave][h][c * 64 + lane] = am[h][c];
          part_h[wave][h][c * 64 + lane] = ah[h][c];
        }
      __syncthreads();
      if (wave == q) {
#pragma unroll
        for (int h = 0; h < H; ++h)
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int w = 0; w < kSkWaves; ++w) {
              am[h][c] = min_u32x2(am[h][c], part_m[w][h][c * 64 + lane]);
              ah[h][c] = max_u8x4(ah[h][c], part_h[w][h][c * 64 + lane]);
            }
        masked_rows<H, NC>(rm[side], rh[side], am, ah);
      }
      __syncthreads();
    }
  }
  if (live)
    pair_estimates<H, NC>(wave, lane, l, P, p, C, lc, rm[0], rm[1], rh[0], rh[1], s_i, s_e, out_match, out_t, out_z,
                          out_inter);
  pair_features<H>(live, wave, lane, l, s_i, s_e, out_feat);
}

bool bad_shape(int64_t num_nodes, int32_t hops, int32_t num_perm, int32_t hll_p) {
  return num_nodes < 1 || num_nodes > S3GRL_SKETCH_MAX_NODES || hops < 1 || hops > S3GRL_SKETCH_MAX_HOPS ||
         num_perm < 64 || num_perm > 512 || num_perm % 64 || hll_p < 7 || hll_p > 10;
}

int cols_per_lane(int32_t num_perm, int32_t hll_p) {
  const int words = std::max(num_perm / 2, (1 << hll_p) / 4);
  return words <= 64 ? 1 : words <= 128 ? 2 : 4;
}

// every endpoint is checked on the host before any GPU work
s3grl_status check_links(s3grl_context* ctx, const int32_t* links, int64_t num_links, int64_t num_nodes) {
  return check_ids(ctx, links, 2 * num_links, num_nodes, "sketch: a link endpoint outside [0, N)");
}

template <int H>
void launch_pairs(int nc, dim3 grid, hipStream_t st, int64_t L, const int32_t* links, int64_t n, int P, int p, double C,
                  const double* lc, const uint2* mh, const uint32_t* hl, int32_t* match, int64_t* t, int32_t* z,
                  float* inter, float* feat) {
  auto* k = nc == 1 ? sketch_pairs_kernel<H, 1> : nc == 2 ? sketch_pairs_kernel<H, 2> : sketch_pairs_kernel<H, 4>;
  hipLaunchKernelGGL(k, grid, dim3(kSkBlock), 0, st, L, links, n, P, p, C, lc, mh, hl, match, t, z, inter, feat);
}

template <int H>
void launch_masked_pairs(int nc, dim3 grid, hipStream_t st, int64_t L, const int32_t* links, int64_t n,
                         const int64_t* ptr, const int32_t* idx, int P, int p, double C, const double* lc,
                         const uint2* mh, const uint32_t* hl, int32_t* match, int64_t* t, int32_t* z, float* inter,
                         float* feat) {
  auto* k = nc == 1 ? sketch_masked_pairs_kernel<H, 1>
            : nc == 2 ? sketch_masked_pairs_kernel<H, 2> : sketch_masked_pairs_kernel<H, 4>;
  hipLaunchKernelGGL(k, grid, dim3(kSkBlock), 0, st, L, links, n, ptr, idx, P, p, C, lc, mh, hl, match, t, z, inter,
                     feat);
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

extern "C" {

s3grl_status s3grl_sketch_build(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                                int64_t num_entries, int32_t hops, int32_t num_perm, int32_t hll_p, uint32_t seed,
                                uint32_t* minhash, uint8_t* hll) {
  if (!ctx || !indptr || !minhash || !hll || num_entries < 0 || (num_entries > 0 && !indices) ||
      num_entries >= (int64_t(1) << 31) || bad_shape(num_nodes, hops, num_perm, hll_p)) {
    set_last_error("sketch: need 1 <= N <= 2^24, nnz < 2^31, 1 <= hops <= 4, num_perm a multiple of 64 in [64, 512] "
                   "and 7 <= hll_p <= 10");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  {   // the kernels trust the CSR: it is checked on the host once
    std::vector<int64_t> ip;
    std::vector<int32_t> ix;
    S3GRL_TRY(check_csr(ctx, num_nodes, indptr, indices, num_entries, /*ascending=*/false,
                        "sketch: malformed CSR (indptr not monotone from 0 to nnz, or a column outside [0, N))", &ip,
                        &ix));
  }
  const int P2 = num_perm / 2, M4 = (1 << hll_p) / 4, nc = cols_per_lane(num_perm, hll_p);
  const int64_t mh_hop = num_nodes * P2, hl_hop = num_nodes * M4;   // in uint2 / uint32 words
  auto* mh = reinterpret_cast<uint2*>(minhash);
  auto* hl = reinterpret_cast<uint32_t*>(hll);
  const int64_t items = num_nodes * std::max<int64_t>(num_perm, M4);
  hipLaunchKernelGGL(sketch_init_kernel, dim3(std::min<unsigned>(grid_of(items, kSkBlock), 1u << 16)), dim3(kSkBlock),
                     0, st, num_nodes, num_perm, hll_p, seed, minhash, hl);
  S3GRL_HIP_TRY(hipGetLastError());
  auto* k = nc == 1 ? sketch_propagate_kernel<1> : nc == 2 ? sketch_propagate_kernel<2> : sketch_propagate_kernel<4>;
  for (int i = 1; i <= hops; ++i) {
    hipLaunchKernelGGL(k, dim3(grid_of(num_nodes, kSkWaves)), dim3(kSkBlock), 0, st, num_nodes, indptr, indices, P2,
                       M4, mh + (i - 1) * mh_hop, hl + (i - 1) * hl_hop, mh + i * mh_hop, hl + i * hl_hop);
    S3GRL_HIP_TRY(hipGetLastError());
  }
  return S3GRL_OK;
}

s3grl_status s3grl_sketch_cardinality(s3grl_context* ctx, int32_t hll_p, const double* lc, double c,
                                      const uint8_t* registers, int64_t num_rows, float* out) {
  if (!ctx || hll_p < 7 || hll_p > 10 || !lc || num_rows < 0 || (num_rows > 0 && (!registers || !out)) ||
      num_rows > (int64_t(1) << 31))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_rows == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(sketch_cardinality_kernel, dim3(grid_of(num_rows, kSkWaves)), dim3(kSkBlock), 0, ctx->stream,
                     num_rows, hll_p, c, lc, reinterpret_cast<const uint32_t*>(registers), out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_sketch_pairs(s3grl_context* ctx, int64_t num_nodes, int32_t hops, int32_t num_perm, int32_t hll_p,
                                const uint32_t* minhash, const uint8_t* hll, const double* lc, double c,
                                const int32_t* links, int64_t num_links, int32_t* match, int64_t* t, int32_t* z,
                                float* intersections, float* features) {
  if (!ctx || !minhash || !hll || !lc || num_links < 0 || (num_links > 0 && !links) ||
      num_links >= (int64_t(1) << 31) || bad_shape(num_nodes, hops, num_perm, hll_p))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_links == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  S3GRL_TRY(check_links(ctx, links, num_links, num_nodes));
  const dim3 grid(grid_of(num_links, kSkWaves));
  const int nc = cols_per_lane(num_perm, hll_p);
  auto* mh = reinterpret_cast<const uint2*>(minhash);
  auto* hl = reinterpret_cast<const uint32_t*>(hll);
  auto* launch = hops == 1 ? launch_pairs<1> : hops == 2 ? launch_pairs<2> : hops == 3 ? launch_pairs<3> : launch_pairs<4>;
  launch(nc, grid, st, num_links, links, num_nodes, num_perm, hll_p, c, lc, mh, hl, match, t, z, intersections,
         features);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_masked_sketch_pairs(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr,
                                       const int32_t* indices, int64_t num_entries, int32_t hops, int32_t num_perm,
                                       int32_t hll_p, const uint32_t* minhash, const uint8_t* hll, const double* lc,
                                       double c, const int32_t* links, int64_t num_links, int32_t* match, int64_t* t,
                                       int32_t* z, float* intersections, float* features) {
  if (bad_shape(num_nodes, hops, num_perm, hll_p) || num_entries < 0 || num_entries >= (int64_t(1) << 31) ||
      num_links < 0 || num_links >= (int64_t(1) << 31))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (hops > 2) {
    set_last_error("sketch: masking a link's own edge is exact on the unmasked tables for hops <= 2 only (beyond, "
                   "the rows of an endpoint's neighbours change too)");
    return S3GRL_ERR_NOT_IMPLEMENTED;
  }
  if (!ctx || !indptr || (num_entries > 0 && !indices) || !minhash || !hll || !lc || (num_links > 0 && !links))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_links == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  S3GRL_TRY(check_links(ctx, links, num_links, num_nodes));
  const dim3 grid(grid_of(num_links, kSkWaves));
  const int nc = cols_per_lane(num_perm, hll_p);
  auto* mh = reinterpret_cast<const uint2*>(minhash);
  auto* hl = reinterpret_cast<const uint32_t*>(hll);
  auto* launch = hops == 1 ? launch_masked_pairs<1> : launch_masked_pairs<2>;
  launch(nc, grid, st, num_links, links, num_nodes, indptr, indices, num_perm, hll_p, c, lc, mh, hl, match, t, z,
         intersections, features);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

}  // extern "C"
