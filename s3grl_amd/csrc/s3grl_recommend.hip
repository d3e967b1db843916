// Top-K link recommendation on gfx950: which new links does a node most likely have?  Two kernels; everything
// between them (precompute, SIGNNet scores, the heuristics) is the existing code.
//
//   candidates_kernel   one workgroup per source u: a level-synchronous BFS over the undirected CSR with TWO N-bit
//                       bitmaps A and B that together hold two bits of state per node:
//                           (A, B) = (0, 0) not reached   (1, 0) reached at an earlier level
//                                    (1, 1) the frontier  (0, 1) reached at this level
//                       A level walks the rows of the frontier (A & B) and sets B where A is clear, so A is read-only
//                       while a level runs and A & B does not change under the walkers' feet; the step between two
//                       levels is A |= B, B &= ~A(old) on the words a thread owns.  Rows of up to kSerialRow entries
//                       are walked by the lane that owns the frontier word, longer ones by the whole wavefront.  After
//                       h levels A is the ball of radius h; u, its row and the excluded pairs (a binary search over
//                       the sorted keys min·N + max) are cleared from it, and what is left is the segment.  A count
//                       launch writes the segment's length; after the host's exclusive scan a fill launch repeats the
//                       same walk and writes the set bits in ascending id order at the scanned offset: a popcount
//                       scan over the bitmap words (DPP wave scan, wave totals in a small LDS table, one barrier per
//                       chunk of T words), the idiom of count_balls_kernel.  No sort, no float, no atomics on output:
//                       two runs give the same bytes.
//                       The bitmaps live in LDS up to 524 288 nodes (2 x 64 KiB, the bound of the LDS bitmaps in
//                       s3grl_relabel.hip / s3grl_segsort.hip), beyond in an HBM workspace: one slice of 2 N bits per
//                       resident workgroup, zeroed by the launch, cleared again by the workgroup after every source
//                       it takes (the workgroups stride over the sources).
//   segment_topk_kernel one workgroup per segment: order = score descending, then position ascending.  Scores map to
//                       an order-preserving 32-bit key (-0.0 as +0.0, every NaN below -inf).  A segment of up to
//                       kTopSort entries is sorted whole in LDS (bitonic, 64-bit keys (~key << 32 | position)).  A
//                       longer one: an MSB-first radix select of the k-th key (four 8-bit digits, a 256-bin LDS
//                       histogram each), then one ordered sweep that collects the keys above the threshold and the
//                       lowest-position ties, and the same bitonic sort over the <= k survivors.  Integer LDS atomics
//                       only (the histograms and the slot counter of the keys above the threshold, whose order the
//                       sort settles): a call repeated gives the same bytes.
#include "s3grl_device.hpp"

#include <algorithm>

namespace s3grl {
namespace {

constexpr int64_t kCandLdsNodes = 524288;   // two bitmaps of N bits in LDS up to here
constexpr int kCandMaxHops = 8;
constexpr int kSerialRow = 16;              // rows up to this long are walked by one lane
constexpr int kCandResident = 512;          // workgroups of the HBM flavour: 256 CUs x 2 (1024 threads each)

constexpr int kTopT = 256;
constexpr int kTopSort = 2048;              // segments up to this long are sorted whole in LDS
constexpr int kTopMaxK = 1024;

int cand_threads(int64_t W) { return W <= 128 ? 64 : W <= 4096 ? 256 : 1024; }

// inclusive scan of one int over the wavefront on the DPP path (see wave_incl_scan in s3grl_balls.hip)
__device__ __forceinline__ int wave_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
  return v;
}

// Bitmap words in LDS or in an HBM slice (G).  Wavefronts read words that others OR into during a level, so every
// access is a relaxed atomic: workgroup scope in LDS (the same ds_read / ds_write as a plain access), agent scope in
// HBM, so that a word another wavefront of the workgroup has set is never served from a stale vector-L1 line.
template <bool G>
struct Word {
  static constexpr int kScope = G ? __HIP_MEMORY_SCOPE_AGENT : __HIP_MEMORY_SCOPE_WORKGROUP;
  static __device__ __forceinline__ uint32_t load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, kScope);
  }
  static __device__ __forceinline__ void store(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, kScope);
  }
  static __device__ __forceinline__ void set(uint32_t* p, uint32_t m) {
    (void)__hip_atomic_fetch_or(p, m, __ATOMIC_RELAXED, kScope);
  }
  static __device__ __forceinline__ void clear(uint32_t* p, uint32_t m) {
    (void)__hip_atomic_fetch_and(p, ~m, __ATOMIC_RELAXED, kScope);
  }
};

__device__ __forceinline__ bool excluded(const uint64_t* __restrict__ keys, int64_t E, uint64_t key) {
  int64_t lo = 0, hi = E;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < E && keys[lo] == key;
}

// err: 1 a source outside [0, N); 2 (fill) a segment of seg_ptr that is not as long as the walk finds it
template <int T, bool G, bool FILL>
__global__ __launch_bounds__(T) void candidates_kernel(const int32_t* __restrict__ indptr,
                                                       const int32_t* __restrict__ indices, int N, int W,
                                                       const int32_t* __restrict__ sources, int64_t S, int hops,
                                                       const uint64_t* __restrict__ excl, int64_t E,
                                                       uint32_t* __restrict__ slices, int32_t* __restrict__ cnt,
                                                       const int64_t* __restrict__ seg_ptr,
                                                       int32_t* __restrict__ cand, int32_t* __restrict__ err) {
  constexpr int NW = T / 64;
  extern __shared__ uint32_t smem[];
  __shared__ int sh[NW];
  __shared__ int tab[2][NW];
  const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  uint32_t* A = G ? slices + (int64_t)blockIdx.x * 2 * W : smem;
  uint32_t* B = A + W;
  using M = Word<G>;
  for (int64_t i = blockIdx.x; i < S; i += gridDim.x) {
    const int u = sources[i];
    if (u < 0 || u >= N) {   // uniform
      if (tid == 0) {
        atomicMax(err, 1);
        if (!FILL) cnt[i] = 0;
      }
      continue;
    }
    if (!G) {
      for (int w = tid; w < 2 * W; w += T) A[w] = 0u;
      __syncthreads();
    }
    if (tid == 0) {
      M::store(A + (u >> 5), 1u << (u & 31));
      M::store(B + (u >> 5), 1u << (u & 31));
    }
    __syncthreads();
    auto visit = [&](int v) {
      const uint32_t bit = 1u << (v & 31);
      if (((M::load(A + (v >> 5)) | M::load(B + (v >> 5))) & bit) == 0u) M::set(B + (v >> 5), bit);
    };
    for (int d = 1; d <= hops; ++d) {
      for (int c0 = wid * 64; c0 < W; c0 += T) {   // a wavefront per 64 words
        const int w = c0 + lane;
        uint32_t f = w < W ? (M::load(A + w) & M::load(B + w)) : 0u;
        uint32_t big = 0u;
        while (f) {
          const int b = __ffs(f) - 1;
          f &= f - 1;
          const int x = w * 32 + b;
          const int e0 = indptr[x], e1 = indptr[x + 1];
          if (e1 - e0 > kSerialRow) {
            big |= 1u << b;
            continue;
          }
          for (int e = e0; e < e1; ++e) visit(indices[e]);
        }
        unsigned long long m = __ballot(big != 0u);
        while (m) {   // the long rows of the chunk, one after the other, all lanes on one row
          const int l = __ffsll(m) - 1;
          m &= m - 1;
          uint32_t bw = (uint32_t)__shfl((int)big, l);
          while (bw) {
            const int b = __ffs(bw) - 1;
            bw &= bw - 1;
            const int x = (c0 + l) * 32 + b;
            const int e1 = indptr[x + 1];
            for (int e = indptr[x] + lane; e < e1; e += 64) visit(indices[e]);
          }
        }
      }
      __syncthreads();
      int fresh = 0;
      for (int w = tid; w < W; w += T) {
        const uint32_t b = M::load(B + w);
        if (b == 0u) continue;
        const uint32_t a = M::load(A + w);
        M::store(A + w, a | b);
        M::store(B + w, b & ~a);
        fresh |= (b & ~a) != 0u;
      }
      if (!__syncthreads_or(fresh)) break;   // (also the barrier between the levels)
    }
    // u itself and its neighbours are no candidates
    if (tid == 0) M::clear(A + (u >> 5), 1u << (u & 31));
    for (int e = indptr[u] + tid, e1 = indptr[u + 1]; e < e1; e += T) {
      const int v = indices[e];
      M::clear(A + (v >> 5), 1u << (v & 31));
    }
    __syncthreads();
    int mine = 0;
    for (int w = tid; w < W; w += T) {
      uint32_t a = M::load(A + w);
      if (E > 0 && a) {
        uint32_t keep = a, rest = a;
        while (rest) {
          const int b = __ffs(rest) - 1;
          rest &= rest - 1;
          const int v = w * 32 + b;
          const uint64_t lo = (uint64_t)min(u, v), hi = (uint64_t)max(u, v);
          if (excluded(excl, E, lo * (uint64_t)N + hi)) keep &= ~(1u << b);
        }
        if (keep != a) M::store(A + w, keep);
        a = keep;
      }
      mine += __popc(a);
    }
    const int total = block_sum<T>(mine, sh);   // (its barriers also publish the filtered words)
    if (!FILL) {
      if (tid == 0) cnt[i] = total;
    } else {
      const int64_t base = seg_ptr[i];
      if (seg_ptr[i + 1] - base != (int64_t)total || base < 0) {   // uniform
        if (tid == 0) atomicMax(err, 2);
      } else {
        int32_t* out = cand + base;
        int run = 0, par = 0;
        for (int c0 = 0; c0 < W; c0 += T) {   // ascending ids: word order, chunk by chunk, wave by wave
          const int w = c0 + tid;
          uint32_t a = w < W ? M::load(A + w) : 0u;
          const int c = __popc(a);
          const int inc = wave_scan(c);
          if (lane == 63) tab[par][wid] = inc;
          __syncthreads();
          int before = 0, chunk = 0;
#pragma unroll
          for (int j = 0; j < NW; ++j) {
            const int s = tab[par][j];
            before += j < wid ? s : 0;
            chunk += s;
          }
          int p = run + before + inc - c;
          while (a) {
            const int b = __ffs(a) - 1;
            a &= a - 1;
            out[p++] = w * 32 + b;
          }
          run += chunk;
          par ^= 1;
        }
      }
    }
    if (G) {   // leave the slice zeroed for the next source
      __syncthreads();
      for (int w = tid; w < 2 * W; w += T) M::store(A + w, 0u);
      __syncthreads();
    }
  }
}

// ---- segment top-K -------------------------------------------------------------------------------------------

// larger key = better: +inf > ... > +0.0 = -0.0 > ... > -inf > NaN
__device__ __forceinline__ uint32_t order_key(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ascending order of these = key descending, then position ascending
__device__ __forceinline__ uint64_t sort_word(uint32_t key, uint32_t pos) { return ((uint64_t)(~key) << 32) | pos; }

// ascending bitonic sort of s[0, M), M a power of two
__device__ __forceinline__ void bitonic_sort(uint64_t* s, int M) {
  for (int k2 = 2; k2 <= M; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (M >> 1); t += kTopT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t x = s[i], y = s[l];
        if ((x > y) == ((i & k2) == 0)) {
          s[i] = y;
          s[l] = x;
        }
      }
      __syncthreads();
    }
}

// err: 1 seg_ptr not monotone, negative, beyond num_pairs, or a segment of 2^31 entries or more
__global__ __launch_bounds__(kTopT) void segment_topk_kernel(const float* __restrict__ scores,
                                                             const int64_t* __restrict__ seg_ptr,
                                                             const int32_t* __restrict__ cand, int64_t P, int k,
                                                             int32_t* __restrict__ top_nodes,
                                                             float* __restrict__ top_scores,
                                                             int32_t* __restrict__ top_count,
                                                             int32_t* __restrict__ err) {
  constexpr int NW = kTopT / 64;
  __shared__ uint64_t s[kTopSort];
  __shared__ int hist[256];
  __shared__ int sh[NW];
  __shared__ int tab[2][NW];
  __shared__ int pick[4][2];   // per pass of the radix select: the selected digit and what is still to take inside it
  __shared__ int n_above;
  const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
  const int64_t seg = blockIdx.x;
  const int64_t b0 = seg_ptr[seg], b1 = seg_ptr[seg + 1];
  int n = 0;
  if (b0 < 0 || b1 < b0 || b1 > P || b1 - b0 >= ((int64_t)1 << 31)) {
    if (tid == 0) atomicMax(err, 1);
  } else {
    n = (int)(b1 - b0);
  }
  const float* __restrict__ sc = scores + b0;
  const int kk = min(k, n);
  if (n > 0 && n <= kTopSort) {
    int M = 2;
    while (M < n) M <<= 1;
    for (int j = tid; j < M; j += kTopT) s[j] = j < n ? sort_word(order_key(sc[j]), (uint32_t)j) : ~0ull;
    __syncthreads();
    bitonic_sort(s, M);
  } else if (n > kTopSort) {
    // the kk-th largest key, digit by digit from the top
    uint32_t prefix = 0u, mask = 0u;
    int rem = kk;
    if (tid < 4) {   // a slot per pass: a pass's pick is written once and never again, so reading it needs no
      pick[tid][0] = 0;   // barrier against the next pass
      pick[tid][1] = 1;
    }
    for (int shift = 24, pass = 0; shift >= 0; shift -= 8, ++pass) {
      hist[tid] = 0;   // (every thread read its bin of the pass before ahead of block_excl_scan's barriers)
      __syncthreads();
      for (int j = tid; j < n; j += kTopT) {
        const uint32_t key = order_key(sc[j]);
        if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
      }
      __syncthreads();
      const int digit = 255 - tid, h = hist[digit];
      int tot;
      const int above = block_excl_scan<kTopT>(h, sh, tot);   // keys of this prefix with a larger digit
      if (above < rem && rem <= above + h) {                  // exactly one thread
        pick[pass][0] = digit;
        pick[pass][1] = rem - above;
      }
      __syncthreads();
      prefix |= (uint32_t)pick[pass][0] << shift;
      mask |= 255u << shift;
      rem = pick[pass][1];   // 1 <= rem <= what the pass before left: the same value in every thread
    }
    // every key above the threshold, and of the keys equal to it the `rem` of lowest position
    const int first_tie = kk - rem;
    if (tid == 0) n_above = 0;
    __syncthreads();
    int ties = 0, par = 0;
    for (int c0 = 0; c0 < n; c0 += kTopT) {
      const int j = c0 + tid;
      const uint32_t key = j < n ? order_key(sc[j]) : 0u;
      if (j < n && key > prefix) {
        const int slot = atomicAdd(&n_above, 1);   // exactly first_tie of them
        if (slot < first_tie) s[slot] = sort_word(key, (uint32_t)j);
      }
      if (ties < rem) {   // uniform
        const bool tie = j < n && key == prefix;
        const unsigned long long m = __ballot(tie);
        if (lane == 0) tab[par][wid] = __popcll(m);
        __syncthreads();
        int before = 0, chunk = 0;
#pragma unroll
        for (int q = 0; q < NW; ++q) {
          const int c = tab[par][q];
          before += q < wid ? c : 0;
          chunk += c;
        }
        const int rank = ties + before + __popcll(m & ((1ull << lane) - 1ull));
        if (tie && rank < rem) s[first_tie + rank] = sort_word(key, (uint32_t)j);
        ties += chunk;
        par ^= 1;
      }
    }
    int M = 2;
    while (M < kk) M <<= 1;
    for (int j = kk + tid; j < M; j += kTopT) s[j] = ~0ull;
    __syncthreads();
    bitonic_sort(s, M);
  }
  for (int j = tid; j < k; j += kTopT) {
    const int64_t o = seg * k + j;
    if (j < kk) {
      const uint32_t pos = (uint32_t)s[j];
      top_nodes[o] = cand[b0 + pos];
      top_scores[o] = sc[pos];
    } else {
      top_nodes[o] = -1;
      top_scores[o] = -INFINITY;
    }
  }
  if (tid == 0) top_count[seg] = kk;
}

struct CandLayout {
  bool hbm;
  int64_t words;      // of one bitmap
  int threads;
  int64_t lds_bytes, slice_bytes;
};

CandLayout cand_layout(int64_t num_nodes) {
  CandLayout l;
  l.hbm = num_nodes > kCandLdsNodes;
  l.words = (num_nodes + 31) / 32;
  l.threads = cand_threads(l.words);
  l.lds_bytes = l.hbm ? 0 : 2 * l.words * 4;
  l.slice_bytes = l.hbm ? 2 * l.words * 4 : 0;
  return l;
}

template <bool FILL>
s3grl_status launch_candidates(s3grl_context* ctx, const s3grl_graph* g, const int32_t* sources, int64_t S, int hops,
                               const uint64_t* excl, int64_t E, uint32_t* slices, int grid, int32_t* cnt,
                               const int64_t* seg_ptr, int32_t* cand, int32_t* err) {
  const CandLayout l = cand_layout(g->num_nodes);
  const int N = (int)g->num_nodes, W = (int)l.words;
  auto launch = [&](auto kern, int T) -> s3grl_status {
    if (l.lds_bytes > 65536 - 1024)
      S3GRL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)l.lds_bytes));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(T), (size_t)l.lds_bytes, ctx->stream, g->indptr, g->indices, N,
                       W, sources, S, hops, excl, E, slices, cnt, seg_ptr, cand, err);
    S3GRL_HIP_TRY(hipGetLastError());
    return S3GRL_OK;
  };
  if (l.hbm) return launch(candidates_kernel<1024, true, FILL>, 1024);
  if (l.threads == 64) return launch(candidates_kernel<64, false, FILL>, 64);
  if (l.threads == 256) return launch(candidates_kernel<256, false, FILL>, 256);
  return launch(candidates_kernel<1024, false, FILL>, 1024);
}

s3grl_status check_candidates_args(const s3grl_context* ctx, const s3grl_graph* g, const int32_t* sources, int64_t S,
                                   int32_t hops, const uint64_t* excl, int64_t E, const int64_t* seg_ptr) {
  if (hops > kCandMaxHops) {
    set_last_error("candidates: hops <= 8");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (hops < 2) {
    set_last_error("candidates: hops >= 2 (distance 1 is the graph itself)");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (!ctx || !g || S < 0 || E < 0 || (S > 0 && !sources) || (E > 0 && !excl) || !seg_ptr || S >= ((int64_t)1 << 31))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (g->directed) {
    set_last_error("candidates: directed graphs are not implemented");
    return S3GRL_ERR_NOT_IMPLEMENTED;
  }
  return S3GRL_OK;
}

// the HBM flavour's slices (zeroed) and its grid; nothing and one workgroup per source for the LDS flavour
s3grl_status cand_workspace(s3grl_context* ctx, const s3grl_graph* g, int64_t S, Transient& tmp, uint32_t** slices,
                            int* grid) {
  const CandLayout l = cand_layout(g->num_nodes);
  *slices = nullptr;
  *grid = (int)S;
  if (!l.hbm) return S3GRL_OK;
  *grid = (int)std::min<int64_t>(S, kCandResident);
  void* q = nullptr;
  S3GRL_TRY(ctx->arena.alloc((size_t)*grid * (size_t)l.slice_bytes, &q));
  tmp.ptrs.push_back(q);
  S3GRL_HIP_TRY(hipMemsetAsync(q, 0, (size_t)*grid * (size_t)l.slice_bytes, ctx->stream));
  *slices = static_cast<uint32_t*>(q);
  return S3GRL_OK;
}

s3grl_status cand_error(int64_t flag) {
  if (flag == 1) {
    set_last_error("candidates: a source outside [0, N)");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (flag == 2) {
    set_last_error("candidates: seg_ptr is not what s3grl_candidates_count wrote for these arguments");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  return S3GRL_OK;
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

extern "C" {

s3grl_status s3grl_candidates_layout(int64_t num_nodes, int32_t hops, int64_t* out) {
  if (!out || num_nodes < 1 || num_nodes >= ((int64_t)1 << 31) || hops < 2 || hops > kCandMaxHops)
    return S3GRL_ERR_INVALID_ARGUMENT;
  const CandLayout l = cand_layout(num_nodes);
  out[0] = l.hbm ? 1 : 0;
  out[1] = l.words;
  out[2] = l.threads;
  out[3] = l.lds_bytes;
  out[4] = l.slice_bytes;
  out[5] = l.hbm ? kCandResident : 0;
  out[6] = kCandLdsNodes;
  out[7] = 0;
  return S3GRL_OK;
}

s3grl_status s3grl_candidates_count(s3grl_context* ctx, const s3grl_graph* g, const int32_t* sources,
                                    int64_t num_sources, int32_t hops, const uint64_t* exclude_keys,
                                    int64_t num_exclude, int64_t* seg_ptr, int64_t* total) {
  S3GRL_TRY(check_candidates_args(ctx, g, sources, num_sources, hops, exclude_keys, num_exclude, seg_ptr));
  if (!total) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t S = num_sources;
  *total = 0;
  if (S == 0) {
    S3GRL_HIP_TRY(hipMemsetAsync(seg_ptr, 0, 8, ctx->stream));
    return S3GRL_OK;
  }
  Transient tmp{ctx, {}};
  void *cnt = nullptr, *ws = nullptr;
  S3GRL_TRY(ctx->arena.alloc((size_t)S * 4, &cnt));
  tmp.ptrs.push_back(cnt);
  S3GRL_TRY(ctx->arena.alloc((size_t)scan_workspace_elems(S) * 8, &ws));
  tmp.ptrs.push_back(ws);
  uint32_t* slices = nullptr;
  int grid = 0;
  S3GRL_TRY(cand_workspace(ctx, g, S, tmp, &slices, &grid));
  S3GRL_HIP_TRY(hipMemsetAsync(ctx->d_scalars, 0, 8, ctx->stream));
  S3GRL_TRY(launch_candidates<false>(ctx, g, sources, S, hops, exclude_keys, num_exclude, slices, grid,
                                     static_cast<int32_t*>(cnt), nullptr, nullptr,
                                     reinterpret_cast<int32_t*>(ctx->d_scalars)));
  S3GRL_TRY(launch_scan_i32_to_i64(ctx, static_cast<int32_t*>(cnt), S, seg_ptr, static_cast<int64_t*>(ws)));
  S3GRL_HIP_TRY(hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
  S3GRL_HIP_TRY(hipMemcpyAsync(ctx->h_scalars + 1, seg_ptr + S, 8, hipMemcpyDeviceToHost, ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));   // the one wait: the total, and the workspace is released
  S3GRL_TRY(cand_error(ctx->h_scalars[0] & 0xffffffff));
  *total = ctx->h_scalars[1];
  return S3GRL_OK;
}

s3grl_status s3grl_candidates_fill(s3grl_context* ctx, const s3grl_graph* g, const int32_t* sources,
                                   int64_t num_sources, int32_t hops, const uint64_t* exclude_keys,
                                   int64_t num_exclude, const int64_t* seg_ptr, int32_t* cand) {
  S3GRL_TRY(check_candidates_args(ctx, g, sources, num_sources, hops, exclude_keys, num_exclude, seg_ptr));
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t S = num_sources;
  if (S == 0) return S3GRL_OK;
  Transient tmp{ctx, {}};
  uint32_t* slices = nullptr;
  int grid = 0;
  S3GRL_TRY(cand_workspace(ctx, g, S, tmp, &slices, &grid));
  S3GRL_HIP_TRY(hipMemsetAsync(ctx->d_scalars, 0, 8, ctx->stream));
  S3GRL_TRY(launch_candidates<true>(ctx, g, sources, S, hops, exclude_keys, num_exclude, slices, grid, nullptr,
                                    seg_ptr, cand, reinterpret_cast<int32_t*>(ctx->d_scalars)));
  S3GRL_HIP_TRY(hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));   // a segment that does not match is reported, not written
  return cand_error(ctx->h_scalars[0] & 0xffffffff);
}

s3grl_status s3grl_segment_topk(s3grl_context* ctx, const float* scores, const int64_t* seg_ptr, const int32_t* cand,
                                int64_t num_pairs, int64_t num_segments, int32_t k, int32_t* top_nodes,
                                float* top_scores, int32_t* top_count) {
  if (k > kTopMaxK) {
    set_last_error("segment_topk: k <= 1024 (the survivors are sorted in LDS)");
    return S3GRL_ERR_NOT_IMPLEMENTED;
  }
  if (k < 1) {
    set_last_error("segment_topk: k >= 1");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (!ctx || num_pairs < 0 || num_segments < 0 || num_segments >= ((int64_t)1 << 31) || !seg_ptr ||
      (num_pairs > 0 && (!scores || !cand)) || (num_segments > 0 && (!top_nodes || !top_scores || !top_count)))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_segments == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  S3GRL_HIP_TRY(hipMemsetAsync(ctx->d_scalars, 0, 8, ctx->stream));
  hipLaunchKernelGGL(segment_topk_kernel, dim3((unsigned)num_segments), dim3(kTopT), 0, ctx->stream, scores, seg_ptr,
                     cand, num_pairs, (int)k, top_nodes, top_scores, top_count,
                     reinterpret_cast<int32_t*>(ctx->d_scalars));
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_HIP_TRY(hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (ctx->h_scalars[0] & 0xffffffff) {
    set_last_error("segment_topk: seg_ptr must rise from >= 0 to <= num_pairs, segments shorter than 2^31; the rows "
                   "of the bad segments were written as empty");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  return S3GRL_OK;
}

}  // extern "C"
