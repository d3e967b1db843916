// Sizing pass from cached node balls (plain multi-hop plans on graphs whose balls fit: PubMed, Cora, USAir).
//
// The subgraph of a link is the union of the BFS balls of its two endpoints on the UNMASKED graph
// (reference utils.py:53-74: the target link is removed afterwards, utils.py:76-80), level d of the link =
// (ball_d(src) ∪ ball_d(dst)) minus (ball_{d-1}(src) ∪ ball_{d-1}(dst)).  A node is an endpoint of ~16
// links of a split, and count_kernel (s3grl_structure.hip) walks its ball again for every one of them —
// level-synchronous, with atomics into LDS bitmaps.  Here the balls ball_1 .. ball_h of EVERY node are
// built once per graph as N-bit bitmaps (level d = OR of level d-1 over the node's row: nnz * N/32 word
// operations per level; PubMed, 3 hops: 146 MB, 0.3 ms) and the sizing pass of a plan becomes word-parallel
// bitmap arithmetic: two rows of N/32 words per level, read once with coalesced wave-loads, a popcount scan,
// and the level's nodes placed in ascending id order in an LDS window that goes to HBM in whole wave-stores
// (count_balls_kernel) — the same n, level ends, node lists (the hand-over to link_kernel),
// |P| and PoS Plus row counts as count_kernel's, bit for bit.  Sampled, random-walk, directed and
// one-hop-on-big-graph plans, and graphs whose balls would take more than 1 GiB, keep their own sizing pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "s3grl_device.hpp"

namespace s3grl {
namespace {

constexpr int kBallWordsPerThread = 10;  // bitmap words a thread of count_balls_kernel keeps in registers, at most
                                         // (N <= 327 680; 12 and 16 words spilled, and the 1 GiB cap ends at N = 92 681)
constexpr int kBallWordsTarget = 5;      // ... and what the launcher aims for (PubMed, 617 words, structure phase of
                                         // the headline: 128 threads x 5 words 0.63 ms; 64 x 10: 0.61, at 96 VGPRs;
                                         // 256 x 3: 0.81; the contiguous runs this kernel had before: 0.99)

constexpr int kBallWindow = 1024;        // nodes of a level that count_balls_kernel places in LDS per copy to the stash

// level 1: x and its stored neighbours (one thread per node, then one per arc)
__global__ void ball_self_kernel(int64_t N, int W, uint32_t* __restrict__ bits) {
  const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x < N) atomicOr(&bits[x * W + (x >> 5)], 1u << (x & 31));
}

__global__ void ball_arcs_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t N,
                                 int W, uint32_t* __restrict__ bits) {
  // eight lanes per node stride its row
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t x = gid >> 3;
  if (x >= N) return;
  const int e1 = indptr[x + 1];
  for (int e = indptr[x] + (int)(gid & 7); e < e1; e += 8) {
    const int u = indices[e];
    atomicOr(&bits[x * W + (u >> 5)], 1u << (u & 31));
  }
}

// level d from level d-1: ball_d(x) = ball_{d-1}(x) ∪ ⋃_{u ∈ N(x)} ball_{d-1}(u); one workgroup per node
__global__ __launch_bounds__(256) void ball_next_kernel(const int32_t* __restrict__ indptr,
                                                        const int32_t* __restrict__ indices, int W,
                                                        const uint32_t* __restrict__ prev, uint32_t* __restrict__ cur) {
  const int64_t x = blockIdx.x;
  const int e0 = indptr[x], e1 = indptr[x + 1];
  for (int w = threadIdx.x; w < W; w += 256) {
    uint32_t acc = prev[x * W + w];
    for (int e = e0; e < e1; ++e) acc |= prev[(int64_t)indices[e] * W + w];
    cur[x * W + w] = acc;
  }
}

// inclusive scan over the wavefront of two 16-bit counts packed into one int (each total <= 64 * 32), on
// the DPP path: shifts within the rows of 16 lanes, then lane 15 of a row into the next row, then lane 31
// into the upper half
__device__ __forceinline__ int wave_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
  return v;
}

// The sizing pass of one link from the cached balls; outputs exactly those of count_kernel.  The bitmap
// words are dealt round-robin: thread t owns words t, t + T, .. (chunk c = words cT .. cT + T - 1), so a
// chunk is one coalesced wave-load per ball row and every thread draws from CW different degree regions
// (ids are in descending degree order and a subgraph is degree-biased: with contiguous runs the threads
// of the low ids held most of a level's bits and the others waited for them).  A level's nodes still go
// out in ascending id order, i.e. in word order chunk by chunk: a wave scan of the popcounts per chunk,
// the (chunk, wave) totals in a small LDS table, one barrier, and every thread adds the table's prefix;
// the level total is the table's sum.  The nodes are placed in an LDS window at their position within
// the level and the workgroup copies the window to the stash with lane i on entry i — full, contiguous
// wave-stores, cut at `slot`; what a level has beyond the window is stored node by node in a second walk.
template <int T, int CW>
__global__ __launch_bounds__(T) void count_balls_kernel(
    const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices, int N, int W,
    const uint32_t* __restrict__ balls, int64_t level_stride, const int64_t* __restrict__ links, int hops, int plus,
    int K, const int32_t* __restrict__ partner, const int32_t* __restrict__ mirror_of, int32_t* __restrict__ n_nodes,
    int32_t* __restrict__ p_nodes, int32_t* __restrict__ n_rows, int32_t* __restrict__ n_jobs,
    int32_t* __restrict__ lvl_max, int32_t* __restrict__ err_flag, unsigned long long* __restrict__ tot_nodes_alg,
    int32_t* __restrict__ stash, int slot, int32_t* __restrict__ lvl_stash, const int32_t* __restrict__ perm) {
  constexpr int NW = T / 64;
  __shared__ int tab[2][CW * NW];          // (chunk, wave) totals of a level; levels alternate between the two
  __shared__ int32_t win[kBallWindow + 1]; // a level's nodes at their positions
  const int tid = threadIdx.x;
  const int l = perm ? perm[blockIdx.x] : (int)blockIdx.x;
  const int64_t s64 = links[2 * (int64_t)l], d64 = links[2 * (int64_t)l + 1];
  if (s64 < 0 || s64 >= N || d64 < 0 || d64 >= N || s64 == d64) {
    if (tid == 0) {
      atomicMax(err_flag, s64 == d64 ? 2 : 1);
      n_nodes[l] = 0;
      p_nodes[l] = 0;
      n_rows[l] = 0;
      n_jobs[l] = 0;
      lvl_max[l] = 0;
    }
    return;
  }
  if (partner && partner[l] >= 0) {  // reversed duplicate: the primary link does the work
    if (tid == 0) {
      n_nodes[l] = 0;
      p_nodes[l] = 0;
      n_rows[l] = 0;  // copied from the primary by mirror_rows_kernel
      n_jobs[l] = 0;
      lvl_max[l] = 0;
    }
    return;
  }
  const int src = (int)s64, dst = (int)d64;
  int32_t* stash_l = stash ? stash + (int64_t)l * slot : nullptr;
  int32_t* lvl_l = lvl_stash ? lvl_stash + (int64_t)l * kMaxLevels : nullptr;
  if (lvl_l && tid == 0) lvl_l[0] = 2;
  const int lane = lane_id(), wid = wave_id();
  uint32_t prev[CW];   // the link's nodes so far, as bits: word tid + c T (W <= CW T, the launcher's choice);
                       // all ones for a word beyond W, whose loads (of word W - 1) then never add a node
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const int w = tid + c * T;
    prev[c] = w >= W ? ~0u
                     : (w == (src >> 5) ? 1u << (src & 31) : 0u) | (w == (dst >> 5) ? 1u << (dst & 31) : 0u);
  }
  int n = 2, cum_a = 2, cum_b = 2, biggest = 2, nlev_seen = 1;
  for (int d = 1; d <= hops; ++d) {
    const uint32_t* __restrict__ bs = balls + (int64_t)(d - 1) * level_stride + (int64_t)src * W;
    const uint32_t* __restrict__ bd = balls + (int64_t)(d - 1) * level_stride + (int64_t)dst * W;
    uint32_t fresh[CW];
    int t = tid;                    // the thread's first word, opaque to the compiler: the word offsets and
    asm volatile("" : "+v"(t));     // node ids derived from it are worked out per level, not kept in registers
#pragma unroll
    for (int c = 0; c < CW; ++c) {
      const unsigned w = (unsigned)min(t + c * T, W - 1);   // (unsigned: one 32-bit offset serves both rows)
      const uint32_t cur = bs[w] | bd[w];
      fresh[c] = cur & ~prev[c];
      prev[c] |= cur;
    }
    int pos[CW];   // the position in the level of the word's first node: within the wave, then within the level
    int* tb = tab[d & 1];
#pragma unroll
    for (int c = 0; c < CW; c += 2) {
      const int mine = __popc(fresh[c]) | (c + 1 < CW ? __popc(fresh[c + 1]) << 16 : 0);
      const int v = wave_incl_scan(mine);
      if (lane == 63) {
        tb[c * NW + wid] = v & 0xffff;
        if (c + 1 < CW) tb[(c + 1) * NW + wid] = v >> 16;
      }
      pos[c] = (v - mine) & 0xffff;
      if (c + 1 < CW) pos[c + 1] = (v - mine) >> 16;
    }
    __syncthreads();
    int added = 0;
#pragma unroll
    for (int c = 0; c < CW; ++c) {   // word order: chunk by chunk, wave by wave
      int before = 0, chunk = 0;
#pragma unroll 4
      for (int j = 0; j < NW; ++j) {
        const int s = tb[c * NW + j];
        before += j < wid ? s : 0;
        chunk += s;
      }
      pos[c] += added + before;
      added += chunk;
    }
    if (added == 0) break;   // (uniform: a block-wide total)
    const int room = min(added, slot - (n - 2));   // what of the level the slot still takes (uniform)
    if (stash_l && room > 0) {                     // the level in ascending id order, hop 1 onwards
      int32_t* out = stash_l + (n - 2);
#pragma unroll
      for (int c = 0; c < CW; ++c) {   // (the window's last entry takes what lies beyond it)
        uint32_t w = fresh[c];
        int p = pos[c];
        while (w) {
          const int b = __ffs(w) - 1;
          w &= w - 1;
          win[min(p, kBallWindow)] = (t + c * T) * 32 + b;
          ++p;
        }
      }
      __syncthreads();
      const int m = min(room, kBallWindow);
#pragma unroll 2
      for (int i = tid; i < m; i += T) out[i] = win[i];
      if (room > kBallWindow) {   // a level beyond the window: the rest node by node
#pragma unroll
        for (int c = 0; c < CW; ++c) {
          uint32_t w = fresh[c];
          int p = pos[c];
          if (p + __popc(w) <= kBallWindow) continue;
          while (w) {
            const int b = __ffs(w) - 1;
            w &= w - 1;
            if (p >= kBallWindow && p < room) out[p] = (t + c * T) * 32 + b;
            ++p;
          }
        }
      }
    }
    if (lvl_l && tid == 0) lvl_l[d] = n + added;
    n += added;
    nlev_seen = d + 1;
    biggest = max(biggest, added);
    if (d <= K - 1) cum_a = n;
    if (d <= K) cum_b = n;
  }
  int R = 2;
  if (plus && (tid >> 6) == 0) {
    const uint32_t* __restrict__ bs = balls + (int64_t)(hops - 1) * level_stride + (int64_t)src * W;
    const uint32_t* __restrict__ bd = balls + (int64_t)(hops - 1) * level_stride + (int64_t)dst * W;
    R = 2 + common_neighbours(
                indptr, indices, [&](int x) { return (((bs[x >> 5] | bd[x >> 5]) >> (x & 31)) & 1u) != 0u || x == src || x == dst; },
                src, dst, nullptr);
  }
  if (tid == 0) {
    if (lvl_l) lvl_l[kMaxLevels - 1] = nlev_seen;   // levels 0 .. nlev_seen-1 are complete
    n_nodes[l] = n;
    p_nodes[l] = R > 2 ? cum_b : cum_a;
    n_rows[l] = R;
    n_jobs[l] = (R + 1) / 2;
    lvl_max[l] = biggest;
    const unsigned long long mult = (mirror_of && mirror_of[l] >= 0) ? 2ull : 1ull;
    atomicAdd(stat_slot(tot_nodes_alg), mult * (unsigned long long)n);
  }
}

}  // namespace

void release_ball_cache(s3grl_graph* g) {
  g->ctx->arena.release(g->balls.bits);
  g->balls = BallCache{};
}

// balls 1 .. hops of every node of the degree-ordered graph, built level by level on first use
s3grl_status ensure_ball_cache(s3grl_context* ctx, s3grl_graph* g, int hops, bool* usable) {
  *usable = false;
  if (!g->r_indptr || g->directed || hops < 1 || getenv("S3GRL_NO_BALL_CACHE")) return S3GRL_OK;
  const int64_t N = g->num_nodes;
  const int W = (int)((N + 31) / 32);
  if ((W + 1023) / 1024 > kBallWordsPerThread) return S3GRL_OK;
  const int64_t bytes = (int64_t)hops * N * W * 4;
  int64_t cap = (int64_t)1 << 30;
  if (const char* e = getenv("S3GRL_BALL_CACHE_BYTES")) cap = atoll(e);   // test hook
  if (bytes > cap) return S3GRL_OK;
  BallCache& bc = g->balls;
  if (bc.hops < hops) {
    void* q = nullptr;
    S3GRL_TRY(ctx->arena.alloc((size_t)bytes, &q));
    uint32_t* bits = static_cast<uint32_t*>(q);
    const int64_t stride = N * W;
    int have = 0;
    if (bc.bits) {   // keep the levels already built
      S3GRL_HIP_TRY(hipMemcpyAsync(bits, bc.bits, (size_t)bc.hops * stride * 4, hipMemcpyDeviceToDevice, ctx->stream));
      have = bc.hops;
    }
    if (have == 0) {
      S3GRL_HIP_TRY(hipMemsetAsync(bits, 0, (size_t)stride * 4, ctx->stream));
      hipLaunchKernelGGL(ball_self_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, N, W, bits);
      hipLaunchKernelGGL(ball_arcs_kernel, dim3((unsigned)((N * 8 + 255) / 256)), dim3(256), 0, ctx->stream,
                         g->r_indptr, g->r_indices, N, W, bits);
      have = 1;
    }
    for (int d = have; d < hops; ++d)
      hipLaunchKernelGGL(ball_next_kernel, dim3((unsigned)N), dim3(256), 0, ctx->stream, g->r_indptr, g->r_indices, W,
                         bits + (int64_t)(d - 1) * stride, bits + (int64_t)d * stride);
    S3GRL_HIP_TRY(hipGetLastError());
    S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));   // (the old block is released below)
    if (bc.bits) ctx->arena.release(bc.bits);
    bc.bits = bits;
    bc.hops = hops;
    bc.level_stride = stride;
  }
  *usable = true;
  return S3GRL_OK;
}

s3grl_status launch_count_balls(s3grl_context* ctx, const s3grl_graph* g, const int64_t* links, int64_t L, int hops,
                                int plus, int K, const int32_t* partner, const int32_t* mirror_of, int32_t* n_nodes,
                                int32_t* p_nodes, int32_t* n_rows, int32_t* n_jobs, int32_t* lvl_max,
                                int32_t* err_flag, int64_t* tot_nodes_alg, int32_t* stash, int slot,
                                int32_t* lvl_stash, const int32_t* perm) {
  if (L == 0) return S3GRL_OK;
  const int N = (int)g->num_nodes;
  const int W = (N + 31) / 32;
  const BallCache& bc = g->balls;
  auto launch = [&](auto kern, int T) {
    hipLaunchKernelGGL(kern, dim3((unsigned)L), dim3(T), 0, ctx->stream, g->indptr, g->indices, N, W, bc.bits,
                       bc.level_stride, links, hops, plus, K, partner, mirror_of, n_nodes, p_nodes, n_rows, n_jobs,
                       lvl_max, err_flag, reinterpret_cast<unsigned long long*>(tot_nodes_alg), stash, slot, lvl_stash,
                       perm);
  };
  // threads per link: the smallest workgroup that gives a thread at most `target` words (a thread keeps
  // its words in registers and writes their nodes out one by one)
  int T = 64;
  while (T < 1024 && W > T * kBallWordsTarget) T *= 2;
  const int C = (W + T - 1) / T;   // <= kBallWordsPerThread (ensure_ball_cache checked W <= 1024 * that)
#define S3GRL_BALLS_CW(TT, CW) launch(count_balls_kernel<TT, CW>, TT)
  // (below 1024 threads the loop above leaves at most kBallWordsTarget words per thread)
#define S3GRL_BALLS_T(TT)                                                                                      \
  (C <= 1 ? S3GRL_BALLS_CW(TT, 1) : C <= 2 ? S3GRL_BALLS_CW(TT, 2) : C <= 3 ? S3GRL_BALLS_CW(TT, 3)             \
   : C <= 4 ? S3GRL_BALLS_CW(TT, 4) : S3GRL_BALLS_CW(TT, 5))
  static_assert(kBallWordsTarget <= 5 && kBallWordsPerThread <= 10, "count_balls_kernel: instantiations below");
  switch (T) {
    case 64: S3GRL_BALLS_T(64); break;
    case 128: S3GRL_BALLS_T(128); break;
    case 256: S3GRL_BALLS_T(256); break;
    case 512: S3GRL_BALLS_T(512); break;
    default:
      if (C <= 5) S3GRL_BALLS_T(1024);
      else if (C <= 6) S3GRL_BALLS_CW(1024, 6);
      else if (C <= 8) S3GRL_BALLS_CW(1024, 8);
      else S3GRL_BALLS_CW(1024, 10);
      break;
  }
#undef S3GRL_BALLS_T
#undef S3GRL_BALLS_CW
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

}  // namespace s3grl

S3GRL_DEFINE_TOUCH(balls)
