// Neural Common Neighbour (NCN, Wang et al., ICLR 2024): the operator C[l] = sum over w in N(u_l) ∩ N(v_l) of Z[w],
// as a list of every link's common neighbours and a rectangular segment sum over it.  DESIGN.md section 26 is the
// specification; tests/ncn_reference.py restates it in numpy, and every output here equals that restatement to the
// bit.
//
//   cn_lists_kernel<FILL>   a wavefront per link, four links per workgroup.  The lanes walk the shorter of the two
//                           sorted rows 64 keys at a time (pick_walk of s3grl_rows.hpp, as pairs_kernel of
//                           s3grl_heuristics.hip) and each searches the other row for its key; the survivors' positions
//                           are a ballot and a popcount below the lane, on a running base.  FILL = false writes the
//                           count, FILL = true the keys at cn_ptr[l] + rank: ascending whichever row was walked, since
//                           both are.  No atomics.  A row of tens of thousands of keys is a serial tail of one
//                           wavefront.
//   segment_sum_kernel<VEC> out[r, :] = sum of h[idx[j], :] over a row's entries, a wavefront per row, lanes across
//                           columns (one float4 per lane, or four columns 64 apart where the rows are not 16-byte
//                           words), column blocks of 256 looped.  The ORDER of the fp32 additions is the specification:
//                           a row is cut into chunks of kChunk = 64 entries; a chunk's partial is the sequential sum of
//                           its entries from its first one; the row is the sequential sum of the partials from the
//                           first one; an empty row is +0.0.  A row of more than kChunk entries has its chunks dealt to
//                           the four wavefronts of its workgroup, four chunks a round, and thread t adds the round's
//                           partials of column t from LDS in chunk order.  kBatch rows are in flight before they are
//                           added.  Only additions occur (nothing to contract) and there are no atomics: any launch
//                           gives the same bits.
//
// NCNC's completion step (tests/ncnc_reference.py):
//   cn_split_kernel<FILL>   a wavefront per link, four links per workgroup, no barrier, no atomics.  The list of (u, v)
//                           is three sections, each ascending: S0 = N(u) ∩ N(v), S1 = N(u) \ N(v), S2 = N(v) \ N(u).
//                           The lanes walk u's row 64 keys a trip and search v's row: a hit goes to S0, a miss to S1
//                           (two ballots, two running bases); then they walk v's row and search u's: a miss goes to
//                           S2.  pick_walk's shorter-row choice cannot serve: both rows are walked in full.
//   segment_sum_kernel<VEC, true>   the same kernel with a weight per entry: every term is the fp32 product
//                           w[j]·h[idx[j], c] rounded once (mul_rn, never contracted into the addition) and the terms
//                           are added in the order above, so unit weights give the bits of the unweighted kernel.
//   segment_dot_kernel<VEC> out_w[j] = sum over c of g[r(j), c]·h[idx[j], c], a wavefront per list.  Lane t is slot t
//                           and owns the columns c with (c mod 256) / 4 == t, whether they are loaded as one 16-byte
//                           word or as four scalars; it adds its rounded products in ascending c from its first
//                           product (+0.0 without a column), and the 64 slots are combined by the halving tree
//                           s = 32, 16, .., 1 (slot t < s becomes slot t + slot t+s; run as a butterfly, which gives
//                           every lane slot 0's bits since fp32 addition commutes).  The list's g row of the first
//                           256 columns stays in registers, further column blocks are read again per entry.
#include "s3grl_internal.hpp"
#include "s3grl_rows.hpp"

namespace s3grl {
namespace {

constexpr int kNcnBlock = 256, kNcnWaves = 4;
constexpr int kChunk = 64;           // entries per partial sum: part of the specification
constexpr int kBatch = 4;            // neighbour rows a wavefront loads before it adds them
constexpr int kColBlock = 256;       // columns a wavefront holds at once: four per lane

__device__ __forceinline__ int wave_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

// links int32 [2, L].  FILL = false: cnt[l] = |list of l|.  FILL = true: the list at cn_idx[cn_ptr[l] ..), never
// outside [0, total).
template <bool FILL>
__global__ __launch_bounds__(kNcnBlock) void cn_lists_kernel(int64_t L, const int32_t* __restrict__ links,
                                                             const int64_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ idx, int exclude,
                                                             int64_t* __restrict__ cnt,
                                                             const int64_t* __restrict__ cn_ptr, int64_t total,
                                                             int32_t* __restrict__ cn_idx) {
  const int wave = wave_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t l = (int64_t)blockIdx.x * kNcnWaves + wave;
  if (l >= L) return;   // wave-uniform; the kernel has no barrier
  const int u = wave_uniform(links[l]), v = wave_uniform(links[L + l]);
  const int u0 = wave_uniform((int)ptr[u]), u1 = wave_uniform((int)ptr[u + 1]);
  const int v0 = wave_uniform((int)ptr[v]), v1 = wave_uniform((int)ptr[v + 1]);
  const RowWalk<int> rows = pick_walk(u0, u1, v0, v1, u, v);
  int64_t base = 0;
  if (FILL) base = cn_ptr[l];
  int64_t found = 0;
  for (int e0 = rows.w0; e0 < rows.w1; e0 += 64) {
    const bool have = e0 + lane < rows.w1;
    const int32_t key = have ? idx[e0 + lane] : 0;
    const bool keep = have && !(exclude && (key == u || key == v)) && find_sorted(idx, rows.o0, rows.o1, key) >= 0;
    const uint64_t kept = __ballot(keep);
    if (FILL && keep) {
      const int64_t at = base + found + __popcll(kept & ((uint64_t(1) << lane) - 1));
      if (at >= 0 && at < total) cn_idx[at] = key;
    }
    found += __popcll(kept);
  }
  if (!FILL && lane == 0) cnt[l] = found;
}

// links int32 [2, L].  FILL = false: cnt[s·L + l] = |section s of l|.  FILL = true: the three sections one after the
// other at sp_idx[sp_ptr[l] ..) with their section in sp_side, never outside [0, total); cnt is read for the bases.
template <bool FILL>
__global__ __launch_bounds__(kNcnBlock) void cn_split_kernel(int64_t L, const int32_t* __restrict__ links,
                                                             const int64_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ idx, int exclude,
                                                             int64_t* __restrict__ cnt_out,
                                                             const int64_t* __restrict__ cnt_in,
                                                             const int64_t* __restrict__ sp_ptr, int64_t total,
                                                             int32_t* __restrict__ sp_idx,
                                                             int32_t* __restrict__ sp_side) {
  const int wave = wave_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t l = (int64_t)blockIdx.x * kNcnWaves + wave;
  if (l >= L) return;   // wave-uniform; the kernel has no barrier
  const int u = wave_uniform(links[l]), v = wave_uniform(links[L + l]);
  const int u0 = wave_uniform((int)ptr[u]), u1 = wave_uniform((int)ptr[u + 1]);
  const int v0 = wave_uniform((int)ptr[v]), v1 = wave_uniform((int)ptr[v + 1]);
  int64_t base0 = 0, base1 = 0, base2 = 0;   // where the next key of each section goes
  if (FILL) {
    base0 = sp_ptr[l];
    base1 = base0 + cnt_in[l];
    base2 = base1 + cnt_in[L + l];
  }
  const uint64_t below = (uint64_t(1) << lane) - 1;
  int64_t n0 = 0, n1 = 0, n2 = 0;
  for (int e0 = u0; e0 < u1; e0 += 64) {   // u's row: a hit in v's row is common, a miss is u's alone
    const bool have = e0 + lane < u1;
    const int32_t key = have ? idx[e0 + lane] : 0;
    const bool live = have && !(exclude && (key == u || key == v));
    const bool hit = live && find_sorted(idx, v0, v1, key) >= 0;
    const uint64_t hits = __ballot(hit), misses = __ballot(live && !hit);
    if (FILL && live) {
      const int64_t at = hit ? base0 + n0 + __popcll(hits & below) : base1 + n1 + __popcll(misses & below);
      if (at >= 0 && at < total) {
        sp_idx[at] = key;
        sp_side[at] = hit ? 0 : 1;
      }
    }
    n0 += __popcll(hits);
    n1 += __popcll(misses);
  }
  for (int e0 = v0; e0 < v1; e0 += 64) {   // v's row: a miss in u's row is v's alone
    const bool have = e0 + lane < v1;
    const int32_t key = have ? idx[e0 + lane] : 0;
    const bool miss = have && !(exclude && (key == u || key == v)) && find_sorted(idx, u0, u1, key) < 0;
    const uint64_t misses = __ballot(miss);
    if (FILL && miss) {
      const int64_t at = base2 + n2 + __popcll(misses & below);
      if (at >= 0 && at < total) {
        sp_idx[at] = key;
        sp_side[at] = 2;
      }
    }
    n2 += __popcll(misses);
  }
  if (!FILL && lane == 0) {
    cnt_out[l] = n0;
    cnt_out[L + l] = n1;
    cnt_out[2 * L + l] = n2;
  }
}

struct Cols {
  float c[4];
};

// The four columns of row w that a lane holds in the block starting at col0.  VEC: col0 + 4 lane .. + 3 as one
// 16-byte word; else col0 + lane + 64 k.  Columns past H read as 0 and are never stored.
template <bool VEC>
__device__ __forceinline__ Cols load_cols(const float* __restrict__ h, int64_t w, int64_t H, int64_t col0, int lane) {
  Cols r;
  if (VEC) {
    const int64_t col = col0 + 4 * lane;
    const float4 t = col < H ? *reinterpret_cast<const float4*>(h + w * H + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    r.c[0] = t.x, r.c[1] = t.y, r.c[2] = t.z, r.c[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t col = col0 + lane + 64 * k;
      r.c[k] = col < H ? h[w * H + col] : 0.f;
    }
  }
  return r;
}

__device__ __forceinline__ void add_cols(Cols& a, const Cols& b) {
#pragma unroll
  for (int k = 0; k < 4; ++k) a.c[k] = a.c[k] + b.c[k];
}

// the fp32 product rounded once: what __fmul_rn promises, with contraction into a following addition switched off
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

__device__ __forceinline__ void scale_cols(Cols& a, float w) {
#pragma unroll
  for (int k = 0; k < 4; ++k) a.c[k] = mul_rn(w, a.c[k]);
}

__device__ __forceinline__ float readlane_f(float x, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

// where a lane's column k sits inside its block of kColBlock
template <bool VEC>
__device__ __forceinline__ int col_offset(int lane, int k) { return VEC ? 4 * lane + k : lane + 64 * k; }

// The partial of one chunk, entries [begin, end) with 1 <= end - begin <= kChunk: the terms added one after the other
// in ascending entry, starting from the first term itself.  A term is h's row, or with WEIGHTED w[j] times it, each
// product rounded once.  The ids (and weights) are loaded once and handed round by readlane.
template <bool VEC, bool WEIGHTED>
__device__ __forceinline__ Cols term_cols(int mine, float mine_w, int j, const float* __restrict__ h, int64_t H,
                                          int64_t col0, int lane) {
  Cols t = load_cols<VEC>(h, __builtin_amdgcn_readlane(mine, j), H, col0, lane);
  if (WEIGHTED) scale_cols(t, readlane_f(mine_w, j));
  return t;
}

template <bool VEC, bool WEIGHTED>
__device__ __forceinline__ Cols chunk_sum(int lane, const int32_t* __restrict__ idx, const float* __restrict__ w,
                                          int64_t begin, int64_t end, const float* __restrict__ h, int64_t H,
                                          int64_t col0) {
  const int count = (int)(end - begin);
  const int mine = lane < count ? idx[begin + lane] : 0;
  float mine_w = 0.f;
  if (WEIGHTED) mine_w = lane < count ? w[begin + lane] : 0.f;
  Cols acc = term_cols<VEC, WEIGHTED>(mine, mine_w, 0, h, H, col0, lane);
  int j = 1;
  for (; j + kBatch <= count; j += kBatch) {   // kBatch rows in flight: the loads do not wait for each other
    Cols t[kBatch];
#pragma unroll
    for (int q = 0; q < kBatch; ++q) t[q] = term_cols<VEC, WEIGHTED>(mine, mine_w, j + q, h, H, col0, lane);
#pragma unroll
    for (int q = 0; q < kBatch; ++q) add_cols(acc, t[q]);
  }
  for (; j < count; ++j) add_cols(acc, term_cols<VEC, WEIGHTED>(mine, mine_w, j, h, H, col0, lane));
  return acc;
}

template <bool VEC>
__device__ __forceinline__ void store_cols(float* __restrict__ out, int64_t r, int64_t H, int64_t col0, int lane,
                                           const Cols& a) {
  if (VEC) {
    const int64_t col = col0 + 4 * lane;
    if (col < H) *reinterpret_cast<float4*>(out + r * H + col) = make_float4(a.c[0], a.c[1], a.c[2], a.c[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t col = col0 + lane + 64 * k;
      if (col < H) out[r * H + col] = a.c[k];
    }
  }
}

// h fp32 [M, H], ptr int64 [R + 1], idx int32 [ptr[R]] with every entry in [0, M) (the caller's promise), out fp32
// [R, H].  A workgroup takes four consecutive rows.  Rows of at most kChunk entries: one per wavefront.  Longer rows:
// one after the other, their chunks dealt to the four wavefronts.  WEIGHTED: w fp32 [ptr[R]], a weight per entry.
template <bool VEC, bool WEIGHTED>
__global__ __launch_bounds__(kNcnBlock) void segment_sum_kernel(int64_t R, int64_t H, const int64_t* __restrict__ ptr,
                                                                const int32_t* __restrict__ idx,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ h,
                                                                float* __restrict__ out) {
  __shared__ float part[kNcnWaves][kColBlock];
  const int wave = wave_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t first = (int64_t)blockIdx.x * kNcnWaves;
  {
    const int64_t r = first + wave;
    if (r < R) {
      const int64_t begin = ptr[r], end = ptr[r + 1];
      if (end - begin <= kChunk) {
        for (int64_t col0 = 0; col0 < H; col0 += kColBlock) {
          Cols acc;
          if (end > begin) {
            acc = chunk_sum<VEC, WEIGHTED>(lane, idx, w, begin, end, h, H, col0);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc.c[k] = 0.f;
          }
          store_cols<VEC>(out, r, H, col0, lane, acc);
        }
      }
    }
  }
  for (int q = 0; q < kNcnWaves; ++q) {   // every wavefront of the workgroup takes the same path from here on
    const int64_t r = first + q;
    if (r >= R) break;
    const int64_t begin = ptr[r], end = ptr[r + 1];
    if (end - begin <= kChunk) continue;
    const int64_t chunks = (end - begin + kChunk - 1) / kChunk;
    for (int64_t col0 = 0; col0 < H; col0 += kColBlock) {
      float row = 0.f;                    // thread t: column col0 + t of the row, the partials added in chunk order
      for (int64_t c0 = 0; c0 < chunks; c0 += kNcnWaves) {
        const int64_t c = c0 + wave;
        if (c < chunks) {
          const int64_t b = begin + c * kChunk;
          const Cols acc = chunk_sum<VEC, WEIGHTED>(lane, idx, w, b, b + kChunk < end ? b + kChunk : end, h, H, col0);
#pragma unroll
          for (int k = 0; k < 4; ++k) part[wave][col_offset<VEC>(lane, k)] = acc.c[k];
        }
        __syncthreads();
        const int live = chunks - c0 < kNcnWaves ? (int)(chunks - c0) : kNcnWaves;
        for (int w = 0; w < live; ++w) row = (c0 == 0 && w == 0) ? part[0][threadIdx.x] : row + part[w][threadIdx.x];
        __syncthreads();
      }
      if (col0 + threadIdx.x < H) out[r * H + col0 + threadIdx.x] = row;
    }
  }
}

// The four columns col0 + 4 lane .. + 3 of row w: slot `lane` of the dot, as one 16-byte word (VEC) or four scalars.
// Columns past H read as 0 and are never used.
template <bool VEC>
__device__ __forceinline__ Cols load_slot(const float* __restrict__ h, int64_t w, int64_t H, int64_t col0, int lane) {
  if (VEC) return load_cols<true>(h, w, H, col0, lane);
  Cols r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t col = col0 + 4 * lane + k;
    r.c[k] = col < H ? h[w * H + col] : 0.f;
  }
  return r;
}

// acc plus the slot's products of one column block, in ascending column; the slot's first product (column 4 lane of
// block 0) starts the sum.  A column past H adds nothing, not +0.0: -0.0 stays -0.0.
__device__ __forceinline__ float slot_add(float acc, const Cols& a, const Cols& b, int64_t H, int64_t col0, int lane) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float p = mul_rn(a.c[k], b.c[k]);
    if (col0 + 4 * lane + k < H) acc = (col0 == 0 && k == 0) ? p : acc + p;
  }
  return acc;
}

// slot `lane` of <g[r, :], h[w, :]>; g0 is g's block 0 of the list, held by the caller
template <bool VEC>
__device__ __forceinline__ float slot_dot(const float* __restrict__ g, int64_t r, const Cols& g0,
                                          const float* __restrict__ h, int64_t w, int64_t H, int lane) {
  float acc = slot_add(0.f, g0, load_slot<VEC>(h, w, H, 0, lane), H, 0, lane);
  for (int64_t col0 = kColBlock; col0 < H; col0 += kColBlock)
    acc = slot_add(acc, load_slot<VEC>(g, r, H, col0, lane), load_slot<VEC>(h, w, H, col0, lane), H, col0, lane);
  return acc;
}

// the halving tree over the 64 slots, s = 32 .. 1: every lane ends with slot 0's value
__device__ __forceinline__ float slot_tree(float x) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x = x + __shfl_xor(x, s, 64);
  return x;
}

// g fp32 [R, H], h fp32 [M, H], ptr int64 [R + 1], idx int32 [ptr[R]] with every entry in [0, M) (the caller's
// promise), out_w fp32 [ptr[R]].  A wavefront per list, four lists per workgroup, no barrier; the entries are streamed
// 64 ids a trip, kBatch rows in flight, and lane e keeps entry e's result for one coalesced store a trip.
template <bool VEC>
__global__ __launch_bounds__(kNcnBlock) void segment_dot_kernel(int64_t R, int64_t H, const int64_t* __restrict__ ptr,
                                                                const int32_t* __restrict__ idx,
                                                                const float* __restrict__ g,
                                                                const float* __restrict__ h,
                                                                float* __restrict__ out_w) {
  const int wave = wave_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kNcnWaves + wave;
  if (r >= R) return;   // wave-uniform; the kernel has no barrier
  const int64_t begin = ptr[r], end = ptr[r + 1];
  if (end <= begin) return;
  const Cols g0 = load_slot<VEC>(g, r, H, 0, lane);
  for (int64_t b = begin; b < end; b += kChunk) {
    const int count = end - b < kChunk ? (int)(end - b) : kChunk;
    const int mine = lane < count ? idx[b + lane] : 0;
    float res = 0.f;
    int j = 0;
    for (; j + kBatch <= count; j += kBatch) {
      float t[kBatch];
#pragma unroll
      for (int q = 0; q < kBatch; ++q) t[q] = slot_dot<VEC>(g, r, g0, h, __builtin_amdgcn_readlane(mine, j + q), H, lane);
#pragma unroll
      for (int q = 0; q < kBatch; ++q) {
        const float d = slot_tree(t[q]);
        if (lane == j + q) res = d;
      }
    }
    for (; j < count; ++j) {
      const float d = slot_tree(slot_dot<VEC>(g, r, g0, h, __builtin_amdgcn_readlane(mine, j), H, lane));
      if (lane == j) res = d;
    }
    if (lane < count) out_w[b + lane] = res;
  }
}

bool bad_graph(int64_t num_nodes, int64_t num_entries, int64_t num_links) {
  return num_nodes < 1 || num_nodes >= (int64_t(1) << 31) || num_entries < 0 || num_entries >= (int64_t(1) << 31) ||
         num_links < 0 || num_links >= (int64_t(1) << 31);
}

// every endpoint is checked on the host before any GPU work
s3grl_status check_links(s3grl_context* ctx, const int32_t* links, int64_t num_links, int64_t num_nodes) {
  return check_ids(ctx, links, 2 * num_links, num_nodes, "ncn: a link endpoint outside [0, N)");
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

extern "C" {

s3grl_status s3grl_cn_count(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                            int64_t num_entries, const int32_t* links, int64_t num_links, int32_t exclude_endpoints,
                            int64_t* counts) {
  if (!ctx || !indptr || bad_graph(num_nodes, num_entries, num_links) || (num_entries > 0 && !indices) ||
      (num_links > 0 && (!links || !counts)) || (exclude_endpoints != 0 && exclude_endpoints != 1)) {
    set_last_error("ncn: need 1 <= N < 2^31, nnz < 2^31, fewer than 2^31 links and exclude_endpoints 0 or 1");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (num_links == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  S3GRL_TRY(check_links(ctx, links, num_links, num_nodes));
  hipLaunchKernelGGL(cn_lists_kernel<false>, dim3(grid_of(num_links, kNcnWaves)), dim3(kNcnBlock), 0, st, num_links,
                     links, indptr, indices, (int)exclude_endpoints, counts, (const int64_t*)nullptr, (int64_t)0,
                     (int32_t*)nullptr);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_cn_fill(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                           int64_t num_entries, const int32_t* links, int64_t num_links, int32_t exclude_endpoints,
                           const int64_t* cn_ptr, int64_t total, int32_t* cn_idx) {
  if (!ctx || !indptr || bad_graph(num_nodes, num_entries, num_links) || (num_entries > 0 && !indices) ||
      (num_links > 0 && (!links || !cn_ptr)) || total < 0 || (total > 0 && !cn_idx) ||
      (exclude_endpoints != 0 && exclude_endpoints != 1)) {
    set_last_error("ncn: need 1 <= N < 2^31, nnz < 2^31, fewer than 2^31 links, total >= 0 and exclude_endpoints 0 "
                   "or 1");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (num_links == 0 || total == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  S3GRL_TRY(check_links(ctx, links, num_links, num_nodes));
  hipLaunchKernelGGL(cn_lists_kernel<true>, dim3(grid_of(num_links, kNcnWaves)), dim3(kNcnBlock), 0, st, num_links,
                     links, indptr, indices, (int)exclude_endpoints, (int64_t*)nullptr, cn_ptr, total, cn_idx);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_segment_sum(s3grl_context* ctx, const float* h, int64_t num_source_rows, int64_t dim,
                               const int64_t* ptr, const int32_t* idx, int64_t num_rows, float* out) {
  if (!ctx || num_source_rows < 0 || num_source_rows >= (int64_t(1) << 31) || dim < 1 || dim > 65536 ||
      num_rows < 0 || num_rows >= (int64_t(1) << 31) || (num_rows > 0 && (!ptr || !out)) ||
      (num_source_rows > 0 && !h)) {
    set_last_error("segment_sum: need 0 <= M < 2^31, 1 <= H <= 65536 and 0 <= R < 2^31");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (num_rows == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const bool vec = dim % 4 == 0 && reinterpret_cast<uintptr_t>(h) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  auto* k = vec ? segment_sum_kernel<true, false> : segment_sum_kernel<false, false>;
  hipLaunchKernelGGL(k, dim3(grid_of(num_rows, kNcnWaves)), dim3(kNcnBlock), 0, ctx->stream, num_rows, dim, ptr, idx,
                     (const float*)nullptr, h, out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_cn_split_count(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                                  int64_t num_entries, const int32_t* links, int64_t num_links,
                                  int32_t exclude_endpoints, int64_t* counts) {
  if (!ctx || !indptr || bad_graph(num_nodes, num_entries, num_links) || (num_entries > 0 && !indices) ||
      (num_links > 0 && (!links || !counts)) || (exclude_endpoints != 0 && exclude_endpoints != 1)) {
    set_last_error("ncnc: need 1 <= N < 2^31, nnz < 2^31, fewer than 2^31 links and exclude_endpoints 0 or 1");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (num_links == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  S3GRL_TRY(check_links(ctx, links, num_links, num_nodes));
  hipLaunchKernelGGL(cn_split_kernel<false>, dim3(grid_of(num_links, kNcnWaves)), dim3(kNcnBlock), 0, st, num_links,
                     links, indptr, indices, (int)exclude_endpoints, counts, (const int64_t*)nullptr,
                     (const int64_t*)nullptr, (int64_t)0, (int32_t*)nullptr, (int32_t*)nullptr);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_cn_split_fill(s3grl_context* ctx, int64_t num_nodes, const int64_t* indptr, const int32_t* indices,
                                 int64_t num_entries, const int32_t* links, int64_t num_links,
                                 int32_t exclude_endpoints, const int64_t* counts, const int64_t* ptr, int64_t total,
                                 int32_t* idx, int32_t* side) {
  if (!ctx || !indptr || bad_graph(num_nodes, num_entries, num_links) || (num_entries > 0 && !indices) ||
      (num_links > 0 && (!links || !counts || !ptr)) || total < 0 || (total > 0 && (!idx || !side)) ||
      (exclude_endpoints != 0 && exclude_endpoints != 1)) {
    set_last_error("ncnc: need 1 <= N < 2^31, nnz < 2^31, fewer than 2^31 links, total >= 0 and exclude_endpoints 0 "
                   "or 1");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (num_links == 0 || total == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  S3GRL_TRY(check_links(ctx, links, num_links, num_nodes));
  hipLaunchKernelGGL(cn_split_kernel<true>, dim3(grid_of(num_links, kNcnWaves)), dim3(kNcnBlock), 0, st, num_links,
                     links, indptr, indices, (int)exclude_endpoints, (int64_t*)nullptr, counts, ptr, total, idx, side);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_segment_wsum(s3grl_context* ctx, const float* h, int64_t num_source_rows, int64_t dim,
                                const int64_t* ptr, const int32_t* idx, const float* w, int64_t num_rows, float* out) {
  if (!ctx || num_source_rows < 0 || num_source_rows >= (int64_t(1) << 31) || dim < 1 || dim > 65536 ||
      num_rows < 0 || num_rows >= (int64_t(1) << 31) || (num_rows > 0 && (!ptr || !out)) ||
      (num_source_rows > 0 && !h)) {
    set_last_error("segment_wsum: need 0 <= M < 2^31, 1 <= H <= 65536 and 0 <= R < 2^31");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (num_rows == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const bool vec = dim % 4 == 0 && reinterpret_cast<uintptr_t>(h) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  auto* k = vec ? segment_sum_kernel<true, true> : segment_sum_kernel<false, true>;
  hipLaunchKernelGGL(k, dim3(grid_of(num_rows, kNcnWaves)), dim3(kNcnBlock), 0, ctx->stream, num_rows, dim, ptr, idx, w,
                     h, out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_segment_dot(s3grl_context* ctx, const float* g, int64_t num_rows, const float* h,
                               int64_t num_source_rows, int64_t dim, const int64_t* ptr, const int32_t* idx,
                               float* out_w) {
  if (!ctx || num_source_rows < 0 || num_source_rows >= (int64_t(1) << 31) || dim < 1 || dim > 65536 ||
      num_rows < 0 || num_rows >= (int64_t(1) << 31) || (num_rows > 0 && (!ptr || !g)) ||
      (num_source_rows > 0 && !h)) {
    set_last_error("segment_dot: need 0 <= M < 2^31, 1 <= H <= 65536 and 0 <= R < 2^31");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (num_rows == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const bool vec = dim % 4 == 0 && reinterpret_cast<uintptr_t>(g) % 16 == 0 && reinterpret_cast<uintptr_t>(h) % 16 == 0;
  auto* k = vec ? segment_dot_kernel<true> : segment_dot_kernel<false>;
  hipLaunchKernelGGL(k, dim3(grid_of(num_rows, kNcnWaves)), dim3(kNcnBlock), 0, ctx->stream, num_rows, dim, ptr, idx, g,
                     h, out_w);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

}  // extern "C"
