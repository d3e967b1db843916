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

// where a lane's column k sits inside its block of kColBlock
template <bool VEC>
__device__ __forceinline__ int col_offset(int lane, int k) { return VEC ? 4 * lane + k : lane + 64 * k; }

// The partial of one chunk, entries [begin, end) with 1 <= end - begin <= kChunk: h's rows added one after the other
// in ascending entry, starting from the first entry itself.  The ids are loaded once and handed round by readlane.
template <bool VEC>
__device__ __forceinline__ Cols chunk_sum(int lane, const int32_t* __restrict__ idx, int64_t begin, int64_t end,
                                          const float* __restrict__ h, int64_t H, int64_t col0) {
  const int count = (int)(end - begin);
  const int mine = lane < count ? idx[begin + lane] : 0;
  Cols acc = load_cols<VEC>(h, __builtin_amdgcn_readlane(mine, 0), H, col0, lane);
  int j = 1;
  for (; j + kBatch <= count; j += kBatch) {   // kBatch rows in flight: the loads do not wait for each other
    Cols t[kBatch];
#pragma unroll
    for (int q = 0; q < kBatch; ++q) t[q] = load_cols<VEC>(h, __builtin_amdgcn_readlane(mine, j + q), H, col0, lane);
#pragma unroll
    for (int q = 0; q < kBatch; ++q) add_cols(acc, t[q]);
  }
  for (; j < count; ++j) add_cols(acc, load_cols<VEC>(h, __builtin_amdgcn_readlane(mine, j), H, col0, lane));
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
// one after the other, their chunks dealt to the four wavefronts.
template <bool VEC>
__global__ __launch_bounds__(kNcnBlock) void segment_sum_kernel(int64_t R, int64_t H, const int64_t* __restrict__ ptr,
                                                                const int32_t* __restrict__ idx,
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
            acc = chunk_sum<VEC>(lane, idx, begin, end, h, H, col0);
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
          const Cols acc = chunk_sum<VEC>(lane, idx, b, b + kChunk < end ? b + kChunk : end, h, H, col0);
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
  auto* k = vec ? segment_sum_kernel<true> : segment_sum_kernel<false>;
  hipLaunchKernelGGL(k, dim3(grid_of(num_rows, kNcnWaves)), dim3(kNcnBlock), 0, ctx->stream, num_rows, dim, ptr, idx,
                     h, out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

}  // extern "C"
