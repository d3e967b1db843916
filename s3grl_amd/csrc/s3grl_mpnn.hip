// global_mean_pool (the segment mean) for the GIN twin, gfx950.  Deterministic: no float atomics, every output element
// is summed in a fixed order, two runs are bit-identical.  (The neighbour aggregation of SAGEConv and GINConv is in
// s3grl_propagate.hip.)
//
// Segment mean: graph g owns the rows node_ptr[g] .. node_ptr[g+1].  A workgroup takes one chunk of kSegChunk rows of
// one graph and one tile of CL columns (CL lanes side by side, coalesced), its 256 / CL row slices each summed in
// row order and then combined by a fixed butterfly (lanes) and a fixed order (waves).  A graph of one chunk is
// finished there; longer graphs leave one partial row per chunk, added in chunk order by a second launch.
#include "s3grl_internal.hpp"

#include <algorithm>

namespace s3grl {
namespace {

constexpr int kMpBlock = 256;
constexpr int kMpWaves = kMpBlock / 64;
constexpr int64_t kSegChunk = 2048;   // rows of a graph per workgroup: at most kSegChunk·CL / 256 rows per lane

// grid (graphs, column tiles, chunks); CL column lanes (a power of two dividing 64), 256 / CL row slices
template <int CL>
__global__ __launch_bounds__(kMpBlock) void seg_mean_fwd_kernel(const float* __restrict__ x,
                                                               const int64_t* __restrict__ node_ptr, int W,
                                                               int chunks, float* __restrict__ partial,
                                                               float* __restrict__ out) {
  constexpr int kSlicesPerWave = 64 / CL;
  constexpr int kSlices = kMpWaves * kSlicesPerWave;
  __shared__ float s_part[kMpWaves][CL];
  const int64_t g = blockIdx.x;
  const int64_t r0 = node_ptr[g];
  const int64_t n = node_ptr[g + 1] - r0;
  const int64_t z = blockIdx.z;
  // chunks == 1: the caller promised no graph is longer than a chunk; a longer one is still walked whole here
  const bool direct = chunks == 1 || n <= kSegChunk;
  const int64_t a = z * kSegChunk;
  const int64_t b = (chunks == 1 || a + kSegChunk > n) ? n : a + kSegChunk;
  if (z > 0 && a >= n) return;               // past the graph's last chunk (workgroup-uniform)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cl = lane % CL;
  const int c = blockIdx.y * CL + cl;
  const int slice = wave * kSlicesPerWave + lane / CL;
  float acc = 0.f;
  if (c < W) {
    const float* __restrict__ xc = x + r0 * W + c;
    int64_t i = a + slice;
    for (; i + 3 * kSlices < b; i += 4 * kSlices) {   // four loads in flight, added in row order
      const float v0 = xc[i * W], v1 = xc[(i + kSlices) * W], v2 = xc[(i + 2 * kSlices) * W],
                  v3 = xc[(i + 3 * kSlices) * W];
      acc += v0;
      acc += v1;
      acc += v2;
      acc += v3;
    }
    for (; i < b; i += kSlices) acc += xc[i * W];
  }
  for (int o = CL; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);   // the wave's slices, fixed butterfly
  if (lane < CL) s_part[wave][lane] = acc;
  __syncthreads();
  if (threadIdx.x < CL && c < W) {
    float s = s_part[0][threadIdx.x];
    for (int w = 1; w < kMpWaves; ++w) s += s_part[w][threadIdx.x];
    if (direct)
      out[g * W + c] = s / (float)(n > 0 ? n : 1);
    else
      partial[(g * chunks + z) * W + c] = s;
  }
}

// graphs longer than one chunk: out[g] = (Σ_z partial[g, z]) / n in chunk order
__global__ __launch_bounds__(kMpBlock) void seg_mean_combine_kernel(const int64_t* __restrict__ node_ptr,
                                                                   int64_t num_graphs, int W, int chunks,
                                                                   const float* __restrict__ partial,
                                                                   float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kMpBlock + threadIdx.x;
  if (i >= num_graphs * W) return;
  const int64_t g = i / W;
  const int c = (int)(i - g * W);
  const int64_t n = node_ptr[g + 1] - node_ptr[g];
  if (chunks == 1 || n <= kSegChunk) return;
  int64_t used = (n + kSegChunk - 1) / kSegChunk;
  if (used > chunks) used = chunks;          // a graph longer than the caller's max_nodes: never past the buffer
  const float* __restrict__ p = partial + g * chunks * W + c;
  float s = 0.f;
  for (int64_t z = 0; z < used; ++z) s += p[z * W];
  out[i] = s / (float)n;
}

// grid (graphs, chunks): grad_x[r] = grad_out[g] / max(n, 1) for the chunk's rows
__global__ __launch_bounds__(kMpBlock) void seg_mean_bwd_kernel(const int64_t* __restrict__ node_ptr, int W,
                                                               const float* __restrict__ gout,
                                                               float* __restrict__ gx) {
  const int64_t g = blockIdx.x;
  const int64_t r0 = node_ptr[g];
  const int64_t n = node_ptr[g + 1] - r0;
  const int64_t a = (int64_t)blockIdx.y * kSegChunk;
  const int64_t b = a + kSegChunk > n ? n : a + kSegChunk;
  if (a >= n) return;
  const float dn = (float)n;
  const float* __restrict__ go = gout + g * W;
  float* __restrict__ d = gx + (r0 + a) * W;
  if (kMpBlock % W == 0) {   // W divides the block: a thread keeps one column, one read of grad_out
    const float v = go[threadIdx.x % W] / dn;
    const int64_t total = (b - a) * W;
    for (int64_t i = threadIdx.x; i < total; i += kMpBlock) d[i] = v;
  } else {                   // a wavefront per row
    const int lane = threadIdx.x & 63;
    for (int64_t i = threadIdx.x >> 6; i < b - a; i += kMpWaves)
      for (int c = lane; c < W; c += 64) d[i * W + c] = go[c] / dn;
  }
}

int64_t seg_chunks(int64_t max_nodes) { return std::max<int64_t>((max_nodes + kSegChunk - 1) / kSegChunk, 1); }

}  // namespace
}  // namespace s3grl

using namespace s3grl;

extern "C" {

s3grl_status s3grl_segment_mean_forward(s3grl_context* ctx, const float* x, const int64_t* node_ptr,
                                        int64_t num_graphs, int64_t width, int64_t max_nodes, float* partial,
                                        float* out) {
  if (!ctx || num_graphs < 0 || num_graphs >= (int64_t(1) << 31) || width <= 0 || width > (1 << 20) ||
      max_nodes < 0 || max_nodes >= (int64_t(1) << 31))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_graphs > 0 && (!node_ptr || !out || (max_nodes > 0 && !x))) return S3GRL_ERR_INVALID_ARGUMENT;
  const int64_t chunks = seg_chunks(max_nodes);
  if (chunks > 1 && !partial) {
    set_last_error("segment mean: a graph of max_nodes spans several chunks and no partial buffer was given");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (chunks > 65535) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_graphs == 0) return S3GRL_OK;
  int cl = 1;
  while (cl < width && cl < 64) cl <<= 1;
  const int64_t tiles = (width + cl - 1) / cl;
  if (tiles > 65535) return S3GRL_ERR_INVALID_ARGUMENT;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const dim3 grid((unsigned)num_graphs, (unsigned)tiles, (unsigned)chunks), block(kMpBlock);
#define SEG_CASE(L)                                                                                          \
  case L:                                                                                                    \
    hipLaunchKernelGGL((seg_mean_fwd_kernel<L>), grid, block, 0, ctx->stream, x, node_ptr, (int)width, (int)chunks, \
                       partial, out);                                                                        \
    break;
  switch (cl) {
    SEG_CASE(1)
    SEG_CASE(2)
    SEG_CASE(4)
    SEG_CASE(8)
    SEG_CASE(16)
    SEG_CASE(32)
    SEG_CASE(64)
  }
#undef SEG_CASE
  S3GRL_HIP_TRY(hipGetLastError());
  if (chunks > 1) {
    const int64_t total = num_graphs * width;
    hipLaunchKernelGGL(seg_mean_combine_kernel, dim3((unsigned)((total + kMpBlock - 1) / kMpBlock)), block, 0,
                       ctx->stream, node_ptr, num_graphs, (int)width, (int)chunks, partial, out);
    S3GRL_HIP_TRY(hipGetLastError());
  }
  return S3GRL_OK;
}

s3grl_status s3grl_segment_mean_backward(s3grl_context* ctx, const int64_t* node_ptr, int64_t num_graphs,
                                         int64_t width, int64_t max_nodes, const float* grad_out, float* grad_x) {
  if (!ctx || num_graphs < 0 || num_graphs >= (int64_t(1) << 31) || width <= 0 || width > (1 << 20) ||
      max_nodes < 0 || max_nodes >= (int64_t(1) << 31))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_graphs > 0 && (!node_ptr || !grad_out || (max_nodes > 0 && !grad_x))) return S3GRL_ERR_INVALID_ARGUMENT;
  const int64_t chunks = seg_chunks(max_nodes);
  if (chunks > 65535) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_graphs == 0 || max_nodes == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(seg_mean_bwd_kernel, dim3((unsigned)num_graphs, (unsigned)chunks), dim3(kMpBlock), 0, ctx->stream,
                     node_ptr, (int)width, grad_out, grad_x);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

}  // extern "C"
