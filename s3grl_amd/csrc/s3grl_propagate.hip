// Neighbour aggregation over a batch of subgraphs, gfx950: the one kernel behind GCNConv's propagation (PyG GCNConv
// message passing after its linear, with gcn_norm and add_remaining_self_loops; reference models.py:12-76 GCN,
// :139-222 DGCNN) and behind the raw-edge sum and mean of SAGEConv and GINConv.  Deterministic: no float atomics,
// every output element is summed in a fixed order, two runs are bit-identical.
//
// The operator's structure is a property of the split, not of the batch: the caller builds once per split a CSR over
// the split's nodes (ptr / nbr, nbr a position inside the node's own subgraph) grouped by destination for the forward
// and by source for the backward (the transposed operator).  A batch is a set of whole links laid out back to back;
// `rows` names the split node of every batch row, `loc` that node's position in its subgraph, so the batch row of
// neighbour nbr[e] is  r - loc[rows[r]] + nbr[e].  What differs between the operators is where an entry's weight
// comes from (WEIGHT) and the term added last:
//   kWeightEdge      out[r] = Σ_e coef[e] · h[row of nbr[e]]  (+ bias)                GCN, coef = dinv[j] · w_ji · dinv[i]
//   SCALE_NONE       out[r] = self·h[r] + Σ_e h[row of nbr[e]]                        sum, forward and backward
//   SCALE_OWN        out[r] = self·h[r] + scale[rows[r]] · Σ_e h[row of nbr[e]]       mean forward (CSR by destination)
//   SCALE_NEIGHBOUR  out[r] = self·h[r] + Σ_e scale[node of nbr[e]] · h[row of ..]    mean backward (CSR by source):
//                                                                the weight belongs to the arc's destination
// On the raw edge list nothing is normalised per edge and nothing is added or removed: input (i, i) entries are edges,
// a duplicated arc counts twice; the edge stream is nbr alone (4 bytes per edge) and the mean's 1 / indeg a per-NODE
// array.  One group of LPN lanes per node, VEC channels per lane (float4 when H % 4 == 0): H = 256 is a wavefront per
// node, H = 32 eight nodes per wavefront, H = 1 one node per lane; the channel loop covers H > 256.  Neighbours are
// walked in CSR order, four loads in flight, summed in that order; bias or the self term is added last.
#include "s3grl_internal.hpp"
#include "s3grl_device.hpp"

namespace s3grl {
namespace {

constexpr int kAggBlock = 256;
constexpr int kAggWaves = kAggBlock / 64;
constexpr int kWeightEdge = 3;   // a coefficient per CSR entry; beside the S3GRL_SCALE_* of the header, never in the ABI
static_assert(kWeightEdge != S3GRL_SCALE_NONE && kWeightEdge != S3GRL_SCALE_OWN && kWeightEdge != S3GRL_SCALE_NEIGHBOUR,
              "kWeightEdge must not be a scale side");

// deg[i] = Σ in-weights of i (loop included) in CSR order; dinv = deg^-1/2, 0 where deg == 0 (PyG: inf -> 0)
__global__ __launch_bounds__(kAggBlock) void gcn_norm_kernel(int64_t n, const int64_t* __restrict__ ptr,
                                                            const float* __restrict__ w, float* __restrict__ dinv) {
  const int64_t i = (int64_t)blockIdx.x * kAggBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t a = ptr[i], b = ptr[i + 1];
  float deg = 0.f;
  if (w) {
    for (int64_t e = a; e < b; ++e) deg += w[e];
  } else {
    deg = (float)(b - a);
  }
  const float d = 1.0f / sqrtf(deg);
  dinv[i] = isinf(d) ? 0.f : d;
}

// LPN lanes per node (a power of two dividing 64), VEC channels per lane, WEIGHT kWeightEdge or one of S3GRL_SCALE_*;
// `weight` is coef[entry] for kWeightEdge and scale[split node] for OWN / NEIGHBOUR.  kWeightEdge ends with bias (may be
// NULL) and never reads self_coef; the others end with self_coef · h[r] and never read bias.
template <int VEC, int LPN, int WEIGHT>
__global__ __launch_bounds__(kAggBlock) void nbr_agg_kernel(int64_t n_rows, int H, const int64_t* __restrict__ rows,
                                                           const int32_t* __restrict__ loc,
                                                           const int64_t* __restrict__ ptr,
                                                           const int32_t* __restrict__ nbr,
                                                           const float* __restrict__ weight,
                                                           const float* __restrict__ bias, float self_coef,
                                                           const float* __restrict__ h, float* __restrict__ out) {
  typedef Vec<VEC> V;
  typedef typename V::T T;
  constexpr int kNodesPerWave = 64 / LPN;
  constexpr bool kPerEntry = WEIGHT == kWeightEdge || WEIGHT == S3GRL_SCALE_NEIGHBOUR;
  const int lane = threadIdx.x & 63;
  const int q = lane % LPN;
  const int64_t r = ((int64_t)blockIdx.x * kAggWaves + (threadIdx.x >> 6)) * kNodesPerWave + lane / LPN;
  if (r >= n_rows) return;
  const int64_t g = rows[r];
  const int64_t lg = loc[g];
  const int64_t base = r - lg;                // batch row of the subgraph's first node
  const float* __restrict__ sc = WEIGHT == S3GRL_SCALE_NEIGHBOUR ? weight + (g - lg) : nullptr;   // its split node
  const int64_t e0 = ptr[g], e1 = ptr[g + 1];
  const float own = WEIGHT == S3GRL_SCALE_OWN ? weight[g] : 1.f;
  const auto w_of = [&](int64_t e, int32_t j) { return WEIGHT == kWeightEdge ? weight[e] : sc[j]; };
  for (int c = q * VEC; c < H; c += LPN * VEC) {
    const float* __restrict__ hc = h + c;
    T acc = (T)(0.f);
    int64_t e = e0;
    for (; e + 4 <= e1; e += 4) {   // four loads in flight, summed in CSR order
      const int32_t j0 = nbr[e], j1 = nbr[e + 1], j2 = nbr[e + 2], j3 = nbr[e + 3];
      const T v0 = V::load(hc + (base + j0) * H);
      const T v1 = V::load(hc + (base + j1) * H);
      const T v2 = V::load(hc + (base + j2) * H);
      const T v3 = V::load(hc + (base + j3) * H);
      if (kPerEntry) {
        const float w0 = w_of(e, j0), w1 = w_of(e + 1, j1), w2 = w_of(e + 2, j2), w3 = w_of(e + 3, j3);
        acc += w0 * v0;
        acc += w1 * v1;
        acc += w2 * v2;
        acc += w3 * v3;
      } else {
        acc += v0;
        acc += v1;
        acc += v2;
        acc += v3;
      }
    }
    for (; e < e1; ++e) {
      const int32_t j = nbr[e];
      const T v = V::load(hc + (base + j) * H);
      if (kPerEntry)
        acc += w_of(e, j) * v;
      else
        acc += v;
    }
    if (WEIGHT == S3GRL_SCALE_OWN) acc = own * acc;
    if (WEIGHT == kWeightEdge) {
      if (bias) acc += V::load(bias + c);
    } else {
      if (self_coef != 0.f) acc += self_coef * V::load(hc + r * H);
    }
    V::store(out + r * H + c, acc);
  }
}

template <int VEC, int WEIGHT>
s3grl_status launch_agg(hipStream_t st, int64_t n_rows, int H, const int64_t* rows, const int32_t* loc,
                        const int64_t* ptr, const int32_t* nbr, const float* weight, const float* bias,
                        float self_coef, const float* h, float* out) {
  const int cols = H / VEC;
  int lpn = 1;
  while (lpn < cols && lpn < 64) lpn <<= 1;
  const int64_t per_block = (int64_t)kAggWaves * (64 / lpn);
  const dim3 grid((unsigned)((n_rows + per_block - 1) / per_block)), block(kAggBlock);
#define AGG_CASE(L)                                                                                                \
  case L:                                                                                                          \
    hipLaunchKernelGGL((nbr_agg_kernel<VEC, L, WEIGHT>), grid, block, 0, st, n_rows, H, rows, loc, ptr, nbr, weight, \
                       bias, self_coef, h, out);                                                                   \
    break;
  switch (lpn) {
    AGG_CASE(1)
    AGG_CASE(2)
    AGG_CASE(4)
    AGG_CASE(8)
    AGG_CASE(16)
    AGG_CASE(32)
    AGG_CASE(64)
  }
#undef AGG_CASE
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

template <int WEIGHT>
s3grl_status launch_vec(s3grl_context* ctx, int64_t n_rows, int64_t H, const int64_t* rows, const int32_t* loc,
                        const int64_t* ptr, const int32_t* nbr, const float* weight, const float* bias,
                        float self_coef, const float* h, float* out) {
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  if (H % 4 == 0)
    return launch_agg<4, WEIGHT>(ctx->stream, n_rows, (int)H, rows, loc, ptr, nbr, weight, bias, self_coef, h, out);
  return launch_agg<1, WEIGHT>(ctx->stream, n_rows, (int)H, rows, loc, ptr, nbr, weight, bias, self_coef, h, out);
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

extern "C" {

s3grl_status s3grl_gcn_norm(s3grl_context* ctx, int64_t num_nodes, const int64_t* ptr, const float* weight,
                            float* dinv) {
  if (!ctx || num_nodes < 0 || (num_nodes > 0 && (!ptr || !dinv))) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_nodes == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(gcn_norm_kernel, dim3((unsigned)((num_nodes + kAggBlock - 1) / kAggBlock)), dim3(kAggBlock), 0,
                     ctx->stream, num_nodes, ptr, weight, dinv);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_gcn_propagate(s3grl_context* ctx, int64_t num_rows, int64_t hidden, const int64_t* rows,
                                 const int32_t* loc, const int64_t* ptr, const int32_t* nbr, const float* coef,
                                 const float* h, const float* bias, float* out) {
  if (!ctx || num_rows < 0 || hidden <= 0 || hidden > (1 << 20)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_rows > 0 && (!rows || !loc || !ptr || !nbr || !coef || !h || !out)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_rows == 0) return S3GRL_OK;
  return launch_vec<kWeightEdge>(ctx, num_rows, hidden, rows, loc, ptr, nbr, coef, bias, 0.f, h, out);
}

s3grl_status s3grl_nbr_aggregate(s3grl_context* ctx, int64_t num_rows, int64_t hidden, const int64_t* rows,
                                 const int32_t* loc, const int64_t* ptr, const int32_t* nbr, const float* scale,
                                 int32_t scale_side, float self_coef, const float* h, float* out) {
  if (!ctx || num_rows < 0 || hidden <= 0 || hidden > (1 << 20)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (scale_side != S3GRL_SCALE_NONE && scale_side != S3GRL_SCALE_OWN && scale_side != S3GRL_SCALE_NEIGHBOUR)
    return S3GRL_ERR_INVALID_ARGUMENT;
  if ((scale_side != S3GRL_SCALE_NONE) != (scale != nullptr)) {
    set_last_error("nbr_aggregate: scale and scale_side disagree (OWN / NEIGHBOUR need scale, NONE takes NULL)");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (!(self_coef == self_coef)) return S3GRL_ERR_INVALID_ARGUMENT;
  // ptr may be non-NULL with nbr NULL: a split without a single edge
  if (num_rows > 0 && (!rows || !loc || !ptr || !h || !out)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (num_rows == 0) return S3GRL_OK;
  switch (scale_side) {
    case S3GRL_SCALE_OWN:
      return launch_vec<S3GRL_SCALE_OWN>(ctx, num_rows, hidden, rows, loc, ptr, nbr, scale, nullptr, self_coef, h, out);
    case S3GRL_SCALE_NEIGHBOUR:
      return launch_vec<S3GRL_SCALE_NEIGHBOUR>(ctx, num_rows, hidden, rows, loc, ptr, nbr, scale, nullptr, self_coef, h,
                                               out);
    default:
      return launch_vec<S3GRL_SCALE_NONE>(ctx, num_rows, hidden, rows, loc, ptr, nbr, nullptr, nullptr, self_coef, h,
                                          out);
  }
}

}  // extern "C"
