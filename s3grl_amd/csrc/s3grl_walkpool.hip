// WalkPool's own operator on a batch of enclosing subgraphs (reference Software/WalkPooling/src/model.py:74-219),
// gfx950: the attention weights of every arc, normalised per target node on the graph with (E+) and without (E-) the
// candidate link, and the walk profile of the powers 2 .. walk_len + 1 of those two row-stochastic matrices.
// Deterministic: no float atomics, every sum in a fixed order, two runs are bit-identical in values and gradients.
//
// Structure (s3grl_wp_batch): the arcs of E+ of every link of the batch, grouped by target node (in_*) and by source
// node (out_*, with the position of the same arc in the in-order), a node as its position in its own subgraph;
// local nodes 0 and 1 are the candidate link, its two arcs carry in_flag = 1.  Per-arc arrays are [e, heads] in the
// in-order.
//
// Attention: one wavefront per target node c, lanes over its in-arcs, heads in a loop.  Pass 1 writes the logit
// w = <q[r,h], k[c,h]> / sqrt(hidden) and finds the maximum over E+, pass 2 sums exp(w - max) over E+ and over E-,
// pass 3 divides (PyG softmax's + 1e-16 in both).  The wavefront of local node 0 also writes omega.  Backward:
// one wavefront per target node turns the three upstream gradients into d w per arc; a second launch sums d k over
// the arcs into a node and d q over the arcs out of it, lanes over (head, channel), arcs in CSR order.
//
// Walk profile: the columns of X = P^tau are independent, X_tau[:, col] = P X_{tau-1}[:, col] with P[c, r] the
// weight of r -> c.  A workgroup owns column blocks of one (link, head, sign), W columns each, and keeps the
// n x W ping-pong in LDS as rows of W floats, one float4 per lane.  A pull's stores go to consecutive rows, which
// fall on distinct banks for W = 4 and 8; its reads are a gather by neighbour id (rows nbr[e]), whose bank conflicts
// depend on the graph and have not been counted.  It pulls along the in-arc CSR once per power, eight lanes sharing a row's arcs so
// that a hub row is no long chain (slot s adds arcs s, s + 8, .., then a butterfly), and emits its own diagonal entries
// (a partial trace) and, from block 0, the four entries of local nodes 0 and 1.  `groups` workgroups share a
// (link, head, sign): group g takes blocks g, g + groups, ..; a second launch adds the groups' partial traces in
// group order.  An element of X never depends on W or on the flavour, so only the traces do.
// Backward, the reverse chain over the same column block: the powers X_1 .. X_{T-1} (T = walk_len + 1) are
// recomputed and kept, A_T = G_T, A_{tau-1} = G_{tau-1} + P^T A_tau along the out-arc CSR, and every arc adds
// sum_cols A_tau[c, .] X_{tau-1}[r, .] to the group's own partial slice; a second launch adds the slices in group
// order.  G is the upstream gradient on the diagonal and on the four entries.  Nothing of size n x n is in HBM.
// A batch whose largest subgraph does not fit the LDS budget at W = 4 runs the same kernels with the block's
// arrays in an HBM workspace (flavour 1).
#include "s3grl_internal.hpp"
#include "s3grl_device.hpp"
#include "s3grl_train.hpp"

#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

namespace s3grl {
namespace {

constexpr int kWpBlock = 256;
constexpr int kWpWaves = kWpBlock / 64;
constexpr int64_t kWpMaxNodes = 4096;
constexpr int kWpMaxWalk = 16;
constexpr int kWpMaxGroups = 8;                 // workgroups per (link, head, sign)
constexpr int kWpSlots = 8;                      // lanes that share a row's arcs in a pull
constexpr int kWpArcRegs = 20;                  // arc sums a backward thread keeps in registers: links of <= 5120 arcs
constexpr int64_t kWpDefaultLds = 80 << 10;     // 160 KiB per CU: leaves room for one more workgroup
constexpr int64_t kWpMaxLds = 159 << 10;

struct WpPlan {
  int W;            // columns per block
  int groups;       // workgroups per (link, head, sign)
  int hbm;          // 1: the block's arrays live in the workspace
  int64_t arrays;   // n x W arrays a workgroup holds
  int64_t ws_link;  // workspace bytes per link
};

int64_t wp_budget(int64_t lds_budget) { return lds_budget > 1 ? std::min(lds_budget, kWpMaxLds) : kWpDefaultLds; }

// forward: the ping-pong (2 arrays); backward: X_1 .. X_{T-1} and the ping-pong of A (T + 1 arrays)
WpPlan wp_plan(int64_t n_max, int64_t e_max, int heads, int walk_len, int64_t lds_budget, bool backward) {
  WpPlan p;
  p.arrays = backward ? walk_len + 2 : 2;
  const int64_t n = std::max<int64_t>(n_max, 2);
  const int64_t budget = wp_budget(lds_budget);
  p.W = 0;
  if (lds_budget != 1)
    for (int w = 32; w >= 4; w >>= 1)
      if (p.arrays * n * w * 4 <= budget && (w == 4 || w < 2 * n)) {
        p.W = w;
        break;
      }
  p.hbm = p.W == 0;
  if (p.hbm) p.W = 4;
  p.groups = (int)std::min<int64_t>((n + p.W - 1) / p.W, kWpMaxGroups);
  const int64_t per_group = (backward ? 0 : walk_len) + (p.hbm ? p.arrays * n * p.W : 0);
  p.ws_link = 4 * ((int64_t)heads * 2 * p.groups * per_group + (backward ? (int64_t)p.groups * 2 * e_max * heads : 0));
  return p;
}

__device__ __forceinline__ float wp_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wp_wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wp_dot(const float* __restrict__ a, const float* __restrict__ b, int d) {
  float s = 0.f;
  for (int i = 0; i < d; ++i) s = fmaf(a[i], b[i], s);
  return s;
}

// ---- attention -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWpBlock) void wp_attn_fwd_kernel(s3grl_wp_batch bt, int heads, int hidden,
                                                              const float* __restrict__ q,
                                                              const float* __restrict__ k, float* __restrict__ w,
                                                              float* __restrict__ wp, float* __restrict__ wm,
                                                              float* __restrict__ omega) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWpWaves + (threadIdx.x >> 6);
  if (r >= bt.num_nodes) return;
  const int64_t b = bt.link[r];
  const int64_t base = bt.node_ptr[b];
  const int64_t e0 = bt.in_ptr[r], e1 = bt.in_ptr[r + 1];
  const float root = sqrtf((float)hidden);
  for (int h = 0; h < heads; ++h) {
    const float* __restrict__ kc = k + (r * heads + h) * hidden;
    float mx = -INFINITY;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const float v = wp_dot(q + ((base + bt.in_nbr[e]) * heads + h) * hidden, kc, hidden) / root;
      w[e * heads + h] = v;
      mx = fmaxf(mx, v);
    }
    mx = wp_wave_max(mx);
    float sp = 0.f, sm = 0.f;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const float ex = expf(w[e * heads + h] - mx);
      sp += ex;
      if (!bt.in_flag[e]) sm += ex;
    }
    sp = wp_wave_sum(sp) + 1e-16f;
    sm = wp_wave_sum(sm) + 1e-16f;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const float ex = expf(w[e * heads + h] - mx);
      wp[e * heads + h] = ex / sp;
      wm[e * heads + h] = bt.in_flag[e] ? 0.f : ex / sm;
    }
  }
  if (r == base && lane < heads && bt.node_ptr[b + 1] - base >= 2) {   // local node 0: the link's omega
    const int h = lane;
    const float wij = wp_dot(q + (base * heads + h) * hidden, k + ((base + 1) * heads + h) * hidden, hidden) / root;
    const float wji = wp_dot(q + ((base + 1) * heads + h) * hidden, k + (base * heads + h) * hidden, hidden) / root;
    omega[b * heads + h] = sigmoid32(wij) + sigmoid32(wji);
  }
}

// d w per arc from the gradients of weights_p, weights_m and omega (the maximum is a constant, as in PyG's softmax)
__global__ __launch_bounds__(kWpBlock) void wp_attn_dw_kernel(s3grl_wp_batch bt, int heads,
                                                             const float* __restrict__ w,
                                                             const float* __restrict__ wp,
                                                             const float* __restrict__ wm,
                                                             const float* __restrict__ gp,
                                                             const float* __restrict__ gm,
                                                             const float* __restrict__ gomega,
                                                             float* __restrict__ dw) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWpWaves + (threadIdx.x >> 6);
  if (r >= bt.num_nodes) return;
  const int64_t b = bt.link[r];
  const int64_t e0 = bt.in_ptr[r], e1 = bt.in_ptr[r + 1];
  for (int h = 0; h < heads; ++h) {
    float a = 0.f, c = 0.f;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      a = fmaf(wp[e * heads + h], gp[e * heads + h], a);
      c = fmaf(wm[e * heads + h], gm[e * heads + h], c);
    }
    a = wp_wave_sum(a);
    c = wp_wave_sum(c);
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const int64_t i = e * heads + h;
      float d = wp[i] * (gp[i] - a) + wm[i] * (gm[i] - c);
      if (bt.in_flag[e]) {
        const float s = sigmoid32(w[i]);
        d = fmaf(gomega[b * heads + h], s * (1.f - s), d);
      }
      dw[i] = d;
    }
  }
}

// dk[c] over the arcs into c, dq[r] over the arcs out of r; lanes over (head, channel)
__global__ __launch_bounds__(kWpBlock) void wp_attn_dqk_kernel(s3grl_wp_batch bt, int heads, int hidden,
                                                              const float* __restrict__ q,
                                                              const float* __restrict__ k,
                                                              const float* __restrict__ dw, float* __restrict__ dq,
                                                              float* __restrict__ dk) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWpWaves + (threadIdx.x >> 6);
  if (r >= bt.num_nodes) return;
  const int64_t base = bt.node_ptr[bt.link[r]];
  const int HD = heads * hidden;
  const float root = sqrtf((float)hidden);
  for (int i = lane; i < HD; i += 64) {
    const int h = i / hidden;
    float sk = 0.f, sq = 0.f;
    for (int64_t e = bt.in_ptr[r]; e < bt.in_ptr[r + 1]; ++e)
      sk = fmaf(dw[e * heads + h], q[(base + bt.in_nbr[e]) * HD + i], sk);
    for (int64_t e = bt.out_ptr[r]; e < bt.out_ptr[r + 1]; ++e)
      sq = fmaf(dw[bt.out_arc[e] * heads + h], k[(base + bt.out_nbr[e]) * HD + i], sq);
    dk[r * HD + i] = sk / root;
    dq[r * HD + i] = sq / root;
  }
}

// ---- walk profile ------------------------------------------------------------------------------------------------
struct WpBlockId {
  int g, sign, h;
  int64_t b;
};
__device__ __forceinline__ WpBlockId wp_block_id(int heads, int groups) {
  WpBlockId id;
  int64_t t = blockIdx.x;
  id.g = (int)(t % groups);
  t /= groups;
  id.sign = (int)(t & 1);
  t >>= 1;
  id.h = (int)(t % heads);
  id.b = t / heads;
  return id;
}

// A row's arcs are shared by kWpSlots lanes per float4 of columns: slot s adds the arcs s, s + kWpSlots, .. in CSR order,
// then the slots are added by a butterfly.  The order does not depend on W, and the longest chain of a hub row is
// degree / kWpSlots.  A node's lanes are kWpSlots · W / 4 consecutive ones of a wavefront: item = (node, slot, sub).
template <int W>
__device__ __forceinline__ float4_t wp_slot_sum(float4_t acc) {
  constexpr int Q = W / 4;
#pragma unroll
  for (int o = Q; o < kWpSlots * Q; o <<= 1) {
    acc[0] += __shfl_xor(acc[0], o);
    acc[1] += __shfl_xor(acc[1], o);
    acc[2] += __shfl_xor(acc[2], o);
    acc[3] += __shfl_xor(acc[3], o);
  }
  return acc;
}

// nxt[node] = seed + sum over the arcs of `node` of weight * cur[other end]: along the in-arcs (OUT = false, a power's
// pull) or along the out-arcs with the weight at the arc's in-order position (OUT = true, the backward's P^T)
template <int W, bool OUT, typename Seed>
__device__ __forceinline__ void wp_pull(const s3grl_wp_batch& bt, int64_t base, int n, int heads, int h,
                                        const float* __restrict__ wgt, const float* cur, float* nxt, Seed seed) {
  constexpr int Q = W / 4, G = kWpSlots * Q;
  const int64_t* __restrict__ ptr = OUT ? bt.out_ptr : bt.in_ptr;
  const int32_t* __restrict__ nbr = OUT ? bt.out_nbr : bt.in_nbr;
  const int total = (n * G + kWpBlock - 1) / kWpBlock * kWpBlock;   // whole wavefronts take part in the butterfly
  for (int item = threadIdx.x; item < total; item += kWpBlock) {
    const int node = item / G, slot = (item % G) / Q, sub = item % Q;
    float4_t acc = (float4_t)(0.f);
    if (node < n) {
      const int64_t e1 = ptr[base + node + 1];
      for (int64_t e = ptr[base + node] + slot; e < e1; e += kWpSlots) {
        const int64_t a = OUT ? bt.out_arc[e] : e;
        acc += wgt[a * heads + h] * *reinterpret_cast<const float4_t*>(cur + nbr[e] * W + sub * 4);
      }
    }
    acc = wp_slot_sum<W>(acc);
    if (node < n && slot == 0) *reinterpret_cast<float4_t*>(nxt + node * W + sub * 4) = acc + seed(node, sub);
  }
}

struct WpNoSeed {
  __device__ __forceinline__ float4_t operator()(int, int) const { return (float4_t)(0.f); }
};

// X_1 of the block: the pull of the identity's columns c0 .. c0 + W (at most one arc per entry: exact)
template <int W>
__device__ __forceinline__ void wp_first(const s3grl_wp_batch& bt, int64_t base, int n, int heads, int h, int c0,
                                         const float* __restrict__ wgt, float* nxt) {
  constexpr int Q = W / 4, G = kWpSlots * Q;
  const int total = (n * G + kWpBlock - 1) / kWpBlock * kWpBlock;
  for (int item = threadIdx.x; item < total; item += kWpBlock) {
    const int node = item / G, slot = (item % G) / Q, sub = item % Q;
    float4_t acc = (float4_t)(0.f);
    if (node < n) {
      const int64_t e1 = bt.in_ptr[base + node + 1];
      for (int64_t e = bt.in_ptr[base + node] + slot; e < e1; e += kWpSlots) {
        const int d = bt.in_nbr[e] - c0 - sub * 4;
        if (d >= 0 && d < 4) acc[d] += wgt[e * heads + h];
      }
    }
    acc = wp_slot_sum<W>(acc);
    if (node < n && slot == 0) *reinterpret_cast<float4_t*>(nxt + node * W + sub * 4) = acc;
  }
}

template <int W, bool LDS>
__global__ __launch_bounds__(kWpBlock) void wp_walk_fwd_kernel(s3grl_wp_batch bt, int heads, int walk_len, int groups,
                                                              int n_cap, const float* __restrict__ wp,
                                                              const float* __restrict__ wm, float* __restrict__ ws,
                                                              float* __restrict__ part, float* __restrict__ out) {
  extern __shared__ __align__(16) float s_wp[];
  __shared__ float s_tr[kWpMaxWalk];
  const WpBlockId id = wp_block_id(heads, groups);
  const int64_t base = bt.node_ptr[id.b];
  const int64_t n64 = bt.node_ptr[id.b + 1] - base;
  const int n = n64 >= 2 && n64 <= n_cap ? (int)n64 : 0;   // outside the host's promise: zero features
  const float* __restrict__ wgt = id.sign ? wm : wp;
  float* cur = LDS ? s_wp : ws + (int64_t)blockIdx.x * 2 * n_cap * W;
  float* nxt = cur + (int64_t)n_cap * W;
  float* o = out + (id.b * heads + id.h) * walk_len * 5;
  if (threadIdx.x < walk_len) s_tr[threadIdx.x] = 0.f;
  if (n == 0 && id.g == 0 && threadIdx.x < walk_len) {
    o[threadIdx.x * 5 + 1 + id.sign] = 0.f;
    o[threadIdx.x * 5 + 3 + id.sign] = 0.f;
  }
  __syncthreads();
  const int nblk = (n + W - 1) / W;
  for (int blk = id.g; blk < nblk; blk += groups) {
    const int c0 = blk * W;
    wp_first<W>(bt, base, n, heads, id.h, c0, wgt, cur);
    __syncthreads();
    for (int t = 0; t < walk_len; ++t) {   // cur = X_{t+1}, nxt becomes X_{t+2}
      wp_pull<W, false>(bt, base, n, heads, id.h, wgt, cur, nxt, WpNoSeed());
      __syncthreads();
      float* s = cur;
      cur = nxt;
      nxt = s;
      if (threadIdx.x == 0) {
        float tr = s_tr[t];
        for (int c = c0; c < c0 + W && c < n; ++c) tr += cur[c * W + (c - c0)];
        s_tr[t] = tr;
        if (blk == 0) {
          o[t * 5 + 1 + id.sign] = cur[0] + cur[W + 1];       // X[i,i] + X[j,j]
          o[t * 5 + 3 + id.sign] = cur[1] + cur[W];           // X[i,j] + X[j,i]
        }
      }
    }
    __syncthreads();   // thread 0 has read the last power before the next block overwrites it
  }
  if (threadIdx.x < walk_len) part[(int64_t)blockIdx.x * walk_len + threadIdx.x] = s_tr[threadIdx.x];
}

// graphlevel = tr(X+) - tr(X-), each trace the groups' partials added in group order
__global__ __launch_bounds__(kWpBlock) void wp_trace_kernel(int64_t count, int walk_len, int groups,
                                                           const float* __restrict__ part, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kWpBlock + threadIdx.x;   // (link, head, t)
  if (i >= count) return;
  const int64_t bh = i / walk_len;
  const int t = (int)(i % walk_len);
  float tr[2];
  for (int sign = 0; sign < 2; ++sign) {
    float s = 0.f;
    for (int g = 0; g < groups; ++g) s += part[((bh * 2 + sign) * groups + g) * walk_len + t];
    tr[sign] = s;
  }
  out[i * 5] = tr[0] - tr[1];
}

// the upstream gradient of X_tau[node, col] (tau = t + 2): the trace's on the diagonal, the node and link
// features' on the four entries of local nodes 0 and 1
__device__ __forceinline__ float wp_seed(int node, int col, float g_tr, float g_node, float g_link) {
  float s = node == col ? g_tr : 0.f;
  if (node < 2 && col < 2) s += node == col ? g_node : g_link;
  return s;
}

template <int W, bool LDS>
__global__ __launch_bounds__(kWpBlock) void wp_walk_bwd_kernel(s3grl_wp_batch bt, int heads, int walk_len, int groups,
                                                              int n_cap, const float* __restrict__ wp,
                                                              const float* __restrict__ wm,
                                                              const float* __restrict__ gout, float* __restrict__ ws,
                                                              float* __restrict__ dpart) {
  extern __shared__ __align__(16) float s_wp[];
  constexpr int Q = W / 4;
  const WpBlockId id = wp_block_id(heads, groups);
  const int64_t base = bt.node_ptr[id.b];
  const int64_t n64 = bt.node_ptr[id.b + 1] - base;
  if (n64 < 2 || n64 > n_cap) return;   // uniform for the workgroup; its slice stays zero
  const int n = (int)n64;
  const int h = id.h;
  const float* __restrict__ wgt = id.sign ? wm : wp;
  const int64_t stride = (int64_t)n_cap * W;
  float* pw = LDS ? s_wp : ws + (int64_t)blockIdx.x * (walk_len + 2) * stride;   // X_tau at pw + (tau - 1) stride
  float* a_cur = pw + walk_len * stride;
  float* a_nxt = a_cur + stride;
  const float* __restrict__ go = gout + (id.b * heads + h) * walk_len * 5;
  const float sgn = id.sign ? -1.f : 1.f;
  const int64_t ea = bt.in_ptr[base], eb = bt.in_ptr[base + n];
  float* __restrict__ dp = dpart + ((int64_t)(id.g * 2 + id.sign) * bt.num_arcs) * heads;
  const int T = walk_len + 1;
  const int nblk = (n + W - 1) / W;
  const bool in_regs = eb - ea <= (int64_t)kWpArcRegs * kWpBlock;
  float acc[kWpArcRegs];
#pragma unroll
  for (int j = 0; j < kWpArcRegs; ++j) acc[j] = 0.f;
  for (int blk = id.g; blk < nblk; blk += groups) {
    const int c0 = blk * W;
    wp_first<W>(bt, base, n, heads, h, c0, wgt, pw);
    __syncthreads();
    for (int tau = 2; tau < T; ++tau) {
      wp_pull<W, false>(bt, base, n, heads, h, wgt, pw + (tau - 2) * stride, pw + (tau - 1) * stride, WpNoSeed());
      __syncthreads();
    }
    {   // A_T = G_T
      const int t = T - 2;
      const float g_tr = sgn * go[t * 5], g_node = go[t * 5 + 1 + id.sign], g_link = go[t * 5 + 3 + id.sign];
      for (int item = threadIdx.x; item < n * Q; item += kWpBlock) {
        const int node = item / Q, sub = item % Q;
        float4_t v;
        for (int d = 0; d < 4; ++d) v[d] = wp_seed(node, c0 + sub * 4 + d, g_tr, g_node, g_link);
        *reinterpret_cast<float4_t*>(a_cur + node * W + sub * 4) = v;
      }
    }
    __syncthreads();
    for (int tau = T; tau >= 1; --tau) {
      // every arc r -> c of the link: dP[c, r] += sum_cols A_tau[c, .] X_{tau-1}[r, .]   (X_0 = I); an arc is
      // always this thread's, so its sum stays in a register while the link's arcs fit kWpArcRegs per thread
      const float* xp = tau > 1 ? pw + (tau - 2) * stride : pw;
      const auto arc_term = [&](int64_t e) {
        const int c = bt.in_dst[e], r = bt.in_nbr[e];
        float s = 0.f;
        if (tau == 1) {
          if (r >= c0 && r < c0 + W) s = a_cur[c * W + (r - c0)];
        } else {
          for (int u = 0; u < Q; ++u) {
            const float4_t av = *reinterpret_cast<const float4_t*>(a_cur + c * W + u * 4);
            const float4_t xv = *reinterpret_cast<const float4_t*>(xp + r * W + u * 4);
            s = fmaf(av[0], xv[0], s);
            s = fmaf(av[1], xv[1], s);
            s = fmaf(av[2], xv[2], s);
            s = fmaf(av[3], xv[3], s);
          }
        }
        return s;
      };
      if (in_regs) {
#pragma unroll
        for (int j = 0; j < kWpArcRegs; ++j) {
          const int64_t e = ea + threadIdx.x + j * kWpBlock;
          if (e < eb) acc[j] += arc_term(e);
        }
      } else {
        for (int64_t e = ea + threadIdx.x; e < eb; e += kWpBlock) dp[e * heads + h] += arc_term(e);
      }
      if (tau > 1) {   // A_{tau-1} = G_{tau-1} + P^T A_tau, along the arcs out of every node
        const int t = tau - 3;
        float g_tr = 0.f, g_node = 0.f, g_link = 0.f;
        if (t >= 0) {
          g_tr = sgn * go[t * 5];
          g_node = go[t * 5 + 1 + id.sign];
          g_link = go[t * 5 + 3 + id.sign];
        }
        wp_pull<W, true>(bt, base, n, heads, h, wgt, a_cur, a_nxt, [&](int node, int sub) {
          float4_t g = (float4_t)(0.f);
          if (t >= 0)
            for (int d = 0; d < 4; ++d) g[d] = wp_seed(node, c0 + sub * 4 + d, g_tr, g_node, g_link);
          return g;
        });
      }
      __syncthreads();
      float* s = a_cur;
      a_cur = a_nxt;
      a_nxt = s;
    }
  }
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < kWpArcRegs; ++j) {
      const int64_t e = ea + threadIdx.x + j * kWpBlock;
      if (e < eb) dp[e * heads + h] = acc[j];
    }
  }
}

// d weights_p / d weights_m of every arc: the groups' slices added in group order
__global__ __launch_bounds__(kWpBlock) void wp_arc_sum_kernel(int64_t count, int groups,
                                                             const float* __restrict__ dpart,
                                                             float* __restrict__ dwp, float* __restrict__ dwm) {
  const int64_t i = (int64_t)blockIdx.x * kWpBlock + threadIdx.x;   // (arc, head)
  if (i >= count) return;
  float sp = 0.f, sm = 0.f;
  for (int g = 0; g < groups; ++g) {
    sp += dpart[(int64_t)(g * 2) * count + i];
    sm += dpart[(int64_t)(g * 2 + 1) * count + i];
  }
  dwp[i] = sp;
  dwm[i] = sm;
}

bool wp_batch_ok(const s3grl_wp_batch* bt) {
  if (!bt || bt->num_links < 0 || bt->num_nodes < 0 || bt->num_arcs < 0 || bt->max_nodes < 0 || bt->max_arcs < 0)
    return false;
  if (bt->num_nodes >= (int64_t(1) << 31) || bt->num_arcs >= (int64_t(1) << 31)) return false;
  if (bt->num_links > 0 && (!bt->node_ptr || !bt->link || !bt->in_ptr || !bt->out_ptr)) return false;
  if (bt->num_arcs > 0 && (!bt->in_nbr || !bt->in_dst || !bt->in_flag || !bt->out_nbr || !bt->out_arc)) return false;
  return true;
}

s3grl_status wp_walk_check(s3grl_context* ctx, const s3grl_wp_batch* bt, int32_t heads, int32_t walk_len,
                           int64_t lds_budget) {
  if (!ctx || !wp_batch_ok(bt) || heads < 1 || heads > 64 || lds_budget < 0) return S3GRL_ERR_INVALID_ARGUMENT;
  if (walk_len < 1 || walk_len > kWpMaxWalk) {
    set_last_error("walk pool: walk_len must be in [1, 16]");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  if (bt->max_nodes > kWpMaxNodes) {
    set_last_error("walk pool: a subgraph of more than 4096 nodes");
    return S3GRL_ERR_NOT_IMPLEMENTED;
  }
  return S3GRL_OK;
}

// hipFuncSetAttribute once per instantiation and size: the largest dynamic LDS size each kernel has been given
template <typename K>
s3grl_status wp_set_lds(K kernel, unsigned dyn, int device) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, unsigned> granted;   // (kernel, device)
  if (dyn <= (48u << 10)) return S3GRL_OK;
  const void* fn = reinterpret_cast<const void*>(kernel);
  std::lock_guard<std::mutex> lock(mu);
  unsigned& have = granted[std::make_pair(fn, device)];
  if (dyn > have) {
    S3GRL_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    have = dyn;
  }
  return S3GRL_OK;
}

}  // namespace
}  // namespace s3grl

using namespace s3grl;

extern "C" {

s3grl_status s3grl_wp_layout(int64_t n_max, int64_t e_max, int32_t heads, int32_t walk_len, int64_t lds_budget,
                             int64_t* out) {
  if (!out || n_max < 0 || e_max < 0 || heads < 1 || heads > 64 || lds_budget < 0 || walk_len < 1 ||
      walk_len > kWpMaxWalk)
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (n_max > kWpMaxNodes) return S3GRL_ERR_NOT_IMPLEMENTED;
  for (int back = 0; back < 2; ++back) {
    const WpPlan p = wp_plan(n_max, e_max, heads, walk_len, lds_budget, back != 0);
    out[back * 4 + 0] = p.W;
    out[back * 4 + 1] = p.groups;
    out[back * 4 + 2] = p.hbm;
    out[back * 4 + 3] = p.ws_link;
  }
  return S3GRL_OK;
}

s3grl_status s3grl_wp_attention_forward(s3grl_context* ctx, const s3grl_wp_batch* batch, int32_t heads,
                                        int32_t hidden, const float* q, const float* k, float* w, float* weights_p,
                                        float* weights_m, float* omega) {
  if (!ctx || !wp_batch_ok(batch) || heads < 1 || heads > 64 || hidden < 1 || hidden > 4096)
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (batch->num_nodes > 0 && (!q || !k || !omega)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (batch->num_arcs > 0 && (!w || !weights_p || !weights_m)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (batch->num_nodes == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(wp_attn_fwd_kernel, dim3((unsigned)((batch->num_nodes + kWpWaves - 1) / kWpWaves)),
                     dim3(kWpBlock), 0, ctx->stream, *batch, (int)heads, (int)hidden, q, k, w, weights_p, weights_m,
                     omega);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_wp_attention_backward(s3grl_context* ctx, const s3grl_wp_batch* batch, int32_t heads,
                                         int32_t hidden, const float* q, const float* k, const float* w,
                                         const float* weights_p, const float* weights_m, const float* grad_p,
                                         const float* grad_m, const float* grad_omega, float* grad_w, float* grad_q,
                                         float* grad_k) {
  if (!ctx || !wp_batch_ok(batch) || heads < 1 || heads > 64 || hidden < 1 || hidden > 4096)
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (batch->num_nodes > 0 && (!q || !k || !grad_omega || !grad_q || !grad_k)) return S3GRL_ERR_INVALID_ARGUMENT;
  if (batch->num_arcs > 0 && (!w || !weights_p || !weights_m || !grad_p || !grad_m || !grad_w))
    return S3GRL_ERR_INVALID_ARGUMENT;
  if (batch->num_nodes == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const dim3 grid((unsigned)((batch->num_nodes + kWpWaves - 1) / kWpWaves)), block(kWpBlock);
  hipLaunchKernelGGL(wp_attn_dw_kernel, grid, block, 0, ctx->stream, *batch, (int)heads, w, weights_p, weights_m,
                     grad_p, grad_m, grad_omega, grad_w);
  S3GRL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(wp_attn_dqk_kernel, grid, block, 0, ctx->stream, *batch, (int)heads, (int)hidden, q, k, grad_w,
                     grad_q, grad_k);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

#define WP_LAUNCH(KERNEL, ...)                                                                                    \
  do {                                                                                                            \
    if (p.hbm) {                                                                                                  \
      hipLaunchKernelGGL((KERNEL<4, false>), grid, dim3(kWpBlock), 0, ctx->stream, __VA_ARGS__);                  \
    } else {                                                                                                      \
      switch (p.W) {                                                                                              \
        case 4:                                                                                                   \
          if (wp_set_lds(KERNEL<4, true>, dyn, ctx->device)) return S3GRL_ERR_HIP;                                \
          hipLaunchKernelGGL((KERNEL<4, true>), grid, dim3(kWpBlock), dyn, ctx->stream, __VA_ARGS__);             \
          break;                                                                                                  \
        case 8:                                                                                                   \
          if (wp_set_lds(KERNEL<8, true>, dyn, ctx->device)) return S3GRL_ERR_HIP;                                \
          hipLaunchKernelGGL((KERNEL<8, true>), grid, dim3(kWpBlock), dyn, ctx->stream, __VA_ARGS__);             \
          break;                                                                                                  \
        case 16:                                                                                                  \
          if (wp_set_lds(KERNEL<16, true>, dyn, ctx->device)) return S3GRL_ERR_HIP;                               \
          hipLaunchKernelGGL((KERNEL<16, true>), grid, dim3(kWpBlock), dyn, ctx->stream, __VA_ARGS__);            \
          break;                                                                                                  \
        default:                                                                                                  \
          if (wp_set_lds(KERNEL<32, true>, dyn, ctx->device)) return S3GRL_ERR_HIP;                               \
          hipLaunchKernelGGL((KERNEL<32, true>), grid, dim3(kWpBlock), dyn, ctx->stream, __VA_ARGS__);            \
          break;                                                                                                  \
      }                                                                                                           \
    }                                                                                                             \
  } while (0)

s3grl_status s3grl_wp_walk_forward(s3grl_context* ctx, const s3grl_wp_batch* batch, int32_t heads, int32_t walk_len,
                                   int64_t lds_budget, const float* weights_p, const float* weights_m,
                                   void* workspace, int64_t workspace_bytes, float* out) {
  const s3grl_status st = wp_walk_check(ctx, batch, heads, walk_len, lds_budget);
  if (st != S3GRL_OK) return st;
  const int64_t B = batch->num_links;
  if (B == 0) return S3GRL_OK;
  if (!out || !workspace || (batch->num_arcs > 0 && (!weights_p || !weights_m))) return S3GRL_ERR_INVALID_ARGUMENT;
  const WpPlan p = wp_plan(batch->max_nodes, batch->max_arcs, heads, walk_len, lds_budget, false);
  const int n_cap = (int)std::max<int64_t>(batch->max_nodes, 2);
  const int64_t wgs = B * heads * 2 * p.groups;
  const int64_t part_floats = wgs * walk_len;
  const int64_t block_floats = p.hbm ? wgs * 2 * n_cap * p.W : 0;
  if (workspace_bytes < 4 * (part_floats + block_floats) || wgs >= (int64_t(1) << 31)) {
    set_last_error("walk pool forward: the workspace is smaller than links x s3grl_wp_layout's bytes per link");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  float* blocks = static_cast<float*>(workspace);   // 16-byte aligned rows first, the partial traces behind them
  float* part = blocks + block_floats;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  const dim3 grid((unsigned)wgs);
  const unsigned dyn = (unsigned)(2 * (int64_t)n_cap * p.W * 4);
  WP_LAUNCH(wp_walk_fwd_kernel, *batch, (int)heads, (int)walk_len, p.groups, n_cap, weights_p, weights_m, blocks,
            part, out);
  S3GRL_HIP_TRY(hipGetLastError());
  const int64_t count = B * heads * walk_len;
  hipLaunchKernelGGL(wp_trace_kernel, dim3((unsigned)((count + kWpBlock - 1) / kWpBlock)), dim3(kWpBlock), 0,
                     ctx->stream, count, (int)walk_len, p.groups, part, out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status s3grl_wp_walk_backward(s3grl_context* ctx, const s3grl_wp_batch* batch, int32_t heads,
                                    int32_t walk_len, int64_t lds_budget, const float* weights_p,
                                    const float* weights_m, const float* grad_out, void* workspace,
                                    int64_t workspace_bytes, float* grad_p, float* grad_m) {
  const s3grl_status st = wp_walk_check(ctx, batch, heads, walk_len, lds_budget);
  if (st != S3GRL_OK) return st;
  const int64_t B = batch->num_links, E = batch->num_arcs;
  if (B == 0 || E == 0) return S3GRL_OK;
  if (!grad_out || !workspace || !weights_p || !weights_m || !grad_p || !grad_m) return S3GRL_ERR_INVALID_ARGUMENT;
  const WpPlan p = wp_plan(batch->max_nodes, batch->max_arcs, heads, walk_len, lds_budget, true);
  const int n_cap = (int)std::max<int64_t>(batch->max_nodes, 2);
  const int64_t wgs = B * heads * 2 * p.groups;
  const int64_t arc_floats = (int64_t)p.groups * 2 * E * heads;
  const int64_t block_floats = p.hbm ? wgs * p.arrays * n_cap * p.W : 0;
  if (workspace_bytes < 4 * (arc_floats + block_floats) || wgs >= (int64_t(1) << 31)) {
    set_last_error("walk pool backward: the workspace is smaller than links x s3grl_wp_layout's bytes per link");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  float* blocks = static_cast<float*>(workspace);
  float* dpart = blocks + block_floats;
  S3GRL_HIP_TRY(hipSetDevice(ctx->device));
  S3GRL_HIP_TRY(hipMemsetAsync(dpart, 0, (size_t)arc_floats * 4, ctx->stream));
  const dim3 grid((unsigned)wgs);
  const unsigned dyn = (unsigned)(p.arrays * n_cap * p.W * 4);
  WP_LAUNCH(wp_walk_bwd_kernel, *batch, (int)heads, (int)walk_len, p.groups, n_cap, weights_p, weights_m, grad_out,
            blocks, dpart);
  S3GRL_HIP_TRY(hipGetLastError());
  const int64_t count = E * heads;
  hipLaunchKernelGGL(wp_arc_sum_kernel, dim3((unsigned)((count + kWpBlock - 1) / kWpBlock)), dim3(kWpBlock), 0,
                     ctx->stream, count, p.groups, dpart, grad_p, grad_m);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

#undef WP_LAUNCH

}  // extern "C"
