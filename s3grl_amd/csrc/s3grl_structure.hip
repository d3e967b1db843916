// Plan stages of the PoS / PoS Plus path (feature independent), gfx950: everything a plan computes
// before and around its link kernels (s3grl_link_kernels.inl).
//
//   count_kernel     BFS to num_hops from {src,dst} on the unmasked graph -> n, vol(S), R
//   count1_kernel    the same for one-hop plans on big graphs, by intersecting two sorted rows
//   scan_*           multi-block exclusive scan int32 -> int64 offsets
//   classify_kernel  bins links by subgraph size (one launch of a link kernel per LDS class)
//   launch_links     scratch of the classes, then launch_links_k<K> (s3grl_links_k*.hip)
//
// Restates (not translates) reference utils.py:47-85 (k_hop_subgraph) and utils.py:33-44 (neighbors).

#include <cstdlib>

#include "s3grl_internal.hpp"
#include "s3grl_device.hpp"
#include "s3grl_link_classes.hpp"

namespace s3grl {
namespace {

// ---------------------------------------------------------------------------------------
// count: level-synchronous BFS on LDS bitmaps, one thread per frontier word (reference
// utils.py:53-74: `fringe = neighbors(fringe, A) - visited`, early break on an empty fringe).
// Outputs per link: n = |S|, R rows, and p = |P|, the hop-major prefix of S that can carry a
// non-zero entry of r_{K-1}: the only nodes link_kernel keeps propagation state for.
// Frontier list of count_kernel and its threads per link.  Most links are small (PubMed: two thirds
// have under 250 nodes) and pay for the uniform part of the kernel once per wavefront: two waves
// and a 1 024-entry list (12 KB of LDS per link on PubMed, 12 links per CU) measured 1.34 ms
// against 1.70 for four waves and 3 072 entries, 1.60 for one wave; graphs whose bitmaps leave
// room for only a few workgroups per CU get four waves per link.
constexpr int kCountList = 1024;

// EXT: the N-bit bitmaps live in an HBM slice per workgroup (`ext`, `ext_stride` words) instead of
// LDS — graphs of more than kMaxNodesLds nodes; same code, slower memory.  Launched over chunks of the
// link list (`link_base`), so that a bounded number of slices serves any number of links.
template <int G, int kCountBlock, bool EXT = false>
__global__ __launch_bounds__(kCountBlock) void count_kernel(
    const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices, int N, int W,
    const int64_t* __restrict__ links, int hops, int plus, int K, int hubs,
    const WalkSets ws, const int32_t* __restrict__ partner, const int32_t* __restrict__ mirror_of,
    int32_t* __restrict__ n_nodes, int32_t* __restrict__ p_nodes, int32_t* __restrict__ n_rows,
    int32_t* __restrict__ n_jobs, int32_t* __restrict__ lvl_max, int32_t* __restrict__ err_flag,
    unsigned long long* __restrict__ tot_nodes_alg, HopSampling smp, int32_t* __restrict__ stash,
    int slot, int32_t* __restrict__ lvl_stash, const int32_t* __restrict__ cn_indptr,
    const int32_t* __restrict__ cn_indices, int full_p, uint32_t* __restrict__ ext, int64_t ext_stride,
    int link_base, const int32_t* __restrict__ perm) {
  extern __shared__ uint32_t smem[];
  const bool walks = walks_on(ws);
  // `cur` (the frontier as a bitmap, for levels too big for the frontier list) is only needed when
  // a level below `hops` is expanded again: with one hop (and for ScaLed walks) the launcher
  // leaves it out — a third of the LDS of a big graph
  const bool one_hop = hops <= 1 || walks;
  const int nbm = one_hop ? 2 : 3;
  // per-hop sampling: `vis` also holds discovered-but-dropped nodes, so the members of S get a
  // bitmap of their own (the launcher adds W words behind the list when sampling is on)
  const bool sampling = !walks && sampling_on(smp);
  uint32_t *vis, *cur, *nxt, *mem;
  int* sh;
  if constexpr (EXT) {
    uint32_t* bm = ext + (int64_t)blockIdx.x * ext_stride;
    vis = bm;
    cur = one_hop ? nullptr : bm + W;
    nxt = bm + (nbm - 1) * W;
    mem = sampling ? bm + nbm * W : nullptr;
    sh = reinterpret_cast<int*>(smem);
  } else {
    vis = smem;
    cur = one_hop ? nullptr : smem + W;
    nxt = smem + (nbm - 1) * W;
    sh = reinterpret_cast<int*>(smem + nbm * W);
    mem = sampling ? smem + nbm * W + 8 + kHubWords + kCountList : nullptr;
  }
  const int tid = threadIdx.x;
  const int l = perm ? perm[link_base + blockIdx.x] : link_base + blockIdx.x;
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
  int* hub = hubs ? sh + 8 : nullptr;
  int32_t* list = reinterpret_cast<int32_t*>(sh + 8 + kHubWords);   // frontier nodes of the levels < hops
  // The node list found here is left in HBM for link_kernel (hop 1 onwards, `slot` entries per
  // link, level ends in lvl_stash): it then rebuilds its LDS state from the list instead of
  // repeating the BFS.  A list longer than the slot is simply not used (link_kernel walks again).
  int32_t* stash_l = stash ? stash + (int64_t)l * slot : nullptr;
  int32_t* lvl_l = stash ? lvl_stash + (int64_t)l * kMaxLevels : nullptr;
  if (lvl_l && tid == 0) lvl_l[0] = 2;
  for (int t = tid; t < W; t += kCountBlock) {
    vis[t] = 0;
    if (cur) cur[t] = 0;
    nxt[t] = 0;
    if (mem) mem[t] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    atomicOr(&vis[src >> 5], 1u << (src & 31));
    atomicOr(&vis[dst >> 5], 1u << (dst & 31));
    if (mem) {
      atomicOr(&mem[src >> 5], 1u << (src & 31));
      atomicOr(&mem[dst >> 5], 1u << (dst & 31));
    }
    list[0] = src;
    list[1] = dst;
  }
  hub_rows_clear<kCountBlock>(hub);
  __syncthreads();
  // The frontier is a node list (G lanes per node: no serial row walks) as long as the levels
  // below `hops` fit kCountList entries; beyond that it degrades to a bitmap walked one thread
  // per word.  cum_a / cum_b: nodes within K-1 / K hops (P for a row at hop 0 / hop 1).
  int n = 2, cum_a = 2, cum_b = 2, f0 = 0, f1 = 2, biggest = 2, nlev_seen = 1;
  bool use_list = true;
  if (walks) hops = 1;  // ScaLed: the "hop" is what the cached random walks of src and dst visited
  for (int d = 1; d <= hops; ++d) {
    if (walks) {
      for_each_walk_node(ws, src, dst, l, tid, kCountBlock, [&](int u) {
        const uint32_t m = 1u << (u & 31);
        const uint32_t old = atomicOr(&vis[u >> 5], m);
        if (!(old & m)) atomicOr(&nxt[u >> 5], m);
      });
    } else if (use_list) {
      walk_rows<kCountBlock, G, 2>(
          f0, f1, list, indptr, indices, hub,
          [&](RowAcc&, int, int u, bool valid) {
            if (valid) {
              const uint32_t m = 1u << (u & 31);
              const uint32_t old = atomicOr(&vis[u >> 5], m);
              if (!(old & m)) atomicOr(&nxt[u >> 5], m);
            }
          },
          [](RowAcc&, int, int) {});
    } else {
      for (int t = tid; t < W; t += kCountBlock) {
        uint32_t w = cur[t];
        while (w) {
          const int b = __ffs(w) - 1;
          w &= w - 1;
          const int v = t * 32 + b;
          const int e1 = indptr[v + 1];
          for (int e = indptr[v]; e < e1; ++e) {
            const int u = indices[e];
            const uint32_t m = 1u << (u & 31);
            const uint32_t old = atomicOr(&vis[u >> 5], m);
            if (!(old & m)) atomicOr(&nxt[u >> 5], m);
          }
        }
      }
    }
    __syncthreads();
    // every thread owns a contiguous run of bitmap words: one block scan per level
    const int C = (W + kCountBlock - 1) / kCountBlock;
    const int w0 = min(tid * C, W), w1 = min(w0 + C, W);
    int mine = 0;
    for (int t = w0; t < w1; ++t) mine += __popc(nxt[t]);
    int added;
    int pos = f1 + block_excl_scan<kCountBlock>(mine, sh, added);
    if (added == 0) break;
    if (sampling) {  // utils.py:66-70, the same draw link_kernel's BFS makes
      const int keep = hop_keep(smp, added);
      if (keep == 0) break;                     // utils.py:71-72
      if (keep < added) {
        sample_level<kCountBlock>(nxt, W, keep, smp.seed, min(src, dst), max(src, dst), sh);
        mine = 0;
        for (int t = w0; t < w1; ++t) mine += __popc(nxt[t]);
        pos = f1 + block_excl_scan<kCountBlock>(mine, sh, added);
      }
      for (int t = w0; t < w1; ++t) mem[t] |= nxt[t];
    }
    // enumerate the new level in ascending id order: into the LDS frontier list (levels below
    // `hops`, while they fit) and into the HBM stash
    const bool to_list = d < hops && use_list && f1 + added <= kCountList;
    if (to_list || stash_l) {
      int lp = pos;
      int sp = n - 2 + (pos - f1);
      for (int t = w0; t < w1; ++t) {
        uint32_t w = nxt[t];
        while (w) {
          const int b = __ffs(w) - 1;
          w &= w - 1;
          if (to_list) list[lp++] = t * 32 + b;
          if (stash_l && sp < slot) stash_l[sp] = t * 32 + b;
          ++sp;
        }
      }
    }
    if (lvl_l && tid == 0) lvl_l[d] = n + added;
    if (d < hops) {  // the new level is the next frontier
      if (to_list) {
        for (int t = w0; t < w1; ++t) nxt[t] = 0;
        f0 = f1;
        f1 += added;
      } else {
        use_list = false;
        for (int t = w0; t < w1; ++t) {
          cur[t] = nxt[t];
          nxt[t] = 0;
        }
      }
      __syncthreads();
    }
    n += added;
    nlev_seen = d + 1;
    biggest = max(biggest, added);
    if (d <= K - 1) cum_a = n;
    if (d <= K) cum_b = n;
  }
  int R = 2;
  if (sampling) __syncthreads();   // mem is complete
  const uint32_t* member = sampling ? mem : vis;
  if (plus && wave_id() == 0)
    R = 2 + common_neighbours(cn_indptr, cn_indices, [&](int x) { return test_bit(member, x); }, src, dst, nullptr);
  if (tid == 0) {
    if (lvl_l) lvl_l[kMaxLevels - 1] = nlev_seen;   // levels 0 .. nlev_seen-1 are complete
    n_nodes[l] = n;
    // (directed plans keep D^-1/2 — an OUT-degree — and state for every node of S: full_p)
    p_nodes[l] = full_p ? n : (R > 2 ? cum_b : cum_a);
    n_rows[l] = R;
    n_jobs[l] = (R + 1) / 2;
    lvl_max[l] = biggest;
    // algorithmic totals count a folded link as if it had been extracted on its own
    const unsigned long long mult = (mirror_of && mirror_of[l] >= 0) ? 2ull : 1ull;
    atomicAdd(stat_slot(tot_nodes_alg), mult * (unsigned long long)n);
  }
}

// ---------------------------------------------------------------------------------------
// ScaLed subgraphs (reference utils.py:86-150 with sign=True, cache built by create_rw_cache
// utils.py:425-443): M random walks of length m from every node, cached per NODE; the subgraph of
// a link is {src,dst} plus everything the walks of src and of dst visited.  torch_cluster's
// uniform walk is restated with a counter-based generator keyed by (seed, node, walk, step), so a
// node's walks are the same in every link and every kernel that re-derives the subgraph.
__device__ __forceinline__ uint32_t rw_random(uint32_t seed, uint32_t node, uint32_t walk,
                                              uint32_t step) {
  uint64_t x = ((uint64_t)seed << 32) ^ ((uint64_t)node * 0x9E3779B97F4A7C15ull) ^
               ((uint64_t)walk << 20) ^ step;
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return (uint32_t)(x >> 16);
}

__global__ void random_walks_kernel(const int32_t* __restrict__ indptr,
                                    const int32_t* __restrict__ indices, int64_t N, int m, int M,
                                    uint32_t seed, int32_t* __restrict__ raw /* [N, M*m] */) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * M) return;
  const int64_t v = i / M;
  const int w = (int)(i - v * M);
  int cur = (int)v;
  for (int s = 0; s < m; ++s) {
    const int b = indptr[cur], deg = indptr[cur + 1] - b;
    if (deg > 0) cur = indices[b + rw_random(seed, (uint32_t)v, (uint32_t)w, (uint32_t)s) % deg];
    raw[(v * M + w) * m + s] = cur;   // an isolated node stays where it is
  }
}

// The cache reference utils.create_rw_cache builds (utils.py:425-443): for every start node the
// sorted unique nodes of its M walks of length m, the start itself included (torch_cluster's walk
// tensor begins with the start; torch.unique sorts).  Same walks as random_walks_kernel for the
// same (seed, node): a plan built on these sets equals the plan that draws the walks itself.
// One workgroup per start node: walks into LDS, bitonic sort, unique -> padded scratch + count.
constexpr int kWalkSetBlock = 256;
constexpr int kWalkSetMax = 8192;   // M * m + 1 rounded up to a power of two: 32 KiB of LDS

__global__ __launch_bounds__(kWalkSetBlock) void walk_sets_kernel(
    const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t N,
    const int64_t* __restrict__ starts, int m, int M, uint32_t seed, int P, int cap,
    int32_t* __restrict__ scratch /* [num_starts, cap] */, int32_t* __restrict__ count,
    int32_t* __restrict__ err_flag) {
  extern __shared__ uint32_t smem[];
  int32_t* e = reinterpret_cast<int32_t*>(smem);   // [P]
  __shared__ int sh[kWalkSetBlock / 64];
  const int tid = threadIdx.x;
  const int64_t i = blockIdx.x;
  const int64_t v64 = starts[i];
  if (v64 < 0 || v64 >= N) {
    if (tid == 0) {
      atomicMax(err_flag, 1);
      count[i] = 0;
    }
    return;
  }
  const int v = (int)v64;
  for (int t = tid; t < P; t += kWalkSetBlock) e[t] = t == 0 ? v : 0x7fffffff;
  __syncthreads();
  for (int w = tid; w < M; w += kWalkSetBlock) {
    int cur = v;
    for (int st = 0; st < m; ++st) {
      const int b = indptr[cur], deg = indptr[cur + 1] - b;
      if (deg > 0) cur = indices[b + rw_random(seed, (uint32_t)v, (uint32_t)w, (uint32_t)st) % deg];
      e[1 + w * m + st] = cur;
    }
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P; t += kWalkSetBlock) {
        const int u = t ^ j;
        if (u > t) {
          const int a = e[t], b = e[u];
          if ((a > b) == ((t & k) == 0)) {
            e[t] = b;
            e[u] = a;
          }
        }
      }
      __syncthreads();
    }
  // unique: thread-contiguous runs, one block scan
  const int C = (P + kWalkSetBlock - 1) / kWalkSetBlock;
  const int t0 = min(tid * C, P), t1 = min(t0 + C, P);
  int mine = 0;
  for (int t = t0; t < t1; ++t) mine += (e[t] != 0x7fffffff && (t == 0 || e[t] != e[t - 1])) ? 1 : 0;
  int total;
  int pos = block_excl_scan<kWalkSetBlock>(mine, sh, total);
  for (int t = t0; t < t1; ++t)
    if (e[t] != 0x7fffffff && (t == 0 || e[t] != e[t - 1])) scratch[i * cap + pos++] = e[t];
  if (tid == 0) count[i] = total;
}

__global__ void walk_sets_compact_kernel(const int32_t* __restrict__ scratch, int cap,
                                         const int64_t* __restrict__ set_ptr, int32_t* __restrict__ set_nodes) {
  const int64_t i = blockIdx.x;
  const int64_t o = set_ptr[i];
  const int n = (int)(set_ptr[i + 1] - o);
  for (int t = threadIdx.x; t < n; t += blockDim.x) set_nodes[o + t] = scratch[i * cap + t];
}

__global__ void validate_sets_kernel(const int64_t* __restrict__ set_ptr, const int32_t* __restrict__ set_nodes,
                                     int64_t num_sets, int64_t total, int64_t N, int64_t* __restrict__ flags) {
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < num_sets;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = set_ptr[i], e = set_ptr[i + 1];
    if (b > e || b < 0 || e > total || (i == 0 && b != 0) || (i == num_sets - 1 && e != total)) {
      bad |= 1;
      continue;
    }
    for (int64_t c = b; c < e; ++c) {
      const int u = set_nodes[c];
      if (u < 0 || u >= N) bad |= 2;
    }
  }
  if (bad) atomicOr(reinterpret_cast<unsigned long long*>(flags), (unsigned long long)bad);
}

// ---- split jobs (Job::split, kSplitThreshold) ---------------------------------------------------
// pieces per job: ceil(support / 2^seg_shift) for a split job, none otherwise
__global__ void split_count_kernel(const Job* __restrict__ jobs, int64_t njobs, int seg_shift,
                                   int32_t* __restrict__ cnt) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= njobs) return;
  const Job job = jobs[j];
  cnt[j] = job.split ? (job.support + (1 << seg_shift) - 1) >> seg_shift : 0;
}

// piece s of job j as a gather unit of its own: list entries [s·SEG, min((s+1)·SEG, support)), its
// coefficient block (laid out by the link kernel), operator reach clamped to the piece, and two
// rows of the partial-row scratch as output.  No mirror, no label column: combine_kernel does those.
// The pieces sit behind the plan's jobs in ONE array of gather units (gjobs[njobs + q]); the launch
// order starts with the pieces (they belong to the longest lists of the plan) and goes on with the
// plan's own largest-first order.
__global__ void split_fill_kernel(const Job* __restrict__ jobs, const int32_t* __restrict__ job_lim,
                                  const int32_t* __restrict__ job_order, int64_t njobs, int K, int seg_shift,
                                  const int64_t* __restrict__ piece_off, int64_t npieces, Job* __restrict__ gjobs,
                                  int32_t* __restrict__ g_lim, int32_t* __restrict__ g_order,
                                  int32_t* __restrict__ piece_job) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= njobs) return;
  const Job job = jobs[j];
  gjobs[j] = job;
  for (int i = 0; i < K; ++i) g_lim[j * K + i] = job_lim[j * K + i];
  g_order[npieces + j] = job_order[j];
  const int64_t p0 = piece_off[j], p1 = piece_off[j + 1];
  for (int64_t q = p0; q < p1; ++q) {
    const int s0 = (int)(q - p0) << seg_shift;
    const int len = min(1 << seg_shift, job.support - s0);
    Job g = job;
    g.coef_off = job.coef_off + piece_coef_off(s0, K);
    g.ids_off = job.ids_off + s0;
    g.out_row = 2 * q;
    g.support = len;
    g.mirror_row = -1;
    g.mirror_swap = 0;
    g.split = 2;
    gjobs[njobs + q] = g;
    for (int i = 0; i < K; ++i) g_lim[(njobs + q) * K + i] = min(max(job_lim[j * K + i] - s0, 0), len);
    g_order[q] = (int32_t)(njobs + q);
    piece_job[q] = (int32_t)j;
  }
}

// Rows of a split job: operator i+1 = Σ over its pieces (ascending, in f64) of the pieces' partial
// rows; operator 0 = [z | X[node]]; label column from job_z; the folded reversed link gets the same
// rows swapped.  Launched over the pieces: the workgroup of a job's FIRST piece does the job's row.
__global__ __launch_bounds__(256) void combine_kernel(
    const Job* __restrict__ jobs, const int64_t* __restrict__ piece_off, const int32_t* __restrict__ piece_job,
    const float* __restrict__ job_z, int K, const float* __restrict__ prows, const float* __restrict__ X,
    int64_t ldx, int F, float* __restrict__ rows) {
  const int64_t j = piece_job[blockIdx.x];
  const int r = blockIdx.y;
  const int64_t p0 = piece_off[j], p1 = piece_off[j + 1];
  if (p0 != (int64_t)blockIdx.x) return;
  const Job job = jobs[j];
  if (r == 1 && job.node_b < 0) return;
  const int Fp = F + 1;
  const int64_t rstride = (int64_t)(K + 1) * Fp;
  const int node = r == 0 ? job.node_a : job.node_b;
  float* __restrict__ out = rows + (job.out_row + r) * rstride;
  float* __restrict__ mir = job.mirror_row >= 0
                                ? rows + (job.mirror_row + (job.mirror_swap ? 1 - r : r)) * rstride : nullptr;
  for (int e = threadIdx.x; e < (K + 1) * Fp; e += blockDim.x) {
    const int i = e / Fp, c = e - i * Fp;
    float v;
    if (c == 0) {
      v = i == 0 ? (float)(r == 0 ? job.z_a : job.z_b) : job_z[(j * K + (i - 1)) * 2 + r];
    } else if (i == 0) {
      v = X[(int64_t)node * ldx + (c - 1)];
    } else {
      double acc = 0.0;
      for (int64_t q = p0; q < p1; ++q) acc += (double)prows[(2 * q + r) * rstride + e];
      v = (float)acc;
    }
    out[e] = v;
    if (mir) mir[e] = v;
  }
}

// ---------------------------------------------------------------------------------------
// Reversed duplicates.  The reference's train split holds BOTH directions of every train edge
// (PyG to_undirected, consumed at utils.py:628), and the link (d,s) has exactly the subgraph,
// the masked operator and the rows of (s,d) with src/dst swapped.  One open-addressing table
// over the links with src < dst, one lookup per link with src > dst; at most one fold per link.
constexpr uint64_t kEmptyKey = ~0ull;

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

__global__ void mirror_insert_kernel(const int64_t* __restrict__ links, int64_t L, int64_t N,
                                     uint64_t* __restrict__ keys, int32_t* __restrict__ vals,
                                     uint64_t mask) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const int64_t s = links[2 * l], d = links[2 * l + 1];
  if (s < 0 || d < 0 || s >= N || d >= N || s >= d) return;
  const uint64_t key = ((uint64_t)s << 32) | (uint64_t)d;
  uint64_t slot = mix64(key) & mask;
  for (;;) {
    const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(&keys[slot]), kEmptyKey, key);
    if (old == kEmptyKey || old == key) {
      atomicMin(&vals[slot], (int32_t)l);  // the lowest link index owns the key: deterministic
      return;
    }
    slot = (slot + 1) & mask;  // the table has >= 2L slots: a free one exists
  }
}

__global__ void mirror_lookup_kernel(const int64_t* __restrict__ links, int64_t L, int64_t N,
                                     const uint64_t* __restrict__ keys,
                                     const int32_t* __restrict__ vals, uint64_t mask,
                                     int32_t* __restrict__ partner, int32_t* __restrict__ mirror_of,
                                     unsigned long long* __restrict__ n_mirrored) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const int64_t s = links[2 * l], d = links[2 * l + 1];
  if (s < 0 || d < 0 || s >= N || d >= N || s <= d) return;
  const uint64_t key = ((uint64_t)d << 32) | (uint64_t)s;
  uint64_t slot = mix64(key) & mask;
  for (;;) {
    const uint64_t k = keys[slot];
    if (k == kEmptyKey) return;
    if (k == key) {
      const int32_t P = vals[slot];
      if (atomicCAS(&mirror_of[P], -1, (int32_t)l) == -1) {
        partner[l] = P;
        atomicAdd(n_mirrored, 1ull);
      }
      return;
    }
    slot = (slot + 1) & mask;
  }
}

__global__ void mirror_rows_kernel(const int32_t* __restrict__ partner, int64_t L,
                                   int32_t* __restrict__ n_rows) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const int32_t P = partner[l];
  if (P >= 0) n_rows[l] = n_rows[P];
}

// ---------------------------------------------------------------------------------------
// exclusive scan int32[n] -> int64[n+1], three small launches (tile = 1024 elements)
constexpr int kScanTile = 1024;

__global__ __launch_bounds__(256) void scan_partials_kernel(const int32_t* __restrict__ in,
                                                            int64_t n, int64_t* __restrict__ part) {
  __shared__ int sh[4];
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  int s = 0;
  for (int k = threadIdx.x; k < kScanTile; k += 256)
    if (base + k < n) s += in[base + k];
  s = block_sum<256>(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(1024) void scan_top_kernel(int64_t* __restrict__ part, int64_t nb,
                                                        int64_t* __restrict__ total_out) {
  __shared__ int64_t sh[1024];
  const int tid = threadIdx.x;
  const int64_t chunk = (nb + 1023) / 1024;
  const int64_t b = tid * chunk, e = min(nb, b + chunk);
  int64_t s = 0;
  for (int64_t i = b; i < e; ++i) s += part[i];
  sh[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int64_t t = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += t;
    __syncthreads();
  }
  int64_t run = tid ? sh[tid - 1] : 0;
  for (int64_t i = b; i < e; ++i) {
    const int64_t v = part[i];
    part[i] = run;
    run += v;
  }
  if (tid == 1023) *total_out = sh[1023];
}

__global__ __launch_bounds__(256) void scan_apply_kernel(const int32_t* __restrict__ in, int64_t n,
                                                         const int64_t* __restrict__ part,
                                                         int64_t* __restrict__ out) {
  __shared__ int sh[4];
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  const int64_t i0 = base + threadIdx.x * 4;
  int v[4], s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = i0 + k < n ? in[i0 + k] : 0;
    s += v[k];
  }
  int total;
  int64_t run = part[blockIdx.x] + block_excl_scan<256>(s, sh, total);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < n) out[i0 + k] = run;
    run += v[k];
  }
}

// The three offset arrays of a plan (nodes, rows, row pairs per link) in ONE set of launches
// (blockIdx.y picks the array) instead of three, with their maxima and totals written next to the
// plan's other scalars: a plan is a few dozen small launches, and on a sharded list their fixed cost
// is paid once per piece (0.5 ms per plan before this).
struct Scan3 {
  const int32_t* in[3];
  int64_t* out[3];
  int64_t* part[3];
  long long* max_out[3];   // may be null
  int64_t* total_out[3];   // may be null
};

__global__ __launch_bounds__(256) void scan3_partials_kernel(Scan3 a, int64_t n) {
  __shared__ int sh[4];
  const int y = blockIdx.y;
  const int32_t* __restrict__ in = a.in[y];
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  int s = 0, m = 0;
  for (int k = threadIdx.x; k < kScanTile; k += 256)
    if (base + k < n) {
      const int v = in[base + k];
      s += v;
      m = max(m, v);
    }
  s = block_sum<256>(s, sh);
  if (threadIdx.x == 0) a.part[y][blockIdx.x] = s;
  if (a.max_out[y]) {
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(a.max_out[y], (long long)m);
  }
}

__global__ __launch_bounds__(1024) void scan3_top_kernel(Scan3 a, int64_t nb, int64_t n) {
  __shared__ int64_t sh[1024];
  const int y = blockIdx.x;
  int64_t* __restrict__ part = a.part[y];
  const int tid = threadIdx.x;
  const int64_t chunk = (nb + 1023) / 1024;
  const int64_t b = tid * chunk, e = min(nb, b + chunk);
  int64_t s = 0;
  for (int64_t i = b; i < e; ++i) s += part[i];
  sh[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int64_t t = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += t;
    __syncthreads();
  }
  int64_t run = tid ? sh[tid - 1] : 0;
  for (int64_t i = b; i < e; ++i) {
    const int64_t v = part[i];
    part[i] = run;
    run += v;
  }
  if (tid == 1023) {
    a.out[y][n] = sh[1023];
    if (a.total_out[y]) *a.total_out[y] = sh[1023];
  }
}

__global__ __launch_bounds__(256) void scan3_apply_kernel(Scan3 a, int64_t n) {
  __shared__ int sh[4];
  const int y = blockIdx.y;
  const int32_t* __restrict__ in = a.in[y];
  int64_t* __restrict__ out = a.out[y];
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  const int64_t i0 = base + threadIdx.x * 4;
  int v[4], s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = i0 + k < n ? in[i0 + k] : 0;
    s += v[k];
  }
  int total;
  int64_t run = a.part[y][blockIdx.x] + block_excl_scan<256>(s, sh, total);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < n) out[i0 + k] = run;
    run += v[k];
  }
}

// ---------------------------------------------------------------------------------------
// One-hop plans on big graphs (link_full_kernel in s3grl_link_kernels.inl): the degree-oriented rows
// that kernel walks, and count1_kernel, which sizes a one-hop subgraph without bitmaps.

// ---- degree-oriented rows ------------------------------------------------------------------
// fwd(u) = { v in N(u) : (deg v, v) > (deg u, u) } ∪ ({u} if u has a self-loop), ascending id.
// Every undirected edge sits in exactly one oriented row; the longest oriented row of a graph
// with m edges has at most sqrt(2m) entries.
__device__ __forceinline__ bool fwd_keep(int du, int u, int dv, int v) {
  return v == u || dv > du || (dv == du && v > u);
}

__global__ void fwd_count_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                 int64_t N, int32_t* __restrict__ cnt) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= N) return;
  const int b = indptr[u], e = indptr[u + 1], du = e - b;
  int c = 0;
  for (int k = b; k < e; ++k) {
    const int v = indices[k];
    c += fwd_keep(du, (int)u, indptr[v + 1] - indptr[v], v) ? 1 : 0;
  }
  cnt[u] = c;
}

__global__ void fwd_fill_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                int64_t N, const int64_t* __restrict__ off64, int32_t* __restrict__ fwd_indptr,
                                int32_t* __restrict__ fwd_indices, uint16_t* __restrict__ fwd_deg) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u > N) return;
  fwd_indptr[u] = (int32_t)off64[u];
  if (u == N) return;
  // 16-bit copy of the oriented degree for the sizing pass (an oriented row has at most sqrt(2m)
  // entries; saturated beyond 65535, which only loosens a bound)
  fwd_deg[u] = (uint16_t)min((long long)(off64[u + 1] - off64[u]), 65535ll);
  const int b = indptr[u], e = indptr[u + 1], du = e - b;
  int o = (int)off64[u];
  for (int k = b; k < e; ++k) {
    const int v = indices[k];
    if (fwd_keep(du, (int)u, indptr[v + 1] - indptr[v], v)) fwd_indices[o++] = v;
  }
}

constexpr int kCount1Waves = 4;

__global__ __launch_bounds__(64 * kCount1Waves) void count1_kernel(
    const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const uint16_t* __restrict__ fwd_deg, int N, const int64_t* __restrict__ links, int64_t L, int plus,
    int K, const int32_t* __restrict__ partner, const int32_t* __restrict__ mirror_of,
    int32_t* __restrict__ n_nodes, int32_t* __restrict__ p_nodes, int32_t* __restrict__ n_rows,
    int32_t* __restrict__ n_jobs, int32_t* __restrict__ lvl_max, int32_t* __restrict__ e_cap,
    int32_t* __restrict__ err_flag, unsigned long long* __restrict__ tot_nodes_alg,
    unsigned long long* __restrict__ tot_oriented, const int32_t* __restrict__ perm, const HubCache hub,
    int64_t* __restrict__ x_cap) {
  const int lane = threadIdx.x & 63;
  const int64_t li = (int64_t)blockIdx.x * kCount1Waves + (threadIdx.x >> 6);
  if (li >= L) return;
  const int64_t l = perm ? perm[li] : li;   // processing order (launch_link_order)
  const int64_t s64 = links[2 * l], d64 = links[2 * l + 1];
  const bool bad = s64 < 0 || s64 >= N || d64 < 0 || d64 >= N || s64 == d64;
  if (bad || (partner && partner[l] >= 0)) {   // invalid link, or a reversed duplicate (its primary works)
    if (lane == 0) {
      if (bad) atomicMax(err_flag, s64 == d64 ? 2 : 1);
      n_nodes[l] = 0;
      p_nodes[l] = 0;
      n_rows[l] = 0;
      n_jobs[l] = 0;
      lvl_max[l] = 0;
      e_cap[l] = 0;
      if (x_cap) x_cap[l] = -1;
    }
    return;
  }
  const int s = (int)s64, d = (int)d64;
  const int cs = indptr[s + 1] - indptr[s], cd = indptr[d + 1] - indptr[d];
  // the SHORTER row is searched in the longer one (a leaf against a hub: one chunk of searches
  // instead of forty); the longer row is only swept for its oriented degrees
  const bool s_short = cs <= cd;
  const int32_t* __restrict__ ra = indices + indptr[s_short ? s : d];   // shorter
  const int32_t* __restrict__ rb = indices + indptr[s_short ? d : s];   // longer
  const int ca = s_short ? cs : cd, cb = s_short ? cd : cs;
  const int a_own = s_short ? s : d, b_own = s_short ? d : s;
  // src / dst themselves inside a row are not members; a node in its own row is a self-loop
  int members = 0, common = 0, loops = 0;
  long long fsum = lane == 0 ? (long long)fwd_deg[s] + fwd_deg[d] : 0ll;
  for (int c0 = 0; c0 < ca; c0 += 64) {
    const int c = c0 + lane;
    if (c < ca) {
      const int x = ra[c];
      loops += x == a_own ? 1 : 0;
      if (x != s && x != d) {
        const int lb = row_lower_bound(rb, cb, x);
        const bool dup = lb < cb && rb[lb] == x;
        members += 1;
        common += dup ? 1 : 0;
        if (!dup) fsum += fwd_deg[x];            // common ones are counted from the longer row
      }
    }
  }
  for (int c0 = 0; c0 < cb; c0 += 64) {
    const int c = c0 + lane;
    if (c < cb) {
      const int y = rb[c];
      loops += y == b_own ? 1 : 0;
      if (y != s && y != d) {
        members += 1;
        fsum += fwd_deg[y];
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    members += __shfl_xor(members, o);
    common += __shfl_xor(common, o);
    loops += __shfl_xor(loops, o);
    fsum += __shfl_xor(fsum, o);
  }
  if (lane == 0) {
    const int n = 2 + members - common;
    // PoS Plus rows (common_neighbours above: N'(0) ∩ N'(1) on the masked sub-CSR): the common
    // neighbours, plus src / dst themselves when they carry a self-loop
    const int R = plus ? 2 + common + loops : 2;
    const int cum_a = K >= 2 ? n : 2, cum_b = n;
    n_nodes[l] = n;
    p_nodes[l] = R > 2 ? cum_b : cum_a;
    n_rows[l] = R;
    n_jobs[l] = (R + 1) / 2;
    lvl_max[l] = max(2, n - 2);
    e_cap[l] = (int)min(2ll * fsum, (long long)0x3fffffff);
    if (x_cap) {
      // Can link_hub_kernel (s3grl_hub.hip) take this link?  Decided from the graph and the link alone.
      // hub = the endpoint of higher degree (then lower id); the edges outside its cached neighbourhood
      // are at most Σ degree over N(other) ∪ {other}, and at most the oriented entries of S less the
      // hub's star and the cached edges (every induced edge sits in one oriented row of S).
      long long xc = -1;
      const bool s_hub = cs > cd || (cs == cd && s < d);
      const int hb = s_hub ? s : d, ot = s_hub ? d : s;
      const int hk = hub.slot[hb];
      if (hk >= 0 && n <= 65535) {
        const long long c_h = s_hub ? cs : cd, c_o = s_hub ? cd : cs;
        const long long vb = (long long)hub.voln[ot] + c_o;
        const long long eh = hub.col_base[hk + 1] - hub.col_base[hk];
        const long long xb = min(vb, max(fsum - c_h - eh / 2, 0ll));
        if (vb <= kHubVolMax) xc = (hub_stage_bytes(c_h, eh) << 32) | xb;   // (staged bytes of the cache, bound)
      }
      x_cap[l] = xc;
    }
    const unsigned long long mult = (mirror_of && mirror_of[l] >= 0) ? 2ull : 1ull;
    atomicAdd(stat_slot(tot_nodes_alg), mult * (unsigned long long)n);
    // oriented-row entries link_full_kernel will probe for this link (measurement: bench.py's
    // physical-bytes figure of the one-hop path)
    atomicAdd(stat_slot(tot_oriented), (unsigned long long)fsum);
  }
}


__global__ void classify_kernel(const int32_t* __restrict__ n_nodes,
                                const int32_t* __restrict__ p_nodes,
                                const int32_t* __restrict__ lvl_max, int64_t L, ClassBounds bound,
                                int sparse_mode, ClassBounds sbound, const int32_t* __restrict__ e_cap,
                                ClassBounds fbound, int bm_limit, int dm_max_n, int dm_class_mask,
                                int32_t* __restrict__ class_count, int32_t* __restrict__ class_list,
                                const int32_t* __restrict__ perm, const int64_t* __restrict__ x_cap,
                                ClassBounds hbound, const int32_t* __restrict__ csr_e, CsrBounds cbound, int W,
                                int tiny_max_n) {
  const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // (perm: the class lists come out in the plan's processing order, up to the order of the atomics)
  const int64_t l = li < L ? (perm ? (int64_t)perm[li] : li) : L;
  const int n = l < L ? n_nodes[l] : 0;
  const int p = l < L ? p_nodes[l] : 0;
  int need = link_lds_need(n, p);
  int c = 0;
  bool sparse = false;
  // one-hop plan (e_cap is only produced for those), every operator reaches all of S, local ids fit
  // 16 bits: link_full_kernel, by its LDS need with or without the bit matrix on chip
  // every operator reaches all of S and the sizing kernel of the induced-CSR flavour counted the link's
  // entries (s3grl_csr.hip): link_csr_kernel, by its exact LDS need
  if (csr_e && n > 0 && p == n && csr_e[l] >= 0) {
    const int need_c = csr_lds_need(n, csr_e[l], W);
    if (need_c <= cbound.b[kCsrClasses - 1]) {
      sparse = true;
#pragma unroll
      for (int k = 0; k < kCsrClasses; ++k) c += need_c > cbound.b[k] ? 1 : 0;
      c += kCsrBase;
    }
  }
  if (!sparse && x_cap && n > 0 && p == n && x_cap[l] >= 0) {
    const int64_t stage = x_cap[l] >> 32, xb = x_cap[l] & 0xffffffffll;
    const int64_t need_h = hub_lds_need(n, xb) + stage;
    if (!hbound.b[kHubClasses] && need_h <= hbound.b[kHubClasses - 1]) {   // (b[kHubClasses]: test hook)
      sparse = true;
#pragma unroll
      for (int k = 0; k < kHubClasses; ++k) c += need_h > hbound.b[k] ? 1 : 0;
      c += kHubBase;
    } else if (hub_lds_need(n, 0) + stage <= hbound.b[kHubClasses - 1]) {
      sparse = true;
      c = kHubBase + kHubClasses;
      atomicMax(&class_count[29], (int)xb);   // sizes the HBM slices of that class
    }
  }
  if (!sparse && e_cap && n > 0 && p == n && n <= tiny_max_n) {   // (tiny_max_n = 0: plans with common-neighbour rows)
    sparse = true;
    c = kTinyList + (n > 32 ? 1 : 0);
  }
  if (!sparse && e_cap && n > 0 && p == n && n <= 65535) {
    const int ec = e_cap[l];
    const int need_a = full_lds_need(n, ec, true), need_b = full_lds_need(n, ec, false);
    if (need_a <= min(fbound.b[kNumClasses - 1], bm_limit)) {
      sparse = true;
#pragma unroll
      for (int k = 0; k < kNumClasses; ++k) c += need_a > fbound.b[k] ? 1 : 0;
      c += kFullBase;
    } else if (need_b <= fbound.b[kNumClasses - 1]) {
      sparse = true;
      c = kFullBig;
      atomicMax(&class_count[31], ec);   // sizes the HBM slices of that class
      atomicMax(&class_count[30], need_b);   // and its LDS
    }
  }
  if (!sparse && sparse_mode == 2 && n > 0 && n <= dm_max_n && need <= sbound.b[kNumClasses - 1]) {
    // direct-map flavour: sbound = what the map leaves of the LDS; the list must be in the stash;
    // class by class where the host found the map to pay (dm_class_mask)
    int k_dm = 0;
#pragma unroll
    for (int k = 0; k < kNumClasses; ++k) k_dm += need > sbound.b[k] ? 1 : 0;
    if ((dm_class_mask >> k_dm) & 1) {
      sparse = true;
      c = k_dm + kSparseBase;
    }
  }
  if (!sparse && sparse_mode == 1 && n > 0 && lvl_max[l] <= kSparseLevelMax) {
    const int sneed = link_lds_need_sparse(n, p);
    if (sneed <= sbound.b[kNumClasses - 1]) {
      sparse = true;
#pragma unroll
      for (int k = 0; k < kNumClasses; ++k) c += sneed > sbound.b[k] ? 1 : 0;
      c += kSparseBase;
    }
  }
  if (!sparse) {
#pragma unroll
    for (int k = 0; k < kNumClasses; ++k) c += need > bound.b[k] ? 1 : 0;
  }
  if (n == 0) c = -1;
  // one atomic per (wave, class) instead of one per link
  // (only the classes present in the wavefront are visited: two or three of kNumLists)
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(c >= 0);
  while (todo) {
    const int k = __shfl(c, __ffsll((long long)todo) - 1);
    const unsigned long long m = __ballot(c == k);
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&class_count[k], __popcll(m));
    base = __shfl(base, leader);
    if (c == k) class_list[(int64_t)k * L + base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)l;
    todo &= ~m;
  }
  // class kNumClasses = links that do not fit LDS: they run with their lists in HBM scratch
  if (c == kNumClasses) atomicMax(&class_count[kNumClasses + 1], need);
}

// hop distance of every exported node from the per-link level ends
__global__ void dists_kernel(const int64_t* __restrict__ node_off, const int32_t* __restrict__ lvl,
                             int64_t L, int8_t* __restrict__ dists) {
  const int64_t l = blockIdx.x;
  const int64_t o = node_off[l];
  const int n = (int)(node_off[l + 1] - o);
  const int32_t* lv = lvl + l * kMaxLevels;
  for (int t = threadIdx.x; t < n; t += blockDim.x) {
    int d = 0;
    while (d < kMaxLevels - 1 && t >= lv[d]) ++d;
    dists[o + t] = (int8_t)d;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------
int64_t mirror_table_slots(int64_t L) {
  int64_t s = 1024;
  while (s < 2 * L) s <<= 1;
  return s;
}

s3grl_status launch_find_mirrors(s3grl_context* ctx, const int64_t* links, int64_t L, int64_t N,
                                 uint64_t* keys, int32_t* vals, int64_t slots, int32_t* partner,
                                 int32_t* mirror_of, int64_t* n_mirrored) {
  if (L == 0) return S3GRL_OK;
  S3GRL_HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)slots * 8, ctx->stream));
  S3GRL_HIP_TRY(hipMemsetAsync(vals, 0x7f, (size_t)slots * 4, ctx->stream));
  S3GRL_HIP_TRY(hipMemsetAsync(partner, 0xff, (size_t)L * 4, ctx->stream));
  S3GRL_HIP_TRY(hipMemsetAsync(mirror_of, 0xff, (size_t)L * 4, ctx->stream));
  const unsigned grid = (unsigned)((L + 255) / 256);
  hipLaunchKernelGGL(mirror_insert_kernel, dim3(grid), dim3(256), 0, ctx->stream, links, L, N, keys,
                     vals, (uint64_t)(slots - 1));
  hipLaunchKernelGGL(mirror_lookup_kernel, dim3(grid), dim3(256), 0, ctx->stream, links, L, N, keys,
                     vals, (uint64_t)(slots - 1), partner, mirror_of,
                     reinterpret_cast<unsigned long long*>(n_mirrored));
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_random_walks(s3grl_context* ctx, const s3grl_graph* g, int m, int M,
                                 uint32_t seed, int32_t* raw) {
  const int64_t total = g->num_nodes * M;
  // (a directed graph is walked along its arcs, like torch_cluster walks the directed edge_index)
  hipLaunchKernelGGL(random_walks_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     ctx->stream, g->directed ? g->out_indptr : g->indptr, g->directed ? g->out_indices : g->indices,
                     g->num_nodes, m, M, seed, raw);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_validate_sets(s3grl_context* ctx, const int64_t* set_ptr, const int32_t* set_nodes,
                                  int64_t num_sets, int64_t total, int64_t num_nodes, int64_t* flags) {
  if (num_sets == 0) return S3GRL_OK;
  hipLaunchKernelGGL(validate_sets_kernel, dim3(512), dim3(256), 0, ctx->stream, set_ptr, set_nodes, num_sets,
                     total, num_nodes, flags);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_walk_sets(s3grl_context* ctx, const s3grl_graph* g, const int64_t* starts, int64_t num_starts,
                              int m, int M, uint32_t seed, int64_t* set_ptr, int32_t* set_nodes) {
  if (num_starts == 0) {
    S3GRL_HIP_TRY(hipMemsetAsync(set_ptr, 0, 8, ctx->stream));
    return S3GRL_OK;
  }
  const int64_t cap64 = (int64_t)m * M + 1;
  int P = 2;
  while (P < cap64 && P < kWalkSetMax) P <<= 1;
  if (cap64 > P) {
    set_last_error("rw_m * rw_M + 1 = " + std::to_string(cap64) + " entries per node exceed " +
                   std::to_string(kWalkSetMax));
    return S3GRL_ERR_GRAPH_TOO_LARGE;
  }
  const int cap = (int)cap64;
  Transient tmp{ctx, {}};
  void *scratch = nullptr, *cnt = nullptr, *ws = nullptr;
  S3GRL_TRY(ctx->arena.alloc((size_t)num_starts * cap * 4, &scratch));
  tmp.ptrs.push_back(scratch);
  S3GRL_TRY(ctx->arena.alloc((size_t)num_starts * 4, &cnt));
  tmp.ptrs.push_back(cnt);
  S3GRL_TRY(ctx->arena.alloc((size_t)scan_workspace_elems(num_starts) * 8, &ws));
  tmp.ptrs.push_back(ws);
  S3GRL_HIP_TRY(hipMemsetAsync(ctx->d_scalars, 0, 8, ctx->stream));
  hipLaunchKernelGGL(walk_sets_kernel, dim3((unsigned)num_starts), dim3(kWalkSetBlock), (size_t)P * 4, ctx->stream,
                     g->directed ? g->out_indptr : g->indptr, g->directed ? g->out_indices : g->indices,
                     g->num_nodes, starts, m, M, seed, P, cap, static_cast<int32_t*>(scratch),
                     static_cast<int32_t*>(cnt), reinterpret_cast<int32_t*>(ctx->d_scalars));
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(launch_scan_i32_to_i64(ctx, static_cast<int32_t*>(cnt), num_starts, set_ptr,
                                   static_cast<int64_t*>(ws)));
  hipLaunchKernelGGL(walk_sets_compact_kernel, dim3((unsigned)num_starts), dim3(64), 0, ctx->stream,
                     static_cast<int32_t*>(scratch), cap, set_ptr, set_nodes);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_HIP_TRY(hipMemcpyAsync(ctx->h_scalars, ctx->d_scalars, 8, hipMemcpyDeviceToHost, ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));   // tmp is released on return
  if (ctx->h_scalars[0] & 0xffffffff) {
    set_last_error("a start node is outside [0, num_nodes)");
    return S3GRL_ERR_INVALID_ARGUMENT;
  }
  return S3GRL_OK;
}

s3grl_status launch_split_count(s3grl_context* ctx, const Job* jobs, int64_t njobs, int seg_shift,
                                int32_t* cnt, int64_t* piece_off, int64_t* scan_ws) {
  if (njobs == 0) return S3GRL_OK;
  hipLaunchKernelGGL(split_count_kernel, dim3((unsigned)((njobs + 255) / 256)), dim3(256), 0, ctx->stream, jobs,
                     njobs, seg_shift, cnt);
  S3GRL_HIP_TRY(hipGetLastError());
  return launch_scan_i32_to_i64(ctx, cnt, njobs, piece_off, scan_ws);
}

s3grl_status launch_split_fill(s3grl_context* ctx, const Job* jobs, const int32_t* job_lim, int64_t njobs,
                               const int32_t* job_order, int K, int seg_shift, const int64_t* piece_off,
                               int64_t npieces, Job* gjobs, int32_t* g_lim, int32_t* g_order, int32_t* piece_job) {
  if (njobs == 0) return S3GRL_OK;
  hipLaunchKernelGGL(split_fill_kernel, dim3((unsigned)((njobs + 255) / 256)), dim3(256), 0, ctx->stream, jobs,
                     job_lim, job_order, njobs, K, seg_shift, piece_off, npieces, gjobs, g_lim, g_order, piece_job);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_combine(s3grl_context* ctx, const s3grl_plan* p, const float* prows, const float* X,
                            int64_t ldx, int64_t F, float* rows) {
  if (p->njobs == 0 || p->npieces == 0) return S3GRL_OK;
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)p->npieces, 2), dim3(256), 0, ctx->stream, p->jobs,
                     p->piece_off, p->piece_job, p->job_z, p->cfg.sign_k, prows, X, ldx, (int)F, rows);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_mirror_rows(s3grl_context* ctx, const int32_t* partner, int64_t L,
                                int32_t* n_rows) {
  if (L == 0) return S3GRL_OK;
  hipLaunchKernelGGL(mirror_rows_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, ctx->stream,
                     partner, L, n_rows);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_count(s3grl_context* ctx, const s3grl_graph* g, const int64_t* links, int64_t L,
                          int hops, int plus, int K, WalkSets ws,
                          const int32_t* partner, const int32_t* mirror_of, int32_t* n_nodes, int32_t* p_nodes,
                          int32_t* n_rows, int32_t* n_jobs, int32_t* lvl_max, int32_t* err_flag,
                          int64_t* tot_nodes_alg, HopSampling smp, int32_t* stash, int slot,
                          int32_t* lvl_stash, const int32_t* perm) {
  if (L == 0) return S3GRL_OK;
  const int W = words_for(g->num_nodes);
  const int nbm = (hops <= 1 || walks_on(ws)) ? 2 : 3;   // see count_kernel: no frontier bitmap for one hop
  const int nsets = nbm + (hop_sampling_on(smp) ? 1 : 0);
  const size_t lds = (size_t)(nsets * W + 8 + kHubWords + kCountList) * 4;
  const bool sparse = (double)g->nnz / (double)std::max<int64_t>(g->num_nodes, 1) <= 6.0;
  const int32_t* cn_ip = g->directed ? g->out_indptr : g->indptr;
  const int32_t* cn_ix = g->directed ? g->out_indices : g->indices;
  if (lds > 163840 || getenv("S3GRL_FORCE_EXT_BITMAPS")) {
    // The N-bit bitmaps do not fit a CU's LDS (num_nodes > ~327 680): they live in HBM, one slice per
    // workgroup of a launch, and the list is processed in chunks that share the slices.
    const int64_t stride = ((int64_t)nsets * W + 63) / 64 * 64;
    const int chunk = (int)std::min<int64_t>(L, std::max<int64_t>(256, ((int64_t)1 << 29) / (stride * 4)));   // <= 512 MiB of slices
    Transient tmp{ctx, {}};
    void* q = nullptr;
    S3GRL_TRY(ctx->arena.alloc((size_t)stride * 4 * chunk, &q));
    tmp.ptrs.push_back(q);
    const size_t lds_ext = (size_t)(8 + kHubWords + kCountList) * 4;
    auto kern = sparse ? count_kernel<4, 256, true> : count_kernel<8, 256, true>;
    for (int64_t base = 0; base < L; base += chunk) {
      const int64_t cnt = std::min<int64_t>(chunk, L - base);
      hipLaunchKernelGGL(kern, dim3((unsigned)cnt), dim3(256), lds_ext, ctx->stream, g->indptr, g->indices,
                         (int)g->num_nodes, W, links, hops, plus, K, g->max_degree > kHubArmDegree ? 1 : 0, ws,
                         partner, mirror_of, n_nodes, p_nodes, n_rows, n_jobs, lvl_max, err_flag,
                         reinterpret_cast<unsigned long long*>(tot_nodes_alg), smp, stash, slot, lvl_stash, cn_ip,
                         cn_ix, g->directed ? 1 : 0, static_cast<uint32_t*>(q), stride, (int)base, perm);
      S3GRL_HIP_TRY(hipGetLastError());
    }
    S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));   // the slices are released on return
    return S3GRL_OK;
  }
  const bool small = lds <= 24 * 1024;
  auto kern = small ? (sparse ? count_kernel<4, 128> : count_kernel<8, 128>)
                    : (sparse ? count_kernel<4, 256> : count_kernel<8, 256>);
  S3GRL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)L), dim3(small ? 128 : 256), lds, ctx->stream, g->indptr,
                     g->indices, (int)g->num_nodes, W, links, hops, plus, K,
                     g->max_degree > kHubArmDegree ? 1 : 0, ws, partner, mirror_of, n_nodes,
                     p_nodes, n_rows, n_jobs, lvl_max, err_flag,
                     reinterpret_cast<unsigned long long*>(tot_nodes_alg), smp, stash, slot, lvl_stash,
                     cn_ip, cn_ix, g->directed ? 1 : 0, nullptr, 0, 0, perm);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

// ---------------------------------------------------------------------------------------
// Gather order: one wavefront per job, and the jobs differ in length by two orders of magnitude.
// Started in list order, a long job that begins late is the tail of the launch; started longest
// first (LPT) the tail is made of short ones (PubMed: 10.7 -> 9.7 ms).  A counting sort of the
// jobs by their link's node count in kOrderBuckets descending buckets; inside a bucket the order
// is whatever the atomics give (results do not depend on it).
constexpr int kOrderBuckets = 256;
constexpr int kOrderShift = 5;   // 32 nodes per bucket, everything >= 8160 nodes in the first

__device__ __forceinline__ int order_bucket(int n) {
  return kOrderBuckets - 1 - min(n >> kOrderShift, kOrderBuckets - 1);
}

// Both passes keep a workgroup-local histogram in LDS and touch the global one once per
// (workgroup, bucket): 164 000 global atomics on 256 counters cost 0.2 ms per pass otherwise.
constexpr int kOrderThreads = 1024;

__global__ __launch_bounds__(kOrderThreads) void order_hist_kernel(
    const int32_t* __restrict__ n_nodes, const int32_t* __restrict__ n_jobs, int64_t L, int64_t per_block,
    int32_t* __restrict__ hist) {
  __shared__ int h[kOrderBuckets];
  const int t = threadIdx.x;
  if (t < kOrderBuckets) h[t] = 0;
  __syncthreads();
  const int64_t l0 = (int64_t)blockIdx.x * per_block, l1 = min(l0 + per_block, L);
  for (int64_t l = l0 + t; l < l1; l += kOrderThreads) {
    const int nj = n_jobs[l];
    if (nj > 0) atomicAdd(&h[order_bucket(n_nodes[l])], nj);
  }
  __syncthreads();
  if (t < kOrderBuckets && h[t]) atomicAdd(&hist[t], h[t]);
}

__global__ void order_scan_kernel(int32_t* __restrict__ hist /* in: counts, out: cursors */) {
  __shared__ int sh[kOrderBuckets];
  const int t = threadIdx.x;
  sh[t] = hist[t];
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int b = 0; b < kOrderBuckets; ++b) {
      const int c = sh[b];
      sh[b] = run;
      run += c;
    }
  }
  __syncthreads();
  hist[t] = sh[t];
}

__global__ __launch_bounds__(kOrderThreads) void order_fill_kernel(
    const int32_t* __restrict__ n_nodes, const int32_t* __restrict__ n_jobs,
    const int64_t* __restrict__ job_off, int64_t L, int64_t per_block, int32_t* __restrict__ cursor,
    int32_t* __restrict__ job_order) {
  __shared__ int h[kOrderBuckets];     // this workgroup's jobs per bucket, then its running cursor
  __shared__ int base[kOrderBuckets];  // where its share of the bucket starts
  const int t = threadIdx.x;
  if (t < kOrderBuckets) h[t] = 0;
  __syncthreads();
  const int64_t l0 = (int64_t)blockIdx.x * per_block, l1 = min(l0 + per_block, L);
  for (int64_t l = l0 + t; l < l1; l += kOrderThreads) {
    const int nj = n_jobs[l];
    if (nj > 0) atomicAdd(&h[order_bucket(n_nodes[l])], nj);
  }
  __syncthreads();
  if (t < kOrderBuckets) {
    base[t] = h[t] ? atomicAdd(&cursor[t], h[t]) : 0;
    h[t] = 0;
  }
  __syncthreads();
  for (int64_t l = l0 + t; l < l1; l += kOrderThreads) {
    const int nj = n_jobs[l];
    if (nj <= 0) continue;
    const int b = order_bucket(n_nodes[l]);
    const int at = base[b] + atomicAdd(&h[b], nj);
    const int j0 = (int)job_off[l];
    for (int j = 0; j < nj; ++j) job_order[at + j] = j0 + j;
  }
}

// Plans with a processing order (launch_link_order): the gather takes the jobs link by link in that
// order — neighbours in the order read the same rows of X — instead of longest first.
__global__ void perm_jobs_kernel(const int32_t* __restrict__ perm, const int32_t* __restrict__ n_jobs, int64_t L,
                                 int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L) cnt[i] = n_jobs[perm[i]];
}

__global__ void perm_fill_kernel(const int32_t* __restrict__ perm, const int32_t* __restrict__ n_jobs,
                                 const int64_t* __restrict__ job_off, const int64_t* __restrict__ at, int64_t L,
                                 int32_t* __restrict__ job_order) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  const int l = perm[i];
  const int nj = n_jobs[l];
  const int j0 = (int)job_off[l];
  const int64_t a = at[i];
  for (int j = 0; j < nj; ++j) job_order[a + j] = j0 + j;
}

s3grl_status launch_job_order(s3grl_context* ctx, const int32_t* n_nodes, const int32_t* n_jobs,
                              const int64_t* job_off, int64_t L, int32_t* hist /* [256] scratch */,
                              int32_t* job_order, const int32_t* perm, int32_t* scratch_cnt,
                              int64_t* scratch_off, int64_t* scan_ws) {
  if (L == 0) return S3GRL_OK;
  if (perm) {
    const unsigned grid = (unsigned)((L + 255) / 256);
    hipLaunchKernelGGL(perm_jobs_kernel, dim3(grid), dim3(256), 0, ctx->stream, perm, n_jobs, L, scratch_cnt);
    S3GRL_HIP_TRY(hipGetLastError());
    S3GRL_TRY(launch_scan_i32_to_i64(ctx, scratch_cnt, L, scratch_off, scan_ws));
    hipLaunchKernelGGL(perm_fill_kernel, dim3(grid), dim3(256), 0, ctx->stream, perm, n_jobs, job_off, scratch_off,
                       L, job_order);
    S3GRL_HIP_TRY(hipGetLastError());
    return S3GRL_OK;
  }
  S3GRL_HIP_TRY(hipMemsetAsync(hist, 0, kOrderBuckets * sizeof(int32_t), ctx->stream));
  const int64_t per_block = std::max<int64_t>((L + 255) / 256, 4 * kOrderThreads);
  const unsigned grid = (unsigned)((L + per_block - 1) / per_block);
  hipLaunchKernelGGL(order_hist_kernel, dim3(grid), dim3(kOrderThreads), 0, ctx->stream, n_nodes, n_jobs, L,
                     per_block, hist);
  hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(kOrderBuckets), 0, ctx->stream, hist);
  hipLaunchKernelGGL(order_fill_kernel, dim3(grid), dim3(kOrderThreads), 0, ctx->stream, n_nodes, n_jobs, job_off,
                     L, per_block, hist, job_order);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

int64_t scan_workspace_elems(int64_t n) { return (n + kScanTile - 1) / kScanTile + 1; }

s3grl_status launch_scan3(s3grl_context* ctx, const int32_t* in0, const int32_t* in1, const int32_t* in2,
                          int64_t n, int64_t* out0, int64_t* out1, int64_t* out2, int64_t* workspace3,
                          int64_t* max0, int64_t* max1, int64_t* totals) {
  const int64_t nb = (n + kScanTile - 1) / kScanTile;
  const int64_t wsz = scan_workspace_elems(n);
  Scan3 a;
  a.in[0] = in0; a.in[1] = in1; a.in[2] = in2;
  a.out[0] = out0; a.out[1] = out1; a.out[2] = out2;
  for (int y = 0; y < 3; ++y) {
    a.part[y] = workspace3 + y * wsz;
    a.total_out[y] = totals ? totals + y : nullptr;
  }
  a.max_out[0] = reinterpret_cast<long long*>(max0);
  a.max_out[1] = reinterpret_cast<long long*>(max1);
  a.max_out[2] = nullptr;
  hipLaunchKernelGGL(scan3_partials_kernel, dim3((unsigned)nb, 3), dim3(256), 0, ctx->stream, a, n);
  hipLaunchKernelGGL(scan3_top_kernel, dim3(3), dim3(1024), 0, ctx->stream, a, nb, n);
  hipLaunchKernelGGL(scan3_apply_kernel, dim3((unsigned)nb, 3), dim3(256), 0, ctx->stream, a, n);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_scan_i32_to_i64(s3grl_context* ctx, const int32_t* in, int64_t n, int64_t* out,
                                    int64_t* workspace) {
  if (n == 0) {
    S3GRL_HIP_TRY(hipMemsetAsync(out, 0, 8, ctx->stream));
    return S3GRL_OK;
  }
  const int64_t nb = (n + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(scan_partials_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, in, n,
                     workspace);
  hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(1024), 0, ctx->stream, workspace, nb, out + n);
  hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, in, n,
                     workspace, out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}


// The hash flavour pays off when the bitmaps alone would hold a CU to a few workgroups.
bool sparse_mode_for(const s3grl_graph* g) {
  if (getenv("S3GRL_FORCE_HASH")) return true;   // test hook
  return 3 * (size_t)words_for(g->num_nodes) * 4 > 24 * 1024;
}

int num_class_lists() { return kNumListsAll; }

// One-hop plans take the row-intersection path on graphs where the hash flavour is in use anyway.
bool onehop_mode_for(const s3grl_graph* g) {
  if (getenv("S3GRL_FORCE_ONEHOP")) return true;   // test hook
  return sparse_mode_for(g);
}

s3grl_status build_forward_rows(s3grl_context* ctx, s3grl_graph* g) {
  const int64_t N = g->num_nodes;
  Transient tmp{ctx, {}};
  void* q = nullptr;
  S3GRL_TRY(ctx->arena.alloc((size_t)N * 4, &q));
  tmp.ptrs.push_back(q);
  int32_t* cnt = static_cast<int32_t*>(q);
  S3GRL_TRY(ctx->arena.alloc((size_t)(N + 1) * 8, &q));
  tmp.ptrs.push_back(q);
  int64_t* off64 = static_cast<int64_t*>(q);
  S3GRL_TRY(ctx->arena.alloc((size_t)scan_workspace_elems(N) * 8, &q));
  tmp.ptrs.push_back(q);
  int64_t* ws = static_cast<int64_t*>(q);
  const unsigned grid = (unsigned)((N + 255) / 256);
  hipLaunchKernelGGL(fwd_count_kernel, dim3(grid), dim3(256), 0, ctx->stream, g->indptr, g->indices, N, cnt);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(launch_scan_i32_to_i64(ctx, cnt, N, off64, ws));
  S3GRL_HIP_TRY(hipMemcpyAsync(ctx->h_scalars, off64 + N, 8, hipMemcpyDeviceToHost, ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const int64_t fnnz = ctx->h_scalars[0];
  S3GRL_TRY(ctx->arena.alloc((size_t)(N + 1) * 4, &q));
  g->fwd_indptr = static_cast<int32_t*>(q);
  S3GRL_TRY(ctx->arena.alloc((size_t)std::max<int64_t>(fnnz, 1) * 4, &q));
  g->fwd_indices = static_cast<int32_t*>(q);
  S3GRL_TRY(ctx->arena.alloc((size_t)N * 2, &q));
  g->fwd_deg = static_cast<uint16_t*>(q);
  hipLaunchKernelGGL(fwd_fill_kernel, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, ctx->stream,
                     g->indptr, g->indices, N, off64, g->fwd_indptr, g->fwd_indices, g->fwd_deg);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));   // tmp is released on return
  return S3GRL_OK;
}

s3grl_status launch_count1(s3grl_context* ctx, const s3grl_graph* g, const int64_t* links, int64_t L,
                           int plus, int K, const int32_t* partner, const int32_t* mirror_of,
                           int32_t* n_nodes, int32_t* p_nodes, int32_t* n_rows, int32_t* n_jobs,
                           int32_t* lvl_max, int32_t* e_cap, int32_t* err_flag, int64_t* tot_nodes_alg,
                           int64_t* tot_oriented, const int32_t* perm, int64_t* x_cap) {
  if (L == 0) return S3GRL_OK;
  hipLaunchKernelGGL(count1_kernel, dim3((unsigned)((L + kCount1Waves - 1) / kCount1Waves)),
                     dim3(64 * kCount1Waves), 0, ctx->stream, g->indptr, g->indices, g->fwd_deg,
                     (int)g->num_nodes, links, L, plus, K, partner, mirror_of, n_nodes, p_nodes, n_rows,
                     n_jobs, lvl_max, e_cap, err_flag, reinterpret_cast<unsigned long long*>(tot_nodes_alg),
                     reinterpret_cast<unsigned long long*>(tot_oriented), perm, g->hub,
                     (x_cap && g->hub.nh > 0) ? x_cap : nullptr);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_classify(s3grl_context* ctx, const s3grl_graph* g, int cn_cap, int K,
                             const int32_t* n_nodes, const int32_t* p_nodes,
                             const int32_t* lvl_max, int64_t L, int32_t* class_count,
                             int32_t* class_list, bool allow_hash, const int32_t* e_cap, int stash_slot,
                             const int32_t* perm, const int64_t* x_cap, const int32_t* csr_e, bool tiny_ok) {
  if (L == 0) return S3GRL_OK;
  // link_tiny_kernel takes the smallest one-hop links of plans without common-neighbour rows (never a list that
  // a test hook would split: S3GRL_SPLIT_SEG_SHIFT below 6)
  const char* segs = getenv("S3GRL_SPLIT_SEG_SHIFT");
  const int tiny_max_n = (tiny_ok && !getenv("S3GRL_NO_TINY") && !(segs && atoi(segs) < 6)) ? kTinyNodes : 0;
  ClassBounds cb = class_bounds(g, cn_cap, K);
  const bool dm = allow_hash && stash_slot > 0 && dm_mode_for(g);
  if (cb.b[kNumClasses - 1] < 0 || getenv("S3GRL_FORCE_EXT_BITMAPS")) {
    // the N-bit bitmaps of the bitmap flavour do not fit LDS: apart from the hash / one-hop classes
    // there is only the HBM-scratch class, with its bitmaps in the slice too
    for (int c = 0; c < kNumClasses; ++c) cb.b[c] = -1;   // every link "overflows" the LDS classes
  }
  ClassBounds hb{};
  static_assert(kHubClasses <= kNumClasses, "hub class bounds travel in a ClassBounds");
  static_assert(kHubClasses < kNumClasses, "one more entry for the test hook");
  for (int c = 0; c < kHubClasses; ++c) hb.b[c] = hub_class_bound(c, cn_cap, K);
  hb.b[kHubClasses] = getenv("S3GRL_FORCE_HUB_SLICES") ? 1 : 0;   // test hook: found edges in HBM slices
  CsrBounds csrb{};
  for (int c = 0; c < kCsrClasses; ++c) csrb.b[c] = csr_class_bound(c, cn_cap, K);
  hipLaunchKernelGGL(classify_kernel, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, ctx->stream,
                     n_nodes, p_nodes, lvl_max, L, cb, dm ? 2 : ((allow_hash && sparse_mode_for(g)) ? 1 : 0),
                     dm ? class_bounds_dm(g, cn_cap, K) : class_bounds_sparse(g, cn_cap, K), e_cap,
                     class_bounds_full(cn_cap, K),
                     getenv("S3GRL_FORCE_BM_HBM") ? 0 : (1 << 30),   // test hook: bit matrices in HBM
                     dm ? std::min(stash_slot + 2, 65535) : 0, dm ? dm_class_mask_for(g, cn_cap, K) : 0,
                     class_count, class_list, perm, x_cap, hb, csr_e, csrb, words_for(g->num_nodes), tiny_max_n);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}


s3grl_status launch_links(s3grl_context* ctx, const s3grl_graph* g, const int64_t* links, int64_t L,
                          const int32_t* class_list, const int32_t* class_count_host, int hops,
                          int plus, int cn_cap, int full_stats, int K, WalkSets ws, const int32_t* p_nodes,
                          const LinkOut& out, HopSampling smp, const int32_t* stash, int slot,
                          const int32_t* e_cap, const int32_t* new_of_old, const int64_t* x_cap,
                          const uint16_t* csr_cnt, const int32_t* csr_e, int sop2) {
  if (L == 0) return S3GRL_OK;
  // links too large for LDS keep their lists in HBM scratch: one 256-byte aligned slice each
  Transient scratch_owner{ctx, {}};
  char* scratch = nullptr;
  int64_t scratch_stride = 0;
  int bm_ext_words = 0, gs_chunk = 0;
  if (class_count_host[kNumClasses] > 0) {
    scratch_stride = ((int64_t)class_count_host[kNumClasses + 1] + 255) / 256 * 256;
    int64_t slices = class_count_host[kNumClasses];
    if (4 * (int64_t)link_fixed_words(g, cn_cap, K) > kLdsBytes || getenv("S3GRL_FORCE_EXT_BITMAPS")) {
      // the graph's bitmaps do not fit LDS: they go to the head of every slice, and the class runs in
      // chunks over at most 512 MiB of slices
      bm_ext_words = (3 * words_for(g->num_nodes) + 63) / 64 * 64;
      scratch_stride += (int64_t)bm_ext_words * 4;
      gs_chunk = (int)std::min<int64_t>(slices, std::max<int64_t>(64, ((int64_t)1 << 29) / scratch_stride));
      slices = gs_chunk;
    }
    void* q = nullptr;
    S3GRL_TRY(ctx->arena.alloc((size_t)scratch_stride * slices, &q));
    scratch_owner.ptrs.push_back(q);
    scratch = static_cast<char*>(q);
  }
  LinkArgs a{g, links, class_list, hops, plus, cn_cap, full_stats, ws, p_nodes, out, scratch, scratch_stride,
             getenv("S3GRL_DEBUG_STAMPS") ? reinterpret_cast<unsigned long long*>(ctx->d_scalars + 16) : nullptr,
             smp, stash, slot, e_cap, nullptr, 0, 0, 0, new_of_old,
             (out.old_of_new && !getenv("S3GRL_NO_LEAF_WALK")) ? g->deg_le2_from : -1,
             DirGraph{g->out_indptr, g->out_indices, g->in_indptr, g->in_indices}, bm_ext_words, gs_chunk, 0,
             x_cap, nullptr, 0, 0, csr_cnt, csr_e, sop2};
  if (class_count_host[kHubBase + kHubClasses] > 0) {   // list of found edges (uint32) + columns (2 x uint16) per slice
    const int64_t xmax = ((int64_t)class_count_host[29] + 63) / 64 * 64;
    a.hub_slice_words = 2 * xmax;
    a.hub_slice_grid = (int)std::min<int64_t>(class_count_host[kHubBase + kHubClasses], 256);
    void* q = nullptr;
    S3GRL_TRY(ctx->arena.alloc((size_t)a.hub_slice_words * 4 * a.hub_slice_grid, &q));
    scratch_owner.ptrs.push_back(q);
    a.hub_slices = static_cast<uint32_t*>(q);
  }
  // the class whose bit matrix does not fit LDS: one slice per resident workgroup of a persistent grid
  if (class_count_host[kFullBig] > 0) {
    // slice = list of found edges (uint32, at most ecap / 2) + CSR columns (uint16 x ecap) of the
    // link with the largest bound
    a.bm_stride_words = ((int64_t)class_count_host[31] / 2 + 2 + (class_count_host[31] + 2) / 2 + 63) / 64 * 64;
    // all of a CU's LDS for one 1024-thread workgroup: whatever the hash and the per-node arrays
    // leave holds the CSR columns whenever the exact entry count allows (see link_full_kernel)
    a.big_need = 163840 - 4 * full_fixed_words(cn_cap, K);
    a.bm_grid = (int)std::min<int64_t>(class_count_host[kFullBig], 256);
    void* q = nullptr;
    S3GRL_TRY(ctx->arena.alloc((size_t)a.bm_stride_words * 4 * a.bm_grid, &q));
    scratch_owner.ptrs.push_back(q);
    a.bm_scratch = static_cast<uint32_t*>(q);
  }
  switch (K) {
    case 1: return launch_links_k<1>(ctx, a, L, class_count_host);
    case 2: return launch_links_k<2>(ctx, a, L, class_count_host);
    case 3: return launch_links_k<3>(ctx, a, L, class_count_host);
    case 4: return launch_links_k<4>(ctx, a, L, class_count_host);
    case 5: return launch_links_k<5>(ctx, a, L, class_count_host);
    case 6: return launch_links_k<6>(ctx, a, L, class_count_host);
    case 7: return launch_links_k<7>(ctx, a, L, class_count_host);
    case 8: return launch_links_k<8>(ctx, a, L, class_count_host);
    default:
      set_last_error("sign_k must be in 1..8");
      return S3GRL_ERR_INVALID_ARGUMENT;
  }
}


s3grl_status launch_dists(s3grl_context* ctx, const int64_t* node_off, const int32_t* lvl, int64_t L,
                          int8_t* dists) {
  if (L == 0) return S3GRL_OK;
  hipLaunchKernelGGL(dists_kernel, dim3((unsigned)L), dim3(256), 0, ctx->stream, node_off, lvl, L,
                     dists);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

}  // namespace s3grl

S3GRL_DEFINE_TOUCH(structure)
