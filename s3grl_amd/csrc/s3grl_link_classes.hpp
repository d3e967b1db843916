// Link classes: what the plan stages (s3grl_structure.hip) and the link kernels (s3grl_link_kernels.inl,
// compiled by s3grl_links_k*.hip) agree on.  Class ids and LDS needs, the host bounds and threads per class,
// the arguments of a plan's link launches and the per-sign_k launcher.  This header defines no kernel that
// is not a template: every unit that includes it would carry a copy of it.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "s3grl_internal.hpp"
#include "s3grl_device.hpp"

namespace s3grl {
namespace {

// ---------------------------------------------------------------------------------------
// LDS bytes link_kernel needs beyond its fixed part: list[n] + dinvP[p] + two float2 state
// arrays [p] (+ alignment slack); the hash flavour adds its keys/vals tables.
// When every operator reaches the whole subgraph (p == n) and the subgraph is small, link_kernel
// also keeps its adjacency as an n x n bit matrix (+ two index maps), see there.
constexpr int kBmMaxNodes = 512;
__host__ __device__ __forceinline__ int link_bm_bytes(int n, int p) {
  return (p == n && n <= kBmMaxNodes) ? 4 * n * ((n + 31) >> 5) + 4 * n + 8 : 0;
}
__host__ __device__ __forceinline__ int link_lds_need(int n, int p) { return 4 * n + 20 * p + 16; }
__host__ __device__ __forceinline__ int link_lds_need_sparse(int n, int p) {
  int C = 64;
  while (C < 2 * n) C <<= 1;
  return 8 * C + link_lds_need(n, p) + link_bm_bytes(n, p);
}

// link_kernel's fixed LDS behind its visited set, in words: cn[cn_cap] lvl_end[kMaxLevels] zbuf[4K] sh[32] and,
// only where the hub path of walk_rows is armed (`hubs`), the deferred-hub bitmap.  The kernel places list[] right
// behind it and the host sizes classes and launches by it: the one statement of this layout.
__host__ __device__ __forceinline__ int link_tail_words(int cn_cap, int K, bool hubs) {
  return cn_cap + kMaxLevels + 4 * K + 32 + (hubs ? kHubWords : 0);
}

struct ClassBounds {
  int b[kNumClasses];
};

// class ids: 0..kNumClasses-1 bitmap flavour by LDS need, kNumClasses = HBM-scratch flavour,
// kSparseBase.. = hash flavour by LDS need.  class_count[kNumClasses + 1] = max need of the
// HBM-scratch class.
constexpr int kSparseBase = kNumClasses + 2;
// kFullBase.. = one-hop full-reach links for link_full_kernel by LDS need (bit matrix in LDS),
// kFullBig = the same with the bit matrix in an HBM slice (subgraphs of more than ~700 nodes)
constexpr int kFullBase = kSparseBase + kNumClasses;
constexpr int kFullBig = kFullBase + kNumClasses;
// kHubBase.. = one-hop links with a cached hub neighbourhood, link_hub_kernel (s3grl_hub.hip) by LDS need
constexpr int kHubBase = kFullBig + 1;
constexpr int kNumLists = kHubBase + kHubClasses + 1;   // (+ the class with its found edges in HBM slices)
constexpr int kTinyList = kNumLists;   // one-hop PoS links of at most kTinyNodes nodes: link_tiny_kernel (s3grl_hub.hip)
static_assert(kTinyList + 1 < 29, "class_count[29..31] carry maxima");
// kCsrBase.. (s3grl_internal.hpp) = full-reach links on their induced LDS CSR, link_csr_kernel (s3grl_csr.hip)
constexpr int kNumListsAll = kCsrBase + kCsrClasses;

// ---- sizes of a one-hop subgraph (count1_kernel in s3grl_structure.hip, link_full_kernel) -------
// lower bound of x in an ascending row, through unsigned offsets on a uniform base
__device__ __forceinline__ int row_lower_bound(const int32_t* __restrict__ a, int n, int x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// LDS bytes of link_full_kernel beyond its fixed part; `with_bm`: the bit matrix in LDS too
__host__ __device__ __forceinline__ int full_hash_slots(int n) {
  int C = 64;
  while (C < 2 * n) C <<= 1;
  return C;
}
// on_chip: the bit matrix and the CSR columns in LDS too (otherwise both sit in an HBM slice)
__host__ __device__ __forceinline__ int full_lds_need(int n, int ecap, bool on_chip) {
  const int WB = (n + 31) >> 5;
  return 8 * full_hash_slots(n) + 12 * n + 16 + (on_chip ? 2 * ((ecap + 1) & ~1) + 4 * n * WB : 64 * WB);
}

constexpr int kLongRow = 96;    // CSR rows longer than this are summed by a whole wavefront
constexpr int kLongCap = 128;   // ... at most this many per link (the others stay with their 4 lanes)

}  // namespace

// ---------------------------------------------------------------------------------------
static inline int words_for(int64_t N) { return (int)((N + 31) / 32); }

// The hub path of walk_rows (s3grl_device.hpp) is armed for graphs that have a row of more than kHubArmDegree
// entries: the launchers' `hubs` argument and the LDS layout below both come from here.
static inline bool hub_armed(const s3grl_graph* g) { return g->max_degree > kHubArmDegree; }

// fixed part of link_kernel's LDS: the visited set (3 bitmaps / the direct map / nothing: the hash tables are
// sized per link) + link_tail_words (cn + lvl_end + zbuf + scan scratch + the hub bitmap where it is armed)
static inline int link_fixed_words(const s3grl_graph* g, int cn_cap, int K) {
  return 3 * words_for(g->num_nodes) + link_tail_words(cn_cap, K, hub_armed(g));
}
static inline int link_fixed_words_sparse(const s3grl_graph* g, int cn_cap, int K) {
  return link_tail_words(cn_cap, K, hub_armed(g));
}
static inline int link_fixed_words_dm(const s3grl_graph* g, int cn_cap, int K) {
  return 16 * words_for(g->num_nodes) + link_tail_words(cn_cap, K, hub_armed(g));
}

// nominal class bounds: variable LDS bytes per link (list + state on the propagation prefix), upper
// bound per class
static constexpr int kNominalBounds[kNumClasses] = {6144, 12288, 24576, 49152, 98304, 163840};

// A CU has 160 KiB of LDS and hands it out in granules of 320 words.
constexpr int kLdsBytes = 163840;
constexpr int kLdsGranule = 1280;
// the most LDS a workgroup may take if k of them are to be resident on a CU
static inline int lds_share(int k) { return kLdsBytes / k / kLdsGranule * kLdsGranule; }

// The bounds are cut by what fits, not at the nominal values: a class of k resident workgroups takes every link
// up to the LAST byte at which k still fit, lds_share(k) less the graph's fixed part.  k is, of the two counts
// around the nominal bound, the one whose cut lies nearer to it (PubMed, fixed part 7.7 KB: 6 368 / 12 768 /
// 24 288 / 46 048 / 74 208 bytes at 11 / 8 / 5 / 3 / 2 workgroups per CU; the nominal bounds gave 10 / 7 / 4 / 2 / 1).
// A function of the graph and of (cn_cap, K) only, like everything that decides a link's class.
static ClassBounds cut_bounds(int fixed_bytes, int avail) {
  ClassBounds cb;
  for (int c = 0; c < kNumClasses; ++c) {
    const int k0 = std::max(1, kLdsBytes / std::max(fixed_bytes + kNominalBounds[c], 1));
    const int lo = lds_share(k0 + 1) - fixed_bytes, hi = lds_share(k0) - fixed_bytes;   // lo <= nominal-ish <= hi
    int b = kNominalBounds[c];
    if (hi > 0) b = (lo > 0 && kNominalBounds[c] - lo < hi - kNominalBounds[c]) ? lo : hi;
    cb.b[c] = std::min(b, avail);
  }
  cb.b[kNumClasses - 1] = avail;
  return cb;
}
// resident workgroups per CU of a class that takes `lds` bytes (what the cut above aims at; debug statistics)
static inline int lds_resident(size_t lds) {
  return (int)(kLdsBytes / std::max<size_t>((lds + kLdsGranule - 1) / kLdsGranule * kLdsGranule, kLdsGranule));
}

// class c holds the links whose variable LDS need is <= bound[c] bytes; the last bound is
// whatever the 160 KiB of a CU leave after the fixed part
static ClassBounds class_bounds(const s3grl_graph* g, int cn_cap, int K) {
  const int fixed = 4 * link_fixed_words(g, cn_cap, K);
  int avail = kLdsBytes - fixed;
  if (const char* e = getenv("S3GRL_LDS_BUDGET")) avail = std::min(avail, atoi(e));  // test hook
  return cut_bounds(fixed, avail);
}
static ClassBounds class_bounds_sparse(const s3grl_graph* g, int cn_cap, int K) {
  static const int nominal[kNumClasses] = {4096, 8192, 16384, 32768, 65536, 131072};
  const int avail = kLdsBytes - 4 * link_fixed_words_sparse(g, cn_cap, K);
  ClassBounds cb;
  for (int c = 0; c < kNumClasses; ++c) cb.b[c] = std::min(nominal[c], avail);
  return cb;
}

// link_full_kernel: fixed LDS = cn + cnpos + lvl_end[2] + zbuf + scan scratch + long-row list
static inline int full_fixed_words(int cn_cap, int K) { return 2 * cn_cap + 2 + 4 * K + 32 + kLongCap / 2; }
static ClassBounds class_bounds_full(int cn_cap, int K) {
  static const int nominal[kNumClasses] = {3072, 6144, 12288, 24576, 65536, 160000};
  const int avail = 163840 - 4 * full_fixed_words(cn_cap, K);
  ClassBounds cb;
  for (int c = 0; c < kNumClasses; ++c) cb.b[c] = std::min(nominal[c], avail);
  return cb;
}

// threads per link of an LDS class
static int threads_for_class(size_t lds, int c) {
  // the smallest subgraphs (a few hundred nodes at most): two wavefronts per link — the uniform part
  // of the kernel is most of their cost, and ten such links fit a CU either way
  if (c == 0 && lds <= 40 * 1024) return 128;
  return lds <= 40 * 1024 ? 256 : (lds <= 80 * 1024 ? 512 : 1024);
}

static ClassBounds class_bounds_dm(const s3grl_graph* g, int cn_cap, int K) {
  const int fixed = 4 * link_fixed_words_dm(g, cn_cap, K);
  return cut_bounds(fixed, kLdsBytes - fixed);
}

// The direct-map flavour: graphs whose 2N-byte map leaves nearly all of a CU's LDS to the lists.
static bool dm_mode_for(const s3grl_graph* g) {
  if (sparse_mode_for(g) || getenv("S3GRL_NO_DM")) return false;
  // measured after the degree order: USAir (332 nodes) link kernels 0.077 -> 0.058 ms, Cora (2 708)
  // 0.35 -> 0.34, PubMed (19 717: 39 KB of map per link) 3.94 -> 4.13 — the map has to be small
  return g->num_nodes <= 8192;
}

// The map costs LDS, i.e. resident wavefronts: class by class, the direct-map flavour is used where
// it fits at least 4/5 of the waves the bitmap flavour fits on a CU (measured: a loss of up to 1/5
// is paid back by the cheaper visits; PubMed, 39 KB of map: every class but the smallest).
static int waves_per_cu(size_t lds, int c) {
  return std::min<int>(32, lds_resident(lds) * (threads_for_class(lds, c) / 64));
}
static int dm_class_mask_for(const s3grl_graph* g, int cn_cap, int K) {
  const ClassBounds bb = class_bounds(g, cn_cap, K), bd = class_bounds_dm(g, cn_cap, K);
  int mask = 0;
  for (int c = 0; c < kNumClasses; ++c) {
    if (bd.b[c] <= 0) continue;
    if (bb.b[c] <= 0) { mask |= 1 << c; continue; }
    const size_t lb = (size_t)4 * link_fixed_words(g, cn_cap, K) + bb.b[c];
    const size_t ld = (size_t)4 * link_fixed_words_dm(g, cn_cap, K) + bd.b[c];
    const int wb = waves_per_cu(lb, c), wd = waves_per_cu(ld, c);
    // the smallest class is bound by links in flight, not by waves: at least half as many must fit
    if (c == 0 && 2 * std::min(lds_resident(ld), 16) < std::min(lds_resident(lb), 16)) continue;
    if (5 * wd >= 4 * wb) mask |= 1 << c;
  }
  return mask;
}

// The arguments of a plan's link launches (launch_links -> launch_links_k<K>)
struct LinkArgs {
  const s3grl_graph* g;
  const int64_t* links;
  const int32_t* class_list;
  int hops, plus, cn_cap, full_stats;
  WalkSets ws;
  const int32_t* p_nodes;
  LinkOut out;
  char* scratch;
  int64_t scratch_stride;
  unsigned long long* dbg;
  HopSampling smp;
  const int32_t* stash;
  int slot;
  const int32_t* e_cap;
  uint32_t* bm_scratch;
  int64_t bm_stride_words;
  int bm_grid;
  int big_need;   // LDS need of the biggest link of the class whose matrix / columns sit in HBM
  const int32_t* new_of_old;                // non-null: the graph is walked in its degree order
  int lo_id;                                // then: ids >= lo_id have at most two stored neighbours (else -1)
  DirGraph dg;                              // arcs of a directed graph (null otherwise)
  int bm_ext_words;                         // HBM-scratch class: words of the bitmaps at the head of a slice (0: LDS)
  int gs_chunk;                             // ... and how many slices there are (the class runs in chunks)
  int64_t list_offset;                      // first entry of the class list a launch works on
  const int64_t* x_cap;                     // one-hop plans: bound of the edges outside the hub's cache (-1: no hub)
  uint32_t* hub_slices;                     // link_hub_kernel's overflow class: found-edge list + columns per workgroup
  int64_t hub_slice_words;
  int hub_slice_grid;
  const uint16_t* csr_cnt;                  // induced-CSR flavour (s3grl_csr.hip): members per list entry,
  const int32_t* csr_e;                     // ... and per link
  int sop2;                                 // S3GRL_MODE_SOP_RESTRICTED: global normalisation, nothing masked (link_kernel)
};

// The link launches of a plan at sign_k K, largest subgraphs first; instantiated by s3grl_links_k*.hip
template <int K>
s3grl_status launch_links_k(s3grl_context* ctx, const LinkArgs& a, int64_t L, const int32_t* class_count_in);

}  // namespace s3grl
