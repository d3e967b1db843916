// Packed-row feature operand and its gather kernel, gfx950.
//
// The reference hands its operators a dense fp32 X, but the matrices it is run on are row-
// normalised bag-of-words / TF-IDF / one-hot rows (sgrl_link_pred.py:851,961-963): PubMed has
// ~50 non-zeros in 500 columns, Cora ~18 in 1433.  The dense gather (s3grl_gather.hip) is bound
// by the bytes it pulls through the fabric, and two thirds of its 16-byte lane loads fetch four
// zeros.  Here X is stored a second time with the all-zero 16-byte chunks squeezed out:
//
//   pk_hdr[tile][row] = { 128-bit mask of the non-zero chunks of the 512-column tile, offset }
//   pk_data           = one chunk of zeros, then the non-zero chunks in (tile, row, chunk) order
//
// The kernel is the dense one with a different fetch: a lane still OWNS chunk `lane` and chunk
// `64 + lane` of the tile and keeps their 2K accumulators in registers (no LDS, no atomics —
// the (column, value)-pair format of s3grl_features.hip lost to the dense kernel exactly there);
// the row's header arrives through the scalar cache (the row id is wave-uniform), the lane's
// chunk sits at offset + popcount(mask bits below the lane) = one v_mbcnt pair, and a lane whose
// mask bit is clear reads a shared chunk of zeros instead.  c·0 adds nothing, so the sums are the dense
// kernel's sums bit for bit.  PubMed: 33 % of the chunks are non-zero -> 0.7 KB instead of 2 KB
// per subgraph node.
//
// Beside them the features keep element rows (s3grl_features.hip: per tile and row its non-zeros as
// (value, slot) pairs, range in PackedHdr::el).  The rows beyond the prefix the leading operators reach
// feed the last operator only (PubMed K = 3: 83 % of the row visits); there the kernel accumulates in
// LDS by column and fetches a row as ONE 8-byte-per-lane load (50 entries: 400 B) instead of two
// 1-KiB chunk wave-loads — the texture addresser, not bytes, bounded those.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "s3grl_internal.hpp"
#include "s3grl_gather_common.hpp"

namespace s3grl {
namespace {


constexpr int kTile = 512;          // feature columns per tile = 128 chunks = 2 mask words
// one wavefront per workgroup: the jobs of a workgroup differ in length by an order of magnitude
// (positive vs negative links), and a workgroup holds its registers until its longest job is
// done.  Measured on PubMed K=3: 8 waves per workgroup 16.9 ms, 4: 13.6 ms, 2: 11.1 ms, 1: 10.7 ms.
constexpr int kWavesPerBlock = 1;
// pass2 of the packed gather (up to three operators): rows whose ids and coefficients are fetched by one set of
// vector loads (one row per lane) and staged in LDS, one record of kRecStride dwords per group of four rows
constexpr int kPrefixWindow = 64;
constexpr int kRecStride = 32;
constexpr int kStageDwords = kPrefixWindow / 4 * kRecStride + 64;   // + the read-ahead of a window's last step (64 lanes, unused)

__device__ __forceinline__ int below(uint64_t m) {   // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// chunk `j` of tile `tile` of row `row` of the dense X (rows 16-byte aligned, ld % 4 == 0,
// ld >= F rounded up to 4); columns >= F read as zero, whatever a borrowed X holds there
__device__ __forceinline__ float4_t dense_chunk(const float* __restrict__ X, int64_t ld, int F, int64_t row,
                                                int tile, int j) {
  const int col = tile * kTile + j * 4;
  if (col >= F) return (float4_t)(0.f);
  float4_t v = *reinterpret_cast<const float4_t*>(X + row * ld + col);
  if (col + 1 >= F) v.y = 0.f;
  if (col + 2 >= F) v.z = 0.f;
  if (col + 3 >= F) v.w = 0.f;
  return v;
}

__device__ __forceinline__ bool nonzero(float4_t v) {
  return v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f;
}

// one wave per (tile, row): number of non-zero chunks
__global__ __launch_bounds__(256) void pk_count_kernel(const float* __restrict__ X, int64_t ld, int F,
                                                       int64_t N, int tiles, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= N * tiles) return;
  const int tile = (int)(item / N);
  const int64_t row = item - (int64_t)tile * N;
  const uint64_t m0 = __ballot(nonzero(dense_chunk(X, ld, F, row, tile, lane)));
  const uint64_t m1 = __ballot(nonzero(dense_chunk(X, ld, F, row, tile, 64 + lane)));
  if (lane == 0) cnt[item] = __popcll(m0) + __popcll(m1);
}

__global__ __launch_bounds__(256) void pk_fill_kernel(const float* __restrict__ X, int64_t ld, int F,
                                                      int64_t N, int tiles, const int64_t* __restrict__ ptr,
                                                      PackedHdr* __restrict__ hdr,
                                                      float4_t* __restrict__ data) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= N * tiles) return;
  const int tile = (int)(item / N);
  const int64_t row = item - (int64_t)tile * N;
  const float4_t v0 = dense_chunk(X, ld, F, row, tile, lane);
  const float4_t v1 = dense_chunk(X, ld, F, row, tile, 64 + lane);
  const uint64_t m0 = __ballot(nonzero(v0));
  const uint64_t m1 = __ballot(nonzero(v1));
  const int64_t off = ptr[item] + 1;   // pk_data[0] is a chunk of zeros (what a masked-off lane loads)
  if (item == 0 && lane == 0) data[0] = (float4_t)(0.f);
  if ((m0 >> lane) & 1) data[off + below(m0)] = v0;
  if ((m1 >> lane) & 1) data[off + __popcll(m0) + below(m1)] = v1;
  if (lane == 0) {
    PackedHdr h;
    h.m0 = m0;
    h.m1 = m1;
    h.off = (uint64_t)off;
    h.el = 0;
    hdr[item] = h;
  }
}

// One wavefront owns one row pair and one 512-column tile; see the file comment.
//
// Schedule.  At 0.7 KB per row the kernel is no longer bound by bytes but by how well the chain
// id -> header -> chunk loads -> multiply-adds overlaps inside a wavefront.  It is software-
// pipelined by hand over groups of U = 4 rows with two register buffers: while the FMAs of group
// g run, the chunk loads of group g+1 are in flight and the ids/headers of group g+2 are on
// their way through the scalar cache.  For the compiler to wait for "all but the newest 2U
// loads" (vmcnt) rather than for all of them, the loads must not sit behind divergent branches:
// a lane whose mask bit is clear loads pk_data[0], a chunk of zeros (one line, L1-resident),
// chosen with one v_cndmask on the wave-uniform mask — so every load is unconditional.  The
// phases are kept apart with scheduling barriers; left alone, the compiler serialises the scalar
// loads (load, wait, use, load, wait, ...).
// Measured on PubMed PoS K=3 (164 000 links), step by step: no pipelining 17.8 ms; two buffers
// 14.4; skipping the operators that cannot reach a row 13.6; one wavefront per workgroup 10.8;
// jobs started largest first 9.7; two phases with a third buffer for the last-operator rows 8.2.
// What lost: U=2 x 4 buffers 16.6 ms (more scalar instructions per row); a third or fifth buffer
// for ALL rows 17.1 / 19.0 ms (156-250 VGPRs: fewer waves per SIMD, and the unrolled body
// outgrows the instruction cache); an XCD-contiguous job mapping 19 ms (load imbalance).
//
// Chunk fetch.  The unconditional form above (the kernel's first version) makes every lane of a
// wave-instruction fetch 16 bytes — a masked-off lane the shared chunk of zeros —
// so a row with a third of its chunks populated still pushes 2 x 1 KiB through the CU's texture
// path: 206 M wave-loads x 1 KiB per PubMed launch against a vector-L1 return path of 64 B/clk/CU
// is 6 of the kernel's 8 ms.  Here the chunks are read through a raw BUFFER descriptor over
// pk_data and a masked-off lane is given an offset beyond the buffer: the hardware's range check
// returns zeros for it without a memory request.  Still one unconditional, compiler-visible load
// per lane (no branches, vmcnt tracked by the compiler) — only populated chunks travel.
// (An EXEC-masked global_load in inline assembly does the same on paper; the compiler cannot know
// that such a load is still in flight when it copies or reuses the destination registers, and the
// kernel faulted at PubMed scale.)
typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));
constexpr uint32_t kOobOffset = 0x80000000u;   // >= any pk_data size (build_packed_rows keeps it below 2 GiB)

__device__ __forceinline__ uint32_t select_or_oob(uint64_t mask, uint32_t if_set, uint32_t oob) {
  uint32_t r;   // lane-wise: bit `lane` of the wave-uniform mask ? if_set : oob
  asm("v_cndmask_b32_e64 %0, %3, %1, %2" : "=v"(r) : "v"(if_set), "s"(mask), "v"(oob));
  return r;
}

// First list row of an element plan's phase B (gather_packed_kernel<K, 1, 3>), cnt if the job has none:
// jobs whose last operator alone reaches beyond the prefix (nb == 1), and whose list does not end inside
// phase A (groups [gA, ngf) non-empty).  The same arithmetic as the run<NB> choice of the kernel below.
template <int K>
__device__ __forceinline__ int el_phase_b_start(const int (&lim)[K], int cnt) {
  constexpr int U = 4;
  int nb = 1;
#pragma unroll
  for (int i = K - 2; i >= 0; --i)
    if (lim[i] == lim[K - 1] && nb == K - 1 - i) nb = K - i;
  if (nb != 1) return cnt;
  const int ngf = cnt / U;
  const int limA = K >= 2 ? lim[K >= 2 ? K - 2 : 0] : 0;
  const int gA = min(ngf, (limA + U - 1) / U);
  return gA < ngf ? gA * U : cnt;
}

typedef unsigned int uint2_t __attribute__((ext_vector_type(2)));

// Phase B of an element plan as a launch of its own, right behind phase A (EL == 2) on the same stream.
// Phase A left the last operator's sums over the prefix rows in that operator's output rows (primary
// copy); one wave per (job, tile) loads them into a float2 per column in LDS (rows a, b; slot =
// column-in-tile + 1), adds the rows [j0, cnt) of the list in list order — ds_read_b64, two multiply-adds,
// ds_write_b64 per entry, as the one-launch kernel did — and writes the finished rows, the label column
// and the mirror copy.  A stored and reloaded fp32 partial is exact: every column takes the same addends
// in the same order as on the chunk path, bit for bit.
// Why a launch of its own: the chain is latency-bound and wants waves; phase A holds all K operators'
// accumulators (121 VGPRs, four waves per SIMD) and phase B needs a few registers per row.  Here nothing
// of the chain waits on the scalar counter: a window of 64 rows has its ids, element ranges and
// coefficients fetched by VECTOR loads (lane j: row j of the window) and handed out with v_readlane, so the
// lgkmcnt waits of the chain are LDS-only, and the id -> range -> entries fetches are ordered by vmcnt.
template <int K>
__device__ __forceinline__ void el_phase_b(const Job* __restrict__ jobs, int njobs, const int32_t* __restrict__ c_ids,
                                           const float* __restrict__ c_coef, const float* __restrict__ job_z,
                                           const int32_t* __restrict__ job_lim, const int32_t* __restrict__ job_order,
                                           const PackedHdr* __restrict__ hdr, const ElemEntry* __restrict__ el,
                                           uint32_t el_bytes, int64_t N, const float* __restrict__ X, int64_t ldx,
                                           int F, float* __restrict__ rows_out, float* __restrict__ prows) {
  constexpr int CH = 2;
  constexpr int U = 4;    // rows per group
  constexpr int W = 64;   // rows per window (one per lane)
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (wid >= njobs) return;
  const int jid = __builtin_amdgcn_readfirstlane(job_order[wid]);   // longest jobs start first
  const Job job = jobs[jid];
  if (job.split == 1) return;
  const int cnt = __builtin_amdgcn_readfirstlane(job.support);
  int lim[K];
#pragma unroll
  for (int i = 0; i < K; ++i) lim[i] = __builtin_amdgcn_readfirstlane(job_lim[(int64_t)jid * K + i]);
  const int j0 = el_phase_b_start<K>(lim, cnt);
  if (j0 >= cnt) return;   // finished by phase A
  float* __restrict__ rows = job.split == 2 ? prows : rows_out;
  const int col0 = blockIdx.y * kTile;
  const int Fp = F + 1;
  const int64_t rstride = (int64_t)(K + 1) * Fp;
  const int nrow = job.node_b >= 0 ? 2 : 1;
  int coff[CH];
  bool cok[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    coff[c] = col0 + (lane + 64 * c) * 4;
    cok[c] = coff[c] < F;
  }
  float4_t acc[K][2][CH];   // only acc[K - 1] is used (the epilogue's signature)
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[i][r][c] = (float4_t)(0.f);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r >= nrow) break;
    const float* __restrict__ src = rows + (job.out_row + r) * rstride + (int64_t)K * Fp + 1;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (cok[c]) {
        const int nv = min(4, F - coff[c]);
        if (nv == 4) {
          acc[K - 1][r][c] = *reinterpret_cast<const float4_u*>(src + coff[c]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < nv) acc[K - 1][r][c][e] = src[coff[c] + e];
        }
      }
    }
  }
  __shared__ __attribute__((aligned(16))) float2 el_lds[2 + kTile];
  float2* const eacc = el_lds + 1;   // slot s at eacc[s]; slot 0 takes the zeros of lanes beyond a row's end
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) eacc[1 + (lane + 64 * c) * 4 + e] = make_float2(acc[K - 1][0][c][e], acc[K - 1][1][c][e]);
  __syncthreads();   // one wave per workgroup: orders nothing in hardware; keeps the compiler honest

  const uint32_t* __restrict__ uid = reinterpret_cast<const uint32_t*>(c_ids + job.ids_off);
  const float2* __restrict__ cq = reinterpret_cast<const float2*>(c_coef) + job.coef_off + (int64_t)(K - 1) * cnt;
  const PackedHdr* __restrict__ th = hdr + (int64_t)blockIdx.y * N;
  const __amdgpu_buffer_rsrc_t ersrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<ElemEntry*>(el), 0, (int)el_bytes, 0x00020000);
  const uint32_t oobv = kOobOffset;
  auto load_e = [&](uint32_t s, uint32_t k, uint32_t n) __attribute__((always_inline)) {   // entries k + lane of a row (k >= 64)
    const uint32_t a = (s + k + (uint32_t)lane) << 3;
    return __builtin_bit_cast(uint2_t, __builtin_amdgcn_raw_buffer_load_b64(
                                           ersrc, (int)(k + (uint32_t)lane < n ? a : oobv), 0, 0));
  };
  auto rmw = [&](uint2_t e, float qx, float qy) __attribute__((always_inline)) {
    float2 a = eacc[e.y];
    const float v = __builtin_bit_cast(float, e.x);
    a.x += qx * v;
    a.y += qy * v;
    eacc[e.y] = a;
  };
  // Two rows per load.  A wave-load costs the texture addresser little more at 16 bytes per lane than
  // at 8 (20 against 16.5 cycles on L2-resident rows), so the rows 2p, 2p + 1 of a group
  // share one: lanes 0-31 fetch the entries 2l, 2l + 1 of the first row, lanes 32-63 those of the second (an
  // element row starts 16-byte aligned and ends on an even entry: el_fill_kernel), a lane with 2l beyond its
  // row's count goes out of range.  Two v_permlane32_swap — value dwords, slot dwords — exchange the upper
  // half of the even entries with the lower half of the odd ones: the first row's entries across all 64 lanes,
  // then the second's, the operands of the read-modify-writes as one row per load handed them over.
  struct EBuf {
    uint4_t v[U / 2];   // rows 2p, 2p + 1 as loaded: this half-wave's row, entries 2l and 2l + 1 (value bits, slot)
    uint32_t s[U];      // first entry, entry count (wave-uniform)
    uint32_t n[U];
  };
  const bool hi = lane >= 32;
  const uint32_t l2 = (uint32_t)(lane & 31) * 2u;
  uint32_t idn = j0 + lane < cnt ? uid[j0 + lane] : 0u;   // ids of the first window
  for (int w0 = j0; w0 < cnt; w0 += W) {
    const int nw = min(W, cnt - w0);
    const bool mine = lane < nw;
    const uint64_t rg = mine ? th[idn].el : 0ull;   // lanes beyond the window: count 0
    const float2 q = mine ? cq[w0 + lane] : make_float2(0.f, 0.f);
    if (w0 + W + lane < cnt) idn = uid[w0 + W + lane];   // the next window's ids, under this window's rows
    const uint32_t es = (uint32_t)rg, en = (uint32_t)(rg >> 32);
    const int ng = (nw + U - 1) / U;
    // group g: rows g*U .. g*U+U-1 of the window; a row beyond it has count 0 (every lane out of range).
    // W and the phase's first row are even: a pair never straddles a window, an odd last row pairs with count 0.
    auto issue = [&](int g, EBuf& b) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = g * U + u;
        const int l = min(j, W - 1);
        b.s[u] = (uint32_t)__builtin_amdgcn_readlane((int)es, l);
        b.n[u] = j < W ? (uint32_t)__builtin_amdgcn_readlane((int)en, l) : 0u;
      }
#pragma unroll
      for (int p = 0; p < U / 2; ++p) {
        const uint32_t sp = hi ? b.s[2 * p + 1] : b.s[2 * p];
        const uint32_t np = hi ? b.n[2 * p + 1] : b.n[2 * p];
        b.v[p] = __builtin_bit_cast(uint4_t, __builtin_amdgcn_raw_buffer_load_b128(
                                                 ersrc, (int)(l2 < np ? (sp + l2) << 3 : oobv), 0, 0));
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    auto rmw_grp = [&](int g, const EBuf& b) __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < U / 2; ++p) {
        const auto ev = __builtin_amdgcn_permlane32_swap(b.v[p].x, b.v[p].z, false, false);   // values
        const auto sl = __builtin_amdgcn_permlane32_swap(b.v[p].y, b.v[p].w, false, false);   // slots
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int u = 2 * p + r;
          const int l = min(g * U + u, W - 1);
          const float qx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, q.x), l));
          const float qy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, q.y), l));
          uint2_t e;
          e.x = ev[r];
          e.y = sl[r];
          rmw(e, qx, qy);
          if (__builtin_expect(b.n[u] > 64, 0)) {
#pragma nounroll
            for (uint32_t k = 64; k < b.n[u]; k += 64)   // rows with more than 64 entries in the tile (kept rolled)
              rmw(load_e(b.s[u], k, b.n[u]), qx, qy);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    // two entry buffers: the loads of group g+1 are in flight under the read-modify-writes of group g
    EBuf bA, bB;
    issue(0, bA);
    for (int g = 0; g < ng; g += 2) {
      issue(g + 1, bB);
      rmw_grp(g, bA);
      if (g + 1 < ng) {
        issue(g + 2, bA);
        rmw_grp(g + 1, bB);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float2 a = eacc[1 + (lane + 64 * c) * 4 + e];
      acc[K - 1][0][c][e] = a.x;
      acc[K - 1][1][c][e] = a.y;
    }
  write_pair_rows_part<K, CH, K - 1, K, false, true>(job, jid, acc, coff, cok, job_z, X, ldx, F, rows,
                                                     blockIdx.y == 0);
}

// MINNB = 2: a plan whose last two operators reach the whole list in every job (sign_k - 1 >=
// num_hops): the variant that holds every operator's accumulators at once (NB = 1) is left out, and
// with it its registers — PubMed sign_k = 5: 128 instead of 166 VGPRs, four waves per SIMD.
// EL = 1: phase B (NB = 1) reads the element rows instead of the chunks (pass3e below); EL = 2: phase A of the
// same as two launches, EL = 3: their phase B (el_phase_b).
//
// Waves per SIMD the register allocation is held to: the instantiations that fit four waves (128 VGPRs) say
// so — left to itself the allocator renames a few accumulators inside the unrolled multiply-adds and lands
// just above the boundary (131-134 for the K = 3 kernels), which costs a quarter of the resident waves; the lean phase B
// (EL == 3) runs at eight.  The wider kernels (more operators' accumulators than fit) are left alone.
// The attribute is a bound the allocator MEETS, by spilling if it has to: <3,1,1> sits at 127 of 128 VGPRs, and
// a compiler that needs two more would put them in scratch without a word instead of dropping a wave.  After a
// compiler update, or a change to pass2, read the resource report (-Rpass-analysis=kernel-resource-usage):
// scratch must stay 0 for every instantiation (DESIGN Part II has the table).
template <int K, int MINNB, int EL>
constexpr int packed_min_waves() {
  return EL == 3 ? 8 : (K <= 3 || (MINNB == 2 && K <= 5)) ? 4 : 1;
}

template <int K, int MINNB, int EL>
__global__ __launch_bounds__(kWavesPerBlock * 64)
__attribute__((amdgpu_waves_per_eu(packed_min_waves<K, MINNB, EL>()))) void gather_packed_kernel(
    const Job* __restrict__ jobs, int njobs, const int32_t* __restrict__ c_ids,
    const float* __restrict__ c_coef, const float* __restrict__ job_z,
    const int32_t* __restrict__ job_lim, const int32_t* __restrict__ job_order,
    const PackedHdr* __restrict__ hdr,
    const float4_t* __restrict__ data, uint32_t data_bytes, const ElemEntry* __restrict__ el, uint32_t el_bytes,
    int64_t N, const float* __restrict__ X, int64_t ldx, int F, float* __restrict__ rows_out,
    float* __restrict__ prows) {
  if constexpr (EL == 3) {
    el_phase_b<K>(jobs, njobs, c_ids, c_coef, job_z, job_lim, job_order, hdr, el, el_bytes, N, X, ldx, F, rows_out,
                  prows);
    return;
  }
  constexpr int CH = 2;
  constexpr int U = 4;   // rows per group
  // phase A multiplies every operator over whole groups: up to U - 1 rows beyond the prefix, where the link
  // kernels still store the middle operators' zeros (coef_zero_end); beyond that nothing is written
  static_assert(U == kCoefGroup, "the link kernels' zero fill covers phase A's last group");
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (wid >= njobs) return;
  const int jid = __builtin_amdgcn_readfirstlane(job_order[wid]);   // longest jobs start first
  const int col0 = blockIdx.y * kTile;
  const Job job = jobs[jid];
  if (job.split == 1) return;   // gathered piece by piece (the entries with split == 2)
  float* __restrict__ rows = job.split == 2 ? prows : rows_out;   // a piece writes partial rows
  const int cnt = __builtin_amdgcn_readfirstlane(job.support);
  const uint32_t* __restrict__ uid = reinterpret_cast<const uint32_t*>(c_ids + job.ids_off);
  const float2* __restrict__ cf = reinterpret_cast<const float2*>(c_coef) + job.coef_off;
  const PackedHdr* __restrict__ th = hdr + (int64_t)blockIdx.y * N;
  // raw buffer over pk_data (dword 3 = 0x00020000: gfx9-family untyped 32-bit data format), stride 0:
  // an offset at or beyond data_bytes is out of range and reads as zero
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float4_t*>(data), 0, (int)data_bytes, 0x00020000);
  const uint32_t oobv = kOobOffset;
  // Operator i+1 has no non-zero coefficient at list positions >= lim[i] (a walk of i+1 steps
  // stays within i+1 hops, and the list is hop-major), lim non-decreasing: its multiply-adds are
  // skipped there.  On PubMed (3 hops, K = 3) four fifths of the rows only feed the last operator.
  int lim[K];
#pragma unroll
  for (int i = 0; i < K; ++i) lim[i] = __builtin_amdgcn_readfirstlane(job_lim[(int64_t)jid * K + i]);

  int coff[CH];
  bool cok[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    coff[c] = col0 + (lane + 64 * c) * 4;
    cok[c] = coff[c] < F;
  }
  float4_t acc[K][2][CH];
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[i][r][c] = (float4_t)(0.f);

  // a header through the scalar cache: the row id as a 32-bit byte offset on the uniform base (s_load with an
  // offset register: one shift per row instead of a 64-bit shift and add; build_packed_rows keeps N * 32 < 2^32)
  auto hdr_of = [&](uint32_t id) __attribute__((always_inline)) -> PackedHdr {
    static_assert(sizeof(PackedHdr) == 32, "the shift below");
    return *reinterpret_cast<const PackedHdr*>(reinterpret_cast<const char*>(th) + (id << 5));
  };
  auto load_hdrs = [&](int g, PackedHdr(&h)[U]) __attribute__((always_inline)) {   // scalar: ids (one wide load), then headers
    uint32_t id[U];
#pragma unroll
    for (int u = 0; u < U; ++u) id[u] = uid[g * U + u];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) h[u] = hdr_of(id[u]);
    __builtin_amdgcn_sched_barrier(0);
  };
  // the same in two halves for the steady-state loops: the ids of a group are fetched one step
  // before its headers, so that no step waits for a scalar round trip it has just started
  auto load_ids = [&](int g, uint32_t(&id)[U]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) id[u] = uid[g * U + u];
    __builtin_amdgcn_sched_barrier(0);
  };
  auto hdrs_from = [&](const uint32_t(&id)[U], PackedHdr(&h)[U]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) h[u] = hdr_of(id[u]);
    __builtin_amdgcn_sched_barrier(0);
  };
  // phase B's form: the ids pass through an opaque statement — without it the header addresses
  // (plain arithmetic on the ids) are computed right behind the id load of the step before, and
  // the wait moves there with them
  auto hdrs_from_late = [&](const uint32_t(&id)[U], PackedHdr(&h)[U]) __attribute__((always_inline)) {
    uint32_t idv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) idv[u] = id[u];
    asm volatile("" : "+s"(idv[0]), "+s"(idv[1]), "+s"(idv[2]), "+s"(idv[3]));
    static_assert(U == 4, "the opaque statement above lists four ids");
#pragma unroll
    for (int u = 0; u < U; ++u) h[u] = hdr_of(idv[u]);
    __builtin_amdgcn_sched_barrier(0);
  };
  // (valid = false: a group beyond the end of the list — every lane reads as zero)
  auto issue = [&](const PackedHdr(&h)[U], float4_t(&v)[U][CH], bool valid = true) __attribute__((always_inline)) {   // 2U unconditional loads
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // a group beyond the end gets a base whose every chunk address is out of range (one scalar select
      // per row instead of one per mask word)
      const uint32_t base = valid ? (uint32_t)h[u].off : (kOobOffset >> 4);
      const uint32_t a0 = (base + (uint32_t)below(h[u].m0)) << 4;
      const uint32_t a1 = (base + (uint32_t)__popcll(h[u].m0) + (uint32_t)below(h[u].m1)) << 4;
      v[u][0] = __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(
                                                 rsrc, (int)select_or_oob(h[u].m0, a0, oobv), 0, 0));
      v[u][1] = __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(
                                                 rsrc, (int)select_or_oob(h[u].m1, a1, oobv), 0, 0));
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto fma_from = [&](auto first, auto last, int g, const float4_t(&v)[U][CH]) __attribute__((always_inline)) {   // operators first+1 .. last
    constexpr int I0 = decltype(first)::value, I1 = decltype(last)::value;
#pragma unroll
    for (int i = I0; i < I1; ++i) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float2 q = cf[(int64_t)i * cnt + g * U + u];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          acc[i][0][c] += q.x * v[u][c];
          acc[i][1][c] += q.y * v[u][c];
        }
      }
    }
  };
  // Two phases.  The last NB operators all reach the whole list (lim[K-NB .. K-1] == cnt; NB = 1 when
  // sign_k - 1 < num_hops, more when the operators outrun the BFS depth; capped at 3).  A: the list
  // prefix the operators before them can reach (rows < lim[K-NB-1]), all accumulators live, two
  // chunk buffers.  Then the rows of operators 1..K-NB are complete and are written out, which
  // frees their accumulator registers.  B: the rest of the list feeds the last NB operators only;
  // with NB = 1 the freed registers hold a third chunk buffer (8 rows in flight under the
  // multiply-adds of 4), with NB = 2, 3 the rows do 2 or 3 operators' multiply-adds instead of K
  // (PubMed sign_k = 5: four fifths of the rows, 3 operators instead of 5).
  auto tail_rows = [&](auto first, auto last, int j0) __attribute__((always_inline)) {   // at most U-1 rows, operators first+1 .. last
    constexpr int I0 = decltype(first)::value, I1 = decltype(last)::value;
    for (int j = j0; j < cnt; ++j) {
      const PackedHdr h = hdr_of(uid[j]);
      const uint32_t base = (uint32_t)h.off;
      const uint32_t a0 = (base + (uint32_t)below(h.m0)) << 4;
      const uint32_t a1 = (base + (uint32_t)__popcll(h.m0) + (uint32_t)below(h.m1)) << 4;
      float4_t v[CH];
      v[0] = __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(
                                              rsrc, (int)select_or_oob(h.m0, a0, oobv), 0, 0));
      v[1] = __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(
                                              rsrc, (int)select_or_oob(h.m1, a1, oobv), 0, 0));
#pragma unroll
      for (int i = I0; i < I1; ++i) {
        const float2 q = cf[(int64_t)i * cnt + j];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          acc[i][0][c] += q.x * v[c];
          acc[i][1][c] += q.y * v[c];
        }
      }
    }
  };

  // Groups [g0, g1) through two chunk buffers, operators first+1 .. last.
  //
  // Up to 3 operators (every pass2 of the sign_k <= 3 plans and of the MINNB = 2 kernels up to sign_k = 5):
  // nothing cold on the per-step scalar chain.  The ids and coefficient lists were written by the link
  // kernels a phase earlier and come from HBM; as scalar loads they put one HBM round trip into every
  // half-step (a wave waits for ALL its scalar loads).  Here a window of kPrefixWindow rows is fetched by
  // vector loads — lane j: the coefficients of row j of the window and the id of the row two groups further
  // on — and laid out in LDS as one record per group: dwords 0..3 the ids of group g+2, then q.x, q.y per
  // (operator, row) of group g.  A half-step reads its record with ONE ds_read_b32 (lane l: dword l), a
  // half-step before it is used, and hands the values out with v_readlane.  The headers stay on the scalar
  // path (the table is L2-resident), requested right behind the chunk loads that consumed the previous ones,
  // so that the one wait of a half-step — at the top of the next one — is for loads that had the
  // multiply-adds to arrive: one header buffer instead of two.  The multiply-adds are the former ones,
  // operand for operand.
  __shared__ __attribute__((aligned(16))) float2 el_lds[EL == 1 || EL == 2 ? 2 + kTile : kStageDwords / 2];
  static_assert(2 * (2 + kTile) >= kStageDwords, "the staging records share the element accumulators' LDS");
  uint32_t* const stage = reinterpret_cast<uint32_t*>(el_lds);
  auto pass2 = [&](auto first, auto last, int g0, int g1) __attribute__((always_inline)) {
    constexpr int I0 = decltype(first)::value;
    constexpr int NO_RAW = decltype(last)::value - I0;
    constexpr int NO = NO_RAW > 0 ? NO_RAW : 1;   // (an empty operator range, NB == K: nothing to do)
    if (NO_RAW <= 0) return;
    if (g1 <= g0) return;
    int g = g0;
    if constexpr (NO <= 3) {
      static_assert(4 + 2 * U * 3 <= kRecStride && kRecStride <= 64, "a record is one dword per lane");
      constexpr int WG = kPrefixWindow / U;   // groups per window
      PackedHdr h[U];
      float4_t vA[U][CH], vB[U][CH];
      uint32_t rec;
      // records 0 .. WG-1 of the window whose first group is gw.  The loads stop at the pass's own last row
      // (lanes beyond it repeat that row's address, and their records are never used): what the rows after
      // g1 * U need is fetched by the pass that covers them, once — gather_traffic_kernel counts on it.
      const int rlast = g1 * U - 1;   // (g1 <= cnt / U: inside the list)
      auto fill = [&](int gw) __attribute__((always_inline)) {
        // (wave-uniform bases and one 32-bit lane offset: no 64-bit lane addresses live across the loop)
        const int r0 = gw * U;
        const uint32_t oq = (uint32_t)min(lane, rlast - r0);
        const uint32_t oi = (uint32_t)min(lane + 2 * U, rlast - r0);
        const uint32_t idv = (uid + r0)[oi];
        float2 qv[NO];
#pragma unroll
        for (int i = 0; i < NO; ++i) qv[i] = (cf + ((int64_t)(I0 + i) * cnt + r0))[oq];
        __syncthreads();   // one wave per workgroup: orders nothing in hardware; keeps the compiler honest
        int ll = lane;   // (opaque: the write addresses are computed here, not kept live across the loop)
        asm volatile("" : "+v"(ll));
        uint32_t* const r = stage + (ll >> 2) * kRecStride;
        r[ll & 3] = idv;
#pragma unroll
        for (int i = 0; i < NO; ++i)
          *reinterpret_cast<uint2_t*>(r + 4 + (i * U + (ll & 3)) * 2) =
              uint2_t{__builtin_bit_cast(uint32_t, qv[i].x), __builtin_bit_cast(uint32_t, qv[i].y)};
        __syncthreads();
        rec = stage[lane];
        __builtin_amdgcn_sched_barrier(0);
      };
      auto ids_at = [&](uint32_t r, int l0, uint32_t(&id)[U]) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < U; ++u) id[u] = (uint32_t)__builtin_amdgcn_readlane((int)r, l0 + u);
      };
      auto q_of = [&](float2(&qa)[NO][U]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NO; ++i)
#pragma unroll
          for (int u = 0; u < U; ++u) {
            qa[i][u].x = __builtin_bit_cast(float, __builtin_amdgcn_readlane((int)rec, 4 + (i * U + u) * 2));
            qa[i][u].y = __builtin_bit_cast(float, __builtin_amdgcn_readlane((int)rec, 5 + (i * U + u) * 2));
          }
      };
      // (row by row, the order the chunk loads arrive in; per accumulator the addends keep their order)
      auto fma_rec = [&](const float2(&qa)[NO][U], const float4_t(&v)[U][CH]) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int i = 0; i < NO; ++i)
#pragma unroll
            for (int c = 0; c < CH; ++c) {
              acc[I0 + i][0][c] += qa[i][u].x * v[u][c];
              acc[I0 + i][1][c] += qa[i][u].y * v[u][c];
            }
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      // rec = the record of group gq, h = the headers of group gq+1: chunk loads of gq+1 into vi, headers of
      // gq+2, the record at snext, multiply-adds of gq from vf
      auto half = [&](int snext, float4_t(&vi)[U][CH], bool valid, const float4_t(&vf)[U][CH]) __attribute__((always_inline)) {
        issue(h, vi, valid);
        uint32_t id[U];
        float2 qa[NO][U];
        ids_at(rec, 0, id);
        q_of(qa);
        __builtin_amdgcn_sched_barrier(0);
        hdrs_from(id, h);
        rec = stage[snext * kRecStride + lane];
        __builtin_amdgcn_sched_barrier(0);
        fma_rec(qa, vf);
      };
      {
        // the ids of the first two groups straight from a vector register (lanes 0 .. 2U-1: the rows the
        // window's own id load, which starts two groups further on, leaves out — no id is fetched twice)
        const uint32_t id0v = (uid + g0 * U)[(uint32_t)min(lane, min(2 * U - 1, rlast - g0 * U))];
        fill(g0);
        uint32_t id[U];
        ids_at(id0v, 0, id);
        hdrs_from(id, h);
        issue(h, vA);
        ids_at(id0v, U, id);
        hdrs_from(id, h);
      }
      // at the top: vA = group g in flight, h = headers of group g+1, rec = record s of the window = group g
      int s = 0;
      for (; g + 1 < g1; g += 2) {
        if (s == WG) {
          fill(g);
          s = 0;
        }
        half(s + 1, vB, true, vA);
        half(s + 2, vA, g + 2 < g1, vB);   // (record WG: spare, never used)
        s += 2;
      }
      if (g < g1) {
        if (s == WG) fill(g);
        float2 qa[NO][U];
        q_of(qa);
        __builtin_amdgcn_sched_barrier(0);
        fma_rec(qa, vA);
      }
    } else {
      // four operators and more (sign_k >= 4 plans deeper than their operators): the scalar schedule.  The
      // coefficients of a group are loaded where they are used; 2 x 5 x U of them beside the headers measured
      // 6 % slower when they were all requested ahead.
      PackedHdr hA[U], hB[U];
      float4_t vA[U][CH], vB[U][CH];
      uint32_t idn[U];
      load_hdrs(g0, hA);
      issue(hA, vA);
      if (g1 - g0 > 1) load_hdrs(g0 + 1, hB);
      if (g1 - g0 > 2) load_ids(g0 + 2, idn);
      // steady state: vA = group g in flight, hB = headers of group g+1, idn = ids of group g+2
      auto fma_g = [&](int gq, const float4_t(&v)[U][CH]) {
        fma_from(first, last, gq, v);
        __builtin_amdgcn_sched_barrier(0);
      };
      for (; g + 4 < g1; g += 2) {
        issue(hB, vB);
        hdrs_from(idn, hA);
        load_ids(g + 3, idn);
        fma_g(g, vA);
        issue(hA, vA);
        hdrs_from(idn, hB);
        load_ids(g + 4, idn);
        fma_g(g + 1, vB);
      }
      fma_g(g, vA);
      ++g;
      for (; g < g1; ++g) {   // at most 3 groups
        load_hdrs(g, hA);
        issue(hA, vA);
        fma_g(g, vA);
      }
    }
  };

  // Groups [g0, g1) through three chunk buffers, the last operator only.
  // Every scalar load is issued a whole step before its first use.  A wavefront can only wait for
  // ALL of its outstanding scalar loads (they return out of order: lgkmcnt(0)), so a step that loads
  // ids, then headers through them, then coefficients at the multiply-adds exposes two scalar round
  // trips (~800 cycles each through the scalar cache to L2) with four waves per SIMD to cover them
  // — that, not bytes or cache misses, was two thirds of a step (with the whole operand resident in
  // L2 the kernel ran 4 % faster).  Step k multiplies group k; at its top the ids of group k+3, the
  // headers of k+2 and the coefficients of k are complete (loaded during step k-1): it loads the
  // headers of k+3, the ids of k+4 and the coefficients of k+1, issues the chunk loads of k+2 and
  // multiplies.  One wait per step, for loads that had a step to arrive.  Scalar buffers alternate
  // (X/Y), chunk buffers rotate over three: six steps per trip.  Groups beyond the end are clamped
  // to the last one and their chunk loads read as zero (out-of-range offsets): the multiply-adds
  // stay unconditional — behind a branch the compiler sinks the scalar loads to their use.
  auto pass3 = [&](int g0, int g1) __attribute__((always_inline)) {
    const int nB = g1 - g0;
    if (nB <= 0) return;
    auto grp = [&](int k) { return g0 + min(k, nB - 1); };
    uint32_t idX[U], idY[U];
    PackedHdr hX[U], hY[U];
    float2 qX[U], qY[U];
    float4_t v0[U][CH], v1[U][CH], v2[U][CH];
    auto load_q = [&](int g, float2(&q)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) q[u] = cf[(int64_t)(K - 1) * cnt + g * U + u];
      __builtin_amdgcn_sched_barrier(0);
    };
    auto fma_q = [&](const float2(&q)[U], const float4_t(&v)[U][CH]) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          acc[K - 1][0][c] += q[u].x * v[u][c];
          acc[K - 1][1][c] += q[u].y * v[u][c];
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    load_ids(grp(0), idX);
    hdrs_from(idX, hX);
    issue(hX, v0);
    load_ids(grp(1), idX);
    hdrs_from(idX, hY);
    issue(hY, v1, 1 < nB);
    load_ids(grp(2), idX);
    hdrs_from(idX, hX);    // headers of group 2
    load_ids(grp(3), idX);   // ids of group 3
    load_q(grp(0), qX);
#define S3GRL_GATHER_STEP(k, IDr, IDl, Hr, Hl, Qr, Ql, Vissue, Vfma) \
  hdrs_from_late(IDr, Hl);                                            \
  load_ids(grp((k) + 4), IDl);                                        \
  load_q(grp((k) + 1), Ql);                                           \
  issue(Hr, Vissue, (k) + 2 < nB);                                    \
  fma_q(Qr, Vfma);
    for (int k = 0; k < nB; k += 6) {
      S3GRL_GATHER_STEP(k, idX, idY, hX, hY, qX, qY, v2, v0)
      S3GRL_GATHER_STEP(k + 1, idY, idX, hY, hX, qY, qX, v0, v1)
      S3GRL_GATHER_STEP(k + 2, idX, idY, hX, hY, qX, qY, v1, v2)
      S3GRL_GATHER_STEP(k + 3, idY, idX, hY, hX, qY, qX, v2, v0)
      S3GRL_GATHER_STEP(k + 4, idX, idY, hX, hY, qX, qY, v0, v1)
      S3GRL_GATHER_STEP(k + 5, idY, idX, hY, hX, qY, qX, v1, v2)
    }
#undef S3GRL_GATHER_STEP
  };

  // Phase B on the element rows (EL == 1; with EL == 2 only for jobs whose list ends inside phase A, the
  // longer phase B being el_phase_b's).  The last operator's accumulators move from the lanes' registers
  // into a float2 per column in LDS (rows a, b), slot = column-in-tile + 1; a row of the list is then
  // ONE 8-byte-per-lane load of its (slot, value) entries (s3grl_features.hip, el_fill_kernel) instead of
  // two 16-byte-per-lane chunk loads, and each lane adds its entry into its column's slot: ds_read_b64,
  // two multiply-adds, ds_write_b64.  A lane beyond the row's end gets an out-of-range offset, reads
  // {slot 0, 0} and adds zero into the spare slot 0 (every such lane writes back the value they all
  // read).  The slots of one row are distinct, and one wave's LDS operations execute in order, so every
  // column takes its addends in list order with the register path's multiply-adds (a skipped zero adds
  // nothing: the sums never hold -0): the sums are the chunk path's bit for bit.  Rows with more than 64
  // entries in the tile take further loads, in order, before the next row.
  // The schedule is pass3's: three entry buffers (2 VGPRs per row), scalar loads a step ahead.
  // (el_lds: declared above pass2, whose staging records it holds while a pass2 runs)
  float2* const eacc = el_lds + 1;   // slot s at eacc[s]: the column slots 1.. start 16-byte aligned
  const __amdgpu_buffer_rsrc_t ersrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<ElemEntry*>(el), 0, (int)el_bytes, 0x00020000);
  struct EBuf {
    uint2_t e[U];     // this lane's entry of each row (value bits, slot)
    uint32_t s[U];    // first entry, entry count (wave-uniform)
    uint32_t n[U];
  };
  auto issue_e = [&](const PackedHdr(&h)[U], EBuf& b, bool valid) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      b.s[u] = (uint32_t)h[u].el;
      b.n[u] = valid ? (uint32_t)(h[u].el >> 32) : 0u;
      const uint32_t a = (b.s[u] + (uint32_t)lane) << 3;
      b.e[u] = __builtin_bit_cast(uint2_t, __builtin_amdgcn_raw_buffer_load_b64(
                                               ersrc, (int)((uint32_t)lane < b.n[u] ? a : oobv), 0, 0));
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto rmw = [&](uint2_t e, float2 q) __attribute__((always_inline)) {
    float2 a = eacc[e.y];
    const float v = __builtin_bit_cast(float, e.x);
    a.x += q.x * v;
    a.y += q.y * v;
    eacc[e.y] = a;
  };
  auto rmw_row = [&](uint2_t e, uint32_t s, uint32_t n, float2 q) __attribute__((always_inline)) {
    rmw(e, q);
    if (__builtin_expect(n <= 64, 1)) return;
#pragma nounroll
    for (uint32_t k = 64; k < n; k += 64) {   // rows with more than 64 entries in the tile (kept rolled: code size)
      const uint32_t a = (s + k + (uint32_t)lane) << 3;
      const uint2_t t = __builtin_bit_cast(uint2_t, __builtin_amdgcn_raw_buffer_load_b64(
                                                        ersrc, (int)(k + (uint32_t)lane < n ? a : oobv), 0, 0));
      rmw(t, q);
    }
  };
  auto pass3e = [&](int g0, int g1) __attribute__((always_inline)) {
    const int nB = g1 - g0;
    if (nB <= 0) return;
    auto grp = [&](int k) { return g0 + min(k, nB - 1); };
    uint32_t idX[U], idY[U];
    PackedHdr hX[U], hY[U];
    float2 qX[U], qY[U];
    EBuf v0, v1, v2;
    auto load_q = [&](int g, float2(&q)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) q[u] = cf[(int64_t)(K - 1) * cnt + g * U + u];
      __builtin_amdgcn_sched_barrier(0);
    };
    auto rmw_q = [&](const float2(&q)[U], const EBuf& b) {
#pragma unroll
      for (int u = 0; u < U; ++u) rmw_row(b.e[u], b.s[u], b.n[u], q[u]);
      __builtin_amdgcn_sched_barrier(0);
    };
    load_ids(grp(0), idX);
    hdrs_from(idX, hX);
    issue_e(hX, v0, true);
    load_ids(grp(1), idX);
    hdrs_from(idX, hY);
    issue_e(hY, v1, 1 < nB);
    load_ids(grp(2), idX);
    hdrs_from(idX, hX);    // headers of group 2
    load_ids(grp(3), idX);   // ids of group 3
    load_q(grp(0), qX);
#define S3GRL_GATHER_STEP(k, IDr, IDl, Hr, Hl, Qr, Ql, Vissue, Vrmw) \
  hdrs_from_late(IDr, Hl);                                            \
  load_ids(grp((k) + 4), IDl);                                        \
  load_q(grp((k) + 1), Ql);                                           \
  issue_e(Hr, Vissue, (k) + 2 < nB);                                  \
  if ((k) < nB) rmw_q(Qr, Vrmw);   /* (a group beyond the end would only add zeros into slot 0) */
    for (int k = 0; k < nB; k += 6) {
      S3GRL_GATHER_STEP(k, idX, idY, hX, hY, qX, qY, v2, v0)
      S3GRL_GATHER_STEP(k + 1, idY, idX, hY, hX, qY, qX, v0, v1)
      S3GRL_GATHER_STEP(k + 2, idX, idY, hX, hY, qX, qY, v1, v2)
      S3GRL_GATHER_STEP(k + 3, idY, idX, hY, hX, qY, qX, v2, v0)
      S3GRL_GATHER_STEP(k + 4, idX, idY, hX, hY, qX, qY, v0, v1)
      S3GRL_GATHER_STEP(k + 5, idY, idX, hY, hX, qY, qX, v1, v2)
    }
#undef S3GRL_GATHER_STEP
  };
  auto tail_rows_e = [&](int j0) __attribute__((always_inline)) {   // at most U-1 rows, the last operator
    for (int j = j0; j < cnt; ++j) {
      const PackedHdr h = hdr_of(uid[j]);
      const uint32_t es = (uint32_t)h.el, en = (uint32_t)(h.el >> 32);
      const uint2_t e = __builtin_bit_cast(uint2_t, __builtin_amdgcn_raw_buffer_load_b64(
                                                        ersrc, (int)((uint32_t)lane < en ? (es + (uint32_t)lane) << 3 : oobv), 0, 0));
      rmw_row(e, es, en, cf[(int64_t)(K - 1) * cnt + j]);
    }
  };
  // registers <-> LDS: lane's float4 c covers columns (lane + 64 c) * 4 .. + 3 of the tile
  auto acc_to_lds = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) eacc[1 + (lane + 64 * c) * 4 + e] = make_float2(acc[K - 1][0][c][e], acc[K - 1][1][c][e]);
    __syncthreads();   // one wave per workgroup: orders nothing in hardware; keeps the compiler honest
  };
  auto lds_to_acc = [&]() __attribute__((always_inline)) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float2 a = eacc[1 + (lane + 64 * c) * 4 + e];
        acc[K - 1][0][c][e] = a.x;
        acc[K - 1][1][c][e] = a.y;
      }
  };

  const int ngf = cnt / U;   // full groups
  auto run = [&](auto nb_c) __attribute__((always_inline)) {
    constexpr int NB = decltype(nb_c)::value;   // trailing operators that reach the whole list
    using IC0 = std::integral_constant<int, 0>;
    using ICS = std::integral_constant<int, K - NB>;   // first trailing operator
    using ICK = std::integral_constant<int, K>;
    const int limA = NB < K ? lim[NB < K ? K - NB - 1 : 0] : 0;
    const int gA = min(ngf, (limA + U - 1) / U);       // groups [0, gA): the prefix the leading operators reach
    const bool tail_in_A = limA > ngf * U;
    if constexpr (NB == 1) {
      // A: every operator on the prefix; B: the last operator on the rest through three chunk buffers
      pass2(IC0{}, ICK{}, 0, gA);
      if (tail_in_A) tail_rows(IC0{}, ICK{}, ngf * U);
      write_pair_rows_part<K, CH, 0, K - NB, true, false>(job, jid, acc, coff, cok, job_z, X, ldx, F, rows,
                                                          blockIdx.y == 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (EL == 2) {
        if (gA < ngf) {
          // the phase-B launch (EL == 3) finishes this job: the last operator's sums over the prefix go to
          // where its rows will be (primary copy; no label column yet), exact as fp32
          Job jp = job;
          jp.mirror_row = -1;
          write_pair_rows_part<K, CH, K - 1, K, false, false>(jp, jid, acc, coff, cok, job_z, X, ldx, F, rows,
                                                              false);
          return;
        }
        acc_to_lds();
        if (!tail_in_A) tail_rows_e(ngf * U);
        lds_to_acc();
      } else if constexpr (EL == 1) {
        acc_to_lds();
        pass3e(gA, ngf);
        if (!tail_in_A) tail_rows_e(ngf * U);
        lds_to_acc();
      } else {
        pass3(gA, ngf);
        if (!tail_in_A) tail_rows(ICS{}, ICK{}, ngf * U);
      }
    } else {
      // A: the LEADING operators only, on the prefix; B: the trailing ones on the WHOLE list (the
      // prefix rows are fetched twice — a fifth more row loads on PubMed sign_k = 5 — but no phase
      // holds more than max(K-NB, NB) operators' accumulators: 128 instead of 166 VGPRs there,
      // four waves per SIMD instead of three)
      pass2(IC0{}, ICS{}, 0, gA);
      if (tail_in_A) tail_rows(IC0{}, ICS{}, ngf * U);
      write_pair_rows_part<K, CH, 0, K - NB, true, false>(job, jid, acc, coff, cok, job_z, X, ldx, F, rows,
                                                          blockIdx.y == 0);
      __builtin_amdgcn_sched_barrier(0);
      pass2(ICS{}, ICK{}, 0, ngf);
      tail_rows(ICS{}, ICK{}, ngf * U);
    }
    write_pair_rows_part<K, CH, K - NB, K, false, true>(job, jid, acc, coff, cok, job_z, X, ldx, F, rows,
                                                        blockIdx.y == 0);
  };
  int nb = 1;
#pragma unroll
  for (int i = K - 2; i >= 0; --i)
    if (lim[i] == lim[K - 1] && nb == K - 1 - i) nb = K - i;
  if constexpr (K >= 3) {
    if (nb >= 3) return run(std::integral_constant<int, 3>{});
  }
  if constexpr (K >= 2) {
    if (nb >= 2 || MINNB >= 2) return run(std::integral_constant<int, 2>{});
  }
  // (NB never exceeds the job's own count of trailing operators that reach the whole list: a trailing
  // operator is multiplied over ALL rows, and the link kernels write a middle operator's zeros only up to
  // coef_zero_end.  MINNB >= 2 is chosen for plans with sign_k - 1 >= depth, where lim[K-2] == lim[K-1] in
  // every job: the last level end is the support.  A SMALLER NB than the job's is always right — phase A
  // then covers rows that every operator reaches)
  if constexpr (MINNB <= 1 || K < 2) run(std::integral_constant<int, 1>{});
}

// Measurement only (s3grl_plan_gather_traffic): the bytes the gather launch of a plan requests,
// summed exactly over its jobs with the same phase arithmetic the kernels use (element rows: 8 bytes
// per entry in an nb == 1 job's phase B, a row of up to 64 entries in el_phase_b rounded up to whole pairs; phase B as a launch of its own: 8 bytes of the row's header, the job
// read twice, the partial rows written and read back).  One wavefront per
// job; out[0..7] as documented in include/s3grl.h.
__global__ __launch_bounds__(256) void gather_traffic_kernel(
    const Job* __restrict__ jobs, int njobs, const int32_t* __restrict__ c_ids,
    const int32_t* __restrict__ job_lim, int K, int packed, int elements, const PackedHdr* __restrict__ hdr,
    int64_t N, int F, int pieces, unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int jid = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (jid >= njobs) return;
  const Job job = jobs[jid];
  if (job.split == 1) {   // gathered piece by piece; the combine step writes its rows (and reads X for operator 0)
    if (lane == 0) {
      const unsigned long long nr = (job.node_b >= 0 ? 2 : 1) * (job.mirror_row >= 0 ? 2 : 1);
      atomicAdd(&out[4], 4ull * nr * (K + 1) * (unsigned long long)(F + 1));
      atomicAdd(&out[5], 16ull * ((F + 3) / 4) * (job.node_b >= 0 ? 2 : 1));
    }
    return;
  }
  const int cnt = job.support;
  const int32_t* __restrict__ ids = c_ids + job.ids_off;
  const int tile_cols = packed ? kTile : (F <= 256 ? 256 : 512);
  const int tiles = (F + tile_cols - 1) / tile_cols;
  const unsigned long long chunks_row = (unsigned long long)((F + 3) / 4);   // 16-byte loads inside a row
  // phase arithmetic of gather_packed_kernel: nb trailing operators reach the whole list; with nb >= 2
  // the nA rows of the prefix are fetched twice (leading operators, then trailing ones)
  int nb = 1, nA = 0;
  if (packed) {
    constexpr int U = 4;
    const int ngf = cnt / U;
    for (int i = K - 2; i >= 0; --i)
      if (job_lim[(int64_t)jid * K + i] == job_lim[(int64_t)jid * K + K - 1] && nb == K - 1 - i) nb = K - i;
    nb = min(nb, 3);
    const int limA = nb < K ? job_lim[(int64_t)jid * K + (K - nb - 1)] : 0;
    const int gA = min(ngf, (limA + U - 1) / U);
    const bool tail_in_A = limA > ngf * U;
    nA = tail_in_A ? cnt : gA * U;
  }
  const int twice = (packed && nb >= 2) ? nA : 0;
  // phase B of an nb == 1 job on element rows: 8 bytes per entry instead of 16 per chunk
  const int el_from = (packed && elements && nb == 1) ? nA : cnt;
  // ... and as a launch of its own (elements == 2, el_phase_b) when the list goes on beyond phase A: it
  // re-reads the job, fetches 8 bytes of each row's header (the element range), reads back the partial rows
  const bool split_b = elements == 2 && el_from < cnt / 4 * 4;   // (groups [gA, ngf) non-empty: el_phase_b_start)
  unsigned long long feat = 0;
  if (packed) {
    for (int j = lane; j < cnt; j += 64) {
      const int id = ids[j];
      for (int t = 0; t < tiles; ++t) {
        const PackedHdr h = hdr[(int64_t)t * N + id];
        const unsigned long long en = h.el >> 32;   // split phase B: rows of up to 64 entries come as whole pairs
        feat += j >= el_from ? 8ull * (split_b && en <= 64 ? (en + 1) & ~1ull : en)
                             : (j < twice ? 32ull : 16ull) * (unsigned long long)(__popcll(h.m0) + __popcll(h.m1));
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) feat += __shfl_xor(feat, o);
  } else {
    feat = 16ull * chunks_row * (unsigned long long)cnt;
  }
  if (lane != 0) return;
  // coefficient entries read per tile: nb == 1: every operator on the prefix, the last one beyond it;
  // nb >= 2: the leading operators on the prefix, the trailing ones everywhere; dense kernel: all K
  unsigned long long coef_entries = (unsigned long long)K * cnt;
  if (packed)
    coef_entries = nb == 1 ? (unsigned long long)K * nA + (unsigned long long)(cnt - nA)
                           : (unsigned long long)(K - nb) * nA + (unsigned long long)nb * cnt;
  const int nrow = job.node_b >= 0 ? 2 : 1;
  const int ncopy = job.mirror_row >= 0 ? 2 : 1;
  atomicAdd(&out[0], 4ull * (cnt + twice) * tiles);
  atomicAdd(&out[1], packed ? (split_b ? 32ull * el_from + 8ull * (cnt - el_from) : 32ull * (cnt + twice)) * tiles
                            : 0ull);
  atomicAdd(&out[2], feat);
  atomicAdd(&out[3], 8ull * coef_entries * tiles);
  const unsigned long long partial = split_b ? 4ull * nrow * (unsigned long long)F : 0ull;   // phase A -> phase B
  atomicAdd(&out[4], 4ull * nrow * ncopy * (K + 1) * (unsigned long long)(F + 1) + partial);
  // a piece's partial rows are read back once by the combine step
  atomicAdd(&out[5], 16ull * chunks_row * nrow + (pieces ? 4ull * nrow * (K + 1) * (unsigned long long)(F + 1) : 0ull) +
                         partial);
  atomicAdd(&out[6], (unsigned long long)tiles * (sizeof(Job) + 4ull * K + 4ull) * (split_b ? 2ull : 1ull) + 8ull * K);
  atomicAdd(&out[7], (unsigned long long)tiles);
}

// Element rows serve the one-operator phase B of a plan (0: they do not); 1: inside the one gather launch,
// 2: phase B as a launch of its own (el_phase_b).  The split pays where a row-tile holds many entries
// (PubMed: 50 on average, gather 6.3 -> 5.5 ms); with few (Cora, ~6) the second launch's fixed costs — the
// job, its ids and the partial rows once more — outweigh the waves it gains (1.54 -> 1.64 ms per step).
constexpr int64_t kSplitMinEntries = 24;   // average entries per element row-tile from which phase B is split
int element_mode(const s3grl_plan* p, const s3grl_features* f) {
  const int depth = p->walk_plan ? 1 : p->cfg.num_hops;   // (one hop for random-walk subgraphs)
  const int K = p->cfg.sign_k;
  if (!f->packed || !f->elements || (K >= 2 && K - 1 >= depth)) return 0;
  return f->el_nnz >= kSplitMinEntries * f->N * (int64_t)f->tiles ? 2 : 1;
}

template <int K>
s3grl_status launch_packed_k(s3grl_context* ctx, const s3grl_plan* p, const GatherView& v,
                             const s3grl_features* f, float* rows) {
  hipStream_t stream = ctx->stream;
  const unsigned gx = (unsigned)((v.njobs + kWavesPerBlock - 1) / kWavesPerBlock);
  const uint32_t data_bytes = (uint32_t)((f->pk_chunks + 1) * 16);
  const ElemEntry* el = static_cast<const ElemEntry*>(f->el_ent);
  const uint32_t el_bytes = f->elements ? (uint32_t)(f->el_nnz * (int64_t)sizeof(ElemEntry)) : 0u;
  // every job's last two operators reach its whole list when sign_k - 1 >= the BFS depth (one hop for
  // random-walk subgraphs); the element rows serve only the one-operator phase B of the others
  const int depth = p->walk_plan ? 1 : p->cfg.num_hops;
  const int el_mode = element_mode(p, f);
  auto kern = gather_packed_kernel<K, 1, 0>;
  if (K >= 2 && K - 1 >= depth)
    kern = gather_packed_kernel<K, (K >= 2 ? 2 : 1), 0>;
  else if (el_mode == 1)
    kern = gather_packed_kernel<K, 1, 1>;
  else if (el_mode == 2)
    kern = gather_packed_kernel<K, 1, 2>;
  // split element plans: phase A, then phase B (the last operator beyond the prefix) as a launch of its own
  for (int ph = 0; ph < (el_mode == 2 ? 2 : 1); ++ph) {
    const auto kph = ph == 0 ? kern : gather_packed_kernel<K, 1, 3>;
    hipLaunchKernelGGL(kph, dim3(gx, (unsigned)f->tiles),
                       dim3(kWavesPerBlock * 64), 0, stream, v.jobs, (int)v.njobs, p->c_ids, p->c_coef, v.job_z,
                       v.job_lim, v.job_order, static_cast<const PackedHdr*>(f->pk_hdr),
                       static_cast<const float4_t*>(f->pk_data), data_bytes, el, el_bytes, f->N, f->dense, f->ld,
                       (int)f->F, rows, v.prows);
    S3GRL_HIP_TRY(hipGetLastError());
  }
  return S3GRL_OK;
}

}  // namespace

// Builds the packed copy of f->dense when at most `max_density` of its chunks are non-zero
// (otherwise leaves f->packed false: the dense kernel moves no more bytes and issues fewer
// instructions).  One host round trip for the chunk total.
s3grl_status build_packed_rows(s3grl_context* ctx, s3grl_features* f, double max_density, bool elements) {
  const int64_t N = f->N;
  const int tiles = (int)((f->F + kTile - 1) / kTile);
  const int64_t items = N * tiles;
  Transient tmp{ctx, {}};
  void* q = nullptr;
  S3GRL_TRY(ctx->arena.alloc((size_t)items * 4, &q));
  tmp.ptrs.push_back(q);
  int32_t* cnt = static_cast<int32_t*>(q);
  S3GRL_TRY(ctx->arena.alloc((size_t)(items + 1) * 8, &q));
  tmp.ptrs.push_back(q);
  int64_t* ptr = static_cast<int64_t*>(q);
  S3GRL_TRY(ctx->arena.alloc((size_t)scan_workspace_elems(items) * 8, &q));
  tmp.ptrs.push_back(q);
  int64_t* ws = static_cast<int64_t*>(q);
  const unsigned grid = (unsigned)((items + 3) / 4);
  hipLaunchKernelGGL(pk_count_kernel, dim3(grid), dim3(256), 0, ctx->stream, f->dense, f->ld, (int)f->F, N, tiles, cnt);
  S3GRL_HIP_TRY(hipGetLastError());
  S3GRL_TRY(launch_scan_i32_to_i64(ctx, cnt, items, ptr, ws));
  S3GRL_HIP_TRY(hipMemcpyAsync(ctx->h_scalars, ptr + items, 8, hipMemcpyDeviceToHost, ctx->stream));
  S3GRL_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const int64_t chunks = ctx->h_scalars[0];
  const double slots = (double)N * (double)((f->F + 3) / 4);
  f->pk_chunks = chunks;
  if ((double)chunks > max_density * slots) return S3GRL_OK;
  if ((chunks + 1) * 16 >= ((int64_t)1 << 31)) return S3GRL_OK;   // 32-bit byte offsets, and room for the out-of-range one
  if (N >= ((int64_t)1 << 27)) return S3GRL_OK;                   // 32-bit byte offsets into a tile's headers
  void* hdr = nullptr;
  void* data = nullptr;
  S3GRL_TRY(ctx->arena.alloc((size_t)items * sizeof(PackedHdr), &hdr));
  f->owned.push_back(hdr);
  S3GRL_TRY(ctx->arena.alloc((size_t)(chunks + 1) * 16, &data));
  f->owned.push_back(data);
  hipLaunchKernelGGL(pk_fill_kernel, dim3(grid), dim3(256), 0, ctx->stream, f->dense, f->ld, (int)f->F, N, tiles, ptr,
                     static_cast<PackedHdr*>(hdr), static_cast<float4_t*>(data));
  S3GRL_HIP_TRY(hipGetLastError());
  f->pk_hdr = hdr;
  f->pk_data = data;
  f->packed = true;
  if (elements) S3GRL_TRY(build_element_rows(ctx, f));
  return S3GRL_OK;
}

s3grl_status launch_gather_traffic(s3grl_context* ctx, const s3grl_plan* p, const s3grl_features* f,
                                   unsigned long long* d_out) {
  if (p->njobs == 0) return S3GRL_OK;
  if (f->sparse) {
    set_last_error("gather traffic accounting covers the dense and the packed operand");
    return S3GRL_ERR_NOT_IMPLEMENTED;
  }
  const int el = element_mode(p, f);   // the kernels launch_packed_k picks
  hipLaunchKernelGGL(gather_traffic_kernel, dim3((unsigned)((p->njobs + 3) / 4)), dim3(256), 0, ctx->stream,
                     p->jobs, (int)p->njobs, p->c_ids, p->job_lim, p->cfg.sign_k, f->packed ? 1 : 0, el,
                     static_cast<const PackedHdr*>(f->pk_hdr), f->N, (int)f->F, 0, d_out);
  if (p->npieces)
    hipLaunchKernelGGL(gather_traffic_kernel, dim3((unsigned)((p->npieces + 3) / 4)), dim3(256), 0, ctx->stream,
                       p->gjobs + p->njobs, (int)p->npieces, p->c_ids, p->g_lim + p->njobs * p->cfg.sign_k,
                       p->cfg.sign_k, f->packed ? 1 : 0, el, static_cast<const PackedHdr*>(f->pk_hdr), f->N, (int)f->F, 1,
                       d_out);
  S3GRL_HIP_TRY(hipGetLastError());
  return S3GRL_OK;
}

s3grl_status launch_gather_packed(s3grl_context* ctx, const s3grl_plan* p, const GatherView& v,
                                  const s3grl_features* f, float* rows) {
  if (v.njobs == 0) return S3GRL_OK;
  switch (p->cfg.sign_k) {
    case 1: return launch_packed_k<1>(ctx, p, v, f, rows);
    case 2: return launch_packed_k<2>(ctx, p, v, f, rows);
    case 3: return launch_packed_k<3>(ctx, p, v, f, rows);
    case 4: return launch_packed_k<4>(ctx, p, v, f, rows);
    case 5: return launch_packed_k<5>(ctx, p, v, f, rows);
    case 6: return launch_packed_k<6>(ctx, p, v, f, rows);
    case 7: return launch_packed_k<7>(ctx, p, v, f, rows);
    case 8: return launch_packed_k<8>(ctx, p, v, f, rows);
    default:
      set_last_error("sign_k must be in 1..8");
      return S3GRL_ERR_INVALID_ARGUMENT;
  }
}

}  // namespace s3grl

S3GRL_DEFINE_TOUCH(packed)
