// Wave-load probe: what a buffer wave-load of an element row costs at 8 and at 16 bytes per lane, gfx950.
//
//   build:  hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/wave_load_probe.hip -o build/wave_load_probe
//   run:    build/wave_load_probe [entries-per-row = 50] [rows-per-wave = 8192] [table KiB = 14336]      (GPU box)
//
// The packed gather's element phase (s3grl_packed.hip, el_phase_b) fetches a row of n (value, slot) entries
// as ONE raw_buffer_load_b64: lane j < n entry j, the other lanes out of range.  DESIGN.md Appendix B prices
// that path per wave-load instruction, not per byte.  This program measures the premise on its own: one wave
// per workgroup, eight waves per SIMD, every wave walks a pseudo-random sequence of rows of a 14 MB table of
// 8-byte entries (the size of PubMed's element rows: resident in the Infinity Cache) and sums what it loads.
// Three shapes over the same rows:
//   a  one b64 load per row: lanes < n in range, the rest out of range                       (today)
//   b  one b128 load per TWO rows: lanes 0-31 entries 2l, 2l+1 of row A, lanes 32-63 of row B, 2l >= n out of range
//   c  shape b + two v_permlane32_swap_b32 (values, slots): row A across 64 lanes, then row B across 64 lanes
// Rows start at even entries (16-byte aligned) in every shape.  Prints ms, cycles per row and per load
// instruction per CU at the device's clock rate (hipDeviceAttributeClockRate: the cycles are nominal).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned int uint2_t __attribute__((ext_vector_type(2)));
typedef unsigned int uint4_t __attribute__((ext_vector_type(4)));

#define HIP_OK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));    \
      std::exit(1);                                                                      \
    }                                                                                    \
  } while (0)

constexpr uint32_t kOob = 0x80000000u;   // beyond the buffer: the range check answers zeros, no request
constexpr int U = 4;                     // rows per group, as in el_phase_b

__device__ __forceinline__ uint32_t next_row(uint32_t& x, uint32_t range) {   // wave-uniform even entry index
  x = x * 1664525u + 1013904223u;
  return __builtin_amdgcn_readfirstlane(__umulhi(x, range) & ~1u);
}

template <int SHAPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8))) void probe_kernel(
    const uint2_t* __restrict__ table, uint32_t table_bytes, uint32_t range, uint32_t n, int rows,
    uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x;
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint2_t*>(table), 0, (int)table_bytes, 0x00020000);
  uint32_t x = __builtin_amdgcn_readfirstlane(blockIdx.x * 2654435761u + 12345u);
  float fs = 0.f;
  uint32_t us = 0u;
  const uint32_t l2 = (lane & 31u) * 2u;
  for (int g = 0; g < rows; g += U) {
    uint32_t s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = next_row(x, range);
    if constexpr (SHAPE == 0) {
      uint2_t e[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        e[u] = __builtin_bit_cast(uint2_t, __builtin_amdgcn_raw_buffer_load_b64(
                                               rsrc, (int)(lane < n ? (s[u] + lane) << 3 : kOob), 0, 0));
#pragma unroll
      for (int u = 0; u < U; ++u) {
        fs += __builtin_bit_cast(float, e[u].x);
        us ^= e[u].y;
      }
    } else {
      uint4_t e[U / 2];
#pragma unroll
      for (int p = 0; p < U / 2; ++p) {
        const uint32_t sp = lane >= 32u ? s[2 * p + 1] : s[2 * p];
        e[p] = __builtin_bit_cast(uint4_t, __builtin_amdgcn_raw_buffer_load_b128(
                                               rsrc, (int)(l2 < n ? (sp + l2) << 3 : kOob), 0, 0));
      }
#pragma unroll
      for (int p = 0; p < U / 2; ++p) {
        if constexpr (SHAPE == 2) {
          const auto v = __builtin_amdgcn_permlane32_swap(e[p].x, e[p].z, false, false);
          const auto t = __builtin_amdgcn_permlane32_swap(e[p].y, e[p].w, false, false);
          fs += __builtin_bit_cast(float, (uint32_t)v[0]);
          us ^= t[0];
          fs += __builtin_bit_cast(float, (uint32_t)v[1]);
          us ^= t[1];
        } else {
          fs += __builtin_bit_cast(float, e[p].x);
          us ^= e[p].y;
          fs += __builtin_bit_cast(float, e[p].z);
          us ^= e[p].w;
        }
      }
    }
  }
  out[(size_t)blockIdx.x * 64 + lane] = us ^ __builtin_bit_cast(uint32_t, fs);
}

int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 50u;
  const int rows = argc > 2 ? std::atoi(argv[2]) / U * U : 8192;
  const uint32_t kib = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 14u * 1024u;   // smaller: resident in L2, in the vector L1
  if (n < 1 || n > 64 || rows < U || kib < 2 || kib > 1024u * 1024u) {
    std::fprintf(stderr, "usage: wave_load_probe [entries-per-row 1..64] [rows-per-wave >= 4] [table KiB 2..1048576]\n");
    return 2;
  }
  int dev = 0, cus = 0, khz = 0;
  HIP_OK(hipGetDevice(&dev));
  HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  HIP_OK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, dev));
  const uint32_t entries = kib * 1024u / 8u;
  const uint32_t table_bytes = entries * 8u;
  const uint32_t range = entries - 128u;   // a row's 64 lanes stay inside the table
  const int waves = cus * 4 * 8;           // eight per SIMD, one per workgroup
  std::vector<uint2_t> h(entries);
  for (uint32_t i = 0; i < entries; ++i) {
    h[i].x = 0x3f800000u;   // 1.0f
    h[i].y = i & 511u;
  }
  uint2_t* table = nullptr;
  uint32_t* out = nullptr;
  HIP_OK(hipMalloc(&table, table_bytes));
  HIP_OK(hipMalloc(&out, (size_t)waves * 64 * 4));
  HIP_OK(hipMemcpy(table, h.data(), table_bytes, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  std::printf("wave_load_probe: %d CUs at %d MHz, %d waves x %d rows of %u entries, table %u bytes\n", cus,
              khz / 1000, waves, rows, n, table_bytes);
  const char* names[3] = {"a  b64, one row per load", "b  b128, two rows per load", "c  b128 + 2 permlane32_swap"};
  for (int rep = 0; rep < 3; ++rep) {   // the first round warms the caches and the clocks
    for (int shape = 0; shape < 3; ++shape) {
      HIP_OK(hipEventRecord(e0, nullptr));
      if (shape == 0) hipLaunchKernelGGL(probe_kernel<0>, dim3(waves), dim3(64), 0, nullptr, table, table_bytes, range, n, rows, out);
      if (shape == 1) hipLaunchKernelGGL(probe_kernel<1>, dim3(waves), dim3(64), 0, nullptr, table, table_bytes, range, n, rows, out);
      if (shape == 2) hipLaunchKernelGGL(probe_kernel<2>, dim3(waves), dim3(64), 0, nullptr, table, table_bytes, range, n, rows, out);
      HIP_OK(hipGetLastError());
      HIP_OK(hipEventRecord(e1, nullptr));
      HIP_OK(hipEventSynchronize(e1));
      float ms = 0.f;
      HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      const double cyc_cu = (double)ms * khz;              // cycles of one CU
      const double rows_cu = (double)rows * 32;            // rows per CU (32 waves)
      const double loads_cu = shape == 0 ? rows_cu : rows_cu / 2;
      std::printf("round %d  %-28s %8.3f ms  %6.2f cycles/row  %6.2f cycles/load\n", rep, names[shape], ms,
                  cyc_cu / rows_cu, cyc_cu / loads_cu);
    }
  }
  HIP_OK(hipFree(table));
  HIP_OK(hipFree(out));
  return 0;
}
