// The walk over two sorted CSR rows that the pairwise scorers share (pairs_kernel of s3grl_heuristics.hip,
// cn_lists_kernel of s3grl_ncn.hip): the lanes walk the shorter row and each searches the longer one for its key.
// Device only.  Off is the caller's offset type: the heuristics keep the CSR's int64 offsets, NCN wave-uniform ints.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace s3grl {

// position of `key` in the ascending idx[lo, end), or -1
template <typename Off>
__device__ __forceinline__ Off find_sorted(const int32_t* __restrict__ idx, Off lo, Off end, int32_t key) {
  Off hi = end;
  while (lo < hi) {
    const Off mid = lo + ((hi - lo) >> 1);
    if (idx[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return (lo < end && idx[lo] == key) ? lo : Off(-1);
}

// the walked row [w0, w1), the searched row [o0, o1), and whether the walked one is the first node's
template <typename Off>
struct RowWalk {
  Off w0, w1, o0, o1;
  bool first;
};

// Rows [a0, a1) of node a and [b0, b1) of node b.  The shorter row is walked; a tie walks the row of the smaller node
// id, so that (a, b) and (b, a) take the same path.  This is part of the scorers' specification: the walked row fixes
// which lane adds which common key, and with it the order of a link's fp64 sum.
template <typename Off>
__device__ __forceinline__ RowWalk<Off> pick_walk(Off a0, Off a1, Off b0, Off b1, int32_t a, int32_t b) {
  const bool first = (a1 - a0) < (b1 - b0) || ((a1 - a0) == (b1 - b0) && a <= b);
  return {first ? a0 : b0, first ? a1 : b1, first ? b0 : a0, first ? b1 : a1, first};
}

}  // namespace s3grl
