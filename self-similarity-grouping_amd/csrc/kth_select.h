// kth_select.h -- the k-th smallest entry of one matrix row, exact for every k in [1, N]: what the core distances of OPTICS
// (optics.hip) and of HDBSCAN (hdbscan.hip) share.  One wave per row: radix select over order-preserving 64-bit keys, eight 8-bit digits
// from the top, one stream of the row per digit.  The key and its inverse are scalar rules of optics.hip (tests/test_optics_host.py
// compiles their text for x86); they are declared here and defined there, and optics.hip comes before hdbscan.hip in the unity TU.
#pragma once
#include "matview.h"

namespace ssg {

__device__ __forceinline__ uint64_t optics_key(double d);
__device__ __forceinline__ double optics_unkey(uint64_t k);

// The k-th smallest (1-based) entry of local row `il` of the view, the diagonal counted as it stands.  `h` is this wave's histogram of
// 256 ints in LDS.  Every wave of the workgroup calls this the same number of times (it holds barriers): a wave past the end of the
// matrix repeats the last row and drops the result.  All lanes return the same value.
template <int MODE>
__device__ __forceinline__ double row_kth_smallest(const MatView& mv, int il, int k, int* h) {
  const int lane = lane_id();
  const int gi = mv.row0 + il;
  RowStream rs(il, mv.N, mv.nrows);
  uint64_t prefix = 0;      // the digits chosen so far
  int want = k;             // 1-based rank among the keys that carry the prefix
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int b = lane; b < 256; b += 64) h[b] = 0;
    __syncthreads();
    for (int c = 0; c < rs.nchunks; c++) {
      double d[8];
      load_vals<MODE>(mv, rs, c, lane, gi, d);
      const int j0 = rs.col0(c, lane);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int j = j0 + e;
        if (j < 0 || j >= mv.N) continue;
        const uint64_t key = optics_key(d[e]);
        if (shift == 56 || (key >> (shift + 8)) == prefix) atomicAdd(&h[(int)((key >> shift) & 255u)], 1);
      }
    }
    __syncthreads();
    int c4[4], tot = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) { c4[q] = h[lane * 4 + q]; tot += c4[q]; }
    int inc = tot;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const int o = __shfl_up(inc, s, 64); if (lane >= s) inc += o; }
    int below = inc - tot, digit = lane * 4 + 3;
    const bool mine = below < want && want <= inc;       // exactly one lane: the counts add up to at least `want`
    bool found = !mine;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      if (found) continue;
      if (want <= below + c4[q]) { digit = lane * 4 + q; found = true; }
      else below += c4[q];
    }
    const uint64_t m = __ballot(mine);
    const int src = m ? __ffsll((long long)m) - 1 : 0;
    digit = __shfl(digit, src, 64); below = __shfl(below, src, 64);
    prefix = (prefix << 8) | (uint64_t)digit;
    want -= below;
    __syncthreads();
  }
  return optics_unkey(prefix);
}

}  // namespace ssg
