// orbx_match_node.h — what the matchers that walk the FeatureVector share (k_match_bow of SearchByBoW, orbx_match_bow_kernel.hip;
// k_match_tri of SearchForTriangulation, orbx_match_tri_kernel.hip): a count clamped to the capacity, the bounds of a node's run in
// a FeatureVector, and the Hamming distance of two descriptors held as two uint4 each.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <cstdint>

namespace orbx {

__device__ __forceinline__ int mbClamp(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

// first index in [lo, hi) whose node is >= (upper == false) or > (upper == true) `node`; any content keeps it inside [lo, hi]
__device__ __forceinline__ int mbBound(const uint32_t* __restrict__ nodes, int lo, int hi, uint32_t node, bool upper) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const uint32_t v = nodes[mid];
    if (upper ? v <= node : v < node) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// both bounds of `node` in nodes[0, n) at once: *lb = mbBound(nodes, 0, n, node, false), *ub = mbBound(nodes, 0, n, node, true).  The
// two searches advance in one loop, so that their loads are in flight together: one memory round trip per step instead of two
__device__ __forceinline__ void mbRange(const uint32_t* __restrict__ nodes, int n, uint32_t node, int* lb, int* ub) {
  int lo1 = 0, hi1 = n, lo2 = 0, hi2 = n;
  while (lo1 < hi1 || lo2 < hi2) {
    const int mid1 = (lo1 + hi1) >> 1, mid2 = (lo2 + hi2) >> 1;
    const uint32_t v1 = lo1 < hi1 ? nodes[mid1] : 0u, v2 = lo2 < hi2 ? nodes[mid2] : 0u;
    if (lo1 < hi1) {
      if (v1 < node) lo1 = mid1 + 1;
      else hi1 = mid1;
    }
    if (lo2 < hi2) {
      if (v2 <= node) lo2 = mid2 + 1;
      else hi2 = mid2;
    }
  }
  *lb = lo1;
  *ub = lo2;
}

__device__ __forceinline__ int mbDistance(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
         __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

}  // namespace orbx
#endif
