// orbx_match_grid.h — a frame's grid in LDS, for the kernels that search windows of it (orbx_match_proj_kernel.hip,
// orbx_match_local_kernel.hip, orbx_match_kfproj_kernel.hip, through orbx_match_rounds.h, which walks the windows):
// Frame::PosInGrid (SlamTypes/Frame.cpp:89-99) as the cells' start table plus the features' indices by cell, and the cell range of
// Frame::GetFeaturesInArea (:163-206).  Device code; every function is called by all MP_THREADS threads of a workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include "orbx_device.h"

namespace orbx {
namespace {

constexpr int MP_CELLS = ORBX_GRID_COLS * ORBX_GRID_ROWS;
constexpr int MP_CELLS_PER_THREAD = MP_CELLS / MP_THREADS;
static_assert(MP_CELLS_PER_THREAD * MP_THREADS == MP_CELLS, "the scan gives every thread the same number of cells");
constexpr int MP_START_WORDS = (MP_CELLS + 1 + 3) & ~3;  // cell starts [MP_CELLS + 1], padded to 16 bytes

__device__ __forceinline__ int mpClamp(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }
__device__ __forceinline__ bool mpFinite(float x) { return fabsf(x) <= 3.402823466e38f; }  // (false for a NaN)

__device__ __forceinline__ int mpDistance(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
         __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// the image bounds as the grid sees them (Frame.cpp:46-47)
struct MpGrid {
  float minX, maxX, minY, maxY, wInv, hInv;
};
__device__ __forceinline__ MpGrid mpGridOf(const orbx_bounds& b) {
  MpGrid g;
  g.minX = (float)b.min_x; g.maxX = (float)b.max_x;
  g.minY = (float)b.min_y; g.maxY = (float)b.max_y;
  g.wInv = (float)ORBX_GRID_COLS / (float)(b.max_x - b.min_x);
  g.hInv = (float)ORBX_GRID_ROWS / (float)(b.max_y - b.min_y);
  return g;
}

// Frame::PosInGrid: the cell (x * ORBX_GRID_ROWS + y) of a keypoint, -1 outside the grid
__device__ __forceinline__ int mpCell(const MpGrid& P, float x, float y) {
  const float px = roundf((x - P.minX) * P.wInv), py = roundf((y - P.minY) * P.hInv);
  if (!(px >= 0.0f && px < (float)ORBX_GRID_COLS && py >= 0.0f && py < (float)ORBX_GRID_ROWS)) return -1;
  return (int)px * ORBX_GRID_ROWS + (int)py;
}

// Counts the n keypoints into cellStart [MP_START_WORDS], which the caller zeroed behind a barrier.  Ends without a barrier.
__device__ __forceinline__ void mpGridCount(const MpGrid& P, const orbx_keypoint* kps, int n, int* cellStart) {
  for (int j = threadIdx.x; j < n; j += MP_THREADS) {
    const int c = mpCell(P, kps[j].x, kps[j].y);
    if (c >= 0) atomicAdd(&cellStart[c + 1], 1);
  }
}

// Behind mpGridCount and a barrier: the exclusive scan of the counts in place (a thread owns MP_CELLS_PER_THREAD consecutive
// cells; sWave holds one int per wave), then the fill: cell c holds cellIdx[cellStart[c] .. cellStart[c + 1]), in the order the
// fill's atomics left them.  Ends without a barrier.
__device__ __forceinline__ void mpGridFill(const MpGrid& P, const orbx_keypoint* kps, int n, int* cellStart, uint16_t* cellIdx,
                                           int* sWave) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  {
    int cnt[MP_CELLS_PER_THREAD], sum = 0;
#pragma unroll
    for (int k = 0; k < MP_CELLS_PER_THREAD; k++) { cnt[k] = cellStart[1 + t * MP_CELLS_PER_THREAD + k]; sum += cnt[k]; }
    int incl = sum;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int o = __shfl_up(incl, s);
      if (lane >= s) incl += o;
    }
    if (lane == 63) sWave[w] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int k = 0; k < w; k++) run += sWave[k];
#pragma unroll
    for (int k = 0; k < MP_CELLS_PER_THREAD; k++) { cellStart[1 + t * MP_CELLS_PER_THREAD + k] = run; run += cnt[k]; }
  }
  __syncthreads();
  // (cellStart[c + 1] is cell c's fill position; once every feature is placed it is the cell's end = the next cell's start)
  for (int j = t; j < n; j += MP_THREADS) {
    const int c = mpCell(P, kps[j].x, kps[j].y);
    if (c >= 0) cellIdx[atomicAdd(&cellStart[c + 1], 1)] = (uint16_t)j;
  }
}

// GetFeaturesInArea's cell range around (u, v) with radius r, clamped as floats; false when the window misses the grid
__device__ __forceinline__ bool mpWindow(const MpGrid& P, float u, float v, float r, int* x0, int* x1, int* y0, int* y1) {
  const float lox = floorf(((u - P.minX) - r) * P.wInv), hix = ceilf(((u - P.minX) + r) * P.wInv);
  const float loy = floorf(((v - P.minY) - r) * P.hInv), hiy = ceilf(((v - P.minY) + r) * P.hInv);
  *x0 = lox < 0.0f ? 0 : (int)lox;
  *x1 = hix > (float)(ORBX_GRID_COLS - 1) ? ORBX_GRID_COLS - 1 : (int)hix;
  *y0 = loy < 0.0f ? 0 : (int)loy;
  *y1 = hiy > (float)(ORBX_GRID_ROWS - 1) ? ORBX_GRID_ROWS - 1 : (int)hiy;
  return !(lox >= (float)ORBX_GRID_COLS || hix < 0.0f || loy >= (float)ORBX_GRID_ROWS || hiy < 0.0f);
}

}  // namespace
}  // namespace orbx
