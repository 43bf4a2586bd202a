// orbx_match_rounds.h — what the SearchByProjection kernels share on top of the grid (orbx_match_grid.h): the pose, the camera,
// bit sets, the window walk and the launcher for all of them (orbx_match_proj_kernel.hip, orbx_match_local_kernel.hip,
// orbx_match_kfproj_kernel.hip, orbx_match_scw_kernel.hip), and for the kernels that keep a list of points (local, kfproj, scw)
// the key, the LDS layout, the entry pass, the ordered append, a round's head and the counter flush.  Each kernel keeps its own
// phases A and B, its decision and its counters: those are what differs, and what a reader compares with the reference's rule.
// Device code apart from the launcher; every function with a barrier in it is called by all MP_THREADS threads of a workgroup.
//
// The sequential rule in claim rounds (k_match_local, k_match_kfproj, k_match_scw; k_match_proj's pick-then-claim rounds and
// their argument are in its own file).  The points of the list are visited by the reference in ascending position p.  Point
// p's outcome (its match, or none, and why) is a function of U(p), the candidates of its window that nobody has taken when its
// turn comes.  Each kernel names a claim set C(p), a subset of the untaken candidates of p's window chosen by a test on (p, j) alone, with ONE
// property: every untaken candidate that can still become part of p's outcome -- that p's decision reads, now or once others
// are taken -- is in C(p); a candidate outside it can be struck from U(p) without changing the outcome.  In particular a
// point's match is always in its claim set.  A round:
//   A. every pending p claims, with an LDS atomicMin of p into claim[j], every j of C(p).
//   B. p is final iff claim[j] == p for every j of C(p) (none at all included).  Only then it decides.  A match sets
//      MR_MATCHED in claim[bestIdx], which no other point's test is changed by (it fails on that j with or without the bit), and
//      the "taken" bit is set at the start of the next round (mrRoundHead), so that a round reads one state of "taken"
//      throughout and `rounds` is the same on every run.
// This equals the sequential walk.  Call a state sound when every final point holds its sequential outcome and "taken" is the
// entry's set plus the final points' matches.  The start is sound.  In a sound state let p be pending and hold every claim of
// C(p).  (a) No final point q > p matched a candidate j that belongs to p's claim set: in the round q became final, p was
// pending (it is still) and j was untaken, so p claimed it, claim[j] <= p < q, and q -- whose match is in C(q) -- was not final.
// (b) No pending point q < p can take a candidate j of C(p) later: j is untaken now (taken only grows), q's match is in C(q), so
// q claims j and claim[j] <= q < p.  Points before p that are final have their sequential matches, which are in "taken".  So
// the untaken candidates of p's window now, as far as p's outcome can tell, are exactly U(p) of the sequential walk, and p's
// outcome computed from them is the sequential one: the state stays sound.  The smallest pending point holds every claim it
// makes, so every round resolves at least one point and the loop ends; points in different parts of the image never meet, and
// the rounds needed are the longest chain of points that wait for one another.
// No float atomics; integer atomics are min, or, and, add only, so nothing depends on the order in which they land.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "orbx_match_grid.h"

namespace orbx {
namespace {

// ---- bit sets over uint32_t words
__host__ __device__ constexpr int mrBitWords(int n) { return (n + 31) >> 5; }
__device__ __forceinline__ bool mrBit(const uint32_t* w, int i) { return (w[i >> 5] >> (i & 31)) & 1u; }
__device__ __forceinline__ void mrSetBit(uint32_t* w, int i) { atomicOr(&w[i >> 5], 1u << (i & 31)); }
__device__ __forceinline__ void mrClearBit(uint32_t* w, int i) { atomicAnd(&w[i >> 5], ~(1u << (i & 31))); }

// ---- the pose of a pair: row-major R, then t
struct MrPose {
  float R[9], t[3];
};
// loads pose[12 * pair ..]; false when one of the twelve is not finite
__device__ __forceinline__ bool mrLoadPose(const float* pose, int pair, MrPose* P) {
  pose += (size_t)pair * 12;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; k++) { P->R[k] = pose[k]; ok = ok && mpFinite(P->R[k]); }
#pragma unroll
  for (int k = 0; k < 3; k++) { P->t[k] = pose[9 + k]; ok = ok && mpFinite(P->t[k]); }
  return ok;
}
// the camera centre -R^T t
__device__ __forceinline__ void mrCameraCentre(const MrPose& P, float* Ow) {
#pragma unroll
  for (int k = 0; k < 3; k++) Ow[k] = -((P.R[k] * P.t[0] + P.R[3 + k] * P.t[1]) + P.R[6 + k] * P.t[2]);
}

// ---- the camera: point i of pts [..][3] in the camera's frame, and its image from xc, yc and 1 / zc.  What a kernel does about
// a point behind the camera lies between the two calls.  (The sums are associated as the CPU restatements associate them.)
__device__ __forceinline__ void mrToCamera(const MrPose& P, const float* pts, int i, float* xc, float* yc, float* zc) {
  const float X = pts[3 * (size_t)i], Y = pts[3 * (size_t)i + 1], Z = pts[3 * (size_t)i + 2];
  *xc = ((P.R[0] * X + P.R[1] * Y) + P.R[2] * Z) + P.t[0];
  *yc = ((P.R[3] * X + P.R[4] * Y) + P.R[5] * Z) + P.t[1];
  *zc = ((P.R[6] * X + P.R[7] * Y) + P.R[8] * Z) + P.t[2];
}
// false when (u, v) is not finite or outside the bounds
__device__ __forceinline__ bool mrToImage(const MatchCamArgs& c, const MpGrid& g, float xc, float yc, float invz, float* u, float* v) {
  const float pu = (c.fx * xc) * invz + c.cx, pv = (c.fy * yc) * invz + c.cy;
  if (!mpFinite(pu) || !mpFinite(pv)) return false;
  if (pu < g.minX || pu > g.maxX || pv < g.minY || pv > g.maxY) return false;
  *u = pu;
  *v = pv;
  return true;
}

// ---- the window walk (GetFeaturesInArea): calls f(j, cell) for every feature j of the window around (u, v) with radius r whose
// level is in [lo, hi], cells x outer, y inner, a cell's features in the grid's order, until f returns false; returns whether f
// never did.  (bCheckLevels holds in every caller: hi >= 0.)
template <class F>
__device__ __forceinline__ bool mrWalk(const MpGrid& g, const orbx_keypoint* kps, const int* cellStart, const uint16_t* cellIdx, float u,
                                       float v, float r, int lo, int hi, F f) {
  int x0, x1, y0, y1;
  if (!mpWindow(g, u, v, r, &x0, &x1, &y0, &y1)) return true;
  for (int cx = x0; cx <= x1; cx++)
    for (int cy = y0; cy <= y1; cy++) {
      const int c = cx * ORBX_GRID_ROWS + cy;
      const int k1 = cellStart[c + 1];
      for (int k = cellStart[c]; k < k1; k++) {
        const int j = cellIdx[k];
        const orbx_keypoint* kp = kps + j;
        const int lev = kp->octave;
        if (!(lev >= lo && lev <= hi)) continue;
        const float dx = kp->x - u, dy = kp->y - v;
        if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
        if constexpr (std::is_void_v<decltype(f(j, c))>) f(j, c);
        else if (!f(j, c)) return false;
      }
    }
  return true;
}

// ---- the launcher: one workgroup of MP_THREADS per pair with `lds` bytes of dynamic LDS
template <class A>
hipError_t mrLaunch(void (*kernel)(A), int nPairs, size_t lds, hipStream_t st, const A& a) {
  if (lds > 48 * 1024) {  // (beyond the default limit of a launch's dynamic LDS)
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)nPairs), dim3(MP_THREADS), lds, st, a);
  return hipGetLastError();
}

// ======== for the kernels with a list of points (k_match_local, k_match_kfproj, k_match_scw) ========

constexpr int MR_FREE = 0x3fffffff;       // claim[j]: nobody claims j
constexpr int MR_MATCHED = 0x40000000;    // claim[j]: ... | this bit: the claimant is final on j (a new match)
constexpr uint32_t MR_INDEX = 0x3fffu;    // list[p]: the point's index (< 16384) ...
constexpr uint32_t MR_PENDING = 0x8000u;  // ... not final yet (bit 14 is the kernel's own)
static_assert(BOW_MAX_FEATURES <= (int)MR_INDEX + 1, "a list entry's index is 14 bits");

// the window's order is (cell, index), so "the first smallest distance" is the smallest key (distance, cell, index)
__device__ __forceinline__ uint64_t mrKey(int d, int cell, int j) {
  return ((uint64_t)(uint32_t)d << 32) | ((uint32_t)cell << 16) | (uint32_t)j;
}
constexpr uint64_t MR_NO_KEY = ~0ull;
__device__ __forceinline__ int mrKeyDistance(uint64_t key) { return (int)(key >> 32); }
__device__ __forceinline__ int mrKeyIndex(uint64_t key) { return (int)(key & 0xffffu); }

// The dynamic LDS of a workgroup for `cap` features and `listCap` points.  The claim words hold the entry pass's bits over the
// points ("seen", "found") until the list is built, so there are max(cap, mrBitWords(listCap)) of them.
struct MrLds {
  int* cellStart;     // [MP_CELLS + 1]: cell c holds cellIdx[cellStart[c] .. cellStart[c + 1])
  int* claim;         // [cap] per feature: the smallest claimant
  uint32_t* had;      // the same words until the list is built: bits over the points the entry names
  uint32_t* taken;    // [mrBitWords(cap)] bits over the features
  uint16_t* cellIdx;  // [cap] the features by cell
  uint16_t* list;     // [listCap] the points to search, ascending: index | flags
  uint8_t* lev;       // [listCap] their levels

  __host__ __device__ static constexpr int claimWords(int cap, int listCap) {
    return cap > mrBitWords(listCap) ? cap : mrBitWords(listCap);
  }
  __host__ __device__ static constexpr size_t bytes(int cap, int listCap) {
    return (size_t)4 * (MP_START_WORDS + claimWords(cap, listCap) + mrBitWords(cap)) + (size_t)2 * ((cap + 1) & ~1) +
           (size_t)2 * ((listCap + 1) & ~1) + (size_t)((listCap + 3) & ~3);
  }
  __device__ __forceinline__ MrLds(uint32_t* base, int cap, int listCap) {
    cellStart = (int*)base;
    claim = cellStart + MP_START_WORDS;
    had = (uint32_t*)claim;
    taken = (uint32_t*)(claim + claimWords(cap, listCap));
    cellIdx = (uint16_t*)(taken + mrBitWords(cap));
    list = cellIdx + ((cap + 1) & ~1);
    lev = (uint8_t*)(list + ((listCap + 1) & ~1));
  }
  // the start state of the cell starts and of both bit sets, for nPts points.  Ends without a barrier.
  __device__ __forceinline__ void clear(int cap, int nPts) const {
    const int t = threadIdx.x;
    for (int c = t; c < MP_START_WORDS; c += MP_THREADS) cellStart[c] = 0;
    for (int k = t; k < mrBitWords(nPts); k += MP_THREADS) had[k] = 0;
    for (int k = t; k < mrBitWords(cap); k += MP_THREADS) taken[k] = 0;
  }
};

// The entry pass over the match row of the nF features: a feature that names a point (of nPts) marks it in L.had and keeps it
// ("taken"), unless it is an outlier: then its entry is cleared (counted in *cleared).  An entry >= nPts: the feature is taken
// and *status |= badInput.  Ends without a barrier.
// With `xlate` (k_match_scw; the other callers pass none and are as they were) an entry i >= 0 is an index into xlate [nXlate],
// which holds the point or a negative value: the point is written back to the row; a negative one writes `unmappedMark` there,
// keeps the feature taken, marks no point and counts in *unmapped, as does an entry that holds the mark already (a mark of 0
// is none).  An entry >= nXlate or a translated value >= nPts stays as it is: the feature is taken and *status |= badInput.
__device__ __forceinline__ void mrEntryPass(const MrLds& L, int* row, int nF, int nPts, const uint8_t* outl, int badInput, int* status,
                                            int* cleared, const int32_t* xlate = nullptr, int nXlate = 0, int unmappedMark = 0,
                                            int* unmapped = nullptr) {
  for (int j = threadIdx.x; j < nF; j += MP_THREADS) {
    int i = row[j];
    if (unmappedMark != 0 && i == unmappedMark) {
      mrSetBit(L.taken, j);
      (*unmapped)++;
      continue;
    }
    if (i < 0) continue;
    if (xlate) {
      if (i >= nXlate) {
        *status |= badInput;
        mrSetBit(L.taken, j);
        continue;
      }
      i = xlate[i];
      if (i < 0) {
        row[j] = unmappedMark;
        mrSetBit(L.taken, j);
        (*unmapped)++;
        continue;
      }
      if (i < nPts) row[j] = i;
    }
    if (i >= nPts) {
      *status |= badInput;
      mrSetBit(L.taken, j);
      continue;
    }
    mrSetBit(L.had, i);
    if (outl && outl[j] != 0) {
      row[j] = -1;
      (*cleared)++;
    } else {
      mrSetBit(L.taken, j);
    }
  }
}

// One slice of the ordered append: the threads with `in` append their entry and level to the list in thread order (ballot inside
// a wave, the waves' sums through sWave [MP_THREADS / 64]); *sListN is the list's length, zero before the first slice and valid
// behind a barrier after the last.  (At most one entry per point: the position stays below listCap.)
__device__ __forceinline__ void mrAppend(const MrLds& L, bool in, uint32_t entry, int level, int* sWave, int* sListN) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint64_t ballot = __ballot(in);
  if (lane == 0) sWave[w] = __popcll(ballot);
  __syncthreads();
  int pos = *sListN + __popcll(ballot & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; k++) pos += sWave[k];
  if (in) {
    L.list[pos] = (uint16_t)(entry | MR_PENDING);
    L.lev[pos] = (uint8_t)level;
  }
  __syncthreads();
  if (t == MP_THREADS - 1) *sListN = pos + (in ? 1 : 0);
}

// Behind the last slice: the list's length; *sAny = there is a round to run; every claim free (L.had is read no more).
__device__ __forceinline__ int mrListDone(const MrLds& L, int nF, const int* sListN, int* sAny) {
  __syncthreads();
  const int nList = *sListN;
  if (threadIdx.x == 0) *sAny = nList > 0;
  for (int j = threadIdx.x; j < nF; j += MP_THREADS) L.claim[j] = MR_FREE;
  __syncthreads();
  return nList;
}

// A round's head: last round's matches are taken, everything else untaken is free again; *sAny = 0 for phase B to set.
__device__ __forceinline__ void mrRoundHead(const MrLds& L, int nF, int* sAny) {
  for (int j = threadIdx.x; j < nF; j += MP_THREADS) {
    if (L.claim[j] & MR_MATCHED) mrSetBit(L.taken, j);
    else L.claim[j] = MR_FREE;
  }
  __syncthreads();
  if (threadIdx.x == 0) *sAny = 0;
}

// The threads' counters into the pair's result record of FIELDS int32: field 0 the status bits, the last one `rounds`, the others
// sums.  sCnt [FIELDS] is zero.
template <int FIELDS>
__device__ __forceinline__ void mrFlush(const int (&cnt)[FIELDS], int status, int rounds, int* sCnt, int32_t* res) {
  if (status) atomicOr(&sCnt[0], status);
#pragma unroll
  for (int k = 1; k < FIELDS - 1; k++)
    if (cnt[k]) atomicAdd(&sCnt[k], cnt[k]);
  __syncthreads();
  const int t = threadIdx.x;
  if (t < FIELDS) res[t] = t == FIELDS - 1 ? rounds : sCnt[t];
}

}  // namespace
}  // namespace orbx
