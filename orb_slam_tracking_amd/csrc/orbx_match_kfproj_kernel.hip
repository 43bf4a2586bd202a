// orbx_match_kfproj_kernel.hip — the relocalisation overload ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF,
// const set<MapPoint*>& sAlreadyFound, th, ORBdist) for a batch of (keyframe KF, current frame C) pairs (include/orbx.h,
// "matching a keyframe's points by projection").  gfx950, wave64.
//
// One workgroup of MP_THREADS threads per pair, one launch per call.
//   rule 1   every feature of C reads its entry of the match row: the keyframe's points C has become "found" (a bit set over
//            KF's features), the features that keep their point "taken" (a bit set over C), outliers' entries are cleared.
//   grid     C's grid in LDS as k_match_proj builds it (orbx_match_grid.h).
//   rules 2-3 ONE pass over KF's points in slices of MP_THREADS: the projection (no depth test), the f64 distance and the level,
//            and an order-preserving scan (ballot inside a wave, the waves' sums through LDS) that appends the survivors to an
//            LDS list in ascending point index: from here on a point is its position p in the list.  An entry keeps the index and
//            a "pending" bit; the level lies in a byte beside it.  (u, v) are recomputed from the point, by the same arithmetic,
//            when a point walks its window.
//   rules 4-6 in rounds, see below; rule 7 over the new matches; then a feature with a new match that stays writes it.
//
// The sequential rule, in §4j's form with the claims narrowed.  Point p's outcome is a function of the set U(p) of candidates of
// its window that nobody has taken when its turn comes: the first smallest of U(p) under the key (distance, position in the
// window's order), a match iff that distance is <= orb_dist.  Only N(p) = the members of U(p) with d <= orb_dist matter: a farther
// candidate is never p's match, and removing it from U(p) changes neither p's match nor the fact that it has none.  A round:
//   A. every pending p claims, with an LDS atomicMin of p into claim[j], every untaken candidate j of its window with
//      d(p, j) <= orb_dist.
//   B. p is final iff claim[j] == p for every such j (none at all included).  Only then it decides: its match is the smallest
//      key among them, which sets a bit in claim[bestIdx]; no other point's test is changed by that bit (it fails on that j
//      with or without it), and the "taken" bit is set at the start of the next round, so that a round reads one state of
//      "taken" throughout and `rounds` is the same on every run.
// This equals the sequential walk.  Call a state sound when every final point holds its sequential outcome and "taken" is the
// entry's set plus the final points' matches.  The start is sound.  In a sound state let p be pending and hold every claim it
// made.  (a) No final point q > p matched a candidate j of N(p): in the round q became final, p was pending (it is still) and j
// was untaken and within orb_dist of p, so claim[j] <= p < q and q was not final.  (b) No pending point q < p can take a candidate
// j that p claims now: j is untaken now (taken only grows), q could only take it with d(q, j) <= orb_dist, so q claims it and
// claim[j] <= q < p.  Points before p that are final have their sequential matches, which are in "taken".  So the untaken
// candidates within orb_dist of p now are exactly those of the sequential walk at p's turn, and p's outcome computed from them is
// the sequential one: the state stays sound.  The smallest pending point holds every claim it makes, so every round resolves at
// least one point and the loop ends.  The narrowing costs a distance pass in phase A and saves rounds: with th = 10 a window
// holds many features, few of which lie within orb_dist of a given point.
// No float atomics; integer atomics are min, or and add only, so nothing depends on the order in which they land.
//
// LDS, sized from the capacity by the launcher (kpLdsBytes): 12304 bytes of cell starts; 4 bytes of claims per feature of C (the
// same words hold rule 1's "found" bits until the list is built); a bit per feature; 2 bytes of cell-ordered indices per
// feature; 2 bytes of list entry and 1 of level per point of KF -- 21.1 KB at capacity 1024, 158.0 KB at ORBX_BOW_MAX_FEATURES,
// plus 320 bytes of static LDS.  77 VGPRs, no scratch (profiles/match_kfproj_kernel_stats.txt).
#include <hip/hip_runtime.h>

#include "orbx_launch.h"
#include "orbx_match_grid.h"
#include "orbx_match_hist.h"

namespace orbx {
namespace {

constexpr int KP_FREE = 0x3fffffff;      // claim[j]: nobody claims j
constexpr int KP_MATCHED = 0x40000000;   // claim[j]: ... | this bit: the claimant is final on j (a new match)
constexpr uint32_t KP_INDEX = 0x3fffu;   // list[p]: the point's index (< 16384) ...
constexpr uint32_t KP_PENDING = 0x8000u; // ... not final yet
static_assert(BOW_MAX_FEATURES <= (int)KP_INDEX + 1, "a list entry's index is 14 bits");
enum { KP_DROPPED, KP_OUT_IMAGE, KP_OUT_DISTANCE, KP_SEARCHED };
// sCnt: the fields of orbx_kfproj_result in their order
enum { C_STATUS, C_NMATCHES, C_POINTS, C_FOUND, C_BEHIND_KEPT, C_OUT_IMAGE, C_OUT_DISTANCE, C_WITH_CAND, C_OVER_DIST, C_DISPLACED,
       C_ROT_REMOVED, C_CLEARED, C_ROUNDS, C_FIELDS };

__host__ __device__ constexpr int kpBitWords(int n) { return (n + 31) >> 5; }
__host__ __device__ constexpr size_t kpLdsBytes(int cap) {
  return (size_t)4 * (MP_START_WORDS + cap + kpBitWords(cap)) + (size_t)2 * 2 * ((cap + 1) & ~1) + (size_t)((cap + 3) & ~3);
}

struct KpPair {
  const orbx_keypoint* kpsC;
  const float *pts, *dist;
  float R[9], t[3], Ow[3];
  MpGrid g;
};

// rule 2's projection of point i: false when (u, v) is not finite or outside the bounds; *behind = zc < 0 (no test: a count)
__device__ __forceinline__ bool kpProject(const MatchKfProjArgs& a, const KpPair& P, int i, float* u, float* v, bool* behind) {
  const float X = P.pts[3 * (size_t)i], Y = P.pts[3 * (size_t)i + 1], Z = P.pts[3 * (size_t)i + 2];
  const float xc = ((P.R[0] * X + P.R[1] * Y) + P.R[2] * Z) + P.t[0];
  const float yc = ((P.R[3] * X + P.R[4] * Y) + P.R[5] * Z) + P.t[1];
  const float zc = ((P.R[6] * X + P.R[7] * Y) + P.R[8] * Z) + P.t[2];
  *behind = zc < 0.0f;
  const float invz = 1.0f / zc;
  const float pu = (a.fx * xc) * invz + a.cx, pv = (a.fy * yc) * invz + a.cy;
  if (!mpFinite(pu) || !mpFinite(pv)) return false;
  if (pu < P.g.minX || pu > P.g.maxX || pv < P.g.minY || pv > P.g.maxY) return false;
  *u = pu;
  *v = pv;
  return true;
}

// rules 2 and 3 for point i (mask set, not found, finite pose): where it ends, and for KP_SEARCHED the level
__device__ __forceinline__ int kpSearched(const MatchKfProjArgs& a, const KpPair& P, const float* __restrict__ scale, int i, int* level,
                                          bool* behind, int* status) {
  const float* X = P.pts + 3 * (size_t)i;
  const float minD = P.dist[2 * (size_t)i], maxD = P.dist[2 * (size_t)i + 1];
  if (!(mpFinite(X[0]) && mpFinite(X[1]) && mpFinite(X[2]) && mpFinite(minD) && mpFinite(maxD))) {
    *status |= ORBX_KFPROJ_NONFINITE;
    return KP_DROPPED;
  }
  float u, v;
  if (!kpProject(a, P, i, &u, &v, behind)) return KP_OUT_IMAGE;
  const float px = X[0] - P.Ow[0], py = X[1] - P.Ow[1], pz = X[2] - P.Ow[2];
  const float dist = (float)sqrt(((double)px * (double)px + (double)py * (double)py) + (double)pz * (double)pz);
  if (dist < 0.8f * minD || dist > 1.2f * maxD) return KP_OUT_DISTANCE;
  const float ratio = maxD / dist;
  if (ratio != ratio) {
    *status |= ORBX_KFPROJ_NONFINITE;
    return KP_DROPPED;
  }
  int lv = 0;
  for (int n = 0; n < a.nLevels - 1; n++) lv += ratio > scale[n];
  *level = lv;
  return KP_SEARCHED;
}

// Calls f(j, cell) for every candidate of the window (rule 4)
template <class F>
__device__ __forceinline__ void kpWalk(const KpPair& P, const int* cellStart, const uint16_t* cellIdx, float u, float v, float r,
                                       int level, F f) {
  int x0, x1, y0, y1;
  if (!mpWindow(P.g, u, v, r, &x0, &x1, &y0, &y1)) return;
  for (int cx = x0; cx <= x1; cx++)
    for (int cy = y0; cy <= y1; cy++) {
      const int c = cx * ORBX_GRID_ROWS + cy;
      const int k1 = cellStart[c + 1];
      for (int k = cellStart[c]; k < k1; k++) {
        const int j = cellIdx[k];
        const orbx_keypoint* kp = P.kpsC + j;
        const int lev = kp->octave;
        if (!(lev >= level - 1 && lev <= level + 1)) continue;  // (bCheckLevels holds: maxLevel = level + 1 >= 0)
        const float dx = kp->x - u, dy = kp->y - v;
        if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
        f(j, c);
      }
    }
}

// the key of rule 5: the window's order is (cell, index), so "the first smallest" is the smallest (distance, cell, index)
__device__ __forceinline__ uint64_t kpKey(int d, int cell, int j) {
  return ((uint64_t)(uint32_t)d << 32) | ((uint32_t)cell << 16) | (uint32_t)j;
}
__device__ __forceinline__ int kpDecide(uint64_t key, int orbDist) {
  return (key != ~0ull && (int)(key >> 32) <= orbDist) ? (int)(key & 0xffffu) : -1;
}

__global__ __launch_bounds__(MP_THREADS) void k_match_kfproj(MatchKfProjArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t kpLds[];
  __shared__ float sScale[ORBX_MAX_LEVELS];
  __shared__ int hist[MATCH_HISTO_LENGTH];
  __shared__ int sKeep[3], sKeepV[3];
  __shared__ int sWave[MP_THREADS / 64];
  __shared__ int sCnt[C_FIELDS];
  __shared__ int sAny, sListN;
  const int pair = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int cap = a.cap, words = kpBitWords(cap);
  int* const cellStart = (int*)kpLds;                            // [MP_CELLS + 1]
  int* const claim = cellStart + MP_START_WORDS;                 // [cap] per feature of C: the smallest claimant
  uint32_t* const found = (uint32_t*)claim;                      // until the list is built: bits over KF's features
  uint32_t* const taken = (uint32_t*)(claim + cap);              // [words] bits over C's features
  uint16_t* const cellIdx = (uint16_t*)(taken + words);          // [cap] C's features by cell
  uint16_t* const list = cellIdx + ((cap + 1) & ~1);             // [cap] the searched points, ascending
  uint8_t* const lev = (uint8_t*)(list + ((cap + 1) & ~1));      // [cap] their levels

  const int fk = a.pairs[pair], fc = a.pairs[a.nPairs + pair], ps = a.pairs[2 * a.nPairs + pair];
  const int rawK = a.n[fk], rawC = a.n[fc];
  const int nK = mpClamp(rawK, cap), nC = mpClamp(rawC, cap);
  KpPair P;
  P.kpsC = a.kps + (size_t)fc * cap;
  const orbx_keypoint* kpsK = a.kps + (size_t)fk * cap;
  P.pts = a.points + (size_t)ps * cap * 3;
  P.dist = a.pointDist + (size_t)ps * cap * 2;
  const uint8_t* mask = a.pointMask ? a.pointMask + (size_t)ps * cap : nullptr;
  const uint8_t* outl = a.outlier ? a.outlier + (size_t)pair * cap : nullptr;
  int status = (rawK != nK || rawC != nC) ? ORBX_KFPROJ_BAD_INPUT : 0;
  bool poseOk = true;
  {
    const float* pose = a.pose + (size_t)pair * 12;
#pragma unroll
    for (int k = 0; k < 9; k++) { P.R[k] = pose[k]; poseOk = poseOk && mpFinite(P.R[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) { P.t[k] = pose[9 + k]; poseOk = poseOk && mpFinite(P.t[k]); }
    if (!poseOk) status |= ORBX_KFPROJ_NONFINITE;
#pragma unroll
    for (int k = 0; k < 3; k++) P.Ow[k] = -((P.R[k] * P.t[0] + P.R[3 + k] * P.t[1]) + P.R[6 + k] * P.t[2]);
  }
  if (t != 0) status = 0;  // (what all threads see alike is reported once)
  P.g = mpGridOf(a.b);
  const uint4* __restrict__ descC = (const uint4*)a.desc + (size_t)fc * cap * 2;
  const uint4* __restrict__ descQ = a.pointDesc ? (const uint4*)a.pointDesc + (size_t)ps * cap * 2 : (const uint4*)a.desc + (size_t)fk * cap * 2;
  int* __restrict__ row = a.matches + (size_t)pair * cap;
  const int orbDist = a.orbDist < 255 ? a.orbDist : 255;  // (`dist < bestDist` from 256 never picks a candidate at 256)

  // ---- start state
  for (int c = t; c < MP_START_WORDS; c += MP_THREADS) cellStart[c] = 0;
  for (int k = t; k < kpBitWords(nK); k += MP_THREADS) found[k] = 0;
  for (int k = t; k < words; k += MP_THREADS) taken[k] = 0;
  if (t < ORBX_MAX_LEVELS) sScale[t] = a.scale[t];
  if (t < MATCH_HISTO_LENGTH) hist[t] = 0;
  if (t < 3) { sKeep[t] = -1; sKeepV[t] = 0; }
  if (t < C_FIELDS) sCnt[t] = 0;
  if (t == 0) { sAny = 0; sListN = 0; }
  __syncthreads();
  // ---- rule 1, and the grid's counts
  int cnt[C_FIELDS];
#pragma unroll
  for (int k = 0; k < C_FIELDS; k++) cnt[k] = 0;
  for (int j = t; j < nC; j += MP_THREADS) {
    const int i = row[j];
    if (i < 0) continue;
    if (i >= nK) {
      status |= ORBX_KFPROJ_BAD_INPUT;
      atomicOr(&taken[j >> 5], 1u << (j & 31));
      continue;
    }
    atomicOr(&found[i >> 5], 1u << (i & 31));
    if (outl && outl[j] != 0) {
      row[j] = -1;
      cnt[C_CLEARED]++;
    } else {
      atomicOr(&taken[j >> 5], 1u << (j & 31));
    }
  }
  mpGridCount(P.g, P.kpsC, nC, cellStart);
  __syncthreads();
  mpGridFill(P.g, P.kpsC, nC, cellStart, cellIdx, sWave);
  __syncthreads();

  // ---- rules 2 and 3: one pass over KF's points, the survivors appended in ascending index
  for (int base = 0; base < nK; base += MP_THREADS) {  // (uniform)
    const int i = base + t;
    int where = -1, level = 0;  // -1: not a point of rule 2
    if (i < nK) {
      const bool isFound = (found[i >> 5] >> (i & 31)) & 1u;
      cnt[C_FOUND] += isFound;
      if (!isFound && (!mask || mask[i] != 0)) {
        cnt[C_POINTS]++;
        bool behind = false;
        where = poseOk ? kpSearched(a, P, sScale, i, &level, &behind, &status) : (int)KP_DROPPED;
        cnt[C_BEHIND_KEPT] += behind && where != KP_OUT_IMAGE && where != KP_DROPPED;
        cnt[C_OUT_IMAGE] += where == KP_OUT_IMAGE;
        cnt[C_OUT_DISTANCE] += where == KP_OUT_DISTANCE;
      }
    }
    const bool in = where == KP_SEARCHED;
    const uint64_t ballot = __ballot(in);
    if (lane == 0) sWave[w] = __popcll(ballot);
    __syncthreads();
    int pos = sListN + __popcll(ballot & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; k++) pos += sWave[k];
    if (in) {  // (pos < nK <= cap: at most one entry per point)
      list[pos] = (uint16_t)((uint32_t)i | KP_PENDING);
      lev[pos] = (uint8_t)level;
    }
    __syncthreads();
    if (t == MP_THREADS - 1) sListN = pos + (in ? 1 : 0);
  }
  __syncthreads();
  const int nList = sListN;
  if (t == 0) sAny = nList > 0;
  for (int j = t; j < nC; j += MP_THREADS) claim[j] = KP_FREE;  // (the "found" bits are read no more)
  __syncthreads();

  // ---- the rounds
  int rounds = 0;
  while (sAny) {  // (uniform: read behind a barrier, written again only behind the next one)
    // last round's matches are taken; everything else untaken is free again
    for (int j = t; j < nC; j += MP_THREADS) {
      if (claim[j] & KP_MATCHED) atomicOr(&taken[j >> 5], 1u << (j & 31));
      else claim[j] = KP_FREE;
    }
    __syncthreads();
    if (t == 0) sAny = 0;
    // A. the claims: the untaken candidates within orb_dist
    for (int p = t; p < nList; p += MP_THREADS) {
      const uint32_t e = list[p];
      if (!(e & KP_PENDING)) continue;
      const int i = (int)(e & KP_INDEX), level = lev[p];
      float u = 0.0f, v = 0.0f;
      bool ignored;
      kpProject(a, P, i, &u, &v, &ignored);  // (the same arithmetic as in the pass: it succeeds again)
      const uint4 q0 = descQ[(size_t)i * 2], q1 = descQ[(size_t)i * 2 + 1];
      kpWalk(P, cellStart, cellIdx, u, v, a.th * sScale[level], level, [&](int j, int) {
        if ((taken[j >> 5] >> (j & 31)) & 1u) return;
        if (mpDistance(q0, q1, descC[(size_t)j * 2], descC[(size_t)j * 2 + 1]) <= orbDist) atomicMin(&claim[j], p);
      });
    }
    __syncthreads();
    // B. a point that holds every claim it made is final
    for (int p = t; p < nList; p += MP_THREADS) {
      const uint32_t e = list[p];
      if (!(e & KP_PENDING)) continue;
      const int i = (int)(e & KP_INDEX), level = lev[p];
      float u = 0.0f, v = 0.0f;
      bool ignored;
      kpProject(a, P, i, &u, &v, &ignored);
      const uint4 q0 = descQ[(size_t)i * 2], q1 = descQ[(size_t)i * 2 + 1];
      // rule 5 on what is untaken now, and on what the entry left untaken (a taken feature without the match bit is the entry's)
      uint64_t now = ~0ull, alone = ~0ull;
      int nCand = 0;
      bool mine = true;
      kpWalk(P, cellStart, cellIdx, u, v, a.th * sScale[level], level, [&](int j, int c) {
        nCand++;
        const bool isTaken = (taken[j >> 5] >> (j & 31)) & 1u;
        const int cl = claim[j];
        if (isTaken && !(cl & KP_MATCHED)) return;
        const int d = mpDistance(q0, q1, descC[(size_t)j * 2], descC[(size_t)j * 2 + 1]);
        const uint64_t key = kpKey(d, c, j);
        alone = key < alone ? key : alone;
        if (isTaken) return;
        now = key < now ? key : now;
        if (d <= orbDist && (cl & ~KP_MATCHED) != p) mine = false;
      });
      if (!mine) {
        sAny = 1;
        continue;
      }
      list[p] = (uint16_t)(e & ~KP_PENDING);
      if (nCand == 0) continue;
      cnt[C_WITH_CAND]++;
      const int got = kpDecide(now, orbDist), free = kpDecide(alone, orbDist);
      cnt[C_OVER_DIST] += got < 0;
      cnt[C_DISPLACED] += got != free;
      if (got >= 0) {
        claim[got] = p | KP_MATCHED;  // (claim[got] == p: only this thread writes it now)
        cnt[C_NMATCHES]++;
      }
    }
    rounds++;
    __syncthreads();
  }

  // ---- rule 7 over the new matches, then a feature with a new match that stays writes it
  if (a.checkOri) {  // (uniform)
    for (int j = t; j < nC; j += MP_THREADS) {
      const int c = claim[j];
      if (c & KP_MATCHED) {
        const int bin = matchRotBin(kpsK[list[c & ~KP_MATCHED] & KP_INDEX].angle, P.kpsC[j].angle);
        if (bin >= 0) atomicAdd(&hist[bin], 1);
      }
    }
    __syncthreads();
    if (t < MATCH_HISTO_LENGTH) {
      const int v = hist[t], place = matchHistPlace(hist, t);
      if (v > 0 && place < 3) { sKeep[place] = t; sKeepV[place] = v; }
    }
    __syncthreads();
  }
  const int ind1 = sKeep[0];
  int ind2 = sKeep[1], ind3 = sKeep[2];
  matchDropMaxima(sKeepV[0], sKeepV[1], sKeepV[2], &ind2, &ind3);
  for (int j = t; j < nC; j += MP_THREADS) {
    const int c = claim[j];
    if (!(c & KP_MATCHED)) continue;
    int m = (int)(list[c & ~KP_MATCHED] & KP_INDEX);
    if (a.checkOri) {
      const int bin = matchRotBin(kpsK[m].angle, P.kpsC[j].angle);
      if (bin >= 0 && bin != ind1 && bin != ind2 && bin != ind3) {
        m = -1;
        cnt[C_ROT_REMOVED]++;
        cnt[C_NMATCHES]--;
      }
    }
    row[j] = m;
  }
  if (status) atomicOr(&sCnt[C_STATUS], status);
#pragma unroll
  for (int k = 1; k < C_ROUNDS; k++)
    if (cnt[k]) atomicAdd(&sCnt[k], cnt[k]);
  __syncthreads();
  if (t < C_FIELDS) ((int32_t*)(a.res + pair))[t] = t == C_ROUNDS ? rounds : sCnt[t];
}

}  // namespace

hipError_t launch_match_kfproj(hipStream_t st, const MatchKfProjArgs& a) {
  static_assert(sizeof(orbx_kfproj_result) == 4 * C_FIELDS, "thirteen int32");
  static_assert(kpLdsBytes(BOW_MAX_FEATURES) + 512 <= 160 * 1024, "a workgroup's LDS at the largest capacity");
  const size_t lds = kpLdsBytes(a.cap);
  if (lds > 48 * 1024) {  // (beyond the default limit of a launch's dynamic LDS)
    const hipError_t e = hipFuncSetAttribute((const void*)k_match_kfproj, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_match_kfproj, dim3((unsigned)a.nPairs), dim3(MP_THREADS), lds, st, a);
  return hipGetLastError();
}

}  // namespace orbx
