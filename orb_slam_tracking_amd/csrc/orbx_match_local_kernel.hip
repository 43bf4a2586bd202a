// orbx_match_local_kernel.hip — Tracking::SearchLocalPoints: Frame::isInFrustum, MapPoint::PredictScale and
// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) for a batch of (frame F, map set) pairs (include/orbx.h,
// "matching the local map by projection").  gfx950, wave64.
//
// One workgroup of MP_THREADS threads per pair, one launch per call.
//   step 1  every feature of F reads its entry of the match row: the points the frame has become "seen" (a bit set over the map
//           set), the features that keep their point "taken" (a bit set over F), outliers' entries are cleared.
//   grid    F's grid in LDS as k_match_proj builds it (orbx_match_grid.h).
//   step 2-3 ONE pass over the map set in slices of MP_THREADS points: the frustum test and the scale, and an order-preserving
//           scan (ballot inside a wave, the waves' sums through LDS) that appends the points in view to an LDS list in
//           ascending point index -- a local map is mostly out of view, and "earlier" must remain "smaller": from here on a
//           point is its position p in the list.  An entry keeps the index, the radius class (viewCos > 0.998) and a
//           "pending" bit; the level lies in a byte beside it.  (u, v) are not kept -- at 16384 points they do not fit beside
//           the claims -- and are recomputed from the point, by the same arithmetic, when a point walks its window: three
//           dot products and one division, none of the f64 work.
//   steps 4-6 in rounds, see below; then a feature with a new match writes it to the row.
//
// The sequential rule with a second-best.  Point p's outcome (its match, or none by TH_HIGH or by the ratio test) is a function
// of the set U(p) of candidates of its window that nobody has taken when its turn comes: best and second-best are the two
// smallest of U(p) under the key (distance, position in the window's order), whatever order a walk meets them in.  A round:
//   A. every pending p claims, with an LDS atomicMin of p into claim[j], EVERY untaken candidate j of its window -- all of them,
//      not a subset narrowed by distance: any of them can become best or second-best once others are taken.
//   B. p is final iff claim[j] == p for every untaken candidate j of its window (none at all included).  Only then it computes
//      the distances, the two smallest and the decision; a match sets a bit in claim[bestIdx], which no other point's test is
//      changed by (it fails on that j with or without the bit), and the "taken" bit is set at the start of the next round, so
//      that a round reads one state of "taken" throughout and `rounds` is the same on every run.
// This equals the sequential walk.  Call a state sound when every final point holds its sequential outcome and "taken" is the
// entry's set plus the final points' matches.  The start is sound.  In a sound state let p be pending and hold every claim of
// its window.  (a) No final point q > p matched inside p's window: in the round q became final, p was pending (it is still), so
// an untaken candidate of both windows carried a claim <= p < q and q was not final.  (b) No pending point q < p can take a
// candidate j of p's window later: j would be untaken now (taken only grows) and in q's window, so claim[j] <= q < p.  Points
// before p that are final have their sequential matches, which are in "taken".  So the untaken candidates of p's window now are
// exactly U(p) of the sequential walk, and p's outcome computed from them is the sequential one: the state stays sound.  The
// smallest pending point holds every claim it makes, so every round resolves at least one point and the loop ends; points in
// different parts of the image never meet, and the rounds needed are the longest chain of points that wait for one another.
// No float atomics; integer atomics are min, or and add only, so nothing depends on the order in which they land.
//
// LDS, sized from both capacities by the launcher (mlLdsBytes): 12304 bytes of cell starts; 4 bytes of claims per feature (the
// same words hold step 1's "seen" bits until the list is built); a bit per feature; 2 bytes of cell-ordered indices per feature;
// 2 bytes of list entry and 1 of level per map point -- 30.1 KB for capacity 1024 with a map capacity of 4096, 158.0 KB with both
// at ORBX_BOW_MAX_FEATURES, plus 176 bytes of static LDS.  93 VGPRs, no scratch (profiles/match_local_kernel_stats.txt).
#include <hip/hip_runtime.h>

#include "orbx_launch.h"
#include "orbx_match_grid.h"

namespace orbx {
namespace {

constexpr int ML_TH_HIGH = 100;          // ORBmatcher::TH_HIGH
constexpr int ML_FREE = 0x3fffffff;      // claim[j]: nobody claims j
constexpr int ML_MATCHED = 0x40000000;   // claim[j]: ... | this bit: the claimant is final on j (a new match)
constexpr uint32_t ML_INDEX = 0x3fffu;   // list[p]: the point's index (< 16384) ...
constexpr uint32_t ML_CLOSE = 0x4000u;   // ... viewCos > 0.998
constexpr uint32_t ML_PENDING = 0x8000u; // ... not final yet
static_assert(BOW_MAX_FEATURES <= (int)ML_INDEX + 1, "a list entry's index is 14 bits");
enum { ML_DROPPED, ML_BEHIND, ML_OUT_IMAGE, ML_OUT_DISTANCE, ML_OUT_ANGLE, ML_IN_VIEW };
// sCnt: the fields of orbx_local_result in their order
enum { C_STATUS, C_NMATCHES, C_POINTS, C_SEEN, C_BEHIND, C_OUT_IMAGE, C_OUT_DISTANCE, C_OUT_ANGLE, C_IN_VIEW, C_WITH_CAND,
       C_OVER_TH, C_RATIO, C_DISPLACED, C_CLEARED, C_ROUNDS, C_FIELDS };

__host__ __device__ constexpr int mlBitWords(int n) { return (n + 31) >> 5; }
__host__ __device__ constexpr int mlClaimWords(int cap, int mapCap) { return cap > mlBitWords(mapCap) ? cap : mlBitWords(mapCap); }
__host__ __device__ constexpr size_t mlLdsBytes(int cap, int mapCap) {
  return (size_t)4 * (MP_START_WORDS + mlClaimWords(cap, mapCap) + mlBitWords(cap)) + (size_t)2 * ((cap + 1) & ~1) +
         (size_t)2 * ((mapCap + 1) & ~1) + (size_t)((mapCap + 3) & ~3);
}

struct MlPair {
  const orbx_keypoint* kps;
  const float *pts, *normals, *dist;
  float R[9], t[3], Ow[3];
  MpGrid g;
};

// step 2's projection of point i: false when it is behind the camera or outside the image (*why says which)
__device__ __forceinline__ bool mlProject(const MatchLocalArgs& a, const MlPair& P, int i, float* u, float* v, int* why) {
  const float X = P.pts[3 * (size_t)i], Y = P.pts[3 * (size_t)i + 1], Z = P.pts[3 * (size_t)i + 2];
  const float xc = ((P.R[0] * X + P.R[1] * Y) + P.R[2] * Z) + P.t[0];
  const float yc = ((P.R[3] * X + P.R[4] * Y) + P.R[5] * Z) + P.t[1];
  const float zc = ((P.R[6] * X + P.R[7] * Y) + P.R[8] * Z) + P.t[2];
  *why = ML_BEHIND;
  if (zc < 0.0f) return false;
  const float invz = 1.0f / zc;
  const float pu = (a.fx * xc) * invz + a.cx, pv = (a.fy * yc) * invz + a.cy;
  *why = ML_OUT_IMAGE;
  if (!mpFinite(pu) || !mpFinite(pv)) return false;
  if (pu < P.g.minX || pu > P.g.maxX || pv < P.g.minY || pv > P.g.maxY) return false;
  *u = pu;
  *v = pv;
  return true;
}

// steps 2 and 3 for point i (mask set, not seen, finite pose): where it ends, and for ML_IN_VIEW the level and the radius class
__device__ __forceinline__ int mlFrustum(const MatchLocalArgs& a, const MlPair& P, const float* __restrict__ scale, int i, int* level,
                                         bool* close, int* status) {
  const float* X = P.pts + 3 * (size_t)i;
  const float* N = P.normals + 3 * (size_t)i;
  const float minD = P.dist[2 * (size_t)i], maxD = P.dist[2 * (size_t)i + 1];
  if (!(mpFinite(X[0]) && mpFinite(X[1]) && mpFinite(X[2]) && mpFinite(N[0]) && mpFinite(N[1]) && mpFinite(N[2]) && mpFinite(minD) &&
        mpFinite(maxD))) {
    *status |= ORBX_LOCAL_NONFINITE;
    return ML_DROPPED;
  }
  float u, v;
  int why;
  if (!mlProject(a, P, i, &u, &v, &why)) return why;
  const float px = X[0] - P.Ow[0], py = X[1] - P.Ow[1], pz = X[2] - P.Ow[2];
  const float dist = (float)sqrt(((double)px * (double)px + (double)py * (double)py) + (double)pz * (double)pz);
  if (dist < 0.8f * minD || dist > 1.2f * maxD) return ML_OUT_DISTANCE;
  const float viewCos = (float)((((double)px * (double)N[0] + (double)py * (double)N[1]) + (double)pz * (double)N[2]) / (double)dist);
  if (viewCos < 0.5f) return ML_OUT_ANGLE;
  const float ratio = maxD / dist;
  if (ratio != ratio) {
    *status |= ORBX_LOCAL_NONFINITE;
    return ML_DROPPED;
  }
  int lv = 0;
  for (int n = 0; n < a.nLevels - 1; n++) lv += ratio > scale[n];
  *level = lv;
  *close = viewCos > 0.998f;
  return ML_IN_VIEW;
}

// Calls f(j, cell) for every candidate of the window (step 4) until f returns false; returns whether f never did.
template <class F>
__device__ __forceinline__ bool mlWalk(const MlPair& P, const int* cellStart, const uint16_t* cellIdx, float u, float v, float r,
                                       int level, F f) {
  int x0, x1, y0, y1;
  if (!mpWindow(P.g, u, v, r, &x0, &x1, &y0, &y1)) return true;
  for (int cx = x0; cx <= x1; cx++)
    for (int cy = y0; cy <= y1; cy++) {
      const int c = cx * ORBX_GRID_ROWS + cy;
      const int k1 = cellStart[c + 1];
      for (int k = cellStart[c]; k < k1; k++) {
        const int j = cellIdx[k];
        const orbx_keypoint* kp = P.kps + j;
        const int lev = kp->octave;
        if (!(lev >= level - 1 && lev <= level)) continue;  // (bCheckLevels holds: maxLevel = level >= 0)
        const float dx = kp->x - u, dy = kp->y - v;
        if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
        if (!f(j, c)) return false;
      }
    }
  return true;
}

// the streaming update of step 5 as the two smallest keys (distance, cell, index): the window's order is (cell, index)
struct MlTwo {
  uint64_t k1 = ~0ull, k2 = ~0ull;
  int lev1 = -1, lev2 = -1;
  __device__ __forceinline__ void add(int d, int cell, int j, int lev) {
    const uint64_t k = ((uint64_t)(uint32_t)d << 32) | ((uint32_t)cell << 16) | (uint32_t)j;
    if (k < k1) { k2 = k1; lev2 = lev1; k1 = k; lev1 = lev; }
    else if (k < k2) { k2 = k; lev2 = lev; }
  }
  // step 6: the feature, or -1 with *why = 1 (over TH_HIGH) or 2 (the ratio test)
  __device__ __forceinline__ int decide(float nnratio, int* why) const {
    const int d1 = k1 == ~0ull ? 256 : (int)(k1 >> 32), d2 = k2 == ~0ull ? 256 : (int)(k2 >> 32);
    *why = 1;
    if (d1 > ML_TH_HIGH) return -1;
    *why = 2;
    if (lev1 == lev2 && (float)d1 > nnratio * (float)d2) return -1;
    *why = 0;
    return (int)(k1 & 0xffffu);
  }
};

__global__ __launch_bounds__(MP_THREADS) void k_match_local(MatchLocalArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t mlLds[];
  __shared__ float sScale[ORBX_MAX_LEVELS];
  __shared__ int sWave[MP_THREADS / 64];
  __shared__ int sCnt[C_FIELDS];
  __shared__ int sAny, sListN;
  const int pair = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int cap = a.cap, mapCap = a.mapCap, words = mlBitWords(cap);
  int* const cellStart = (int*)mlLds;                                    // [MP_CELLS + 1]
  int* const claim = cellStart + MP_START_WORDS;                         // [cap] per feature: the smallest claimant
  uint32_t* const seen = (uint32_t*)claim;                               // until the list is built: bits over the map set
  uint32_t* const taken = (uint32_t*)(claim + mlClaimWords(cap, mapCap));  // [words] bits over F's features
  uint16_t* const cellIdx = (uint16_t*)(taken + words);                  // [cap] F's features by cell
  uint16_t* const list = cellIdx + ((cap + 1) & ~1);                     // [mapCap] the points in view, ascending
  uint8_t* const lev = (uint8_t*)(list + ((mapCap + 1) & ~1));           // [mapCap] their levels

  const int fr = a.pairs[pair], set = a.pairs[a.nPairs + pair];
  const int rawF = a.n[fr], rawM = a.mapN[set];
  const int nF = mpClamp(rawF, cap), nM = mpClamp(rawM, mapCap);
  MlPair P;
  P.kps = a.kps + (size_t)fr * cap;
  P.pts = a.mapPoints + (size_t)set * mapCap * 3;
  P.normals = a.mapNormals + (size_t)set * mapCap * 3;
  P.dist = a.mapDist + (size_t)set * mapCap * 2;
  const uint8_t* mask = a.mapMask ? a.mapMask + (size_t)set * mapCap : nullptr;
  const uint8_t* outl = a.outlier ? a.outlier + (size_t)pair * cap : nullptr;
  uint8_t* view = a.pointView ? a.pointView + (size_t)pair * mapCap : nullptr;
  int status = (rawF != nF || rawM != nM) ? ORBX_LOCAL_BAD_INPUT : 0;
  bool poseOk = true;
  {
    const float* pose = a.pose + (size_t)pair * 12;
#pragma unroll
    for (int k = 0; k < 9; k++) { P.R[k] = pose[k]; poseOk = poseOk && mpFinite(P.R[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) { P.t[k] = pose[9 + k]; poseOk = poseOk && mpFinite(P.t[k]); }
    if (!poseOk) status |= ORBX_LOCAL_NONFINITE;
#pragma unroll
    for (int k = 0; k < 3; k++) P.Ow[k] = -((P.R[k] * P.t[0] + P.R[3 + k] * P.t[1]) + P.R[6 + k] * P.t[2]);
  }
  if (t != 0) status = 0;  // (what all threads see alike is reported once)
  P.g = mpGridOf(a.b);
  const uint4* __restrict__ descF = (const uint4*)a.desc + (size_t)fr * cap * 2;
  const uint4* __restrict__ descM = (const uint4*)a.mapDesc + (size_t)set * mapCap * 2;
  int* __restrict__ row = a.matches + (size_t)pair * cap;

  // ---- start state
  for (int c = t; c < MP_START_WORDS; c += MP_THREADS) cellStart[c] = 0;
  for (int k = t; k < mlBitWords(nM); k += MP_THREADS) seen[k] = 0;
  for (int k = t; k < words; k += MP_THREADS) taken[k] = 0;
  if (t < ORBX_MAX_LEVELS) sScale[t] = a.scale[t];
  if (t < C_FIELDS) sCnt[t] = 0;
  if (t == 0) { sAny = 0; sListN = 0; }
  __syncthreads();
  // ---- step 1, and the grid's counts
  int cnt[C_FIELDS];
#pragma unroll
  for (int k = 0; k < C_FIELDS; k++) cnt[k] = 0;
  for (int j = t; j < nF; j += MP_THREADS) {
    const int i = row[j];
    if (i < 0) continue;
    if (i >= nM) {
      status |= ORBX_LOCAL_BAD_INPUT;
      atomicOr(&taken[j >> 5], 1u << (j & 31));
      continue;
    }
    atomicOr(&seen[i >> 5], 1u << (i & 31));
    if (outl && outl[j] != 0) {
      row[j] = -1;
      cnt[C_CLEARED]++;
    } else {
      atomicOr(&taken[j >> 5], 1u << (j & 31));
    }
  }
  mpGridCount(P.g, P.kps, nF, cellStart);
  __syncthreads();
  mpGridFill(P.g, P.kps, nF, cellStart, cellIdx, sWave);
  __syncthreads();

  // ---- steps 2 and 3: one pass over the map set, the points in view appended in ascending index
  for (int base = 0; base < nM; base += MP_THREADS) {  // (uniform)
    const int i = base + t;
    int where = -1, level = 0;  // -1: not a point of step 2
    bool close = false, isSeen = false;
    if (i < nM) {
      isSeen = (seen[i >> 5] >> (i & 31)) & 1u;
      cnt[C_SEEN] += isSeen;
      if (!isSeen && (!mask || mask[i] != 0)) {
        cnt[C_POINTS]++;
        where = poseOk ? mlFrustum(a, P, sScale, i, &level, &close, &status) : (int)ML_DROPPED;
        cnt[C_BEHIND] += where == ML_BEHIND;
        cnt[C_OUT_IMAGE] += where == ML_OUT_IMAGE;
        cnt[C_OUT_DISTANCE] += where == ML_OUT_DISTANCE;
        cnt[C_OUT_ANGLE] += where == ML_OUT_ANGLE;
        cnt[C_IN_VIEW] += where == ML_IN_VIEW;
      }
      if (view) view[i] = isSeen ? (uint8_t)ORBX_LOCAL_SEEN : (where == ML_IN_VIEW ? (uint8_t)level : (uint8_t)ORBX_LOCAL_NOT_IN_VIEW);
    }
    const bool in = where == ML_IN_VIEW;
    const uint64_t ballot = __ballot(in);
    if (lane == 0) sWave[w] = __popcll(ballot);
    __syncthreads();
    int pos = sListN + __popcll(ballot & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; k++) pos += sWave[k];
    if (in) {  // (pos < nM <= mapCap: at most one entry per point)
      list[pos] = (uint16_t)((uint32_t)i | (close ? ML_CLOSE : 0u) | ML_PENDING);
      lev[pos] = (uint8_t)level;
    }
    __syncthreads();
    if (t == MP_THREADS - 1) sListN = pos + (in ? 1 : 0);
  }
  __syncthreads();
  const int nList = sListN;
  if (t == 0) sAny = nList > 0;
  for (int j = t; j < nF; j += MP_THREADS) claim[j] = ML_FREE;  // (the "seen" bits are read no more)
  __syncthreads();

  // ---- the rounds
  int rounds = 0;
  while (sAny) {  // (uniform: read behind a barrier, written again only behind the next one)
    // last round's matches are taken; everything else untaken is free again
    for (int j = t; j < nF; j += MP_THREADS) {
      if (claim[j] & ML_MATCHED) atomicOr(&taken[j >> 5], 1u << (j & 31));
      else claim[j] = ML_FREE;
    }
    __syncthreads();
    if (t == 0) sAny = 0;
    // A. the claims
    for (int p = t; p < nList; p += MP_THREADS) {
      const uint32_t e = list[p];
      if (!(e & ML_PENDING)) continue;
      const int i = (int)(e & ML_INDEX), level = lev[p];
      float u = 0.0f, v = 0.0f;
      int ignored;
      mlProject(a, P, i, &u, &v, &ignored);  // (the same arithmetic as in the pass: it succeeds again)
      float r = (e & ML_CLOSE) ? 2.5f : 4.0f;
      if (a.th != 1.0f) r *= a.th;
      mlWalk(P, cellStart, cellIdx, u, v, r * sScale[level], level, [&](int j, int) {
        if (!((taken[j >> 5] >> (j & 31)) & 1u)) atomicMin(&claim[j], p);
        return true;
      });
    }
    __syncthreads();
    // B. a point that holds every claim of its window is final
    for (int p = t; p < nList; p += MP_THREADS) {
      const uint32_t e = list[p];
      if (!(e & ML_PENDING)) continue;
      const int i = (int)(e & ML_INDEX), level = lev[p];
      float u = 0.0f, v = 0.0f;
      int ignored;
      mlProject(a, P, i, &u, &v, &ignored);
      float r = (e & ML_CLOSE) ? 2.5f : 4.0f;
      if (a.th != 1.0f) r *= a.th;
      r *= sScale[level];
      const bool mine = mlWalk(P, cellStart, cellIdx, u, v, r, level, [&](int j, int) {
        return ((taken[j >> 5] >> (j & 31)) & 1u) || (claim[j] & ~ML_MATCHED) == p;
      });
      if (!mine) {
        sAny = 1;
        continue;
      }
      list[p] = (uint16_t)(e & ~ML_PENDING);
      // steps 5 and 6 on what is untaken now, and on what the entry left untaken (a taken feature without the match bit)
      const uint4 q0 = descM[(size_t)i * 2], q1 = descM[(size_t)i * 2 + 1];
      MlTwo now, alone;
      int nCand = 0;
      mlWalk(P, cellStart, cellIdx, u, v, r, level, [&](int j, int c) {
        nCand++;
        const bool isTaken = (taken[j >> 5] >> (j & 31)) & 1u;
        if (isTaken && !(claim[j] & ML_MATCHED)) return true;
        const int d = mpDistance(q0, q1, descF[(size_t)j * 2], descF[(size_t)j * 2 + 1]);
        const int o = P.kps[j].octave;
        alone.add(d, c, j, o);
        if (!isTaken) now.add(d, c, j, o);
        return true;
      });
      if (nCand == 0) continue;
      cnt[C_WITH_CAND]++;
      int why, whyAlone;
      const int got = now.decide(a.nnratio, &why), free = alone.decide(a.nnratio, &whyAlone);
      cnt[C_OVER_TH] += why == 1;
      cnt[C_RATIO] += why == 2;
      cnt[C_DISPLACED] += got != free;
      if (got >= 0) {
        claim[got] = p | ML_MATCHED;  // (claim[got] == p: only this thread writes it now)
        cnt[C_NMATCHES]++;
      }
    }
    rounds++;
    __syncthreads();
  }

  // ---- a feature with a new match writes it
  for (int j = t; j < nF; j += MP_THREADS) {
    const int c = claim[j];
    if (c & ML_MATCHED) row[j] = (int)(list[c & ~ML_MATCHED] & ML_INDEX);
  }
  if (status) atomicOr(&sCnt[C_STATUS], status);
#pragma unroll
  for (int k = 1; k < C_ROUNDS; k++)
    if (cnt[k]) atomicAdd(&sCnt[k], cnt[k]);
  __syncthreads();
  if (t < C_FIELDS) ((int32_t*)(a.res + pair))[t] = t == C_ROUNDS ? rounds : sCnt[t];
}

}  // namespace

hipError_t launch_match_local(hipStream_t st, const MatchLocalArgs& a) {
  static_assert(sizeof(orbx_local_result) == 4 * C_FIELDS, "fifteen int32");
  static_assert(mlLdsBytes(BOW_MAX_FEATURES, BOW_MAX_FEATURES) + 512 <= 160 * 1024, "a workgroup's LDS at the largest capacities");
  const size_t lds = mlLdsBytes(a.cap, a.mapCap);
  if (lds > 48 * 1024) {  // (beyond the default limit of a launch's dynamic LDS)
    const hipError_t e = hipFuncSetAttribute((const void*)k_match_local, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_match_local, dim3((unsigned)a.nPairs), dim3(MP_THREADS), lds, st, a);
  return hipGetLastError();
}

}  // namespace orbx
