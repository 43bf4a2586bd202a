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
// The sequential rule in orbx_match_rounds.h's claim rounds (the argument is there), with the claims narrowed.  Point p's outcome
// is a function of the set U(p) of candidates of its window that nobody has taken when its turn comes: the first smallest of
// U(p) under the key (distance, position in the window's order), a match iff that distance is <= orb_dist.  The claim set: C(p) =
// the untaken candidates of p's window with d(p, j) <= orb_dist, because a farther one is never the match: removing it from U(p)
// changes neither p's match nor the fact that it has none.  So
//   A. every pending p claims every untaken candidate j of its window with d(p, j) <= orb_dist;
//   B. p is final iff it holds the claim on every such j; only then it decides: its match is the smallest key among them.
// The narrowing costs a distance pass in phase A and saves rounds: with th = 10 a window holds many features, few of which lie
// within orb_dist of a given point.
//
// LDS, sized from the capacity by the launcher (MrLds::bytes with the list as long as the row): 12304 bytes of cell starts; 4
// bytes of claims per feature of C (the same words hold rule 1's "found" bits until the list is built); a bit per feature; 2 bytes
// of cell-ordered indices per feature; 2 bytes of list entry and 1 of level per point of KF -- 21.1 KB at capacity 1024, 158.0 KB
// at ORBX_BOW_MAX_FEATURES, plus 320 bytes of static LDS.  77 VGPRs, no scratch (profiles/match_kfproj_kernel_stats.txt).
#include <hip/hip_runtime.h>

#include "orbx_launch.h"
#include "orbx_match_hist.h"
#include "orbx_match_rounds.h"

namespace orbx {
namespace {

enum { KP_DROPPED, KP_OUT_IMAGE, KP_OUT_DISTANCE, KP_SEARCHED };
// sCnt: the fields of orbx_kfproj_result in their order
enum { C_STATUS, C_NMATCHES, C_POINTS, C_FOUND, C_BEHIND_KEPT, C_OUT_IMAGE, C_OUT_DISTANCE, C_WITH_CAND, C_OVER_DIST, C_DISPLACED,
       C_ROT_REMOVED, C_CLEARED, C_ROUNDS, C_FIELDS };

struct KpPair {
  const orbx_keypoint* kpsC;
  const float *pts, *dist;
  MrPose pose;
  float Ow[3];
  MpGrid g;
};

// rule 2's projection of point i: false when (u, v) is not finite or outside the bounds; *behind = zc < 0 (no test: a count)
__device__ __forceinline__ bool kpProject(const MatchKfProjArgs& a, const KpPair& P, int i, float* u, float* v, bool* behind) {
  float xc, yc, zc;
  mrToCamera(P.pose, P.pts, i, &xc, &yc, &zc);
  *behind = zc < 0.0f;
  return mrToImage(a.cam, P.g, xc, yc, 1.0f / zc, u, v);
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
  for (int n = 0; n < a.cam.nLevels - 1; n++) lv += ratio > scale[n];
  *level = lv;
  return KP_SEARCHED;
}

// rule 5's decision on the smallest key
__device__ __forceinline__ int kpDecide(uint64_t key, int orbDist) {
  return (key != MR_NO_KEY && mrKeyDistance(key) <= orbDist) ? mrKeyIndex(key) : -1;
}

__global__ __launch_bounds__(MP_THREADS) void k_match_kfproj(MatchKfProjArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t kpLds[];
  __shared__ float sScale[ORBX_MAX_LEVELS];
  __shared__ int hist[MATCH_HISTO_LENGTH];
  __shared__ int sKeep[3], sKeepV[3];
  __shared__ int sWave[MP_THREADS / 64];
  __shared__ int sCnt[C_FIELDS];
  __shared__ int sAny, sListN;
  const int pair = blockIdx.x, t = threadIdx.x;
  const int cap = a.cap;
  const MrLds L(kpLds, cap, cap);  // (L.had: the "found" bits over KF's features; L.list: the searched points)

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
  const bool poseOk = mrLoadPose(a.pose, pair, &P.pose);
  if (!poseOk) status |= ORBX_KFPROJ_NONFINITE;
  mrCameraCentre(P.pose, P.Ow);
  if (t != 0) status = 0;  // (what all threads see alike is reported once)
  P.g = mpGridOf(a.cam.b);
  const uint4* __restrict__ descC = (const uint4*)a.desc + (size_t)fc * cap * 2;
  const uint4* __restrict__ descQ = a.pointDesc ? (const uint4*)a.pointDesc + (size_t)ps * cap * 2 : (const uint4*)a.desc + (size_t)fk * cap * 2;
  int* __restrict__ row = a.matches + (size_t)pair * cap;
  const int orbDist = a.orbDist < 255 ? a.orbDist : 255;  // (`dist < bestDist` from 256 never picks a candidate at 256)

  // ---- start state
  L.clear(cap, nK);
  if (t < ORBX_MAX_LEVELS) sScale[t] = a.cam.scale[t];
  if (t < MATCH_HISTO_LENGTH) hist[t] = 0;
  if (t < 3) { sKeep[t] = -1; sKeepV[t] = 0; }
  if (t < C_FIELDS) sCnt[t] = 0;
  if (t == 0) { sAny = 0; sListN = 0; }
  __syncthreads();
  // ---- rule 1, and the grid's counts
  int cnt[C_FIELDS];
#pragma unroll
  for (int k = 0; k < C_FIELDS; k++) cnt[k] = 0;
  mrEntryPass(L, row, nC, nK, outl, ORBX_KFPROJ_BAD_INPUT, &status, &cnt[C_CLEARED]);
  mpGridCount(P.g, P.kpsC, nC, L.cellStart);
  __syncthreads();
  mpGridFill(P.g, P.kpsC, nC, L.cellStart, L.cellIdx, sWave);
  __syncthreads();

  // ---- rules 2 and 3: one pass over KF's points, the survivors appended in ascending index
  for (int base = 0; base < nK; base += MP_THREADS) {  // (uniform)
    const int i = base + t;
    int where = -1, level = 0;  // -1: not a point of rule 2
    if (i < nK) {
      const bool isFound = mrBit(L.had, i);
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
    mrAppend(L, where == KP_SEARCHED, (uint32_t)i, level, sWave, &sListN);
  }
  const int nList = mrListDone(L, nC, &sListN, &sAny);

  // ---- the rounds
  int rounds = 0;
  while (sAny) {  // (uniform: read behind a barrier, written again only behind the next one)
    mrRoundHead(L, nC, &sAny);
    // A. the claims: the untaken candidates within orb_dist
    for (int p = t; p < nList; p += MP_THREADS) {
      const uint32_t e = L.list[p];
      if (!(e & MR_PENDING)) continue;
      const int i = (int)(e & MR_INDEX), level = L.lev[p];
      float u = 0.0f, v = 0.0f;
      bool ignored;
      kpProject(a, P, i, &u, &v, &ignored);  // (the same arithmetic as in the pass: it succeeds again)
      const uint4 q0 = descQ[(size_t)i * 2], q1 = descQ[(size_t)i * 2 + 1];
      mrWalk(P.g, P.kpsC, L.cellStart, L.cellIdx, u, v, a.cam.th * sScale[level], level - 1, level + 1, [&](int j, int) {
        if (mrBit(L.taken, j)) return;
        if (mpDistance(q0, q1, descC[(size_t)j * 2], descC[(size_t)j * 2 + 1]) <= orbDist) atomicMin(&L.claim[j], p);
      });
    }
    __syncthreads();
    // B. a point that holds every claim it made is final
    for (int p = t; p < nList; p += MP_THREADS) {
      const uint32_t e = L.list[p];
      if (!(e & MR_PENDING)) continue;
      const int i = (int)(e & MR_INDEX), level = L.lev[p];
      float u = 0.0f, v = 0.0f;
      bool ignored;
      kpProject(a, P, i, &u, &v, &ignored);
      const uint4 q0 = descQ[(size_t)i * 2], q1 = descQ[(size_t)i * 2 + 1];
      // rule 5 on what is untaken now, and on what the entry left untaken (a taken feature without the match bit is the entry's)
      uint64_t now = MR_NO_KEY, alone = MR_NO_KEY;
      int nCand = 0;
      bool mine = true;
      mrWalk(P.g, P.kpsC, L.cellStart, L.cellIdx, u, v, a.cam.th * sScale[level], level - 1, level + 1, [&](int j, int c) {
        nCand++;
        const bool isTaken = mrBit(L.taken, j);
        const int cl = L.claim[j];
        if (isTaken && !(cl & MR_MATCHED)) return;
        const int d = mpDistance(q0, q1, descC[(size_t)j * 2], descC[(size_t)j * 2 + 1]);
        const uint64_t key = mrKey(d, c, j);
        alone = key < alone ? key : alone;
        if (isTaken) return;
        now = key < now ? key : now;
        if (d <= orbDist && (cl & ~MR_MATCHED) != p) mine = false;
      });
      if (!mine) {
        sAny = 1;
        continue;
      }
      L.list[p] = (uint16_t)(e & ~MR_PENDING);
      if (nCand == 0) continue;
      cnt[C_WITH_CAND]++;
      const int got = kpDecide(now, orbDist), free = kpDecide(alone, orbDist);
      cnt[C_OVER_DIST] += got < 0;
      cnt[C_DISPLACED] += got != free;
      if (got >= 0) {
        L.claim[got] = p | MR_MATCHED;  // (claim[got] == p: only this thread writes it now)
        cnt[C_NMATCHES]++;
      }
    }
    rounds++;
    __syncthreads();
  }

  // ---- rule 7 over the new matches, then a feature with a new match that stays writes it
  if (a.checkOri) {  // (uniform)
    for (int j = t; j < nC; j += MP_THREADS) {
      const int c = L.claim[j];
      if (c & MR_MATCHED) {
        const int bin = matchRotBin(kpsK[L.list[c & ~MR_MATCHED] & MR_INDEX].angle, P.kpsC[j].angle);
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
    const int c = L.claim[j];
    if (!(c & MR_MATCHED)) continue;
    int m = (int)(L.list[c & ~MR_MATCHED] & MR_INDEX);
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
  mrFlush(cnt, status, rounds, sCnt, (int32_t*)(a.res + pair));
}

}  // namespace

hipError_t launch_match_kfproj(hipStream_t st, const MatchKfProjArgs& a) {
  static_assert(sizeof(orbx_kfproj_result) == 4 * C_FIELDS && C_STATUS == 0 && C_ROUNDS == C_FIELDS - 1, "thirteen int32, as mrFlush writes them");
  static_assert(MrLds::bytes(BOW_MAX_FEATURES, BOW_MAX_FEATURES) + 512 <= 160 * 1024, "a workgroup's LDS at the largest capacity");
  static_assert(MrLds::bytes(1, 1) == 12324 && MrLds::bytes(1024, 1024) == 21648 && MrLds::bytes(16384, 16384) == 161808,
                "a list as long as the row, at capacities 1, 1024 and 16384: the layout decides the occupancy");
  return mrLaunch(k_match_kfproj, a.nPairs, MrLds::bytes(a.cap, a.cap), st, a);
}

}  // namespace orbx
