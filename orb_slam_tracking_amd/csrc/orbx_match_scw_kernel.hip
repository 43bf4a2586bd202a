// orbx_match_scw_kernel.hip — the loop-closing overload ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const
// vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, th) for a batch of (current keyframe C, map set) pairs, and the
// composition Scw = S12 * Tmw that LoopClosing::ComputeSim3 makes in front of it (include/orbx.h, "loop closing: matching the
// loop's points under Scw").  gfx950, wave64.
//
// k_match_scw: one workgroup of MP_THREADS threads per pair, one launch per call.
//   rule 1   every thread decomposes Scw into scw, Rcw, tcw and Ow (twelve divisions; all threads hold the same values).
//   rule 2   every feature of C reads its entry of the match row, through the table from the matched keyframe's features to the
//            map set when one is given: the points C has are "found" (a bit set over the map set), their features "taken" (a
//            bit set over C); an entry without a point in the set keeps its feature taken and finds nothing.
//   grid     C's grid in LDS as k_match_proj builds it (orbx_match_grid.h).
//   rules 3-6 ONE pass over the map set in slices of MP_THREADS points: the strict depth test, the half-open image test, the f64
//            distance, the f64 viewing-angle test and the level, and an order-preserving scan (ballot inside a wave, the waves'
//            sums through LDS) that appends the survivors to an LDS list in ascending point index: from here on a point is its
//            position p in the list.  An entry keeps the index and a "pending" bit; the level lies in a byte beside it.  (u, v)
//            are recomputed from the point, by the same arithmetic, when a point walks its window.
//   rule 7   in rounds, see below; then a feature with a new match writes it, and every feature that is not free counts in
//            n_total (rule 8).
//
// The sequential rule in orbx_match_rounds.h's claim rounds (the argument is there), with the claims narrowed as k_match_kfproj
// narrows them.  Point p's outcome is a function of the set U(p) of candidates of its window (octave in [level - 1, level]) that
// nobody has taken when its turn comes: the first smallest of U(p) under the key (distance, position in the window's order), a
// match iff that distance is <= th_low.  The claim set: C(p) = the untaken candidates of p's window with d(p, j) <= th_low.
// Nothing outside it can change p's outcome: the decision reads only the minimum of U(p).  A candidate j with d(p, j) > th_low
// is the minimum only when every candidate within th_low is gone, and then the outcome is "no match" whether j is in U(p) or
// not; when some candidate within th_low is left, the minimum lies among those and j is not it.  So striking j from U(p)
// changes neither p's match nor the fact that it has none -- which is the one property the rounds need.  (n_over_dist counts a
// point without a match, and does not record the distance; n_displaced compares picks, not distances.)  So
//   A. every pending p claims every untaken candidate j of its window with d(p, j) <= th_low;
//   B. p is final iff it holds the claim on every such j; only then it decides: its match is the smallest key among them.
//
// LDS, sized from both capacities by the launcher (MrLds::bytes): 12304 bytes of cell starts; 4 bytes of claims per feature (the
// same words hold rule 2's "found" bits until the list is built); a bit per feature; 2 bytes of cell-ordered indices per feature;
// 2 bytes of list entry and 1 of level per map point -- 30.1 KB for capacity 1024 with a map capacity of 4096, 158.0 KB with both
// at ORBX_BOW_MAX_FEATURES, plus 160 bytes of static LDS.  91 VGPRs, no scratch (profiles/match_scw_kernel_stats.txt).
//
// k_sim3_compose_scw: a lane per pair, f64 from the f32 inputs, no LDS.
#include <hip/hip_runtime.h>

#include "orbx_launch.h"
#include "orbx_match_rounds.h"

namespace orbx {
namespace {

enum { SC_DROPPED, SC_BEHIND, SC_OUT_IMAGE, SC_OUT_DISTANCE, SC_OUT_ANGLE, SC_SEARCHED };
// sCnt: the fields of orbx_scw_result in their order
enum { C_STATUS, C_NMATCHES, C_TOTAL, C_POINTS, C_FOUND, C_UNMAPPED, C_BEHIND, C_OUT_IMAGE, C_OUT_DISTANCE, C_OUT_ANGLE, C_WITH_CAND,
       C_OVER_DIST, C_DISPLACED, C_ROUNDS, C_FIELDS };

struct ScPair {
  const orbx_keypoint* kps;
  const float *pts, *normals, *dist;
  MrPose pose;  // Rcw, tcw of rule 1
  float Ow[3];
  MpGrid g;
};

// rule 1: Scw [12] (sR row-major, then t) -> Rcw = sR / scw, tcw = t / scw; false when a value is not finite or scw is not > 0
__device__ __forceinline__ bool scDecompose(const float* scw, int pair, MrPose* P) {
  scw += (size_t)pair * 12;
  float s[12];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 12; k++) { s[k] = scw[k]; ok = ok && mpFinite(s[k]); }
  const float norm = (float)sqrt((double)((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]));
  ok = ok && norm > 0.0f && mpFinite(norm);
#pragma unroll
  for (int k = 0; k < 9; k++) { P->R[k] = s[k] / norm; ok = ok && mpFinite(P->R[k]); }
#pragma unroll
  for (int k = 0; k < 3; k++) { P->t[k] = s[9 + k] / norm; ok = ok && mpFinite(P->t[k]); }
  return ok;
}

// rule 3's projection of point i: false when it is behind the camera or outside the image (*why says which)
__device__ __forceinline__ bool scProject(const MatchScwArgs& a, const ScPair& P, int i, float* u, float* v, int* why) {
  float xc, yc, zc;
  mrToCamera(P.pose, P.pts, i, &xc, &yc, &zc);
  *why = SC_BEHIND;
  if (zc < 0.0f) return false;
  *why = SC_OUT_IMAGE;
  const float invz = 1.0f / zc;
  const float pu = a.cam.fx * (xc * invz) + a.cam.cx, pv = a.cam.fy * (yc * invz) + a.cam.cy;
  if (!(pu >= P.g.minX && pu < P.g.maxX && pv >= P.g.minY && pv < P.g.maxY)) return false;  // (a NaN fails)
  *u = pu;
  *v = pv;
  return true;
}

// rules 3 to 6 for point i (mask set, not found, a finite similarity): where it ends, and for SC_SEARCHED the level
__device__ __forceinline__ int scSearched(const MatchScwArgs& a, const ScPair& P, const float* __restrict__ scale, int i, int* level,
                                          int* status) {
  const float* X = P.pts + 3 * (size_t)i;
  const float* N = P.normals + 3 * (size_t)i;
  const float minD = P.dist[2 * (size_t)i], maxD = P.dist[2 * (size_t)i + 1];
  if (!(mpFinite(X[0]) && mpFinite(X[1]) && mpFinite(X[2]) && mpFinite(N[0]) && mpFinite(N[1]) && mpFinite(N[2]) && mpFinite(minD) &&
        mpFinite(maxD))) {
    *status |= ORBX_SCW_NONFINITE;
    return SC_DROPPED;
  }
  float u, v;
  int why;
  if (!scProject(a, P, i, &u, &v, &why)) return why;
  const float px = X[0] - P.Ow[0], py = X[1] - P.Ow[1], pz = X[2] - P.Ow[2];
  const float dist = (float)sqrt(((double)px * (double)px + (double)py * (double)py) + (double)pz * (double)pz);
  if (dist < 0.8f * minD || dist > 1.2f * maxD) return SC_OUT_DISTANCE;
  const double dot = ((double)px * (double)N[0] + (double)py * (double)N[1]) + (double)pz * (double)N[2];
  if (dot < 0.5 * (double)dist) return SC_OUT_ANGLE;
  const float ratio = maxD / dist;
  if (ratio != ratio) {
    *status |= ORBX_SCW_NONFINITE;
    return SC_DROPPED;
  }
  int lv = 0;
  for (int n = 0; n < a.cam.nLevels - 1; n++) lv += ratio > scale[n];
  *level = lv;
  return SC_SEARCHED;
}

// rule 7's decision on the smallest key
__device__ __forceinline__ int scDecide(uint64_t key, int thLow) {
  return (key != MR_NO_KEY && mrKeyDistance(key) <= thLow) ? mrKeyIndex(key) : -1;
}

__global__ __launch_bounds__(MP_THREADS) void k_match_scw(MatchScwArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t scLds[];
  __shared__ float sScale[ORBX_MAX_LEVELS];
  __shared__ int sWave[MP_THREADS / 64];
  __shared__ int sCnt[C_FIELDS];
  __shared__ int sAny, sListN;
  const int pair = blockIdx.x, t = threadIdx.x;
  const int cap = a.cap, mapCap = a.mapCap;
  const MrLds L(scLds, cap, mapCap);  // (L.had: the "found" bits over the map set; L.list: the searched points)

  const int fc = a.pairs[pair], set = a.pairs[a.nPairs + pair];
  const int rawC = a.n[fc], rawM = a.mapN[set];
  const int nC = mpClamp(rawC, cap), nM = mpClamp(rawM, mapCap);
  ScPair P;
  P.kps = a.kps + (size_t)fc * cap;
  P.pts = a.mapPoints + (size_t)set * mapCap * 3;
  P.normals = a.mapNormals + (size_t)set * mapCap * 3;
  P.dist = a.mapDist + (size_t)set * mapCap * 2;
  const uint8_t* mask = a.mapMask ? a.mapMask + (size_t)set * mapCap : nullptr;
  const int32_t* xlate = a.kf2ToMap ? a.kf2ToMap + (size_t)pair * cap : nullptr;
  int status = (rawC != nC || rawM != nM) ? ORBX_SCW_BAD_INPUT : 0;
  const bool simOk = scDecompose(a.scw, pair, &P.pose);
  if (!simOk) status |= ORBX_SCW_NONFINITE;
  mrCameraCentre(P.pose, P.Ow);
  if (t != 0) status = 0;  // (what all threads see alike is reported once)
  P.g = mpGridOf(a.cam.b);
  const uint4* __restrict__ descC = (const uint4*)a.desc + (size_t)fc * cap * 2;
  const uint4* __restrict__ descM = (const uint4*)a.mapDesc + (size_t)set * mapCap * 2;
  int* __restrict__ row = a.matches + (size_t)pair * cap;
  const int thLow = a.thLow < 255 ? a.thLow : 255;  // (`dist < bestDist` from 256 never picks a candidate at 256)

  // ---- start state
  L.clear(cap, nM);
  if (t < ORBX_MAX_LEVELS) sScale[t] = a.cam.scale[t];
  if (t < C_FIELDS) sCnt[t] = 0;
  if (t == 0) { sAny = 0; sListN = 0; }
  __syncthreads();
  // ---- rule 2, and the grid's counts
  int cnt[C_FIELDS];
#pragma unroll
  for (int k = 0; k < C_FIELDS; k++) cnt[k] = 0;
  int never = 0;  // (no outlier input: nothing is cleared)
  mrEntryPass(L, row, nC, nM, nullptr, ORBX_SCW_BAD_INPUT, &status, &never, xlate, cap, ORBX_SCW_TAKEN_UNMAPPED, &cnt[C_UNMAPPED]);
  mpGridCount(P.g, P.kps, nC, L.cellStart);
  __syncthreads();
  mpGridFill(P.g, P.kps, nC, L.cellStart, L.cellIdx, sWave);
  __syncthreads();

  // ---- rules 3 to 6: one pass over the map set, the survivors appended in ascending index
  for (int base = 0; base < nM; base += MP_THREADS) {  // (uniform)
    const int i = base + t;
    int where = -1, level = 0;  // -1: not a point of rule 3
    if (i < nM) {
      const bool isFound = mrBit(L.had, i);
      cnt[C_FOUND] += isFound;
      if (!isFound && (!mask || mask[i] != 0)) {
        cnt[C_POINTS]++;
        where = simOk ? scSearched(a, P, sScale, i, &level, &status) : (int)SC_DROPPED;
        cnt[C_BEHIND] += where == SC_BEHIND;
        cnt[C_OUT_IMAGE] += where == SC_OUT_IMAGE;
        cnt[C_OUT_DISTANCE] += where == SC_OUT_DISTANCE;
        cnt[C_OUT_ANGLE] += where == SC_OUT_ANGLE;
      }
    }
    mrAppend(L, where == SC_SEARCHED, (uint32_t)i, level, sWave, &sListN);
  }
  const int nList = mrListDone(L, nC, &sListN, &sAny);

  // ---- the rounds
  int rounds = 0;
  while (sAny) {  // (uniform: read behind a barrier, written again only behind the next one)
    mrRoundHead(L, nC, &sAny);
    // A. the claims: the untaken candidates within th_low
    for (int p = t; p < nList; p += MP_THREADS) {
      const uint32_t e = L.list[p];
      if (!(e & MR_PENDING)) continue;
      const int i = (int)(e & MR_INDEX), level = L.lev[p];
      float u = 0.0f, v = 0.0f;
      int ignored;
      scProject(a, P, i, &u, &v, &ignored);  // (the same arithmetic as in the pass: it succeeds again)
      const uint4 q0 = descM[(size_t)i * 2], q1 = descM[(size_t)i * 2 + 1];
      mrWalk(P.g, P.kps, L.cellStart, L.cellIdx, u, v, a.cam.th * sScale[level], level - 1, level, [&](int j, int) {
        if (mrBit(L.taken, j)) return;
        if (mpDistance(q0, q1, descC[(size_t)j * 2], descC[(size_t)j * 2 + 1]) <= thLow) atomicMin(&L.claim[j], p);
      });
    }
    __syncthreads();
    // B. a point that holds every claim it made is final
    for (int p = t; p < nList; p += MP_THREADS) {
      const uint32_t e = L.list[p];
      if (!(e & MR_PENDING)) continue;
      const int i = (int)(e & MR_INDEX), level = L.lev[p];
      float u = 0.0f, v = 0.0f;
      int ignored;
      scProject(a, P, i, &u, &v, &ignored);
      const uint4 q0 = descM[(size_t)i * 2], q1 = descM[(size_t)i * 2 + 1];
      // rule 7 on what is untaken now, and on what the entry left untaken (a taken feature without the match bit is the entry's)
      uint64_t now = MR_NO_KEY, alone = MR_NO_KEY;
      int nCand = 0;
      bool mine = true;
      mrWalk(P.g, P.kps, L.cellStart, L.cellIdx, u, v, a.cam.th * sScale[level], level - 1, level, [&](int j, int c) {
        nCand++;
        const bool isTaken = mrBit(L.taken, j);
        const int cl = L.claim[j];
        if (isTaken && !(cl & MR_MATCHED)) return;
        const int d = mpDistance(q0, q1, descC[(size_t)j * 2], descC[(size_t)j * 2 + 1]);
        const uint64_t key = mrKey(d, c, j);
        alone = key < alone ? key : alone;
        if (isTaken) return;
        now = key < now ? key : now;
        if (d <= thLow && (cl & ~MR_MATCHED) != p) mine = false;
      });
      if (!mine) {
        sAny = 1;
        continue;
      }
      L.list[p] = (uint16_t)(e & ~MR_PENDING);
      if (nCand == 0) continue;
      cnt[C_WITH_CAND]++;
      const int got = scDecide(now, thLow), free = scDecide(alone, thLow);
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

  // ---- a feature with a new match writes it; rule 8 counts every feature that is not free
  for (int j = t; j < nC; j += MP_THREADS) {
    const int c = L.claim[j];
    if (c & MR_MATCHED) row[j] = (int)(L.list[c & ~MR_MATCHED] & MR_INDEX);
    cnt[C_TOTAL] += (c & MR_MATCHED) || mrBit(L.taken, j);
  }
  mrFlush(cnt, status, rounds, sCnt, (int32_t*)(a.res + pair));
}

// Scw = S12 * Tmw for pair p in f64 from the f32 inputs: sR = s12 * (R12 * Rmw), t = s12 * (R12 * tmw) + t12, every sum of three
// products as (a + b) + c; twelve zeros when an input is not finite or s12 is not > 0.
__global__ __launch_bounds__(64) void k_sim3_compose_scw(Sim3ComposeArgs a) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= a.nPairs) return;
  const float* sim = a.sim3 + (size_t)p * 13;
  const float* pose = a.pose + (size_t)a.kf2[p] * 12;
  float* out = a.scw + (size_t)p * 12;
  double R12[9], t12[3], Rmw[9], tmw[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    ok = ok && mpFinite(sim[k]) && mpFinite(pose[k]);
    R12[k] = (double)sim[k];
    Rmw[k] = (double)pose[k];
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    ok = ok && mpFinite(sim[9 + k]) && mpFinite(pose[9 + k]);
    t12[k] = (double)sim[9 + k];
    tmw[k] = (double)pose[9 + k];
  }
  const float s12 = sim[12];
  ok = ok && mpFinite(s12) && s12 > 0.0f;
  const double s = (double)s12;
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double m = (R12[3 * r] * Rmw[c] + R12[3 * r + 1] * Rmw[3 + c]) + R12[3 * r + 2] * Rmw[6 + c];
      out[3 * r + c] = ok ? (float)(s * m) : 0.0f;
    }
    const double q = (R12[3 * r] * tmw[0] + R12[3 * r + 1] * tmw[1]) + R12[3 * r + 2] * tmw[2];
    out[9 + r] = ok ? (float)(s * q + t12[r]) : 0.0f;
  }
}

}  // namespace

hipError_t launch_match_scw(hipStream_t st, const MatchScwArgs& a) {
  static_assert(sizeof(orbx_scw_result) == 4 * C_FIELDS && C_STATUS == 0 && C_ROUNDS == C_FIELDS - 1, "fourteen int32, as mrFlush writes them");
  static_assert(MrLds::bytes(BOW_MAX_FEATURES, BOW_MAX_FEATURES) + 512 <= 160 * 1024, "a workgroup's LDS at the largest capacities");
  static_assert(MrLds::bytes(1024, 4096) == 30864, "capacity 1024 with a map capacity of 4096: the layout decides the occupancy");
  return mrLaunch(k_match_scw, a.nPairs, MrLds::bytes(a.cap, a.mapCap), st, a);
}

hipError_t launch_sim3_compose_scw(hipStream_t st, const Sim3ComposeArgs& a) {
  hipLaunchKernelGGL(k_sim3_compose_scw, dim3((unsigned)((a.nPairs + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
