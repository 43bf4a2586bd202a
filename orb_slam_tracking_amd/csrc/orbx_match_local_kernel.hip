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
// The sequential rule with a second-best, in orbx_match_rounds.h's claim rounds (the argument is there).  Point p's outcome (its
// match, or none by TH_HIGH or by the ratio test) is a function of the set U(p) of candidates of its window that nobody has
// taken when its turn comes: best and second-best are the two smallest of U(p) under the key (distance, position in the window's
// order), whatever order a walk meets them in.  The claim set: C(p) = ALL untaken candidates of p's window, not a subset narrowed
// by distance, because of the second-best: any of them can become best or second-best once others are taken.  So
//   A. every pending p claims every untaken candidate of its window;
//   B. p is final iff it holds the claim on every one of them; only then it computes the distances, the two smallest and the
//      decision.
//
// LDS, sized from both capacities by the launcher (MrLds::bytes): 12304 bytes of cell starts; 4 bytes of claims per feature (the
// same words hold step 1's "seen" bits until the list is built); a bit per feature; 2 bytes of cell-ordered indices per feature;
// 2 bytes of list entry and 1 of level per map point -- 30.1 KB for capacity 1024 with a map capacity of 4096, 158.0 KB with both
// at ORBX_BOW_MAX_FEATURES, plus 176 bytes of static LDS.  91 VGPRs, no scratch (profiles/match_local_kernel_stats.txt).
#include <hip/hip_runtime.h>

#include "orbx_launch.h"
#include "orbx_match_rounds.h"

namespace orbx {
namespace {

constexpr int ML_TH_HIGH = 100;          // ORBmatcher::TH_HIGH
constexpr uint32_t ML_CLOSE = 0x4000u;   // list[p]: beside MR_INDEX and MR_PENDING, viewCos > 0.998
enum { ML_DROPPED, ML_BEHIND, ML_OUT_IMAGE, ML_OUT_DISTANCE, ML_OUT_ANGLE, ML_IN_VIEW };
// sCnt: the fields of orbx_local_result in their order
enum { C_STATUS, C_NMATCHES, C_POINTS, C_SEEN, C_BEHIND, C_OUT_IMAGE, C_OUT_DISTANCE, C_OUT_ANGLE, C_IN_VIEW, C_WITH_CAND,
       C_OVER_TH, C_RATIO, C_DISPLACED, C_CLEARED, C_ROUNDS, C_FIELDS };

struct MlPair {
  const orbx_keypoint* kps;
  const float *pts, *normals, *dist;
  MrPose pose;
  float Ow[3];
  MpGrid g;
};

// step 2's projection of point i: false when it is behind the camera or outside the image (*why says which)
__device__ __forceinline__ bool mlProject(const MatchLocalArgs& a, const MlPair& P, int i, float* u, float* v, int* why) {
  float xc, yc, zc;
  mrToCamera(P.pose, P.pts, i, &xc, &yc, &zc);
  *why = ML_BEHIND;
  if (zc < 0.0f) return false;
  *why = ML_OUT_IMAGE;
  return mrToImage(a.cam, P.g, xc, yc, 1.0f / zc, u, v);
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
  for (int n = 0; n < a.cam.nLevels - 1; n++) lv += ratio > scale[n];
  *level = lv;
  *close = viewCos > 0.998f;
  return ML_IN_VIEW;
}

// the streaming update of step 5 as the two smallest keys (distance, cell, index): the window's order is (cell, index)
struct MlTwo {
  uint64_t k1 = MR_NO_KEY, k2 = MR_NO_KEY;
  int lev1 = -1, lev2 = -1;
  __device__ __forceinline__ void add(int d, int cell, int j, int lev) {
    const uint64_t k = mrKey(d, cell, j);
    if (k < k1) { k2 = k1; lev2 = lev1; k1 = k; lev1 = lev; }
    else if (k < k2) { k2 = k; lev2 = lev; }
  }
  // step 6: the feature, or -1 with *why = 1 (over TH_HIGH) or 2 (the ratio test)
  __device__ __forceinline__ int decide(float nnratio, int* why) const {
    const int d1 = k1 == MR_NO_KEY ? 256 : mrKeyDistance(k1), d2 = k2 == MR_NO_KEY ? 256 : mrKeyDistance(k2);
    *why = 1;
    if (d1 > ML_TH_HIGH) return -1;
    *why = 2;
    if (lev1 == lev2 && (float)d1 > nnratio * (float)d2) return -1;
    *why = 0;
    return mrKeyIndex(k1);
  }
};

__global__ __launch_bounds__(MP_THREADS) void k_match_local(MatchLocalArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t mlLds[];
  __shared__ float sScale[ORBX_MAX_LEVELS];
  __shared__ int sWave[MP_THREADS / 64];
  __shared__ int sCnt[C_FIELDS];
  __shared__ int sAny, sListN;
  const int pair = blockIdx.x, t = threadIdx.x;
  const int cap = a.cap, mapCap = a.mapCap;
  const MrLds L(mlLds, cap, mapCap);  // (L.had: the "seen" bits over the map set; L.list: the points in view)

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
  const bool poseOk = mrLoadPose(a.pose, pair, &P.pose);
  if (!poseOk) status |= ORBX_LOCAL_NONFINITE;
  mrCameraCentre(P.pose, P.Ow);
  if (t != 0) status = 0;  // (what all threads see alike is reported once)
  P.g = mpGridOf(a.cam.b);
  const uint4* __restrict__ descF = (const uint4*)a.desc + (size_t)fr * cap * 2;
  const uint4* __restrict__ descM = (const uint4*)a.mapDesc + (size_t)set * mapCap * 2;
  int* __restrict__ row = a.matches + (size_t)pair * cap;

  // ---- start state
  L.clear(cap, nM);
  if (t < ORBX_MAX_LEVELS) sScale[t] = a.cam.scale[t];
  if (t < C_FIELDS) sCnt[t] = 0;
  if (t == 0) { sAny = 0; sListN = 0; }
  __syncthreads();
  // ---- step 1, and the grid's counts
  int cnt[C_FIELDS];
#pragma unroll
  for (int k = 0; k < C_FIELDS; k++) cnt[k] = 0;
  mrEntryPass(L, row, nF, nM, outl, ORBX_LOCAL_BAD_INPUT, &status, &cnt[C_CLEARED]);
  mpGridCount(P.g, P.kps, nF, L.cellStart);
  __syncthreads();
  mpGridFill(P.g, P.kps, nF, L.cellStart, L.cellIdx, sWave);
  __syncthreads();

  // ---- steps 2 and 3: one pass over the map set, the points in view appended in ascending index
  for (int base = 0; base < nM; base += MP_THREADS) {  // (uniform)
    const int i = base + t;
    int where = -1, level = 0;  // -1: not a point of step 2
    bool close = false, isSeen = false;
    if (i < nM) {
      isSeen = mrBit(L.had, i);
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
    mrAppend(L, where == ML_IN_VIEW, (uint32_t)i | (close ? ML_CLOSE : 0u), level, sWave, &sListN);
  }
  const int nList = mrListDone(L, nF, &sListN, &sAny);

  // ---- the rounds
  int rounds = 0;
  while (sAny) {  // (uniform: read behind a barrier, written again only behind the next one)
    mrRoundHead(L, nF, &sAny);
    // A. the claims
    for (int p = t; p < nList; p += MP_THREADS) {
      const uint32_t e = L.list[p];
      if (!(e & MR_PENDING)) continue;
      const int i = (int)(e & MR_INDEX), level = L.lev[p];
      float u = 0.0f, v = 0.0f;
      int ignored;
      mlProject(a, P, i, &u, &v, &ignored);  // (the same arithmetic as in the pass: it succeeds again)
      float r = (e & ML_CLOSE) ? 2.5f : 4.0f;
      if (a.cam.th != 1.0f) r *= a.cam.th;
      mrWalk(P.g, P.kps, L.cellStart, L.cellIdx, u, v, r * sScale[level], level - 1, level, [&](int j, int) {
        if (!mrBit(L.taken, j)) atomicMin(&L.claim[j], p);
        return true;
      });
    }
    __syncthreads();
    // B. a point that holds every claim of its window is final
    for (int p = t; p < nList; p += MP_THREADS) {
      const uint32_t e = L.list[p];
      if (!(e & MR_PENDING)) continue;
      const int i = (int)(e & MR_INDEX), level = L.lev[p];
      float u = 0.0f, v = 0.0f;
      int ignored;
      mlProject(a, P, i, &u, &v, &ignored);
      float r = (e & ML_CLOSE) ? 2.5f : 4.0f;
      if (a.cam.th != 1.0f) r *= a.cam.th;
      r *= sScale[level];
      const bool mine = mrWalk(P.g, P.kps, L.cellStart, L.cellIdx, u, v, r, level - 1, level, [&](int j, int) {
        return mrBit(L.taken, j) || (L.claim[j] & ~MR_MATCHED) == p;
      });
      if (!mine) {
        sAny = 1;
        continue;
      }
      L.list[p] = (uint16_t)(e & ~MR_PENDING);
      // steps 5 and 6 on what is untaken now, and on what the entry left untaken (a taken feature without the match bit)
      const uint4 q0 = descM[(size_t)i * 2], q1 = descM[(size_t)i * 2 + 1];
      MlTwo now, alone;
      int nCand = 0;
      mrWalk(P.g, P.kps, L.cellStart, L.cellIdx, u, v, r, level - 1, level, [&](int j, int c) {
        nCand++;
        const bool isTaken = mrBit(L.taken, j);
        if (isTaken && !(L.claim[j] & MR_MATCHED)) return true;
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
        L.claim[got] = p | MR_MATCHED;  // (claim[got] == p: only this thread writes it now)
        cnt[C_NMATCHES]++;
      }
    }
    rounds++;
    __syncthreads();
  }

  // ---- a feature with a new match writes it
  for (int j = t; j < nF; j += MP_THREADS) {
    const int c = L.claim[j];
    if (c & MR_MATCHED) row[j] = (int)(L.list[c & ~MR_MATCHED] & MR_INDEX);
  }
  mrFlush(cnt, status, rounds, sCnt, (int32_t*)(a.res + pair));
}

}  // namespace

hipError_t launch_match_local(hipStream_t st, const MatchLocalArgs& a) {
  static_assert(sizeof(orbx_local_result) == 4 * C_FIELDS && C_STATUS == 0 && C_ROUNDS == C_FIELDS - 1, "fifteen int32, as mrFlush writes them");
  static_assert(MrLds::bytes(BOW_MAX_FEATURES, BOW_MAX_FEATURES) + 512 <= 160 * 1024, "a workgroup's LDS at the largest capacities");
  static_assert(MrLds::bytes(1024, 4096) == 30864, "capacity 1024 with a map capacity of 4096: the layout decides the occupancy");
  return mrLaunch(k_match_local, a.nPairs, MrLds::bytes(a.cap, a.mapCap), st, a);
}

}  // namespace orbx
