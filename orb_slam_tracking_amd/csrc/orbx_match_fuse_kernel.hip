// orbx_match_fuse_kernel.hip — ORBmatcher::Fuse(pKF, vpMapPoints, th) of LocalMapping::SearchInNeighbors and
// ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) of LoopClosing::SearchAndFuse for a batch of (keyframe, map set) pairs
// (include/orbx.h, "fusing map points into a keyframe").  gfx950, wave64.
//
// k_match_fuse<SCW>: one workgroup of MP_THREADS threads per pair, one launch per call; the form is a compile-time parameter.
//   phase 1  every feature reads its entry of the row: the points the keyframe has are a bit set over the map set (IsInKeyFrame).
//            The keyframe's grid in LDS as k_match_proj builds it (orbx_match_grid.h).
//   phase 2  a thread per point in a stride loop: the depth, image, distance and angle tests, the level, the window walk.  The
//            search has no "taken" rule, so a point's pick is its own: the first smallest distance is the smallest key (distance,
//            cell, index), as in k_match_sim3.  The pick goes to d_fuse_idx and, as 16 bits, to LDS.
//   phase 3  the resolution, in rounds.  Every pending point does an LDS atomicMin of its index into head[pick]; the point that
//            holds the head applies R1 to R4 to its feature and retires; a barrier; again until nothing is pending.  The lists of
//            different features never meet, and within one list the head is the smallest pending index, so round r resolves the
//            r-th point of every list in ascending order: the outcome is the sequential loop's, a function of the inputs alone,
//            and `rounds` is the longest list.  A decision is "chained" iff it is made in a round behind the first and meets no
//            bad occupant.  Worst case: every point of the set on one feature takes one round per point.
//            The state of a feature between rounds: its occupant is row[f] itself (the pair's own row in global memory, written
//            by one thread in one round and read by another behind the barrier); its modelled count is kept SATURATED at 65536 in
//            17 bits (16 in LDS plus a bit set): R3 compares it only with obs_i <= 65535, so every count above that decides
//            alike, and the CPU restatement, which keeps the plain sums, says the same.
// No float atomics; integer atomics are min, or and add only; nothing depends on the order in which they land.
//
// LDS, sized from both capacities by the launcher (FuLds::bytes): 2 bytes of pick per map point, a bit per map point, a bit per
// feature, and ONE region that holds the grid (12304 bytes of cell starts, 2 bytes of cell-ordered index per feature) during the
// search and the heads (4 bytes per feature) and counts (2 bytes per feature) during the resolution: 22.6 KB for capacity 1024
// with a map capacity of 4096, 132.0 KB with both at ORBX_BOW_MAX_FEATURES, plus 240 (pose form) or 176 (Scw form) bytes of static
// LDS.  75 / 87 VGPRs, no scratch (profiles/match_fuse_kernel_stats.txt).
#include <hip/hip_runtime.h>

#include "orbx_launch.h"
#include "orbx_match_rounds.h"

namespace orbx {
namespace {

enum { FU_DROPPED, FU_BEHIND, FU_OUT_IMAGE, FU_OUT_DISTANCE, FU_OUT_ANGLE, FU_SEARCHED };
// sCnt: the fields of orbx_fuse_result in their order
enum { C_STATUS, C_FUSED, C_POINTS, C_IN_KF, C_BEHIND, C_OUT_IMAGE, C_OUT_DISTANCE, C_OUT_ANGLE, C_WITH_CAND, C_OVER_DIST, C_ADDED,
       C_KEPT, C_REPLACED, C_BAD_OCC, C_CHAINED, C_ROUNDS, C_FIELDS };

constexpr int FU_NO_PICK = 0xffff;
constexpr int FU_MAX_OBS = 65535;

struct FuLds {
  uint16_t* pick;     // [mapCap] per point: the feature picked, FU_NO_PICK once resolved or without one
  uint32_t* inKf;     // [mrBitWords(mapCap)] bits over the points the row names
  uint32_t* over;     // [mrBitWords(cap)] bits over the features: the modelled count is 65536 (count[f] holds 0)
  int* cellStart;     // the region, during the search: [MP_START_WORDS] ...
  uint16_t* cellIdx;  // ... and [cap] the features by cell
  int* head;          // the region, during the resolution: [cap] the smallest pending point on the feature ...
  uint16_t* count;    // ... and [cap] the modelled count's low 16 bits

  __host__ __device__ static constexpr size_t region(int cap) {
    const size_t grid = (size_t)4 * MP_START_WORDS + (size_t)2 * ((cap + 1) & ~1), state = (size_t)4 * cap + (size_t)2 * ((cap + 1) & ~1);
    return grid > state ? grid : state;
  }
  __host__ __device__ static constexpr size_t bytes(int cap, int mapCap) {
    return (size_t)2 * ((mapCap + 1) & ~1) + (size_t)4 * (mrBitWords(mapCap) + mrBitWords(cap)) + region(cap);
  }
  __device__ __forceinline__ FuLds(uint32_t* base, int cap, int mapCap) {
    inKf = base;
    over = inKf + mrBitWords(mapCap);
    cellStart = (int*)(over + mrBitWords(cap));
    cellIdx = (uint16_t*)(cellStart + MP_START_WORDS);
    head = cellStart;
    count = (uint16_t*)(head + cap);
    pick = (uint16_t*)((uint8_t*)cellStart + region(cap));
  }
};

struct FuPair {
  const orbx_keypoint* kps;
  const float *pts, *normals, *dist;
  MrPose pose;
  float Ow[3];
  MpGrid g;
};

// rule 1 of the Scw matcher: Scw [12] (sR row-major, then t) -> Rcw = sR / scw, tcw = t / scw; false when a value is not finite or
// scw is not > 0
__device__ __forceinline__ bool fuDecompose(const float* scw, int pair, MrPose* P) {
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

// rules 2 to 4 for point i (mask set, not in the keyframe, a usable pose): where it ends, and for FU_SEARCHED (u, v) and the level
__device__ __forceinline__ int fuSearched(const MatchFuseArgs& a, const FuPair& P, const float* __restrict__ scale, int i, float* u,
                                          float* v, int* level, int* status) {
  const float* X = P.pts + 3 * (size_t)i;
  const float* N = P.normals + 3 * (size_t)i;
  const float minD = P.dist[2 * (size_t)i], maxD = P.dist[2 * (size_t)i + 1];
  if (!(mpFinite(X[0]) && mpFinite(X[1]) && mpFinite(X[2]) && mpFinite(N[0]) && mpFinite(N[1]) && mpFinite(N[2]) && mpFinite(minD) &&
        mpFinite(maxD))) {
    *status |= ORBX_FUSE_NONFINITE;
    return FU_DROPPED;
  }
  float xc, yc, zc;
  mrToCamera(P.pose, P.pts, i, &xc, &yc, &zc);
  if (zc < 0.0f) return FU_BEHIND;
  const float invz = 1.0f / zc;
  const float pu = a.cam.fx * (xc * invz) + a.cam.cx, pv = a.cam.fy * (yc * invz) + a.cam.cy;
  if (!(pu >= P.g.minX && pu < P.g.maxX && pv >= P.g.minY && pv < P.g.maxY)) return FU_OUT_IMAGE;  // (a NaN fails)
  const float px = X[0] - P.Ow[0], py = X[1] - P.Ow[1], pz = X[2] - P.Ow[2];
  const float dist = (float)sqrt(((double)px * (double)px + (double)py * (double)py) + (double)pz * (double)pz);
  if (dist < 0.8f * minD || dist > 1.2f * maxD) return FU_OUT_DISTANCE;
  const double dot = ((double)px * (double)N[0] + (double)py * (double)N[1]) + (double)pz * (double)N[2];
  if (dot < 0.5 * (double)dist) return FU_OUT_ANGLE;
  const float ratio = maxD / dist;
  if (ratio != ratio) {
    *status |= ORBX_FUSE_NONFINITE;
    return FU_DROPPED;
  }
  int lv = 0;
  for (int n = 0; n < a.cam.nLevels - 1; n++) lv += ratio > scale[n];
  *u = pu;
  *v = pv;
  *level = lv;
  return FU_SEARCHED;
}

// a count as R3 reads it: clamped into [0, 65535], flagged when that changed it
__device__ __forceinline__ int fuObs(int raw, int* status) {
  const int c = raw < 0 ? 0 : (raw > FU_MAX_OBS ? FU_MAX_OBS : raw);
  if (c != raw) *status |= ORBX_FUSE_BAD_INPUT;
  return c;
}

template <bool SCW>
__global__ __launch_bounds__(MP_THREADS) void k_match_fuse(MatchFuseArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t fuLds[];
  __shared__ float sScale[ORBX_MAX_LEVELS], sInvSigma2[ORBX_MAX_LEVELS];
  __shared__ int sWave[MP_THREADS / 64];
  __shared__ int sCnt[C_FIELDS];
  __shared__ int sAny;
  const int pair = blockIdx.x, t = threadIdx.x;
  const int cap = a.cap, mapCap = a.mapCap;
  const FuLds L(fuLds, cap, mapCap);

  const int fc = a.pairs[pair], set = a.pairs[a.nPairs + pair];
  const int rawC = a.n[fc], rawM = a.mapN[set];
  const int nC = mpClamp(rawC, cap), nM = mpClamp(rawM, mapCap);
  FuPair P;
  P.kps = a.kps + (size_t)fc * cap;
  P.pts = a.mapPoints + (size_t)set * mapCap * 3;
  P.normals = a.mapNormals + (size_t)set * mapCap * 3;
  P.dist = a.mapDist + (size_t)set * mapCap * 2;
  const uint8_t* mask = a.mapMask ? a.mapMask + (size_t)set * mapCap : nullptr;
  const int32_t* mapObs = SCW ? nullptr : a.mapObs + (size_t)set * mapCap;
  const int32_t* occObs = a.occObs ? a.occObs + (size_t)pair * cap : nullptr;
  int status = (rawC != nC || rawM != nM) ? ORBX_FUSE_BAD_INPUT : 0;
  const bool poseOk = SCW ? fuDecompose(a.pose, pair, &P.pose) : mrLoadPose(a.pose, pair, &P.pose);
  if (!poseOk) status |= ORBX_FUSE_NONFINITE;
  mrCameraCentre(P.pose, P.Ow);
  if (t != 0) status = 0;  // (what all threads see alike is reported once)
  P.g = mpGridOf(a.cam.b);
  const uint4* __restrict__ descC = (const uint4*)a.desc + (size_t)fc * cap * 2;
  const uint4* __restrict__ descM = (const uint4*)a.mapDesc + (size_t)set * mapCap * 2;
  int* row = a.matches + (size_t)pair * cap;
  int32_t* outIdx = a.fuseIdx + (size_t)pair * mapCap;
  uint8_t* outAct = a.fuseAct + (size_t)pair * mapCap;
  int32_t* outOther = a.fuseOther + (size_t)pair * mapCap;
  const int thLow = a.thLow;

  // ---- start state
  for (int c = t; c < MP_START_WORDS; c += MP_THREADS) L.cellStart[c] = 0;
  for (int k = t; k < mrBitWords(nM); k += MP_THREADS) L.inKf[k] = 0;
  for (int k = t; k < mrBitWords(cap); k += MP_THREADS) L.over[k] = 0;
  if (t < ORBX_MAX_LEVELS) { sScale[t] = a.cam.scale[t]; sInvSigma2[t] = a.invSigma2[t]; }
  if (t < C_FIELDS) sCnt[t] = 0;
  if (t == 0) sAny = 0;
  __syncthreads();
  int cnt[C_FIELDS];
#pragma unroll
  for (int k = 0; k < C_FIELDS; k++) cnt[k] = 0;

  // ---- phase 1: the entry pass and the grid's counts
  for (int j = t; j < nC; j += MP_THREADS) {
    const int e = row[j];
    if (e >= nM) status |= ORBX_FUSE_BAD_INPUT;
    else if (e >= 0) mrSetBit(L.inKf, e);
    else if (!SCW && e == ORBX_FUSE_OCCUPIED_UNMAPPED && !occObs) status |= ORBX_FUSE_BAD_INPUT;
  }
  mpGridCount(P.g, P.kps, nC, L.cellStart);
  __syncthreads();
  mpGridFill(P.g, P.kps, nC, L.cellStart, L.cellIdx, sWave);
  __syncthreads();

  // ---- phase 2: the search
  bool any = false;
  for (int i = t; i < nM; i += MP_THREADS) {
    int got = -1;
    const bool isIn = mrBit(L.inKf, i);
    cnt[C_IN_KF] += isIn;
    if (!isIn && (!mask || mask[i] != 0)) {
      cnt[C_POINTS]++;
      float u = 0.0f, v = 0.0f;
      int level = 0;
      const int where = poseOk ? fuSearched(a, P, sScale, i, &u, &v, &level, &status) : (int)FU_DROPPED;
      cnt[C_BEHIND] += where == FU_BEHIND;
      cnt[C_OUT_IMAGE] += where == FU_OUT_IMAGE;
      cnt[C_OUT_DISTANCE] += where == FU_OUT_DISTANCE;
      cnt[C_OUT_ANGLE] += where == FU_OUT_ANGLE;
      if (where == FU_SEARCHED) {
        const uint4 q0 = descM[(size_t)i * 2], q1 = descM[(size_t)i * 2 + 1];
        uint64_t best = MR_NO_KEY;
        int nCand = 0;
        mrWalk(P.g, P.kps, L.cellStart, L.cellIdx, u, v, a.cam.th * sScale[level], INT32_MIN, INT32_MAX, [&](int j, int c) {
          nCand++;
          const orbx_keypoint* kp = P.kps + j;
          const int oct = kp->octave;
          if (oct < level - 1 || oct > level) return;
          if (!SCW) {  // the chi-square gate
            if (oct < 0) return;
            const float ex = u - kp->x, ey = v - kp->y;
            const float e2 = ex * ex + ey * ey;
            if ((double)(e2 * sInvSigma2[oct]) > 5.99) return;
          }
          const int d = mpDistance(q0, q1, descC[(size_t)j * 2], descC[(size_t)j * 2 + 1]);
          if (!SCW && d >= 256) return;  // (`dist < bestDist` from 256)
          const uint64_t key = mrKey(d, c, j);
          best = key < best ? key : best;
        });
        if (nCand > 0) {
          cnt[C_WITH_CAND]++;
          if (best != MR_NO_KEY && mrKeyDistance(best) <= thLow) got = mrKeyIndex(best);
          cnt[C_OVER_DIST] += got < 0;
        }
      }
    }
    outIdx[i] = got;
    outAct[i] = ORBX_FUSE_NONE;
    outOther[i] = -1;
    L.pick[i] = (uint16_t)(got < 0 ? FU_NO_PICK : got);
    any = any || got >= 0;
  }
  if (any) sAny = 1;
  __syncthreads();  // (the grid is read no more: the region holds the heads and the counts from here on)

  // ---- phase 3: the resolution
  int rounds = 0;
  while (sAny) {  // (uniform: read behind a barrier, written again only behind the next one)
    for (int i = t; i < nM; i += MP_THREADS) {
      const int f = L.pick[i];
      if (f != FU_NO_PICK) L.head[f] = MR_FREE;
    }
    __syncthreads();
    if (t == 0) sAny = 0;
    for (int i = t; i < nM; i += MP_THREADS) {
      const int f = L.pick[i];
      if (f != FU_NO_PICK) atomicMin(&L.head[f], i);
    }
    __syncthreads();
    for (int i = t; i < nM; i += MP_THREADS) {
      const int f = L.pick[i];
      if (f == FU_NO_PICK) continue;
      if (L.head[f] != i) {
        sAny = 1;
        continue;
      }
      L.pick[i] = FU_NO_PICK;
      cnt[C_FUSED]++;
      const int occ = row[f];
      const int obs = SCW ? 0 : fuObs(mapObs[i], &status);
      if (occ < 0 && occ != ORBX_FUSE_OCCUPIED_UNMAPPED) {  // R1
        row[f] = i;
        outAct[i] = ORBX_FUSE_ADD;
        cnt[C_ADDED]++;
        if (!SCW) {
          if (obs + 1 > FU_MAX_OBS) mrSetBit(L.over, f);
          L.count[f] = (uint16_t)(obs + 1);
        }
        continue;
      }
      outOther[i] = occ;
      bool bad;
      if (occ >= nM) bad = true;
      else if (occ >= 0) bad = mask && mask[occ] == 0;
      else bad = SCW ? (occObs && occObs[f] < 0) : (!occObs || occObs[f] < 0);
      if (bad) {  // R2
        outAct[i] = ORBX_FUSE_BAD_OCCUPANT;
        cnt[C_BAD_OCC]++;
        continue;
      }
      cnt[C_CHAINED] += rounds > 0;
      if (SCW) {  // R4
        outAct[i] = ORBX_FUSE_KEEP_OCCUPANT;
        cnt[C_KEPT]++;
        continue;
      }
      // R3: the count is the occupant's own at the first decision on f, the modelled one behind it
      int c;
      if (rounds == 0) c = fuObs(occ >= 0 ? mapObs[occ] : occObs[f], &status);
      else c = mrBit(L.over, f) ? FU_MAX_OBS + 1 : (int)L.count[f];
      if (c > obs) {
        outAct[i] = ORBX_FUSE_KEEP_OCCUPANT;
        cnt[C_KEPT]++;
      } else {
        outAct[i] = ORBX_FUSE_REPLACE_OCCUPANT;
        row[f] = i;
        cnt[C_REPLACED]++;
      }
      c += obs;
      if (c > FU_MAX_OBS) mrSetBit(L.over, f);
      L.count[f] = (uint16_t)c;
    }
    rounds++;
    __syncthreads();
  }
  mrFlush(cnt, status, rounds, sCnt, (int32_t*)(a.res + pair));
}

}  // namespace

hipError_t launch_match_fuse(hipStream_t st, const MatchFuseArgs& a, bool scwForm) {
  static_assert(sizeof(orbx_fuse_result) == 4 * C_FIELDS && C_STATUS == 0 && C_ROUNDS == C_FIELDS - 1, "sixteen int32, as mrFlush writes them");
  static_assert(FuLds::bytes(BOW_MAX_FEATURES, BOW_MAX_FEATURES) + 512 <= 160 * 1024, "a workgroup's LDS at the largest capacities");
  static_assert(FuLds::bytes(1024, 4096) == 23184 && FuLds::bytes(BOW_MAX_FEATURES, BOW_MAX_FEATURES) == 135168,
"capacity 1024 with a map capacity of 4096: the layout decides the occupancy");
  static_assert(BOW_MAX_FEATURES <= FU_NO_PICK, "a pick is 16 bits");
  const size_t lds = FuLds::bytes(a.cap, a.mapCap);
  return scwForm ? mrLaunch(k_match_fuse<true>, a.nPairs, lds, st, a) : mrLaunch(k_match_fuse<false>, a.nPairs, lds, st, a);
}

}  // namespace orbx
