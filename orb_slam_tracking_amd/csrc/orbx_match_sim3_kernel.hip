// orbx_match_sim3_kernel.hip — ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) for a batch of (KF1, KF2)
// pairs (include/orbx.h, "loop closing: matching under a similarity").  gfx950, wave64.
//
// One workgroup of MP_THREADS threads per pair, one launch per call, three phases separated by barriers; no claim rounds, since
// the searches have no "taken" rule: a point's pick depends on nothing another point does.
//   rule 1   every feature of KF1 reads its entry of the row: vbAlreadyMatched1 is the entry itself, vbAlreadyMatched2 a bit set
//            over KF2's features in LDS.
//   rule 2   KF2's grid in LDS (orbx_match_grid.h); a thread per point of KF1: the transform, the tests, the window walk
//            (orbx_match_rounds.h) and the first smallest distance as the smallest key (distance, cell, index); vnMatch1 in LDS.
//   rule 3   KF1's grid in the SAME LDS, the mirror image over KF2's points; vnMatch2 in LDS.
//   rule 4   a thread per feature of KF1: the agreement, and the row's new entries.
//
// LDS, sized from the capacity by the launcher: 12304 bytes of cell starts, then per feature 2 bytes of cell-ordered indices, 2
// + 2 bytes of vnMatch1 / vnMatch2 (int16: an index is below 16384) and a bit of vbAlreadyMatched2: 18.1 KB at capacity 1024,
// 110.0 KB at ORBX_BOW_MAX_FEATURES, plus under 200 bytes of static LDS.
#include <hip/hip_runtime.h>

#include "orbx_launch.h"
#include "orbx_match_rounds.h"

namespace orbx {
namespace {

// sCnt: the fields of orbx_msim3_result in their order; a direction's six counters start at C_DIR1 / C_DIR2
enum { C_STATUS, C_FOUND, C_DIR1, C_DIR2 = C_DIR1 + 6, C_ONE_SIDED = C_DIR2 + 6, C_RESERVED, C_FIELDS };
enum { D_POINTS, D_BEHIND, D_OUT_IMAGE, D_OUT_DISTANCE, D_WITH_CAND, D_OVER_DIST };

struct Ms3Lds {
  int* cellStart;     // [MP_START_WORDS]
  uint32_t* matched2; // [mrBitWords(cap)] vbAlreadyMatched2
  uint16_t* cellIdx;  // [cap]
  int16_t* vn1;       // [cap] vnMatch1
  int16_t* vn2;       // [cap] vnMatch2
  __host__ __device__ static constexpr size_t bytes(int cap) {
    return (size_t)4 * (MP_START_WORDS + mrBitWords(cap)) + (size_t)3 * 2 * ((cap + 1) & ~1);
  }
  __device__ __forceinline__ Ms3Lds(uint32_t* base, int cap) {
    cellStart = (int*)base;
    matched2 = base + MP_START_WORDS;
    cellIdx = (uint16_t*)(matched2 + mrBitWords(cap));
    vn1 = (int16_t*)(cellIdx + ((cap + 1) & ~1));
    vn2 = vn1 + ((cap + 1) & ~1);
  }
};

// a keyframe as a direction reads it
struct Ms3Side {
  const orbx_keypoint* kps;
  const float *pts, *dist;
  const uint8_t* mask;
  const uint4 *desc, *pdesc;  // the features' descriptors; the points' (the features' own when the call gives none)
  MrPose pose;
  int n;
};

// the grid of keyframe G's n features into L (all threads; ends behind a barrier)
__device__ __forceinline__ void ms3Grid(const MpGrid& g, const Ms3Side& G, const Ms3Lds& L, int* sWave) {
  for (int c = threadIdx.x; c < MP_START_WORDS; c += MP_THREADS) L.cellStart[c] = 0;
  __syncthreads();
  mpGridCount(g, G.kps, G.n, L.cellStart);
  __syncthreads();
  mpGridFill(g, G.kps, G.n, L.cellStart, L.cellIdx, sWave);
  __syncthreads();
}

// Rules 2 / 3 for point i of keyframe A (a point, not already matched), searched in keyframe B whose grid is in L: M [9], tv
// [3] take A's camera frame to B's.  Returns the pick or -1.
__device__ __forceinline__ int ms3Search(const MatchSim3Args& a, const MpGrid& g, const Ms3Side& A, const Ms3Side& B, const float* M,
                                         const float* tv, const Ms3Lds& L, const float* __restrict__ scale, int orbDist, int i, int* cnt,
                                         int* status) {
  const float* X = A.pts + 3 * (size_t)i;
  const float minD = A.dist[2 * (size_t)i], maxD = A.dist[2 * (size_t)i + 1];
  if (!(mpFinite(X[0]) && mpFinite(X[1]) && mpFinite(X[2]) && mpFinite(minD) && mpFinite(maxD))) {
    *status |= ORBX_MSIM3_NONFINITE;
    return -1;
  }
  float xa, ya, za;
  mrToCamera(A.pose, A.pts, i, &xa, &ya, &za);
  const float x = ((M[0] * xa + M[1] * ya) + M[2] * za) + tv[0];
  const float y = ((M[3] * xa + M[4] * ya) + M[5] * za) + tv[1];
  const float z = ((M[6] * xa + M[7] * ya) + M[8] * za) + tv[2];
  if (z < 0.0f) {
    cnt[D_BEHIND]++;
    return -1;
  }
  const float invz = 1.0f / z;
  const float u = a.cam.fx * (x * invz) + a.cam.cx, v = a.cam.fy * (y * invz) + a.cam.cy;
  // IsInImage: >= min and < max (a coordinate that is no number is outside)
  if (!(mpFinite(u) && mpFinite(v) && u >= g.minX && u < g.maxX && v >= g.minY && v < g.maxY)) {
    cnt[D_OUT_IMAGE]++;
    return -1;
  }
  const float dist3D = (float)sqrt(((double)x * (double)x + (double)y * (double)y) + (double)z * (double)z);
  if (dist3D < 0.8f * minD || dist3D > 1.2f * maxD) {
    cnt[D_OUT_DISTANCE]++;
    return -1;
  }
  const float ratio = maxD / dist3D;
  if (ratio != ratio) {
    *status |= ORBX_MSIM3_NONFINITE;
    return -1;
  }
  int level = 0;
  for (int n = 0; n < a.cam.nLevels - 1; n++) level += ratio > scale[n];
  const uint4 q0 = A.pdesc[(size_t)i * 2], q1 = A.pdesc[(size_t)i * 2 + 1];
  uint64_t best = MR_NO_KEY;
  mrWalk(g, B.kps, L.cellStart, L.cellIdx, u, v, a.cam.th * scale[level], level - 1, level, [&](int j, int c) {
    const uint64_t key = mrKey(mpDistance(q0, q1, B.desc[(size_t)j * 2], B.desc[(size_t)j * 2 + 1]), c, j);
    best = key < best ? key : best;
  });
  if (best == MR_NO_KEY) return -1;
  cnt[D_WITH_CAND]++;
  if (mrKeyDistance(best) > orbDist) {
    cnt[D_OVER_DIST]++;
    return -1;
  }
  return mrKeyIndex(best);
}

__global__ __launch_bounds__(MP_THREADS) void k_match_sim3(MatchSim3Args a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ms3Lds[];
  __shared__ float sScale[ORBX_MAX_LEVELS];
  __shared__ int sWave[MP_THREADS / 64];
  __shared__ int sCnt[C_FIELDS];
  const int pair = blockIdx.x, t = threadIdx.x;
  const int cap = a.cap;
  const Ms3Lds L(ms3Lds, cap);
  const int f1 = a.pairs[pair], f2 = a.pairs[a.nPairs + pair], s1 = a.pairs[2 * a.nPairs + pair], s2 = a.pairs[3 * a.nPairs + pair];
  const int raw1 = a.n[f1], raw2 = a.n[f2];
  Ms3Side S1, S2;
  S1.n = mpClamp(raw1, cap);
  S2.n = mpClamp(raw2, cap);
  int status = (raw1 != S1.n || raw2 != S2.n) ? ORBX_MSIM3_BAD_INPUT : 0;
  S1.kps = a.kps + (size_t)f1 * cap;
  S2.kps = a.kps + (size_t)f2 * cap;
  S1.pts = a.points + (size_t)s1 * cap * 3;
  S2.pts = a.points + (size_t)s2 * cap * 3;
  S1.dist = a.pointDist + (size_t)s1 * cap * 2;
  S2.dist = a.pointDist + (size_t)s2 * cap * 2;
  S1.mask = a.pointMask ? a.pointMask + (size_t)s1 * cap : nullptr;
  S2.mask = a.pointMask ? a.pointMask + (size_t)s2 * cap : nullptr;
  S1.desc = (const uint4*)a.desc + (size_t)f1 * cap * 2;
  S2.desc = (const uint4*)a.desc + (size_t)f2 * cap * 2;
  S1.pdesc = a.pointDesc ? (const uint4*)a.pointDesc + (size_t)s1 * cap * 2 : S1.desc;
  S2.pdesc = a.pointDesc ? (const uint4*)a.pointDesc + (size_t)s2 * cap * 2 : S2.desc;
  bool ok = mrLoadPose(a.pose, f1, &S1.pose);
  ok = mrLoadPose(a.pose, f2, &S2.pose) && ok;
  // the similarity: sR12 = s12 * R12, t12; sR21 = (1.0 / s12) * R12^T with the quotient in f64, t21 = -sR21 * t12
  const float* sim = a.sim3 + (size_t)pair * 13;
  float sR12[9], t12[3], sR21[9], t21[3];
  const float s12 = sim[12];
  ok = ok && mpFinite(s12) && s12 > 0.0f;
  const double inv = 1.0 / (double)s12;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      ok = ok && mpFinite(sim[3 * i + j]);
      sR12[3 * i + j] = s12 * sim[3 * i + j];
      sR21[3 * i + j] = (float)(inv * (double)sim[3 * j + i]);
    }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    t12[i] = sim[9 + i];
    ok = ok && mpFinite(t12[i]);
  }
#pragma unroll
  for (int i = 0; i < 3; i++) t21[i] = -((sR21[3 * i] * t12[0] + sR21[3 * i + 1] * t12[1]) + sR21[3 * i + 2] * t12[2]);
  if (!ok) status |= ORBX_MSIM3_NONFINITE;
  if (t != 0) status = 0;  // (what all threads see alike is reported once)
  const MpGrid g = mpGridOf(a.cam.b);
  int* __restrict__ row = a.matches + (size_t)pair * cap;
  const int orbDist = a.orbDist;

  // ---- start state
  for (int k = t; k < mrBitWords(cap); k += MP_THREADS) L.matched2[k] = 0;
  for (int k = t; k < cap; k += MP_THREADS) { L.vn1[k] = -1; L.vn2[k] = -1; }
  if (t < ORBX_MAX_LEVELS) sScale[t] = a.cam.scale[t];
  if (t < C_FIELDS) sCnt[t] = 0;
  __syncthreads();
  int cnt[C_FIELDS];
#pragma unroll
  for (int k = 0; k < C_FIELDS; k++) cnt[k] = 0;
  // ---- rule 1
  for (int i1 = t; i1 < S1.n; i1 += MP_THREADS) {
    const int i2 = row[i1];
    if (i2 < 0) continue;
    if (i2 >= S2.n) status |= ORBX_MSIM3_BAD_INPUT;
    else mrSetBit(L.matched2, i2);
  }
  // ---- rule 2: KF1's points into KF2
  ms3Grid(g, S2, L, sWave);  // (its first barrier also closes rule 1)
  if (ok)
    for (int i1 = t; i1 < S1.n; i1 += MP_THREADS) {
      if ((S1.mask && S1.mask[i1] == 0) || row[i1] >= 0) continue;
      cnt[C_DIR1 + D_POINTS]++;
      L.vn1[i1] = (int16_t)ms3Search(a, g, S1, S2, sR21, t21, L, sScale, orbDist, i1, cnt + C_DIR1, &status);
    }
  __syncthreads();
  // ---- rule 3: KF2's points into KF1
  ms3Grid(g, S1, L, sWave);
  if (ok)
    for (int i2 = t; i2 < S2.n; i2 += MP_THREADS) {
      if ((S2.mask && S2.mask[i2] == 0) || mrBit(L.matched2, i2)) continue;
      cnt[C_DIR2 + D_POINTS]++;
      L.vn2[i2] = (int16_t)ms3Search(a, g, S2, S1, sR12, t12, L, sScale, orbDist, i2, cnt + C_DIR2, &status);
    }
  __syncthreads();
  // ---- rule 4: the agreement
  for (int i1 = t; i1 < S1.n; i1 += MP_THREADS) {
    const int i2 = L.vn1[i1];
    if (i2 < 0) continue;
    if (L.vn2[i2] == i1) {
      row[i1] = i2;
      cnt[C_FOUND]++;
    } else {
      cnt[C_ONE_SIDED]++;
    }
  }
  if (status) atomicOr(&sCnt[C_STATUS], status);
#pragma unroll
  for (int k = 1; k < C_FIELDS; k++)
    if (cnt[k]) atomicAdd(&sCnt[k], cnt[k]);
  __syncthreads();
  if (t < C_FIELDS) ((int32_t*)(a.res + pair))[t] = sCnt[t];
}

}  // namespace

hipError_t launch_match_sim3(hipStream_t st, const MatchSim3Args& a) {
  static_assert(sizeof(orbx_msim3_result) == 4 * C_FIELDS && C_FIELDS == 16, "sixteen int32, in the enum's order");
  static_assert(Ms3Lds::bytes(BOW_MAX_FEATURES) + 512 <= 160 * 1024, "a workgroup's LDS at the largest capacity");
  static_assert(Ms3Lds::bytes(1024) == 18576 && Ms3Lds::bytes(16384) == 112656, "the layout at capacities 1024 and 16384");
  return mrLaunch(k_match_sim3, a.nPairs, Ms3Lds::bytes(a.cap), st, a);
}

}  // namespace orbx
