// orbx_sim3_kernel.hip — Sim3Solver on the device (include/orbx.h, "loop closing: Sim3 RANSAC"): Horn's closed-form similarity
// inside RANSAC for a batch of independent keyframe pairs, in three launches.
//
//   k_sim3_prep         wave per problem              the checks of the device data, the correspondences in ascending order of
//                                                     KF1's feature (ballot + prefix): camera-frame points, projections, bounds
//   k_sim3_hypotheses   lane per (problem, iteration) the three draws, Horn's solution, CheckInliers over the problem's N
//                                                     correspondences (every lane of a wave reads the same one: uniform reads)
//   k_sim3_resolve      wave per problem              iterate() resolved in iteration order, then the winner's inliers again for
//                                                     the row and the flags, the result and d_sim3
//
// All arithmetic is csrc/orbx_sim3_math.inc, shared with the CPU restatement; this file fixes who computes what.  Nothing is
// summed across lanes, so there is no order to fix beyond the include's.  No LDS and no scratch: Horn's 4x4 Jacobi keeps its
// matrix and its vectors in registers, indexed with constants.  f64 / f32 without contraction (-ffp-contract=off).
// Bounds: 12 sweeps; every index is checked before it is followed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/orbx.h"
#include "orbx_launch.h"

#define ORBX_SIM3_FN __device__
#include "orbx_sim3_math.inc"

namespace orbx {
using namespace orbx_sim3;

static_assert(sizeof(Corr) == SIM3_CORR_BYTES && sizeof(Hyp) == SIM3_HYP_BYTES && sizeof(Meta) == 16, "workspace records");
static_assert(SIM3_MAX_CAPACITY == ORBX_BOW_MAX_FEATURES, "the largest keyframe");
static_assert(sizeof(orbx_sim3_result) == 96, "orbx_sim3_result layout");

namespace {

__device__ inline Cam camOf(const Sim3Args& a) { return Cam{a.fx, a.fy, a.cx, a.cy}; }

// ---- k_sim3_prep: the constructor and SetRansacParameters -----------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sim3_prep(const Sim3Args a) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const size_t cap = (size_t)a.cap;
  const int P = a.nProblems;
  const int kf1 = a.problems[p], kf2 = a.problems[P + p], set1 = a.problems[2 * P + p], set2 = a.problems[3 * P + p];  // (checked on the host)
  const orbx_keypoint *kps1 = a.kps + (size_t)kf1 * cap, *kps2 = a.kps + (size_t)kf2 * cap;
  const int32_t* match = a.match + (size_t)p * cap;
  const float *points1 = a.points + (size_t)set1 * cap * 3, *points2 = a.points + (size_t)set2 * cap * 3;
  const uint8_t *mask1 = a.mask ? a.mask + (size_t)set1 * cap : nullptr, *mask2 = a.mask ? a.mask + (size_t)set2 * cap : nullptr;
  Corr* corr = reinterpret_cast<Corr*>(a.corr) + (size_t)p * cap;
  int32_t* corrOf = a.corrOf + (size_t)p * cap;
  const Cam K = camOf(a);
  int n1 = a.nKps[kf1], n2 = a.nKps[kf2];
  int bad = 0, nonfinite = 0;
  if (n1 < 0 || n1 > a.cap || n2 < 0 || n2 > a.cap) {
    bad = 1;
    n1 = 0;
  }
  float pose1[12], pose2[12];
#pragma unroll
  for (int k = 0; k < 12; k++) {
    pose1[k] = a.pose[(size_t)kf1 * 12 + k];
    pose2[k] = a.pose[(size_t)kf2 * 12 + k];
    if (!finite32(pose1[k]) || !finite32(pose2[k])) nonfinite = 1;
  }
  int N = 0;
  for (int j0 = 0; j0 < a.cap; j0 += 64) {
    const int i1 = j0 + lane;
    bool take = false;
    Corr c{};
    if (i1 < n1) {
      const int i2 = match[i1];
      if (i2 >= n2) bad = 1;
      bool has = i2 >= 0 && i2 < n2;
      if (has && mask1 && (mask1[i1] == 0 || mask2[i2] == 0)) has = false;
      if (has) {
        const orbx_keypoint k1 = kps1[i1], k2 = kps2[i2];
        if (k1.octave < 0 || k1.octave >= a.nLevels || k2.octave < 0 || k2.octave >= a.nLevels) {
          bad = 1;
        } else {
          float X1[3], X2[3];
#pragma unroll
          for (int k = 0; k < 3; k++) {
            X1[k] = points1[(size_t)i1 * 3 + k];
            X2[k] = points2[(size_t)i2 * 3 + k];
          }
          toCamera(pose1, X1, c.X1);
          toCamera(pose2, X2, c.X2);
          toImage(c.X1, K, c.p1);
          toImage(c.X2, K, c.p2);
          c.maxErr1 = a.th2 * a.sigma2[k1.octave];
          c.maxErr2 = a.th2 * a.sigma2[k2.octave];
          c.i1 = i1; c.i2 = i2;
          if (finite32(X1[0]) && finite32(X1[1]) && finite32(X1[2]) && finite32(X2[0]) && finite32(X2[1]) && finite32(X2[2]) &&
              finite32(k1.x) && finite32(k1.y) && finite32(k2.x) && finite32(k2.y))
            take = true;
          else
            nonfinite = 1;
        }
      }
    }
    const unsigned long long m = __ballot(take);
    const int slot = N + __popcll(m & ((1ull << lane) - 1ull));
    if (take) corr[slot] = c;
    if (i1 < a.cap) corrOf[i1] = take ? slot : -1;
    N += (int)__popcll(m);
  }
  const int status = (__any(bad) ? SIM3_BAD_INPUT : 0) | (__any(nonfinite) ? SIM3_NONFINITE : 0);
  if (status) N = 0;
  if (lane == 0) {
    Meta m;
    m.N = N;
    m.maxIts = a.table[N];  // (N <= cap, the table's last entry)
    m.status = status;
    m.pad = 0;
    reinterpret_cast<Meta*>(a.meta)[p] = m;
  }
}

// ---- k_sim3_hypotheses ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sim3_hypotheses(const Sim3Args a) {
  const long long gid = (long long)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (long long)a.nProblems * a.nIter) return;  // (no barrier below)
  const int p = (int)(gid / a.nIter), it = (int)(gid % a.nIter);
  const Meta m = reinterpret_cast<const Meta*>(a.meta)[p];
  // what iterate() never runs is never read: a refused problem, bNoMore, iterations beyond mRansacMaxIts
  if (m.status != 0 || m.N < a.minInliers || it >= m.maxIts) return;
  const Corr* corr = reinterpret_cast<const Corr*>(a.corr) + (size_t)p * a.cap;
  const Cam K = camOf(a);
  Hyp h;
  Sim3Pair T;
  if (hypothesis(a.draws + gid * 3, corr, m.N, a.fixScale != 0, &h, &T)) {
    int count = 0;
    for (int c = 0; c < m.N; c++) count += isInlier(T, corr[c], K) ? 1 : 0;
    h.count = count;
  }
  reinterpret_cast<Hyp*>(a.hyp)[gid] = h;
}

// ---- k_sim3_resolve -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sim3_resolve(const Sim3Args a) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const size_t cap = (size_t)a.cap;
  const Meta m = reinterpret_cast<const Meta*>(a.meta)[p];
  const Corr* corr = reinterpret_cast<const Corr*>(a.corr) + (size_t)p * cap;
  const int32_t* corrOf = a.corrOf + (size_t)p * cap;
  const Hyp* hyp = reinterpret_cast<const Hyp*>(a.hyp) + (size_t)p * a.nIter;
  const Cam K = camOf(a);

  int status = m.status;
  if (status == 0 && m.N < a.minInliers) status = SIM3_FEW_POINTS;
  Outcome o{};
  o.foundIt = o.bestIt = -1;
  if (status == 0) {  // (every lane walks the same records: wave-uniform)
    resolveIterations(hyp, a.nIter < m.maxIts ? a.nIter : m.maxIts, a.minInliers, &o);
    if (o.badDraws) status |= SIM3_BAD_DRAWS;
  }
  const bool have = o.foundIt >= 0;
  if (!have) status |= SIM3_NO_RESULT;
  float sim[13];
#pragma unroll
  for (int k = 0; k < 13; k++) sim[k] = have ? hyp[o.foundIt].sim[k] : 0.f;
  Sim3Pair T{};
  if (have) (void)pairOf(sim, &T);

  // ---- the row and the flags: every entry is written ----
  int32_t* row = a.matchInliers + (size_t)p * cap;
  uint8_t* flags = a.inliers ? a.inliers + (size_t)p * cap : nullptr;
  int nIn = 0;
  for (int j0 = 0; j0 < a.cap; j0 += 64) {
    const int j = j0 + lane;
    bool in = false;
    int i2 = -1;
    if (j < a.cap && have) {
      const int c = corrOf[j];
      if (c >= 0) {
        const Corr cc = corr[c];
        in = isInlier(T, cc, K);
        i2 = cc.i2;
      }
    }
    if (j < a.cap) {
      row[j] = in ? i2 : -1;
      if (flags) flags[j] = in ? 1 : 0;
    }
    nIn += (int)__popcll(__ballot(in));
  }
  // ---- the result (every lane holds it: lane 0 writes) ----
  if (lane == 0) {
    orbx_sim3_result* out = a.res + p;
    float* dst = a.sim3 + (size_t)p * 13;
    const bool counted = (status & (SIM3_BAD_INPUT | SIM3_NONFINITE)) == 0;
    out->status = status;
    out->n_correspondences = counted ? m.N : 0;
    out->max_its = m.maxIts;
    out->its_run = o.itsRun;
    out->found_it = o.foundIt;
    out->best_it = o.bestIt;
    out->n_inliers = nIn;
    out->n_best_inliers = o.nBestInliers;
    out->n_degenerate = o.nDegenerate;
    out->reserved[0] = out->reserved[1] = 0;
    out->s12 = sim[12];
#pragma unroll
    for (int k = 0; k < 9; k++) out->R12[k] = sim[k];
#pragma unroll
    for (int k = 0; k < 3; k++) out->t12[k] = sim[9 + k];
#pragma unroll
    for (int k = 0; k < 13; k++) dst[k] = sim[k];
  }
}

}  // namespace

hipError_t launch_sim3_prep(hipStream_t st, const Sim3Args& a) {
  hipLaunchKernelGGL(k_sim3_prep, dim3(a.nProblems), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_sim3_hypotheses(hipStream_t st, const Sim3Args& a) {
  const long long lanes = (long long)a.nProblems * a.nIter;
  hipLaunchKernelGGL(k_sim3_hypotheses, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_sim3_resolve(hipStream_t st, const Sim3Args& a) {
  hipLaunchKernelGGL(k_sim3_resolve, dim3(a.nProblems), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
