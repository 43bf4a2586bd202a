// orbx_pose_kernel.hip — Optimizer::PoseOptimization on the device (include/orbx.h, "behind SearchByBoW: pose optimisation"):
// motion-only bundle adjustment, g2o's Levenberg-Marquardt over one free pose and fixed points, four rounds with the outlier
// classification behind each.
//
//   k_pose   wave (64 lanes) per problem, four problems per workgroup   the checks of the device data, every round, iteration and
//                                                                        trial, the flags, the result
//
// A problem is 28 running sums over a few hundred edges and one 6x6 solve per trial, so it is given to one wave and the waves of
// a workgroup share nothing: no barrier, and LDS only as each lane's own copy of its first edges (WaveOps).  Lane l walks the
// features l, l + 64, ... of the frame in ascending order and keeps the sums in registers; a butterfly of six __shfl_xor steps
// (32, 16, ... 1) leaves the same bits in every lane, those lane 0 would hold after the fold include/orbx.h documents (deviation
// 1; f64 addition is commutative).  Every lane then runs the 6x6 solve, the judgement of the trial and the round logic
// redundantly on those equal bits, so all control flow is wave-uniform without a broadcast.  A feature's flag lives in the
// problem's row of the outlier array (and next to its cached edge) and is read and written by the feature's own lane only.  All
// arithmetic and the round logic are in csrc/orbx_pose_math.inc, shared with the CPU restatement; this file fixes who computes
// what and the order of the sums.  f64 without contraction (-ffp-contract=off).
// Bounds: 4 rounds x n_iterations x 10 trials; every index is checked before it is followed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/orbx.h"
#include "orbx_launch.h"

#define ORBX_BA_FN __device__
#include "orbx_pose_math.inc"

namespace orbx {
using namespace orbx_pose;

namespace {

// the wave's sum of v in every lane, in the documented order
__device__ inline double waveSum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}
__device__ inline int waveSumInt(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The three passes of optimiseRounds over the features of one problem, by one wave.  A lane's first POSE_CACHE edges are kept in
// the wave's own block of LDS as the f32 values they are read from (point, observation, information, feature index, flag), field
// by field and slot by slot in rows of 64 lanes: a lane reads back only what it wrote itself, so there is no barrier and no
// traffic between lanes, and a pass is not two dependent global loads per feature.  What does not fit is read from the problem's
// arrays as before, behind the cached edges: the lane's order of the sums stays the ascending order of its features.
constexpr int POSE_FIELDS = 8;  // X[3], u, v, w, the feature's index, its flag
struct WaveOps {
  const Problem& P;
  int lane;
  float* cache;  // [POSE_FIELDS][POSE_CACHE][64] of this wave
  int cached;    // edges of this lane in the cache
  int jRest;     // the lane's first feature behind them (>= n: none)

  __device__ int at(int field, int k) const { return (field * POSE_CACHE + k) * 64 + lane; }

  __device__ void stage() {
    cached = 0;
    jRest = P.n;
    int st = 0;
    for (int j = lane; j < P.n; j += 64) {
      const int i = pointOf(P, j, &st);
      if (i < 0) continue;
      if (cached == POSE_CACHE) {
        jRest = j;
        break;
      }
      for (int c = 0; c < 3; c++) cache[at(c, cached)] = P.points[(size_t)i * 3 + c];
      cache[at(3, cached)] = P.kps[j].x;
      cache[at(4, cached)] = P.kps[j].y;
      cache[at(5, cached)] = P.invSigma2[P.kps[j].octave];
      cache[at(6, cached)] = __int_as_float(j);
      cache[at(7, cached)] = __int_as_float(0);
      cached++;
    }
  }

  // f(edge, feature, whether it is flagged) -> its new flag, or -1 to leave it, for every edge of the lane in ascending order
  template <class F>
  __device__ void walk(F f) {
    for (int k = 0; k < cached; k++) {
      Edge E;
      for (int c = 0; c < 3; c++) E.X[c] = (double)cache[at(c, k)];
      E.u = (double)cache[at(3, k)];
      E.v = (double)cache[at(4, k)];
      E.w = (double)cache[at(5, k)];
      const int j = __float_as_int(cache[at(6, k)]);
      const int flag = f(E, j, __float_as_int(cache[at(7, k)]) != 0);
      if (flag >= 0) {
        cache[at(7, k)] = __int_as_float(flag);
        P.outlier[j] = (uint8_t)flag;
      }
    }
    int st = 0;
    for (int j = jRest; j < P.n; j += 64) {
      const int i = pointOf(P, j, &st);
      if (i < 0) continue;
      Edge E;
      loadEdge(P, j, i, &E);
      const int flag = f(E, j, P.outlier[j] != 0);
      if (flag >= 0) P.outlier[j] = (uint8_t)flag;
    }
  }

  __device__ void build(const Pose& T, bool robust, double* sum, Branches* br) {
    double acc[POSE_ACC_BUILD];
#pragma unroll
    for (int k = 0; k < POSE_ACC_BUILD; k++) acc[k] = 0.0;
    const double delta = deltaOf(P, robust);
    int huber = 0;
    walk([&](const Edge& E, int, bool flagged) {
      if (!flagged) huber += edgeBuild(T, E, P.K, delta, acc);
      return -1;
    });
    br->lm.huberOutliers += huber;
#pragma unroll
    for (int k = 0; k < POSE_ACC_BUILD; k++) sum[k] = waveSum(acc[k]);
  }

  __device__ double trial(const Pose& T, bool robust) {
    double acc = 0.0;
    const double delta = deltaOf(P, robust);
    walk([&](const Edge& E, int, bool flagged) {
      if (!flagged) acc = acc + edgeRho(T, E, P.K, delta);
      return -1;
    });
    return waveSum(acc);
  }

  __device__ int classify(const Pose& Tfinal, const Pose& Ttrial, int) {
    int bad = 0;
    walk([&](const Edge& E, int, bool flagged) {
      const int out = edgeIsOutlier(Tfinal, Ttrial, flagged, E, P.K) ? 1 : 0;
      bad += out;
      return out;
    });
    return waveSumInt(bad);
  }
};

__global__ __launch_bounds__(POSE_THREADS) void k_pose(const PoseArgs a) {
  __shared__ float cache[POSE_WAVES][POSE_FIELDS * POSE_CACHE * 64];
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * POSE_WAVES + (threadIdx.x >> 6);
  if (p >= a.nProblems) return;  // (a whole wave: the waves of a workgroup never meet)
  const size_t cap = (size_t)a.cap;
  const int frame = a.problems[p], set = a.problems[a.nProblems + p];  // (checked on the host)
  const float* pose0 = a.pose0 + (size_t)p * 12;
  orbx_pose_result* out = a.res + p;

  Problem P;
  P.kps = a.kps + (size_t)frame * cap;
  P.match = a.match ? a.match + (size_t)p * cap : nullptr;
  P.points = a.points + (size_t)set * cap * 3;
  P.mask = a.mask ? a.mask + (size_t)set * cap : nullptr;
  P.invSigma2 = a.invSigma2;
  P.outlier = a.outlier + (size_t)p * cap;
  P.n = a.nKps[frame];
  P.cap = a.cap;
  P.nLevels = a.nLevels;
  P.K = Cam{a.fx, a.fy, a.cx, a.cy};
  P.delta = a.delta;

  // ---- the device data checked before it is followed; every feature's flag starts false ----
  int status = 0, nCorr = 0;
  if (P.n < 0 || P.n > a.cap) {
    status |= ORBX_POSE_BAD_INPUT;
    P.n = 0;
  }
  for (int k = 0; k < 12; k++)
    if (!isFiniteF(pose0[k])) status |= ORBX_POSE_NONFINITE;
  for (size_t j = lane; j < cap; j += 64) P.outlier[j] = 0;
  for (int j = lane; j < P.n; j += 64) nCorr += checkFeature(P, j, &status) ? 1 : 0;
  // (status bits differ between the lanes: each bit is voted on)
  status = (__any(status & ORBX_POSE_BAD_INPUT) ? ORBX_POSE_BAD_INPUT : 0) | (__any(status & ORBX_POSE_NONFINITE) ? ORBX_POSE_NONFINITE : 0);
  nCorr = waveSumInt(nCorr);
  if (status == 0 && nCorr < 3) status = ORBX_POSE_FEW_POINTS;

  Rounds r;
  Pose T;
  if (status == 0) {
    Branches br{};
    WaveOps ops{P, lane, cache[threadIdx.x >> 6], 0, 0};
    ops.stage();
    poseFromRt(pose0, pose0 + 9, &T);
    optimiseRounds(ops, &T, nCorr, a.nIterations, &r, &br);
    bool fin = isFinite(r.chi2Initial) && isFinite(r.chi2Final) && isFinite(r.lambda);
    for (int k = 0; k < 4; k++) fin = fin && isFinite(T.q[k]);
    for (int k = 0; k < 3; k++) fin = fin && isFinite(T.t[k]);
    if (!fin) {
      status = ORBX_POSE_NONFINITE;
      for (int j = lane; j < P.n; j += 64) P.outlier[j] = 0;
    }
  }

  // ---- the result (every lane holds it: lane 0 writes) ----
  if (lane == 0) {
    const bool optimised = status == 0;
    const bool counted = optimised || status == ORBX_POSE_FEW_POINTS;
    out->status = status;
    out->n_correspondences = counted ? nCorr : 0;
    out->n_bad = optimised ? r.nBad : 0;
    out->n_inliers = counted ? nCorr - (optimised ? r.nBad : 0) : 0;
    out->rounds = optimised ? r.rounds : 0;
    for (int k = 0; k < 4; k++) {
      out->iterations[k] = optimised ? r.iterations[k] : 0;
      out->stop_reason[k] = optimised ? r.stopReason[k] : 0;
    }
    out->lm_trials = optimised ? r.lmTrials : 0;
    out->rejected_trials = optimised ? r.rejected : 0;
    out->solver_failures = optimised ? r.solverFailures : 0;
    if (optimised) {
      out->chi2_initial = r.chi2Initial;
      out->chi2_final = r.chi2Final;
      out->lambda = r.lambda;
      double R[3][3];
      quatToMatrix(T.q, R);
      for (int k = 0; k < 4; k++) out->q[k] = T.q[k];
      for (int k = 0; k < 3; k++) out->t[k] = T.t[k];
      for (int k = 0; k < 9; k++) out->R[k] = (float)R[k / 3][k % 3];
      for (int k = 0; k < 3; k++) out->tcw[k] = (float)T.t[k];
    } else {
      out->chi2_initial = out->chi2_final = out->lambda = 0.0;
      for (int k = 0; k < 4; k++) out->q[k] = 0.0;
      for (int k = 0; k < 3; k++) out->t[k] = 0.0;
      for (int k = 0; k < 9; k++) out->R[k] = pose0[k];
      for (int k = 0; k < 3; k++) out->tcw[k] = pose0[9 + k];
    }
  }
}

}  // namespace

hipError_t launch_pose(hipStream_t st, const PoseArgs& a) {
  hipLaunchKernelGGL(k_pose, dim3((a.nProblems + POSE_WAVES - 1) / POSE_WAVES), dim3(POSE_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
