// pose_ref.cpp — CPU restatement of Optimizer::PoseOptimization (include/orbx.h, "behind SearchByBoW: pose optimisation"), TEST
// INFRASTRUCTURE: built by tests/pose_ref_lib.py with g++ -O2 -ffp-contract=off.  The arithmetic and the round logic are
// orb_slam_tracking_amd/csrc/orbx_pose_math.inc, the include the device kernel compiles too; this file restates on its own what
// surrounds them: the checks of the inputs, the order of the sums of deviation 1 (64 lanes, each walking its features in turn,
// then lane l + 32, + 16, ... + 1 added to lane l), and the result record.  Beyond the result it reports the flags behind every
// round and counters that show which branches a world ran.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbx.h"

#define ORBX_BA_FN
#include "../../orb_slam_tracking_amd/csrc/orbx_pose_math.inc"

using namespace orbx_pose;

namespace {

constexpr int WAVE = 64;

// the 64 lanes' sums of quantity k folded as include/orbx.h documents: the result is lane 0's
double fold(const double* acc, int stride, int k) {
  double v[WAVE];
  for (int l = 0; l < WAVE; l++) v[l] = acc[(size_t)l * stride + k];
  for (int off = WAVE / 2; off >= 1; off >>= 1)
    for (int l = 0; l < off; l++) v[l] = v[l] + v[l + off];
  return v[0];
}

struct HostOps {
  const Problem& P;
  uint8_t* roundFlags;  // nullable [4][cap]
  int staleDiffers;     // flags the stale-error rule decided differently from a recomputation at the round's final pose

  void build(const Pose& T, bool robust, double* sum, Branches* br) {
    std::vector<double> acc((size_t)WAVE * POSE_ACC_BUILD, 0.0);
    int st = 0;
    for (int j = 0; j < P.n; j++) {
      const int i = pointOf(P, j, &st);
      if (i < 0 || P.outlier[j]) continue;
      Edge E;
      loadEdge(P, j, i, &E);
      br->lm.huberOutliers += edgeBuild(T, E, P.K, deltaOf(P, robust), &acc[(size_t)(j % WAVE) * POSE_ACC_BUILD]);
    }
    for (int k = 0; k < POSE_ACC_BUILD; k++) sum[k] = fold(acc.data(), POSE_ACC_BUILD, k);
  }

  double trial(const Pose& T, bool robust) {
    double acc[WAVE] = {0.0};
    int st = 0;
    for (int j = 0; j < P.n; j++) {
      const int i = pointOf(P, j, &st);
      if (i < 0 || P.outlier[j]) continue;
      Edge E;
      loadEdge(P, j, i, &E);
      acc[j % WAVE] = acc[j % WAVE] + edgeRho(T, E, P.K, deltaOf(P, robust));
    }
    return fold(acc, 1, 0);
  }

  int classify(const Pose& Tfinal, const Pose& Ttrial, int round) {
    int bad = 0, st = 0;
    for (int j = 0; j < P.n; j++) {
      const int i = pointOf(P, j, &st);
      if (i < 0) continue;
      Edge E;
      loadEdge(P, j, i, &E);
      const bool was = P.outlier[j] != 0;
      const bool out = edgeIsOutlier(Tfinal, Ttrial, was, E, P.K);
      if (!was && out != edgeIsOutlier(Tfinal, Tfinal, true, E, P.K)) staleDiffers++;
      P.outlier[j] = out ? 1 : 0;
      bad += out ? 1 : 0;
    }
    if (roundFlags) std::memcpy(roundFlags + (size_t)round * P.cap, P.outlier, (size_t)P.cap);
    return bad;
  }
};

double deltaHuber() { return (double)(float)std::sqrt(5.991); }

// the checks -> status bits and the number of edges
int gather(Problem& P, const float* pose0, int* nCorr) {
  int status = 0;
  *nCorr = 0;
  if (P.n < 0 || P.n > P.cap) {
    status |= ORBX_POSE_BAD_INPUT;
    P.n = 0;
  }
  for (int k = 0; k < 12; k++)
    if (!isFiniteF(pose0[k])) status |= ORBX_POSE_NONFINITE;
  std::memset(P.outlier, 0, (size_t)P.cap);
  for (int j = 0; j < P.n; j++) *nCorr += checkFeature(P, j, &status) ? 1 : 0;
  if (status == 0 && *nCorr < 3) status = ORBX_POSE_FEW_POINTS;
  return status;
}

Problem problem(const orbx_keypoint* kps, int n, int cap, const int32_t* match, const float* points, const uint8_t* mask,
                const float* K, const float* invSigma2, int nLevels, uint8_t* outlier) {
  Problem P;
  P.kps = kps; P.match = match; P.points = points; P.mask = mask; P.invSigma2 = invSigma2; P.outlier = outlier;
  P.n = n; P.cap = cap; P.nLevels = nLevels;
  P.K = Cam{(double)K[0], (double)K[4], (double)K[2], (double)K[5]};
  P.delta = deltaHuber();
  return P;
}

}  // namespace

extern "C" {

// The whole call for one problem; the arrays are the problem's own rows (kps [cap], match [cap] nullable, points [cap][3], mask
// [cap] nullable).  roundFlags nullable [4][cap]: the flags behind each round that ran.  counters [6]: accepted trials,
// rejected trials, edges in Huber's outlier branch (summed over every linearisation), uses of the theta < 1e-5 branch, rounds
// whose last trial was rejected, flags the stale-error rule decided differently from a recomputation.
void por_pose_optimize(const orbx_keypoint* kps, int n, int cap, const int32_t* match, const float* points, const uint8_t* mask,
                       const float* pose0, const float* K, const float* invSigma2, int nLevels, int nIterations, orbx_pose_result* out,
                       uint8_t* outlier, uint8_t* roundFlags, int64_t* counters) {
  Problem P = problem(kps, n, cap, match, points, mask, K, invSigma2, nLevels, outlier);
  int nCorr = 0;
  int status = gather(P, pose0, &nCorr);
  Rounds r{};
  Branches br{};
  Pose T{};
  HostOps ops{P, roundFlags, 0};
  if (roundFlags) std::memset(roundFlags, 0, (size_t)4 * cap);
  if (status == 0) {
    poseFromRt(pose0, pose0 + 9, &T);
    optimiseRounds(ops, &T, nCorr, nIterations, &r, &br);
    bool fin = isFinite(r.chi2Initial) && isFinite(r.chi2Final) && isFinite(r.lambda);
    for (int k = 0; k < 4; k++) fin = fin && isFinite(T.q[k]);
    for (int k = 0; k < 3; k++) fin = fin && isFinite(T.t[k]);
    if (!fin) {
      status = ORBX_POSE_NONFINITE;
      std::memset(outlier, 0, (size_t)cap);
    }
  }
  std::memset(out, 0, sizeof *out);
  out->status = status;
  if (status == 0 || status == ORBX_POSE_FEW_POINTS) out->n_correspondences = out->n_inliers = nCorr;
  if (status == 0) {
    out->n_bad = r.nBad;
    out->n_inliers = nCorr - r.nBad;
    out->rounds = r.rounds;
    for (int k = 0; k < 4; k++) {
      out->iterations[k] = r.iterations[k];
      out->stop_reason[k] = r.stopReason[k];
    }
    out->lm_trials = r.lmTrials;
    out->rejected_trials = r.rejected;
    out->solver_failures = r.solverFailures;
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
    std::memcpy(out->R, pose0, sizeof out->R);
    std::memcpy(out->tcw, pose0 + 9, sizeof out->tcw);
  }
  if (counters) {
    counters[0] = br.lm.accepted;
    counters[1] = br.lm.rejected;
    counters[2] = br.lm.huberOutliers;
    counters[3] = br.lm.smallTheta;
    counters[4] = br.endedOnRejected;
    counters[5] = ops.staleDiffers;
  }
}

// The first trial of iteration 0 of round 0 alone, for the independent statement: the start pose (q, t), lambda, chi2_initial and
// the step xp [6] = (omega, upsilon).  Returns the number of edges, or -1 when the inputs are refused or the solve failed.
int por_first_step(const orbx_keypoint* kps, int n, int cap, const int32_t* match, const float* points, const uint8_t* mask,
                   const float* pose0, const float* K, const float* invSigma2, int nLevels, double* pose7, double* lambda,
                   double* chi2Initial, double* xp) {
  std::vector<uint8_t> outlier((size_t)(cap > 0 ? cap : 1));
  Problem P = problem(kps, n, cap, match, points, mask, K, invSigma2, nLevels, outlier.data());
  int nCorr = 0;
  if (gather(P, pose0, &nCorr) != 0) return -1;
  Pose T;
  poseFromRt(pose0, pose0 + 9, &T);
  for (int k = 0; k < 4; k++) pose7[k] = T.q[k];
  for (int k = 0; k < 3; k++) pose7[4 + k] = T.t[k];
  HostOps ops{P, nullptr, 0};
  Branches br{};
  double sum[POSE_ACC_BUILD];
  const double zero[21] = {0.0};
  ops.build(T, true, sum, &br);
  Lm m;
  std::memset(&m, 0, sizeof m);
  for (int k = 0; k < 21; k++) m.Hpp[k] = sum[POSE_ACC_HPP + k];
  for (int k = 0; k < 6; k++) m.bp[k] = sum[POSE_ACC_BP + k];
  *chi2Initial = sum[POSE_ACC_CHI2];
  m.lambda = *lambda = lmLambdaInit(m.Hpp, 0.0);
  if (!lmSolvePose(&m, zero, zero)) return -1;
  for (int k = 0; k < 6; k++) xp[k] = m.xp[k];
  return nCorr;
}

double por_huber_delta() { return deltaHuber(); }

}  // extern "C"
