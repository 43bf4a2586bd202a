// orbx_pose_math.inc — the pose-only problem of Optimizer::PoseOptimization (include/orbx.h, "behind SearchByBoW: pose
// optimisation"): what one edge adds to the 6x6 system, an edge's chi2, the checks of a feature and the four rounds with their
// Levenberg-Marquardt loops, as plain f64 operations on top of orbx_ba_math.inc.  Shared by orbx_pose_kernel.hip (device) and
// tests/cpp/pose_ref.cpp (the CPU restatement, g++ -ffp-contract=off): one source, so both sides take the same operations in the
// same order and agree bit for bit.  What is NOT shared is how the features are spread over lanes and how the lanes' sums are
// combined: `Ops` below.  include/orbx.h fixes that order and each side implements it on its own.  [from-knowledge] restatements
// of ORB-SLAM2 / g2o, PARITY UNPINNED.
#include "orbx_ba_math.inc"

namespace orbx_pose {
using namespace orbx_ba;

// sums over the active edges (the indices of a lane's accumulator array)
enum {
  POSE_ACC_HPP = 0,    // 21: upper triangle of Hpp, row by row
  POSE_ACC_BP = 21,    // 6
  POSE_ACC_CHI2 = 27,  // activeRobustChi2
  POSE_ACC_BUILD = 28
};

// One problem's arrays, each already at the problem's frame / point set / row.
struct Problem {
  const orbx_keypoint* kps;  // [cap] mvKeysUn of the frame
  const int32_t* match;      // nullable [cap]: feature j's point is match[j]
  const float* points;       // [cap][3]
  const uint8_t* mask;       // nullable [cap]
  const float* invSigma2;    // [nLevels]
  uint8_t* outlier;          // [cap] the features' flags = the edges' levels
  int n, cap, nLevels;
  Cam K;
  double delta;              // RobustKernelHuber's
};

struct Edge {
  double X[3], u, v, w;
};

// what the rounds report besides the pose
struct Rounds {
  int rounds, nBad, lmTrials, rejected, solverFailures;
  int iterations[4], stopReason[4];
  double chi2Initial, chi2Final, lambda;
};
// which branches ran (the restatement reports them; the device drops them)
struct Branches {
  Counters lm;
  int endedOnRejected;  // rounds whose last trial was rejected
};

constexpr int POSE_STATUS_BAD_INPUT = 2, POSE_STATUS_NONFINITE = 4;  // ORBX_POSE_BAD_INPUT, ORBX_POSE_NONFINITE

// Feature j (< n <= cap) of a problem: the index of its map point in the point set, or -1 without one.  A match index >= cap
// sets BAD_INPUT and is not followed.
ORBX_BA_FN inline int pointOf(const Problem& P, int j, int* status) {
  int i = j;
  if (P.match) {
    i = P.match[j];
    if (i >= P.cap) {
      *status |= POSE_STATUS_BAD_INPUT;
      return -1;
    }
    if (i < 0) return -1;
  }
  if (P.mask && P.mask[i] == 0) return -1;
  return i;
}

// The checks of feature j before anything is optimised: whether it has an edge; an octave outside the table and a non-finite
// point set their bits.
ORBX_BA_FN inline bool checkFeature(const Problem& P, int j, int* status) {
  const int i = pointOf(P, j, status);
  if (i < 0) return false;
  const int o = P.kps[j].octave;
  if (o < 0 || o >= P.nLevels) {
    *status |= POSE_STATUS_BAD_INPUT;
    return false;
  }
  for (int c = 0; c < 3; c++)
    if (!isFiniteF(P.points[(size_t)i * 3 + c])) *status |= POSE_STATUS_NONFINITE;
  return true;
}

// the edge of a feature that passed checkFeature (i = pointOf)
ORBX_BA_FN inline void loadEdge(const Problem& P, int j, int i, Edge* E) {
  for (int c = 0; c < 3; c++) E->X[c] = (double)P.points[(size_t)i * 3 + c];
  E->u = (double)P.kps[j].x;
  E->v = (double)P.kps[j].y;
  E->w = (double)P.invSigma2[P.kps[j].octave];
}

// RobustKernelHuber's delta, or none: with an infinite delta robustify's first branch gives rho[0] = chi2, rho[1] = 1
ORBX_BA_FN inline double deltaOf(const Problem& P, bool robust) { return robust ? P.delta : __builtin_inf(); }

// One active edge's part of buildSystem: computeError, the robust chi2, linearizeOplus' pose Jacobian and constructQuadraticForm
// for the pose block (the point is fixed: base_binary_edge.hpp:65-113 adds no other block).  Returns 1 in Huber's outlier branch.
ORBX_BA_FN inline int edgeBuild(const Pose& T, const Edge& E, const Cam& K, double delta, double* acc) {
  double pc[3], e[2], rho[2], A[2][3], B[2][6];
  const double I[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  poseMap(T, E.X, pc);
  edgeError(pc, E.u, E.v, E.w, K, delta, e, rho);
  acc[POSE_ACC_CHI2] = acc[POSE_ACC_CHI2] + rho[0];
  edgeJacobians(pc, I, true, K, A, B);  // (A, the fixed point's Jacobian, is not used)
  const double r[2] = {-(E.w * e[0]) * rho[1], -(E.w * e[1]) * rho[1]};
  const double o = rho[1] * E.w;
  int k = 0;
  for (int p = 0; p < 6; p++) {
    for (int q = p; q < 6; q++, k++)
      acc[POSE_ACC_HPP + k] = acc[POSE_ACC_HPP + k] + (B[0][p] * (o * B[0][q]) + B[1][p] * (o * B[1][q]));
    acc[POSE_ACC_BP + p] = acc[POSE_ACC_BP + p] + (B[0][p] * r[0] + B[1][p] * r[1]);
  }
  return rho[1] != 1.0 ? 1 : 0;
}

// rho[0] of an edge at T (a trial's activeRobustChi2), and with an infinite delta its plain chi2 = e . (information e)
ORBX_BA_FN inline double edgeRho(const Pose& T, const Edge& E, const Cam& K, double delta) {
  double pc[3], e[2], rho[2];
  poseMap(T, E.X, pc);
  edgeError(pc, E.u, E.v, E.w, K, delta, e, rho);
  return rho[0];
}

// The classification of one edge behind a round: `const float chi2 = e->chi2(); if (chi2 > chi2Mono[it])` with chi2Mono = 5.991f.
// An edge that was active keeps the error of the round's last trial; one that was an outlier is recomputed at the round's pose.
ORBX_BA_FN inline bool edgeIsOutlier(const Pose& Tfinal, const Pose& Ttrial, bool wasOutlier, const Edge& E, const Cam& K) {
  const double chi2 = edgeRho(wasOutlier ? Tfinal : Ttrial, E, K, __builtin_inf());
  return (float)chi2 > 5.991f;
}

// The four rounds.  Ops supplies the three passes over the features, each in the documented lane order:
//   void build(const Pose& T, bool robust, double sum[POSE_ACC_BUILD], Branches*)  the active edges' sums
//   double trial(const Pose& T, bool robust)                                      the active edges' robust chi2
//   int classify(const Pose& Tfinal, const Pose& Ttrial, int round)               new flags, returns the outliers
// T comes in as the initial estimate and goes out as the pose after the last round that ran.
template <class Ops>
ORBX_BA_FN inline void optimiseRounds(Ops& ops, Pose* T, int nCorrespondences, int nIterations, Rounds* r, Branches* br) {
  const Pose T0 = *T;
  const double zero[21] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  Lm m;
  m.lambda = 0.0; m.ni = 2.0; m.currentChi = 0.0; m.iniChi = 0.0; m.rho = 0.0;
  m.nBad = 0; m.qmax = 0; m.ok = 0;
  m.iterations = 0; m.lmTrials = 0; m.rejected = 0; m.solverFailures = 0; m.stopReason = 0;
  r->rounds = 0; r->nBad = 0;
  r->chi2Initial = 0.0; r->chi2Final = 0.0; r->lambda = 0.0;
  for (int k = 0; k < 4; k++) r->iterations[k] = r->stopReason[k] = 0;
  for (int it = 0; it < 4; it++) {
    const bool robust = it < 3;  // `if (it == 2) e->setRobustKernel(0)`
    Pose cur = T0, Ttrial = T0;  // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw))
    int iterations = 0, stop = 0, lastAccepted = 1;
    if (nCorrespondences - r->nBad > 0) {
      for (int i = 0; i < nIterations; i++) {
        double sum[POSE_ACC_BUILD];
        ops.build(cur, robust, sum, br);
        for (int k = 0; k < 21; k++) m.Hpp[k] = sum[POSE_ACC_HPP + k];
        for (int k = 0; k < 6; k++) m.bp[k] = sum[POSE_ACC_BP + k];
        m.currentChi = m.iniChi = sum[POSE_ACC_CHI2];
        if (i == 0) {
          if (it == 0) r->chi2Initial = m.currentChi;
          m.lambda = lmLambdaInit(m.Hpp, 0.0);
          m.ni = 2.0;
          m.nBad = 0;
        }
        m.rho = 0.0;
        m.qmax = 0;
        do {
          const Pose backup = cur;
          m.ok = lmSolvePose(&m, zero, zero) ? 1 : 0;
          double tchi = 0.0;
          if (!m.ok) {
            m.solverFailures++;
          } else {
            if (poseOplus(m.xp, &cur)) br->lm.smallTheta++;
            tchi = ops.trial(cur, robust);
          }
          Ttrial = cur;
          lastAccepted = lmJudge(&m, tchi, 0.0, &br->lm);
          if (!lastAccepted) cur = backup;
        } while (lmAnotherTrial(&m));
        stop = lmEndIteration(&m);
        iterations++;
        if (stop) break;
      }
      r->chi2Final = m.currentChi;
      r->lambda = m.lambda;
    }
    if (iterations > 0 && !lastAccepted) br->endedOnRejected++;
    r->nBad = ops.classify(cur, Ttrial, it);
    r->iterations[it] = iterations;
    r->stopReason[it] = stop;
    r->rounds = it + 1;
    *T = cur;
    if (nCorrespondences < 10) break;  // `if (optimizer.edges().size() < 10) break`
  }
  r->lmTrials = m.lmTrials;
  r->rejected = m.rejected;
  r->solverFailures = m.solverFailures;
}

}  // namespace orbx_pose
