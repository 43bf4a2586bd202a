// orbx_sim3opt_math.inc — Optimizer::OptimizeSim3 (include/orbx.h, "loop closing: Sim3 optimisation"): g2o's Sim3 (types/sim3.h),
// VertexSim3Expmap's oplus, the errors of EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ (types/types_seven_dof_expmap.h), the
// numeric Jacobian of BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp:131-200), the 7x7 system with its Levenberg-
// Marquardt bookkeeping and the two rounds with their classifications, as plain f64 operations on top of orbx_ba_math.inc.
// Shared by orbx_sim3opt_kernel.hip (device) and tests/cpp/sim3opt_ref.cpp (the CPU restatement, g++ -ffp-contract=off): one
// source, so both sides take the same operations in the same order and agree bit for bit.  What is NOT shared is how the
// correspondences are spread over lanes, how the lanes' sums are combined and who computes the fourteen perturbed similarities:
// `Ops` below.  include/orbx.h fixes that order and each side implements it on its own.  Only +, -, *, /, sqrt, comparisons and
// one bit copy (the scaling by 2^k in expF64) are used.  [from-knowledge] restatements of ORB-SLAM2 / g2o, PARITY UNPINNED.
#include "orbx_ba_math.inc"

// An int every lane of the device's wave holds with equal bits, because it was computed from the folded sums: the device takes
// lane 0's copy, which tells its compiler that the branches on it are scalar and keeps the counters out of the vector registers.
// The value is unchanged; nothing on the host.
#ifndef ORBX_S3O_UNIFORM
#define ORBX_S3O_UNIFORM(v) (v)
#endif

namespace orbx_sim3opt {
using namespace orbx_ba;

// sums over a round's edges (the indices of a lane's accumulator array)
enum {
  S3O_ACC_H = 0,      // 28: upper triangle of the 7x7 H, row by row
  S3O_ACC_B = 28,     // 7
  S3O_ACC_CHI2 = 35,  // activeRobustChi2
  S3O_ACC_BUILD = 36
};

constexpr int S3O_STATUS_BAD_INPUT = 2, S3O_STATUS_NONFINITE = 4;  // ORBX_SIM3OPT_BAD_INPUT, ORBX_SIM3OPT_NONFINITE
// A row entry removed by the first classification holds i2 + S3O_REMOVED until the call ends (no entry of a problem that runs
// is that large: i2 < KF2's count <= capacity <= 16384), so that a non-finite result can still return the row untouched.
constexpr int S3O_REMOVED = 1 << 30;

// g2o's Sim3: Quaterniond r (x y z w, never normalised), Vector3d t, double s
struct Sim3 {
  double q[4], t[3], s;
};

// ---- exp on [-700, 700]: fdlibm's e_exp.c.  x = k ln2 + r with ln2 in two parts (k * ln2Hi is exact: |k| <= 1010 and ln2Hi
// ends in 21 zero bits), the polynomial of e_exp.c on |r| <= 0.5 ln2, and the scaling by 2^k as a multiplication by the double
// with the exponent field 1023 + k, which is exact here: the result is a normal number.  |x| < 2^-28 gives 1 + x.  Outside the
// domain (or NaN) the result is NaN.
constexpr double S3O_EXP_HALF_LN2 = 0.34657359027997264, S3O_EXP_THREE_HALVES_LN2 = 1.0397207708399179,
                 S3O_EXP_TINY = 3.725290298461914e-09, S3O_EXP_MAX = 700.0;
ORBX_BA_FN inline double expF64(double x) {
  if (!(x >= -S3O_EXP_MAX && x <= S3O_EXP_MAX)) return notANumber();
  const double ln2Hi = 6.93147180369123816490e-01, ln2Lo = 1.90821492927058770002e-10, invLn2 = 1.44269504088896338700e+00;
  const double P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
               P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
  const double ax = x < 0.0 ? -x : x;
  double hi = 0.0, lo = 0.0;
  int k = 0;
  if (ax > S3O_EXP_HALF_LN2) {
    if (ax < S3O_EXP_THREE_HALVES_LN2) {
      k = x < 0.0 ? -1 : 1;
      hi = x < 0.0 ? x + ln2Hi : x - ln2Hi;
      lo = x < 0.0 ? -ln2Lo : ln2Lo;
    } else {
      k = (int)(invLn2 * x + (x < 0.0 ? -0.5 : 0.5));
      const double fk = (double)k;
      hi = x - fk * ln2Hi;
      lo = fk * ln2Lo;
    }
    x = hi - lo;
  } else if (ax < S3O_EXP_TINY) {
    return 1.0 + x;
  }
  const double t = x * x;
  const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
  if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
  const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
  const unsigned long long bits = (unsigned long long)(1023 + k) << 52;
  double twoK;
  __builtin_memcpy(&twoK, &bits, sizeof twoK);
  return y * twoK;
}

// ---- g2o's Sim3 ------------------------------------------------------------------------------------------------
// Quaterniond * Quaterniond (Eigen's quat_product), not normalised
ORBX_BA_FN inline void quatMul(const double a[4], const double b[4], double out[4]) {
  out[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
  out[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
  out[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
  out[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
}

// Sim3(Matrix3d R, Vector3d t, double s) (sim3.h:64-67) from the f32 row R12 row-major, t12, s12: no sign flip, no normalisation
ORBX_BA_FN inline void sim3FromRow(const float* sim, Sim3* S) {
  double m[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) m[i][j] = (double)sim[i * 3 + j];
  quatFromMatrix(m, S->q);
  for (int i = 0; i < 3; i++) S->t[i] = (double)sim[9 + i];
  S->s = (double)sim[12];
}

// which branches of Sim3(Vector7d) ran
constexpr int S3O_SMALL_THETA = 1, S3O_SMALL_SIGMA = 2;

// Sim3(const Vector7d& update) (sim3.h:70-142); update = (omega, upsilon, sigma).  Returns S3O_SMALL_* of the branches taken.
ORBX_BA_FN inline int sim3Exp(const double u[7], Sim3* S) {
  const double om[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
  const double sigma = u[6];
  const double theta = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
  const double O[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
  const double s = expF64(sigma);
  double O2[3][3], R[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) O2[i][j] = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j];
  const double eps = 0.00001;
  const bool smallSigma = (sigma < 0.0 ? -sigma : sigma) < eps, smallTheta = theta < eps;
  double A, B, C;
  if (smallTheta) {  // R = (I + Omega + Omega * Omega): kept without the 1/2
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
  } else {  // R = I + sin(theta) / theta * Omega + (1 - cos(theta)) / (theta * theta) * Omega2
    double sn, cs;
    sinCos(theta, &sn, &cs);
    const double a = sn / theta, b = (1.0 - cs) / (theta * theta);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + a * O[i][j]) + b * O2[i][j];
  }
  if (smallSigma) {
    C = 1.0;
    if (smallTheta) {
      A = 1.0 / 2.0;
      B = 1.0 / 6.0;
    } else {
      double sn, cs;
      sinCos(theta, &sn, &cs);
      const double theta2 = theta * theta;
      A = (1.0 - cs) / theta2;
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (s - 1.0) / sigma;
    if (smallTheta) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1.0) * s + 1.0) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma);
    } else {
      double sn, cs;
      sinCos(theta, &sn, &cs);
      const double a = s * sn, b = s * cs;
      const double theta2 = theta * theta, sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1.0 - b) * theta) / (theta * c);
      B = (C - ((b - 1.0) * sigma + a * theta) / c) / theta2;  // (`* 1. / (theta2)`: the product with 1 is exact)
    }
  }
  quatFromMatrix(R, S->q);
  // W = A * Omega + B * Omega2 + C * I; t = W * upsilon
  for (int i = 0; i < 3; i++) {
    double W[3];
    for (int j = 0; j < 3; j++) W[j] = (A * O[i][j] + B * O2[i][j]) + C * (i == j ? 1.0 : 0.0);
    S->t[i] = (W[0] * up[0] + W[1] * up[1]) + W[2] * up[2];
  }
  S->s = s;
  return (smallTheta ? S3O_SMALL_THETA : 0) | (smallSigma ? S3O_SMALL_SIGMA : 0);
}

// Sim3::map (sim3.h:144-146): s * (r * xyz) + t
ORBX_BA_FN inline void sim3Map(const Sim3& S, const double X[3], double out[3]) {
  double r[3];
  quatRotate(S.q, X, r);
  for (int i = 0; i < 3; i++) out[i] = S.s * r[i] + S.t[i];
}

// Sim3::operator* (sim3.h:266-272)
ORBX_BA_FN inline void sim3Mul(const Sim3& a, const Sim3& b, Sim3* out) {
  Sim3 r;
  quatMul(a.q, b.q, r.q);
  sim3Map(a, b.t, r.t);
  r.s = a.s * b.s;
  *out = r;
}

// Sim3::inverse (sim3.h:233-236): Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
ORBX_BA_FN inline void sim3Inverse(const Sim3& S, Sim3* out) {
  Sim3 r;
  r.q[0] = -S.q[0]; r.q[1] = -S.q[1]; r.q[2] = -S.q[2]; r.q[3] = S.q[3];
  const double f = -1.0 / S.s;
  const double v[3] = {f * S.t[0], f * S.t[1], f * S.t[2]};
  quatRotate(r.q, v, r.t);
  r.s = 1.0 / S.s;
  *out = r;
}

// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69): update[6] = 0 under _fix_scale, then Sim3(update) * estimate
ORBX_BA_FN inline int sim3Oplus(const double update[7], bool fixScale, Sim3* S) {
  double u[7];
  for (int i = 0; i < 7; i++) u[i] = update[i];
  if (fixScale) u[6] = 0.0;
  Sim3 E;
  const int branches = sim3Exp(u, &E);
  sim3Mul(E, *S, S);
  return branches;
}

// The estimate linearizeOplus evaluates for perturbation k = 2 d + (0: +1e-9, 1: -1e-9) of dimension d, and its inverse
// (base_binary_edge.hpp:147, :181-193).  They depend on the estimate alone, not on the edge.
ORBX_BA_FN inline void sim3Perturbed(const Sim3& S, bool fixScale, int k, Sim3* out, Sim3* outInverse) {
  const double delta = 1e-9;
  double u[7];
  for (int i = 0; i < 7; i++) u[i] = i == (k >> 1) ? ((k & 1) ? -delta : delta) : 0.0;
  *out = S;
  (void)sim3Oplus(u, fixScale, out);
  sim3Inverse(*out, outInverse);
}

// ---- the two edges ------------------------------------------------------------------------------------------------
// VertexSim3Expmap::cam_map1 / cam_map2 (types_seven_dof_expmap.h:74-88) of project(P) = (P[0] / P[2], P[1] / P[2])
ORBX_BA_FN inline void camMap(const double P[3], const Cam& K, double uv[2]) {
  const double v[2] = {P[0] / P[2], P[1] / P[2]};
  uv[0] = v[0] * K.fx + K.cx;
  uv[1] = v[1] * K.fy + K.cy;
}

// computeError of either edge (:138-145 with the estimate, :160-167 with its inverse): obs - cam_map(project(S.map(P)))
ORBX_BA_FN inline void edgeErr(const Sim3& S, const double P[3], double u, double v, const Cam& K, double e[2]) {
  double pc[3], uv[2];
  sim3Map(S, P, pc);
  camMap(pc, K, uv);
  e[0] = u - uv[0];
  e[1] = v - uv[1];
}

// chi2() = e . (information e) with information = w I
ORBX_BA_FN inline double edgeChi2(const double e[2], double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1]
ORBX_BA_FN inline void huber(double chi2, double delta, double rho[2]) {
  const double dsqr = delta * delta;
  if (chi2 <= dsqr) {
    rho[0] = chi2;
    rho[1] = 1.0;
  } else {
    const double sqrte = sqrt(chi2);
    rho[0] = 2.0 * sqrte * delta - dsqr;
    rho[1] = delta / sqrte;
  }
}

// One correspondence: the fixed points of both cameras' frames, both observations and informations
struct Edge {
  double P1[3], P2[3];  // the point of KF1 in camera 1's frame, of KF2 in camera 2's
  double u1, v1, w1, u2, v2, w2;
};

// One edge's part of buildSystem.  S: the estimate (e12) or its inverse (e21); pert [14]: the perturbed estimates (e12) or their
// inverses (e21), k = 2 d + sign.  computeError, the robust chi2, the numeric Jacobian -- column d = (1 / (2 * 1e-9)) * (error at
// +1e-9 e_d - error at -1e-9 e_d), the subtraction first -- and constructQuadraticForm's robust branch for the Sim3 block (the
// point is fixed: base_binary_edge.hpp:91-113 adds no other block).  Returns 1 in Huber's outlier branch.
template <class PertPtr>
ORBX_BA_FN inline int edgeBuild(const Sim3& S, PertPtr pert, const double P[3], double u, double v, double w, const Cam& K,
                                double delta, double* acc) {
  const double scalar = 1.0 / (2 * 1e-9);
  double e[2], rho[2], J[2][7];
  edgeErr(S, P, u, v, K, e);
  huber(edgeChi2(e, w), delta, rho);
  acc[S3O_ACC_CHI2] = acc[S3O_ACC_CHI2] + rho[0];
  for (int d = 0; d < 7; d++) {
    double ep[2], em[2];
    const Sim3 Sp = pert[2 * d], Sm = pert[2 * d + 1];
    edgeErr(Sp, P, u, v, K, ep);
    edgeErr(Sm, P, u, v, K, em);
    J[0][d] = scalar * (ep[0] - em[0]);
    J[1][d] = scalar * (ep[1] - em[1]);
  }
  // omega_r = -(omega e) * rho[1]; weightedOmega = rho[1] * omega
  const double r[2] = {-(w * e[0]) * rho[1], -(w * e[1]) * rho[1]};
  const double o = rho[1] * w;
  int k = 0;
  for (int p = 0; p < 7; p++) {
    for (int q = p; q < 7; q++, k++) acc[S3O_ACC_H + k] = acc[S3O_ACC_H + k] + (J[0][p] * (o * J[0][q]) + J[1][p] * (o * J[1][q]));
    acc[S3O_ACC_B + p] = acc[S3O_ACC_B + p] + (J[0][p] * r[0] + J[1][p] * r[1]);
  }
  return rho[1] != 1.0 ? 1 : 0;
}

// A correspondence's part of buildSystem: e12 before e21.  pert [2][14]: the perturbed estimates, then their inverses.
template <class PertPtr>
ORBX_BA_FN inline int pairBuild(const Sim3& S, const Sim3& Sinv, PertPtr pert, const Edge& E, const Cam& K, double delta, double* acc) {
  int n = edgeBuild(S, pert, E.P2, E.u1, E.v1, E.w1, K, delta, acc);
  n += edgeBuild(Sinv, pert + 14, E.P1, E.u2, E.v2, E.w2, K, delta, acc);
  return n;
}

// A correspondence's part of a trial's activeRobustChi2 added to *chi2, e12 before e21
ORBX_BA_FN inline void pairRho(const Sim3& S, const Sim3& Sinv, const Edge& E, const Cam& K, double delta, double* chi2) {
  double e[2], rho[2];
  edgeErr(S, E.P2, E.u1, E.v1, K, e);
  huber(edgeChi2(e, E.w1), delta, rho);
  *chi2 = *chi2 + rho[0];
  edgeErr(Sinv, E.P1, E.u2, E.v2, K, e);
  huber(edgeChi2(e, E.w2), delta, rho);
  *chi2 = *chi2 + rho[0];
}

// The classification of a correspondence: `e12->chi2() > th2 || e21->chi2() > th2`, unrobustified, f64.  which (nullable): bit 0
// = e12 fails, bit 1 = e21 fails.
ORBX_BA_FN inline bool pairIsOutlier(const Sim3& S, const Sim3& Sinv, const Edge& E, const Cam& K, double th2, int* which) {
  double e[2];
  edgeErr(S, E.P2, E.u1, E.v1, K, e);
  const bool bad12 = edgeChi2(e, E.w1) > th2;
  edgeErr(Sinv, E.P1, E.u2, E.v2, K, e);
  const bool bad21 = edgeChi2(e, E.w2) > th2;
  if (which) *which = (bad12 ? 1 : 0) | (bad21 ? 2 : 0);
  return bad12 || bad21;
}

// ---- a problem's arrays and the checks of a feature --------------------------------------------------------------
struct Problem {
  const orbx_keypoint *kps1, *kps2;  // [cap] mvKeysUn of KF1 / KF2
  int32_t* row;                      // [cap] vpMatches1: KF2's feature of KF1's feature, in and out
  const float *points1, *points2;    // [cap][3], each indexed by its own keyframe's feature
  const uint8_t *mask1, *mask2;      // nullable [cap]
  const float *pose1, *pose2;        // [12] Tcw of KF1 / KF2
  const float* invSigma2;            // [nLevels]
  int n1, n2, cap, nLevels;
  Cam K;
  double delta, th2;
  bool fixScale;
};

// Feature i1 (< n1) of KF1: its feature of KF2 when they are a correspondence, or -1.  A row entry >= n2 sets BAD_INPUT (an
// entry the first classification removed is passed over) and is not followed.
ORBX_BA_FN inline int partnerOf(const Problem& P, int i1, int* status) {
  const int i2 = P.row[i1];
  if (i2 < 0 || i2 >= S3O_REMOVED) return -1;
  if (i2 >= P.n2) {
    *status |= S3O_STATUS_BAD_INPUT;
    return -1;
  }
  if (P.mask1 && (P.mask1[i1] == 0 || P.mask2[i2] == 0)) return -1;
  return i2;
}

// The checks of feature i1 before anything is optimised: whether it is a correspondence; an octave outside the table sets
// BAD_INPUT, a non-finite point or keypoint NONFINITE.
ORBX_BA_FN inline bool checkFeature(const Problem& P, int i1, int* status) {
  if (P.row[i1] >= P.n2) {  // (before any removal: an entry of S3O_REMOVED or more is garbage like every other one >= n2)
    *status |= S3O_STATUS_BAD_INPUT;
    return false;
  }
  const int i2 = partnerOf(P, i1, status);
  if (i2 < 0) return false;
  const int o1 = P.kps1[i1].octave, o2 = P.kps2[i2].octave;
  if (o1 < 0 || o1 >= P.nLevels || o2 < 0 || o2 >= P.nLevels) {
    *status |= S3O_STATUS_BAD_INPUT;
    return false;
  }
  bool fin = isFiniteF(P.kps1[i1].x) && isFiniteF(P.kps1[i1].y) && isFiniteF(P.kps2[i2].x) && isFiniteF(P.kps2[i2].y);
  for (int c = 0; c < 3; c++) fin = fin && isFiniteF(P.points1[(size_t)i1 * 3 + c]) && isFiniteF(P.points2[(size_t)i2 * 3 + c]);
  if (!fin) *status |= S3O_STATUS_NONFINITE;
  return true;
}

// Rcw * Xw + tcw in f32, each row's products added left to right, then the translation ("loop closing: Sim3 RANSAC", rule 1),
// taken to f64 afterwards
ORBX_BA_FN inline void toCamera(const float* pose, const float* X, double out[3]) {
  for (int r = 0; r < 3; r++) out[r] = (double)(pose[3 * r] * X[0] + pose[3 * r + 1] * X[1] + pose[3 * r + 2] * X[2] + pose[9 + r]);
}

// the two edges of a correspondence that passed checkFeature (i2 = partnerOf)
ORBX_BA_FN inline void loadEdge(const Problem& P, int i1, int i2, Edge* E) {
  toCamera(P.pose1, P.points1 + (size_t)i1 * 3, E->P1);
  toCamera(P.pose2, P.points2 + (size_t)i2 * 3, E->P2);
  E->u1 = (double)P.kps1[i1].x;
  E->v1 = (double)P.kps1[i1].y;
  E->w1 = (double)P.invSigma2[P.kps1[i1].octave];
  E->u2 = (double)P.kps2[i2].x;
  E->v2 = (double)P.kps2[i2].y;
  E->w2 = (double)P.invSigma2[P.kps2[i2].octave];
}

// ---- the 7x7 system and the Levenberg-Marquardt bookkeeping: run by every lane on equal bits ----------------------
struct Lm7 {
  double H[28], b[7];  // of the current linearisation (upper triangle)
  double lambda, ni, currentChi, iniChi, rho;
  double x[7];
  int nBad, qmax, ok;
  int lmTrials, rejected, solverFailures;
};

// (H + lambda I) x = b by the project's unblocked lower Cholesky (g2o's LinearSolverDense is an Eigen::LDLT: a documented
// deviation).  A pivot <= 0 or non-finite, or a non-finite solution, is a failed solve: x = 0.  Returns whether it solved.
ORBX_BA_FN inline bool lmSolve7(Lm7* m) {
  double L[7][7], y[7];
  int k = 0;
  for (int p = 0; p < 7; p++) {
    for (int q = p; q < 7; q++, k++) {
      double h = m->H[k];
      if (p == q) h = h + m->lambda;
      L[q][p] = h;  // lower triangle
    }
    m->x[p] = 0.0;
  }
  for (int j = 0; j < 7; j++) {
    double d = L[j][j];
    for (int c = 0; c < j; c++) d = d - L[j][c] * L[j][c];
    if (ORBX_S3O_UNIFORM((int)(!(d > 0.0) || !isFinite(d)))) return false;
    const double ljj = sqrt(d);
    L[j][j] = ljj;
    for (int i = j + 1; i < 7; i++) {
      double v = L[i][j];
      for (int c = 0; c < j; c++) v = v - L[i][c] * L[j][c];
      L[i][j] = v / ljj;
    }
  }
  for (int i = 0; i < 7; i++) {
    double v = m->b[i];
    for (int c = 0; c < i; c++) v = v - L[i][c] * y[c];
    y[i] = v / L[i][i];
  }
  for (int i = 6; i >= 0; i--) {
    double v = y[i];
    for (int c = i + 1; c < 7; c++) v = v - L[c][i] * m->x[c];
    m->x[i] = v / L[i][i];
  }
  bool fin = true;
  for (int i = 0; i < 7; i++) fin = fin && isFinite(m->x[i]);
  fin = ORBX_S3O_UNIFORM((int)fin) != 0;
  if (!fin)
    for (int c = 0; c < 7; c++) m->x[c] = 0.0;
  return fin;
}

// computeLambdaInit (optimization_algorithm_levenberg.cpp:166-180) over the seven diagonal entries
ORBX_BA_FN inline double lmLambdaInit7(const double* H) {
  double mx = 0.0;
  int k = 0;
  for (int p = 0; p < 7; k += 7 - p, p++) {
    const double a = H[k] < 0.0 ? -H[k] : H[k];
    if (a > mx) mx = a;
  }
  return 1e-5 * mx;
}

// One trial's verdict (:123-149), computeScale (:182-189) over the seven terms.  Returns 1 = accepted, 0 = rejected.
ORBX_BA_FN inline int lmJudge7(Lm7* m, double tempChi, Counters* cnt) {
  if (!m->ok) tempChi = 1.7976931348623157e308;  // std::numeric_limits<double>::max()
  double rho = m->currentChi - tempChi;
  double scale = 0.0;
  for (int i = 0; i < 7; i++) scale = scale + m->x[i] * (m->lambda * m->x[i] + m->b[i]);
  scale = scale + 1e-3;
  rho = rho / scale;
  int accepted;
  if (ORBX_S3O_UNIFORM((int)(rho > 0.0 && isFinite(tempChi)))) {
    const double t = 2.0 * rho - 1.0;
    double alpha = 1.0 - (t * t) * t;
    if (!(alpha < 2.0 / 3.0)) alpha = alpha != alpha ? alpha : 2.0 / 3.0;  // std::min(alpha, 2/3): a NaN alpha stays
    const double scaleFactor = 1.0 / 3.0 < alpha ? alpha : 1.0 / 3.0;       // std::max(1/3, alpha)
    m->lambda = m->lambda * scaleFactor;
    m->ni = 2.0;
    m->currentChi = tempChi;
    accepted = 1;
    cnt->accepted++;
  } else {
    m->lambda = m->lambda * m->ni;
    m->ni = m->ni * 2.0;
    accepted = 0;
    m->rejected++;
    cnt->rejected++;
  }
  m->rho = rho;
  m->qmax++;
  m->lmTrials++;
  return accepted;
}

// what the rounds report besides the similarity
struct Rounds {
  int rounds, nBad, nInliers, lmTrials, rejected, solverFailures;
  int iterations[2], stopReason[2];
  int smallTheta, smallSigma, smallBoth;  // LM steps whose Sim3(update) took the theta < 1e-5 / |sigma| < 1e-5 / both branches
  double chi2Initial, chi2Final, lambda;
};
// which branches ran (the restatement reports them; the device drops them)
struct Branches {
  Counters lm;
  int endedOnRejected;  // rounds whose last trial was rejected
};

// The two rounds.  Ops supplies the three passes over the correspondences, each in the documented lane order:
//   void build(const Sim3& S, double sum[S3O_ACC_BUILD], Branches*)   the linearisation at S: the sums of all edges
//   double trial(const Sim3& S)                                       the edges' robust chi2 at S
//   void keep(const Sim3& S)                                          remembers the estimate of the round's last trial
//   int classify()                                                    removes the correspondences that fail at the estimate
//                                                                     kept last from the row, returns their number
// S comes in as the initial estimate and goes out as the vertex' estimate; false: `nCorrespondences - nBad < 10`, the caller
// keeps the similarity it gave (and makes the start estimate again if it wants it: nothing here holds it that long).  nIterations: of the first round and of a second round behind nBad == 0; nMoreIterations: of a
// second round behind nBad > 0.
template <class Ops>
ORBX_BA_FN inline bool optimiseSim3(Ops& ops, Sim3* S, bool fixScale, int nCorrespondences, int nIterations, int nMoreIterations,
                                    Rounds* r, Branches* br) {
  Lm7 m;
  m.lambda = 0.0; m.ni = 2.0; m.currentChi = 0.0; m.iniChi = 0.0; m.rho = 0.0;
  m.nBad = 0; m.qmax = 0; m.ok = 0;
  m.lmTrials = 0; m.rejected = 0; m.solverFailures = 0;
  r->rounds = 0; r->nBad = 0; r->nInliers = 0;
  r->smallTheta = 0; r->smallSigma = 0; r->smallBoth = 0;
  r->chi2Initial = 0.0; r->chi2Final = 0.0; r->lambda = 0.0;
  for (int k = 0; k < 2; k++) r->iterations[k] = r->stopReason[k] = 0;
  Sim3 cur = *S;
  bool recovered = false;
  for (int it = 0; it < 2; it++) {
    const int nIts = it == 0 ? nIterations : (r->nBad > 0 ? nMoreIterations : nIterations);
    ops.keep(cur);  // (the second round continues from the current estimate: there is no reset)
    int iterations = 0, stop = 0, lastAccepted = 1;
    for (int i = 0; i < nIts; i++) {
      double sum[S3O_ACC_BUILD];
      ops.build(cur, sum, br);
      for (int k = 0; k < 28; k++) m.H[k] = sum[S3O_ACC_H + k];
      for (int k = 0; k < 7; k++) m.b[k] = sum[S3O_ACC_B + k];
      m.currentChi = m.iniChi = sum[S3O_ACC_CHI2];
      if (i == 0) {
        if (it == 0) r->chi2Initial = m.currentChi;
        m.lambda = lmLambdaInit7(m.H);
        m.ni = 2.0;
        m.nBad = 0;
      }
      m.rho = 0.0;
      m.qmax = 0;
      do {
        const Sim3 backup = cur;
        m.ok = lmSolve7(&m) ? 1 : 0;
        double tchi = 0.0;
        if (!m.ok) {
          m.solverFailures++;
        } else {
          const int branches = ORBX_S3O_UNIFORM(sim3Oplus(m.x, fixScale, &cur));
          r->smallTheta += (branches & S3O_SMALL_THETA) ? 1 : 0;
          r->smallSigma += (branches & S3O_SMALL_SIGMA) ? 1 : 0;
          r->smallBoth += branches == (S3O_SMALL_THETA | S3O_SMALL_SIGMA) ? 1 : 0;
          tchi = ops.trial(cur);
        }
        ops.keep(cur);  // accepted or not: the edges keep this trial's errors
        lastAccepted = lmJudge7(&m, tchi, &br->lm);
        if (!lastAccepted) cur = backup;
      } while (ORBX_S3O_UNIFORM((int)(m.rho < 0.0 && m.qmax < 10)));
      // the end of solve() (:151-163): 1 = Terminate by `qmax == 10 || rho == 0`, 2 = Terminate by `_nBad >= 3`
      if (ORBX_S3O_UNIFORM((int)(m.qmax == 10 || m.rho == 0.0))) {
        stop = 1;
      } else {
        if (ORBX_S3O_UNIFORM((int)((m.iniChi - m.currentChi) * 1e3 < m.iniChi)))
          m.nBad++;
        else
          m.nBad = 0;
        stop = m.nBad >= 3 ? 2 : 0;
      }
      iterations++;
      if (stop) break;
    }
    if (iterations > 0) {
      r->chi2Final = m.currentChi;
      r->lambda = m.lambda;
      if (!lastAccepted) br->endedOnRejected++;
    }
    const int bad = ORBX_S3O_UNIFORM(ops.classify());
    r->rounds = it + 1;
    if (it == 0) {  // (constant indices: the record stays in registers on the device)
      r->iterations[0] = iterations;
      r->stopReason[0] = stop;
      r->nBad = bad;
      if (nCorrespondences - bad < 10) break;  // `if (nCorrespondences - nBad < 10) return 0`
    } else {
      r->iterations[1] = iterations;
      r->stopReason[1] = stop;
      r->nInliers = (nCorrespondences - r->nBad) - bad;
      recovered = true;
    }
  }
  r->lmTrials = m.lmTrials;
  r->rejected = m.rejected;
  r->solverFailures = m.solverFailures;
  *S = cur;
  return recovered;
}

}  // namespace orbx_sim3opt
