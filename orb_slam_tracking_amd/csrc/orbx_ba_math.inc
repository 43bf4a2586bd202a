// orbx_ba_math.inc — the arithmetic of the two-view bundle adjustment (include/orbx.h, "behind the Initializer: two-view bundle
// adjustment") as plain f64 operations, shared by orbx_ba_kernel.hip (device) and tests/cpp/ba_ref.cpp (the CPU restatement,
// g++ -ffp-contract=off): one source, so both sides take the same operations in the same order and agree bit for bit.  What is
// NOT shared is how the points are spread over lanes and how the lanes' sums are combined; include/orbx.h fixes that order and
// each side implements it on its own.  Correctness is tested against an independent numpy statement and against ground truth
// (tests/test_ba_host.py), not against the other side.  [from-knowledge] restatements of g2o / Eigen, PARITY UNPINNED.
// Only +, -, *, /, sqrt and comparisons on doubles are used: no libm call, nothing the compiler may contract.
#ifndef ORBX_BA_FN
#define ORBX_BA_FN
#endif

namespace orbx_ba {

// sums a lane keeps while it walks its points (BA_ACC_* index the lane's accumulator array)
enum {
  BA_ACC_HPP = 0,     // 21: upper triangle of Hpp, row by row
  BA_ACC_BP = 21,     // 6
  BA_ACC_CHI2 = 27,   // activeRobustChi2
  BA_ACC_BUILD = 28,  // size of the build pass's array
  BA_ACC_S = 0,       // 21: upper triangle of sum Hpl Dinv Hpl^T
  BA_ACC_COEF = 21,   // 6: sum Hpl Dinv bl
  BA_ACC_SCHUR = 27,
  BA_ACC_TCHI2 = 0,   // the trial's chi2
  BA_ACC_SCALE = 1,   // the points' part of computeScale
  BA_ACC_TRIAL = 2,
  BA_ACC_MAX = 28
};

struct Cam {
  double fx, fy, cx, cy;
};
struct Pose {
  double q[4];  // x y z w (Eigen's coeffs())
  double t[3];
};
struct Counters {
  int accepted, rejected, huberOutliers, smallTheta;
};

ORBX_BA_FN inline bool isFinite(double v) { return v - v == 0.0; }
ORBX_BA_FN inline bool isFiniteF(float v) { return v - v == 0.0f; }
ORBX_BA_FN inline double notANumber() { return __builtin_nan(""); }

// ---- sin and cos of an angle in [0, 2^19): Cody-Waite reduction by pi/2 in two parts (33 + 53 bits; k < 2^20, so k * pio2Hi is
// exact), then the minimax polynomials of the freely distributable fdlibm (k_sin.c, k_cos.c) on [-pi/4, pi/4] with the reduction's
// tail.  Outside the domain (or NaN) both are NaN.
ORBX_BA_FN inline void sinCos(double x, double* s, double* c) {
  if (!(x >= 0.0 && x < 524288.0)) {
    *s = *c = notANumber();
    return;
  }
  const double invPio2 = 6.36619772367581382433e-01, pio2Hi = 1.57079632673412561417e+00, pio2Lo = 6.07710050650619224932e-11;
  const long long k = (long long)(x * invPio2 + 0.5);
  const double fn = (double)k;
  const double r = x - fn * pio2Hi, w = fn * pio2Lo;
  const double y0 = r - w, y1 = (r - y0) - w;
  const double z = y0 * y0;
  // sin(y0 + y1)
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double v = z * y0;
  const double rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
  const double sn = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * S1);
  // cos(y0 + y1)
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double zz = z * z;
  const double rc = z * (C1 + z * (C2 + z * C3)) + (zz * zz) * (C4 + z * (C5 + z * C6));
  const double hz = 0.5 * z, w2 = 1.0 - hz;
  const double cs = w2 + (((1.0 - w2) - hz) + (z * rc - y0 * y1));
  switch ((int)(k & 3)) {
    case 0: *s = sn; *c = cs; break;
    case 1: *s = cs; *c = -sn; break;
    case 2: *s = -sn; *c = -cs; break;
    default: *s = -cs; *c = sn; break;
  }
}

// ---- Eigen's Quaterniond and g2o's SE3Quat ------------------------------------------------------------
// Quaterniond(Matrix3d): the four-branch rule of Eigen's quaternionbase_assign_impl<Other, 3, 3>
ORBX_BA_FN inline void quatFromMatrix(const double m[3][3], double q[4]) {
  double t = (m[0][0] + m[1][1]) + m[2][2];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[2][1] - m[1][2]) * t;
    q[1] = (m[0][2] - m[2][0]) * t;
    q[2] = (m[1][0] - m[0][1]) * t;
  } else if (m[0][0] >= m[1][1] && m[0][0] >= m[2][2]) {  // i = 0 (i moves on only for a strictly larger diagonal entry)
    t = sqrt(((m[0][0] - m[1][1]) - m[2][2]) + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[2][1] - m[1][2]) * t;
    q[1] = (m[1][0] + m[0][1]) * t;
    q[2] = (m[2][0] + m[0][2]) * t;
  } else if (m[1][1] > m[0][0] && m[1][1] >= m[2][2]) {  // i = 1
    t = sqrt(((m[1][1] - m[2][2]) - m[0][0]) + 1.0);
    q[1] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[0][2] - m[2][0]) * t;
    q[2] = (m[2][1] + m[1][2]) * t;
    q[0] = (m[0][1] + m[1][0]) * t;
  } else {  // i = 2
    t = sqrt(((m[2][2] - m[0][0]) - m[1][1]) + 1.0);
    q[2] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[1][0] - m[0][1]) * t;
    q[0] = (m[0][2] + m[2][0]) * t;
    q[1] = (m[1][2] + m[2][1]) * t;
  }
}

// SE3Quat::normalizeRotation (se3quat.h:280-285)
ORBX_BA_FN inline void normalizeRotation(double q[4]) {
  if (q[3] < 0.0)
    for (int i = 0; i < 4; i++) q[i] = -q[i];
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] = q[i] / n;
}

// Quaterniond::toRotationMatrix
ORBX_BA_FN inline void quatToMatrix(const double q[4], double R[3][3]) {
  const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0][0] = 1.0 - (tyy + tzz); R[0][1] = txy - twz;         R[0][2] = txz + twy;
  R[1][0] = txy + twz;         R[1][1] = 1.0 - (txx + tzz); R[1][2] = tyz - twx;
  R[2][0] = txz - twy;         R[2][1] = tyz + twx;         R[2][2] = 1.0 - (txx + tyy);
}

// Quaterniond * Vector3d (QuaternionBase::_transformVector)
ORBX_BA_FN inline void quatRotate(const double q[4], const double v[3], double out[3]) {
  double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
  for (int i = 0; i < 3; i++) uv[i] = uv[i] + uv[i];
  const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int i = 0; i < 3; i++) out[i] = (v[i] + q[3] * uv[i]) + c[i];
}

// SE3Quat::map (se3quat.h:217-220)
ORBX_BA_FN inline void poseMap(const Pose& T, const double X[3], double out[3]) {
  double r[3];
  quatRotate(T.q, X, r);
  for (int i = 0; i < 3; i++) out[i] = r[i] + T.t[i];
}

// SE3Quat(R, t) (se3quat.h:58-60) from the Initializer's f32 (R21, t21)
ORBX_BA_FN inline void poseFromRt(const float* R21, const float* t21, Pose* T) {
  double m[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) m[i][j] = (double)R21[i * 3 + j];
  quatFromMatrix(m, T->q);
  normalizeRotation(T->q);
  for (int i = 0; i < 3; i++) T->t[i] = (double)t21[i];
}

// VertexSE3Expmap::oplusImpl: SE3Quat::exp(update) * estimate (se3quat.h:223-257, :104-110); update = (omega, upsilon).
// pow(theta, 3) is theta * theta * theta here.  Returns whether the theta < 1e-5 branch ran.
ORBX_BA_FN inline bool poseOplus(const double u[6], Pose* T) {
  const double om[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
  const double theta = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
  const double O[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
  double O2[3][3], R[3][3], V[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) O2[i][j] = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j];
  const bool small = theta < 0.00001;
  if (small) {
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) V[i][j] = R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
  } else {
    double s, c;
    sinCos(theta, &s, &c);
    const double a = s / theta, b = (1.0 - c) / (theta * theta), d = (theta - s) / ((theta * theta) * theta);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const double I = i == j ? 1.0 : 0.0;
        R[i][j] = (I + a * O[i][j]) + b * O2[i][j];
        V[i][j] = (I + b * O[i][j]) + d * O2[i][j];
      }
  }
  Pose E;
  quatFromMatrix(R, E.q);
  normalizeRotation(E.q);
  for (int i = 0; i < 3; i++) E.t[i] = (V[i][0] * up[0] + V[i][1] * up[1]) + V[i][2] * up[2];
  // E * T
  double rt[3];
  quatRotate(E.q, T->t, rt);
  const double* a = E.q;
  const double b[4] = {T->q[0], T->q[1], T->q[2], T->q[3]};
  T->q[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
  T->q[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
  T->q[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
  T->q[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
  for (int i = 0; i < 3; i++) T->t[i] = E.t[i] + rt[i];
  normalizeRotation(T->q);
  return small;
}

// ---- one EdgeSE3ProjectXYZ ------------------------------------------------------------------------------
// computeError (types_six_dof_expmap.h: obs - cam_project(map(X))) for a point `pc` already in the camera's frame, chi2() =
// e . (information e) with information = w I, and RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1]
ORBX_BA_FN inline void edgeError(const double pc[3], double u, double v, double w, const Cam& K, double delta, double e[2],
                                 double rho[2]) {
  e[0] = u - ((pc[0] / pc[2]) * K.fx + K.cx);
  e[1] = v - ((pc[1] / pc[2]) * K.fy + K.cy);
  const double chi2 = e[0] * (w * e[0]) + e[1] * (w * e[1]);
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

// the robust chi2 of a point's two edges added to *chi2, edge of frame 1 first (frame 1 is the fixed identity: map(X) = X)
ORBX_BA_FN inline void pointChi2(const Pose& T, const double X[3], const float obs[6], const Cam& K, double delta, double* chi2) {
  double e[2], rho[2], pc[3];
  edgeError(X, (double)obs[0], (double)obs[1], (double)obs[4], K, delta, e, rho);
  *chi2 = *chi2 + rho[0];
  poseMap(T, X, pc);
  edgeError(pc, (double)obs[2], (double)obs[3], (double)obs[5], K, delta, e, rho);
  *chi2 = *chi2 + rho[0];
}

// linearizeOplus (types_six_dof_expmap.cpp:98-134): A = d e / d point (2x3), B = d e / d pose (2x6), R = T's rotation matrix
ORBX_BA_FN inline void edgeJacobians(const double pc[3], const double R[3][3], bool identity, const Cam& K, double A[2][3],
                                     double B[2][6]) {
  const double x = pc[0], y = pc[1], z = pc[2], z_2 = z * z;
  const double tmp[2][3] = {{K.fx, 0.0, -x / z * K.fx}, {0.0, K.fy, -y / z * K.fy}};
  const double s = -1.0 / z;
  for (int r = 0; r < 2; r++)
    for (int c = 0; c < 3; c++) {
      if (identity)
        A[r][c] = s * tmp[r][c];
      else
        A[r][c] = ((s * tmp[r][0]) * R[0][c] + (s * tmp[r][1]) * R[1][c]) + (s * tmp[r][2]) * R[2][c];
    }
  B[0][0] = x * y / z_2 * K.fx;
  B[0][1] = -(1.0 + (x * x / z_2)) * K.fx;
  B[0][2] = y / z * K.fx;
  B[0][3] = -1.0 / z * K.fx;
  B[0][4] = 0.0;
  B[0][5] = x / z_2 * K.fx;
  B[1][0] = (1.0 + y * y / z_2) * K.fy;
  B[1][1] = -x * y / z_2 * K.fy;
  B[1][2] = -x / z * K.fy;
  B[1][3] = 0.0;
  B[1][4] = -1.0 / z * K.fy;
  B[1][5] = y / z_2 * K.fy;
}

// One point's part of buildSystem: errors, robust chi2 (acc[BA_ACC_CHI2]), linearizeOplus and constructQuadraticForm's robust
// branch (base_binary_edge.hpp:91-113) for its two edges.  Hll (upper triangle, 6), bl (3), Hpl (6 x 3) are the point's own
// blocks; Hpp and bp are added into the lane's sums.  Returns the number of the point's edges in Huber's outlier branch.
ORBX_BA_FN inline int pointBuild(const Pose& T, const double R[3][3], const double X[3], const float obs[6], const Cam& K,
                                 double delta, double Hll[6], double bl[3], double Hpl[18], double* acc) {
  double e1[2], e2[2], rho1[2], rho2[2], pc[3], A1[2][3], A2[2][3], B[2][6];
  const double w1 = (double)obs[4], w2 = (double)obs[5];
  edgeError(X, (double)obs[0], (double)obs[1], w1, K, delta, e1, rho1);
  acc[BA_ACC_CHI2] = acc[BA_ACC_CHI2] + rho1[0];
  poseMap(T, X, pc);
  edgeError(pc, (double)obs[2], (double)obs[3], w2, K, delta, e2, rho2);
  acc[BA_ACC_CHI2] = acc[BA_ACC_CHI2] + rho2[0];
  edgeJacobians(X, R, true, K, A1, B);  // (B of the fixed frame is not used)
  edgeJacobians(pc, R, false, K, A2, B);
  // omega_r = -(omega e) * rho[1]; weightedOmega = rho[1] * omega
  const double r1[2] = {-(w1 * e1[0]) * rho1[1], -(w1 * e1[1]) * rho1[1]};
  const double r2[2] = {-(w2 * e2[0]) * rho2[1], -(w2 * e2[1]) * rho2[1]};
  const double o1 = rho1[1] * w1, o2 = rho2[1] * w2;
  int k = 0;
  for (int r = 0; r < 3; r++) {
    for (int c = r; c < 3; c++, k++)
      Hll[k] = (A1[0][r] * (o1 * A1[0][c]) + A1[1][r] * (o1 * A1[1][c])) + (A2[0][r] * (o2 * A2[0][c]) + A2[1][r] * (o2 * A2[1][c]));
    bl[r] = (A1[0][r] * r1[0] + A1[1][r] * r1[1]) + (A2[0][r] * r2[0] + A2[1][r] * r2[1]);
  }
  k = 0;
  for (int p = 0; p < 6; p++) {
    for (int l = 0; l < 3; l++) Hpl[p * 3 + l] = B[0][p] * (o2 * A2[0][l]) + B[1][p] * (o2 * A2[1][l]);
    for (int q = p; q < 6; q++, k++)
      acc[BA_ACC_HPP + k] = acc[BA_ACC_HPP + k] + (B[0][p] * (o2 * B[0][q]) + B[1][p] * (o2 * B[1][q]));
    acc[BA_ACC_BP + p] = acc[BA_ACC_BP + p] + (B[0][p] * r2[0] + B[1][p] * r2[1]);
  }
  return (rho1[1] != 1.0 ? 1 : 0) + (rho2[1] != 1.0 ? 1 : 0);
}

// (Hll + lambda I)^-1 by cofactors and one reciprocal of the determinant (upper triangle in, symmetric 3x3 out)
ORBX_BA_FN inline void pointDinv(const double Hll[6], double lambda, double Di[3][3]) {
  const double d00 = Hll[0] + lambda, d01 = Hll[1], d02 = Hll[2], d11 = Hll[3] + lambda, d12 = Hll[4], d22 = Hll[5] + lambda;
  const double c00 = d11 * d22 - d12 * d12, c01 = d02 * d12 - d01 * d22, c02 = d01 * d12 - d02 * d11;
  const double det = (d00 * c00 + d01 * c01) + d02 * c02;
  const double id = 1.0 / det;
  Di[0][0] = c00 * id;
  Di[0][1] = Di[1][0] = c01 * id;
  Di[0][2] = Di[2][0] = c02 * id;
  Di[1][1] = (d00 * d22 - d02 * d02) * id;
  Di[1][2] = Di[2][1] = (d01 * d02 - d00 * d12) * id;
  Di[2][2] = (d00 * d11 - d01 * d01) * id;
}

// One point's part of the Schur complement (block_solver.hpp:381-432): Hpl Dinv Hpl^T and Hpl Dinv bl into the lane's sums
ORBX_BA_FN inline void pointSchur(const double Hll[6], const double bl[3], const double Hpl[18], double lambda, double* acc) {
  double Di[3][3], db[3], BD[6][3];
  pointDinv(Hll, lambda, Di);
  for (int l = 0; l < 3; l++) db[l] = (Di[l][0] * bl[0] + Di[l][1] * bl[1]) + Di[l][2] * bl[2];
  for (int p = 0; p < 6; p++) {
    for (int l = 0; l < 3; l++) BD[p][l] = (Hpl[p * 3] * Di[0][l] + Hpl[p * 3 + 1] * Di[1][l]) + Hpl[p * 3 + 2] * Di[2][l];
    acc[BA_ACC_COEF + p] = acc[BA_ACC_COEF + p] + ((Hpl[p * 3] * db[0] + Hpl[p * 3 + 1] * db[1]) + Hpl[p * 3 + 2] * db[2]);
  }
  int k = 0;
  for (int p = 0; p < 6; p++)
    for (int q = p; q < 6; q++, k++)
      acc[BA_ACC_S + k] = acc[BA_ACC_S + k] + ((BD[p][0] * Hpl[q * 3] + BD[p][1] * Hpl[q * 3 + 1]) + BD[p][2] * Hpl[q * 3 + 2]);
}

// The point's step (block_solver.hpp:459-481): xl = Dinv (bl - Hpl^T xp), its part of computeScale
// (optimization_algorithm_levenberg.cpp:182-189) into acc[BA_ACC_SCALE], and oplus (X += xl)
ORBX_BA_FN inline void pointStep(const double Hll[6], const double bl[3], const double Hpl[18], double lambda, const double xp[6],
                                 double X[3], double xl[3], double* acc) {
  double Di[3][3], cl[3];
  pointDinv(Hll, lambda, Di);
  for (int l = 0; l < 3; l++) {
    cl[l] = bl[l];
    for (int p = 0; p < 6; p++) cl[l] = cl[l] + Hpl[p * 3 + l] * (-xp[p]);
  }
  for (int l = 0; l < 3; l++) {
    xl[l] = (Di[l][0] * cl[0] + Di[l][1] * cl[1]) + Di[l][2] * cl[2];
    acc[BA_ACC_SCALE] = acc[BA_ACC_SCALE] + xl[l] * (lambda * xl[l] + bl[l]);
    X[l] = X[l] + xl[l];
  }
}

// ---- the pose's 6x6 system and the Levenberg-Marquardt bookkeeping: run by one lane ----------------------------
struct Lm {
  double Hpp[21], bp[6];  // of the current linearisation (upper triangle)
  double lambda, ni, currentChi, iniChi, rho;
  double xp[6];
  int nBad, qmax, ok;
  int iterations, lmTrials, rejected, solverFailures, stopReason;
};

// Hschur = Hpp + lambda I - S, bschur = bp - coef, solved by an unblocked lower Cholesky (a pivot <= 0 or non-finite = failed:
// xp = 0 then).  Returns whether it solved.
ORBX_BA_FN inline bool lmSolvePose(Lm* m, const double* S, const double* coef) {
  double L[6][6], b[6];
  int k = 0;
  for (int p = 0; p < 6; p++) {
    for (int q = p; q < 6; q++, k++) {
      double h = m->Hpp[k];
      if (p == q) h = h + m->lambda;
      L[q][p] = h - S[k];  // lower triangle
    }
    b[p] = m->bp[p] - coef[p];
    m->xp[p] = 0.0;
  }
  for (int j = 0; j < 6; j++) {
    double d = L[j][j];
    for (int c = 0; c < j; c++) d = d - L[j][c] * L[j][c];
    if (!(d > 0.0) || !isFinite(d)) return false;
    const double ljj = sqrt(d);
    L[j][j] = ljj;
    for (int i = j + 1; i < 6; i++) {
      double v = L[i][j];
      for (int c = 0; c < j; c++) v = v - L[i][c] * L[j][c];
      L[i][j] = v / ljj;
    }
  }
  double y[6];
  for (int i = 0; i < 6; i++) {
    double v = b[i];
    for (int c = 0; c < i; c++) v = v - L[i][c] * y[c];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; i--) {
    double v = y[i];
    for (int c = i + 1; c < 6; c++) v = v - L[c][i] * m->xp[c];
    m->xp[i] = v / L[i][i];
  }
  for (int i = 0; i < 6; i++)
    if (!isFinite(m->xp[i])) {
      for (int c = 0; c < 6; c++) m->xp[c] = 0.0;
      return false;
    }
  return true;
}

// computeLambdaInit (optimization_algorithm_levenberg.cpp:166-180): tau = 1e-5 times the largest |diagonal entry|, `maxPoint`
// being the largest over the points' Hll
ORBX_BA_FN inline double lmLambdaInit(const double* Hpp, double maxPoint) {
  double mx = 0.0;
  int k = 0;
  for (int p = 0; p < 6; k += 6 - p, p++) {
    const double a = Hpp[k] < 0.0 ? -Hpp[k] : Hpp[k];
    if (a > mx) mx = a;
  }
  if (maxPoint > mx) mx = maxPoint;
  return 1e-5 * mx;
}

// One trial's verdict (optimization_algorithm_levenberg.cpp:123-149) from the trial's chi2 and the points' part of computeScale.
// Returns 1 = accepted, 0 = rejected (the caller restores the state); m->rho and m->qmax say whether another trial follows.
ORBX_BA_FN inline int lmJudge(Lm* m, double tempChi, double scalePoints, Counters* cnt) {
  if (!m->ok) tempChi = 1.7976931348623157e308;  // std::numeric_limits<double>::max()
  double rho = m->currentChi - tempChi;
  double scale = 0.0;
  for (int i = 0; i < 6; i++) scale = scale + m->xp[i] * (m->lambda * m->xp[i] + m->bp[i]);
  scale = scale + scalePoints;
  scale = scale + 1e-3;
  rho = rho / scale;
  int accepted;
  if (rho > 0.0 && isFinite(tempChi)) {
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
ORBX_BA_FN inline bool lmAnotherTrial(const Lm* m) { return m->rho < 0.0 && m->qmax < 10; }

// The end of solve() (:151-163): 0 = OK, 1 = Terminate by `qmax == 10 || rho == 0`, 2 = Terminate by `_nBad >= 3`
ORBX_BA_FN inline int lmEndIteration(Lm* m) {
  if (m->qmax == 10 || m->rho == 0.0) return 1;
  if ((m->iniChi - m->currentChi) * 1e3 < m->iniChi)
    m->nBad++;
  else
    m->nBad = 0;
  return m->nBad >= 3 ? 2 : 0;
}

}  // namespace orbx_ba
