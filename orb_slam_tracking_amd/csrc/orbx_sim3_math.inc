// orbx_sim3_math.inc — Sim3Solver (include/orbx.h, "loop closing: Sim3 RANSAC"): the constructor's arithmetic, Horn's closed-form
// similarity from three 3D-3D correspondences, CheckInliers and the resolution of iterate() as plain operations.  Shared by
// orbx_sim3_kernel.hip (device) and tests/cpp/sim3_ref.cpp (the CPU restatement, g++ -ffp-contract=off): one source, so both
// sides take the same operations in the same order and agree bit for bit.  The sampler is orbx_pnp_math.inc's, on three draws.
// Every loop has constant bounds and every array is indexed with constants once the loops are unrolled, so that on the device
// nothing lives in memory.  [from-knowledge] restatements of ORB-SLAM2's Sim3Solver.cc, PARITY UNPINNED.
#ifndef ORBX_SIM3_FN
#define ORBX_SIM3_FN
#endif
#ifndef ORBX_PNP_FN
#define ORBX_PNP_FN ORBX_SIM3_FN
#endif
#include "orbx_pnp_math.inc"

#define ORBX_SIM3_INL ORBX_SIM3_FN inline __attribute__((always_inline))

namespace orbx_sim3 {

using orbx_pnp::finite32;
using orbx_pnp::finite64;

constexpr int SIM3_SWEEPS = 12;  // of the 4x4 Jacobi: fixed, no convergence test
// ORBX_SIM3_* of include/orbx.h
constexpr int SIM3_BAD_INPUT = 2, SIM3_NONFINITE = 4, SIM3_FEW_POINTS = 8, SIM3_BAD_DRAWS = 16, SIM3_NO_RESULT = 32;
// a hypothesis' flags
constexpr int HYP_DEGENERATE = 1, HYP_BAD_DRAWS = 2;

struct Cam {
  float fx, fy, cx, cy;
};
// one correspondence as the constructor takes it: mvX3Dc1, mvX3Dc2, mvP1im1, mvP2im2, mvnMaxError1 / 2, mvnIndices1 and the
// feature of KF2
struct Corr {
  float X1[3], X2[3], p1[2], p2[2], maxErr1, maxErr2;
  int32_t i1, i2;
};
// what a hypothesis leaves behind: R12 row-major, t12, s12 (d_sim3's layout), rounded to f32
struct Hyp {
  float sim[13];
  int32_t count, flags, pad;
};
// T12 = [s12 R12 | t12] and T21 = [(1 / s12) R12^T | -(1 / s12) R12^T t12] as CheckInliers multiplies with them (f32)
struct Sim3Pair {
  float sR12[9], t12[3], sR21[9], t21[3];
};

// Rcw * X + tcw in f32, products and sums left to right (pose: R row-major, then t)
ORBX_SIM3_INL void toCamera(const float* pose, const float* X, float* out) {
ORBX_PNP_UNROLL
  for (int r = 0; r < 3; r++) out[r] = pose[3 * r] * X[0] + pose[3 * r + 1] * X[1] + pose[3 * r + 2] * X[2] + pose[9 + r];
}
// FromCameraToImage / Project: no sign test on z
ORBX_SIM3_INL void toImage(const float* P, const Cam& K, float* uv) {
  const float invz = 1.0f / P[2];
  const float x = P[0] * invz, y = P[1] * invz;
  uv[0] = K.fx * x + K.cx;
  uv[1] = K.fy * y + K.cy;
}

// ---- the symmetric 4x4 eigenproblem of Horn's N ----------------------------------------------------------------------------------
// one two-sided Jacobi rotation in the plane (P, Q) of the symmetric A (full storage, both triangles kept) and of the vectors V
template <int P, int Q>
ORBX_SIM3_INL void rotate4(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double app = A[P][P], aqq = A[Q][Q];
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  A[P][P] = app - t * apq;
  A[Q][Q] = aqq + t * apq;
  A[P][Q] = A[Q][P] = 0.0;
ORBX_PNP_UNROLL
  for (int k = 0; k < 4; k++) {
    if (k == P || k == Q) continue;
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = A[P][k] = c * akp - s * akq;
    A[k][Q] = A[Q][k] = s * akp + c * akq;
  }
ORBX_PNP_UNROLL
  for (int r = 0; r < 4; r++) {
    const double vp = V[r][P], vq = V[r][Q];
    V[r][P] = c * vp - s * vq;
    V[r][Q] = s * vp + c * vq;
  }
}

// The eigenvector of the largest SIGNED eigenvalue of the symmetric 4x4 A (of equal values the lowest column): cyclic Jacobi,
// SIM3_SWEEPS sweeps over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  Returns the eigenvalue.
ORBX_SIM3_INL double eigTop4(double (&A)[4][4], double* q) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
ORBX_PNP_NOUNROLL
  for (int sweep = 0; sweep < SIM3_SWEEPS; sweep++) {
    rotate4<0, 1>(A, V);
    rotate4<0, 2>(A, V);
    rotate4<0, 3>(A, V);
    rotate4<1, 2>(A, V);
    rotate4<1, 3>(A, V);
    rotate4<2, 3>(A, V);
  }
  double top = A[0][0];
ORBX_PNP_UNROLL
  for (int r = 0; r < 4; r++) q[r] = V[r][0];
ORBX_PNP_UNROLL
  for (int c = 1; c < 4; c++) {
    const bool larger = A[c][c] > top;
    top = larger ? A[c][c] : top;
ORBX_PNP_UNROLL
    for (int r = 0; r < 4; r++) q[r] = larger ? V[r][c] : q[r];
  }
  return top;
}

// ---- ComputeSim3 (Horn 1987) over three correspondences, f64 from the f32 camera-frame points -----------------------------------
// P1[k] / P2[k]: point k of the triple in camera 1 / camera 2.  R row-major, t, *s.  (A degenerate triple gives non-finite values.)
ORBX_SIM3_INL void hornSim3(const double (&P1)[3][3], const double (&P2)[3][3], bool fixScale, double* R, double* t, double* s) {
  double O1[3], O2[3], Pr1[3][3], Pr2[3][3];  // Pr[k][i]: coordinate i of point k relative to the centroid
ORBX_PNP_UNROLL
  for (int i = 0; i < 3; i++) {
    // (relative to the first point: three coincident points give Pr = 0 exactly, which (p + p + p) / 3.0 does not)
    O1[i] = P1[0][i] + ((P1[1][i] - P1[0][i]) + (P1[2][i] - P1[0][i])) / 3.0;
    O2[i] = P2[0][i] + ((P2[1][i] - P2[0][i]) + (P2[2][i] - P2[0][i])) / 3.0;
  }
ORBX_PNP_UNROLL
  for (int k = 0; k < 3; k++)
ORBX_PNP_UNROLL
    for (int i = 0; i < 3; i++) {
      Pr1[k][i] = P1[k][i] - O1[i];
      Pr2[k][i] = P2[k][i] - O2[i];
    }
  // M = Pr2 * Pr1^T: M[i][j] = sum over the points k = 0, 1, 2 of Pr2[k][i] * Pr1[k][j]
  double M[3][3];
ORBX_PNP_UNROLL
  for (int i = 0; i < 3; i++)
ORBX_PNP_UNROLL
    for (int j = 0; j < 3; j++) M[i][j] = Pr2[0][i] * Pr1[0][j] + Pr2[1][i] * Pr1[1][j] + Pr2[2][i] * Pr1[2][j];
  double N[4][4];
  N[0][0] = M[0][0] + M[1][1] + M[2][2];
  N[0][1] = N[1][0] = M[1][2] - M[2][1];
  N[0][2] = N[2][0] = M[2][0] - M[0][2];
  N[0][3] = N[3][0] = M[0][1] - M[1][0];
  N[1][1] = M[0][0] - M[1][1] - M[2][2];
  N[1][2] = N[2][1] = M[0][1] + M[1][0];
  N[1][3] = N[3][1] = M[2][0] + M[0][2];
  N[2][2] = -M[0][0] + M[1][1] - M[2][2];
  N[2][3] = N[3][2] = M[1][2] + M[2][1];
  N[3][3] = -M[0][0] - M[1][1] + M[2][2];
  double q[4];
  (void)eigTop4(N, q);
  // the unit quaternion (w, x, y, z) -> R12, directly
  const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
  if (fixScale) {
    *s = 1.0;
  } else {
    // P3 = R12 * Pr2; nom = Pr1 . P3 and den = sum of P3 .* P3, both over the coordinates i (outer) and the points k (inner)
    double nom = 0.0, den = 0.0;
ORBX_PNP_UNROLL
    for (int i = 0; i < 3; i++)
ORBX_PNP_UNROLL
      for (int k = 0; k < 3; k++) {
        const double p3 = R[3 * i] * Pr2[k][0] + R[3 * i + 1] * Pr2[k][1] + R[3 * i + 2] * Pr2[k][2];
        nom = nom + Pr1[k][i] * p3;
        den = den + p3 * p3;
      }
    *s = nom / den;
  }
ORBX_PNP_UNROLL
  for (int i = 0; i < 3; i++) t[i] = O1[i] - *s * (R[3 * i] * O2[0] + R[3 * i + 1] * O2[1] + R[3 * i + 2] * O2[2]);
}

// the matrices of CheckInliers from the f32 similarity (R12 row-major, t12, s12); false when any entry of either is non-finite
ORBX_SIM3_INL bool pairOf(const float* sim, Sim3Pair* T) {
  const float s = sim[12];
  const double inv = 1.0 / (double)s;
  bool f = finite32(s);
ORBX_PNP_UNROLL
  for (int i = 0; i < 3; i++)
ORBX_PNP_UNROLL
    for (int j = 0; j < 3; j++) {
      T->sR12[3 * i + j] = s * sim[3 * i + j];
      T->sR21[3 * i + j] = (float)(inv * (double)sim[3 * j + i]);
    }
ORBX_PNP_UNROLL
  for (int i = 0; i < 3; i++) {
    T->t12[i] = sim[9 + i];
    T->t21[i] = -(T->sR21[3 * i] * sim[9] + T->sR21[3 * i + 1] * sim[10] + T->sR21[3 * i + 2] * sim[11]);
  }
ORBX_PNP_UNROLL
  for (int k = 0; k < 9; k++) f = f && finite32(sim[k]) && finite32(T->sR12[k]) && finite32(T->sR21[k]);
ORBX_PNP_UNROLL
  for (int k = 0; k < 3; k++) f = f && finite32(T->t12[k]) && finite32(T->t21[k]);
  return f;
}

// ---- CheckInliers, one correspondence: f32 ---------------------------------------------------------------------------------------
ORBX_SIM3_INL bool isInlier(const Sim3Pair& T, const Corr& c, const Cam& K) {
  float P[3], uv[2];
ORBX_PNP_UNROLL
  for (int r = 0; r < 3; r++) P[r] = T.sR12[3 * r] * c.X2[0] + T.sR12[3 * r + 1] * c.X2[1] + T.sR12[3 * r + 2] * c.X2[2] + T.t12[r];
  toImage(P, K, uv);  // vP2im1
  const float d1x = c.p1[0] - uv[0], d1y = c.p1[1] - uv[1];
  const float err1 = d1x * d1x + d1y * d1y;
ORBX_PNP_UNROLL
  for (int r = 0; r < 3; r++) P[r] = T.sR21[3 * r] * c.X1[0] + T.sR21[3 * r + 1] * c.X1[1] + T.sR21[3 * r + 2] * c.X1[2] + T.t21[r];
  toImage(P, K, uv);  // vP1im2
  const float d2x = uv[0] - c.p2[0], d2y = uv[1] - c.p2[1];
  const float err2 = d2x * d2x + d2y * d2y;
  return err1 < c.maxErr1 && err2 < c.maxErr2;
}

// ---- one hypothesis: the three draws, Horn, the rounding to f32; the caller counts its inliers -----------------------------------
// Returns true when the hypothesis is finite; h->flags says why not.  corr: the problem's N >= 3 correspondences.
ORBX_SIM3_INL bool hypothesis(const int32_t* draws, const Corr* corr, int N, bool fixScale, Hyp* h, Sim3Pair* T) {
  int sel[3];
ORBX_PNP_UNROLL
  for (int k = 0; k < 13; k++) h->sim[k] = 0.f;
  h->count = 0; h->flags = 0; h->pad = 0;
  if (!orbx_pnp::sampleDraws<3>(draws, N, sel)) {
    h->flags = HYP_BAD_DRAWS;
    return false;
  }
  double P1[3][3], P2[3][3], R[9], t[3], s;
ORBX_PNP_UNROLL
  for (int k = 0; k < 3; k++)
ORBX_PNP_UNROLL
    for (int i = 0; i < 3; i++) {
      P1[k][i] = (double)corr[sel[k]].X1[i];
      P2[k][i] = (double)corr[sel[k]].X2[i];
    }
  hornSim3(P1, P2, fixScale, R, t, &s);
  float sim[13];
ORBX_PNP_UNROLL
  for (int k = 0; k < 9; k++) sim[k] = (float)R[k];
ORBX_PNP_UNROLL
  for (int k = 0; k < 3; k++) sim[9 + k] = (float)t[k];
  sim[12] = (float)s;
  if (!pairOf(sim, T)) {
    h->flags = HYP_DEGENERATE;
    return false;
  }
ORBX_PNP_UNROLL
  for (int k = 0; k < 13; k++) h->sim[k] = sim[k];
  return true;
}

// ---- iterate(), resolved after the fact -----------------------------------------------------------------------------------------
// what a problem's prep leaves: N, mRansacMaxIts, the status bits of its device data
struct Meta {
  int32_t N, maxIts, status, pad;
};
struct Outcome {
  int itsRun, foundIt, bestIt, nBestInliers, nDegenerate, badDraws;
};

// The hypotheses' counts in iteration order; nIts = min(n_iter, mRansacMaxIts).  A hypothesis becomes the best under >= (the last
// of equals), one that does so with more than minInliers ends the solver.  Non-finite hypotheses and bad draws are never kept.
ORBX_SIM3_INL void resolveIterations(const Hyp* hyp, int nIts, int minInliers, Outcome* o) {
  int best = -1, bestCount = 0;
  o->itsRun = nIts; o->foundIt = -1; o->nDegenerate = 0; o->badDraws = 0;
  for (int it = 0; it < nIts; it++) {
    const int c = hyp[it].count, fl = hyp[it].flags;
    o->nDegenerate += (fl & HYP_DEGENERATE) ? 1 : 0;
    o->badDraws |= (fl & HYP_BAD_DRAWS) ? 1 : 0;
    if (fl != 0 || c < bestCount) continue;
    best = it;
    bestCount = c;
    if (c > minInliers) {
      o->foundIt = it;
      o->itsRun = it + 1;
      break;
    }
  }
  o->bestIt = best;
  o->nBestInliers = bestCount;
}

}  // namespace orbx_sim3
