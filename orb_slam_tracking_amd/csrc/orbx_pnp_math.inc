// orbx_pnp_math.inc — PnPsolver (include/orbx.h, "behind SearchByBoW: PnP RANSAC"): the sampler, EPnP's compute_pose, CheckInliers
// and the resolution of iterate() as plain operations, f64 unless the rules say f32.  Shared by orbx_pnp_kernel.hip (device) and
// tests/cpp/pnp_ref.cpp (the CPU restatement, g++ -ffp-contract=off): one source, so both sides take the same operations in the
// same order and agree bit for bit.  What is NOT shared is how a sum over the points of a set is taken: `Ops` below.  A
// hypothesis adds its four points one after the other (SeqOps, here); Refine's sets are spread over the 64 lanes of a wave in
// the order include/orbx.h fixes, and each side implements that on its own.  Every loop has constant bounds and every array is
// indexed with constants once the loops are unrolled, so that on the device nothing is addressed at run time but V (VStore).
// [from-knowledge] restatements of ORB-SLAM2's PnPsolver.cc / EPnP, PARITY UNPINNED.
#ifndef ORBX_PNP_FN
#define ORBX_PNP_FN
#endif
// (everything below is inlined into its kernel: an array handed to a call that is not would live in memory)
#define ORBX_PNP_INL ORBX_PNP_FN inline __attribute__((always_inline))
#ifndef ORBX_DECOMP_FN
#define ORBX_DECOMP_FN ORBX_PNP_FN
#endif
#if defined(__clang__)
#define ORBX_PNP_UNROLL _Pragma("unroll")
#define ORBX_PNP_NOUNROLL _Pragma("nounroll")
#else
#define ORBX_PNP_UNROLL
#define ORBX_PNP_NOUNROLL
#endif
#include <utility>

#include "orbx_init_decomp.inc"

namespace orbx_pnp {

constexpr int PNP_SWEEPS = 12;   // of every Jacobi: fixed, no convergence test
constexpr int PNP_GN_STEPS = 5;  // gauss_newton's `const int iterations_number = 5`
constexpr int PNP_RAND_MAX = 2147483647;
// ORBX_PNP_* of include/orbx.h
constexpr int PNP_BAD_INPUT = 2, PNP_NONFINITE = 4, PNP_FEW_POINTS = 8, PNP_BAD_DRAWS = 16, PNP_NO_POSE = 32;
// a hypothesis' flags
constexpr int HYP_DEGENERATE = 1, HYP_BAD_DRAWS = 2;

struct Cam {
  double fu, fv, uc, vc;
};
// one correspondence as the constructor takes it: mvP3Dw, mvP2D, mvMaxError (= mvSigma2 * th2, f32), mvKeyIndices and the
// point's entry in its set
struct Corr {
  float X[3], u, v, maxErr;
  int32_t j, i;
};
struct Pt {
  double X[3], u, v;
};
// what a hypothesis leaves behind
struct Hyp {
  double R[9], t[3];
  int32_t count, flags, choice, pad;
};

ORBX_PNP_INL Pt ptOf(const Corr& c) {
  Pt P;
  P.X[0] = (double)c.X[0]; P.X[1] = (double)c.X[1]; P.X[2] = (double)c.X[2];
  P.u = (double)c.u; P.v = (double)c.v;
  return P;
}
ORBX_PNP_INL bool finite64(double x) { return (x - x) == 0.0; }
ORBX_PNP_INL bool finite32(float x) { return (x - x) == 0.0f; }

// ---- sampling: DUtils::Random::RandomInt(0, size - 1) on the caller's rand() values, and vAvailableIndices' swap-and-pop --------
// K draws change at most K entries of the list 0 .. N-1, so the changes are remembered instead of the list.  N >= K.
// Returns false (and picks nothing) when a draw lies outside [0, RAND_MAX].  (K = 4 here; 3 for orbx_sim3_math.inc.)
template <int K>
ORBX_PNP_INL bool sampleDraws(const int32_t* draws, int N, int* sel) {
  int pos[K], val[K];
  bool ok = true;
ORBX_PNP_UNROLL
  for (int i = 0; i < K; i++) ok = ok && draws[i] >= 0;  // (an int32 cannot exceed RAND_MAX)
  if (!ok) return false;
ORBX_PNP_UNROLL
  for (int i = 0; i < K; i++) {
    const int size = N - i;
    const int randi = (int)(((double)draws[i] / ((double)PNP_RAND_MAX + 1.0)) * (double)size);
    int idx = randi, last = size - 1;
ORBX_PNP_UNROLL
    for (int k = 0; k < i; k++) {  // later changes override earlier ones
      idx = pos[k] == randi ? val[k] : idx;
      last = pos[k] == size - 1 ? val[k] : last;
    }
    sel[i] = idx;
    pos[i] = randi;
    val[i] = last;
  }
  return true;
}
ORBX_PNP_INL bool sampleFour(const int32_t* draws, int N, int* sel) { return sampleDraws<4>(draws, N, sel); }

// ---- CheckInliers, one point: the reference's mixed types -----------------------------------------------------------------------
ORBX_PNP_INL bool isInlier(const double* R, const double* t, const Corr& c, const Cam& K) {
  const double X = (double)c.X[0], Y = (double)c.X[1], Z = (double)c.X[2];
  const float Xc = (float)(R[0] * X + R[1] * Y + R[2] * Z + t[0]);
  const float Yc = (float)(R[3] * X + R[4] * Y + R[5] * Z + t[1]);
  const float invZc = (float)(1.0 / (R[6] * X + R[7] * Y + R[8] * Z + t[2]));
  const double ue = K.uc + K.fu * (double)Xc * (double)invZc;
  const double ve = K.vc + K.fv * (double)Yc * (double)invZc;
  const float distX = (float)((double)c.u - ue), distY = (float)((double)c.v - ve);
  const float error2 = distX * distX + distY * distY;
  return error2 < c.maxErr;
}
ORBX_PNP_INL bool poseFinite(const double* R, const double* t) {
  bool f = true;
ORBX_PNP_UNROLL
  for (int k = 0; k < 9; k++) f = f && finite64(R[k]);
ORBX_PNP_UNROLL
  for (int k = 0; k < 3; k++) f = f && finite64(t[k]);
  return f;
}

// ---- the 12x12 eigenproblem of M^T M ------------------------------------------------------------------------------------------
// packed upper triangle of a symmetric 12 x 12 matrix
constexpr int sidx12(int i, int j) { return i <= j ? i * 12 - i * (i - 1) / 2 + (j - i) : j * 12 - j * (j - 1) / 2 + (i - j); }

// where the eigenvector matrix lives: V[k][i] at base[(k * 12 + i) * stride] (the device: LDS, one double per lane and entry)
struct VStore {
  double* base;
  int stride;
  ORBX_PNP_FN double& at(int k, int i) const { return base[(k * 12 + i) * stride]; }
};

// One rotation of the cyclic Jacobi on the packed A for the pair (P, Q), P < Q, as a template so that every index is a constant:
// the rotation of Golub & Van Loan 8.4, as orbx_decomp::eig3.  A pair whose off-diagonal entry is exactly 0 is skipped.
template <int P, int Q>
ORBX_PNP_INL void rotate12(double* A, const VStore& V) {
  const double apq = A[sidx12(P, Q)];
  if (apq != 0.0) {
    const double app = A[sidx12(P, P)], aqq = A[sidx12(Q, Q)];
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[sidx12(P, P)] = app - t * apq;
    A[sidx12(Q, Q)] = aqq + t * apq;
    A[sidx12(P, Q)] = 0.0;
ORBX_PNP_UNROLL
    for (int k = 0; k < 12; k++) {
      if (k == P || k == Q) continue;
      const double akp = A[sidx12(k, P)], akq = A[sidx12(k, Q)];
      A[sidx12(k, P)] = c * akp - s * akq;
      A[sidx12(k, Q)] = s * akp + c * akq;
    }
ORBX_PNP_UNROLL
    for (int k = 0; k < 12; k++) {
      const double vkp = V.at(k, P), vkq = V.at(k, Q);
      V.at(k, P) = c * vkp - s * vkq;
      V.at(k, Q) = s * vkp + c * vkq;
    }
  }
}
// the pair with number E in row order: (0,1) (0,2) ... (0,11) (1,2) ... (10,11)
constexpr int pairP(int e) {
  int p = 0;
  while (e >= 11 - p) {
    e -= 11 - p;
    p++;
  }
  return p;
}
constexpr int pairQ(int e) {
  int p = 0;
  while (e >= 11 - p) {
    e -= 11 - p;
    p++;
  }
  return p + 1 + e;
}
template <int... E>
ORBX_PNP_INL void sweep12(double* A, const VStore& V, std::integer_sequence<int, E...>) {
  (rotate12<pairP(E), pairQ(E)>(A, V), ...);
}

// Cyclic Jacobi on the packed A (destroyed: its diagonal ends as the eigenvalues), PNP_SWEEPS sweeps over the 66 pairs (p, q),
// p < q, in row order.  V's columns end as the eigenvectors.
ORBX_PNP_INL void jacobi12(double* A, const VStore& V) {
ORBX_PNP_UNROLL
  for (int k = 0; k < 12; k++)
ORBX_PNP_UNROLL
    for (int i = 0; i < 12; i++) V.at(k, i) = i == k ? 1.0 : 0.0;
ORBX_PNP_NOUNROLL
  for (int sweep = 0; sweep < PNP_SWEEPS; sweep++) sweep12(A, V, std::make_integer_sequence<int, 66>());
}

// v[r] = row 11 - r of `ut`: the eigenvector of the (r + 1)-th smallest eigenvalue, the eigenvalues sorted descending and stable
// (of equal values the one of the lower column comes first).  A column's place is counted, not sorted for.
ORBX_PNP_INL void smallestFour(const double* A, const VStore& V, double v[4][12]) {
ORBX_PNP_UNROLL
  for (int r = 0; r < 4; r++)
ORBX_PNP_UNROLL
    for (int k = 0; k < 12; k++) v[r][k] = 0.0;
ORBX_PNP_UNROLL
  for (int i = 0; i < 12; i++) {
    const double di = A[sidx12(i, i)];
    int place = 0;
ORBX_PNP_UNROLL
    for (int j = 0; j < 12; j++) {
      if (j == i) continue;
      const double dj = A[sidx12(j, j)];
      place += (dj > di || (dj == di && j < i)) ? 1 : 0;
    }
ORBX_PNP_UNROLL
    for (int r = 0; r < 4; r++)
      if (place == 11 - r) {
ORBX_PNP_UNROLL
        for (int k = 0; k < 12; k++) v[r][k] = V.at(k, i);
      }
  }
}

// ---- least squares for six equations: Householder QR, then back substitution (find_betas_approx_*'s cvSolve(CV_SVD) and
// gauss_newton's qr_solve).  A and b are destroyed.  A column without a norm divides by zero: the result is not finite and
// the hypothesis is dropped by the caller's check.
template <int N>
ORBX_PNP_INL void lsq6(double A[6][N], double* b, double* x) {
  double diag[N];
ORBX_PNP_UNROLL
  for (int k = 0; k < N; k++) {
    double s = 0.0;
ORBX_PNP_UNROLL
    for (int i = k; i < 6; i++) s = s + A[i][k] * A[i][k];
    const double nrm = sqrt(s);
    const double akk = A[k][k];
    const double alpha = akk >= 0.0 ? -nrm : nrm;
    const double half = s - alpha * akk;  // v^T v / 2 with v = a_k - alpha e_k
    A[k][k] = akk - alpha;
ORBX_PNP_UNROLL
    for (int j = k + 1; j < N; j++) {
      double d = 0.0;
ORBX_PNP_UNROLL
      for (int i = k; i < 6; i++) d = d + A[i][k] * A[i][j];
      const double f = d / half;
ORBX_PNP_UNROLL
      for (int i = k; i < 6; i++) A[i][j] = A[i][j] - f * A[i][k];
    }
    double d = 0.0;
ORBX_PNP_UNROLL
    for (int i = k; i < 6; i++) d = d + A[i][k] * b[i];
    const double f = d / half;
ORBX_PNP_UNROLL
    for (int i = k; i < 6; i++) b[i] = b[i] - f * A[i][k];
    diag[k] = alpha;
  }
ORBX_PNP_UNROLL
  for (int k = N - 1; k >= 0; k--) {
    double s = b[k];
ORBX_PNP_UNROLL
    for (int j = k + 1; j < N; j++) s = s - A[k][j] * x[j];
    x[k] = s / diag[k];
  }
}

// ---- the sums of a hypothesis: four points, one after the other -----------------------------------------------------------------
struct SeqOps {
  Pt p[4];
  ORBX_PNP_FN int count() const { return 4; }
  ORBX_PNP_FN Pt first() const { return p[0]; }
  template <int K, class F>
  ORBX_PNP_FN __attribute__((always_inline)) void sum(double* out, F f) const {
ORBX_PNP_UNROLL
    for (int k = 0; k < K; k++) out[k] = 0.0;
ORBX_PNP_UNROLL
    for (int i = 0; i < 4; i++) f(p[i], out);
  }
};

// compute_barycentric_coordinates for one point
ORBX_PNP_INL void alphasOf(const double cws[4][3], const double* ci, const Pt& P, double* a) {
  const double d0 = P.X[0] - cws[0][0], d1 = P.X[1] - cws[0][1], d2 = P.X[2] - cws[0][2];
ORBX_PNP_UNROLL
  for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
  a[0] = 1.0 - a[1] - a[2] - a[3];
}

ORBX_PNP_INL double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
ORBX_PNP_INL double dist2(const double* a, const double* b) {
  return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// compute_R_and_t for one set of betas: compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error.
// The 3x3 SVD of ABt: eig3 of ABt^T ABt gives V and the squared singular values; u_i = ABt v_i / |ABt v_i| for the two largest,
// u_2 = +-(u_0 x u_1) with the sign that gives det(U V^T) the sign of det(ABt), as a full SVD with non-negative singular values
// has it.  Returns the mean reprojection error.
template <class Ops>
ORBX_PNP_INL double computeRt(const Ops& ops, const Cam& K, const double cws[4][3], const double* ci, const double v[4][12],
                                    const double* betas, double* R, double* t) {
  const double n = (double)ops.count();
  double ccs[4][3];
ORBX_PNP_UNROLL
  for (int j = 0; j < 4; j++)
ORBX_PNP_UNROLL
    for (int k = 0; k < 3; k++) ccs[j][k] = 0.0;
ORBX_PNP_UNROLL
  for (int i = 0; i < 4; i++)
ORBX_PNP_UNROLL
    for (int j = 0; j < 4; j++)
ORBX_PNP_UNROLL
      for (int k = 0; k < 3; k++) ccs[j][k] = ccs[j][k] + betas[i] * v[i][3 * j + k];
  // solve_for_sign: the first point's depth
  {
    double a[4];
    alphasOf(cws, ci, ops.first(), a);
    const double z = a[0] * ccs[0][2] + a[1] * ccs[1][2] + a[2] * ccs[2][2] + a[3] * ccs[3][2];
    if (z < 0.0) {
ORBX_PNP_UNROLL
      for (int j = 0; j < 4; j++)
ORBX_PNP_UNROLL
        for (int k = 0; k < 3; k++) ccs[j][k] = -ccs[j][k];
    }
  }
  auto pcOf = [&](const Pt& P, double* pc) {
    double a[4];
    alphasOf(cws, ci, P, a);
ORBX_PNP_UNROLL
    for (int k = 0; k < 3; k++) pc[k] = a[0] * ccs[0][k] + a[1] * ccs[1][k] + a[2] * ccs[2][k] + a[3] * ccs[3][k];
  };
  double pc0[3];
  ops.template sum<3>(pc0, [&](const Pt& P, double* acc) {
    double pc[3];
    pcOf(P, pc);
ORBX_PNP_UNROLL
    for (int k = 0; k < 3; k++) acc[k] = acc[k] + pc[k];
  });
ORBX_PNP_UNROLL
  for (int k = 0; k < 3; k++) pc0[k] = pc0[k] / n;
  const double* pw0 = cws[0];  // (the centroid of the points: the same sum and the same division)
  double abt[9];
  ops.template sum<9>(abt, [&](const Pt& P, double* acc) {
    double pc[3];
    pcOf(P, pc);
ORBX_PNP_UNROLL
    for (int j = 0; j < 3; j++)
ORBX_PNP_UNROLL
      for (int k = 0; k < 3; k++) acc[3 * j + k] = acc[3 * j + k] + (pc[j] - pc0[j]) * (P.X[k] - pw0[k]);
  });
  double G[6], Vv[3][3], w[3], U[9];
  orbx_decomp::gram3(abt, G);
  orbx_decomp::eig3(G, Vv, w);
ORBX_PNP_UNROLL
  for (int c = 0; c < 2; c++) {
    double u[3];
ORBX_PNP_UNROLL
    for (int r = 0; r < 3; r++) u[r] = abt[r * 3] * Vv[0][c] + abt[r * 3 + 1] * Vv[1][c] + abt[r * 3 + 2] * Vv[2][c];
    const double nn = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
ORBX_PNP_UNROLL
    for (int r = 0; r < 3; r++) U[r * 3 + c] = u[r] / nn;
  }
  double Vt[9];
ORBX_PNP_UNROLL
  for (int i = 0; i < 3; i++)
ORBX_PNP_UNROLL
    for (int j = 0; j < 3; j++) Vt[i * 3 + j] = Vv[j][i];
  const double sg = (orbx_decomp::det3(abt) < 0.0) != (orbx_decomp::det3(Vt) < 0.0) ? -1.0 : 1.0;
  U[2] = sg * (U[3] * U[7] - U[6] * U[4]);
  U[5] = sg * (U[6] * U[1] - U[0] * U[7]);
  U[8] = sg * (U[0] * U[4] - U[3] * U[1]);
  orbx_decomp::mul33(U, Vt, R);
  if (orbx_decomp::det3(R) < 0.0) {
    R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8];
  }
ORBX_PNP_UNROLL
  for (int k = 0; k < 3; k++) t[k] = pc0[k] - dot3(R + 3 * k, pw0);
  double e[1];
  ops.template sum<1>(e, [&](const Pt& P, double* acc) {
    const double Xc = dot3(R, P.X) + t[0], Yc = dot3(R + 3, P.X) + t[1], invZc = 1.0 / (dot3(R + 6, P.X) + t[2]);
    const double ue = K.uc + K.fu * Xc * invZc, ve = K.vc + K.fv * Yc * invZc;
    acc[0] = acc[0] + sqrt((P.u - ue) * (P.u - ue) + (P.v - ve) * (P.v - ve));
  });
  return e[0] / n;
}

// epnp::compute_pose over the points of `ops`; V is working storage.  Returns the betas' choice (1 .. 3); R row-major.
template <class Ops>
ORBX_PNP_INL int computePose(const Ops& ops, const Cam& K, const VStore& V, double* R, double* t) {
  const double n = (double)ops.count();
  // choose_control_points
  double cws[4][3];
  {
    double s[3];
    ops.template sum<3>(s, [&](const Pt& P, double* acc) {
ORBX_PNP_UNROLL
      for (int k = 0; k < 3; k++) acc[k] = acc[k] + P.X[k];
    });
ORBX_PNP_UNROLL
    for (int k = 0; k < 3; k++) cws[0][k] = s[k] / n;
    double G[6], Vc[3][3], w[3];
    ops.template sum<6>(G, [&](const Pt& P, double* acc) {
      const double d0 = P.X[0] - cws[0][0], d1 = P.X[1] - cws[0][1], d2 = P.X[2] - cws[0][2];
      acc[0] = acc[0] + d0 * d0; acc[1] = acc[1] + d0 * d1; acc[2] = acc[2] + d0 * d2;
      acc[3] = acc[3] + d1 * d1; acc[4] = acc[4] + d1 * d2; acc[5] = acc[5] + d2 * d2;
    });
    orbx_decomp::eig3(G, Vc, w);
ORBX_PNP_UNROLL
    for (int i = 1; i < 4; i++) {
      const double k = orbx_decomp::sqrt0(w[i - 1] / n);
ORBX_PNP_UNROLL
      for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * Vc[j][i - 1];
    }
  }
  // compute_barycentric_coordinates: the inverse once, the coordinates per point where they are needed
  double cc[9], ci[9];
ORBX_PNP_UNROLL
  for (int i = 0; i < 3; i++)
ORBX_PNP_UNROLL
    for (int j = 0; j < 3; j++) cc[3 * i + j] = cws[j + 1][i] - cws[0][i];
  orbx_decomp::inv33(cc, ci);
  // fill_M and M^T M
  double A[78];
  ops.template sum<78>(A, [&](const Pt& P, double* acc) {
    double a[4], r1[12], r2[12];
    alphasOf(cws, ci, P, a);
ORBX_PNP_UNROLL
    for (int i = 0; i < 4; i++) {
      r1[3 * i] = a[i] * K.fu; r1[3 * i + 1] = 0.0; r1[3 * i + 2] = a[i] * (K.uc - P.u);
      r2[3 * i] = 0.0; r2[3 * i + 1] = a[i] * K.fv; r2[3 * i + 2] = a[i] * (K.vc - P.v);
    }
ORBX_PNP_UNROLL
    for (int p = 0; p < 12; p++)
ORBX_PNP_UNROLL
      for (int q = p; q < 12; q++) {  // (entries that are 0 by construction add nothing)
        const double t1 = (p % 3 != 1 && q % 3 != 1) ? r1[p] * r1[q] : 0.0;
        const double t2 = (p % 3 != 0 && q % 3 != 0) ? r2[p] * r2[q] : 0.0;
        acc[sidx12(p, q)] = acc[sidx12(p, q)] + (t1 + t2);
      }
  });
  jacobi12(A, V);
  double v[4][12];
  smallestFour(A, V, v);
  // compute_L_6x10 and compute_rho
  double L[6][10], rho[6];
  {
    double dv[4][6][3];
ORBX_PNP_UNROLL
    for (int i = 0; i < 4; i++) {
      int a = 0, b = 1;
ORBX_PNP_UNROLL
      for (int j = 0; j < 6; j++) {
ORBX_PNP_UNROLL
        for (int k = 0; k < 3; k++) dv[i][j][k] = v[i][3 * a + k] - v[i][3 * b + k];
        b++;
        if (b > 3) {
          a++;
          b = a + 1;
        }
      }
    }
ORBX_PNP_UNROLL
    for (int i = 0; i < 6; i++) {
      L[i][0] = dot3(dv[0][i], dv[0][i]);
      L[i][1] = 2.0 * dot3(dv[0][i], dv[1][i]);
      L[i][2] = dot3(dv[1][i], dv[1][i]);
      L[i][3] = 2.0 * dot3(dv[0][i], dv[2][i]);
      L[i][4] = 2.0 * dot3(dv[1][i], dv[2][i]);
      L[i][5] = dot3(dv[2][i], dv[2][i]);
      L[i][6] = 2.0 * dot3(dv[0][i], dv[3][i]);
      L[i][7] = 2.0 * dot3(dv[1][i], dv[3][i]);
      L[i][8] = 2.0 * dot3(dv[2][i], dv[3][i]);
      L[i][9] = dot3(dv[3][i], dv[3][i]);
    }
    rho[0] = dist2(cws[0], cws[1]); rho[1] = dist2(cws[0], cws[2]); rho[2] = dist2(cws[0], cws[3]);
    rho[3] = dist2(cws[1], cws[2]); rho[4] = dist2(cws[1], cws[3]); rho[5] = dist2(cws[2], cws[3]);
  }
  // find_betas_approx_1 / 2 / 3
  double B1[4], B2[4], B3[4];
  {
    double M[6][4], b[6], x[4];
    const int col[4] = {0, 1, 3, 6};
ORBX_PNP_UNROLL
    for (int i = 0; i < 6; i++) {
ORBX_PNP_UNROLL
      for (int c = 0; c < 4; c++) M[i][c] = L[i][col[c]];
      b[i] = rho[i];
    }
    lsq6<4>(M, b, x);
    if (x[0] < 0.0) {
      B1[0] = sqrt(-x[0]); B1[1] = -x[1] / B1[0]; B1[2] = -x[2] / B1[0]; B1[3] = -x[3] / B1[0];
    } else {
      B1[0] = sqrt(x[0]); B1[1] = x[1] / B1[0]; B1[2] = x[2] / B1[0]; B1[3] = x[3] / B1[0];
    }
  }
  {
    double M[6][3], b[6], x[3];
ORBX_PNP_UNROLL
    for (int i = 0; i < 6; i++) {
ORBX_PNP_UNROLL
      for (int c = 0; c < 3; c++) M[i][c] = L[i][c];
      b[i] = rho[i];
    }
    lsq6<3>(M, b, x);
    if (x[0] < 0.0) {
      B2[0] = sqrt(-x[0]); B2[1] = x[2] < 0.0 ? sqrt(-x[2]) : 0.0;
    } else {
      B2[0] = sqrt(x[0]); B2[1] = x[2] > 0.0 ? sqrt(x[2]) : 0.0;
    }
    if (x[1] < 0.0) B2[0] = -B2[0];
    B2[2] = 0.0; B2[3] = 0.0;
  }
  {
    double M[6][5], b[6], x[5];
ORBX_PNP_UNROLL
    for (int i = 0; i < 6; i++) {
ORBX_PNP_UNROLL
      for (int c = 0; c < 5; c++) M[i][c] = L[i][c];
      b[i] = rho[i];
    }
    lsq6<5>(M, b, x);
    if (x[0] < 0.0) {
      B3[0] = sqrt(-x[0]); B3[1] = x[2] < 0.0 ? sqrt(-x[2]) : 0.0;
    } else {
      B3[0] = sqrt(x[0]); B3[1] = x[2] > 0.0 ? sqrt(x[2]) : 0.0;
    }
    if (x[1] < 0.0) B3[0] = -B3[0];
    B3[2] = x[3] / B3[0]; B3[3] = 0.0;
  }
  // gauss_newton and compute_R_and_t for each, then `N = 1; if (rep[2] < rep[1]) N = 2; if (rep[3] < rep[N]) N = 3`
  int choice = 1;
  double best = 0.0;
ORBX_PNP_NOUNROLL
  for (int set = 0; set < 3; set++) {
    double be[4];
ORBX_PNP_UNROLL
    for (int k = 0; k < 4; k++) be[k] = set == 0 ? B1[k] : set == 1 ? B2[k] : B3[k];
ORBX_PNP_NOUNROLL
    for (int step = 0; step < PNP_GN_STEPS; step++) {
      double Am[6][4], b[6], x[4];
ORBX_PNP_UNROLL
      for (int i = 0; i < 6; i++) {
        const double* l = L[i];
        Am[i][0] = 2.0 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
        Am[i][1] = l[1] * be[0] + 2.0 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
        Am[i][2] = l[3] * be[0] + l[4] * be[1] + 2.0 * l[5] * be[2] + l[8] * be[3];
        Am[i][3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2.0 * l[9] * be[3];
        b[i] = rho[i] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] +
                         l[4] * be[1] * be[2] + l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] +
                         l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
      }
      lsq6<4>(Am, b, x);
ORBX_PNP_UNROLL
      for (int k = 0; k < 4; k++) be[k] = be[k] + x[k];
    }
    double Rs[9], ts[3];
    const double err = computeRt(ops, K, cws, ci, v, be, Rs, ts);
    if (set == 0 || err < best) {
      best = err;
      choice = set + 1;
ORBX_PNP_UNROLL
      for (int k = 0; k < 9; k++) R[k] = Rs[k];
ORBX_PNP_UNROLL
      for (int k = 0; k < 3; k++) t[k] = ts[k];
    }
  }
  return choice;
}

// ---- iterate(), resolved after the fact ------------------------------------------------------------------------------------------
// what a problem's prep leaves: N, mRansacMinInliers, mRansacMaxIts, the status bits of its device data
struct Meta {
  int32_t N, minInliers, maxIts, status;
};
struct Outcome {
  int itsRun, foundIt, bestIt, refined, nBestInliers, nRefines, nDegenerate, badDraws;
};

// The hypotheses' counts in iteration order.  `refine(it)` runs Refine() over the inlier set of hypothesis `it` and returns its
// success; since that depends on the best alone, it is asked once per distinct best.  nIts = min(n_iter, mRansacMaxIts).
template <class RefineFn>
ORBX_PNP_INL void resolveIterations(const Hyp* hyp, int nIts, int minInliers, RefineFn refine, Outcome* o) {
  int best = -1, bestCount = 0, lastRefined = -1;
  o->itsRun = nIts; o->foundIt = -1; o->refined = 0; o->nRefines = 0; o->nDegenerate = 0; o->badDraws = 0;
  for (int it = 0; it < nIts; it++) {
    const int c = hyp[it].count, fl = hyp[it].flags;
    o->nDegenerate += (fl & HYP_DEGENERATE) ? 1 : 0;
    o->badDraws |= (fl & HYP_BAD_DRAWS) ? 1 : 0;
    if (c < minInliers) continue;
    if (c > bestCount) {
      best = it;
      bestCount = c;
    }
    if (best == lastRefined) continue;  // the same set failed before
    lastRefined = best;
    o->nRefines++;
    if (refine(best)) {
      o->foundIt = it;
      o->itsRun = it + 1;
      o->refined = 1;
      break;
    }
  }
  o->bestIt = best;
  o->nBestInliers = bestCount;
}

}  // namespace orbx_pnp
