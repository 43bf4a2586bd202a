// orbx_init_decomp.inc — the decompositions of ReconstructHF (Initialization/Initializer.cpp:440-488) and its selection and
// acceptance rules (:490-545) as plain arithmetic, shared by orbx_init_kernel.hip (device) and tests/cpp/init_ref.cpp (the CPU
// restatement, g++ -ffp-contract=off): one source, so both sides take the same operations.  Their correctness is tested against
// ground truth (tests/test_initializer_host.py), not against each other.  [from-knowledge] restatements of OpenCV / Eigen,
// PARITY UNPINNED; the deviations are listed in include/orbx.h.
#ifndef ORBX_DECOMP_FN
#define ORBX_DECOMP_FN
#endif

namespace orbx_decomp {

// cyclic Jacobi on a symmetric 3x3 (packed a00 a01 a02 a11 a12 a22), 12 fixed sweeps over (0,1) (0,2) (1,2); V's columns = the
// eigenvectors, w = the eigenvalues sorted descending (equal values keep their column order)
ORBX_DECOMP_FN inline void eig3(const double* Ain, double V[3][3], double w[3]) {
  double A[6];
  for (int i = 0; i < 6; i++) A[i] = Ain[i];
  double Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const int ix[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  for (int sweep = 0; sweep < 12; sweep++)
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        const double apq = A[ix[p][q]];
        if (apq == 0.0) continue;
        const double app = A[ix[p][p]], aqq = A[ix[q][q]];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[ix[p][p]] = app - t * apq;
        A[ix[q][q]] = aqq + t * apq;
        A[ix[p][q]] = 0.0;
        const int k = 3 - p - q;
        const double akp = A[ix[k][p]], akq = A[ix[k][q]];
        A[ix[k][p]] = c * akp - s * akq;
        A[ix[k][q]] = s * akp + c * akq;
        for (int r = 0; r < 3; r++) {
          const double vkp = Q[r][p], vkq = Q[r][q];
          Q[r][p] = c * vkp - s * vkq;
          Q[r][q] = s * vkp + c * vkq;
        }
      }
  int o[3] = {0, 1, 2};
  const double d[3] = {A[0], A[3], A[5]};
  for (int i = 1; i < 3; i++)  // insertion sort, descending
    for (int j = i; j > 0 && d[o[j]] > d[o[j - 1]]; j--) { const int tmp = o[j]; o[j] = o[j - 1]; o[j - 1] = tmp; }
  for (int i = 0; i < 3; i++) {
    w[i] = d[o[i]];
    for (int r = 0; r < 3; r++) V[r][i] = Q[r][o[i]];
  }
}

ORBX_DECOMP_FN inline double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
ORBX_DECOMP_FN inline void mul33(const double* a, const double* b, double* c) {
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) c[r * 3 + q] = a[r * 3] * b[q] + a[r * 3 + 1] * b[3 + q] + a[r * 3 + 2] * b[6 + q];
}
ORBX_DECOMP_FN inline void inv33(const double* m, double* r) {  // adjugate / determinant, f64
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double id = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
  r[0] = c00 * id; r[1] = (m[2] * m[7] - m[1] * m[8]) * id; r[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  r[3] = c01 * id; r[4] = (m[0] * m[8] - m[2] * m[6]) * id; r[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  r[6] = c02 * id; r[7] = (m[1] * m[6] - m[0] * m[7]) * id; r[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}
ORBX_DECOMP_FN inline void gram3(const double* M, double* G) {  // packed M^T M
  const int pr[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
  for (int k = 0; k < 6; k++) {
    const int i = pr[k][0], j = pr[k][1];
    G[k] = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
  }
}

// Eigen's K.transpose() * F * K in f32 (Initializer.cpp:452): entries a0*b0 + (a1*b1 + a2*b2) (the unrolled redux), left first
ORBX_DECOMP_FN inline void essentialFromF(const float* F, const float* K, float* E) {
  float T[9];
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) T[r * 3 + q] = K[r] * F[q] + (K[3 + r] * F[3 + q] + K[6 + r] * F[6 + q]);
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) E[r * 3 + q] = T[r * 3] * K[q] + (T[r * 3 + 1] * K[3 + q] + T[r * 3 + 2] * K[6 + q]);
}

// cv::decomposeEssentialMat: E = U D V^T, here in f64 from the eigenvectors v_i of E^T E (u_i = E v_i / |E v_i| for the two
// largest, u_2 = u_0 x u_1, so det U = +1; V^T negated when its determinant is negative), W = [0 1 0; -1 0 0; 0 0 1],
// R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2]; the candidates in the order of :458-466: (R1, t), (R1, -t), (R2, t), (R2, -t).
// Returns 4, or 0 when E has rank < 2.
ORBX_DECOMP_FN inline int decomposeEssential(const float* Ef, float R[4][9], float t[4][3]) {
  double E[9], G[6], V[3][3], w[3], U[9];
  for (int i = 0; i < 9; i++) E[i] = Ef[i];
  gram3(E, G);
  eig3(G, V, w);
  for (int c = 0; c < 2; c++) {
    double u[3], nn = 0;
    for (int r = 0; r < 3; r++) {
      u[r] = E[r * 3] * V[0][c] + E[r * 3 + 1] * V[1][c] + E[r * 3 + 2] * V[2][c];
      nn += u[r] * u[r];
    }
    nn = sqrt(nn);
    if (!(nn > 0)) return 0;
    for (int r = 0; r < 3; r++) U[r * 3 + c] = u[r] / nn;
  }
  U[2] = U[3] * U[7] - U[6] * U[4];
  U[5] = U[6] * U[1] - U[0] * U[7];
  U[8] = U[0] * U[4] - U[3] * U[1];
  double Vt[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Vt[i * 3 + j] = V[j][i];
  if (det3(Vt) < 0)
    for (int i = 0; i < 9; i++) Vt[i] = -Vt[i];
  const double W[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1}, Wt[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
  double T1[9], R1[9], R2[9];
  mul33(U, W, T1);
  mul33(T1, Vt, R1);
  mul33(U, Wt, T1);
  mul33(T1, Vt, R2);
  for (int k = 0; k < 4; k++) {
    const double* Rk = k < 2 ? R1 : R2;
    const double sg = (k & 1) ? -1.0 : 1.0;
    for (int i = 0; i < 9; i++) R[k][i] = (float)Rk[i];
    for (int i = 0; i < 3; i++) t[k][i] = (float)(sg * U[i * 3 + 2]);
  }
  return 4;
}

ORBX_DECOMP_FN inline double oppositeOfMinor(const double* M, int row, int col) {
  const int x1 = col == 0 ? 1 : 0, x2 = col == 2 ? 1 : 2, y1 = row == 0 ? 1 : 0, y2 = row == 2 ? 1 : 2;
  return M[y1 * 3 + x2] * M[y2 * 3 + x1] - M[y1 * 3 + x1] * M[y2 * 3 + x2];
}
ORBX_DECOMP_FN inline double sqrt0(double v) { return sqrt(v > 0 ? v : 0.0); }

// cv::decomposeHomographyMat (HomographyDecompInria, the analytical decomposition of Malis & Vargas, INRIA RR-6303, 2007):
// Hn = K^-1 H K / sigma_2(K^-1 H K); S = Hn^T Hn - I; every |S_ij| < 0.001: a pure rotation, one solution (Hn, 0, 0); else the
// two normals from the row of the largest |S_ii|, and (Ra, ta, na), (Ra, -ta, -na), (Rb, tb, nb), (Rb, -tb, -nb) in OpenCV's
// order, R = Hn (I - 2/v t* n^T), t = R t*.  t is the translation over the plane's distance.  Square roots of quantities that
// are negative by rounding are taken at 0 (OpenCV returns NaNs there).  Returns the number of solutions (1 or 4).
ORBX_DECOMP_FN inline int decomposeHomography(const float* Hf, const float* Kf, float R[4][9], float t[4][3], float n[4][3]) {
  double H[9], K[9], Ki[9], T[9], Hn[9], G[6], V[3][3], w[3];
  for (int i = 0; i < 9; i++) { H[i] = Hf[i]; K[i] = Kf[i]; }
  inv33(K, Ki);
  mul33(Ki, H, T);
  mul33(T, K, Hn);
  gram3(Hn, G);
  eig3(G, V, w);
  const double is1 = 1.0 / sqrt0(w[1]);
  for (int i = 0; i < 9; i++) Hn[i] *= is1;
  double S[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) S[i * 3 + j] = Hn[i] * Hn[j] + Hn[3 + i] * Hn[3 + j] + Hn[6 + i] * Hn[6 + j] - (i == j ? 1.0 : 0.0);
  double mx = 0;
  for (int i = 0; i < 9; i++) mx = fabs(S[i]) > mx ? fabs(S[i]) : mx;
  if (mx < 0.001) {
    for (int i = 0; i < 9; i++) R[0][i] = (float)Hn[i];
    for (int i = 0; i < 3; i++) { t[0][i] = 0.f; n[0][i] = 0.f; }
    return 1;
  }
  const double M00 = oppositeOfMinor(S, 0, 0), M11 = oppositeOfMinor(S, 1, 1), M22 = oppositeOfMinor(S, 2, 2);
  const double rtM00 = sqrt0(M00), rtM11 = sqrt0(M11), rtM22 = sqrt0(M22);
  const double M01 = oppositeOfMinor(S, 0, 1), M12 = oppositeOfMinor(S, 1, 2), M02 = oppositeOfMinor(S, 0, 2);
  const double e12 = M12 >= 0 ? 1.0 : -1.0, e02 = M02 >= 0 ? 1.0 : -1.0, e01 = M01 >= 0 ? 1.0 : -1.0;
  const double nS00 = fabs(S[0]), nS11 = fabs(S[4]), nS22 = fabs(S[8]);
  int indx = 0;
  if (nS00 < nS11) {
    indx = 1;
    if (nS11 < nS22) indx = 2;
  } else if (nS00 < nS22) {
    indx = 2;
  }
  double npa[3], npb[3];
  if (indx == 0) {
    npa[0] = S[0]; npa[1] = S[1] + rtM22; npa[2] = S[2] + e12 * rtM11;
    npb[0] = S[0]; npb[1] = S[1] - rtM22; npb[2] = S[2] - e12 * rtM11;
  } else if (indx == 1) {
    npa[0] = S[1] + rtM22; npa[1] = S[4]; npa[2] = S[5] - e02 * rtM00;
    npb[0] = S[1] - rtM22; npb[1] = S[4]; npb[2] = S[5] + e02 * rtM00;
  } else {
    npa[0] = S[2] + e01 * rtM11; npa[1] = S[5] + rtM00; npa[2] = S[8];
    npb[0] = S[2] - e01 * rtM11; npb[1] = S[5] - rtM00; npb[2] = S[8];
  }
  const double traceS = S[0] + S[4] + S[8];
  const double v = 2.0 * sqrt0(1 + traceS - M00 - M11 - M22);
  const double ESii = S[indx * 4] >= 0 ? 1.0 : -1.0;
  const double r = sqrt0(2 + traceS + v), nt = sqrt0(2 + traceS - v);
  const double la = sqrt(npa[0] * npa[0] + npa[1] * npa[1] + npa[2] * npa[2]);
  const double lb = sqrt(npb[0] * npb[0] + npb[1] * npb[1] + npb[2] * npb[2]);
  double na[3], nb[3], tas[3], tbs[3];
  for (int i = 0; i < 3; i++) { na[i] = npa[i] / la; nb[i] = npb[i] / lb; }
  const double half_nt = 0.5 * nt, esii_t_r = ESii * r;
  for (int i = 0; i < 3; i++) {
    tas[i] = half_nt * (esii_t_r * nb[i] - nt * na[i]);
    tbs[i] = half_nt * (esii_t_r * na[i] - nt * nb[i]);
  }
  for (int s = 0; s < 2; s++) {
    const double* ts = s == 0 ? tas : tbs;
    const double* nn = s == 0 ? na : nb;
    double M[9], Rm[9], tt[3];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) M[i * 3 + j] = (i == j ? 1.0 : 0.0) - (2.0 / v) * ts[i] * nn[j];
    mul33(Hn, M, Rm);
    for (int i = 0; i < 3; i++) tt[i] = Rm[i * 3] * ts[0] + Rm[i * 3 + 1] * ts[1] + Rm[i * 3 + 2] * ts[2];
    for (int k = 0; k < 2; k++) {
      const int idx = 2 * s + k;
      const double sg = k ? -1.0 : 1.0;
      for (int i = 0; i < 9; i++) R[idx][i] = (float)Rm[i];
      for (int i = 0; i < 3; i++) { t[idx][i] = (float)(sg * tt[i]); n[idx][i] = (float)(sg * nn[i]); }
    }
  }
  return 4;
}

// ReconstructHF's choice among the candidates' CheckRT results (:490-507) and its acceptance rules (:509-545); returns the
// ORBX_INIT_AMBIGUOUS (8) / LOW_PARALLAX (16) / FEW_TRIANGULATED (32) / FEW_INLIERS (64) bits.  nInliers = the inliers of the
// chosen model; minParallax as the reference passes it (`int minParallax = 1.0`, :103, converted to float).
ORBX_DECOMP_FN inline int reconstructRules(int nSol, const int* nGood, const float* parallax, int nInliers, float minParallax,
                                    int minTriangulated, int* bestIdx, int* bestGood, int* secondGood, float* bestParallax) {
  int bg = 0, sg = 0, bi = -1;
  float bp = -1;
  for (int i = 0; i < nSol; i++) {
    if (nGood[i] > bg) {
      sg = bg; bg = nGood[i]; bi = i; bp = parallax[i];
    } else if (nGood[i] > sg) {
      sg = nGood[i];
    }
  }
  int st = 0;
  if (sg > 0.7 * bg) st |= 8;
  if (bp < minParallax) st |= 16;
  if (bg < minTriangulated) st |= 32;
  if (bg < 0.9 * nInliers) st |= 64;
  *bestIdx = bi; *bestGood = bg; *secondGood = sg; *bestParallax = bp;
  return st;
}

}  // namespace orbx_decomp
