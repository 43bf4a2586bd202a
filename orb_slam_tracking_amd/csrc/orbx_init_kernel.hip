// orbx_init_kernel.hip — the RANSAC stage of Initializer::Initialize (Initialization/Initializer.cpp:19-111) on the device, for
// a batch of frame pairs: mvMatches12, the 8-point H and F hypotheses of every iteration, and, behind the scoring kernel
// (k_check_model, orbx_kernels.hip), the kept hypotheses, SH / SF / RH and the model choice.
//
//   k_init_prep    block (one wave) per pair   mvMatches12 compacted in order (:24-33), N, checks of the device data
//   k_init_solve   lane per (pair, iteration)  blockIdx.y = 0: cv::findHomography(src, dst, 0), 1: cv::findFundamentalMat(
//                                              FM_8POINT) [from-knowledge], f64, then toMatrix3f and (H) Eigen's inverse()
//   k_init_select  block (one wave) per pair   first maximum of each loop, nH / nF, SH, SF, RH, model (:78-111); for
//                                              orbx_initialize* also the chosen model's decomposition (:440-488) and its
//                                              inliers for k_check_rt (orbx_checkrt_kernel.hip, batched form)
//   k_init_finish  block (one wave) per pair   ReconstructHF's choice and rules (:490-566), orbx_init_result, vP3D
//
// All floating point is IEEE f64 / f32 without contraction (-ffp-contract=off), so tests/cpp/init_ref.cpp repeats it bit for
// bit.  The solver keeps the 9x9 Gram matrix (packed upper triangle, 45 doubles) and the eigenvector matrix (81 doubles) in
// registers: every index below is a compile-time constant once the loops are unrolled.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/orbx.h"
#include "orbx_launch.h"

#define ORBX_DECOMP_FN __device__
#include "orbx_init_decomp.inc"

namespace orbx {

constexpr int INIT_JACOBI_SWEEPS = 12;  // fixed: no convergence test, so the host restatement takes the same path

// packed upper triangle of a symmetric n x n matrix
template <int n>
__host__ __device__ constexpr int sidx(int i, int j) {
  return i <= j ? i * n - i * (i - 1) / 2 + (j - i) : j * n - j * (j - 1) / 2 + (i - j);
}

// Eigenvector of the smallest eigenvalue of the symmetric n x n matrix A (packed, destroyed): cyclic Jacobi, INIT_JACOBI_SWEEPS
// sweeps over the pairs (p, q), p < q, in row order; a pair whose off-diagonal entry is exactly 0 is skipped.  Rotation as in
// Golub & Van Loan 8.4 (theta = (a_qq - a_pp) / 2 a_pq, t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1),
// s = t c).  The smallest eigenvalue is the smallest diagonal entry, the first among equals.  *nTiny = the number of
// eigenvalues with |lambda| < DBL_EPSILON (findFundamentalMat's rank test).
template <int n>
__device__ __forceinline__ void jacobiSmallest(double* A, double* v, int* nTiny) {
  double V[n][n];
#pragma unroll
  for (int i = 0; i < n; i++)
#pragma unroll
    for (int k = 0; k < n; k++) V[i][k] = i == k ? 1.0 : 0.0;
  for (int sweep = 0; sweep < INIT_JACOBI_SWEEPS; sweep++) {
#pragma unroll
    for (int p = 0; p < n - 1; p++)
#pragma unroll
      for (int q = p + 1; q < n; q++) {
        const double apq = A[sidx<n>(p, q)];
        if (apq != 0.0) {
          const double app = A[sidx<n>(p, p)], aqq = A[sidx<n>(q, q)];
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          A[sidx<n>(p, p)] = app - t * apq;
          A[sidx<n>(q, q)] = aqq + t * apq;
          A[sidx<n>(p, q)] = 0.0;
#pragma unroll
          for (int k = 0; k < n; k++) {
            if (k == p || k == q) continue;
            const double akp = A[sidx<n>(k, p)], akq = A[sidx<n>(k, q)];
            A[sidx<n>(k, p)] = c * akp - s * akq;
            A[sidx<n>(k, q)] = s * akp + c * akq;
          }
#pragma unroll
          for (int k = 0; k < n; k++) {
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = c * vkp - s * vkq;
            V[k][q] = s * vkp + c * vkq;
          }
        }
      }
  }
  double wb = A[sidx<n>(0, 0)];
  int tiny = 0;
#pragma unroll
  for (int k = 0; k < n; k++) v[k] = V[k][0];
#pragma unroll
  for (int i = 0; i < n; i++) {
    const double w = A[sidx<n>(i, i)];
    tiny += fabs(w) < 2.2204460492503131e-16 ? 1 : 0;
    if (i == 0) continue;
    const bool lt = w < wb;
    wb = lt ? w : wb;
#pragma unroll
    for (int k = 0; k < n; k++) v[k] = lt ? V[k][i] : v[k];
  }
  *nTiny = tiny;
}

// row-major 3x3 products in f64, sums in k order
__device__ __forceinline__ void mul3(const double* a, const double* b, double* c) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int q = 0; q < 3; q++) c[r * 3 + q] = a[r * 3] * b[q] + a[r * 3 + 1] * b[3 + q] + a[r * 3 + 2] * b[6 + q];
}

// Eigen::Matrix3f::inverse() (Eigen/src/LU/InverseImpl.h, compute_inverse<3>) [from-knowledge]: cofactors of column 0, det =
// c0*m00 + (c1*m10 + c2*m20) (the unrolled redux), invdet = 1 / det, result(i, j) = cofactor(j, i) * invdet, all f32.
__device__ __forceinline__ float cof3(const float* m, int i, int j) {
  const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
  return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}
__device__ __forceinline__ void eigenInverse3(const float* m, float* r) {
  const float c0 = cof3(m, 0, 0), c1 = cof3(m, 1, 0), c2 = cof3(m, 2, 0);
  const float det = c0 * m[0] + (c1 * m[3] + c2 * m[6]);
  const float invdet = 1.0f / det;
  r[0] = c0 * invdet; r[1] = c1 * invdet; r[2] = c2 * invdet;
#pragma unroll
  for (int i = 1; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) r[i * 3 + j] = cof3(m, j, i) * invdet;
}

// ---- k_init_prep: mvMatches12 of every pair, in order (Initializer.cpp:24-33) -------------------------------------------
__global__ __launch_bounds__(64) void k_init_prep(const InitArgs a) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int f1 = a.frames[p], f2 = a.frames[a.nPairs + p];
  const int n1 = a.nKps[f1], n2 = a.nKps[f2];
  int st = 0;
  if (n1 < 0 || n1 > a.cap || n2 < 0 || n2 > a.cap) st |= ORBX_INIT_BAD_MATCHES;
  const int n1c = (st & ORBX_INIT_BAD_MATCHES) ? 0 : n1;
  const int32_t* m12 = a.m12 + (size_t)p * a.cap;
  int32_t* first = a.first + (size_t)p * a.cap;
  int32_t* second = a.second + (size_t)p * a.cap;
  int N = 0;
  bool bad = false;
  for (int i0 = 0; i0 < n1c; i0 += 64) {
    const int i = i0 + lane;
    const int m = i < n1c ? m12[i] : -1;
    const bool take = m >= 0;
    bad |= m >= n2;
    const unsigned long long mask = __ballot(take);
    if (take) {
      const int slot = N + __popcll(mask & ((1ull << lane) - 1ull));
      first[slot] = i;
      second[slot] = m;
    }
    N += (int)__popcll(mask);
  }
  if (__ballot(bad)) st |= ORBX_INIT_BAD_MATCHES;
  if (N < 8) st |= ORBX_INIT_TOO_FEW_MATCHES;
  if (lane == 0) {
    a.N[p] = N;
    a.scoreN[p] = (st & ORBX_INIT_BAD_MATCHES) ? 0 : N;
    a.pstat[p] = st;
  }
}

// ---- k_init_solve: one 8-point hypothesis per lane ------------------------------------------------------------------------
// H (cv::findHomography, method 0: HomographyEstimatorCallback::runKernel without the LM refinement):
//   centroids cM (src = frame 1), cm (dst = frame 2); per axis mean absolute deviation, count / sum as the scale (a sum below
//   DBL_EPSILON: degenerate); rows Lx = (X, Y, 1, 0, 0, 0, -xX, -xY, -x), Ly = (0, 0, 0, X, Y, 1, -yX, -yY, -y) of the
//   normalised points accumulated into the upper triangle of LtL, point by point; H0 = invHnorm * h * Hnorm2, scaled by
//   1 / H0(2,2).
// F (cv::findFundamentalMat, FM_8POINT: run8Point): centroids m1c, m2c; scale = sqrt(2) / mean distance to the centroid (a mean
//   below FLT_EPSILON: degenerate); rows r = (x2x1, x2y1, x2, y2x1, y2y1, y2, x1, y1, 1) accumulated into the upper triangle of
//   A; two or more eigenvalues below DBL_EPSILON: degenerate; rank 2: F0 - (F0 v) v^T with v the eigenvector of the smallest
//   eigenvalue of F0^T F0; F = T2^T F0 T1, scaled by 1 / F(2,2) when |F(2,2)| > FLT_EPSILON.
__global__ __launch_bounds__(64) void k_init_solve(const InitArgs a) {
  const int hyp = blockIdx.x * 64 + threadIdx.x;
  const int kind = blockIdx.y;
  if (hyp >= a.nPairs * a.nIter) return;
  const int p = hyp / a.nIter;
  const int N = a.scoreN[p];
  const int32_t* set = a.sets + (size_t)hyp * 8;
  // the set is checked before anything is read through it
  int idx[8];
  bool ok = N >= 8;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    idx[j] = set[j];
    ok = ok && idx[j] >= 0 && idx[j] < N;
  }
#pragma unroll
  for (int j = 1; j < 8; j++)
#pragma unroll
    for (int k = 0; k < j; k++) ok = ok && idx[j] != idx[k];
  float* out = (kind == 0 ? a.H21 : a.F21) + (size_t)hyp * 9;
  if (!ok) {
#pragma unroll
    for (int q = 0; q < 9; q++) out[q] = 0.f;
    if (kind == 0) {
#pragma unroll
      for (int q = 0; q < 9; q++) a.H12[(size_t)hyp * 9 + q] = 0.f;
    }
    // (a pair with too few matches is reported by k_init_prep, a bad index of a usable pair here)
    a.flags[(size_t)kind * a.nPairs * a.nIter + hyp] =
        (uint8_t)((kind == 0 ? INIT_FLAG_H_DEGENERATE : INIT_FLAG_F_DEGENERATE) | (N >= 8 ? INIT_FLAG_BAD_SET : 0));
    return;
  }
  const orbx_keypoint* k1 = a.kps + (size_t)a.frames[p] * a.cap;
  const orbx_keypoint* k2 = a.kps + (size_t)a.frames[a.nPairs + p] * a.cap;
  const int32_t* first = a.first + (size_t)p * a.cap;
  const int32_t* second = a.second + (size_t)p * a.cap;
  float sx[8], sy[8], dx[8], dy[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const orbx_keypoint q1 = k1[first[idx[j]]], q2 = k2[second[idx[j]]];
    sx[j] = q1.x; sy[j] = q1.y; dx[j] = q2.x; dy[j] = q2.y;
  }
  double M[9];
  bool degenerate = false;
  double A[45];
#pragma unroll
  for (int q = 0; q < 45; q++) A[q] = 0.0;
  if (kind == 0) {
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { cmx += dx[j]; cmy += dy[j]; cMx += sx[j]; cMy += sy[j]; }
    const double t8 = 1.0 / 8;
    cmx *= t8; cmy *= t8; cMx *= t8; cMy *= t8;
    double smx = 0, smy = 0, sMx = 0, sMy = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      smx += fabs(dx[j] - cmx); smy += fabs(dy[j] - cmy);
      sMx += fabs(sx[j] - cMx); sMy += fabs(sy[j] - cMy);
    }
    const double eps = 2.2204460492503131e-16;
    degenerate = fabs(smx) < eps || fabs(smy) < eps || fabs(sMx) < eps || fabs(sMy) < eps;
    smx = 8 / smx; smy = 8 / smy; sMx = 8 / sMx; sMy = 8 / sMy;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const double x = (dx[j] - cmx) * smx, y = (dy[j] - cmy) * smy;
      const double X = (sx[j] - cMx) * sMx, Y = (sy[j] - cMy) * sMy;
      const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
      const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
#pragma unroll
      for (int r = 0; r < 9; r++)
#pragma unroll
        for (int q = r; q < 9; q++) A[sidx<9>(r, q)] += Lx[r] * Lx[q] + Ly[r] * Ly[q];
    }
    double h[9];
    int nTiny;
    jacobiSmallest<9>(A, h, &nTiny);
    const double invHnorm[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
    const double Hnorm2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
    double T[9];
    mul3(invHnorm, h, T);
    mul3(T, Hnorm2, M);
    const double s22 = 1. / M[8];
#pragma unroll
    for (int q = 0; q < 9; q++) M[q] *= s22;
  } else {
    double m1x = 0, m1y = 0, m2x = 0, m2y = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { m1x += sx[j]; m1y += sy[j]; m2x += dx[j]; m2y += dy[j]; }
    const double t8 = 1.0 / 8;
    m1x *= t8; m1y *= t8; m2x *= t8; m2y *= t8;
    double s1 = 0, s2 = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const double ax = sx[j] - m1x, ay = sy[j] - m1y, bx = dx[j] - m2x, by = dy[j] - m2y;
      s1 += sqrt(ax * ax + ay * ay);
      s2 += sqrt(bx * bx + by * by);
    }
    s1 *= t8; s2 *= t8;
    const double feps = 1.1920928955078125e-07;
    degenerate = s1 < feps || s2 < feps;
    s1 = 1.4142135623730951 / s1; s2 = 1.4142135623730951 / s2;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const double x1 = (sx[j] - m1x) * s1, y1 = (sy[j] - m1y) * s1;
      const double x2 = (dx[j] - m2x) * s2, y2 = (dy[j] - m2y) * s2;
      const double r[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1};
#pragma unroll
      for (int i = 0; i < 9; i++)
#pragma unroll
        for (int q = i; q < 9; q++) A[sidx<9>(i, q)] += r[i] * r[q];
    }
    double f[9];
    int nTiny;
    jacobiSmallest<9>(A, f, &nTiny);
    degenerate = degenerate || nTiny >= 2;
    // rank 2: the component of F0 along the smallest right singular vector is removed
    double G[6];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int q = i; q < 3; q++) G[sidx<3>(i, q)] = f[i] * f[q] + f[3 + i] * f[3 + q] + f[6 + i] * f[6 + q];
    double w[3];
    int nTiny3;
    jacobiSmallest<3>(G, w, &nTiny3);
    double F0[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double fw = f[r * 3] * w[0] + f[r * 3 + 1] * w[1] + f[r * 3 + 2] * w[2];
#pragma unroll
      for (int q = 0; q < 3; q++) F0[r * 3 + q] = f[r * 3 + q] - fw * w[q];
    }
    const double T1[9] = {s1, 0, -s1 * m1x, 0, s1, -s1 * m1y, 0, 0, 1};
    const double T2t[9] = {s2, 0, 0, 0, s2, 0, -s2 * m2x, -s2 * m2y, 1};
    double T[9];
    mul3(T2t, F0, T);
    mul3(T, T1, M);
    if (fabs(M[8]) > 1.1920928955078125e-07) {
      const double s22 = 1. / M[8];
#pragma unroll
      for (int q = 0; q < 9; q++) M[q] *= s22;
    }
  }
  float Mf[9];
  bool finite = true;
#pragma unroll
  for (int q = 0; q < 9; q++) {
    Mf[q] = (float)M[q];
    finite = finite && isfinite(Mf[q]);
  }
  degenerate = degenerate || !finite;
#pragma unroll
  for (int q = 0; q < 9; q++) out[q] = degenerate ? 0.f : Mf[q];
  if (kind == 0) {
    float Mi[9];
    eigenInverse3(Mf, Mi);
#pragma unroll
    for (int q = 0; q < 9; q++) a.H12[(size_t)hyp * 9 + q] = degenerate ? 0.f : Mi[q];
  }
  a.flags[(size_t)kind * a.nPairs * a.nIter + hyp] = (uint8_t)(degenerate ? (kind == 0 ? INIT_FLAG_H_DEGENERATE : INIT_FLAG_F_DEGENERATE) : 0);
}

// ---- k_init_select: what Initialize does with the two loops' results (:78-111) -------------------------------------------
// first maximum over iterations of each loop (`currentScore > score`, score from 0; a degenerate hypothesis does not compete)
__device__ __forceinline__ void bestOf(const float* scores, const uint8_t* flags, int nIter, int lane, float* bestScore, int* bestIt) {
  float s = 0.f;
  int it = -1;
  for (int i = lane; i < nIter; i += 64) {
    const float v = flags[i] ? 0.f : scores[i];
    if (v > s) { s = v; it = i; }  // (a lane's own iterations ascend: its first maximum)
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float s2 = __shfl_xor(s, o);
    const int it2 = __shfl_xor(it, o);
    if (s2 > s || (s2 == s && it2 >= 0 && (it < 0 || it2 < it))) { s = s2; it = it2; }
  }
  *bestScore = s;
  *bestIt = it;
}

__global__ __launch_bounds__(64) void k_init_select(const InitArgs a) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const size_t nh = (size_t)a.nPairs * a.nIter, base = (size_t)p * a.nIter;
  const int N = a.N[p], sN = a.scoreN[p];
  const uint8_t* flH = a.flags + base;
  const uint8_t* flF = a.flags + nh + base;
  float SH, SF;
  int itH, itF;
  bestOf(a.scoresH + base, flH, a.nIter, lane, &SH, &itH);
  bestOf(a.scoresF + base, flF, a.nIter, lane, &SF, &itF);
  bool badSet = false;
  for (int i = lane; i < a.nIter; i += 64) badSet |= (flH[i] & INIT_FLAG_BAD_SET) != 0;
  int nH = 0, nF = 0;
  const uint8_t* iH = itH >= 0 ? a.inlH + (base + itH) * a.cap : nullptr;
  const uint8_t* iF = itF >= 0 ? a.inlF + (base + itF) * a.cap : nullptr;
  uint8_t* oH = a.inlOut ? a.inlOut + (size_t)p * 2 * a.cap : nullptr;
  uint8_t* oF = oH ? oH + a.cap : nullptr;
  for (int i = lane; i < sN; i += 64) {
    const uint8_t h = iH ? iH[i] : 0, f = iF ? iF[i] : 0;
    nH += h; nF += f;
    if (oH) { oH[i] = h; oF[i] = f; }
  }
  if (oH)
    for (int i = sN + lane; i < N && i < a.cap; i += 64) { oH[i] = 0; oF[i] = 0; }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { nH += __shfl_xor(nH, o); nF += __shfl_xor(nF, o); }
  const bool anyBadSet = __ballot(badSet) != 0;
  orbx_hf_result* r = a.res + p;
  if (lane < 9) {
    r->H21[lane] = itH >= 0 ? a.H21[(base + itH) * 9 + lane] : 0.f;
    r->H12[lane] = itH >= 0 ? a.H12[(base + itH) * 9 + lane] : 0.f;
    r->F21[lane] = itF >= 0 ? a.F21[(base + itF) * 9 + lane] : 0.f;
  }
  if (lane == 0) {
    int st = a.pstat[p] | (anyBadSet ? ORBX_INIT_BAD_SETS : 0);
    const float sum = SH + SF;
    if (sum == 0.f) st |= ORBX_INIT_NO_SCORE;
    const float RH = sum == 0.f ? 0.f : SH / sum;
    r->status = st;
    r->model = sum == 0.f ? -1 : (RH > 0.50 ? 0 : 1);
    r->n_matches = N;
    r->best_it_h = itH; r->best_it_f = itF;
    r->n_inliers_h = nH; r->n_inliers_f = nF;
    r->reserved = 0;
    r->score_h = SH; r->score_f = SF; r->rh = RH;
  }
  if (!a.reconstruct) return;
  // ---- ReconstructHF's input (:440-488): the chosen model's inliers in match order for CheckRT, its (R, t) candidates ----
  const int st1 = a.pstat[p] | (anyBadSet ? ORBX_INIT_BAD_SETS : 0) | ((SH + SF) == 0.f ? ORBX_INIT_NO_SCORE : 0);
  const bool go = st1 == 0;  // Initialize reconstructs only behind a clean model stage
  const bool isF = !(SH / (SH + SF) > 0.50);
  const uint8_t* ic = isF ? iF : iH;
  const orbx_keypoint* k1 = a.kps + (size_t)a.frames[p] * a.cap;
  const orbx_keypoint* k2 = a.kps + (size_t)a.frames[a.nPairs + p] * a.cap;
  const int32_t* first = a.first + (size_t)p * a.cap;
  const int32_t* second = a.second + (size_t)p * a.cap;
  float4* pts = reinterpret_cast<float4*>(a.pts) + (size_t)p * a.cap;
  int32_t* book = a.book + (size_t)p * a.cap;
  int nI = 0;
  for (int i0 = 0; go && ic && i0 < sN; i0 += 64) {
    const int i = i0 + lane;
    const bool in = i < sN && ic[i];
    const unsigned long long mask = __ballot(in);
    if (in) {
      const int j = nI + __popcll(mask & ((1ull << lane) - 1ull));
      const orbx_keypoint q1 = k1[first[i]], q2 = k2[second[i]];
      pts[j] = make_float4(q1.x, q1.y, q2.x, q2.y);
      book[j] = first[j];
    }
    nI += (int)__popcll(mask);
  }
  if (lane == 0) {
    int nSol = 0;
    float R[4][9], t[4][3], nrm[4][3];
    if (go) {  // (go: the chosen loop kept a hypothesis, so its iteration is >= 0)
      float M[9];
      for (int q = 0; q < 9; q++) M[q] = isF ? a.F21[(base + itF) * 9 + q] : a.H21[(base + itH) * 9 + q];
      if (isF) {
        float E[9];
        orbx_decomp::essentialFromF(M, a.K, E);
        nSol = orbx_decomp::decomposeEssential(E, R, t);
      } else {
        nSol = orbx_decomp::decomposeHomography(M, a.K, R, t, nrm);
      }
    }
    for (int k = 0; k < nSol; k++) {
      for (int q = 0; q < 9; q++) a.R4[((size_t)p * 4 + k) * 9 + q] = R[k][q];
      for (int q = 0; q < 3; q++) a.t4[((size_t)p * 4 + k) * 3 + q] = t[k][q];
    }
    a.nSol[p] = nSol;
    a.nInl[p] = nI;
  }
}

// ---- k_init_finish: ReconstructHF's choice and acceptance (:490-566), the orbx_init_result of every pair --------------------
__global__ __launch_bounds__(64) void k_init_finish(const InitArgs a) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const orbx_hf_result* h = a.res + p;
  orbx_init_result* r = a.ires + p;
  const int nSol = a.nSol[p];
  int ng[4];
  float par[4];
  for (int k = 0; k < 4; k++) {
    ng[k] = k < nSol ? a.nGood[p * 4 + k] : 0;
    par[k] = k < nSol ? a.parallax[p * 4 + k] : 0.f;
  }
  int st = h->status;
  int bi = -1, bg = 0, sg = 0;
  float bp = -1.f;
  if (st == 0)
    st |= orbx_decomp::reconstructRules(nSol, ng, par, h->model == 0 ? h->n_inliers_h : h->n_inliers_f, a.minParallax,
                                        a.minTriangulated, &bi, &bg, &sg, &bp);
  const uint8_t* gsrc = bi >= 0 ? a.good + ((size_t)p * 4 + bi) * a.cap : nullptr;
  const float* psrc = bi >= 0 ? a.p3d4 + ((size_t)p * 4 + bi) * a.cap * 3 : nullptr;
  for (int i = lane; i < a.cap; i += 64) {
    if (a.triOut) a.triOut[(size_t)p * a.cap + i] = gsrc ? gsrc[i] : 0;
    if (a.p3dOut)
      for (int c = 0; c < 3; c++) a.p3dOut[((size_t)p * a.cap + i) * 3 + c] = psrc ? psrc[i * 3 + c] : 0.f;
  }
  if (lane < 9) {
    r->R21[lane] = bi >= 0 ? a.R4[((size_t)p * 4 + bi) * 9 + lane] : 0.f;
    r->H21[lane] = h->H21[lane];
    r->F21[lane] = h->F21[lane];
    if (lane < 3) r->t21[lane] = bi >= 0 ? a.t4[((size_t)p * 4 + bi) * 3 + lane] : 0.f;
  }
  if (lane == 0) {
    r->status = st;
    r->model = h->model;
    r->n_matches = h->n_matches;
    r->best_it_h = h->best_it_h; r->best_it_f = h->best_it_f;
    r->n_inliers_h = h->n_inliers_h; r->n_inliers_f = h->n_inliers_f;
    r->n_solutions = nSol;
    r->best_solution = bi; r->best_good = bg; r->second_good = sg;
    r->reserved = 0;
    r->score_h = h->score_h; r->score_f = h->score_f; r->rh = h->rh;
    r->parallax = bp;
  }
}

hipError_t launch_init_prep(hipStream_t st, const InitArgs& a) {
  hipLaunchKernelGGL(k_init_prep, dim3(a.nPairs), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_init_solve(hipStream_t st, const InitArgs& a) {
  const int n = a.nPairs * a.nIter;
  hipLaunchKernelGGL(k_init_solve, dim3((n + 63) / 64, 2), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_init_finish(hipStream_t st, const InitArgs& a) {
  hipLaunchKernelGGL(k_init_finish, dim3(a.nPairs), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_init_select(hipStream_t st, const InitArgs& a) {
  hipLaunchKernelGGL(k_init_select, dim3(a.nPairs), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
