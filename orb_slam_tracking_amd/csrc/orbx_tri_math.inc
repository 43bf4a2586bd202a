// orbx_tri_math.inc — the arithmetic of LocalMapping::CreateNewMapPoints (include/orbx.h, "growing the map") as plain f32 / f64
// operations, shared by orbx_match_tri_kernel.hip (device) and tests/cpp/tri_ref.cpp (the CPU restatement, g++ -ffp-contract=off):
// one source, so both sides take the same operations in the same order and agree bit for bit, as orbx_ba_math.inc does for the
// bundle adjustment.  What is NOT shared is the walk: which features meet, in which order, who takes whom, the histogram, the
// counters; each side writes that on its own.  Correctness is tested against an independent numpy statement and against ground
// truth (tests/test_tri_host.py), not against the other side.
// f32 without contraction; a matrix product is "gemm on CV_32F": the products and their sum in f64 in ascending k, one rounding.
// Only +, -, *, /, sqrt and comparisons: no libm call beyond sqrt on doubles.  The includer defines ORBX_TRI_FN (__device__ on the
// device, nothing on the host, where it also defines __device__ to nothing for orbx_svd4.inc).
#ifndef ORBX_TRI_FN
#define ORBX_TRI_FN
#endif

namespace orbx_tri {

#include "orbx_svd4.inc"

// what one (KF1, KF2) pair's two poses and K give (rule 1 of SearchForTriangulation)
struct PairGeom {
  float F12[9];
  float ex, ey;        // KF1's camera centre in KF2's image
  float baseline;      // |Ow2 - Ow1|
  float Ow1[3], Ow2[3];
  int nonfinite;       // one of the 24 pose values is no finite number: nothing else is set
};

// the outcomes of one match in the triangulation (rule numbers of orbx_triangulate_matches*)
enum { TRI_KEPT = 1, TRI_LOW_PARALLAX, TRI_W_ZERO, TRI_BEHIND_1, TRI_BEHIND_2, TRI_REPROJ_1, TRI_REPROJ_2, TRI_ZERO_DIST, TRI_SCALE };

struct TriPoint {
  float X[3], normal[3], minDist, maxDist;
};

ORBX_TRI_FN inline bool isFinite(float v) { return v - v == 0.0f; }

// C = A * B, 3x3 row-major
ORBX_TRI_FN inline void mul33(const float* A, const float* B, float* C) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double sd = 0;
      for (int k = 0; k < 3; k++) sd += (double)A[r * 3 + k] * (double)B[k * 3 + c];
      C[r * 3 + c] = (float)sd;
    }
}

// Ow = -Rcw^T * tcw (KeyFrame::SetPose: Ow = -Rwc * tcw)
ORBX_TRI_FN inline void cameraCentre(const float* pose, float* Ow) {
  for (int r = 0; r < 3; r++) {
    double sd = 0;
    for (int k = 0; k < 3; k++) sd += (double)pose[k * 3 + r] * (double)pose[9 + k];
    Ow[r] = (float)(-1.0 * sd);
  }
}

// cv::norm of a CV_32F 3-vector
ORBX_TRI_FN inline float norm3(float x, float y, float z) {
  return (float)sqrt(((double)x * (double)x + (double)y * (double)y) + (double)z * (double)z);
}

ORBX_TRI_FN inline void pairGeometry(const float* p1, const float* p2, float fx, float fy, float cx, float cy, PairGeom* g) {
  g->nonfinite = 0;
  for (int k = 0; k < 12; k++)
    if (!isFinite(p1[k]) || !isFinite(p2[k])) g->nonfinite = 1;
  for (int k = 0; k < 9; k++) g->F12[k] = 0.0f;
  g->ex = g->ey = g->baseline = 0.0f;
  for (int k = 0; k < 3; k++) g->Ow1[k] = g->Ow2[k] = 0.0f;
  if (g->nonfinite) return;
  // R12 = R1w * R2w^T, t12 = -R12 * t2w + t1w
  float R12[9], t12[3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double sd = 0;
      for (int k = 0; k < 3; k++) sd += (double)p1[r * 3 + k] * (double)p2[c * 3 + k];
      R12[r * 3 + c] = (float)sd;
    }
  for (int r = 0; r < 3; r++) {
    double sd = 0;
    for (int k = 0; k < 3; k++) sd += (double)R12[r * 3 + k] * (double)p2[9 + k];
    t12[r] = (float)(-1.0 * sd + 1.0 * (double)p1[9 + r]);
  }
  // F12 = K^-T * [t12]x * R12 * K^-1, left to right, K^-1 in closed form
  const float invfx = 1.0f / fx, invfy = 1.0f / fy;
  const float Kinv[9] = {invfx, 0.0f, -cx * invfx, 0.0f, invfy, -cy * invfy, 0.0f, 0.0f, 1.0f};
  const float KinvT[9] = {Kinv[0], 0.0f, 0.0f, 0.0f, Kinv[4], 0.0f, Kinv[2], Kinv[5], 1.0f};
  const float tx[9] = {0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f};
  float M1[9], M2[9];
  mul33(KinvT, tx, M1);
  mul33(M1, R12, M2);
  mul33(M2, Kinv, g->F12);
  // the epipole: KF1's centre seen from KF2
  cameraCentre(p1, g->Ow1);
  cameraCentre(p2, g->Ow2);
  float C2[3];
  for (int r = 0; r < 3; r++) {
    double sd = 0;
    for (int k = 0; k < 3; k++) sd += (double)p2[r * 3 + k] * (double)g->Ow1[k];
    C2[r] = (float)(1.0 * sd + 1.0 * (double)p2[9 + r]);
  }
  const float invz = 1.0f / C2[2];
  g->ex = (fx * C2[0]) * invz + cx;
  g->ey = (fy * C2[1]) * invz + cy;
  g->baseline = norm3(g->Ow2[0] - g->Ow1[0], g->Ow2[1] - g->Ow1[1], g->Ow2[2] - g->Ow1[2]);
}

// the epipolar line of KF1's (x1, y1) in KF2: l = x1^T F12
ORBX_TRI_FN inline void epipolarLine(const float* F, float x1, float y1, float* abc) {
  abc[0] = (x1 * F[0] + y1 * F[3]) + F[6];
  abc[1] = (x1 * F[1] + y1 * F[4]) + F[7];
  abc[2] = (x1 * F[2] + y1 * F[5]) + F[8];
}

// a candidate that is near enough in Hamming distance: 0 = passes, 1 = too close to the epipole, 2 = too far from the line.
// epiThr = 100.0f * scale[octave2], lineThr = 3.84f * sigma2[octave2]
ORBX_TRI_FN inline int candidateTest(float ex, float ey, const float* abc, float x2, float y2, float epiThr, float lineThr) {
  const float dx = ex - x2, dy = ey - y2;
  if (dx * dx + dy * dy < epiThr) return 1;
  const float num = (abc[0] * x2 + abc[1] * y2) + abc[2];
  const float den = abc[0] * abc[0] + abc[1] * abc[1];
  if (den == 0.0f) return 2;
  return num * num / den < lineThr ? 0 : 2;
}

// row r of Tcw (R row-major, then t) times (X, 1): gemm's f64 dot, plus t, one rounding
ORBX_TRI_FN inline float camCoord(const float* pose, int r, const float* X) {
  const double sd = ((double)pose[r * 3] * (double)X[0] + (double)pose[r * 3 + 1] * (double)X[1]) + (double)pose[r * 3 + 2] * (double)X[2];
  return (float)(sd + (double)pose[9 + r]);
}

// One match (x1, y1) <-> (x2, y2): the body of CreateNewMapPoints' loop, monocular.  th1 = 5.991f * sigma2[octave1], th2 likewise;
// s1 = scale[octave1], s2 = scale[octave2], ratioFactor = 1.5f * scaleFactor, sLast = scale[nlevels - 1].
ORBX_TRI_FN inline int triangulate(const float* p1, const float* p2, const float* Ow1, const float* Ow2, float fx, float fy, float cx,
                                   float cy, float x1, float y1, float x2, float y2, float th1, float th2, float s1, float s2,
                                   float ratioFactor, float sLast, TriPoint* out) {
  const float invfx = 1.0f / fx, invfy = 1.0f / fy;
  const float xn1[3] = {(x1 - cx) * invfx, (y1 - cy) * invfy, 1.0f};
  const float xn2[3] = {(x2 - cx) * invfx, (y2 - cy) * invfy, 1.0f};
  // ray = Rwc * xn
  float ray1[3], ray2[3];
  for (int r = 0; r < 3; r++) {
    double a = 0, b = 0;
    for (int k = 0; k < 3; k++) {
      a += (double)p1[k * 3 + r] * (double)xn1[k];
      b += (double)p2[k * 3 + r] * (double)xn2[k];
    }
    ray1[r] = (float)a;
    ray2[r] = (float)b;
  }
  const double dot = ((double)ray1[0] * (double)ray2[0] + (double)ray1[1] * (double)ray2[1]) + (double)ray1[2] * (double)ray2[2];
  const double n1 = sqrt(((double)ray1[0] * (double)ray1[0] + (double)ray1[1] * (double)ray1[1]) + (double)ray1[2] * (double)ray1[2]);
  const double n2 = sqrt(((double)ray2[0] * (double)ray2[0] + (double)ray2[1] * (double)ray2[1]) + (double)ray2[2] * (double)ray2[2]);
  const float cosRays = (float)(dot / (n1 * n2));
  if (!(cosRays > 0.0f && cosRays < 0.9998f)) return TRI_LOW_PARALLAX;
  // A = [xn1.x * T1.row(2) - T1.row(0); xn1.y * T1.row(2) - T1.row(1); the same for camera 2], CV_32F
  double A[16];
  for (int k = 0; k < 4; k++) {
    const float r10 = k < 3 ? p1[k] : p1[9], r11 = k < 3 ? p1[3 + k] : p1[10], r12 = k < 3 ? p1[6 + k] : p1[11];
    const float r20 = k < 3 ? p2[k] : p2[9], r21 = k < 3 ? p2[3 + k] : p2[10], r22 = k < 3 ? p2[6 + k] : p2[11];
    A[0 * 4 + k] = (double)(xn1[0] * r12 - r10);
    A[1 * 4 + k] = (double)(xn1[1] * r12 - r11);
    A[2 * 4 + k] = (double)(xn2[0] * r22 - r20);
    A[3 * 4 + k] = (double)(xn2[1] * r22 - r21);
  }
  double xd[4];
  smallestRightSingularVector4(A, xd);
  const float X0 = (float)xd[0], X1 = (float)xd[1], X2 = (float)xd[2], X3 = (float)xd[3];
  if (X3 == 0.0f || !isFinite(X0) || !isFinite(X1) || !isFinite(X2) || !isFinite(X3)) return TRI_W_ZERO;
  float* X = out->X;
  X[0] = X0 / X3;
  X[1] = X1 / X3;
  X[2] = X2 / X3;
  if (!isFinite(X[0]) || !isFinite(X[1]) || !isFinite(X[2])) return TRI_W_ZERO;
  const float z1 = camCoord(p1, 2, X);
  if (!(z1 > 0.0f)) return TRI_BEHIND_1;
  const float z2 = camCoord(p2, 2, X);
  if (!(z2 > 0.0f)) return TRI_BEHIND_2;
  {
    const float xc = camCoord(p1, 0, X), yc = camCoord(p1, 1, X), invz = 1.0f / z1;
    const float u = (fx * xc) * invz + cx, v = (fy * yc) * invz + cy;
    const float eX = u - x1, eY = v - y1;
    if (!(eX * eX + eY * eY <= th1)) return TRI_REPROJ_1;
  }
  {
    const float xc = camCoord(p2, 0, X), yc = camCoord(p2, 1, X), invz = 1.0f / z2;
    const float u = (fx * xc) * invz + cx, v = (fy * yc) * invz + cy;
    const float eX = u - x2, eY = v - y2;
    if (!(eX * eX + eY * eY <= th2)) return TRI_REPROJ_2;
  }
  const float d1[3] = {X[0] - Ow1[0], X[1] - Ow1[1], X[2] - Ow1[2]};
  const float d2[3] = {X[0] - Ow2[0], X[1] - Ow2[1], X[2] - Ow2[2]};
  const float dist1 = norm3(d1[0], d1[1], d1[2]), dist2 = norm3(d2[0], d2[1], d2[2]);
  if (dist1 == 0.0f || dist2 == 0.0f) return TRI_ZERO_DIST;
  const float ratioDist = dist2 / dist1, ratioOctave = s1 / s2;
  if (!(ratioDist * ratioFactor >= ratioOctave && ratioDist <= ratioOctave * ratioFactor)) return TRI_SCALE;
  // MapPoint::UpdateNormalAndDepth with two observations, KF1 the reference keyframe
  for (int k = 0; k < 3; k++) out->normal[k] = (d1[k] / dist1 + d2[k] / dist2) / 2.0f;
  out->maxDist = dist1 * s1;
  out->minDist = out->maxDist / sLast;
  return TRI_KEPT;
}

}  // namespace orbx_tri
