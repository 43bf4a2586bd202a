// sim3_ref.cpp — CPU restatement of Sim3Solver (include/orbx.h, "loop closing: Sim3 RANSAC"), TEST INFRASTRUCTURE: built by
// tests/sim3_ref_lib.py with g++ -O2 -ffp-contract=off.  The arithmetic is orb_slam_tracking_amd/csrc/orbx_sim3_math.inc, the
// include the device kernels compile too; this file restates on its own what surrounds it: the constructor's checks and order,
// and iterate() twice -- the literal sequential loop with its early return, and "all hypotheses, then the rule in iteration
// order" as the device resolves it.  SetRansacParameters' table comes from the caller.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbx.h"

#define ORBX_SIM3_FN
#include "../../orb_slam_tracking_amd/csrc/orbx_sim3_math.inc"

using namespace orbx_sim3;

namespace {

struct Solver {
  std::vector<Corr> corr;
  std::vector<int32_t> corrOf;
  Cam K;
  int N = 0, status = 0;

  // the constructor: the correspondences in ascending order of KF1's feature, garbage flagged and not followed
  Solver(const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, int cap, const int32_t* match, const float* points1,
         const uint8_t* mask1, const float* points2, const uint8_t* mask2, const float* pose1, const float* pose2, const float* Kf,
         const float* sigma2, int nLevels, float th2) {
    K = Cam{Kf[0], Kf[4], Kf[2], Kf[5]};
    corrOf.assign(cap, -1);
    if (n1 < 0 || n1 > cap || n2 < 0 || n2 > cap) {
      status |= SIM3_BAD_INPUT;
      n1 = 0;
    }
    for (int k = 0; k < 12; k++)
      if (!std::isfinite(pose1[k]) || !std::isfinite(pose2[k])) status |= SIM3_NONFINITE;
    for (int i1 = 0; i1 < n1; i1++) {
      const int i2 = match[i1];
      if (i2 >= n2) {
        status |= SIM3_BAD_INPUT;
        continue;
      }
      if (i2 < 0) continue;
      if (mask1 && (mask1[i1] == 0 || mask2[i2] == 0)) continue;
      const int o1 = kps1[i1].octave, o2 = kps2[i2].octave;
      if (o1 < 0 || o1 >= nLevels || o2 < 0 || o2 >= nLevels) {
        status |= SIM3_BAD_INPUT;
        continue;
      }
      Corr c{};
      const float *X1 = points1 + (size_t)i1 * 3, *X2 = points2 + (size_t)i2 * 3;
      toCamera(pose1, X1, c.X1);
      toCamera(pose2, X2, c.X2);
      toImage(c.X1, K, c.p1);
      toImage(c.X2, K, c.p2);
      c.maxErr1 = th2 * sigma2[o1];
      c.maxErr2 = th2 * sigma2[o2];
      c.i1 = i1;
      c.i2 = i2;
      bool fin = std::isfinite(kps1[i1].x) && std::isfinite(kps1[i1].y) && std::isfinite(kps2[i2].x) && std::isfinite(kps2[i2].y);
      for (int k = 0; k < 3; k++) fin = fin && std::isfinite(X1[k]) && std::isfinite(X2[k]);
      if (!fin) {
        status |= SIM3_NONFINITE;
        continue;
      }
      corrOf[i1] = (int)corr.size();
      corr.push_back(c);
    }
    N = status ? 0 : (int)corr.size();
    if (status) corr.clear();
  }

  int checkInliers(const Sim3Pair& T, std::vector<uint8_t>* in) const {
    int count = 0;
    in->assign(corr.size(), 0);
    for (size_t c = 0; c < corr.size(); c++)
      if (isInlier(T, corr[c], K)) {
        (*in)[c] = 1;
        count++;
      }
    return count;
  }

  Hyp hyp(const int32_t* draws, bool fixScale) const {
    Hyp h;
    Sim3Pair T;
    if (hypothesis(draws, corr.data(), N, fixScale, &h, &T)) {
      std::vector<uint8_t> in;
      h.count = checkInliers(T, &in);
    }
    return h;
  }
};

}  // namespace

extern "C" {

// mode 0: the literal sequential loop; mode 1: every hypothesis first, then rule 6 in iteration order.  table [cap + 1].
void s3r_solve(const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, int cap, const int32_t* match,
               const float* points1, const uint8_t* mask1, const float* points2, const uint8_t* mask2, const float* pose1,
               const float* pose2, const float* Kf, const float* sigma2, int nLevels, const int32_t* table, int fixScale, int minInliers,
               float th2, int nIter, const int32_t* draws, int mode, orbx_sim3_result* res, float* sim3, int32_t* row,
               uint8_t* inliers) {
  Solver S(kps1, n1, kps2, n2, cap, match, points1, mask1, points2, mask2, pose1, pose2, Kf, sigma2, nLevels, th2);
  const int maxIts = table[S.N];
  int status = S.status;
  if (status == 0 && S.N < minInliers) status = SIM3_FEW_POINTS;
  Outcome o{};
  o.foundIt = o.bestIt = -1;
  Hyp result{};
  if (status == 0) {
    const int nIts = nIter < maxIts ? nIter : maxIts;
    if (mode == 0) {
      // iterate(): mnBestInliers carries over; the first hypothesis that becomes the best above minInliers returns
      int mnBestInliers = 0;
      o.itsRun = nIts;
      for (int it = 0; it < nIts; it++) {
        const Hyp h = S.hyp(draws + (size_t)it * 3, fixScale != 0);
        if (h.flags & HYP_DEGENERATE) o.nDegenerate++;
        if (h.flags & HYP_BAD_DRAWS) o.badDraws = 1;
        if (h.flags) continue;
        if (h.count >= mnBestInliers) {
          mnBestInliers = h.count;
          o.bestIt = it;
          if (h.count > minInliers) {
            o.foundIt = it;
            o.itsRun = it + 1;
            result = h;
            break;
          }
        }
      }
      o.nBestInliers = mnBestInliers;
    } else {
      std::vector<Hyp> hyp(nIts);
      for (int it = 0; it < nIts; it++) hyp[it] = S.hyp(draws + (size_t)it * 3, fixScale != 0);
      resolveIterations(hyp.data(), nIts, minInliers, &o);
      if (o.foundIt >= 0) result = hyp[o.foundIt];
    }
    if (o.badDraws) status |= SIM3_BAD_DRAWS;
  }
  const bool have = o.foundIt >= 0;
  if (!have) status |= SIM3_NO_RESULT;
  std::vector<uint8_t> in;
  int nIn = 0;
  if (have) {
    Sim3Pair T;
    (void)pairOf(result.sim, &T);
    nIn = S.checkInliers(T, &in);
  }
  for (int j = 0; j < cap; j++) {
    const int c = have ? S.corrOf[j] : -1;
    const bool isIn = c >= 0 && in[c];
    row[j] = isIn ? S.corr[c].i2 : -1;
    if (inliers) inliers[j] = isIn ? 1 : 0;
  }
  const bool counted = (status & (SIM3_BAD_INPUT | SIM3_NONFINITE)) == 0;
  std::memset(res, 0, sizeof *res);
  res->status = status;
  res->n_correspondences = counted ? S.N : 0;
  res->max_its = maxIts;
  res->its_run = o.itsRun;
  res->found_it = o.foundIt;
  res->best_it = o.bestIt;
  res->n_inliers = nIn;
  res->n_best_inliers = o.nBestInliers;
  res->n_degenerate = o.nDegenerate;
  for (int k = 0; k < 13; k++) sim3[k] = have ? result.sim[k] : 0.f;
  res->s12 = sim3[12];
  for (int k = 0; k < 9; k++) res->R12[k] = sim3[k];
  for (int k = 0; k < 3; k++) res->t12[k] = sim3[9 + k];
}

// every hypothesis of a problem on its own -> counts [nIter], flags [nIter], sims [nIter][13]; returns N (-1: refused)
int s3r_hypotheses(const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, int cap, const int32_t* match,
                   const float* points1, const uint8_t* mask1, const float* points2, const uint8_t* mask2, const float* pose1,
                   const float* pose2, const float* Kf, const float* sigma2, int nLevels, int fixScale, float th2, int nIter,
                   const int32_t* draws, int32_t* counts, int32_t* flags, float* sims) {
  Solver S(kps1, n1, kps2, n2, cap, match, points1, mask1, points2, mask2, pose1, pose2, Kf, sigma2, nLevels, th2);
  if (S.status || S.N < 3) return -1;
  for (int it = 0; it < nIter; it++) {
    const Hyp h = S.hyp(draws + (size_t)it * 3, fixScale != 0);
    counts[it] = h.count;
    flags[it] = h.flags;
    std::memcpy(sims + (size_t)it * 13, h.sim, sizeof h.sim);
  }
  return S.N;
}

// the constructor's arrays and CheckInliers' errors under a similarity sim [13] (R12, t12, s12), per correspondence: i1, i2,
// err [4] = err1, err2, maxErr1, maxErr2 (f32, as rule 5 computes them), X [6] = mvX3Dc1, mvX3Dc2.  Returns N (-1: refused).
int s3r_errors(const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, int cap, const int32_t* match, const float* points1,
               const uint8_t* mask1, const float* points2, const uint8_t* mask2, const float* pose1, const float* pose2, const float* Kf,
               const float* sigma2, int nLevels, float th2, const float* sim, int32_t* i1, int32_t* i2, float* err, float* X,
               uint8_t* in) {
  Solver S(kps1, n1, kps2, n2, cap, match, points1, mask1, points2, mask2, pose1, pose2, Kf, sigma2, nLevels, th2);
  if (S.status) return -1;
  Sim3Pair T;
  const bool fin = pairOf(sim, &T);
  for (int c = 0; c < S.N; c++) {
    const Corr& k = S.corr[c];
    i1[c] = k.i1;
    i2[c] = k.i2;
    float P[3], uv[2];
    for (int r = 0; r < 3; r++) P[r] = T.sR12[3 * r] * k.X2[0] + T.sR12[3 * r + 1] * k.X2[1] + T.sR12[3 * r + 2] * k.X2[2] + T.t12[r];
    toImage(P, S.K, uv);
    const float ax = k.p1[0] - uv[0], ay = k.p1[1] - uv[1];
    err[4 * c] = ax * ax + ay * ay;
    for (int r = 0; r < 3; r++) P[r] = T.sR21[3 * r] * k.X1[0] + T.sR21[3 * r + 1] * k.X1[1] + T.sR21[3 * r + 2] * k.X1[2] + T.t21[r];
    toImage(P, S.K, uv);
    const float bx = uv[0] - k.p2[0], by = uv[1] - k.p2[1];
    err[4 * c + 1] = bx * bx + by * by;
    err[4 * c + 2] = k.maxErr1;
    err[4 * c + 3] = k.maxErr2;
    for (int r = 0; r < 3; r++) {
      X[6 * c + r] = k.X1[r];
      X[6 * c + 3 + r] = k.X2[r];
    }
    in[c] = fin && isInlier(T, k, S.K) ? 1 : 0;
  }
  return S.N;
}

// the sampler alone: three draws on a list of N -> sel[3]; returns 1, or 0 for a draw out of range
int s3r_sample(const int32_t* draws, int N, int32_t* sel) {
  int s[3] = {0, 0, 0};
  const bool ok = orbx_pnp::sampleDraws<3>(draws, N, s);
  for (int i = 0; i < 3; i++) sel[i] = s[i];
  return ok ? 1 : 0;
}

// Horn's solution alone: P1, P2 [3 points][3] f64 -> R [9], t [3], s
void s3r_horn(const double* P1, const double* P2, int fixScale, double* R, double* t, double* s) {
  double A[3][3], B[3][3];
  for (int k = 0; k < 3; k++)
    for (int i = 0; i < 3; i++) {
      A[k][i] = P1[3 * k + i];
      B[k][i] = P2[3 * k + i];
    }
  hornSim3(A, B, fixScale != 0, R, t, s);
}

// the eigenvector of the largest signed eigenvalue of a symmetric 4x4 (row-major) -> q [4]; returns the eigenvalue
double s3r_eig_top(const double* Nin, double* q) {
  double A[4][4];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) A[i][j] = Nin[4 * i + j];
  return eigTop4(A, q);
}

int s3r_result_size() { return (int)sizeof(orbx_sim3_result); }

}  // extern "C"

// ======== ORBmatcher::SearchBySim3 (include/orbx.h, "loop closing: matching under a similarity") ================================
// The literal statements: rule 1, the two loops over the points and the agreement loop, with the keyframe's grid of
// SlamTypes/Frame.cpp as vectors per cell.  Nothing here is shared with the library.
namespace {

const int GRID_COLS = 64, GRID_ROWS = 48;
const int MSIM3_BAD_INPUT = 2, MSIM3_NONFINITE = 4;

struct Grid {
  std::vector<int> cell[GRID_COLS][GRID_ROWS];
  float minX, minY, wInv, hInv;
  const orbx_keypoint* kps;

  Grid(const orbx_keypoint* k, int n, const int32_t* b) : kps(k) {
    minX = static_cast<float>(b[0]);
    minY = static_cast<float>(b[2]);
    wInv = static_cast<float>(GRID_COLS) / static_cast<float>(b[1] - b[0]);
    hInv = static_cast<float>(GRID_ROWS) / static_cast<float>(b[3] - b[2]);
    for (int i = 0; i < n; i++) {
      const float px = roundf((k[i].x - minX) * wInv), py = roundf((k[i].y - minY) * hInv);
      if (!(px >= 0.0f && px < GRID_COLS && py >= 0.0f && py < GRID_ROWS)) continue;
      cell[(int)px][(int)py].push_back(i);
    }
  }
  // KeyFrame::GetFeaturesInArea(x, y, r): no level bounds
  std::vector<int> area(float x, float y, float r) const {
    std::vector<int> out;
    const float lox = floorf((x - minX - r) * wInv), hix = ceilf((x - minX + r) * wInv);
    const float loy = floorf((y - minY - r) * hInv), hiy = ceilf((y - minY + r) * hInv);
    if (lox >= GRID_COLS) return out;
    const int x0 = lox < 0.0f ? 0 : (int)lox;
    if (hix < 0.0f) return out;
    const int x1 = hix > GRID_COLS - 1 ? GRID_COLS - 1 : (int)hix;
    if (loy >= GRID_ROWS) return out;
    const int y0 = loy < 0.0f ? 0 : (int)loy;
    if (hiy < 0.0f) return out;
    const int y1 = hiy > GRID_ROWS - 1 ? GRID_ROWS - 1 : (int)hiy;
    for (int ix = x0; ix <= x1; ix++)
      for (int iy = y0; iy <= y1; iy++)
        for (int j : cell[ix][iy]) {
          const float dx = kps[j].x - x, dy = kps[j].y - y;
          if (fabsf(dx) < r && fabsf(dy) < r) out.push_back(j);
        }
    return out;
  }
};

int hamming(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

struct KeyFrame {
  const orbx_keypoint* kps;
  const uint8_t* desc;
  int n;
  const float *points, *dists;
  const uint8_t *mask, *pointDesc;
  const float* pose;
};

// One direction: the points of A that `skip` does not hold, searched in B under p_B = M * p_A + tv.  vnMatch [A.n]; cnt [6]:
// points, behind, out of the image, out of distance, with candidates, over orb_dist.  proj (nullable) [A.n][5]: u, v, radius,
// level, stage (0 none, 1 behind, 2 image, 3 distance, 5 searched).
void direction(const KeyFrame& A, const KeyFrame& B, const std::vector<char>& skip, const float* M, const float* tv, const float* K,
               const int32_t* bounds, const float* scale, int nLevels, float th, int orbDist, std::vector<int>& vnMatch, int32_t* cnt,
               int32_t* status, float* proj) {
  const Grid grid(B.kps, B.n, bounds);
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const float minX = static_cast<float>(bounds[0]), maxX = static_cast<float>(bounds[1]);
  const float minY = static_cast<float>(bounds[2]), maxY = static_cast<float>(bounds[3]);
  const float* R = A.pose;
  const float* t = A.pose + 9;
  for (int i = 0; i < A.n; i++) {
    if (proj) for (int k = 0; k < 5; k++) proj[5 * i + k] = 0.0f;
    if (A.mask && A.mask[i] == 0) continue;
    if (skip[i]) continue;
    cnt[0]++;
    const float* P = A.points + 3 * (size_t)i;
    const float minDist = A.dists[2 * (size_t)i], maxDist = A.dists[2 * (size_t)i + 1];
    bool fin = std::isfinite(minDist) && std::isfinite(maxDist);
    for (int k = 0; k < 3; k++) fin = fin && std::isfinite(P[k]);
    if (!fin) {
      *status |= MSIM3_NONFINITE;
      continue;
    }
    const float ax = ((R[0] * P[0] + R[1] * P[1]) + R[2] * P[2]) + t[0];
    const float ay = ((R[3] * P[0] + R[4] * P[1]) + R[5] * P[2]) + t[1];
    const float az = ((R[6] * P[0] + R[7] * P[1]) + R[8] * P[2]) + t[2];
    const float x = ((M[0] * ax + M[1] * ay) + M[2] * az) + tv[0];
    const float y = ((M[3] * ax + M[4] * ay) + M[5] * az) + tv[1];
    const float z = ((M[6] * ax + M[7] * ay) + M[8] * az) + tv[2];
    if (z < 0.0f) {
      cnt[1]++;
      if (proj) proj[5 * i + 4] = 1.0f;
      continue;
    }
    const float invz = 1.0f / z;
    const float u = fx * (x * invz) + cx, v = fy * (y * invz) + cy;
    if (!(std::isfinite(u) && std::isfinite(v) && u >= minX && u < maxX && v >= minY && v < maxY)) {
      cnt[2]++;
      if (proj) proj[5 * i + 4] = 2.0f;
      continue;
    }
    const float dist3D = static_cast<float>(std::sqrt(((double)x * x + (double)y * y) + (double)z * z));
    if (proj) { proj[5 * i] = u; proj[5 * i + 1] = v; }
    if (dist3D < 0.8f * minDist || dist3D > 1.2f * maxDist) {
      cnt[3]++;
      if (proj) proj[5 * i + 4] = 3.0f;
      continue;
    }
    const float ratio = maxDist / dist3D;
    if (ratio != ratio) {
      *status |= MSIM3_NONFINITE;
      continue;
    }
    int level = 0;
    for (int n = 0; n < nLevels - 1; n++)
      if (ratio > scale[n]) level++;
    const float radius = th * scale[level];
    if (proj) { proj[5 * i + 2] = radius; proj[5 * i + 3] = (float)level; proj[5 * i + 4] = 5.0f; }
    const std::vector<int> vIndices = grid.area(u, v, radius);
    const uint8_t* dMP = A.pointDesc ? A.pointDesc + 32 * (size_t)i : A.desc + 32 * (size_t)i;
    int bestDist = INT32_MAX, bestIdx = -1, inWindow = 0;
    for (int idx : vIndices) {
      const orbx_keypoint& kp = B.kps[idx];
      if (kp.octave < level - 1 || kp.octave > level) continue;
      inWindow++;
      const int dist = hamming(dMP, B.desc + 32 * (size_t)idx);
      if (dist < bestDist) {
        bestDist = dist;
        bestIdx = idx;
      }
    }
    if (!inWindow) continue;
    cnt[4]++;
    if (bestDist <= orbDist) vnMatch[i] = bestIdx;
    else cnt[5]++;
  }
}

}  // namespace

extern "C" {

// One pair; pointDesc1 / 2 and mask1 / 2 nullable; res [16] in the order of orbx_msim3_result; matches [n1] in and out; vn1 [n1],
// vn2 [n2], proj1 [n1][5], proj2 [n2][5] nullable.
void s3r_search_by_sim3(const orbx_keypoint* kps1, const uint8_t* desc1, int n1, const float* points1, const uint8_t* mask1,
                        const uint8_t* pointDesc1, const float* dists1, const float* pose1, const orbx_keypoint* kps2,
                        const uint8_t* desc2, int n2, const float* points2, const uint8_t* mask2, const uint8_t* pointDesc2,
                        const float* dists2, const float* pose2, const float* sim, const float* K, const int32_t* bounds,
                        const float* scale, int nLevels, float th, int orbDist, int32_t* matches, int32_t* res, int32_t* vn1,
                        int32_t* vn2, float* proj1, float* proj2) {
  for (int c = 0; c < 16; c++) res[c] = 0;
  const KeyFrame KF1{kps1, desc1, n1, points1, dists1, mask1, pointDesc1, pose1}, KF2{kps2, desc2, n2, points2, dists2, mask2, pointDesc2, pose2};
  // rule 1
  std::vector<char> vbAlreadyMatched1(n1 > 0 ? n1 : 1, 0), vbAlreadyMatched2(n2 > 0 ? n2 : 1, 0);
  for (int i1 = 0; i1 < n1; i1++) {
    const int i2 = matches[i1];
    if (i2 < 0) continue;
    vbAlreadyMatched1[i1] = 1;
    if (i2 >= n2) res[0] |= MSIM3_BAD_INPUT;
    else vbAlreadyMatched2[i2] = 1;
  }
  std::vector<int> vnMatch1(n1 > 0 ? n1 : 1, -1), vnMatch2(n2 > 0 ? n2 : 1, -1);
  const float s12 = sim[12];
  bool ok = std::isfinite(s12) && s12 > 0.0f;
  for (int k = 0; k < 12; k++) ok = ok && std::isfinite(sim[k]) && std::isfinite(pose1[k]) && std::isfinite(pose2[k]);
  if (!ok) {
    res[0] |= MSIM3_NONFINITE;
  } else {
    float sR12[9], sR21[9], t21[3];
    const float* t12 = sim + 9;
    const double inv = 1.0 / (double)s12;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        sR12[3 * i + j] = s12 * sim[3 * i + j];
        sR21[3 * i + j] = (float)(inv * (double)sim[3 * j + i]);
      }
    for (int i = 0; i < 3; i++) t21[i] = -((sR21[3 * i] * t12[0] + sR21[3 * i + 1] * t12[1]) + sR21[3 * i + 2] * t12[2]);
    direction(KF1, KF2, vbAlreadyMatched1, sR21, t21, K, bounds, scale, nLevels, th, orbDist, vnMatch1, res + 2, res, proj1);  // rule 2
    direction(KF2, KF1, vbAlreadyMatched2, sR12, t12, K, bounds, scale, nLevels, th, orbDist, vnMatch2, res + 8, res, proj2);  // rule 3
    // rule 4
    for (int i1 = 0; i1 < n1; i1++) {
      const int i2 = vnMatch1[i1];
      if (i2 < 0) continue;
      if (vnMatch2[i2] == i1) {
        matches[i1] = i2;
        res[1]++;
      } else {
        res[14]++;
      }
    }
  }
  for (int i = 0; i < n1 && vn1; i++) vn1[i] = vnMatch1[i];
  for (int i = 0; i < n2 && vn2; i++) vn2[i] = vnMatch2[i];
}

int s3r_features_in_area(const orbx_keypoint* kps, int n, const int32_t* bounds, float x, float y, float r, int32_t* out) {
  const Grid g(kps, n, bounds);
  const std::vector<int> c = g.area(x, y, r);
  for (size_t k = 0; k < c.size(); k++) out[k] = c[k];
  return (int)c.size();
}

int s3r_msim3_result_size() { return (int)sizeof(orbx_msim3_result); }

}  // extern "C"
