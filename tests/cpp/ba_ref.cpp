// ba_ref.cpp — CPU restatement of the two-view bundle adjustment (include/orbx.h, "behind the Initializer: two-view bundle
// adjustment"), TEST INFRASTRUCTURE: built by tests/ba_ref_lib.py with g++ -O2 -ffp-contract=off.  The arithmetic is
// orb_slam_tracking_amd/csrc/orbx_ba_math.inc, the include the device kernel compiles too; this file restates on its own the rules
// around it: the checks of the inputs, the point list, the order of the sums of deviation 1 (256 lanes, each walking its points in
// turn, the shuffle tree inside a wave of 64, the waves in order), the loops of solve() and optimize(), the median and the
// normalisation.  Beyond the result it reports counters that show which branches a world ran.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbx.h"

#define ORBX_BA_FN
#include "../../orb_slam_tracking_amd/csrc/orbx_ba_math.inc"

using namespace orbx_ba;

namespace {

constexpr int LANES = 256, WAVE = 64;

// the lanes' sums of `n` quantities folded as the device folds them
void fold(const std::vector<double>& acc, int n, double* sum) {
  for (int k = 0; k < n; k++) {
    double total = 0.0;
    for (int w = 0; w < LANES / WAVE; w++) {
      double v[WAVE];
      for (int l = 0; l < WAVE; l++) v[l] = acc[(size_t)(w * WAVE + l) * BA_ACC_MAX + k];
      for (int off = WAVE / 2; off >= 1; off >>= 1)
        for (int l = 0; l < off; l++) v[l] = v[l] + v[l + off];
      total = w == 0 ? v[0] : total + v[0];
    }
    sum[k] = total;
  }
}

struct Point {
  double X[3], Xb[3], Hll[6], bl[3], Hpl[18];
  float obs[6];
  int i;
};

struct Problem {
  std::vector<Point> pts;
  Pose T;
  Cam K;
  double delta;
};

double deltaHuber() { return (double)(float)std::sqrt(5.99); }

// buildSystem over every point; returns the largest |diagonal entry| of the points' blocks
double build(Problem& P, double* sum, Counters* cnt) {
  std::vector<double> acc((size_t)LANES * BA_ACC_MAX, 0.0);
  double R[3][3];
  quatToMatrix(P.T.q, R);
  double maxd = 0.0;
  for (size_t j = 0; j < P.pts.size(); j++) {
    Point& q = P.pts[j];
    cnt->huberOutliers += pointBuild(P.T, R, q.X, q.obs, P.K, P.delta, q.Hll, q.bl, q.Hpl, &acc[(j % LANES) * BA_ACC_MAX]);
    for (int k : {0, 3, 5}) maxd = std::max(maxd, std::fabs(q.Hll[k]));
  }
  fold(acc, BA_ACC_BUILD, sum);
  return maxd;
}

void schur(Problem& P, double lambda, double* sum) {
  std::vector<double> acc((size_t)LANES * BA_ACC_MAX, 0.0);
  for (size_t j = 0; j < P.pts.size(); j++) {
    Point& q = P.pts[j];
    for (int c = 0; c < 3; c++) q.Xb[c] = q.X[c];
    pointSchur(q.Hll, q.bl, q.Hpl, lambda, &acc[(j % LANES) * BA_ACC_MAX]);
  }
  fold(acc, BA_ACC_SCHUR, sum);
}

void step(Problem& P, double lambda, const double* xp, double* sum, double* xlOut) {
  std::vector<double> acc((size_t)LANES * BA_ACC_MAX, 0.0);
  for (size_t j = 0; j < P.pts.size(); j++) {
    Point& q = P.pts[j];
    double xl[3];
    pointStep(q.Hll, q.bl, q.Hpl, lambda, xp, q.X, xl, &acc[(j % LANES) * BA_ACC_MAX]);
    if (xlOut)
      for (int c = 0; c < 3; c++) xlOut[j * 3 + c] = xl[c];
    pointChi2(P.T, q.X, q.obs, P.K, P.delta, &acc[(j % LANES) * BA_ACC_MAX + BA_ACC_TCHI2]);
  }
  fold(acc, BA_ACC_TRIAL, sum);
}

void startLm(Lm* m) {
  std::memset(m, 0, sizeof *m);
  m->ni = 2.0;
}

// one trial of solve()'s loop; returns whether it was accepted
int trial(Problem& P, Lm* m, Counters* cnt, double* xlOut) {
  double sum[BA_ACC_MAX];
  const double lambda = m->lambda;
  schur(P, lambda, sum);
  const Pose backup = P.T;
  m->ok = lmSolvePose(m, sum + BA_ACC_S, sum + BA_ACC_COEF) ? 1 : 0;
  double tchi = 0.0, scale = 0.0;
  if (!m->ok) {
    m->solverFailures++;
  } else {
    if (poseOplus(m->xp, &P.T)) cnt->smallTheta++;
    step(P, lambda, m->xp, sum, xlOut);
    tchi = sum[BA_ACC_TCHI2];
    scale = sum[BA_ACC_SCALE];
  }
  const int accepted = lmJudge(m, tchi, scale, cnt);
  if (!accepted) {
    P.T = backup;
    if (m->ok)
      for (Point& q : P.pts)
        for (int c = 0; c < 3; c++) q.X[c] = q.Xb[c];
  }
  return accepted;
}

// the start of solve(): errors, chi2, the linearisation, lambda at iteration 0
void linearise(Problem& P, Lm* m, Counters* cnt, int it, double* chi2Initial) {
  double sum[BA_ACC_MAX];
  const double maxd = build(P, sum, cnt);
  for (int k = 0; k < 21; k++) m->Hpp[k] = sum[BA_ACC_HPP + k];
  for (int k = 0; k < 6; k++) m->bp[k] = sum[BA_ACC_BP + k];
  m->currentChi = m->iniChi = sum[BA_ACC_CHI2];
  if (it == 0) {
    *chi2Initial = m->currentChi;
    m->lambda = lmLambdaInit(m->Hpp, maxd);
    m->ni = 2.0;
    m->nBad = 0;
  }
  m->rho = 0.0;
  m->qmax = 0;
}

struct Inputs {
  const orbx_keypoint *k1, *k2;
  int n1, n2, cap;
  const int32_t* m12;
  const orbx_init_result* ir;
  const float* p3d;
  const uint8_t* tri;
  const float* K;
  const float* invSigma2;
  int nLevels;
};

// the checks and the point list -> status bits; the problem is filled when they are 0
int gather(const Inputs& in, Problem& P, int* nPts) {
  *nPts = 0;
  if (in.ir->status != 0) return ORBX_BA_SKIPPED;
  int st = 0;
  if (in.n1 < 0 || in.n1 > in.cap || in.n2 < 0 || in.n2 > in.cap) st |= ORBX_BA_BAD_INPUT;
  for (int i = 0; i < 9; i++)
    if (!isFiniteF(in.ir->R21[i])) st |= ORBX_BA_NONFINITE;
  for (int i = 0; i < 3; i++)
    if (!isFiniteF(in.ir->t21[i])) st |= ORBX_BA_NONFINITE;
  if (st) return st;
  for (int i = 0; i < in.n1; i++) {
    const int m = in.m12[i];
    if (m >= in.n2) {
      st |= ORBX_BA_BAD_INPUT;
      continue;
    }
    if (m < 0 || !in.tri[i]) continue;
    const int o1 = in.k1[i].octave, o2 = in.k2[m].octave;
    if (o1 < 0 || o1 >= in.nLevels || o2 < 0 || o2 >= in.nLevels) {
      st |= ORBX_BA_BAD_INPUT;
      continue;
    }
    Point q{};
    q.i = i;
    for (int c = 0; c < 3; c++) {
      const float v = in.p3d[(size_t)i * 3 + c];
      if (!isFiniteF(v)) st |= ORBX_BA_NONFINITE;
      q.X[c] = (double)v;
    }
    q.obs[0] = in.k1[i].x; q.obs[1] = in.k1[i].y;
    q.obs[2] = in.k2[m].x; q.obs[3] = in.k2[m].y;
    q.obs[4] = in.invSigma2[o1]; q.obs[5] = in.invSigma2[o2];
    P.pts.push_back(q);
  }
  *nPts = (int)P.pts.size();
  P.K = Cam{(double)in.K[0], (double)in.K[4], (double)in.K[2], (double)in.K[5]};
  P.delta = deltaHuber();
  if (st == 0) poseFromRt(in.ir->R21, in.ir->t21, &P.T);
  return st;
}

}  // namespace

extern "C" {

// The whole call for one pair.  counters: accepted trials, rejected trials, edges in Huber's outlier branch (summed over every
// linearisation), uses of the theta < 1e-5 branch.
void bar_bundle_adjust(const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, int cap, const int32_t* m12,
                       const orbx_init_result* ir, const float* p3d, const uint8_t* tri, const float* K, const float* invSigma2,
                       int nLevels, int nIterations, int minPoints, int normalize, orbx_ba_result* out, float* p3dOut,
                       int64_t* counters) {
  const Inputs in{k1, k2, n1, n2, cap, m12, ir, p3d, tri, K, invSigma2, nLevels};
  Problem P;
  Counters cnt{0, 0, 0, 0};
  Lm m;
  startLm(&m);
  int nPts = 0;
  int status = gather(in, P, &nPts);
  double chi2Initial = 0.0;
  if (status == 0 && nPts > 0) {
    for (int it = 0; it < nIterations; it++) {
      linearise(P, &m, &cnt, it, &chi2Initial);
      do {
        trial(P, &m, &cnt, nullptr);
      } while (lmAnotherTrial(&m));
      const int r = lmEndIteration(&m);
      m.iterations++;
      m.stopReason = r;
      if (r) break;
    }
  }
  bool optimised = status == 0;
  std::vector<float> Xf((size_t)nPts * 3);
  if (optimised) {
    bool fin = isFinite(chi2Initial) && isFinite(m.currentChi) && isFinite(m.lambda);
    for (int k = 0; k < 4; k++) fin = fin && isFinite(P.T.q[k]);
    for (int k = 0; k < 3; k++) fin = fin && isFinite(P.T.t[k]);
    for (int j = 0; j < nPts; j++)
      for (int c = 0; c < 3; c++) {
        fin = fin && isFinite(P.pts[j].X[c]);
        Xf[(size_t)j * 3 + c] = (float)P.pts[j].X[c];
      }
    if (!fin) {
      status |= ORBX_BA_NONFINITE;
      optimised = false;
    }
  }
  float median = 0.f, inv = 1.f;
  bool scaled = false;
  if (optimised) {
    if (nPts > 0) {  // ComputeSceneMedianDepth: sort, element (n - 1) / 2
      std::vector<float> z(nPts);
      for (int j = 0; j < nPts; j++) z[j] = Xf[(size_t)j * 3 + 2];
      std::stable_sort(z.begin(), z.end());
      median = z[(nPts - 1) / 2];
    }
    if (nPts < minPoints) status |= ORBX_BA_FEW_POINTS;
    if (nPts > 0 && median < 0.f) status |= ORBX_BA_NEGATIVE_DEPTH;
    if (normalize && status == 0 && median > 0.f) {
      inv = 1.0f / median;
      scaled = true;
    }
  }
  std::memmove(p3dOut, p3d, (size_t)cap * 12);
  std::memset(out, 0, sizeof *out);
  out->status = status;
  out->n_points = (status & (ORBX_BA_SKIPPED | ORBX_BA_BAD_INPUT)) ? 0 : nPts;
  out->iterations = m.iterations;
  out->lm_trials = m.lmTrials;
  out->rejected_trials = m.rejected;
  out->solver_failures = m.solverFailures;
  out->stop_reason = m.stopReason;
  if (optimised) {
    for (int j = 0; j < nPts; j++)
      for (int c = 0; c < 3; c++) {
        const float v = Xf[(size_t)j * 3 + c];
        p3dOut[(size_t)P.pts[j].i * 3 + c] = scaled ? v * inv : v;
      }
    out->chi2_initial = chi2Initial;
    out->chi2_final = m.currentChi;
    out->lambda = m.lambda;
    double R[3][3];
    quatToMatrix(P.T.q, R);
    for (int k = 0; k < 4; k++) out->q[k] = P.T.q[k];
    for (int k = 0; k < 3; k++) out->t[k] = P.T.t[k];
    for (int k = 0; k < 9; k++) out->R21[k] = (float)R[k / 3][k % 3];
    for (int k = 0; k < 3; k++) {
      const float t = (float)P.T.t[k];
      out->t21[k] = scaled ? t * inv : t;
    }
    out->median_depth = median;
  } else {
    std::memcpy(out->R21, ir->R21, sizeof out->R21);
    std::memcpy(out->t21, ir->t21, sizeof out->t21);
  }
  if (counters) {
    counters[0] = cnt.accepted;
    counters[1] = cnt.rejected;
    counters[2] = cnt.huberOutliers;
    counters[3] = cnt.smallTheta;
  }
}

// The first trial of iteration 0 alone, for the independent statement: the point list (idx [n1] = the vertices' keypoints of
// frame 1), the start pose, lambda, chi2_initial, and the step (xp [6] = (omega, upsilon), xl [n][3]).  Returns the number of
// points, or -1 when the inputs are refused or the solve failed.
int bar_first_step(const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, int cap, const int32_t* m12,
                   const orbx_init_result* ir, const float* p3d, const uint8_t* tri, const float* K, const float* invSigma2,
                   int nLevels, int32_t* idx, double* pose7, double* lambda, double* chi2Initial, double* xp, double* xl) {
  const Inputs in{k1, k2, n1, n2, cap, m12, ir, p3d, tri, K, invSigma2, nLevels};
  Problem P;
  Counters cnt{0, 0, 0, 0};
  Lm m;
  startLm(&m);
  int nPts = 0;
  if (gather(in, P, &nPts) != 0 || nPts == 0) return -1;
  for (int k = 0; k < 4; k++) pose7[k] = P.T.q[k];
  for (int k = 0; k < 3; k++) pose7[4 + k] = P.T.t[k];
  for (int j = 0; j < nPts; j++) idx[j] = P.pts[j].i;
  linearise(P, &m, &cnt, 0, chi2Initial);
  *lambda = m.lambda;
  trial(P, &m, &cnt, xl);
  if (!m.ok) return -1;
  for (int k = 0; k < 6; k++) xp[k] = m.xp[k];
  return nPts;
}

void bar_sincos(double x, double* s, double* c) { sinCos(x, s, c); }
double bar_huber_delta() { return deltaHuber(); }

}  // extern "C"
