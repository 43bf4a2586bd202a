// lba_ref.cpp — CPU restatement of the local bundle adjustment (include/orbx.h, "local mapping: local bundle adjustment"), TEST
// INFRASTRUCTURE: built by tests/lba_ref_lib.py with g++ -O2 -ffp-contract=off.  The phases and their arithmetic are
// orb_slam_tracking_amd/csrc/orbx_lba_math.inc over orbx_ba_math.inc, the includes the device kernel compiles too; a phase is
// run here for lane 0 .. 255 one after the other.  This file restates on its own the sequence of the phases (the loops of
// optimize() and solve(), the two rounds), the two folds of the lanes' sums (the tree over 256 lanes, the tree inside a wave)
// and the copy-through of the outputs.  Beyond the result it reports counters that show which branches a world ran.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbx.h"

#define ORBX_BA_FN
#include "../../orb_slam_tracking_amd/csrc/orbx_ba_math.inc"
#define ORBX_LBA_ADD(p, v) (*(p) += (v), *(p) - (v))
#define ORBX_LBA_OR64(p, v) (*(p) |= (v))
#include "../../orb_slam_tracking_amd/csrc/orbx_lba_math.inc"

using namespace orbx_lba;

namespace {

#define LANES(tid) for (int tid = 0; tid < LBA_NT; tid++)

double deltaHuber() { return (double)(float)std::sqrt(5.991); }

double treeSum(double* v) {
  for (int off = LBA_NT / 2; off >= 1; off >>= 1)
    for (int t = 0; t < off; t++) v[t] = v[t] + v[t + off];
  return v[0];
}
double treeMax(double* v) {
  for (int off = LBA_NT / 2; off >= 1; off >>= 1)
    for (int t = 0; t < off; t++)
      if (v[t + off] > v[t]) v[t] = v[t + off];
  return v[0];
}

struct Run {
  Prob v{};
  Shared s{};
  std::vector<unsigned char> ws;
  int status = 0;
  bool counted = false, run = false;
};

int gather(Run& r, int bits) {
  r.s.status |= bits;
  return r.s.status;
}

// the checks and the graph -> status
void buildGraph(Run& r) {
  Prob& v = r.v;
  Shared& s = r.s;
  r.ws.assign(layout(&v, 0) + 256, 0xA5);  // (whatever the device's workspace held: nothing is read before it is written)
  layout(&v, ((uintptr_t)r.ws.data() + 255) / 256 * 256);
  s.status = (v.mapN < 0 || v.mapN > v.mapCap) ? ST_BAD : 0;
  s.nP = s.nEdges = s.nLevel1 = s.nErased = 0;
  s.cnt = Counters{0, 0, 0, 0};
  int status = s.status;
  if (!status) {
    LANES(t) gather(r, checkEntries(v, t));
    status = s.status;
  }
  if (!status) {
    LANES(t) clearGraph(v, t);
    LANES(t) gather(r, countEdges(v, t));
    status = s.status;
  }
  if (!status) {
    LANES(t) countVertices(v, s, t);
    scanLanes(s);
    s.nP = s.scan[LBA_NT];
    LANES(t) gather(r, fillVertices(v, s, t));
    status = s.status;
  }
  if (!status) {
    LANES(t) countSlots(v, s, t);
    scanLanes(s);
    s.nEdges = s.scan[LBA_NT];
    LANES(t) fillStarts(v, s, t);
    LANES(t) fillEdges(v, t);
    LANES(t) gather(r, sortEdges(v, s, t));
    status = s.status;
  }
  if (!status) LANES(t) loadPoses(v, t);
  r.status = status;
  r.counted = status == 0;
  r.run = status == 0 && v.nF > 0 && s.nEdges > 0;
}

void startRound(Run& r, int round) {
  roundClear(r.s);
  LANES(t) activate(r.v, r.s, t);
  roundStart(r.v, r.s, round);
}

// buildSystem and solve()'s head
void linearize(Run& r, int round, int it) {
  Prob& v = r.v;
  Shared& s = r.s;
  const bool robust = round == 0;
  double chi[LBA_NT], maxd[LBA_NT];
  LANES(t) {
    chi[t] = maxd[t] = 0.0;
    buildPoints(v, s, t, robust, &chi[t], &maxd[t]);
  }
  for (int ar = 0; ar < s.nA; ar++) {
    double acc[64][27];
    for (int l = 0; l < 64; l++) buildPoseLane(v, s.actEnt[ar], l, robust, acc[l]);
    for (int k = 0; k < 27; k++)
      for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; l++) acc[l][k] = acc[l][k] + acc[l + off][k];
    buildPoseKeep(s, ar, acc[0]);
  }
  const double chiAll = treeSum(chi), maxAll = treeMax(maxd);
  iterationStart(s, round, it, chiAll, maxAll);
}

// the reduced system set up and solved -> ok
int solveReduced(Run& r) {
  Prob& v = r.v;
  Shared& s = r.s;
  LANES(t) trialPoints(v, s, t);
  LANES(t) schurOwners(v, s, t);
  int ok = 1;
  for (int jc = 0; jc < s.n && ok; jc++) {
    LANES(t) if (!cholColumn(v, s, jc, t)) ok = 0;
    if (ok) LANES(t) cholUpdate(v, s, jc, t);
  }
  if (ok) {
    for (int jc = 0; jc < s.n; jc++) LANES(t) solveForward(v, s, jc, t);
    for (int jc = s.n - 1; jc >= 0; jc--) LANES(t) solveBackward(v, s, jc, t);
    int bad = 0;
    LANES(t) bad |= solutionBad(s, t);
    ok = bad ? 0 : 1;
  }
  s.lm.ok = ok;
  if (!ok) s.lm.solverFailures++;
  return ok;
}

void optimise(Run& r, int round, int nIt) {
  Prob& v = r.v;
  Shared& s = r.s;
  const bool robust = round == 0;
  startRound(r, round);
  if (s.nActEdges > 0) {
    LANES(t) activeErrors(v, s, t, robust);
    for (int it = 0; it < nIt; it++) {
      linearize(r, round, it);
      int more;
      do {
        const int ok = solveReduced(r);
        double scale[LBA_NT], tchi[LBA_NT];
        LANES(t) scale[t] = tchi[t] = 0.0;
        if (ok) {
          LANES(t) trialStep(v, s, t, &scale[t]);
          LANES(t) tchi[t] = activeErrors(v, s, t, robust);
        }
        const double scaleAll = treeSum(scale), tchiAll = treeSum(tchi);
        s.accepted = lmJudge(&s.lm, ok ? tchiAll : 0.0, ok ? poseScale(s, scaleAll) : 0.0, &s.cnt);
        more = lmAnotherTrial(&s.lm) ? 1 : 0;
        if (!s.accepted && ok) LANES(t) trialRestore(v, s, t);
      } while (more);
      const int stop = lmEndIteration(&s.lm);
      s.lm.iterations++;
      s.lm.stopReason = stop;
      if (stop) break;
    }
  }
  roundEnd(s, round);
  if (round == 0) LANES(t) s.nLevel1 += classify(v, s, t, nullptr);
}

void fillProb(Prob& v, const orbx_keypoint* kps, const int32_t* nKps, const float* poseIn, const int32_t* frameOf, int nE, int nF,
              const int32_t* rows, int cap, const float* mapPts, const uint8_t* mapMask, int mapN, int mapCap, const float* K,
              const float* invSigma2, int nLevels) {
  v.kps = kps;
  v.nKps = nKps;
  v.poseIn = poseIn;
  v.frameOf = frameOf;
  v.rows = rows;
  v.mapPts = mapPts;
  v.mapMask = mapMask;
  v.invSigma2 = invSigma2;
  v.nLevels = nLevels;
  v.cap = cap;
  v.mapCap = mapCap;
  v.mapN = mapN;
  v.nE = nE;
  v.nF = nF;
  v.K = Cam{(double)K[0], (double)K[4], (double)K[2], (double)K[5]};
  v.delta = deltaHuber();
}

}  // namespace

extern "C" {

double lbar_huber_delta() { return deltaHuber(); }

// One problem.  kps / nKps / poseIn are the batch's frame arrays, frameOf [nE] the problem's entries (the first nF free), rows
// [nE][cap]; mapPts [mapCap][3], mapMask [mapCap] or null.  Outputs: poseOut [nE][12], mapOut [mapCap][3] (every point: the
// copy-through is part of it), outlier [nE][cap], res, counters [4] (accepted, rejected, huber outliers: unused, small theta).
void lbar_local_ba(const orbx_keypoint* kps, const int32_t* nKps, const float* poseIn, const int32_t* frameOf, int nE, int nF,
                   const int32_t* rows, int cap, const float* mapPts, const uint8_t* mapMask, int mapN, int mapCap, const float* K,
                   const float* invSigma2, int nLevels, int nIterations, int nMoreIterations, float* poseOut, float* mapOut,
                   uint8_t* outlier, orbx_lba_result* res, long long* counters) {
  Run* rp = new Run;
  Run& r = *rp;
  fillProb(r.v, kps, nKps, poseIn, frameOf, nE, nF, rows, cap, mapPts, mapMask, mapN, mapCap, K, invSigma2, nLevels);
  for (int k = 0; k < 2; k++) {
    r.s.iterations[k] = r.s.trials[k] = r.s.rejected[k] = r.s.failures[k] = r.s.stopReason[k] = r.s.nActP[k] = r.s.nActF[k] = 0;
    r.s.chi2Initial[k] = r.s.chi2Final[k] = r.s.lambda[k] = 0.0;
  }
  std::memset(outlier, 0, (size_t)nE * cap);
  if (mapOut != mapPts) std::memcpy(mapOut, mapPts, (size_t)mapCap * 3 * sizeof(float));
  buildGraph(r);
  int status = r.status;
  if (r.run) {
    optimise(r, 0, nIterations);
    optimise(r, 1, nMoreIterations);
  }
  bool optimised = r.run;
  if (r.run) {
    int bad = 0;
    LANES(t) bad |= resultBad(r.v, r.s, t);
    if (bad) {
      status |= ST_NONFINITE;
      optimised = false;
    }
  }
  if (optimised) LANES(t) r.s.nErased += classify(r.v, r.s, t, outlier);
  LANES(t) writeOutputs(r.v, r.s, t, optimised, poseOut, mapOut);
  writeResult(r.v, r.s, status, r.counted, r.run, res);
  if (counters) {
    counters[0] = r.s.cnt.accepted;
    counters[1] = r.s.cnt.rejected;
    counters[2] = r.s.cnt.huberOutliers;
    counters[3] = r.s.cnt.smallTheta;
  }
  delete rp;
}

// The first trial of iteration 0 of round 1 -> the number of point vertices, or -1 when the problem does not run or the solve
// fails.  pidx [mapCap] the vertices' map points, actEnt [64] / *nA the active free entries in the system's order, xp [6 * nA],
// xl [nP][3], *lambda, *chi2.
int lbar_first_step(const orbx_keypoint* kps, const int32_t* nKps, const float* poseIn, const int32_t* frameOf, int nE, int nF,
                    const int32_t* rows, int cap, const float* mapPts, const uint8_t* mapMask, int mapN, int mapCap, const float* K,
                    const float* invSigma2, int nLevels, int32_t* pidx, int32_t* actEnt, int32_t* nA, double* xp, double* xl,
                    double* lambda, double* chi2) {
  Run* rp = new Run;
  Run& r = *rp;
  fillProb(r.v, kps, nKps, poseIn, frameOf, nE, nF, rows, cap, mapPts, mapMask, mapN, mapCap, K, invSigma2, nLevels);
  buildGraph(r);
  int n = -1;
  if (r.run) {
    startRound(r, 0);
    LANES(t) activeErrors(r.v, r.s, t, true);
    linearize(r, 0, 0);
    if (solveReduced(r)) {
      double scale = 0.0;
      LANES(t) trialStep(r.v, r.s, t, &scale, xl);
      n = r.s.nP;
      for (int j = 0; j < n; j++) pidx[j] = r.v.pidx[j];
      *nA = r.s.nA;
      for (int a = 0; a < r.s.nA; a++) actEnt[a] = r.s.actEnt[a];
      for (int k = 0; k < r.s.n; k++) xp[k] = r.s.x[k];
      *lambda = r.s.lm.lambda;
      *chi2 = r.s.chi2Initial[0];
    }
  }
  delete rp;
  return n;
}

}  // extern "C"
