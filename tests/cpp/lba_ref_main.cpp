// lba_ref_main.cpp — a stand-alone program over tests/cpp/lba_ref.cpp for the sanitizers (TEST INFRASTRUCTURE; built by
// tests/test_lba_host.py with -fsanitize=address,undefined): the restatement over small synthetic windows and over every
// garbage case of include/orbx.h, "local mapping: local bundle adjustment", deviation 6.  It checks the status of each run and
// that a flagged problem comes back as it went in; what it is for is that the sanitizers see every phase run, also on garbage.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/orbx.h"

extern "C" void lbar_local_ba(const orbx_keypoint* kps, const int32_t* nKps, const float* poseIn, const int32_t* frameOf, int nE, int nF,
                              const int32_t* rows, int cap, const float* mapPts, const uint8_t* mapMask, int mapN, int mapCap,
                              const float* K, const float* invSigma2, int nLevels, int nIterations, int nMoreIterations, float* poseOut,
                              float* mapOut, uint8_t* outlier, orbx_lba_result* res, long long* counters);

namespace {

struct Rng {
  uint64_t s;
  double next() {  // [0, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  }
  double sym(double a) { return (2.0 * next() - 1.0) * a; }
};

struct Window {
  int nE, nF, cap, mapN, mapCap;
  std::vector<orbx_keypoint> kps;
  std::vector<int32_t> n, rows, frames;
  std::vector<float> pose, pts;
  std::vector<uint8_t> mask;
};

// nE cameras on a baseline (identity rotations), nP points 4 to 8 deep, every camera sees every `stride`-th point
Window make(int nE, int nF, int nP, int stride, uint64_t seed) {
  Rng r{seed};
  Window w;
  w.nE = nE; w.nF = nF; w.cap = nP + 4; w.mapN = nP; w.mapCap = nP + 2;
  w.kps.assign((size_t)nE * w.cap, orbx_keypoint{});
  w.n.assign(nE, 0);
  w.rows.assign((size_t)nE * w.cap, -1);
  w.frames.resize(nE);
  w.pose.assign((size_t)nE * 12, 0.f);
  w.pts.assign((size_t)w.mapCap * 3, 0.f);
  w.mask.assign(w.mapCap, 0);
  std::vector<double> X((size_t)nP * 3);
  for (int j = 0; j < nP; j++) {
    X[j * 3] = r.sym(2.0); X[j * 3 + 1] = r.sym(1.5); X[j * 3 + 2] = 4.0 + 4.0 * r.next();
    for (int c = 0; c < 3; c++) w.pts[j * 3 + c] = (float)(X[j * 3 + c] + r.sym(0.02));
    w.mask[j] = 1;
  }
  for (int e = 0; e < nE; e++) {
    w.frames[e] = e;
    const double tx = -0.25 * e;
    float* p = &w.pose[(size_t)e * 12];
    p[0] = p[4] = p[8] = 1.f;
    p[9] = (float)(tx + (e < nF ? r.sym(0.02) : 0.0));
    p[10] = (float)(e < nF ? r.sym(0.02) : 0.0);
    int f = 0;
    for (int j = e % stride; j < nP; j += stride, f++) {
      orbx_keypoint& k = w.kps[(size_t)e * w.cap + f];
      k.x = (float)((X[j * 3] + tx) / X[j * 3 + 2] * 520.0 + 320.0 + r.sym(0.5));
      k.y = (float)(X[j * 3 + 1] / X[j * 3 + 2] * 520.0 + 240.0 + r.sym(0.5));
      k.octave = (int)(r.next() * 8) & 7;
      if (j % 11 == 3) k.x += 30.f;  // a gross mismatch
      w.rows[(size_t)e * w.cap + f] = j;
    }
    w.rows[(size_t)e * w.cap + f++] = -2;
    w.rows[(size_t)e * w.cap + f++] = -1;
    w.n[e] = f;
  }
  return w;
}

int failures = 0;

orbx_lba_result run(const Window& w, int nIt, int nMore, const float* table, bool passThrough, int wantStatus, const char* what) {
  const float K[9] = {520.f, 0.f, 320.f, 0.f, 520.f, 240.f, 0.f, 0.f, 1.f};
  std::vector<float> poseOut((size_t)w.nE * 12 + 1), mapOut((size_t)w.mapCap * 3);
  std::vector<uint8_t> outlier((size_t)w.nE * w.cap + 1);
  orbx_lba_result res;
  long long counters[4];
  lbar_local_ba(w.kps.data(), w.n.data(), w.pose.data(), w.frames.data(), w.nE, w.nF, w.rows.data(), w.cap, w.pts.data(), w.mask.data(),
                w.mapN, w.mapCap, K, table, 8, nIt, nMore, poseOut.data(), mapOut.data(), outlier.data(), &res, counters);
  bool ok = res.status == wantStatus;
  if (passThrough) {
    ok = ok && std::memcmp(mapOut.data(), w.pts.data(), mapOut.size() * sizeof(float)) == 0;
    for (int e = 0; e < w.nE; e++)
      ok = ok && std::memcmp(&poseOut[(size_t)e * 12], &w.pose[(size_t)w.frames[e] * 12], 12 * sizeof(float)) == 0;
    for (size_t k = 0; k + 1 < outlier.size(); k++) ok = ok && outlier[k] == 0;
  }
  std::printf("%-28s status %d iterations %d %d trials %d %d failures %d %d points %d edges %d level1 %d erased %d %s\n", what, res.status,
              res.iterations[0], res.iterations[1], res.lm_trials[0], res.lm_trials[1], res.solver_failures[0], res.solver_failures[1],
              res.n_points, res.n_edges, res.n_level1, res.n_erased, ok ? "ok" : "WRONG");
  if (!ok) failures++;
  return res;
}

}  // namespace

int main() {
  float table[8], zeros[8] = {0};
  float scale = 1.f;
  for (int i = 0; i < 8; i++) {
    table[i] = 1.f / (scale * scale);
    scale *= 1.2f;
  }
  const Window base = make(5, 3, 60, 2, 7);
  if (run(base, 5, 10, table, false, 0, "window").iterations[0] == 0) failures++;
  run(make(3, 3, 40, 1, 8), 5, 10, table, false, 0, "no fixed keyframe");
  run(make(70, 64, 300, 5, 9), 2, 2, table, false, 0, "64 free keyframes");
  run(make(4, 0, 30, 1, 10), 5, 10, table, true, 0, "no free keyframe");
  run(make(0, 0, 5, 1, 11), 5, 10, table, true, 0, "no keyframe");
  run(base, 0, 0, table, false, 0, "no iteration");
  if (run(base, 5, 10, zeros, false, 0, "table of zeros").solver_failures[0] != 10) failures++;
  Window g = base;
  g.n[1] = g.cap + 1;
  run(g, 5, 10, table, true, ORBX_LBA_BAD_INPUT, "count above capacity");
  g = base; g.n[0] = -1;
  run(g, 5, 10, table, true, ORBX_LBA_BAD_INPUT, "negative count");
  g = base; g.mapN = g.mapCap + 1;
  run(g, 5, 10, table, true, ORBX_LBA_BAD_INPUT, "map count above capacity");
  g = base; g.mapN = -3;
  run(g, 5, 10, table, true, ORBX_LBA_BAD_INPUT, "negative map count");
  g = base; g.rows[0] = g.mapN;
  run(g, 5, 10, table, true, ORBX_LBA_BAD_INPUT, "row entry >= map_n");
  g = base; g.rows[2] = 0x7fffffff;
  run(g, 5, 10, table, true, ORBX_LBA_BAD_INPUT, "row entry INT_MAX");
  g = base; g.kps[0].octave = 8;
  run(g, 5, 10, table, true, ORBX_LBA_BAD_INPUT, "octave 8");
  g = base; g.kps[1].octave = -1;
  run(g, 5, 10, table, true, ORBX_LBA_BAD_INPUT, "octave -1");
  g = base; g.rows[g.n[0] - 1] = g.rows[0];
  run(g, 5, 10, table, true, ORBX_LBA_BAD_INPUT, "one point twice in a keyframe");
  g = base; g.frames[3] = g.frames[1];
  run(g, 5, 10, table, true, ORBX_LBA_BAD_INPUT, "a frame twice");
  g = base; g.pose[(size_t)4 * 12 + 3] = NAN;
  run(g, 5, 10, table, true, ORBX_LBA_NONFINITE, "NaN in a fixed pose");
  g = base; g.pts[3 * g.rows[1] + 2] = INFINITY;
  run(g, 5, 10, table, true, ORBX_LBA_NONFINITE, "infinite point");
  g = base; g.pts[3 * g.rows[1] + 2] = 0.f;  // a point in the camera's plane: a division by zero, a non-finite RESULT
  run(g, 5, 10, table, true, ORBX_LBA_NONFINITE, "point at depth 0");
  std::printf(failures ? "FAILED: %d\n" : "all fine\n", failures);
  return failures ? 1 : 0;
}
