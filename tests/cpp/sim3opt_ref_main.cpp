// sim3opt_ref_main.cpp — a stand-alone program around tests/cpp/sim3opt_ref.cpp, TEST INFRASTRUCTURE: two small worlds through
// both forms of the linearisation (the fourteen perturbed estimates per edge, as g2o computes them, and once per linearisation),
// which must agree byte for byte.  Built by tests/test_sim3opt_host.py with -fsanitize=address,undefined: the restatement's
// indexing under the sanitizers, in a process of its own.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/orbx.h"

extern "C" void s3o_optimize(const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, int cap, int32_t* row,
                             const float* points1, const uint8_t* mask1, const float* points2, const uint8_t* mask2, const float* pose1,
                             const float* pose2, const float* K, const float* invSigma2, int nLevels, const float* sim, int fixScale,
                             float th2, int nIterations, int nMoreIterations, int perEdge, orbx_sim3opt_result* out, float* simOut,
                             int64_t* counters);

namespace {

uint32_t state = 54321u;
uint32_t next() {  // a small LCG: the worlds are the same on every run
  state = state * 1664525u + 1013904223u;
  return state >> 1;
}
double unit() { return (double)next() / 2147483648.0; }

// n correspondences of which every fifth names its neighbour's feature when `gross`; KF1's points are s * Y2 + t (R12 = I), both
// poses the identity; the start similarity is a little off.  Returns 0 when both forms agree and the answer is as expected.
int world(int n, int cap, bool gross, int fixScale) {
  const int nLevels = 8;
  std::vector<orbx_keypoint> k1(cap), k2(cap);
  std::vector<float> p1((size_t)cap * 3, 0.f), p2((size_t)cap * 3, 0.f);
  std::vector<uint8_t> m1(cap, 0), m2(cap, 0);
  std::vector<int32_t> match(cap, -1);
  std::memset(k1.data(), 0, sizeof(orbx_keypoint) * cap);
  std::memset(k2.data(), 0, sizeof(orbx_keypoint) * cap);
  const double s = fixScale ? 1.0 : 1.25, t[3] = {0.2, -0.1, 0.3}, f = 520, cx = 320, cy = 240;
  for (int i = 0; i < n; i++) {
    const int j = n - 1 - i;  // KF2 holds them in reverse
    const double z = 4 + 16 * unit(), Y[3] = {(unit() - 0.5) * 0.8 * z, (unit() - 0.5) * 0.6 * z, z};
    double X[3];
    for (int c = 0; c < 3; c++) {
      X[c] = s * Y[c] + t[c];
      p2[(size_t)j * 3 + c] = (float)Y[c];
      p1[(size_t)i * 3 + c] = (float)X[c];
    }
    k1[i].x = (float)(X[0] / X[2] * f + cx); k1[i].y = (float)(X[1] / X[2] * f + cy);
    k2[j].x = (float)(Y[0] / Y[2] * f + cx); k2[j].y = (float)(Y[1] / Y[2] * f + cy);
    k1[i].octave = (int)(next() % nLevels);
    k2[j].octave = (int)(next() % nLevels);
    m1[i] = m2[j] = 1;
    match[i] = j;
  }
  int planted = 0;
  for (int i = 4; gross && i + 1 < n; i += 5, planted++) match[i] = n - 1 - (i + 1);
  const float pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, K[9] = {520, 0, 320, 0, 520, 240, 0, 0, 1};
  float inv[nLevels];
  for (int l = 0; l < nLevels; l++) inv[l] = (float)(1.0 / std::pow(1.44, l));
  const float c = std::cos(0.01f), sn = std::sin(0.01f);
  const float sim[13] = {c, -sn, 0, sn, c, 0, 0, 0, 1, (float)(t[0] * 1.02), (float)t[1], (float)(t[2] * 0.98), (float)(fixScale ? 1.0 : s * 1.03)};
  orbx_sim3opt_result res[2];
  float out[2][13];
  std::vector<int32_t> row[2] = {match, match};
  for (int mode = 0; mode < 2; mode++)
    s3o_optimize(k1.data(), n, k2.data(), n, cap, row[mode].data(), p1.data(), m1.data(), p2.data(), m2.data(), pose, pose, K, inv,
                 nLevels, sim, fixScale, 10.f, 5, 10, mode, &res[mode], out[mode], nullptr);
  if (std::memcmp(&res[0], &res[1], sizeof res[0]) || std::memcmp(out[0], out[1], sizeof out[0]) || row[0] != row[1]) {
    std::printf("the two forms differ (n = %d)\n", n);
    return 1;
  }
  if (res[0].status != 0 || res[0].n_correspondences != n || res[0].n_bad < planted || res[0].n_inliers != n - res[0].n_bad ||
      std::fabs(res[0].s - s) > 1e-3) {
    std::printf("n = %d: status %d, %d correspondences, %d bad (%d planted), %d inliers, s = %.9g\n", n, res[0].status,
                res[0].n_correspondences, res[0].n_bad, planted, res[0].n_inliers, res[0].s);
    return 1;
  }
  return 0;
}

}  // namespace

int main() {
  int bad = world(70, 80, true, 0);
  bad += world(130, 130, false, 1);
  if (bad) return 1;
  std::printf("SIM3OPT REF OK\n");
  return 0;
}
