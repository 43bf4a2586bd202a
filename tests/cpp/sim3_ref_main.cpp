// sim3_ref_main.cpp — a stand-alone program around tests/cpp/sim3_ref.cpp, TEST INFRASTRUCTURE: two small worlds through both
// forms of iterate() (the literal loop and the after-the-fact resolution), which must agree byte for byte.  Built by
// tests/test_sim3_host.py with -fsanitize=address,undefined: the restatement's indexing under the sanitizers, in a process of
// its own.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/orbx.h"

extern "C" void s3r_solve(const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, int cap, const int32_t* match,
                          const float* points1, const uint8_t* mask1, const float* points2, const uint8_t* mask2, const float* pose1,
                          const float* pose2, const float* Kf, const float* sigma2, int nLevels, const int32_t* table, int fixScale,
                          int minInliers, float th2, int nIter, const int32_t* draws, int mode, orbx_sim3_result* res, float* sim3,
                          int32_t* row, uint8_t* inliers);

namespace {

uint32_t state = 12345u;
uint32_t next() {  // a small LCG: the worlds are the same on every run
  state = state * 1664525u + 1013904223u;
  return state >> 1;
}
double unit() { return (double)next() / 2147483648.0; }

// n correspondences of which every fifth is a gross mismatch when `gross`; KF1's points are s * Y2 + t (R12 = I), both poses
// the identity.  Returns 0 when both forms agree and the answer is as expected.
int world(int n, int cap, bool gross, int minInliers, bool expectResult) {
  const int nLevels = 8, nIter = 60;
  std::vector<orbx_keypoint> k1(cap), k2(cap);
  std::vector<float> p1((size_t)cap * 3, 0.f), p2((size_t)cap * 3, 0.f);
  std::vector<uint8_t> m1(cap, 0), m2(cap, 0);
  std::vector<int32_t> match(cap, -1), table(cap + 1), draws((size_t)nIter * 3);
  std::memset(k1.data(), 0, sizeof(orbx_keypoint) * cap);
  std::memset(k2.data(), 0, sizeof(orbx_keypoint) * cap);
  const double s = 1.25, t[3] = {0.2, -0.1, 0.3};
  for (int i = 0; i < n; i++) {
    const int j = n - 1 - i;  // KF2 holds them in reverse
    const double z = 4 + 16 * unit(), Y[3] = {(unit() - 0.5) * 0.8 * z, (unit() - 0.5) * 0.6 * z, z};
    for (int c = 0; c < 3; c++) {
      p2[(size_t)j * 3 + c] = (float)(Y[c] + (gross && i % 5 == 4 ? 2.0 : 0.0));
      p1[(size_t)i * 3 + c] = (float)(s * Y[c] + t[c]);
    }
    k1[i].octave = (int)(next() % nLevels);
    k2[j].octave = (int)(next() % nLevels);
    m1[i] = m2[j] = 1;
    match[i] = j;
  }
  const float pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, K[9] = {520, 0, 320, 0, 520, 240, 0, 0, 1};
  float sigma2[nLevels];
  for (int l = 0; l < nLevels; l++) sigma2[l] = (float)std::pow(1.44, l);
  for (int N = 0; N <= cap; N++) {  // SetRansacParameters(0.99, minInliers, 300)
    const double eps = (double)((float)minInliers / (float)(N > 0 ? N : 1));
    table[N] = N < minInliers ? 300 : N == minInliers ? 1 : (int)std::fmax(1.0, std::fmin(300.0, std::ceil(std::log(0.01) / std::log(1 - eps * eps * eps))));
  }
  for (auto& d : draws) d = (int32_t)next();
  orbx_sim3_result res[2];
  float sim[2][13];
  std::vector<int32_t> row[2] = {std::vector<int32_t>(cap), std::vector<int32_t>(cap)};
  std::vector<uint8_t> inl[2] = {std::vector<uint8_t>(cap), std::vector<uint8_t>(cap)};
  for (int mode = 0; mode < 2; mode++)
    s3r_solve(k1.data(), n, k2.data(), n, cap, match.data(), p1.data(), m1.data(), p2.data(), m2.data(), pose, pose, K, sigma2, nLevels,
              table.data(), 0, minInliers, 9.21f, nIter, draws.data(), mode, &res[mode], sim[mode], row[mode].data(), inl[mode].data());
  if (std::memcmp(&res[0], &res[1], sizeof res[0]) || std::memcmp(sim[0], sim[1], sizeof sim[0]) || row[0] != row[1] || inl[0] != inl[1]) {
    std::printf("the two forms of iterate differ (n = %d)\n", n);
    return 1;
  }
  std::printf("n %d: status %d, N %d, found_it %d, %d inliers, s12 %.6f\n", n, res[0].status, res[0].n_correspondences, res[0].found_it,
              res[0].n_inliers, res[0].s12);
  if (expectResult != (res[0].found_it >= 0)) return 1;
  if (expectResult && (std::fabs(res[0].s12 - s) > 1e-3 || res[0].n_inliers < (gross ? n - n / 5 - 2 : n))) return 1;
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad += world(100, 128, true, 20, true);   // a fifth gross mismatches
  bad += world(19, 19, false, 20, false);   // capacity = count, below minInliers: bNoMore
  if (bad) return 1;
  std::printf("SIM3 REF OK\n");
  return 0;
}
