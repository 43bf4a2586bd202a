// LoopClosing::ComputeSim3's last step over include/orbx_shim.hpp, POD build: two keyframes as KeyFrameViews of a synthetic scene
// seen by two cameras whose maps differ by a similarity with scale 1.25, a tenth of the matches naming a neighbour's feature
// (gross mismatches), a start similarity that is a little off, then Optimizer::OptimizeSim3(..., th2 = 10, bFixScale = false) as
// ComputeSim3 calls it.  The same inputs go through the C ABI (orbx_optimize_sim3); both must give the same bytes.
// Usage: shim_sim3opt <seed>; prints RESULT <status> <nIn> <correspondences> <removed> <planted mismatches left in the row>
// <agrees with the C ABI> <scale>.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }

int main(int argc, char** argv) {
  const int seed = argc > 1 ? atoi(argv[1]) : 0;
  srand(seed);
  const int n = 150, nf = n + 8;
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  const float K[9] = {517.25f, 0.f, 318.75f, 0.f, 388.5f, 255.5f, 0.f, 0.f, 1.f};
  std::vector<KeyPointT> keys1(nf), keys2(nf);
  // Y1 = s R Y2 + t between the camera frames; KF1's map is its camera frame moved by t1, KF2's its own camera frame
  const double a = 0.06, R[3][3] = {{std::cos(a), 0, std::sin(a)}, {0, 1, 0}, {-std::sin(a), 0, std::cos(a)}}, t[3] = {0.3, -0.1, 0.2};
  const double s = 1.25, t1[3] = {0.5, -1.0, 2.0};
  std::vector<float> p1(3 * nf, 0.f), p2(3 * nf, 0.f);
  std::vector<uint8_t> h1(nf, 0), h2(nf, 0);
  std::vector<int> vpMatches1(nf, -1);
  for (int i = 0; i < n; i++) {
    const int j = n - 1 - i;  // KF2 holds the points in reverse
    const double z = uniform(4, 20), Y2[3] = {uniform(-0.45, 0.45) * z, uniform(-0.32, 0.32) * z, z};
    double Y1[3];
    for (int r = 0; r < 3; r++) Y1[r] = s * (R[r][0] * Y2[0] + R[r][1] * Y2[1] + R[r][2] * Y2[2]) + t[r];
    for (int c = 0; c < 3; c++) {
      p1[3 * i + c] = (float)(Y1[c] - t1[c]);
      p2[3 * j + c] = (float)Y2[c];
    }
    keys1[i].octave = rand() % 8;
    keys2[j].octave = rand() % 8;
    keys1[i].pt.x = (float)(517.25 * Y1[0] / Y1[2] + 318.75 + uniform(-0.3, 0.3));
    keys1[i].pt.y = (float)(388.5 * Y1[1] / Y1[2] + 255.5 + uniform(-0.3, 0.3));
    keys2[j].pt.x = (float)(517.25 * Y2[0] / Y2[2] + 318.75 + uniform(-0.3, 0.3));
    keys2[j].pt.y = (float)(388.5 * Y2[1] / Y2[2] + 255.5 + uniform(-0.3, 0.3));
    h1[i] = h2[j] = 1;
    vpMatches1[i] = j;
  }
  std::vector<int> planted;
  for (int i = 5; i + 1 < n; i += 10) {  // a tenth of the matches name the next point's feature
    vpMatches1[i] = n - 1 - (i + 1);
    planted.push_back(i);
  }
  vpMatches1[n] = n + 1;  // a match between two features without a point
  const float pose1[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, (float)t1[0], (float)t1[1], (float)t1[2]}, pose2[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  const double a0 = a + 0.01;
  float sim[13] = {(float)std::cos(a0), 0, (float)std::sin(a0), 0, 1, 0, (float)-std::sin(a0), 0, (float)std::cos(a0),
                   (float)(t[0] * 1.03), (float)t[1], (float)(t[2] * 0.97), (float)(s * 1.02)};

  // the C ABI
  std::vector<int32_t> row(vpMatches1.begin(), vpMatches1.end());
  orbx_sim3opt_result res;
  float out[13];
  const int rc = orbx_optimize_sim3(extractor.context(), reinterpret_cast<const orbx_keypoint*>(keys1.data()), nf, p1.data(), h1.data(), pose1,
                                    reinterpret_cast<const orbx_keypoint*>(keys2.data()), nf, p2.data(), h2.data(), pose2, row.data(), sim, K,
                                    nullptr, 0, 10.f, 5, 10, &res, out);
  if (rc != ORBX_OK) {
    std::printf("orbx_optimize_sim3: %d\n", rc);
    return 1;
  }

  // the shim
  KeyFrameView V1, V2;
  V1.N = V2.N = nf;
  V1.mvKeysUn = keys1.data(); V2.mvKeysUn = keys2.data();
  V1.mWorldPos = p1.data(); V2.mWorldPos = p2.data();
  V1.mbGood = h1.data(); V2.mbGood = h2.data();
  V1.mTcw = pose1; V2.mTcw = pose2;
  float s12 = sim[12], R12[9], t12[3];
  std::memcpy(R12, sim, sizeof R12);
  std::memcpy(t12, sim + 9, sizeof t12);
  orbx_sim3opt_result resShim;
  const int nIn = Optimizer::OptimizeSim3(&extractor, V1, V2, vpMatches1, s12, R12, t12, 10.f, false, K, &resShim);
  bool same = std::memcmp(&res, &resShim, sizeof res) == 0 && nIn == res.n_inliers && s12 == out[12] &&
              std::memcmp(R12, out, sizeof R12) == 0 && std::memcmp(t12, out + 9, sizeof t12) == 0;
  for (int i = 0; same && i < nf; i++) same = vpMatches1[i] == row[i];
  int left = 0;
  for (int i : planted) left += row[i] >= 0;
  std::printf("RESULT %d %d %d %d %d %d %.6f\n", res.status, nIn, res.n_correspondences, res.n_bad + (res.n_correspondences - res.n_bad - nIn),
              left, same ? 1 : 0, (double)out[12]);
  return 0;
}
