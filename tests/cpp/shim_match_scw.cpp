// The loop-closing SearchByProjection under Scw over include/orbx_shim.hpp, POD build: the current keyframe behind a KeyFrameView
// and the loop's map points behind a MapView for a synthetic scene -- a similarity Scw with scale 1.25, the keyframe's features
// on the projections of the map points that land in the image in front of the camera, their descriptors copies with a few bits
// flipped, their octaves the predicted levels, a fifth of them already matched on entry -- then
// ORBmatcher::SearchByProjection(KF, Scw, map, vpMatched, th, K, bounds).  The same inputs go through the C ABI
// (orbx_match_scw); both must give the same row and the same record.  Usage: shim_match_scw <seed>; prints
// RESULT <new matches> <of them the true feature> <features without an entry> <nTotalMatches> <agree>.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }

int main(int argc, char** argv) {
  srand(argc > 1 ? atoi(argv[1]) : 0);
  const int n = 400;
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  const float K[9] = {517.25f, 0.f, 318.75f, 0.f, 388.5f, 255.5f, 0.f, 0.f, 1.f};
  const orbx_bounds bounds{0, 640, 0, 480};
  const double s = 1.25, a = 0.03, R[3][3] = {{std::cos(a), 0, std::sin(a)}, {0, 1, 0}, {-std::sin(a), 0, std::cos(a)}},
               t[3] = {0.1, -0.05, 0.1};
  PoseT Scw;  // s * [R | t]: Rcw = R, tcw = t
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Scw(r, c) = (float)(s * R[r][c]);
    Scw(r, 3) = (float)(s * t[r]);
  }
  double Ow[3];  // -R^T t
  for (int c = 0; c < 3; c++) Ow[c] = -(R[0][c] * t[0] + R[1][c] * t[1] + R[2][c] * t[2]);
  std::vector<float> pos(3 * n), nrm(3 * n), dist(2 * n);
  std::vector<uint8_t> mdesc(32 * n), good(n);
  std::vector<KeyPointT> keys;
  std::vector<uint8_t> kdesc;
  std::vector<int> entry, truth;  // per feature: the map point it has on entry (-1 none), the point it shows
  for (int i = 0; i < n; i++) {
    const double z = uniform(3, 15) * (i % 11 == 3 ? -1 : 1), u = uniform(-150, 790), v = uniform(-100, 580);
    const double Y[3] = {(u - 318.75) / 517.25 * z, (v - 255.5) / 388.5 * z, z};
    double X[3], d = 0;  // X = R^T (Y - t)
    for (int c = 0; c < 3; c++) X[c] = R[0][c] * (Y[0] - t[0]) + R[1][c] * (Y[1] - t[1]) + R[2][c] * (Y[2] - t[2]);
    for (int c = 0; c < 3; c++) d += (X[c] - Ow[c]) * (X[c] - Ow[c]);
    d = std::sqrt(d);
    const int level = rand() % 8;
    for (int c = 0; c < 3; c++) {
      pos[3 * i + c] = (float)X[c];
      nrm[3 * i + c] = (float)((X[c] - Ow[c]) / d);  // seen head-on
    }
    dist[2 * i + 1] = (float)(d * std::pow(1.2, level) * 0.95);  // PredictScale gives `level` (0 for level 0: the ratio is below 1)
    dist[2 * i] = dist[2 * i + 1] / 4.f;
    good[i] = i % 9 != 0;
    for (int b = 0; b < 32; b++) mdesc[32 * i + b] = (uint8_t)(rand() & 255);
    if (z < 0 || u < 2 || u > 630 || v < 2 || v > 470 || i % 5 == 0) continue;  // (no feature shows it)
    KeyPointT k;
    k.pt.x = (float)(u + uniform(-1, 1));
    k.pt.y = (float)(v + uniform(-1, 1));
    k.octave = level;
    keys.push_back(k);
    for (int b = 0; b < 32; b++) kdesc.push_back(mdesc[32 * i + b]);
    for (int f = 0; f < 10; f++) kdesc[kdesc.size() - 32 + rand() % 32] ^= (uint8_t)(1 << (rand() % 8));
    truth.push_back(i);
    entry.push_back(i % 4 == 1 ? i : -1);
  }
  KeyFrameView KF;
  KF.N = (int)keys.size();
  KF.mvKeysUn = keys.data();
  KF.mDescriptors = kdesc.data();
  MapView map;
  map.N = n;
  map.mWorldPos = pos.data();
  map.mNormalVector = nrm.data();
  map.mfMinMaxDistance = dist.data();
  map.mDescriptors = mdesc.data();
  map.mbGood = good.data();

  // the C ABI on the same inputs
  float scw[12];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) scw[r * 3 + c] = (float)Scw(r, c);
    scw[9 + r] = (float)Scw(r, 3);
  }
  std::vector<int32_t> viaC(entry.begin(), entry.end());
  if (viaC.empty()) viaC.push_back(-1);
  orbx_scw_result res;
  const int rc = orbx_match_scw(extractor.context(), reinterpret_cast<const orbx_keypoint*>(keys.data()), kdesc.data(), KF.N, n, pos.data(),
                                nrm.data(), dist.data(), mdesc.data(), good.data(), scw, K, &bounds, 10.f, 50, viaC.data(), nullptr, 0,
                                &res);
  if (rc != ORBX_OK) {
    std::printf("orbx_match_scw: %d\n", rc);
    return 1;
  }

  ORBmatcher matcher(0.75f, true, &extractor);
  std::vector<int> vpMatched(entry);
  orbx_scw_result viaShim;
  const int nmatches = matcher.SearchByProjection(KF, Scw, map, vpMatched, 10.f, K, bounds, 50, &viaShim);
  bool same = nmatches == res.nmatches && std::memcmp(&viaShim, &res, sizeof res) == 0 && (int)vpMatched.size() == KF.N;
  int right = 0, searched = 0;
  for (int j = 0; same && j < KF.N; j++) {
    same = same && vpMatched[j] == viaC[j];
    if (entry[j] >= 0) {  // an entry stays
      same = same && vpMatched[j] == entry[j];
      continue;
    }
    searched += good[truth[j]];
    right += vpMatched[j] == truth[j];
  }
  std::printf("RESULT %d %d %d %d %d\n", nmatches, right, searched, res.n_total, (int)same);
  return same ? 0 : 2;
}
