// Tracking::SearchLocalPoints over include/orbx_shim.hpp, POD build: a Frame-like type that holds what the reference's Frame has
// (mvKeysUn, mDescriptors, N, mpORBextractor, mK, the static bounds) and a local map as arrays behind a MapView for a synthetic
// scene -- the frame's features are the projections of the map points in front of the camera, their descriptors copies with a
// few bits flipped, a fifth of them already matched on entry -- then ORBmatcher::SearchByProjection(F, map, th, Tcw, vnMatches)
// on the frame and on a FrameView of it.  The same inputs go through the C ABI (orbx_match_local_map); all three must give the
// same rows.  Usage: shim_match_local <seed>; prints RESULT <new matches> <of them the true feature> <points searched that have
// a feature> <agree>.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

struct Frame {
  std::vector<KeyPointT> mvKeysUn;
  std::vector<uint8_t> mDescriptors;
  int N = 0;
  ORBextractor* mpORBextractor = nullptr;
  float mK[9] = {517.25f, 0.f, 318.75f, 0.f, 388.5f, 255.5f, 0.f, 0.f, 1.f};
  static int mnMinX, mnMaxX, mnMinY, mnMaxY;
};
int Frame::mnMinX = 0, Frame::mnMaxX = 640, Frame::mnMinY = 0, Frame::mnMaxY = 480;

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }

int main(int argc, char** argv) {
  srand(argc > 1 ? atoi(argv[1]) : 0);
  const int n = 400;
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  Frame F;
  F.mpORBextractor = &extractor;
  const double a = 0.03, R[3][3] = {{std::cos(a), 0, std::sin(a)}, {0, 1, 0}, {-std::sin(a), 0, std::cos(a)}}, t[3] = {0.1, -0.05, 0.1};
  PoseT Tcw;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Tcw(r, c) = (float)R[r][c];
    Tcw(r, 3) = (float)t[r];
  }
  double Ow[3];  // -R^T t
  for (int c = 0; c < 3; c++) Ow[c] = -(R[0][c] * t[0] + R[1][c] * t[1] + R[2][c] * t[2]);
  std::vector<float> pos(3 * n), normal(3 * n), dist(2 * n);
  std::vector<uint8_t> mdesc(32 * n), good(n);
  std::vector<int> entry, truth;  // per feature: the point it has on entry (-1 none), the point it shows
  for (int i = 0; i < n; i++) {
    const double z = uniform(3, 15) * (i % 11 == 3 ? -1 : 1), u = uniform(-150, 790), v = uniform(-100, 580);
    const double Y[3] = {(u - 318.75) / 517.25 * z, (v - 255.5) / 388.5 * z, z};
    double X[3], PO[3], d = 0;  // X = R^T (Y - t)
    for (int c = 0; c < 3; c++) X[c] = R[0][c] * (Y[0] - t[0]) + R[1][c] * (Y[1] - t[1]) + R[2][c] * (Y[2] - t[2]);
    for (int c = 0; c < 3; c++) { PO[c] = X[c] - Ow[c]; d += PO[c] * PO[c]; }
    d = std::sqrt(d);
    const int level = rand() % 8;
    for (int c = 0; c < 3; c++) { pos[3 * i + c] = (float)X[c]; normal[3 * i + c] = (float)(PO[c] / d * (i % 7 == 2 ? -1 : 1)); }
    dist[2 * i + 1] = (float)(d * std::pow(1.2, level) * 0.95);  // PredictScale gives `level` (0 for level 0: the ratio is below 1)
    dist[2 * i] = dist[2 * i + 1] / 4.f;
    good[i] = i % 9 != 0;
    for (int b = 0; b < 32; b++) mdesc[32 * i + b] = (uint8_t)(rand() & 255);
    if (z < 0 || u < 2 || u > 630 || v < 2 || v > 470 || i % 5 == 0) continue;  // (no feature shows it)
    KeyPointT k;
    k.pt.x = (float)(u + uniform(-1, 1));
    k.pt.y = (float)(v + uniform(-1, 1));
    k.octave = level;
    k.angle = (float)(rand() % 360);
    F.mvKeysUn.push_back(k);
    for (int b = 0; b < 32; b++) F.mDescriptors.push_back(mdesc[32 * i + b]);
    for (int f = 0; f < 10; f++) F.mDescriptors[F.mDescriptors.size() - 32 + rand() % 32] ^= (uint8_t)(1 << (rand() % 8));
    truth.push_back(i);
    entry.push_back(i % 4 == 1 ? i : -1);
  }
  F.N = (int)F.mvKeysUn.size();
  std::vector<bool> vbOutlier(F.N);
  for (int j = 0; j < F.N; j++) vbOutlier[j] = entry[j] >= 0 && j % 3 == 0;
  MapView map;
  map.N = n;
  map.mWorldPos = pos.data();
  map.mNormalVector = normal.data();
  map.mfMinMaxDistance = dist.data();
  map.mDescriptors = mdesc.data();
  map.mbGood = good.data();

  // the C ABI on the same inputs
  float pose[12];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) pose[r * 3 + c] = (float)Tcw(r, c);
    pose[9 + r] = (float)Tcw(r, 3);
  }
  std::vector<uint8_t> out(F.N > 0 ? F.N : 1), viewC(n);
  for (int j = 0; j < F.N; j++) out[j] = vbOutlier[j];
  const orbx_bounds b{Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY};
  std::vector<int32_t> viaC(entry.begin(), entry.end());
  if (viaC.empty()) viaC.push_back(-1);
  orbx_local_result res;
  const int rc = orbx_match_local_map(extractor.context(), reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data()), F.mDescriptors.data(),
                                      F.N, n, pos.data(), normal.data(), dist.data(), mdesc.data(), good.data(), pose, F.mK, &b, 1.f, 0.8f,
                                      viaC.data(), out.data(), viewC.data(), &res);
  if (rc != ORBX_OK) {
    std::printf("orbx_match_local_map: %d\n", rc);
    return 1;
  }

  ORBmatcher matcher(0.8f, true);
  std::vector<int> vnMatches(entry), viaViews(entry);
  std::vector<uint8_t> view, viewViews;
  orbx_local_result viaShim;
  const int nmatches = matcher.SearchByProjection(F, map, 1.f, Tcw, vnMatches, &vbOutlier, &view, &viaShim);
  ORBmatcher onViews(0.8f, true, &extractor);
  const int nviews = onViews.SearchByProjection(ORBmatcher::frameView(F), map, 1.f, Tcw, F.mK, viaViews, &vbOutlier, &viewViews);
  bool same = nmatches == res.nmatches && nviews == nmatches && std::memcmp(&viaShim, &res, sizeof res) == 0 &&
              (int)vnMatches.size() == F.N && viaViews == vnMatches && view == viewC && viewViews == viewC;
  int right = 0, searched = 0;
  for (int j = 0; same && j < F.N; j++) {
    same = same && vnMatches[j] == viaC[j];
    if (entry[j] >= 0) {  // kept, or cleared as an outlier -- unless a point in view took the freed feature
      same = same && (vbOutlier[j] ? vnMatches[j] != entry[j] : vnMatches[j] == entry[j]);
      continue;
    }
    searched += good[truth[j]] && view[truth[j]] < ORBX_LOCAL_SEEN;
    right += vnMatches[j] == truth[j];
  }
  std::printf("RESULT %d %d %d %d\n", nmatches, right, searched, (int)same);
  return same ? 0 : 2;
}
