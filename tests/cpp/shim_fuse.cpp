// Both overloads of ORBmatcher::Fuse over include/orbx_shim.hpp, POD build: a keyframe behind a KeyFrameView and map points behind
// a MapView (with their observation counts) for a synthetic scene -- the keyframe's features on the projections of the map points
// that land in the image in front of the camera, their descriptors copies with a few bits flipped, their octaves the predicted
// levels; a quarter of the features hold an unmapped point on entry, with 0 to 9 observations -- then ORBmatcher::Fuse(KF, Tcw,
// map, th, K, bounds, outcome) and the Scw overload under 1.25 * Tcw.  The same inputs go through the C ABI (orbx_fuse,
// orbx_fuse_scw); both must give the same rows, outputs and records.  Usage: shim_fuse <seed>; prints
// RESULT <nFused pose> <of them on the true feature> <nFused Scw> <replace points> <agree>.
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
  const double a = 0.03, R[3][3] = {{std::cos(a), 0, std::sin(a)}, {0, 1, 0}, {-std::sin(a), 0, std::cos(a)}}, t[3] = {0.1, -0.05, 0.1};
  PoseT Tcw, Scw;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {
      Tcw(r, c) = (float)R[r][c];
      Scw(r, c) = (float)(1.25 * R[r][c]);
    }
    Tcw(r, 3) = (float)t[r];
    Scw(r, 3) = (float)(1.25 * t[r]);
  }
  double Ow[3];  // -R^T t
  for (int c = 0; c < 3; c++) Ow[c] = -(R[0][c] * t[0] + R[1][c] * t[1] + R[2][c] * t[2]);
  std::vector<float> pos(3 * n), nrm(3 * n), dist(2 * n);
  std::vector<uint8_t> mdesc(32 * n), good(n);
  std::vector<int32_t> obs(n);
  std::vector<KeyPointT> keys;
  std::vector<uint8_t> kdesc;
  std::vector<int> entry, occObs, truth;  // per feature: its row entry, its unmapped occupant's count, the point it shows
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
    dist[2 * i + 1] = (float)(d * std::pow(1.2, level) * 0.95);  // PredictScale gives `level`
    dist[2 * i] = dist[2 * i + 1] / 4.f;
    good[i] = i % 9 != 0;
    obs[i] = 1 + rand() % 9;
    for (int b = 0; b < 32; b++) mdesc[32 * i + b] = (uint8_t)(rand() & 255);
    if (z < 0 || u < 2 || u > 630 || v < 2 || v > 470 || i % 5 == 0) continue;  // (no feature shows it)
    KeyPointT k;
    k.pt.x = (float)(u + uniform(-0.7, 0.7));
    k.pt.y = (float)(v + uniform(-0.7, 0.7));
    k.octave = level;
    keys.push_back(k);
    for (int b = 0; b < 32; b++) kdesc.push_back(mdesc[32 * i + b]);
    for (int f = 0; f < 10; f++) kdesc[kdesc.size() - 32 + rand() % 32] ^= (uint8_t)(1 << (rand() % 8));
    truth.push_back(i);
    entry.push_back(i % 4 == 1 ? ORBX_FUSE_OCCUPIED_UNMAPPED : -1);
    occObs.push_back(rand() % 10);
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
  map.mnObs = obs.data();

  ORBmatcher matcher(0.75f, true, &extractor);
  bool same = true;
  int fused[2] = {0, 0}, right = 0, replace = 0;
  for (int form = 0; form < 2; form++) {
    const PoseT& T = form ? Scw : Tcw;
    float t12[12];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) t12[r * 3 + c] = (float)T(r, c);
      t12[9 + r] = (float)T(r, 3);
    }
    // the C ABI
    std::vector<int32_t> rowC(entry.begin(), entry.end()), occC(occObs.begin(), occObs.end()), idx(n), other(n);
    if (rowC.empty()) { rowC.push_back(-1); occC.push_back(-1); }
    std::vector<uint8_t> act(n);
    orbx_fuse_result res;
    const orbx_keypoint* kps = reinterpret_cast<const orbx_keypoint*>(keys.data());
    const int rc = form ? orbx_fuse_scw(extractor.context(), kps, kdesc.data(), KF.N, n, pos.data(), nrm.data(), dist.data(), mdesc.data(),
                                        good.data(), t12, K, &bounds, 4.f, 50, rowC.data(), occC.data(), idx.data(), act.data(),
                                        other.data(), &res)
                        : orbx_fuse(extractor.context(), kps, kdesc.data(), KF.N, n, pos.data(), nrm.data(), dist.data(), mdesc.data(),
                                    good.data(), obs.data(), t12, K, &bounds, 3.f, 50, rowC.data(), occC.data(), idx.data(), act.data(),
                                    other.data(), &res);
    if (rc != ORBX_OK) {
      std::printf("orbx_fuse%s: %d\n", form ? "_scw" : "", rc);
      return 1;
    }
    // the shim
    FuseOutcome out;
    std::vector<int> row(entry), vpReplacePoint;
    fused[form] = form ? matcher.Fuse(KF, T, map, 4.f, vpReplacePoint, K, bounds, out, &row, &occObs)
                       : matcher.Fuse(KF, T, map, 3.f, K, bounds, out, &row, &occObs);
    same = same && fused[form] == res.n_fused && std::memcmp(&out.result, &res, sizeof res) == 0 && (int)row.size() == KF.N &&
           (int)out.vnFeature.size() == n;
    for (int j = 0; same && j < KF.N; j++) same = row[j] == rowC[j];
    for (int i = 0; same && i < n; i++) {
      same = out.vnFeature[i] == idx[i] && out.vnAction[i] == act[i] && out.vnOccupant[i] == other[i];
      if (form) {
        same = same && vpReplacePoint[i] == (act[i] == ORBX_FUSE_KEEP_OCCUPANT ? other[i] : -1);
        replace += vpReplacePoint[i] != -1;
      } else if (idx[i] >= 0) {
        right += truth[idx[i]] == i;
      }
    }
  }
  std::printf("RESULT %d %d %d %d %d\n", fused[0], right, fused[1], replace, (int)same);
  return same ? 0 : 2;
}
