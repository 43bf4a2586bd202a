// LocalMapping::CreateNewMapPoints over include/orbx_shim.hpp, POD build: two keyframes as arrays behind KeyFrameViews for a
// synthetic scene -- 3D points in front of both cameras, their projections as the two keyframes' features (KF2's in another order,
// with a few descriptor bits flipped and the angle turned by 20 degrees), a FeatureVector that puts a point's two features under
// one node -- then ORBmatcher::SearchForTriangulation(KF1, KF2, K, vMatchedPairs) and CreateNewMapPoints over its pairs.  The same
// inputs go through the C ABI (orbx_match_triangulation, orbx_triangulate_matches); both must give the same pairs and points.
// Usage: shim_tri <seed>; prints RESULT <pairs> <of them the true feature> <points> <worst |X - truth| / |truth|> <agree>.
#include <algorithm>
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
  const int n = 300;
  const float K[9] = {517.25f, 0.f, 318.75f, 0.f, 388.5f, 255.5f, 0.f, 0.f, 1.f};
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  // KF1 at the origin; KF2 turned by a about y, its centre at C
  const double a = 0.05, R[3][3] = {{std::cos(a), 0, std::sin(a)}, {0, 1, 0}, {-std::sin(a), 0, std::cos(a)}}, C[3] = {0.7, 0.05, 0.1};
  float pose1[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, pose2[12];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) pose2[r * 3 + c] = (float)R[r][c];
    pose2[9 + r] = (float)-(R[r][0] * C[0] + R[r][1] * C[1] + R[r][2] * C[2]);
  }
  std::vector<KeyPointT> keys1, keys2;
  std::vector<uint8_t> desc1, desc2;
  std::vector<int> order;  // KF2's features are filled in this order of the points
  for (int i = 0; i < n; i++) order.push_back(i);
  for (int i = n - 1; i > 0; i--) std::swap(order[i], order[rand() % (i + 1)]);
  std::vector<int> at2(n, -1);  // point -> KF2 feature
  std::vector<double> pts;
  std::vector<int> level;
  for (int i = 0; i < n; i++) {
    const double z = uniform(3, 9), u = uniform(20, 620), v = uniform(20, 460);
    pts.push_back((u - 318.75) / 517.25 * z);
    pts.push_back((v - 255.5) / 388.5 * z);
    pts.push_back(z);
    level.push_back(rand() % 4);
    KeyPointT k;
    k.pt.x = (float)u;
    k.pt.y = (float)v;
    k.octave = level[i];
    k.angle = (float)(rand() % 360);
    keys1.push_back(k);
    for (int b = 0; b < 32; b++) desc1.push_back((uint8_t)(rand() & 255));
  }
  DBoW2::FeatureVector fv1, fv2;
  for (int i = 0; i < n; i++) fv1[100 + i % 37].push_back((unsigned)i);
  for (int q = 0; q < n; q++) {
    const int i = order[q];
    double Y[3];
    for (int r = 0; r < 3; r++) Y[r] = R[r][0] * (pts[3 * i] - C[0]) + R[r][1] * (pts[3 * i + 1] - C[1]) + R[r][2] * (pts[3 * i + 2] - C[2]);
    const double u = 517.25 * Y[0] / Y[2] + 318.75, v = 388.5 * Y[1] / Y[2] + 255.5;
    if (Y[2] < 0.5 || u < 2 || u > 638 || v < 2 || v > 478) continue;  // (KF2 does not see it)
    KeyPointT k;
    k.pt.x = (float)u;
    k.pt.y = (float)v;
    k.octave = level[i];
    k.angle = (float)(((int)keys1[i].angle + 340) % 360);
    at2[i] = (int)keys2.size();
    keys2.push_back(k);
    for (int b = 0; b < 32; b++) desc2.push_back(desc1[32 * i + b]);
    for (int f = 0; f < 8; f++) desc2[desc2.size() - 32 + rand() % 32] ^= (uint8_t)(1 << (rand() % 8));
  }
  std::vector<std::pair<int, int> > byFeature;  // (ascending feature index inside a node, as ComputeBoW leaves it)
  for (int i = 0; i < n; i++)
    if (at2[i] >= 0) byFeature.push_back(std::make_pair(at2[i], i));
  std::sort(byFeature.begin(), byFeature.end());
  for (const auto& p : byFeature) fv2[100 + p.second % 37].push_back((unsigned)p.first);
  const int n2 = (int)keys2.size();

  KeyFrameView KF1, KF2;
  KF1.N = n;
  KF1.mvKeysUn = keys1.data();
  KF1.mDescriptors = desc1.data();
  KF1.mFeatVec = &fv1;
  KF1.mTcw = pose1;
  KF2.N = n2;
  KF2.mvKeysUn = keys2.data();
  KF2.mDescriptors = desc2.data();
  KF2.mFeatVec = &fv2;
  KF2.mTcw = pose2;

  ORBmatcher matcher(0.6f, true, &extractor);
  std::vector<std::pair<size_t, size_t> > vMatchedPairs;
  orbx_tri_match_result viaShim;
  const int npairs = matcher.SearchForTriangulation(KF1, KF2, K, vMatchedPairs, 0.0f, &viaShim);
  NewMapPoints made;
  const int npoints = CreateNewMapPoints(&extractor, KF1, KF2, K, vMatchedPairs, made);

  // the C ABI on the same inputs
  std::vector<uint32_t> node[2], feat[2];
  const DBoW2::FeatureVector* fv[2] = {&fv1, &fv2};
  for (int s = 0; s < 2; s++)
    for (const auto& kv : *fv[s])
      for (unsigned int i : kv.second) {
        node[s].push_back(kv.first);
        feat[s].push_back(i);
      }
  std::vector<int32_t> m12(n, -1);
  orbx_tri_match_result mres;
  int rc = orbx_match_triangulation(extractor.context(), reinterpret_cast<const orbx_keypoint*>(keys1.data()), desc1.data(), n, node[0].data(),
                                    feat[0].data(), (int)node[0].size(), nullptr, pose1, reinterpret_cast<const orbx_keypoint*>(keys2.data()),
                                    desc2.data(), n2, node[1].data(), feat[1].data(), (int)node[1].size(), nullptr, pose2, K, 0.0f, 1,
                                    m12.data(), &mres);
  if (rc != ORBX_OK) {
    std::printf("orbx_match_triangulation: %d\n", rc);
    return 1;
  }
  std::vector<float> P(3 * n), Nrm(3 * n), D(2 * n);
  std::vector<uint8_t> good(n);
  orbx_tri_result tres;
  rc = orbx_triangulate_matches(extractor.context(), reinterpret_cast<const orbx_keypoint*>(keys1.data()), n, pose1,
                                reinterpret_cast<const orbx_keypoint*>(keys2.data()), n2, pose2, K, m12.data(), P.data(), good.data(),
                                Nrm.data(), D.data(), &tres);
  if (rc != ORBX_OK) {
    std::printf("orbx_triangulate_matches: %d\n", rc);
    return 1;
  }
  bool same = npairs == mres.nmatches && std::memcmp(&viaShim, &mres, sizeof mres) == 0 && npoints == tres.n_points &&
              std::memcmp(&made.result, &tres, sizeof tres) == 0 && made.mWorldPos == P && made.mbGood == good && made.mNormalVector == Nrm &&
              made.mfMinMaxDistance == D;
  size_t q = 0;
  for (int i = 0; i < n; i++)  // the pairs are the row's entries in ascending KF1 index
    if (m12[i] >= 0) {
      same = same && q < vMatchedPairs.size() && vMatchedPairs[q].first == (size_t)i && vMatchedPairs[q].second == (size_t)m12[i];
      q++;
    }
  same = same && q == vMatchedPairs.size();
  int right = 0;
  double worst = 0;
  for (const auto& pr : vMatchedPairs) {
    const int i = (int)pr.first;
    if (at2[i] != (int)pr.second) continue;
    right++;
    if (!made.mbGood[i]) continue;
    double e = 0, nn = 0;
    for (int c = 0; c < 3; c++) {
      e = std::max(e, std::fabs((double)made.mWorldPos[3 * i + c] - pts[3 * i + c]));
      nn += pts[3 * i + c] * pts[3 * i + c];
    }
    worst = std::max(worst, e / std::sqrt(nn));
  }
  std::printf("RESULT %d %d %d %.3g %d\n", npairs, right, npoints, worst, (int)same);
  return same ? 0 : 2;
}
