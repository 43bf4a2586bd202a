// LoopClosing::ComputeSim3's solver over include/orbx_shim.hpp, POD build: two KeyFrame-like objects that hold what the
// reference's KeyFrame has (mvKeysUn, mpORBextractor, mK) for a synthetic scene seen by two cameras whose maps differ by a
// similarity with scale 1.25, map points as coordinates with a has-point flag per feature, a fifth of the matches gross
// mismatches, then Sim3Solver(KF1, ..., KF2, ..., vnMatches12, false), SetRansacParameters(0.99, 20, 300) and iterate(5) in
// turns, as ComputeSim3 calls it.  The same inputs and the same rand() values go through the C ABI (orbx_sim3_solve); both must
// give the same bytes, and the turn in which the similarity arrives must be found_it's.  Then ORBmatcher::SearchBySim3 on the
// solver's row and similarity, through the shim and through orbx_match_sim3: the same bytes again; it finds the ten true pairs
// the row lacks (line MATCHER <found> <one-sided>).
// Usage: shim_sim3 <seed>; prints RESULT <status> <inliers> <correspondences> <planted mismatches among the inliers> <turns>
// <agrees with the C ABI>.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

struct KeyFrame {
  std::vector<KeyPointT> mvKeysUn;
  ORBextractor* mpORBextractor = nullptr;
  float mK[9] = {517.25f, 0.f, 318.75f, 0.f, 388.5f, 255.5f, 0.f, 0.f, 1.f};
};

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }

int main(int argc, char** argv) {
  const int seed = argc > 1 ? atoi(argv[1]) : 0;
  srand(seed);
  const int n = 150, planted = 30, nf = n + 8;
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  KeyFrame KF1, KF2;
  KF1.mpORBextractor = KF2.mpORBextractor = &extractor;
  KF1.mvKeysUn.resize(nf);
  KF2.mvKeysUn.resize(nf);
  // Y1 = s R Y2 + t between the camera frames; KF1's map is its camera frame moved by t1, KF2's its own camera frame
  const double a = 0.06, R[3][3] = {{std::cos(a), 0, std::sin(a)}, {0, 1, 0}, {-std::sin(a), 0, std::cos(a)}}, t[3] = {0.3, -0.1, 0.2};
  const double s = 1.25, t1[3] = {0.5, -1.0, 2.0};
  std::vector<Point3T> vP3D1(nf), vP3D2(nf);
  std::vector<bool> vbHas1(nf, false), vbHas2(nf, false);
  std::vector<int> vnMatches12(nf, -1);
  // for the matcher behind the solver: the features at the points' projections, a descriptor per physical point in both
  // keyframes, and distance ranges under which PredictScale returns the features' octave
  std::vector<uint8_t> desc1((size_t)nf * 32), desc2((size_t)nf * 32);
  std::vector<float> dist1((size_t)nf * 2, 1.f), dist2((size_t)nf * 2, 1.f);
  for (auto& b : desc1) b = (uint8_t)rand();
  for (auto& b : desc2) b = (uint8_t)rand();
  PoseT Tcw1, Tcw2;
  for (int r = 0; r < 3; r++) Tcw1(r, 3) = t1[r];
  for (int i = 0; i < n; i++) {
    const int j = n - 1 - i;  // KF2 holds the points in reverse
    const double z = uniform(4, 20), Y2[3] = {uniform(-0.45, 0.45) * z, uniform(-0.32, 0.32) * z, z};
    double Y1[3];
    for (int r = 0; r < 3; r++) Y1[r] = s * (R[r][0] * Y2[0] + R[r][1] * Y2[1] + R[r][2] * Y2[2]) + t[r];
    const double off = i < planted ? 2.0 : 0.0;  // (the first matches are gross mismatches: two units off)
    vP3D1[i].x = (float)(Y1[0] - t1[0]);
    vP3D1[i].y = (float)(Y1[1] - t1[1]);
    vP3D1[i].z = (float)(Y1[2] - t1[2]);
    vP3D2[j].x = (float)(Y2[0] + off + uniform(-0.002, 0.002));
    vP3D2[j].y = (float)(Y2[1] - off + uniform(-0.002, 0.002));
    vP3D2[j].z = (float)(Y2[2] + uniform(-0.002, 0.002));
    const int level = rand() % 8;
    KF1.mvKeysUn[i].octave = KF2.mvKeysUn[j].octave = level;
    KF1.mvKeysUn[i].pt.x = (float)(517.25 * Y1[0] / Y1[2] + 318.75);
    KF1.mvKeysUn[i].pt.y = (float)(388.5 * Y1[1] / Y1[2] + 255.5);
    KF2.mvKeysUn[j].pt.x = (float)(517.25 * Y2[0] / Y2[2] + 318.75);
    KF2.mvKeysUn[j].pt.y = (float)(388.5 * Y2[1] / Y2[2] + 255.5);
    std::memcpy(&desc2[(size_t)j * 32], &desc1[(size_t)i * 32], 32);
    const double d1 = std::sqrt(Y1[0] * Y1[0] + Y1[1] * Y1[1] + Y1[2] * Y1[2]), d2 = std::sqrt(Y2[0] * Y2[0] + Y2[1] * Y2[1] + Y2[2] * Y2[2]);
    dist1[2 * i] = (float)(0.3 * d2);
    dist1[2 * i + 1] = (float)(0.95 * d2 * std::pow(1.2, level));  // (KF1's point is searched at its distance from camera 2)
    dist2[2 * j] = (float)(0.3 * d1);
    dist2[2 * j + 1] = (float)(0.95 * d1 * std::pow(1.2, level));
    vbHas1[i] = vbHas2[j] = true;
    vnMatches12[i] = (i >= planted && i < planted + 10) ? -1 : j;  // (ten true pairs are left for SearchBySim3 to find)
  }
  vnMatches12[n] = n + 1;  // a match between two features without a point

  // the C ABI on the same inputs and the rand() values the shim will draw
  std::vector<float> p1(3 * nf), p2(3 * nf);
  std::vector<uint8_t> h1(nf), h2(nf), inl(nf);
  std::vector<int32_t> match(vnMatches12.begin(), vnMatches12.end()), row(nf);
  for (int i = 0; i < nf; i++) {
    p1[3 * i] = vP3D1[i].x; p1[3 * i + 1] = vP3D1[i].y; p1[3 * i + 2] = vP3D1[i].z;
    p2[3 * i] = vP3D2[i].x; p2[3 * i + 1] = vP3D2[i].y; p2[3 * i + 2] = vP3D2[i].z;
    h1[i] = vbHas1[i];
    h2[i] = vbHas2[i];
  }
  float pose1[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, (float)t1[0], (float)t1[1], (float)t1[2]}, pose2[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  srand(seed + 1000);
  std::vector<int32_t> draws(3 * 300);
  for (size_t i = 0; i < draws.size(); i++) draws[i] = rand();
  orbx_sim3_result res;
  float sim[13];
  const int rc = orbx_sim3_solve(extractor.context(), reinterpret_cast<const orbx_keypoint*>(KF1.mvKeysUn.data()), nf, p1.data(), h1.data(),
                                 pose1, reinterpret_cast<const orbx_keypoint*>(KF2.mvKeysUn.data()), nf, p2.data(), h2.data(), pose2,
                                 match.data(), KF1.mK, nullptr, 0, 0.99, 20, 300, 9.210f, 300, draws.data(), &res, sim, row.data(),
                                 inl.data());
  if (rc != ORBX_OK) {
    std::printf("orbx_sim3_solve: %d\n", rc);
    return 1;
  }

  srand(seed + 1000);
  Sim3Solver solver(KF1, vP3D1, vbHas1, Tcw1, KF2, vP3D2, vbHas2, Tcw2, vnMatches12, false);
  solver.SetRansacParameters(0.99, 20, 300);
  std::vector<bool> vbInliers;
  int nInliers = 0, turns = 0;
  bool bNoMore = false;
  Sim3Solver::Mat T12;
  while (T12.empty() && !bNoMore) {
    T12 = solver.iterate(5, bNoMore, vbInliers, nInliers);
    turns++;
  }
  bool same = std::memcmp(&solver.result(), &res, sizeof res) == 0 && !T12.empty() && nInliers == res.n_inliers &&
              vbInliers.size() == inl.size() && res.found_it >= 0 && turns == res.found_it / 5 + 1 && !bNoMore &&
              solver.GetEstimatedScale() == sim[12] && std::memcmp(solver.GetEstimatedRotation(), sim, 9 * sizeof(float)) == 0 &&
              std::memcmp(solver.GetEstimatedTranslation(), sim + 9, 3 * sizeof(float)) == 0 &&
              std::memcmp(solver.inlierMatches().data(), row.data(), nf * sizeof(int32_t)) == 0;
  for (int r = 0; same && r < 3; r++) {
    for (int c = 0; c < 3; c++) same = same && T12.at(r, c) == sim[12] * sim[r * 3 + c];
    same = same && T12.at(r, 3) == sim[9 + r];
  }
  int wrong = 0;
  for (size_t i = 0; same && i < inl.size(); i++) {
    same = same && vbInliers[i] == (inl[i] != 0);
    wrong += (int)i < planted && inl[i];
  }
  // SearchBySim3 behind it, as ComputeSim3 calls it: the row of the solver's inliers, widened under the similarity found
  const orbx_bounds bounds = {0, 640, 0, 480};
  std::vector<int32_t> rowC(row);
  orbx_msim3_result mres, mresShim;
  const int rm = orbx_match_sim3(extractor.context(), reinterpret_cast<const orbx_keypoint*>(KF1.mvKeysUn.data()), desc1.data(), nf, p1.data(),
                                 h1.data(), nullptr, dist1.data(), pose1, reinterpret_cast<const orbx_keypoint*>(KF2.mvKeysUn.data()),
                                 desc2.data(), nf, p2.data(), h2.data(), nullptr, dist2.data(), pose2, sim, KF1.mK, &bounds, 7.5f, 100,
                                 rowC.data(), &mres);
  if (rm != ORBX_OK) {
    std::printf("orbx_match_sim3: %d\n", rm);
    return 1;
  }
  KeyFrameView V1, V2;
  V1.N = V2.N = nf;
  V1.mvKeysUn = KF1.mvKeysUn.data(); V2.mvKeysUn = KF2.mvKeysUn.data();
  V1.mDescriptors = desc1.data(); V2.mDescriptors = desc2.data();
  V1.mWorldPos = p1.data(); V2.mWorldPos = p2.data();
  V1.mfMinMaxDistance = dist1.data(); V2.mfMinMaxDistance = dist2.data();
  V1.mbGood = h1.data(); V2.mbGood = h2.data();
  V1.mTcw = pose1; V2.mTcw = pose2;
  std::vector<int> vpMatches12(solver.inlierMatches().begin(), solver.inlierMatches().end());
  ORBmatcher matcher(0.75f, true, &extractor);
  const int nFound = matcher.SearchBySim3(V1, V2, vpMatches12, solver.GetEstimatedScale(), solver.GetEstimatedRotation(),
                                          solver.GetEstimatedTranslation(), 7.5f, KF1.mK, bounds, &mresShim);
  same = same && nFound == mres.n_found && std::memcmp(&mres, &mresShim, sizeof mres) == 0 && mres.status == 0;
  for (int i = 0; same && i < nf; i++) same = same && vpMatches12[i] == rowC[i] && (row[i] < 0 || rowC[i] == row[i]);
  std::printf("RESULT %d %d %d %d %d %d\n", res.status, nInliers, res.n_correspondences, wrong, turns, (int)same);
  std::printf("MATCHER %d found, %d one-sided\n", mres.n_found, mres.n_one_sided);
  std::printf("s12 %.5f (1.25)\n", res.s12);
  return same ? 0 : 2;
}
