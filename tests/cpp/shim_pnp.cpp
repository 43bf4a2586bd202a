// Tracking::Relocalization's solver over include/orbx_shim.hpp, POD build: a Frame-like object that holds what the reference's
// Frame has (mvKeysUn, mpORBextractor, mK) for a synthetic scene, map points as coordinates with a has-point flag per feature,
// a fifth of them gross mismatches, then PnPsolver(F, vP3D, vbHasPoint), SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) and
// iterate(5) in turns, as Relocalization calls it.  The same inputs and the same rand() values go through the C ABI
// (orbx_pnp_solve); both must give the same bytes, and the turn in which the pose arrives must be found_it's.
// Usage: shim_pnp <seed>; prints RESULT <status> <inliers> <correspondences> <planted mismatches among the inliers> <turns>
// <agrees with the C ABI>.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

struct Frame {
  std::vector<KeyPointT> mvKeysUn;
  ORBextractor* mpORBextractor = nullptr;
  float mK[9] = {517.25f, 0.f, 318.75f, 0.f, 388.5f, 255.5f, 0.f, 0.f, 1.f};
};

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }

int main(int argc, char** argv) {
  const int seed = argc > 1 ? atoi(argv[1]) : 0;
  srand(seed);
  const int n = 150, planted = 30;
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  Frame F;
  F.mpORBextractor = &extractor;
  const double a = 0.04, R[3][3] = {{std::cos(a), 0, std::sin(a)}, {0, 1, 0}, {-std::sin(a), 0, std::cos(a)}}, t[3] = {0.3, -0.1, 0.2};
  F.mvKeysUn.resize(n + 8);
  std::vector<Point3T> vP3D(n + 8);
  std::vector<bool> vbHasPoint(n + 8, false);
  for (int i = 0; i < n; i++) {
    const double z = uniform(4, 20), Y[3] = {uniform(-0.5, 0.5) * z, uniform(-0.4, 0.4) * z, z};
    double X[3];  // R^T (Y - t)
    for (int c = 0; c < 3; c++) X[c] = R[0][c] * (Y[0] - t[0]) + R[1][c] * (Y[1] - t[1]) + R[2][c] * (Y[2] - t[2]);
    KeyPointT& k = F.mvKeysUn[i];
    k.octave = rand() % 8;
    const double s = std::pow(1.2, k.octave), off = i < planted ? 30 * s : 0;  // (the first features are gross mismatches)
    k.pt.x = (float)(517.25 * Y[0] / Y[2] + 318.75 + uniform(-0.5, 0.5) * s + off);
    k.pt.y = (float)(388.5 * Y[1] / Y[2] + 255.5 + uniform(-0.5, 0.5) * s - off);
    vP3D[i].x = (float)X[0];
    vP3D[i].y = (float)X[1];
    vP3D[i].z = (float)X[2];
    vbHasPoint[i] = true;
  }

  // the C ABI on the same inputs and the rand() values the shim will draw
  std::vector<float> p3d(3 * vP3D.size());
  std::vector<uint8_t> has(vP3D.size()), inl(vP3D.size());
  for (size_t i = 0; i < vP3D.size(); i++) {
    p3d[3 * i] = vP3D[i].x; p3d[3 * i + 1] = vP3D[i].y; p3d[3 * i + 2] = vP3D[i].z;
    has[i] = vbHasPoint[i];
  }
  srand(seed + 1000);
  std::vector<int32_t> draws(4 * 300);
  for (size_t i = 0; i < draws.size(); i++) draws[i] = rand();
  orbx_pnp_result res;
  const int rc = orbx_pnp_solve(extractor.context(), reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data()), (int)F.mvKeysUn.size(),
                                p3d.data(), has.data(), F.mK, nullptr, 0.99, 10, 300, 0.5f, 5.991f, 300, draws.data(), &res, inl.data());
  if (rc != ORBX_OK) {
    std::printf("orbx_pnp_solve: %d\n", rc);
    return 1;
  }

  srand(seed + 1000);
  PnPsolver solver(F, vP3D, vbHasPoint);
  solver.SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);
  std::vector<bool> vbInliers;
  int nInliers = 0, turns = 0;
  bool bNoMore = false;
  PnPsolver::Mat Tcw;
  while (Tcw.empty() && !bNoMore) {
    Tcw = solver.iterate(5, bNoMore, vbInliers, nInliers);
    turns++;
  }
  bool same = std::memcmp(&solver.result(), &res, sizeof res) == 0 && !Tcw.empty() && nInliers == res.n_inliers &&
              vbInliers.size() == inl.size() && res.refined == 1 && turns == res.found_it / 5 + 1 && !bNoMore;
  for (int r = 0; same && r < 3; r++) {
    for (int c = 0; c < 3; c++) same = same && Tcw.at(r, c) == res.Tcw[r * 3 + c];
    same = same && Tcw.at(r, 3) == res.Tcw[9 + r];
  }
  int wrong = 0;
  for (size_t i = 0; same && i < inl.size(); i++) {
    same = same && vbInliers[i] == (inl[i] != 0);
    wrong += (int)i < planted && inl[i];
  }
  std::printf("RESULT %d %d %d %d %d %d\n", res.status, nInliers, res.n_correspondences, wrong, turns, (int)same);
  return same ? 0 : 2;
}
