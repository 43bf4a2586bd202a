// Tracking::CreateInitialMapMonocular's adjustment over include/orbx_shim.hpp, POD build: two Frame-like objects that hold what
// the reference's Frame has (mvKeysUn, mpORBextractor, mK) for a synthetic general scene, the values Initializer::Initialize
// would have returned (a perturbed pose, noisy points), then Optimizer::BundleAdjustmentTwoView(F1, F2, vMatches12, Tcw, vP3D,
// vbTriangulated, 20).  The same inputs go through the C ABI (orbx_bundle_adjust); both must give the same bytes.
// Usage: shim_ba <seed>; prints RESULT <status> <iterations> <n points> <agrees with the C ABI>.
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
  float mK[9] = {520.f, 0.f, 320.f, 0.f, 520.f, 240.f, 0.f, 0.f, 1.f};
};

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }

int main(int argc, char** argv) {
  srand(argc > 1 ? atoi(argv[1]) : 0);
  const int n = 180;
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  Frame F1, F2;
  F1.mpORBextractor = F2.mpORBextractor = &extractor;
  // the true motion: a small rotation about y, a sideways step
  const double a = -0.05, R[3][3] = {{std::cos(a), 0, std::sin(a)}, {0, 1, 0}, {-std::sin(a), 0, std::cos(a)}}, t[3] = {-0.3, 0.02, 0.05};
  std::vector<int> vMatches12(n + 10, -1);
  std::vector<Point3T> vP3D(n + 10);
  std::vector<bool> vbTriangulated(n + 10, false);
  F1.mvKeysUn.resize(n + 10);
  F2.mvKeysUn.resize(n);
  for (int i = 0; i < n; i++) {
    const double X[3] = {uniform(-2, 2), uniform(-1.5, 1.5), uniform(4, 8)};
    double Y[3];
    for (int r = 0; r < 3; r++) Y[r] = R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + t[r];
    KeyPointT &k1 = F1.mvKeysUn[i], &k2 = F2.mvKeysUn[n - 1 - i];
    k1.pt.x = (float)(520 * X[0] / X[2] + 320 + uniform(-0.5, 0.5));
    k1.pt.y = (float)(520 * X[1] / X[2] + 240 + uniform(-0.5, 0.5));
    k2.pt.x = (float)(520 * Y[0] / Y[2] + 320 + uniform(-0.5, 0.5));
    k2.pt.y = (float)(520 * Y[1] / Y[2] + 240 + uniform(-0.5, 0.5));
    k1.octave = rand() % 8;
    k2.octave = rand() % 8;
    vMatches12[i] = n - 1 - i;
    vbTriangulated[i] = i % 9 != 0;  // (some matches were not triangulated)
    vP3D[i].x = (float)(X[0] + uniform(-0.03, 0.03));
    vP3D[i].y = (float)(X[1] + uniform(-0.03, 0.03));
    vP3D[i].z = (float)(X[2] + uniform(-0.03, 0.03));
  }
  PoseT Tcw;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Tcw(r, c) = (float)R[r][c];
    Tcw(r, 3) = (float)(t[r] * 1.05 + 0.01);
  }

  // the C ABI on the same inputs
  orbx_init_result ir = {};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) ir.R21[r * 3 + c] = (float)Tcw(r, c);
    ir.t21[r] = (float)Tcw(r, 3);
  }
  std::vector<float> p3d(3 * vP3D.size());
  std::vector<uint8_t> tri(vP3D.size());
  for (size_t i = 0; i < vP3D.size(); i++) {
    p3d[3 * i] = vP3D[i].x; p3d[3 * i + 1] = vP3D[i].y; p3d[3 * i + 2] = vP3D[i].z;
    tri[i] = vbTriangulated[i];
  }
  orbx_ba_result res;
  std::vector<float> out(p3d.size());
  const int rc = orbx_bundle_adjust(extractor.context(), reinterpret_cast<const orbx_keypoint*>(F1.mvKeysUn.data()), (int)F1.mvKeysUn.size(),
                                    reinterpret_cast<const orbx_keypoint*>(F2.mvKeysUn.data()), (int)F2.mvKeysUn.size(), vMatches12.data(),
                                    &ir, p3d.data(), tri.data(), F1.mK, nullptr, 20, 100, 1, &res, out.data());
  if (rc != ORBX_OK) {
    std::printf("orbx_bundle_adjust: %d\n", rc);
    return 1;
  }

  const int status = Optimizer::BundleAdjustmentTwoView(F1, F2, vMatches12, Tcw, vP3D, vbTriangulated, 20);
  bool same = status == res.status;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) same = same && (float)Tcw(r, c) == res.R21[r * 3 + c];
    same = same && (float)Tcw(r, 3) == res.t21[r];
  }
  for (size_t i = 0; i < vP3D.size(); i++) {
    const float v[3] = {vP3D[i].x, vP3D[i].y, vP3D[i].z};
    same = same && std::memcmp(v, &out[3 * i], sizeof v) == 0;
  }
  std::printf("RESULT %d %d %d %d\n", status, res.iterations, res.n_points, (int)same);
  return same ? 0 : 2;
}
