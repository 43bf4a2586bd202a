// Tracking::TrackReferenceKeyFrame's optimisation over include/orbx_shim.hpp, POD build: a Frame-like object that holds what the
// reference's Frame has (mvKeysUn, mpORBextractor, mK) for a synthetic scene, map points as coordinates with a has-point flag
// per feature, a start pose that is off, then Optimizer::PoseOptimization(F, vP3D, vbHasPoint, Tcw, vbOutlier).  The same inputs
// go through the C ABI (orbx_pose_optimize); both must give the same bytes.
// Usage: shim_pose <seed>; prints RESULT <status> <inliers> <correspondences> <flagged planted mismatches> <agrees with the C ABI>.
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
  srand(argc > 1 ? atoi(argv[1]) : 0);
  const int n = 150, planted = 12;
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  Frame F;
  F.mpORBextractor = &extractor;
  // the true pose: a small rotation about y, a step
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
  PoseT Tcw;  // 2 degrees about z and 5 % off
  const double b = 0.035, Z[3][3] = {{std::cos(b), -std::sin(b), 0}, {std::sin(b), std::cos(b), 0}, {0, 0, 1}};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Tcw(r, c) = (float)(Z[r][0] * R[0][c] + Z[r][1] * R[1][c] + Z[r][2] * R[2][c]);
    Tcw(r, 3) = (float)((Z[r][0] * t[0] + Z[r][1] * t[1] + Z[r][2] * t[2]) * 1.05);
  }

  // the C ABI on the same inputs
  float pose0[12];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) pose0[r * 3 + c] = (float)Tcw(r, c);
    pose0[9 + r] = (float)Tcw(r, 3);
  }
  std::vector<float> p3d(3 * vP3D.size());
  std::vector<uint8_t> has(vP3D.size()), out(vP3D.size());
  for (size_t i = 0; i < vP3D.size(); i++) {
    p3d[3 * i] = vP3D[i].x; p3d[3 * i + 1] = vP3D[i].y; p3d[3 * i + 2] = vP3D[i].z;
    has[i] = vbHasPoint[i];
  }
  orbx_pose_result res;
  const int rc = orbx_pose_optimize(extractor.context(), reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data()), (int)F.mvKeysUn.size(),
                                    p3d.data(), has.data(), pose0, F.mK, nullptr, 10, &res, out.data());
  if (rc != ORBX_OK) {
    std::printf("orbx_pose_optimize: %d\n", rc);
    return 1;
  }

  std::vector<bool> vbOutlier;
  orbx_pose_result viaShim;
  const int inliers = Optimizer::PoseOptimization(F, vP3D, vbHasPoint, Tcw, vbOutlier, 10, &viaShim);
  bool same = inliers == res.n_inliers && std::memcmp(&viaShim, &res, sizeof res) == 0 && vbOutlier.size() == out.size();
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) same = same && (float)Tcw(r, c) == res.R[r * 3 + c];
    same = same && (float)Tcw(r, 3) == res.tcw[r];
  }
  int flagged = 0;
  for (size_t i = 0; same && i < out.size(); i++) {
    same = same && vbOutlier[i] == (out[i] != 0);
    flagged += (int)i < planted && out[i];
  }
  std::printf("RESULT %d %d %d %d %d\n", res.status, inliers, res.n_correspondences, flagged, (int)same);
  return same ? 0 : 2;
}
