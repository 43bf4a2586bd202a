// Tracking::TrackWithMotionModel's matching over include/orbx_shim.hpp, POD build: a Frame-like type that holds what the
// reference's Frame has (mvKeysUn, mDescriptors, N, mpORBextractor, mK, the static bounds) for a synthetic scene -- the current
// frame's features are the projections of the last frame's map points, their descriptors copies with a few bits flipped -- then
// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, vP3D, vbHasPoint, Tcw, vnMatchesCur) on the frames and on
// FrameViews of them.  The same inputs go through the C ABI (orbx_match_projection); all three must give the same matches.
// Usage: shim_match_proj <seed>; prints RESULT <matches> <matches that are the true feature> <points with a feature> <agree>.
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
  const int n = 200;
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  Frame last, cur;
  last.mpORBextractor = cur.mpORBextractor = &extractor;
  const double a = 0.03, R[3][3] = {{std::cos(a), 0, std::sin(a)}, {0, 1, 0}, {-std::sin(a), 0, std::cos(a)}}, t[3] = {0.1, -0.05, 0.1};
  PoseT Tcw;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Tcw(r, c) = (float)R[r][c];
    Tcw(r, 3) = (float)t[r];
  }
  last.mvKeysUn.resize(n);
  last.mDescriptors.resize(32 * n);
  std::vector<Point3T> vP3D(n);
  std::vector<bool> vbHasPoint(n), vbLastOutlier(n);
  std::vector<int> truth;  // per feature of the current frame: the last frame's feature it shows
  for (int i = 0; i < n; i++) {
    const double z = uniform(3, 15), u = uniform(-20, 660), v = uniform(-20, 500);
    const double Y[3] = {(u - 318.75) / 517.25 * z, (v - 255.5) / 388.5 * z, z};
    double X[3];  // R^T (Y - t)
    for (int c = 0; c < 3; c++) X[c] = R[0][c] * (Y[0] - t[0]) + R[1][c] * (Y[1] - t[1]) + R[2][c] * (Y[2] - t[2]);
    vP3D[i].x = (float)X[0];
    vP3D[i].y = (float)X[1];
    vP3D[i].z = (float)X[2];
    vbHasPoint[i] = i % 9 != 0;
    vbLastOutlier[i] = i % 31 == 5;
    KeyPointT& k = last.mvKeysUn[i];
    k.octave = rand() % 8;
    k.angle = (float)(rand() % 360);
    for (int b = 0; b < 32; b++) last.mDescriptors[32 * i + b] = (uint8_t)(rand() & 255);
    if (u < 2 || u > 630 || v < 2 || v > 470 || i % 5 == 0) continue;  // (not seen in the current frame)
    KeyPointT c = k;
    c.pt.x = (float)(u + uniform(-1, 1));
    c.pt.y = (float)(v + uniform(-1, 1));
    c.angle = k.angle >= 25.f ? k.angle - 25.f : k.angle + 335.f;
    cur.mvKeysUn.push_back(c);
    for (int b = 0; b < 32; b++) cur.mDescriptors.push_back(last.mDescriptors[32 * i + b]);
    for (int f = 0; f < 10; f++) cur.mDescriptors[cur.mDescriptors.size() - 32 + rand() % 32] ^= (uint8_t)(1 << (rand() % 8));
    truth.push_back(i);
  }
  last.N = n;
  cur.N = (int)cur.mvKeysUn.size();

  // the C ABI on the same inputs
  float pose[12];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) pose[r * 3 + c] = (float)Tcw(r, c);
    pose[9 + r] = (float)Tcw(r, 3);
  }
  std::vector<float> p3d(3 * n);
  std::vector<uint8_t> has(n), out(n);
  for (int i = 0; i < n; i++) {
    p3d[3 * i] = vP3D[i].x; p3d[3 * i + 1] = vP3D[i].y; p3d[3 * i + 2] = vP3D[i].z;
    has[i] = vbHasPoint[i];
    out[i] = vbLastOutlier[i];
  }
  const orbx_bounds b{Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY};
  std::vector<int32_t> viaC(cur.N > 0 ? cur.N : 1);
  orbx_proj_result res;
  const int rc = orbx_match_projection(extractor.context(), reinterpret_cast<const orbx_keypoint*>(last.mvKeysUn.data()),
                                       last.mDescriptors.data(), last.N, reinterpret_cast<const orbx_keypoint*>(cur.mvKeysUn.data()),
                                       cur.mDescriptors.data(), cur.N, p3d.data(), has.data(), nullptr, out.data(), pose, cur.mK, &b,
                                       15.f, 1, viaC.data(), &res);
  if (rc != ORBX_OK) {
    std::printf("orbx_match_projection: %d\n", rc);
    return 1;
  }

  ORBmatcher matcher(0.9f, true);
  std::vector<int> vnMatchesCur, viaViews;
  orbx_proj_result viaShim;
  const int nmatches = matcher.SearchByProjection(cur, last, 15.f, vP3D, vbHasPoint, Tcw, vnMatchesCur, &vbLastOutlier, &viaShim);
  ORBmatcher onViews(0.9f, true, &extractor);
  const int nviews = onViews.SearchByProjection(ORBmatcher::frameView(cur), ORBmatcher::frameView(last), 15.f, vP3D, vbHasPoint, Tcw,
                                                cur.mK, viaViews, &vbLastOutlier);
  bool same = nmatches == res.nmatches && nviews == nmatches && std::memcmp(&viaShim, &res, sizeof res) == 0 &&
              (int)vnMatchesCur.size() == cur.N && viaViews == vnMatchesCur;
  int right = 0;
  for (int j = 0; same && j < cur.N; j++) {
    same = same && vnMatchesCur[j] == viaC[j];
    right += vnMatchesCur[j] == truth[j];
  }
  std::printf("RESULT %d %d %d %d\n", nmatches, right, cur.N, (int)same);
  return same ? 0 : 2;
}
