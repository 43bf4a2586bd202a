// The reference's Tracking::Initialize call sequence (tracking.cpp:96-115) over include/orbx_shim.hpp, POD build: a Frame-like
// type with the members the reference's Frame has (mvKeysUn, mDescriptors, N, mpORBextractor, mK, the static bounds),
// ORBmatcher::SearchForInitialization, then Initializer(mInitialFrame, 1.0, 200).Initialize(mCurrentFrame, mvIniMatches, Tcw,
// mvIniP3D, vbTriangulated).  Usage: shim_initializer <seed>; prints RESULT <nmatches> <initialized> <n triangulated>.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

struct Frame {
  std::vector<KeyPointT> mvKeysUn;
  std::vector<uint8_t> mDescriptors;
  int N = 0;
  ORBextractor* mpORBextractor = nullptr;
  float mK[9] = {520.f, 0.f, 320.f, 0.f, 520.f, 240.f, 0.f, 0.f, 1.f};
  static int mnMinX, mnMaxX, mnMinY, mnMaxY;
  Frame(const std::vector<uint8_t>& im, int w, int h, ORBextractor* e) : mpORBextractor(e) {
    std::vector<int> lap{0, 0};
    orbx::Image8 img{im.data(), w, h, w};
    (*e)(img, orbx::Image8{}, mvKeysUn, mDescriptors, lap);
    N = (int)mvKeysUn.size();
  }
};
int Frame::mnMinX = 0, Frame::mnMaxX = 640, Frame::mnMinY = 0, Frame::mnMaxY = 480;

int main(int argc, char** argv) {
  const int w = 640, h = 480;
  srand(argc > 1 ? atoi(argv[1]) : 0);
  // two views of a textured plane: random blobs, shifted by a few pixels
  std::vector<uint8_t> a(w * h, 128), b(w * h, 128);
  for (int k = 0; k < 3000; k++) {
    const int x = rand() % (w - 20) + 10, y = rand() % (h - 20) + 10, v = rand() % 256, r = 1 + rand() % 4;
    for (int dy = -r; dy <= r; dy++)
      for (int dx = -r; dx <= r; dx++) {
        a[(y + dy) * w + x + dx] = (uint8_t)v;
        const int x2 = x + dx + 6 + (x * 5) / w, y2 = y + dy + 3;
        if (x2 >= 0 && x2 < w && y2 >= 0 && y2 < h) b[y2 * w + x2] = (uint8_t)v;
      }
  }
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  Frame mInitialFrame(a, w, h, &extractor), mCurrentFrame(b, w, h, &extractor);
  Initializer* mpInitializer = new Initializer(mInitialFrame, 1.0, 200);  // tracking.cpp:84
  std::vector<int> mvIniMatches;
  ORBmatcher matcher(0.9, true);  // tracking.cpp:101-102
  int nmatches = matcher.SearchForInitialization(mInitialFrame, mCurrentFrame, mvIniMatches, 100);
  PoseT Tcw;
  std::vector<Point3T> mvIniP3D;
  std::vector<bool> vbTriangulated;
  bool isTriangulated = mpInitializer->Initialize(mCurrentFrame, mvIniMatches, Tcw, mvIniP3D, vbTriangulated);  // :113-115
  int nt = 0;
  for (bool t : vbTriangulated) nt += t;
  std::printf("RESULT %d %d %d\n", nmatches, (int)isTriangulated, nt);
  delete mpInitializer;
  return 0;
}
