// The stereo Frame constructor over include/orbx_shim.hpp, POD build: two raw 8-bit images in, mvuRight and mvDepth out.
// Usage: shim_stereo <left.raw> <right.raw> <width> <height> <nfeatures> <bf> <b> <out.raw>; writes N floats of mvuRight, then N of
// mvDepth, and prints RESULT <N> <matches> <before the median> <unprojected>.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

static bool readAll(const char* path, std::vector<uint8_t>& buf) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(buf.data(), 1, buf.size(), f);
  fclose(f);
  return got == buf.size();
}

int main(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: shim_stereo left.raw right.raw width height nfeatures bf b out.raw\n");
    return 2;
  }
  const int w = atoi(argv[3]), h = atoi(argv[4]), nfeatures = atoi(argv[5]);
  const float bf = (float)atof(argv[6]), b = (float)atof(argv[7]);
  if (w < 1 || h < 1 || nfeatures < 1) return 2;
  std::vector<uint8_t> left((size_t)w * h), right((size_t)w * h);
  if (!readAll(argv[1], left) || !readAll(argv[2], right)) {
    fprintf(stderr, "shim_stereo: cannot read the images\n");
    return 2;
  }
  try {
    ORBextractor extractor(nfeatures, 1.2f, 8, 20, 7, w, h);
    StereoFrame frame(left.data(), right.data(), w, h, w, &extractor, bf, b);
    const float K[9] = {260.f, 0.f, w / 2.f, 0.f, 260.f, h / 2.f, 0.f, 0.f, 1.f};
    int unprojected = 0;
    for (int i = 0; i < frame.N; i++) {
      float x3D[3];
      if (frame.UnprojectStereo(i, K, nullptr, x3D)) unprojected += x3D[2] == frame.mvDepth[(size_t)i];
    }
    FILE* f = fopen(argv[8], "wb");
    if (!f) return 2;
    fwrite(frame.mvuRight.data(), sizeof(float), frame.mvuRight.size(), f);
    fwrite(frame.mvDepth.data(), sizeof(float), frame.mvDepth.size(), f);
    fclose(f);
    printf("RESULT %d %d %d %d\n", frame.N, frame.result.n_matches, frame.result.n_before_median, unprojected);
    return unprojected == frame.result.n_matches ? 0 : 1;
  } catch (const orbx::Error& e) {
    fprintf(stderr, "shim_stereo: %s\n", e.what());
    return 3;
  }
}
