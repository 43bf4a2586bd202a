// Frame::ComputeBoW's call sequence over include/orbx_shim.hpp, POD build: an ORBextractor (the device context), an ORBVocabulary
// loaded from a text file, transform(mDescriptors, mBowVec, mFeatVec, 4) and the L1 score of the frame with itself.
// Usage: shim_bow <vocabulary.txt> <descriptors.bin (N x 32 bytes)>; prints RESULT <words> <feature-vector nodes> <score>.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[2], std::ios::binary);
  std::vector<uint8_t> desc((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  orbx::verbose() = false;
  try {
    ORBextractor extractor(1000, 1.2f, 8, 20, 7);
    ORBVocabulary voc(&extractor);
    voc.loadFromTextFile(argv[1]);
    DBoW2::BowVector mBowVec;
    DBoW2::FeatureVector mFeatVec;
    voc.transform(desc, mBowVec, mFeatVec, 4);
    const double s = voc.score(mBowVec, mBowVec);
    printf("RESULT %zu %zu %.17g\n", mBowVec.size(), mFeatVec.size(), s);
  } catch (const orbx::Error& e) {
    fprintf(stderr, "orbx error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
