// DBoW2's vocabulary-creation call sequence over include/orbx_shim.hpp, -DORBX_WITH_OPENCV build: documents of 1 x 32 cv::Mat
// descriptors, create(training_features, k, L, weighting, scoring) with DBoW2's signature, saveToTextFile, then a transform and
// the L1 score with what was trained.  Usage: shim_voc_train <out.txt>; prints "shim_voc_train ok <words>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  orbx::verbose() = false;
  uint64_t s = 88172645463325252ull;  // xorshift64: the documents' bytes
  std::vector<std::vector<cv::Mat> > training_features(6);
  for (size_t d = 0; d < training_features.size(); d++)
    for (int i = 0; i < 30 + 5 * (int)d; i++) {
      cv::Mat f(1, 32, CV_8U);
      for (int j = 0; j < 32; j++) {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        f.data[j] = (uchar)(s >> 24);
      }
      training_features[d].push_back(f);
    }
  try {
    ORBextractor extractor(1000, 1.2f, 8, 20, 7);
    ORBVocabulary voc(&extractor);
    voc.setSeed(7);
    voc.create(training_features, 4, 3, DBoW2::TF_IDF, DBoW2::L1_NORM);
    if (voc.empty()) return 3;
    voc.saveToTextFile(argv[1]);
    DBoW2::BowVector a, b;
    DBoW2::FeatureVector fa, fb;
    voc.transform(training_features[0], a, fa, 2);
    voc.transform(training_features[1], b, fb, 2);
    const double self = voc.score(a, a);  // L1 score of a normalised vector with itself: 1 up to rounding
    if (a.empty() || fa.empty() || self < 1.0 - 1e-12 || self > 1.0 + 1e-12) {
      fprintf(stderr, "unexpected: %zu words, %zu feature-vector nodes, self score %.17g\n", a.size(), fa.size(), self);
      return 4;
    }
    printf("shim_voc_train ok %u %.6f\n", voc.size(), voc.score(a, b));
  } catch (const orbx::Error& e) {
    fprintf(stderr, "orbx error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
