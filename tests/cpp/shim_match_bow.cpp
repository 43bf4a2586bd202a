// A relocaliser's call sequence over include/orbx_shim.hpp, -DORBX_WITH_OPENCV build: two Frame-like objects with the
// reference's members (mvKeysUn, mDescriptors, N, mpORBextractor, mBowVec, mFeatVec), ComputeBoW's transform at the given
// levelsup for both, then ORBmatcher::SearchByBoW(KF, F, vnMatchesF, &kfHasPoint) -- on the frames and on their FrameViews.
// Usage: shim_match_bow <vocabulary.txt> <kf desc.bin> <kf angles.bin (f32)> <kf mask.bin (bytes)> <f desc.bin> <f angles.bin>
//        <levelsup>; prints RESULT <nmatches> and one line with F.N entries of vnMatchesF.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

struct Frame {
  std::vector<cv::KeyPoint> mvKeysUn;
  cv::Mat mDescriptors;
  int N = 0;
  ORBextractor* mpORBextractor = nullptr;
  DBoW2::BowVector mBowVec;
  DBoW2::FeatureVector mFeatVec;
  static int mnMinX, mnMaxX, mnMinY, mnMaxY;
};
int Frame::mnMinX = 0, Frame::mnMaxX = 640, Frame::mnMinY = 0, Frame::mnMaxY = 480;

static std::vector<char> bytesOf(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void load(Frame& F, const char* descPath, const char* anglePath, ORBextractor* e, const ORBVocabulary& voc, int levelsup) {
  const std::vector<char> d = bytesOf(descPath), a = bytesOf(anglePath);
  F.N = (int)(d.size() / 32);
  F.mDescriptors.create(F.N > 0 ? F.N : 1, 32, CV_8U);
  if (F.N) memcpy(F.mDescriptors.data, d.data(), (size_t)F.N * 32);
  F.mvKeysUn.resize(F.N);
  for (int i = 0; i < F.N; i++) memcpy(&F.mvKeysUn[i].angle, a.data() + (size_t)i * 4, 4);
  F.mpORBextractor = e;
  voc.transform(F.mDescriptors.data, F.N, F.mBowVec, F.mFeatVec, levelsup);
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  orbx::verbose() = false;
  try {
    ORBextractor extractor(1000, 1.2f, 8, 20, 7);
    ORBVocabulary voc(&extractor);
    voc.loadFromTextFile(argv[1]);
    const int levelsup = atoi(argv[7]);
    Frame KF, F;
    load(KF, argv[2], argv[3], &extractor, voc, levelsup);
    load(F, argv[5], argv[6], &extractor, voc, levelsup);
    const std::vector<char> m = bytesOf(argv[4]);
    if ((int)m.size() != KF.N) return 3;
    std::vector<bool> kfHasPoint(KF.N);
    for (int i = 0; i < KF.N; i++) kfHasPoint[i] = m[i] != 0;
    ORBmatcher matcher(0.6f, true);
    std::vector<int> vnMatchesF, viaViews;
    const int nmatches = matcher.SearchByBoW(KF, F, vnMatchesF, &kfHasPoint);
    ORBmatcher pinned(0.6f, true, &extractor);
    const int n2 = pinned.SearchByBoW(ORBmatcher::frameView(KF), ORBmatcher::frameView(F), viaViews, &kfHasPoint);
    if (n2 != nmatches || viaViews != vnMatchesF || (int)vnMatchesF.size() != F.N) return 4;
    bool threw = false;  // a view without mFeatVec is refused
    try {
      FrameView bare = ORBmatcher::frameView(F);
      bare.mFeatVec = nullptr;
      pinned.SearchByBoW(ORBmatcher::frameView(KF), bare, viaViews);
    } catch (const orbx::Error& e) {
      threw = e.code == ORBX_E_BADARG;
    }
    if (!threw) return 5;
    printf("RESULT %d\n", nmatches);
    for (int v : vnMatchesF) printf("%d ", v);
    printf("\n");
  } catch (const orbx::Error& e) {
    fprintf(stderr, "orbx error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
