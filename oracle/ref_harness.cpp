// ref_harness.cpp -- a C API over the reference's own compiled code (oracle/Makefile, target `ref`, into oracle/_ref/libref.so):
// DBoW2's text loader, transform and scoring objects (Thirdparty/DBoW2), Frame::PosInGrid / GetFeaturesInArea
// (SlamTypes/Frame.cpp) and ORBmatcher::SearchForInitialization (Features/ORBmatcher.cpp).  TEST INFRASTRUCTURE only
// (tests/ref_lib.py): this file only calls those sources, it restates none of them.  Every entry point catches every C++
// exception and returns an error code instead:
//   REF_OK 0, REF_E_EXCEPTION -1 (std::exception, e.g. an OpenCV stand-in that must not be reached), REF_E_THROWN -2 (anything
//   else, e.g. the std::string the vocabulary throws), REF_E_BADARG -3 (a bad argument to the harness itself),
//   REF_E_CAPACITY -4 (an output array too small).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <exception>
#include <sstream>
#include <string>
#include <vector>

#include "DBoW2/ScoringObject.h"
#include "Features/ORBVocabulary.hpp"
#include "Features/ORBextractor.hpp"
#include "Features/ORBmatcher.hpp"
#include "SlamTypes/Frame.hpp"

namespace ORB_SLAM_Tracking {
// the one out-of-line extractor member Frame.cpp calls (its Frame(im, ...) constructor); the harness never constructs a frame
// that way
int ORBextractor::operator()(cv::InputArray, cv::InputArray, std::vector<cv::KeyPoint>&, cv::OutputArray, std::vector<int>&) {
  cv::refStubUnreachable("ORBextractor::operator()");
}
}  // namespace ORB_SLAM_Tracking

namespace {

using ORB_SLAM_Tracking::Frame;
using ORB_SLAM_Tracking::ORBVocabulary;

enum { REF_OK = 0, REF_E_EXCEPTION = -1, REF_E_THROWN = -2, REF_E_BADARG = -3, REF_E_CAPACITY = -4 };

thread_local std::string gLastError;

template <typename Fn>
int guarded(Fn fn) {
  try {
    return fn();
  } catch (const std::exception& e) {
    gLastError = e.what();
    return REF_E_EXCEPTION;
  } catch (const std::string& s) {
    gLastError = s;
    return REF_E_THROWN;
  } catch (...) {
    gLastError = "unknown exception";
    return REF_E_THROWN;
  }
}

// the vocabulary with read access to its loaded tree (protected members of the reference class)
class Voc : public ORBVocabulary {
 public:
  int nodeCount() const { return (int)m_nodes.size() - 1; }  // without the root; -1 when the loader kept nothing
  int wordCount() const { return (int)m_words.size(); }
  const Node& node(int i) const { return m_nodes[i]; }
  int wordNode(int w) const { return (int)m_words[w]->id; }
};

// harness keypoint: the 28-byte layout of cv::KeyPoint's fields (include/orbx.h orbx_keypoint)
struct RefKeypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
};

cv::KeyPoint toKeyPoint(const RefKeypoint& k) {
  cv::KeyPoint o;
  o.pt.x = k.x;
  o.pt.y = k.y;
  o.size = k.size;
  o.angle = k.angle;
  o.response = k.response;
  o.octave = k.octave;
  o.class_id = k.class_id;
  return o;
}

// the rows of an [n, 32] byte array as the vector of 1 x 32 descriptors DBoW2's transform takes
std::vector<cv::Mat> descriptorRows(const uint8_t* desc32, int n) {
  cv::Mat all(n, 32, CV_8U);
  if (n > 0) std::memcpy(all.ptr<uint8_t>(), desc32, (size_t)n * 32);
  std::vector<cv::Mat> rows;
  rows.reserve(n);
  for (int i = 0; i < n; i++) rows.push_back(all.row(i));
  return rows;
}

// the frame-grid statics (Frame.hpp) for image bounds {min_x, max_x, min_y, max_y}: the values Frame's constructor gives them
void setGridStatics(const int32_t* bounds) {
  Frame::mnMinX = bounds[0];
  Frame::mnMaxX = bounds[1];
  Frame::mnMinY = bounds[2];
  Frame::mnMaxY = bounds[3];
  Frame::mfGridElementWidthInv = static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(bounds[1] - bounds[0]);
  Frame::mfGridElementHeightInv = static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(bounds[3] - bounds[2]);
  Frame::mbInitialComputations = false;
}

// a default-constructed Frame with its public members set as Frame's constructor sets them for undistorted keypoints: N,
// mvKeys = mvKeysUn, mDescriptors, and each keypoint in the grid cell PosInGrid gives it
void fillFrame(Frame* f, const RefKeypoint* kps, const uint8_t* desc32, int n) {
  f->N = n;
  f->mvKeys.resize(n);
  for (int i = 0; i < n; i++) f->mvKeys[i] = toKeyPoint(kps[i]);
  f->mvKeysUn = f->mvKeys;
  f->mDescriptors = cv::Mat(n, 32, CV_8U);
  if (n > 0 && desc32) std::memcpy(f->mDescriptors.ptr<uint8_t>(), desc32, (size_t)n * 32);
  for (int i = 0; i < n; i++) {
    int x, y;
    if (f->PosInGrid(f->mvKeysUn[i], x, y)) f->mGrid[x][y].push_back(i);
  }
}

}  // namespace

extern "C" {

const char* ref_last_error() { return gLastError.c_str(); }

// ---- vocabulary --------------------------------------------------------------------------------------------------------

// TemplatedVocabulary::loadFromTextFile(path) into a new vocabulary (*out; free it with ref_voc_free)
int ref_voc_load(const char* path, void** out) {
  if (!path || !out) return REF_E_BADARG;
  *out = nullptr;
  return guarded([&]() -> int {
    Voc* v = new Voc();
    try {
      v->loadFromTextFile(path);
    } catch (...) {
      delete v;
      throw;
    }
    *out = v;
    return REF_OK;
  });
}

void ref_voc_free(void* h) { delete static_cast<Voc*>(h); }

// info6 = {k, L, scoring, weighting, nodes without the root (-1: the loader kept no tree), words}
int ref_voc_info(const void* h, int32_t* info6) {
  if (!h || !info6) return REF_E_BADARG;
  return guarded([&]() -> int {
    const Voc* v = static_cast<const Voc*>(h);
    info6[0] = v->getBranchingFactor();
    info6[1] = v->getDepthLevels();
    info6[2] = (int32_t)v->getScoringType();
    info6[3] = (int32_t)v->getWeightingType();
    info6[4] = v->nodeCount();
    info6[5] = v->wordCount();
    return REF_OK;
  });
}

// the loaded tree, node i + 1 for i in [0, n): parent, number of children, descriptor bytes, weight; word_node [words]: the
// node id of each word id.  Returns n, 0 when the loader kept no tree (then nothing is written)
int ref_voc_nodes(const void* h, int32_t* parent, int32_t* n_children, uint8_t* desc32, double* weight, int32_t* word_node,
                  int32_t capacity) {
  if (!h) return REF_E_BADARG;
  return guarded([&]() -> int {
    const Voc* v = static_cast<const Voc*>(h);
    const int n = std::max(v->nodeCount(), 0), nw = v->wordCount();
    if (n > capacity || nw > capacity) return REF_E_CAPACITY;
    for (int i = 0; i < n; i++) {
      const auto& nd = v->node(i + 1);
      if (parent) parent[i] = (int32_t)nd.parent;
      if (n_children) n_children[i] = (int32_t)nd.children.size();
      if (desc32) {
        if (nd.descriptor.rows != 1 || nd.descriptor.cols != 32) return REF_E_BADARG;
        std::memcpy(desc32 + (size_t)i * 32, nd.descriptor.ptr<uint8_t>(), 32);
      }
      if (weight) weight[i] = nd.weight;
    }
    if (word_node)
      for (int w = 0; w < nw; w++) word_node[w] = v->wordNode(w);
    return n;
  });
}

// transform(features, BowVector&) (fv_* NULL) or transform(features, BowVector&, FeatureVector&, levelsup): the BowVector in
// its map order (ascending word id), the FeatureVector as (node, feature) pairs in map then vector order; feat_word [n]
// (nullable): transform(feature), each feature's word id.  Outputs hold up to `capacity` entries.
int ref_transform(const void* h, const uint8_t* desc32, int n, int levelsup, uint32_t* bow_word, double* bow_value, int32_t* bow_n,
                  uint32_t* fv_node, uint32_t* fv_feat, int32_t* fv_n, uint32_t* feat_word, int32_t capacity) {
  if (!h || n < 0 || (n > 0 && !desc32) || !bow_word || !bow_value || !bow_n) return REF_E_BADARG;
  if ((fv_node == nullptr) != (fv_feat == nullptr) || (fv_node == nullptr) != (fv_n == nullptr)) return REF_E_BADARG;
  return guarded([&]() -> int {
    const Voc* v = static_cast<const Voc*>(h);
    const std::vector<cv::Mat> feats = descriptorRows(desc32, n);
    DBoW2::BowVector bv;
    DBoW2::FeatureVector fv;
    if (fv_node)
      v->transform(feats, bv, fv, levelsup);
    else
      v->transform(feats, bv);
    if ((int)bv.size() > capacity) return REF_E_CAPACITY;
    int i = 0;
    for (const auto& e : bv) {
      bow_word[i] = e.first;
      bow_value[i] = e.second;
      i++;
    }
    *bow_n = i;
    if (fv_node) {
      int j = 0;
      for (const auto& e : fv)
        for (unsigned int f : e.second) {
          if (j >= capacity) return REF_E_CAPACITY;
          fv_node[j] = e.first;
          fv_feat[j] = f;
          j++;
        }
      *fv_n = j;
    }
    if (feat_word)
      for (int k = 0; k < n; k++) feat_word[k] = v->transform(feats[k]);
    return REF_OK;
  });
}

// ScoringObject `scoring` (0 L1, 1 L2, 2 chi-square, 3 KL, 4 Bhattacharyya, 5 dot product)::score(v1, v2) of two BowVectors
// given as word / value arrays
int ref_score(int scoring, const uint32_t* w1, const double* v1, int n1, const uint32_t* w2, const double* v2, int n2,
              double* out) {
  if (!out || n1 < 0 || n2 < 0 || (n1 && (!w1 || !v1)) || (n2 && (!w2 || !v2))) return REF_E_BADARG;
  return guarded([&]() -> int {
    DBoW2::BowVector a, b;
    for (int i = 0; i < n1; i++) a[w1[i]] = v1[i];
    for (int i = 0; i < n2; i++) b[w2[i]] = v2[i];
    switch (scoring) {
      case 0: *out = DBoW2::L1Scoring().score(a, b); break;
      case 1: *out = DBoW2::L2Scoring().score(a, b); break;
      case 2: *out = DBoW2::ChiSquareScoring().score(a, b); break;
      case 3: *out = DBoW2::KLScoring().score(a, b); break;
      case 4: *out = DBoW2::BhattacharyyaScoring().score(a, b); break;
      case 5: *out = DBoW2::DotProductScoring().score(a, b); break;
      default: return REF_E_BADARG;
    }
    return REF_OK;
  });
}

// ---- frame grid and matcher --------------------------------------------------------------------------------------------

// Frame::PosInGrid for each keypoint: pos [n][2] = (posX, posY), ok [n]
int ref_pos_in_grid(const RefKeypoint* kps, int n, const int32_t* bounds, int32_t* pos, int32_t* ok) {
  if (n < 0 || (n && (!kps || !pos || !ok)) || !bounds) return REF_E_BADARG;
  return guarded([&]() -> int {
    setGridStatics(bounds);
    Frame f;
    for (int i = 0; i < n; i++) {
      int x = 0, y = 0;
      ok[i] = f.PosInGrid(toKeyPoint(kps[i]), x, y) ? 1 : 0;
      pos[2 * i] = x;
      pos[2 * i + 1] = y;
    }
    return REF_OK;
  });
}

// Frame::GetFeaturesInArea(x, y, r, min_level, max_level) of a frame of n keypoints within bounds: returns the number of
// indices (written to out, in the reference's order, up to capacity)
int ref_features_in_area(const RefKeypoint* kps, int n, const int32_t* bounds, float x, float y, float r, int min_level,
                         int max_level, int32_t* out, int32_t capacity) {
  if (n < 0 || (n && !kps) || !bounds || !out) return REF_E_BADARG;
  return guarded([&]() -> int {
    setGridStatics(bounds);
    Frame f;
    fillFrame(&f, kps, nullptr, n);
    const std::vector<size_t> idx = f.GetFeaturesInArea(x, y, r, min_level, max_level);
    if ((int)idx.size() > capacity) return REF_E_CAPACITY;
    for (size_t i = 0; i < idx.size(); i++) out[i] = (int32_t)idx[i];
    return (int)idx.size();
  });
}

// ORBmatcher(nnratio, check_ori).SearchForInitialization(F1, F2, vnMatches12, window) with both frames in the same bounds:
// *nmatches, matches12 [n1], stats [3] = the three counters the call prints (invalid by distance, ratio, orientation)
int ref_match_init(const RefKeypoint* k1, const uint8_t* d1, int n1, const RefKeypoint* k2, const uint8_t* d2, int n2,
                   const int32_t* bounds, int window, float nnratio, int check_ori, int32_t* matches12, int32_t* nmatches,
                   int32_t* stats) {
  if (n1 < 0 || n2 < 0 || (n1 && (!k1 || !d1 || !matches12)) || (n2 && (!k2 || !d2)) || !bounds || !nmatches || !stats)
    return REF_E_BADARG;
  return guarded([&]() -> int {
    setGridStatics(bounds);
    Frame f1, f2;
    fillFrame(&f1, k1, d1, n1);
    fillFrame(&f2, k2, d2, n2);
    ORB_SLAM_Tracking::ORBmatcher matcher(nnratio, check_ori != 0);
    std::vector<int> m12;
    std::ostringstream printed;
    std::streambuf* saved = std::cout.rdbuf(printed.rdbuf());
    int nm;
    try {
      nm = matcher.SearchForInitialization(f1, f2, m12, window);
    } catch (...) {
      std::cout.rdbuf(saved);
      throw;
    }
    std::cout.rdbuf(saved);
    if ((int)m12.size() != n1) return REF_E_BADARG;
    for (int i = 0; i < n1; i++) matches12[i] = m12[i];
    *nmatches = nm;
    // "<label>: <count>" lines, in the order the call prints them
    std::istringstream lines(printed.str());
    std::string line;
    int k = 0;
    while (std::getline(lines, line) && k < 3) {
      const size_t colon = line.rfind(": ");
      if (line.rfind("invalidMatchBy", 0) == 0 && colon != std::string::npos) stats[k++] = std::stoi(line.substr(colon + 2));
    }
    return k == 3 ? REF_OK : REF_E_BADARG;
  });
}

}  // extern "C"
