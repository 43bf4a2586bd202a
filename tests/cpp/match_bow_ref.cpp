// match_bow_ref.cpp — CPU restatement of ORBmatcher::SearchByBoW as include/orbx.h states it ("matching through the
// FeatureVector"): plain loops over std::map<node, std::vector<feature>>, nothing shared with the library.  TEST INFRASTRUCTURE
// only; compiled on first use by tests/match_bow_ref_lib.py with g++ -O2 -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

namespace {

const int TH_LOW = 50;
const int HISTO_LENGTH = 30;

typedef std::map<uint32_t, std::vector<uint32_t>> FeatureVector;

// the device form's rule for a malformed vector: a pair that names no feature of the frame is skipped
FeatureVector featureVector(const uint32_t* node, const uint32_t* feat, int fvN, int n) {
  FeatureVector fv;
  for (int i = 0; i < fvN; i++)
    if (feat[i] < (uint32_t)n) fv[node[i]].push_back(feat[i]);
  return fv;
}

int distance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

// Features/ORBmatcher.cpp:152-183
void computeThreeMaxima(const std::vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  for (int i = 0; i < L; i++) {
    const int s = (int)histo[i].size();
    if (s > max1) {
      max3 = max2; max2 = max1; max1 = s;
      ind3 = ind2; ind2 = ind1; ind1 = i;
    } else if (s > max2) {
      max3 = max2; max2 = s;
      ind3 = ind2; ind2 = i;
    } else if (s > max3) {
      max3 = s;
      ind3 = i;
    }
  }
  if (max2 < 0.1f * static_cast<float>(max1)) {
    ind2 = -1;
    ind3 = -1;
  } else if (max3 < 0.1f * static_cast<float>(max1)) {
    ind3 = -1;
  }
}

struct Best {
  int best1, best2, idx;
  bool accepted;
};

// steps 2.1-2.4 and the test of step 3 for one keyframe feature over the node's frame features; with `matches` the features
// already taken are skipped
Best search(const uint8_t* d, const std::vector<uint32_t>& feats, const uint8_t* descF, const int32_t* matches, float nnratio) {
  Best b = {256, 256, -1, false};
  for (uint32_t j : feats) {
    if (matches && matches[j] >= 0) continue;
    const int dist = distance(d, descF + (size_t)j * 32);
    if (dist < b.best1) {
      b.best2 = b.best1;
      b.best1 = dist;
      b.idx = (int)j;
    } else if (dist < b.best2) {
      b.best2 = dist;
    }
  }
  b.accepted = b.best1 <= TH_LOW && static_cast<float>(b.best1) < nnratio * static_cast<float>(b.best2);
  return b;
}

}  // namespace

// angles: the keypoints' angle fields.  counters[4]: rejected by distance, rejected by ratio, keyframe features whose result
// (accepted or not, and the frame feature) differs because a frame feature was already taken, removed by orientation.
// Returns nmatches; matchesF holds nF entries.
extern "C" int mbr_search_by_bow(const float* angK, const uint8_t* descK, int nK, const uint32_t* nodeK, const uint32_t* featK,
                                 int fvnK, const float* angF, const uint8_t* descF, int nF, const uint32_t* nodeF,
                                 const uint32_t* featF, int fvnF, const uint8_t* maskK, float nnratio, int checkOrientation,
                                 int32_t* matchesF, int64_t* counters) {
  const FeatureVector fvK = featureVector(nodeK, featK, fvnK, nK), fvF = featureVector(nodeF, featF, fvnF, nF);
  for (int j = 0; j < nF; j++) matchesF[j] = -1;
  for (int c = 0; c < 4; c++) counters[c] = 0;
  std::vector<int> rotHist[HISTO_LENGTH];
  const float factor = HISTO_LENGTH / 360.0f;
  int nmatches = 0;
  for (const auto& kv : fvK) {
    const auto it = fvF.find(kv.first);
    if (it == fvF.end()) continue;
    for (uint32_t i : kv.second) {
      if (maskK && maskK[i] == 0) continue;
      const uint8_t* d = descK + (size_t)i * 32;
      const Best b = search(d, it->second, descF, matchesF, nnratio);
      const Best all = search(d, it->second, descF, nullptr, nnratio);
      if (b.accepted != all.accepted || (b.accepted && b.idx != all.idx)) counters[2]++;
      if (b.best1 > TH_LOW) {
        counters[0]++;
        continue;
      }
      if (!b.accepted) {
        counters[1]++;
        continue;
      }
      matchesF[b.idx] = (int32_t)i;
      nmatches++;
      if (checkOrientation) {
        float rot = angK[i] - angF[b.idx];
        if (rot < 0.0f) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == HISTO_LENGTH) bin = 0;
        if (bin >= 0 && bin < HISTO_LENGTH) rotHist[bin].push_back(b.idx);
      }
    }
  }
  if (checkOrientation) {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    computeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
    for (int i = 0; i < HISTO_LENGTH; i++) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (int j : rotHist[i]) {
        matchesF[j] = -1;
        nmatches--;
        counters[3]++;
      }
    }
  }
  return nmatches;
}
