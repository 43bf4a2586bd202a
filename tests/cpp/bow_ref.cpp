// bow_ref.cpp — CPU restatement of DBoW2's TemplatedVocabulary<FORB> text loader, transform (BowVector, FeatureVector) and
// L1Scoring::score, written from the semantics in include/orbx.h ("bag of words") with std::map vectors as DBoW2 keeps them.
// Node ids, word ids and the descent follow the loader; the documented deviations are applied (blank lines skipped, a shallow
// leaf's own node id).  Compiled by tests/bow_ref_lib.py with g++ -O2 -ffp-contract=off.  TEST INFRASTRUCTURE only.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace {

struct Node {
  std::vector<unsigned> children;
  unsigned wordId = 0;
  double weight = 0.0;
  uint8_t desc[32] = {};
};

struct Voc {
  int k = 0, L = 0, scoring = 0, weighting = 0;
  std::vector<Node> nodes;  // [0] root
  int nWords = 0;
};

int distance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

// one feature's descent (TemplatedVocabulary.h:1230-1270)
void descend(const Voc& v, const uint8_t* f, unsigned* word, double* weight, unsigned* nid, int levelsup) {
  const int nidLevel = v.L - levelsup;
  bool nidSet = false;
  if (nidLevel <= 0) {
    *nid = 0;
    nidSet = true;
  }
  unsigned cur = 0;
  int level = 0;
  while (!v.nodes[cur].children.empty()) {
    ++level;
    const std::vector<unsigned>& ch = v.nodes[cur].children;
    unsigned best = ch[0];
    int bestD = distance(f, v.nodes[best].desc);
    for (size_t i = 1; i < ch.size(); i++) {
      const int d = distance(f, v.nodes[ch[i]].desc);
      if (d < bestD) {
        bestD = d;
        best = ch[i];
      }
    }
    if (level == nidLevel) {
      *nid = best;
      nidSet = true;
    }
    cur = best;
  }
  if (!nidSet) *nid = cur;  // deviation 2
  *word = v.nodes[cur].wordId;
  *weight = v.nodes[cur].weight;
}

}  // namespace

extern "C" {

void* br_voc_create(int k, int L, int scoring, int weighting, int n, const int32_t* parent, const int32_t* leaf, const uint8_t* desc,
                    const double* weight) {
  Voc* v = new Voc();
  v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting;
  v->nodes.resize(n + 1);
  for (int i = 0; i < n; i++) {
    Node& nd = v->nodes[i + 1];
    v->nodes[parent[i]].children.push_back(i + 1);
    memcpy(nd.desc, desc + (size_t)i * 32, 32);
    nd.weight = weight[i];
    if (leaf[i] > 0) nd.wordId = v->nWords++;
  }
  return v;
}

void br_voc_free(void* h) { delete (Voc*)h; }

// transform(features, BowVector&, FeatureVector&, levelsup) (:1139-1205; :1078-1133 is the same BowVector).  Outputs: the
// BowVector's (word, value) in map order, the FeatureVector flattened to (node, feature) pairs in map order, each feature's word.
void br_transform(void* h, const uint8_t* feats, int n, int levelsup, uint32_t* bowWord, double* bowValue, int32_t* bowN,
                  uint32_t* fvNode, uint32_t* fvFeat, int32_t* fvN, uint32_t* featWord) {
  const Voc& v = *(const Voc*)h;
  std::map<unsigned, double> bow;
  std::map<unsigned, std::vector<unsigned>> fv;
  std::vector<unsigned> nids(n);
  std::vector<double> wts(n);
  for (int i = 0; i < n; i++) descend(v, feats + (size_t)i * 32, &featWord[i], &wts[i], &nids[i], levelsup);
  if (v.nWords > 0) {
    const bool must = v.scoring != 5;                // mustNormalize: every scoring but DOT_PRODUCT
    const bool l2 = v.scoring == 1;                  // L2_NORM normalises with L2, the others with L1
    const bool tf = v.weighting == 0 || v.weighting == 1;
    for (int i = 0; i < n; i++) {
      const unsigned w = featWord[i], nid = nids[i];
      const double wt = wts[i];
      if (!(wt > 0)) continue;  // stopped
      auto it = bow.lower_bound(w);
      if (it != bow.end() && it->first == w) {
        if (tf) it->second += wt;  // addWeight; IDF / BINARY: addIfNotExist
      } else {
        bow.insert(it, std::make_pair(w, wt));
      }
      fv[nid].push_back((unsigned)i);
    }
    if (tf && !bow.empty() && !must) {
      const double nd = (double)bow.size();
      for (auto& e : bow) e.second /= nd;
    }
    if (must) {  // BowVector::normalize
      double norm = 0.0;
      if (!l2) {
        for (auto& e : bow) norm += std::fabs(e.second);
      } else {
        for (auto& e : bow) norm += e.second * e.second;
        norm = std::sqrt(norm);
      }
      if (norm > 0.0)
        for (auto& e : bow) e.second /= norm;
    }
  }
  int j = 0;
  for (auto& e : bow) {
    bowWord[j] = e.first;
    bowValue[j] = e.second;
    j++;
  }
  *bowN = j;
  j = 0;
  for (auto& e : fv)
    for (unsigned f : e.second) {
      fvNode[j] = e.first;
      fvFeat[j] = f;
      j++;
    }
  *fvN = j;
}

// L1Scoring::score (src/ScoringObject.cpp:23-66), over maps built from the two sorted lists
double br_score_l1(int n1, const uint32_t* w1, const double* v1, int n2, const uint32_t* w2, const double* v2) {
  std::map<unsigned, double> a, b;
  for (int i = 0; i < n1; i++) a[w1[i]] = v1[i];
  for (int i = 0; i < n2; i++) b[w2[i]] = v2[i];
  auto ai = a.begin(), bi = b.begin();
  double score = 0;
  while (ai != a.end() && bi != b.end()) {
    const double vi = ai->second, wi = bi->second;
    if (ai->first == bi->first) {
      score += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
      ++ai;
      ++bi;
    } else if (ai->first < bi->first) {
      ai = a.lower_bound(bi->first);
    } else {
      bi = b.lower_bound(ai->first);
    }
  }
  return -score / 2.0;
}

// the text loader (:1542-1620) with deviation 1 (blank lines skipped); returns the node count, -1 for a header outside the
// reference's ranges.  Arrays nullable (count only).
int br_parse_text(const char* path, int32_t* header, int32_t* parent, int32_t* leaf, uint8_t* desc, double* weight) {
  std::ifstream f(path);
  std::string s;
  std::getline(f, s);
  std::stringstream ss(s);
  int k = -1, L = -1, n1 = -1, n2 = -1;
  ss >> k >> L >> n1 >> n2;
  if (k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3) return -1;
  if (header) {
    header[0] = k; header[1] = L; header[2] = n1; header[3] = n2;
  }
  int n = 0;
  while (std::getline(f, s)) {
    if (s.find_first_not_of(" \t\r\n\v\f") == std::string::npos) continue;
    std::stringstream sn(s);
    int pid, isLeaf;
    sn >> pid >> isLeaf;
    uint8_t d[32];
    for (int i = 0; i < 32; i++) {
      int e;
      sn >> e;
      d[i] = (unsigned char)e;
    }
    double w;
    sn >> w;
    if (parent) {
      parent[n] = pid;
      leaf[n] = isLeaf;
      memcpy(desc + (size_t)n * 32, d, 32);
      weight[n] = w;
    }
    n++;
  }
  return n;
}

}  // extern "C"
