// voc_train_ref.cpp — CPU restatement of DBoW2's TemplatedVocabulary<FORB>::create (Thirdparty/DBoW2/include/DBoW2/
// TemplatedVocabulary.h:569-1008, src/FORB.cpp:24-73), recursive and depth-first as the reference writes it (std::vector groups,
// meanValue, nodes pushed back in create's order), with the three deviations of include/orbx.h ("training"): the draws are a
// function of (seed, node path, draw index), an emptied cluster keeps its centre, and a run stops after max_rounds rounds.
// TEST INFRASTRUCTURE only (tests/voc_train_ref_lib.py compiles it on first use).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Desc {
  uint8_t b[32];
};
struct Node {
  int parent = 0;
  std::vector<int> children;
  Desc d{};
  double weight = 0;
  int word = -1;
};
struct State {
  int k = 0, L = 0, weighting = 0, maxRounds = 0;
  uint64_t seed = 0;
  const Desc* feat = nullptr;
  std::vector<Node> nodes;
  std::vector<int> featNode;
  std::vector<uint32_t> featWord;
  int32_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
} S;

uint64_t mix(uint64_t z) {  // the splitmix64 step
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint32_t draw(uint64_t key, uint64_t j) { return (uint32_t)(mix(mix(S.seed ^ mix(key)) + j) >> 33); }

int distance(const Desc& a, const Desc& b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a.b[i] ^ b.b[i]));
  return d;
}

// FORB::meanValue; an empty group leaves the centre as it is (deviation 2)
bool meanValue(const std::vector<const Desc*>& ds, Desc* mean) {
  if (ds.empty()) return false;
  if (ds.size() == 1) {
    *mean = *ds[0];
    return true;
  }
  std::vector<int> sum(256, 0);
  for (const Desc* d : ds)
    for (int j = 0; j < 32; j++)
      for (int bit = 0; bit < 8; bit++)
        if (d->b[j] & (1 << (7 - bit))) ++sum[j * 8 + bit];
  const int N2 = (int)ds.size() / 2 + (int)ds.size() % 2;
  memset(mean->b, 0, 32);
  for (int i = 0; i < 256; i++)
    if (sum[i] >= N2) mean->b[i / 8] |= (uint8_t)(1 << (7 - (i % 8)));
  return true;
}

// initiateClustersKMpp (:846-925) with the draws of deviation 1
void seedKMpp(const std::vector<int>& f, uint64_t key, std::vector<Desc>* clusters) {
  const int n = (int)f.size();
  uint64_t j = 0;
  std::vector<double> minD(n);
  int ifeature = (int)((double)draw(key, j++) / 2147483648.0 * n);
  clusters->push_back(S.feat[f[ifeature]]);
  for (int i = 0; i < n; i++) minD[i] = distance(S.feat[f[i]], clusters->back());
  while ((int)clusters->size() < S.k) {
    for (int i = 0; i < n; i++)
      if (minD[i] > 0) {
        const double d = distance(S.feat[f[i]], clusters->back());
        if (d < minD[i]) minD[i] = d;
      }
    double sum = 0;
    for (int i = 0; i < n; i++) sum += minD[i];
    if (!(sum > 0)) {
      S.stats[6]++;
      break;
    }
    double cut;
    do cut = (double)draw(key, j++) / 2147483647.0 * sum;
    while (cut == 0.0);
    double up = 0;
    int i = 0;
    for (; i < n; i++) {
      up += minD[i];
      if (up >= cut) break;
    }
    ifeature = i == n ? n - 1 : i;
    clusters->push_back(S.feat[f[ifeature]]);
  }
}

void step(int parentId, const std::vector<int>& f, int level, uint64_t key) {
  if (f.empty()) return;
  std::vector<Desc> clusters;
  std::vector<std::vector<int>> groups;
  const int n = (int)f.size();
  if (n <= S.k) {
    S.stats[7]++;
    groups.resize(n);
    for (int i = 0; i < n; i++) {
      groups[i].push_back(i);
      clusters.push_back(S.feat[f[i]]);
    }
  } else {
    S.stats[2]++;
    std::vector<int> last, cur(n);
    int rounds = 0;
    for (;;) {
      if (rounds == 0) {
        seedKMpp(f, key, &clusters);
      } else {
        for (size_t c = 0; c < clusters.size(); c++) {
          std::vector<const Desc*> cd;
          for (int i : groups[c]) cd.push_back(&S.feat[f[i]]);
          if (!meanValue(cd, &clusters[c])) S.stats[5]++;
        }
      }
      groups.assign(clusters.size(), std::vector<int>());
      for (int i = 0; i < n; i++) {
        int best = distance(S.feat[f[i]], clusters[0]), ic = 0;
        for (size_t c = 1; c < clusters.size(); c++) {
          const int d = distance(S.feat[f[i]], clusters[c]);
          if (d < best) {
            best = d;
            ic = (int)c;
          }
        }
        groups[ic].push_back(i);
        cur[i] = ic;
      }
      ++rounds;
      if (rounds > 1 && cur == last) break;
      if (rounds >= S.maxRounds) {  // deviation 3
        S.stats[4]++;
        break;
      }
      last = cur;
    }
    if (rounds > S.stats[3]) S.stats[3] = rounds;
  }
  std::vector<int> ids;
  for (size_t i = 0; i < clusters.size(); i++) {
    const int id = (int)S.nodes.size();
    S.nodes.emplace_back();
    S.nodes.back().d = clusters[i];
    S.nodes.back().parent = parentId;
    S.nodes[parentId].children.push_back(id);
    ids.push_back(id);
  }
  for (size_t i = 0; i < clusters.size(); i++) {
    std::vector<int> child;
    for (int g : groups[i]) child.push_back(f[g]);
    if (level < S.L && child.size() > 1)
      step(ids[i], child, level + 1, 21 * key + i + 1);
    else
      for (int g : child) S.featNode[g] = ids[i];
  }
}

int descend(const Desc& q) {  // transform(feature, word_id) (:1230-1270)
  int cur = 0;
  while (!S.nodes[cur].children.empty()) {
    const std::vector<int>& ch = S.nodes[cur].children;
    int best = ch[0], bd = distance(q, S.nodes[ch[0]].d);
    for (size_t c = 1; c < ch.size(); c++) {
      const int d = distance(q, S.nodes[ch[c]].d);
      if (d < bd) {
        bd = d;
        best = ch[c];
      }
    }
    cur = best;
  }
  return cur;
}

}  // namespace

extern "C" {

// Trains on documents concatenated in desc32 (doc_n[n_docs] features each); the result stays in the library until the next call.
// Returns the node count without the root.
int vt_train(int k, int L, int weighting, uint64_t seed, int max_rounds, int n_docs, const uint8_t* desc32, const int32_t* doc_n) {
  S = State();
  S.k = k;
  S.L = L;
  S.weighting = weighting;
  S.seed = seed;
  S.maxRounds = max_rounds;
  S.feat = reinterpret_cast<const Desc*>(desc32);
  int N = 0;
  for (int d = 0; d < n_docs; d++) N += doc_n[d];
  S.featNode.assign(N, 0);
  S.featWord.assign(N, 0);
  if (N == 0) return 0;
  S.nodes.emplace_back();  // root
  std::vector<int> all(N);
  for (int i = 0; i < N; i++) all[i] = i;
  step(0, all, 1, 0);
  int nWords = 0;  // createWords
  for (size_t id = 1; id < S.nodes.size(); id++)
    if (S.nodes[id].children.empty()) S.nodes[id].word = nWords++;
  // setNodeWeights
  std::vector<unsigned> Ni(nWords, 0);
  std::vector<int> counted(nWords, -1);
  int g = 0;
  for (int d = 0; d < n_docs; d++)
    for (int i = 0; i < doc_n[d]; i++, g++) {
      const int w = S.nodes[descend(S.feat[g])].word;
      S.featWord[g] = (uint32_t)w;
      if (counted[w] != d) {
        counted[w] = d;
        Ni[w]++;
      }
    }
  for (size_t id = 1; id < S.nodes.size(); id++) {
    Node& nd = S.nodes[id];
    if (nd.word < 0) continue;
    if (weighting == 1 || weighting == 3)
      nd.weight = 1;
    else if (Ni[nd.word] > 0)
      nd.weight = log((double)n_docs / (double)Ni[nd.word]);
  }
  S.stats[0] = (int)S.nodes.size() - 1;
  S.stats[1] = nWords;
  return S.stats[0];
}

// nodes 1..n in id order (orbx_vocabulary_parse_text's layout), the statistics, and per feature the node of its final training
// group and the word its descent ends in
void vt_get(int32_t* parent, int32_t* is_leaf, uint8_t* desc32, double* weight, int32_t* stats8, int32_t* feat_node,
            uint32_t* feat_word) {
  for (size_t id = 1; id < S.nodes.size(); id++) {
    parent[id - 1] = S.nodes[id].parent;
    is_leaf[id - 1] = S.nodes[id].children.empty() ? 1 : 0;
    memcpy(desc32 + (id - 1) * 32, S.nodes[id].d.b, 32);
    weight[id - 1] = S.nodes[id].weight;
  }
  memcpy(stats8, S.stats, sizeof S.stats);
  if (!S.featNode.empty()) {
    memcpy(feat_node, S.featNode.data(), S.featNode.size() * 4);
    memcpy(feat_word, S.featWord.data(), S.featWord.size() * 4);
  }
}

}  // extern "C"
