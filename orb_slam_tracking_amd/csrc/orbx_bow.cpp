// orbx_bow.cpp — host side of the bag-of-words path (include/orbx.h, "bag of words"): the text parser of DBoW2's
// TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1542-1620), the checks of the tree, its breadth-first device
// layout and the C entry points of the transform and the L1 score.  The kernels are in orbx_bow_kernel.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "orbx_host.h"

using namespace orbx;

struct orbx_vocabulary {
  orbx_ctx* ctx = nullptr;
  int device = 0;
  int k = 0, L = 0, scoring = 0, weighting = 0, nNodes = 0, nWords = 0;
  int nStaged = 0;            // breadth-first nodes k_bow_descend stages in LDS
  DeviceBuf<BowNode> dNodes;  // [nNodes + 1]
  DeviceBuf<uint32_t> dDesc;  // [nNodes + 1][8]
  // scratch of the calls (grown on demand; the stream is drained before a buffer is replaced)
  DeviceBuf<uint32_t> dScratch;  // fin, nid: [2][frames * capacity]
  DeviceBuf<uint8_t> dIo;        // staging of orbx_bow_transform / orbx_bow_score
  HeldArray<int32_t> pairs;      // orbx_bow_score_batch_device's pair list [2][n_pairs] of the last call
  // nodes 1..nNodes in file order as they were given (orbx_vocabulary_get_nodes, orbx_vocabulary_save_text)
  std::vector<int32_t> hParent, hLeaf;
  std::vector<uint8_t> hDesc;
  std::vector<double> hWeight;
};

namespace {

// the reference's own ranges (:1561-1566)
bool headerOk(int k, int L, int scoring, int weighting) {
  return k >= 0 && k <= 20 && L >= 1 && L <= 10 && scoring >= 0 && scoring <= 5 && weighting >= 0 && weighting <= 3;
}

// deviation 3: parents in [0, own id), at most k children, depth <= L; *depth [n + 1] of every node (root 0)
bool treeOk(int k, int L, int n, const int32_t* parent, std::vector<int>* depth, std::vector<int>* nChild) {
  depth->assign((size_t)n + 1, 0);
  nChild->assign((size_t)n + 1, 0);
  for (int id = 1; id <= n; id++) {
    const int p = parent[id - 1];
    if (p < 0 || p >= id) return false;
    if (++(*nChild)[p] > k) return false;
    if (((*depth)[id] = (*depth)[p] + 1) > L) return false;
  }
  return true;
}

// istream >> int on one whitespace-separated token: an optional sign and decimal digits, within int
bool parseInt(const char** s, int* out) {
  const char* p = *s;
  while (*p && isspace((unsigned char)*p)) p++;
  if (!*p) return false;
  char* end = nullptr;
  errno = 0;
  const long v = strtol(p, &end, 10);
  if (end == p || errno == ERANGE || v < -2147483647L - 1 || v > 2147483647L) return false;
  if (*end && !isspace((unsigned char)*end)) return false;
  *out = (int)v;
  *s = end;
  return true;
}

// istream >> double on one whitespace-separated token that is a complete finite decimal number, [+-]? (d+ (.d*)? | .d+)
// ([eE] [+-]? d+)?: for those, libstdc++'s num_get hands exactly the token to strtod, so the value is strtod's.  Refused
// (deviation 3), because the reference reads them without a reported error into another value: no number (inf, nan, "1e": 0),
// a hexadecimal float (its leading 0), trailing characters (the number before them) and an overflow (+-DBL_MAX).
bool parseDouble(const char** s, double* out) {
  const char* p = *s;
  while (*p && isspace((unsigned char)*p)) p++;
  const char* q = p;
  if (*q == '+' || *q == '-') q++;
  const char* mant = q;
  while (isdigit((unsigned char)*q)) q++;
  bool digits = q != mant;
  if (*q == '.') {
    const char* frac = ++q;
    while (isdigit((unsigned char)*q)) q++;
    digits = digits || q != frac;
  }
  if (!digits) return false;
  if (*q == 'e' || *q == 'E') {
    q++;
    if (*q == '+' || *q == '-') q++;
    const char* exp = q;
    while (isdigit((unsigned char)*q)) q++;
    if (q == exp) return false;
  }
  if (*q && !isspace((unsigned char)*q)) return false;
  char* end = nullptr;
  const double v = strtod(p, &end);
  if (end != q || std::isinf(v)) return false;
  *out = v;
  *s = end;
  return true;
}

bool blankLine(const std::string& s) {
  for (char c : s)
    if (!isspace((unsigned char)c)) return false;
  return true;
}

struct ParsedVoc {
  int header[4];
  std::vector<int32_t> parent, leaf;
  std::vector<uint8_t> desc;
  std::vector<double> weight;
};

int parseFile(const char* path, ParsedVoc* v) {
  if (!path) return ORBX_E_BADARG;
  FILE* fp = fopen(path, "rb");
  if (!fp) return ORBX_E_BADARG;
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, got);
  fclose(fp);
  size_t pos = 0;
  bool first = true;
  while (pos < text.size()) {
    size_t eol = text.find('\n', pos);
    if (eol == std::string::npos) eol = text.size();
    const std::string line = text.substr(pos, eol - pos);
    pos = eol + 1;
    const char* s = line.c_str();
    if (first) {
      first = false;
      for (int i = 0; i < 4; i++)
        if (!parseInt(&s, &v->header[i])) return ORBX_E_BADARG;
      if (!headerOk(v->header[0], v->header[1], v->header[2], v->header[3])) return ORBX_E_BADARG;
      continue;
    }
    if (blankLine(line)) continue;  // deviation 1
    int p, leaf, d;
    double w;
    if (!parseInt(&s, &p) || !parseInt(&s, &leaf)) return ORBX_E_BADARG;
    v->parent.push_back(p);
    v->leaf.push_back(leaf);
    for (int i = 0; i < 32; i++) {
      if (!parseInt(&s, &d)) return ORBX_E_BADARG;
      v->desc.push_back((uint8_t)d);  // FORB::fromString: int, then (unsigned char)
    }
    if (!parseDouble(&s, &w)) return ORBX_E_BADARG;
    v->weight.push_back(w);
  }
  if (first) return ORBX_E_BADARG;  // no header
  std::vector<int> depth, nChild;
  if (!treeOk(v->header[0], v->header[1], (int)v->parent.size(), v->parent.data(), &depth, &nChild)) return ORBX_E_BADARG;
  return ORBX_OK;
}

// (the buffers are freed on the vocabulary's device: when it cannot be made current, the vocabulary is left as it is)
void freeVoc(orbx_vocabulary* v) {
  if (hipSetDevice(v->device) == hipSuccess) delete v;
}

int transformIssue(orbx_ctx* ctx, orbx_vocabulary* v, int n_frames, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                   int levelsup, uint32_t* d_bow_word, double* d_bow_value, int32_t* d_bow_n, uint32_t* d_fv_node,
                   uint32_t* d_fv_feat, int32_t* d_fv_n, uint32_t* d_feat_word) {
  const size_t entries = (size_t)n_frames * capacity;
  HIPCHK(v->dScratch.grow(entries * 2 * sizeof(uint32_t), ctxStream(ctx)));  // fin, nid
  BowArgs a{};
  a.nodes = v->dNodes;
  a.desc = v->dDesc;
  a.nStaged = v->nStaged;
  a.nidLevel = v->L - levelsup;
  a.fdesc = d_desc32;
  a.n = d_n;
  a.cap = capacity;
  a.nFrames = n_frames;
  a.fin = v->dScratch;
  a.nid = v->dScratch + entries;
  a.weighting = v->weighting;
  a.norm = v->scoring == ORBX_BOW_DOT_PRODUCT ? 0 : (v->scoring == ORBX_BOW_L2_NORM ? 2 : 1);  // mustNormalize (ScoringObject.h:72-88)
  a.hasWords = v->nWords > 0;
  a.bowWord = d_bow_word;
  a.bowValue = d_bow_value;
  a.bowN = d_bow_n;
  a.fvNode = d_fv_node;
  a.fvFeat = d_fv_feat;
  a.fvN = d_fv_n;
  a.featWord = d_feat_word;
  HIPCHK(launch_bow_transform(ctxStream(ctx), a));
  return ORBX_OK;
}

int checkVoc(orbx_ctx* ctx, const orbx_vocabulary* voc) {
  if (!ctx || !voc) return ORBX_E_BADARG;
  if (voc->ctx != ctx) {
    ctxSetError(ctx, "the vocabulary belongs to another context");
    return ORBX_E_BADARG;
  }
  return ORBX_OK;
}

}  // namespace

namespace orbx {
// what orbx_db.cpp and orbx_voc_train.cpp need of a vocabulary (orbx_host.h)
orbx_ctx* vocCtx(const orbx_vocabulary* v) { return v->ctx; }

int vocDescend(orbx_ctx* ctx, orbx_vocabulary* v, int n_frames, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
               const BowNode** nodes, const uint32_t** fin) {
  const size_t entries = (size_t)n_frames * capacity;
  HIPCHK(v->dScratch.grow(entries * 2 * sizeof(uint32_t), ctxStream(ctx)));
  BowArgs a{};
  a.nodes = v->dNodes;
  a.desc = v->dDesc;
  a.nStaged = v->nStaged;
  a.nidLevel = v->L;
  a.fdesc = d_desc32;
  a.n = d_n;
  a.cap = capacity;
  a.nFrames = n_frames;
  a.fin = v->dScratch;
  a.nid = v->dScratch + entries;
  HIPCHK(launch_bow_descend(ctxStream(ctx), a));
  *nodes = v->dNodes;
  *fin = v->dScratch;
  return ORBX_OK;
}
}  // namespace orbx

extern "C" {

int orbx_vocabulary_parse_text(const char* path, int32_t* header, int32_t* n_nodes, int32_t* parent, int32_t* is_leaf,
                               uint8_t* desc32, double* weight, int32_t capacity) {
  ParsedVoc v;
  const int r = parseFile(path, &v);
  if (r != ORBX_OK) return r;
  const int n = (int)v.parent.size();
  if (header) memcpy(header, v.header, sizeof v.header);
  if (n_nodes) *n_nodes = n;
  if (parent || is_leaf || desc32 || weight) {
    if (capacity < n) return ORBX_E_CAPACITY;
    if (parent && n) memcpy(parent, v.parent.data(), (size_t)n * 4);
    if (is_leaf && n) memcpy(is_leaf, v.leaf.data(), (size_t)n * 4);
    if (desc32 && n) memcpy(desc32, v.desc.data(), (size_t)n * 32);
    if (weight && n) memcpy(weight, v.weight.data(), (size_t)n * 8);
  }
  return n;
}

int orbx_vocabulary_create(orbx_ctx* ctx, int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                           const int32_t* is_leaf, const uint8_t* desc32, const double* weight, orbx_vocabulary** out) {
  if (!out) return ORBX_E_BADARG;
  *out = nullptr;
  if (!headerOk(k, L, scoring, weighting) || n_nodes < 0 || (n_nodes > 0 && (!parent || !is_leaf || !desc32 || !weight)))
    return ORBX_E_BADARG;
  std::vector<int> depth, nChild;
  if (!treeOk(k, L, n_nodes, parent, &depth, &nChild)) {
    if (ctx) ctxSetError(ctx, "vocabulary: a parent outside [0, id), more than k children or deeper than L");
    return ORBX_E_BADARG;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  // breadth-first order: the root, then level by level, each node's children contiguous and in file order
  const int N = n_nodes + 1;
  std::vector<int> firstChild(N, 0), childStart(N + 1, 0);
  for (int id = 1; id < N; id++) childStart[parent[id - 1] + 1]++;
  for (int i = 0; i < N; i++) childStart[i + 1] += childStart[i];
  std::vector<int> children(n_nodes), fill(childStart.begin(), childStart.end() - 1);
  for (int id = 1; id < N; id++) children[fill[parent[id - 1]]++] = id;  // ids ascending = file order
  std::vector<int> order;  // breadth-first position -> node id
  order.reserve(N);
  order.push_back(0);
  for (size_t h = 0; h < order.size(); h++) {
    const int id = order[h];
    for (int c = childStart[id]; c < childStart[id + 1]; c++) order.push_back(children[c]);
  }
  std::vector<int> bfs(N);
  for (int i = 0; i < N; i++) bfs[order[i]] = i;
  std::vector<uint32_t> wordOf(N, 0);
  int nWords = 0;
  for (int id = 1; id < N; id++)
    if (is_leaf[id - 1] > 0) wordOf[id] = (uint32_t)nWords++;
  std::vector<BowNode> nodes(N);
  std::vector<uint32_t> desc((size_t)N * 8, 0);
  int nStaged = 0;
  for (int i = 0; i < N; i++) {
    const int id = order[i];
    BowNode& b = nodes[i];
    b.nChild = nChild[id];
    b.first = b.nChild ? bfs[children[childStart[id]]] : 0;
    b.word = wordOf[id];
    b.id = (uint32_t)id;
    b.weight = id ? weight[id - 1] : 0.0;
    if (id) memcpy(&desc[(size_t)i * 8], desc32 + (size_t)(id - 1) * 32, 32);
    if (depth[id] <= 3 && i < BOW_LDS_NODES) nStaged = i + 1;  // levels 0-3, a prefix of the breadth-first order
  }
  orbx_vocabulary* v = new orbx_vocabulary();
  v->ctx = ctx;
  v->device = ctxDevice(ctx);
  v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting;
  v->nNodes = n_nodes; v->nWords = nWords; v->nStaged = nStaged;
  if (n_nodes > 0) {
    v->hParent.assign(parent, parent + n_nodes);
    v->hLeaf.assign(is_leaf, is_leaf + n_nodes);
    v->hDesc.assign(desc32, desc32 + (size_t)n_nodes * 32);
    v->hWeight.assign(weight, weight + n_nodes);
  }
  auto body = [&]() -> int {
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(v->dNodes.grow(sizeof(BowNode) * N));
    HIPCHK(v->dDesc.grow((size_t)32 * N));
    HIPCHK(hipMemcpy(v->dNodes, nodes.data(), sizeof(BowNode) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(v->dDesc, desc.data(), (size_t)32 * N, hipMemcpyHostToDevice));
    return ORBX_OK;
  };
  const int r = body();
  if (r != ORBX_OK) {
    freeVoc(v);
    return r;
  }
  *out = v;
  return ORBX_OK;
}

int orbx_vocabulary_load_text(orbx_ctx* ctx, const char* path, orbx_vocabulary** out) {
  if (!out) return ORBX_E_BADARG;
  *out = nullptr;
  ParsedVoc v;
  const int r = parseFile(path, &v);
  if (r != ORBX_OK) {
    if (ctx) ctxSetError(ctx, "vocabulary: the file cannot be read or is not a vocabulary text file");
    return r;
  }
  return orbx_vocabulary_create(ctx, v.header[0], v.header[1], v.header[2], v.header[3], (int)v.parent.size(), v.parent.data(),
                                v.leaf.data(), v.desc.data(), v.weight.data(), out);
}

void orbx_vocabulary_destroy(orbx_vocabulary* voc) {
  if (voc) freeVoc(voc);
}

int orbx_vocabulary_info(const orbx_vocabulary* voc, int32_t* info6) {
  if (!voc || !info6) return ORBX_E_BADARG;
  const int32_t v[6] = {voc->k, voc->L, voc->scoring, voc->weighting, voc->nNodes, voc->nWords};
  memcpy(info6, v, sizeof v);
  return ORBX_OK;
}

int orbx_vocabulary_get_nodes(const orbx_vocabulary* voc, int32_t* parent, int32_t* is_leaf, uint8_t* desc32, double* weight,
                              int32_t capacity) {
  if (!voc) return ORBX_E_BADARG;
  const int n = voc->nNodes;
  if (parent || is_leaf || desc32 || weight) {
    if (capacity < n) return ORBX_E_CAPACITY;
    if (parent && n) memcpy(parent, voc->hParent.data(), (size_t)n * 4);
    if (is_leaf && n) memcpy(is_leaf, voc->hLeaf.data(), (size_t)n * 4);
    if (desc32 && n) memcpy(desc32, voc->hDesc.data(), (size_t)n * 32);
    if (weight && n) memcpy(weight, voc->hWeight.data(), (size_t)n * 8);
  }
  return n;
}

int orbx_vocabulary_save_text(const orbx_vocabulary* voc, const char* path, int exact) {
  if (!voc || !path) return ORBX_E_BADARG;
  FILE* fp = fopen(path, "wb");
  if (!fp) return ORBX_E_BADARG;
  // saveToTextFile (:1626-1645): "k L  scoring weighting", then per node "parent flag d0 .. d31 weight"
  fprintf(fp, "%d %d  %d %d\n", voc->k, voc->L, voc->scoring, voc->weighting);
  for (int i = 0; i < voc->nNodes; i++) {
    fprintf(fp, "%d %d ", voc->hParent[i], voc->hLeaf[i]);
    for (int j = 0; j < 32; j++) fprintf(fp, "%d ", (int)voc->hDesc[(size_t)i * 32 + j]);  // FORB::toString
    fprintf(fp, exact ? "%.17g\n" : "%g\n", voc->hWeight[i]);  // (%g: an ostream's default, 6 significant digits)
  }
  const bool bad = ferror(fp) != 0;
  return (fclose(fp) != 0 || bad) ? ORBX_E_BADARG : ORBX_OK;
}

int orbx_bow_transform_batch_device(orbx_ctx* ctx, const orbx_vocabulary* voc, int n_frames, const uint8_t* d_desc32,
                                    const int32_t* d_n, int capacity, int levelsup, uint32_t* d_bow_word, double* d_bow_value,
                                    int32_t* d_bow_n, uint32_t* d_fv_node, uint32_t* d_fv_feat, int32_t* d_fv_n,
                                    uint32_t* d_feat_word) {
  int r = checkVoc(ctx, voc);
  if (r != ORBX_OK) return r;
  const int fv = (d_fv_node != nullptr) + (d_fv_feat != nullptr) + (d_fv_n != nullptr);
  if (n_frames < 0 || capacity < 1 || !d_desc32 || !d_n || !d_bow_word || !d_bow_value || !d_bow_n || (fv != 0 && fv != 3))
    return ORBX_E_BADARG;
  if (capacity > ORBX_BOW_MAX_FEATURES) {
    ctxSetError(ctx, "bow transform: capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  if (n_frames == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  return transformIssue(ctx, const_cast<orbx_vocabulary*>(voc), n_frames, d_desc32, d_n, capacity, levelsup, d_bow_word,
                        d_bow_value, d_bow_n, d_fv_node, d_fv_feat, d_fv_n, d_feat_word);
}

int orbx_bow_transform(orbx_ctx* ctx, const orbx_vocabulary* voc, const uint8_t* desc32, int n, int levelsup, uint32_t* bow_word,
                       double* bow_value, int32_t* bow_n, uint32_t* fv_node, uint32_t* fv_feat, int32_t* fv_n, uint32_t* feat_word) {
  int r = checkVoc(ctx, voc);
  if (r != ORBX_OK) return r;
  const int fv = (fv_node != nullptr) + (fv_feat != nullptr) + (fv_n != nullptr);
  if (n < 0 || (n > 0 && (!desc32 || !bow_word || !bow_value)) || !bow_n || (fv != 0 && fv != 3)) return ORBX_E_BADARG;
  if (n > ORBX_BOW_MAX_FEATURES) {
    ctxSetError(ctx, "bow transform: more than ORBX_BOW_MAX_FEATURES descriptors");
    return ORBX_E_CAPACITY;
  }
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  orbx_vocabulary* v = const_cast<orbx_vocabulary*>(voc);
  const int cap = n > 0 ? n : 1;
  const size_t c = (size_t)cap;
  const int32_t hn = n;
  int32_t counts[3] = {0, 0, 0};
  Staged io(v->dIo, ctxStream(ctx));
  auto dD = io.in(desc32, (size_t)n * 32, c * 32);  // descriptors
  auto dN = io.in(&hn, 1, 4);                        // counts: n, bow_n, fv_n
  io.out(dN, 0, counts, 3);
  auto dW = io.room<uint32_t>(c);                    // bow words
  auto dFn = io.room<uint32_t>(c);                   // fv nodes
  auto dFf = io.room<uint32_t>(c);                   // fv features
  auto dFw = io.optOut(feat_word, n, c);             // feat words
  auto dV = io.room<double>(c);                      // bow values
  HIPCHK(io.open());
  r = transformIssue(ctx, v, 1, io[dD], io[dN], cap, levelsup, io[dW], io[dV], io[dN] + 1, fv ? io[dFn] : nullptr, fv ? io[dFf] : nullptr,
                     fv ? io[dN] + 2 : nullptr, io[dFw]);
  r = io.close(ctx, r);
  if (r != ORBX_OK) return r;
  // what the counts, now here, say there is of each
  *bow_n = counts[1];
  io.out(dW, 0, bow_word, counts[1]);
  io.out(dV, 0, bow_value, counts[1]);
  if (fv) {
    *fv_n = counts[2];
    io.out(dFn, 0, fv_node, counts[2]);
    io.out(dFf, 0, fv_feat, counts[2]);
  }
  return io.close(ctx, ORBX_OK);
}

int orbx_bow_score_batch_device(orbx_ctx* ctx, const orbx_vocabulary* voc, int n_frames, int n_pairs, const int32_t* h_first,
                                const int32_t* h_second, const uint32_t* d_bow_word, const double* d_bow_value,
                                const int32_t* d_bow_n, int capacity, double* d_score_f64) {
  int r = checkVoc(ctx, voc);
  if (r != ORBX_OK) return r;
  if (voc->scoring != ORBX_BOW_L1_NORM) {
    ctxSetError(ctx, "bow score: only L1Scoring is offered");
    return ORBX_E_BADARG;
  }
  if (n_frames < 1 || n_pairs < 0 || capacity < 1 || capacity > ORBX_BOW_MAX_FEATURES || (n_pairs > 0 && (!h_first || !h_second)) ||
      !d_bow_word || !d_bow_value || !d_bow_n || !d_score_f64)
    return ORBX_E_BADARG;
  if (!pairsInRange(h_first, h_second, n_pairs, n_frames)) {
    ctxSetError(ctx, "pair index outside [0, n_frames)");
    return ORBX_E_BADARG;
  }
  if (n_pairs == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  orbx_vocabulary* v = const_cast<orbx_vocabulary*>(voc);
  hipStream_t st = ctxStream(ctx);
  HIPCHK(HeldUploads(st)(v->pairs, {h_first, h_second}, n_pairs));
  BowScoreArgs s{};
  s.word = d_bow_word;
  s.value = d_bow_value;
  s.n = d_bow_n;
  s.cap = capacity;
  s.nPairs = n_pairs;
  s.pairs = v->pairs;
  s.score = d_score_f64;
  HIPCHK(launch_bow_score_l1(st, s));
  return ORBX_OK;
}

int orbx_bow_score(orbx_ctx* ctx, const orbx_vocabulary* voc, const uint32_t* w1, const double* v1, int n1, const uint32_t* w2,
                   const double* v2, int n2, double* score) {
  int r = checkVoc(ctx, voc);
  if (r != ORBX_OK) return r;
  if (!score || n1 < 0 || n2 < 0 || (n1 > 0 && (!w1 || !v1)) || (n2 > 0 && (!w2 || !v2))) return ORBX_E_BADARG;
  const int cap = std::max(std::max(n1, n2), 1);
  if (cap > ORBX_BOW_MAX_FEATURES) return ORBX_E_CAPACITY;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  orbx_vocabulary* v = const_cast<orbx_vocabulary*>(voc);
  const size_t c = (size_t)cap;
  const int32_t hn[2] = {n1, n2};
  Staged io(v->dIo, ctxStream(ctx));  // the two frames' words and values, their counts, the score
  auto dW = io.in(w1, n1, 2 * c);
  io.in(dW, c, w2, n2);
  auto dV = io.in(v1, n1, 2 * c);
  io.in(dV, c, v2, n2);
  auto dN = io.in(hn, 2, 2);
  auto dS = io.out(score, 1, 1);
  HIPCHK(io.open());
  const int32_t f0 = 0, f1 = 1;
  r = orbx_bow_score_batch_device(ctx, voc, 2, 1, &f0, &f1, io[dW], io[dV], io[dN], cap, io[dS]);
  return io.close(ctx, r);
}

}  // extern "C"
