// orbx_voc_train.cpp — host side of orbx_vocabulary_train (include/orbx.h, "training"): DBoW2's TemplatedVocabulary::create
// (TemplatedVocabulary.h:569-1008) level by level.  The host keeps the tree, cuts every level's nodes into the block and chunk
// tables of orbx_voc_train_kernel.hip, waits for each round's count of running nodes, numbers the finished tree as create does
// (a node's children together, then each child's subtree, depth first) and computes the IDF weights with libm from the device's
// integer document counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx_host.h"

using namespace orbx;

namespace {

// nodes with more features than this are seeded by the grid-wide kernels (orbx_debug_voc_train_seed_grid_min; at most VT_SEED_LDS)
std::atomic<long long> g_seedGridMin{VT_SEED_LDS};

int checkHeader(int k, int L, int scoring, int weighting) {
  return k >= 2 && k <= VT_KMAX && L >= 1 && L <= 10 && scoring >= 0 && scoring <= 5 && weighting >= 0 && weighting <= 3;
}

struct Active {  // a node the next level splits
  int tnode;     // its index in the level-order tree
  int start, n;
  uint64_t key;
};

struct Tree {  // level order: the root, then every level's nodes, each node's children together
  std::vector<int> parent, first, nChild;
  std::vector<uint8_t> desc;
  int add(int p, const uint32_t* d) {
    parent.push_back(p);
    first.push_back(0);
    nChild.push_back(0);
    desc.resize(desc.size() + 32);
    if (d) memcpy(&desc[desc.size() - 32], d, 32);
    return (int)parent.size() - 1;
  }
};

template <class T>
hipError_t upload(DeviceBuf<T>& b, const std::vector<T>& v, hipStream_t st) {
  if (v.empty()) return hipSuccess;
  hipError_t e = b.grow(v.size() * sizeof(T), st);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(b, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
}

}  // namespace

extern "C" {

int orbx_debug_voc_train_seed_grid_min(long long n) {
  g_seedGridMin.store(n < 0 ? (long long)VT_SEED_LDS : std::min<long long>(n, VT_SEED_LDS));
  return ORBX_OK;
}

int orbx_vocabulary_train_device(orbx_ctx* ctx, int k, int L, int scoring, int weighting, uint64_t seed, int max_rounds, int n_docs,
                                 const uint8_t* d_desc32, const int32_t* d_n, int capacity, orbx_vocabulary** out, int32_t* stats8,
                                 uint32_t* d_feat_word) {
  if (!out) return ORBX_E_BADARG;
  *out = nullptr;
  if (!checkHeader(k, L, scoring, weighting) || n_docs < 0 || capacity < 1 || (n_docs > 0 && (!d_desc32 || !d_n))) return ORBX_E_BADARG;
  if (max_rounds <= 0) max_rounds = 100;
  if (capacity > ORBX_BOW_MAX_FEATURES || (long long)n_docs * capacity > ORBX_VOC_TRAIN_MAX_SLOTS) {
    if (ctx) ctxSetError(ctx, "vocabulary training: capacity above ORBX_BOW_MAX_FEATURES or more than ORBX_VOC_TRAIN_MAX_SLOTS feature slots");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  HIPCHK(hipSetDevice(ctxDevice(ctx)));
  hipStream_t st = ctxStream(ctx);
  int32_t stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};

  // getFeatures: the documents' features in order
  std::vector<int32_t> hn((size_t)n_docs), docOff((size_t)n_docs);
  if (n_docs) HIPCHK(hipMemcpyAsync(hn.data(), d_n, (size_t)n_docs * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  long long total = 0;
  for (int f = 0; f < n_docs; f++) {
    docOff[f] = (int32_t)total;
    total += std::min(std::max(hn[f], 0), capacity);
  }
  const int N = (int)total;
  Tree tree;
  tree.add(0, nullptr);  // root
  std::vector<uint32_t> hCentres;
  if (N > 0) {
    DeviceBuf<int32_t> dDocOff, dMinDist, dBlkNode, dBlkStart, dBlkHist, dNodeHist, dChildBase, dList, dChNode, dChStart, dStats;
    DeviceBuf<uint32_t> dPermA, dPermB, dCentres, dBlkSum, dGCnt;
    DeviceBuf<uint8_t> dAssoc;
    DeviceBuf<VtNode> dNodes;
    HIPCHK(upload(dDocOff, docOff, st));
    HIPCHK(dPermA.grow((size_t)N * 4));
    HIPCHK(dPermB.grow((size_t)N * 4));
    HIPCHK(dAssoc.grow((size_t)N));
    HIPCHK(dMinDist.grow((size_t)N * 4));
    HIPCHK(dStats.grow(sizeof stats));
    HIPCHK(hipMemsetAsync(dStats, 0, sizeof stats, st));
    HIPCHK(vtLaunchPermInit(st, d_n, dDocOff, capacity, n_docs, dPermA));
    uint32_t *perm = dPermA, *permOut = dPermB;
    const long long gridMin = g_seedGridMin.load();

    std::vector<Active> cur{{0, 0, N, 0}};
    for (int level = 1; level <= L && !cur.empty(); level++) {
      const int nNodes = (int)cur.size();
      std::vector<VtNode> hNodes((size_t)nNodes);
      std::vector<int32_t> blkNode, blkStart, chNode, chStart, lists, large, multi;
      int nKmeans = 0;
      for (int i = 0; i < nNodes; i++) {
        VtNode& nd = hNodes[i];
        memset(&nd, 0, sizeof nd);
        nd.key = cur[i].key;
        nd.start = cur[i].start;
        nd.n = cur[i].n;
        nd.blk0 = (int)blkNode.size();
        nd.multi = -1;
        const bool trivial = nd.n <= k;
        if (trivial) {
          stats[7]++;
        } else {
          stats[2]++;
          nKmeans++;
        }
        if (!trivial && nd.n > gridMin) {
          nd.form = 1;
          large.push_back(i);
        } else {
          lists.push_back(i);
        }
        for (int p = 0; p < nd.n; p += VT_THREADS) {
          blkNode.push_back(i);
          blkStart.push_back(nd.start + p);
        }
        if (!trivial) {
          if (nd.n > VT_CHUNK) {
            nd.multi = (int)multi.size();
            multi.push_back(i);
          }
          for (int p = 0; p < nd.n; p += VT_CHUNK) {
            chNode.push_back(i);
            chStart.push_back(nd.start + p);
          }
        }
      }
      const int nSmall = (int)lists.size(), nLarge = (int)large.size(), nMulti = (int)multi.size();
      lists.insert(lists.end(), large.begin(), large.end());
      lists.insert(lists.end(), multi.begin(), multi.end());
      const int nBlk = (int)blkNode.size();
      HIPCHK(upload(dNodes, hNodes, st));
      HIPCHK(upload(dBlkNode, blkNode, st));
      HIPCHK(upload(dBlkStart, blkStart, st));
      HIPCHK(upload(dChNode, chNode, st));
      HIPCHK(upload(dChStart, chStart, st));
      HIPCHK(upload(dList, lists, st));
      HIPCHK(dCentres.grow((size_t)nNodes * k * 32, st));
      HIPCHK(dBlkSum.grow((size_t)nBlk * 4, st));
      HIPCHK(dBlkHist.grow((size_t)nBlk * k * 4, st));
      HIPCHK(dNodeHist.grow((size_t)nNodes * k * 4, st));
      HIPCHK(dChildBase.grow((size_t)nNodes * k * 4, st));
      if (nMulti) {
        const size_t bytes = (size_t)nMulti * k * (VT_THREADS + 1) * 4;
        HIPCHK(dGCnt.grow(bytes, st));
        HIPCHK(hipMemsetAsync(dGCnt, 0, bytes, st));
      }
      HIPCHK(hipMemsetAsync(dAssoc, 0xff, (size_t)N, st));

      VtArgs a{};
      a.feat = reinterpret_cast<const uint32_t*>(d_desc32);
      a.perm = perm;
      a.permOut = permOut;
      a.assoc = dAssoc;
      a.minDist = dMinDist;
      a.nodes = dNodes;
      a.centres = dCentres;
      a.nNodes = nNodes;
      a.k = k;
      a.maxRounds = max_rounds;
      a.nBlk = nBlk;
      a.seed = seed;
      a.blkNode = dBlkNode;
      a.blkStart = dBlkStart;
      a.blkSum = dBlkSum;
      a.blkHist = dBlkHist;
      a.nodeHist = dNodeHist;
      a.childBase = dChildBase;
      a.nChunk = (int)chNode.size();
      a.chNode = dChNode;
      a.chStart = dChStart;
      a.gCnt = dGCnt;
      a.stats = dStats;
      VtArgs aSmall = a, aLarge = a, aMulti = a;
      aSmall.list = dList;
      aSmall.nList = nSmall;
      aLarge.list = dList + nSmall;
      aLarge.nList = nLarge;
      aMulti.list = dList + nSmall + nLarge;
      aMulti.nList = nMulti;

      // seeding (and the trivial nodes)
      HIPCHK(vtLaunchSeedSmall(st, aSmall));
      if (nLarge) {
        HIPCHK(vtLaunchSeedFirst(st, aLarge));
        for (int c = 1; c < k; c++) {
          HIPCHK(vtLaunchSeedUpdate(st, aLarge, c));
          HIPCHK(vtLaunchSeedPick(st, aLarge, c));
        }
      }
      // rounds, until no node of the level is running
      for (int round = 0; nKmeans > 0; round++) {
        HIPCHK(hipMemsetAsync(dStats + 8, 0, 4, st));
        HIPCHK(vtLaunchAssign(st, a));
        HIPCHK(vtLaunchRound(st, a));
        int32_t running = 0;
        HIPCHK(hipMemcpyAsync(&running, dStats + 8, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (running == 0 || round >= max_rounds) break;
        HIPCHK(vtLaunchCount(st, a));
        HIPCHK(vtLaunchCentreFinal(st, aMulti));
      }
      // the next level's groups
      HIPCHK(vtLaunchHist(st, a));
      HIPCHK(vtLaunchScan(st, a));
      HIPCHK(vtLaunchScatter(st, a));
      std::swap(perm, permOut);
      std::vector<int32_t> hHist((size_t)nNodes * k);
      hCentres.resize((size_t)nNodes * k * 8);
      HIPCHK(hipMemcpyAsync(hNodes.data(), dNodes, (size_t)nNodes * sizeof(VtNode), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hHist.data(), dNodeHist, hHist.size() * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hCentres.data(), dCentres, hCentres.size() * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      std::vector<Active> next;
      for (int i = 0; i < nNodes; i++) {
        const int nC = hNodes[i].nC, tn = cur[i].tnode;
        tree.nChild[tn] = nC;
        int pos = cur[i].start;
        for (int c = 0; c < nC; c++) {
          const int child = tree.add(tn, &hCentres[((size_t)i * k + c) * 8]);
          if (c == 0) tree.first[tn] = child;
          const int m = hHist[(size_t)i * k + c];
          if (level < L && m > 1) next.push_back({child, pos, m, 21 * cur[i].key + (uint64_t)c + 1});
          pos += m;
        }
      }
      cur.swap(next);
    }
    int32_t dev[9];  // the kernels' counters: most rounds, capped runs, emptied clusters, short seedings
    HIPCHK(hipMemcpyAsync(dev, dStats, sizeof dev, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 3; i <= 6; i++) stats[i] = dev[i];
  }

  // create's numbering: a node's children together, then each child's subtree in order
  const int nTree = (int)tree.parent.size(), nOut = N > 0 ? nTree - 1 : 0;
  std::vector<int> newId((size_t)nTree, 0), order;  // order: new id -> level-order index
  order.reserve(nTree);
  order.push_back(0);
  {
    int nextId = 1;
    std::vector<std::pair<int, int>> stack;  // (node, next child to descend into)
    stack.push_back({0, -1});
    while (!stack.empty()) {
      auto& top = stack.back();
      const int nd = top.first;
      if (top.second < 0) {
        for (int c = 0; c < tree.nChild[nd]; c++) {
          newId[tree.first[nd] + c] = nextId++;
          order.push_back(tree.first[nd] + c);
        }
        top.second = 0;
      }
      if (top.second >= tree.nChild[nd]) {
        stack.pop_back();
        continue;
      }
      const int child = tree.first[nd] + top.second++;
      if (tree.nChild[child] > 0) stack.push_back({child, -1});
    }
  }
  std::vector<int32_t> parent((size_t)nOut), leaf((size_t)nOut);
  std::vector<uint8_t> desc((size_t)nOut * 32);
  std::vector<double> weight((size_t)nOut, 0.0);
  std::vector<int> wordNode;  // word id -> output index
  for (int id = 1; id <= nOut; id++) {
    const int t = order[id];
    parent[id - 1] = newId[tree.parent[t]];
    leaf[id - 1] = tree.nChild[t] == 0;
    memcpy(&desc[(size_t)(id - 1) * 32], &tree.desc[(size_t)t * 32], 32);
    if (leaf[id - 1]) {
      weight[id - 1] = 1.0;  // (every word reachable for the descent below; TF and BINARY keep it)
      wordNode.push_back(id - 1);
    }
  }
  const int nWords = (int)wordNode.size();
  orbx_vocabulary* voc = nullptr;
  r = orbx_vocabulary_create(ctx, k, L, scoring, weighting, nOut, parent.data(), leaf.data(), desc.data(), weight.data(), &voc);
  if (r != ORBX_OK) return r;
  const bool idf = weighting == ORBX_BOW_TF_IDF || weighting == ORBX_BOW_IDF;
  if (nOut > 0 && (idf || d_feat_word)) {
    auto body = [&]() -> int {
      const BowNode* dBowNodes = nullptr;
      const uint32_t* dFin = nullptr;
      int rr = vocDescend(ctx, voc, n_docs, d_desc32, d_n, capacity, &dBowNodes, &dFin);
      if (rr != ORBX_OK) return rr;
      DeviceBuf<uint32_t> dNi;
      std::vector<uint32_t> Ni((size_t)nWords, 0);
      if (idf) {
        HIPCHK(dNi.grow((size_t)nWords * 4));
        HIPCHK(hipMemsetAsync(dNi, 0, (size_t)nWords * 4, st));
      }
      HIPCHK(vtLaunchDocFreq(st, dBowNodes, dFin, d_n, capacity, n_docs, d_feat_word, idf ? (uint32_t*)dNi : nullptr));
      if (idf) HIPCHK(hipMemcpyAsync(Ni.data(), dNi, (size_t)nWords * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (idf)  // setNodeWeights (:997-1004): ln(NDocs / Ni) with the host's libm, 0 for a word no document reaches
        for (int w = 0; w < nWords; w++) weight[wordNode[w]] = Ni[w] > 0 ? log((double)n_docs / (double)Ni[w]) : 0.0;
      return ORBX_OK;
    };
    r = body();
    if (r == ORBX_OK && idf) {
      orbx_vocabulary_destroy(voc);
      voc = nullptr;
      r = orbx_vocabulary_create(ctx, k, L, scoring, weighting, nOut, parent.data(), leaf.data(), desc.data(), weight.data(), &voc);
    }
    if (r != ORBX_OK) {
      if (voc) orbx_vocabulary_destroy(voc);
      return r;
    }
  }
  stats[0] = nOut;
  stats[1] = nWords;
  if (stats8) memcpy(stats8, stats, 8 * sizeof(int32_t));
  *out = voc;
  return ORBX_OK;
}

int orbx_vocabulary_train(orbx_ctx* ctx, int k, int L, int scoring, int weighting, uint64_t seed, int max_rounds, int n_docs,
                          const uint8_t* desc32, const int32_t* doc_n, orbx_vocabulary** out, int32_t* stats8, uint32_t* feat_word) {
  if (!out) return ORBX_E_BADARG;
  *out = nullptr;
  if (!checkHeader(k, L, scoring, weighting) || n_docs < 0 || (n_docs > 0 && !doc_n)) return ORBX_E_BADARG;
  int cap = 1;
  long long total = 0;
  for (int f = 0; f < n_docs; f++) {
    if (doc_n[f] < 0) return ORBX_E_BADARG;
    cap = std::max(cap, doc_n[f]);
    total += doc_n[f];
  }
  if (total > 0 && !desc32) return ORBX_E_BADARG;
  if (cap > ORBX_BOW_MAX_FEATURES || (long long)n_docs * cap > ORBX_VOC_TRAIN_MAX_SLOTS) {
    if (ctx) ctxSetError(ctx, "vocabulary training: a document above ORBX_BOW_MAX_FEATURES or more than ORBX_VOC_TRAIN_MAX_SLOTS feature slots");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  HIPCHK(hipSetDevice(ctxDevice(ctx)));
  hipStream_t st = ctxStream(ctx);
  // the extractor's batch layout: document f at f * cap
  const size_t slots = std::max<size_t>((size_t)n_docs * cap, 1);
  std::vector<uint8_t> padded(slots * 32, 0);
  size_t off = 0;
  for (int f = 0; f < n_docs; f++) {
    if (doc_n[f]) memcpy(&padded[(size_t)f * cap * 32], desc32 + off * 32, (size_t)doc_n[f] * 32);
    off += doc_n[f];
  }
  DeviceBuf<uint8_t> dDesc;
  DeviceBuf<int32_t> dN;
  DeviceBuf<uint32_t> dFw;
  HIPCHK(dDesc.grow(slots * 32));
  HIPCHK(dN.grow(std::max<size_t>((size_t)n_docs, 1) * 4));
  if (feat_word) HIPCHK(dFw.grow(slots * 4));
  HIPCHK(hipMemcpyAsync(dDesc, padded.data(), slots * 32, hipMemcpyHostToDevice, st));
  if (n_docs) HIPCHK(hipMemcpyAsync(dN, doc_n, (size_t)n_docs * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  r = orbx_vocabulary_train_device(ctx, k, L, scoring, weighting, seed, max_rounds, n_docs, dDesc, dN, cap, out, stats8,
                                   feat_word ? (uint32_t*)dFw : nullptr);
  if (r != ORBX_OK) return r;
  if (feat_word && total > 0) {
    std::vector<uint32_t> fw(slots);
    HIPCHK(hipMemcpyAsync(fw.data(), dFw, slots * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    off = 0;
    for (int f = 0; f < n_docs; f++) {
      if (doc_n[f]) memcpy(feat_word + off, &fw[(size_t)f * cap], (size_t)doc_n[f] * 4);
      off += doc_n[f];
    }
  }
  return ORBX_OK;
}

}  // extern "C"
