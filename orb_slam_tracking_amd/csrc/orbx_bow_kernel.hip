// orbx_bow_kernel.hip — DBoW2's TemplatedVocabulary<FORB>::transform (BowVector, FeatureVector) and L1Scoring::score on the
// device, for batches of frames (Thirdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1078-1270, src/BowVector.cpp:36-86,
// src/FeatureVector.cpp:31-45, src/ScoringObject.cpp:23-66).
//
//   k_bow_descend      lane per descriptor        the descent of one feature (:1230-1270): at every level the child with the
//                                                 smallest Hamming distance, the first among equals; the breadth-first prefix of
//                                                 the tree (levels 1-3 at k = 10) is read from LDS, deeper levels from global
//   k_bow_assemble     workgroup per frame        both vectors: (word, feature) keys sorted in LDS, one f64 chain per word in
//                                                 feature order, the norm as ONE ordered f64 chain over the words, the division;
//                                                 then (node, feature) keys sorted for the FeatureVector
//   k_bow_score_l1     wave per pair              L1Scoring::score: each word of v1 searched in v2, the terms of the common words
//                                                 added in ascending word order
//
// Integer distances and f64 arithmetic without contraction (-ffp-contract=off), every sum in the reference's order, so the
// results equal a CPU restatement (tests/cpp/bow_ref.cpp) bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orbx_bow_terms.h"
#include "orbx_launch.h"

namespace orbx {

namespace {

constexpr int BOW_CHUNK = 10;  // children whose descriptors are loaded before the first distance (one chunk per level at k = 10)

__device__ __forceinline__ uint32_t hamming32(const uint4& qa, const uint4& qb, const uint4& a, const uint4& b) {
  return __popc(qa.x ^ a.x) + __popc(qa.y ^ a.y) + __popc(qa.z ^ a.z) + __popc(qa.w ^ a.w) + __popc(qb.x ^ b.x) +
         __popc(qb.y ^ b.y) + __popc(qb.z ^ b.z) + __popc(qb.w ^ b.w);
}

}  // namespace

__global__ __launch_bounds__(BOW_DESCEND_THREADS) void k_bow_descend(BowArgs a) {
  __shared__ uint4 sDesc[BOW_LDS_NODES * 2];
  const long long g = (long long)blockIdx.x * BOW_DESCEND_THREADS + threadIdx.x;
  const int f = (int)(g / a.cap), i = (int)(g - (long long)f * a.cap);
  const bool active = f < a.nFrames && i < clampN(a.n, f, a.cap);
  if (!__syncthreads_or(active)) return;  // (a whole workgroup beyond every frame's count: nothing to stage)
  const uint4* gDesc = reinterpret_cast<const uint4*>(a.desc);
  for (int j = threadIdx.x; j < 2 * a.nStaged; j += BOW_DESCEND_THREADS) sDesc[j] = gDesc[j];
  __syncthreads();
  if (!active) return;
  const uint4* q = reinterpret_cast<const uint4*>(a.fdesc + ((size_t)f * a.cap + i) * 32);
  const uint4 qa = q[0], qb = q[1];
  int cur = 0, depth = 0, nidNode = a.nidLevel <= 0 ? 0 : -1;  // breadth-first index of the FeatureVector's node (root: 0)
  for (;;) {
    const BowNode nd = a.nodes[cur];
    if (nd.nChild == 0) break;  // isLeaf()
    ++depth;
    int best = nd.first;
    uint32_t bestD = 0xffffffffu;  // every distance is < this: child 0 is taken first, then only a strictly smaller one
    for (int c0 = 0; c0 < nd.nChild; c0 += BOW_CHUNK) {
      uint4 ca[BOW_CHUNK], cb[BOW_CHUNK];
#pragma unroll
      for (int j = 0; j < BOW_CHUNK; j++) {  // every load of the chunk issued before the first distance (clamped: no branch)
        const int idx = nd.first + min(c0 + j, nd.nChild - 1);
        if (idx < a.nStaged) {
          ca[j] = sDesc[2 * idx];
          cb[j] = sDesc[2 * idx + 1];
        } else {
          ca[j] = gDesc[2 * idx];
          cb[j] = gDesc[2 * idx + 1];
        }
      }
#pragma unroll
      for (int j = 0; j < BOW_CHUNK; j++) {
        const uint32_t d = hamming32(qa, qb, ca[j], cb[j]);
        if (c0 + j < nd.nChild && d < bestD) {
          bestD = d;
          best = nd.first + c0 + j;
        }
      }
    }
    if (depth == a.nidLevel) nidNode = best;
    cur = best;
  }
  const size_t o = (size_t)f * a.cap + i;
  a.fin[o] = (uint32_t)cur;
  // a leaf above depth nidLevel leaves the reference's nid uninitialised (UB): the leaf's own node id here
  a.nid[o] = nidNode < 0 ? a.nodes[cur].id : a.nodes[nidNode].id;
}

namespace {

// ascending bitonic sort of keys[0, P) in LDS, P a power of two; every thread of the workgroup takes part
__device__ void bitonicSort(uint64_t* keys, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += BOW_ASSEMBLE_THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t x = keys[i], y = keys[ixj];
          if ((x > y) == ((i & k) == 0)) {
            keys[i] = y;
            keys[ixj] = x;
          }
        }
      }
      __syncthreads();
    }
  }
}

// exclusive prefix sum of one int per thread over the workgroup; *total = the sum (scan: BOW_ASSEMBLE_THREADS ints of LDS)
__device__ int blockExclusiveScan(int v, int* scan, int* total) {
  const int t = threadIdx.x;
  scan[t] = v;
  __syncthreads();
  for (int d = 1; d < BOW_ASSEMBLE_THREADS; d <<= 1) {
    const int add = t >= d ? scan[t - d] : 0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const int incl = scan[t];
  *total = scan[BOW_ASSEMBLE_THREADS - 1];
  __syncthreads();
  return incl - v;
}

}  // namespace

template <int NMAX>
__global__ __launch_bounds__(BOW_ASSEMBLE_THREADS) void k_bow_assemble(BowArgs a) {
  __shared__ uint64_t keys[NMAX];
  __shared__ int scan[BOW_ASSEMBLE_THREADS];
  __shared__ int sCount;
  __shared__ double sNorm;
  const int f = blockIdx.x, t = threadIdx.x;
  const int n = clampN(a.n, f, a.cap);
  const size_t base = (size_t)f * a.cap;
  int P = 1;
  while (P < n) P <<= 1;
  if (t == 0) sCount = 0;
  __syncthreads();
  // (word, feature) keys of the features that are not stopped (weight > 0); the stopped ones sort behind them
  int mine = 0;
  for (int i = t; i < P; i += BOW_ASSEMBLE_THREADS) {
    uint64_t key = ~0ull;
    if (i < n) {
      const BowNode nd = a.nodes[a.fin[base + i]];
      if (a.featWord) a.featWord[base + i] = nd.word;
      if (nd.weight > 0) {
        key = ((uint64_t)nd.word << 32) | (uint32_t)i;
        ++mine;
      }
    }
    keys[i] = key;
  }
  if (mine) atomicAdd(&sCount, mine);
  __syncthreads();
  const int m = a.hasWords ? sCount : 0;  // empty(): both vectors empty (:1083-1086)
  if (m) bitonicSort(keys, P);

  // BowVector: thread t owns the sorted entries [t E, (t + 1) E); a word's entry goes to its rank among the distinct words
  const int E = (m + BOW_ASSEMBLE_THREADS - 1) / BOW_ASSEMBLE_THREADS;
  const int lo = min(t * E, m), hi = min(lo + E, m);
  int heads = 0;
  for (int i = lo; i < hi; i++) heads += i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32);
  int nw = 0;
  int pos = blockExclusiveScan(heads, scan, &nw);
  const bool tf = a.weighting == 0 || a.weighting == 1;
  for (int i = lo; i < hi; i++) {
    const uint32_t w = (uint32_t)(keys[i] >> 32);
    if (i != 0 && (uint32_t)(keys[i - 1] >> 32) == w) continue;
    double v = a.nodes[a.fin[base + (uint32_t)keys[i]]].weight;
    if (tf) {  // addWeight: the first value, then += for every further feature of the word, in feature order
      for (int j = i + 1; j < m && (uint32_t)(keys[j] >> 32) == w; j++) v += a.nodes[a.fin[base + (uint32_t)keys[j]]].weight;
      if (a.norm == 0) v /= (double)nw;  // :1109-1115: divided by the number of WORDS (v.size()), not of features
    }                                    // (IDF / BINARY: addIfNotExist, the first value wins)
    a.bowWord[base + pos] = w;
    a.bowValue[base + pos] = v;
    ++pos;
  }
  if (a.norm != 0 && nw > 0) {
    __syncthreads();  // the values written above are read back by the workgroup (workgroup-scope release / acquire)
    if (t < 64) {     // BowVector::normalize: one ordered f64 chain over the words in ascending order, on the first wave
      double acc = 0.0;
      double x = t < nw ? a.bowValue[base + t] : 0.0;
      for (int b = 0; b < nw; b += 64) {
        const double cur = x;
        if (b + 64 < nw) x = b + 64 + t < nw ? a.bowValue[base + b + 64 + t] : 0.0;  // the next 64 in flight behind the chain
        const int cnt = min(64, nw - b);
        if (a.norm == 1) {
          for (int j = 0; j < cnt; j++) acc += fabs(readlaneF64(cur, j));
        } else {
          for (int j = 0; j < cnt; j++) {
            const double y = readlaneF64(cur, j);
            acc += y * y;
          }
        }
      }
      if (a.norm == 2) acc = sqrt(acc);
      if (t == 0) sNorm = acc;
    }
    __syncthreads();
    const double norm = sNorm;
    if (norm > 0.0)
      for (int j = t; j < nw; j += BOW_ASSEMBLE_THREADS) a.bowValue[base + j] = a.bowValue[base + j] / norm;
  }
  if (t == 0) a.bowN[f] = nw;
  if (!a.fvNode) return;

  // FeatureVector: (node, feature) keys of the same features, sorted
  __syncthreads();
  for (int i = t; i < P; i += BOW_ASSEMBLE_THREADS) {
    uint64_t key = ~0ull;
    if (i < n && m) {
      const BowNode nd = a.nodes[a.fin[base + i]];
      if (nd.weight > 0) key = ((uint64_t)a.nid[base + i] << 32) | (uint32_t)i;
    }
    keys[i] = key;
  }
  __syncthreads();
  if (m) bitonicSort(keys, P);
  for (int i = t; i < m; i += BOW_ASSEMBLE_THREADS) {
    a.fvNode[base + i] = (uint32_t)(keys[i] >> 32);
    a.fvFeat[base + i] = (uint32_t)keys[i];
  }
  if (t == 0) a.fvN[f] = m;
}

__global__ __launch_bounds__(64 * BOW_SCORE_WAVES) void k_bow_score_l1(BowScoreArgs s) {
  const int p = blockIdx.x * BOW_SCORE_WAVES + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (p >= s.nPairs) return;
  const int f1 = s.pairs[p], f2 = s.pairs[s.nPairs + p];
  const int n1 = clampN(s.n, f1, s.cap), n2 = clampN(s.n, f2, s.cap);
  const uint32_t* w1 = s.word + (size_t)f1 * s.cap;
  const uint32_t* w2 = s.word + (size_t)f2 * s.cap;
  const double* v1 = s.value + (size_t)f1 * s.cap;
  const double* v2 = s.value + (size_t)f2 * s.cap;
  double acc = 0.0;
  for (int b = 0; b < n1; b += 64) {
    const int i = b + lane;
    bool found = false;
    double term = 0.0;
    if (i < n1 && n2 > 0) {
      const uint32_t w = w1[i];
      int lo = 0, hi = n2;  // lower_bound of w in v2's ascending words
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (w2[mid] < w) lo = mid + 1;
        else hi = mid;
      }
      if (lo < n2 && w2[lo] == w) {
        const double vi = v1[i], wi = v2[lo];
        term = bowTermL1(vi, wi);
        found = true;
      }
    }
    // the common words' terms, compacted in word order, added one after another (src/ScoringObject.cpp:36-40)
    for (uint64_t mask = __ballot(found); mask; mask &= mask - 1) acc += readlaneF64(term, __builtin_ctzll(mask));
  }
  if (lane == 0) s.score[p] = -acc / 2.0;
}

// the descent alone (vocabulary training: the word of every training feature)
hipError_t launch_bow_descend(hipStream_t st, const BowArgs& a) {
  const long long lanes = (long long)a.nFrames * a.cap;
  hipLaunchKernelGGL(k_bow_descend, dim3((unsigned)((lanes + BOW_DESCEND_THREADS - 1) / BOW_DESCEND_THREADS)),
                     dim3(BOW_DESCEND_THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_bow_transform(hipStream_t st, const BowArgs& a) {
  const long long lanes = (long long)a.nFrames * a.cap;
  hipLaunchKernelGGL(k_bow_descend, dim3((unsigned)((lanes + BOW_DESCEND_THREADS - 1) / BOW_DESCEND_THREADS)),
                     dim3(BOW_DESCEND_THREADS), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.cap <= 4096)
    hipLaunchKernelGGL(k_bow_assemble<4096>, dim3(a.nFrames), dim3(BOW_ASSEMBLE_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL(k_bow_assemble<BOW_MAX_FEATURES>, dim3(a.nFrames), dim3(BOW_ASSEMBLE_THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_bow_score_l1(hipStream_t st, const BowScoreArgs& s) {
  hipLaunchKernelGGL(k_bow_score_l1, dim3((s.nPairs + BOW_SCORE_WAVES - 1) / BOW_SCORE_WAVES), dim3(64 * BOW_SCORE_WAVES), 0, st, s);
  return hipGetLastError();
}

}  // namespace orbx
