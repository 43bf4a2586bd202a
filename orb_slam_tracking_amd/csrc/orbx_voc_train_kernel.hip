// orbx_voc_train_kernel.hip — DBoW2's TemplatedVocabulary<FORB>::create on the device (Thirdparty/DBoW2/include/DBoW2/
// TemplatedVocabulary.h:569-1008, src/FORB.cpp:24-73): hierarchical k-means over 256-bit descriptors, one tree level at a time,
// all nodes of the level in one set of launches (the host side, orbx_voc_train.cpp, walks the levels and builds the tree).
//
// perm[] holds the features (slots of the caller's batch layout) so that every node's features are contiguous and in ascending
// original order; a block table cuts the nodes being split into blocks of VT_THREADS positions.
//
//   k_vt_perm_init    lane per slot              the features of all documents in order (getFeatures, :633-649)
//   k_vt_seed_small   workgroup per node         initiateClustersKMpp (:846-925) with the distances in LDS; the trivial case n <= k
//   k_vt_seed_first / _update / _pick            the same seeding for nodes of any size: per further centre one launch over the
//                                                blocks (distance update, block sums) and one workgroup per node (exact sum, the
//                                                draw, the first position whose running sum reaches it)
//   k_vt_assign       lane per feature           nearest centre, the first among equals (:744-763); a changed association flags the node
//   k_vt_round        lane per node              convergence (:768-784) and the round limit
//   k_vt_count / k_vt_centre_final               FORB::meanValue: thread b owns bit b, LDS counters [k][256] over a chunk of one
//                                                node; nodes of several chunks add them up in global integer counters
//   k_vt_hist / _scan / _scatter                 stable partition of every node's features by cluster (the next level's groups)
//   k_vt_docfreq      workgroup per document     distinct words of the document -> Ni (setNodeWeights, :974-995)
//
// Everything is integer arithmetic except the seeding's cut, one f64 division and product as the reference computes it; integer
// sums do not depend on their order, so the result equals the recursive CPU restatement (tests/cpp/voc_train_ref.cpp) bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orbx_launch.h"

namespace orbx {

namespace {

__device__ __forceinline__ uint64_t vtMix(uint64_t z) {  // the splitmix64 step
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// draw j of the node with this key: 31 bits, as rand() gives (include/orbx.h, training, deviation 1)
__device__ __forceinline__ uint32_t vtDraw(uint64_t seed, uint64_t key, uint32_t j) {
  return (uint32_t)(vtMix(vtMix(seed ^ vtMix(key)) + j) >> 33);
}

__device__ __forceinline__ int vtDist(const uint4& qa, const uint4& qb, const uint32_t* c) {
  return __popc(qa.x ^ c[0]) + __popc(qa.y ^ c[1]) + __popc(qa.z ^ c[2]) + __popc(qa.w ^ c[3]) + __popc(qb.x ^ c[4]) +
         __popc(qb.y ^ c[5]) + __popc(qb.z ^ c[6]) + __popc(qb.w ^ c[7]);
}

__device__ __forceinline__ void vtLoad(const uint32_t* feat, uint32_t slot, uint4* qa, uint4* qb) {
  const uint4* q = reinterpret_cast<const uint4*>(feat + (size_t)slot * 8);
  *qa = q[0];
  *qb = q[1];
}

// exclusive prefix sum over the workgroup's VT_THREADS threads; *total = the sum (scan: VT_THREADS entries of LDS)
template <class T>
__device__ T vtScan(T v, T* scan, T* total) {
  const int t = threadIdx.x;
  scan[t] = v;
  __syncthreads();
  for (int d = 1; d < VT_THREADS; d <<= 1) {
    const T add = t >= d ? scan[t - d] : (T)0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const T incl = scan[t];
  *total = scan[VT_THREADS - 1];
  __syncthreads();
  return incl - v;
}

// the cut of one seeding step: RandomValue<double>(0, dist_sum), drawn again while it is exactly 0 (:899-903)
__device__ double vtCut(uint64_t seed, uint64_t key, int32_t* draws, double sum) {
  double cut;
  do cut = (double)vtDraw(seed, key, (uint32_t)(*draws)++) / 2147483647.0 * sum;
  while (cut == 0.0);
  return cut;
}

}  // namespace

__global__ __launch_bounds__(VT_THREADS) void k_vt_perm_init(const int32_t* n, const int32_t* docOff, int cap, int nDocs, uint32_t* perm) {
  const long long g = (long long)blockIdx.x * VT_THREADS + threadIdx.x;
  const int f = (int)(g / cap), i = (int)(g - (long long)f * cap);
  if (f >= nDocs) return;
  const int v = n[f], cnt = v < 0 ? 0 : (v > cap ? cap : v);
  if (i < cnt) perm[docOff[f] + i] = (uint32_t)g;
}

__global__ __launch_bounds__(VT_THREADS) void k_vt_seed_small(VtArgs a) {
  __shared__ int md[VT_SEED_LDS];
  __shared__ int scan[VT_THREADS];
  __shared__ uint32_t sC[8];
  __shared__ int sIdx;
  __shared__ double sCut;
  const int t = threadIdx.x, ni = a.list[blockIdx.x];
  VtNode* nd = a.nodes + ni;
  const int n = nd->n, start = nd->start;
  uint32_t* cen = a.centres + (size_t)ni * a.k * 8;
  if (n <= a.k) {  // trivial case: one cluster per feature, in order (:672-682)
    for (int j = t; j < n * 8; j += VT_THREADS) cen[j] = a.feat[(size_t)a.perm[start + (j >> 3)] * 8 + (j & 7)];
    if (t < n) a.assoc[start + t] = (uint8_t)t;
    if (t == 0) {
      nd->nC = n;
      nd->state = VT_TRIVIAL;
    }
    return;
  }
  const uint64_t key = nd->key;
  int draws = 0;
  if (t == 0) sIdx = (int)((double)vtDraw(a.seed, key, (uint32_t)draws++) / 2147483648.0 * n);  // RandomInt(0, n - 1)
  __syncthreads();
  int nC = 0;
  const int E = (n + VT_THREADS - 1) / VT_THREADS, lo = min(t * E, n), hi = min(lo + E, n);
  for (;;) {
    const int pick = sIdx;
    if (t < 8) cen[nC * 8 + t] = sC[t] = a.feat[(size_t)a.perm[start + pick] * 8 + t];
    ++nC;
    __syncthreads();
    if (nC == a.k) break;
    // distances to the newest centre: all of them for the first, afterwards only where the kept one is > 0 and larger
    for (int i = t; i < n; i += VT_THREADS) {
      const int old = nC == 1 ? 0x7fffffff : md[i];
      if (old > 0) {
        uint4 qa, qb;
        vtLoad(a.feat, a.perm[start + i], &qa, &qb);
        const int d = vtDist(qa, qb, sC);
        if (d < old) md[i] = d;
      }
    }
    __syncthreads();
    int local = 0, total = 0;
    for (int i = lo; i < hi; i++) local += md[i];
    const int excl = vtScan(local, scan, &total);
    if (total == 0) {  // every feature coincides with a centre: fewer than k clusters (:920-921)
      if (t == 0) atomicAdd(&a.stats[6], 1);
      break;
    }
    if (t == 0) {
      sCut = vtCut(a.seed, key, &draws, (double)total);
      sIdx = n - 1;
    }
    __syncthreads();
    const double cut = sCut;
    if ((double)excl < cut && (double)(excl + local) >= cut) {
      int up = excl;
      for (int i = lo; i < hi; i++) {
        up += md[i];
        if ((double)up >= cut) {
          sIdx = i;
          break;
        }
      }
    }
    __syncthreads();
  }
  if (t == 0) nd->nC = nC;
}

__global__ __launch_bounds__(64) void k_vt_seed_first(VtArgs a) {
  const int t = threadIdx.x, ni = a.list[blockIdx.x];
  VtNode* nd = a.nodes + ni;
  const int first = (int)((double)vtDraw(a.seed, nd->key, 0) / 2147483648.0 * nd->n);
  if (t < 8) a.centres[(size_t)ni * a.k * 8 + t] = a.feat[(size_t)a.perm[nd->start + first] * 8 + t];
  if (t == 0) {
    nd->nC = 1;
    nd->draws = 1;
  }
}

// step c (the centre with ordinal c is chosen next): distances to centre c - 1 and the block's sum
__global__ __launch_bounds__(VT_THREADS) void k_vt_seed_update(VtArgs a, int c) {
  __shared__ uint32_t scan[VT_THREADS];
  const int t = threadIdx.x, b = blockIdx.x, ni = a.blkNode[b];
  const VtNode* nd = a.nodes + ni;
  if (nd->form != 1 || nd->seedDone) return;
  const int p = a.blkStart[b] + t;
  int v = 0;
  if (p < nd->start + nd->n) {
    const int old = c == 1 ? 0x7fffffff : a.minDist[p];
    v = old;
    if (old > 0) {
      uint4 qa, qb;
      vtLoad(a.feat, a.perm[p], &qa, &qb);
      const int d = vtDist(qa, qb, a.centres + ((size_t)ni * a.k + (c - 1)) * 8);
      if (d < old) a.minDist[p] = v = d;
    }
  }
  uint32_t total;
  vtScan((uint32_t)v, scan, &total);
  if (t == 0) a.blkSum[b] = total;
}

__global__ __launch_bounds__(VT_THREADS) void k_vt_seed_pick(VtArgs a, int c) {
  __shared__ uint64_t scan64[VT_THREADS];
  __shared__ uint32_t scan[VT_THREADS];
  __shared__ double sCut;
  __shared__ unsigned long long sUp;
  __shared__ int sBlk, sIdx;
  const int t = threadIdx.x, ni = a.list[blockIdx.x];
  VtNode* nd = a.nodes + ni;
  const int done = nd->seedDone;  // (read by every thread before thread 0 may set it)
  __syncthreads();
  if (done) return;
  const int n = nd->n, start = nd->start, nb = (n + VT_THREADS - 1) / VT_THREADS, b0 = nd->blk0;
  const int E = (nb + VT_THREADS - 1) / VT_THREADS, lo = min(t * E, nb), hi = min(lo + E, nb);
  uint64_t local = 0, total = 0;
  for (int j = lo; j < hi; j++) local += a.blkSum[b0 + j];
  const uint64_t excl = vtScan(local, scan64, &total);
  if (total == 0) {
    if (t == 0) {
      nd->seedDone = 1;
      atomicAdd(&a.stats[6], 1);
    }
    return;
  }
  if (t == 0) {
    int draws = nd->draws;
    sCut = vtCut(a.seed, nd->key, &draws, (double)total);
    nd->draws = draws;
    sBlk = -1;
    sIdx = n - 1;
  }
  __syncthreads();
  const double cut = sCut;
  if ((double)excl < cut && (double)(excl + local) >= cut) {
    uint64_t up = excl;
    for (int j = lo; j < hi; j++) {
      const uint64_t s = a.blkSum[b0 + j];
      if ((double)(up + s) >= cut) {
        sBlk = j;
        sUp = up;
        break;
      }
      up += s;
    }
  }
  __syncthreads();
  const int blk = sBlk;
  if (blk >= 0) {  // the position inside the block
    const int p = a.blkStart[b0 + blk] + t;
    const uint32_t v = p < start + n ? (uint32_t)a.minDist[p] : 0u;
    uint32_t bt;
    const uint32_t ex = vtScan(v, scan, &bt);
    const uint64_t up = sUp;
    if ((double)(up + ex) < cut && (double)(up + ex + v) >= cut) sIdx = p - start;
    __syncthreads();
  }
  const int pick = sIdx;
  if (t < 8) a.centres[((size_t)ni * a.k + c) * 8 + t] = a.feat[(size_t)a.perm[start + pick] * 8 + t];
  if (t == 0) {
    nd->nC = c + 1;
    if (c + 1 == a.k) nd->seedDone = 1;
  }
}

__global__ __launch_bounds__(VT_THREADS) void k_vt_assign(VtArgs a) {
  __shared__ uint32_t sC[VT_KMAX * 8];
  const int t = threadIdx.x, b = blockIdx.x, ni = a.blkNode[b];
  VtNode* nd = a.nodes + ni;
  if (nd->state != VT_RUNNING) return;
  const int nC = nd->nC;
  if (t < nC * 8) sC[t] = a.centres[(size_t)ni * a.k * 8 + t];
  __syncthreads();
  const int p = a.blkStart[b] + t;
  int flag = 0;
  if (p < nd->start + nd->n) {
    uint4 qa, qb;
    vtLoad(a.feat, a.perm[p], &qa, &qb);
    int best = vtDist(qa, qb, sC), ic = 0;
    for (int c = 1; c < nC; c++) {
      const int d = vtDist(qa, qb, sC + c * 8);
      if (d < best) {
        best = d;
        ic = c;
      }
    }
    if (a.assoc[p] != (uint8_t)ic) {
      a.assoc[p] = (uint8_t)ic;
      flag = 1;
    }
  }
  if (__syncthreads_or(flag) && t == 0) atomicOr(&nd->changed, 1);
}

__global__ __launch_bounds__(VT_THREADS) void k_vt_round(VtArgs a) {
  const int ni = blockIdx.x * VT_THREADS + threadIdx.x;
  if (ni >= a.nNodes) return;
  VtNode* nd = a.nodes + ni;
  if (nd->state != VT_RUNNING) return;
  const int rounds = ++nd->rounds;
  if (rounds > 1 && !nd->changed) {
    nd->state = VT_CONVERGED;
  } else if (rounds >= a.maxRounds) {  // deviation 3
    nd->state = VT_CAPPED;
    atomicAdd(&a.stats[4], 1);
  } else {
    nd->changed = 0;
    atomicAdd(&a.stats[8], 1);
    return;
  }
  atomicMax(&a.stats[3], rounds);
}

namespace {

// FORB::meanValue of cluster c from the counts of bit b (thread b) and the group's size; an empty group keeps its centre
__device__ __forceinline__ void vtMean(const VtArgs& a, int ni, int c, uint32_t count, uint32_t size) {
  const int t = threadIdx.x;
  if (size == 0) {  // deviation 2
    if (t == 0) atomicAdd(&a.stats[5], 1);
    return;
  }
  const uint32_t N2 = size / 2 + size % 2;  // (one member: its copy)
  const uint64_t m = __ballot(count >= N2);
  if ((t & 63) == 0) {
    uint32_t* cen = a.centres + ((size_t)ni * a.k + c) * 8 + (t >> 6) * 2;
    cen[0] = (uint32_t)m;
    cen[1] = (uint32_t)(m >> 32);
  }
}

}  // namespace

__global__ __launch_bounds__(VT_THREADS) void k_vt_count(VtArgs a) {
  __shared__ uint32_t cnt[VT_KMAX * VT_THREADS];
  __shared__ uint32_t size[VT_KMAX];
  __shared__ uint4 sW4[VT_THREADS * 2];
  const uint32_t* sW = reinterpret_cast<const uint32_t*>(sW4);
  __shared__ uint8_t cls[VT_THREADS];
  const int t = threadIdx.x, ch = blockIdx.x, ni = a.chNode[ch];
  const VtNode* nd = a.nodes + ni;
  if (nd->state != VT_RUNNING) return;
  const int nC = nd->nC, p0 = a.chStart[ch], p1 = min(p0 + VT_CHUNK, nd->start + nd->n);
  for (int c = 0; c < nC; c++) cnt[c * VT_THREADS + t] = 0;
  if (t < VT_KMAX) size[t] = 0;
  for (int base = p0; base < p1; base += VT_THREADS) {
    __syncthreads();
    const int m = min(VT_THREADS, p1 - base);
    if (t < m) {
      cls[t] = a.assoc[base + t];
      const uint4* q = reinterpret_cast<const uint4*>(a.feat + (size_t)a.perm[base + t] * 8);
      sW4[2 * t] = q[0];
      sW4[2 * t + 1] = q[1];
    }
    __syncthreads();
    for (int i = 0; i < m; i++) {
      const int c = cls[i];
      cnt[c * VT_THREADS + t] += (sW[i * 8 + (t >> 5)] >> (t & 31)) & 1u;
      if (t == 0) size[c]++;
    }
  }
  __syncthreads();
  if (nd->multi < 0) {
    for (int c = 0; c < nC; c++) vtMean(a, ni, c, cnt[c * VT_THREADS + t], size[c]);
  } else {
    uint32_t* g = a.gCnt + (size_t)nd->multi * a.k * (VT_THREADS + 1);
    for (int c = 0; c < nC; c++) {
      const uint32_t v = cnt[c * VT_THREADS + t];
      if (v) atomicAdd(&g[c * (VT_THREADS + 1) + t], v);
      if (t == 0 && size[c]) atomicAdd(&g[c * (VT_THREADS + 1) + VT_THREADS], size[c]);
    }
  }
}

__global__ __launch_bounds__(VT_THREADS) void k_vt_centre_final(VtArgs a) {
  const int t = threadIdx.x, ni = a.list[blockIdx.x];
  const VtNode* nd = a.nodes + ni;
  if (nd->state != VT_RUNNING) return;
  uint32_t* g = a.gCnt + (size_t)nd->multi * a.k * (VT_THREADS + 1);
  for (int c = 0; c < nd->nC; c++) {
    uint32_t* gc = g + c * (VT_THREADS + 1);
    const uint32_t count = gc[t], size = gc[VT_THREADS];
    __syncthreads();  // (every thread has read the size before it is cleared)
    gc[t] = 0;
    if (t == 0) gc[VT_THREADS] = 0;
    vtMean(a, ni, c, count, size);
  }
}

__global__ __launch_bounds__(VT_THREADS) void k_vt_hist(VtArgs a) {
  __shared__ int h[VT_KMAX];
  const int t = threadIdx.x, b = blockIdx.x;
  const VtNode* nd = a.nodes + a.blkNode[b];
  if (t < VT_KMAX) h[t] = 0;
  __syncthreads();
  const int p = a.blkStart[b] + t;
  if (p < nd->start + nd->n) atomicAdd(&h[a.assoc[p]], 1);
  __syncthreads();
  if (t < a.k) a.blkHist[(size_t)b * a.k + t] = h[t];
}

__global__ __launch_bounds__(64) void k_vt_scan(VtArgs a) {
  __shared__ int tot[VT_KMAX];
  const int c = threadIdx.x, ni = blockIdx.x;
  const VtNode* nd = a.nodes + ni;
  const int nb = (nd->n + VT_THREADS - 1) / VT_THREADS;
  if (c < a.k) {
    int run = 0;
    for (int j = 0; j < nb; j++) {
      int* h = a.blkHist + (size_t)(nd->blk0 + j) * a.k + c;
      const int v = *h;
      *h = run;
      run += v;
    }
    tot[c] = run;
    a.nodeHist[(size_t)ni * a.k + c] = run;
  }
  __syncthreads();
  if (c < a.k) {
    int base = nd->start;
    for (int j = 0; j < c; j++) base += tot[j];
    a.childBase[(size_t)ni * a.k + c] = base;
  }
}

__global__ __launch_bounds__(VT_THREADS) void k_vt_scatter(VtArgs a) {
  __shared__ int wc[VT_THREADS / 64][VT_KMAX];
  const int t = threadIdx.x, b = blockIdx.x, ni = a.blkNode[b], w = t >> 6, lane = t & 63;
  const VtNode* nd = a.nodes + ni;
  const int p = a.blkStart[b] + t;
  const bool valid = p < nd->start + nd->n;
  const int mine = valid ? a.assoc[p] : -1;
  int rank = 0;
  for (int c = 0; c < nd->nC; c++) {
    const uint64_t m = __ballot(mine == c);
    if (mine == c) rank = __popcll(m & ((1ull << lane) - 1));
    if (lane == 0) wc[w][c] = __popcll(m);
  }
  __syncthreads();
  if (!valid) return;
  int dst = a.childBase[(size_t)ni * a.k + mine] + a.blkHist[(size_t)b * a.k + mine] + rank;
  for (int j = 0; j < w; j++) dst += wc[j][mine];
  a.permOut[dst] = a.perm[p];
}

// the word every training feature descends to (fin: k_bow_descend's end nodes), and Ni += 1 per distinct word of a document
__global__ __launch_bounds__(VT_DF_THREADS) void k_vt_docfreq(const BowNode* nodes, const uint32_t* fin, const int32_t* n, int cap,
                                                               int P, uint32_t* featWord, uint32_t* Ni) {
  extern __shared__ uint32_t keys[];
  const int f = blockIdx.x, t = threadIdx.x;
  const int v = n[f], cnt = v < 0 ? 0 : (v > cap ? cap : v);
  const size_t base = (size_t)f * cap;
  for (int i = t; i < P; i += VT_DF_THREADS) {
    uint32_t key = 0xffffffffu;
    if (i < cnt) {
      key = nodes[fin[base + i]].word;
      if (featWord) featWord[base + i] = key;
    }
    keys[i] = key;
  }
  __syncthreads();
  if (!Ni) return;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < P; i += VT_DF_THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint32_t x = keys[i], y = keys[ixj];
          if ((x > y) == ((i & k) == 0)) {
            keys[i] = y;
            keys[ixj] = x;
          }
        }
      }
      __syncthreads();
    }
  for (int i = t; i < cnt; i += VT_DF_THREADS)
    if (i == 0 || keys[i] != keys[i - 1]) atomicAdd(&Ni[keys[i]], 1u);
}

// ---- launchers (orbx_voc_train.cpp) ----
#define VT_LAUNCH(kern, grid, block, ...)                                   \
  do {                                                                      \
    if ((grid) > 0) hipLaunchKernelGGL(kern, dim3((unsigned)(grid)), dim3(block), 0, st, __VA_ARGS__); \
    return hipGetLastError();                                               \
  } while (0)

hipError_t vtLaunchPermInit(hipStream_t st, const int32_t* n, const int32_t* docOff, int cap, int nDocs, uint32_t* perm) {
  VT_LAUNCH(k_vt_perm_init, ((long long)nDocs * cap + VT_THREADS - 1) / VT_THREADS, VT_THREADS, n, docOff, cap, nDocs, perm);
}
hipError_t vtLaunchSeedSmall(hipStream_t st, const VtArgs& a) { VT_LAUNCH(k_vt_seed_small, a.nList, VT_THREADS, a); }
hipError_t vtLaunchSeedFirst(hipStream_t st, const VtArgs& a) { VT_LAUNCH(k_vt_seed_first, a.nList, 64, a); }
hipError_t vtLaunchSeedUpdate(hipStream_t st, const VtArgs& a, int c) { VT_LAUNCH(k_vt_seed_update, a.nBlk, VT_THREADS, a, c); }
hipError_t vtLaunchSeedPick(hipStream_t st, const VtArgs& a, int c) { VT_LAUNCH(k_vt_seed_pick, a.nList, VT_THREADS, a, c); }
hipError_t vtLaunchAssign(hipStream_t st, const VtArgs& a) { VT_LAUNCH(k_vt_assign, a.nBlk, VT_THREADS, a); }
hipError_t vtLaunchRound(hipStream_t st, const VtArgs& a) { VT_LAUNCH(k_vt_round, (a.nNodes + VT_THREADS - 1) / VT_THREADS, VT_THREADS, a); }
hipError_t vtLaunchCount(hipStream_t st, const VtArgs& a) { VT_LAUNCH(k_vt_count, a.nChunk, VT_THREADS, a); }
hipError_t vtLaunchCentreFinal(hipStream_t st, const VtArgs& a) { VT_LAUNCH(k_vt_centre_final, a.nList, VT_THREADS, a); }
hipError_t vtLaunchHist(hipStream_t st, const VtArgs& a) { VT_LAUNCH(k_vt_hist, a.nBlk, VT_THREADS, a); }
hipError_t vtLaunchScan(hipStream_t st, const VtArgs& a) { VT_LAUNCH(k_vt_scan, a.nNodes, 64, a); }
hipError_t vtLaunchScatter(hipStream_t st, const VtArgs& a) { VT_LAUNCH(k_vt_scatter, a.nBlk, VT_THREADS, a); }
hipError_t vtLaunchDocFreq(hipStream_t st, const BowNode* nodes, const uint32_t* fin, const int32_t* n, int cap, int nDocs,
                           uint32_t* featWord, uint32_t* Ni) {
  int P = 1;
  while (P < cap) P <<= 1;
  if (nDocs > 0) hipLaunchKernelGGL(k_vt_docfreq, dim3(nDocs), dim3(VT_DF_THREADS), (size_t)P * 4, st, nodes, fin, n, cap, P, featWord, Ni);
  return hipGetLastError();
}

}  // namespace orbx
