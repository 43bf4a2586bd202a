// orbx_octree_body.inc — device code of the quadtree selection (see orbx_octree_kernel.hip), written against the
// workgroup size OCT_T and included once per size: 256 threads for the LDS-resident kernel, 1024 threads for the units
// whose arrays live in global scratch (there the work is bound by memory latency, and four times the waves hide four
// times as much of it).  No include guard on purpose.
// IDX = type of a sorted-key position (0 .. n): int for the global-scratch units (n < 2^19), uint16_t in the LDS kernel
// (n <= 2048), where the node records and hiOf[] then take half the space
// KEY = type of a sort key: u64 = (16-level path code << 24) | candidate index; uint32_t (LDS kernel, n <= 2048, levels whose
// cells shrink to one pixel within D = depthBits splits with rootBits + 2 D <= 21) = (the code's top rootBits + 2 D bits << 11) |
// candidate index -- the digits beyond depth D are all 0 (a one-pixel cell sends its key to quadrant 0 for ever), so nothing
// is lost, and 2048 keys take 8 KB instead of 16 (the 2048-candidate unit fits 32 KB: five per CU instead of four)
// REGC (LDS kernel: NMAX / OCT_T; 0 = off) = candidate words a thread keeps in REGISTERS from step 1 to step 6, where they are
// exchanged through LDS (nodes[]'s space, dead by then): the unit then never stores or gathers them through global memory -- with
// every unit of a launch writing its candE at once that round trip cost 25 k cycles of the 166 k a level-0 unit takes under load
template <class IDX, class KEY = u64, int REGC = 0>
struct OctScratchT {
  static constexpr int kRegCand = REGC;
  KEY* keys;          // [nPad]   sort keys (see KEY), sorted ascending
  int keyShift;       //          2 * (16 - D): the keys carry the top rootBits + 2 D bits of the path code (the digits beyond D are
                      //          0; the global units' radix sort gets by with three 9-bit passes instead of four at 1080p / 4K)
  u64* nodes;         // [mPad]   (17 - blockDepth) << 59 | orderKey << 19 | lo, sorted ascending = std::list order
  uint8_t* div;       // [n + 1]  divergence depth between sorted neighbours (255 at both ends = "separated"); the first depth
                      //          at which key i is the only key of its node is max(div[i], div[i + 1]) (octAlone)
  IDX* hiOf;          // [n]      end of the node that starts at sorted position lo
  IDX* nodeLo;        // [mCap + fCap]  node records: list nodes first, then the nodes pushed during the partial pass
  IDX* nodeHi;
  uint8_t* nodeDepth;  // depth of the node (0 .. 17); bit 7 set = the node has been split (no longer in the list)
  u64* sized;         // [2 * qCap]  count << 40 | UL.x << 20 | node, two buffers (partitioned / stably sorted)
  int* pending;       // [2 * qCap]  two buffers
  int* childCnt;      // [qCap]      per sorted entry: children | multi-key children << 8
  const uint32_t* cand;     // [n] positions of the unit's candidates inside its candidate area (gatherCandidates); only step 1
                            // reads it, so in the LDS kernel it shares its space with nodes[]
  const uint32_t* segBase;  // the unit's candidate area: cell c's survivors at segBase + c * segCap
  u64* xchg;          // LDS exchange buffer for the register sort when keys/nodes live in global memory, else nullptr
  int xchgCap;        // its capacity in keys (>= 1024): larger arrays are sorted in global memory (radix sort / in-memory bitonic)
  uint32_t* parScr;   // OCT_PAR_SCR_FOR(parCap) dwords of LDS that are free during the partial pass (parallel std::sort replay)
  int parCap;         // largest array the parallel replay may take there (512 or 256 keys); larger ones use the one-lane replay
  u64* sortTmp;       // [n] second key buffer of the radix sort (global-scratch units only, else nullptr); afterwards free, and
                      //     reused by the partial pass's stable sort
  uint32_t* candE;    // [n] the candidate words in candidate-list order, in GLOBAL scratch (written by step 1; the global-scratch
                      //     units write it over the position list they have just read, the LDS kernel into the head of the unit's
                      //     scratch area): the sort keys carry the candidate's INDEX, and step 6 gathers from this compact array
  uint32_t* ceBuf;    // [n] the candidates in sorted-key order, filled and read by step 6 only (LDS kernel: nodes[]'s space, dead
                      //     by then; global-scratch units: sortTmp's space)
  uint32_t* radixCnt2 = nullptr;  // k_octree_global: a second set of radix counters (512 x waves dwords of LDS): a pass's scatter
                      //     counts the next pass's digits on the way
  // k_octree_big only (LDS): the list nodes by creation index -- lo | (hi - lo) << 19 and UL.x -- and the pending nodes' records
  uint32_t* nodeLH = nullptr;  // [OCTBIG_NODES]
  uint16_t* nodeUlx = nullptr; // [OCTBIG_NODES]
  int* pNd = nullptr;          // [OCTBIG_PEND] node id
  int* pLo = nullptr;          // [OCTBIG_PEND]
  int* pHiD = nullptr;         // [OCTBIG_PEND] hi << 5 | depth
  uint16_t* pUlx = nullptr;    // [OCTBIG_PEND]
};
using OctScratch = OctScratchT<int>;
// path code (16-level layout) and candidate index of sorted key i
template <class SCR>
__device__ __forceinline__ u64 keyCode(const SCR& S, int i) {
  if constexpr (sizeof(*S.keys) == 4) return (u64)(S.keys[i] >> 11) << S.keyShift;
  else return (S.keys[i] >> 24) << S.keyShift;
}
template <class SCR>
__device__ __forceinline__ uint32_t keyIndex(const SCR& S, int i) {
  if constexpr (sizeof(*S.keys) == 4) return S.keys[i] & 2047u;
  else return (uint32_t)(S.keys[i] & 0xffffff);
}
// first depth at which sorted key i is the only key of its node
__device__ __forceinline__ int octAlone(const uint8_t* div, int i) {
  const int dl = div[i] == 255 ? -1 : (int)div[i], dr = div[i + 1] == 255 ? -1 : (int)div[i + 1];
  return max(max(dl, dr), 0);
}

__device__ __forceinline__ int divDepth(u64 a, u64 b) {  // first depth at which two path codes differ
  const u64 x = a ^ b;
  if (!x) return OCT_DEPTH + 1;
  const int hb = 63 - __builtin_clzll(x);
  return hb >= 2 * OCT_DEPTH ? 0 : OCT_DEPTH - hb / 2;
}

// bitonic sort in memory, one barrier per stage: only for arrays too large for the register version below
template <class T>
__device__ __forceinline__ void bitonicSortMem(T* a, int nPow2, int tid) {
  for (int k = 2; k <= nPow2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < nPow2; i += OCT_T) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const T x = a[i], y = a[ixj];
          const bool asc = (i & k) == 0;
          if ((x > y) == asc) { a[i] = y; a[ixj] = x; }
        }
      }
      __syncthreads();
    }
}

// the value of lane (l ^ LM), LM a power of two: one DPP lane select where one exists (quad_perm for 1 and 2, row_ror:8 for 8),
// ds_bpermute for 4, 16 and 32.  (Round 4 measured the all-VALU form -- two bank-masked row shifts for 4, gfx950's
// v_permlane16_swap / v_permlane32_swap + v_cndmask for 16 / 32: correct, and slower -- key sort 16.5 k -> 22.2 k cycles, node
// sort 5.7 k -> 15.8 k: a lone wave issues eight independent ds_bpermute back to back and the LDS crossbar works beside the VALU.)
template <int LM>
__device__ __forceinline__ uint32_t laneXorT(uint32_t v) {
  if constexpr (LM == 1) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false);
  else if constexpr (LM == 2) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false);
  else if constexpr (LM == 8) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xf, 0xf, false);
  else return __shfl_xor(v, LM);
}
template <int LM>
__device__ __forceinline__ u64 laneXorT(u64 v) {
  return ((u64)laneXorT<LM>((uint32_t)(v >> 32)) << 32) | laneXorT<LM>((uint32_t)v);
}
// one compare-exchange stage of the register bitonic sorts at lane distance LM (element distance j = LM * E, merge size k)
template <int LM, int E, class T>
__device__ __forceinline__ void bitonicLaneStage(T (&v)[E], int tid, int j, int k) {
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int i = tid * E + e;
    const T o = laneXorT<LM>(v[e]);
    const bool lower = (i & j) == 0, asc = (i & k) == 0;
    const bool keepMin = lower == asc;
    v[e] = keepMin ? (o < v[e] ? o : v[e]) : (o > v[e] ? o : v[e]);
  }
}
// the lane stages of one bitonic merge of size k, from the largest lane distance the merge has (k / 2 E, at most 32) down to 1:
// straight-line code with one uniform guard per distance (a switch per stage cost more in scalar branches than the stages' work)
template <int E, class T>
__device__ __forceinline__ void bitonicLaneStages(T (&v)[E], int tid, int k) {
  if (k >= 64 * E) bitonicLaneStage<32>(v, tid, 32 * E, k);
  if (k >= 32 * E) bitonicLaneStage<16>(v, tid, 16 * E, k);
  if (k >= 16 * E) bitonicLaneStage<8>(v, tid, 8 * E, k);
  if (k >= 8 * E) bitonicLaneStage<4>(v, tid, 4 * E, k);
  if (k >= 4 * E) bitonicLaneStage<2>(v, tid, 2 * E, k);
  if (k >= 2 * E) bitonicLaneStage<1>(v, tid, E, k);
}

// Bitonic sort of OCT_T*E keys held E per thread (thread t owns elements t*E .. t*E+E-1).  Compare-exchange partners at
// distance < E are registers of the same thread, at distance < 64*E lanes of the same wave (shuffles), and only the
// last stages (distance >= 64*E, three of them) go through memory with a barrier.
template <int E, class T>
__device__ __forceinline__ void bitonicSortRegs(T* a, int tid) {
  constexpr int NTOT = OCT_T * E;
  T v[E];
#pragma unroll
  for (int e = 0; e < E; e++) v[e] = a[tid * E + e];
  for (int k = 2; k <= NTOT; k <<= 1) {
    for (int j = k >> 1; j >= 64 * E; j >>= 1) {  // partner in another wave
      __syncthreads();
#pragma unroll
      for (int e = 0; e < E; e++) a[tid * E + e] = v[e];
      __syncthreads();
#pragma unroll
      for (int e = 0; e < E; e++) {
        const int i = tid * E + e;
        const T o = a[i ^ j];
        const bool lower = (i & j) == 0, asc = (i & k) == 0;
        const bool keepMin = lower == asc;
        v[e] = keepMin ? (o < v[e] ? o : v[e]) : (o > v[e] ? o : v[e]);
      }
    }
    bitonicLaneStages<E>(v, tid, k);  // partner lanes of the same wave
    // partner register of the same thread: distances E/2 .. 1 (compile-time, so v[] stays in registers)
#pragma unroll
    for (int jj = E / 2; jj > 0; jj >>= 1) {
      if (jj < k) {
#pragma unroll
        for (int e = 0; e < E; e++) {
          const int pe = e ^ jj;
          if (pe > e) {
            const bool asc = ((tid * E + e) & k) == 0;
            const T x = v[e], y = v[pe];
            const bool sw = (x > y) == asc;
            v[e] = sw ? y : x;
            v[pe] = sw ? x : y;
          }
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < E; e++) a[tid * E + e] = v[e];
  __syncthreads();
}

// sorts a[0 .. nPow2) ascending; entries beyond the real data must be padded with ~0 up to max(nPow2, OCT_T).
// `xchg`: LDS buffer of xchgCap (<= OCT_SORT_LDS) keys used when `a` itself is not in LDS (the register sort exchanges its
// last stages through LDS only); arrays larger than that are sorted in place, one barrier per stage.
template <class T>
__device__ __forceinline__ void bitonicSort(T* a, int nPow2, int tid, T* xchg, int xchgCap) {
  if (nPow2 > (xchg ? min(xchgCap, OCT_SORT_LDS) : OCT_SORT_LDS)) {
    bitonicSortMem(a, nPow2, tid);
    return;
  }
  const int np = nPow2 < OCT_T ? OCT_T : nPow2;
  T* s = a;
  if (xchg) {
    for (int i = tid; i < np; i += OCT_T) xchg[i] = a[i];
    __syncthreads();
    s = xchg;
  }
  static_assert(OCT_T < 256 || (OCT_SORT_LDS / OCT_T >= 1 && OCT_SORT_LDS / OCT_T <= 8), "elements per thread of the register sort");  // (the single-wave instance calls bitonicSortRegs itself)
  const int e = np / OCT_T;  // elements per thread: 1 .. OCT_SORT_LDS / OCT_T
  if (e == 1) bitonicSortRegs<1>(s, tid);
  else if (e == 2) bitonicSortRegs<2>(s, tid);
  else if (OCT_SORT_LDS / OCT_T >= 4 && e == 4) bitonicSortRegs<(OCT_SORT_LDS / OCT_T >= 4 ? 4 : 1)>(s, tid);
  else if (OCT_SORT_LDS / OCT_T >= 8) bitonicSortRegs<(OCT_SORT_LDS / OCT_T >= 8 ? 8 : 1)>(s, tid);
  if (xchg) {
    for (int i = tid; i < np; i += OCT_T) a[i] = xchg[i];
    __syncthreads();
  }
}

// inclusive prefix sum of v over the wave (lane 63 holds the wave's sum): six DPP adds -- row_shr 1 / 2 / 4 / 8 inside the rows
// of 16 lanes, then row_bcast 15 (rows 1 and 3 take the total of the row before them) and row_bcast 31 (rows 2 and 3 take the
// total of rows 0 + 1) -- instead of six ds_bpermute round trips
__device__ __forceinline__ int waveScanIncl(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}
__device__ __forceinline__ int waveSumLane63(int v) { return waveScanIncl(v); }
// maximum of v (>= 0) over the wave, valid in lane 63 (the same six DPP steps)
__device__ __forceinline__ int waveMaxLane63(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));
  return v;
}

// exclusive prefix sum of one int per thread over the workgroup; *total = sum.  `ws` = 4 ints of LDS.
// lead = false: the caller has passed a workgroup barrier since the previous scan read ws
__device__ __forceinline__ int blockScanExcl(int v, int tid, int* ws, int* total, bool lead = true) {
  const int lane = tid & 63, wave = tid >> 6;
  const int inc = waveScanIncl(v);
  if (lead) __syncthreads();  // ws may still be read from a previous call
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < OCT_T / 64; w++) {
    const int s = ws[w];
    if (w < wave) base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

// Stable LSD radix sort of a[0 .. n) by the path code (bits 24 .. 24 + codeBits of the key), W = 8 or 9 bits per pass, for the
// units whose keys live in global memory (more than OCT_SORT_LDS candidates: the in-memory bitonic network needs
// log2(n)^2 / 2 barrier-separated sweeps, 120 at n = 32768).  The keys arrive ordered by their low 24 bits (the candidate
// index), so a stable sort by the code alone yields the full key order.
// Wave w owns the contiguous block [w * chunk, (w + 1) * chunk) and walks it 64 keys at a time (coalesced): the count
// sweep adds into cnt[digit][w]; the 2^W x nWaves counters are scanned digit-major; the scatter sweep ranks the 64 keys of
// a step among the equal digits below them with W ballots, so the order inside a digit is the array order; its keys are
// loaded a group of four steps ahead (one step ahead left the wave waiting for every load: 71 k cycles per pass at 50 k keys).
// A pass in which every key has the same digit is skipped.  `cnt` = 2^W * OCT_T / 64 dwords of LDS (9-bit digits -- four
// passes instead of five over the 33 code bits of a 16:9 level -- where the caller's exchange buffer holds 512 x nWaves
// counters), `ws` = OCT_T / 64 ints of LDS, b = second buffer of n keys.  Result in a.
// With a second counter array (cnt2) the scatter sweep of a pass also counts the next pass's digits -- the key's destination tells
// which wave will own it then -- so only the first pass walks the keys twice (4 sweeps instead of 6 at three passes).
template <int W>
__device__ __forceinline__ void radixSortCodes(u64* a, u64* b, int n, int tid, uint32_t* cnt, int* ws, int codeBits,
                                               uint32_t* cnt2 = nullptr) {
  constexpr int NW = OCT_T / 64;
  constexpr int ND = 1 << W;
  constexpr int PER = ND * NW / OCT_T;  // counters per thread in the scan
  static_assert(PER >= 1 && PER * OCT_T == ND * NW, "counters per thread");
  const int lane = tid & 63, wave = tid >> 6;
  const int chunk = ((n + NW - 1) / NW + 63) & ~63;
  const int lo = min(wave * chunk, n), hi = min(lo + chunk, n);
  const unsigned long long below = (1ull << lane) - 1ull;
  u64* src = a;
  u64* dst = b;
  bool counted = false;  // cnt holds this pass's counts already (the previous pass's scatter made them)
  for (int shift = 24; shift < 24 + codeBits; shift += W) {
    if (!counted) {
      for (int i = tid; i < ND * NW; i += OCT_T) cnt[i] = 0;
      __syncthreads();
      const int d0 = (int)((src[0] >> shift) & (ND - 1));
      bool same = true;
      for (int i = lo + lane; i < hi; i += 256) {  // four loads in flight
        u64 kk[4];
#pragma unroll
        for (int j = 0; j < 4; j++) kk[j] = (i + 64 * j) < hi ? src[i + 64 * j] : 0ull;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (i + 64 * j >= hi) break;
          const int d = (int)((kk[j] >> shift) & (ND - 1));
          same &= d == d0;
          atomicAdd(&cnt[d * NW + wave], 1u);
        }
      }
      if (__syncthreads_and(same ? 1 : 0)) continue;  // (also the barrier after the counting)
    }
    const bool fuse = cnt2 != nullptr && shift + W < 24 + codeBits;  // (uniform) count the next pass's digits while scattering
    if (fuse)
      for (int i = tid; i < ND * NW; i += OCT_T) cnt2[i] = 0;  // (its last readers left at the barrier that ended the previous pass)
    // exclusive scan of the counters in (digit, wave) order: thread t owns entries [PER t, PER t + PER)
    uint32_t loc[PER];
    int sum = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) { loc[k] = cnt[PER * tid + k]; sum += (int)loc[k]; }
    int total;
    uint32_t run = (uint32_t)blockScanExcl(sum, tid, ws, &total);
#pragma unroll
    for (int k = 0; k < PER; k++) { cnt[PER * tid + k] = run; run += loc[k]; }
    __syncthreads();
    // G = steps per group: four in the 1024-thread instance; one in the 256-thread instance, which only runs as the LDS
    // kernels' rare in-workgroup fallback and must not raise their register count (73 VGPRs)
    constexpr int G = OCT_T >= 1024 ? 4 : 1;
    u64 nxt[G];
#pragma unroll
    for (int j = 0; j < G; j++) nxt[j] = (lo + 64 * j + lane) < hi ? src[lo + 64 * j + lane] : 0ull;
    for (int g0 = lo; g0 < hi; g0 += 64 * G) {  // wave-uniform trip count; the next group's keys are in flight while this one is placed
      u64 cur[G];
#pragma unroll
      for (int j = 0; j < G; j++) cur[j] = nxt[j];
#pragma unroll
      for (int j = 0; j < G; j++) nxt[j] = (g0 + 64 * G + 64 * j + lane) < hi ? src[g0 + 64 * G + 64 * j + lane] : 0ull;
#pragma unroll
      for (int j = 0; j < G; j++) {
        const int i0 = g0 + 64 * j;
        if (i0 >= hi) break;  // (uniform)
        const bool valid = i0 + lane < hi;
        const u64 key = cur[j];
        const int d = (int)((key >> shift) & (ND - 1));
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < W; bit++) {
          const unsigned long long bb = __ballot((d >> bit) & 1);
          m &= ((d >> bit) & 1) ? bb : ~bb;
        }
        // m = the valid lanes with my digit
        if (valid) {
          const uint32_t base = cnt[d * NW + wave];
          const uint32_t pos = base + (uint32_t)__popcll(m & below);
          dst[pos] = key;
          if ((m & below) == 0ull) cnt[d * NW + wave] = base + (uint32_t)__popcll(m);  // lowest lane of the digit
          if (fuse) atomicAdd(&cnt2[(int)((key >> (shift + W)) & (ND - 1)) * NW + (int)(pos / (uint32_t)chunk)], 1u);
        }
      }
    }
    __syncthreads();
    u64* t2 = src; src = dst; dst = t2;
    counted = fuse;
    if (fuse) { uint32_t* t3 = cnt; cnt = cnt2; cnt2 = t3; }
  }
  if (src != a) {
    for (int i = tid; i < n; i += OCT_T) a[i] = src[i];
    __syncthreads();
  }
}

// ---- literal replay of the PARTITION PHASE of libstdc++'s std::sort (bits/stl_algo.h: __introsort_loop) on packed
//      keys; the comparator (compareNodes: count, then UL.x) is "a >> 20 < b >> 20" -----------------------------------

// key array accessor for the replay (LDS or global memory)
struct MemKeys {
  u64* p;
  __device__ __forceinline__ u64 get(int i) const { return p[i]; }
  __device__ __forceinline__ void set(int i, u64 v) { p[i] = v; }
};
template <class A>
__device__ __forceinline__ void stdAdjustHeap(A& p, int first, int holeIndex, int len, u64 value) {
  const int topIndex = holeIndex;
  int secondChild = holeIndex;
  while (secondChild < (len - 1) / 2) {
    secondChild = 2 * (secondChild + 1);
    if (SLESS(p.get(first + secondChild), p.get(first + (secondChild - 1)))) secondChild--;
    p.set(first + holeIndex, p.get(first + secondChild));
    holeIndex = secondChild;
  }
  if ((len & 1) == 0 && secondChild == (len - 2) / 2) {
    secondChild = 2 * (secondChild + 1);
    p.set(first + holeIndex, p.get(first + (secondChild - 1)));
    holeIndex = secondChild - 1;
  }
  int parent = (holeIndex - 1) / 2;  // __push_heap
  while (holeIndex > topIndex && SLESS(p.get(first + parent), value)) {
    p.set(first + holeIndex, p.get(first + parent));
    holeIndex = parent;
    parent = (holeIndex - 1) / 2;
  }
  p.set(first + holeIndex, value);
}

template <class A>
__device__ __forceinline__ void stdHeapSortRange(A& p, int first, int last) {  // __partial_sort(first, last, last)
  const int len = last - first;
  if (len >= 2) {  // __make_heap
    int parent = (len - 2) / 2;
    for (;;) {
      stdAdjustHeap(p, first, parent, len, p.get(first + parent));
      if (parent == 0) break;
      parent--;
    }
  }
  int l = last;  // __sort_heap
  while (l - first > 1) {
    --l;
    const u64 v = p.get(l);  // __pop_heap(first, l, l)
    p.set(l, p.get(first));
    stdAdjustHeap(p, first, 0, l - first, v);
  }
}

template <class A>
__device__ __forceinline__ void stdIntrosortLoop(A& p, int n, u64* stack /* LDS, >= 40 entries: at most 2*log2(n) <= 38 pending ranges */) {
  if (n <= 16) return;
  int sp = 0, first = 0, last = n;
  int depth = 2 * (31 - __builtin_clz((unsigned)n));
  for (;;) {
    while (last - first > 16) {
      if (depth == 0) { stdHeapSortRange(p, first, last); break; }
      --depth;
      const int mid = first + (last - first) / 2;
      {  // __move_median_to_first(first, first + 1, mid, last - 1)
        const int ia = first + 1, ib = mid, ic = last - 1;
        const u64 a = p.get(ia), b = p.get(ib), c = p.get(ic), f = p.get(first);
        int sel;
        if (SLESS(a, b)) sel = SLESS(b, c) ? ib : (SLESS(a, c) ? ic : ia);
        else sel = SLESS(a, c) ? ia : (SLESS(b, c) ? ic : ib);
        p.set(first, p.get(sel));
        p.set(sel, f);
      }
      const u64 pivot = p.get(first);
      int lo = first + 1, hi = last;
      for (;;) {  // __unguarded_partition(first + 1, last, first)
        u64 vlo = p.get(lo);
        while (SLESS(vlo, pivot)) vlo = p.get(++lo);
        --hi;
        u64 vhi = p.get(hi);
        while (SLESS(pivot, vhi)) vhi = p.get(--hi);
        if (!(lo < hi)) break;
        p.set(lo, vhi);
        p.set(hi, vlo);
        ++lo;
      }
      // the library recurses on [cut, last) and loops on [first, cut): disjoint ranges, same depth budget
      stack[sp++] = (u64)first | ((u64)lo << 20) | ((u64)depth << 40);  // private arrays would live in (slow) scratch memory
      first = lo;
    }
    if (sp == 0) break;
    const u64 top = stack[--sp];
    first = (int)(top & 0xfffff); last = (int)((top >> 20) & 0xfffff); depth = (int)(top >> 40);
  }
}

// partition phase of std::sort on p[0..n), replayed by one lane (a register-resident variant read through v_readlane
// was measured slower: a lone wave spends ~100 cycles per serial step either way).  Call with the whole workgroup.
__device__ __forceinline__ void stdSortPartitionPhase(u64* p, int n, int tid) {
  __shared__ u64 sortStack[40];
  if (n <= 16 || tid != 0) return;
  MemKeys A{p};
  stdIntrosortLoop(A, n, sortStack);
}

// (orders a wave's own LDS traffic: DS operations of a wave execute in program order, so what its lanes wrote is what its lanes
// read behind this point -- no workgroup barrier)
#define OCT_WAVE_SYNC()                                         \
  do {                                                          \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      \
    __builtin_amdgcn_wave_barrier();                            \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");      \
  } while (0)

// The partition phase of ONE range p[base, end) of at most 128 keys, replayed by ONE wave: the recursion levels of
// stdSortPartitionPhasePar below (same closed form, same arrays) with lane t holding the positions base + 2 t and base + 2 t + 1,
// the prefix sums by one DPP wave scan, its prefix words in a wave-private array (SLRw: 129 dwords) and no workgroup barrier --
// a level costs a wave ~1.5 k cycles instead of the ~4-7 k of a barrier-separated level of the whole workgroup, and the waves
// work on different ranges.  LR is the workgroup's array: a range only touches its own positions' entries (and reads, without using
// it, the entry of the position behind its end).  `depth` = what is left of the introsort depth budget.  writeRanges: leave
// every position's final range (first | last << 16) in LR[position] for the caller's rank step.  Call with the whole wave.
__device__ __forceinline__ void stdSortPartitionWaveTask(u64* p, int base, int end, int depth, int lane, uint32_t* LR, uint32_t* SLRw,
                                                         bool writeRanges) {
  uint16_t* LR16 = reinterpret_cast<uint16_t*>(LR);
  MemKeys A{p};
  const int pos[2] = {base + 2 * lane, base + 2 * lane + 1};
  int f[2] = {base, base}, l[2] = {end, end};
  for (;;) {
    bool act[2];
#pragma unroll
    for (int j = 0; j < 2; j++) act[j] = pos[j] < end && (l[j] - f[j] > 16);
    if (__ballot(act[0] || act[1]) == 0ull) break;
    if (depth == 0) {
      const int own = (act[0] && pos[0] == f[0]) ? 0 : ((act[1] && pos[1] == f[1]) ? 1 : -1);
      if (own >= 0) stdHeapSortRange(A, own ? f[1] : f[0], own ? l[1] : l[0]);
      break;
    }
    --depth;
    // ---- owners: __move_median_to_first(first, first + 1, mid, last - 1) ----
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (act[j] && pos[j] == f[j]) {
        const int first = f[j], last = l[j];
        const int ia = first + 1, ib = first + (last - first) / 2, ic = last - 1;
        const u64 a = p[ia], b = p[ib], c = p[ic], fv = p[first];
        int sel;
        if (SLESS(a, b)) sel = SLESS(b, c) ? ib : (SLESS(a, c) ? ic : ia);
        else sel = SLESS(a, c) ? ia : (SLESS(b, c) ? ic : ib);
        p[first] = sel == ia ? a : (sel == ib ? b : c);
        p[sel] = fv;
      }
    OCT_WAVE_SYNC();
    // ---- stop flags and their prefixes ----
    int gl[2] = {0, 0}, ll[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (act[j] && pos[j] > f[j]) {
        const u64 v = p[pos[j]], pv = p[f[j]];
        gl[j] = !SLESS(v, pv);
        ll[j] = !SLESS(pv, v);
      }
    const int w0 = gl[0] | (ll[0] << 16), wsum = w0 + (gl[1] | (ll[1] << 16));
    const int inc = waveScanIncl(wsum);
    const int tot = __builtin_amdgcn_readlane(inc, 63);
    if (tot == 0) break;
    const uint32_t e[2] = {(uint32_t)(inc - wsum), (uint32_t)(inc - wsum + w0)};
    *reinterpret_cast<uint2*>(&SLRw[2 * lane]) = make_uint2(e[0], e[1]);
    if (lane == 63) SLRw[128] = (uint32_t)tot;
    OCT_WAVE_SYNC();
    // ---- scatter the stop positions by rank ----
    int nL[2] = {0, 0}, nR[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (act[j] && pos[j] > f[j]) {
        const uint32_t bb = SLRw[f[j] + 1 - base], be = SLRw[l[j] - base], bi = e[j];
        const int bL = (int)(bb & 0xffff), bR = (int)(bb >> 16);
        nL[j] = (int)(be & 0xffff) - bL;
        nR[j] = (int)(be >> 16) - bR;
        if (gl[j]) LR16[2 * (f[j] + 1 + ((int)(bi & 0xffff) - bL))] = (uint16_t)pos[j];
        if (ll[j]) LR16[2 * (f[j] + 1 + (nR[j] - 1 - ((int)(bi >> 16) - bR))) + 1] = (uint16_t)pos[j];
      }
    OCT_WAVE_SYNC();
    // ---- the swaps and the cut ----
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (act[j] && pos[j] > f[j]) {
        const int i = pos[j], k = i - (f[j] + 1), m = min(nL[j], nR[j]);
        const uint32_t lr0 = LR[i], lr1 = LR[i + 1];
        int a = 4096, b = -1;
        bool sw = false, nextSw = false;
        if (k < m) {
          a = (int)(lr0 & 0xffff); b = (int)(lr0 >> 16);
          sw = a < b;
          if (sw && k + 1 < m) nextSw = (int)(lr1 & 0xffff) < (int)(lr1 >> 16);
        }
        int cut = -1;
        if (sw && !nextSw) cut = min(k + 1 < nL[j] ? (int)(lr1 & 0xffff) : 4096, b);
        if (!sw && k == 0) cut = nL[j] > 0 ? (int)(lr0 & 0xffff) : 4096;
        if (sw) {
          const u64 va = p[a], vb = p[b];
          p[a] = vb;
          p[b] = va;
        }
        if (cut >= 0) LR16[2 * f[j]] = (uint16_t)cut;
      }
    OCT_WAVE_SYNC();
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (act[j]) {
        const int c = (int)(LR[f[j]] & 0xffff);
        if (pos[j] < c) l[j] = c; else f[j] = c;
      }
    OCT_WAVE_SYNC();  // (LR[first] has been read before the next level's rank slots overwrite it)
  }
  if (writeRanges) {
    OCT_WAVE_SYNC();
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (pos[j] < end) LR[pos[j]] = (uint32_t)f[j] | ((uint32_t)l[j] << 16);
  }
}

// The same partition phase with the whole workgroup, for n <= OCT_PAR_MAX keys in LDS.  std::sort's recursion is a tree of
// disjoint ranges that are partitioned independently, so all ranges of one recursion level are processed together
// (breadth first), and one __unguarded_partition is evaluated in closed form: with L[k] = position of the k-th element that
// stops the upward scan (!(a < pivot), ascending) and R[k] = position of the k-th element that stops the downward scan
// (!(pivot < a), descending), the library swaps exactly the pairs (L[k], R[k]) with L[k] < R[k] -- a prefix k < K because L
// increases and R decreases -- and returns cut = min(L[K], R[K-1]) (the upward scan then stops at the next original stop
// or at the element the last swap put at R[K-1], whichever comes first).  Ranks come from one workgroup prefix sum.
// A thread owns two positions and keeps the range [first, last) of each in registers: a range's children are [first, cut) and
// [cut, last), so a position finds its next range from the cut alone -- no range table, no search; the thread that holds position
// `first` is the range's owner (median of three), the thread of pair K - 1 reports the cut.  All ranges of a recursion level
// share one depth budget (both children inherit depth - 1), so the heapsort fallback is a test of the level counter, and the
// loop ends when the level's stop flags sum to zero.  Five barriers per level.
// `ws` = 4 ints of LDS (blockScanExcl); scr = OCT_PAR_SCR_FOR(capN) dwords for at most capN keys (capN = 256, 512, or 2048 with
// 1024 threads): four u16 arrays of capN + 8 entries.
// rankedOut (optional, global or LDS, n keys): the whole std::sort -- the final insertion sort is a stable sort, and the partition phase
// leaves ranges of at most 16 keys (heapsorted ones may be longer) that are ordered among themselves: every key of a range is
// <= every key of the next (the pivot stays at the head of the left part).  So a key's final place is its range's start plus
// its stable rank inside the range, which the thread that holds the position computes from its registers.
__device__ __forceinline__ void stdSortPartitionPhasePar(u64* p, int n, int tid, uint32_t* scr, int* ws, int capN, u64* rankedOut = nullptr) {
  int f[2] = {0, 0}, l[2] = {n, n};
  auto rankOut = [&]() {
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int i = 2 * tid + j;
      if (i < n) {
        const u64 v = p[i], kv = v >> 20;
        int rank = 0;
        for (int q = f[j]; q < l[j]; q++) {
          const u64 kq = p[q] >> 20;
          rank += (kq < kv) || (kq == kv && q < i);
        }
        rankedOut[f[j] + rank] = v;
      }
    }
  };
  if (n <= 16) {
    if (rankedOut) rankOut();
    return;
  }
  // scr: two dword arrays.  LR[capN + 8]: low half = upward stops by rank (ascending), high half = downward stops by rank
  // (descending); LR[first] low = the range's cut.  SLR[capN + 2]: exclusive prefixes of the upward- (low half) and
  // downward-stop flags (high half) by position, [capN] = the totals.  (One dword per position and array instead of two
  // 16-bit arrays each: the phases below are bound by the CU's LDS instruction rate -- 16 waves x ~40 LDS instructions per
  // recursion level before, ~24 now -- and a wave none of whose positions lies in a range of more than 16 keys skips them.)
  uint32_t* LR = scr;
  uint32_t* SLR = scr + (capN + 8);
  uint16_t* LR16 = reinterpret_cast<uint16_t*>(LR);
  // the wave tasks' arrays (see below): SLRw of task wave w = SLR + 130 w; the task list behind them
  constexpr int NW = OCT_T / 64;
  const int nwb = min(NW, max(4, capN >> 7));
  uint32_t* taskList = SLR + max(capN + 2, 130 * nwb);  // [capN / 16 + 1] tasks + [1] their number
  uint32_t* taskCnt = taskList + (capN / 16 + 1);
  if (tid == 0) *taskCnt = 0;
  bool inTask[2] = {false, false};
  MemKeys A{p};
  int depth = 2 * (31 - __builtin_clz((unsigned)n));
  for (;;) {
    bool act[2];
#pragma unroll
    for (int j = 0; j < 2; j++) act[j] = (2 * tid + j) < n && (l[j] - f[j] > 16);
    // Once no range is longer than 128 keys the recursion goes on wave by wave: every range still to be partitioned becomes a
    // task of one wave (stdSortPartitionWaveTask), which runs all of its remaining levels without a workgroup barrier.
    if (!__syncthreads_or((act[0] && l[0] - f[0] > 128) || (act[1] && l[1] - f[1] > 128))) {
#pragma unroll
      for (int j = 0; j < 2; j++) {
        inTask[j] = act[j];
        if (act[j] && 2 * tid + j == f[j]) taskList[atomicAdd(taskCnt, 1u)] = (uint32_t)f[j] | ((uint32_t)l[j] << 16);
      }
      __syncthreads();
      const int nTasks = __builtin_amdgcn_readfirstlane((int)*taskCnt);
      const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
      if (wave < nwb)
        for (int r = wave; r < nTasks; r += nwb) {
          const uint32_t t = taskList[r];
          stdSortPartitionWaveTask(p, (int)(t & 0xffff), (int)(t >> 16), depth, tid & 63, LR, SLR + 130 * wave, rankedOut != nullptr);
        }
      break;
    }
    const bool wAct = __ballot(act[0] || act[1]) != 0ull;  // (wave-uniform)
    if (depth == 0) {  // __introsort_loop: heapsort of what is left of the ranges
      // (a range of more than 16 keys starts at one of a thread's two positions at most)
      const int own = (act[0] && 2 * tid == f[0]) ? 0 : ((act[1] && 2 * tid + 1 == f[1]) ? 1 : -1);
      if (own >= 0) stdHeapSortRange(A, own ? f[1] : f[0], own ? l[1] : l[0]);
      break;
    }
    --depth;
    // ---- owners: __move_median_to_first(first, first + 1, mid, last - 1) ----
    if (wAct) {
#pragma unroll
      for (int j = 0; j < 2; j++)
        if (act[j] && 2 * tid + j == f[j]) {
          const int first = f[j], last = l[j];
          const int ia = first + 1, ib = first + (last - first) / 2, ic = last - 1;
          const u64 a = p[ia], b = p[ib], c = p[ic], fv = p[first];
          int sel;
          if (SLESS(a, b)) sel = SLESS(b, c) ? ib : (SLESS(a, c) ? ic : ia);
          else sel = SLESS(a, c) ? ia : (SLESS(b, c) ? ic : ib);
          p[first] = sel == ia ? a : (sel == ib ? b : c);
          p[sel] = fv;
        }
    }
    __syncthreads();
    // ---- every position inside a range: its stop flags ----
    int gl[2] = {0, 0}, ll[2] = {0, 0};
    if (wAct) {
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int i = 2 * tid + j;
        if (act[j] && i > f[j]) {
          const u64 v = p[i], pv = p[f[j]];
          gl[j] = !SLESS(v, pv);
          ll[j] = !SLESS(pv, v);
        }
      }
    }
    // one workgroup scan for both flag sets: the counts (<= 2 x OCT_T <= 2048) ride in the two halves of one word
    int totLR;
    const int exLR = blockScanExcl((gl[0] + gl[1]) | ((ll[0] + ll[1]) << 16), tid, ws, &totLR, false);  // (barrier after the owners' phase)
    if (totLR == 0) break;  // no range left to partition (every range has a stop: its pivot's neighbours by the median of three)
    if (2 * tid < capN) {  // (flags beyond n are 0: the prefix stays at the total there; every position's entry is read as some range's end)
      const uint32_t e0 = (uint32_t)exLR, e1 = (uint32_t)(exLR + (gl[0] | (ll[0] << 16)));
      *reinterpret_cast<uint2*>(&SLR[2 * tid]) = make_uint2(e0, e1);
    }
    if (tid == 0) SLR[capN] = (uint32_t)totLR;
    __syncthreads();
    // ---- scatter the stop positions by rank: upward stops ascending, downward stops descending ----
    int nL[2] = {0, 0}, nR[2] = {0, 0};
    if (wAct) {
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int i = 2 * tid + j;
        if (act[j] && i > f[j]) {
          const uint32_t bb = SLR[f[j] + 1], be = SLR[l[j]], bi = SLR[i];
          const int bL = (int)(bb & 0xffff), bR = (int)(bb >> 16);
          nL[j] = (int)(be & 0xffff) - bL;
          nR[j] = (int)(be >> 16) - bR;
          if (gl[j]) LR16[2 * (f[j] + 1 + ((int)(bi & 0xffff) - bL))] = (uint16_t)i;
          if (ll[j]) LR16[2 * (f[j] + 1 + (nR[j] - 1 - ((int)(bi >> 16) - bR))) + 1] = (uint16_t)i;
        }
      }
    }
    __syncthreads();
    // ---- the swaps: pair k of a range lives at index first + 1 + k; the thread of pair K - 1 (pair 0 when K = 0) reports
    //      cut = min(L[K], R[K - 1]) at LR[first] (low half), which is never a rank slot ----
    if (wAct) {
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int i = 2 * tid + j;
        if (act[j] && i > f[j]) {
          const int k = i - (f[j] + 1), m = min(nL[j], nR[j]);
          const uint32_t lr0 = LR[i], lr1 = LR[i + 1];
          int a = 4096, b = -1;
          bool sw = false, nextSw = false;
          if (k < m) {
            a = (int)(lr0 & 0xffff); b = (int)(lr0 >> 16);
            sw = a < b;
            if (sw && k + 1 < m) nextSw = (int)(lr1 & 0xffff) < (int)(lr1 >> 16);
          }
          int cut = -1;
          if (sw && !nextSw) cut = min(k + 1 < nL[j] ? (int)(lr1 & 0xffff) : 4096, b);
          if (!sw && k == 0) cut = nL[j] > 0 ? (int)(lr0 & 0xffff) : 4096;
          if (sw) {
            const u64 va = p[a], vb = p[b];
            p[a] = vb;
            p[b] = va;
          }
          if (cut >= 0) LR16[2 * f[j]] = (uint16_t)cut;
        }
      }
    }
    __syncthreads();
    // ---- every position of a partitioned range moves to the child that holds it ----
    if (act[0]) {
      const int c = (int)(LR[f[0]] & 0xffff);
      if (2 * tid < c) l[0] = c; else f[0] = c;
    }
    if (act[1]) {
      const int c = (int)(LR[f[1]] & 0xffff);
      if (2 * tid + 1 < c) l[1] = c; else f[1] = c;
    }
  }
  if (rankedOut) {
    __syncthreads();  // (the last swaps / a heapsort have been written)
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (inTask[j]) {  // the position's final range, left behind by the wave that partitioned it
        const uint32_t fl = LR[2 * tid + j];
        f[j] = (int)(fl & 0xffff);
        l[j] = (int)(fl >> 16);
      }
    rankOut();
  }
}

// The boundaries of a node's children: the positions i in (lo, hi) of the sorted keys with div[i] <= t (t = the node's depth + 1),
// ascending -- at most three, a node has at most four children; h1..h3 = hi where there is none.  Sixteen depths per LDS read
// (div 16-byte aligned, readable up to the next multiple of 16 behind hi), tested as bytes inside dwords: depths are <= 17 or 255,
// so (byte | 0x80) - (t + 1) keeps its high bit exactly when byte > t, without borrows between the bytes.  Returns their number.
__device__ __forceinline__ int octChildBounds(const uint8_t* div, int lo, int hi, int t, int& h1, int& h2, int& h3) {
  int nh = 0;
  h1 = hi; h2 = hi; h3 = hi;
  const uint32_t sub = 0x01010101u * (uint32_t)(t + 1);
  for (int w = (lo + 1) & ~15; w < hi; w += 16) {
    const uint4 d = *reinterpret_cast<const uint4*>(div + w);
    auto nib = [&](uint32_t x) {  // bit b = byte b of x is <= t
      const uint32_t hb = (~((x | 0x80808080u) - sub) & 0x80808080u) >> 7;
      return ((hb * 0x00204081u) >> 21) & 0xfu;
    };
    uint32_t m = nib(d.x) | (nib(d.y) << 4) | (nib(d.z) << 8) | (nib(d.w) << 12);
    if (w <= lo) m &= ~((2u << (lo - w)) - 1u);
    if (hi - w < 16) m &= (1u << (hi - w)) - 1u;
    while (m) {
      const int pos = w + __builtin_ctz(m);
      if (nh == 0) h1 = pos; else if (nh == 1) h2 = pos; else h3 = pos;
      nh++;
      m &= m - 1u;
    }
  }
  return nh;
}

// reference candidate order (cell row, cell col, y, x) of a packed candidate (cpp:1078-1137; cv::FAST is row-major)
__device__ __forceinline__ u64 candRank(uint32_t e, const OctLevel& L) {
  const int x = e & 0xfff, y = (e >> 12) & 0xfff;
  const int cr = max(y - 3, 0) / L.hCell, cc = max(x - 3, 0) / L.wCell;
  return ((u64)(cr * L.nCols + cc) << 24) | ((u64)y << 12) | (u64)x;
}

__device__ __forceinline__ void rootRect(const OctLevel& L, int root, int& ulx, int& uly, int& brx, int& bry) {
  ulx = (int)(L.hX * (float)root);
  brx = (int)(L.hX * (float)(root + 1));
  uly = 0;
  bry = L.height;
}

// Lists the candidates of one (frame, level) unit: k_fast writes every cell's survivors into the cell's own segment
// (without atomics); dst[0 .. n) receives the positions (cell * segCap + k) of the n survivors inside the unit's candidate
// area, cells in index order.  The position doubles as the candidate's index in the sort keys, so the candidates themselves
// are read from the segments where they lie (L2) and never copied.  Returns n to every thread; nothing is written when
// n > cap.  `ws` = 4 ints of LDS.  Call with the whole workgroup.
__device__ __forceinline__ int gatherCandidates(const int* __restrict__ cellCnt, int nCells, int segCap, uint32_t* dst, int cap, int tid, int* ws) {
  const int chunk = (nCells + OCT_T - 1) / OCT_T;
  const int b = min(tid * chunk, nCells), e = min(b + chunk, nCells);
  int c = 0;
  for (int i = b; i < e; i++) c += cellCnt[i];
  int n;
  int pos = blockScanExcl(c, tid, ws, &n, false);  // (first scan of the unit, or behind the previous unit's last barrier)
  if (n <= cap)
    for (int i = b; i < e; i++) {
      const int k = chunk == 1 ? c : cellCnt[i];
      for (int j = 0; j < k; j++) dst[pos++] = (uint32_t)(i * segCap + j);
    }
  __syncthreads();
  return n;
}

// The whole selection for one (frame, level).  S.cand: n unordered packed candidates.  Writes min(#nodes, quota) SelKp
// records (list order) to `out` and the count to *nOut (-2: scratch too small for this unit).
//
// SCRATCH INVARIANTS (every array of OctScratch, who sizes it, and what keeps every write inside it).  Callers: the LDS
// kernels (capacities NMAX / MCAP = 4 QMAX / FCAP = 2 QMAX / qCap = QMAX, all powers of two >= OCT_T) and octreeGlobalUnit
// (layout = octScratchBytes(nMax, qMax): nPadAlloc = max(1024, pow2ceil(nMax)), mPadAlloc = max(1024, pow2ceil(4 qMax)),
// mCap = 4 qMax, fCap = 16 qMax, qCap = qMax).  OCT_T <= 1024 in both instances.
//   keys[0 .. nPad)        nPad = max(pow2ceil(n), OCT_T) <= nPadAlloc because n <= nMax (checked by the caller) and OCT_T <= 1024.
//                          The register sort reads and writes exactly max(nPad, OCT_T) padded entries: this is the array that
//                          overran in the round-1 fault (DESIGN.md section 9) when its allocation was pow2ceil(n) for small n.
//   nodes[0 .. mPad)       mPad = max(pow2ceil(M), OCT_T); M <= mCap is checked below (-2 otherwise), so mPad <= mPadAlloc.
//   div[0 .. n]                       n + 1 <= nPadAlloc + 8 (global) / NMAX + 4 (LDS).
//   hiOf[lo], lo < n       one entry per sorted position.
//   nodeLo/Hi/Depth/Alive[0 .. mCap + fCap)   list nodes use [0, M) with M <= mCap; pushed nodes use mCap + nFront + k with
//                          nFront + totC <= fCap checked before any is written (-2 otherwise).
//   pending[2][qCap], sized[2][qCap], childCnt[qCap]   indexed by j < nPend; nPend <= qCap is checked at entry of the partial
//                          pass and for every further round (totM <= qCap unless the round is the last one, whose multi-key
//                          children are not listed).
//   parScr                 OCT_PAR_SCR_FOR(parCap) dwords: static_asserts at the two call sites.
//   sortTmp[0 .. n)        radix sort's second buffer (global units only), nPadAlloc entries; the partial pass's stable sort
//                          pads nPend <= n keys to max(pow2ceil(nPend), OCT_T) <= nPadAlloc entries there.
//   ceBuf[0 .. n)          step 6: NMAX entries in nodes[]'s space (LDS kernel, static_assert there); sortTmp's 2 nPadAlloc dwords.
//   candE[0 .. n)          = the position list's nPadAlloc entries (global units).
//   IDX (hiOf, nodeLo, nodeHi)   hold sorted positions 0 .. n: uint16_t in the LDS kernel (n <= NMAX <= 65535, static_assert there),
//                          int in the global units (n < 2^19).
//   cand (LDS kernel)      the position list shares nodes[]: step 1 is its last reader, step 4 the first writer of nodes[].
// A -2 makes the LDS kernel redo the unit on global scratch; there it becomes -1 = ORBX_E_CAPACITY for the batch.
template <class SCR>
__device__ __forceinline__ void octreeSelect(const SCR S, int n, const OctLevel L, const uint32_t* __restrict__ codeTab, int level,
                             SelKp* __restrict__ out, int* __restrict__ nOut, int mCap, int fCap, int qCap) {
  __shared__ int cntDiv[OCT_DEPTH + 2], cntAlone[OCT_DEPTH + 2];
  __shared__ int sK, sPhase2, sM, sFront, sSize, sCut, sFinish;
  __shared__ int ws[OCT_T / 64];
  const int tid = threadIdx.x;
  const int N = L.quota;
  if (n <= 0 || N <= 0) {  // nothing to select (an empty quota truncates everything, cpp:1159-1161)
    if (tid == 0) *nOut = 0;
    return;
  }
  int nPad = 1;
  while (nPad < n) nPad <<= 1;
  if (nPad < OCT_T) nPad = OCT_T;  // the register sort works on at least OCT_T (padded) keys

  // ---- 1. path codes -----------------------------------------------------------------------------------------
  constexpr int RC = SCR::kRegCand;
  uint32_t myE[RC > 0 ? RC : 1];  // candidate tid + q * OCT_T in slot q (RC > 0)
  static_assert(RC % 4 == 0, "register-resident candidates come in steps of four");
  // four candidates per step: their dependent loads are in flight together.  The 16 quadrant digits of DivideNode (cpp:617-676)
  // come from the level's tables: x and y are routed independently, so code = root << 32 | xDigits(x) | yDigits(y)
  // (octCodeTable on the host walks the splits once per coordinate value instead of once per candidate here)
  const uint2* __restrict__ tabX = reinterpret_cast<const uint2*>(codeTab + L.tabOff);
  const uint32_t* __restrict__ tabY = codeTab + L.tabOff + 2 * L.tabW;
  // (GS candidates per step: eight in the 1024-thread units, whose three dependent loads all go to global memory)
  constexpr int GS = OCT_T >= 1024 ? 8 : 4;
  static_assert(RC == 0 || GS == 4, "the register-resident candidates come in groups of four");
  auto codesOf = [&](const int i0, uint32_t* keep) {
    uint32_t gi[GS], ce[GS], ty[GS];
    uint2 tx[GS];
#pragma unroll
    for (int j = 0; j < GS; j++) {
      const int i = i0 + j * OCT_T;
      gi[j] = i < n ? S.cand[i] : 0u;  // position of candidate i in the unit's candidate area
    }
#pragma unroll
    for (int j = 0; j < GS; j++) ce[j] = (i0 + j * OCT_T) < n ? S.segBase[gi[j]] : 0u;
#pragma unroll
    for (int j = 0; j < GS; j++) {
      tx[j] = tabX[min((int)(ce[j] & 0xfff), L.tabW - 1)];
      ty[j] = tabY[min((int)((ce[j] >> 12) & 0xfff), L.tabH - 1)];
    }
#pragma unroll
    for (int j = 0; j < GS; j++)
      if (keep) keep[j] = ce[j];
#pragma unroll
    for (int j = 0; j < GS; j++) {
      const int i = i0 + j * OCT_T;
      if (i >= nPad) break;
      if constexpr (sizeof(*S.keys) == 4) {
        // the top rootBits + 2 D bits of the code (keyShift = 32 - 2 D >= 12), then the candidate's index
        const uint32_t code = (tx[j].y << (32 - S.keyShift)) | ((tx[j].x | ty[j]) >> S.keyShift);
        S.keys[i] = i < n ? (code << 11) | (uint32_t)i : ~0u;
      } else {
        // (the index grows with the position in the candidate area: same order among equal codes as the reference's list index)
        const u64 code = (((u64)tx[j].y << 32) | (u64)(tx[j].x | ty[j])) >> S.keyShift;
        S.keys[i] = i < n ? (code << 24) | (u64)(uint32_t)i : ~0ull;
      }
      if constexpr (RC == 0)
        if (i < n) S.candE[i] = ce[j];
    }
  };
  if constexpr (RC > 0) {
#pragma unroll
    for (int it = 0; it < RC / 4; it++) {
#pragma unroll
      for (int j = 0; j < 4; j++) myE[4 * it + j] = 0u;
      if (tid + it * 4 * OCT_T < nPad) codesOf(tid + it * 4 * OCT_T, &myE[4 * it]);
    }
  } else {
    for (int i0 = tid; i0 < nPad; i0 += GS * OCT_T) codesOf(i0, nullptr);
  }
  if (tid < OCT_DEPTH + 2) { cntDiv[tid] = 0; cntAlone[tid] = 0; }
  __syncthreads();
  if constexpr (sizeof(*S.keys) == 4) {
    bitonicSort(S.keys, nPad, tid, (uint32_t*)nullptr, 0);  // 32-bit keys exist in the LDS kernel only
  } else {
    if (S.sortTmp && S.xchg && nPad > min(S.xchgCap, OCT_SORT_LDS)) {
      const int rootBits = L.nIni > 1 ? 32 - __builtin_clz((unsigned)(L.nIni - 1)) : 0;
      if (OCT_T >= 1024 && 2 * S.xchgCap >= 512 * (OCT_T / 64))  // (uniform) the exchange buffer holds 512 x nWaves counters
        radixSortCodes<9>(S.keys, S.sortTmp, n, tid, reinterpret_cast<uint32_t*>(S.xchg), ws, 2 * OCT_DEPTH - S.keyShift + rootBits,
                          S.radixCnt2);
      else
        radixSortCodes<8>(S.keys, S.sortTmp, n, tid, reinterpret_cast<uint32_t*>(S.xchg), ws, 2 * OCT_DEPTH - S.keyShift + rootBits);
    } else {
      bitonicSort(S.keys, nPad, tid, S.xchg, S.xchgCap);
    }
  }

  // ---- 2. divergence depths, S_d (distinct depth-d prefixes), singles_d -----------------------------------------
  for (int i = tid; i <= n; i += OCT_T) {
    int d = 255;
    if (i > 0 && i < n) {
      d = divDepth(keyCode(S, i - 1), keyCode(S, i));
      atomicAdd(&cntDiv[d], 1);
    }
    S.div[i] = (uint8_t)d;
  }
  __syncthreads();
  for (int i = tid; i < n; i += OCT_T) atomicAdd(&cntAlone[octAlone(S.div, i)], 1);
  __syncthreads();
  // ---- 3. replay the pass loop on sizes only (cpp:781-895) ------------------------------------------------------
  if (tid == 0) {
    int Sd[OCT_DEPTH + 2], sg[OCT_DEPTH + 2];
    int accD = 0, accA = 0;
    for (int d = 0; d <= OCT_DEPTH; d++) {
      accD += cntDiv[d];
      accA += cntAlone[d];
      Sd[d] = 1 + accD;
      sg[d] = accA;
    }
    Sd[OCT_DEPTH + 1] = Sd[OCT_DEPTH];
    sg[OCT_DEPTH + 1] = sg[OCT_DEPTH];
    int k = 0, phase2 = 0;
    for (;;) {
      const int prevSize = Sd[k];
      if (k < OCT_DEPTH) k++;
      const int size = Sd[k], nToExpand = size - sg[k];
      if (size >= N || size == prevSize) break;
      if (size + 3 * nToExpand > N) { phase2 = 1; break; }
    }
    sK = k;
    sPhase2 = phase2;
    sM = Sd[k];
    sFront = 0;
  }
  __syncthreads();
  const int k = sK;
  const int M = sM;  // nodes in the list after k full passes
  if (M > mCap) {    // cannot happen for capacities sized from the quota (M < 4N) unless N < nIni; guard anyway
    if (tid == 0) *nOut = -2;
    return;
  }
  // ---- 4. node list in std::list order ---------------------------------------------------------------------------
  // node starts: a leaf key (alone < k) or the first key of a depth-k group
  {
    const int chunk = (n + OCT_T - 1) / OCT_T;
    const int b = min(tid * chunk, n), e = min(b + chunk, n);
    int c = 0;
    for (int i = b; i < e; i++) c += (octAlone(S.div, i) < k) || (S.div[i] == 255 || (int)S.div[i] <= k);
    int tot;
    int m = blockScanExcl(c, tid, ws, &tot, false);  // (barrier behind step 3)
    for (int i = b; i < e; i++) {
      const int al = octAlone(S.div, i);
      const bool leaf = al < k;
      if (leaf || (S.div[i] == 255 || (int)S.div[i] <= k)) {
        const int j = leaf ? al : k;  // block depth
        const u64 code = keyCode(S, i);
        // order key: first j digits, digit m flipped when (j - m) is even, root flipped when j is odd
        const u64 prefix = code >> (2 * (OCT_DEPTH - j));
        u64 flip = 0;
        for (int mm = j; mm >= 1; mm -= 2) flip |= (u64)3 << (2 * (j - mm));
        u64 okey = prefix ^ flip;
        if (j & 1) {
          const u64 root = okey >> (2 * j);
          okey = (okey & (((u64)1 << (2 * j)) - 1)) | ((u64)(255 - root) << (2 * j));
        }
        S.nodes[m++] = ((u64)(OCT_DEPTH + 1 - j) << 59) | (okey << 19) | (u64)i;
      }
    }
    __syncthreads();
  }
  int mPad = 1;
  while (mPad < M) mPad <<= 1;
  if (mPad < OCT_T) mPad = OCT_T;
  for (int m = tid; m < M; m += OCT_T) {  // ends of the nodes, from the position-ordered list before it is re-sorted
    const int lo = (int)(S.nodes[m] & 0x7ffff);
    const int hi = (m + 1 < M) ? (int)(S.nodes[m + 1] & 0x7ffff) : n;
    S.hiOf[lo] = hi;
  }
  __syncthreads();
  for (int m = M + tid; m < mPad; m += OCT_T) S.nodes[m] = ~0ull;
  __syncthreads();
  bitonicSort(S.nodes, mPad, tid, S.xchg, S.xchgCap);
  for (int m = tid; m < M; m += OCT_T) {
    const u64 v = S.nodes[m];
    const int lo = (int)(v & 0x7ffff);
    S.nodeLo[m] = lo;
    S.nodeHi[m] = (int)S.hiOf[lo];
    S.nodeDepth[m] = (uint8_t)(OCT_DEPTH + 1 - (int)(v >> 59));
  }
  __syncthreads();

  // ---- 5. partial pass(es), cpp:897-965 ---------------------------------------------------------------------------
  if (sPhase2) {
    int* pendA = S.pending;
    int* pendB = S.pending + qCap;
    u64* sizedA = S.sized;
    u64* sizedB = S.sized + qCap;
    // pending = multi-key depth-k nodes in creation order = reverse of the depth-k block order
    int nPend;
    {
      const int chunk = (M + OCT_T - 1) / OCT_T;
      const int b = min(tid * chunk, M), e = min(b + chunk, M);
      int c = 0;
      for (int r = b; r < e; r++) {  // r = reversed list index
        const int i = M - 1 - r;
        c += (S.nodeDepth[i] == k) && (S.nodeHi[i] - S.nodeLo[i] > 1);
      }
      int p = blockScanExcl(c, tid, ws, &nPend, false);  // (barriers of step 4)
      if (nPend <= qCap)
        for (int r = b; r < e; r++) {
          const int i = M - 1 - r;
          if ((S.nodeDepth[i] == k) && (S.nodeHi[i] - S.nodeLo[i] > 1)) pendA[p++] = i;
        }
    }
    if (tid == 0) { sSize = M; sFinish = 0; }
    __syncthreads();
    if (nPend > qCap) {  // E_k < N <= qCap always; guard anyway
      if (tid == 0) *nOut = -2;
      return;
    }
    int nFront = 0;
    for (;;) {
      // (a) sort keys: count << 40 | UL.x << 20 | node
      for (int j = tid; j < nPend; j += OCT_T) {
        const int nd = pendA[j];
        const int lo = S.nodeLo[nd];
        const u64 code = keyCode(S, lo);
        int ulx, uly, brx, bry;
        rootRect(L, (int)(code >> (2 * OCT_DEPTH)), ulx, uly, brx, bry);
        const int depth = S.nodeDepth[nd];
        for (int d = 1; d <= depth; d++) {
          const int q = (int)((code >> (2 * (OCT_DEPTH - d))) & 3);
          const int halfX = (brx - ulx + 1) >> 1, halfY = (bry - uly + 1) >> 1;
          if (q & 1) ulx += halfX; else brx = ulx + halfX;
          if (q & 2) uly += halfY; else bry = uly + halfY;
        }
        sizedA[j] = ((u64)(S.nodeHi[nd] - lo) << 40) | ((u64)(ulx & 0xfffff) << 20) | (u64)nd;
      }
      __syncthreads();
      // (b) std::sort (cpp:912): partition phase replayed, final insertion sort as a parallel stable rank sort
      constexpr bool ldsUnit = sizeof(*S.nodeLo) == 2;  // the LDS kernel: at most 256 pending nodes, everything in LDS
      if (nPend <= S.parCap && S.parScr) {
        // keys in global memory: the replay works on a copy in the sort exchange buffer (its phases are chains of scattered
        // reads) when the replay's own scratch lives elsewhere
        const bool viaLds = S.xchg && S.parScr != reinterpret_cast<uint32_t*>(S.xchg) && nPend <= S.xchgCap;
        u64* pk = sizedA;
        if (viaLds) {
          for (int j = tid; j < nPend; j += OCT_T) S.xchg[j] = sizedA[j];
          __syncthreads();
          pk = S.xchg;
        }
        stdSortPartitionPhasePar(pk, nPend, tid, S.parScr, ws, S.parCap);
        if (viaLds) {
          __syncthreads();
          for (int j = tid; j < nPend; j += OCT_T) sizedA[j] = S.xchg[j];
        }
      } else {
        stdSortPartitionPhase(sizedA, nPend, tid);
      }
      __syncthreads();
      if constexpr (ldsUnit) {
        // the insertion sort is stable on the partition phase's output: rank by (count, UL.x, position) -- 12 + 12 + 8 bits here
        // (a node holds at most 2048 candidates, UL.x < 4096, at most 256 pending nodes), read four at a time
        uint32_t* kc = reinterpret_cast<uint32_t*>(S.childCnt);  // (written by (c) only)
        const int n4 = (nPend + 3) & ~3;
        if (tid < n4) {
          const u64 v = tid < nPend ? sizedA[tid] : ~0ull;
          kc[tid] = tid < nPend ? ((uint32_t)(v >> 40) << 20) | (((uint32_t)(v >> 20) & 0xfffu) << 8) | (uint32_t)tid : ~0u;
        }
        __syncthreads();
        if (tid < nPend) {
          const uint32_t kv = kc[tid];
          int rank = 0;
          for (int i = 0; i < n4; i += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4*>(&kc[i]);
            rank += (int)(k4.x < kv) + (int)(k4.y < kv) + (int)(k4.z < kv) + (int)(k4.w < kv);
          }
          sizedB[rank] = sizedA[tid];
        }
      } else if (OCT_T >= 1024 && S.sortTmp && nPend > 128) {  // (global-scratch units)
        // (global-scratch units) a stable sort by (count, UL.x) as ONE bitonic sort of (count, UL.x, position): the rank
        // counting below reads every element for every element -- 97 k cycles of a 1080p / 4K level-0 unit
        int sp = OCT_T;
        while (sp < nPend) sp <<= 1;
        for (int j = tid; j < sp; j += OCT_T) S.sortTmp[j] = j < nPend ? ((sizedA[j] >> 20) << 20) | (u64)j : ~0ull;
        __syncthreads();
        bitonicSort(S.sortTmp, sp, tid, S.xchg, S.xchgCap);
        for (int r = tid; r < nPend; r += OCT_T) sizedB[r] = sizedA[(int)(S.sortTmp[r] & 0xfffff)];
      } else {
        for (int j = tid; j < nPend; j += OCT_T) {
          const u64 v = sizedA[j];
          const u64 kv = v >> 20;
          int rank = 0;
          for (int i = 0; i < nPend; i++) {
            const u64 ki = sizedA[i] >> 20;
            rank += (ki < kv) || (ki == kv && i < j);
          }
          sizedB[rank] = v;
        }
      }
      __syncthreads();
      // (c) children of every pending node (in sorted order)
      uint32_t* childB = S.parScr;  // (LDS kernels) [2 nPend]: the children's boundaries h1 | h2 << 16, h3 -- (e) creates from them
      for (int j = tid; j < nPend; j += OCT_T) {
        const int nd = (int)(sizedB[j] & 0xfffff);
        const int lo = S.nodeLo[nd], hi = S.nodeHi[nd], pd = S.nodeDepth[nd];
        int nch = 1, nmulti = 1;
        if constexpr (ldsUnit) {
          if (pd < OCT_DEPTH) {
            int h1, h2, h3;
            nch = octChildBounds(S.div, lo, hi, pd + 1, h1, h2, h3) + 1;
            nmulti = (int)(h1 - lo > 1) + (int)(h2 - h1 > 1) + (int)(h3 - h2 > 1) + (int)(hi - h3 > 1);
            *reinterpret_cast<uint2*>(&childB[2 * j]) = make_uint2((uint32_t)h1 | ((uint32_t)h2 << 16), (uint32_t)h3);
          }
        } else
        if (pd < OCT_DEPTH) {
          nch = 0;
          nmulti = 0;
          // (four depths per round trip: the loop is a chain of LDS reads, and the largest pending node sets the phase's time)
          int start = lo;
          for (int i = lo + 1; i < hi; i += 4) {
            int dv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) dv[q] = (i + q < hi) ? (int)S.div[i + q] : 255;
#pragma unroll
            for (int q = 0; q < 4; q++)
              if (i + q < hi && dv[q] <= pd + 1) {
                nch++;
                nmulti += (i + q - start > 1);
                start = i + q;
              }
          }
          nch++;  // the child that ends at hi
          nmulti += (hi - start > 1);
        }
        S.childCnt[j] = nch | (nmulti << 8);
      }
      __syncthreads();
      // (d) cut point: nodes are split from the back of the sorted array until the list holds N nodes
      {
        // growth of the list when the last t+1 sorted nodes are split: inclusive prefix over t = nPend-1-j
        const int prevSize = sSize;
        const int chunk = (nPend + OCT_T - 1) / OCT_T;
        const int b = min(tid * chunk, nPend), e = min(b + chunk, nPend);
        int c = 0;
        for (int t = b; t < e; t++) c += (S.childCnt[nPend - 1 - t] & 0xff) - 1;
        int totalGrowth;
        int acc = blockScanExcl(c, tid, ws, &totalGrowth, false);  // (barrier behind (c))
        if (tid == 0) { sCut = 0; sSize = prevSize + totalGrowth; sFinish = (totalGrowth == 0 || prevSize + totalGrowth >= N) ? 1 : 0; }
        __syncthreads();
        // growth is >= 0 per split, so the first t whose inclusive sum reaches N - prevSize is unique: that thread reports
        for (int t = b; t < e; t++) {
          const int before = acc;
          acc += (S.childCnt[nPend - 1 - t] & 0xff) - 1;
          if (prevSize + before < N && prevSize + acc >= N) { sCut = nPend - 1 - t; sSize = prevSize + acc; sFinish = 1; }
        }
      }
      __syncthreads();
      const int cut = sCut, finish = sFinish;
      // (e) create the children: processing order t = nPend-1-j; children are push_front'ed in quadrant order
      {
        const int nProc = nPend - cut;
        const int chunk = (nProc + OCT_T - 1) / OCT_T;
        const int b = min(tid * chunk, nProc), e = min(b + chunk, nProc);
        int cc = 0, cm = 0;
        for (int t = b; t < e; t++) {
          const int v = S.childCnt[nPend - 1 - t];
          cc += v & 0xff;
          cm += v >> 8;
        }
        // both counts in one scan: at most 4 children per processed node, nProc <= qCap
        int totC, totM, offC, offM;
        if (4 * nProc < 65536) {
          int totCM;
          const int offCM = blockScanExcl(cc | (cm << 16), tid, ws, &totCM, false);  // (barrier behind (d))
          offC = offCM & 0xffff; offM = offCM >> 16; totC = totCM & 0xffff; totM = totCM >> 16;
        } else {
          offC = blockScanExcl(cc, tid, ws, &totC, false);
          offM = blockScanExcl(cm, tid, ws, &totM);
        }
        // (the multi-key children are listed only for another round; a finishing round may create up to N + 4 of them)
        if (nFront + totC > fCap || (!finish && totM > qCap)) {  // scratch too small: the caller re-runs the unit with more
          if (tid == 0) *nOut = -2;
          return;
        }
        for (int t = b; t < e; t++) {
          const int j = nPend - 1 - t;
          const int nd = (int)(sizedB[j] & 0xfffff);
          const int lo = S.nodeLo[nd], hi = S.nodeHi[nd], pd = S.nodeDepth[nd];
          if (pd >= OCT_DEPTH) {  // coincident keys: cannot be split further, stays one node
            const int id = mCap + nFront + offC++;
            S.nodeLo[id] = lo; S.nodeHi[id] = hi; S.nodeDepth[id] = (uint8_t)pd;
            if (!finish) pendB[offM++] = id;
          } else if constexpr (ldsUnit) {  // the boundaries (c) found
            const uint2 hb = *reinterpret_cast<const uint2*>(&childB[2 * j]);
            const int bnd[5] = {lo, (int)(hb.x & 0xffff), (int)(hb.x >> 16), (int)hb.y, hi};
            const int nch = S.childCnt[j] & 0xff;
#pragma unroll
            for (int q = 0; q < 4; q++)
              if (q < nch) {
                const int id = mCap + nFront + offC++;
                const int start = bnd[q], end = bnd[q + 1];
                S.nodeLo[id] = start; S.nodeHi[id] = end; S.nodeDepth[id] = (uint8_t)(pd + 1);
                if (!finish && end - start > 1) pendB[offM++] = id;
              }
          } else {
            int start = lo;
            auto child = [&](int end) {
              const int id = mCap + nFront + offC++;
              S.nodeLo[id] = start; S.nodeHi[id] = end; S.nodeDepth[id] = (uint8_t)(pd + 1);
              if (!finish && end - start > 1) pendB[offM++] = id;
              start = end;
            };
            for (int i = lo + 1; i < hi; i += 4) {
              int dv[4];
#pragma unroll
              for (int q = 0; q < 4; q++) dv[q] = (i + q < hi) ? (int)S.div[i + q] : 255;
#pragma unroll
              for (int q = 0; q < 4; q++)
                if (i + q < hi && dv[q] <= pd + 1) child(i + q);
            }
            child(hi);
          }
          S.nodeDepth[nd] = (uint8_t)(pd | 0x80);
        }
        nFront += totC;
        nPend = totM;
      }
      __syncthreads();
      if (finish) break;
      { int* t = pendA; pendA = pendB; pendB = t; }
    }
    if (tid == 0) sFront = nFront;
    __syncthreads();
  }
  // ---- 6. output positions: reverse(front alive) ++ list alive; keep the first `quota` ------------------------------
  const int nFront = sFront;
  const int total = nFront + M;  // virtual sequence: pushed nodes in reverse push order, then the list
  {
    const int chunk = (total + OCT_T - 1) / OCT_T;
    const int b = min(tid * chunk, total), e = min(b + chunk, total);
    auto nodeAt = [&](int v) { return v < nFront ? mCap + (nFront - 1 - v) : v - nFront; };
    // the candidates in sorted-key order, fetched by all threads at once (independent loads): the per-node loops below then
    // walk contiguous entries instead of chasing key -> position -> candidate through two dependent loads per key (22 % of a
    // 4K level-0 unit)
    if constexpr (RC > 0) {
      // the candidate words leave the registers: ceBuf[candidate index]; the loops below go through the key's index
#pragma unroll
      for (int q = 0; q < RC; q++)
        if (tid + q * OCT_T < n) S.ceBuf[tid + q * OCT_T] = myE[q];
    } else {
      for (int i0 = tid; i0 < n; i0 += 4 * OCT_T) {
        uint32_t pos[4], ce[4];
#pragma unroll
        for (int j = 0; j < 4; j++) pos[j] = (i0 + j * OCT_T) < n ? keyIndex(S, i0 + j * OCT_T) : 0u;
#pragma unroll
        for (int j = 0; j < 4; j++) ce[j] = (i0 + j * OCT_T) < n ? S.candE[pos[j]] : 0u;
#pragma unroll
        for (int j = 0; j < 4; j++)
          if ((i0 + j * OCT_T) < n) S.ceBuf[i0 + j * OCT_T] = ce[j];
      }
    }
    __syncthreads();
    int c = 0;
    for (int v = b; v < e; v++) c += (S.nodeDepth[nodeAt(v)] & 0x80) ? 0 : 1;
    if constexpr (RC > 0) {
      // The LDS kernels: every sorted key gets a 64-bit score = response << 40 | (2^40 - 1 - reference candidate order), computed
      // by all threads at once (the FAST cell of a candidate by 2^24 reciprocals, as in k_octree_buckets: exact for coordinates
      // below 4096 and cells of at least 16 pixels) and laid over keys[] / nodes[], which are dead from here on; a node's keypoint
      // is then the maximum over a contiguous range of scores -- "first key with the highest response" (cpp:984-1007) -- instead
      // of a per-node loop of two dependent LDS reads, a comparison chain and two integer divisions per key.
      const uint32_t wInv = ((1u << 24) + (uint32_t)L.wCell - 1u) / (uint32_t)L.wCell, hInv = ((1u << 24) + (uint32_t)L.hCell - 1u) / (uint32_t)L.hCell;
      constexpr u64 M40 = (1ull << 40) - 1ull;
      u64 sc[RC];
#pragma unroll
      for (int q = 0; q < RC; q++) {
        const int i = tid + q * OCT_T;
        sc[q] = 0;
        if (i < n) {
          const uint32_t ce = S.ceBuf[keyIndex(S, i)];
          const uint32_t cx = ce & 0xfffu, cy = (ce >> 12) & 0xfffu;
          const uint32_t cc = (uint32_t)(((u64)(cx > 3u ? cx - 3u : 0u) * (u64)wInv) >> 24), cr = (uint32_t)(((u64)(cy > 3u ? cy - 3u : 0u) * (u64)hInv) >> 24);
          const u64 rank = ((u64)(cr * (uint32_t)L.nCols + cc) << 24) | (u64)(ce & 0xffffffu);
          sc[q] = ((u64)(ce >> 24) << 40) | (M40 - rank);
        }
      }
      int alive;
      int p = blockScanExcl(c, tid, ws, &alive, true);  // (its barriers also separate the reads above from the writes below)
      u64* score = reinterpret_cast<u64*>(S.keys);
#pragma unroll
      for (int q = 0; q < RC; q++)
        if (tid + q * OCT_T < n) score[tid + q * OCT_T] = sc[q];
      __syncthreads();
      for (int v = b; v < e && p < N; v++) {
        const int nd = nodeAt(v);
        if (S.nodeDepth[nd] & 0x80) continue;
        const int lo = S.nodeLo[nd], hi = S.nodeHi[nd];
        u64 best = score[lo];
        for (int i = lo + 1; i < hi; i += 4) {
          u64 sv[4];
#pragma unroll
          for (int q = 0; q < 4; q++) sv[q] = (i + q < hi) ? score[i + q] : 0ull;
          const u64 m01 = sv[0] > sv[1] ? sv[0] : sv[1], m23 = sv[2] > sv[3] ? sv[2] : sv[3];
          const u64 m = m01 > m23 ? m01 : m23;
          best = m > best ? m : best;
        }
        const uint32_t r24 = (uint32_t)((M40 - (best & M40)) & 0xffffffu);  // y << 12 | x
        SelKp kp;
        kp.x = (uint16_t)((r24 & 0xfff) + ORBX_MIN_BORDER);  // cpp:1171-1172
        kp.y = (uint16_t)(((r24 >> 12) & 0xfff) + ORBX_MIN_BORDER);
        kp.level = (uint8_t)level;
        kp.response = (uint8_t)(best >> 40);
        kp.pad = 0;
        out[p++] = kp;
      }
      if (tid == 0) *nOut = min(alive, N);
      return;
    }
    auto ceAt = [&](int i) -> uint32_t { return S.ceBuf[i]; };  // candidate word of sorted key i
    int alive;
    int p = blockScanExcl(c, tid, ws, &alive, false);  // (barrier above)
    for (int v = b; v < e && p < N; v++) {
      const int nd = nodeAt(v);
      if (S.nodeDepth[nd] & 0x80) continue;
      // first key with the highest response (cpp:984-1007); "first" = reference candidate order
      const int lo = S.nodeLo[nd], hi = S.nodeHi[nd];
      uint32_t bestE = ceAt(lo);
      if (hi - lo > 1) {
        u64 bestRank = candRank(bestE, L);
        for (int i = lo + 1; i < hi; i += 4) {
          uint32_t ev[4];
#pragma unroll
          for (int q = 0; q < 4; q++) ev[q] = (i + q < hi) ? ceAt(i + q) : 0u;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            if (i + q >= hi) break;
            const uint32_t e2 = ev[q];
            const uint32_t s1 = bestE >> 24, s2 = e2 >> 24;
            if (s2 < s1) continue;
            const u64 r2 = candRank(e2, L);
            if (s2 > s1 || r2 < bestRank) { bestE = e2; bestRank = r2; }
          }
        }
      }
      SelKp kp;
      kp.x = (uint16_t)((bestE & 0xfff) + ORBX_MIN_BORDER);  // cpp:1171-1172
      kp.y = (uint16_t)(((bestE >> 12) & 0xfff) + ORBX_MIN_BORDER);
      kp.level = (uint8_t)level;
      kp.response = (uint8_t)(bestE >> 24);
      kp.pad = 0;
      out[p++] = kp;
    }
    if (tid == 0) *nOut = min(alive, N);
  }
}

// The unit's arrays inside its global scratch area (layout = octScratchBytes(nMax, qMax) on the host); candBuf = the position
// list of the one-workgroup units / the bucket records of the many-workgroup ones
__device__ __forceinline__ OctScratch octCarve(const OctLaunch& P, int level, int f, uint8_t* __restrict__ scratch, uint32_t** candBuf,
                                              int* mCapOut, int* fCapOut, int* qMaxOut) {
  const int nMax = P.scrNMax[level], qMax = max(max(P.lev[level].quota, P.lev[level].nIni), 1);
  size_t nPad = 1024;  // (= octScratchBytes; at least the largest workgroup size)
  while ((int)nPad < nMax) nPad <<= 1;
  const int mCap = 4 * qMax, fCap = 16 * qMax;
  size_t mPad = 1024;
  while ((int)mPad < mCap) mPad <<= 1;
  uint8_t* p = scratch + P.scrOff[level] + (int64_t)f * P.scrStride[level];
  OctScratch S;
  S.keys = (u64*)p; p += nPad * 8;
  {
    const int D = P.lev[level].depthBits;
    S.keyShift = (D >= 1 && D <= OCT_DEPTH) ? 2 * (OCT_DEPTH - D) : 0;
  }
  S.nodes = (u64*)p; p += mPad * 8;
  S.sized = (u64*)p; p += (size_t)2 * qMax * 8;
  S.hiOf = (int*)p; p += nPad * 4;
  S.nodeLo = (int*)p; p += (size_t)(mCap + fCap) * 4;
  S.nodeHi = (int*)p; p += (size_t)(mCap + fCap) * 4;
  S.pending = (int*)p; p += (size_t)2 * qMax * 4;
  S.childCnt = (int*)p; p += (size_t)qMax * 4;
  p = (uint8_t*)(((uintptr_t)p + 15) & ~(uintptr_t)15);  // (k_octree_big reads the divergence bytes sixteen at a time)
  S.div = p; p += nPad + 8;
  p += nPad + 8;  // (formerly alone[]: the layout, and with it octScratchBytes on the host, is unchanged)
  S.nodeDepth = p; p += (size_t)(mCap + fCap + 8);
  p += (size_t)(mCap + fCap + 8);  // (formerly nodeAlive[]: the layout, and with it octScratchBytes on the host, is unchanged)
  p = (uint8_t*)(((uintptr_t)p + 15) & ~(uintptr_t)15);
  *candBuf = (uint32_t*)p;           // [nPad]
  p += nPad * 4;
  S.sortTmp = (u64*)p;               // [nPad] (p stays 16-byte aligned: nPad is a multiple of 256)
  S.cand = nullptr; S.segBase = nullptr; S.xchg = nullptr; S.xchgCap = 0; S.parScr = nullptr; S.parCap = 0; S.candE = nullptr; S.ceBuf = nullptr;
  *mCapOut = mCap; *fCapOut = fCap; *qMaxOut = qMax;
  return S;
}

// first depth at which the keys of two buckets differ (bucket id = root << 2 D0 | the D0 top quadrant digits)
__device__ __forceinline__ int octBucketDiv(int a, int b, int d0) {
  const uint32_t x = (uint32_t)(a ^ b);
  if ((x >> (2 * d0)) != 0u) return 0;
  return d0 - (31 - __builtin_clz(x)) / 2;
}

#if OCT_T >= 1024
// ---- The selection of one LARGE (frame, level) unit whose keys k_octree_buckets has sorted bucket by bucket ------------------
// Everything that walks all n keys has happened there, on many workgroups: path codes, the key sort, the divergence depths
// inside the buckets and their histograms, and a SCORE per sorted key (response << 40 | inverted reference candidate order:
// "first of the highest responses", cpp:984-1007, is the maximum of the scores of a node's keys).  What is left for this one
// workgroup is the tree arithmetic on the M < 4 N nodes of the list: the pass loop on the histograms, the node list (scan of
// the divergence bytes, 16 per load), its sort, the partial pass (cpp:897-965) and the output.  Positions are SLOT positions
// (bucket b's keys at [b capB, b capB + cnt_b)); a list node never spans two buckets because bigD0 <= k (octBigPlan; checked).
// Differences to octreeSelect's partial pass: a pending node's children are found by three binary searches on the digit of the
// next depth (the keys of a node are sorted by it) instead of a walk over its divergence bytes; the stable sort behind the
// std::sort replay ranks every key inside its final partition range (<= 16 keys; ranges are ordered among themselves).
// score / info: the unit's sortTmp / candBuf regions.  xchg: LDS exchange buffer of xchgCap keys (>= mPad wanted).
__device__ __forceinline__ void octreeSelectBig(OctScratch S, const u64* __restrict__ score, const int* __restrict__ info, const OctLevel L,
                                               int level, SelKp* __restrict__ out, int* __restrict__ nOut, int mCap, int fCap, int qCap,
                                               int* __restrict__ nKeysOut) {
  __shared__ int cntDiv[OCT_DEPTH + 2], cntAlone[OCT_DEPTH + 2];
  __shared__ int sK, sPhase2, sM, sFront, sSize, sCut, sFinish, sBad, sMaxB;
  __shared__ int ws[OCT_T / 64];
  __shared__ int bCnt[ORBX_OCTB_MAX_BUCKETS + 1], bPre[ORBX_OCTB_MAX_BUCKETS + 1];  // keys of bucket b; chunks of 16 keys before it
  __shared__ int neList[ORBX_OCTB_MAX_BUCKETS];                                     // the non-empty buckets in order
  const int tid = threadIdx.x, lane = tid & 63;
  const int N = L.quota, nB = L.bigBuckets, capB = L.bigCapB, d0 = L.bigD0;
  static_assert(OCT_T >= ORBX_OCTB_MAX_BUCKETS, "one thread per bucket record");
  if (tid < OCT_DEPTH + 2) { cntDiv[tid] = 0; cntAlone[tid] = 0; }
  if (tid == 0) { sBad = 0; sMaxB = 0; }
  __syncthreads();
  // ---- 0. the buckets' records: counts, histograms, and what only the neighbours in key order can tell -------------------
  // (the records come from other XCDs' workgroups, i.e. from the fabric: one bulk load per thread, everything in flight at once)
  int rec[ORBX_OCTB_INFO];
  {
    const int4* r4 = reinterpret_cast<const int4*>(info + (size_t)min(tid, nB - 1) * ORBX_OCTB_INFO);
#pragma unroll
    for (int j = 0; j < ORBX_OCTB_INFO / 4; j++) {
      const int4 v = r4[j];
      rec[4 * j] = v.x; rec[4 * j + 1] = v.y; rec[4 * j + 2] = v.z; rec[4 * j + 3] = v.w;
    }
  }
  const int cnt = tid < nB ? rec[0] : 0, dFirst = rec[1], dLast = rec[2];
  if (tid < nB && (rec[3] || cnt < 0 || cnt >= capB)) sBad = 1;  // a slot overflowed (its last entry holds the divergence to the next bucket)
  if (tid < nB) bCnt[tid] = cnt;
  if (tid == 0) bCnt[nB] = 0;
  {  // the unit's fullest bucket: reported with the key count (ORBX_OCT_FEEDBACK) for the next batch's choice of k_octree_buckets' LDS slots
    const int wm = waveMaxLane63(cnt);
    if (lane == 63 && wm > 0) atomicMax(&sMaxB, wm);
  }
  // one scan for both: rank among the non-empty buckets (<= 1024) | chunks of 16 keys before the bucket (<= 2^15) << 12
  int totNC;
  const int exNC = blockScanExcl((cnt > 0 ? 1 : 0) | (((cnt + 15) >> 4) << 12), tid, ws, &totNC, false);
  const int rankNE = exNC & 0xfff, chunkPre = exNC >> 12, nNE = totNC & 0xfff, nChunks = totNC >> 12;
  if (cnt > 0) neList[rankNE] = tid;
  if (tid < nB) bPre[tid] = chunkPre;
  if (tid == 0) bPre[nB] = nChunks;
  __syncthreads();
  if (sBad || nNE == 0 || N <= 0) {
    // (an overfull bucket: the count reported for the next batch's choice of bucket depth asks for the deepest one)
    if (tid == 0) { *nOut = (sBad ? -2 : 0); if (nKeysOut) *nKeysOut = sBad ? ORBX_OCT_FEEDBACK(ORBX_OCT_MAX_CAND, ORBX_OCTB_CAP, d0) : 0; }
    return;
  }
  {
    const bool mine = tid < nB && cnt > 0;
    int binDiv = -1, binA1 = -1, binA2 = -1;  // what the neighbouring buckets add to this bucket's histogram rows
    if (mine) {
      const int prevB = rankNE > 0 ? neList[rankNE - 1] : -1, nextB = rankNE + 1 < nNE ? neList[rankNE + 1] : -1;
      const int dl = prevB >= 0 ? octBucketDiv(prevB, tid, d0) : 255, dr = nextB >= 0 ? octBucketDiv(tid, nextB, d0) : 255;
      S.div[(size_t)tid * capB] = (uint8_t)dl;
      S.div[(size_t)tid * capB + cnt] = (uint8_t)dr;
      const int dlv = dl == 255 ? -1 : dl, drv = dr == 255 ? -1 : dr;
      if (prevB >= 0) binDiv = dl;
      binA1 = max(max(dlv, cnt == 1 ? drv : (dFirst == 255 ? -1 : dFirst)), 0);              // the bucket's first key
      if (cnt >= 2) binA2 = max(max(dLast == 255 ? -1 : dLast, drv), 0);                      // ... and its last one
    }
    // histogram rows of the buckets: wave sums, then one atomic per wave and bin.  A bucket's row counts at most ORBX_OCTB_CAP keys,
    // so the divergence bin and the lonely-depth bin of a depth travel as the two halves of one word (64 rows: < 2^16), and only
    // the depths the level can have are summed (the workgroup's 16 waves share four SIMDs: every instruction counts 16 times)
    static_assert(64 * ORBX_OCTB_CAP <= 65535 + 1, "a wave's bin sums fit 16 bits");
    const int dTop = min(OCT_DEPTH + 1, (S.keyShift > 0 ? OCT_DEPTH - S.keyShift / 2 : OCT_DEPTH) + 1);
    if (__ballot(mine) != 0ull) {  // (wave-uniform)
#pragma unroll
      for (int j = 0; j < OCT_DEPTH + 2; j++) {
        if (j <= dTop) {  // (uniform)
          int v = 0;
          if (mine) v = (rec[4 + j] + (j == binDiv)) | ((rec[4 + OCT_DEPTH + 2 + j] + (j == binA1) + (j == binA2)) << 16);
          v = waveSumLane63(v);
          if (lane == 63 && v) {
            if (v & 0xffff) atomicAdd(&cntDiv[j], v & 0xffff);
            if (v >> 16) atomicAdd(&cntAlone[j], (int)((uint32_t)v >> 16));
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- 3. replay the pass loop on sizes only (cpp:781-895) ------------------------------------------------------
  if (tid == 0) {
    int Sd[OCT_DEPTH + 2], sg[OCT_DEPTH + 2];
    int accD = 0, accA = 0;
    for (int d = 0; d <= OCT_DEPTH; d++) {
      accD += cntDiv[d];
      accA += cntAlone[d];
      Sd[d] = 1 + accD;
      sg[d] = accA;
    }
    Sd[OCT_DEPTH + 1] = Sd[OCT_DEPTH];
    sg[OCT_DEPTH + 1] = sg[OCT_DEPTH];
    int k = 0, phase2 = 0;
    for (;;) {
      const int prevSize = Sd[k];
      if (k < OCT_DEPTH) k++;
      const int size = Sd[k], nToExpand = size - sg[k];
      if (size >= N || size == prevSize) break;
      if (size + 3 * nToExpand > N) { phase2 = 1; break; }
    }
    sK = k;
    sPhase2 = phase2;
    sM = Sd[k];
    sFront = 0;
    // the unit's candidate count (every key but the first diverges from its left neighbour at some depth): feedback for the next
    // batch's choice of kernel and bucket depth (reduced by k_sel_compact)
    if (nKeysOut) *nKeysOut = ORBX_OCT_FEEDBACK(Sd[OCT_DEPTH] + cntDiv[OCT_DEPTH + 1], sMaxB, d0);
  }
  __syncthreads();
  const int k = sK;
  const int M = sM;  // nodes in the list after k full passes
  if (M > mCap || k < d0) {  // (k < d0: the level's candidates ran out before the guaranteed depth -- a list node could span buckets)
    if (tid == 0) *nOut = -2;
    return;
  }
  // ---- 4. node list in std::list order ---------------------------------------------------------------------------
  // node starts = keys whose divergence from their left neighbour lies at depth <= k (a leaf key's does: its first lonely depth is
  // the larger of its two divergences).  A thread owns consecutive chunks of 16 keys; starts are counted, scanned and then listed
  // with their two divergence depths: position | left << 19 | right << 24 (255 -> 31).
  int* startInfo = reinterpret_cast<int*>(S.sized);  // [M <= 4 qCap]: free until the partial pass
  if (M > OCTBIG_NODES) {  // (the node tables below live in LDS)
    if (tid == 0) *nOut = -2;
    return;
  }
  {
    const int per = (nChunks + OCT_T - 1) / OCT_T;
    const int c0 = min(tid * per, nChunks), c1 = min(c0 + per, nChunks);
    int b0 = 0;
    if (c0 < c1) {  // bucket of my first chunk: last b with bPre[b] <= c0 (a non-empty one: its successor's number is larger)
      int lo = 0, hi = nB;  // invariant: bPre[lo] <= c0 < bPre[hi]  (bPre[nB] = nChunks)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bPre[mid] <= c0) lo = mid; else hi = mid;
      }
      b0 = lo;
    }
    // a chunk's 16 divergence bytes as four dwords: bit 7 of a byte of `(w & 0x7f7f7f7f) + (0x7f - k) * 0x01010101` is set iff the
    // byte's low seven bits exceed k, so a start (depth <= k, or 255 = the key's left neighbour lies in no bucket) is a byte with
    // that bit clear or its own bit 7 set; the bytes beyond the bucket's keys are masked off
    const uint32_t kAdd = (uint32_t)(0x7f - k) * 0x01010101u;
    auto walk = [&](auto&& onChunk) {
      int b = b0;
      for (int c = c0; c < c1; c++) {
        while (c >= bPre[b + 1] || bCnt[b] == 0) b++;
        const int off = (c - bPre[b]) << 4, nIn = min(16, bCnt[b] - off);
        const int pos0 = b * capB + off;
        const uint4 w = *reinterpret_cast<const uint4*>(S.div + pos0);  // (slots and chunks are multiples of 16 bytes)
        const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
        uint32_t flags = 0;  // bit q: key q of the chunk starts a node
#pragma unroll
        for (int q4 = 0; q4 < 4; q4++) {
          const uint32_t st = (~((wv[q4] & 0x7f7f7f7fu) + kAdd) | wv[q4]) & 0x80808080u;
          flags |= (((st >> 7) & 1u) | ((st >> 14) & 2u) | ((st >> 21) & 4u) | ((st >> 28) & 8u)) << (4 * q4);
        }
        flags &= nIn >= 16 ? 0xffffu : ((1u << nIn) - 1u);
        onChunk(pos0, flags, w);
      }
    };
    int c = 0;
    walk([&](int, uint32_t flags, const uint4&) { c += __popc(flags); });
    int tot;
    int m = blockScanExcl(c, tid, ws, &tot, false);  // (barrier behind step 3)
    if (tot != M) sBad = 1;                          // (cannot happen: the histograms count the same bytes)
    walk([&](int pos0, uint32_t flags, const uint4& w) {
      if (!flags) return;
      const uint32_t w4 = *reinterpret_cast<const uint32_t*>(S.div + pos0 + 16);  // the divergence behind the chunk's last key
      const uint32_t wv[5] = {w.x, w.y, w.z, w.w, w4};
      while (flags) {
        const int q = __builtin_ctz(flags);
        flags &= flags - 1u;
        // (dynamic dword select without a private array: four compares)
        const uint32_t wa = q < 4 ? wv[0] : (q < 8 ? wv[1] : (q < 12 ? wv[2] : wv[3]));
        const uint32_t wb = q + 1 < 4 ? wv[0] : (q + 1 < 8 ? wv[1] : (q + 1 < 12 ? wv[2] : (q + 1 < 16 ? wv[3] : wv[4])));
        const int d = (int)((wa >> (8 * (q & 3))) & 0xffu), dn = (int)((wb >> (8 * ((q + 1) & 3))) & 0xffu);
        if (m < mCap) startInfo[m] = (pos0 + q) | (min(d, 31) << 19) | (min(dn, 31) << 24);
        m++;
      }
    });
  }
  __syncthreads();
  if (sBad) {
    if (tid == 0) *nOut = -2;
    return;
  }
  int mPad = OCT_T;
  while (mPad < M) mPad <<= 1;
  // sort keys of the list nodes: (k - block depth) | order key | creation index.  32 bits whenever they fit (half the shuffles
  // of the sort): k <= 7 with at most four roots on VGA ... 4K levels; else 64 bits for up to OCTBIG_XCHG keys
  const int rootBits = L.nIni > 1 ? 32 - __builtin_clz((unsigned)(L.nIni - 1)) : 0;
  const int cBits = 32 - __builtin_clz((unsigned)k | 1u), okBits = rootBits + 2 * k;
  const bool use32 = cBits + okBits + 13 <= 32;
  if (!use32 && mPad > S.xchgCap) {
    if (tid == 0) *nOut = -2;
    return;
  }
  uint32_t* k32 = reinterpret_cast<uint32_t*>(S.xchg);
  for (int m0 = tid; m0 < mPad; m0 += 4 * OCT_T) {  // four nodes per step: their loads are in flight together
    int si[4], nxt[4];
    u64 kc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int m = m0 + j * OCT_T;
      si[j] = m < M ? startInfo[m] : 0;
      nxt[j] = m + 1 < M ? (startInfo[m + 1] & 0x7ffff) : 0x7fffffff;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) kc[j] = S.keys[si[j] & 0x7ffff];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int m = m0 + j * OCT_T;
      if (m >= mPad) break;
      if (m >= M) {
        if (use32) k32[m] = ~0u; else S.xchg[m] = ~0ull;
        continue;
      }
      const int pos = si[j] & 0x7ffff, dA = (si[j] >> 19) & 31, dB = (si[j] >> 24) & 31;
      const int al = max(max(dA == 31 ? -1 : dA, dB == 31 ? -1 : dB), 0);
      const int jd = al < k ? al : k;  // block depth: a leaf stays where it became lonely
      const u64 code = (kc[j] >> 24) << S.keyShift;
      // order key: first jd digits, digit m flipped when (jd - m) is even (every other digit, from the last one up), root flipped
      // when jd is odd
      const u64 prefix = code >> (2 * (OCT_DEPTH - jd));
      const uint32_t digMask = jd >= 16 ? 0xffffffffu : ((1u << (2 * jd)) - 1u);
      const uint32_t root = (uint32_t)(prefix >> (2 * jd)), dig = ((uint32_t)prefix ^ 0x33333333u) & digMask;
      if (use32) {
        const uint32_t rootC = (jd & 1) ? (uint32_t)(L.nIni - 1) - root : root;
        k32[m] = ((uint32_t)(k - jd) << (okBits + 13)) | (((rootC << (2 * jd)) | dig) << 13) | (uint32_t)m;
      } else {
        const u64 okey = (u64)dig | ((u64)((jd & 1) ? 255u - root : root) << (2 * jd));
        S.xchg[m] = ((u64)(OCT_DEPTH + 1 - jd) << 59) | (okey << 19) | (u64)m;
      }
      const int bk = pos / capB;
      const int hi = min(nxt[j], bk * capB + bCnt[bk]);  // the node ends at the next start, or with its bucket
      S.nodeLH[m] = (uint32_t)pos | ((uint32_t)(hi - pos) << 19);
      // UL.x of the node's rectangle (cpp:617-676 walked down the node's digits): the partial pass sorts its pending nodes -- the
      // multi-key ones of depth k -- by it
      if (jd == k && hi - pos > 1) {
        int ulx, uly, brx, bry;
        rootRect(L, (int)(code >> (2 * OCT_DEPTH)), ulx, uly, brx, bry);
        for (int d = 1; d <= k; d++) {
          const int q = (int)((code >> (2 * (OCT_DEPTH - d))) & 3);
          const int halfX = (brx - ulx + 1) >> 1;
          if (q & 1) ulx += halfX; else brx = ulx + halfX;
        }
        S.nodeUlx[m] = (uint16_t)ulx;
      }
    }
  }
  __syncthreads();
  {
    const int e = mPad / OCT_T;
    if (use32) {
      if (e == 1) bitonicSortRegs<1>(k32, tid);
      else if (e == 2) bitonicSortRegs<2>(k32, tid);
      else if (e == 4) bitonicSortRegs<4>(k32, tid);
      else bitonicSortRegs<8>(k32, tid);
    } else {
      if (e == 1) bitonicSortRegs<1>(S.xchg, tid);
      else if (e == 2) bitonicSortRegs<2>(S.xchg, tid);
      else bitonicSortRegs<4>(S.xchg, tid);
    }
  }
  // node records in list order (global: the partial pass appends to them); the pending nodes of the partial pass -- the
  // multi-key depth-k nodes in creation order = reverse list order -- get their records in LDS, where the sorted order reads them
  int nPend = 0;
  {
    auto listNode = [&](int m, int& lo, int& hi, int& depth, int& mp) {
      if (use32) { const uint32_t v = k32[m]; mp = (int)(v & 0x1fffu); depth = k - (int)(v >> (okBits + 13)); }
      else { const u64 v = S.xchg[m]; mp = (int)(v & 0x7ffff); depth = OCT_DEPTH + 1 - (int)(v >> 59); }
      const uint32_t lh = S.nodeLH[mp];
      lo = (int)(lh & 0x7ffffu); hi = lo + (int)(lh >> 19);
    };
    for (int m = tid; m < M; m += OCT_T) {
      int lo, hi, depth, mp;
      listNode(m, lo, hi, depth, mp);
      S.nodeLo[m] = lo; S.nodeHi[m] = hi; S.nodeDepth[m] = (uint8_t)depth;
    }
    if (sPhase2) {
      const int chunk = (M + OCT_T - 1) / OCT_T;
      const int b = min(tid * chunk, M), e = min(b + chunk, M);
      int c = 0;
      for (int r = b; r < e; r++) {  // r = reversed list index
        int lo, hi, depth, mp;
        listNode(M - 1 - r, lo, hi, depth, mp);
        c += depth == k && hi - lo > 1;
      }
      int p = blockScanExcl(c, tid, ws, &nPend, false);  // (barrier behind the sort)
      if (nPend <= min(min(qCap, S.parCap), OCTBIG_PEND))
        for (int r = b; r < e; r++) {
          int lo, hi, depth, mp;
          listNode(M - 1 - r, lo, hi, depth, mp);
          if (depth == k && hi - lo > 1) {
            S.pNd[p] = M - 1 - r; S.pLo[p] = lo; S.pHiD[p] = (hi << 5) | depth; S.pUlx[p] = S.nodeUlx[mp];
            p++;
          }
        }
    }
  }
  if (tid == 0) { sSize = M; sFinish = 0; }
  __syncthreads();

  // ---- 5. partial pass(es), cpp:897-965 ---------------------------------------------------------------------------
  if (sPhase2) {
    int* pendB = S.pending + qCap;     // the multi-key children of a round, for the next one
    u64* sizedB = reinterpret_cast<u64*>(S.nodeLH);  // [OCTBIG_PEND]: the sorted keys (the list's table is dead)
    int* bnd = reinterpret_cast<int*>(S.nodes);      // [3 qCap]: the children's boundaries of the sorted pending nodes (global)
    static_assert(OCTBIG_NODES * 4 >= OCTBIG_PEND * 8, "the sorted pending keys take the place of the list nodes' table");
    if (nPend > min(min(qCap, S.parCap), OCTBIG_PEND)) {  // (the one-workgroup kernel has the one-lane replay for such a unit)
      if (tid == 0) *nOut = -2;
      return;
    }
    int nFront = 0;
    for (;;) {
      // (a) sort keys: count << 40 | UL.x << 20 | pending index, straight into the LDS buffer the replay works on
      for (int j = tid; j < nPend; j += OCT_T)
        S.xchg[j] = ((u64)((S.pHiD[j] >> 5) - S.pLo[j]) << 40) | ((u64)S.pUlx[j] << 20) | (u64)j;
      __syncthreads();
      // (b) std::sort (cpp:912): partition phase replayed; the final insertion sort is a stable sort, and the partition phase
      // leaves ranges of at most 16 keys that are ordered among themselves (every key of a range <= every key of the next), so a
      // key's place is its range's start plus its stable rank inside the range
      stdSortPartitionPhasePar(S.xchg, nPend, tid, S.parScr, ws, S.parCap, sizedB);
      __syncthreads();
      // (c) children of every pending node (in sorted order): a child starts where the divergence depth equals the node's depth
      // + 1 (at most three places).  The bytes of a node are scanned 64 at a time, all loads of a step in flight
      for (int j = tid; j < nPend; j += OCT_T) {
        const int jj = (int)(sizedB[j] & 0xfffff);
        const int lo = S.pLo[jj], hi = S.pHiD[jj] >> 5, pd = S.pHiD[jj] & 31;
        int b1 = hi, b2 = hi, b3 = hi, nb = 0;
        if (pd < OCT_DEPTH && hi - lo > 96) {
          // a large node (rare; its walk would set the phase's time): its keys are sorted by the digit of depth pd + 1, so the three
          // places where the digit changes are found by binary searches that run side by side
          const int sh = 2 * (OCT_DEPTH - (pd + 1)) - S.keyShift + 24;  // the digit inside a key (below 24: beyond the level's one-pixel depth, all 0)
          int lA = lo, hA = hi, lB = lo, hB = hi, lC = lo, hC = hi;
          while (lA < hA || lB < hB || lC < hC) {
            const int mA = (lA + hA) >> 1, mB = (lB + hB) >> 1, mC = (lC + hC) >> 1;
            const u64 kA = S.keys[min(mA, hi - 1)], kB = S.keys[min(mB, hi - 1)], kC = S.keys[min(mC, hi - 1)];
            const int qA = sh >= 24 ? (int)((kA >> sh) & 3) : 0, qB = sh >= 24 ? (int)((kB >> sh) & 3) : 0, qC = sh >= 24 ? (int)((kC >> sh) & 3) : 0;
            if (lA < hA) { if (qA >= 1) hA = mA; else lA = mA + 1; }
            if (lB < hB) { if (qB >= 2) hB = mB; else lB = mB + 1; }
            if (lC < hC) { if (qC >= 3) hC = mC; else lC = mC + 1; }
          }
          // (as the walk reports them: the boundaries that exist, in order, then hi)
          const int c1 = lA, c2 = lB, c3 = lC;
          int t1 = hi, t2 = hi, t3 = hi;
          if (c1 > lo && c1 < hi) t1 = c1;
          if (c2 > c1 && c2 < hi) { if (t1 == hi) t1 = c2; else t2 = c2; }
          if (c3 > c2 && c3 < hi) { if (t1 == hi) t1 = c3; else if (t2 == hi) t2 = c3; else t3 = c3; }
          b1 = t1; b2 = t2; b3 = t3;
        } else if (pd < OCT_DEPTH) {
          // branch-free: 32 bytes -> a 32-bit mask of the bytes equal to pd + 1 (inside a node none is smaller) -> its lowest
          // three set bits (a version with a branch per byte ran ~600 instructions per step through every lane's path)
          const uint32_t want = (uint32_t)(pd + 1) * 0x01010101u;
          for (int a0 = (lo + 1) & ~15; a0 < hi && nb < 3; a0 += 32) {  // two 16-byte loads in flight (most nodes need no more)
            const uint4 u0 = *reinterpret_cast<const uint4*>(S.div + a0);
            const uint4 u1 = *reinterpret_cast<const uint4*>(S.div + min(a0 + 16, (hi - 1) & ~15));
            const uint32_t w[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
            uint32_t hits = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
              const uint32_t x = w[q] ^ want;
              const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);  // bit 7 of every zero byte, exactly
              hits |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * q);
            }
            // positions a0 + e with lo < a0 + e < hi (the second load is a repeat when the node ends before it: masked by < hi)
            const int eLo = lo + 1 - a0, eHi = hi - a0;  // valid bits [max(eLo, 0), min(eHi, 32))
            const uint32_t mLo = eLo <= 0 ? 0xffffffffu : (eLo >= 32 ? 0u : ~((1u << eLo) - 1u));
            const uint32_t mHi = eHi >= 32 ? 0xffffffffu : ((1u << max(eHi, 0)) - 1u);
            uint32_t h = hits & mLo & mHi;
#pragma unroll
            for (int t = 0; t < 3; t++) {
              const bool take = h != 0u && nb < 3;
              const int pos = a0 + (int)__builtin_ctz(h | 0x80000000u);
              b1 = (take && nb == 0) ? pos : b1;
              b2 = (take && nb == 1) ? pos : b2;
              b3 = (take && nb == 2) ? pos : b3;
              nb += take ? 1 : 0;
              h &= h - 1u;
            }
          }
        }
        int nch = 1, nmulti = 1;
        if (pd < OCT_DEPTH) {
          nch = (b1 > lo) + (b2 > b1) + (b3 > b2) + (hi > b3);
          nmulti = (b1 - lo > 1) + (b2 - b1 > 1) + (b3 - b2 > 1) + (hi - b3 > 1);
        }
        S.childCnt[j] = nch | (nmulti << 8);
        bnd[3 * j] = b1; bnd[3 * j + 1] = b2; bnd[3 * j + 2] = b3;
      }
      __syncthreads();
      // (d) cut point: nodes are split from the back of the sorted array until the list holds N nodes
      {
        // growth of the list when the last t+1 sorted nodes are split: inclusive prefix over t = nPend-1-j
        const int prevSize = sSize;
        const int chunk = (nPend + OCT_T - 1) / OCT_T;
        const int b = min(tid * chunk, nPend), e = min(b + chunk, nPend);
        int c = 0;
        for (int t = b; t < e; t++) c += (S.childCnt[nPend - 1 - t] & 0xff) - 1;
        int totalGrowth;
        int acc = blockScanExcl(c, tid, ws, &totalGrowth, false);  // (barrier behind (c))
        if (tid == 0) { sCut = 0; sSize = prevSize + totalGrowth; sFinish = (totalGrowth == 0 || prevSize + totalGrowth >= N) ? 1 : 0; }
        __syncthreads();
        // growth is >= 0 per split, so the first t whose inclusive sum reaches N - prevSize is unique: that thread reports
        for (int t = b; t < e; t++) {
          const int before = acc;
          acc += (S.childCnt[nPend - 1 - t] & 0xff) - 1;
          if (prevSize + before < N && prevSize + acc >= N) { sCut = nPend - 1 - t; sSize = prevSize + acc; sFinish = 1; }
        }
      }
      __syncthreads();
      const int cut = sCut, finish = sFinish;
      // (e) create the children: processing order t = nPend-1-j; children are push_front'ed in quadrant order
      int totM;
      {
        const int nProc = nPend - cut;
        const int chunk = (nProc + OCT_T - 1) / OCT_T;
        const int b = min(tid * chunk, nProc), e = min(b + chunk, nProc);
        int cc = 0, cm = 0;
        for (int t = b; t < e; t++) {
          const int v = S.childCnt[nPend - 1 - t];
          cc += v & 0xff;
          cm += v >> 8;
        }
        // both counts in one scan: at most 4 children per processed node, nProc <= qCap
        int totC, offC, offM;
        if (4 * nProc < 65536) {
          int totCM;
          const int offCM = blockScanExcl(cc | (cm << 16), tid, ws, &totCM, false);  // (barrier behind (d))
          offC = offCM & 0xffff; offM = offCM >> 16; totC = totCM & 0xffff; totM = totCM >> 16;
        } else {
          offC = blockScanExcl(cc, tid, ws, &totC, false);
          offM = blockScanExcl(cm, tid, ws, &totM);
        }
        // (the multi-key children are listed only for another round; a finishing round may create up to N + 4 of them)
        if (nFront + totC > fCap || (!finish && totM > min(min(qCap, S.parCap), OCTBIG_PEND))) {  // the one-workgroup kernel gets the unit
          if (tid == 0) *nOut = -2;
          return;
        }
        for (int t = b; t < e; t++) {
          const int j = nPend - 1 - t;
          const int jj = (int)(sizedB[j] & 0xfffff);
          const int nd = S.pNd[jj], lo = S.pLo[jj], hi = S.pHiD[jj] >> 5, pd = S.pHiD[jj] & 31;
          if (pd >= OCT_DEPTH) {  // coincident keys: cannot be split further, stays one node
            const int id = mCap + nFront + offC++;
            S.nodeLo[id] = lo; S.nodeHi[id] = hi; S.nodeDepth[id] = (uint8_t)pd;
            if (!finish) pendB[offM++] = id;
          } else {
            const int bb[5] = {lo, bnd[3 * j], bnd[3 * j + 1], bnd[3 * j + 2], hi};
#pragma unroll
            for (int q = 0; q < 4; q++) {
              const int start = bb[q], end = bb[q + 1];
              if (end > start) {
                const int id = mCap + nFront + offC++;
                S.nodeLo[id] = start; S.nodeHi[id] = end; S.nodeDepth[id] = (uint8_t)(pd + 1);
                if (!finish && end - start > 1) pendB[offM++] = id;
              }
            }
          }
          S.nodeDepth[nd] = (uint8_t)(pd | 0x80);
        }
        nFront += totC;
      }
      __syncthreads();
      if (finish) break;
      // another round (rare: the first one did not reach N): the new pending nodes' records, from the global tables
      nPend = totM;
      for (int j = tid; j < nPend; j += OCT_T) {
        const int nd = pendB[j];
        const int lo = S.nodeLo[nd], depth = S.nodeDepth[nd];
        const u64 code = keyCode(S, lo);
        int ulx, uly, brx, bry;
        rootRect(L, (int)(code >> (2 * OCT_DEPTH)), ulx, uly, brx, bry);
        for (int d = 1; d <= depth; d++) {
          const int q = (int)((code >> (2 * (OCT_DEPTH - d))) & 3);
          const int halfX = (brx - ulx + 1) >> 1;
          if (q & 1) ulx += halfX; else brx = ulx + halfX;
        }
        S.pNd[j] = nd; S.pLo[j] = lo; S.pHiD[j] = (S.nodeHi[nd] << 5) | depth; S.pUlx[j] = (uint16_t)ulx;
      }
      __syncthreads();
    }
    if (tid == 0) sFront = nFront;
    __syncthreads();
  }
  // ---- 6. output: reverse(front alive) ++ list alive, the first `quota` of them -- as a list of key ranges: k_octree_emit finds
  //         every range's first key with the highest response (many workgroups: one CU's L1 takes ~4 cycles per scattered line,
  //         45 k cycles for the 1737 nodes of a 4K level 0) -------------------------------------------------------------------
  const int nFront = sFront;
  const int total = nFront + M;  // virtual sequence: pushed nodes in reverse push order, then the list
  {
    const int chunk = (total + OCT_T - 1) / OCT_T;
    const int b = min(tid * chunk, total), e = min(b + chunk, total);
    auto nodeAt = [&](int v) { return v < nFront ? mCap + (nFront - 1 - v) : v - nFront; };
    int c = 0;
    for (int v = b; v < e; v++) c += (S.nodeDepth[nodeAt(v)] & 0x80) ? 0 : 1;
    int alive;
    int p = blockScanExcl(c, tid, ws, &alive, false);  // (barrier above)
    int* emitList = S.pending;  // [N <= qCap]: lo | (hi - lo) << 19
    for (int v = b; v < e && p < N; v++) {
      const int nd = nodeAt(v);
      if (!(S.nodeDepth[nd] & 0x80)) {
        const int lo = S.nodeLo[nd];
        emitList[p++] = lo | ((S.nodeHi[nd] - lo) << 19);
      }
    }
    if (tid == 0) *nOut = min(alive, N);
  }
}
#endif  // OCT_T >= 1024

// One (frame, level) unit on the global-scratch layout (octScratchBytes()); `xchg` = xchgCap u64 of LDS for the sorts (at least
// 1024: the register sort of a workgroup's worth of padded keys, the radix sort's 256 x nWaves digit counters and the parallel
// std::sort replay's scratch all live in it; the callers static_assert that).
// Scratch of unit (f, level) starts at scrOff[level] + f * scrStride[level].
__device__ __forceinline__ void octreeGlobalUnit(const uint32_t* __restrict__ cand, const int* __restrict__ cellCount, const OctLaunch& P,
                                 SelKp* __restrict__ selStage, int* __restrict__ nselLevel, uint8_t* __restrict__ scratch,
                                 int level, int f, u64* xchg, int xchgCap, uint32_t* parScr, int parCap,
                                 uint32_t* radixCnt2 = nullptr) {
  __shared__ int gws[OCT_T / 64];
  int* nOut = &nselLevel[f * P.nlevels + level];
  // (capacities from the quota, or from the number of roots when that is larger: the first pass splits every root)
  const int nMax = P.scrNMax[level], qMax = max(max(P.lev[level].quota, P.lev[level].nIni), 1);
  size_t nPad = 1024;  // (= octScratchBytes; at least the largest workgroup size)
  while ((int)nPad < nMax) nPad <<= 1;
  const int mCap = 4 * qMax, fCap = 16 * qMax;
  size_t mPad = 1024;
  while ((int)mPad < mCap) mPad <<= 1;
  uint8_t* p = scratch + P.scrOff[level] + (int64_t)f * P.scrStride[level];
  OctScratch S;
  S.keys = (u64*)p; p += nPad * 8;
  {
    const int D = P.lev[level].depthBits;
    S.keyShift = (D >= 1 && D <= OCT_DEPTH) ? 2 * (OCT_DEPTH - D) : 0;
  }
  S.nodes = (u64*)p; p += mPad * 8;
  S.sized = (u64*)p; p += (size_t)2 * qMax * 8;
  S.hiOf = (int*)p; p += nPad * 4;
  S.nodeLo = (int*)p; p += (size_t)(mCap + fCap) * 4;
  S.nodeHi = (int*)p; p += (size_t)(mCap + fCap) * 4;
  S.pending = (int*)p; p += (size_t)2 * qMax * 4;
  S.childCnt = (int*)p; p += (size_t)qMax * 4;
  p = (uint8_t*)(((uintptr_t)p + 15) & ~(uintptr_t)15);  // (= octCarve)
  S.div = p; p += nPad + 8;
  p += nPad + 8;  // (formerly alone[]: the layout, and with it octScratchBytes on the host, is unchanged)
  S.nodeDepth = p; p += (size_t)(mCap + fCap + 8);
  p += (size_t)(mCap + fCap + 8);  // (formerly nodeAlive[]: the layout, and with it octScratchBytes on the host, is unchanged)
  p = (uint8_t*)(((uintptr_t)p + 15) & ~(uintptr_t)15);
  uint32_t* candBuf = (uint32_t*)p;  // [nPad] positions of the unit's candidates
  p += nPad * 4;
  S.sortTmp = (u64*)p;               // [nPad] (p stays 16-byte aligned: nPad is a multiple of 256)
  S.segBase = cand + P.candOff[level] + (int64_t)f * P.candCap[level];
  const int n = gatherCandidates(cellCount + (int64_t)f * P.nCellsTotal + P.lev[level].cellBase, P.lev[level].nCells,
                                 P.lev[level].segCap, candBuf, nMax, threadIdx.x, gws);
  if (n > nMax) {  // more candidates than the selection stage can index (2^19 - 1)
    if (threadIdx.x == 0) *nOut = -1;
    return;
  }
  S.cand = candBuf;
  S.xchg = xchg;
  S.xchgCap = xchgCap;
  // scratch of the parallel std::sort replay: the caller's (k_octree_global: 2048 keys), else the sort exchange buffer, which
  // is idle during the partition phase (512 keys)
  S.parScr = parScr ? parScr : reinterpret_cast<uint32_t*>(xchg);
  S.parCap = parScr ? parCap : OCT_PAR_MAX;
  S.radixCnt2 = radixCnt2;
  S.candE = candBuf;  // (every entry of the position list is read by the thread that overwrites it)
  S.ceBuf = reinterpret_cast<uint32_t*>(S.sortTmp);  // step 6 only: free since the partial pass's stable sort
  octreeSelect(S, n, P.lev[level], P.codeTab, level, selStage + (int64_t)f * P.selStride + P.selOff[level], nOut, mCap, fCap, qMax);
  __syncthreads();
  if (threadIdx.x == 0 && *nOut == -2) *nOut = -1;  // even the large scratch was too small: hard error
}
