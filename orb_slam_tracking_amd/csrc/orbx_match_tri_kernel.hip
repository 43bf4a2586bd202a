// orbx_match_tri_kernel.hip — LocalMapping::CreateNewMapPoints for a batch of (KF1, KF2) keyframe pairs (include/orbx.h, "growing
// the map"): ORBmatcher::SearchForTriangulation, then the triangulation of its matches with the gates on parallax, depth,
// reprojection error and scale.  gfx950.  The arithmetic is orbx_tri_math.inc, which the CPU restatement compiles too.
//
// k_match_tri has k_match_bow's shape: one workgroup of MB_WAVES waves per pair; the nodes the two FeatureVectors share are
// independent of each other and go to the waves in turn; inside a node KF1's features are a sequential chain (a later one does
// not see the KF2 features an earlier one took), so a wave walks them one after the other and spreads the node's KF2 features
// over its lanes.  The walk's `d > bestDist` with a non-strict test means: of the candidates that pass the two geometric tests,
// the smallest distance, and among equals the LAST one -- a maximum over ((64 - d) << 16 | position), which needs no order.
//
// k_triangulate: a lane per KF1 feature, TT_THREADS features per workgroup, capacity / TT_THREADS workgroups per pair, so that a
// pair spreads over several CUs.  The 4x4 Jacobi is a long f64 chain per lane (as in k_check_rt); the lanes without a match only
// clear their entries.  The counters are integer sums: a workgroup adds its own to the pair's record, in any order.
#include <hip/hip_runtime.h>

#include "orbx_launch.h"
#include "orbx_match_hist.h"
#include "orbx_match_node.h"

#define ORBX_TRI_FN __device__
#include "orbx_tri_math.inc"

namespace orbx {
namespace {

using namespace orbx_tri;

constexpr int MT_TAKEN_WORDS = BOW_MAX_FEATURES / 32;  // a node holds at most a whole frame

struct MtCounters {
  int made, queries, withCand, epipole, epiline, bad;  // (epipole, epiline: the lane's own; the others wave-uniform)
};

// One node by one wave: KF1's FeatureVector entries [a0, a1) against KF2's [b0, b1).  A KF2 feature is named by its position p in
// [0, nb): positions ascend with the feature index.
// Nothing the chain of KF1 features waits for comes from memory: the wave loads 64 KF1 features at a time, one per lane (index,
// descriptor, epipolar line, angle), and the chain takes them from the lanes' registers one after the other; a node of up to 64 KF2
// features stays in registers too (one per lane: descriptor, position, octave, angle, index, and its own "taken" flag), so that a
// step of the chain is eight popcounts, the two tests and a shuffle tree.  A larger node is walked in chunks of 64 per KF1
// feature from memory, with `taken` the wave's bit set over the positions in LDS; EVERY lane writes every update of it (the same
// value to the same word), so that a lane only ever reads what it wrote itself.
__device__ void mtNode(const int lane, const uint32_t* __restrict__ aFeat, const int a0, const int a1,
                       const uint32_t* __restrict__ bFeat, const int b0, const int b1, const uint4* __restrict__ desc1,
                       const uint4* __restrict__ desc2, const orbx_keypoint* __restrict__ kps1,
                       const orbx_keypoint* __restrict__ kps2, const uint8_t* __restrict__ mask1, const uint8_t* __restrict__ mask2,
                       const int n1, const int n2, const int nLevels, const bool checkOri, const PairGeom* g, const float* epiThr,
                       const float* lineThr, int* __restrict__ m12, volatile uint32_t* taken, int* hist, MtCounters& ct) {
  const int nb = b1 - b0;
  const bool cached = nb <= 64;
  uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0;
  float cX = 0.0f, cY = 0.0f, cAng = 0.0f;
  int cOct = 0, cJ = 0;
  bool cOk = false;  // (in the cached form it also goes false when the lane's feature is taken)
  if (cached) {
    if (lane < nb) {
      const uint32_t j = bFeat[b0 + lane];
      cOk = j < (uint32_t)n2 && !(mask2 && mask2[j] != 0);  // (an entry that names no feature of KF2 is skipped)
      if (cOk) {
        const orbx_keypoint k = kps2[j];
        c0 = desc2[(size_t)j * 2]; c1 = desc2[(size_t)j * 2 + 1];
        cX = k.x; cY = k.y; cOct = k.octave; cAng = k.angle; cJ = (int)j;
      }
    }
  } else {
    const int words = (nb + 31) >> 5;
    for (int k = 0; k < words; k++) taken[k] = 0;
  }
  const float ex = g->ex, ey = g->ey;
  for (int base = a0; base < a1; base += 64) {
    // this chunk's KF1 features, one per lane
    uint32_t myI = 0;
    uint4 my0 = make_uint4(0, 0, 0, 0), my1 = my0;
    float myAbc[3] = {0.0f, 0.0f, 0.0f}, myAng = 0.0f;
    bool myOk = false;
    if (base + lane < a1) {
      myI = aFeat[base + lane];
      myOk = myI < (uint32_t)n1 && !(mask1 && mask1[myI] != 0);
      if (myOk) {
        const orbx_keypoint k = kps1[myI];
        my0 = desc1[(size_t)myI * 2]; my1 = desc1[(size_t)myI * 2 + 1];
        epipolarLine(g->F12, k.x, k.y, myAbc);
        myAng = k.angle;
      }
    }
    unsigned long long todo = __ballot(myOk);
    ct.queries += (int)__popcll(todo);
    while (todo) {  // (ascending lanes: the FeatureVector's order)
      const int src = __ffsll(todo) - 1;
      todo &= todo - 1;
      const uint32_t i = (uint32_t)__shfl((int)myI, src);
      uint4 q0, q1;
      q0.x = __shfl(my0.x, src); q0.y = __shfl(my0.y, src); q0.z = __shfl(my0.z, src); q0.w = __shfl(my0.w, src);
      q1.x = __shfl(my1.x, src); q1.y = __shfl(my1.y, src); q1.z = __shfl(my1.z, src); q1.w = __shfl(my1.w, src);
      const float abc[3] = {__shfl(myAbc[0], src), __shfl(myAbc[1], src), __shfl(myAbc[2], src)};
      uint32_t key = 0;  // the lane's best over its positions: (64 - d) << 16 | position, 0 = none
      bool any = false;
      for (int p = lane; p < nb; p += 64) {
        uint4 f0, f1;
        float x2, y2;
        int oct;
        if (cached) {
          if (!cOk) continue;
          f0 = c0; f1 = c1; x2 = cX; y2 = cY; oct = cOct;
        } else {
          if ((taken[p >> 5] >> (p & 31)) & 1u) continue;
          const uint32_t j = bFeat[b0 + p];
          if (j >= (uint32_t)n2) continue;
          if (mask2 && mask2[j] != 0) continue;
          f0 = desc2[(size_t)j * 2]; f1 = desc2[(size_t)j * 2 + 1];
          x2 = kps2[j].x; y2 = kps2[j].y; oct = kps2[j].octave;
        }
        const int d = mbDistance(q0, q1, f0, f1);
        if (d > MATCH_TH_LOW) continue;
        any = true;
        if ((uint32_t)oct >= (uint32_t)nLevels) { ct.bad = 1; continue; }
        const int verdict = candidateTest(ex, ey, abc, x2, y2, epiThr[oct], lineThr[oct]);
        if (verdict == 1) ct.epipole++;
        else if (verdict == 2) ct.epiline++;
        else {
          const uint32_t k = ((uint32_t)(64 - d) << 16) | (uint32_t)p;
          key = k > key ? k : key;
        }
      }
      if (__any(any)) ct.withCand++;
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const uint32_t ok = (uint32_t)__shfl_xor((int)key, s);
        key = key > ok ? key : ok;
      }
      if (key != 0) {
        const int p = (int)(key & 0xffffu);
        int j;
        float ang2;
        if (cached) {  // (position p is lane p's)
          j = __shfl(cJ, p);
          ang2 = __shfl(cAng, p);
          if (lane == p) cOk = false;
        } else {
          j = (int)bFeat[b0 + p];  // (< n2: it was a candidate)
          ang2 = kps2[j].angle;
          taken[p >> 5] = taken[p >> 5] | (1u << (p & 31));
        }
        const float ang1 = __shfl(myAng, src);
        ct.made++;
        if (lane == 0) {
          m12[i] = j;
          if (checkOri) {
            const int bin = matchRotBin(ang1, ang2);
            if (bin >= 0) atomicAdd(&hist[bin], 1);
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(MB_THREADS) void k_match_tri(MatchTriArgs a) {
  __shared__ uint32_t sTaken[MB_WAVES][MT_TAKEN_WORDS];
  __shared__ int hist[MATCH_HISTO_LENGTH];
  __shared__ int sCt[6], sKeep[3], sKeepV[3], sRemoved;
  __shared__ PairGeom sG;
  __shared__ float sEpiThr[ORBX_MAX_LEVELS], sLineThr[ORBX_MAX_LEVELS];
  __shared__ int sRefused, sBadMedian;
  const int pair = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int f1 = a.pairs[pair], f2 = a.pairs[a.nPairs + pair];
  const size_t off1 = (size_t)f1 * a.cap, off2 = (size_t)f2 * a.cap;
  const int rn1 = a.n[f1], rn2 = a.n[f2], rA = a.fvN[f1], rB = a.fvN[f2];
  const int n1 = mbClamp(rn1, a.cap), n2 = mbClamp(rn2, a.cap), nA = mbClamp(rA, a.cap), nB = mbClamp(rB, a.cap);
  const bool clamped = n1 != rn1 || n2 != rn2 || nA != rA || nB != rB;
  const uint32_t* __restrict__ aNode = a.fvNode + off1;
  const uint32_t* __restrict__ aFeat = a.fvFeat + off1;
  const uint32_t* __restrict__ bNode = a.fvNode + off2;
  const uint32_t* __restrict__ bFeat = a.fvFeat + off2;
  const orbx_keypoint* __restrict__ kps1 = a.kps + off1;
  const orbx_keypoint* __restrict__ kps2 = a.kps + off2;
  int* __restrict__ m12 = a.matches12 + (size_t)pair * a.cap;

  for (int i = t; i < a.cap; i += MB_THREADS) m12[i] = -1;
  if (t < MATCH_HISTO_LENGTH) hist[t] = 0;
  if (t < 3) { sKeep[t] = -1; sKeepV[t] = 0; }
  if (t < 6) sCt[t] = 0;
  if (t < ORBX_MAX_LEVELS) {
    sEpiThr[t] = 100.0f * a.cam.scale[t];
    sLineThr[t] = 3.84f * a.cam.sigma2[t];
  }
  if (t == 0) {
    sRemoved = 0;
    sBadMedian = 0;
    pairGeometry(a.pose + (size_t)f1 * 12, a.pose + (size_t)f2 * 12, a.cam.fx, a.cam.fy, a.cam.cx, a.cam.cy, &sG);
    int refused = 0;
    if (sG.nonfinite) refused = ORBX_TRI_NONFINITE;
    else if (sG.baseline == 0.0f) {
      refused = ORBX_TRI_ZERO_BASELINE;
      for (int k = 0; k < 9; k++) sG.F12[k] = 0.0f;
      sG.ex = sG.ey = 0.0f;
    } else if (a.medianDepth) {  // (a median that is no positive number is garbage: flagged, no gate)
      const float median = a.medianDepth[f2];
      if (!(median > 0.0f) || !isFinite(median)) sBadMedian = 1;
      else if (sG.baseline / median < 0.01f) refused = ORBX_TRI_LOW_BASELINE;
    }
    sRefused = refused;
  }
  __syncthreads();

  if (sRefused == 0) {  // (uniform)
    // the runs of KF1's FeatureVector, 64 entries at a time per wave: a lane that sits on the first entry of a run looks the run's
    // node up in KF2's FeatureVector (both ends at once); the wave then takes the nodes found one after the other.  A run ends at
    // the next run's first entry -- a ballot -- or, when it reaches the end of the 64 entries, where a probe of the entries
    // behind them says (64 at a time): no search per node.
    MtCounters ct{};
    for (int c = w * 64; c < nA; c += MB_THREADS) {
      const int i = c + lane;
      uint32_t node = 0;
      int lb = 0, ub = 0;
      bool first = false;
      if (i < nA) {
        node = aNode[i];
        first = i == 0 || aNode[i - 1] != node;
      }
      const unsigned long long firsts = __ballot(first);
      bool start = false;
      if (first) {
        mbRange(bNode, nB, node, &lb, &ub);
        start = lb < ub;
      }
      unsigned long long m = __ballot(start);
      while (m) {
        const int src = __ffsll(m) - 1;
        m &= m - 1;
        const uint32_t nd = (uint32_t)__shfl((int)node, src);
        const int a0 = c + src, b0 = __shfl(lb, src), b1 = __shfl(ub, src);
        const unsigned long long above = firsts & ~((2ull << src) - 1ull);
        int a1;
        if (above) a1 = c + __ffsll(above) - 1;
        else {
          a1 = min(c + 64, nA);
          while (a1 < nA) {
            const unsigned long long same = __ballot(a1 + lane < nA && aNode[a1 + lane] == nd);
            const int run = same == ~0ull ? 64 : __ffsll(~same) - 1;
            a1 += run;
            if (run < 64) break;
          }
        }
        mtNode(lane, aFeat, a0, a1, bFeat, b0, b1, (const uint4*)a.desc + off1 * 2, (const uint4*)a.desc + off2 * 2, kps1, kps2,
               a.mask ? a.mask + off1 : nullptr, a.mask ? a.mask + off2 : nullptr, n1, n2, a.cam.nLevels, a.checkOri != 0, &sG,
               sEpiThr, sLineThr, m12, sTaken[w], hist, ct);
      }
    }
    // the lanes' own counts summed over the wave; the wave-uniform ones once
    int epi = ct.epipole, line = ct.epiline, bad = ct.bad;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      epi += __shfl_xor(epi, s);
      line += __shfl_xor(line, s);
      bad |= __shfl_xor(bad, s);
    }
    if (lane == 0) {
      if (ct.made) atomicAdd(&sCt[0], ct.made);
      if (ct.queries) atomicAdd(&sCt[1], ct.queries);
      if (ct.withCand) atomicAdd(&sCt[2], ct.withCand);
      if (epi) atomicAdd(&sCt[3], epi);
      if (line) atomicAdd(&sCt[4], line);
      if (bad) atomicOr(&sCt[5], 1);
    }
    __syncthreads();

    if (a.checkOri) {  // (uniform)
      if (t < MATCH_HISTO_LENGTH) {
        const int v = hist[t], place = matchHistPlace(hist, t);
        if (v > 0 && place < 3) { sKeep[place] = t; sKeepV[place] = v; }
      }
      __syncthreads();
      const int ind1 = sKeep[0];
      int ind2 = sKeep[1], ind3 = sKeep[2];
      matchDropMaxima(sKeepV[0], sKeepV[1], sKeepV[2], &ind2, &ind3);
      // a match's bin is a function of the match: recomputed here from the two angles instead of kept in a list per bin
      int dropped = 0;
      for (int i = t; i < n1; i += MB_THREADS) {
        const int j = m12[i];
        if (j < 0) continue;
        const int bin = matchRotBin(kps1[i].angle, kps2[j].angle);
        if (bin >= 0 && bin != ind1 && bin != ind2 && bin != ind3) {
          m12[i] = -1;
          dropped++;
        }
      }
      if (dropped) atomicAdd(&sRemoved, dropped);
      __syncthreads();
    }
  }
  if (t == 0) {
    orbx_tri_match_result r;
    r.status = sRefused | ((clamped || sCt[5] || sBadMedian) ? ORBX_TRI_BAD_INPUT : 0);
    r.nmatches = sCt[0] - sRemoved;
    r.n_queries = sCt[1];
    r.n_with_candidates = sCt[2];
    r.n_epipole_rejected = sCt[3];
    r.n_epiline_rejected = sCt[4];
    r.n_rot_removed = sRemoved;
    r.baseline = sG.baseline;
    r.ex = sG.ex;
    r.ey = sG.ey;
    for (int k = 0; k < 9; k++) r.F12[k] = sG.F12[k];
    a.res[pair] = r;
  }
}

// counters of k_triangulate in the order of orbx_tri_result behind its status: n_matches, n_points, then one per gate
constexpr int TT_COUNTERS = 10;

__global__ __launch_bounds__(TT_THREADS) void k_triangulate(TriangulateArgs a) {
  __shared__ int sCt[TT_COUNTERS], sStatus;
  __shared__ float sScale[ORBX_MAX_LEVELS], sTh[ORBX_MAX_LEVELS];
  const int chunks = (a.cap + TT_THREADS - 1) / TT_THREADS;
  const int pair = blockIdx.x / chunks, t = threadIdx.x, i = (blockIdx.x % chunks) * TT_THREADS + t;
  const int f1 = a.pairs[pair], f2 = a.pairs[a.nPairs + pair];
  const size_t off1 = (size_t)f1 * a.cap, off2 = (size_t)f2 * a.cap, row = (size_t)pair * a.cap;
  const int rn1 = a.n[f1], rn2 = a.n[f2];
  const int n1 = mbClamp(rn1, a.cap), n2 = mbClamp(rn2, a.cap);
  if (t < TT_COUNTERS) sCt[t] = 0;
  if (t == 0) sStatus = 0;
  if (t < ORBX_MAX_LEVELS) {
    sScale[t] = a.cam.scale[t];
    sTh[t] = 5.991f * a.cam.sigma2[t];
  }
  __syncthreads();
  // (uniform addresses: every lane holds the two poses)
  float p1[12], p2[12];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    p1[k] = a.pose[(size_t)f1 * 12 + k];
    p2[k] = a.pose[(size_t)f2 * 12 + k];
    finite = finite && isFinite(p1[k]) && isFinite(p2[k]);
  }
  int status = (n1 != rn1 || n2 != rn2) ? ORBX_TRI_BAD_INPUT : 0;
  if (!finite) status |= ORBX_TRI_NONFINITE;
  int outcome = 0;
  TriPoint pt{};
  if (finite && i < n1) {
    const int j = a.matches12[row + i];
    if (j >= 0) {
      const orbx_keypoint k1 = a.kps[off1 + i];
      if (j >= n2 || (uint32_t)k1.octave >= (uint32_t)a.cam.nLevels) status |= ORBX_TRI_BAD_INPUT;
      else {
        const orbx_keypoint k2 = a.kps[off2 + j];
        if ((uint32_t)k2.octave >= (uint32_t)a.cam.nLevels) status |= ORBX_TRI_BAD_INPUT;
        else {
          float Ow1[3], Ow2[3];
          cameraCentre(p1, Ow1);
          cameraCentre(p2, Ow2);
          const int nl = a.cam.nLevels;
          outcome = triangulate(p1, p2, Ow1, Ow2, a.cam.fx, a.cam.fy, a.cam.cx, a.cam.cy, k1.x, k1.y, k2.x, k2.y,
                                sTh[k1.octave], sTh[k2.octave], sScale[k1.octave], sScale[k2.octave], 1.5f * a.cam.scaleFactor,
                                sScale[nl - 1], &pt);
        }
      }
    }
  }
  if (i < a.cap) {
    const bool kept = outcome == TRI_KEPT;
    a.pointMask[row + i] = kept ? 1 : 0;
    float* P = a.points + (row + i) * 3;
    float* N = a.pointNormal + (row + i) * 3;
    float* D = a.pointDist + (row + i) * 2;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      P[k] = kept ? pt.X[k] : 0.0f;
      N[k] = kept ? pt.normal[k] : 0.0f;
    }
    D[0] = kept ? pt.minDist : 0.0f;
    D[1] = kept ? pt.maxDist : 0.0f;
  }
  // the workgroup's counts: a ballot per outcome and wave, then one add per counter to the pair's record
  if (__any(outcome != 0)) {
    const unsigned long long all = __ballot(outcome != 0);
    if ((t & 63) == 0) atomicAdd(&sCt[0], (int)__popcll(all));
#pragma unroll
    for (int o = TRI_KEPT; o <= TRI_SCALE; o++) {
      const unsigned long long m = __ballot(outcome == o);
      if ((t & 63) == 0 && m) atomicAdd(&sCt[o], (int)__popcll(m));
    }
  }
  if (__any(status != 0)) {
    int s = status;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) s |= __shfl_xor(s, k);
    if ((t & 63) == 0) atomicOr(&sStatus, s);
  }
  __syncthreads();
  int32_t* r = reinterpret_cast<int32_t*>(a.res + pair);
  if (t == 0 && sStatus) atomicOr(&r[0], sStatus);
  if (t < TT_COUNTERS && sCt[t]) atomicAdd(&r[1 + t], sCt[t]);
}

static_assert(sizeof(orbx_tri_result) == (1 + TT_COUNTERS) * 4 && TRI_SCALE == TT_COUNTERS - 1, "k_triangulate's counters are orbx_tri_result's");

}  // namespace

hipError_t launch_match_tri(hipStream_t st, const MatchTriArgs& a) {
  hipLaunchKernelGGL(k_match_tri, dim3((unsigned)a.nPairs), dim3(MB_THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_triangulate(hipStream_t st, const TriangulateArgs& a) {
  const hipError_t e = hipMemsetAsync(a.res, 0, (size_t)a.nPairs * sizeof(orbx_tri_result), st);
  if (e != hipSuccess) return e;
  const long long blocks = (long long)((a.cap + TT_THREADS - 1) / TT_THREADS) * a.nPairs;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_triangulate, dim3((unsigned)blocks), dim3(TT_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
