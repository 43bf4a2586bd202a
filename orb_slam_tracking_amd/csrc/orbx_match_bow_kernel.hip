// orbx_match_bow_kernel.hip — ORBmatcher::SearchByBoW for a batch of (keyframe, frame) pairs (include/orbx.h, "matching
// through the FeatureVector"): matches restricted to features under the same vocabulary node.  gfx950.
//
// One workgroup of MB_WAVES waves per pair.  A feature belongs to one node, so the nodes the two FeatureVectors share are
// independent of each other and go to the waves in turn; inside a node the keyframe's features are a sequential chain (a later
// one does not see the frame features an earlier one took), so a wave walks them one after the other and spreads the node's
// frame features over its lanes.  Integer arithmetic apart from the ratio test and the rotation bin; no float atomics.
#include <hip/hip_runtime.h>

#include "orbx_launch.h"
#include "orbx_match_hist.h"
#include "orbx_match_node.h"

namespace orbx {
namespace {

constexpr uint32_t MB_NONE = (256u << 16) | 0xffffu;  // distance 256 (best1 = best2 = 256 at the start), no position
constexpr int MB_TAKEN_WORDS = BOW_MAX_FEATURES / 32;  // a node holds at most a whole frame

// One node by one wave: the keyframe's FeatureVector entries [a0, a1) against the frame's [b0, b1).  A frame feature is named
// by its position p in [0, nb): positions ascend with the feature index, so the smallest (distance, position) is the lowest
// feature index attaining the smallest distance.  `taken` is the wave's bit set over the positions; EVERY lane writes every
// update of it (the same value to the same word), so that a lane only ever reads what it wrote itself.
// Up to 64 frame features stay in registers (one per lane) for the whole node; a larger node is walked in chunks of 64
// per keyframe feature.  Returns the matches made (wave-uniform).
__device__ int mbNode(const MatchBowArgs& a, const int lane, const uint32_t* __restrict__ aFeat, const int a0, const int a1,
                      const uint32_t* __restrict__ bFeat, const int b0, const int b1, const uint4* __restrict__ descK,
                      const uint4* __restrict__ descF, const orbx_keypoint* __restrict__ kpsK,
                      const orbx_keypoint* __restrict__ kpsF, const uint8_t* __restrict__ maskK, const int nK, const int nF,
                      int* __restrict__ mF, volatile uint32_t* taken, int* hist) {
  const int nb = b1 - b0;
  const int words = (nb + 31) >> 5;
  for (int k = 0; k < words; k++) taken[k] = 0;
  const bool cached = nb <= 64;
  uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0;
  bool cOk = false;
  if (cached && lane < nb) {
    const uint32_t j = bFeat[b0 + lane];
    cOk = j < (uint32_t)nF;  // (a pair that names no feature of the frame is skipped)
    if (cOk) { c0 = descF[(size_t)j * 2]; c1 = descF[(size_t)j * 2 + 1]; }
  }
  int made = 0;
  for (int ia = a0; ia < a1; ia++) {
    const uint32_t i = aFeat[ia];  // (wave-uniform)
    if (i >= (uint32_t)nK) continue;
    if (maskK && maskK[i] == 0) continue;
    const uint4 q0 = descK[(size_t)i * 2], q1 = descK[(size_t)i * 2 + 1];
    // the lane's own (best1 << 16 | position, best2) over its positions, in ascending position
    uint32_t key = MB_NONE;
    int second = 256;
    for (int p = lane; p < nb; p += 64) {
      if ((taken[p >> 5] >> (p & 31)) & 1u) continue;
      uint4 f0, f1;
      if (cached) {
        if (!cOk) continue;
        f0 = c0; f1 = c1;
      } else {
        const uint32_t j = bFeat[b0 + p];
        if (j >= (uint32_t)nF) continue;
        f0 = descF[(size_t)j * 2]; f1 = descF[(size_t)j * 2 + 1];
      }
      const int d = mbDistance(q0, q1, f0, f1);
      if (d < (int)(key >> 16)) { second = (int)(key >> 16); key = ((uint32_t)d << 16) | (uint32_t)p; }
      else if (d < second) second = d;
    }
    // the wave's: smallest key, and the second smallest distance counting duplicates
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t ok = (uint32_t)__shfl_xor((int)key, s);
      const int os = __shfl_xor(second, s);
      const int hi = (int)((key > ok ? key : ok) >> 16);
      second = min(min(second, os), hi);
      key = key < ok ? key : ok;
    }
    const int best1 = (int)(key >> 16);
    if (best1 <= MATCH_TH_LOW && (float)best1 < a.nnratio * (float)second) {
      const int p = (int)(key & 0xffffu);
      const uint32_t j = bFeat[b0 + p];  // (< nF: it was a candidate)
      taken[p >> 5] = taken[p >> 5] | (1u << (p & 31));
      made++;
      if (lane == 0) {
        mF[j] = (int)i;
        if (a.checkOri) {
          const int bin = matchRotBin(kpsK[i].angle, kpsF[j].angle);
          if (bin >= 0) atomicAdd(&hist[bin], 1);
        }
      }
    }
  }
  return made;
}

__global__ __launch_bounds__(MB_THREADS) void k_match_bow(MatchBowArgs a) {
  __shared__ uint32_t sTaken[MB_WAVES][MB_TAKEN_WORDS];
  __shared__ int hist[MATCH_HISTO_LENGTH];
  __shared__ int sNm, sKeep[3], sKeepV[3];
  const int pair = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int fk = a.pairs[pair], ff = a.pairs[a.nPairs + pair];
  const size_t offK = (size_t)fk * a.cap, offF = (size_t)ff * a.cap;
  const int nK = mbClamp(a.n[fk], a.cap), nF = mbClamp(a.n[ff], a.cap);
  const int nA = mbClamp(a.fvN[fk], a.cap), nB = mbClamp(a.fvN[ff], a.cap);
  const uint32_t* __restrict__ aNode = a.fvNode + offK;
  const uint32_t* __restrict__ aFeat = a.fvFeat + offK;
  const uint32_t* __restrict__ bNode = a.fvNode + offF;
  const uint32_t* __restrict__ bFeat = a.fvFeat + offF;
  const orbx_keypoint* __restrict__ kpsK = a.kps + offK;
  const orbx_keypoint* __restrict__ kpsF = a.kps + offF;
  int* __restrict__ mF = a.matchesF + (size_t)pair * a.cap;

  for (int j = t; j < nF; j += MB_THREADS) mF[j] = -1;
  if (t < MATCH_HISTO_LENGTH) hist[t] = 0;
  if (t < 3) { sKeep[t] = -1; sKeepV[t] = 0; }
  if (t == 0) sNm = 0;
  __syncthreads();

  // the runs of the keyframe's FeatureVector, 64 entries at a time per wave: a lane that sits on the first entry of a run looks
  // the run's node up in the frame's FeatureVector; the wave then takes the nodes found one after the other
  int made = 0;
  for (int c = w * 64; c < nA; c += MB_THREADS) {
    const int i = c + lane;
    uint32_t node = 0;
    int lb = 0;
    bool start = false;
    if (i < nA) {
      node = aNode[i];
      start = i == 0 || aNode[i - 1] != node;
    }
    if (start) {
      lb = mbBound(bNode, 0, nB, node, false);
      start = lb < nB && bNode[lb] == node;
    }
    unsigned long long m = __ballot(start);
    while (m) {
      const int src = __ffsll(m) - 1;
      m &= m - 1;
      const uint32_t nd = (uint32_t)__shfl((int)node, src);
      const int a0 = c + src, b0 = __shfl(lb, src);
      const int a1 = mbBound(aNode, a0 + 1, nA, nd, true), b1 = mbBound(bNode, b0 + 1, nB, nd, true);
      made += mbNode(a, lane, aFeat, a0, a1, bFeat, b0, b1, (const uint4*)a.desc + offK * 2, (const uint4*)a.desc + offF * 2, kpsK,
                     kpsF, a.mask ? a.mask + offK : nullptr, nK, nF, mF, sTaken[w], hist);
    }
  }
  if (lane == 0 && made) atomicAdd(&sNm, made);
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
    for (int j = t; j < nF; j += MB_THREADS) {
      const int i = mF[j];
      if (i < 0) continue;
      const int bin = matchRotBin(kpsK[i].angle, kpsF[j].angle);
      if (bin >= 0 && bin != ind1 && bin != ind2 && bin != ind3) {
        mF[j] = -1;
        dropped++;
      }
    }
    if (dropped) atomicSub(&sNm, dropped);
    __syncthreads();
  }
  if (t == 0) a.nmatches[pair] = sNm;
}

}  // namespace

hipError_t launch_match_bow(hipStream_t st, const MatchBowArgs& a) {
  hipLaunchKernelGGL(k_match_bow, dim3((unsigned)a.nPairs), dim3(MB_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
