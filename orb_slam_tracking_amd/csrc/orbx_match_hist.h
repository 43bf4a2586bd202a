// orbx_match_hist.h — the rotation histogram of ORBmatcher (Features/ORBmatcher.cpp:106-116, 152-183) as the matcher kernels
// compute it: a match's bin, a bin's place among the three maxima and the 0.1 rule, as k_match* of SearchForInitialization
// (orbx_kernels.hip) write them out in place; SearchByBoW's kernel (orbx_match_bow_kernel.hip) takes them from here.
#pragma once
#if defined(__HIPCC__)

namespace orbx {

constexpr int MATCH_TH_LOW = 50;        // ORBmatcher::TH_LOW
constexpr int MATCH_HISTO_LENGTH = 30;  // ORBmatcher::HISTO_LENGTH

// bin of a match whose query / train keypoints have these angles (:109-113, the corrected factor HISTO_LENGTH / 360.0f of :23);
// -1 where the reference asserts (:114): such a match joins no bin and is kept
__device__ __forceinline__ int matchRotBin(float angQ, float angT) {
  float rot = angQ - angT;
  if (rot < 0.0f) rot += 360.0f;
  int bin = (int)roundf(rot * (MATCH_HISTO_LENGTH / 360.0f));
  if (bin == MATCH_HISTO_LENGTH) bin = 0;
  if (bin < 0 || bin >= MATCH_HISTO_LENGTH) bin = -1;
  return bin;
}

// ComputeThreeMaxima (:152-175): its strict-greater cascade keeps the three largest bins by (size descending, index ascending)
// among the non-empty ones -- bin t's place is the number of bins that come before it in that order
__device__ __forceinline__ int matchHistPlace(const int* hist, int t) {
  const int v = hist[t];
  int place = 0;
  for (int i = 0; i < MATCH_HISTO_LENGTH; i++) {
    const int o = hist[i];
    place += (o > v) || (o == v && i < t);
  }
  return place;
}

// the 0.1 rule (:177-182) on the three maxima's sizes
__device__ __forceinline__ void matchDropMaxima(int max1, int max2, int max3, int* ind2, int* ind3) {
  if ((float)max2 < 0.1f * (float)max1) { *ind2 = -1; *ind3 = -1; }
  else if ((float)max3 < 0.1f * (float)max1) { *ind3 = -1; }
}

}  // namespace orbx
#endif
