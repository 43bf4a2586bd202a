// orbx_bow_terms.h — device helpers shared by orbx_bow_kernel.hip and orbx_db_kernel.hip: the per-word term of DBoW2's scorings
// (src/ScoringObject.cpp, include/DBoW2/TemplatedDatabase.h:615-1113), the database's final score and two lane helpers.  f64
// without contraction; divide and sqrt are the correctly rounded ones.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace orbx {

__device__ __forceinline__ int clampN(const int32_t* n, int f, int cap) {
  const int v = n[f];
  return v < 0 ? 0 : (v > cap ? cap : v);
}

__device__ __forceinline__ double readlaneF64(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(uint32_t)b, lane);
  const int hi = __builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
  return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}

// scoring: 0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE, 4 BHATTACHARYYA, 5 DOT_PRODUCT (3, KL, is not offered)
__device__ __forceinline__ double bowTermL1(double q, double d) { return fabs(q - d) - fabs(q) - fabs(d); }

// the term of one common word: q the query's value, d the entry's; binary: the vocabulary's weighting is BINARY (DOT_PRODUCT)
__device__ __forceinline__ double bowTerm(int scoring, int binary, double q, double d) {
  switch (scoring) {
    case 0: return bowTermL1(q, d);
    case 1: return -q * d;
    case 2: return q + d != 0.0 ? -q * d / (q + d) : 0.0;
    case 4: return sqrt(q * d);
    default: return binary ? 1.0 : q * d;
  }
}

// the score of a listed entry from the sum of its terms (applied after the list is cut)
__device__ __forceinline__ double dbFinalScore(int scoring, double raw) {
  switch (scoring) {
    case 0: return -raw / 2.0;
    case 1: return raw <= -1.0 ? 1.0 : 1.0 - sqrt(1.0 + raw);
    case 2: return -2. * raw;
    default: return raw;
  }
}

}  // namespace orbx
