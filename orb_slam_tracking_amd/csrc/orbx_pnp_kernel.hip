// orbx_pnp_kernel.hip — PnPsolver on the device (include/orbx.h, "behind SearchByBoW: PnP RANSAC"): EPnP inside RANSAC for a batch
// of independent problems, in three launches.
//
//   k_pnp_prep         wave per problem              the checks of the device data, the correspondences in ascending feature order
//                                                    (ballot + prefix), N and the two values of the host's table
//   k_pnp_hypotheses   lane per (problem, iteration) the four draws, the four-point EPnP, CheckInliers over the problem's N points
//   k_pnp_refine       wave per problem              iterate() resolved in iteration order: Refine over the inliers of each distinct
//                                                    best until one succeeds, then the result, the pose, the row and the flags
//
// All arithmetic is csrc/orbx_pnp_math.inc, shared with the CPU restatement; this file fixes who computes what and the order of
// Refine's sums.  EPnP's 12x12 eigenproblem is the register problem: the packed matrix (78 doubles) stays in registers, indexed
// with constants, and the eigenvector matrix V (144 doubles) lives in LDS, one double per lane and entry -- V[k][i] of lane l at
// (k * 12 + i) * 64 + l, so a wave's access to one entry is 64 consecutive doubles: 72 KB per wave, two one-wave workgroups per
// CU.  k_pnp_refine runs the small algebra in every lane on equal bits (the sums leave the same bits in every lane), so all
// control flow is wave-uniform without a broadcast, and a set's inlier bits are kept in LDS as one 64-bit word per 64
// correspondences that every lane writes with the same ballot.  f64 without contraction (-ffp-contract=off).
// Bounds: 12 sweeps, 5 Gauss-Newton steps, at most n_iter refines; every index is checked before it is followed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/orbx.h"
#include "orbx_launch.h"

#define ORBX_PNP_FN __device__
#include "orbx_pnp_math.inc"

namespace orbx {
using namespace orbx_pnp;

static_assert(sizeof(Corr) == PNP_CORR_BYTES && sizeof(Hyp) == PNP_HYP_BYTES && sizeof(Meta) == 16, "workspace records");
static_assert(PNP_MAX_CAPACITY == ORBX_BOW_MAX_FEATURES, "the bit sets are sized for the largest frame");

namespace {

constexpr int PNP_BIT_WORDS = PNP_MAX_CAPACITY / 64;

// the wave's sum of v in every lane, in the documented order
__device__ inline double waveSum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

__device__ inline Cam camOf(const PnpArgs& a) { return Cam{a.fu, a.fv, a.uc, a.vc}; }

// ---- k_pnp_prep: the constructor and SetRansacParameters ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pnp_prep(const PnpArgs a) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const size_t cap = (size_t)a.cap;
  const int frame = a.problems[p], set = a.problems[a.nProblems + p];  // (checked on the host)
  const orbx_keypoint* kps = a.kps + (size_t)frame * cap;
  const int32_t* match = a.match ? a.match + (size_t)p * cap : nullptr;
  const float* points = a.points + (size_t)set * cap * 3;
  const uint8_t* mask = a.mask ? a.mask + (size_t)set * cap : nullptr;
  Corr* corr = reinterpret_cast<Corr*>(a.corr) + (size_t)p * cap;
  int32_t* corrOf = a.corrOf + (size_t)p * cap;
  int n = a.nKps[frame];
  int bad = 0, nonfinite = 0;
  if (n < 0 || n > a.cap) {
    bad = 1;
    n = 0;
  }
  int N = 0;
  for (int j0 = 0; j0 < a.cap; j0 += 64) {
    const int j = j0 + lane;
    bool take = false;
    Corr c{};
    if (j < n) {
      int i = j;
      bool has = true;
      if (match) {
        i = match[j];
        if (i >= a.cap) bad = 1;
        has = i >= 0 && i < a.cap;
      }
      if (has && mask && mask[i] == 0) has = false;
      if (has) {
        const orbx_keypoint k = kps[j];
        if (k.octave < 0 || k.octave >= a.nLevels) {
          bad = 1;
        } else {
          c.X[0] = points[(size_t)i * 3]; c.X[1] = points[(size_t)i * 3 + 1]; c.X[2] = points[(size_t)i * 3 + 2];
          c.u = k.x; c.v = k.y;
          c.maxErr = a.sigma2[k.octave] * a.th2;
          c.j = j; c.i = i;
          if (finite32(c.X[0]) && finite32(c.X[1]) && finite32(c.X[2]) && finite32(c.u) && finite32(c.v)) take = true;
          else nonfinite = 1;
        }
      }
    }
    const unsigned long long m = __ballot(take);
    const int slot = N + __popcll(m & ((1ull << lane) - 1ull));
    if (take) corr[slot] = c;
    if (j < a.cap) corrOf[j] = take ? slot : -1;
    N += (int)__popcll(m);
  }
  const int status = (__any(bad) ? PNP_BAD_INPUT : 0) | (__any(nonfinite) ? PNP_NONFINITE : 0);
  if (status) N = 0;
  if (lane == 0) {
    Meta m;
    m.N = N;
    m.minInliers = a.table[2 * N];  // (N <= cap, the table's last entry)
    m.maxIts = a.table[2 * N + 1];
    m.status = status;
    reinterpret_cast<Meta*>(a.meta)[p] = m;
  }
}

// ---- k_pnp_hypotheses -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pnp_hypotheses(const PnpArgs a) {
  __shared__ double Vl[144 * 64];
  const int lane = threadIdx.x;
  const long long gid = (long long)blockIdx.x * 64 + lane;
  if (gid >= (long long)a.nProblems * a.nIter) return;  // (no barrier below)
  const int p = (int)(gid / a.nIter), it = (int)(gid % a.nIter);
  const Meta m = reinterpret_cast<const Meta*>(a.meta)[p];
  // what iterate() never runs is never read: a refused problem, bNoMore, iterations beyond mRansacMaxIts
  if (m.status != 0 || m.N < m.minInliers || it >= m.maxIts) return;
  const Corr* corr = reinterpret_cast<const Corr*>(a.corr) + (size_t)p * a.cap;
  Hyp* out = reinterpret_cast<Hyp*>(a.hyp) + gid;
  const Cam K = camOf(a);
  Hyp h{};
  int sel[4];
  if (!sampleFour(a.draws + gid * 4, m.N, sel)) {
    h.flags = HYP_BAD_DRAWS;
  } else {
    SeqOps ops;
#pragma unroll
    for (int i = 0; i < 4; i++) ops.p[i] = ptOf(corr[sel[i]]);
    const VStore V{Vl + lane, 64};
    double R[9], t[3];
    h.choice = computePose(ops, K, V, R, t);
    if (!poseFinite(R, t)) {
      h.flags = HYP_DEGENERATE;
    } else {
      int count = 0;
      for (int c = 0; c < m.N; c++) count += isInlier(R, t, corr[c], K) ? 1 : 0;
      h.count = count;
#pragma unroll
      for (int k = 0; k < 9; k++) h.R[k] = R[k];
#pragma unroll
      for (int k = 0; k < 3; k++) h.t[k] = t[k];
    }
  }
  *out = h;
}

// ---- k_pnp_refine ---------------------------------------------------------------------------------------------------------------
// CheckInliers by the wave: the set's bits (every lane stores the same word) and its size
__device__ inline int markInliers(const double* R, const double* t, const Corr* corr, int N, const Cam& K, unsigned long long* bits,
                                  int lane) {
  int total = 0;
  for (int c0 = 0; c0 < N; c0 += 64) {
    const int c = c0 + lane;
    const bool in = c < N && isInlier(R, t, corr[c], K);
    const unsigned long long m = __ballot(in);
    bits[c0 >> 6] = m;
    total += (int)__popcll(m);
  }
  return total;
}

// Refine's sums in the documented order: lane l adds its inliers l, l + 64, ... then the xor tree
struct WaveOps {
  const Corr* corr;
  const unsigned long long* bits;
  int N, lane, n, firstC;
  __device__ int count() const { return n; }
  __device__ Pt first() const { return ptOf(corr[firstC]); }
  template <int K, class F>
  __device__ __forceinline__ void sum(double* out, F f) const {
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = 0.0;
    for (int c = lane; c < N; c += 64)
      if ((bits[c >> 6] >> lane) & 1ull) f(ptOf(corr[c]), out);
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = waveSum(out[k]);
  }
};

__global__ __launch_bounds__(64) void k_pnp_refine(const PnpArgs a) {
  __shared__ double Vl[144 * 64];
  __shared__ unsigned long long bitsBest[PNP_BIT_WORDS], bitsRefined[PNP_BIT_WORDS];
  __shared__ double refined[12];  // Refine's pose while the iterations are resolved (every lane stores the same values)
  const int p = blockIdx.x, lane = threadIdx.x;
  const size_t cap = (size_t)a.cap;
  const Meta m = reinterpret_cast<const Meta*>(a.meta)[p];
  const Corr* corr = reinterpret_cast<const Corr*>(a.corr) + (size_t)p * cap;
  const int32_t* corrOf = a.corrOf + (size_t)p * cap;
  const Hyp* hyp = reinterpret_cast<const Hyp*>(a.hyp) + (size_t)p * a.nIter;
  const Cam K = camOf(a);
  const VStore V{Vl + lane, 64};

  int status = m.status;
  if (status == 0 && m.N < m.minInliers) status = PNP_FEW_POINTS;
  Outcome o{};
  o.foundIt = o.bestIt = -1;
  double R[9] = {0.0}, t[3] = {0.0};
  int choice = 0, nIn = 0;
  const unsigned long long* outBits = nullptr;
  if (status == 0) {
    const int nIts = a.nIter < m.maxIts ? a.nIter : m.maxIts;
    double *const Rr = refined, *const tr = refined + 9;
    int rChoice = 0, rCount = 0;
    resolveIterations(hyp, nIts, m.minInliers, [&](int best) {
      double Rb[9], tb[3];
      for (int k = 0; k < 9; k++) Rb[k] = hyp[best].R[k];
      for (int k = 0; k < 3; k++) tb[k] = hyp[best].t[k];
      const int nb = markInliers(Rb, tb, corr, m.N, K, bitsBest, lane);
      int firstC = 0;
      for (int w = 0; w * 64 < m.N; w++)
        if (bitsBest[w]) {
          firstC = w * 64 + (int)__builtin_ctzll(bitsBest[w]);
          break;
        }
      const WaveOps ops{corr, bitsBest, m.N, lane, nb, firstC};
      rChoice = computePose(ops, K, V, Rr, tr);
      if (!poseFinite(Rr, tr)) return false;
      rCount = markInliers(Rr, tr, corr, m.N, K, bitsRefined, lane);
      return rCount > m.minInliers;
    }, &o);
    if (o.badDraws) status |= PNP_BAD_DRAWS;
    if (o.refined) {
      for (int k = 0; k < 9; k++) R[k] = Rr[k];
      for (int k = 0; k < 3; k++) t[k] = tr[k];
      nIn = rCount;
      choice = rChoice;
      outBits = bitsRefined;
    } else if (o.bestIt >= 0 && o.nBestInliers >= m.minInliers) {
      for (int k = 0; k < 9; k++) R[k] = hyp[o.bestIt].R[k];
      for (int k = 0; k < 3; k++) t[k] = hyp[o.bestIt].t[k];
      nIn = markInliers(R, t, corr, m.N, K, bitsBest, lane);
      choice = hyp[o.bestIt].choice;
      outBits = bitsBest;
    }
  } else {
    o.itsRun = 0;
  }
  if (!outBits) status |= PNP_NO_POSE;

  // ---- the row and the flags: every entry is written ----
  int32_t* row = a.matchInliers + (size_t)p * cap;
  uint8_t* flags = a.inliers ? a.inliers + (size_t)p * cap : nullptr;
  for (int j = lane; j < a.cap; j += 64) {
    const int c = outBits ? corrOf[j] : -1;
    const bool in = c >= 0 && ((outBits[c >> 6] >> (c & 63)) & 1ull);
    row[j] = in ? corr[c].i : -1;
    if (flags) flags[j] = in ? 1 : 0;
  }
  // ---- the result (every lane holds it: lane 0 writes) ----
  if (lane == 0) {
    orbx_pnp_result* out = a.res + p;
    float* pose = a.pose + (size_t)p * 12;
    const bool counted = (status & (PNP_BAD_INPUT | PNP_NONFINITE)) == 0;
    out->status = status;
    out->n_correspondences = counted ? m.N : 0;
    out->min_inliers = m.minInliers;
    out->max_its = m.maxIts;
    out->its_run = o.itsRun;
    out->found_it = o.foundIt;
    out->best_it = o.bestIt;
    out->refined = o.refined;
    out->n_inliers = nIn;
    out->n_best_inliers = o.nBestInliers;
    out->n_refines = o.nRefines;
    out->n_degenerate = o.nDegenerate;
    out->beta_choice = outBits ? choice : 0;
    out->reserved = 0;
    for (int k = 0; k < 9; k++) {
      out->R[k] = outBits ? R[k] : 0.0;
      out->Tcw[k] = pose[k] = outBits ? (float)R[k] : 0.f;
    }
    for (int k = 0; k < 3; k++) {
      out->t[k] = outBits ? t[k] : 0.0;
      out->Tcw[9 + k] = pose[9 + k] = outBits ? (float)t[k] : 0.f;
    }
  }
}

}  // namespace

hipError_t launch_pnp_prep(hipStream_t st, const PnpArgs& a) {
  hipLaunchKernelGGL(k_pnp_prep, dim3(a.nProblems), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_pnp_hypotheses(hipStream_t st, const PnpArgs& a) {
  const long long lanes = (long long)a.nProblems * a.nIter;
  hipLaunchKernelGGL(k_pnp_hypotheses, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_pnp_refine(hipStream_t st, const PnpArgs& a) {
  hipLaunchKernelGGL(k_pnp_refine, dim3(a.nProblems), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
