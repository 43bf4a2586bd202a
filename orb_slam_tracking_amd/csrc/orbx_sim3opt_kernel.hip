// orbx_sim3opt_kernel.hip — Optimizer::OptimizeSim3 on the device (include/orbx.h, "loop closing: Sim3 optimisation"): g2o's
// Levenberg-Marquardt over one free 7-dof similarity and fixed points, numeric Jacobians, two rounds with the classification
// behind each.
//
//   k_sim3_optimize   wave (64 lanes) per problem, four problems per workgroup   the checks of the device data, both rounds, every
//                                                                                 iteration and trial, the row, the result
//
// k_pose's shape: a problem is 36 running sums over a few hundred correspondences and one 7x7 solve per trial, so it is given to
// one wave and the waves of a workgroup share nothing and never meet at a barrier.  Lane l walks the features l, l + 64, ... of
// KF1 in ascending order and keeps the sums in registers; a butterfly of six __shfl_xor steps leaves the same bits in every
// lane, those lane 0 would hold after the fold include/orbx.h documents.  Every lane then runs the 7x7 solve, the judgement of
// the trial and the round logic redundantly on those equal bits, so all control flow is wave-uniform without a broadcast.
// The fourteen perturbed estimates of a linearisation and their inverses depend on the estimate alone: lane k < 14 computes
// estimate k and its inverse and hands both over through the wave's own 1792 bytes of LDS, so a correspondence costs 30
// map-and-project evaluations per linearisation and 2 per trial.  A row entry is read and written by its own lane only; there
// is no workspace in HBM and no cache of edges (a correspondence is read again in every pass: seven dependent loads against
// some 2000 f64 operations of a linearisation).  All arithmetic and the round logic are in csrc/orbx_sim3opt_math.inc, shared
// with the CPU restatement; this file fixes who computes what and the order of the sums.  f64 without contraction
// (-ffp-contract=off).
// Bounds: 2 rounds x n_iterations x 10 trials; every index is checked before it is followed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/orbx.h"
#include "orbx_launch.h"

#define ORBX_BA_FN __device__
#define ORBX_S3O_UNIFORM(v) __builtin_amdgcn_readfirstlane(v)
#include "orbx_sim3opt_math.inc"

namespace orbx {
using namespace orbx_sim3opt;

static_assert(sizeof(orbx_sim3opt_result) == 208, "orbx_sim3opt_result layout");
static_assert(sizeof(Sim3) == 64, "a perturbed estimate in LDS");
static_assert(SIM3OPT_MAX_CAPACITY == ORBX_BOW_MAX_FEATURES && SIM3OPT_MAX_CAPACITY < S3O_REMOVED, "the largest keyframe");

namespace {

// the wave's sum of v in every lane, in the documented order
__device__ inline double waveSum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}
__device__ inline int waveSumInt(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The three passes of optimiseSim3 over the correspondences of one problem, by one wave.
struct WaveOps {
  const Problem& P;
  int lane;
  Sim3* pert;    // [2][14] of this wave, in LDS: the perturbed estimates, then their inverses
  Sim3 kept;     // the estimate of the round's last trial

  // f(edge, feature of KF1, feature of KF2) for every correspondence of the lane in ascending order
  template <class F>
  __device__ void walk(F f) {
    int st = 0;
    for (int i1 = lane; i1 < P.n1; i1 += 64) {
      // (the perturbed estimates are read from LDS again for every correspondence: hoisted out of this loop they would take
      // 448 registers and spill)
      asm volatile("" ::: "memory");
      const int i2 = partnerOf(P, i1, &st);
      if (i2 < 0) continue;
      Edge E;
      loadEdge(P, i1, i2, &E);
      f(E, i1, i2);
    }
  }

  __device__ void build(const Sim3& S, double* sum, Branches* br) {
    // the wave's earlier reads of the perturbed estimates are done before lanes 0 .. 13 replace them, and their writes are
    // done before any lane reads them (the fences order the LDS accesses of the wave's own lanes; the waves share nothing)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < 14) {
      Sim3 Sk, SkInv;
      sim3Perturbed(S, P.fixScale, lane, &Sk, &SkInv);
      pert[lane] = Sk;
      pert[14 + lane] = SkInv;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    Sim3 Sinv;
    sim3Inverse(S, &Sinv);
    double acc[S3O_ACC_BUILD];
#pragma unroll
    for (int k = 0; k < S3O_ACC_BUILD; k++) acc[k] = 0.0;
    int huberOutliers = 0;
    const Sim3* pertRead = pert;
    walk([&](const Edge& E, int, int) { huberOutliers += pairBuild(S, Sinv, pertRead, E, P.K, P.delta, acc); });
    br->lm.huberOutliers += huberOutliers;
#pragma unroll
    for (int k = 0; k < S3O_ACC_BUILD; k++) sum[k] = waveSum(acc[k]);
  }

  __device__ double trial(const Sim3& S) {
    Sim3 Sinv;
    sim3Inverse(S, &Sinv);
    double acc = 0.0;
    walk([&](const Edge& E, int, int) { pairRho(S, Sinv, E, P.K, P.delta, &acc); });
    return waveSum(acc);
  }

  __device__ void keep(const Sim3& S) { kept = S; }

  __device__ int classify() {
    const Sim3 Strial = kept;
    Sim3 Sinv;
    sim3Inverse(Strial, &Sinv);
    int bad = 0;
    walk([&](const Edge& E, int i1, int i2) {
      if (pairIsOutlier(Strial, Sinv, E, P.K, P.th2, nullptr)) {
        P.row[i1] = i2 + S3O_REMOVED;  // (made -1, or given back, when the call ends)
        bad++;
      }
    });
    return waveSumInt(bad);
  }
};

__global__ __launch_bounds__(SIM3OPT_THREADS) void k_sim3_optimize(const Sim3OptArgs a) {
  __shared__ Sim3 pert[SIM3OPT_WAVES][28];
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * SIM3OPT_WAVES + (threadIdx.x >> 6);
  if (p >= a.nProblems) return;  // (a whole wave: the waves of a workgroup never meet)
  const size_t cap = (size_t)a.cap;
  const int np = a.nProblems;
  const int kf1 = a.problems[p], kf2 = a.problems[np + p], set1 = a.problems[2 * np + p], set2 = a.problems[3 * np + p];  // (checked on the host)
  const float* simIn = a.sim3 + (size_t)p * 13;
  orbx_sim3opt_result* out = a.res + p;

  Problem P;
  P.kps1 = a.kps + (size_t)kf1 * cap;
  P.kps2 = a.kps + (size_t)kf2 * cap;
  P.row = a.row + (size_t)p * cap;
  P.points1 = a.points + (size_t)set1 * cap * 3;
  P.points2 = a.points + (size_t)set2 * cap * 3;
  P.mask1 = a.mask ? a.mask + (size_t)set1 * cap : nullptr;
  P.mask2 = a.mask ? a.mask + (size_t)set2 * cap : nullptr;
  P.pose1 = a.pose + (size_t)kf1 * 12;
  P.pose2 = a.pose + (size_t)kf2 * 12;
  P.invSigma2 = a.invSigma2;
  P.n1 = a.nKps[kf1];
  P.n2 = a.nKps[kf2];
  P.cap = a.cap;
  P.nLevels = a.nLevels;
  P.K = Cam{a.fx, a.fy, a.cx, a.cy};
  P.delta = a.delta;
  P.th2 = a.th2;
  P.fixScale = a.fixScale != 0;

  // ---- the device data checked before it is followed ----
  int status = 0, nCorr = 0;
  if (P.n1 < 0 || P.n1 > a.cap || P.n2 < 0 || P.n2 > a.cap) {
    status |= ORBX_SIM3OPT_BAD_INPUT;
    P.n1 = 0;
  }
  for (int k = 0; k < 12; k++)
    if (!isFiniteF(P.pose1[k]) || !isFiniteF(P.pose2[k])) status |= ORBX_SIM3OPT_NONFINITE;
  for (int k = 0; k < 13; k++)
    if (!isFiniteF(simIn[k])) status |= ORBX_SIM3OPT_NONFINITE;
  if (!(simIn[12] > 0.f)) status |= ORBX_SIM3OPT_NONFINITE;
  for (int i1 = lane; i1 < P.n1; i1 += 64) nCorr += checkFeature(P, i1, &status) ? 1 : 0;
  // (status bits differ between the lanes: each bit is voted on)
  status = (__any(status & ORBX_SIM3OPT_BAD_INPUT) ? ORBX_SIM3OPT_BAD_INPUT : 0) |
           (__any(status & ORBX_SIM3OPT_NONFINITE) ? ORBX_SIM3OPT_NONFINITE : 0);
  nCorr = __builtin_amdgcn_readfirstlane(waveSumInt(nCorr));

  Rounds r;
  Sim3 S;
  bool recovered = false;
  const bool ran = status == 0 && nCorr > 0;
  if (ran) {
    Branches br{};
    WaveOps ops{P, lane, pert[threadIdx.x >> 6], Sim3{}};
    sim3FromRow(simIn, &S);
    recovered = optimiseSim3(ops, &S, P.fixScale, nCorr, a.nIterations, a.nMoreIterations, &r, &br);
    bool fin = isFinite(r.chi2Initial) && isFinite(r.chi2Final) && isFinite(r.lambda) && isFinite(S.s);
    for (int k = 0; k < 4; k++) fin = fin && isFinite(S.q[k]);
    for (int k = 0; k < 3; k++) fin = fin && isFinite(S.t[k]);
    if (!fin) status = ORBX_SIM3OPT_NONFINITE;
    if (!recovered) sim3FromRow(simIn, &S);  // (the start estimate again: not kept in registers through the rounds)
    // the row: a non-finite result gives the removed entries back, every other one makes them -1
    for (int i1 = lane; i1 < P.n1; i1 += 64) {
      const int v = P.row[i1];
      if (v >= S3O_REMOVED) P.row[i1] = status ? v - S3O_REMOVED : -1;
    }
  }

  // ---- the result (every lane holds it: lane 0 writes) ----
  if (lane == 0) {
    const bool optimised = ran && status == 0;
    float simOut[13];  // (d_sim3_out may be d_sim3: the row is read again before anything of it is written)
#pragma unroll
    for (int k = 0; k < 13; k++) simOut[k] = simIn[k];
    out->status = status;
    out->n_correspondences = optimised ? nCorr : 0;
    out->n_bad = optimised ? r.nBad : 0;
    out->n_inliers = optimised ? r.nInliers : 0;
    out->rounds = optimised ? r.rounds : 0;
    for (int k = 0; k < 2; k++) {
      out->iterations[k] = optimised ? r.iterations[k] : 0;
      out->stop_reason[k] = optimised ? r.stopReason[k] : 0;
    }
    out->lm_trials = optimised ? r.lmTrials : 0;
    out->rejected_trials = optimised ? r.rejected : 0;
    out->solver_failures = optimised ? r.solverFailures : 0;
    out->small_theta = optimised ? r.smallTheta : 0;
    out->small_sigma = optimised ? r.smallSigma : 0;
    out->small_both = optimised ? r.smallBoth : 0;
    out->reserved = 0;
    out->chi2_initial = optimised ? r.chi2Initial : 0.0;
    out->chi2_final = optimised ? r.chi2Final : 0.0;
    out->lambda = optimised ? r.lambda : 0.0;
    for (int k = 0; k < 4; k++) out->q[k] = optimised ? S.q[k] : 0.0;
    for (int k = 0; k < 3; k++) out->t[k] = optimised ? S.t[k] : 0.0;
    out->s = optimised ? S.s : 0.0;
    if (optimised && recovered) {
      double R[3][3];
      quatToMatrix(S.q, R);
      for (int k = 0; k < 9; k++) simOut[k] = (float)R[k / 3][k % 3];
      for (int k = 0; k < 3; k++) simOut[9 + k] = (float)S.t[k];
      simOut[12] = (float)S.s;
    }
    out->s12 = simOut[12];
    for (int k = 0; k < 9; k++) out->R12[k] = simOut[k];
    for (int k = 0; k < 3; k++) out->t12[k] = simOut[9 + k];
    out->reserved_f = 0.f;
    float* so = a.sim3Out + (size_t)p * 13;
    for (int k = 0; k < 13; k++) so[k] = simOut[k];
  }
}

}  // namespace

hipError_t launch_sim3_optimize(hipStream_t st, const Sim3OptArgs& a) {
  hipLaunchKernelGGL(k_sim3_optimize, dim3((a.nProblems + SIM3OPT_WAVES - 1) / SIM3OPT_WAVES), dim3(SIM3OPT_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
