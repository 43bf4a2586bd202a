// orbx_lba_kernel.hip — Optimizer::LocalBundleAdjustment on the device (include/orbx.h, "local mapping: local bundle
// adjustment"): g2o's Levenberg-Marquardt with the Schur complement over the free keyframes of a local window, their map points
// and the fixed keyframes that see them, two rounds with the outlier classification between them.
//
//   k_lba   workgroup (256 lanes = 4 waves) per problem   the checks of the device data, the graph built from the rows (observer
//                                                         words, edge lists by count / scan / fill / sort), both rounds with
//                                                         every iteration and trial, the classification, the outputs
//
// Everything a lane computes is a phase of csrc/orbx_lba_math.inc, shared with the CPU restatement: that file fixes who owns
// what and the order of every sum.  This file is the sequence of the phases with a barrier between two that depend on each
// other, and the two folds the phases leave open: laneSum (a tree over the 256 lanes' values: lane l += lane l + 128, + 64, ...
// + 1) and waveFold (lane l += lane l + 32, ... + 1 inside a wave).  The per-vertex and per-edge blocks, the poses and the
// reduced system (dense, packed lower triangle, up to 384 x 384) live in the problem's part of the context's workspace -- the
// packed factor of a problem with at most LBA_LDS_MAX_FREE free keyframes in dynamic LDS instead --; the
// system's diagonal, its right-hand side, the solution and the free poses' diagonal blocks are in LDS.  Every control decision
// (a failed pivot, a trial's verdict, the end of a round) is read from LDS behind a barrier, so the workgroup never diverges at
// one.  f64 without contraction (-ffp-contract=off); integer atomics only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/orbx.h"
#include "orbx_launch.h"

#define ORBX_BA_FN __device__
#include "orbx_ba_math.inc"
#define ORBX_LBA_ADD(p, v) atomicAdd((p), (v))
#define ORBX_LBA_OR64(p, v) atomicOr((p), (unsigned long long)(v))
#include "orbx_lba_math.inc"

namespace orbx {
using namespace orbx_lba;

namespace {

static_assert(LBA_THREADS == LBA_NT, "a problem's lanes");

// the lanes' status bits gathered: every lane gets the union
__device__ int gather(Shared& s, int bits) {
  if (bits) atomicOr(&s.status, bits);
  __syncthreads();
  return s.status;
}
__device__ double laneSum(double* red, double v, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int off = LBA_NT / 2; off >= 1; off >>= 1) {
    if (tid < off) red[tid] = red[tid] + red[tid + off];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
__device__ double laneMax(double* red, double v, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int off = LBA_NT / 2; off >= 1; off >>= 1) {
    if (tid < off && red[tid + off] > red[tid]) red[tid] = red[tid + off];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(LBA_THREADS) void k_lba(const LbaArgs a) {
  __shared__ Shared s;
  extern __shared__ double ldsFactor[];  // a.ldsBytes: the largest packed factor among the batch's problems that keep theirs here
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = a.nProblems;
  const int first = a.problems[p], set = a.problems[3 * P + p];
  Prob v;
  v.kps = a.kps;
  v.nKps = a.nKps;
  v.poseIn = a.pose;
  v.frameOf = a.entryFrame + first;
  v.rows = a.rows + (size_t)first * a.cap;
  v.mapPts = a.mapPts + (size_t)set * a.mapCap * 3;
  v.mapMask = a.mapMask ? a.mapMask + (size_t)set * a.mapCap : nullptr;
  v.invSigma2 = a.invSigma2;
  v.nLevels = a.nLevels;
  v.cap = a.cap;
  v.mapCap = a.mapCap;
  v.mapN = a.mapN[set];
  v.nE = a.problems[P + p];
  v.nF = a.problems[2 * P + p];
  v.K = Cam{a.fx, a.fy, a.cx, a.cy};
  v.delta = a.delta;
  layout(&v, (uintptr_t)(a.ws + (size_t)a.problems[4 * P + p] * 256));
  if (v.nF <= a.ldsMaxFree) v.H = ldsFactor;  // (factorBytes(nF) <= a.ldsBytes: the host sized it so)
  float* poseOut = a.poseOut + (size_t)first * 12;
  float* mapOut = a.mapOut + (size_t)set * a.mapCap * 3;
  uint8_t* outlier = a.outlier + (size_t)first * a.cap;
  orbx_lba_result* out = a.res + p;

  if (tid == 0) {
    s.status = (v.mapN < 0 || v.mapN > v.mapCap) ? ST_BAD : 0;
    s.nP = s.nEdges = s.nLevel1 = s.nErased = 0;
    s.cnt = Counters{0, 0, 0, 0};
    for (int r = 0; r < 2; r++) {
      s.iterations[r] = s.trials[r] = s.rejected[r] = s.failures[r] = s.stopReason[r] = s.nActP[r] = s.nActF[r] = 0;
      s.chi2Initial[r] = s.chi2Final[r] = s.lambda[r] = 0.0;
    }
  }
  for (size_t k = tid; k < (size_t)v.nE * v.cap; k += LBA_NT) outlier[k] = 0;
  __syncthreads();
  int status = s.status;

  // ---- the graph, the device data checked before it is followed ----
  if (!status) status = gather(s, checkEntries(v, tid));
  if (!status) {
    clearGraph(v, tid);
    __syncthreads();
    status = gather(s, countEdges(v, tid));
  }
  if (!status) {
    countVertices(v, s, tid);
    __syncthreads();
    if (tid == 0) {
      scanLanes(s);
      s.nP = s.scan[LBA_NT];
    }
    __syncthreads();
    status = gather(s, fillVertices(v, s, tid));
  }
  if (!status) {
    countSlots(v, s, tid);
    __syncthreads();
    if (tid == 0) {
      scanLanes(s);
      s.nEdges = s.scan[LBA_NT];
    }
    __syncthreads();
    fillStarts(v, s, tid);
    __syncthreads();
    fillEdges(v, tid);
    __syncthreads();
    status = gather(s, sortEdges(v, s, tid));
  }
  if (!status) loadPoses(v, tid);
  __syncthreads();
  const bool counted = status == 0;
  const bool run = status == 0 && v.nF > 0 && s.nEdges > 0;

  // ---- the two rounds ----
  if (run) {
    for (int round = 0; round < 2; round++) {
      const bool robust = round == 0;
      const int nIt = round == 0 ? a.nIterations : a.nMoreIterations;
      if (tid == 0) roundClear(s);
      __syncthreads();
      activate(v, s, tid);
      __syncthreads();
      if (tid == 0) roundStart(v, s, round);
      __syncthreads();
      if (s.nActEdges > 0) {
        activeErrors(v, s, tid, robust);
        __syncthreads();
        for (int it = 0; it < nIt; it++) {
          double chi = 0.0, maxd = 0.0;
          buildPoints(v, s, tid, robust, &chi, &maxd);
          for (int ar = wave; ar < s.nA; ar += LBA_NT / 64) {
            double acc[27];
            buildPoseLane(v, s.actEnt[ar], lane, robust, acc);
#pragma unroll
            for (int k = 0; k < 27; k++) {
              double t = acc[k];
#pragma unroll
              for (int off = 32; off >= 1; off >>= 1) t = t + __shfl_down(t, off, 64);
              acc[k] = t;
            }
            if (lane == 0) buildPoseKeep(s, ar, acc);
          }
          const double chiAll = laneSum(s.red, chi, tid);
          const double maxAll = laneMax(s.red2, maxd, tid);
          if (tid == 0) iterationStart(s, round, it, chiAll, maxAll);
          __syncthreads();
          int more;
          do {
            trialPoints(v, s, tid);
            __syncthreads();
            schurOwners(v, s, tid);
            __syncthreads();
            int ok = 1;
            const int n = s.n;
            for (int jc = 0; jc < n; jc++) {
              if (!cholColumn(v, s, jc, tid)) {  // (the pivot is in LDS: every lane takes the same way)
                ok = 0;
                break;
              }
              __syncthreads();
              cholUpdate(v, s, jc, tid);
              __syncthreads();
            }
            if (ok) {
              for (int jc = 0; jc < n; jc++) {
                solveForward(v, s, jc, tid);
                __syncthreads();
              }
              for (int jc = n - 1; jc >= 0; jc--) {
                solveBackward(v, s, jc, tid);
                __syncthreads();
              }
              ok = __syncthreads_or(solutionBad(s, tid)) ? 0 : 1;
            }
            if (tid == 0) {
              s.lm.ok = ok;
              if (!ok) s.lm.solverFailures++;
            }
            double scale = 0.0, tchi = 0.0;
            if (ok) {
              trialStep(v, s, tid, &scale);
              __syncthreads();
              tchi = activeErrors(v, s, tid, robust);
            }
            const double scaleAll = laneSum(s.red, scale, tid);
            const double tchiAll = laneSum(s.red2, tchi, tid);
            if (tid == 0) {
              s.accepted = lmJudge(&s.lm, ok ? tchiAll : 0.0, ok ? poseScale(s, scaleAll) : 0.0, &s.cnt);
              s.more = lmAnotherTrial(&s.lm) ? 1 : 0;
            }
            __syncthreads();
            more = s.more;
            if (!s.accepted && ok) trialRestore(v, s, tid);
            __syncthreads();
          } while (more);
          if (tid == 0) {
            const int r = lmEndIteration(&s.lm);
            s.lm.iterations++;
            s.lm.stopReason = r;
            s.stop = r;
          }
          __syncthreads();
          if (s.stop) break;
        }
      }
      if (tid == 0) roundEnd(s, round);
      __syncthreads();
      if (round == 0) {
        const int n = classify(v, s, tid, nullptr);
        if (n) atomicAdd(&s.nLevel1, n);
        __syncthreads();
      }
    }
  }

  // ---- the classification behind round 2, the outputs ----
  bool optimised = run;
  if (run && __syncthreads_or(resultBad(v, s, tid))) {
    status |= ST_NONFINITE;
    optimised = false;
  }
  if (optimised) {
    const int n = classify(v, s, tid, outlier);
    if (n) atomicAdd(&s.nErased, n);
  }
  writeOutputs(v, s, tid, optimised, poseOut, mapOut);
  __syncthreads();
  if (tid == 0) writeResult(v, s, status, counted, run, out);
}

}  // namespace

hipError_t launch_lba(hipStream_t st, const LbaArgs& a) {
  // (beyond 64 KiB of LDS per workgroup a kernel asks for it explicitly)
  if (a.ldsBytes + sizeof(Shared) > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lba), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.ldsBytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_lba, dim3(a.nProblems), dim3(LBA_THREADS), a.ldsBytes, st, a);
  return hipGetLastError();
}

}  // namespace orbx
