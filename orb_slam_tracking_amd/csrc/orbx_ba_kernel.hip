// orbx_ba_kernel.hip — two-view bundle adjustment on the device (include/orbx.h, "behind the Initializer: two-view bundle
// adjustment"): g2o's Levenberg-Marquardt with the Schur complement over one free pose and the pair's points.
//
//   k_ba   workgroup (256 lanes = 4 waves) per pair   the checks of the device data, the point list compacted in order, every
//                                                     iteration and trial, the median depth, the normalisation, the result
//
// The whole optimisation of a pair runs inside one launch: the 6x6 reduced system is solved and the trial judged by lane 0, which
// broadcasts its verdict through LDS; the points are strided over the lanes (point j belongs to lane j % 256) and their blocks
// (Hll, bl, Hpl, the estimate and its backup) live in the context's workspace, [array][cap] per pair so that a wave's accesses are
// contiguous.  All arithmetic is in csrc/orbx_ba_math.inc, shared with the CPU restatement; this file fixes who computes what and
// the order of the sums (include/orbx.h, deviation 1): a lane adds its points' terms one after the other, a wave folds its lanes
// with shuffles (+32, +16, ... +1), lane 0 of the workgroup adds the four waves' sums in order.  f64 without contraction
// (-ffp-contract=off).  Every control decision is read from LDS behind a barrier, so the workgroup never diverges at a barrier.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/orbx.h"
#include "orbx_launch.h"

#define ORBX_BA_FN __device__
#include "orbx_ba_math.inc"

namespace orbx {
using namespace orbx_ba;

namespace {

constexpr int BA_WAVES = BA_THREADS / 64;

struct BaShared {
  double red[BA_WAVES][BA_ACC_MAX];
  double sum[BA_ACC_MAX];
  double maxDiag[BA_WAVES];
  Lm lm;
  Pose T, Tb;
  Counters cnt;
  double chi2Initial;
  float median;
  int waveCnt[BA_WAVES];
  int status, n1, n2, f1, f2;
  int accepted, more, stop;
};

// the lanes' N sums folded into s.sum[0 .. N) in the documented order; two barriers
template <int N>
__device__ void blockReduce(BaShared& s, const double* acc, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < N; k++) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    if (lane == 0) s.red[wave][k] = v;
  }
  __syncthreads();
  if (tid < N) {
    double v = s.red[0][tid];
    for (int w = 1; w < BA_WAVES; w++) v = v + s.red[w][tid];
    s.sum[tid] = v;
  }
  __syncthreads();
}

__device__ inline void loadPoint(const double* ws, size_t cap, int j, int first, int n, double* out) {
  for (int k = 0; k < n; k++) out[k] = ws[(size_t)(first + k) * cap + j];
}
__device__ inline void storePoint(double* ws, size_t cap, int j, int first, int n, const double* in) {
  for (int k = 0; k < n; k++) ws[(size_t)(first + k) * cap + j] = in[k];
}
// workspace arrays of a point (BA_WS_DOUBLES)
constexpr int WS_X = 0, WS_XB = 3, WS_HLL = 6, WS_BL = 12, WS_HPL = 15;

__global__ __launch_bounds__(BA_THREADS) void k_ba(const BaArgs a) {
  __shared__ BaShared s;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t cap = (size_t)a.cap;
  const float* pin = a.p3d + (size_t)p * cap * 3;
  float* pout = a.p3dOut + (size_t)p * cap * 3;
  const uint8_t* tri = a.tri + (size_t)p * cap;
  const int32_t* m12 = a.m12 + (size_t)p * cap;
  double* ws = a.ws + (size_t)p * cap * BA_WS_DOUBLES;
  float* wf = a.wf + (size_t)p * cap * BA_WS_FLOATS;
  int32_t* widx = a.widx + (size_t)p * cap;
  const orbx_init_result* ir = a.ires + p;
  orbx_ba_result* out = a.res + p;
  const Cam K{a.fx, a.fy, a.cx, a.cy};

  if (tid == 0) {
    int st = 0, n1 = 0, n2 = 0;
    const int f1 = a.frames[p], f2 = a.frames[a.nPairs + p];  // (checked on the host)
    if (ir->status != 0) {
      st = ORBX_BA_SKIPPED;
    } else {
      n1 = a.nKps[f1];
      n2 = a.nKps[f2];
      if (n1 < 0 || n1 > a.cap || n2 < 0 || n2 > a.cap) st |= ORBX_BA_BAD_INPUT;
      bool fin = true;
      for (int i = 0; i < 9; i++) fin = fin && isFiniteF(ir->R21[i]);
      for (int i = 0; i < 3; i++) fin = fin && isFiniteF(ir->t21[i]);
      if (!fin) st |= ORBX_BA_NONFINITE;
    }
    s.status = st;
    s.n1 = n1; s.n2 = n2; s.f1 = f1; s.f2 = f2;
  }
  __syncthreads();
  int status = s.status;
  int nPts = 0;

  // ---- the point vertices in ascending i, the device data checked before it is followed ----
  if (status == 0) {
    const int n1 = s.n1, n2 = s.n2;
    const orbx_keypoint* k1 = a.kps + (size_t)s.f1 * cap;
    const orbx_keypoint* k2 = a.kps + (size_t)s.f2 * cap;
    int bad = 0, nonfin = 0;
    for (int i0 = 0; i0 < n1; i0 += BA_THREADS) {
      const int i = i0 + tid;
      bool flag = false;
      int m = -1, o1 = 0, o2 = 0;
      if (i < n1) {
        m = m12[i];
        if (m >= n2) {
          bad = 1;
        } else if (m >= 0 && tri[i] != 0) {
          o1 = k1[i].octave;
          o2 = k2[m].octave;
          if (o1 < 0 || o1 >= a.nLevels || o2 < 0 || o2 >= a.nLevels)
            bad = 1;
          else
            flag = true;
        }
      }
      const unsigned long long ballot = __ballot(flag);
      if (lane == 0) s.waveCnt[wave] = __popcll(ballot);
      __syncthreads();
      int off = nPts, total = 0;
      for (int w = 0; w < BA_WAVES; w++) {
        if (w < wave) off += s.waveCnt[w];
        total += s.waveCnt[w];
      }
      if (flag) {
        const int j = off + __popcll(ballot & ((1ull << lane) - 1ull));  // < n1 <= cap
        for (int c = 0; c < 3; c++) {
          const float v = pin[(size_t)i * 3 + c];
          if (!isFiniteF(v)) nonfin = 1;
          ws[(size_t)(WS_X + c) * cap + j] = (double)v;
        }
        wf[0 * cap + j] = k1[i].x;
        wf[1 * cap + j] = k1[i].y;
        wf[2 * cap + j] = k2[m].x;
        wf[3 * cap + j] = k2[m].y;
        wf[4 * cap + j] = a.invSigma2[o1];
        wf[5 * cap + j] = a.invSigma2[o2];
        widx[j] = i;
      }
      nPts += total;
      __syncthreads();  // (before waveCnt is written again)
    }
    if (__syncthreads_or(bad)) status |= ORBX_BA_BAD_INPUT;
    if (__syncthreads_or(nonfin)) status |= ORBX_BA_NONFINITE;
  }

  if (tid == 0) {
    Lm& m = s.lm;
    m.lambda = 0.0; m.ni = 2.0; m.currentChi = 0.0; m.iniChi = 0.0; m.rho = 0.0;
    m.nBad = 0; m.qmax = 0; m.ok = 0;
    m.iterations = 0; m.lmTrials = 0; m.rejected = 0; m.solverFailures = 0; m.stopReason = 0;
    s.cnt = Counters{0, 0, 0, 0};
    s.chi2Initial = 0.0;
    s.median = 0.f;
    if (status == 0) poseFromRt(ir->R21, ir->t21, &s.T);
  }
  __syncthreads();

  // ---- SparseOptimizer::optimize ----
  if (status == 0 && nPts > 0) {
    for (int it = 0; it < a.nIterations; it++) {
      {  // computeActiveErrors, activeRobustChi2, buildSystem
        double acc[BA_ACC_BUILD];
#pragma unroll
        for (int k = 0; k < BA_ACC_BUILD; k++) acc[k] = 0.0;
        const Pose T = s.T;
        double R[3][3];
        quatToMatrix(T.q, R);
        double maxd = 0.0;
        for (int j = tid; j < nPts; j += BA_THREADS) {
          double X[3], Hll[6], bl[3], Hpl[18];
          float obs[6];
          loadPoint(ws, cap, j, WS_X, 3, X);
          for (int k = 0; k < 6; k++) obs[k] = wf[(size_t)k * cap + j];
          pointBuild(T, R, X, obs, K, a.delta, Hll, bl, Hpl, acc);
          storePoint(ws, cap, j, WS_HLL, 6, Hll);
          storePoint(ws, cap, j, WS_BL, 3, bl);
          storePoint(ws, cap, j, WS_HPL, 18, Hpl);
          for (int k = 0; k < 6; k += (k == 0 ? 3 : 2)) {  // Hll's diagonal: 0, 3, 5
            const double d = Hll[k] < 0.0 ? -Hll[k] : Hll[k];
            if (d > maxd) maxd = d;
          }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const double o = __shfl_down(maxd, off, 64);
          if (o > maxd) maxd = o;
        }
        if (lane == 0) s.maxDiag[wave] = maxd;
        blockReduce<BA_ACC_BUILD>(s, acc, tid);
      }
      if (tid == 0) {
        Lm& m = s.lm;
        for (int k = 0; k < 21; k++) m.Hpp[k] = s.sum[BA_ACC_HPP + k];
        for (int k = 0; k < 6; k++) m.bp[k] = s.sum[BA_ACC_BP + k];
        m.currentChi = m.iniChi = s.sum[BA_ACC_CHI2];
        if (it == 0) {
          double mx = 0.0;
          for (int w = 0; w < BA_WAVES; w++)
            if (s.maxDiag[w] > mx) mx = s.maxDiag[w];
          s.chi2Initial = m.currentChi;
          m.lambda = lmLambdaInit(m.Hpp, mx);
          m.ni = 2.0;
          m.nBad = 0;
        }
        m.rho = 0.0;
        m.qmax = 0;
      }
      __syncthreads();
      int more;
      do {
        const double lambda = s.lm.lambda;
        {  // push, setLambda, the Schur complement
          double acc[BA_ACC_SCHUR];
#pragma unroll
          for (int k = 0; k < BA_ACC_SCHUR; k++) acc[k] = 0.0;
          for (int j = tid; j < nPts; j += BA_THREADS) {
            double X[3], Hll[6], bl[3], Hpl[18];
            loadPoint(ws, cap, j, WS_X, 3, X);
            storePoint(ws, cap, j, WS_XB, 3, X);
            loadPoint(ws, cap, j, WS_HLL, 6, Hll);
            loadPoint(ws, cap, j, WS_BL, 3, bl);
            loadPoint(ws, cap, j, WS_HPL, 18, Hpl);
            pointSchur(Hll, bl, Hpl, lambda, acc);
          }
          blockReduce<BA_ACC_SCHUR>(s, acc, tid);
        }
        if (tid == 0) {
          Lm& m = s.lm;
          s.Tb = s.T;
          m.ok = lmSolvePose(&m, s.sum + BA_ACC_S, s.sum + BA_ACC_COEF) ? 1 : 0;
          if (!m.ok)
            m.solverFailures++;
          else if (poseOplus(m.xp, &s.T))
            s.cnt.smallTheta++;
        }
        __syncthreads();
        const int ok = s.lm.ok;
        if (ok) {  // the points' step, the trial's errors
          double acc[BA_ACC_TRIAL] = {0.0, 0.0};
          double xp[6];
          for (int k = 0; k < 6; k++) xp[k] = s.lm.xp[k];
          const Pose T = s.T;
          for (int j = tid; j < nPts; j += BA_THREADS) {
            double X[3], xl[3], Hll[6], bl[3], Hpl[18];
            float obs[6];
            loadPoint(ws, cap, j, WS_X, 3, X);
            loadPoint(ws, cap, j, WS_HLL, 6, Hll);
            loadPoint(ws, cap, j, WS_BL, 3, bl);
            loadPoint(ws, cap, j, WS_HPL, 18, Hpl);
            for (int k = 0; k < 6; k++) obs[k] = wf[(size_t)k * cap + j];
            pointStep(Hll, bl, Hpl, lambda, xp, X, xl, acc);
            storePoint(ws, cap, j, WS_X, 3, X);
            pointChi2(T, X, obs, K, a.delta, &acc[BA_ACC_TCHI2]);
          }
          blockReduce<BA_ACC_TRIAL>(s, acc, tid);
        }
        if (tid == 0) {
          const int acc = lmJudge(&s.lm, ok ? s.sum[BA_ACC_TCHI2] : 0.0, ok ? s.sum[BA_ACC_SCALE] : 0.0, &s.cnt);
          if (!acc) s.T = s.Tb;
          s.accepted = acc;
          s.more = lmAnotherTrial(&s.lm) ? 1 : 0;
        }
        __syncthreads();
        more = s.more;
        if (!s.accepted && ok) {  // pop
          for (int j = tid; j < nPts; j += BA_THREADS) {
            double X[3];
            loadPoint(ws, cap, j, WS_XB, 3, X);
            storePoint(ws, cap, j, WS_X, 3, X);
          }
        }
        __syncthreads();  // (s.accepted / s.more are read before lane 0 writes them again; the restored points before they are read)
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
  __syncthreads();

  // ---- behind the optimisation: f32 points, the median depth, the tests of CreateInitialMapMonocular ----
  bool optimised = status == 0;
  if (optimised) {
    int nonfin = 0;
    for (int j = tid; j < nPts; j += BA_THREADS)
      for (int c = 0; c < 3; c++) {
        const double v = ws[(size_t)(WS_X + c) * cap + j];
        if (!isFinite(v)) nonfin = 1;
        wf[(size_t)c * cap + j] = (float)v;  // (the observations are no longer needed)
      }
    if (tid == 0) {
      for (int k = 0; k < 4; k++) nonfin |= !isFinite(s.T.q[k]);
      for (int k = 0; k < 3; k++) nonfin |= !isFinite(s.T.t[k]);
      nonfin |= !isFinite(s.chi2Initial) || !isFinite(s.lm.currentChi) || !isFinite(s.lm.lambda);
    }
    if (__syncthreads_or(nonfin)) {
      status |= ORBX_BA_NONFINITE;
      optimised = false;
    }
  }
  float inv = 1.f;
  bool scaled = false;
  if (optimised) {
    if (nPts > 0) {  // the exact order statistic: the element with (nPts - 1) / 2 elements in front of it
      const int want = (nPts - 1) / 2;
      const float* z = wf + 2 * cap;
      for (int j = tid; j < nPts; j += BA_THREADS) {
        const float zj = z[j];
        int before = 0;
        for (int k = 0; k < nPts; k++) {
          const float zk = z[k];
          before += (zk < zj || (zk == zj && k < j)) ? 1 : 0;
        }
        if (before == want) s.median = zj;
      }
    }
    __syncthreads();
    const float median = s.median;
    if (nPts < a.minPoints) status |= ORBX_BA_FEW_POINTS;
    if (nPts > 0 && median < 0.f) status |= ORBX_BA_NEGATIVE_DEPTH;
    if (a.normalize && status == 0 && median > 0.f) {
      inv = 1.0f / median;
      scaled = true;
    }
  }

  // ---- outputs ----
  for (size_t k = tid; k < cap * 3; k += BA_THREADS) pout[k] = pin[k];  // (in place: each element onto itself)
  __syncthreads();
  if (optimised)
    for (int j = tid; j < nPts; j += BA_THREADS) {
      const size_t i = (size_t)widx[j];
      for (int c = 0; c < 3; c++) {
        const float v = wf[(size_t)c * cap + j];
        pout[i * 3 + c] = scaled ? v * inv : v;
      }
    }
  if (tid == 0) {
    const Lm& m = s.lm;
    out->status = status;
    out->n_points = (status & (ORBX_BA_SKIPPED | ORBX_BA_BAD_INPUT)) ? 0 : nPts;
    out->iterations = m.iterations;
    out->lm_trials = m.lmTrials;
    out->rejected_trials = m.rejected;
    out->solver_failures = m.solverFailures;
    out->stop_reason = m.stopReason;
    out->reserved = 0;
    out->reserved2 = 0.f;
    if (optimised) {
      out->chi2_initial = s.chi2Initial;
      out->chi2_final = m.currentChi;
      out->lambda = m.lambda;
      double R[3][3];
      quatToMatrix(s.T.q, R);
      for (int k = 0; k < 4; k++) out->q[k] = s.T.q[k];
      for (int k = 0; k < 3; k++) out->t[k] = s.T.t[k];
      for (int k = 0; k < 9; k++) out->R21[k] = (float)R[k / 3][k % 3];
      for (int k = 0; k < 3; k++) {
        const float t = (float)s.T.t[k];
        out->t21[k] = scaled ? t * inv : t;
      }
      out->median_depth = s.median;
    } else {
      out->chi2_initial = out->chi2_final = out->lambda = 0.0;
      for (int k = 0; k < 4; k++) out->q[k] = 0.0;
      for (int k = 0; k < 3; k++) out->t[k] = 0.0;
      for (int k = 0; k < 9; k++) out->R21[k] = ir->R21[k];
      for (int k = 0; k < 3; k++) out->t21[k] = ir->t21[k];
      out->median_depth = 0.f;
    }
  }
}

}  // namespace

hipError_t launch_ba(hipStream_t st, const BaArgs& a) {
  hipLaunchKernelGGL(k_ba, dim3(a.nPairs), dim3(BA_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
