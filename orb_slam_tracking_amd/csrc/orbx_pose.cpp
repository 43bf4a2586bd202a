// orbx_pose.cpp — host side of Optimizer::PoseOptimization (include/orbx.h, "behind SearchByBoW: pose optimisation"): the
// argument checks, the problem list and the C entry points.  The kernel is in orbx_pose_kernel.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "orbx_host.h"

using namespace orbx;

namespace {

constexpr int POSE_MAX_CAPACITY = 1 << 20;

}  // namespace

extern "C" {

int orbx_pose_optimize_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_frame, const int32_t* h_point_set,
                                    const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const int32_t* d_match,
                                    int n_point_sets, const float* d_points, const uint8_t* d_point_mask, const float* d_pose0,
                                    const float* K, const float* inv_sigma2, int n_iterations, orbx_pose_result* d_res,
                                    uint8_t* d_outlier) {
  if (n_frames < 0 || n_problems < 0 || n_point_sets < 0 || capacity < 1 || n_iterations < 0 ||
      (n_problems > 0 && (!h_frame || !h_point_set)) || !d_kps_un || !d_n || !d_points || !d_pose0 || !K || !d_res || !d_outlier)
    return ORBX_E_BADARG;
  if (!pairsInRange(h_frame, h_point_set, n_problems, n_frames, n_point_sets)) {
    if (ctx) ctxSetError(ctx, "pose optimize: frame outside [0, n_frames) or point set outside [0, n_point_sets)");
    return ORBX_E_BADARG;
  }
  if (capacity >= POSE_MAX_CAPACITY) {
    if (ctx) ctxSetError(ctx, "pose optimize: capacity of 2^20 or more");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_problems == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  PoseScratch* s = ctxPose(ctx);
  hipStream_t st = ctxStream(ctx);
  int nLevels = 0;
  const float* table = ctxInvSigma2(ctx, &nLevels);
  // the problem list and the table go up only when they differ from the last call's.  Such a call first waits for the context
  // stream -- the host copies an earlier upload may still be reading are replaced -- and is the documented exception to "returns
  // once queued" (include/orbx.h)
  const float* sig = inv_sigma2 ? inv_sigma2 : table;
  const bool sameList = s->problems.holds(h_frame, n_problems, h_point_set, n_problems), sameSigma = s->sigma.holds(sig, nLevels);
  if (!sameList || !sameSigma) HIPCHK(hipStreamSynchronize(st));
  if (!sameList) HIPCHK(s->problems.replace(st, h_frame, n_problems, h_point_set, n_problems));
  if (!sameSigma) HIPCHK(s->sigma.replace(st, sig, nLevels));
  PoseArgs a{};
  a.kps = d_kps_un;
  a.nKps = d_n;
  a.problems = s->problems;
  a.match = d_match;
  a.points = d_points;
  a.mask = d_point_mask;
  a.pose0 = d_pose0;
  a.invSigma2 = s->sigma;
  a.res = d_res;
  a.outlier = d_outlier;
  intrinsics(K, &a.fx, &a.fy, &a.cx, &a.cy);
  a.delta = (double)(float)std::sqrt(5.991);  // `const float deltaMono = sqrt(5.991)` of the ORB-SLAM2 design
  a.nProblems = n_problems;
  a.cap = capacity;
  a.nLevels = nLevels;
  a.nIterations = n_iterations;
  HIPCHK(launch_pose(st, a));
  return ORBX_OK;
}

int orbx_pose_optimize(orbx_ctx* ctx, const orbx_keypoint* kps_un, int n, const float* points, const uint8_t* mask,
                       const float* pose0, const float* K, const float* inv_sigma2, int n_iterations, orbx_pose_result* res,
                       uint8_t* outlier) {
  if (n < 0 || n_iterations < 0 || !pose0 || !K || !res || (n > 0 && (!kps_un || !points || !outlier))) return ORBX_E_BADARG;
  const int cap = std::max(n, 1);
  if (cap >= POSE_MAX_CAPACITY) {
    if (ctx) ctxSetError(ctx, "pose optimize: 2^20 keypoints or more");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  PoseScratch* s = ctxPose(ctx);
  hipStream_t st = ctxStream(ctx);
  orbx_keypoint* dK;
  int32_t* dN;
  float *dP, *dPose;
  uint8_t *dM, *dO;
  orbx_pose_result* dR;
  auto staging = [&](Layout L) {  // one frame and one point set in the batch layout, then the results
    dK = L.take<orbx_keypoint>(cap);
    dN = L.take<int32_t>(1);
    dP = L.take<float>((size_t)cap * 3);
    dPose = L.take<float>(12);
    dM = L.take<uint8_t>(cap);
    dO = L.take<uint8_t>(cap);
    dR = L.take<orbx_pose_result>(1);
    return L.size();
  };
  const size_t bytes = staging(Layout());
  HIPCHK(s->dIo.grow(bytes, st));
  staging(Layout(s->dIo));
  HIPCHK(hipMemsetAsync(s->dIo, 0, bytes, st));
  const int32_t hn = n, zero = 0;
  HIPCHK(up(dK, kps_un, n, st));
  HIPCHK(up(dP, points, (size_t)n * 3, st));
  if (mask) HIPCHK(up(dM, mask, n, st));
  HIPCHK(up(dN, &hn, 1, st));
  HIPCHK(up(dPose, pose0, 12, st));
  r = orbx_pose_optimize_batch_device(ctx, 1, 1, &zero, &zero, dK, dN, cap, nullptr, 1, dP, mask ? dM : nullptr, dPose, K, inv_sigma2,
                                      n_iterations, dR, dO);
  if (r != ORBX_OK) {
    (void)hipStreamSynchronize(st);  // (the uploads queued above read this frame's variables)
    return r;
  }
  HIPCHK(down(res, dR, 1, st));
  HIPCHK(down(outlier, dO, n, st));
  HIPCHK(hipStreamSynchronize(st));
  return ORBX_OK;
}

}  // extern "C"
