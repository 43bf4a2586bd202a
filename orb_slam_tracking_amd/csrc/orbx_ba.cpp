// orbx_ba.cpp — host side of the two-view bundle adjustment (include/orbx.h, "behind the Initializer: two-view bundle
// adjustment"): the argument checks, the pair list, the workspace and the C entry points.  The kernel is in orbx_ba_kernel.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "orbx_host.h"

using namespace orbx;

namespace {

constexpr int BA_MAX_CAPACITY = 1 << 20;

}  // namespace

extern "C" {

int orbx_bundle_adjust_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_first, const int32_t* h_second,
                                    const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const int32_t* d_matches12,
                                    const orbx_init_result* d_init_res, const float* d_p3d, const uint8_t* d_triangulated,
                                    const float* K, const float* inv_sigma2, int n_iterations, int min_points, int normalize,
                                    orbx_ba_result* d_res, float* d_p3d_out) {
  if (n_frames < 0 || n_pairs < 0 || capacity < 1 || n_iterations < 0 || (n_pairs > 0 && (!h_first || !h_second)) || !d_kps_un ||
      !d_n || !d_matches12 || !d_init_res || !d_p3d || !d_triangulated || !K || !d_res || !d_p3d_out)
    return ORBX_E_BADARG;
  if (!pairsInRange(h_first, h_second, n_pairs, n_frames)) {
    if (ctx) ctxSetError(ctx, "bundle adjust: pair index outside [0, n_frames)");
    return ORBX_E_BADARG;
  }
  if (capacity >= BA_MAX_CAPACITY) {
    if (ctx) ctxSetError(ctx, "bundle adjust: capacity of 2^20 or more");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  BaScratch* s = ctxBa(ctx);
  hipStream_t st = ctxStream(ctx);
  int nLevels = 0;
  const float* table = ctxInvSigma2(ctx, &nLevels);
  // the pair list and the table go up only when they differ from the last call's.  Such a call first waits for the context stream
  // -- the host copies an earlier upload may still be reading are replaced -- and is the documented exception to "returns once
  // queued" (include/orbx.h); a pipeline that adjusts the same pairs of every batch uploads once
  const float* sig = inv_sigma2 ? inv_sigma2 : table;
  const bool samePairs = s->pairs.holds(h_first, n_pairs, h_second, n_pairs), sameSigma = s->sigma.holds(sig, nLevels);
  if (!samePairs || !sameSigma) HIPCHK(hipStreamSynchronize(st));
  if (!samePairs) HIPCHK(s->pairs.replace(st, h_first, n_pairs, h_second, n_pairs));
  if (!sameSigma) HIPCHK(s->sigma.replace(st, sig, nLevels));
  BaArgs a{};
  const size_t points = (size_t)n_pairs * (size_t)capacity;
  auto work = [&](Layout L) {
    a.ws = L.take<double>(points * BA_WS_DOUBLES);
    a.wf = L.take<float>(points * BA_WS_FLOATS);
    a.widx = L.take<int32_t>(points);
    return L.size();
  };
  HIPCHK(s->dWork.grow(work(Layout()), st));
  work(Layout(s->dWork));
  a.kps = d_kps_un;
  a.nKps = d_n;
  a.m12 = d_matches12;
  a.frames = s->pairs;
  a.ires = d_init_res;
  a.p3d = d_p3d;
  a.tri = d_triangulated;
  a.invSigma2 = s->sigma;
  a.res = d_res;
  a.p3dOut = d_p3d_out;
  intrinsics(K, &a.fx, &a.fy, &a.cx, &a.cy);
  a.delta = (double)(float)std::sqrt(5.99);  // `const float thHuber2D = sqrt(5.99)` of the ORB-SLAM design
  a.nPairs = n_pairs;
  a.cap = capacity;
  a.nLevels = nLevels;
  a.nIterations = n_iterations;
  a.minPoints = min_points;
  a.normalize = normalize != 0;
  HIPCHK(launch_ba(st, a));
  return ORBX_OK;
}

int orbx_bundle_adjust(orbx_ctx* ctx, const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, const int32_t* matches12,
                       const orbx_init_result* init_res, const float* p3d, const uint8_t* triangulated, const float* K,
                       const float* inv_sigma2, int n_iterations, int min_points, int normalize, orbx_ba_result* res,
                       float* p3d_out) {
  if (n1 < 0 || n2 < 0 || n_iterations < 0 || !init_res || !K || !res || (n1 > 0 && (!k1 || !matches12 || !p3d || !triangulated || !p3d_out)) ||
      (n2 > 0 && !k2))
    return ORBX_E_BADARG;
  const int cap = std::max(std::max(n1, n2), 1);
  if (cap >= BA_MAX_CAPACITY) {
    if (ctx) ctxSetError(ctx, "bundle adjust: 2^20 keypoints or more");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  BaScratch* s = ctxBa(ctx);
  hipStream_t st = ctxStream(ctx);
  orbx_keypoint* dK;
  int32_t *dN, *dM;
  orbx_init_result* dIR;
  orbx_ba_result* dR;
  float* dP;
  uint8_t* dT;
  auto staging = [&](Layout L) {  // the two frames (0 and 1) in the batch layout, then the results
    dK = L.take<orbx_keypoint>((size_t)2 * cap);
    dN = L.take<int32_t>(2);
    dM = L.take<int32_t>(cap);
    dIR = L.take<orbx_init_result>(1);
    dR = L.take<orbx_ba_result>(1);
    dP = L.take<float>((size_t)cap * 3);
    dT = L.take<uint8_t>(cap);
    return L.size();
  };
  const size_t bytes = staging(Layout());
  HIPCHK(s->dIo.grow(bytes, st));
  staging(Layout(s->dIo));
  HIPCHK(hipMemsetAsync(s->dIo, 0, bytes, st));  // (entries beyond n1: no match, not triangulated)
  const int32_t hn[2] = {n1, n2};
  HIPCHK(up(dK, k1, n1, st));
  HIPCHK(up(dM, matches12, n1, st));
  HIPCHK(up(dP, p3d, (size_t)n1 * 3, st));
  HIPCHK(up(dT, triangulated, n1, st));
  HIPCHK(up(dK + cap, k2, n2, st));
  HIPCHK(up(dN, hn, 2, st));
  HIPCHK(up(dIR, init_res, 1, st));
  const int32_t f0 = 0, f1 = 1;
  r = orbx_bundle_adjust_batch_device(ctx, 2, 1, &f0, &f1, dK, dN, cap, dM, dIR, dP, dT, K, inv_sigma2, n_iterations, min_points,
                                      normalize, dR, dP);
  if (r != ORBX_OK) {
    (void)hipStreamSynchronize(st);  // (the uploads queued above read this frame's variables)
    return r;
  }
  HIPCHK(down(res, dR, 1, st));
  HIPCHK(down(p3d_out, dP, (size_t)n1 * 3, st));
  HIPCHK(hipStreamSynchronize(st));
  return ORBX_OK;
}

}  // extern "C"
