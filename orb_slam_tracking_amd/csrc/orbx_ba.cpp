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
  HeldUploads hold(st);
  HIPCHK(hold(s->pairs, {h_first, h_second}, n_pairs));
  HIPCHK(hold(s->sigma, {inv_sigma2 ? inv_sigma2 : table}, nLevels));
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
  const size_t c = (size_t)cap;
  const int32_t hn[2] = {n1, n2};
  Staged io(ctxIo(ctx), ctxStream(ctx));  // the two frames (0 and 1) in the batch layout, then the results
  auto dK = io.in(k1, n1, 2 * c);
  io.in(dK, c, k2, n2);
  auto dN = io.in(hn, 2, 2);
  auto dM = io.in(matches12, n1, c);
  auto dIR = io.in(init_res, 1, 1);
  auto dR = io.out(res, 1, 1);
  auto dP = io.in(p3d, (size_t)n1 * 3, c * 3);  // (adjusted in place)
  io.out(dP, 0, p3d_out, (size_t)n1 * 3);
  auto dT = io.in(triangulated, n1, c);
  HIPCHK(io.open(Staged::Zeroed));  // (entries beyond n1: no match, not triangulated)
  const int32_t f0 = 0, f1 = 1;
  r = orbx_bundle_adjust_batch_device(ctx, 2, 1, &f0, &f1, io[dK], io[dN], cap, io[dM], io[dIR], io[dP], io[dT], K, inv_sigma2,
                                      n_iterations, min_points, normalize, io[dR], io[dP]);
  return io.close(ctx, r);
}

}  // extern "C"
