// orbx_pose.cpp — host side of what runs behind SearchByBoW: Optimizer::PoseOptimization (include/orbx.h, "behind SearchByBoW:
// pose optimisation"; the kernel is in orbx_pose_kernel.hip) and, below it, PnPsolver, which gives a lost frame the start pose
// ("behind SearchByBoW: PnP RANSAC"; orbx_pnp_kernel.hip), and Sim3Solver, PnPsolver's 3D-3D sibling of loop closing ("loop
// closing: Sim3 RANSAC"; orbx_sim3_kernel.hip), and at the end Optimizer::OptimizeSim3 ("loop closing: Sim3 optimisation";
// orbx_sim3opt_kernel.hip).  For each: the argument checks, the problem list, the held tables and the C
// entry points.
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
  HeldUploads hold(st);
  HIPCHK(hold(s->problems, {h_frame, h_point_set}, n_problems));
  HIPCHK(hold(s->sigma, {inv_sigma2 ? inv_sigma2 : table}, nLevels));
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
  const size_t c = (size_t)cap;
  const int32_t hn = n, zero = 0;
  Staged io(ctxIo(ctx), ctxStream(ctx));  // one frame and one point set in the batch layout, then the results
  auto dK = io.in(kps_un, n, c);
  auto dN = io.in(&hn, 1, 1);
  auto dP = io.in(points, (size_t)n * 3, c * 3);
  auto dPose = io.in(pose0, 12, 12);
  auto dM = io.optIn(mask, n, c);
  auto dO = io.out(outlier, n, c);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  r = orbx_pose_optimize_batch_device(ctx, 1, 1, &zero, &zero, io[dK], io[dN], cap, nullptr, 1, io[dP], io[dM], io[dPose], K, inv_sigma2,
                                      n_iterations, io[dR], io[dO]);
  return io.close(ctx, r);
}

}  // extern "C"

// ---- PnPsolver: SetRansacParameters' table, the workspace of the three launches and the C entry points ---------------------------
namespace {

bool paramsOk(double probability, int minInliers, int maxIterations, float epsilon) {
  return probability > 0.0 && probability < 1.0 && epsilon > 0.f && epsilon < 1.f && minInliers >= 4 && maxIterations >= 1;
}

// SetRansacParameters for one N, with the design's expression types (include/orbx.h, rule 2)
void ransacEntry(int N, double mRansacProb, int minInliers, int mRansacMaxIts, float mRansacEpsilon, int32_t* out) {
  const int minSet = 4;
  int nMinInliers = (int)((float)N * mRansacEpsilon);
  if (nMinInliers < minInliers) nMinInliers = minInliers;
  if (nMinInliers < minSet) nMinInliers = minSet;
  const int Nd = N > 0 ? N : 1;  // (the design divides by N = 0; such a solver is bNoMore before it iterates)
  if (mRansacEpsilon < (float)nMinInliers / Nd) mRansacEpsilon = (float)nMinInliers / Nd;
  int nIterations;
  if (nMinInliers == Nd) {
    nIterations = 1;
  } else {
    const double it = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow((double)mRansacEpsilon, 3)));
    // (epsilon >= 1 gives log(<= 0): no finite count; mRansacMaxIts bounds it either way)
    nIterations = (it >= 1.0 && it < 2147483647.0) ? (int)it : (it < 1.0 ? 1 : mRansacMaxIts);
  }
  out[0] = nMinInliers;
  out[1] = std::max(1, std::min(nIterations, mRansacMaxIts));
}

}  // namespace

extern "C" {

int orbx_pnp_ransac_table(double probability, int min_inliers, int max_iterations, float epsilon, int n_max, int32_t* out) {
  if (!paramsOk(probability, min_inliers, max_iterations, epsilon) || n_max < 0 || !out) return ORBX_E_BADARG;
  for (int N = 0; N <= n_max; N++) ransacEntry(N, probability, min_inliers, max_iterations, epsilon, out + 2 * (size_t)N);
  return ORBX_OK;
}

int orbx_pnp_solve_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_frame, const int32_t* h_point_set,
                                const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const int32_t* d_match,
                                int n_point_sets, const float* d_points, const uint8_t* d_point_mask, const float* K,
                                const float* sigma2, double probability, int min_inliers, int max_iterations, float epsilon, float th2,
                                int n_iter, const int32_t* d_draws, orbx_pnp_result* d_res, float* d_pose, int32_t* d_match_inliers,
                                uint8_t* d_inliers) {
  if (n_frames < 0 || n_problems < 0 || n_point_sets < 0 || capacity < 1 || n_iter < 1 ||
      (n_problems > 0 && (!h_frame || !h_point_set)) || !d_kps_un || !d_n || !d_points || !K || !d_draws || !d_res || !d_pose ||
      !d_match_inliers || !paramsOk(probability, min_inliers, max_iterations, epsilon) || !(th2 > 0.f) || !std::isfinite(th2))
    return ORBX_E_BADARG;
  if (!pairsInRange(h_frame, h_point_set, n_problems, n_frames, n_point_sets)) {
    if (ctx) ctxSetError(ctx, "pnp solve: frame outside [0, n_frames) or point set outside [0, n_point_sets)");
    return ORBX_E_BADARG;
  }
  if (capacity > PNP_MAX_CAPACITY) {
    if (ctx) ctxSetError(ctx, "pnp solve: capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_problems == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  PnpScratch* s = ctxPnp(ctx);
  hipStream_t st = ctxStream(ctx);
  int nLevels = 0;
  const float* own = ctxSigma2(ctx, &nLevels);
  const float* sig = sigma2 ? sigma2 : own;
  // the table of these parameters up to this capacity (computed again only when they change)
  const size_t tableLen = 2 * ((size_t)capacity + 1);
  if (s->hTable.size() != tableLen || s->keyProbability != probability || s->keyEpsilon != epsilon ||
      s->keyMinInliers != min_inliers || s->keyMaxIterations != max_iterations) {
    s->hTable.resize(tableLen);
    (void)orbx_pnp_ransac_table(probability, min_inliers, max_iterations, epsilon, capacity, s->hTable.data());
    s->keyProbability = probability;
    s->keyEpsilon = epsilon;
    s->keyMinInliers = min_inliers;
    s->keyMaxIterations = max_iterations;
  }
  // the workspace of the three launches
  PnpArgs a{};
  auto workspace = [&](Layout L) {
    a.corr = L.take<uint8_t>((size_t)n_problems * capacity * PNP_CORR_BYTES);
    a.corrOf = L.take<int32_t>((size_t)n_problems * capacity);
    a.meta = L.take<int32_t>((size_t)n_problems * 4);
    a.hyp = L.take<uint8_t>((size_t)n_problems * n_iter * PNP_HYP_BYTES);
    return L.size();
  };
  const size_t bytes = workspace(Layout());
  HeldUploads hold(st);
  HIPCHK(hold(s->problems, {h_frame, h_point_set}, n_problems));
  HIPCHK(hold(s->sigma2, {sig}, nLevels));
  HIPCHK(hold(s->table, {s->hTable.data()}, tableLen));
  HIPCHK(s->dWork.grow(bytes, st));
  workspace(Layout(s->dWork));
  a.kps = d_kps_un;
  a.nKps = d_n;
  a.problems = s->problems;
  a.match = d_match;
  a.points = d_points;
  a.mask = d_point_mask;
  a.sigma2 = s->sigma2;
  a.table = s->table;
  a.draws = d_draws;
  a.res = d_res;
  a.pose = d_pose;
  a.matchInliers = d_match_inliers;
  a.inliers = d_inliers;
  intrinsics(K, &a.fu, &a.fv, &a.uc, &a.vc);
  a.th2 = th2;
  a.nProblems = n_problems;
  a.cap = capacity;
  a.nLevels = nLevels;
  a.nIter = n_iter;
  HIPCHK(launch_pnp_prep(st, a));
  HIPCHK(launch_pnp_hypotheses(st, a));
  HIPCHK(launch_pnp_refine(st, a));
  return ORBX_OK;
}

int orbx_pnp_solve(orbx_ctx* ctx, const orbx_keypoint* kps_un, int n, const float* points, const uint8_t* mask, const float* K,
                   const float* sigma2, double probability, int min_inliers, int max_iterations, float epsilon, float th2, int n_iter,
                   const int32_t* draws, orbx_pnp_result* res, uint8_t* inliers) {
  if (n < 0 || n_iter < 1 || !K || !draws || !res || (n > 0 && (!kps_un || !points || !inliers)) ||
      !paramsOk(probability, min_inliers, max_iterations, epsilon) || !(th2 > 0.f) || !std::isfinite(th2))
    return ORBX_E_BADARG;
  const int cap = std::max(n, 1);
  if (cap > PNP_MAX_CAPACITY) {
    if (ctx) ctxSetError(ctx, "pnp solve: more than ORBX_BOW_MAX_FEATURES keypoints");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const size_t c = (size_t)cap;
  const int32_t hn = n, zero = 0;
  Staged io(ctxIo(ctx), ctxStream(ctx));  // one frame and one point set in the batch layout, then the results
  auto dK = io.in(kps_un, n, c);
  auto dN = io.in(&hn, 1, 1);
  auto dP = io.in(points, (size_t)n * 3, c * 3);
  auto dM = io.optIn(mask, n, c);
  auto dDraws = io.in(draws, (size_t)n_iter * 4, (size_t)n_iter * 4);
  auto dPose = io.room<float>(12);
  auto dRow = io.room<int32_t>(c);
  auto dI = io.out(inliers, n, c);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  r = orbx_pnp_solve_batch_device(ctx, 1, 1, &zero, &zero, io[dK], io[dN], cap, nullptr, 1, io[dP], io[dM], K, sigma2, probability,
                                  min_inliers, max_iterations, epsilon, th2, n_iter, io[dDraws], io[dR], io[dPose], io[dRow], io[dI]);
  return io.close(ctx, r);
}

}  // extern "C"

// ---- Sim3Solver: SetRansacParameters' table, the workspace of the three launches and the C entry points -------------------------
namespace {

bool sim3ParamsOk(double probability, int minInliers, int maxIterations, float th2, int fixScale) {
  return probability > 0.0 && probability < 1.0 && minInliers >= 3 && maxIterations >= 1 && th2 > 0.f && std::isfinite(th2) &&
         (fixScale == 0 || fixScale == 1);
}

// SetRansacParameters for one N, with the design's expression types (include/orbx.h, rule 2)
int32_t sim3RansacEntry(int N, double mRansacProb, int minInliers, int maxIterations) {
  if (N < minInliers) return maxIterations;  // (the design takes log of a negative number; such a solver is bNoMore at once)
  const float epsilon = (float)minInliers / N;
  int nIterations;
  if (minInliers == N) {
    nIterations = 1;
  } else {
    const double it = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow((double)epsilon, 3)));
    nIterations = (it >= 1.0 && it < 2147483647.0) ? (int)it : (it < 1.0 ? 1 : maxIterations);
  }
  return std::max(1, std::min(nIterations, maxIterations));
}

}  // namespace

extern "C" {

int orbx_sim3_ransac_table(double probability, int min_inliers, int max_iterations, int n_max, int32_t* out) {
  if (!sim3ParamsOk(probability, min_inliers, max_iterations, 1.f, 0) || n_max < 0 || !out) return ORBX_E_BADARG;
  for (int N = 0; N <= n_max; N++) out[N] = sim3RansacEntry(N, probability, min_inliers, max_iterations);
  return ORBX_OK;
}

int orbx_sim3_solve_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_kf1, const int32_t* h_kf2,
                                 const int32_t* h_set1, const int32_t* h_set2, const orbx_keypoint* d_kps_un, const int32_t* d_n,
                                 int capacity, const int32_t* d_match, int n_point_sets, const float* d_points,
                                 const uint8_t* d_point_mask, const float* d_pose, const float* K, const float* sigma2, int fix_scale,
                                 double probability, int min_inliers, int max_iterations, float th2, int n_iter,
                                 const int32_t* d_draws, orbx_sim3_result* d_res, float* d_sim3, int32_t* d_match_inliers,
                                 uint8_t* d_inliers) {
  if (n_frames < 0 || n_problems < 0 || n_point_sets < 0 || capacity < 1 || n_iter < 1 ||
      (n_problems > 0 && (!h_kf1 || !h_kf2 || !h_set1 || !h_set2)) || !d_kps_un || !d_n || !d_match || !d_points || !d_pose || !K ||
      !d_draws || !d_res || !d_sim3 || !d_match_inliers || !sim3ParamsOk(probability, min_inliers, max_iterations, th2, fix_scale))
    return ORBX_E_BADARG;
  if (!pairsInRange(h_kf1, h_kf2, n_problems, n_frames) || !pairsInRange(h_set1, h_set2, n_problems, n_point_sets)) {
    if (ctx) ctxSetError(ctx, "sim3 solve: keyframe outside [0, n_frames) or point set outside [0, n_point_sets)");
    return ORBX_E_BADARG;
  }
  if (capacity > SIM3_MAX_CAPACITY) {
    if (ctx) ctxSetError(ctx, "sim3 solve: capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  if ((long long)n_problems * n_iter > SIM3_MAX_HYPOTHESES) {  // (a lane each: the launch's grid)
    if (ctx) ctxSetError(ctx, "sim3 solve: n_problems * n_iter above 2^31 - 64");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_problems == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  Sim3Scratch* s = ctxSim3(ctx);
  hipStream_t st = ctxStream(ctx);
  int nLevels = 0;
  const float* own = ctxSigma2(ctx, &nLevels);
  const float* sig = sigma2 ? sigma2 : own;
  // the table of these parameters up to this capacity (computed again only when they change)
  const size_t tableLen = (size_t)capacity + 1;
  if (s->hTable.size() != tableLen || s->keyProbability != probability || s->keyMinInliers != min_inliers ||
      s->keyMaxIterations != max_iterations) {
    s->hTable.resize(tableLen);
    (void)orbx_sim3_ransac_table(probability, min_inliers, max_iterations, capacity, s->hTable.data());
    s->keyProbability = probability;
    s->keyMinInliers = min_inliers;
    s->keyMaxIterations = max_iterations;
  }
  // the workspace of the three launches
  Sim3Args a{};
  auto workspace = [&](Layout L) {
    a.corr = L.take<uint8_t>((size_t)n_problems * capacity * SIM3_CORR_BYTES);
    a.corrOf = L.take<int32_t>((size_t)n_problems * capacity);
    a.meta = L.take<int32_t>((size_t)n_problems * 4);
    a.hyp = L.take<uint8_t>((size_t)n_problems * n_iter * SIM3_HYP_BYTES);
    return L.size();
  };
  const size_t bytes = workspace(Layout());
  HeldUploads hold(st);
  HIPCHK(hold(s->problems, {h_kf1, h_kf2, h_set1, h_set2}, n_problems));
  HIPCHK(hold(s->sigma2, {sig}, nLevels));
  HIPCHK(hold(s->table, {s->hTable.data()}, tableLen));
  HIPCHK(s->dWork.grow(bytes, st));
  workspace(Layout(s->dWork));
  a.kps = d_kps_un;
  a.nKps = d_n;
  a.problems = s->problems;
  a.match = d_match;
  a.points = d_points;
  a.mask = d_point_mask;
  a.pose = d_pose;
  a.sigma2 = s->sigma2;
  a.table = s->table;
  a.draws = d_draws;
  a.res = d_res;
  a.sim3 = d_sim3;
  a.matchInliers = d_match_inliers;
  a.inliers = d_inliers;
  a.fx = K[0];
  a.fy = K[4];
  a.cx = K[2];
  a.cy = K[5];
  a.th2 = th2;
  a.nProblems = n_problems;
  a.cap = capacity;
  a.nLevels = nLevels;
  a.nIter = n_iter;
  a.minInliers = min_inliers;
  a.fixScale = fix_scale;
  HIPCHK(launch_sim3_prep(st, a));
  HIPCHK(launch_sim3_hypotheses(st, a));
  HIPCHK(launch_sim3_resolve(st, a));
  return ORBX_OK;
}

int orbx_sim3_solve(orbx_ctx* ctx, const orbx_keypoint* kps_un1, int n1, const float* points1, const uint8_t* mask1,
                    const float* pose1, const orbx_keypoint* kps_un2, int n2, const float* points2, const uint8_t* mask2,
                    const float* pose2, const int32_t* match12, const float* K, const float* sigma2, int fix_scale,
                    double probability, int min_inliers, int max_iterations, float th2, int n_iter, const int32_t* draws,
                    orbx_sim3_result* res, float* sim3, int32_t* match_inliers, uint8_t* inliers) {
  if (n1 < 0 || n2 < 0 || n_iter < 1 || !pose1 || !pose2 || !K || !draws || !res || !sim3 ||
      (n1 > 0 && (!kps_un1 || !points1 || !match12 || !match_inliers)) || (n2 > 0 && (!kps_un2 || !points2)) ||
      (mask1 == nullptr) != (mask2 == nullptr) || !sim3ParamsOk(probability, min_inliers, max_iterations, th2, fix_scale))
    return ORBX_E_BADARG;
  const int cap = std::max(std::max(n1, n2), 1);
  if (cap > SIM3_MAX_CAPACITY) {
    if (ctx) ctxSetError(ctx, "sim3 solve: more than ORBX_BOW_MAX_FEATURES keypoints");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const size_t c = (size_t)cap;
  const int32_t hn[2] = {n1, n2}, zero = 0, one = 1;
  Staged io(ctxIo(ctx), ctxStream(ctx));  // two frames and two point sets in the batch layout, then the results
  auto dK = io.in(kps_un1, n1, 2 * c);
  io.in(dK, c, kps_un2, n2);
  auto dN = io.in(hn, 2, 2);
  auto dP = io.in(points1, (size_t)n1 * 3, 2 * c * 3);
  io.in(dP, c * 3, points2, (size_t)n2 * 3);
  auto dM = io.optIn(mask1, n1, 2 * c);  // (both frames bring a mask, or neither does)
  io.in(dM, c, mask2, n2);
  auto dPose = io.in(pose1, 12, 24);
  io.in(dPose, 12, pose2, 12);
  auto dMatch = io.in(match12, n1, c);
  auto dDraws = io.in(draws, (size_t)n_iter * 3, (size_t)n_iter * 3);
  auto dSim = io.out(sim3, 13, 13);
  auto dRow = io.out(match_inliers, n1, c);
  auto dI = io.out(inliers, n1, c);  // (the kernel writes them whether the caller takes them or not)
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  r = orbx_sim3_solve_batch_device(ctx, 2, 1, &zero, &one, &zero, &one, io[dK], io[dN], cap, io[dMatch], 2, io[dP], io[dM], io[dPose], K,
                                   sigma2, fix_scale, probability, min_inliers, max_iterations, th2, n_iter, io[dDraws], io[dR], io[dSim],
                                   io[dRow], io[dI]);
  return io.close(ctx, r);
}

}  // extern "C"

// ---- Optimizer::OptimizeSim3 (include/orbx.h, "loop closing: Sim3 optimisation"; orbx_sim3opt_kernel.hip) ------------------------
namespace {

bool sim3OptParamsOk(int fixScale, float th2, int nIterations, int nMoreIterations) {
  return (fixScale == 0 || fixScale == 1) && th2 > 0.f && std::isfinite(th2) && nIterations >= 0 && nMoreIterations >= 0;
}

}  // namespace

extern "C" {

int orbx_optimize_sim3_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_kf1, const int32_t* h_kf2,
                                    const int32_t* h_set1, const int32_t* h_set2, const orbx_keypoint* d_kps_un, const int32_t* d_n,
                                    int capacity, int32_t* d_matches, int n_point_sets, const float* d_points,
                                    const uint8_t* d_point_mask, const float* d_pose, const float* d_sim3, const float* K,
                                    const float* inv_sigma2, int fix_scale, float th2, int n_iterations, int n_more_iterations,
                                    orbx_sim3opt_result* d_res, float* d_sim3_out) {
  if (n_frames < 0 || n_problems < 0 || n_point_sets < 0 || capacity < 1 ||
      (n_problems > 0 && (!h_kf1 || !h_kf2 || !h_set1 || !h_set2)) || !d_kps_un || !d_n || !d_matches || !d_points || !d_pose ||
      !d_sim3 || !K || !d_res || !d_sim3_out || !sim3OptParamsOk(fix_scale, th2, n_iterations, n_more_iterations))
    return ORBX_E_BADARG;
  if (!pairsInRange(h_kf1, h_kf2, n_problems, n_frames) || !pairsInRange(h_set1, h_set2, n_problems, n_point_sets)) {
    if (ctx) ctxSetError(ctx, "optimize sim3: keyframe outside [0, n_frames) or point set outside [0, n_point_sets)");
    return ORBX_E_BADARG;
  }
  if (capacity > SIM3OPT_MAX_CAPACITY) {
    if (ctx) ctxSetError(ctx, "optimize sim3: capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_problems == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  Sim3OptScratch* s = ctxSim3Opt(ctx);
  hipStream_t st = ctxStream(ctx);
  int nLevels = 0;
  const float* table = ctxInvSigma2(ctx, &nLevels);
  HeldUploads hold(st);
  HIPCHK(hold(s->problems, {h_kf1, h_kf2, h_set1, h_set2}, n_problems));
  HIPCHK(hold(s->sigma, {inv_sigma2 ? inv_sigma2 : table}, nLevels));
  Sim3OptArgs a{};
  a.kps = d_kps_un;
  a.nKps = d_n;
  a.problems = s->problems;
  a.row = d_matches;
  a.points = d_points;
  a.mask = d_point_mask;
  a.pose = d_pose;
  a.sim3 = d_sim3;
  a.invSigma2 = s->sigma;
  a.res = d_res;
  a.sim3Out = d_sim3_out;
  intrinsics(K, &a.fx, &a.fy, &a.cx, &a.cy);
  a.delta = (double)(float)std::sqrt((double)th2);  // `const float deltaHuber = sqrt(th2)` of the ORB-SLAM2 design
  a.th2 = (double)th2;
  a.nProblems = n_problems;
  a.cap = capacity;
  a.nLevels = nLevels;
  a.nIterations = n_iterations;
  a.nMoreIterations = n_more_iterations;
  a.fixScale = fix_scale;
  HIPCHK(launch_sim3_optimize(st, a));
  return ORBX_OK;
}

int orbx_optimize_sim3(orbx_ctx* ctx, const orbx_keypoint* kps_un1, int n1, const float* points1, const uint8_t* mask1,
                       const float* pose1, const orbx_keypoint* kps_un2, int n2, const float* points2, const uint8_t* mask2,
                       const float* pose2, int32_t* matches12, const float* sim3, const float* K, const float* inv_sigma2,
                       int fix_scale, float th2, int n_iterations, int n_more_iterations, orbx_sim3opt_result* res, float* sim3_out) {
  if (n1 < 0 || n2 < 0 || !pose1 || !pose2 || !sim3 || !K || !res || !sim3_out || (n1 > 0 && (!kps_un1 || !points1 || !matches12)) ||
      (n2 > 0 && (!kps_un2 || !points2)) || (mask1 == nullptr) != (mask2 == nullptr) ||
      !sim3OptParamsOk(fix_scale, th2, n_iterations, n_more_iterations))
    return ORBX_E_BADARG;
  const int cap = std::max(std::max(n1, n2), 1);
  if (cap > SIM3OPT_MAX_CAPACITY) {
    if (ctx) ctxSetError(ctx, "optimize sim3: more than ORBX_BOW_MAX_FEATURES keypoints");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const size_t c = (size_t)cap;
  const int32_t hn[2] = {n1, n2}, zero = 0, one = 1;
  Staged io(ctxIo(ctx), ctxStream(ctx));  // two frames and two point sets in the batch layout, then the results
  auto dK = io.in(kps_un1, n1, 2 * c);
  io.in(dK, c, kps_un2, n2);
  auto dN = io.in(hn, 2, 2);
  auto dP = io.in(points1, (size_t)n1 * 3, 2 * c * 3);
  io.in(dP, c * 3, points2, (size_t)n2 * 3);
  auto dM = io.optIn(mask1, n1, 2 * c);  // (both frames bring a mask, or neither does)
  io.in(dM, c, mask2, n2);
  auto dPose = io.in(pose1, 12, 24);
  io.in(dPose, 12, pose2, 12);
  auto dRow = io.inout(matches12, n1, c);
  auto dSim = io.in(sim3, 13, 13);
  auto dSimOut = io.out(sim3_out, 13, 13);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  r = orbx_optimize_sim3_batch_device(ctx, 2, 1, &zero, &one, &zero, &one, io[dK], io[dN], cap, io[dRow], 2, io[dP], io[dM], io[dPose],
                                      io[dSim], K, inv_sigma2, fix_scale, th2, n_iterations, n_more_iterations, io[dR], io[dSimOut]);
  return io.close(ctx, r);
}

}  // extern "C"
