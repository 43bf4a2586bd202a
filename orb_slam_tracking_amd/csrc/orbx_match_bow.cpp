// orbx_match_bow.cpp — host side of the matchers that walk the FeatureVector: ORBmatcher::SearchByBoW (include/orbx.h, "matching
// through the FeatureVector") and LocalMapping::CreateNewMapPoints ("growing the map": ORBmatcher::SearchForTriangulation and the
// triangulation behind it): the argument checks, the pair lists and the C entry points.  The kernels are in
// orbx_match_bow_kernel.hip and orbx_match_tri_kernel.hip.  (The matchers by projection are in orbx_match_proj.cpp.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "orbx_host.h"

using namespace orbx;

namespace {

// a FeatureVector in host memory: every feature index below the frame's count
bool featuresOk(const uint32_t* feat, int fvN, int n) {
  for (int i = 0; i < fvN; i++)
    if (feat[i] >= (uint32_t)n) return false;
  return true;
}

// What the four calls of CreateNewMapPoints refuse alike, all of it before the context -> ORBX_OK or the code, with the complaint
// left in the context when there is one.
int triRefused(orbx_ctx* ctx, const char* name, int n_frames, int n_pairs, const int32_t* h_kf1, const int32_t* h_kf2, int capacity,
               const float* K) {
  const char* why = nullptr;
  if (!pairsInRange(h_kf1, h_kf2, n_pairs, n_frames)) why = "pair index outside [0, n_frames)";
  else if (!std::isfinite(K[0]) || !std::isfinite(K[4]) || !std::isfinite(K[2]) || !std::isfinite(K[5]) || !(K[0] > 0.0f) || !(K[4] > 0.0f))
    why = "K is not finite or has no positive focal lengths";
  const bool over = capacity > ORBX_BOW_MAX_FEATURES;
  if (!why && !over) return ORBX_OK;
  if (ctx) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", name, why ? why : "capacity above ORBX_BOW_MAX_FEATURES");
    ctxSetError(ctx, msg);
  }
  return why ? ORBX_E_BADARG : ORBX_E_CAPACITY;
}

// the camera K[9] (row-major) and the context's pyramid tables as the two kernels take them
TriCamArgs triCam(const orbx_ctx* ctx, const float* K) {
  TriCamArgs c{};
  c.fx = K[0];
  c.fy = K[4];
  c.cx = K[2];
  c.cy = K[5];
  c.scaleFactor = orbx_get_scale_factor(ctx);
  int nl = 0;
  const float* scale = ctxScale(ctx, &c.nLevels);
  const float* sigma2 = ctxSigma2(ctx, &nl);
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) {
    c.scale[l] = l < c.nLevels ? scale[l] : 0.0f;
    c.sigma2[l] = l < nl ? sigma2[l] : 0.0f;
  }
  return c;
}

}  // namespace

extern "C" {

int orbx_match_bow_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_f,
                                const orbx_keypoint* d_kps, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                                const uint32_t* d_fv_node, const uint32_t* d_fv_feat, const int32_t* d_fv_n, const uint8_t* d_kf_mask,
                                float nnratio, int check_orientation, int32_t* d_matches_f, int32_t* d_nmatches) {
  if (n_frames < 0 || n_pairs < 0 || capacity < 1 || (n_pairs > 0 && (!h_kf || !h_f)) || !d_kps || !d_desc32 || !d_n || !d_fv_node ||
      !d_fv_feat || !d_fv_n || !d_matches_f || !d_nmatches)
    return ORBX_E_BADARG;
  if (!pairsInRange(h_kf, h_f, n_pairs, n_frames)) {
    if (ctx) ctxSetError(ctx, "match bow: pair index outside [0, n_frames)");
    return ORBX_E_BADARG;
  }
  if (capacity > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "match bow: capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  HIPCHK(HeldUploads(st)(s->pairs, {h_kf, h_f}, n_pairs));
  MatchBowArgs a{};
  a.kps = d_kps;
  a.desc = d_desc32;
  a.n = d_n;
  a.fvNode = d_fv_node;
  a.fvFeat = d_fv_feat;
  a.fvN = d_fv_n;
  a.mask = d_kf_mask;
  a.pairs = s->pairs;
  a.cap = capacity;
  a.nPairs = n_pairs;
  a.checkOri = check_orientation != 0;
  a.nnratio = nnratio;
  a.matchesF = d_matches_f;
  a.nmatches = d_nmatches;
  HIPCHK(launch_match_bow(st, a));
  return ORBX_OK;
}

int orbx_match_bow(orbx_ctx* ctx, const orbx_keypoint* kf_kps, const uint8_t* kf_desc32, int kf_n, const uint32_t* kf_fv_node,
                   const uint32_t* kf_fv_feat, int kf_fv_n, const orbx_keypoint* f_kps, const uint8_t* f_desc32, int f_n,
                   const uint32_t* f_fv_node, const uint32_t* f_fv_feat, int f_fv_n, const uint8_t* kf_mask, float nnratio,
                   int check_orientation, int32_t* matches_f, int32_t* nmatches) {
  if (kf_n < 0 || f_n < 0 || kf_fv_n < 0 || f_fv_n < 0 || !nmatches || (kf_n > 0 && (!kf_kps || !kf_desc32)) ||
      (f_n > 0 && (!f_kps || !f_desc32 || !matches_f)) || (kf_fv_n > 0 && (!kf_fv_node || !kf_fv_feat)) ||
      (f_fv_n > 0 && (!f_fv_node || !f_fv_feat)))
    return ORBX_E_BADARG;
  const int cap = std::max(std::max(std::max(kf_n, f_n), std::max(kf_fv_n, f_fv_n)), 1);
  if (cap > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "match bow: more than ORBX_BOW_MAX_FEATURES features");
    return ORBX_E_CAPACITY;
  }
  if (!featuresOk(kf_fv_feat, kf_fv_n, kf_n) || !featuresOk(f_fv_feat, f_fv_n, f_n)) {
    if (ctx) ctxSetError(ctx, "match bow: a FeatureVector names a feature the frame does not have");
    return ORBX_E_BADARG;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const size_t c = (size_t)cap;
  const int32_t hn[4] = {kf_n, f_n, kf_fv_n, f_fv_n};
  Staged io(ctxIo(ctx), ctxStream(ctx));  // the two frames (keyframe 0, frame 1) in the batch layout, then the results
  auto dK = io.in(kf_kps, kf_n, 2 * c);
  io.in(dK, c, f_kps, f_n);
  auto dD = io.in(kf_desc32, (size_t)kf_n * 32, 2 * c * 32);
  io.in(dD, c * 32, f_desc32, (size_t)f_n * 32);
  auto dNode = io.in(kf_fv_node, kf_fv_n, 2 * c);
  io.in(dNode, c, f_fv_node, f_fv_n);
  auto dFeat = io.in(kf_fv_feat, kf_fv_n, 2 * c);
  io.in(dFeat, c, f_fv_feat, f_fv_n);
  auto dMask = io.optIn(kf_mask, kf_n, 2 * c);
  auto dN = io.in(hn, 4, 5);  // n[2], fv_n[2], nmatches
  io.out(dN, 4, nmatches, 1);
  auto dM = io.out(matches_f, f_n, c);
  HIPCHK(io.open());
  const int32_t kf = 0, f = 1;
  r = orbx_match_bow_batch_device(ctx, 2, 1, &kf, &f, io[dK], io[dD], io[dN], cap, io[dNode], io[dFeat], io[dN] + 2, io[dMask], nnratio,
                                  check_orientation, io[dM], io[dN] + 4);
  return io.close(ctx, r);
}

int orbx_match_triangulation_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf1, const int32_t* h_kf2,
                                          const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                                          const uint32_t* d_fv_node, const uint32_t* d_fv_feat, const int32_t* d_fv_n,
                                          const uint8_t* d_mask, const float* d_pose, const float* K, const float* d_median_depth,
                                          int check_orientation, int32_t* d_matches12, orbx_tri_match_result* d_res) {
  if (n_frames < 0 || n_pairs < 0 || capacity < 1 || (n_pairs > 0 && (!h_kf1 || !h_kf2)) || !d_kps_un || !d_desc32 || !d_n ||
      !d_fv_node || !d_fv_feat || !d_fv_n || !d_pose || !K || !d_matches12 || !d_res)
    return ORBX_E_BADARG;
  int r = triRefused(ctx, "match triangulation", n_frames, n_pairs, h_kf1, h_kf2, capacity, K);
  if (r != ORBX_OK) return r;
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  TriScratch* s = ctxTri(ctx);
  hipStream_t st = ctxStream(ctx);
  HIPCHK(HeldUploads(st)(s->pairs, {h_kf1, h_kf2}, n_pairs));  // (the two calls take the same list: the chain uploads it once)
  MatchTriArgs a{};
  a.kps = d_kps_un;
  a.desc = d_desc32;
  a.n = d_n;
  a.fvNode = d_fv_node;
  a.fvFeat = d_fv_feat;
  a.fvN = d_fv_n;
  a.mask = d_mask;
  a.pose = d_pose;
  a.medianDepth = d_median_depth;
  a.pairs = s->pairs;
  a.cap = capacity;
  a.nPairs = n_pairs;
  a.checkOri = check_orientation != 0;
  a.cam = triCam(ctx, K);
  a.matches12 = d_matches12;
  a.res = d_res;
  HIPCHK(launch_match_tri(st, a));
  return ORBX_OK;
}

int orbx_triangulate_matches_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf1, const int32_t* h_kf2,
                                          const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const float* d_pose,
                                          const float* K, const int32_t* d_matches12, float* d_points, uint8_t* d_point_mask,
                                          float* d_point_normal, float* d_point_dist, orbx_tri_result* d_res) {
  if (n_frames < 0 || n_pairs < 0 || capacity < 1 || (n_pairs > 0 && (!h_kf1 || !h_kf2)) || !d_kps_un || !d_n || !d_pose || !K ||
      !d_matches12 || !d_points || !d_point_mask || !d_point_normal || !d_point_dist || !d_res)
    return ORBX_E_BADARG;
  int r = triRefused(ctx, "triangulate matches", n_frames, n_pairs, h_kf1, h_kf2, capacity, K);
  if (r != ORBX_OK) return r;
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  TriScratch* s = ctxTri(ctx);
  hipStream_t st = ctxStream(ctx);
  HIPCHK(HeldUploads(st)(s->pairs, {h_kf1, h_kf2}, n_pairs));  // (the two calls take the same list: the chain uploads it once)
  TriangulateArgs a{};
  a.kps = d_kps_un;
  a.n = d_n;
  a.pose = d_pose;
  a.pairs = s->pairs;
  a.matches12 = d_matches12;
  a.cap = capacity;
  a.nPairs = n_pairs;
  a.cam = triCam(ctx, K);
  a.points = d_points;
  a.pointMask = d_point_mask;
  a.pointNormal = d_point_normal;
  a.pointDist = d_point_dist;
  a.res = d_res;
  HIPCHK(launch_triangulate(st, a));
  return ORBX_OK;
}

int orbx_match_triangulation(orbx_ctx* ctx, const orbx_keypoint* kps_un1, const uint8_t* desc1, int n1, const uint32_t* fv_node1,
                             const uint32_t* fv_feat1, int fv_n1, const uint8_t* mask1, const float* pose1,
                             const orbx_keypoint* kps_un2, const uint8_t* desc2, int n2, const uint32_t* fv_node2,
                             const uint32_t* fv_feat2, int fv_n2, const uint8_t* mask2, const float* pose2, const float* K,
                             float median_depth2, int check_orientation, int32_t* matches12, orbx_tri_match_result* res) {
  if (n1 < 0 || n2 < 0 || fv_n1 < 0 || fv_n2 < 0 || !pose1 || !pose2 || !K || !res || (n1 > 0 && (!kps_un1 || !desc1 || !matches12)) ||
      (n2 > 0 && (!kps_un2 || !desc2)) || (fv_n1 > 0 && (!fv_node1 || !fv_feat1)) || (fv_n2 > 0 && (!fv_node2 || !fv_feat2)))
    return ORBX_E_BADARG;
  const int cap = std::max(std::max(std::max(n1, n2), std::max(fv_n1, fv_n2)), 1);
  const int32_t kf1 = 0, kf2 = 1;
  int r = triRefused(ctx, "match triangulation", 2, 1, &kf1, &kf2, cap, K);
  if (r != ORBX_OK) return r;
  if (!featuresOk(fv_feat1, fv_n1, n1) || !featuresOk(fv_feat2, fv_n2, n2)) {
    if (ctx) ctxSetError(ctx, "match triangulation: a FeatureVector names a feature the keyframe does not have");
    return ORBX_E_BADARG;
  }
  if (!ctx) return ORBX_E_HIP;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const size_t c = (size_t)cap;
  const bool gate = median_depth2 > 0.0f;
  const float hMed[2] = {0.0f, median_depth2};
  const int32_t hn[4] = {n1, n2, fv_n1, fv_n2};
  Staged io(ctxIo(ctx), ctxStream(ctx));  // the two keyframes (KF1 0, KF2 1) in the batch layout, then the results
  auto dK = io.in(kps_un1, n1, 2 * c);
  io.in(dK, c, kps_un2, n2);
  auto dD = io.in(desc1, (size_t)n1 * 32, 2 * c * 32);
  io.in(dD, c * 32, desc2, (size_t)n2 * 32);
  auto dNode = io.in(fv_node1, fv_n1, 2 * c);
  io.in(dNode, c, fv_node2, fv_n2);
  auto dFeat = io.in(fv_feat1, fv_n1, 2 * c);
  io.in(dFeat, c, fv_feat2, fv_n2);
  auto dMask = io.optIn(mask1, n1, 2 * c);
  io.in(dMask, c, mask2, n2);
  dMask.absent = !mask1 && !mask2;  // (either keyframe may bring one alone: the other's stays zero)
  auto dPose = io.in(pose1, 12, 24);
  io.in(dPose, 12, pose2, 12);
  auto dMed = io.optIn(gate ? hMed : nullptr, 2, 2);
  auto dN = io.in(hn, 4, 4);  // n[2], fv_n[2]
  auto dM = io.out(matches12, n1, c);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  r = orbx_match_triangulation_batch_device(ctx, 2, 1, &kf1, &kf2, io[dK], io[dD], io[dN], cap, io[dNode], io[dFeat], io[dN] + 2,
                                            io[dMask], io[dPose], K, io[dMed], check_orientation, io[dM], io[dR]);
  return io.close(ctx, r);
}

int orbx_triangulate_matches(orbx_ctx* ctx, const orbx_keypoint* kps_un1, int n1, const float* pose1, const orbx_keypoint* kps_un2,
                             int n2, const float* pose2, const float* K, const int32_t* matches12, float* points, uint8_t* point_mask,
                             float* point_normal, float* point_dist, orbx_tri_result* res) {
  if (n1 < 0 || n2 < 0 || !pose1 || !pose2 || !K || !res ||
      (n1 > 0 && (!kps_un1 || !matches12 || !points || !point_mask || !point_normal || !point_dist)) || (n2 > 0 && !kps_un2))
    return ORBX_E_BADARG;
  const int cap = std::max(std::max(n1, n2), 1);
  const int32_t kf1 = 0, kf2 = 1;
  int r = triRefused(ctx, "triangulate matches", 2, 1, &kf1, &kf2, cap, K);
  if (r != ORBX_OK) return r;
  if (!ctx) return ORBX_E_HIP;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const size_t c = (size_t)cap;
  const int32_t hn[2] = {n1, n2};
  Staged io(ctxIo(ctx), ctxStream(ctx));  // the two keyframes in the batch layout, the matches, then the point set and the record
  auto dK = io.in(kps_un1, n1, 2 * c);
  io.in(dK, c, kps_un2, n2);
  auto dPose = io.in(pose1, 12, 24);
  io.in(dPose, 12, pose2, 12);
  auto dN = io.in(hn, 2, 2);
  auto dM = io.in(matches12, n1, c);
  io.fill(dM, 0xff, c);  // (entries at and beyond n1: no match)
  auto dP = io.out(points, (size_t)n1 * 3, c * 3);
  auto dMask = io.out(point_mask, n1, c);
  auto dNrm = io.out(point_normal, (size_t)n1 * 3, c * 3);
  auto dDist = io.out(point_dist, (size_t)n1 * 2, c * 2);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open());
  r = orbx_triangulate_matches_batch_device(ctx, 2, 1, &kf1, &kf2, io[dK], io[dN], cap, io[dPose], K, io[dM], io[dP], io[dMask],
                                            io[dNrm], io[dDist], io[dR]);
  return io.close(ctx, r);
}

}  // extern "C"
