// orbx_match_bow.cpp — host side of ORBmatcher::SearchByBoW (include/orbx.h, "matching through the FeatureVector"), of
// ORBmatcher::SearchByProjection ("matching by projection"), of Tracking::SearchLocalPoints ("matching the local map by
// projection") and of the relocalisation overload ("matching a keyframe's points by projection"): the argument checks, the pair
// lists and the C entry points.  The kernels are in orbx_match_bow_kernel.hip, orbx_match_proj_kernel.hip,
// orbx_match_local_kernel.hip and orbx_match_kfproj_kernel.hip.
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
  // the pair list goes up only when it differs from the last call's.  Such a call first waits for the context stream -- the host
  // copy an earlier upload may still be reading is replaced -- and is the documented exception to "returns once queued"
  if (!s->pairs.holds(h_kf, n_pairs, h_f, n_pairs)) {
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(s->pairs.replace(st, h_kf, n_pairs, h_f, n_pairs));
  }
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
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  orbx_keypoint* dK;
  uint8_t *dD, *dMask;
  uint32_t *dNode, *dFeat;
  int32_t *dN, *dM;
  auto staging = [&](Layout L) {  // the two frames (keyframe 0, frame 1) in the batch layout, then the results
    dK = L.take<orbx_keypoint>((size_t)2 * cap);
    dD = L.take<uint8_t>((size_t)2 * cap * 32);
    dNode = L.take<uint32_t>((size_t)2 * cap);
    dFeat = L.take<uint32_t>((size_t)2 * cap);
    dMask = L.take<uint8_t>((size_t)2 * cap);
    dN = L.take<int32_t>(5);  // n[2], fv_n[2], nmatches
    dM = L.take<int32_t>(cap);
    return L.size();
  };
  HIPCHK(s->dIo.grow(staging(Layout()), st));
  staging(Layout(s->dIo));
  const size_t c = (size_t)cap;
  HIPCHK(up(dK, kf_kps, kf_n, st));
  HIPCHK(up(dD, kf_desc32, (size_t)kf_n * 32, st));
  if (kf_mask) HIPCHK(up(dMask, kf_mask, kf_n, st));
  HIPCHK(up(dK + c, f_kps, f_n, st));
  HIPCHK(up(dD + c * 32, f_desc32, (size_t)f_n * 32, st));
  HIPCHK(up(dNode, kf_fv_node, kf_fv_n, st));
  HIPCHK(up(dFeat, kf_fv_feat, kf_fv_n, st));
  HIPCHK(up(dNode + c, f_fv_node, f_fv_n, st));
  HIPCHK(up(dFeat + c, f_fv_feat, f_fv_n, st));
  const int32_t hn[4] = {kf_n, f_n, kf_fv_n, f_fv_n};
  HIPCHK(up(dN, hn, 4, st));
  const int32_t kf = 0, f = 1;
  r = orbx_match_bow_batch_device(ctx, 2, 1, &kf, &f, dK, dD, dN, cap, dNode, dFeat, dN + 2, kf_mask ? dMask : nullptr, nnratio,
                                  check_orientation, dM, dN + 4);
  if (r != ORBX_OK) return r;
  HIPCHK(down(matches_f, dM, f_n, st));
  HIPCHK(down(nmatches, dN + 4, 1, st));
  HIPCHK(hipStreamSynchronize(st));
  return ORBX_OK;
}

int orbx_match_projection_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_last, const int32_t* h_cur,
                                       const int32_t* h_point_set, const orbx_keypoint* d_kps_un, const uint8_t* d_desc32,
                                       const int32_t* d_n, int capacity, int n_point_sets, const float* d_points,
                                       const uint8_t* d_point_mask, const uint8_t* d_point_desc32, const uint8_t* d_last_outlier,
                                       const float* d_pose_cur, const float* K, const orbx_bounds* bounds, float th,
                                       int check_orientation, int32_t* d_matches_cur, orbx_proj_result* d_res) {
  if (n_frames < 0 || n_pairs < 0 || n_point_sets < 0 || capacity < 1 || (n_pairs > 0 && (!h_last || !h_cur || !h_point_set)) ||
      !d_kps_un || !d_desc32 || !d_n || !d_points || !d_pose_cur || !K || !bounds || !d_matches_cur || !d_res)
    return ORBX_E_BADARG;
  if (!std::isfinite(th) || !(th > 0.0f)) {
    if (ctx) ctxSetError(ctx, "match projection: th is not a positive number");
    return ORBX_E_BADARG;
  }
  // (max - min is an int in Frame's grid: it has to be one)
  if ((long long)bounds->max_x - bounds->min_x < 1 || (long long)bounds->max_x - bounds->min_x > INT32_MAX ||
      (long long)bounds->max_y - bounds->min_y < 1 || (long long)bounds->max_y - bounds->min_y > INT32_MAX) {
    if (ctx) ctxSetError(ctx, "match projection: bounds with max <= min");
    return ORBX_E_BADARG;
  }
  if (!pairsInRange(h_last, h_cur, n_pairs, n_frames) || !pairsInRange(h_cur, h_point_set, n_pairs, n_frames, n_point_sets)) {
    if (ctx) ctxSetError(ctx, "match projection: frame outside [0, n_frames) or point set outside [0, n_point_sets)");
    return ORBX_E_BADARG;
  }
  if (capacity > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "match projection: capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  // the three lists as one array, held as orbx_match_bow_batch_device holds its two: uploaded only when they differ from the
  // last call's, behind a wait for the context stream
  std::vector<int32_t> lists;
  lists.reserve((size_t)3 * n_pairs);
  lists.insert(lists.end(), h_last, h_last + n_pairs);
  lists.insert(lists.end(), h_cur, h_cur + n_pairs);
  lists.insert(lists.end(), h_point_set, h_point_set + n_pairs);
  if (!s->projPairs.holds(lists.data(), lists.size())) {
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(s->projPairs.replace(st, lists.data(), lists.size()));
  }
  MatchProjArgs a{};
  a.kps = d_kps_un;
  a.desc = d_desc32;
  a.n = d_n;
  a.points = d_points;
  a.pointMask = d_point_mask;
  a.pointDesc = d_point_desc32;
  a.lastOutlier = d_last_outlier;
  a.pose = d_pose_cur;
  a.pairs = s->projPairs;
  a.cap = capacity;
  a.nPairs = n_pairs;
  a.checkOri = check_orientation != 0;
  a.fx = K[0];
  a.fy = K[4];
  a.cx = K[2];
  a.cy = K[5];
  a.th = th;
  a.b = *bounds;
  const float* scale = ctxScale(ctx, &a.nLevels);
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) a.scale[l] = l < a.nLevels ? scale[l] : 0.0f;
  a.matchesCur = d_matches_cur;
  a.res = d_res;
  HIPCHK(launch_match_proj(st, a));
  return ORBX_OK;
}

int orbx_match_projection(orbx_ctx* ctx, const orbx_keypoint* last_kps_un, const uint8_t* last_desc32, int last_n,
                          const orbx_keypoint* cur_kps_un, const uint8_t* cur_desc32, int cur_n, const float* points,
                          const uint8_t* mask, const uint8_t* point_desc32, const uint8_t* last_outlier, const float* pose_cur,
                          const float* K, const orbx_bounds* bounds, float th, int check_orientation, int32_t* matches_cur,
                          orbx_proj_result* res) {
  if (last_n < 0 || cur_n < 0 || !pose_cur || !K || !bounds || !res || (last_n > 0 && (!last_kps_un || !last_desc32 || !points)) ||
      (cur_n > 0 && (!cur_kps_un || !cur_desc32 || !matches_cur)))
    return ORBX_E_BADARG;
  const int cap = std::max(std::max(last_n, cur_n), 1);
  if (cap > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "match projection: more than ORBX_BOW_MAX_FEATURES features");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  orbx_keypoint* dK;
  uint8_t *dD, *dPD, *dMask, *dOut;
  float *dP, *dPose;
  int32_t *dN, *dM;
  orbx_proj_result* dR;
  auto staging = [&](Layout L) {  // the two frames (last 0, current 1) and one point set in the batch layout, then the results
    dK = L.take<orbx_keypoint>((size_t)2 * cap);
    dD = L.take<uint8_t>((size_t)2 * cap * 32);
    dP = L.take<float>((size_t)cap * 3);
    dPD = L.take<uint8_t>((size_t)cap * 32);
    dMask = L.take<uint8_t>(cap);
    dOut = L.take<uint8_t>(cap);
    dPose = L.take<float>(12);
    dN = L.take<int32_t>(2);
    dM = L.take<int32_t>(cap);
    dR = L.take<orbx_proj_result>(1);
    return L.size();
  };
  const size_t bytes = staging(Layout());
  HIPCHK(s->dProjIo.grow(bytes, st));
  staging(Layout(s->dProjIo));
  HIPCHK(hipMemsetAsync(s->dProjIo, 0, bytes, st));
  const size_t c = (size_t)cap;
  HIPCHK(up(dK, last_kps_un, last_n, st));
  HIPCHK(up(dD, last_desc32, (size_t)last_n * 32, st));
  HIPCHK(up(dK + c, cur_kps_un, cur_n, st));
  HIPCHK(up(dD + c * 32, cur_desc32, (size_t)cur_n * 32, st));
  HIPCHK(up(dP, points, (size_t)last_n * 3, st));
  if (point_desc32) HIPCHK(up(dPD, point_desc32, (size_t)last_n * 32, st));
  if (mask) HIPCHK(up(dMask, mask, last_n, st));
  if (last_outlier) HIPCHK(up(dOut, last_outlier, last_n, st));
  HIPCHK(up(dPose, pose_cur, 12, st));
  const int32_t hn[2] = {last_n, cur_n};
  HIPCHK(up(dN, hn, 2, st));
  const int32_t last = 0, cur = 1, set = 0;
  r = orbx_match_projection_batch_device(ctx, 2, 1, &last, &cur, &set, dK, dD, dN, cap, 1, dP, mask ? dMask : nullptr,
                                         point_desc32 ? dPD : nullptr, last_outlier ? dOut : nullptr, dPose, K, bounds, th,
                                         check_orientation, dM, dR);
  if (r != ORBX_OK) {
    (void)hipStreamSynchronize(st);  // (the uploads queued above read this frame's variables)
    return r;
  }
  HIPCHK(down(matches_cur, dM, cur_n, st));
  HIPCHK(down(res, dR, 1, st));
  HIPCHK(hipStreamSynchronize(st));
  return ORBX_OK;
}

int orbx_match_local_map_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_frame, const int32_t* h_map_set,
                                      const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                                      int n_map_sets, int map_capacity, const int32_t* d_map_n, const float* d_map_points,
                                      const float* d_map_normals, const float* d_map_dist, const uint8_t* d_map_desc32,
                                      const uint8_t* d_map_mask, const float* d_pose, const float* K, const orbx_bounds* bounds,
                                      float th, float nnratio, int32_t* d_matches, const uint8_t* d_outlier, uint8_t* d_point_view,
                                      orbx_local_result* d_res) {
  if (n_frames < 0 || n_pairs < 0 || n_map_sets < 0 || capacity < 1 || map_capacity < 1 || (n_pairs > 0 && (!h_frame || !h_map_set)) ||
      !d_kps_un || !d_desc32 || !d_n || !d_map_n || !d_map_points || !d_map_normals || !d_map_dist || !d_map_desc32 || !d_pose || !K ||
      !bounds || !d_matches || !d_res)
    return ORBX_E_BADARG;
  if (!std::isfinite(th) || !(th > 0.0f)) {
    if (ctx) ctxSetError(ctx, "match local map: th is not a positive number");
    return ORBX_E_BADARG;
  }
  if (!(nnratio > 0.0f && nnratio <= 1.0f)) {
    if (ctx) ctxSetError(ctx, "match local map: nnratio outside (0, 1]");
    return ORBX_E_BADARG;
  }
  // (max - min is an int in Frame's grid: it has to be one)
  if ((long long)bounds->max_x - bounds->min_x < 1 || (long long)bounds->max_x - bounds->min_x > INT32_MAX ||
      (long long)bounds->max_y - bounds->min_y < 1 || (long long)bounds->max_y - bounds->min_y > INT32_MAX) {
    if (ctx) ctxSetError(ctx, "match local map: bounds with max <= min");
    return ORBX_E_BADARG;
  }
  if (!pairsInRange(h_frame, h_map_set, n_pairs, n_frames, n_map_sets)) {
    if (ctx) ctxSetError(ctx, "match local map: frame outside [0, n_frames) or map set outside [0, n_map_sets)");
    return ORBX_E_BADARG;
  }
  if (capacity > ORBX_BOW_MAX_FEATURES || map_capacity > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "match local map: capacity or map_capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  // the two lists as one array, held as orbx_match_projection_batch_device holds its three
  std::vector<int32_t> lists;
  lists.reserve((size_t)2 * n_pairs);
  lists.insert(lists.end(), h_frame, h_frame + n_pairs);
  lists.insert(lists.end(), h_map_set, h_map_set + n_pairs);
  if (!s->localPairs.holds(lists.data(), lists.size())) {
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(s->localPairs.replace(st, lists.data(), lists.size()));
  }
  MatchLocalArgs a{};
  a.kps = d_kps_un;
  a.desc = d_desc32;
  a.n = d_n;
  a.mapN = d_map_n;
  a.mapPoints = d_map_points;
  a.mapNormals = d_map_normals;
  a.mapDist = d_map_dist;
  a.mapDesc = d_map_desc32;
  a.mapMask = d_map_mask;
  a.outlier = d_outlier;
  a.pose = d_pose;
  a.pairs = s->localPairs;
  a.cap = capacity;
  a.mapCap = map_capacity;
  a.nPairs = n_pairs;
  a.fx = K[0];
  a.fy = K[4];
  a.cx = K[2];
  a.cy = K[5];
  a.th = th;
  a.nnratio = nnratio;
  a.b = *bounds;
  const float* scale = ctxScale(ctx, &a.nLevels);
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) a.scale[l] = l < a.nLevels ? scale[l] : 0.0f;
  a.matches = d_matches;
  a.pointView = d_point_view;
  a.res = d_res;
  HIPCHK(launch_match_local(st, a));
  return ORBX_OK;
}

int orbx_match_local_map(orbx_ctx* ctx, const orbx_keypoint* kps_un, const uint8_t* desc32, int n, int map_n,
                         const float* map_points, const float* map_normals, const float* map_dist, const uint8_t* map_desc32,
                         const uint8_t* map_mask, const float* pose, const float* K, const orbx_bounds* bounds, float th,
                         float nnratio, int32_t* matches, const uint8_t* outlier, uint8_t* point_view, orbx_local_result* res) {
  if (n < 0 || map_n < 0 || !pose || !K || !bounds || !res || (n > 0 && (!kps_un || !desc32 || !matches)) ||
      (map_n > 0 && (!map_points || !map_normals || !map_dist || !map_desc32)))
    return ORBX_E_BADARG;
  const int cap = std::max(n, 1), mapCap = std::max(map_n, 1);
  if (cap > ORBX_BOW_MAX_FEATURES || mapCap > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "match local map: more than ORBX_BOW_MAX_FEATURES features or points");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  orbx_keypoint* dK;
  uint8_t *dD, *dMD, *dMask, *dOut, *dView;
  float *dP, *dNrm, *dDist, *dPose;
  int32_t *dN, *dM;
  orbx_local_result* dR;
  auto staging = [&](Layout L) {  // one frame and one map set in the batch layout, then the results
    dK = L.take<orbx_keypoint>(cap);
    dD = L.take<uint8_t>((size_t)cap * 32);
    dMD = L.take<uint8_t>((size_t)mapCap * 32);
    dP = L.take<float>((size_t)mapCap * 3);
    dNrm = L.take<float>((size_t)mapCap * 3);
    dDist = L.take<float>((size_t)mapCap * 2);
    dMask = L.take<uint8_t>(mapCap);
    dOut = L.take<uint8_t>(cap);
    dView = L.take<uint8_t>(mapCap);
    dPose = L.take<float>(12);
    dN = L.take<int32_t>(2);
    dM = L.take<int32_t>(cap);
    dR = L.take<orbx_local_result>(1);
    return L.size();
  };
  const size_t bytes = staging(Layout());
  HIPCHK(s->dLocalIo.grow(bytes, st));
  staging(Layout(s->dLocalIo));
  HIPCHK(hipMemsetAsync(s->dLocalIo, 0, bytes, st));
  HIPCHK(up(dK, kps_un, n, st));
  HIPCHK(up(dD, desc32, (size_t)n * 32, st));
  HIPCHK(up(dM, matches, n, st));
  HIPCHK(up(dMD, map_desc32, (size_t)map_n * 32, st));
  HIPCHK(up(dP, map_points, (size_t)map_n * 3, st));
  HIPCHK(up(dNrm, map_normals, (size_t)map_n * 3, st));
  HIPCHK(up(dDist, map_dist, (size_t)map_n * 2, st));
  if (map_mask) HIPCHK(up(dMask, map_mask, map_n, st));
  if (outlier) HIPCHK(up(dOut, outlier, n, st));
  HIPCHK(up(dPose, pose, 12, st));
  const int32_t hn[2] = {n, map_n};
  HIPCHK(up(dN, hn, 2, st));
  const int32_t frame = 0, set = 0;
  r = orbx_match_local_map_batch_device(ctx, 1, 1, &frame, &set, dK, dD, dN, cap, 1, mapCap, dN + 1, dP, dNrm, dDist, dMD,
                                        map_mask ? dMask : nullptr, dPose, K, bounds, th, nnratio, dM, outlier ? dOut : nullptr,
                                        point_view ? dView : nullptr, dR);
  if (r != ORBX_OK) {
    (void)hipStreamSynchronize(st);  // (the uploads queued above read this frame's variables)
    return r;
  }
  HIPCHK(down(matches, dM, n, st));
  if (point_view) HIPCHK(down(point_view, dView, map_n, st));
  HIPCHK(down(res, dR, 1, st));
  HIPCHK(hipStreamSynchronize(st));
  return ORBX_OK;
}

int orbx_match_keyframe_projection_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_cur,
                                                const int32_t* h_point_set, const orbx_keypoint* d_kps_un, const uint8_t* d_desc32,
                                                const int32_t* d_n, int capacity, int n_point_sets, const float* d_points,
                                                const uint8_t* d_point_mask, const uint8_t* d_point_desc32, const float* d_point_dist,
                                                const float* d_pose, const float* K, const orbx_bounds* bounds, float th, int orb_dist,
                                                int check_orientation, int32_t* d_matches, const uint8_t* d_outlier,
                                                orbx_kfproj_result* d_res) {
  if (n_frames < 0 || n_pairs < 0 || n_point_sets < 0 || capacity < 1 || (n_pairs > 0 && (!h_kf || !h_cur || !h_point_set)) ||
      !d_kps_un || !d_desc32 || !d_n || !d_points || !d_point_dist || !d_pose || !K || !bounds || !d_matches || !d_res)
    return ORBX_E_BADARG;
  if (!std::isfinite(th) || !(th > 0.0f)) {
    if (ctx) ctxSetError(ctx, "match keyframe projection: th is not a positive number");
    return ORBX_E_BADARG;
  }
  if (orb_dist < 0 || orb_dist > 256) {
    if (ctx) ctxSetError(ctx, "match keyframe projection: orb_dist outside [0, 256]");
    return ORBX_E_BADARG;
  }
  // (max - min is an int in Frame's grid: it has to be one)
  if ((long long)bounds->max_x - bounds->min_x < 1 || (long long)bounds->max_x - bounds->min_x > INT32_MAX ||
      (long long)bounds->max_y - bounds->min_y < 1 || (long long)bounds->max_y - bounds->min_y > INT32_MAX) {
    if (ctx) ctxSetError(ctx, "match keyframe projection: bounds with max <= min");
    return ORBX_E_BADARG;
  }
  if (!pairsInRange(h_kf, h_cur, n_pairs, n_frames) || !pairsInRange(h_cur, h_point_set, n_pairs, n_frames, n_point_sets)) {
    if (ctx) ctxSetError(ctx, "match keyframe projection: frame outside [0, n_frames) or point set outside [0, n_point_sets)");
    return ORBX_E_BADARG;
  }
  if (capacity > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "match keyframe projection: capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  // the three lists as one array, held as orbx_match_projection_batch_device holds its three
  std::vector<int32_t> lists;
  lists.reserve((size_t)3 * n_pairs);
  lists.insert(lists.end(), h_kf, h_kf + n_pairs);
  lists.insert(lists.end(), h_cur, h_cur + n_pairs);
  lists.insert(lists.end(), h_point_set, h_point_set + n_pairs);
  if (!s->kfProjPairs.holds(lists.data(), lists.size())) {
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(s->kfProjPairs.replace(st, lists.data(), lists.size()));
  }
  MatchKfProjArgs a{};
  a.kps = d_kps_un;
  a.desc = d_desc32;
  a.n = d_n;
  a.points = d_points;
  a.pointMask = d_point_mask;
  a.pointDesc = d_point_desc32;
  a.pointDist = d_point_dist;
  a.outlier = d_outlier;
  a.pose = d_pose;
  a.pairs = s->kfProjPairs;
  a.cap = capacity;
  a.nPairs = n_pairs;
  a.orbDist = orb_dist;
  a.checkOri = check_orientation != 0;
  a.fx = K[0];
  a.fy = K[4];
  a.cx = K[2];
  a.cy = K[5];
  a.th = th;
  a.b = *bounds;
  const float* scale = ctxScale(ctx, &a.nLevels);
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) a.scale[l] = l < a.nLevels ? scale[l] : 0.0f;
  a.matches = d_matches;
  a.res = d_res;
  HIPCHK(launch_match_kfproj(st, a));
  return ORBX_OK;
}

int orbx_match_keyframe_projection(orbx_ctx* ctx, const orbx_keypoint* kf_kps_un, const uint8_t* kf_desc32, int kf_n,
                                   const orbx_keypoint* cur_kps_un, const uint8_t* cur_desc32, int cur_n, const float* points,
                                   const uint8_t* mask, const uint8_t* point_desc32, const float* point_dist, const float* pose,
                                   const float* K, const orbx_bounds* bounds, float th, int orb_dist, int check_orientation,
                                   int32_t* matches, const uint8_t* outlier, orbx_kfproj_result* res) {
  if (kf_n < 0 || cur_n < 0 || !pose || !K || !bounds || !res || (kf_n > 0 && (!kf_kps_un || !kf_desc32 || !points || !point_dist)) ||
      (cur_n > 0 && (!cur_kps_un || !cur_desc32 || !matches)))
    return ORBX_E_BADARG;
  const int cap = std::max(std::max(kf_n, cur_n), 1);
  if (cap > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "match keyframe projection: more than ORBX_BOW_MAX_FEATURES features");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  orbx_keypoint* dK;
  uint8_t *dD, *dPD, *dMask, *dOut;
  float *dP, *dDist, *dPose;
  int32_t *dN, *dM;
  orbx_kfproj_result* dR;
  auto staging = [&](Layout L) {  // the two frames (keyframe 0, current 1) and one point set in the batch layout, then the results
    dK = L.take<orbx_keypoint>((size_t)2 * cap);
    dD = L.take<uint8_t>((size_t)2 * cap * 32);
    dP = L.take<float>((size_t)cap * 3);
    dDist = L.take<float>((size_t)cap * 2);
    dPD = L.take<uint8_t>((size_t)cap * 32);
    dMask = L.take<uint8_t>(cap);
    dOut = L.take<uint8_t>(cap);
    dPose = L.take<float>(12);
    dN = L.take<int32_t>(2);
    dM = L.take<int32_t>(cap);
    dR = L.take<orbx_kfproj_result>(1);
    return L.size();
  };
  const size_t bytes = staging(Layout());
  HIPCHK(s->dKfProjIo.grow(bytes, st));
  staging(Layout(s->dKfProjIo));
  HIPCHK(hipMemsetAsync(s->dKfProjIo, 0, bytes, st));
  const size_t c = (size_t)cap;
  HIPCHK(up(dK, kf_kps_un, kf_n, st));
  HIPCHK(up(dD, kf_desc32, (size_t)kf_n * 32, st));
  HIPCHK(up(dK + c, cur_kps_un, cur_n, st));
  HIPCHK(up(dD + c * 32, cur_desc32, (size_t)cur_n * 32, st));
  HIPCHK(up(dP, points, (size_t)kf_n * 3, st));
  HIPCHK(up(dDist, point_dist, (size_t)kf_n * 2, st));
  if (point_desc32) HIPCHK(up(dPD, point_desc32, (size_t)kf_n * 32, st));
  if (mask) HIPCHK(up(dMask, mask, kf_n, st));
  if (outlier) HIPCHK(up(dOut, outlier, cur_n, st));
  HIPCHK(up(dM, matches, cur_n, st));
  HIPCHK(up(dPose, pose, 12, st));
  const int32_t hn[2] = {kf_n, cur_n};
  HIPCHK(up(dN, hn, 2, st));
  const int32_t kf = 0, cur = 1, set = 0;
  r = orbx_match_keyframe_projection_batch_device(ctx, 2, 1, &kf, &cur, &set, dK, dD, dN, cap, 1, dP, mask ? dMask : nullptr,
                                                  point_desc32 ? dPD : nullptr, dDist, dPose, K, bounds, th, orb_dist,
                                                  check_orientation, dM, outlier ? dOut : nullptr, dR);
  if (r != ORBX_OK) {
    (void)hipStreamSynchronize(st);  // (the uploads queued above read this frame's variables)
    return r;
  }
  HIPCHK(down(matches, dM, cur_n, st));
  HIPCHK(down(res, dR, 1, st));
  HIPCHK(hipStreamSynchronize(st));
  return ORBX_OK;
}

}  // extern "C"
