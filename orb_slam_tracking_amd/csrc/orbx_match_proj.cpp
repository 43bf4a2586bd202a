// orbx_match_proj.cpp — host side of the matchers by projection: ORBmatcher::SearchByProjection(CurrentFrame, LastFrame)
// (include/orbx.h, "matching by projection"), Tracking::SearchLocalPoints ("matching the local map by projection") and the
// relocalisation overload ("matching a keyframe's points by projection"): the argument checks, the index lists and the C entry
// points; behind them SearchBySim3 and the loop-closing overload under Scw with its composition.  The kernels are in
// orbx_match_proj_kernel.hip, orbx_match_local_kernel.hip, orbx_match_kfproj_kernel.hip, orbx_match_sim3_kernel.hip and
// orbx_match_scw_kernel.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "orbx_host.h"

using namespace orbx;

namespace {

// What the three batch calls refuse alike, in the order they judge their arguments (all of it before the context): th; `own`,
// the call's own argument; the bounds; `lists`, the index lists; `cap`, the capacities.  own, lists and cap are the complaint,
// or null when there is none.  -> ORBX_OK, or the code with "<name>: <complaint>" left in the context, when there is one.
int refused(orbx_ctx* ctx, const char* name, float th, const char* own, const orbx_bounds* b, const char* lists, const char* cap) {
  const char* why = nullptr;
  // (max - min is an int in Frame's grid: it has to be one)
  const long long w = (long long)b->max_x - b->min_x, h = (long long)b->max_y - b->min_y;
  if (!std::isfinite(th) || !(th > 0.0f)) why = "th is not a positive number";
  else if (own) why = own;
  else if (w < 1 || w > INT32_MAX || h < 1 || h > INT32_MAX) why = "bounds with max <= min";
  else if (lists) why = lists;
  else if (!cap) return ORBX_OK;
  if (ctx) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", name, why ? why : cap);
    ctxSetError(ctx, msg);
  }
  return why ? ORBX_E_BADARG : ORBX_E_CAPACITY;
}

// A call's index lists, each of n_pairs entries, as one array [k][n_pairs] in `held`: uploaded only when they differ from the last
// call's.  Such a call first waits for the context stream -- the host copy an earlier upload may still be reading is replaced --
// and is the documented exception to "returns once queued".
int holdLists(orbx_ctx* ctx, hipStream_t st, HeldArray<int32_t>& held, std::initializer_list<const int32_t*> columns, int nPairs) {
  std::vector<int32_t> lists;
  lists.reserve(columns.size() * nPairs);
  for (const int32_t* c : columns) lists.insert(lists.end(), c, c + nPairs);
  if (!held.holds(lists.data(), lists.size())) {
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(held.replace(st, lists.data(), lists.size()));
  }
  return ORBX_OK;
}

// the camera K[9] (row-major), the radius factor, the bounds and the context's scale factors as the kernels take them
MatchCamArgs camArgs(const orbx_ctx* ctx, const float* K, const orbx_bounds* bounds, float th) {
  MatchCamArgs c{};
  c.fx = K[0];
  c.fy = K[4];
  c.cx = K[2];
  c.cy = K[5];
  c.th = th;
  c.b = *bounds;
  const float* scale = ctxScale(ctx, &c.nLevels);
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) c.scale[l] = l < c.nLevels ? scale[l] : 0.0f;
  return c;
}

}  // namespace

extern "C" {

int orbx_match_projection_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_last, const int32_t* h_cur,
                                       const int32_t* h_point_set, const orbx_keypoint* d_kps_un, const uint8_t* d_desc32,
                                       const int32_t* d_n, int capacity, int n_point_sets, const float* d_points,
                                       const uint8_t* d_point_mask, const uint8_t* d_point_desc32, const uint8_t* d_last_outlier,
                                       const float* d_pose_cur, const float* K, const orbx_bounds* bounds, float th,
                                       int check_orientation, int32_t* d_matches_cur, orbx_proj_result* d_res) {
  if (n_frames < 0 || n_pairs < 0 || n_point_sets < 0 || capacity < 1 || (n_pairs > 0 && (!h_last || !h_cur || !h_point_set)) ||
      !d_kps_un || !d_desc32 || !d_n || !d_points || !d_pose_cur || !K || !bounds || !d_matches_cur || !d_res)
    return ORBX_E_BADARG;
  const bool listsOk = pairsInRange(h_last, h_cur, n_pairs, n_frames) && pairsInRange(h_cur, h_point_set, n_pairs, n_frames, n_point_sets);
  int r = refused(ctx, "match projection", th, nullptr, bounds,
                  listsOk ? nullptr : "frame outside [0, n_frames) or point set outside [0, n_point_sets)",
                  capacity > ORBX_BOW_MAX_FEATURES ? "capacity above ORBX_BOW_MAX_FEATURES" : nullptr);
  if (r != ORBX_OK) return r;
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  r = holdLists(ctx, st, s->projPairs, {h_last, h_cur, h_point_set}, n_pairs);
  if (r != ORBX_OK) return r;
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
  a.cam = camArgs(ctx, K, bounds, th);
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
  int r = refused(ctx, "match local map", th, nnratio > 0.0f && nnratio <= 1.0f ? nullptr : "nnratio outside (0, 1]", bounds,
                  pairsInRange(h_frame, h_map_set, n_pairs, n_frames, n_map_sets)
                      ? nullptr
                      : "frame outside [0, n_frames) or map set outside [0, n_map_sets)",
                  capacity > ORBX_BOW_MAX_FEATURES || map_capacity > ORBX_BOW_MAX_FEATURES
                      ? "capacity or map_capacity above ORBX_BOW_MAX_FEATURES"
                      : nullptr);
  if (r != ORBX_OK) return r;
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  r = holdLists(ctx, st, s->localPairs, {h_frame, h_map_set}, n_pairs);
  if (r != ORBX_OK) return r;
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
  a.nnratio = nnratio;
  a.cam = camArgs(ctx, K, bounds, th);
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
  const bool listsOk = pairsInRange(h_kf, h_cur, n_pairs, n_frames) && pairsInRange(h_cur, h_point_set, n_pairs, n_frames, n_point_sets);
  int r = refused(ctx, "match keyframe projection", th, orb_dist < 0 || orb_dist > 256 ? "orb_dist outside [0, 256]" : nullptr, bounds,
                  listsOk ? nullptr : "frame outside [0, n_frames) or point set outside [0, n_point_sets)",
                  capacity > ORBX_BOW_MAX_FEATURES ? "capacity above ORBX_BOW_MAX_FEATURES" : nullptr);
  if (r != ORBX_OK) return r;
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  r = holdLists(ctx, st, s->kfProjPairs, {h_kf, h_cur, h_point_set}, n_pairs);
  if (r != ORBX_OK) return r;
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
  a.cam = camArgs(ctx, K, bounds, th);
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

// ---- ORBmatcher::SearchBySim3 (include/orbx.h, "loop closing: matching under a similarity"; orbx_match_sim3_kernel.hip)
int orbx_match_sim3_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf1, const int32_t* h_kf2,
                                 const int32_t* h_set1, const int32_t* h_set2, const orbx_keypoint* d_kps_un, const uint8_t* d_desc32,
                                 const int32_t* d_n, int capacity, int n_point_sets, const float* d_points,
                                 const uint8_t* d_point_mask, const uint8_t* d_point_desc32, const float* d_point_dist,
                                 const float* d_pose, const float* d_sim3, const float* K, const orbx_bounds* bounds, float th,
                                 int orb_dist, int32_t* d_matches, orbx_msim3_result* d_res) {
  if (n_frames < 0 || n_pairs < 0 || n_point_sets < 0 || capacity < 1 || (n_pairs > 0 && (!h_kf1 || !h_kf2 || !h_set1 || !h_set2)) ||
      !d_kps_un || !d_desc32 || !d_n || !d_points || !d_point_dist || !d_pose || !d_sim3 || !K || !bounds || !d_matches || !d_res)
    return ORBX_E_BADARG;
  const bool listsOk = pairsInRange(h_kf1, h_kf2, n_pairs, n_frames) && pairsInRange(h_set1, h_set2, n_pairs, n_point_sets);
  int r = refused(ctx, "match sim3", th, orb_dist < 0 || orb_dist > 256 ? "orb_dist outside [0, 256]" : nullptr, bounds,
                  listsOk ? nullptr : "keyframe outside [0, n_frames) or point set outside [0, n_point_sets)",
                  capacity > ORBX_BOW_MAX_FEATURES ? "capacity above ORBX_BOW_MAX_FEATURES" : nullptr);
  if (r != ORBX_OK) return r;
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  r = holdLists(ctx, st, s->sim3Pairs, {h_kf1, h_kf2, h_set1, h_set2}, n_pairs);
  if (r != ORBX_OK) return r;
  MatchSim3Args a{};
  a.kps = d_kps_un;
  a.desc = d_desc32;
  a.n = d_n;
  a.points = d_points;
  a.pointMask = d_point_mask;
  a.pointDesc = d_point_desc32;
  a.pointDist = d_point_dist;
  a.pose = d_pose;
  a.sim3 = d_sim3;
  a.pairs = s->sim3Pairs;
  a.cap = capacity;
  a.nPairs = n_pairs;
  a.orbDist = orb_dist;
  a.cam = camArgs(ctx, K, bounds, th);
  a.matches = d_matches;
  a.res = d_res;
  HIPCHK(launch_match_sim3(st, a));
  return ORBX_OK;
}

int orbx_match_sim3(orbx_ctx* ctx, const orbx_keypoint* kps_un1, const uint8_t* desc1, int n1, const float* points1,
                    const uint8_t* mask1, const uint8_t* point_desc1, const float* point_dist1, const float* pose1,
                    const orbx_keypoint* kps_un2, const uint8_t* desc2, int n2, const float* points2, const uint8_t* mask2,
                    const uint8_t* point_desc2, const float* point_dist2, const float* pose2, const float* sim3, const float* K,
                    const orbx_bounds* bounds, float th, int orb_dist, int32_t* matches12, orbx_msim3_result* res) {
  if (n1 < 0 || n2 < 0 || !pose1 || !pose2 || !sim3 || !K || !bounds || !res ||
      (n1 > 0 && (!kps_un1 || !desc1 || !points1 || !point_dist1 || !matches12)) ||
      (n2 > 0 && (!kps_un2 || !desc2 || !points2 || !point_dist2)) || (mask1 == nullptr) != (mask2 == nullptr) ||
      (point_desc1 == nullptr) != (point_desc2 == nullptr))
    return ORBX_E_BADARG;
  int r = refused(ctx, "match sim3", th, orb_dist < 0 || orb_dist > 256 ? "orb_dist outside [0, 256]" : nullptr, bounds, nullptr, nullptr);
  if (r != ORBX_OK) return r;
  const int cap = std::max(std::max(n1, n2), 1);
  if (cap > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "match sim3: more than ORBX_BOW_MAX_FEATURES features");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  orbx_keypoint* dK;
  uint8_t *dD, *dPD, *dMask;
  float *dP, *dDist, *dPose, *dSim;
  int32_t *dN, *dM;
  orbx_msim3_result* dR;
  auto staging = [&](Layout L) {  // the two keyframes and their point sets in the batch layout, then the results
    dK = L.take<orbx_keypoint>((size_t)2 * cap);
    dD = L.take<uint8_t>((size_t)2 * cap * 32);
    dP = L.take<float>((size_t)2 * cap * 3);
    dDist = L.take<float>((size_t)2 * cap * 2);
    dPD = L.take<uint8_t>((size_t)2 * cap * 32);
    dMask = L.take<uint8_t>((size_t)2 * cap);
    dPose = L.take<float>(24);
    dSim = L.take<float>(13);
    dN = L.take<int32_t>(2);
    dM = L.take<int32_t>(cap);
    dR = L.take<orbx_msim3_result>(1);
    return L.size();
  };
  const size_t bytes = staging(Layout());
  HIPCHK(s->dSim3Io.grow(bytes, st));
  staging(Layout(s->dSim3Io));
  HIPCHK(hipMemsetAsync(s->dSim3Io, 0, bytes, st));
  const size_t c = (size_t)cap;
  HIPCHK(up(dK, kps_un1, n1, st));
  HIPCHK(up(dK + c, kps_un2, n2, st));
  HIPCHK(up(dD, desc1, (size_t)n1 * 32, st));
  HIPCHK(up(dD + c * 32, desc2, (size_t)n2 * 32, st));
  HIPCHK(up(dP, points1, (size_t)n1 * 3, st));
  HIPCHK(up(dP + c * 3, points2, (size_t)n2 * 3, st));
  HIPCHK(up(dDist, point_dist1, (size_t)n1 * 2, st));
  HIPCHK(up(dDist + c * 2, point_dist2, (size_t)n2 * 2, st));
  if (point_desc1) {
    HIPCHK(up(dPD, point_desc1, (size_t)n1 * 32, st));
    HIPCHK(up(dPD + c * 32, point_desc2, (size_t)n2 * 32, st));
  }
  if (mask1) {
    HIPCHK(up(dMask, mask1, n1, st));
    HIPCHK(up(dMask + c, mask2, n2, st));
  }
  HIPCHK(up(dPose, pose1, 12, st));
  HIPCHK(up(dPose + 12, pose2, 12, st));
  HIPCHK(up(dSim, sim3, 13, st));
  HIPCHK(up(dM, matches12, n1, st));
  const int32_t hn[2] = {n1, n2}, zero = 0, one = 1;
  HIPCHK(up(dN, hn, 2, st));
  r = orbx_match_sim3_batch_device(ctx, 2, 1, &zero, &one, &zero, &one, dK, dD, dN, cap, 2, dP, mask1 ? dMask : nullptr,
                                   point_desc1 ? dPD : nullptr, dDist, dPose, dSim, K, bounds, th, orb_dist, dM, dR);
  if (r != ORBX_OK) {
    (void)hipStreamSynchronize(st);  // (the uploads queued above read this frame's variables)
    return r;
  }
  HIPCHK(down(matches12, dM, n1, st));
  HIPCHK(down(res, dR, 1, st));
  HIPCHK(hipStreamSynchronize(st));
  return ORBX_OK;
}

// ---- ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) and the composition of Scw (include/orbx.h, "loop closing:
// matching the loop's points under Scw"; orbx_match_scw_kernel.hip)
int orbx_match_scw_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_map_set,
                                const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                                int n_map_sets, int map_capacity, const int32_t* d_map_n, const float* d_map_points,
                                const float* d_map_normals, const float* d_map_dist, const uint8_t* d_map_desc32,
                                const uint8_t* d_map_mask, const float* d_scw, const float* K, const orbx_bounds* bounds, float th,
                                int th_low, int32_t* d_matches, const int32_t* d_kf2_to_map, orbx_scw_result* d_res) {
  if (n_frames < 0 || n_pairs < 0 || n_map_sets < 0 || capacity < 1 || map_capacity < 1 || (n_pairs > 0 && (!h_kf || !h_map_set)) ||
      !d_kps_un || !d_desc32 || !d_n || !d_map_n || !d_map_points || !d_map_normals || !d_map_dist || !d_map_desc32 || !d_scw || !K ||
      !bounds || !d_matches || !d_res)
    return ORBX_E_BADARG;
  int r = refused(ctx, "match scw", th, th_low < 0 || th_low > 256 ? "th_low outside [0, 256]" : nullptr, bounds,
                  pairsInRange(h_kf, h_map_set, n_pairs, n_frames, n_map_sets)
                      ? nullptr
                      : "keyframe outside [0, n_frames) or map set outside [0, n_map_sets)",
                  capacity > ORBX_BOW_MAX_FEATURES || map_capacity > ORBX_BOW_MAX_FEATURES
                      ? "capacity or map_capacity above ORBX_BOW_MAX_FEATURES"
                      : nullptr);
  if (r != ORBX_OK) return r;
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  r = holdLists(ctx, st, s->scwPairs, {h_kf, h_map_set}, n_pairs);
  if (r != ORBX_OK) return r;
  MatchScwArgs a{};
  a.kps = d_kps_un;
  a.desc = d_desc32;
  a.n = d_n;
  a.mapN = d_map_n;
  a.mapPoints = d_map_points;
  a.mapNormals = d_map_normals;
  a.mapDist = d_map_dist;
  a.mapDesc = d_map_desc32;
  a.mapMask = d_map_mask;
  a.scw = d_scw;
  a.kf2ToMap = d_kf2_to_map;
  a.pairs = s->scwPairs;
  a.cap = capacity;
  a.mapCap = map_capacity;
  a.nPairs = n_pairs;
  a.thLow = th_low;
  a.cam = camArgs(ctx, K, bounds, th);
  a.matches = d_matches;
  a.res = d_res;
  HIPCHK(launch_match_scw(st, a));
  return ORBX_OK;
}

int orbx_match_scw(orbx_ctx* ctx, const orbx_keypoint* kps_un, const uint8_t* desc32, int n, int map_n, const float* map_points,
                   const float* map_normals, const float* map_dist, const uint8_t* map_desc32, const uint8_t* map_mask,
                   const float* scw, const float* K, const orbx_bounds* bounds, float th, int th_low, int32_t* matches,
                   const int32_t* kf2_to_map, int n_table, orbx_scw_result* res) {
  if (n < 0 || map_n < 0 || n_table < 0 || !scw || !K || !bounds || !res || (n > 0 && (!kps_un || !desc32 || !matches)) ||
      (map_n > 0 && (!map_points || !map_normals || !map_dist || !map_desc32)))
    return ORBX_E_BADARG;
  if (!kf2_to_map) n_table = 0;
  const int cap = std::max(std::max(n, n_table), 1), mapCap = std::max(map_n, 1);
  if (cap > ORBX_BOW_MAX_FEATURES || mapCap > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "match scw: more than ORBX_BOW_MAX_FEATURES features, points or table entries");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  orbx_keypoint* dK;
  uint8_t *dD, *dMD, *dMask;
  float *dP, *dNrm, *dDist, *dScw;
  int32_t *dN, *dM, *dTab;
  orbx_scw_result* dR;
  auto staging = [&](Layout L) {  // one keyframe and one map set in the batch layout, then the results
    dK = L.take<orbx_keypoint>(cap);
    dD = L.take<uint8_t>((size_t)cap * 32);
    dMD = L.take<uint8_t>((size_t)mapCap * 32);
    dP = L.take<float>((size_t)mapCap * 3);
    dNrm = L.take<float>((size_t)mapCap * 3);
    dDist = L.take<float>((size_t)mapCap * 2);
    dMask = L.take<uint8_t>(mapCap);
    dScw = L.take<float>(12);
    dN = L.take<int32_t>(2);
    dM = L.take<int32_t>(cap);
    dTab = L.take<int32_t>(cap);
    dR = L.take<orbx_scw_result>(1);
    return L.size();
  };
  const size_t bytes = staging(Layout());
  HIPCHK(s->dScwIo.grow(bytes, st));
  staging(Layout(s->dScwIo));
  HIPCHK(hipMemsetAsync(s->dScwIo, 0, bytes, st));
  // (the table's tail, beyond n_table, names no point of the set: such an entry is never followed)
  std::vector<int32_t> table(kf2_to_map ? cap : 0, INT32_MAX);
  if (kf2_to_map) std::copy(kf2_to_map, kf2_to_map + n_table, table.begin());
  HIPCHK(up(dK, kps_un, n, st));
  HIPCHK(up(dD, desc32, (size_t)n * 32, st));
  HIPCHK(up(dM, matches, n, st));
  HIPCHK(up(dMD, map_desc32, (size_t)map_n * 32, st));
  HIPCHK(up(dP, map_points, (size_t)map_n * 3, st));
  HIPCHK(up(dNrm, map_normals, (size_t)map_n * 3, st));
  HIPCHK(up(dDist, map_dist, (size_t)map_n * 2, st));
  if (map_mask) HIPCHK(up(dMask, map_mask, map_n, st));
  if (kf2_to_map) HIPCHK(up(dTab, table.data(), table.size(), st));
  HIPCHK(up(dScw, scw, 12, st));
  const int32_t hn[2] = {n, map_n};
  HIPCHK(up(dN, hn, 2, st));
  const int32_t frame = 0, set = 0;
  r = orbx_match_scw_batch_device(ctx, 1, 1, &frame, &set, dK, dD, dN, cap, 1, mapCap, dN + 1, dP, dNrm, dDist, dMD,
                                  map_mask ? dMask : nullptr, dScw, K, bounds, th, th_low, dM, kf2_to_map ? dTab : nullptr, dR);
  if (r != ORBX_OK) {
    (void)hipStreamSynchronize(st);  // (the uploads queued above read this frame's variables)
    return r;
  }
  HIPCHK(down(matches, dM, n, st));
  HIPCHK(down(res, dR, 1, st));
  HIPCHK(hipStreamSynchronize(st));
  return ORBX_OK;
}

int orbx_sim3_compose_scw_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf2, const float* d_pose,
                                       const float* d_sim3, float* d_scw) {
  if (n_frames < 0 || n_pairs < 0 || (n_pairs > 0 && !h_kf2) || !d_pose || !d_sim3 || !d_scw) return ORBX_E_BADARG;
  if (!pairsInRange(h_kf2, h_kf2, n_pairs, n_frames)) {
    if (ctx) ctxSetError(ctx, "sim3 compose scw: keyframe outside [0, n_frames)");
    return ORBX_E_BADARG;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  r = holdLists(ctx, st, s->composeKf2, {h_kf2}, n_pairs);
  if (r != ORBX_OK) return r;
  Sim3ComposeArgs a{};
  a.pose = d_pose;
  a.sim3 = d_sim3;
  a.kf2 = s->composeKf2;
  a.nPairs = n_pairs;
  a.scw = d_scw;
  HIPCHK(launch_sim3_compose_scw(st, a));
  return ORBX_OK;
}

int orbx_sim3_compose_scw(orbx_ctx* ctx, const float* pose2, const float* sim3, float* scw) {
  if (!pose2 || !sim3 || !scw) return ORBX_E_BADARG;
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MatchBowScratch* s = ctxMatchBow(ctx);
  hipStream_t st = ctxStream(ctx);
  float *dPose, *dSim, *dScw;
  auto staging = [&](Layout L) {
    dPose = L.take<float>(12);
    dSim = L.take<float>(13);
    dScw = L.take<float>(12);
    return L.size();
  };
  const size_t bytes = staging(Layout());
  HIPCHK(s->dComposeIo.grow(bytes, st));
  staging(Layout(s->dComposeIo));
  HIPCHK(up(dPose, pose2, 12, st));
  HIPCHK(up(dSim, sim3, 13, st));
  const int32_t kf2 = 0;
  r = orbx_sim3_compose_scw_batch_device(ctx, 1, 1, &kf2, dPose, dSim, dScw);
  if (r != ORBX_OK) {
    (void)hipStreamSynchronize(st);  // (the uploads queued above read this call's arguments)
    return r;
  }
  HIPCHK(down(scw, dScw, 12, st));
  HIPCHK(hipStreamSynchronize(st));
  return ORBX_OK;
}

}  // extern "C"
