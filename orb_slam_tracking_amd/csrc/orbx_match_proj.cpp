// orbx_match_proj.cpp — host side of the matchers by projection: ORBmatcher::SearchByProjection(CurrentFrame, LastFrame)
// (include/orbx.h, "matching by projection"), Tracking::SearchLocalPoints ("matching the local map by projection") and the
// relocalisation overload ("matching a keyframe's points by projection"): the argument checks, the index lists and the C entry
// points; behind them SearchBySim3, the loop-closing overload under Scw with its composition, and both overloads of Fuse.  The
// kernels are in orbx_match_proj_kernel.hip, orbx_match_local_kernel.hip, orbx_match_kfproj_kernel.hip,
// orbx_match_sim3_kernel.hip, orbx_match_scw_kernel.hip and orbx_match_fuse_kernel.hip.
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

// What every batch call here does once its arguments stand and there are pairs: the batches issued with the _async calls waited
// for, and the call's index lists, each of n_pairs entries, as one array [k][n_pairs] in `held` (HeldUploads) -> *st, the stream
// to launch on.
int listsHeld(orbx_ctx* ctx, HeldArray<int32_t>& held, HeldArray<int32_t>::Columns columns, int nPairs, hipStream_t* st) {
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  *st = ctxStream(ctx);
  HIPCHK(HeldUploads(*st)(held, columns, nPairs));
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
  HeldArray<int32_t>& pairs = ctxMatchBow(ctx)->projPairs;
  hipStream_t st;
  r = listsHeld(ctx, pairs, {h_last, h_cur, h_point_set}, n_pairs, &st);
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
  a.pairs = pairs;
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
  const size_t c = (size_t)cap;
  const int32_t hn[2] = {last_n, cur_n};
  Staged io(ctxIo(ctx), ctxStream(ctx));  // the two frames (last 0, current 1) and one point set in the batch layout, then the results
  auto dK = io.in(last_kps_un, last_n, 2 * c);
  io.in(dK, c, cur_kps_un, cur_n);
  auto dD = io.in(last_desc32, (size_t)last_n * 32, 2 * c * 32);
  io.in(dD, c * 32, cur_desc32, (size_t)cur_n * 32);
  auto dP = io.in(points, (size_t)last_n * 3, c * 3);
  auto dPD = io.optIn(point_desc32, (size_t)last_n * 32, c * 32);
  auto dMask = io.optIn(mask, last_n, c);
  auto dOut = io.optIn(last_outlier, last_n, c);
  auto dPose = io.in(pose_cur, 12, 12);
  auto dN = io.in(hn, 2, 2);
  auto dM = io.out(matches_cur, cur_n, c);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  const int32_t last = 0, cur = 1, set = 0;
  r = orbx_match_projection_batch_device(ctx, 2, 1, &last, &cur, &set, io[dK], io[dD], io[dN], cap, 1, io[dP], io[dMask], io[dPD],
                                         io[dOut], io[dPose], K, bounds, th, check_orientation, io[dM], io[dR]);
  return io.close(ctx, r);
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
  HeldArray<int32_t>& pairs = ctxMatchBow(ctx)->localPairs;
  hipStream_t st;
  r = listsHeld(ctx, pairs, {h_frame, h_map_set}, n_pairs, &st);
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
  a.pairs = pairs;
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
  const size_t c = (size_t)cap, mc = (size_t)mapCap;
  const int32_t hn[2] = {n, map_n};
  Staged io(ctxIo(ctx), ctxStream(ctx));  // one frame and one map set in the batch layout, then the results
  auto dK = io.in(kps_un, n, c);
  auto dD = io.in(desc32, (size_t)n * 32, c * 32);
  auto dMD = io.in(map_desc32, (size_t)map_n * 32, mc * 32);
  auto dP = io.in(map_points, (size_t)map_n * 3, mc * 3);
  auto dNrm = io.in(map_normals, (size_t)map_n * 3, mc * 3);
  auto dDist = io.in(map_dist, (size_t)map_n * 2, mc * 2);
  auto dMask = io.optIn(map_mask, map_n, mc);
  auto dOut = io.optIn(outlier, n, c);
  auto dView = io.optOut(point_view, map_n, mc);
  auto dPose = io.in(pose, 12, 12);
  auto dN = io.in(hn, 2, 2);
  auto dM = io.inout(matches, n, c);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  const int32_t frame = 0, set = 0;
  r = orbx_match_local_map_batch_device(ctx, 1, 1, &frame, &set, io[dK], io[dD], io[dN], cap, 1, mapCap, io[dN] + 1, io[dP], io[dNrm],
                                        io[dDist], io[dMD], io[dMask], io[dPose], K, bounds, th, nnratio, io[dM], io[dOut], io[dView],
                                        io[dR]);
  return io.close(ctx, r);
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
  HeldArray<int32_t>& pairs = ctxMatchBow(ctx)->kfProjPairs;
  hipStream_t st;
  r = listsHeld(ctx, pairs, {h_kf, h_cur, h_point_set}, n_pairs, &st);
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
  a.pairs = pairs;
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
  const size_t c = (size_t)cap;
  const int32_t hn[2] = {kf_n, cur_n};
  Staged io(ctxIo(ctx), ctxStream(ctx));  // the two frames (keyframe 0, current 1) and one point set in the batch layout, then the results
  auto dK = io.in(kf_kps_un, kf_n, 2 * c);
  io.in(dK, c, cur_kps_un, cur_n);
  auto dD = io.in(kf_desc32, (size_t)kf_n * 32, 2 * c * 32);
  io.in(dD, c * 32, cur_desc32, (size_t)cur_n * 32);
  auto dP = io.in(points, (size_t)kf_n * 3, c * 3);
  auto dDist = io.in(point_dist, (size_t)kf_n * 2, c * 2);
  auto dPD = io.optIn(point_desc32, (size_t)kf_n * 32, c * 32);
  auto dMask = io.optIn(mask, kf_n, c);
  auto dOut = io.optIn(outlier, cur_n, c);
  auto dPose = io.in(pose, 12, 12);
  auto dN = io.in(hn, 2, 2);
  auto dM = io.inout(matches, cur_n, c);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  const int32_t kf = 0, cur = 1, set = 0;
  r = orbx_match_keyframe_projection_batch_device(ctx, 2, 1, &kf, &cur, &set, io[dK], io[dD], io[dN], cap, 1, io[dP], io[dMask], io[dPD],
                                                  io[dDist], io[dPose], K, bounds, th, orb_dist, check_orientation, io[dM], io[dOut],
                                                  io[dR]);
  return io.close(ctx, r);
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
  HeldArray<int32_t>& pairs = ctxMatchBow(ctx)->sim3Pairs;
  hipStream_t st;
  r = listsHeld(ctx, pairs, {h_kf1, h_kf2, h_set1, h_set2}, n_pairs, &st);
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
  a.pairs = pairs;
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
  const size_t c = (size_t)cap;
  const int32_t hn[2] = {n1, n2}, zero = 0, one = 1;
  Staged io(ctxIo(ctx), ctxStream(ctx));  // the two keyframes and their point sets in the batch layout, then the results
  auto dK = io.in(kps_un1, n1, 2 * c);
  io.in(dK, c, kps_un2, n2);
  auto dD = io.in(desc1, (size_t)n1 * 32, 2 * c * 32);
  io.in(dD, c * 32, desc2, (size_t)n2 * 32);
  auto dP = io.in(points1, (size_t)n1 * 3, 2 * c * 3);
  io.in(dP, c * 3, points2, (size_t)n2 * 3);
  auto dDist = io.in(point_dist1, (size_t)n1 * 2, 2 * c * 2);
  io.in(dDist, c * 2, point_dist2, (size_t)n2 * 2);
  auto dPD = io.optIn(point_desc1, (size_t)n1 * 32, 2 * c * 32);  // (both keyframes bring theirs, or neither does)
  io.in(dPD, c * 32, point_desc2, (size_t)n2 * 32);
  auto dMask = io.optIn(mask1, n1, 2 * c);
  io.in(dMask, c, mask2, n2);
  auto dPose = io.in(pose1, 12, 24);
  io.in(dPose, 12, pose2, 12);
  auto dSim = io.in(sim3, 13, 13);
  auto dN = io.in(hn, 2, 2);
  auto dM = io.inout(matches12, n1, c);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  r = orbx_match_sim3_batch_device(ctx, 2, 1, &zero, &one, &zero, &one, io[dK], io[dD], io[dN], cap, 2, io[dP], io[dMask], io[dPD],
                                   io[dDist], io[dPose], io[dSim], K, bounds, th, orb_dist, io[dM], io[dR]);
  return io.close(ctx, r);
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
  HeldArray<int32_t>& pairs = ctxMatchBow(ctx)->scwPairs;
  hipStream_t st;
  r = listsHeld(ctx, pairs, {h_kf, h_map_set}, n_pairs, &st);
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
  a.pairs = pairs;
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
  // (the table's tail, beyond n_table, names no point of the set: such an entry is never followed)
  std::vector<int32_t> table(kf2_to_map ? cap : 0, INT32_MAX);
  if (kf2_to_map) std::copy(kf2_to_map, kf2_to_map + n_table, table.begin());
  const size_t c = (size_t)cap, mc = (size_t)mapCap;
  const int32_t hn[2] = {n, map_n};
  Staged io(ctxIo(ctx), ctxStream(ctx));  // one keyframe and one map set in the batch layout, then the results
  auto dK = io.in(kps_un, n, c);
  auto dD = io.in(desc32, (size_t)n * 32, c * 32);
  auto dMD = io.in(map_desc32, (size_t)map_n * 32, mc * 32);
  auto dP = io.in(map_points, (size_t)map_n * 3, mc * 3);
  auto dNrm = io.in(map_normals, (size_t)map_n * 3, mc * 3);
  auto dDist = io.in(map_dist, (size_t)map_n * 2, mc * 2);
  auto dMask = io.optIn(map_mask, map_n, mc);
  auto dScw = io.in(scw, 12, 12);
  auto dN = io.in(hn, 2, 2);
  auto dM = io.inout(matches, n, c);
  auto dTab = io.optIn(kf2_to_map ? table.data() : nullptr, table.size(), c);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  const int32_t frame = 0, set = 0;
  r = orbx_match_scw_batch_device(ctx, 1, 1, &frame, &set, io[dK], io[dD], io[dN], cap, 1, mapCap, io[dN] + 1, io[dP], io[dNrm], io[dDist],
                                  io[dMD], io[dMask], io[dScw], K, bounds, th, th_low, io[dM], io[dTab], io[dR]);
  return io.close(ctx, r);
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
  HeldArray<int32_t>& kf2 = ctxMatchBow(ctx)->composeKf2;
  hipStream_t st;
  const int r = listsHeld(ctx, kf2, {h_kf2}, n_pairs, &st);
  if (r != ORBX_OK) return r;
  Sim3ComposeArgs a{};
  a.pose = d_pose;
  a.sim3 = d_sim3;
  a.kf2 = kf2;
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
  Staged io(ctxIo(ctx), ctxStream(ctx));
  auto dPose = io.in(pose2, 12, 12);
  auto dSim = io.in(sim3, 13, 13);
  auto dScw = io.out(scw, 12, 12);
  HIPCHK(io.open());
  const int32_t kf2 = 0;
  r = orbx_sim3_compose_scw_batch_device(ctx, 1, 1, &kf2, io[dPose], io[dSim], io[dScw]);
  return io.close(ctx, r);
}

}  // extern "C"

// ---- ORBmatcher::Fuse, both overloads (include/orbx.h, "fusing map points into a keyframe"; orbx_match_fuse_kernel.hip)
namespace {

// Both batch calls: d_pose holds poses (d_map_obs required) or, with scwForm, similarities (d_map_obs null).
int fuseBatch(orbx_ctx* ctx, bool scwForm, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_map_set,
              const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity, int n_map_sets, int map_capacity,
              const int32_t* d_map_n, const float* d_map_points, const float* d_map_normals, const float* d_map_dist,
              const uint8_t* d_map_desc32, const uint8_t* d_map_mask, const int32_t* d_map_obs, const float* d_pose, const float* K,
              const orbx_bounds* bounds, float th, int th_low, int32_t* d_matches, const int32_t* d_occ_obs, int32_t* d_fuse_idx,
              uint8_t* d_fuse_act, int32_t* d_fuse_other, orbx_fuse_result* d_res) {
  if (n_frames < 0 || n_pairs < 0 || n_map_sets < 0 || capacity < 1 || map_capacity < 1 || (n_pairs > 0 && (!h_kf || !h_map_set)) ||
      !d_kps_un || !d_desc32 || !d_n || !d_map_n || !d_map_points || !d_map_normals || !d_map_dist || !d_map_desc32 ||
      (!scwForm && !d_map_obs) || !d_pose || !K || !bounds || !d_matches || !d_fuse_idx || !d_fuse_act || !d_fuse_other || !d_res)
    return ORBX_E_BADARG;
  const char* name = scwForm ? "fuse scw" : "fuse";
  int r = refused(ctx, name, th, th_low < 0 || th_low > 256 ? "th_low outside [0, 256]" : nullptr, bounds,
                  pairsInRange(h_kf, h_map_set, n_pairs, n_frames, n_map_sets)
                      ? nullptr
                      : "keyframe outside [0, n_frames) or map set outside [0, n_map_sets)",
                  capacity > ORBX_BOW_MAX_FEATURES || map_capacity > ORBX_BOW_MAX_FEATURES
                      ? "capacity or map_capacity above ORBX_BOW_MAX_FEATURES"
                      : nullptr);
  if (r != ORBX_OK) return r;
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_pairs == 0) return ORBX_OK;
  HeldArray<int32_t>& pairs = scwForm ? ctxMatchBow(ctx)->fuseScwPairs : ctxMatchBow(ctx)->fusePairs;
  hipStream_t st;
  r = listsHeld(ctx, pairs, {h_kf, h_map_set}, n_pairs, &st);
  if (r != ORBX_OK) return r;
  MatchFuseArgs a{};
  a.kps = d_kps_un;
  a.desc = d_desc32;
  a.n = d_n;
  a.mapN = d_map_n;
  a.mapPoints = d_map_points;
  a.mapNormals = d_map_normals;
  a.mapDist = d_map_dist;
  a.mapDesc = d_map_desc32;
  a.mapMask = d_map_mask;
  a.mapObs = d_map_obs;
  a.pose = d_pose;
  a.pairs = pairs;
  a.cap = capacity;
  a.mapCap = map_capacity;
  a.nPairs = n_pairs;
  a.thLow = th_low;
  a.cam = camArgs(ctx, K, bounds, th);
  int nLevels = 0;
  const float* inv = ctxInvSigma2(ctx, &nLevels);
  for (int l = 0; l < ORBX_MAX_LEVELS; l++) a.invSigma2[l] = l < nLevels ? inv[l] : 0.0f;
  a.matches = d_matches;
  a.occObs = d_occ_obs;
  a.fuseIdx = d_fuse_idx;
  a.fuseAct = d_fuse_act;
  a.fuseOther = d_fuse_other;
  a.res = d_res;
  HIPCHK(launch_match_fuse(st, a, scwForm));
  return ORBX_OK;
}

// Both host forms: one keyframe and one map set in the context's staging block, through fuseBatch as a batch of one.
int fuseOne(orbx_ctx* ctx, bool scwForm, const orbx_keypoint* kps_un, const uint8_t* desc32, int n, int map_n, const float* map_points,
            const float* map_normals, const float* map_dist, const uint8_t* map_desc32, const uint8_t* map_mask, const int32_t* map_obs,
            const float* pose, const float* K, const orbx_bounds* bounds, float th, int th_low, int32_t* matches, const int32_t* occ_obs,
            int32_t* fuse_idx, uint8_t* fuse_act, int32_t* fuse_other, orbx_fuse_result* res) {
  if (n < 0 || map_n < 0 || !pose || !K || !bounds || !res || (n > 0 && (!kps_un || !desc32 || !matches)) ||
      (map_n > 0 && (!map_points || !map_normals || !map_dist || !map_desc32 || (!scwForm && !map_obs) || !fuse_idx || !fuse_act ||
                     !fuse_other)))
    return ORBX_E_BADARG;
  const int cap = std::max(n, 1), mapCap = std::max(map_n, 1);
  if (cap > ORBX_BOW_MAX_FEATURES || mapCap > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "fuse: more than ORBX_BOW_MAX_FEATURES features or points");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const size_t c = (size_t)cap, mc = (size_t)mapCap;
  const int32_t hn[2] = {n, map_n};
  Staged io(ctxIo(ctx), ctxStream(ctx));  // one keyframe and one map set in the batch layout, then the results
  auto dK = io.in(kps_un, n, c);
  auto dD = io.in(desc32, (size_t)n * 32, c * 32);
  auto dMD = io.in(map_desc32, (size_t)map_n * 32, mc * 32);
  auto dP = io.in(map_points, (size_t)map_n * 3, mc * 3);
  auto dNrm = io.in(map_normals, (size_t)map_n * 3, mc * 3);
  auto dDist = io.in(map_dist, (size_t)map_n * 2, mc * 2);
  auto dObs = io.in(map_obs, (size_t)map_n, mc);  // (the Scw form brings none and reads none)
  auto dMask = io.optIn(map_mask, map_n, mc);
  auto dOcc = io.optIn(occ_obs, n, c);
  auto dPose = io.in(pose, 12, 12);
  auto dN = io.in(hn, 2, 2);
  auto dM = io.inout(matches, n, c);
  auto dIdx = io.out(fuse_idx, map_n, mc);
  auto dAct = io.out(fuse_act, map_n, mc);
  auto dOther = io.out(fuse_other, map_n, mc);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  const int32_t frame = 0, set = 0;
  r = fuseBatch(ctx, scwForm, 1, 1, &frame, &set, io[dK], io[dD], io[dN], cap, 1, mapCap, io[dN] + 1, io[dP], io[dNrm], io[dDist], io[dMD],
                io[dMask], scwForm ? nullptr : io[dObs], io[dPose], K, bounds, th, th_low, io[dM], io[dOcc], io[dIdx], io[dAct],
                io[dOther], io[dR]);
  return io.close(ctx, r);
}

}  // namespace

extern "C" {

int orbx_fuse_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_map_set,
                           const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity, int n_map_sets,
                           int map_capacity, const int32_t* d_map_n, const float* d_map_points, const float* d_map_normals,
                           const float* d_map_dist, const uint8_t* d_map_desc32, const uint8_t* d_map_mask, const int32_t* d_map_obs,
                           const float* d_pose, const float* K, const orbx_bounds* bounds, float th, int th_low, int32_t* d_matches,
                           const int32_t* d_occ_obs, int32_t* d_fuse_idx, uint8_t* d_fuse_act, int32_t* d_fuse_other,
                           orbx_fuse_result* d_res) {
  if (!d_map_obs) return ORBX_E_BADARG;
  return fuseBatch(ctx, false, n_frames, n_pairs, h_kf, h_map_set, d_kps_un, d_desc32, d_n, capacity, n_map_sets, map_capacity, d_map_n,
                   d_map_points, d_map_normals, d_map_dist, d_map_desc32, d_map_mask, d_map_obs, d_pose, K, bounds, th, th_low, d_matches,
                   d_occ_obs, d_fuse_idx, d_fuse_act, d_fuse_other, d_res);
}

int orbx_fuse_scw_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_map_set,
                               const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                               int n_map_sets, int map_capacity, const int32_t* d_map_n, const float* d_map_points,
                               const float* d_map_normals, const float* d_map_dist, const uint8_t* d_map_desc32,
                               const uint8_t* d_map_mask, const float* d_scw, const float* K, const orbx_bounds* bounds, float th,
                               int th_low, int32_t* d_matches, const int32_t* d_occ_obs, int32_t* d_fuse_idx, uint8_t* d_fuse_act,
                               int32_t* d_fuse_other, orbx_fuse_result* d_res) {
  return fuseBatch(ctx, true, n_frames, n_pairs, h_kf, h_map_set, d_kps_un, d_desc32, d_n, capacity, n_map_sets, map_capacity, d_map_n,
                   d_map_points, d_map_normals, d_map_dist, d_map_desc32, d_map_mask, nullptr, d_scw, K, bounds, th, th_low, d_matches,
                   d_occ_obs, d_fuse_idx, d_fuse_act, d_fuse_other, d_res);
}

int orbx_fuse(orbx_ctx* ctx, const orbx_keypoint* kps_un, const uint8_t* desc32, int n, int map_n, const float* map_points,
              const float* map_normals, const float* map_dist, const uint8_t* map_desc32, const uint8_t* map_mask,
              const int32_t* map_obs, const float* pose, const float* K, const orbx_bounds* bounds, float th, int th_low,
              int32_t* matches, const int32_t* occ_obs, int32_t* fuse_idx, uint8_t* fuse_act, int32_t* fuse_other,
              orbx_fuse_result* res) {
  return fuseOne(ctx, false, kps_un, desc32, n, map_n, map_points, map_normals, map_dist, map_desc32, map_mask, map_obs, pose, K, bounds,
                 th, th_low, matches, occ_obs, fuse_idx, fuse_act, fuse_other, res);
}

int orbx_fuse_scw(orbx_ctx* ctx, const orbx_keypoint* kps_un, const uint8_t* desc32, int n, int map_n, const float* map_points,
                  const float* map_normals, const float* map_dist, const uint8_t* map_desc32, const uint8_t* map_mask,
                  const float* scw, const float* K, const orbx_bounds* bounds, float th, int th_low, int32_t* matches,
                  const int32_t* occ_obs, int32_t* fuse_idx, uint8_t* fuse_act, int32_t* fuse_other, orbx_fuse_result* res) {
  return fuseOne(ctx, true, kps_un, desc32, n, map_n, map_points, map_normals, map_dist, map_desc32, map_mask, nullptr, scw, K, bounds,
                 th, th_low, matches, occ_obs, fuse_idx, fuse_act, fuse_other, res);
}

}  // extern "C"
