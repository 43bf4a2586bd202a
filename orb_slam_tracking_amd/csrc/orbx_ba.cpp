// orbx_ba.cpp — host side of the two bundle adjustments: the two-view one (include/orbx.h, "behind the Initializer: two-view bundle
// adjustment"; kernel in orbx_ba_kernel.hip) and the local one (include/orbx.h, "local mapping: local bundle adjustment"; kernel in
// orbx_lba_kernel.hip), and of the step behind the local one (include/orbx.h, "local mapping: updating the map points"; kernels in
// orbx_map_kernel.hip): the argument checks, the pair / problem lists, the workspaces and the C entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "orbx_host.h"

// (the local bundle adjustment's workspace layout is the kernel's: one description, in the shared arithmetic file)
#define ORBX_BA_FN
#include "orbx_ba_math.inc"
#define ORBX_LBA_LAYOUT_ONLY
#include "orbx_lba_math.inc"


using namespace orbx;

namespace {

constexpr int BA_MAX_CAPACITY = 1 << 20;
// orbx_debug_local_ba_lds_max_free
std::atomic<int> g_lbaLdsMaxFree{orbx_lba::LBA_LDS_MAX_FREE};

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

// ---- the local bundle adjustment ----

int orbx_local_ba_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_first, const int32_t* h_count,
                               const int32_t* h_n_free, const int32_t* h_map_set, int n_entries, const int32_t* h_entry_frame,
                               const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const float* d_pose,
                               const int32_t* d_rows, int n_map_sets, int map_capacity, const int32_t* d_map_n,
                               const float* d_map_points, const uint8_t* d_map_mask, const float* K, const float* inv_sigma2,
                               int n_iterations, int n_more_iterations, float* d_pose_out, float* d_map_points_out,
                               uint8_t* d_obs_outlier, orbx_lba_result* d_res) {
  if (n_frames < 0 || n_problems < 0 || n_entries < 0 || n_map_sets < 0 || capacity < 1 || map_capacity < 1 || n_iterations < 0 ||
      n_more_iterations < 0 || (n_problems > 0 && (!h_first || !h_count || !h_n_free || !h_map_set)) ||
      (n_entries > 0 && !h_entry_frame) || !d_kps_un || !d_n || !d_pose || !d_rows || !d_map_n || !d_map_points || !K ||
      !d_pose_out || !d_map_points_out || !d_obs_outlier || !d_res)
    return ORBX_E_BADARG;
  for (int e = 0; e < n_entries; e++)
    if (h_entry_frame[e] < 0 || h_entry_frame[e] >= n_frames) {
      if (ctx) ctxSetError(ctx, "local BA: an entry names a frame outside [0, n_frames)");
      return ORBX_E_BADARG;
    }
  for (int p = 0; p < n_problems; p++) {
    const char* what = nullptr;
    if (h_first[p] < 0 || h_count[p] < 0 || h_first[p] > n_entries - h_count[p])
      what = "local BA: a problem's entries lie outside the entry list";
    else if (h_n_free[p] < 0 || h_n_free[p] > h_count[p])
      what = "local BA: n_free outside [0, count]";
    else if (h_n_free[p] > ORBX_LBA_MAX_FREE)
      what = "local BA: more than ORBX_LBA_MAX_FREE free keyframes in a problem";
    else if (h_map_set[p] < 0 || h_map_set[p] >= n_map_sets)
      what = "local BA: a map set outside [0, n_map_sets)";
    if (what) {
      if (ctx) ctxSetError(ctx, what);
      return ORBX_E_BADARG;
    }
  }
  if (capacity > ORBX_BOW_MAX_FEATURES || map_capacity > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "local BA: capacity or map_capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_problems == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  LbaScratch* s = ctxLba(ctx);
  hipStream_t st = ctxStream(ctx);
  int nLevels = 0;
  const float* table = ctxInvSigma2(ctx, &nLevels);

  // each problem's part of the workspace, in units of 256 bytes
  std::vector<int32_t> offset((size_t)n_problems);
  size_t units = 0, ldsBytes = 0;
  const int ldsMaxFree = g_lbaLdsMaxFree.load();
  for (int p = 0; p < n_problems; p++) {
    orbx_lba::Prob v{};
    v.cap = capacity;
    v.mapCap = map_capacity;
    v.nE = h_count[p];
    v.nF = h_n_free[p];
    if (units > 0x7fffffffu) {
      ctxSetError(ctx, "local BA: the batch's workspace exceeds 512 GiB");
      return ORBX_E_CAPACITY;
    }
    offset[(size_t)p] = (int32_t)units;
    units += orbx_lba::layout(&v, 0) / 256;
    if (v.nF <= ldsMaxFree) ldsBytes = std::max(ldsBytes, orbx_lba::factorBytes(v.nF));
  }
  HeldUploads hold(st);
  HIPCHK(hold(s->problems, {h_first, h_count, h_n_free, h_map_set, offset.data()}, n_problems));
  HIPCHK(hold(s->entries, {h_entry_frame}, n_entries));
  HIPCHK(hold(s->sigma, {inv_sigma2 ? inv_sigma2 : table}, nLevels));
  HIPCHK(s->dWork.grow(units * 256, st));  // (a workspace the device cannot take: ORBX_E_HIP, nothing queued)
  if (d_map_points_out != d_map_points)
    HIPCHK(hipMemcpyAsync(d_map_points_out, d_map_points, (size_t)n_map_sets * map_capacity * 3 * sizeof(float),
                          hipMemcpyDeviceToDevice, st));
  LbaArgs a{};
  a.kps = d_kps_un;
  a.nKps = d_n;
  a.pose = d_pose;
  a.rows = d_rows;
  a.problems = s->problems;
  a.entryFrame = s->entries;
  a.mapN = d_map_n;
  a.mapPts = d_map_points;
  a.mapMask = d_map_mask;
  a.invSigma2 = s->sigma;
  a.poseOut = d_pose_out;
  a.mapOut = d_map_points_out;
  a.outlier = d_obs_outlier;
  a.res = d_res;
  a.ws = s->dWork;
  intrinsics(K, &a.fx, &a.fy, &a.cx, &a.cy);
  a.delta = (double)(float)std::sqrt(5.991);  // `const float thHuberMono = sqrt(5.991)` of the ORB-SLAM design
  a.nProblems = n_problems;
  a.cap = capacity;
  a.mapCap = map_capacity;
  a.nLevels = nLevels;
  a.nIterations = n_iterations;
  a.nMoreIterations = n_more_iterations;
  a.ldsMaxFree = ldsMaxFree;
  a.ldsBytes = (uint32_t)((ldsBytes + 15) / 16 * 16);
  HIPCHK(launch_lba(st, a));
  return ORBX_OK;
}

int orbx_debug_local_ba_lds_max_free(int max_free) {
  if (max_free < -1 || max_free > orbx_lba::LBA_LDS_MAX_FREE) return ORBX_E_BADARG;
  g_lbaLdsMaxFree.store(max_free < 0 ? orbx_lba::LBA_LDS_MAX_FREE : max_free);
  return ORBX_OK;
}

int orbx_local_ba(orbx_ctx* ctx, int n_entries, int n_free, const orbx_keypoint* kps_un, const int32_t* n, int capacity,
                  const float* pose, const int32_t* rows, int map_n, const float* map_points, const uint8_t* map_mask,
                  const float* K, const float* inv_sigma2, int n_iterations, int n_more_iterations, float* pose_out,
                  float* map_points_out, uint8_t* obs_outlier, orbx_lba_result* res) {
  if (n_entries < 0 || n_free < 0 || n_free > n_entries || capacity < 1 || map_n < 0 || n_iterations < 0 || n_more_iterations < 0 ||
      !K || !res || (n_entries > 0 && (!kps_un || !n || !pose || !rows || !pose_out || !obs_outlier)) ||
      (map_n > 0 && (!map_points || !map_points_out)))
    return ORBX_E_BADARG;
  if (n_free > ORBX_LBA_MAX_FREE) {
    if (ctx) ctxSetError(ctx, "local BA: more than ORBX_LBA_MAX_FREE free keyframes");
    return ORBX_E_BADARG;
  }
  if (capacity > ORBX_BOW_MAX_FEATURES || map_n > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "local BA: more than ORBX_BOW_MAX_FEATURES features or points");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const size_t ne = (size_t)n_entries, c = (size_t)capacity, mc = (size_t)std::max(map_n, 1), nec = std::max(ne, (size_t)1);
  const int32_t mapN = map_n;
  std::vector<int32_t> frames(nec);
  for (size_t e = 0; e < ne; e++) frames[e] = (int32_t)e;
  Staged io(ctxIo(ctx), ctxStream(ctx));  // entry e is frame e; one map set
  auto dK = io.in(kps_un, ne * c, nec * c);
  auto dN = io.in(n, ne, nec);
  auto dP = io.in(pose, ne * 12, nec * 12);
  auto dRows = io.in(rows, ne * c, nec * c);
  auto dMapN = io.in(&mapN, 1, 1);
  auto dPts = io.in(map_points, (size_t)map_n * 3, mc * 3);  // (adjusted in place)
  io.out(dPts, 0, map_points_out, (size_t)map_n * 3);
  auto dMask = io.optIn(map_mask, (size_t)map_n, mc);
  auto dPo = io.out(pose_out, ne * 12, nec * 12);
  auto dOut = io.out(obs_outlier, ne * c, nec * c);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  const int32_t first = 0, count = n_entries, nFree = n_free, set = 0;
  r = orbx_local_ba_batch_device(ctx, std::max(n_entries, 1), 1, &first, &count, &nFree, &set, n_entries, frames.data(), io[dK], io[dN],
                                 capacity, io[dP], io[dRows], 1, (int)mc, io[dMapN], io[dPts], io[dMask], K, inv_sigma2,
                                 n_iterations, n_more_iterations, io[dPo], io[dPts], io[dOut], io[dR]);
  return io.close(ctx, r);
}

// ---- behind the local bundle adjustment: the map points updated ----

int orbx_map_update_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_first, const int32_t* h_count,
                                 const int32_t* h_n_free, const int32_t* h_map_set, int n_entries, const int32_t* h_entry_frame,
                                 const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                                 const float* d_entry_pose, int32_t* d_rows, const uint8_t* d_obs_outlier, int n_map_sets,
                                 int map_capacity, const int32_t* d_map_n, const float* d_map_points, const uint8_t* d_map_mask,
                                 uint8_t* d_map_mask_out, int32_t* d_map_ref, int what, float* d_map_normals, float* d_map_dist,
                                 uint8_t* d_map_desc32, int32_t* d_map_obs, orbx_map_result* d_res) {
  if (n_frames < 0 || n_problems < 0 || n_entries < 0 || n_map_sets < 0 || capacity < 1 || map_capacity < 1 || what < 0 || what > 3 ||
      (n_problems > 0 && (!h_first || !h_count || !h_n_free || !h_map_set)) || (n_entries > 0 && !h_entry_frame) || !d_kps_un ||
      !d_n || !d_entry_pose || !d_rows || !d_map_n || !d_map_points || !d_map_mask_out || !d_map_obs || !d_res ||
      ((what & ORBX_MAP_NORMALS) && (!d_map_normals || !d_map_dist)) || ((what & ORBX_MAP_DESCRIPTORS) && (!d_desc32 || !d_map_desc32)))
    return ORBX_E_BADARG;
  for (int e = 0; e < n_entries; e++)
    if (h_entry_frame[e] < 0 || h_entry_frame[e] >= n_frames) {
      if (ctx) ctxSetError(ctx, "map update: an entry names a frame outside [0, n_frames)");
      return ORBX_E_BADARG;
    }
  for (int p = 0; p < n_problems; p++) {
    const char* why = nullptr;
    if (h_first[p] < 0 || h_count[p] < 0 || h_first[p] > n_entries - h_count[p])
      why = "map update: a problem's entries lie outside the entry list";
    else if (h_n_free[p] < 0 || h_n_free[p] > h_count[p])
      why = "map update: n_free outside [0, count]";
    else if (h_map_set[p] < 0 || h_map_set[p] >= n_map_sets)
      why = "map update: a map set outside [0, n_map_sets)";
    if (why) {
      if (ctx) ctxSetError(ctx, why);
      return ORBX_E_BADARG;
    }
  }
  if (capacity > ORBX_BOW_MAX_FEATURES || map_capacity > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "map update: capacity or map_capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (n_problems == 0) return ORBX_OK;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  MapScratch* s = ctxMap(ctx);
  hipStream_t st = ctxStream(ctx);
  int nLevels = 0;
  const float* scale = ctxScale(ctx, &nLevels);

  // each problem's part of the workspace, in units of 256 bytes
  std::vector<int32_t> offset((size_t)n_problems);
  size_t units = 0;
  for (int p = 0; p < n_problems; p++) {
    if (units > 0x7fffffffu) {
      ctxSetError(ctx, "map update: the batch's workspace exceeds 512 GiB");
      return ORBX_E_CAPACITY;
    }
    offset[(size_t)p] = (int32_t)units;
    MapWork w;
    units += mapWorkLayout(map_capacity, h_count[p], 0, &w) / 256;
  }
  HeldUploads hold(st);
  HIPCHK(hold(s->problems, {h_first, h_count, h_n_free, h_map_set, offset.data()}, n_problems));
  HIPCHK(hold(s->entries, {h_entry_frame}, n_entries));
  HIPCHK(hold(s->scale, {scale}, nLevels));
  HIPCHK(s->dWork.grow(units * 256, st));  // (a workspace the device cannot take: ORBX_E_HIP, nothing queued)
  MapArgs a{};
  a.kps = d_kps_un;
  a.desc = d_desc32;
  a.nKps = d_n;
  a.entryPose = d_entry_pose;
  a.rows = d_rows;
  a.outlier = d_obs_outlier;
  a.problems = s->problems;
  a.entryFrame = s->entries;
  a.mapN = d_map_n;
  a.mapPts = d_map_points;
  a.mapMask = d_map_mask;
  a.mapMaskOut = d_map_mask_out;
  a.mapRef = d_map_ref;
  a.scale = s->scale;
  a.mapNormals = d_map_normals;
  a.mapDist = d_map_dist;
  a.mapDesc = d_map_desc32;
  a.mapObs = d_map_obs;
  a.res = d_res;
  a.ws = s->dWork;
  a.nProblems = n_problems;
  a.cap = capacity;
  a.mapCap = map_capacity;
  a.nLevels = nLevels;
  a.what = what;
  HIPCHK(launch_map_update(st, a));
  return ORBX_OK;
}

int orbx_map_update(orbx_ctx* ctx, int n_entries, int n_free, const orbx_keypoint* kps_un, const uint8_t* desc32, const int32_t* n,
                    int capacity, const float* pose, int32_t* rows, const uint8_t* obs_outlier, int map_n, const float* map_points,
                    const uint8_t* map_mask, uint8_t* map_mask_out, int32_t* map_ref, int what, float* map_normals, float* map_dist,
                    uint8_t* map_desc32, int32_t* map_obs, orbx_map_result* res) {
  if (n_entries < 0 || n_free < 0 || n_free > n_entries || capacity < 1 || map_n < 0 || what < 0 || what > 3 || !res ||
      (n_entries > 0 && (!kps_un || !n || !pose || !rows || ((what & ORBX_MAP_DESCRIPTORS) && !desc32))) ||
      (map_n > 0 && (!map_points || !map_mask_out || !map_obs || ((what & ORBX_MAP_NORMALS) && (!map_normals || !map_dist)) ||
                     ((what & ORBX_MAP_DESCRIPTORS) && !map_desc32))))
    return ORBX_E_BADARG;
  if (capacity > ORBX_BOW_MAX_FEATURES || map_n > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "map update: more than ORBX_BOW_MAX_FEATURES features or points");
    return ORBX_E_CAPACITY;
  }
  if (!ctx) return ORBX_E_HIP;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const size_t ne = (size_t)n_entries, c = (size_t)capacity, mn = (size_t)map_n, mc = (size_t)std::max(map_n, 1),
               nec = std::max(ne, (size_t)1);
  const int32_t mapN = map_n;
  std::vector<int32_t> frames(nec);
  for (size_t e = 0; e < ne; e++) frames[e] = (int32_t)e;
  Staged io(ctxIo(ctx), ctxStream(ctx));  // entry e is frame e; one map set; what the call leaves alone goes back as it came
  auto dK = io.in(kps_un, ne * c, nec * c);
  auto dD = io.in(desc32, ne * c * 32, nec * c * 32);
  auto dN = io.in(n, ne, nec);
  auto dP = io.in(pose, ne * 12, nec * 12);
  auto dRows = io.inout(rows, ne * c, nec * c);
  auto dOut = io.optIn(obs_outlier, ne * c, nec * c);
  auto dMapN = io.in(&mapN, 1, 1);
  auto dPts = io.in(map_points, mn * 3, mc * 3);
  const bool inPlace = map_mask && map_mask == map_mask_out;
  auto dMaskOut = io.inout(map_mask_out, mn, mc);
  auto dMask = inPlace ? dMaskOut : io.optIn(map_mask, mn, mc);
  auto dRef = io.inout(map_ref, mn, mc);
  dRef.absent = !map_ref;
  auto dNrm = io.inout(map_normals, mn * 3, mc * 3);
  auto dDist = io.inout(map_dist, mn * 2, mc * 2);
  auto dDesc = io.inout(map_desc32, mn * 32, mc * 32);
  auto dObs = io.inout(map_obs, mn, mc);
  auto dR = io.out(res, 1, 1);
  HIPCHK(io.open(Staged::Zeroed));
  const int32_t first = 0, count = n_entries, nFree = n_free, set = 0;
  r = orbx_map_update_batch_device(ctx, std::max(n_entries, 1), 1, &first, &count, &nFree, &set, n_entries, frames.data(), io[dK], io[dD],
                                   io[dN], capacity, io[dP], io[dRows], io[dOut], 1, (int)mc, io[dMapN], io[dPts], io[dMask],
                                   io[dMaskOut], io[dRef], what, io[dNrm], io[dDist], io[dDesc], io[dObs], io[dR]);
  return io.close(ctx, r);
}

}  // extern "C"
