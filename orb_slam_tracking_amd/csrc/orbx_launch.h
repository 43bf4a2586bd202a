// orbx_launch.h — the kernel launchers of liborbx, each declared once.  Included by the .hip file that defines a launcher (so the
// compiler checks the definition against it) and, through orbx_host.h, by every host .cpp that calls one.
#pragma once
#include <hip/hip_runtime.h>

#include "orbx_device.h"

namespace orbx {

// orbx_kernels.hip
hipError_t launch_to_gray(hipStream_t st, int nFrames, const uint8_t* src, long long srcFrameStride, int sstride, int w, int h,
                          int channels, int rgb, uint8_t* dst, long long dstFrameStride, int dstride, int grayVariant);
hipError_t launch_copy_out(hipStream_t st, const CopyOut& c, int nseg, int maxRows);
hipError_t launch_debug_sincos(hipStream_t st, const float* angle, int n, float* c, float* s, int libmFloat);
hipError_t launch_check_model(hipStream_t st, int nModels, const ScoreArgs& a);
hipError_t launch_undistort(hipStream_t st, int nFrames, const orbx_keypoint* in, const int* nkp, int capacity, const CamD& c,
                            orbx_keypoint* out);
hipError_t launch_pyramid_tiles(hipStream_t st, int nFrames, const uint8_t* img0, long long img0FrameStride, uint8_t* pyr,
                                const Geom& g, const PyrTileRect* rects, const PyrTileTap* taps, int nTiles, int buf0Bytes,
                                int bufBytes);
hipError_t launch_resize(hipStream_t st, int nFrames, const uint8_t* src, long long srcFrameStride, int sw, int sh, int sstride,
                         uint8_t* dst, long long dstFrameStride, int dw, int dh, int dstride, const ResizeTab* xtab,
                         const ResizeTab* ytab, int dwordPath, int wideFrames);
hipError_t launch_pyramid_bands(hipStream_t st, int nFrames, const uint8_t* img0, long long img0FrameStride, uint8_t* pyr,
                                const Geom& g, const ResizeTab* tab, const PyrBands& pb);
hipError_t launch_fast(hipStream_t st, int nFrames, const uint8_t* img0, long long img0FrameStride, int img0Aligned,
                       const uint8_t* pyr, const Geom& g, uint32_t* cand, int* cellCount, const FastCell* cells, int waveOk,
                       int* usedWave);
hipError_t launch_describe_patch(hipStream_t st, int nFrames, int maxSel, const uint8_t* img0, long long img0FrameStride,
                                 int img0Aligned, const uint8_t* pyr, const Geom& g, const SelKp* sel, const int* nsel,
                                 orbx_keypoint* kps, uint8_t* desc, int capacity, int gaussVariant, int libmFloat,
                                 const DescStage* staged);
hipError_t launch_match(hipStream_t st, int nPairs, const int* dFirst, const int* dSecond, const orbx_keypoint* kps,
                        const uint8_t* desc, const int* nkp, int capacity, orbx_bounds b, int window, float nnratio, int checkOri,
                        int* matches12, int* nmatches, int* stats, int* scratch, int pair0, int wideMode, int* hostWide,
                        unsigned int* diag);

// orbx_octree_kernel.hip
size_t octScratchBytes(int nMax, int qMax);
hipError_t launch_octree(hipStream_t st, int nFrames, const uint32_t* cand, const int* cellCount, const OctLaunch& P,
                         SelKp* selStage, int* nselLevel, uint8_t* scratch, int* maxN, const int* hintL, int force,
                         int* usedInstance);
hipError_t launch_sel_compact(hipStream_t st, int nFrames, const SelKp* selStage, const int* nselLevel, const OctLaunch& P,
                              SelKp* sel, int* nsel, int* nselUser, int* hostNsel, int selCap, int* hostErr, int* maxN,
                              int* hostMaxN);
hipError_t launch_debug_sort(hipStream_t st, int* triples, int n, unsigned long long* a, unsigned long long* b);

// orbx_checkrt_kernel.hip, orbx_init_kernel.hip
hipError_t launch_check_rt(hipStream_t st, int nModels, const CheckRtArgs& a);
hipError_t launch_init_prep(hipStream_t st, const InitArgs& a);
hipError_t launch_init_solve(hipStream_t st, const InitArgs& a);
hipError_t launch_init_finish(hipStream_t st, const InitArgs& a);
hipError_t launch_init_select(hipStream_t st, const InitArgs& a);

// orbx_bow_kernel.hip
hipError_t launch_bow_descend(hipStream_t st, const BowArgs& a);
hipError_t launch_bow_transform(hipStream_t st, const BowArgs& a);
hipError_t launch_bow_score_l1(hipStream_t st, const BowScoreArgs& s);

// orbx_voc_train_kernel.hip
hipError_t vtLaunchPermInit(hipStream_t st, const int32_t* n, const int32_t* docOff, int cap, int nDocs, uint32_t* perm);
hipError_t vtLaunchSeedSmall(hipStream_t st, const VtArgs& a);
hipError_t vtLaunchSeedFirst(hipStream_t st, const VtArgs& a);
hipError_t vtLaunchSeedUpdate(hipStream_t st, const VtArgs& a, int c);
hipError_t vtLaunchSeedPick(hipStream_t st, const VtArgs& a, int c);
hipError_t vtLaunchAssign(hipStream_t st, const VtArgs& a);
hipError_t vtLaunchRound(hipStream_t st, const VtArgs& a);
hipError_t vtLaunchCount(hipStream_t st, const VtArgs& a);
hipError_t vtLaunchCentreFinal(hipStream_t st, const VtArgs& a);
hipError_t vtLaunchHist(hipStream_t st, const VtArgs& a);
hipError_t vtLaunchScan(hipStream_t st, const VtArgs& a);
hipError_t vtLaunchScatter(hipStream_t st, const VtArgs& a);
hipError_t vtLaunchDocFreq(hipStream_t st, const BowNode* nodes, const uint32_t* fin, const int32_t* n, int cap, int nDocs,
                           uint32_t* featWord, uint32_t* Ni);

// orbx_db_kernel.hip
hipError_t launch_db_add_count(hipStream_t st, const DbAddArgs& a, uint32_t* tileSum);
hipError_t launch_db_add_fill(hipStream_t st, const DbAddArgs& a, uint32_t nNew);
hipError_t launch_db_accumulate(hipStream_t st, const DbQueryArgs& a);
hipError_t launch_db_merge(hipStream_t st, const DbMergeArgs& a);

// orbx_match_bow_kernel.hip, orbx_match_proj_kernel.hip, orbx_match_local_kernel.hip, orbx_match_kfproj_kernel.hip, orbx_ba_kernel.hip,
// orbx_pose_kernel.hip
hipError_t launch_match_bow(hipStream_t st, const MatchBowArgs& a);
hipError_t launch_match_proj(hipStream_t st, const MatchProjArgs& a);
hipError_t launch_match_local(hipStream_t st, const MatchLocalArgs& a);
hipError_t launch_match_kfproj(hipStream_t st, const MatchKfProjArgs& a);
hipError_t launch_ba(hipStream_t st, const BaArgs& a);
hipError_t launch_pose(hipStream_t st, const PoseArgs& a);

// orbx_match_tri_kernel.hip
hipError_t launch_match_tri(hipStream_t st, const MatchTriArgs& a);
hipError_t launch_triangulate(hipStream_t st, const TriangulateArgs& a);  // (zeroes a.res first)

// orbx_pnp_kernel.hip
hipError_t launch_pnp_prep(hipStream_t st, const PnpArgs& a);
hipError_t launch_pnp_hypotheses(hipStream_t st, const PnpArgs& a);
hipError_t launch_pnp_refine(hipStream_t st, const PnpArgs& a);

// orbx_sim3_kernel.hip
hipError_t launch_sim3_prep(hipStream_t st, const Sim3Args& a);
hipError_t launch_sim3_hypotheses(hipStream_t st, const Sim3Args& a);
hipError_t launch_sim3_resolve(hipStream_t st, const Sim3Args& a);

// orbx_match_sim3_kernel.hip
hipError_t launch_match_sim3(hipStream_t st, const MatchSim3Args& a);

// orbx_match_scw_kernel.hip
hipError_t launch_match_scw(hipStream_t st, const MatchScwArgs& a);
hipError_t launch_sim3_compose_scw(hipStream_t st, const Sim3ComposeArgs& a);
// orbx_match_fuse_kernel.hip (scwForm: a.pose holds similarities and there is no chi-square gate)
hipError_t launch_match_fuse(hipStream_t st, const MatchFuseArgs& a, bool scwForm);

// orbx_sim3opt_kernel.hip
hipError_t launch_sim3_optimize(hipStream_t st, const Sim3OptArgs& a);

// orbx_lba_kernel.hip
hipError_t launch_lba(hipStream_t st, const LbaArgs& a);

// orbx_map_kernel.hip: k_map_build, then (what != 0) k_map_points
hipError_t launch_map_update(hipStream_t st, const MapArgs& a);

// orbx_stereo_kernel.hip: a.ws zeroed, k_stereo_match, k_stereo_filter
hipError_t launch_stereo(hipStream_t st, const StereoArgs& a);

}  // namespace orbx
