// orbx_match_bow.cpp — host side of ORBmatcher::SearchByBoW (include/orbx.h, "matching through the FeatureVector"): the argument
// checks, the pair list and the C entry points.  The kernel is in orbx_match_bow_kernel.hip.  (The matchers by projection are in
// orbx_match_proj.cpp.)
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

}  // extern "C"
