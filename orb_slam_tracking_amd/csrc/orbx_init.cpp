// orbx_init.cpp — host side of the two-view Initializer (include/orbx.h): the scoring loops and CheckRT on caller-supplied models,
// the RANSAC stage and the reconstruction for batches of frame pairs, their single-pair forms from host memory, and the C entry
// points.  The kernels are in orbx_kernels.hip (k_check_model), orbx_checkrt_kernel.hip and orbx_init_kernel.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "orbx_host.h"

using namespace orbx;

extern "C" {

// ---- Initializer scoring loops (Initialization/Initializer.cpp:268-438) ---------------------------
namespace {
// mvMatches12 (Initializer.cpp:24-33): the matched keypoints of frame 1 in order (first) and their partners (second); false
// for a partner outside frame 2
bool compactMatches(const int32_t* matches12, int n1, int n2, std::vector<int32_t>* first, std::vector<int32_t>* second) {
  for (int i = 0; i < n1; i++)
    if (matches12[i] >= 0) {
      if (matches12[i] >= n2) return false;
      first->push_back(i);
      second->push_back(matches12[i]);
    }
  return true;
}

int checkModels(orbx_ctx* ctx, int kind, int n_models, const float* M21, const float* M12, const orbx_keypoint* k1, int n1,
                const orbx_keypoint* k2, int n2, const int32_t* matches12, float sigma, float* scores, uint8_t* inliers,
                int* n_matches_out, int* best) {
  if (!ctx || n_models < 0 || n1 < 0 || n2 < 0 || !n_matches_out || (n_models > 0 && (!M21 || (kind == 0 && !M12) || !scores)) ||
      (n1 > 0 && (!k1 || !matches12)) || (n2 > 0 && !k2))
    return ORBX_E_BADARG;
  std::vector<int32_t> fs, sc;
  if (!compactMatches(matches12, n1, n2, &fs, &sc)) return ORBX_E_BADARG;
  const int N = (int)fs.size();
  *n_matches_out = N;
  if (best) *best = -1;
  if (n_models == 0) return ORBX_OK;
  if (N > 0 && !inliers) return ORBX_E_BADARG;
  if (hipSetDevice(ctxDevice(ctx)) != hipSuccess) return ORBX_E_HIP;
  // the batched form with one pair (frames {0, 0} of k1 / k2: the staged keypoint arrays) and the call's models as its
  // hypotheses; one staging block: models | keypoints | matches | pair table | scores | inliers
  const int32_t hTable[3] = {N, 0, 0};
  const size_t models = (size_t)n_models * 9;
  hipStream_t st = ctxStream(ctx);
  Staged io(ctxIo(ctx), st);
  auto dM21 = io.in(M21, models, models);
  auto dM12 = io.in(kind == 0 ? M12 : nullptr, models, models);
  auto dK1 = io.in(k1, n1, n1);
  auto dK2 = io.in(k2, n2, n2);
  auto dFirst = io.in(fs.data(), N, N);
  auto dSecond = io.in(sc.data(), N, N);
  auto dTable = io.in(hTable, 3, 3);  // pairN[1], frames[2]
  auto dScores = io.out(scores, n_models, n_models);
  auto dInliers = io.out(inliers, (size_t)n_models * N, (size_t)n_models * N);
  HIPCHK(io.open());
  ScoreArgs a{};
  a.M21 = io[dM21]; a.M12 = io[dM12]; a.k1 = io[dK1]; a.k2 = io[dK2]; a.first = io[dFirst]; a.second = io[dSecond];
  a.scores = io[dScores]; a.inliers = io[dInliers];
  a.pairN = io[dTable]; a.frames = io[dTable] + 1; a.perPair = n_models; a.stride = N; a.nPairs = 1; a.kind = kind;
  a.invSigmaSquare = (float)(1.0 / (double)(sigma * sigma));  // `const float invSigmaSquare = 1.0 / (sigma * sigma)`
  const int r = io.close(ctx, HIPRC(launch_check_model(st, n_models, a)));
  if (r != ORBX_OK) return r;
  if (best) {  // `if (currentScore > score)` with score starting at 0, Initializer.cpp:205-209 / 259-263
    float sc = 0;
    for (int m = 0; m < n_models; m++)
      if (scores[m] > sc) { sc = scores[m]; *best = m; }
  }
  return ORBX_OK;
}
}  // namespace

int orbx_check_homography(orbx_ctx* ctx, int n_models, const float* H21, const float* H12, const orbx_keypoint* k1, int n1,
                          const orbx_keypoint* k2, int n2, const int32_t* matches12, float sigma, float* scores, uint8_t* inliers,
                          int* n_matches_out, int* best) {
  return checkModels(ctx, 0, n_models, H21, H12, k1, n1, k2, n2, matches12, sigma, scores, inliers, n_matches_out, best);
}

int orbx_check_fundamental(orbx_ctx* ctx, int n_models, const float* F21, const orbx_keypoint* k1, int n1, const orbx_keypoint* k2,
                           int n2, const int32_t* matches12, float sigma, float* scores, uint8_t* inliers, int* n_matches_out,
                           int* best) {
  return checkModels(ctx, 1, n_models, F21, nullptr, k1, n1, k2, n2, matches12, sigma, scores, inliers, n_matches_out, best);
}

// ---- Initializer::CheckRT (Initialization/Initializer.cpp:569-713) -------------------------------------
int orbx_check_rt(orbx_ctx* ctx, int n_models, const float* R21, const float* t21, const float* K, const orbx_keypoint* k1, int n1,
                  const orbx_keypoint* k2, int n2, const int32_t* matches12, const uint8_t* matches_inliers, float th2, int32_t* n_good,
                  uint8_t* tri_good, float* p3d, float* parallax) {
  if (!ctx || n_models < 0 || n1 < 0 || n2 < 0 || !K || (n_models > 0 && (!R21 || !t21 || !n_good || !parallax)) ||
      (n1 > 0 && (!k1 || !matches12)) || (n2 > 0 && !k2) || (n_models > 0 && n1 > 0 && (!tri_good || !p3d)))
    return ORBX_E_BADARG;
  if (n_models == 0) return ORBX_OK;
  // mvMatches12, then the inliers in match order (:617-622); the i-th of them is booked under the i-th MATCH's first keypoint
  // (:643, :700: the reference indexes vMatches12 with the compacted index)
  std::vector<int32_t> fs, sc;
  if (!compactMatches(matches12, n1, n2, &fs, &sc)) return ORBX_E_BADARG;
  const int N = (int)fs.size();
  if (N > 0 && !matches_inliers) return ORBX_E_BADARG;
  std::vector<float> pts;
  std::vector<int32_t> book;
  for (int m = 0; m < N; m++)
    if (matches_inliers[m]) {
      const int i = (int)book.size();
      book.push_back(fs[i]);
      pts.push_back(k1[fs[m]].x); pts.push_back(k1[fs[m]].y); pts.push_back(k2[sc[m]].x); pts.push_back(k2[sc[m]].y);
    }
  const int nInl = (int)book.size();
  if (hipSetDevice(ctxDevice(ctx)) != hipSuccess) return ORBX_E_HIP;
  // the batched form with one pair whose n_models candidates are all solutions (stride n1 >= nInl)
  const int32_t hTable[2] = {nInl, n_models};
  const size_t M = (size_t)n_models, all = M * n1;
  hipStream_t st = ctxStream(ctx);
  Staged io(ctxIo(ctx), st);
  auto dR21 = io.in(R21, M * 9, M * 9);
  auto dT21 = io.in(t21, M * 3, M * 3);
  auto dPts = io.in(pts.data(), (size_t)nInl * 4, (size_t)nInl * 4);
  auto dBook = io.in(book.data(), nInl, nInl);
  auto dTable = io.in(hTable, 2, 2);  // pairNInl[1], pairNSol[1]
  auto dGood = io.out(tri_good, all, all);
  auto dP3d = io.out(p3d, all * 3, all * 3);
  auto dCos = io.room<float>(all);
  auto dNGood = io.out(n_good, M, M);
  auto dParallax = io.out(parallax, M, M);
  HIPCHK(io.open());
  CheckRtArgs a{};
  a.R21 = io[dR21]; a.t21 = io[dT21]; a.pts = io[dPts]; a.book = io[dBook]; a.good = io[dGood]; a.p3d = io[dP3d];
  a.cosBuf = io[dCos]; a.nGood = io[dNGood]; a.parallax = io[dParallax];
  for (int i = 0; i < 9; i++) a.K[i] = K[i];
  a.th2 = th2;
  a.pairNInl = io[dTable]; a.pairNSol = io[dTable] + 1; a.perPair = n_models; a.stride = n1;
  return io.close(ctx, HIPRC(launch_check_rt(st, n_models, a)));
}

// ---- the RANSAC stage of Initializer::Initialize (Initialization/Initializer.cpp:19-111) ----------------------------------
namespace {
struct ReconParams {
  const float* K;
  float minParallax;
  int minTriangulated;
  orbx_init_result* res;
  float* p3d;
  uint8_t* tri;
};
// findModels' work area over `L`: its arrays into a (the H and F scores and inlier flags into sH / sF, CheckRT's into c) in
// order; with `recon`, the reconstruction's part follows.  Returns the area's size.
size_t initWork(Layout L, int nPairs, int nIter, int cap, bool recon, InitArgs& a, ScoreArgs& sH, ScoreArgs& sF, CheckRtArgs& c) {
  const size_t P = nPairs, H = (size_t)nPairs * nIter, C = cap, M = 4 * P;
  a.N = L.take<int32_t>(P);
  a.scoreN = L.take<int32_t>(P);
  a.pstat = L.take<int32_t>(P);
  a.first = L.take<int32_t>(P * C);
  a.second = L.take<int32_t>(P * C);
  a.H21 = L.take<float>(H * 9);
  a.H12 = L.take<float>(H * 9);
  a.F21 = L.take<float>(H * 9);
  a.flags = L.take<uint8_t>(2 * H);
  sH.scores = L.take<float>(H);
  sF.scores = L.take<float>(H);
  sH.inliers = L.take<uint8_t>(H * C);
  sF.inliers = L.take<uint8_t>(H * C);
  a.res = L.take<orbx_hf_result>(P);
  a.inlOut = L.take<uint8_t>(P * 2 * C);
  if (recon) {
    a.R4 = L.take<float>(M * 9);
    a.t4 = L.take<float>(M * 3);
    a.nSol = L.take<int32_t>(P);
    a.nInl = L.take<int32_t>(P);
    a.pts = L.take<float>(P * C * 4);
    a.book = L.take<int32_t>(P * C);
    c.nGood = L.take<int32_t>(M);
    c.parallax = L.take<float>(M);
    c.good = L.take<uint8_t>(M * C);
    c.p3d = L.take<float>(M * C * 3);
    c.cosBuf = L.take<float>(M * C);
  }
  return L.size();
}
size_t initWorkSize(int nPairs, int nIter, int cap, bool recon) {
  InitArgs a{};
  ScoreArgs sH{}, sF{};
  CheckRtArgs c{};
  return initWork(Layout(), nPairs, nIter, cap, recon, a, sH, sF, c);
}
// prep -> solve -> score H -> score F -> select, all on the context stream; `work` holds the work area (initWork); d_models /
// d_scores (nullable) take the hypotheses and their scores in place of the work area's arrays
int findModels(orbx_ctx* ctx, uint8_t* work, int n_pairs, const int32_t* h_first, const int32_t* h_second, const orbx_keypoint* d_kps,
               const int32_t* d_n, int cap, const int32_t* d_m12, int n_iter, const int32_t* d_sets, float sigma, orbx_hf_result* d_res,
               uint8_t* d_inliers, float* d_models, float* d_scores, const ReconParams* rc) {
  hipStream_t st = ctxStream(ctx);
  const size_t H = (size_t)n_pairs * n_iter;
  HeldArray<int32_t>& pairs = ctxInit(ctx)->pairs;
  HIPCHK(HeldUploads(st)(pairs, {h_first, h_second}, n_pairs));
  InitArgs a{};
  ScoreArgs sH{}, sF{};
  CheckRtArgs c{};
  initWork(Layout(work), n_pairs, n_iter, cap, rc != nullptr, a, sH, sF, c);
  if (d_models) { a.H21 = d_models; a.H12 = d_models + H * 9; a.F21 = d_models + 2 * H * 9; }
  if (d_scores) { sH.scores = d_scores; sF.scores = d_scores + H; }
  if (d_res) a.res = d_res;
  if (d_inliers) a.inlOut = d_inliers;
  a.scoresH = sH.scores; a.scoresF = sF.scores; a.inlH = sH.inliers; a.inlF = sF.inliers;
  a.kps = d_kps; a.nKps = d_n; a.m12 = d_m12; a.sets = d_sets; a.frames = pairs;
  a.nPairs = n_pairs; a.nIter = n_iter; a.cap = cap;
  if (rc) {
    a.reconstruct = 1;
    for (int i = 0; i < 9; i++) a.K[i] = rc->K[i];
    a.minParallax = rc->minParallax; a.minTriangulated = rc->minTriangulated;
    a.nGood = c.nGood; a.parallax = c.parallax; a.good = c.good; a.p3d4 = c.p3d;
    a.ires = rc->res; a.p3dOut = rc->p3d; a.triOut = rc->tri;
    c.R21 = a.R4; c.t21 = a.t4; c.pts = a.pts; c.book = a.book;
    for (int i = 0; i < 9; i++) c.K[i] = rc->K[i];
    c.th2 = (float)(4.0 * (double)(sigma * sigma));  // `4.0 * mSigma2` (:499), mSigma2 = sigma * sigma (f32)
    c.pairNInl = a.nInl; c.pairNSol = a.nSol; c.perPair = 4; c.stride = cap;
  }
  HIPCHK(launch_init_prep(st, a));
  HIPCHK(launch_init_solve(st, a));
  for (ScoreArgs* s : {&sH, &sF}) {
    s->k1 = d_kps; s->k2 = d_kps; s->first = a.first; s->second = a.second;
    s->invSigmaSquare = (float)(1.0 / (double)(sigma * sigma));  // `const float invSigmaSquare = 1.0 / (sigma * sigma)`
    s->pairN = a.scoreN; s->frames = a.frames; s->perPair = n_iter; s->stride = cap; s->nPairs = n_pairs;
  }
  sH.kind = 0; sH.M21 = a.H21; sH.M12 = a.H12;
  sF.kind = 1; sF.M21 = a.F21; sF.M12 = nullptr;
  HIPCHK(launch_check_model(st, (int)H, sH));
  HIPCHK(launch_check_model(st, (int)H, sF));
  HIPCHK(launch_init_select(st, a));
  if (rc) {
    HIPCHK(launch_check_rt(st, 4 * n_pairs, c));
    HIPCHK(launch_init_finish(st, a));
  }
  return ORBX_OK;
}
int checkBatchArgs(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_first, const int32_t* h_second, const void* d_kps_un,
                   const void* d_n, int capacity, const void* d_matches12, int n_iter, const void* d_sets, float sigma, const void* d_res) {
  if (!ctx || n_frames <= 0 || n_pairs <= 0 || !h_first || !h_second || !d_kps_un || !d_n || !d_matches12 || !d_sets || !d_res ||
      n_iter <= 0 || capacity < 1 || capacity >= (1 << 20) || !(sigma > 0.f))
    return ORBX_E_BADARG;
  if ((long long)n_pairs * n_iter >= (1LL << 26)) return ORBX_E_BADARG;
  if (!pairsInRange(h_first, h_second, n_pairs, n_frames)) {
    ctxSetError(ctx, "pair index outside [0, n_frames)");
    return ORBX_E_BADARG;
  }
  return ORBX_OK;
}
}  // namespace

int orbx_find_models_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_first, const int32_t* h_second,
                                  const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const int32_t* d_matches12,
                                  int n_iter, const int32_t* d_sets, float sigma, orbx_hf_result* d_res, uint8_t* d_inliers,
                                  float* d_models, float* d_scores) {
  int r = checkBatchArgs(ctx, n_frames, n_pairs, h_first, h_second, d_kps_un, d_n, capacity, d_matches12, n_iter, d_sets, sigma, d_res);
  if (r != ORBX_OK) return r;
  r = ctxDrain(ctx);  // batches issued with the _async calls may still be writing the inputs
  if (r != ORBX_OK) return r;
  DeviceBuf<uint8_t>& dInit = ctxInit(ctx)->dInit;
  HIPCHK(dInit.grow(initWorkSize(n_pairs, n_iter, capacity, false), ctxStream(ctx)));  // (behind the work that may still use it)
  return findModels(ctx, dInit, n_pairs, h_first, h_second, d_kps_un, d_n, capacity, d_matches12, n_iter, d_sets, sigma, d_res,
                    d_inliers, d_models, d_scores, nullptr);
}

int orbx_initialize_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_first, const int32_t* h_second,
                                 const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const int32_t* d_matches12,
                                 int n_iter, const int32_t* d_sets, const float* K, float sigma, float min_parallax,
                                 int min_triangulated, orbx_init_result* d_res, float* d_p3d, uint8_t* d_triangulated) {
  int r = checkBatchArgs(ctx, n_frames, n_pairs, h_first, h_second, d_kps_un, d_n, capacity, d_matches12, n_iter, d_sets, sigma, d_res);
  if (r != ORBX_OK) return r;
  if (!K) return ORBX_E_BADARG;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  DeviceBuf<uint8_t>& dInit = ctxInit(ctx)->dInit;
  HIPCHK(dInit.grow(initWorkSize(n_pairs, n_iter, capacity, true), ctxStream(ctx)));
  const ReconParams rc{K, min_parallax, min_triangulated, d_res, d_p3d, d_triangulated};
  return findModels(ctx, dInit, n_pairs, h_first, h_second, d_kps_un, d_n, capacity, d_matches12, n_iter, d_sets, sigma, nullptr,
                    nullptr, nullptr, nullptr, &rc);
}

namespace {
// one pair from host memory = frames 0 and 1 of a two-frame batch through the batched path; inputs and outputs live behind the
// batched stage's work area; synchronous
int singlePair(orbx_ctx* ctx, const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, const int32_t* matches12, int n_iter,
               const int32_t* sets, float sigma, orbx_hf_result* hres, uint8_t* inliers, float* models, float* scores, const float* K,
               float min_parallax, int min_triangulated, orbx_init_result* ires, float* p3d, uint8_t* tri) {
  if (!ctx || n1 < 0 || n2 < 0 || (n1 > 0 && (!k1 || !matches12)) || (n2 > 0 && !k2) || n_iter <= 0 || !sets || !(sigma > 0.f) ||
      n1 >= (1 << 20) || n2 >= (1 << 20) || n_iter >= (1 << 26) || (!hres && !ires) || (ires && !K))
    return ORBX_E_BADARG;
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const int cap = std::max(std::max(n1, n2), 1);
  const size_t work = initWorkSize(1, n_iter, cap, ires != nullptr);
  const size_t c = (size_t)cap, it = (size_t)n_iter;
  const int32_t hn[2] = {n1, n2};
  DeviceBuf<uint8_t>& dInit = ctxInit(ctx)->dInit;
  // behind the work area; of the results, the caller asks for the H/F stage's (hres ...) or the reconstruction's (ires ...): the
  // others are null here and stay on the device
  Staged io(dInit, ctxStream(ctx), work);
  auto dK = io.in(k1, n1, 2 * c);
  io.in(dK, c, k2, n2);
  auto dN = io.in(hn, 2, 2);
  auto dM = io.in(matches12, n1, c);
  auto dS = io.in(sets, it * 8, it * 8);
  auto dR = io.out(hres, 1, 1);
  auto dIR = io.out(ires, 1, 1);
  auto dI = io.out(inliers, n1, 2 * c);  // [2][n1] from [2][cap]
  io.out(dI, c, inliers ? inliers + n1 : nullptr, n1);
  auto dMo = io.out(models, 3 * it * 9, 3 * it * 9);
  auto dSo = io.out(scores, 2 * it, 2 * it);
  auto dP = io.out(p3d, (size_t)n1 * 3, c * 3);
  auto dT = io.out(tri, n1, c);
  HIPCHK(io.open());
  const int32_t f0 = 0, f1 = 1;
  if (ires) {
    const ReconParams rc{K, min_parallax, min_triangulated, io[dIR], io[dP], io[dT]};
    r = findModels(ctx, dInit, 1, &f0, &f1, io[dK], io[dN], cap, io[dM], n_iter, io[dS], sigma, nullptr, nullptr, nullptr, nullptr, &rc);
  } else {
    r = findModels(ctx, dInit, 1, &f0, &f1, io[dK], io[dN], cap, io[dM], n_iter, io[dS], sigma, io[dR], io[dI], io[dMo], io[dSo], nullptr);
  }
  return io.close(ctx, r);
}
}  // namespace

int orbx_find_models(orbx_ctx* ctx, const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, const int32_t* matches12,
                     int n_iter, const int32_t* sets, float sigma, orbx_hf_result* res, uint8_t* inliers, float* models, float* scores) {
  if (!res) return ORBX_E_BADARG;
  return singlePair(ctx, k1, n1, k2, n2, matches12, n_iter, sets, sigma, res, inliers, models, scores, nullptr, 0.f, 0, nullptr,
                    nullptr, nullptr);
}

int orbx_initialize(orbx_ctx* ctx, const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, const int32_t* matches12,
                    int n_iter, const int32_t* sets, const float* K, float sigma, float min_parallax, int min_triangulated,
                    orbx_init_result* res, float* p3d, uint8_t* triangulated) {
  if (!res || !K) return ORBX_E_BADARG;
  return singlePair(ctx, k1, n1, k2, n2, matches12, n_iter, sets, sigma, nullptr, nullptr, nullptr, nullptr, K, min_parallax,
                    min_triangulated, res, p3d, triangulated);
}

}  // extern "C"
