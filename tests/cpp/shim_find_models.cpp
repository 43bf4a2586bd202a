// Compile check of the C ABI of the RANSAC stage of Initializer::Initialize (orbx_find_models*): prints the layout of
// orbx_hf_result for the Python mirror (orb_slam_tracking_amd.HFResult) and calls nothing.
#include <cstddef>
#include <cstdio>

#include "orbx.h"

int main() {
  int (*single)(orbx_ctx*, const orbx_keypoint*, int, const orbx_keypoint*, int, const int32_t*, int, const int32_t*, float,
                orbx_hf_result*, uint8_t*, float*, float*) = orbx_find_models;
  int (*batch)(orbx_ctx*, int, int, const int32_t*, const int32_t*, const orbx_keypoint*, const int32_t*, int, const int32_t*, int,
               const int32_t*, float, orbx_hf_result*, uint8_t*, float*, float*) = orbx_find_models_batch_device;
  std::printf("size %zu status %zu model %zu n_matches %zu best_it_h %zu n_inliers_f %zu score_h %zu rh %zu H21 %zu H12 %zu F21 %zu\n",
              sizeof(orbx_hf_result), offsetof(orbx_hf_result, status), offsetof(orbx_hf_result, model),
              offsetof(orbx_hf_result, n_matches), offsetof(orbx_hf_result, best_it_h), offsetof(orbx_hf_result, n_inliers_f),
              offsetof(orbx_hf_result, score_h), offsetof(orbx_hf_result, rh), offsetof(orbx_hf_result, H21),
              offsetof(orbx_hf_result, H12), offsetof(orbx_hf_result, F21));
  std::printf("flags %d %d %d %d\n", ORBX_INIT_TOO_FEW_MATCHES, ORBX_INIT_BAD_SETS, ORBX_INIT_NO_SCORE, ORBX_INIT_BAD_MATCHES);
  return (single && batch) ? 0 : 1;
}
