/* orbx.h — C ABI of the MI355X-native ORB extract + initialization-match hot path.
 *
 * Drop-in boundary for zeal-up/ORB_SLAM_Tracking's
 *   ORBextractor::ORBextractor / operator()            (Features/ORBextractor.hpp:68-85, .cpp:492-595, 1531-1653)
 *   ORBextractor getters + mvImagePyramid              (Features/ORBextractor.hpp:87-111)
 *   ORBmatcher::SearchForInitialization                (Features/ORBmatcher.hpp:36, .cpp:11-150)
 *   Frame grid rules the matcher depends on            (SlamTypes/Frame.cpp:70-99, 163-206)
 *   DBoW2 TemplatedVocabulary<FORB>::transform / score (Thirdparty/DBoW2; Frame::mBowVec / mFeatVec, "bag of words" below)
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.  The C++ classes with the
 * reference's own signatures live in include/orbx_shim.hpp and call only the functions below.
 *
 * All compute runs in hand-written HIP kernels for gfx950 (liborbx.so).  There is no CPU fallback:
 * every entry point that computes returns ORBX_E_HIP when no usable device / kernel image exists.
 *
 * Threading: one orbx_ctx is bound to one device; calls on one ctx must be
 * serialised by the caller; different ctxs are independent (multi-GPU = one ctx per device/process).
 */
#ifndef ORBX_H_
#define ORBX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes (negative).  ORBX_E_EMPTY == -1 keeps `operator()`'s "return -1 on empty image"
 * (Features/ORBextractor.cpp:1536). */
#define ORBX_OK 0
#define ORBX_E_EMPTY (-1)
#define ORBX_E_BADARG (-2)
#define ORBX_E_TOOSMALL (-3) /* a pyramid level is narrower than one FAST cell: UB upstream (cpp:1071-1074) */
/* Documented deviation: a frame wider or taller than ORBX_MAX_FRAME_DIM pixels returns ORBX_E_BADARG (orbx_last_error says so).
 * The reference has no such limit (Features/ORBextractor.cpp:1531-1545 takes any cv::Mat); here a FAST candidate is one 32-bit
 * word -- x and y in 12 bits each, the score in 8 -- and the selection kernels' path-code tables are indexed by those
 * coordinates.  4096 x 4096 covers every BASELINE configuration (the largest is 3840 x 2160). */
#define ORBX_MAX_FRAME_DIM 4096
#define ORBX_E_HIP (-4)
#define ORBX_E_CAPACITY (-5)
#define ORBX_E_RCCL (-6)     /* the multi-device context could not load / initialise RCCL, or a collective failed */

/* mirrors cv::KeyPoint (28 bytes): pt.x pt.y size angle response octave class_id */
typedef struct orbx_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} orbx_keypoint;

/* ORBextractor ctor arguments (Features/ORBextractor.hpp:68-69) */
typedef struct orbx_params {
  int32_t nfeatures;
  float scale_factor;
  int32_t nlevels;
  int32_t ini_th_fast;
  int32_t min_th_fast;
} orbx_params;

/* Frame::mnMinX/mnMaxX/mnMinY/mnMaxY (SlamTypes/Frame.hpp, static ints) */
typedef struct orbx_bounds {
  int32_t min_x, max_x, min_y, max_y;
} orbx_bounds;

/* the three counters SearchForInitialization prints (Features/ORBmatcher.cpp:144-147) */
typedef struct orbx_match_stats {
  int32_t invalid_by_distance, invalid_by_ratio, invalid_by_orientation;
} orbx_match_stats;

typedef struct orbx_ctx orbx_ctx;

/* ---- lifetime ---------------------------------------------------------------------------- */
/* Creates a context on `device_id` sized for batches of up to `max_batch` frames of up to
 * max_width x max_height pixels.  The sizes are an initial reservation, not a limit: like
 * ORBextractor::operator() (cpp:1531-1545), every extraction entry point takes any frame size up to ORBX_MAX_FRAME_DIM in either
 * direction (see there), and a call
 * that brings a larger frame or batch drains what is in flight and re-allocates the context's buffers
 * (a one-off cost of milliseconds; results are unaffected).  `stream` is an optional hipStream_t (as
 * void*) the caller wants the work issued on (e.g. torch's current stream); NULL = the ctx creates its own.
 * Replaces ORBextractor::ORBextractor (cpp:492-595); scaleFactor==1 with nlevels>1 returns
 * ORBX_E_BADARG instead of exit(1) (cpp:502-505). */
int orbx_create(const orbx_params* params, int device_id, int max_width, int max_height, int max_batch,
                void* stream, orbx_ctx** out);
void orbx_destroy(orbx_ctx* ctx);

/* The two constants of the path that depend on the OpenCV release the reference is linked against (its CMakeLists.txt:13 pins
 * none), selectable per context so that the library can be diffed against any OpenCV-linked build without touching a kernel:
 *   gaussian_variant  Q8 taps of cv::GaussianBlur(7x7, sigma 2) on 8-bit images (ORBextractor.cpp:1601):
 *     ORBX_GAUSS_ERROR_DIFFUSION (default)  [18,34,48,56,48,34,18], sum 256: getGaussianKernelFixedPoint_ED, OpenCV >= 4.1.1 / 3.4.7
 *     ORBX_GAUSS_ROUNDED                    [18,34,49,55,49,34,18], sum 257: each tap rounded, the bit-exact path of OpenCV
 *                                           3.4.1 .. 3.4.6 / 4.0 .. 4.1.0 and the integer filter of older releases
 *   gray_variant      cv::cvtColor RGB/BGR -> gray on 8-bit (Converter.cpp:11-13):
 *     ORBX_GRAY_14BIT (default)             (R*4899 + G*9617 + B*1868 + 2^13) >> 14: OpenCV 3.x .. 4.0
 *     ORBX_GRAY_15BIT                       (R*9798 + G*19235 + B*3735 + 2^14) >> 15: OpenCV >= 4.1
 * Takes effect for the calls that follow (batches in flight are waited for; like every call that has to wait for an earlier
 * stream-ordered batch, this one returns that batch's error WITHOUT having done its own work: call it again). */
#define ORBX_GAUSS_ERROR_DIFFUSION 0
#define ORBX_GAUSS_ROUNDED 1
#define ORBX_GRAY_14BIT 0
#define ORBX_GRAY_15BIT 1
int orbx_set_opencv_variant(orbx_ctx* ctx, int gaussian_variant, int gray_variant);

/* The libm reading of the reference's two unqualified <cmath> calls on floats: cos(angle) / sin(angle) of computeOrbDescriptor
 * (Features/ORBextractor.cpp:174) and pow(factor, (float)nlevels) of the constructor (cpp:536).  The file has no `using namespace
 * std` (cpp:69-71 import list / pair / vector only), so which function a call resolves to depends on the headers in the
 * translation unit (DESIGN.md section 2 derives it from the reference's includes):
 *   ORBX_LIBM_DOUBLE            only ::cos(double) / ::pow(double, double) are visible in the global namespace (<cmath> alone):
 *                               the float is promoted, the double result converted back -- (float)cos((double)angle).  The
 *                               default of rounds 1-4.
 *   ORBX_LIBM_FLOAT (default)   libstdc++'s <math.h> wrapper is in the include chain (`using std::cos;` ...): std::cos(float) =
 *                               cosf, std::pow(float, float) = powf.  The default since round 5: <opencv2/opencv.hpp>
 *                               (Features/ORBextractor.hpp:24) brings <math.h> in through opencv2/flann/lsh_table.h [from knowledge of
 *                               OpenCV 3.x / 4.x; tools/pin_opencv/libm_probe.cpp lets the compiler confirm it against a real one],
 *                               and the ORB-SLAM sources this file descends from say `using namespace std`.  cosf / sinf = glibc >= 2.28's algorithm, restated in the
 *                               kernel operation for operation (it is not correctly rounded: of the 1,135,869,953 f32 angles
 *                               in [0, 360], 1,484,894 give a different (cos, sin) pair than ORBX_LIBM_DOUBLE, and for 96 of
 *                               them a rotated sample point lands on another pixel); powf = the host libm's.
 *                               SCOPE OF THE CLAIM: "FLOAT" means the sinf / cosf of glibc >= 2.28 (2018; the
 *                               s_sincosf.h algorithm) on an x86-64 host -- with or without FMA contraction, both forms were
 *                               checked against the host's libm for every angle.  A reference built on an OLDER glibc (Ubuntu
 *                               16.04 / 18.04: 2.23 / 2.27) ran another sinf / cosf, which NEITHER reading reproduces exactly;
 *                               and powf(factor, nlevels) in the constructor is the DEPLOY host's libm, so for the rare
 *                               (factor, nlevels, nfeatures) combinations above two hosts may plan different per-level quotas.
 *                               The default stays a reasoned choice, not a measured one, until tools/pin_opencv/libm_probe has
 *                               been compiled against a real OpenCV (neither this image nor the GPU
 *                               box has one).
 * Takes effect for the calls that follow (batches in flight are waited for; an earlier batch's error is returned as by
 * orbx_set_opencv_variant).  If the constructor's pow changes a per-level quota (it does for 138 of 8e8 tried (factor, nlevels,
 * nfeatures) combinations and never for a scale factor with two decimals), the context's buffers are re-planned. */
#define ORBX_LIBM_DOUBLE 0
#define ORBX_LIBM_FLOAT 1
#define ORBX_LIBM_DEFAULT ORBX_LIBM_FLOAT
int orbx_set_libm_variant(orbx_ctx* ctx, int libm_variant);
const char* orbx_last_error(const orbx_ctx* ctx);

/* ---- getters (Features/ORBextractor.hpp:87-108) ------------------------------------------- */
int orbx_get_levels(const orbx_ctx* ctx);
float orbx_get_scale_factor(const orbx_ctx* ctx);
/* each out array has nlevels entries; any pointer may be NULL */
int orbx_get_tables(const orbx_ctx* ctx, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                    int32_t* features_per_level);
int orbx_get_umax(const orbx_ctx* ctx, int32_t* umax16);

/* ---- extraction: ORBextractor::operator() (cpp:1531-1653) --------------------------------- */
/* One frame from host memory.  Returns monoIndex (>= 0; == *n_out when lap0 == lap1 == 0, as in
 * Frame.cpp:58-60) or a negative error.  `kps`/`desc32` must hold `capacity` >= nfeatures entries
 * (keypoints 28 B, descriptors 32 B each). */
int orbx_extract(orbx_ctx* ctx, const uint8_t* img, int width, int height, int stride, int lap0, int lap1,
                 orbx_keypoint* kps, uint8_t* desc32, int capacity, int* n_out);

/* Optional, for a host that keeps its frames in buffers of its own (a camera ring, a decoder's pool): page-locks [ptr, ptr + bytes)
 * so that orbx_extract / orbx_extract_batch copy a frame out of it with one asynchronous DMA instead of through the runtime's
 * staging copy of pageable memory (measured at 640x480: 1-2 us of the call's ~85, BENCH_r04 single_frame.cpp_shim 0.0849 against
 * 0.0836 ms; more for large frames, and it is what keeps orbx_extract_match_batch_host_async's uploads asynchronous).  Thin wrappers over hipHostRegister / hipHostUnregister
 * (a C++ host need not link HIP); the buffer must be unregistered before it is freed.  Results are the same either way. */
int orbx_host_register(orbx_ctx* ctx, void* ptr, size_t bytes);
int orbx_host_unregister(orbx_ctx* ctx, void* ptr);

/* `n_frames` same-sized frames from host memory (frame f at imgs + f*frame_stride_bytes).
 * Outputs: frame f's keypoints at kps + f*capacity, descriptors at desc32 + f*capacity*32,
 * counts n_out[f], return values (monoIndex) mono_out[f] (may be NULL). */
int orbx_extract_batch(orbx_ctx* ctx, int n_frames, const uint8_t* imgs, int width, int height, int stride,
                       size_t frame_stride_bytes, int lap0, int lap1, orbx_keypoint* kps, uint8_t* desc32,
                       int capacity, int* n_out, int* mono_out);

/* Same, but the frames are already resident in device memory (HBM) and results stay there:
 * d_kps / d_desc32 / d_n_out are device pointers (d_n_out: int32[n_frames]).  Nothing is copied
 * to the host except two error flags and the per-frame counts; there is no host round trip between
 * the stages.  The call returns after the work has completed on the ctx stream. */
int orbx_extract_batch_device(orbx_ctx* ctx, int n_frames, const uint8_t* d_imgs, int width, int height,
                              int stride, size_t frame_stride_bytes, orbx_keypoint* d_kps, uint8_t* d_desc32,
                              int capacity, int32_t* d_n_out);

/* mvImagePyramid (hpp:111): copies level `level` of frame `frame` of the last extract call to host.
 * `border` = 0 copies the w x h level; border = 19 reproduces the reference's REFLECT_101 ring
 * (cpp:1689,1708), dst then is (w+38) x (h+38).  dst_stride in bytes. */
int orbx_level_size(const orbx_ctx* ctx, int level, int* width, int* height);
int orbx_download_pyramid(orbx_ctx* ctx, int frame, int level, int border, uint8_t* dst, int dst_stride);

/* ---- matching: ORBmatcher::SearchForInitialization (ORBmatcher.cpp:11-150) ----------------- */
/* k1/d1 = F1.mvKeysUn / F1.mDescriptors (n1 entries), k2/d2 = F2's; `bounds` = Frame::mnMin/Max*;
 * the 64x48 grid of F2 is rebuilt inside with Frame::PosInGrid's rule (Frame.cpp:89-99), so callers
 * do not pass mGrid.  matches12 has n1 entries (-1 = none).  *nmatches receives the reference's return value
 * exactly as it computes it (its double-decrement quirk can make it differ from the number of non-negative
 * entries, even negative), which is why it is an out-parameter; the function returns ORBX_OK or an error.
 * A query keypoint with a NEGATIVE octave (ORBextractor never produces one) is matched against F2's keypoints of EVERY
 * octave, as the reference's GetFeaturesInArea(.., octave, octave) skips its level check for a negative level (Frame.cpp:179);
 * a query of octave 0 against F2's octave-0 keypoints.  Pinned to the reference's compiled matcher (tests/test_gpu_ref_pins.py). */
int orbx_match_init(orbx_ctx* ctx, const orbx_keypoint* k1, const uint8_t* d1, int n1, const orbx_keypoint* k2,
                    const uint8_t* d2, int n2, const orbx_bounds* bounds, int window_size, float nnratio,
                    int check_orientation, int32_t* matches12, int32_t* nmatches, orbx_match_stats* stats);

/* Batched, device-resident: pair p matches frame first[p] against frame second[p] of the arrays a
 * previous orbx_extract_batch_device call filled (same capacity / layout).  d_matches12 is
 * int32[n_pairs*capacity], d_nmatches int32[n_pairs], d_stats (nullable) int32[n_pairs*3];
 * h_first/h_second are host arrays. */
int orbx_match_init_batch_device(orbx_ctx* ctx, int n_pairs, const int32_t* h_first, const int32_t* h_second,
                                 const orbx_keypoint* d_kps, const uint8_t* d_desc32, const int32_t* d_n,
                                 int capacity, const orbx_bounds* bounds, int window_size, float nnratio,
                                 int check_orientation, int32_t* d_matches12, int32_t* d_nmatches,
                                 int32_t* d_stats);

/* The whole hot path of one batch in one call: orbx_extract_batch_device followed by
 * orbx_match_init_batch_device on pairs of frames of the same batch (first[p], second[p] in [0, n_frames)).
 * Large batches are issued as two half-batches on two HIP streams, and a pair whose frames lie in the same half
 * is matched right behind that half's extraction, so the latency-bound stages (quadtree selection, sequential
 * matching) of one half overlap the arithmetic-bound stages of the other.  Results are identical to the two
 * separate calls.  n_pairs may be 0. */
int orbx_extract_match_batch_device(orbx_ctx* ctx, int n_frames, const uint8_t* d_imgs, int width, int height,
                                    int stride, size_t frame_stride_bytes, orbx_keypoint* d_kps, uint8_t* d_desc32,
                                    int capacity, int32_t* d_n_out, int n_pairs, const int32_t* h_first,
                                    const int32_t* h_second, const orbx_bounds* bounds, int window_size, float nnratio,
                                    int check_orientation, int32_t* d_matches12, int32_t* d_nmatches, int32_t* d_stats);

/* Stream-ordered form of the call above for callers that keep the device busy across batches (a tracker that prepares
 * batch k+1 while batch k runs): issues the batch and returns.  At most two batches are in flight (orbx_set_pipeline_depth
 * changes that) - a third call first waits for the oldest.  The outputs, counts and errors of a batch are valid once an orbx_wait_one / orbx_wait has covered
 * it (an error of an earlier batch can also be returned by the call that has to wait for it); batches in flight together
 * must be given different output arrays; the input frames must stay untouched until their batch has been waited for.
 * Every other call on the context may be used in between (the synchronous ones simply queue behind). */
int orbx_extract_match_batch_device_async(orbx_ctx* ctx, int n_frames, const uint8_t* d_imgs, int width, int height,
                                          int stride, size_t frame_stride_bytes, orbx_keypoint* d_kps, uint8_t* d_desc32,
                                          int capacity, int32_t* d_n_out, int n_pairs, const int32_t* h_first,
                                          const int32_t* h_second, const orbx_bounds* bounds, int window_size,
                                          float nnratio, int check_orientation, int32_t* d_matches12,
                                          int32_t* d_nmatches, int32_t* d_stats);

/* The same stream-ordered call for frames and results in HOST memory -- what the reference's call site hands over (a host
 * cv::Mat per frame, SlamTypes/Frame.cpp:58-60), batched: per batch the frames are uploaded, the kernels run and every result array
 * is copied back, all stream-ordered on the lane the batch goes to, so that with orbx_set_pipeline_depth(N >= 2) the upload of one
 * batch runs under the kernels of the batches in front of it and the call is bound by the slower of the PCIe link and the
 * kernels (640x480: the link; bench.py reports the rate beside the H2D rate of the box as `host_pipeline`).  h_imgs and the
 * result arrays should be page-locked (hipHostMalloc, orbx_host_register): from pageable memory the runtime stages every copy
 * synchronously and the call degenerates to orbx_extract_batch's rate.  All arrays are host pointers with the layout of the
 * device call (h_kps [n_frames][capacity], h_desc32 [n_frames][capacity][32], h_n_out [n_frames], h_matches12 [n_pairs][capacity],
 * h_nmatches [n_pairs], h_stats nullable [n_pairs][3]); entries beyond a frame's count are unspecified.  Valid once an
 * orbx_wait_one / orbx_wait has covered the batch; inputs and outputs must stay untouched until then.  With pipeline depth 0 one
 * batch is in flight at a time (the call first waits for the previous one).  From its first use on, every batch of the context
 * carries all of its matcher kernels (as after orbx_order_before): the copies back run behind the kernels, not behind a wait. */
int orbx_extract_match_batch_host_async(orbx_ctx* ctx, int n_frames, const uint8_t* h_imgs, int width, int height,
                                        int stride, size_t frame_stride_bytes, orbx_keypoint* h_kps, uint8_t* h_desc32,
                                        int capacity, int32_t* h_n_out, int n_pairs, const int32_t* h_first,
                                        const int32_t* h_second, const orbx_bounds* bounds, int window_size,
                                        float nnratio, int check_orientation, int32_t* h_matches12,
                                        int32_t* h_nmatches, int32_t* h_stats);

/* Pipeline depth of the stream-ordered call (default 0).  depth 0: a batch is cut into two halves that run on the context's two
 * streams, at most two batches in flight.  depth >= 1: the context keeps `depth` lanes (each with its own stream and its own
 * copy of the internal buffers, sized like the context) and every stream-ordered batch goes, whole, to the next lane; at most
 * `depth` batches are in flight (the call that would exceed it first waits for the oldest), so batches in flight together need
 * `depth` different output arrays.  Whole batches on four lanes measure 341 k frames/s against 323 k with the two halves at
 * 256 frames 640x480 per batch, and 239 k against 109 k at 32 frames per batch on three lanes (MI355X, rounds 3-4).  Waits for
 * everything in flight (and returns an earlier batch's error without changing the depth: call it again); 0 <= depth <= 8; costs depth times the context's
 * device memory; not available (ORBX_E_BADARG) on a context created on a caller's stream, whose order the lanes' own streams could
 * not keep.  orbx_download_pyramid and the profile / debug hooks of the context keep referring to the batches the context
 * ran itself (synchronous calls, depth 0); orbx_profile_get adds what the lanes ran.  (The reference has no counterpart: it
 * extracts one frame per call, Frame.cpp:58-60.) */
int orbx_set_pipeline_depth(orbx_ctx* ctx, int depth);
int orbx_wait_one(orbx_ctx* ctx); /* the oldest batch in flight (ORBX_OK if there is none) */
int orbx_wait(orbx_ctx* ctx);     /* all batches in flight */

/* Stream ordering against a caller's stream.  The context issues its work on its own HIP streams, which nothing
 * orders against the stream the caller produces frames / consumes results on (e.g. torch's current stream):
 *   orbx_order_after(ctx, s):  work issued on ctx from now on starts after everything queued on `s` so far
 *                              (call it between producing the frames on `s` and the device-resident entry points);
 *   orbx_order_before(ctx, s): work queued on `s` from now on starts after everything issued on ctx so far
 *                              (for a consumer that reads the outputs of an _async batch without a host-side wait).
 * `s` is a hipStream_t as void* (NULL = the legacy default stream).  Both only record / wait on events, with one exception:
 * the FIRST orbx_order_before on a context switches it to "event-ordered" mode -- from then on every batch carries all of its
 * matcher kernels (normally the kernels for pairs beyond the fast matcher's tables are issued only while batches need them, and
 * a batch that needed them without having them is completed inside its orbx_wait), and batches already in flight that were
 * issued without them are completed right there with a host-side wait.  After it, outputs (keypoints, descriptors, counts,
 * matches12, nmatches, statistics) read behind the event are final.  Error codes (ORBX_E_CAPACITY of the selection stage) are
 * still reported by orbx_wait_one / orbx_wait only, which an event-ordered consumer calls later, at its leisure. */
int orbx_order_after(orbx_ctx* ctx, void* stream);
int orbx_order_before(orbx_ctx* ctx, void* stream);

/* ---- between extractor and matcher: Frame::UndistortKeyPoints / ComputeImageBounds ---------- */
/* (SlamTypes/Frame.cpp:101-161)  The camera as the reference holds it: mK's four entries and
 * mDistCoef = (k1, k2, p1, p2), all CV_32F (Config/Settings.hpp:28-39). */
typedef struct orbx_camera {
  float fx, fy, cx, cy;
  float k1, k2, p1, p2;
} orbx_camera;

/* mvKeysUn of one frame, host memory: out[i] = kps[i] with pt replaced by cv::undistortPoints(pt, K, dist, R = I, P = K)
 * (5 fixed iterations in f64, result stored as f32).  k1 == 0 copies the keypoints unchanged (Frame.cpp:138-142). */
int orbx_undistort_keypoints(orbx_ctx* ctx, const orbx_keypoint* kps, int n, const orbx_camera* cam, orbx_keypoint* out);

/* Batched, device-resident: frame f's d_n[f] keypoints at d_kps + f*capacity -> d_kps_un + f*capacity (the layout of
 * orbx_extract_batch_device; d_kps_un may equal d_kps).  Feed d_kps_un to orbx_match_init_batch_device. */
int orbx_undistort_batch_device(orbx_ctx* ctx, int n_frames, const orbx_keypoint* d_kps, const int32_t* d_n, int capacity,
                                const orbx_camera* cam, orbx_keypoint* d_kps_un);

/* Frame::ComputeImageBounds (Frame.cpp:101-134): the four image corners undistorted on the device, min/max truncated
 * to the reference's static ints; k1 == 0 gives (0, width, 0, height). */
int orbx_image_bounds(orbx_ctx* ctx, const orbx_camera* cam, int width, int height, orbx_bounds* out);

/* ---- in front of the extractor: Converter::toGray (Utils/Converter.cpp:5-19) -------- */
/* channels == 1 copies, channels == 3 is cv::cvtColor(COLOR_RGB2GRAY if rgb else COLOR_BGR2GRAY) on 8-bit pixels,
 * Y = (R*4899 + G*9617 + B*1868 + 8192) >> 14; any other channel count returns ORBX_E_BADARG ("Wrong image format",
 * the reference's `return false`).  Strides in bytes.  Host buffers: */
int orbx_to_gray(orbx_ctx* ctx, const uint8_t* img, int width, int height, int stride, int channels, int rgb, uint8_t* gray,
                 int gray_stride);
/* device-resident batch: frame f at d_src + f*frame_stride_bytes -> d_gray + f*gray_frame_stride_bytes, ready to be
 * handed to orbx_extract_batch_device / orbx_extract_match_batch_device. */
int orbx_to_gray_batch_device(orbx_ctx* ctx, int n_frames, const uint8_t* d_src, int width, int height, int stride,
                              size_t frame_stride_bytes, int channels, int rgb, uint8_t* d_gray, int gray_stride,
                              size_t gray_frame_stride_bytes);

/* ---- behind the matcher: the Initializer's model scoring (Initialization/Initializer.cpp:268-438) -- */
/* CheckHomography / CheckFundamental for `n_models` RANSAC hypotheses at once (the loops of FindHomography :180-211 and
 * FindFundamental :231-265 call them once per iteration).  H21 / H12 / F21: n_models row-major 3x3 matrices (Eigen's
 * (row, col)); k1 / k2 = mvKeys1 / mvKeys2 (the frames' mvKeysUn); matches12 = the matcher's vnMatches12 (n1 entries),
 * from which mvMatches12 is built as in Initializer::Initialize :24-33 (pairs (i, matches12[i]) with matches12[i] >= 0, in
 * order).  scores[m] = the returned score, inliers[m * N + i] = vbMatchesInliers[i] for the N = *n_matches_out pairs (the
 * caller provides n_models * n1 bytes).  best (nullable) = the hypothesis the RANSAC loop would keep: first maximum of the
 * scores, -1 if none is > 0.  Host pointers. */
int orbx_check_homography(orbx_ctx* ctx, int n_models, const float* H21, const float* H12, const orbx_keypoint* k1, int n1,
                          const orbx_keypoint* k2, int n2, const int32_t* matches12, float sigma, float* scores,
                          uint8_t* inliers, int* n_matches_out, int* best);
int orbx_check_fundamental(orbx_ctx* ctx, int n_models, const float* F21, const orbx_keypoint* k1, int n1,
                           const orbx_keypoint* k2, int n2, const int32_t* matches12, float sigma, float* scores,
                           uint8_t* inliers, int* n_matches_out, int* best);

/* Initializer::CheckRT (Initialization/Initializer.cpp:569-713) for `n_models` (R21, t21) hypotheses at once -- ReconstructHF
 * (:440-567) calls it once per candidate of cv::decomposeEssentialMat / cv::decomposeHomographyMat with the same matches and
 * inlier flags.  R21: n_models row-major 3x3, t21: n_models x 3, K: row-major 3x3 (all CV_32F upstream); k1 / k2 / matches12 as
 * above; matches_inliers[i] = vbMatchesInliers[i] for the N pairs of mvMatches12; th2 = the squared reprojection threshold
 * (4 * sigma^2 upstream).  Outputs per model m: n_good[m] = the return value, tri_good[m * n1 + k] = vbTriGood[k],
 * p3d[(m * n1 + k) * 3 ..] = vP3D[k] (zeros where the reference books nothing), parallax[m] in degrees.  cv::triangulatePoints
 * is restated as a DLT with a fixed one-sided Jacobi SVD in f64; the reference's two quirks in this function (booking under
 * the compacted index, camera-2 depth test on z / z) are kept: see oracle/orbx_oracle.cpp.  Floating point: n_good and
 * tri_good equal the CPU restatement, points and parallax agree with it to 1e-4 relative (in practice bitwise).  Host pointers. */
int orbx_check_rt(orbx_ctx* ctx, int n_models, const float* R21, const float* t21, const float* K, const orbx_keypoint* k1, int n1,
                  const orbx_keypoint* k2, int n2, const int32_t* matches12, const uint8_t* matches_inliers, float th2,
                  int32_t* n_good, uint8_t* tri_good, float* p3d, float* parallax);

/* ---- behind the matcher: the RANSAC stage of Initializer::Initialize (Initialization/Initializer.cpp:19-111) ---------- */
/* For each pair: mvMatches12 (:24-33), then for every iteration `it` the 8-point hypotheses of the loops FindHomography
 * (:169-211) and FindFundamental (:213-265) on the caller's mvSets[it], scored with CheckHomography / CheckFundamental,
 * the first maximum of each loop (`currentScore > score`, score starting at 0), SH, SF, RH = SH / (SH + SF) (:89-90), the
 * inlier counts nH / nF (:95-100) and the model choice RH > 0.50 (:111).  The decomposition of the chosen model and
 * ReconstructHF (:440-566) are not part of this call: orbx_check_rt is their CheckRT.
 *
 * The solvers are restated [from-knowledge] from OpenCV (the reference calls cv::findHomography(src, dst, 0) and
 * cv::findFundamentalMat(src, dst, FM_8POINT)), in f64, then Converter::toMatrix3f (f32); H12 is Eigen's 3x3 inverse() in
 * f32.  PARITY UNPINNED, like every OpenCV-facing stage, and with these documented deviations:
 *  - findHomography's Levenberg-Marquardt refinement of the closed form is left out;
 *  - the 9x9 eigenproblems use a fixed-sweep cyclic Jacobi (not OpenCV's eigen), F's rank-2 step removes the component along
 *    the smallest right singular vector of the 3x3 (same matrix as OpenCV's SVD step, other operations);
 *  - a degenerate sample (OpenCV returns an empty Mat and the reference then reads it in toMatrix3f: UB) gets score 0 and is
 *    never kept; so is a hypothesis with a non-finite entry;
 *  - Initialize as committed upstream spawns FindHomographyCV / FindFundamentalCV (OpenCV's own RANSAC and RNG, which no
 *    library can reproduce) and leaves the mvSets it draws unused; this call runs the 8-point loops over mvSets that the same
 *    file keeps (FindHomography / FindFundamental), as ORB-SLAM does.
 * The sets come from the caller: the library reads no RNG state (the Python package's sample_sets restates the draw of
 * :50-63 for a given rand()). */
typedef struct orbx_hf_result {
  int32_t status;                /* 0, or a bitmask of ORBX_INIT_* reasons; the other fields are written either way */
  int32_t model;                 /* 0 = H (RH > 0.50), 1 = F; -1 when SH + SF == 0 */
  int32_t n_matches;             /* N = |mvMatches12| */
  int32_t best_it_h, best_it_f;  /* the iteration each loop kept, -1 if no score was > 0 */
  int32_t n_inliers_h, n_inliers_f;
  int32_t reserved;
  float score_h, score_f, rh;    /* SH, SF, RH (0 when SH + SF == 0) */
  float H21[9], H12[9], F21[9];  /* the kept hypotheses, row-major (zeros when none was kept) */
} orbx_hf_result;

#define ORBX_INIT_TOO_FEW_MATCHES 1 /* N < 8: the sampler of :50-63 cannot run (rand() % 0 upstream) */
#define ORBX_INIT_BAD_SETS 2        /* a set index outside [0, N) or repeated within its set: that hypothesis is skipped */
#define ORBX_INIT_NO_SCORE 4        /* SH + SF == 0 (:89, Initialize returns false) */
#define ORBX_INIT_BAD_MATCHES 128   /* a matches12 entry >= n2, or a frame's keypoint count outside [0, capacity]: nothing is
                                     * scored for the pair */

#define ORBX_INIT_AMBIGUOUS 8         /* secondBestGood > 0.7 * bestGood (:509) */
#define ORBX_INIT_LOW_PARALLAX 16      /* the best solution's parallax < min_parallax (:515) */
#define ORBX_INIT_FEW_TRIANGULATED 32  /* bestGood < min_triangulated (:521) */
#define ORBX_INIT_FEW_INLIERS 64       /* bestGood < 0.9 * the inliers of the chosen model (:527) */

/* ---- Initializer::Initialize end to end (Initialization/Initializer.cpp:19-125): the stage above, then ReconstructHF
 * (:440-566): the chosen model decomposed -- F: E = K^T F K (Eigen, f32) and cv::decomposeEssentialMat, four candidates in the
 * order of :458-466; H: cv::decomposeHomographyMat (the analytical Malis-Vargas decomposition, 1 or 4 solutions in OpenCV's
 * order) --, CheckRT of every candidate (orbx_check_rt's kernel, th2 = 4 sigma^2), the best / second-best choice (:490-507) and
 * the four acceptance rules (:509-545).  Initialize's `false` is status != 0 here, with ORBX_OK.  [from-knowledge], PARITY
 * UNPINNED; further deviations: both decompositions compute their SVD / eigen-decompositions in f64 with a fixed-sweep Jacobi
 * (decomposeEssentialMat runs on the CV_32F E upstream), so the sign of t and hence the order among the candidates may differ
 * from OpenCV's; square roots of rounding-negative minors in the homography decomposition are taken at 0 (OpenCV yields NaNs);
 * the reconstruction runs only behind a status-0 model stage (otherwise the reference has returned or is UB). */
typedef struct orbx_init_result {
  int32_t status;                /* 0 = reconstructed; else a bitmask of ORBX_INIT_* reasons; every field is written either way */
  int32_t model;                 /* 0 = H (RH > 0.50), 1 = F, -1 when SH + SF == 0 */
  int32_t n_matches;             /* N = |mvMatches12| */
  int32_t best_it_h, best_it_f;  /* the iteration each RANSAC loop kept (-1 if no score > 0) */
  int32_t n_inliers_h, n_inliers_f;
  int32_t n_solutions, best_solution, best_good, second_good;  /* ReconstructHF's candidates and CheckRT counts (-1: none) */
  int32_t reserved;
  float score_h, score_f, rh, parallax;  /* parallax of the best solution in degrees (-1 if none) */
  float R21[9], t21[3];          /* the chosen (R, t), row-major (zeros if none) */
  float H21[9], F21[9];          /* the kept hypotheses */
} orbx_init_result;

/* Batched, device-resident, stream-ordered on the context stream (the call returns once everything is queued; results are
 * valid after a device synchronisation, hipDeviceSynchronize): the layout of orbx_find_models_batch_device, K row-major 3x3 (host, f32),
 * min_parallax in degrees, min_triangulated (the reference passes 1 and 50, :103-111).  Outputs: d_res [n_pairs];
 * d_p3d (nullable) float [n_pairs][capacity][3] = vP3D, d_triangulated (nullable) uint8 [n_pairs][capacity] = vbTriangulated
 * of the best solution (zeros when there is none; entries beyond the pair's first-frame count are 0). */
int orbx_initialize_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_first, const int32_t* h_second,
                                 const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const int32_t* d_matches12,
                                 int n_iter, const int32_t* d_sets, const float* K, float sigma, float min_parallax,
                                 int min_triangulated, orbx_init_result* d_res, float* d_p3d, uint8_t* d_triangulated);
/* The same for one pair in host memory (what Tracking::Initialize holds), run through the batched path; p3d [n1][3] and
 * triangulated [n1] nullable.  Synchronous. */
int orbx_initialize(orbx_ctx* ctx, const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, const int32_t* matches12,
                    int n_iter, const int32_t* sets, const float* K, float sigma, float min_parallax, int min_triangulated,
                    orbx_init_result* res, float* p3d, uint8_t* triangulated);

/* Batched, device-resident, stream-ordered on the context stream (results valid after a device synchronisation, hipDeviceSynchronize): pair p = frame
 * h_first[p] vs h_second[p] (host arrays, in [0, n_frames)) of the extract / undistort layout (d_kps_un [frames][capacity],
 * d_n [frames]) and the matcher's d_matches12 [n_pairs][capacity] (entries beyond d_n[h_first[p]] are not read).
 * d_sets int32 [n_pairs][n_iter][8] = mvSets (indices into mvMatches12).  Device data is checked before it is read: bad
 * values are reported in status, never followed.  Outputs: d_res [n_pairs]; d_inliers (nullable) uint8 [n_pairs][2][capacity]
 * = vbMatchesInliersH, then vbMatchesInliersF, of the kept hypotheses (first N entries; zeros when none was kept); d_models
 * (nullable) float [3][n_pairs][n_iter][9] = every hypothesis's H21, H12, F21; d_scores (nullable) float [2][n_pairs][n_iter]
 * = every hypothesis's CheckHomography / CheckFundamental score (that of a degenerate or skipped hypothesis is unspecified).
 * ORBX_E_BADARG: null pointers, n_pairs / n_frames / n_iter <= 0, capacity outside [1, 2^20), a pair index outside
 * [0, n_frames); nothing is launched then. */
int orbx_find_models_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_first, const int32_t* h_second,
                                  const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const int32_t* d_matches12,
                                  int n_iter, const int32_t* d_sets, float sigma, orbx_hf_result* d_res, uint8_t* d_inliers,
                                  float* d_models, float* d_scores);
/* The same for one pair in host memory (k1 = mvKeys1, k2 = mvKeys2, matches12 = the n1 entries of vnMatches12, sets
 * [n_iter][8]), run through the batched path; inliers [2][n1], models [3][n_iter][9] and scores [2][n_iter] nullable.
 * Synchronous. */
int orbx_find_models(orbx_ctx* ctx, const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, const int32_t* matches12,
                     int n_iter, const int32_t* sets, float sigma, orbx_hf_result* res, uint8_t* inliers, float* models,
                     float* scores);

/* ---- behind the Initializer: two-view bundle adjustment (g2o, as Tracking::CreateInitialMapMonocular uses it) -----------------
 * Optimizer::GlobalBundleAdjustemnt(map, 20) of the ORB-SLAM design on the two initial keyframes and their points, the median-
 * depth normalisation and the "Wrong initialization, reseting" test behind it, for a batch of pairs, read from the arrays
 * orbx_initialize_batch_device left on the device.  The reference vendors the g2o types and solver (Thirdparty/g2o) but nothing
 * in it calls them: every rule below restates the g2o lines it cites, [from-knowledge] where Eigen is involved, PARITY UNPINNED
 * (no Eigen exists to compile g2o against).  The device equals the CPU restatement tests/cpp/ba_ref.cpp bit for bit.
 *
 * Graph.  Frame 1 is the identity pose, fixed.  Frame 2 starts at the Initializer's (R21, t21), f32 -> f64, as SE3Quat(R, t)
 * builds it (types/se3quat.h:58-60, :280-285): rotation matrix -> quaternion, w made non-negative, normalised.  One
 * VertexSBAPointXYZ (types/types_sba.h) per i with matches12[i] >= 0 && triangulated[i], ascending i, from vP3D[i] f32 -> f64.
 * Each point has two EdgeSE3ProjectXYZ (types/types_six_dof_expmap.h): obs = the keypoint's pt in its frame, information =
 * inv_sigma2[octave] * I, RobustKernelHuber with delta = (float)sqrt(5.99), fx fy cx cy from K.
 *
 * Per iteration (core/optimization_algorithm_levenberg.cpp:61-164):
 *  1. computeActiveErrors and activeRobustChi2 (rho[0] of every edge; core/robust_kernel_impl.cpp:78-91).
 *  2. linearizeOplus: the expressions of types/types_six_dof_expmap.cpp:98-134.
 *  3. constructQuadraticForm's robust branch (core/base_binary_edge.hpp:91-113): weightedOmega = rho[1] * omega, omega_r =
 *     -omega e rho[1]; robustInformation's commented-out second-order term stays out.
 *  4. At iteration 0 computeLambdaInit (:166-180): 1e-5 times the largest |diagonal entry| of the pose's and every point's block.
 *  5. Up to 10 trials (:102-149): setLambda on every diagonal; the Schur solve of core/block_solver.hpp:354-486 (Dinv = (Hll +
 *     lambda I)^-1 per point, Hschur = Hpp - sum Hpl Dinv Hpl^T, bschur = bp - sum Hpl Dinv bl, the 6x6 solve, xl = Dinv (bl -
 *     Hpl^T xp)); oplus: the pose by SE3Quat::exp(update) * estimate (se3quat.h:223-257, with its theta < 1e-5 branch and the
 *     normalisation of :104-110), the points by addition; the new errors, tempChi (DBL_MAX when the solve failed), computeScale
 *     (:182-189) + 1e-3, rho; accept (alpha = 1 - (2 rho - 1)^3 clamped to [1/3, 2/3], _ni = 2) or reject (lambda *= _ni,
 *     _ni *= 2, the state restored); another trial while rho < 0.
 *  6. Terminate when qmax == 10 || rho == 0 (:151); Raul Mur-Artal's rule (:155-161): _nBad counts the iterations in a row with
 *     (iniChi - currentChi) * 1e3 < iniChi, Terminate at 3.
 *  7. SparseOptimizer::optimize's loop (core/sparse_optimizer.cpp:376-414) ends on the first result that is not OK.
 * Behind the optimisation: the points go back to f32; ComputeSceneMedianDepth(2) in frame 1 = the z of the f32 points, sorted,
 * at element (n - 1) / 2; with normalize != 0 and no status bit set (and a median > 0), t21 and every refined point are
 * multiplied by 1.0f / median in f32, as CreateInitialMapMonocular does.
 *
 * Documented deviations:
 *  1. Sums.  Every sum over points (chi2, Hpp, bp, the Schur terms, computeScale) is f64 in this order: the workgroup has 256
 *     lanes; lane l adds the terms of points l, l + 256, l + 512, ... one after the other, a point's frame-1 edge before its
 *     frame-2 edge; in each wave of 64 lanes, lane l then adds lane l + 32's sum to its own, then lane l + 16's, + 8, + 4, + 2,
 *     + 1; the four waves' sums are added in wave order, starting from wave 0's.  computeScale adds the pose's six terms first,
 *     then the points' sum, then 1e-3.  g2o adds edge by edge.
 *  2. Small dense algebra.  The 3x3 inverse is by cofactors and one reciprocal of the determinant; the 6x6 solve is an unblocked
 *     lower Cholesky in which a pivot <= 0 or non-finite, or a non-finite solution, means the solve failed, and the whole step
 *     is then zero (g2o applies whatever its solver left); matrix -> quaternion uses Eigen's four-branch rule; pow(x, 3) is
 *     x * x * x.  The same mathematics as Eigen / libm, other rounding.
 *  3. sin(theta) and cos(theta) in SE3Quat::exp come from one restated f64 routine (csrc/orbx_ba_math.inc: Cody-Waite reduction
 *     by pi/2, fdlibm's polynomials), not from a libm; theta >= 2^19 gives NaN (and ORBX_BA_NONFINITE).
 *  4. There are no Map / KeyFrame / MapPoint types and no pbStopFlag.
 *  5. A pair whose orbx_init_result.status != 0 is skipped: the reference never reaches the adjustment for it.
 *  6. Garbage inputs set flags and never lead to an out-of-range read.  A pair with a status bit other than FEW_POINTS /
 *     NEGATIVE_DEPTH is not optimised: its points and (R21, t21) are the inputs, every other number is 0; a non-finite RESULT
 *     keeps its counters.  Without any point no iteration runs.  With n_iterations == 0 (or no point) chi2_initial and
 *     chi2_final are 0, the points and t21 come back bit for bit (f32 -> f64 -> f32), and R21 comes back as the rotation matrix
 *     of the normalised quaternion SE3Quat(R, t) built from it: within a few f32 roundings of the input, not its bits. */
#define ORBX_BA_SKIPPED 1        /* the pair's orbx_init_result.status != 0 */
#define ORBX_BA_BAD_INPUT 2      /* a frame count outside [0, capacity], a matches12 entry >= n2, an octave outside [0, nlevels) */
#define ORBX_BA_NONFINITE 4      /* a non-finite input point or pose, or a non-finite result */
#define ORBX_BA_FEW_POINTS 8     /* n_points < min_points (the reference: TrackedMapPoints(1) < 100) */
#define ORBX_BA_NEGATIVE_DEPTH 16 /* median depth < 0 */
typedef struct orbx_ba_result {
  int32_t status;           /* 0, or a bitmask of ORBX_BA_*; every field is written for every pair */
  int32_t n_points;         /* point vertices */
  int32_t iterations;       /* solve() calls made (g2o's cjIterations) */
  int32_t lm_trials;        /* the sum of qmax */
  int32_t rejected_trials;
  int32_t solver_failures;
  int32_t stop_reason;      /* 0 = all iterations ran, 1 = qmax == 10 || rho == 0, 2 = _nBad >= 3 */
  int32_t reserved;
  double chi2_initial, chi2_final, lambda;
  double q[4], t[3];        /* the refined pose as g2o holds it: quaternion (x, y, z, w) and translation */
  float R21[9], t21[3];     /* as Converter::toCvMat would store it (row-major), after the normalisation if it was applied */
  float median_depth;
  float reserved2;
} orbx_ba_result;

/* Batched, device-resident, stream-ordered on the context stream (results valid after a device synchronisation), in the layout
 * of orbx_initialize_batch_device, whose d_res / d_p3d / d_triangulated are d_init_res / d_p3d / d_triangulated here.  K row-major
 * 3x3 (host, f32); inv_sigma2: host, the context's nlevels floats (mvInvLevelSigma2), NULL = the context's own table;
 * n_iterations >= 0 (the reference passes 20); min_points (100).  Outputs: d_res [n_pairs]; d_p3d_out float [n_pairs][capacity][3]
 * = the refined points where a point vertex exists, d_p3d's entry elsewhere; it may equal d_p3d.  One workgroup per pair runs
 * the whole optimisation in one launch.  The call returns once queued, with one exception: when the pair list or the table differs
 * from the previous call's on this context, the call first waits for the context stream before it uploads them (the first call
 * always does); a caller that adjusts the same pairs of every batch, as the extract + match calls are used, never waits again.
 * ORBX_E_BADARG: null pointers, negative counts, n_frames < 1 with pairs, capacity < 1,
 * a pair index outside [0, n_frames), n_iterations < 0; ORBX_E_CAPACITY: capacity >= 2^20; ORBX_E_HIP: ctx == NULL with otherwise
 * well-formed arguments -- all checked before anything touches a device.  n_pairs == 0 is ORBX_OK. */
int orbx_bundle_adjust_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_first, const int32_t* h_second,
                                    const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const int32_t* d_matches12,
                                    const orbx_init_result* d_init_res, const float* d_p3d, const uint8_t* d_triangulated,
                                    const float* K, const float* inv_sigma2, int n_iterations, int min_points, int normalize,
                                    orbx_ba_result* d_res, float* d_p3d_out);
/* The same for one pair in host memory, run through the batched path as a batch of one; p3d_out [n1][3] may equal p3d.
 * Synchronous. */
int orbx_bundle_adjust(orbx_ctx* ctx, const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, const int32_t* matches12,
                       const orbx_init_result* init_res, const float* p3d, const uint8_t* triangulated, const float* K,
                       const float* inv_sigma2, int n_iterations, int min_points, int normalize, orbx_ba_result* res,
                       float* p3d_out);

/* ---- behind SearchByBoW: pose optimisation (Optimizer::PoseOptimization, motion-only bundle adjustment) ----------------------
 * What a tracker calls behind SearchByBoW in TrackReferenceKeyFrame and Relocalization: one free 6-dof pose, the matched map
 * points held fixed, four rounds of Levenberg-Marquardt with an outlier classification behind each, for a batch of independent
 * problems.  The reference vendors the g2o types and solver but has no Optimizer and no EdgeSE3ProjectXYZOnlyPose: the rules
 * below restate the monocular Optimizer::PoseOptimization of the ORB-SLAM2 design, built from the vendored VertexSE3Expmap, FIXED
 * VertexSBAPointXYZ and EdgeSE3ProjectXYZ (for the pose block the same arithmetic as the only-pose edge), [from-knowledge],
 * PARITY UNPINNED, as the two-view bundle adjustment above.  The device equals the CPU restatement tests/cpp/pose_ref.cpp bit for
 * bit.
 *
 * Graph.  One pose vertex, its start SE3Quat(R, t) of the caller's f32 Tcw (types/se3quat.h:58-60, :280-285, as above).  One
 * EdgeSE3ProjectXYZ per feature j of the frame that has a map point, ascending j: obs = the undistorted keypoint's pt,
 * information = inv_sigma2[octave] * I, RobustKernelHuber with delta = (float)sqrt(5.991) (`const float deltaMono`), fx fy cx
 * cy from K; the point vertex is fixed, so the edge adds a block to the pose only (core/base_binary_edge.hpp:65-113).  Every
 * feature's outlier flag starts false.  n_correspondences = the edges; below 3 the status is ORBX_POSE_FEW_POINTS, the pose is
 * returned as given and nothing runs (`if (nInitialCorrespondences < 3) return 0`).
 *
 * Four rounds, it = 0 .. 3 (`for (size_t it = 0; it < 4; it++)`):
 *  a. The pose is set back to the INITIAL estimate (`vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw))`).
 *  b. initializeOptimization(0): the active edges are those of level 0 = the features not flagged.
 *  c. optimize(n_iterations) (the reference design passes 10 in every round): the loop of core/sparse_optimizer.cpp:376-414 over
 *     OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:61-164), steps 1 to 7 of the bundle
 *     adjustment above without points: no Schur complement, computeLambdaInit over the pose's six diagonal entries,
 *     computeScale over the pose's six terms; _ni, _nBad and lambda start again at iteration 0 of every round (:93-97).  A round
 *     without an active edge runs no iteration (optimize returns at its empty index mapping).
 *  d. Classification.  For every edge `const float chi2 = e->chi2()` = e . (information e), not robustified, f64 -> f32;
 *     chi2 > 5.991f: the feature is flagged and its edge leaves the active set (level 1); otherwise it is not flagged (level 0).
 *     g2o's stale errors are kept: the design recomputes the error only of the edges that were flagged during the round.  An
 *     edge that was active keeps the _error of the last computeActiveErrors, which is that of the round's last TRIAL, accepted or
 *     not (:123, and pop() at :146 restores estimates, not errors).  So: edges flagged during the round are evaluated at the
 *     round's final pose, edges active during the round at the pose of its last trial (a trial whose solve failed applies a
 *     zero step: the pose before it); a round that ran no iteration uses the initial pose for both.  Behind round 2 the robust
 *     kernel is removed (`if (it == 2) e->setRobustKernel(0)`): round 3 runs with rho[0] = chi2, rho[1] = 1.
 *  e. `if (optimizer.edges().size() < 10) break`: the count is of ALL edges = n_correspondences, so with fewer than 10 only round
 *     0 runs.
 * Result: the pose behind the last round that ran, the flags, n_bad of that round, n_inliers = n_correspondences - n_bad (the
 * design's return value).
 *
 * Documented deviations:
 *  1. Sums.  Every sum over edges (chi2, Hpp, bp) is f64 in this order: a problem has 64 lanes; lane l adds the terms of the
 *     active features l, l + 64, l + 128, ... one after the other (features without an edge or flagged are passed over: feature j
 *     always belongs to lane j % 64); lane l then adds lane l + 32's sum to its own, then lane l + 16's, + 8, + 4, + 2, + 1; the
 *     result is lane 0's.  (The device adds lane l ^ 32's, l ^ 16's, ... so that every lane ends with lane 0's bits: f64 addition
 *     is commutative.)  g2o adds edge by edge.
 *  2. The small dense algebra and the sin / cos of deviations 2 and 3 above, through the shared csrc/orbx_ba_math.inc; a failed
 *     6x6 solve applies a zero step.
 *  3. There are no Frame / MapPoint types and no pbStopFlag: map points are coordinates plus a mask.
 *  4. Garbage inputs set flags and are never followed: a frame count outside [0, capacity], a match index >= capacity, an octave
 *     outside the table on a feature with a point (ORBX_POSE_BAD_INPUT), a non-finite point or pose, a non-finite resulting
 *     pose, chi2 or lambda (ORBX_POSE_NONFINITE).  Such a problem returns its inputs: R and tcw are d_pose0's bits, every flag
 *     is 0 and every other number of the result is 0.  So does a problem with ORBX_POSE_FEW_POINTS, except that
 *     n_correspondences and n_inliers are reported.
 *  5. n_iterations == 0 is accepted: nothing is optimised, the rounds only classify at the initial pose, and chi2_initial,
 *     chi2_final and lambda are 0.  Like every optimised pose, R comes back as the rotation matrix of the normalised quaternion
 *     built from it. */
#define ORBX_POSE_BAD_INPUT 2    /* a frame count outside [0, capacity], a match index >= capacity, an octave outside [0, nlevels) */
#define ORBX_POSE_NONFINITE 4    /* a non-finite input point or pose, or a non-finite result */
#define ORBX_POSE_FEW_POINTS 8   /* n_correspondences < 3 */
typedef struct orbx_pose_result {
  int32_t status;            /* 0, or a bitmask of ORBX_POSE_*; every field is written for every problem */
  int32_t n_correspondences; /* edges (nInitialCorrespondences) */
  int32_t n_bad;             /* flagged features behind the last round that ran */
  int32_t n_inliers;         /* n_correspondences - n_bad */
  int32_t rounds;            /* rounds that ran: 4, 1 with fewer than 10 correspondences, 0 when nothing ran */
  int32_t iterations[4];     /* solve() calls of each round */
  int32_t lm_trials;         /* over all rounds: the sum of qmax */
  int32_t rejected_trials;
  int32_t solver_failures;
  int32_t stop_reason[4];    /* per round: 0 = all iterations ran, 1 = qmax == 10 || rho == 0, 2 = _nBad >= 3 */
  double chi2_initial;       /* activeRobustChi2 at the initial pose in round 0 */
  double chi2_final, lambda; /* of the last round that ran an iteration */
  double q[4], t[3];         /* the pose as g2o holds it: quaternion (x, y, z, w) and translation */
  float R[9], tcw[3];        /* as Converter::toCvMat would store it (row-major) */
} orbx_pose_result;

/* Batched, device-resident, stream-ordered on the context stream (results valid after a device synchronisation).  Problem p
 * optimises frame h_frame[p] (its d_kps_un / d_n rows, the layout of the extract calls) against point set h_point_set[p] of
 * d_points float [n_point_sets][capacity][3] and d_point_mask uint8 [n_point_sets][capacity] (NULL = every entry is a point),
 * from d_pose0 float [n_problems][12] (R row-major, then t).  With d_match == NULL feature j's point is entry j of the set, where
 * the mask is set.  With d_match int32 [n_problems][capacity], it is entry i = d_match[p][j] >= 0, where the mask at i is set:
 * the layout of orbx_match_bow_batch_device's d_matches_f with the keyframe's map points as the point set, so SearchByBoW ->
 * PoseOptimization chains on the device without a gather or a copy.  A frame and a point set may appear in any number of
 * problems.  K row-major 3x3 (host, f32); inv_sigma2: host, the context's nlevels floats, NULL = the context's own table;
 * n_iterations >= 0 (10).  Outputs: d_res [n_problems]; d_outlier uint8 [n_problems][capacity]: 1 = feature j is flagged; every
 * entry is written.  One wave of 64 lanes runs a problem's whole optimisation, four problems per workgroup, in one launch.  The
 * call returns once queued, with the one exception orbx_bundle_adjust_batch_device has: when the problem list or the table differs
 * from the previous call's on this context, the call first waits for the context stream before it uploads them.
 * ORBX_E_BADARG: null pointers, negative counts, capacity < 1, n_iterations < 0, a frame index outside [0, n_frames), a point set
 * outside [0, n_point_sets); ORBX_E_CAPACITY: capacity >= 2^20; ORBX_E_HIP: ctx == NULL with otherwise well-formed arguments -- all
 * checked before anything touches a device.  n_problems == 0 is ORBX_OK. */
int orbx_pose_optimize_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_frame, const int32_t* h_point_set,
                                    const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const int32_t* d_match,
                                    int n_point_sets, const float* d_points, const uint8_t* d_point_mask, const float* d_pose0,
                                    const float* K, const float* inv_sigma2, int n_iterations, orbx_pose_result* d_res,
                                    uint8_t* d_outlier);
/* The same for one problem in host memory (the direct form: points [n][3], mask [n] nullable, pose0 [12], outlier [n]), run
 * through the batched path as a batch of one.  Synchronous. */
int orbx_pose_optimize(orbx_ctx* ctx, const orbx_keypoint* kps_un, int n, const float* points, const uint8_t* mask,
                       const float* pose0, const float* K, const float* inv_sigma2, int n_iterations, orbx_pose_result* res,
                       uint8_t* outlier);

/* ---- behind SearchByBoW: PnP RANSAC (PnPsolver: EPnP inside RANSAC, what Relocalization calls before PoseOptimization) ---------
 * A lost frame has no start pose for the call above.  ORB-SLAM2 gets one per candidate keyframe from PnPsolver: RANSAC over the
 * 2D-3D matches of SearchByBoW, each hypothesis Lepetit / Moreno-Noguer's EPnP on four correspondences.  The reference tree ships
 * no PnPsolver: the rules below restate ORB-SLAM2's PnPsolver.cc [from-knowledge], PARITY UNPINNED, as the two sections above.
 * The device equals the CPU restatement tests/cpp/pnp_ref.cpp bit for bit.
 *
 * Rules.
 *  1. Constructor.  For feature j of the frame in ascending j: it has a correspondence when it names a point (d_match == NULL:
 *     entry j; else entry i = d_match[p][j] >= 0) and the point mask there is set, exactly as orbx_pose_optimize_batch_device
 *     reads them.  mvP2D = the undistorted keypoint's pt, mvSigma2 = sigma2[octave], mvP3Dw = the point, mvKeyIndices = j.
 *     N = their number (n_correspondences).
 *  2. SetRansacParameters(probability, minInliers, maxIterations, minSet = 4, epsilon, th2) (the design passes 0.99, 10, 300, 4,
 *     0.5, 5.991): nMinInliers = (int)(N * epsilon) with the product in f32, raised to minInliers and to minSet = 4; epsilon (f32)
 *     raised to (float)nMinInliers / N; nIterations = 1 when nMinInliers == N, else (int)ceil(log(1 - probability) / log(1 -
 *     pow(epsilon, 3))) in f64; mRansacMaxIts = max(1, min(nIterations, maxIterations)); mvMaxError[i] = sigma2 * th2 in f32.  N
 *     is known only on the device and the device has no libm that equals the host's, so the host computes the table N ->
 *     (mRansacMinInliers, mRansacMaxIts) for N in [0, capacity] with these expression types (orbx_pnp_ransac_table) and uploads it.
 *     (nMinInliers grows with N beyond minInliers / epsilon, so the whole range is stored.)
 *  3. Sampling.  d_draws int32 [n_problems][n_iter][4] holds the values rand() returned, each in [0, ORBX_PNP_RAND_MAX]; the
 *     library reads no RNG state.  Draw i of a hypothesis picks entry randi = (int)(((double)r / ((double)RAND_MAX + 1.0)) * size)
 *     of the available list (DUtils::Random::RandomInt(0, size - 1)), size = N - i; the entry is replaced by the list's last and the
 *     list shrinks (vAvailableIndices' swap-and-pop).  The caller need not know N.  A negative draw skips the hypothesis (it counts
 *     no inlier) and sets ORBX_PNP_BAD_DRAWS.
 *  4. epnp compute_pose, all f64: choose_control_points (the centroid, then the eigenvectors of PW0^T PW0 scaled by
 *     sqrt(lambda / n)), compute_barycentric_coordinates, fill_M and M^T M (12x12), the eigenvectors of its four smallest
 *     eigenvalues, compute_L_6x10, compute_rho, find_betas_approx_1 / 2 / 3 over the columns {0,1,3,6}, {0,1,2}, {0,1,2,3,4},
 *     five gauss_newton steps each, compute_R_and_t (compute_ccs, compute_pcs, solve_for_sign on the first point,
 *     estimate_R_and_t with the det < 0 row flip), the mean reprojection error, and the choice N = 1; rep[2] < rep[1]: N = 2;
 *     rep[3] < rep[N]: N = 3 (beta_choice).
 *  5. CheckInliers keeps the reference's types: Xc, Yc, invZc, distX, distY and error2 are f32, ue and ve f64; the test is
 *     error2 < mvMaxError[i].  A hypothesis with a non-finite entry in R or t counts no inlier (n_degenerate) and is never kept.
 *  6. iterate.  Hypothesis `it` qualifies when inliers[it] >= mRansacMinInliers; best(it) is the first maximum of
 *     inliers[0..it] under strict >.  Refine() at a qualifying `it` runs compute_pose over the inliers of best(it) -- the best so
 *     far, not the current one -- and CheckInliers; it succeeds when the refined count is > mRansacMinInliers (strict) and the
 *     refined pose is finite.  The result is the first qualifying `it` whose best refines (found_it, refined = 1: the refined
 *     pose and the refined inliers).  Otherwise, with all min(n_iter, mRansacMaxIts) iterations run, it is the unrefined best
 *     when mnBestInliers >= mRansacMinInliers (refined = 0), else there is no pose.  N < mRansacMinInliers is bNoMore at once
 *     (ORBX_PNP_FEW_POINTS).
 *
 * Documented deviations:
 *  1. Every eigen / SVD step of OpenCV is the project's cyclic Jacobi with 12 fixed sweeps and no convergence test: orbx_decomp's
 *     eig3 for the 3x3s, its rotation on the packed 12x12 for M^T M; eigenvalues sorted descending and stable (of equal values
 *     the lower column first), eigenvector signs as the Jacobi leaves them.  cvInvert(CC) is the adjugate inverse inv33.
 *     The square roots of choose_control_points take a negative eigenvalue as 0.
 *  2. The 3x3 SVD of ABt goes through eig3 of ABt^T ABt: V = its eigenvectors, u_i = ABt v_i / |ABt v_i| for the two largest,
 *     u_2 = +-(u_0 x u_1) with the sign that gives det(U V^T) the sign of det(ABt) (a full SVD's, singular values >= 0).
 *  3. The least-squares solves (6x4, 6x3, 6x5) and gauss_newton's qr_solve are one Householder QR with back substitution; a
 *     singular system gives a non-finite result, which rule 5 drops (qr_solve returns with the betas unchanged there).
 *  4. Sums over points are f64 in this order.  A hypothesis adds its four points in the order drawn.  Refine's sums (the
 *     centroid, PW0^T PW0, the 78 entries of M^T M, for each beta set the camera-frame centroid, ABt and the reprojection
 *     error) run over the correspondences c = 0 .. N-1 in the constructor's order: lane c % 64 adds the terms of its inliers one
 *     after the other; lane l then adds lane l + 32's sum to its own, then l + 16's, + 8, + 4, + 2, + 1; the result is lane 0's
 *     (the order of the pose call's deviation 1).  The barycentric coordinates are recomputed from the point in every pass; pw0
 *     of estimate_R_and_t is the centroid of choose_control_points (the same sum and division).
 *  5. iterate is resolved after the fact: all hypotheses are computed, then the rule 6 is applied in iteration order.  Refine
 *     depends on best(it) alone, so it is evaluated once per distinct best (n_refines) -- a set that failed fails again.  The
 *     answer equals the sequential loop's (tests/cpp/pnp_ref.cpp holds both).
 *  6. One call is a solver's whole life.  ORB-SLAM2 calls iterate(5) in turns over the candidates to ration a CPU; the best state
 *     carries over, so the answer does not depend on the chunking, and found_it tells which turn would have returned it.  The
 *     design's loop condition (`mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`) is taken as the bound
 *     min(n_iter, mRansacMaxIts) on the solver's total.  There is no state across calls.
 *  7. Garbage is flagged and never followed: a frame count outside [0, capacity], a match index >= capacity, an octave outside
 *     the table on a feature with a point (ORBX_PNP_BAD_INPUT); a non-finite point or keypoint (ORBX_PNP_NONFINITE).  A problem
 *     that ends without a pose (these, ORBX_PNP_FEW_POINTS, or no qualifying hypothesis) carries ORBX_PNP_NO_POSE, zeros for
 *     R, t, Tcw and d_pose, and an all -1 row; the pose call then finds zero correspondences and answers ORBX_POSE_FEW_POINTS. */
#define ORBX_PNP_RAND_MAX 2147483647
#define ORBX_PNP_BAD_INPUT 2   /* a frame count outside [0, capacity], a match index >= capacity, an octave outside [0, nlevels) */
#define ORBX_PNP_NONFINITE 4   /* a non-finite input point or keypoint */
#define ORBX_PNP_FEW_POINTS 8  /* N < mRansacMinInliers: bNoMore at once */
#define ORBX_PNP_BAD_DRAWS 16  /* a draw outside [0, ORBX_PNP_RAND_MAX] among the iterations that ran */
#define ORBX_PNP_NO_POSE 32    /* no pose is returned */
typedef struct orbx_pnp_result {
  int32_t status;            /* 0, or a bitmask of ORBX_PNP_*; every field is written for every problem */
  int32_t n_correspondences; /* N (0 with BAD_INPUT / NONFINITE) */
  int32_t min_inliers;       /* mRansacMinInliers of N */
  int32_t max_its;           /* mRansacMaxIts of N */
  int32_t its_run;           /* found_it + 1, or min(n_iter, max_its); 0 when nothing ran */
  int32_t found_it;          /* the iteration whose Refine succeeded, or -1 */
  int32_t best_it;           /* the iteration of the best hypothesis when the solver stopped, or -1 */
  int32_t refined;           /* 1 = the pose is Refine's */
  int32_t n_inliers;         /* of the returned pose (nInliers) */
  int32_t n_best_inliers;    /* mnBestInliers when the solver stopped */
  int32_t n_refines;         /* Refine evaluations (distinct bests) */
  int32_t n_degenerate;      /* non-finite hypotheses among the iterations that ran */
  int32_t beta_choice;       /* 1 .. 3 of the returned pose, 0 without one */
  int32_t reserved;
  double R[9], t[3];         /* mRi / mti of the returned pose (row-major) */
  float Tcw[12];             /* R row-major, then t: d_pose0's layout */
} orbx_pnp_result;

/* The table of rule 2: out int32 [n_max + 1][2] = (mRansacMinInliers, mRansacMaxIts) for N = 0 .. n_max.  Host only.  For N <
 * mRansacMinInliers the design takes the logarithm of a negative number (and divides by N = 0): those entries get max_iterations;
 * such a solver is bNoMore before it iterates.  ORBX_E_BADARG for the parameter ranges below, n_max < 0 or NULL. */
int orbx_pnp_ransac_table(double probability, int min_inliers, int max_iterations, float epsilon, int n_max, int32_t* out);

/* Batched, device-resident, stream-ordered on the context stream.  Every argument up to d_point_mask means what it means in
 * orbx_pose_optimize_batch_device.  K row-major 3x3 (host, f32); sigma2: host, the context's nlevels floats (mvLevelSigma2), NULL =
 * the context's own; probability and epsilon in (0, 1), min_inliers >= 4, max_iterations >= 1, th2 > 0; d_draws int32
 * [n_problems][n_iter][4], n_iter >= 1.  Outputs: d_res [n_problems]; d_pose float [n_problems][12] and d_match_inliers int32
 * [n_problems][capacity] (= d_match[p][j], or j without d_match, for an inlier j and -1 otherwise; every entry is written): the
 * pose call's d_pose0 and d_match for the same problem lists; d_inliers uint8 [n_problems][capacity] (NULL = not wanted):
 * vbInliers.  Three launches: k_pnp_prep (a wave per problem), k_pnp_hypotheses (a lane per problem and iteration), k_pnp_refine
 * (a wave per problem).  The call returns once queued, with the pose call's exception: when the problem list, sigma2 or the
 * parameters' table differ from the previous call's on this context, or the workspace grows, it first waits for the context stream.
 * ORBX_E_BADARG: null required pointers, negative counts, capacity < 1, n_iter < 1, a parameter outside its range, a frame index
 * outside [0, n_frames), a point set outside [0, n_point_sets); ORBX_E_CAPACITY: capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx
 * == NULL with otherwise well-formed arguments -- all checked before anything touches a device.  n_problems == 0 is ORBX_OK. */
int orbx_pnp_solve_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_frame, const int32_t* h_point_set,
                                const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const int32_t* d_match,
                                int n_point_sets, const float* d_points, const uint8_t* d_point_mask, const float* K,
                                const float* sigma2, double probability, int min_inliers, int max_iterations, float epsilon, float th2,
                                int n_iter, const int32_t* d_draws, orbx_pnp_result* d_res, float* d_pose, int32_t* d_match_inliers,
                                uint8_t* d_inliers);
/* The same for one problem in host memory (the direct form: points [n][3], mask [n] nullable, draws [n_iter][4], inliers [n]), run
 * through the batched path as a batch of one.  Synchronous. */
int orbx_pnp_solve(orbx_ctx* ctx, const orbx_keypoint* kps_un, int n, const float* points, const uint8_t* mask, const float* K,
                   const float* sigma2, double probability, int min_inliers, int max_iterations, float epsilon, float th2, int n_iter,
                   const int32_t* draws, orbx_pnp_result* res, uint8_t* inliers);

/* ---- loop closing: Sim3 RANSAC (Sim3Solver: Horn's closed-form similarity inside RANSAC, what LoopClosing::ComputeSim3 calls) ----
 * A loop candidate found by the database and matched by SearchByBoW gives 3D-3D correspondences between the map points of the
 * current keyframe (KF1) and of the candidate (KF2).  ORB-SLAM2's Sim3Solver finds the similarity T12 = [s12 R12 | t12] between
 * the two camera frames by RANSAC, each hypothesis Horn's 1987 closed form on three correspondences.  The reference tree ships
 * no Sim3Solver: the rules below restate ORB-SLAM2's Sim3Solver.cc [from-knowledge], PARITY UNPINNED, as the PnP section above.
 * The device equals the CPU restatement tests/cpp/sim3_ref.cpp bit for bit.  (The guided matcher ORBmatcher::SearchBySim3 that
 * follows it in ComputeSim3 is the section "loop closing: matching under a similarity" below and reads the row and the similarity
 * written here as they are; Optimizer::OptimizeSim3 behind that is the section "loop closing: Sim3 optimisation".)
 *
 * Rules.
 *  1. Constructor.  For feature i1 of KF1 in ascending i1: a correspondence exists when i2 = d_match[p][i1] >= 0 and the point
 *     mask of KF1's set at i1 and of KF2's set at i2 are set (no mask: every entry is a point).  mvX3Dc1 = Rcw1 * X1w + tcw1 and
 *     mvX3Dc2 = Rcw2 * X2w + tcw2 in f32, each row's products added left to right, then the translation.  mvnMaxError1 = th2 *
 *     sigma2[octave(kp1[i1])], mvnMaxError2 = th2 * sigma2[octave(kp2[i2])] (f32).  mvP1im1 / mvP2im2 = FromCameraToImage of
 *     mvX3Dc1 / mvX3Dc2: invz = 1.0f / z, (fx * (x * invz) + cx, fy * (y * invz) + cy), f32, no sign test on z.  mvnIndices1 =
 *     i1.  N = their number (n_correspondences).
 *  2. SetRansacParameters(probability, minInliers, maxIterations) (LoopClosing passes 0.99, 20, 300): epsilon = (float)minInliers
 *     / N (f32); nIterations = 1 when minInliers == N, else (int)ceil(log(1 - probability) / log(1 - pow(epsilon, 3))) in f64;
 *     mRansacMaxIts = max(1, min(nIterations, maxIterations)).  minInliers is NOT raised with N (PnPsolver raises its own).  N is
 *     known only on the device and the device has no libm that equals the host's, so the host computes the table N ->
 *     mRansacMaxIts for N in [0, capacity] with these expression types (orbx_sim3_ransac_table) and uploads it.
 *  3. Sampling.  d_draws int32 [n_problems][n_iter][3] holds the values rand() returned; the three draws of a hypothesis go
 *     through PnP's rule 3 (RandomInt on the available list, swap-and-pop), the same code on three draws.  A negative draw skips
 *     the hypothesis (it counts no inlier and is never kept) and sets ORBX_SIM3_BAD_DRAWS.
 *  4. ComputeSim3 (Horn 1987) on the triple's mvX3Dc1 (P1) and mvX3Dc2 (P2): the centroids O1, O2 and the relative coordinates
 *     Pr1, Pr2; M = Pr2 * Pr1^T; the symmetric traceless 4x4 N with N11 = M00+M11+M22, N12 = M12-M21, N13 = M20-M02, N14 =
 *     M01-M10, N22 = M00-M11-M22, N23 = M01+M10, N24 = M20+M02, N33 = -M00+M11-M22, N34 = M12+M21, N44 = -M00-M11+M22; the
 *     quaternion (w, x, y, z) = the eigenvector of N's largest signed eigenvalue, and R12 from it; P3 = R12 * Pr2; s12 =
 *     dot(Pr1, P3) / sum(P3 .* P3), or 1 with fix_scale; t12 = O1 - s12 * R12 * O2.  T12 = [s12 R12 | t12], T21 = [(1 / s12)
 *     R12^T | -(1 / s12) R12^T t12].
 *  5. CheckInliers, f32: vP2im1 = mvX3Dc2 through T12 and K, vP1im2 = mvX3Dc1 through T21 and K (each row's products added left
 *     to right, then the translation; the projection of rule 1); err1 = |mvP1im1 - vP2im1|^2, err2 = |vP1im2 - mvP2im2|^2 (dx *
 *     dx + dy * dy); a correspondence is an inlier when err1 < mvnMaxError1 && err2 < mvnMaxError2, both strict.  A hypothesis
 *     with a non-finite entry in s12, R12, t12, T12 or T21 counts no inlier (n_degenerate) and is never kept.
 *  6. iterate.  N < minInliers is bNoMore at once (ORBX_SIM3_FEW_POINTS).  Otherwise, in iteration order with mnBestInliers = 0
 *     at the start, a hypothesis becomes the best when its inliers >= mnBestInliers -- non-strict: of equals the LAST wins,
 *     unlike PnPsolver -- and a hypothesis that becomes the best with inliers > minInliers (strict) ends the solver and is the
 *     result (found_it).  Otherwise all min(n_iter, mRansacMaxIts) iterations run and there is no result
 *     (ORBX_SIM3_NO_RESULT).  There is no Refine.
 *
 * Documented deviations:
 *  1. Horn's algebra (rule 4) runs in f64 from the f32 camera-frame points, where the reference keeps f32 cv::Mat: centroids
 *     p0 + ((p1 - p0) + (p2 - p0)) / 3.0 (three coincident points then give Pr = 0 and s12 = 0 / 0 exactly); M[i][j] summed over the triple's points in the order drawn; nom and den summed over the
 *     coordinate (outer) and the point (inner).  s12, R12 and t12 are then rounded to f32 -- these are the values returned --
 *     and rule 5's matrices are made from the rounded values: s12 * R12 an f32 product; (1.0 / s12) in f64, times R12^T, rounded
 *     to f32; t21 = -(row . t12) in f32.
 *  2. cv::eigen is a cyclic two-sided Jacobi on the symmetric 4x4 with 12 fixed sweeps over (0,1) (0,2) (0,3) (1,2) (1,3)
 *     (2,3) and no convergence test (as PnP's deviation 1); the eigenvector is the column of the largest SIGNED eigenvalue, of
 *     equal values the lowest column.  (N is indefinite: for degenerate triples |lambda_min| can exceed lambda_max, which is why
 *     the one-sided routine of orbx_svd4.inc, ordered by singular value, is not used.)
 *  3. R12 comes from the normalised quaternion directly; the reference's atan2 + Rodrigues round trip gives the same rotation
 *     but divides 0 / 0 for the identity.
 *  4. Map points are arrays plus a mask, indexed by their keyframe's feature.
 *  5. iterate is resolved after the fact: all hypotheses are computed, then rule 6 is applied in iteration order; the answer
 *     equals the sequential loop's (tests/cpp/sim3_ref.cpp holds both; DESIGN.md 4n has the argument).
 *  6. One call is a solver's whole life, as PnP's deviation 6: found_it tells which iterate(5) turn would have returned it.
 *  7. Garbage is flagged and never followed: a keyframe count outside [0, capacity], a match index >= KF2's count, an octave
 *     outside the table on either feature of a correspondence (ORBX_SIM3_BAD_INPUT); a non-finite pose, or a non-finite point
 *     or keypoint of a correspondence (ORBX_SIM3_NONFINITE).  A problem that ends without a result (these,
 *     ORBX_SIM3_FEW_POINTS, or no hypothesis above minInliers) carries ORBX_SIM3_NO_RESULT, zeros for s12, R12, t12 and d_sim3,
 *     and an all -1 row. */
#define ORBX_SIM3_BAD_INPUT 2   /* a count outside [0, capacity], a match index >= KF2's count, an octave outside [0, nlevels) */
#define ORBX_SIM3_NONFINITE 4   /* a non-finite pose, point or keypoint */
#define ORBX_SIM3_FEW_POINTS 8  /* N < minInliers: bNoMore at once */
#define ORBX_SIM3_BAD_DRAWS 16  /* a negative draw among the iterations that ran */
#define ORBX_SIM3_NO_RESULT 32  /* no similarity is returned */
typedef struct orbx_sim3_result {
  int32_t status;            /* 0, or a bitmask of ORBX_SIM3_*; every field is written for every problem */
  int32_t n_correspondences; /* N (0 with BAD_INPUT / NONFINITE) */
  int32_t max_its;           /* mRansacMaxIts of N */
  int32_t its_run;           /* found_it + 1, or min(n_iter, max_its); 0 when nothing ran */
  int32_t found_it;          /* the iteration that ended the solver, or -1 */
  int32_t best_it;           /* the iteration of the best hypothesis when the solver stopped, or -1 */
  int32_t n_inliers;         /* of the returned similarity (0 without one) */
  int32_t n_best_inliers;    /* mnBestInliers when the solver stopped */
  int32_t n_degenerate;      /* non-finite hypotheses among the iterations that ran */
  int32_t reserved[2];
  float s12, R12[9], t12[3]; /* the returned similarity (R12 row-major), zeros without one */
} orbx_sim3_result;

/* The table of rule 2: out int32 [n_max + 1] = mRansacMaxIts for N = 0 .. n_max.  Host only.  For N < min_inliers the design
 * takes the logarithm of a negative number (and divides by N = 0): those entries get max_iterations; such a solver is bNoMore
 * before it iterates.  ORBX_E_BADARG for the parameter ranges below, n_max < 0 or NULL. */
int orbx_sim3_ransac_table(double probability, int min_inliers, int max_iterations, int n_max, int32_t* out);

/* Batched, device-resident, stream-ordered on the context stream.  Problem p: KF1 = h_kf1[p] (the current keyframe), KF2 =
 * h_kf2[p] (the candidate), their point sets h_set1[p] and h_set2[p] (d_points float [n_point_sets][capacity][3], d_point_mask
 * uint8 [n_point_sets][capacity] or NULL, each indexed by its own keyframe's feature); a keyframe or a set may be in any number
 * of problems, on either side.  d_kps_un / d_n: the frames as the extract and undistort calls leave them.  d_match int32
 * [n_problems][capacity]: the feature of KF2 matched to feature i1 of KF1, or -1 (orbx_match_bow_batch_device's d_matches_f
 * with KF1 on the frame side).  d_pose float [n_frames][12]: Tcw per frame, R row-major, then t.  K row-major 3x3 (host, f32);
 * sigma2: host, the context's nlevels floats, NULL = the context's own; fix_scale: 0 (monocular) or 1; probability in (0, 1),
 * min_inliers >= 3, max_iterations >= 1, th2 > 0 (ORB-SLAM2's 9.210); d_draws int32 [n_problems][n_iter][3], n_iter >= 1.
 * Outputs: d_res [n_problems]; d_sim3 float [n_problems][13]: R12 row-major, t12, s12; d_match_inliers int32
 * [n_problems][capacity]: d_match[p][i1] where i1 is an inlier of the result and -1 elsewhere (every entry is written), the row
 * LoopClosing builds from vbInliers; d_inliers uint8 [n_problems][capacity] (NULL = not wanted).  Three launches: k_sim3_prep (a
 * wave per problem), k_sim3_hypotheses (a lane per problem and iteration), k_sim3_resolve (a wave per problem).  The call
 * returns once queued, with the PnP call's exception: when the lists, sigma2 or the parameters' table differ from the previous
 * call's on this context, or the workspace grows, it first waits for the context stream.  The workspace is sized from the
 * capacity, not from the counts, which only the device knows: n_problems * capacity * 60 bytes of correspondence records plus
 * n_problems * n_iter * 64 bytes of hypotheses, kept by the context and grown on demand (38 MB at 640 problems of capacity 1000
 * and 300 iterations; 640 problems at capacity 16384 would take 630 MB: batch sparse keyframes at the capacity they need).
 * ORBX_E_BADARG: null required pointers, negative counts, capacity < 1, n_iter < 1, a parameter outside its range, fix_scale
 * not 0 or 1, a keyframe index outside [0, n_frames), a point set outside [0, n_point_sets); ORBX_E_CAPACITY: capacity >
 * ORBX_BOW_MAX_FEATURES, or n_problems * n_iter > 2^31 - 64 (a lane per hypothesis); ORBX_E_HIP: ctx == NULL with otherwise
 * well-formed arguments -- all checked before anything touches a device.  n_problems == 0 is ORBX_OK. */
int orbx_sim3_solve_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_kf1, const int32_t* h_kf2,
                                 const int32_t* h_set1, const int32_t* h_set2, const orbx_keypoint* d_kps_un, const int32_t* d_n,
                                 int capacity, const int32_t* d_match, int n_point_sets, const float* d_points,
                                 const uint8_t* d_point_mask, const float* d_pose, const float* K, const float* sigma2, int fix_scale,
                                 double probability, int min_inliers, int max_iterations, float th2, int n_iter,
                                 const int32_t* d_draws, orbx_sim3_result* d_res, float* d_sim3, int32_t* d_match_inliers,
                                 uint8_t* d_inliers);
/* The same for one problem in host memory: KF1 (n1 features, points1 [n1][3], mask1 [n1] nullable, pose1 [12]), then KF2;
 * match12 [n1]; draws [n_iter][3]; sim3 [13]; match_inliers [n1]; inliers [n1] nullable.  mask1 and mask2 are given together
 * or not at all.  Run through the batched path as a batch of one.  Synchronous. */
int orbx_sim3_solve(orbx_ctx* ctx, const orbx_keypoint* kps_un1, int n1, const float* points1, const uint8_t* mask1,
                    const float* pose1, const orbx_keypoint* kps_un2, int n2, const float* points2, const uint8_t* mask2,
                    const float* pose2, const int32_t* match12, const float* K, const float* sigma2, int fix_scale,
                    double probability, int min_inliers, int max_iterations, float th2, int n_iter, const int32_t* draws,
                    orbx_sim3_result* res, float* sim3, int32_t* match_inliers, uint8_t* inliers);

/* ---- loop closing: Sim3 optimisation (Optimizer::OptimizeSim3, the call that decides whether a candidate closes the loop) -------
 * Behind Sim3Solver and SearchBySim3, LoopClosing::ComputeSim3 refines the similarity over the widened match row and counts the
 * correspondences that survive: `nInliers = Optimizer::OptimizeSim3(mpCurrentKF, pKF, vpMapPointMatches, gScm, 10, mbFixScale)`,
 * accepted when nInliers >= 20.  The reference vendors the g2o types (types/sim3.h, types/types_seven_dof_expmap.h), the
 * Levenberg solver and LinearSolverDense, but has no Optimizer: the rules below restate ORB-SLAM2's Optimizer::OptimizeSim3
 * [from-knowledge], PARITY UNPINNED, as the pose section above.  The device equals the CPU restatement
 * tests/cpp/sim3opt_ref.cpp bit for bit.
 *
 * Graph.  One VertexSim3Expmap with _fix_scale = fix_scale; its start is Sim3(Matrix3d R12, Vector3d t12, double s12) of the f32
 * d_sim3 row (R12 row-major, t12, s12): Quaterniond(R) by Eigen's four-branch rule, with no sign flip and no normalisation
 * (types/sim3.h:64-67 does neither, unlike SE3Quat).  Both cameras' fx fy cx cy come from K.  A correspondence exists for feature
 * i1 of KF1, ascending, when i2 = row[i1] >= 0, i2 < KF2's count, and the point mask of KF1's set at i1 and of KF2's set at i2
 * are set.  Its two fixed points are the camera-frame points of the Sim3 RANSAC section's rule 1 (Rcw * Xw + tcw in f32, each
 * row's products added left to right, then the translation), taken to f64 afterwards: P1c of KF1's point, P2c of KF2's.  Two
 * edges per correspondence, e12 before e21 wherever order matters:
 *   e12  EdgeSim3ProjectXYZ (types_seven_dof_expmap.h:130-149): error = obs1 - cam_map1(project(S12.map(P2c))), obs1 =
 *        kp1[i1].pt, information = inv_sigma2[octave(kp1[i1])] * I
 *   e21  EdgeInverseSim3ProjectXYZ (:152-171): error = obs2 - cam_map2(project(S12.inverse().map(P1c))), obs2 = kp2[i2].pt,
 *        information = inv_sigma2[octave(kp2[i2])] * I; inverse() is sim3.h:233-236
 * both with a RobustKernelHuber of delta = (float)sqrt(th2) (`const float deltaHuber = sqrt(th2)`).  map is s * (r * xyz) + t
 * (sim3.h:144-146), project is (x / z, y / z), cam_map is (v0 * fx + cx, v1 * fy + cy) (:74-88).
 *
 * Jacobians are numeric: both edges have linearizeOplus commented out (:147, :169), so BaseBinaryEdge::linearizeOplus
 * (core/base_binary_edge.hpp:131-200) runs.  The point vertex is fixed, so only the seven columns of the Sim3 vertex exist.
 * Column d = (1.0 / (2 * 1e-9)) * (error(oplus(+1e-9 e_d)) - error(oplus(-1e-9 e_d))), the subtraction first (:181-196).  oplus
 * is Sim3(update) * estimate (types_seven_dof_expmap.h:60-69, sim3.h:266-272): the quaternion product is not normalised, and
 * update[6] is forced to 0 under fix_scale, so column 6 is exactly zero there.  Sim3(const Vector7d&) is sim3.h:70-142 with all
 * four branches on fabs(sigma) < 1e-5 and theta < 1e-5; the small-theta R = I + Omega + Omega * Omega is kept, without the 1/2,
 * and Quaterniond(R) is taken of that matrix as it stands.  sin / cos are those of the bundle adjustment above; exp(sigma) is a
 * restated fdlibm e_exp.c on [-700, 700] (NaN outside): reduction by ln2 in two parts, the polynomial, an exact scaling by 2^k.
 *
 * Optimisation.  initializeOptimization(); optimize(n_iterations) (the design passes 5): the loop of the pose section's rule c,
 * steps 1 to 7, on the 7-dof vertex: computeLambdaInit over seven diagonal entries, computeScale over seven terms.
 * First classification.  For every correspondence `e12->chi2() > th2 || e21->chi2() > th2` removes it: chi2 = e . (information
 * e), unrobustified, f64, against the f32 th2 promoted to f64.  Its row entry becomes -1, both edges leave the graph, nBad counts
 * them.  The stale-error rule of the pose section applies as it stands: an edge's _error is that of the round's last
 * computeActiveErrors, i.e. of the last TRIAL, accepted or not (linearizeOplus restores _error at :200).
 * Second round.  nMoreIterations = nBad > 0 ? 10 : 5.  `if (nCorrespondences - nBad < 10) return 0`: the similarity is NOT
 * recovered (the output equals the input), the row keeps the first classification's removals, n_inliers is 0.  Otherwise
 * initializeOptimization(); optimize(nMoreIterations): it continues FROM THE CURRENT ESTIMATE (no reset, unlike
 * PoseOptimization), the robust kernel is still on, lambda, _ni and _nBad start again at iteration 0.  Then the second
 * classification by the same test: a failing entry becomes -1, the rest count in nIn, the return value.  The result is the
 * vertex' estimate: q, t, s in f64; s12, R12, t12 in f32, R12 = toRotationMatrix of the quaternion as it is.
 *
 * Documented deviations:
 *  1. Sums: the pose section's deviation 1 (feature i1 belongs to lane i1 % 64; the 64 lanes folded + 32, + 16, ... + 1), with a
 *     correspondence's e12 term added before its e21 term.  g2o adds edge by edge, all e12 / e21 pairs in insertion order.
 *  2. The small dense algebra, sin / cos / exp and the 7x7 solve through the shared csrc/orbx_sim3opt_math.inc.  The solve is the
 *     project's unblocked lower Cholesky where g2o's LinearSolverDense is an Eigen::LDLT; a pivot <= 0 or non-finite, or a
 *     non-finite solution, is a failed solve and applies a zero step.  The fourteen perturbed estimates of a linearisation and
 *     their inverses are computed once per linearisation, not once per edge: they depend on the estimate alone, and the bits
 *     are those g2o computes per edge (tests/test_sim3opt_host.py compares both forms).
 *  3. Arrays plus masks stand for KeyFrame / MapPoint; GetIndexInKeyFrame is the row.
 *  4. Garbage is flagged and never followed.  ORBX_SIM3OPT_BAD_INPUT: a count outside [0, capacity], a row entry >= KF2's count,
 *     an octave outside the table on a feature of a correspondence.  ORBX_SIM3OPT_NONFINITE: a non-finite pose, similarity,
 *     point, keypoint or result, or s12 <= 0.  Such a problem returns its inputs: the row untouched, d_sim3 copied through,
 *     every other number of the result 0.
 *  5. n_iterations is two arguments (5 and 10): n_more_iterations is the count behind nBad > 0; behind nBad == 0 the second
 *     round runs the first round's n_iterations.  0 is accepted and only classifies, at the estimate it was given.
 *  6. n_correspondences == 0 runs nothing: rounds = 0, n_inliers = 0, the similarity copied through. */
#define ORBX_SIM3OPT_BAD_INPUT 2 /* a count outside [0, capacity], a row entry >= KF2's count, an octave outside [0, nlevels) */
#define ORBX_SIM3OPT_NONFINITE 4 /* a non-finite pose, similarity, point, keypoint or result, or s12 <= 0 */
typedef struct orbx_sim3opt_result {
  int32_t status;            /* 0, or a bitmask of ORBX_SIM3OPT_*; every field is written for every problem */
  int32_t n_correspondences; /* nCorrespondences (0 with a status) */
  int32_t n_bad;             /* removed by the first classification */
  int32_t n_inliers;         /* nIn, the design's return value: 0 when the second round did not run */
  int32_t rounds;            /* 2; 1 when nCorrespondences - nBad < 10; 0 when nothing ran */
  int32_t iterations[2];     /* solve() calls of each round */
  int32_t lm_trials;         /* over both rounds: the sum of qmax */
  int32_t rejected_trials;
  int32_t solver_failures;
  int32_t stop_reason[2];    /* per round: 0 = all iterations ran, 1 = qmax == 10 || rho == 0, 2 = _nBad >= 3 */
  int32_t small_theta;       /* LM steps (lm_trials - solver_failures of them ran) whose Sim3(update) had theta < 1e-5, */
  int32_t small_sigma;       /* ... |sigma| < 1e-5 (every step under fix_scale), */
  int32_t small_both;        /* ... both: with the two above, how often each of the four branches ran */
  int32_t reserved;
  double chi2_initial;       /* activeRobustChi2 at the given similarity */
  double chi2_final, lambda; /* of the last round that ran an iteration */
  double q[4], t[3], s;      /* the estimate as g2o holds it (quaternion x, y, z, w); the start estimate when rounds == 1 */
  float s12, R12[9], t12[3]; /* as Converter::toCvMat would store it (row-major); d_sim3's bits when nothing was recovered */
  float reserved_f;
} orbx_sim3opt_result;

/* Batched, device-resident, stream-ordered on the context stream.  The problem lists, d_kps_un, d_n, d_points, d_point_mask and
 * d_pose mean what they mean in orbx_sim3_solve_batch_device.  d_matches int32 [n_problems][capacity], in and out: vpMatches1 as
 * orbx_match_sim3_batch_device leaves it; a removed entry becomes -1, every other entry stays.  d_sim3 float [n_problems][13]:
 * R12 row-major, t12, s12, as the solver writes it.  K row-major 3x3 (host, f32); inv_sigma2: host, the context's nlevels floats,
 * NULL = the context's own table; fix_scale 0 or 1; th2 > 0 (the design passes 10); n_iterations, n_more_iterations >= 0 (5,
 * 10).  Outputs: d_res [n_problems]; d_sim3_out float [n_problems][13], which may equal d_sim3.  One wave of 64 lanes runs a
 * problem's whole optimisation, four problems per workgroup, in one launch, without a workspace.  The call returns once queued,
 * with the pose call's exception: when the lists or the table differ from the previous call's on this context, it first waits
 * for the context stream.  ORBX_E_BADARG: null required pointers, negative counts, capacity < 1, fix_scale not 0 or 1, th2 not a
 * finite number > 0, a keyframe index outside [0, n_frames), a point set outside [0, n_point_sets); ORBX_E_CAPACITY: capacity >
 * ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with otherwise well-formed arguments -- all checked before anything touches a
 * device.  n_problems == 0 is ORBX_OK. */
int orbx_optimize_sim3_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_kf1, const int32_t* h_kf2,
                                    const int32_t* h_set1, const int32_t* h_set2, const orbx_keypoint* d_kps_un, const int32_t* d_n,
                                    int capacity, int32_t* d_matches, int n_point_sets, const float* d_points,
                                    const uint8_t* d_point_mask, const float* d_pose, const float* d_sim3, const float* K,
                                    const float* inv_sigma2, int fix_scale, float th2, int n_iterations, int n_more_iterations,
                                    orbx_sim3opt_result* d_res, float* d_sim3_out);
/* The same for one pair in host memory: KF1 (n1 features, points1 [n1][3], mask1 [n1] nullable, pose1 [12]), then KF2; matches12
 * [n1] in and out; sim3 [13] in; sim3_out [13] (may equal sim3).  mask1 and mask2 are given together or not at all.  Run through
 * the batched path as a batch of one.  Synchronous. */
int orbx_optimize_sim3(orbx_ctx* ctx, const orbx_keypoint* kps_un1, int n1, const float* points1, const uint8_t* mask1,
                       const float* pose1, const orbx_keypoint* kps_un2, int n2, const float* points2, const uint8_t* mask2,
                       const float* pose2, int32_t* matches12, const float* sim3, const float* K, const float* inv_sigma2,
                       int fix_scale, float th2, int n_iterations, int n_more_iterations, orbx_sim3opt_result* res, float* sim3_out);

/* ---- loop closing: matching the loop's points under Scw (ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)) ------
 * The tail of LoopClosing::ComputeSim3: once OptimizeSim3 accepts a candidate (nInliers >= 20) it composes mScw = Scm * Smw,
 * projects the map points of the loop keyframe and its covisible neighbours (mvpLoopMapPoints) into the current keyframe with th =
 * 10, and accepts the loop when nTotalMatches >= 40; the row it leaves is mvpCurrentMatchedPoints, which CorrectLoop starts from.
 * The reference ships no such function: this is ORB-SLAM2's code, [from-knowledge], PARITY UNPINNED, bit-identical to a CPU
 * restatement of the rules below (tests/cpp/match_scw_ref.cpp).  The window search alone is pinned: it is the reference's
 * Frame::GetFeaturesInArea (SlamTypes/Frame.cpp:163-206), and the tests compare it with the reference's own compiled code.
 *
 * Pair p: current keyframe C = h_kf[p] (n_C features), map set s = h_map_set[p] (n_s = d_map_n[s] points, the arrays of matching
 * the local map by projection), the similarity d_scw[p] (12 floats: the top three rows of mScw as a CV_32F matrix, sR row-major,
 * then t), the row d_matches[p] (C's feature j -> an index into set s, or a negative value; read and written).  f32 without
 * contraction unless stated.
 *   1. the decomposition: scw = (float)sqrt((double)((sR00*sR00 + sR01*sR01) + sR02*sR02)), the dot product in f32; Rcw = sR /
 *      scw and tcw = t / scw element-wise, correctly rounded; Ow_k = -((Rcw[0][k]*tcw0 + Rcw[1][k]*tcw1) + Rcw[2][k]*tcw2).
 *   2. what C already has (vpMatched[j] != NULL: feature j is taken; the set of those points is spAlreadyFound, and such a point
 *      is not searched).  Without d_kf2_to_map an entry i >= 0 is an index into set s.  With d_kf2_to_map [n_pairs][capacity]
 *      the entry row holds the MATCHED keyframe's feature indices as orbx_optimize_sim3_batch_device leaves them, and the table
 *      maps such a feature to an index in set s, or to a negative value: each entry i2 >= 0 is translated through the table and
 *      the translated value is written back.  An entry that translates to a negative value becomes ORBX_SCW_TAKEN_UNMAPPED: the
 *      feature stays taken, no point is marked found, and the entry counts in n_unmapped; an entry that holds
 *      ORBX_SCW_TAKEN_UNMAPPED on entry is treated, and counted, likewise.  Any other negative entry is free.  An entry >= n_s,
 *      with the table an entry i2 >= capacity, and a translated value >= n_s are never followed: the entry stays as it is, its
 *      feature counts as taken and ORBX_SCW_BAD_INPUT is set.  There is no outlier input.
 *   3. the points searched: points i of the set in ascending order whose mask byte is set and that are not found.  Pc = Rcw*P +
 *      tcw as xc = ((R0*X + R1*Y) + R2*Z) + t0, yc and zc likewise.  zc < 0.0f: skipped (n_behind); zc == 0 goes on and fails the
 *      image test.  invz = 1.0f / zc correctly rounded; u = fx*(xc*invz) + cx, v = fy*(yc*invz) + cy.  KeyFrame::IsInImage: the
 *      point stays iff u >= min_x && u < max_x && v >= min_y && v < max_y -- half-open above; a value that is no number fails.
 *   4. PO = P - Ow; dist = (float)sqrt(((double)POx*POx + (double)POy*POy) + (double)POz*POz), the products and sums in f64 in
 *      that order (cv::norm of a CV_32F vector); dist < 0.8f*minDist || dist > 1.2f*maxDist: skipped (d_map_dist holds the raw
 *      mfMinDistance, mfMaxDistance).
 *   5. the viewing angle: with dot = ((double)POx*Nx + (double)POy*Ny) + (double)POz*Nz, products and sums in f64 in that order,
 *      the point is skipped when dot < 0.5 * (double)dist -- a comparison in f64 (PO.dot(Pn) < 0.5*dist).
 *   6. level = PredictScale in table form on ratio = maxDist / dist (correctly rounded): the number of n in [0, nlevels - 1)
 *      with ratio > scale[n].  r = th * scale[level]; the candidates are GetFeaturesInArea(u, v, r) over C's undistorted
 *      keypoints, the reference's function without level bounds (PosInGrid's rounding, the clamped cell range, the strict
 *      fabs(d) < r in both coordinates), in the order cell x outer, cell y inner, ascending index inside a cell; of them only
 *      those with octave in [level - 1, level] stay.  None stays: the point is skipped (n_with_candidates counts the others).
 *   7. over the candidates that are not taken, neither on entry nor by an earlier point of this call, in that order, with d =
 *      popcount(d_map_desc32[s][i] ^ desc_C[j]): the first smallest wins (dist < bestDist, starting from 256).  bestDist <=
 *      th_low: d_matches[p][bestIdx] = i, bestIdx is taken and nmatches counts it.  No ratio test, no orientation histogram.
 *   8. n_total = the entries of the row that are not free on exit: the entry's matches, unmapped and unfollowed ones included,
 *      plus the new ones.  This is ComputeSim3's nTotalMatches (a loop needs >= 40).
 * Documented deviations from ORB-SLAM2:
 *   1. PredictScale in table form (deviation 1 of matching the local map by projection).
 *   2. Map points are arrays plus a mask (0 = NULL or isBad()), matches are indices into the pair's map set; a matched point
 *      that is not in the set keeps its feature through ORBX_SCW_TAKEN_UNMAPPED.
 *   3. th_low is an argument (ORBmatcher::TH_LOW is 50), accepted in [0, 256]: 0 accepts only an identical descriptor; 255 and
 *      256 accept every candidate but one at distance 256, which `dist < bestDist` never picks.
 *   4. Garbage is flagged and never followed.  Counts outside [0, capacity] / [0, map_capacity] are clamped and set
 *      ORBX_SCW_BAD_INPUT, as do the entries of rule 2.  A similarity with a non-finite value, scw that is not a finite number > 0
 *      or a quotient of rule 1 that is not finite sets ORBX_SCW_NONFINITE, drops every point of rule 3 and leaves the row as
 *      rule 2 left it; a point of rule 3 whose position, normal or two distances hold a non-finite value sets it and is
 *      dropped, as is one whose ratio is no number.  A keypoint whose cell is no number is in no cell; window cells are clamped
 *      as floats.
 * Worst case: points whose windows all share candidates within th_low resolve one per round (see the kernel). */
#define ORBX_SCW_BAD_INPUT 2        /* a count outside its capacity, an entry of rule 2 that is never followed */
#define ORBX_SCW_NONFINITE 4        /* a similarity rule 1 cannot decompose, a non-finite point / normal / distance or ratio */
#define ORBX_SCW_TAKEN_UNMAPPED (-2) /* d_matches: the feature has a map point that is not in the pair's map set */
typedef struct orbx_scw_result {
  int32_t status;             /* 0, or a bitmask of ORBX_SCW_*; every field is written for every pair */
  int32_t nmatches;           /* new matches (rule 7) */
  int32_t n_total;            /* rule 8: nTotalMatches */
  int32_t n_points;           /* points that reach rule 3: mask set, not found */
  int32_t n_found;            /* points some entry of the row names (whatever their mask) */
  int32_t n_unmapped;         /* entries that are ORBX_SCW_TAKEN_UNMAPPED behind rule 2 */
  int32_t n_behind;           /* rule 3: zc < 0 */
  int32_t n_out_image;        /* ... outside [min, max) or no number */
  int32_t n_out_distance;     /* rule 4 */
  int32_t n_out_angle;        /* rule 5 */
  int32_t n_with_candidates;  /* searched points whose window holds a feature of their octaves (rule 6) */
  int32_t n_over_dist;        /* ... whose bestDist is above th_low (256 when every candidate is taken) */
  int32_t n_displaced;        /* searched points whose pick (the feature, or none) differs from what they would get with only
                                 the entry's matches taken */
  int32_t rounds;             /* the device's rounds of claims; a sequential statement reports 0 */
} orbx_scw_result;

/* Batched, device-resident, stream-ordered on the context stream.  d_kps_un / d_desc32 (16-byte aligned) / d_n: the keyframes, in
 * the layout of the extract and undistort calls ([n_frames][capacity]).  Map set s of [n_map_sets][map_capacity], exactly the
 * arrays of orbx_match_local_map_batch_device: d_map_n int32 [n_map_sets], d_map_points float [3], d_map_normals float [3],
 * d_map_dist float [2], d_map_desc32 uint8 [32] (16-byte aligned), d_map_mask uint8 (NULL = every entry is a point); several
 * pairs may share a keyframe or a map set.  d_scw float [n_pairs][12], as orbx_sim3_compose_scw_batch_device writes it.  K
 * row-major 3x3 (host, f32), bounds = the keyframes' image bounds, th > 0 (ComputeSim3 passes 10), th_low in [0, 256] (TH_LOW =
 * 50).  d_matches int32 [n_pairs][capacity], in and out and required; entries at and beyond C's count are not touched.
 * d_kf2_to_map int32 [n_pairs][capacity] or NULL (rule 2).  d_res [n_pairs].
 * One workgroup per pair, one launch.  The call returns once queued, with the exception orbx_match_bow_batch_device has: when the
 * pair lists differ from the previous call's on this context, the call first waits for the context stream before it uploads
 * them.
 * ORBX_E_BADARG: null required pointers, negative counts, capacity or map_capacity < 1, th not finite or <= 0, th_low outside
 * [0, 256], bounds with max <= min, a keyframe outside [0, n_frames), a map set outside [0, n_map_sets) -- all checked before
 * anything touches a device; ORBX_E_CAPACITY: capacity or map_capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with
 * otherwise well-formed arguments.  n_pairs == 0 is ORBX_OK. */
int orbx_match_scw_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_map_set,
                                const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                                int n_map_sets, int map_capacity, const int32_t* d_map_n, const float* d_map_points,
                                const float* d_map_normals, const float* d_map_dist, const uint8_t* d_map_desc32,
                                const uint8_t* d_map_mask, const float* d_scw, const float* K, const orbx_bounds* bounds, float th,
                                int th_low, int32_t* d_matches, const int32_t* d_kf2_to_map, orbx_scw_result* d_res);
/* The same for one pair in host memory, through the batched path as a batch of one: the keyframe (n features), the map (map_n
 * points; map_mask nullable), scw [12]; matches [n] in and out; kf2_to_map [n_table] nullable (an entry >= n_table is an entry
 * beyond the table: never followed).  More than ORBX_BOW_MAX_FEATURES features, points or table entries: ORBX_E_CAPACITY.
 * Synchronous. */
int orbx_match_scw(orbx_ctx* ctx, const orbx_keypoint* kps_un, const uint8_t* desc32, int n, int map_n, const float* map_points,
                   const float* map_normals, const float* map_dist, const uint8_t* map_desc32, const uint8_t* map_mask,
                   const float* scw, const float* K, const orbx_bounds* bounds, float th, int th_low, int32_t* matches,
                   const int32_t* kf2_to_map, int n_table, orbx_scw_result* res);

/* The similarity in front of it: d_scw[p] = S12 * Tmw from d_sim3[p] (13 floats: R12 row-major, t12, s12; keyframe 1 is the
 * current one, as orbx_optimize_sim3_batch_device writes it) and the matched keyframe's pose d_pose[h_kf2[p]] (12 floats: Rmw
 * row-major, then tmw).  In f64 from the f32 inputs: R = R12 * Rmw, each element (a + b) + c; q = R12 * tmw likewise; t = s12*q +
 * t12; the output is (float)(s12 * R) row-major followed by (float)t.
 * Documented deviation: g2o multiplies two Sim3 through unit quaternions and Converter::toCvMat converts back.  Here the matrices
 * are multiplied directly, which differs from g2o's result only by rounding and needs no quaternion normalisation on either side.
 * A non-finite input or s12 that is not > 0 writes twelve zeros, which the matcher flags as ORBX_SCW_NONFINITE.
 * A lane per pair, one launch; stream-ordered, with the list exception above.  ORBX_E_BADARG: null required pointers, negative
 * counts, a keyframe outside [0, n_frames); ORBX_E_HIP: ctx == NULL otherwise.  n_pairs == 0 is ORBX_OK. */
int orbx_sim3_compose_scw_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf2, const float* d_pose,
                                       const float* d_sim3, float* d_scw);
/* The same for one pair in host memory: pose2 [12], sim3 [13] -> scw [12].  Synchronous. */
int orbx_sim3_compose_scw(orbx_ctx* ctx, const float* pose2, const float* sim3, float* scw);

/* ---- fusing map points into a keyframe (ORBmatcher::Fuse, both overloads) ----------------------------------------------------
 * LocalMapping::SearchInNeighbors runs Fuse(pKF, vpMapPoints, th = 3) behind CreateNewMapPoints, the new keyframe's points into
 * every neighbour and the neighbours' points into the new keyframe; LoopClosing::SearchAndFuse runs Fuse(pKF, Scw, vpPoints, th
 * = 4, vpReplacePoint) over the map set the Scw matcher above has read.  The reference ships no Fuse: the rules are ORB-SLAM2's,
 * [from-knowledge], PARITY UNPINNED, bit-identical to a CPU restatement (tests/cpp/fuse_ref.cpp).  The window search alone is
 * pinned: the reference's Frame::GetFeaturesInArea, compared with its compiled code by the tests.
 *
 * Pair p: keyframe h_kf[p] (n_C features), map set s = h_map_set[p] (n_s points), d_pose[p] or d_scw[p] (12 floats), the row
 * d_matches[p] (mvpMapPoints: feature j -> an index into set s, ORBX_FUSE_OCCUPIED_UNMAPPED for a point that is not in the set,
 * any other negative value: free; read and written).  f32 without contraction unless stated.
 * Search, pose form, for every point i in ascending order:
 *   1. the entry: a row entry e with 0 <= e < n_s names point e, which is IsInKeyFrame and not searched, whatever its mask
 *      (n_in_kf counts the points named).  An entry >= n_s is never followed: ORBX_FUSE_BAD_INPUT, and its feature holds a bad
 *      point.  The points searched are those with their mask byte set (d_map_mask NULL: all) that the row does not name
 *      (n_points).
 *   2. Pc = Rcw*P + tcw as xc = ((R0*X + R1*Y) + R2*Z) + t0, yc and zc likewise.  zc < 0.0f: skipped (n_behind); zc == 0 goes on
 *      and fails the image test.  invz = 1.0f / zc correctly rounded; u = fx*(xc*invz) + cx, v = fy*(yc*invz) + cy.
 *      KeyFrame::IsInImage: the point stays iff u >= min_x && u < max_x && v >= min_y && v < max_y; no number fails
 *      (n_out_image).
 *   3. Ow_k = -((R[0][k]*t0 + R[1][k]*t1) + R[2][k]*t2); PO = P - Ow; dist, its two bounds (n_out_distance) and the viewing angle
 *      (n_out_angle) are rules 4 and 5 of "loop closing: matching the loop's points under Scw", verbatim.
 *   4. level = PredictScale in table form on ratio = maxDist / dist: the number of n in [0, nlevels - 1) with ratio > scale[n].
 *      r = th * scale[level]; the candidates are GetFeaturesInArea(u, v, r) without level bounds, in the grid's order (cell x
 *      outer, cell y inner, ascending index inside a cell); n_with_candidates counts the points with at least one.  A
 *      candidate whose octave is outside [level - 1, level] is dropped.
 *   5. the chi-square gate (this form only): ex = u - kp.x, ey = v - kp.y, e2 = ex*ex + ey*ey; the candidate is dropped when
 *      (double)(e2 * invLevelSigma2[octave]) > 5.99, the product in f32; invLevelSigma2 is the context's table.  An octave < 0
 *      is outside the table: dropped.
 *   6. d = popcount(d_map_desc32[s][i] ^ desc_C[j]); bestDist starts at 256 and `d < bestDist` takes the candidate: the first
 *      smallest in the order wins.  The pick stands when bestDist <= th_low; a point with candidates whose pick does not stand
 *      counts in n_over_dist.  A point's pick depends on nothing another point does: there is no "taken" rule.
 * Search, Scw form: rule 1 of the Scw matcher decomposes d_scw[p] (scw from the first row, twelve divisions, Ow = -Rcw^T tcw);
 * rules 1 to 4 above; no chi-square gate; bestDist starts at INT_MAX, so with th_low = 256 a candidate at distance 256 fuses
 * here and never in the pose form.
 * Resolution, per feature f over the points that picked it, in ascending i (each counts in n_fused); obs_i = d_map_obs[s][i]:
 *   R1. f is free: ORBX_FUSE_ADD, row[f] = i, d_fuse_other[i] = -1; the modelled count of f's occupant becomes obs_i + 1.
 *   R2. the occupant is bad (a set entry with mask 0; ORBX_FUSE_OCCUPIED_UNMAPPED with d_occ_obs[f] < 0; an entry >= n_s):
 *       ORBX_FUSE_BAD_OCCUPANT, nothing changes, also for later points; d_fuse_other[i] is the entry.
 *   R3. pose form, a good occupant with count c (d_map_obs of the entry, d_occ_obs[f] of an unmapped one, or the modelled count
 *       when this call has decided on f before): c > obs_i gives ORBX_FUSE_KEEP_OCCUPANT (pMP->Replace(pMPinKF)); otherwise,
 *       equality included, ORBX_FUSE_REPLACE_OCCUPANT (pMPinKF->Replace(pMP)) and row[f] = i; either way c becomes c + obs_i.
 *       d_fuse_other[i] is the occupant met.
 *   R4. Scw form, a good occupant: ORBX_FUSE_KEEP_OCCUPANT and d_fuse_other[i] = vpReplacePoint[i], the occupant; the row
 *       changes only by ORBX_FUSE_ADD, and a later point on a feature an earlier one was added to gets that earlier point.
 *   n_chained counts the decisions that are not the first on their feature and do not meet a bad occupant: those read a count
 *   (or an occupant) this call has changed.
 * Documented deviations from ORB-SLAM2:
 *   1. PredictScale in table form (deviation 1 of matching the local map by projection).
 *   2. Map points are arrays plus a mask (0 = NULL or isBad()), with indices; the points of one set are distinct.
 *   3. No stereo branch.
 *   4. The count model of R1 / R3.  ORB-SLAM2's Replace hands over only the observations in keyframes that do not already see
 *      the survivor; the sum is that number when the two points share no keyframe.  A modelled count is read only where a
 *      feature is picked a second time in one call: n_chained counts exactly those decisions, and d_fuse_idx / d_fuse_act /
 *      d_fuse_other let a caller replay them with the map's own counts.  The Scw form reads no counts and is exact.
 *   5. The pairs of one call are independent.  ORB-SLAM2's loop over neighbours sees the earlier neighbours' fusions: a caller
 *      who needs that issues the neighbours call by call.
 *   6. Replace, AddObservation, ComputeDistinctiveDescriptors and UpdateNormalAndDepth stay the caller's.
 *   7. th_low is an argument (ORBmatcher::TH_LOW is 50), accepted in [0, 256].
 *   8. Garbage is flagged and never followed.  Counts outside [0, capacity] / [0, map_capacity] are clamped and set
 *      ORBX_FUSE_BAD_INPUT, as do a row entry >= n_s and, in the pose form without d_occ_obs, an ORBX_FUSE_OCCUPIED_UNMAPPED
 *      entry (handled as a bad occupant).  The pose form reads obs_i of every point whose pick stands and the count of every
 *      good occupant a first decision meets: a value outside [0, 65535] is clamped into it and sets ORBX_FUSE_BAD_INPUT, so no
 *      sum overflows.  A pose with a non-finite value, a similarity rule 1 of the Scw matcher cannot decompose: ORBX_FUSE_NONFINITE,
 *      every point of rule 1 dropped, the row untouched; a point whose position, normal or two distances hold a non-finite
 *      value sets it and is dropped, as is one whose ratio is no number.
 * Worst case: every point of the set on one feature resolves one point per round (see the kernel). */
#define ORBX_FUSE_BAD_INPUT 2 /* a count outside its range, a row entry that is never followed */
#define ORBX_FUSE_NONFINITE 4 /* a pose or similarity that cannot be used, a non-finite point / normal / distance or ratio */
#define ORBX_FUSE_OCCUPIED_UNMAPPED (-2) /* d_matches: the feature has a map point that is not in the pair's map set */
#define ORBX_FUSE_NONE 0
#define ORBX_FUSE_ADD 1
#define ORBX_FUSE_KEEP_OCCUPANT 2
#define ORBX_FUSE_REPLACE_OCCUPANT 3
#define ORBX_FUSE_BAD_OCCUPANT 4
typedef struct orbx_fuse_result {
  int32_t status;              /* 0, or a bitmask of ORBX_FUSE_*; every field is written for every pair */
  int32_t n_fused;             /* nFused, the design's return value: the points whose pick stands */
  int32_t n_points;            /* points that reach rule 2: mask set, not in the keyframe */
  int32_t n_in_kf;             /* points some entry of the row names (whatever their mask) */
  int32_t n_behind;            /* rule 2: zc < 0 */
  int32_t n_out_image;         /* ... outside [min, max) or no number */
  int32_t n_out_distance;      /* rule 3 */
  int32_t n_out_angle;         /* rule 3 */
  int32_t n_with_candidates;   /* searched points whose window holds a feature (rule 4) */
  int32_t n_over_dist;         /* ... whose pick does not stand (rules 4 to 6) */
  int32_t n_added;             /* R1 */
  int32_t n_kept_occupant;     /* R3 / R4 */
  int32_t n_replaced_occupant; /* R3 */
  int32_t n_bad_occupant;      /* R2 */
  int32_t n_chained;           /* decisions behind an earlier one on the same feature (deviation 4) */
  int32_t rounds;              /* the device's rounds: the longest list of points on one feature; a sequential statement: 0 */
} orbx_fuse_result;

/* Batched, device-resident, stream-ordered on the context stream.  The keyframes and the map sets are exactly the arrays of
 * orbx_match_scw_batch_device, with the same sharing: several pairs may name one keyframe or one set.  d_map_obs int32
 * [n_map_sets][map_capacity]: Observations() of each point (required).  d_pose float [n_pairs][12]: Rcw row-major, then tcw.  K
 * row-major 3x3 (host, f32), bounds = the keyframes' image bounds, th finite and > 0 (SearchInNeighbors passes 3), th_low in [0,
 * 256].  d_matches int32 [n_pairs][capacity], in and out and required; entries at and beyond the keyframe's count are not
 * touched.  d_occ_obs int32 [n_pairs][capacity] or NULL: for an ORBX_FUSE_OCCUPIED_UNMAPPED entry the occupant's
 * Observations(), negative when that occupant isBad().  Outputs per pair and map point i < n_s (entries at and beyond n_s are
 * not touched): d_fuse_idx int32 [n_pairs][map_capacity], the feature picked or -1; d_fuse_act uint8 [n_pairs][map_capacity],
 * ORBX_FUSE_NONE .. ORBX_FUSE_BAD_OCCUPANT; d_fuse_other int32 [n_pairs][map_capacity], the occupant the decision met (a set
 * index, ORBX_FUSE_OCCUPIED_UNMAPPED, an entry >= n_s as it stands) or -1.  d_res [n_pairs].
 * One workgroup per pair, one launch.  The call returns once queued, with the exception orbx_match_bow_batch_device has: when the
 * pair lists differ from the previous call's on this context, the call first waits for the context stream before it uploads
 * them.
 * ORBX_E_BADARG: null required pointers, negative counts, capacity or map_capacity < 1, th not finite or <= 0, th_low outside
 * [0, 256], bounds with max <= min, a keyframe outside [0, n_frames), a map set outside [0, n_map_sets) -- all checked before
 * anything touches a device; ORBX_E_CAPACITY: capacity or map_capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with
 * otherwise well-formed arguments.  n_pairs == 0 is ORBX_OK. */
int orbx_fuse_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_map_set,
                           const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity, int n_map_sets,
                           int map_capacity, const int32_t* d_map_n, const float* d_map_points, const float* d_map_normals,
                           const float* d_map_dist, const uint8_t* d_map_desc32, const uint8_t* d_map_mask, const int32_t* d_map_obs,
                           const float* d_pose, const float* K, const orbx_bounds* bounds, float th, int th_low, int32_t* d_matches,
                           const int32_t* d_occ_obs, int32_t* d_fuse_idx, uint8_t* d_fuse_act, int32_t* d_fuse_other,
                           orbx_fuse_result* d_res);
/* The Scw form: d_scw float [n_pairs][12] as orbx_sim3_compose_scw_batch_device writes it in place of d_pose, no d_map_obs;
 * d_occ_obs is read for its sign only, and with NULL an unmapped occupant is good (SearchAndFuse passes th = 4).  d_fuse_other
 * is vpReplacePoint.  Everything else, the refusals included, as above. */
int orbx_fuse_scw_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_map_set,
                               const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                               int n_map_sets, int map_capacity, const int32_t* d_map_n, const float* d_map_points,
                               const float* d_map_normals, const float* d_map_dist, const uint8_t* d_map_desc32,
                               const uint8_t* d_map_mask, const float* d_scw, const float* K, const orbx_bounds* bounds, float th,
                               int th_low, int32_t* d_matches, const int32_t* d_occ_obs, int32_t* d_fuse_idx, uint8_t* d_fuse_act,
                               int32_t* d_fuse_other, orbx_fuse_result* d_res);
/* The same for one pair in host memory, through the batched path as a batch of one: the keyframe (n features), the map (map_n
 * points; map_mask nullable; map_obs [map_n], required with points in the pose form), pose / scw [12]; matches [n] in and out;
 * occ_obs [n] nullable; fuse_idx, fuse_act, fuse_other [map_n].  More than ORBX_BOW_MAX_FEATURES features or points:
 * ORBX_E_CAPACITY.  Synchronous. */
int orbx_fuse(orbx_ctx* ctx, const orbx_keypoint* kps_un, const uint8_t* desc32, int n, int map_n, const float* map_points,
              const float* map_normals, const float* map_dist, const uint8_t* map_desc32, const uint8_t* map_mask,
              const int32_t* map_obs, const float* pose, const float* K, const orbx_bounds* bounds, float th, int th_low,
              int32_t* matches, const int32_t* occ_obs, int32_t* fuse_idx, uint8_t* fuse_act, int32_t* fuse_other,
              orbx_fuse_result* res);
int orbx_fuse_scw(orbx_ctx* ctx, const orbx_keypoint* kps_un, const uint8_t* desc32, int n, int map_n, const float* map_points,
                  const float* map_normals, const float* map_dist, const uint8_t* map_desc32, const uint8_t* map_mask,
                  const float* scw, const float* K, const orbx_bounds* bounds, float th, int th_low, int32_t* matches,
                  const int32_t* occ_obs, int32_t* fuse_idx, uint8_t* fuse_act, int32_t* fuse_other, orbx_fuse_result* res);

/* ---- local mapping: local bundle adjustment (Optimizer::LocalBundleAdjustment) ------------------------------------------------
 * What LocalMapping calls behind SearchInNeighbors: the keyframes of the local window (free), the keyframes outside it that see
 * the window's points (fixed) and those points are made consistent with each other, for a batch of independent problems, on
 * the rows orbx_match_local_map* / orbx_match_scw* / orbx_fuse* leave and the points orbx_triangulate_matches* writes.  The
 * reference vendors g2o but no Optimizer: the rules restate the monocular Optimizer::LocalBundleAdjustment(pKF, pbStopFlag,
 * pMap) of the ORB-SLAM2 design [from-knowledge] over the vendored g2o sources -- types/types_six_dof_expmap.h:40-102 and
 * .cpp:98-134 (VertexSE3Expmap, EdgeSE3ProjectXYZ), core/block_solver.hpp:354-486 (the Schur complement),
 * core/optimization_algorithm_levenberg.cpp:61-189, core/sparse_optimizer.cpp:376-414, core/robust_kernel_impl.cpp:78-91,
 * solvers/linear_solver_eigen.h (the reduced system's solver, replaced: deviation 1) -- PARITY UNPINNED, as the two-view bundle
 * adjustment above, whose arithmetic (csrc/orbx_ba_math.inc) this shares.  The device equals the CPU restatement
 * tests/cpp/lba_ref.cpp bit for bit.
 *
 * A problem is a run of entries in a flat entry list and one map set.  Entry e names a frame (its row of d_kps_un / d_n /
 * d_pose float [n_frames][12], Rcw row-major then tcw) and owns row e of d_rows int32 [n_entries][capacity]: the keyframe's
 * mvpMapPoints as indices into the problem's map set (d_map_n, d_map_points float [n_map_sets][map_capacity][3], d_map_mask
 * uint8, NULL = every point), entries below 0 (-2 for an unmapped point included) being no observation.  The first n_free
 * entries of a problem are lLocalKeyFrames, the rest lFixedCameras; the caller puts keyframe 0 of the map among the fixed ones.
 *
 * Rules:
 *  1. Graph.  One VertexSE3Expmap per entry, SE3Quat(R, t) of its f32 pose, the free ones first in list order.  One marginalised
 *     VertexSBAPointXYZ per map point below map_n whose mask byte is set and that a free entry observes, ascending index, f32 ->
 *     f64.  One EdgeSE3ProjectXYZ per (entry, feature) whose row names such a point: measurement = the undistorted keypoint,
 *     information = inv_sigma2[octave] * I, RobustKernelHuber with delta = (float)sqrt(5.991) (`const float thHuberMono`).
 *  2. Round 1: optimize(n_iterations) (5): Levenberg-Marquardt exactly as rules 1-7 of the two-view section --
 *     computeLambdaInit over the diagonals of every active free pose and point, up to 10 trials, the _nBad rule -- with
 *     BlockSolver_6_3's Schur complement over all free poses: Hschur = Hpp + lambda I - sum Hpl (Hll + lambda I)^-1 Hpl^T, bschur
 *     = bp - sum Hpl (Hll + lambda I)^-1 bl, xl = (Hll + lambda I)^-1 (bl - Hpl^T xp).  An edge to a fixed keyframe adds to Hll,
 *     bl and chi2 only.
 *  3. Between the rounds every edge with chi2() > 5.991 || !isDepthPositive() goes to level 1 and every edge loses its robust
 *     kernel.  chi2() is e . (information e) of the error as LAST COMPUTED: g2o's stale errors are kept as in
 *     orbx_pose_optimize* (the errors are those of the round's last trial, accepted or not; a trial whose solve failed computes
 *     none).  isDepthPositive uses the current estimates.
 *  4. Round 2: initializeOptimization(0), optimize(n_more_iterations) (10): a fresh run (lambda initialised again, _ni = 2,
 *     _nBad = 0) over the level-0 edges without kernel (rho = (chi2, 1)).  A vertex without an active edge is not part of the
 *     round: its estimate keeps its bits, it adds nothing to the system, to computeLambdaInit or to computeScale.  (The same
 *     holds in round 1 for a free keyframe that observes nothing.)
 *  5. Behind round 2 the test of rule 3, over ALL edges, fills d_obs_outlier (vToErase).  Free poses go out as f32 Tcw: the
 *     rotation matrix of the quaternion, as orbx_bundle_adjust* writes R21; points go out as f32.
 * UpdateNormalAndDepth, the SetWorldPos / SetPose bookkeeping and the erasures themselves (EraseMapPointMatch /
 * EraseObservation for every set byte of d_obs_outlier) stay with the caller, who may hand the erasures, UpdateNormalAndDepth
 * and ComputeDistinctiveDescriptors to orbx_map_update* ("local mapping: updating the map points", below).
 *
 * Documented deviations:
 *  1. Linear solver.  The reduced system of the active free poses (6 x their count, in entry order) is dense and solved by an
 *     unpivoted Cholesky factorisation: column by column, every element receiving its terms in ascending column; L y = b in
 *     ascending and L^T x = y in descending column order.  A pivot that is not > 0 or not finite, or a non-finite solution, is a
 *     failed solve: no step is applied, tempChi is DBL_MAX, the trial is rejected (two-view section, deviation 2).  g2o uses
 *     Eigen's sparse LDLT with a block ordering.
 *  2. Sums.  Every floating-point sum is f64 in an order that depends on the input only (csrc/orbx_lba_math.inc states each):
 *     a problem has 256 lanes; vertex j belongs to lane j % 256.  Hll and bl of a vertex: its owner, over its edges in ascending
 *     entry.  chi2, the points' part of computeScale: a lane adds its vertices' terms in ascending j (a vertex's edges in
 *     ascending entry), then the lanes are folded as a tree: lane l += lane l + 128, then + 64, ... + 1.  Hpp and bp of a free
 *     pose: lane l of 64 adds the terms of the keyframe's features l, l + 64, ...; lane l += lane l + 32, + 16, ... + 1.  Each row
 *     of each 6x6 block (a, c), a <= c, of sum Hpl Dinv Hpl^T, and each row of sum Hpl Dinv bl: one owner, over the vertices in
 *     ascending index whose active observer word has both bits.  computeScale: the poses' terms in order, + the points' sum, +
 *     1e-3.  No floating-point atomic is used.
 *  3. A point's observations are ordered by entry (the reference's std::map<KeyFrame*, size_t> by address).
 *  4. There is no pbStopFlag and there are no Map / KeyFrame / MapPoint types.
 *  5. The errors of a round's active edges are computed once when the round starts, so a round with 0 iterations classifies at
 *     the estimates it was given (g2o would read errors never computed).
 *  6. Garbage is flagged and never followed.  ORBX_LBA_BAD_INPUT: a count outside its capacity (d_n of an entry's frame, d_map_n),
 *     a row entry >= map_n, an octave outside the table on a feature that names a masked point, two features of one keyframe
 *     naming one point vertex, a frame used twice in one problem.  ORBX_LBA_NONFINITE: a non-finite pose of an entry or point
 *     vertex, or a non-finite result.  A flagged problem copies its inputs through: every d_pose_out row is the input's bits,
 *     no point is written, every outlier byte of its entries is 0, every number of the result but status and n_free is 0 (a non-finite RESULT keeps
 *     its counters).
 *  7. n_free == 0 or a problem without an edge runs nothing: status 0, the inputs copied through.
 *  8. Problems are independent: two problems may share a map set as long as no point is a vertex of both (and, in place, none
 *     is a vertex of one and read by the other); the entry runs of two problems do not overlap. */
#define ORBX_LBA_MAX_FREE 64     /* free keyframes per problem: one 64-bit word of free observers per point */
#define ORBX_LBA_BAD_INPUT 2
#define ORBX_LBA_NONFINITE 4
typedef struct orbx_lba_result {
  int32_t status;             /* 0, or a bitmask of ORBX_LBA_*; every field is written for every problem */
  int32_t n_points, n_edges;  /* point vertices, edges (to free and fixed entries) */
  int32_t n_free;
  int32_t iterations[2];      /* per round: solve() calls */
  int32_t lm_trials[2];       /* the sum of qmax */
  int32_t rejected_trials[2];
  int32_t solver_failures[2];
  int32_t stop_reason[2];     /* 0 = all iterations ran, 1 = qmax == 10 || rho == 0, 2 = _nBad >= 3 */
  int32_t n_active_points[2]; /* point vertices / free poses with an active edge in the round */
  int32_t n_active_free[2];
  int32_t n_level1;           /* edges set aside between the rounds */
  int32_t n_erased;           /* set bytes of d_obs_outlier (vToErase) */
  double chi2_initial[2], chi2_final[2], lambda[2];
} orbx_lba_result;

/* Batched, device-resident, stream-ordered on the context stream.  Host arrays [n_problems]: h_first / h_count (the problem's
 * run in the entry list), h_n_free, h_map_set; h_entry_frame [n_entries].  K row-major 3x3 (host, f32); inv_sigma2: host,
 * nlevels floats, NULL = the context's table; n_iterations, n_more_iterations >= 0 (5, 10).  Outputs: d_pose_out float
 * [n_entries][12] (free: the optimised pose; fixed: a copy of its input); d_map_points_out [n_map_sets][map_capacity][3], which
 * may equal d_map_points (otherwise the call first copies d_map_points to it: points outside a problem or without an
 * observation come through bit for bit); d_obs_outlier uint8 [n_entries][capacity], every byte of a problem's entries written;
 * d_res [n_problems].  One workgroup per problem runs both rounds in one launch.  Workspace: per problem the bytes
 * csrc/orbx_lba_math.inc layout() counts (DESIGN.md 4s has the formula), grown in the context; a call whose workspace cannot be
 * allocated returns ORBX_E_HIP and runs nothing.  The call returns once queued, with the exception
 * orbx_bundle_adjust_batch_device has (a list or table that differs from the previous call's is uploaded behind a wait).
 * ORBX_E_BADARG: null required pointers, negative counts, capacity or map_capacity < 1, a run outside [0, n_entries], n_free
 * outside [0, count] or above ORBX_LBA_MAX_FREE, a map set outside [0, n_map_sets), a frame outside [0, n_frames);
 * ORBX_E_CAPACITY: capacity or map_capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with otherwise well-formed
 * arguments -- all checked before anything touches a device; ORBX_E_CAPACITY also for a batch whose workspace would exceed
 * 512 GiB.  n_problems == 0 is ORBX_OK.  The workspace is a block of the context's own (not the staging block of the
 * single-problem calls, which the host form fills while this call runs); it only grows and is freed with the context: a
 * context that once ran 640 local windows keeps their 2.7 GB.  A problem with at most 29 free keyframes keeps the reduced
 * system's packed factor in LDS: the launch asks for the largest such factor of the batch as dynamic LDS, up to 120,408 bytes
 * beside the kernel's 36 KB, and a launch that asks for more than about 45 KB has one workgroup per CU instead of two. */
int orbx_local_ba_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_first, const int32_t* h_count,
                               const int32_t* h_n_free, const int32_t* h_map_set, int n_entries, const int32_t* h_entry_frame,
                               const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const float* d_pose,
                               const int32_t* d_rows, int n_map_sets, int map_capacity, const int32_t* d_map_n,
                               const float* d_map_points, const uint8_t* d_map_mask, const float* K, const float* inv_sigma2,
                               int n_iterations, int n_more_iterations, float* d_pose_out, float* d_map_points_out,
                               uint8_t* d_obs_outlier, orbx_lba_result* d_res);
/* One problem in host memory, run through the batched path as a batch of one: entry e is keyframe e (kps_un
 * [n_entries][capacity], n [n_entries], pose [n_entries][12], rows [n_entries][capacity]), the first n_free free; map_points
 * [map_n][3], map_mask [map_n] nullable; pose_out [n_entries][12], map_points_out [map_n][3] (may equal map_points),
 * obs_outlier [n_entries][capacity].  Synchronous. */
int orbx_local_ba(orbx_ctx* ctx, int n_entries, int n_free, const orbx_keypoint* kps_un, const int32_t* n, int capacity,
                  const float* pose, const int32_t* rows, int map_n, const float* map_points, const uint8_t* map_mask,
                  const float* K, const float* inv_sigma2, int n_iterations, int n_more_iterations, float* pose_out,
                  float* map_points_out, uint8_t* obs_outlier, orbx_lba_result* res);

/* Measurement aid: problems with at most max_free free keyframes keep the reduced system's packed factor in LDS (default and
 * largest value 29: 120,408 bytes beside the kernel's 36 KB); 0 = every problem keeps it in the workspace, -1 restores the
 * default.  Every value gives the same bytes.  Process-wide.  ORBX_E_BADARG outside [-1, 29]. */
int orbx_debug_local_ba_lds_max_free(int max_free);

/* ---- local mapping: updating the map points (MapPoint::Observations, UpdateNormalAndDepth, ComputeDistinctiveDescriptors) ----
 * What LocalMapping does with the result of the local bundle adjustment before the tracker matches against the map again:
 * vToErase is applied (KeyFrame::EraseMapPointMatch / MapPoint::EraseObservation with its nObs <= 2 rule), and every adjusted
 * point gets its observation count, its mean viewing direction and scale-invariance distances and its representative
 * descriptor -- the four arrays per map set that orbx_match_local_map*, orbx_match_scw*, orbx_fuse* and
 * orbx_match_keyframe_projection* read (d_map_normals, d_map_dist, d_map_desc32, d_map_obs), written on the device, for a batch
 * of independent problems, in the layout orbx_local_ba_batch_device uses.  The reference ships no MapPoint: the rules restate
 * MapPoint::EraseObservation, Observations, UpdateNormalAndDepth and ComputeDistinctiveDescriptors of the ORB-SLAM2 design
 * [from-knowledge], PARITY UNPINNED, as Fuse and the local bundle adjustment above.  The device equals the CPU restatement
 * tests/cpp/map_update_ref.cpp bit for bit, which shares csrc/orbx_map_math.inc with it and is itself tested against an
 * independently written numpy statement.
 *
 * A problem is exactly a problem of orbx_local_ba_batch_device: a run of entries in a flat entry list, the first n_free of
 * them free, and one map set.  Entry e names a frame (its row of d_kps_un / d_desc32 / d_n), has its pose in row e of
 * d_entry_pose float [n_entries][12] (orbx_local_ba_batch_device's d_pose_out as it is) and owns row e of d_rows.  Features at
 * or beyond the frame's d_n are not read.  All arithmetic is f32 without contraction unless said otherwise.
 *
 * Rules:
 *  1. Points updated.  The points updated ("vertices") are the local bundle adjustment's: i < map_n, mask byte set (d_map_mask
 *     NULL = every point), named by the row of at least one FREE entry on entry.  With n_free == count that is every point any
 *     entry names: the form for use behind orbx_fuse* / orbx_triangulate_matches*.  A point that is not a vertex is not touched
 *     in any output.
 *  2. Erasures.  With d_obs_outlier, every (entry, feature) whose byte is set and whose row entry names a vertex gets row entry
 *     -1 (n_erased).  A set byte anywhere else is ignored.
 *  3. Observation counts.  obs_i = the number of entries whose row still names vertex i -> d_map_obs.  A vertex that lost at
 *     least one observation in rule 2 and has obs_i <= 2 is bad (EraseObservation -> SetBadFlag): its d_map_mask_out byte is 0,
 *     every row entry of the problem that names it becomes -1 (n_cleared), its d_map_obs is 0 and nothing else is written for
 *     it (n_bad_points).  A vertex that lost nothing keeps its mask byte whatever its count: a freshly triangulated point has
 *     two observations.
 *  4. The reference keyframe.  The observers of a point are ordered by ascending entry.  The reference keyframe (mpRefKF) is
 *     the observer whose frame is d_map_ref[i]; where there is none -- a negative value, d_map_ref NULL, or the keyframe erased
 *     in rule 2 or no observer -- it is the first observer, and d_map_ref[i] is set to its frame (n_ref_moved counts the
 *     non-negative values that changed).
 *  5. ORBX_MAP_NORMALS: UpdateNormalAndDepth.  Ow_e = -Rcw^T tcw of the entry's pose (gemm: f64 products and sum, one rounding).
 *     Per observer in order: d = P - Ow_e, len = cv::norm(d) (f64 inside, rounded to f32), normal_k += d_k / len, starting
 *     from +0.0f; then normal_k / (float)obs_i -> d_map_normals.  dist = cv::norm(P - Ow_ref); max = dist * scale[octave of the
 *     reference's feature]; min = max / scale[nlevels - 1]; d_map_dist[i] = (min, max).  The scale table is the context's.  For
 *     a point with two observers, KF1 the reference, these are the bits rule 6 of orbx_triangulate_matches* writes (one source:
 *     csrc/orbx_tri_math.inc).
 *  6. ORBX_MAP_DESCRIPTORS: ComputeDistinctiveDescriptors.  Over the observers' descriptors D_0 .. D_{N-1} in order:
 *     dist[a][b] = popcount(D_a ^ D_b); median_a = the element at index (N - 1) / 2 (integer division: `0.5 * (N - 1)`
 *     truncated) of row a sorted ascending, the zero on the diagonal included; the first a with the smallest median wins
 *     (`median < BestMedian` from INT_MAX); d_map_desc32[i] = D_a.
 *  7. Garbage is flagged and never followed.  ORBX_MAP_BAD_INPUT: a count outside its capacity (d_n of an entry's frame,
 *     d_map_n), a row entry >= map_n, two features of one entry naming one vertex (an erased one included), a frame twice in
 *     one problem, the octave of a reference keyframe's feature outside the table.  ORBX_MAP_NONFINITE: a non-finite pose of an
 *     entry, a non-finite vertex position, a len that is 0 or no number.  The checks do not depend on `what`.  A flagged
 *     problem changes NOTHING: rows, mask, reference frames and every output keep their bits, every field of the record but
 *     status is 0.
 *
 * Documented deviations:
 *  1. The entry run is assumed to hold every keyframe that observes a vertex, which is how LocalBundleAdjustment builds its
 *     fixed cameras: an observer outside the run is not counted, summed or compared.
 *  2. A point's observations are ordered by entry (the design's std::map<KeyFrame*, size_t> by address): the local bundle
 *     adjustment's deviation 3.
 *  3. There is no KeyFrame::isBad(): a culled keyframe is simply not an entry.
 *  4. max_observers is taken over every vertex, the bad ones with the count that made them bad.
 *  5. Problems are independent as under the local bundle adjustment's deviation 8: two problems may share a map set as long as
 *     no point is a vertex of both (and, with d_map_mask_out == d_map_mask, none is a vertex of one and named by the other);
 *     the entry runs of two problems do not overlap.
 * Out of scope: MapPoint::Replace and replaying orbx_fuse*'s d_fuse_act decisions across keyframes, KeyFrame::UpdateConnections,
 * culling (MapPointCulling / KeyFrameCulling), stereo. */
#define ORBX_MAP_NORMALS 1
#define ORBX_MAP_DESCRIPTORS 2
#define ORBX_MAP_BAD_INPUT 2
#define ORBX_MAP_NONFINITE 4
typedef struct orbx_map_result {
  int32_t status;          /* 0, or a bitmask of ORBX_MAP_BAD_INPUT / ORBX_MAP_NONFINITE; every field is written for every problem */
  int32_t n_points;        /* vertices */
  int32_t n_observations;  /* the sum of obs_i over the vertices that are not bad */
  int32_t n_erased;        /* rule 2 */
  int32_t n_bad_points;    /* rule 3 */
  int32_t n_cleared;       /* rule 3 */
  int32_t n_ref_moved;     /* rule 4 */
  int32_t max_observers;   /* the largest obs_i */
  int32_t n_free;          /* as given */
  int32_t reserved[7];     /* zero */
} orbx_map_result;

/* Batched, device-resident, stream-ordered on the context stream.  Host arrays [n_problems]: h_first / h_count (the problem's
 * run in the entry list), h_n_free, h_map_set; h_entry_frame [n_entries].  d_desc32 uint8 [n_frames][capacity][32] (read with
 * ORBX_MAP_DESCRIPTORS only; 4-byte aligned); d_rows int32 [n_entries][capacity], in and out; d_obs_outlier uint8
 * [n_entries][capacity] or NULL: orbx_local_ba*'s vToErase.  d_map_mask uint8 [n_map_sets][map_capacity] (NULL = every point);
 * d_map_mask_out required, may equal d_map_mask; d_map_ref int32 [n_map_sets][map_capacity] or NULL: mpRefKF as a FRAME index,
 * < 0 = none yet, in and out.  what: a bitmask of ORBX_MAP_NORMALS / ORBX_MAP_DESCRIPTORS (0 = rows, mask, counts and
 * reference frames only).  Outputs, vertices only: d_map_normals float [..][3], d_map_dist float [..][2], d_map_desc32 uint8
 * [..][32], d_map_obs int32 [..]; d_res [n_problems].  Two launches: one workgroup per problem checks the problem, builds the
 * inverse of the rows and writes rows, mask, counts and reference frames; then (what != 0) a grid over (problem, 64 points), a
 * wave per point, writes the rest.  Workspace: per problem 256-byte aligned arrays of 12 map_capacity + 8 map_capacity *
 * count + 12 count + 4 bytes (MapWork of csrc/orbx_device.h), a block of the context's own that only grows and is
 * freed with the context: a context that once ran 640 local windows of 20 keyframes and 2000 points keeps their 220 MB.  The
 * call returns once queued, with the exception orbx_bundle_adjust_batch_device has.  ORBX_E_BADARG: null required pointers
 * (d_map_obs and d_map_mask_out always; d_map_normals and d_map_dist, d_desc32 and d_map_desc32 when `what` names them),
 * negative counts, capacity or map_capacity < 1, what outside [0, 3], a frame outside [0, n_frames), a run outside [0,
 * n_entries], n_free outside [0, count] (no other bound), a map set outside [0, n_map_sets); ORBX_E_CAPACITY: capacity or
 * map_capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with otherwise well-formed arguments -- all checked before
 * anything touches a device; ORBX_E_CAPACITY also for a batch whose workspace would exceed 512 GiB.  n_problems == 0 is
 * ORBX_OK. */
int orbx_map_update_batch_device(orbx_ctx* ctx, int n_frames, int n_problems, const int32_t* h_first, const int32_t* h_count,
                                 const int32_t* h_n_free, const int32_t* h_map_set, int n_entries, const int32_t* h_entry_frame,
                                 const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                                 const float* d_entry_pose, int32_t* d_rows, const uint8_t* d_obs_outlier, int n_map_sets,
                                 int map_capacity, const int32_t* d_map_n, const float* d_map_points, const uint8_t* d_map_mask,
                                 uint8_t* d_map_mask_out, int32_t* d_map_ref, int what, float* d_map_normals, float* d_map_dist,
                                 uint8_t* d_map_desc32, int32_t* d_map_obs, orbx_map_result* d_res);
/* One problem in host memory, run through the batched path as a batch of one: entry e is keyframe e (kps_un
 * [n_entries][capacity], desc32 [n_entries][capacity][32], n [n_entries], pose [n_entries][12], rows [n_entries][capacity] in
 * and out, obs_outlier [n_entries][capacity] or NULL), the first n_free free; map_points [map_n][3], map_mask [map_n] nullable,
 * map_mask_out [map_n] (may equal map_mask), map_ref [map_n] nullable, in and out; map_normals, map_dist, map_desc32, map_obs
 * [map_n] rows in and out: what the call does not write comes back as it went in.  Synchronous. */
int orbx_map_update(orbx_ctx* ctx, int n_entries, int n_free, const orbx_keypoint* kps_un, const uint8_t* desc32, const int32_t* n,
                    int capacity, const float* pose, int32_t* rows, const uint8_t* obs_outlier, int map_n, const float* map_points,
                    const uint8_t* map_mask, uint8_t* map_mask_out, int32_t* map_ref, int what, float* map_normals, float* map_dist,
                    uint8_t* map_desc32, int32_t* map_obs, orbx_map_result* res);

/* ---- stereo: matching left and right ------------------------------------------------------------------------------------------
 * Frame::ComputeStereoMatches (and, as an optional tail, Frame::UnprojectStereo) of ORB-SLAM2's stereo Frame constructor, for
 * batches of rigs.  The reference ships no stereo: this is ORB-SLAM2's code, [from-knowledge], PARITY UNPINNED, as the sections
 * above.  The device equals the CPU restatement tests/cpp/stereo_ref.cpp bit for bit, which shares csrc/orbx_stereo_math.inc
 * with it and is itself tested against an independently written numpy statement and against ground truth.
 *
 * A rig p is a (left frame, right frame) pair of ONE extract batch: L = h_left[p] and R = h_right[p] are frame indices of the
 * context's LAST EXTRACT CALL, whose pyramid is still resident (level 0: the caller's frames, read in place, so they must still
 * be there; levels 1..: the context's own).  The keypoints are the raw mvKeys (stereo input is rectified), bf is mbf, b is mb,
 * scale[] / inv_scale[] are the context's tables (orbx_get_tables), cols_l / rows_l the level sizes (orbx_level_size).  All
 * arithmetic is f32 without contraction unless said otherwise.
 *
 * Rules:
 *  1. Every u_right[i] = -1.0f, depth[i] = -1.0f, match_right[i] = -1, sad[i] = -1 (i < d_n[L]; rows beyond it are not touched).
 *  2. Row bands.  Right keypoint iR: r = 2.0f * scale[oct_R], maxr = (int)ceilf(y_R + r), minr = (int)floorf(y_R - r) (f32
 *     sums).  It is a candidate of row y for minr <= y <= maxr, clipped to [0, rows_0).
 *  3. Limits.  minD = 0, maxD = bf / b (f32 division), thOrbDist = (100 + 50) / 2 = 75.
 *  4. Left keypoint iL: row = (int)y_L (truncation); minU = x_L - maxD, maxU = x_L.  Skipped when maxU < 0.
 *  5. Candidates are the right keypoints that pass all three tests: the band holds `row`; oct_L - 1 <= oct_R <= oct_L + 1;
 *     minU <= x_R <= maxU (both ends inclusive).
 *  6. Descriptor search.  d = popcount(desc_L ^ desc_R); best = the smallest d, among equal d the LOWEST iR (the design's
 *     ascending row lists with a strict <).  bestDist starts at 100 (TH_HIGH), so d >= 100 never matches.  The search continues
 *     only when best < 75.
 *  7. Coordinates at the keypoint's level o = oct_L: su = roundf(x_L * inv_scale[o]), sv = roundf(y_L * inv_scale[o]),
 *     su0 = roundf(x_R(best) * inv_scale[o]): f32 products, rounded half away from zero.
 *  8. Window test.  With w = 5, L = 5: refused (`continue`) when su0 + L - w < 0 || su0 + L + w + 1 >= cols_o.  The test is the
 *     design's as written; it is weaker than what it reads.  That is the design's quirk; see deviation 1.
 *  9. SAD over the shifts.  For inc = -5 .. +5 in ascending order, SAD(inc) = the sum over the 11 x 11 window of
 *     | (IL(sv+dy, su+dx) - IL(sv, su)) - (IR(sv+dy, su0+inc+dx) - IR(sv, su0+inc)) |, both sides read from level o of L and of
 *     R.  Integer arithmetic (at most 121 * 510 = 61 710); it equals the design's convertTo(CV_32F), centre subtraction and
 *     cv::norm(NORM_L1) exactly.  The best is the first inc with the smallest SAD (strict <).  Refused when it is -5 or +5.
 * 10. Parabola.  d1, d2, d3 = SAD at best-1, best, best+1 as f32; delta = (d1 - d3) / (2.0f * ((d1 + d3) - 2.0f * d2)).
 *     Refused when delta < -1 || delta > 1.
 * 11. Disparity.  bestuR = scale[o] * ((su0 + (float)inc) + delta); disp = x_L - bestuR.  Kept when disp >= 0 && disp < maxD.
 *     When disp <= 0: disp = 0.01f and bestuR = (float)((double)x_L - 0.01).  depth[iL] = bf / disp, u_right[iL] = bestuR,
 *     match_right[iL] = best iR, sad[iL] = SAD(best).
 * 12. Median filter.  With M kept matches and M > 0: median = the element of rank M / 2 (0-based) of the kept SADs in ascending
 *     order; thDist = (1.5f * 1.4f) * (float)median; every kept match with (float)sad >= thDist goes back to -1 / -1.0f in all
 *     four arrays.  A median of 0 therefore removes EVERY match: the design's quirk, kept.
 * 13. Optional tail, Frame::UnprojectStereo, when d_points is given.  For depth[i] > 0: z = depth; x = ((u - cx) * z) * invfx,
 *     y = ((v - cy) * z) * invfy with invfx = 1.0f / fx; (u, v) from d_kps_un when given, else from d_kps.  Without d_pose_wc
 *     the point is in camera coordinates; with it (12 floats per rig: Rwc row-major, then Ow) it is
 *     ((R0*x + R1*y) + R2*z) + t0 and so on.  Any other i < d_n[L] gets (0, 0, 0).  d_point_mask[i] = depth[i] > 0.  The row
 *     is a point set that orbx_match_projection* and orbx_pose_optimize* take as it is.
 *
 * Documented deviations:
 *  1. A window or strip that would leave its level is refused and counted (n_out_of_level), never read: sv +- 5 rows and
 *     su +- 5 columns on the left, su0 - 10 .. su0 + 10 columns on the right.  OpenCV would throw.  For the extractor's own
 *     keypoints it cannot happen at scale factors up to 1.5: a keypoint of level l lies at least 16 pixels of ITS level from
 *     that level's edges (EDGE_THRESHOLD - 3), which covers the left window, and a match is at most one octave away, so at
 *     level o the right keypoint lies at least 16 / 1.5 > 10.5 pixels inside, which covers the strip.  (At a factor of 2 a
 *     right keypoint one octave below can come as close as 8 pixels: then the deviation is reached and counted.)  Rule 8 alone
 *     asks su0 >= 0 only, so a hand-made keypoint reaches it at any factor.
 *  2. M == 0: nothing to filter (median_sad 0, th_dist 0).  The design indexes an empty vector.
 *  3. Garbage is flagged and never followed: ORBX_STEREO_BAD_INPUT for an octave outside [0, nlevels), a `row` outside
 *     [0, rows_0), or a count outside [0, capacity] (clamped); ORBX_STEREO_NONFINITE for a non-finite coordinate.  Such a
 *     keypoint is skipped, on either side; the rest of the rig is unaffected.
 *  4. Results are arrays and indices.
 * Out of scope: the stereo edges of the optimisers, the mvuRight tests of the matchers, StereoInitialization. */
#define ORBX_STEREO_BAD_INPUT 2
#define ORBX_STEREO_NONFINITE 4
typedef struct orbx_stereo_result {
  int32_t status;               /* 0, or a bitmask of ORBX_STEREO_BAD_INPUT / ORBX_STEREO_NONFINITE; every field is written for every rig */
  int32_t n_matches;            /* after rule 12 */
  int32_t n_with_candidates;    /* left keypoints with at least one candidate (rule 5) */
  int32_t n_orb_matched;        /* rule 6: best < 75 */
  int32_t n_window_refused;     /* rule 8 */
  int32_t n_out_of_level;       /* deviation 1 */
  int32_t n_edge;               /* rule 9: the best shift is -5 or +5 */
  int32_t n_delta_refused;      /* rule 10 */
  int32_t n_disparity_refused;  /* rule 11 */
  int32_t n_clamped;            /* rule 11: disp <= 0 */
  int32_t n_before_median;      /* M */
  int32_t median_sad;
  float th_dist;
  int32_t n_removed_by_median;
  int32_t reserved[2];          /* zero */
} orbx_stereo_result;

/* Batched, device-resident, stream-ordered on the context stream; returns once queued (with the exception
 * orbx_bundle_adjust_batch_device has).  Host arrays h_left / h_right [n_rigs].  d_kps [n_frames][capacity], d_desc32 uint8
 * [n_frames][capacity][32] (16-byte aligned), d_n [n_frames]: what the last extract call wrote.  Outputs, rows
 * [n_rigs][capacity]: d_u_right, d_depth float; d_match_right, d_sad int32, nullable; d_points float [..][3] and d_point_mask
 * uint8, nullable (rule 13: K is the host 3x3, required with d_points; d_kps_un [n_frames][capacity] nullable; d_pose_wc float
 * [n_rigs][12] nullable); d_res [n_rigs].  Two launches: k_stereo_match over (rig, blocks of 32 left keypoints), k_stereo_filter
 * with a workgroup per rig.  ORBX_E_BADARG, judged before anything touches a device: null required pointers, negative counts,
 * capacity < 1, bf or b not finite or <= 0, a frame index outside [0, n_frames), h_left[p] == h_right[p], d_points without K,
 * d_desc32 not 16-byte aligned; ORBX_E_CAPACITY: capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with otherwise
 * well-formed arguments.  n_rigs == 0 is ORBX_OK.  With a context, ORBX_E_BADARG and a message in orbx_last_error when n_frames
 * differs from the last extract call's frame count, when there was no extract call, and while batches are in flight on lanes
 * (orbx_set_pipeline_depth > 0 with work pending). */
int orbx_stereo_match_batch_device(orbx_ctx* ctx, int n_frames, int n_rigs, const int32_t* h_left, const int32_t* h_right,
                                   const orbx_keypoint* d_kps, const uint8_t* d_desc32, const int32_t* d_n, int capacity, float bf,
                                   float b, float* d_u_right, float* d_depth, int32_t* d_match_right, int32_t* d_sad,
                                   const orbx_keypoint* d_kps_un, const float* K, const float* d_pose_wc, float* d_points,
                                   uint8_t* d_point_mask, orbx_stereo_result* d_res);
/* The stereo Frame constructor for one rig in host memory: both images (width x height, row stride `stride`) go through the
 * batched path as a batch of two, then comes the call above.  kpsL / kpsR, descL / descR hold `capacity` entries (at least the
 * context's feature budget, as orbx_extract_batch asks), u_right / depth `capacity` floats of which the first *nL are written.
 * Synchronous.  The call's pyramid is not kept for later calls (its level 0 lies in the context's staging block): a following
 * orbx_stereo_match_batch_device or orbx_download_pyramid needs an extract call of its own. */
int orbx_extract_stereo(orbx_ctx* ctx, const uint8_t* left, const uint8_t* right, int width, int height, int stride, float bf,
                        float b, orbx_keypoint* kpsL, uint8_t* descL, int32_t* nL, orbx_keypoint* kpsR, uint8_t* descR, int32_t* nR,
                        int capacity, float* u_right, float* depth, orbx_stereo_result* res);

/* ---- bag of words: DBoW2 TemplatedVocabulary<FORB>::transform and L1Scoring::score ---------------------------------------
 * (Thirdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1078-1270, src/BowVector.cpp:36-86, src/FeatureVector.cpp:31-45,
 * include/DBoW2/ScoringObject.h:72-88, src/ScoringObject.cpp:23-66; what Frame::mBowVec / mFeatVec hold, SlamTypes/Frame.hpp:79-81.)
 * Bit-identical to a CPU restatement of those lines (tests/cpp/bow_ref.cpp): word ids, node ids, feature indices and the bytes
 * of every f64.  PINNED to the reference's own compiled code: the restatement is compared bit for bit with DBoW2's own
 * loadFromTextFile / transform / scoring objects (built unmodified into oracle/_ref/libref.so; tests/test_ref_pins.py), and the
 * device directly with them (tests/test_gpu_ref_pins.py), for every weighting x scoring and levelsup 0 .. L + 1; so is this
 * library's text parser (orbx_vocabulary_parse_text) against loadFromTextFile.  Not compared where the reference is undefined:
 * deviations 1 and 2 below, k < 2, trees beyond the k^(L+1) nodes the loader reserves, and what deviation 3 refuses.
 *   node ids      the loader's (:1542-1620): root 0, the file's node lines 1, 2, ... in order; children in file order; word ids in
 *                 file order to the lines whose leaf flag is > 0
 *   descent       at each level the child with the smallest Hamming distance, the first child on a tie; it ends at a node WITHOUT
 *                 CHILDREN (isLeaf()), whatever its flag: a childless node flagged non-leaf gives word id 0 and its own weight,
 *                 a flagged leaf with children is descended through.  The FeatureVector's node is the one at depth L - levelsup
 *                 (the root, 0, when that is <= 0)
 *   BowVector     a feature whose weight is <= 0 is stopped; TF / TF_IDF: repeated f64 additions of the weight, divided by the
 *                 number of distinct WORDS when the scoring does not normalise (DOT_PRODUCT, the reference's quirk); IDF / BINARY:
 *                 the first value; scoring L2_NORM: L2 norm, every other scoring but DOT_PRODUCT: L1 norm, a sequential f64 sum in
 *                 ascending word order (nothing divided when it is 0)
 *   FeatureVector node ids ascending, each with its feature indices ascending; stopped features absent
 *   empty         a vocabulary without words, or a frame without keypoints: both vectors empty
 * Documented deviations from the reference:
 *   1. Trailing empty line: the reference loader turns an empty last line (every file saveToTextFile writes ends in one) into an
 *      extra child of the root with weight 0, word id 0 and an UNINITIALISED descriptor, whose effect is indeterminate; here
 *      empty and whitespace-only lines are skipped.
 *   2. Shallow leaf: a leaf reached above depth L - levelsup leaves the reference's nid uninitialised (UB); here it is the
 *      leaf's own node id.
 *   3. Refused inputs (ORBX_E_BADARG; the reference accepts them with UB, or prints a message and keeps an empty vocabulary): a
 *      parent id outside [0, the line's own id); a node with more than k children; a node deeper than L; a header outside
 *      k 0..20, L 1..10, scoring 0..5, weighting 0..3; a node line with fewer than 35 numbers; a number followed directly
 *      by other characters; an int outside int's range; a weight token that is not one complete finite decimal number
 *      [+-]?(d+(.d*)?|.d+)([eE][+-]?d+)?, where the reference's `istream >> double` reads, without an error it checks: inf, nan
 *      and other tokens without a number (0), a hexadecimal float such as 0x1p3 (its leading 0), a number with trailing
 *      characters such as 1e5x (the number), an overflow such as 1e400 (+-DBL_MAX).
 *   4. Scores: only L1Scoring::score (scoring L1_NORM) is offered; the score entry point returns ORBX_E_BADARG for the other five
 *      scoring types.  transform supports all four weightings and both norms.
 * Descriptor elements are parsed as int and cast to uint8 (an explicit sign, a leading zero and values outside a byte as the
 * reference reads them: +7 -> 7, 07 -> 7, 300 -> 44, -1 -> 255), weights as double (strtod on the whole token, which is what
 * istream >> double computes for the tokens accepted: underflow to 0 or a denormal, -0 and 6- or 17-digit forms included).
 * CRLF line ends and tokens after the weight are accepted and ignored, as by the reference.
 * A frame may hold up to ORBX_BOW_MAX_FEATURES keypoints: a larger capacity returns ORBX_E_CAPACITY. */
#define ORBX_BOW_MAX_FEATURES 16384
#define ORBX_BOW_TF_IDF 0 /* WeightingType */
#define ORBX_BOW_TF 1
#define ORBX_BOW_IDF 2
#define ORBX_BOW_BINARY 3
#define ORBX_BOW_L1_NORM 0 /* ScoringType */
#define ORBX_BOW_L2_NORM 1
#define ORBX_BOW_CHI_SQUARE 2
#define ORBX_BOW_KL 3
#define ORBX_BOW_BHATTACHARYYA 4
#define ORBX_BOW_DOT_PRODUCT 5
typedef struct orbx_vocabulary orbx_vocabulary;

/* Host only, no context: the text format of saveToTextFile (:1626-1645; ORB-SLAM's ORBvoc.txt), a header "k L scoring
 * weighting" and one line "parent leaf_flag d0 .. d31 weight" per node.  header = {k, L, scoring, weighting}; for node i + 1
 * (i in [0, n)): parent[i], is_leaf[i] (the flag as read), desc32[i * 32 .. +32], weight[i].  With NULL arrays only *n_nodes
 * is set; with arrays, capacity < n returns ORBX_E_CAPACITY.  Returns the node count, or ORBX_E_BADARG for an unreadable
 * file, a bad header or line, or a refused tree (deviation 3).  This is the parser of orbx_vocabulary_load_text. */
int orbx_vocabulary_parse_text(const char* path, int32_t* header, int32_t* n_nodes, int32_t* parent, int32_t* is_leaf,
                               uint8_t* desc32, double* weight, int32_t capacity);
/* A vocabulary on the context's device from host arrays for nodes 1..n_nodes in file order (the layout above).  The tree is
 * checked first (ORBX_E_BADARG, deviation 3), then laid out breadth-first on the device.  ctx == NULL (no device: orbx_create
 * returned ORBX_E_HIP) returns ORBX_E_HIP for a well-formed tree.  Destroy vocabularies before their context. */
int orbx_vocabulary_create(orbx_ctx* ctx, int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                           const int32_t* is_leaf, const uint8_t* desc32, const double* weight, orbx_vocabulary** out);
int orbx_vocabulary_load_text(orbx_ctx* ctx, const char* path, orbx_vocabulary** out);
void orbx_vocabulary_destroy(orbx_vocabulary* voc);
/* info = {k, L, scoring, weighting, nodes (without the root), words} */
int orbx_vocabulary_info(const orbx_vocabulary* voc, int32_t* info6);
/* Nodes 1..n of any vocabulary, loaded, created or trained, in file order and in the layout of orbx_vocabulary_parse_text;
 * is_leaf is the flag as it was given (trained vocabularies: 1 for the nodes without children).  With NULL arrays only the
 * count is returned; with arrays, capacity < n returns ORBX_E_CAPACITY.  Returns the node count. */
int orbx_vocabulary_get_nodes(const orbx_vocabulary* voc, int32_t* parent, int32_t* is_leaf, uint8_t* desc32, double* weight,
                              int32_t capacity);
/* saveToTextFile (:1626-1645).  exact == 0 writes every weight as an ostream writes a double (6 significant digits), as the
 * reference does; exact != 0 writes 17 significant digits, so that loading the file returns the same bytes.  ORBX_E_BADARG:
 * null pointers or a file that cannot be written. */
int orbx_vocabulary_save_text(const orbx_vocabulary* voc, const char* path, int exact);

/* ---- training: TemplatedVocabulary<FORB>::create (TemplatedVocabulary.h:569-1008, src/FORB.cpp:24-73) ----------------------
 * Hierarchical k-means over the descriptors of n_docs documents, on the device, one tree level at a time.  It follows the
 * reference: getFeatures' order (:633-649: documents in order, features in order; every group keeps its features in ascending
 * original order); HKmeansStep (:654-831: the trivial case n <= k, the rounds until the association repeats, strict < so the
 * first centre wins a tie, recursion only for level < L and groups of more than one feature); initiateClustersKMpp (:846-925:
 * min_dist updated only where it is > 0, the exact distance sum, a seeding that stops with fewer than k centres when the sum is
 * 0, the cut drawn again while it is 0, the first index whose running sum reaches the cut); FORB::meanValue (a copy for one
 * member, otherwise bit i set iff its count >= n / 2 + n % 2); create's node numbering (a node's children together, then each
 * child's subtree, depth first); createWords (:930-950: word ids in node-id order over the nodes without children);
 * setNodeWeights (:955-1008: TF and BINARY weight 1; IDF and TF_IDF log((double)NDocs / (double)Ni), Ni the documents with a
 * feature whose transform ends in word i, computed with the host's libm from the device's integer counts; 0 where Ni == 0 and
 * for inner nodes).  Three deviations:
 *   1. Draws.  The reference consumes rand() depth first, so every node's draws depend on all earlier subtrees.  Here draw j of
 *      a node is r = mix(mix(seed ^ mix(key)) + j) >> 33 (31 bits, as rand()), mix the splitmix64 step (add 0x9E3779B97F4A7C15;
 *      z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31); the root's key is 0, child i
 *      (0-based) of the node with key K has key 21 K + i + 1.  The first centre is feature int((double)r / 2147483648.0 * n),
 *      a cut is (double)r / 2147483647.0 * dist_sum.
 *   2. Emptied cluster.  A cluster that loses all its members keeps its centre (the reference releases the cv::Mat and reads
 *      through its null pointer at the next distance); one that is empty at the end is a node without children, a word with
 *      Ni = 0.
 *   3. Round limit.  A k-means run stops after max_rounds assignment rounds (<= 0: 100; a safety limit, the reference loops
 *      for ever on a cycle) and keeps its last association.
 * Documents in the layout of orbx_extract_batch_device: document f at d_desc32 + f * capacity * 32, d_n[f] features (clamped to
 * [0, capacity]); n_docs is not bounded by the context's max_batch, n_docs * capacity by ORBX_VOC_TRAIN_MAX_SLOTS.  *out is an
 * ordinary vocabulary, ready for transform and score.  stats8 (nullable) = {nodes, words, k-means runs, most rounds of one run,
 * runs stopped by max_rounds, emptied-cluster events (centre updates that met an empty group), seedings that stopped short,
 * trivial nodes}.  d_feat_word (nullable, [n_docs][capacity]): the word every training feature descends to.  Synchronous.
 * ORBX_E_BADARG: k outside [2, 20], L outside [1, 10], a scoring or weighting type out of range, n_docs < 0, capacity < 1, null
 * pointers; ORBX_E_CAPACITY: capacity > ORBX_BOW_MAX_FEATURES or too many slots; ORBX_E_HIP: ctx == NULL with otherwise
 * well-formed arguments.  Without any feature the vocabulary is empty, as create leaves it. */
#define ORBX_VOC_TRAIN_MAX_SLOTS (1 << 30)
int orbx_vocabulary_train_device(orbx_ctx* ctx, int k, int L, int scoring, int weighting, uint64_t seed, int max_rounds, int n_docs,
                                 const uint8_t* d_desc32, const int32_t* d_n, int capacity, orbx_vocabulary** out, int32_t* stats8,
                                 uint32_t* d_feat_word);
/* The same for host memory: the documents' descriptors concatenated in desc32, doc_n[n_docs] of them each (a negative count:
 * ORBX_E_BADARG; more than ORBX_BOW_MAX_FEATURES in one document: ORBX_E_CAPACITY); feat_word (nullable) concatenated likewise.
 * Runs through the device path. */
int orbx_vocabulary_train(orbx_ctx* ctx, int k, int L, int scoring, int weighting, uint64_t seed, int max_rounds, int n_docs,
                          const uint8_t* desc32, const int32_t* doc_n, orbx_vocabulary** out, int32_t* stats8, uint32_t* feat_word);
/* Diagnostic: nodes with more than n features are seeded by the grid-wide kernels instead of one workgroup (n < 0: the default,
 * which is also the largest value taken).  Both forms give the same result; tests drive the grid-wide form on small inputs. */
int orbx_debug_voc_train_seed_grid_min(long long n);

/* transform(features, BowVector&, FeatureVector&, levelsup) for a batch of frames, device-resident, stream-ordered on the
 * context stream (the call returns once queued; results are valid after a device synchronisation): frame f's descriptors at
 * d_desc32 + f * capacity * 32, its count d_n[f] (clamped to [0, capacity]; the layout of orbx_extract_batch_device).
 * Outputs, [n_frames][capacity] entries each: d_bow_word uint32 / d_bow_value f64 (the BowVector in ascending word order,
 * d_bow_n[f] entries); d_fv_node / d_fv_feat uint32 (the FeatureVector as (node, feature) pairs in ascending order, d_fv_n[f]
 * entries); d_feat_word uint32 (each feature's word id from the descent, stopped or not, first d_n[f] entries).  d_fv_* (all
 * three or none) and d_feat_word may be NULL: without d_fv_* it is the two-argument transform.  ORBX_E_BADARG: a vocabulary of
 * another context, null required pointers, n_frames < 0, capacity < 1; ORBX_E_CAPACITY: capacity > ORBX_BOW_MAX_FEATURES. */
int orbx_bow_transform_batch_device(orbx_ctx* ctx, const orbx_vocabulary* voc, int n_frames, const uint8_t* d_desc32,
                                    const int32_t* d_n, int capacity, int levelsup, uint32_t* d_bow_word, double* d_bow_value,
                                    int32_t* d_bow_n, uint32_t* d_fv_node, uint32_t* d_fv_feat, int32_t* d_fv_n,
                                    uint32_t* d_feat_word);
/* The same for one frame in host memory (desc32 [n][32]), through the batched path; outputs host arrays of n entries (bow_*,
 * fv_*, feat_word; fv_* and feat_word nullable).  Synchronous. */
int orbx_bow_transform(orbx_ctx* ctx, const orbx_vocabulary* voc, const uint8_t* desc32, int n, int levelsup, uint32_t* bow_word,
                       double* bow_value, int32_t* bow_n, uint32_t* fv_node, uint32_t* fv_feat, int32_t* fv_n, uint32_t* feat_word);
/* L1Scoring::score(v1, v2) for pair p = frames h_first[p], h_second[p] (host arrays, each in [0, n_frames), checked before any
 * launch: ORBX_E_BADARG) of the BowVectors transform wrote (d_bow_* with the same capacity); d_score_f64 [n_pairs].
 * Stream-ordered like the transform: the call returns once queued, with one exception: when the pair list differs from the previous
 * call's on this vocabulary, the call first waits for the context stream before it uploads the list (the first call always does); a
 * caller that scores the same pairs of every batch never waits again.
 * ORBX_E_BADARG for a vocabulary whose scoring is not L1_NORM (deviation 4). */
int orbx_bow_score_batch_device(orbx_ctx* ctx, const orbx_vocabulary* voc, int n_frames, int n_pairs, const int32_t* h_first,
                                const int32_t* h_second, const uint32_t* d_bow_word, const double* d_bow_value,
                                const int32_t* d_bow_n, int capacity, double* d_score_f64);
/* The same for two BowVectors in host memory (ascending words w1 [n1] / w2 [n2] with their values), through the batched path.
 * Synchronous. */
int orbx_bow_score(orbx_ctx* ctx, const orbx_vocabulary* voc, const uint32_t* w1, const double* v1, int n1, const uint32_t* w2,
                   const double* v2, int n2, double* score);

/* ---- database: DBoW2 TemplatedDatabase::add and query ------------------------------------------------------------------------
 * (Thirdparty/DBoW2/include/DBoW2/TemplatedDatabase.h:433-464 add, :566-1113 query and the five query* it dispatches to.)
 * The BowVectors of past frames in an inverted file on the device -- row_start [words + 1], and per posting an entry id (uint32)
 * and a value (f64), every row in ascending entry id -- and, for a new BowVector, the best-scoring entries.  A database belongs
 * to one context and takes its scoring and weighting types from the vocabulary it is created with (the vocabulary itself is
 * not kept).  Bit-identical to a CPU restatement of those lines (tests/cpp/db_ref.cpp), which is itself compared with the
 * reference's compiled scoring objects: every score a query returns equals ScoringObject::score(query, entry) byte for byte.
 *   add     every vector gets the next entry id (m_nentries++), an empty one too; each (word, value) is appended to its word's row
 *   query   entry e's sum is built from the words it shares with the query in ascending word id, one sequential f64 chain
 *           that starts from the first term; entries with id < max_id take part (max_id == -1: all); the list is ordered,
 *           cut to max_results, and the final score computed after the cut:
 *             L1_NORM        term fabs(q - d) - fabs(q) - fabs(d)          listed with >= 1 common word   smallest sum first
 *                            score -sum / 2.0
 *             L2_NORM        term -q * d                                   >= 1                           smallest sum first
 *                            score sum <= -1.0 ? 1.0 : 1.0 - sqrt(1.0 + sum)
 *             CHI_SQUARE     term q + d != 0.0 ? -q * d / (q + d) : 0      >= 5 (MIN_COMMON_WORDS)        smallest sum first
 *                            (the word counts either way); score -2. * sum
 *             BHATTACHARYYA  term sqrt(q * d)                              >= 5                           largest sum first
 *             DOT_PRODUCT    term q * d, or 1 under BINARY weighting       >= 1                           largest sum first
 *           f64 divide and sqrt correctly rounded, nothing contracted.
 * Documented deviations from the reference:
 *   1. Equal sums are ordered by ascending entry id (the reference's std::sort leaves their order unspecified).
 *   2. KL is not offered: orbx_database_create returns ORBX_E_BADARG for a KL vocabulary.
 *   3. max_results must lie in [1, ORBX_DB_MAX_RESULTS]: the reference's "<= 0 means all", and a larger value, return
 *      ORBX_E_CAPACITY.
 *   4. The debug fields of Result (nWords, bhatScore, chiScore, sumCommonVi, sumCommonWi, expectedChiScore) are not produced.
 *   5. Word ids: the host forms refuse (ORBX_E_BADARG) a word id >= the vocabulary's word count and words that are not strictly
 *      ascending, where the reference indexes out of range; the device forms skip a posting whose word id is no word.
 * Not offered: the direct index (m_dfile, retrieveFeatures), save / load, allocate.
 * The batch forms read BowVectors in the layout orbx_bow_transform_batch_device writes ([n][capacity], d_bow_n clamped to
 * [0, capacity]) and are stream-ordered on the context stream: adds and queries issued in order see each other in order.  An
 * add rewrites the whole file (one pass over every posting) and reads the file's new length back once, so it returns with the
 * stream idle up to its last three kernels; a query returns once queued.
 * Common refusals: ORBX_E_BADARG for a vocabulary or database of another context, null pointers, negative counts, capacity < 1;
 * ORBX_E_CAPACITY for capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP for ctx == NULL with otherwise well-formed arguments. */
#define ORBX_DB_MAX_RESULTS 256
typedef struct orbx_database orbx_database;
int orbx_database_create(orbx_ctx* ctx, const orbx_vocabulary* voc, orbx_database** out);
/* Destroy databases before their context. */
void orbx_database_destroy(orbx_database* db);
/* clear(): no entries; the next id is 0 again. */
int orbx_database_clear(orbx_database* db);
/* size(): the number of entries (ORBX_E_BADARG for NULL). */
int orbx_database_size(const orbx_database* db);
/* add(v) for a batch: frame f becomes entry *first_entry_id + f. */
int orbx_database_add_batch_device(orbx_ctx* ctx, orbx_database* db, int n_frames, const uint32_t* d_bow_word,
                                   const double* d_bow_value, const int32_t* d_bow_n, int capacity, int32_t* first_entry_id);
/* query(vec, ret, max_results, max_id) for a batch: d_res_entry int32 / d_res_score f64, both [n_queries][max_results], best
 * first; d_res_n[q] entries are written for query q and nothing beyond them. */
int orbx_database_query_batch_device(orbx_ctx* ctx, orbx_database* db, int n_queries, const uint32_t* d_bow_word,
                                     const double* d_bow_value, const int32_t* d_bow_n, int capacity, int max_results, int max_id,
                                     int32_t* d_res_entry, double* d_res_score, int32_t* d_res_n);
/* The same for one BowVector in host memory (ascending words word [n] with their values), through the batched path as a batch
 * of one.  res_entry / res_score hold max_results entries.  More than ORBX_BOW_MAX_FEATURES words: ORBX_E_CAPACITY.
 * Synchronous. */
int orbx_database_add(orbx_ctx* ctx, orbx_database* db, const uint32_t* word, const double* value, int n, int32_t* entry_id);
int orbx_database_query(orbx_ctx* ctx, orbx_database* db, const uint32_t* word, const double* value, int n, int max_results,
                        int max_id, int32_t* res_entry, double* res_score, int32_t* res_n);
/* Diagnostic readback, synchronous: row_start [words + 1], then the postings word by word (post_entry / post_value, capacity
 * entries each; fewer than the file holds: ORBX_E_CAPACITY).  With NULL arrays only the posting count is returned.  Returns the
 * posting count. */
int64_t orbx_database_get_inverted_file(orbx_database* db, uint32_t* row_start, uint32_t* post_entry, double* post_value,
                                        int64_t capacity);
/* Diagnostic: the entries one accumulate workgroup takes (1 .. 2048) and the lists one merge workgroup takes (2 .. 8); negative
 * arguments restore the defaults, which are also the largest values (other values: ORBX_E_BADARG).  Every shape gives the same
 * result; tests drive several slices and merge rounds on small databases. */
int orbx_debug_database_shape(int entries_per_slice, int lists_per_merge);

/* ---- matching through the FeatureVector: ORBmatcher::SearchByBoW -----------------------------------------------------------
 * The step behind a database query: a keyframe KF (a candidate the database returned) is matched against a frame F, every KF
 * feature only against the F features under the same vocabulary node (Frame::mFeatVec, SlamTypes/Frame.hpp:81; what TH_LOW is
 * for, Features/ORBmatcher.hpp:56).  The reference ships no SearchByBoW; this is ORB-SLAM2's
 * SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&), bit-identical to a CPU restatement of the rules below
 * (tests/cpp/match_bow_ref.cpp):
 *   1. every matches_f[j] = -1, the 30 rotation bins empty
 *   2. the node ids present in both FeatureVectors in ascending order; a node's KF features i in ascending index, those with
 *      kf_mask[i] == 0 skipped: over the node's F features j in ascending index that no earlier KF feature took,
 *      d = popcount(desc_KF[i] ^ desc_F[j]); best1 = the smallest d, best2 = the second smallest counting duplicates (both start
 *      at 256), bestIdx = the lowest j attaining best1
 *   3. best1 <= 50 (TH_LOW) and (float)best1 < nnratio * (float)best2 (an f32 product, strict): matches_f[bestIdx] = i, and with
 *      check_orientation the match joins bin (int)roundf(rot * (30 / 360.0f)), rot = angle_KF[i] - angle_F[bestIdx] (+ 360.0f
 *      when negative), bin 30 = bin 0
 *   4. with check_orientation, ComputeThreeMaxima (Features/ORBmatcher.cpp:152-183) on the bin sizes; the matches of every other
 *      bin are set back to -1
 *   nmatches = the entries of matches_f that are not -1.
 * Documented deviations from ORB-SLAM2:
 *   1. The bin factor is the reference's corrected HISTO_LENGTH / 360.0f (Features/ORBmatcher.cpp:21-23), not 1.0f / HISTO_LENGTH.
 *   2. A match whose bin falls outside [0, 30) (an angle that is no angle) joins no bin and is kept, where the reference's
 *      matcher asserts; orbx_match_init* does the same.
 *   3. Map points are a mask (kf_mask, one byte per KF feature: 0 = no map point) and an index (matches_f holds the KF feature),
 *      not MapPoint pointers.
 * Malformed FeatureVectors: the device form skips a (node, feature) pair whose feature index is not below the frame's count, the
 * host form refuses it (ORBX_E_BADARG); a FeatureVector that is not ascending by node and feature, or that names a feature
 * twice, gives unspecified matches (and nothing worse).
 *
 * Batched and device-resident: pair p matches keyframe h_kf[p] against frame h_f[p] (host arrays, each in [0, n_frames); a frame
 * may be in any number of pairs, on either side, also paired with itself) of the arrays orbx_extract_batch_device
 * (d_kps: only angle is read; d_desc32, 16-byte aligned; d_n) and orbx_bow_transform_batch_device (d_fv_node / d_fv_feat /
 * d_fv_n) filled, same capacity and layout, so that the three calls chain without a copy.  d_kf_mask (nullable)
 * [n_frames][capacity].  d_matches_f int32 [n_pairs][capacity]: row p's first d_n[h_f[p]] entries, the rest is unspecified;
 * d_nmatches int32 [n_pairs].  Stream-ordered on the context stream like the transform.  The call returns once queued, with one
 * exception: when the pair list differs from the previous call's on this context, the call first waits for the context stream
 * before it uploads the list (the first call always does); a caller that matches the same pairs of every batch never waits again.
 * ORBX_E_BADARG: null required pointers, negative counts, capacity < 1, a pair index outside [0, n_frames) -- all checked
 * before anything touches a device; ORBX_E_CAPACITY: capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with otherwise
 * well-formed arguments.  n_pairs == 0 is ORBX_OK. */
int orbx_match_bow_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_f,
                                const orbx_keypoint* d_kps, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                                const uint32_t* d_fv_node, const uint32_t* d_fv_feat, const int32_t* d_fv_n, const uint8_t* d_kf_mask,
                                float nnratio, int check_orientation, int32_t* d_matches_f, int32_t* d_nmatches);
/* The same for one pair in host memory, through the batched path as a batch of one: the keyframe's keypoints / descriptors
 * (kf_n of them), its FeatureVector (kf_fv_n pairs) and kf_mask (nullable, kf_n bytes), then the frame's; matches_f holds f_n
 * entries.  More than ORBX_BOW_MAX_FEATURES features or pairs: ORBX_E_CAPACITY.  Synchronous. */
int orbx_match_bow(orbx_ctx* ctx, const orbx_keypoint* kf_kps, const uint8_t* kf_desc32, int kf_n, const uint32_t* kf_fv_node,
                   const uint32_t* kf_fv_feat, int kf_fv_n, const orbx_keypoint* f_kps, const uint8_t* f_desc32, int f_n,
                   const uint32_t* f_fv_node, const uint32_t* f_fv_feat, int f_fv_n, const uint8_t* kf_mask, float nnratio,
                   int check_orientation, int32_t* matches_f, int32_t* nmatches);

/* ---- matching by projection: ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) ------------------------------
 * The matcher of Tracking::TrackWithMotionModel: the last frame's map points are projected with the current frame's predicted
 * pose, each one is matched inside a window of the current frame's grid around its projection, and the matches go to
 * PoseOptimization.  The reference ships no SearchByProjection (it declares TH_HIGH for it, Features/ORBmatcher.hpp:57); this
 * is ORB-SLAM2's SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono) with
 * bMono = true, [from-knowledge], PARITY UNPINNED, bit-identical to a CPU restatement of the rules below
 * (tests/cpp/match_proj_ref.cpp).  The window search alone is pinned: it is the reference's Frame::GetFeaturesInArea
 * (SlamTypes/Frame.cpp:163-206) on the grid Frame::PosInGrid fills (:89-99), and the tests compare it with the reference's own
 * compiled code.
 *
 * Pair p: the last frame L = h_last[p], the current frame C = h_cur[p], point set h_point_set[p] whose entry i is the map point
 * of L's feature i (d_points / d_point_mask as orbx_pose_optimize_batch_device takes them), C's predicted pose d_pose_cur[p]
 * (12 floats: R row-major, then t).
 *   1. every matches_cur[j] = -1 (j over C's features), the 30 rotation bins empty
 *   2. L's features i in ascending order.  Skipped: a feature whose mask byte is 0; one with d_last_outlier[p][i] != 0
 *      (LastFrame.mvbOutlier; the array is nullable); one whose octave o is outside [0, nlevels) (sets ORBX_PROJ_BAD_INPUT)
 *   3. projection, f32, no contraction: xc = ((R0*X + R1*Y) + R2*Z) + t0, yc and zc likewise from rows 1 and 2;
 *      invz = 1.0f / zc correctly rounded; skipped when invz < 0; u = (fx*xc)*invz + cx, v = (fy*yc)*invz + cy; skipped when u or
 *      v is not finite; skipped when u < min_x || u > max_x || v < min_y || v > max_y (a value on a bound stays)
 *   4. r = th * scale[o] (an f32 product with the context's table, orbx_get_tables); the candidates are
 *      GetFeaturesInArea(u, v, r, o - 1, o + 1) over C's undistorted keypoints: PosInGrid's rounding, the cells
 *      floor((u - min_x - r) * inv) .. ceil((u - min_x + r) * inv) clamped to the grid, the level test and the strict
 *      fabs(d) < r in both coordinates, in the order cell x outer, cell y inner, ascending index inside a cell.  No candidate:
 *      skipped
 *   5. over the candidates that no EARLIER feature of L took, in that order: d = popcount(desc_i ^ desc_C[j]); best = the first
 *      candidate with the smallest d (`if (dist < bestDist)`, bestDist starting at 256).  desc_i is d_point_desc32[set][i] when
 *      that array is given (the map point's own descriptor, pMP->GetDescriptor()), otherwise L's descriptor i
 *   6. best <= 100 (TH_HIGH): matches_cur[bestIdx] = i, bestIdx is taken, and with check_orientation the match joins the bin of
 *      angle_L[i] - angle_C[bestIdx] as in SearchByBoW above
 *   7. with check_orientation, ComputeThreeMaxima and its 0.1 rule on the bin sizes; the matches of every other bin go back to -1
 *   nmatches = the entries of matches_cur that are not -1.
 * Documented deviations from ORB-SLAM2:
 *   1. The bin factor and a bin outside [0, 30): deviations 1 and 2 of SearchByBoW.
 *   2. "Taken" (matches_cur[j] >= 0) stands for `CurrentFrame.mvpMapPoints[i2]->Observations() > 0`: every map point counts as
 *      observed.
 *   3. No stereo branches: no bForward / bBackward scale windows and no mvuRight test.
 *   4. Map points are coordinates plus a mask, matches are indices (matches_cur holds L's feature, whose map point it is).
 *   5. Garbage is flagged and never followed.  u or v that is no number skips the feature (the design's comparisons would let a
 *      NaN through); a non-finite pose, or a non-finite point of a feature that step 2 keeps, sets ORBX_PROJ_NONFINITE; a frame
 *      count outside [0, capacity] is clamped and sets ORBX_PROJ_BAD_INPUT, as does an octave outside the table.  A keypoint of C
 *      whose cell is no number is in no cell.  Window cells are clamped as floats, which equals the reference wherever its
 *      float -> int conversion is defined.
 * Worst case: features of L that all claim the same candidates resolve one per round (see the kernel); the common case is a
 * handful of rounds. */
#define ORBX_PROJ_BAD_INPUT 2 /* a frame count outside [0, capacity], an octave of L outside [0, nlevels) */
#define ORBX_PROJ_NONFINITE 4 /* a non-finite pose, or a non-finite point of a feature that step 2 keeps */
typedef struct orbx_proj_result {
  int32_t status;            /* 0, or a bitmask of ORBX_PROJ_*; every field is written for every pair */
  int32_t nmatches;
  int32_t n_points;          /* features of L that survive step 2 */
  int32_t n_in_image;        /* ... and step 3 */
  int32_t n_with_candidates; /* ... and have a candidate in step 4 */
  int32_t n_displaced;       /* features whose outcome (the candidate, or none) differs from what nothing taken would give */
  int32_t n_rot_removed;     /* matches step 7 removed */
  int32_t rounds;            /* the device's rounds of claims; not comparable with a sequential statement, which reports 0 */
} orbx_proj_result;

/* Batched, device-resident, stream-ordered on the context stream.  d_kps_un / d_desc32 (16-byte aligned) / d_n: the frames, in
 * the layout of the extract calls ([n_frames][capacity]); a frame may be L in one pair and C in another, and in any number of
 * pairs.  d_points float [n_point_sets][capacity][3], d_point_mask uint8 [n_point_sets][capacity] (NULL = every entry is a
 * point), d_point_desc32 uint8 [n_point_sets][capacity][32] (NULL = L's descriptors; 16-byte aligned), d_last_outlier uint8
 * [n_pairs][capacity] (NULL = none; the layout of orbx_pose_optimize_batch_device's d_outlier), d_pose_cur float [n_pairs][12].
 * K row-major 3x3 (host, f32), bounds = C's image bounds (every C shares them, as Frame's statics), th > 0 (the design passes 15
 * and 2 * 15), check_orientation.  d_matches_cur int32 [n_pairs][capacity]: row p's first d_n[h_cur[p]] entries hold L's feature
 * index or -1, the rest is unspecified.  That is orbx_pose_optimize_batch_device's d_match: with h_frame = h_cur, the same point
 * sets and d_pose0 = d_pose_cur the two calls chain without a copy.  d_res [n_pairs].  One workgroup per pair, one launch.  The
 * call returns once queued, with the exception orbx_match_bow_batch_device has: when the pair lists differ from the previous
 * call's on this context, the call first waits for the context stream before it uploads them.
 * ORBX_E_BADARG: null required pointers, negative counts, capacity < 1, th not finite or <= 0, bounds with max <= min, a frame
 * index outside [0, n_frames), a point set outside [0, n_point_sets) -- all checked before anything touches a device;
 * ORBX_E_CAPACITY: capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with otherwise well-formed arguments.
 * n_pairs == 0 is ORBX_OK. */
int orbx_match_projection_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_last, const int32_t* h_cur,
                                       const int32_t* h_point_set, const orbx_keypoint* d_kps_un, const uint8_t* d_desc32,
                                       const int32_t* d_n, int capacity, int n_point_sets, const float* d_points,
                                       const uint8_t* d_point_mask, const uint8_t* d_point_desc32, const uint8_t* d_last_outlier,
                                       const float* d_pose_cur, const float* K, const orbx_bounds* bounds, float th,
                                       int check_orientation, int32_t* d_matches_cur, orbx_proj_result* d_res);
/* The same for one pair in host memory, through the batched path as a batch of one: the last frame (last_n features; points
 * [last_n][3]; mask, point_desc32 and last_outlier nullable, one entry per feature of L), then the current frame; pose_cur [12];
 * matches_cur holds cur_n entries.  More than ORBX_BOW_MAX_FEATURES features: ORBX_E_CAPACITY.  Synchronous. */
int orbx_match_projection(orbx_ctx* ctx, const orbx_keypoint* last_kps_un, const uint8_t* last_desc32, int last_n,
                          const orbx_keypoint* cur_kps_un, const uint8_t* cur_desc32, int cur_n, const float* points,
                          const uint8_t* mask, const uint8_t* point_desc32, const uint8_t* last_outlier, const float* pose_cur,
                          const float* K, const orbx_bounds* bounds, float th, int check_orientation, int32_t* matches_cur,
                          orbx_proj_result* res);

/* ---- matching the local map by projection: ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) ---------------
 * The second half of a tracked frame, Tracking::TrackLocalMap: SearchLocalPoints marks the map points the frame already has,
 * tests every other point of the local map with Frame::isInFrustum(pMP, 0.5), predicts its scale (MapPoint::PredictScale) and
 * matches the points in view inside a window of the frame's grid; PoseOptimization follows.  The reference ships neither
 * isInFrustum nor this overload: this is ORB-SLAM2's code, [from-knowledge], PARITY UNPINNED, bit-identical to a CPU restatement
 * of the rules below (tests/cpp/match_local_ref.cpp).  The window search alone is pinned: it is the reference's
 * Frame::GetFeaturesInArea (SlamTypes/Frame.cpp:163-206), and the tests compare it with the reference's own compiled code.
 *
 * Pair p: frame F = h_frame[p], map set s = h_map_set[p] with n_s = d_map_n[s] points, F's pose d_pose[p] (12 floats: R
 * row-major, then t), the row d_matches[p] (feature j's map point as an index into set s, or a negative value).
 *   1. the points F already has (SearchLocalPoints' first loop, with TrackWithMotionModel's clean-up), over F's features j with
 *      i = d_matches[p][j] >= 0: i >= n_s is never followed -- the entry stays, feature j counts as taken and
 *      ORBX_LOCAL_BAD_INPUT is set.  Otherwise point i is "seen" and is not searched; with d_outlier[p][j] != 0 the entry
 *      becomes -1 and feature j is free (the point stays seen: ORB-SLAM2 sets mnLastFrameSeen for a discarded outlier too),
 *      without it feature j is taken.  A negative entry is left as it is.
 *   2. isInFrustum(pMP, 0.5) for every point i that is not seen and whose mask byte is set, in ascending i; f32 without
 *      contraction unless said otherwise.  Pc = R*P + t as xc = ((R0*X + R1*Y) + R2*Z) + t0, yc and zc likewise; PcZ < 0.0f:
 *      out.  invz = 1.0f / PcZ correctly rounded; u = (fx*PcX)*invz + cx, v = (fy*PcY)*invz + cy; u or v not finite: out; u <
 *      min_x || u > max_x || v < min_y || v > max_y: out (a value on a bound stays).  The camera centre Ow_k = -((R[0][k]*t0 +
 *      R[1][k]*t1) + R[2][k]*t2); PO = P - Ow; dist = (float)sqrt((double)POx*POx + (double)POy*POy + (double)POz*POz), the
 *      products and sums in f64 in that order (cv::norm of a CV_32F vector); dist < 0.8f*minDist || dist > 1.2f*maxDist: out;
 *      viewCos = (float)(((double)POx*Nx + (double)POy*Ny + (double)POz*Nz) / (double)dist) with the normal as given;
 *      viewCos < 0.5f: out
 *   3. PredictScale: ratio = maxDist / dist (the raw mfMaxDistance; correctly rounded); a ratio that is no number sets
 *      ORBX_LOCAL_NONFINITE and drops the point; level = the number of n in [0, nlevels - 1) with ratio > scale[n] (the
 *      context's table, orbx_get_tables; scale[0] = 1).  The point is in view (mbTrackInView, nToMatch)
 *   4. r = viewCos > 0.998f ? 2.5f : 4.0f; if th != 1.0f, r *= th; the candidates are GetFeaturesInArea(u, v, r*scale[level],
 *      level - 1, level) over F's undistorted keypoints (the reference's function with its own bCheckLevels reading: PosInGrid's
 *      rounding, the clamped cell range, octave in [level - 1, level], the strict fabs(d) < r in both coordinates), in the order
 *      cell x outer, cell y inner, ascending index inside a cell.  No candidate: the point is skipped
 *   5. over the candidates that are not taken on entry and not taken by an earlier point, in that order, with d =
 *      popcount(d_map_desc32[s][i] ^ desc_F[j]): if (d < bestDist) { bestDist2 = bestDist; bestLevel2 = bestLevel; bestDist = d;
 *      bestLevel = octave_j; bestIdx = j; } else if (d < bestDist2) { bestLevel2 = octave_j; bestDist2 = d; } -- both distances
 *      start at 256, both levels at -1.  (That stream is "the two smallest under the key (d, position in the order of 4)".)
 *   6. bestDist <= 100 (TH_HIGH) is required; the point is rejected when bestLevel == bestLevel2 && (float)bestDist >
 *      nnratio*(float)bestDist2; otherwise d_matches[p][bestIdx] = i and bestIdx is taken.  This overload has no rotation
 *      histogram.
 * Documented deviations from ORB-SLAM2:
 *   1. PredictScale in table form: ORB-SLAM2 takes ceil(log(ratio) / mfLogScaleFactor) clamped to [0, nlevels - 1].  The count
 *      of table entries below the ratio is the same number except where the ratio lies within rounding of a table entry, and
 *      needs no libm on either side.
 *   2. "Taken" stands for `F.mvpMapPoints[idx]->Observations() > 0`: every map point counts as observed (deviation 2 of
 *      matching by projection above).
 *   3. No stereo branch: no mvuRight test.
 *   4. Map points are arrays plus a mask (0 = isBad() or absent), matches are indices into the pair's map set.
 *   5. Garbage is flagged and never followed.  Counts outside [0, capacity] / [0, map_capacity] are clamped and set
 *      ORBX_LOCAL_BAD_INPUT, as does an entry of d_matches >= n_s.  A non-finite pose sets ORBX_LOCAL_NONFINITE and drops every
 *      point of step 2; a point of step 2 whose position, normal or two distances hold a non-finite value sets it and is
 *      dropped, as is one whose ratio is no number.  u or v that is no number is out of the image (the design's comparisons
 *      would let a NaN through).  A keypoint whose cell is no number is in no cell; window cells are clamped as floats.
 * Translating the last-frame feature indices that orbx_match_projection* writes into map-set indices is the caller's gather
 * (map index of the last frame's feature), as is building the local map (UpdateLocalMap).
 * Worst case: points whose windows all share candidates resolve one per round (see the kernel); the common case is a handful. */
#define ORBX_LOCAL_BAD_INPUT 2 /* a count outside its capacity, an entry of d_matches beyond the map set's count */
#define ORBX_LOCAL_NONFINITE 4 /* a non-finite pose, a non-finite point / normal / distance or ratio of a point of step 2 */
#define ORBX_LOCAL_NOT_IN_VIEW 0xFF /* d_point_view */
#define ORBX_LOCAL_SEEN 0xFE
typedef struct orbx_local_result {
  int32_t status;             /* 0, or a bitmask of ORBX_LOCAL_*; every field is written for every pair */
  int32_t nmatches;           /* new matches only */
  int32_t n_points;           /* points that reach step 2: mask set, not seen */
  int32_t n_seen;             /* points some entry of d_matches names (whatever their mask) */
  int32_t n_behind;           /* step 2: PcZ < 0 */
  int32_t n_out_image;        /* ... u or v not finite or outside the bounds */
  int32_t n_out_distance;
  int32_t n_out_angle;
  int32_t n_in_view;          /* the design's nToMatch */
  int32_t n_with_candidates;  /* points in view whose window holds a feature (step 4) */
  int32_t n_over_th;          /* ... whose bestDist is above TH_HIGH (256 when every candidate is taken) */
  int32_t n_ratio_rejected;
  int32_t n_displaced;        /* points in view whose outcome (the feature, or none) differs from what they would get with only
                                 the entry's matches taken */
  int32_t n_outliers_cleared; /* entries step 1 set to -1 */
  int32_t rounds;             /* the device's rounds of claims; a sequential statement reports 0 */
} orbx_local_result;

/* Batched, device-resident, stream-ordered on the context stream.  d_kps_un / d_desc32 (16-byte aligned) / d_n: the frames, in
 * the layout of the extract and undistort calls ([n_frames][capacity]).  Map set s holds d_map_n[s] points of
 * [n_map_sets][map_capacity]: d_map_points float [3] (world position), d_map_normals float [3] (GetNormal(), used as given),
 * d_map_dist float [2] (mfMinDistance, mfMaxDistance; the kernel applies the 0.8f and 1.2f), d_map_desc32 uint8 [32] (16-byte
 * aligned), d_map_mask uint8 (NULL = every entry is a point; 0 = isBad() or absent).  A frame or a map set may be in any number
 * of pairs.  d_pose float [n_pairs][12].  K row-major 3x3 (host, f32), bounds = the frames' image bounds, th > 0 (Tracking passes
 * 1, or 5 just after a relocalisation), nnratio in (0, 1] (Tracking passes 0.8).  d_matches int32 [n_pairs][capacity], in and out
 * and required (a fresh frame is a row of -1): on exit the entry's matches, without those step 1 cleared, plus the new ones;
 * entries at and beyond the frame's count are not touched.  d_outlier uint8 [n_pairs][capacity] (NULL = none): read only,
 * orbx_pose_optimize_batch_device's output.  d_point_view uint8 [n_pairs][map_capacity] (NULL = not wanted; Tracking's
 * IncreaseVisible): for i < n_s ORBX_LOCAL_NOT_IN_VIEW, ORBX_LOCAL_SEEN, or the predicted level of a point in view.
 * d_res [n_pairs].  With map_capacity == capacity the row is orbx_pose_optimize_batch_device's d_match: with the map set as the
 * point set (d_points = d_map_points, d_point_mask = d_map_mask) and the same h_frame the two calls chain without a copy.
 * One workgroup per pair, one launch.  The call returns once queued, with the exception orbx_match_bow_batch_device has: when the
 * pair lists differ from the previous call's on this context, the call first waits for the context stream before it uploads
 * them.
 * ORBX_E_BADARG: null required pointers, negative counts, capacity or map_capacity < 1, th not finite or <= 0, nnratio not in
 * (0, 1], bounds with max <= min, a frame index outside [0, n_frames), a map set outside [0, n_map_sets) -- all checked before
 * anything touches a device; ORBX_E_CAPACITY: capacity or map_capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with
 * otherwise well-formed arguments.  n_pairs == 0 is ORBX_OK. */
int orbx_match_local_map_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_frame, const int32_t* h_map_set,
                                      const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                                      int n_map_sets, int map_capacity, const int32_t* d_map_n, const float* d_map_points,
                                      const float* d_map_normals, const float* d_map_dist, const uint8_t* d_map_desc32,
                                      const uint8_t* d_map_mask, const float* d_pose, const float* K, const orbx_bounds* bounds,
                                      float th, float nnratio, int32_t* d_matches, const uint8_t* d_outlier, uint8_t* d_point_view,
                                      orbx_local_result* d_res);
/* The same for one pair in host memory, through the batched path as a batch of one: the frame (n features), the map (map_n
 * points; map_mask nullable), pose [12]; matches [n] in and out, outlier [n] nullable, point_view [map_n] nullable.  More than
 * ORBX_BOW_MAX_FEATURES features or points: ORBX_E_CAPACITY.  Synchronous. */
int orbx_match_local_map(orbx_ctx* ctx, const orbx_keypoint* kps_un, const uint8_t* desc32, int n, int map_n,
                         const float* map_points, const float* map_normals, const float* map_dist, const uint8_t* map_desc32,
                         const uint8_t* map_mask, const float* pose, const float* K, const orbx_bounds* bounds, float th,
                         float nnratio, int32_t* matches, const uint8_t* outlier, uint8_t* point_view, orbx_local_result* res);

/* ---- matching a keyframe's points by projection: ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) --
 * The tail of Tracking::Relocalization: behind SearchByBoW, PnPsolver and PoseOptimization a candidate keyframe with fewer than
 * 50 inliers has its other map points projected into the lost frame with (th 10, ORBdist 100), the pose optimised again, and
 * with 30 to 50 inliers once more with (th 3, ORBdist 64).  The reference ships no such function: this is ORB-SLAM2's code,
 * [from-knowledge], PARITY UNPINNED, bit-identical to a CPU restatement of the rules below (tests/cpp/match_kfproj_ref.cpp).  The
 * window search alone is pinned: it is the reference's Frame::GetFeaturesInArea (SlamTypes/Frame.cpp:163-206), and the tests
 * compare it with the reference's own compiled code.
 *
 * Pair p: keyframe KF = h_kf[p] (n_K features), current frame C = h_cur[p], point set s = h_point_set[p] whose entry i is the map
 * point of KF's feature i (the layout of matching by projection: d_points, d_point_mask), C's pose d_pose[p] (12 floats: R
 * row-major, then t), the row d_matches[p] (C's feature j -> an index into set s, or a negative value; read and written).
 *   1. what C already has (sAlreadyFound, and CurrentFrame.mvpMapPoints), over C's features j with i = d_matches[p][j] >= 0:
 *      i >= n_K is never followed -- the entry stays, feature j counts as taken and ORBX_KFPROJ_BAD_INPUT is set.  Otherwise point
 *      i is "found" and is not searched; with d_outlier[p][j] != 0 the entry becomes -1 and feature j is free (the point stays
 *      found: Relocalization fills sFound from the PnP inliers before PoseOptimization and clears the outliers' mvpMapPoints
 *      after it), without it feature j is taken.  d_outlier == NULL is Relocalization's second use: sFound is rebuilt from
 *      mvpMapPoints, nothing is cleared.  A negative entry is left as it is.
 *   2. the points searched: KF's features i in ascending order whose mask byte is set and whose point is not found; f32 without
 *      contraction.  Pc = R*P + t as xc = ((R0*X + R1*Y) + R2*Z) + t0, yc and zc likewise; invz = 1.0f / zc correctly rounded;
 *      u = (fx*xc)*invz + cx, v = (fy*yc)*invz + cy.  THERE IS NO DEPTH TEST, as in ORB-SLAM2's overload: a point behind the
 *      camera (zc < 0.0f) whose (u, v) lands inside the bounds goes on (counted in n_behind_kept).  u or v not finite: skipped;
 *      u < min_x || u > max_x || v < min_y || v > max_y: skipped (a value on a bound stays).
 *   3. Ow_k = -((R[0][k]*t0 + R[1][k]*t1) + R[2][k]*t2); PO = P - Ow; dist3D = (float)sqrt((double)POx*POx + (double)POy*POy +
 *      (double)POz*POz), the products and sums in f64 in that order (cv::norm of a CV_32F vector); dist3D < 0.8f*minDist ||
 *      dist3D > 1.2f*maxDist: skipped (d_point_dist holds the raw mfMinDistance, mfMaxDistance).  No viewing-angle test, no
 *      normals.  level = PredictScale in table form on ratio = maxDist / dist3D (correctly rounded): the number of n in
 *      [0, nlevels - 1) with ratio > scale[n]; a ratio that is no number sets ORBX_KFPROJ_NONFINITE and drops the point.
 *   4. r = th * scale[level]; the candidates are GetFeaturesInArea(u, v, r, level - 1, level + 1) over C's undistorted keypoints
 *      (the reference's function: PosInGrid's rounding, the clamped cell range, octave in [level - 1, level + 1], the strict
 *      fabs(d) < r in both coordinates), in the order cell x outer, cell y inner, ascending index inside a cell.  No candidate:
 *      the point is skipped.
 *   5. over the candidates that are not taken, neither on entry nor by an earlier point of this call, in that order, with d =
 *      popcount(desc_i ^ desc_C[j]): the first smallest wins (dist < bestDist, starting from 256).  desc_i is
 *      d_point_desc32[s][i] when that array is given (MapPoint::GetDescriptor), KF's descriptor i otherwise.  No second-best, no
 *      ratio test.
 *   6. bestDist <= orb_dist: d_matches[p][bestIdx] = i and bestIdx is taken.  With check_orientation the match joins the bin of
 *      angle_KF[i] - angle_C[bestIdx] (the corrected factor and the kept out-of-range bin of matching through the
 *      FeatureVector).
 *   7. with check_orientation, ComputeThreeMaxima and its 0.1 rule over the NEW matches only; the new matches of the losing bins
 *      go back to -1 (the entry's matches never vote and never go).  nmatches = the new matches that remain.
 * Documented deviations from ORB-SLAM2:
 *   1. PredictScale in table form (deviation 1 of matching the local map by projection).
 *   2. "Taken" is CurrentFrame.mvpMapPoints[i2] != NULL as in ORB-SLAM2: this overload makes no Observations() test, so the
 *      deviation that matching by projection and matching the local map state for it does not arise here.
 *   3. Map points are arrays plus a mask (0 = NULL or isBad()), matches are indices into the pair's point set.
 *   4. Garbage is flagged and never followed.  Counts outside [0, capacity] are clamped and set ORBX_KFPROJ_BAD_INPUT, as does an
 *      entry of d_matches >= n_K.  A non-finite pose sets ORBX_KFPROJ_NONFINITE and drops every point of rule 2; a point of rule
 *      2 whose position or two distances hold a non-finite value sets it and is dropped, as is one whose ratio is no number.  u
 *      or v that is no number is out of the image.  A keypoint whose cell is no number is in no cell; window cells are clamped
 *      as floats.
 *   5. orb_dist is accepted in [0, 256] (0 accepts only an identical descriptor; 255 and 256 accept every candidate but one at
 *      distance 256, which `dist < bestDist` never picks).
 * Worst case: points whose windows all share candidates within orb_dist resolve one per round (see the kernel). */
#define ORBX_KFPROJ_BAD_INPUT 2 /* a count outside its capacity, an entry of d_matches beyond the keyframe's count */
#define ORBX_KFPROJ_NONFINITE 4 /* a non-finite pose, a non-finite point / distance or ratio of a point of rule 2 */
typedef struct orbx_kfproj_result {
  int32_t status;             /* 0, or a bitmask of ORBX_KFPROJ_*; every field is written for every pair */
  int32_t nmatches;           /* new matches that remain behind rule 7 */
  int32_t n_points;           /* points that reach rule 2: mask set, not found */
  int32_t n_found;            /* points some entry of d_matches names (whatever their mask) */
  int32_t n_behind_kept;      /* rule 2: zc < 0 with (u, v) inside the bounds -- the point goes on to rule 3 all the same */
  int32_t n_out_image;        /* ... u or v not finite or outside the bounds */
  int32_t n_out_distance;
  int32_t n_with_candidates;  /* searched points whose window holds a feature (rule 4) */
  int32_t n_over_dist;        /* ... whose bestDist is above orb_dist (256 when every candidate is taken) */
  int32_t n_displaced;        /* searched points whose pick (the feature, or none) differs from what they would get with only
                                 the entry's matches taken */
  int32_t n_rot_removed;      /* rule 7 */
  int32_t n_outliers_cleared; /* entries rule 1 set to -1 */
  int32_t rounds;             /* the device's rounds of claims; a sequential statement reports 0 */
} orbx_kfproj_result;

/* Batched, device-resident, stream-ordered on the context stream.  d_kps_un / d_desc32 (16-byte aligned) / d_n: the frames, in
 * the layout of the extract and undistort calls ([n_frames][capacity]); a frame may be a keyframe in one pair and a current frame
 * in another.  Point set s of [n_point_sets][capacity]: d_points float [3], d_point_mask uint8 (NULL = every entry is a point),
 * d_point_desc32 uint8 [32] (16-byte aligned; NULL = the keyframe's own descriptors), d_point_dist float [2] (mfMinDistance,
 * mfMaxDistance; the kernel applies the 0.8f and 1.2f; required).  d_pose float [n_pairs][12].  K row-major 3x3 (host, f32),
 * bounds = the frames' image bounds, th > 0 (Relocalization passes 10, then 3), orb_dist in [0, 256] (100, then 64).  d_matches
 * int32 [n_pairs][capacity], in and out and required: it is matching through the FeatureVector's d_matches_f with the keyframe's
 * map points as the point set -- the row orbx_match_bow_batch_device and orbx_pnp_solve_batch_device write and
 * orbx_pose_optimize_batch_device reads as d_match -- so SearchByBoW -> PnP -> pose -> this call -> pose runs on one row without
 * a gather.  Entries at and beyond C's count are not touched.  d_outlier uint8 [n_pairs][capacity] (NULL = none): read only,
 * orbx_pose_optimize_batch_device's output.  d_res [n_pairs].
 * One workgroup per pair, one launch.  The call returns once queued, with the exception orbx_match_bow_batch_device has: when the
 * pair lists differ from the previous call's on this context, the call first waits for the context stream before it uploads
 * them.
 * ORBX_E_BADARG: null required pointers, negative counts, capacity < 1, th not finite or <= 0, orb_dist outside [0, 256], bounds
 * with max <= min, a frame index outside [0, n_frames), a point set outside [0, n_point_sets) -- all checked before anything
 * touches a device; ORBX_E_CAPACITY: capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with otherwise well-formed
 * arguments.  n_pairs == 0 is ORBX_OK. */
int orbx_match_keyframe_projection_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf, const int32_t* h_cur,
                                                const int32_t* h_point_set, const orbx_keypoint* d_kps_un, const uint8_t* d_desc32,
                                                const int32_t* d_n, int capacity, int n_point_sets, const float* d_points,
                                                const uint8_t* d_point_mask, const uint8_t* d_point_desc32, const float* d_point_dist,
                                                const float* d_pose, const float* K, const orbx_bounds* bounds, float th, int orb_dist,
                                                int check_orientation, int32_t* d_matches, const uint8_t* d_outlier,
                                                orbx_kfproj_result* d_res);
/* The same for one pair in host memory, through the batched path as a batch of one: the keyframe (kf_n features; points, point_dist
 * per feature; mask, point_desc32 nullable), the current frame (cur_n features), pose [12]; matches [cur_n] in and out, outlier
 * [cur_n] nullable.  More than ORBX_BOW_MAX_FEATURES features: ORBX_E_CAPACITY.  Synchronous. */
int orbx_match_keyframe_projection(orbx_ctx* ctx, const orbx_keypoint* kf_kps_un, const uint8_t* kf_desc32, int kf_n,
                                   const orbx_keypoint* cur_kps_un, const uint8_t* cur_desc32, int cur_n, const float* points,
                                   const uint8_t* mask, const uint8_t* point_desc32, const float* point_dist, const float* pose,
                                   const float* K, const orbx_bounds* bounds, float th, int orb_dist, int check_orientation,
                                   int32_t* matches, const uint8_t* outlier, orbx_kfproj_result* res);

/* ---- loop closing: matching under a similarity (ORBmatcher::SearchBySim3) ------------------------------------------------------
 * Behind Sim3Solver ("loop closing: Sim3 RANSAC") LoopClosing::ComputeSim3 widens the inlier set: ORBmatcher::SearchBySim3(pKF1,
 * pKF2, vpMatches12, s12, R12, t12, th = 7.5) projects KF1's unmatched map points into KF2 under T21 and KF2's into KF1 under
 * T12, picks the nearest descriptor in a window each way, and keeps a pair where both directions agree.  The reference tree ships
 * no SearchBySim3: the rules restate ORB-SLAM2's ORBmatcher.cc [from-knowledge], PARITY UNPINNED.  The device equals the CPU
 * restatement in tests/cpp/sim3_ref.cpp byte for byte.
 *
 * Rules.
 *  1. vbAlreadyMatched1[i1] = row[i1] >= 0; vbAlreadyMatched2[row[i1]] = true when that index is below KF2's count.
 *  2. Direction 1 -> 2.  For every feature i1 of KF1 whose point mask is set (no mask: every feature) and that is not already
 *     matched: p3Dc1 = R1w * X + t1w; p3Dc2 = sR21 * p3Dc1 + t21 with sR21 = (1 / s12) * R12^T and t21 = -sR21 * t12.  Skip when
 *     z < 0 (z == 0 goes on and fails the next test).  invz = 1 / z, u = fx * (x * invz) + cx, v = fy * (y * invz) + cy; skip
 *     unless IsInImage: u >= min_x, u < max_x, v >= min_y, v < max_y.  dist3D = |p3Dc2|; skip when dist3D < 0.8f * min or >
 *     1.2f * max of the point's d_point_dist.  level = PredictScale in the table form of the local-map matcher (the number of
 *     scale factors below max / dist3D, among the first nlevels - 1); radius = th * scaleFactor[level].
 *     KeyFrame::GetFeaturesInArea(u, v, radius) in KF2 -- the pinned Frame::GetFeaturesInArea without level bounds; the
 *     arithmetic is the same -- then the candidates with octave in [level - 1, level]; the first with the smallest descriptor
 *     distance wins (dist < bestDist from INT_MAX: a distance of 256 can win); when bestDist <= orb_dist, vnMatch1[i1] = bestIdx.
 *     No "taken" rule, no ratio test, no orientation histogram.
 *  3. Direction 2 -> 1: the mirror image over KF2's points that are not already matched, with sR12 = s12 * R12 and t12,
 *     searching KF1; it gives vnMatch2.
 *  4. Agreement, i1 ascending: when vnMatch1[i1] = i2 >= 0 and vnMatch2[i2] == i1, row[i1] = i2 and it counts in n_found.
 *     Entries already >= 0 are never changed.
 * Expression types: f32 as the reference's cv::Mat, every three-term row sum ((a + b) + c) + t; sR12 an f32 product; 1.0 / s12
 * taken in f64, times R12^T, rounded to f32; t21's sum in f32; dist3D the f32 of an f64 square root of f64 squares.
 *
 * Documented deviations: (1) PredictScale is the table walk, not ceil(log(ratio) / log(scaleFactor)); (2) map points are arrays
 * plus a mask, indexed by their keyframe's feature (GetIndexInKeyFrame is the identity), their descriptors d_point_desc32 or,
 * without it, the feature's own; (3) orb_dist in [0, 256]; (4) n_with_candidates counts points with a candidate inside the
 * octave window (the reference tests the unfiltered list, which changes no match); (5) garbage is flagged and dropped: a count
 * outside [0, capacity] (clamped) or an entry of the row >= KF2's count (ORBX_MSIM3_BAD_INPUT: the entry stays and is followed
 * nowhere); a non-finite point, distance or ratio (ORBX_MSIM3_NONFINITE: the point is dropped); a non-finite pose or
 * similarity, or s12 <= 0: ORBX_MSIM3_NONFINITE, every point is dropped and the row stays as it came. */
#define ORBX_MSIM3_BAD_INPUT 2 /* a count outside its capacity, an entry of d_matches beyond KF2's count */
#define ORBX_MSIM3_NONFINITE 4 /* a non-finite pose, similarity (or s12 <= 0), point, distance or ratio */
typedef struct orbx_msim3_result {
  int32_t status;             /* 0, or a bitmask of ORBX_MSIM3_*; every field is written for every pair */
  int32_t n_found;            /* nFound: entries rule 4 wrote */
  int32_t n_points_12;        /* direction 1 -> 2: points searched for (mask set, not already matched) */
  int32_t n_behind_12;        /* ... z < 0 */
  int32_t n_out_image_12;     /* ... not IsInImage */
  int32_t n_out_distance_12;
  int32_t n_with_candidates_12;
  int32_t n_over_dist_12;     /* ... bestDist above orb_dist */
  int32_t n_points_21, n_behind_21, n_out_image_21, n_out_distance_21, n_with_candidates_21, n_over_dist_21; /* direction 2 -> 1 */
  int32_t n_one_sided;        /* vnMatch1 picks that vnMatch2 does not return */
  int32_t reserved;
} orbx_msim3_result;

/* Batched, device-resident, stream-ordered on the context stream.  Pair p: KF1 = h_kf1[p], KF2 = h_kf2[p], their point sets
 * h_set1[p], h_set2[p] (d_points float [n_point_sets][capacity][3], d_point_mask uint8 or NULL, d_point_desc32 uint8
 * [n_point_sets][capacity][32] 16-byte aligned or NULL, d_point_dist float [n_point_sets][capacity][2] = mfMinDistance,
 * mfMaxDistance: the kernel applies 0.8f and 1.2f), each indexed by its own keyframe's feature.  d_pose float [n_frames][12]
 * (Tcw per frame) and d_sim3 float [n_pairs][13] (R12, t12, s12) as orbx_sim3_solve_batch_device takes and writes them.  K
 * row-major 3x3 (host, f32), bounds = the keyframes' image bounds, th > 0 (LoopClosing passes 7.5), orb_dist in [0, 256]
 * (TH_HIGH = 100).  d_matches int32 [n_pairs][capacity], in and out: the solver's d_match_inliers.  d_res [n_pairs].  One
 * workgroup per pair, one launch; dynamic LDS sized from the capacity (110.0 KB at ORBX_BOW_MAX_FEATURES).  The call returns once
 * queued, except that a pair list that differs from the previous call's first waits for the context stream.
 * ORBX_E_BADARG: null required pointers, negative counts, capacity < 1, th not positive, orb_dist outside [0, 256], bounds with
 * max <= min, an index outside its range; ORBX_E_CAPACITY: capacity > ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with
 * otherwise well-formed arguments -- all checked before anything touches a device.  n_pairs == 0 is ORBX_OK. */
int orbx_match_sim3_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf1, const int32_t* h_kf2,
                                 const int32_t* h_set1, const int32_t* h_set2, const orbx_keypoint* d_kps_un, const uint8_t* d_desc32,
                                 const int32_t* d_n, int capacity, int n_point_sets, const float* d_points,
                                 const uint8_t* d_point_mask, const uint8_t* d_point_desc32, const float* d_point_dist,
                                 const float* d_pose, const float* d_sim3, const float* K, const orbx_bounds* bounds, float th,
                                 int orb_dist, int32_t* d_matches, orbx_msim3_result* d_res);
/* The same for one pair in host memory, through the batched path as a batch of one: KF1 (n1 features; points1, point_dist1 per
 * feature; mask1, point_desc1 nullable; pose1 [12]), then KF2; the masks are given together or not at all, and so are the point
 * descriptors; sim3 [13]; matches12 [n1] in and out.  Synchronous. */
int orbx_match_sim3(orbx_ctx* ctx, const orbx_keypoint* kps_un1, const uint8_t* desc1, int n1, const float* points1,
                    const uint8_t* mask1, const uint8_t* point_desc1, const float* point_dist1, const float* pose1,
                    const orbx_keypoint* kps_un2, const uint8_t* desc2, int n2, const float* points2, const uint8_t* mask2,
                    const uint8_t* point_desc2, const float* point_dist2, const float* pose2, const float* sim3, const float* K,
                    const orbx_bounds* bounds, float th, int orb_dist, int32_t* matches12, orbx_msim3_result* res);

/* ---- growing the map: LocalMapping::CreateNewMapPoints ---------------------------------------------------------------------------
 * The one step that makes map points after the Initializer's first pair: a new keyframe KF1 is matched against a covisible
 * neighbour KF2 along the epipolar lines (ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo = false),
 * monocular), and every match is triangulated and gated on parallax, depth, reprojection error and scale.  The reference ships
 * neither function: this is ORB-SLAM2's code, [from-knowledge], PARITY UNPINNED, bit-identical to a CPU restatement of the rules
 * below (tests/cpp/tri_ref.cpp; the arithmetic is csrc/orbx_tri_math.inc on both sides, the walk is written twice) and equal in
 * every discrete outcome to an independent numpy statement away from the thresholds (tests/test_tri_host.py).
 * f32 without contraction unless stated; a matrix product is "gemm on CV_32F" as in the Initializer: the products and their sum
 * in f64 in ascending k, one rounding.  Poses are Tcw per FRAME: d_pose float [n_frames][12], R row-major, then t.
 *
 * orbx_match_triangulation*, pair p = (KF1 = h_kf1[p], KF2 = h_kf2[p]):
 *   1. from the two poses and K: R12 = R1w * R2w^T; t12 = -R12 * t2w + t1w; F12 = K^-T * [t12]x * R12 * K^-1, the three products
 *      left to right; Ow = -Rcw^T * tcw for both keyframes (KeyFrame::SetPose's association); C2 = R2w * Ow1 + t2w;
 *      invz = 1.0f / C2z; ex = (fx * C2x) * invz + cx, ey likewise; baseline = (float)sqrt of the f64 sum of squares of Ow2 - Ow1.
 *   2. every matches12[i] = -1, the 30 rotation bins empty.  The node ids present in both FeatureVectors in ascending order; a
 *      node's KF1 features i in ascending index, those with mask[KF1][i] != 0 (the feature already has a map point) skipped.
 *   3. for each remaining i (a "query"): a = (x1 * F00 + y1 * F10) + F20, b and c likewise from columns 1 and 2; bestDist = 50
 *      (TH_LOW), bestIdx = -1.  Over the node's KF2 features j in ascending index that no earlier KF1 feature of this call took
 *      and whose mask[KF2][j] == 0, d = popcount(desc1[i] ^ desc2[j]); d > 50 || d > bestDist: skipped -- the test is NOT strict,
 *      so among equal distances the LAST passing candidate wins (the opposite of SearchByBoW).  Then
 *        dx = ex - x2, dy = ey - y2; dx * dx + dy * dy < 100.0f * scale[octave2]: skipped (too close to the epipole);
 *        CheckDistEpipolarLine: num = (a * x2 + b * y2) + c, den = a * a + b * b; den == 0: rejected; accepted iff
 *        num * num / den < 3.84f * sigma2[octave2];
 *      on accept bestIdx = j, bestDist = d.
 *   4. bestIdx >= 0: matches12[i] = bestIdx, bestIdx is taken, and with check_orientation the match joins the bin of
 *      angle1[i] - angle2[bestIdx] (the corrected factor and the kept out-of-range bin of SearchByBoW's deviations 1 and 2).
 *   5. with check_orientation, ComputeThreeMaxima and its 0.1 rule; the losing bins' matches go back to -1.  nmatches = the
 *      entries that remain.
 * Optional gate (CreateNewMapPoints' ratioBaselineDepth): with d_median_depth (float [n_frames], ComputeSceneMedianDepth(2) of
 * each keyframe; NULL = no gate), baseline / d_median_depth[KF2] < 0.01f refuses the pair: ORBX_TRI_LOW_BASELINE, rules 2-5 do
 * not run, its row is all -1.  A median that is no positive finite number is garbage: ORBX_TRI_BAD_INPUT is set and the pair is
 * matched without the gate.
 * Documented deviations from ORB-SLAM2:
 *   1. K^-1 is the closed form (1/fx, 0, -cx/fx; 0, 1/fy, -cy/fy; 0, 0, 1), f32; ORB-SLAM2 calls cv::Mat::inv.
 *   2. The bin factor and the out-of-range bin: deviations 1 and 2 of SearchByBoW.
 *   3. The counters n_with_candidates, n_epipole_rejected and n_epiline_rejected are taken over every free, unmasked candidate
 *      with d <= 50, whatever bestDist was when the walk reached it: they do not depend on the order of the walk.
 *   4. baseline == 0 (a keyframe paired with itself) is refused as ORBX_TRI_ZERO_BASELINE: the epipole and F12 of such a pair are
 *      rounding noise; the record holds zeros in their place.
 *   5. Garbage is flagged and never followed: counts outside [0, capacity] are clamped and set ORBX_TRI_BAD_INPUT; a FeatureVector
 *      entry naming no feature is skipped; a non-finite pose sets ORBX_TRI_NONFINITE and matches nothing; a candidate with d <= 50
 *      whose octave is outside [0, nlevels) sets ORBX_TRI_BAD_INPUT and is skipped.  A FeatureVector that is not ascending gives
 *      unspecified matches (and nothing worse).
 *   6. Pairs are independent.  In ORB-SLAM2 a point made with one neighbour takes KF1's feature out of the next neighbour's
 *      search; here two pairs with the same KF1 may both triangulate feature i (SearchInNeighbors fuses such duplicates later;
 *      not part of this library).  A caller that wants the reference's order issues the neighbours in successive calls and
 *      updates the mask between them. */
#define ORBX_TRI_BAD_INPUT 2
#define ORBX_TRI_NONFINITE 4
#define ORBX_TRI_LOW_BASELINE 8
#define ORBX_TRI_ZERO_BASELINE 16
typedef struct orbx_tri_match_result {
  int32_t status;              /* 0, or a bitmask of ORBX_TRI_*; every field is written for every pair */
  int32_t nmatches;            /* matches that remain behind rule 5 */
  int32_t n_queries;           /* KF1 features of common nodes that have no map point (rule 3) */
  int32_t n_with_candidates;   /* ... with a free, unmasked KF2 feature of the node at d <= 50 */
  int32_t n_epipole_rejected;  /* such (i, j) the epipole test skipped */
  int32_t n_epiline_rejected;  /* such (i, j) CheckDistEpipolarLine rejected */
  int32_t n_rot_removed;       /* rule 5 */
  float baseline, ex, ey;      /* rule 1 */
  float F12[9];                /* row-major */
} orbx_tri_match_result;

/* Batched, device-resident, stream-ordered on the context stream.  d_kps_un / d_desc32 (16-byte aligned) / d_n and d_fv_node /
 * d_fv_feat / d_fv_n: the frames as the extract, undistort and bag-of-words calls leave them ([n_frames][capacity]); a frame may
 * be in any number of pairs, on either side.  d_mask uint8 [n_frames][capacity] (NULL = no feature has a map point): != 0 = the
 * feature already has one.  K row-major 3x3 (host, f32; finite, fx and fy > 0).  The scale and sigma2 tables are the context's.
 * d_matches12 int32 [n_pairs][capacity], indexed by KF1's feature -- the Initializer's and the bundle adjustment's matches12
 * layout; the whole row is written.  d_res [n_pairs].
 * One workgroup per pair, one launch.  The call returns once queued, with the exception orbx_match_bow_batch_device has: when the
 * pair list differs from the previous call's on this context, the call first waits for the context stream.
 * ORBX_E_BADARG: null required pointers, negative counts, capacity < 1, a pair index outside [0, n_frames), K not finite or
 * without positive focal lengths -- all checked before anything touches a device; ORBX_E_CAPACITY: capacity >
 * ORBX_BOW_MAX_FEATURES; ORBX_E_HIP: ctx == NULL with otherwise well-formed arguments.  n_pairs == 0 is ORBX_OK. */
int orbx_match_triangulation_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf1, const int32_t* h_kf2,
                                          const orbx_keypoint* d_kps_un, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
                                          const uint32_t* d_fv_node, const uint32_t* d_fv_feat, const int32_t* d_fv_n,
                                          const uint8_t* d_mask, const float* d_pose, const float* K, const float* d_median_depth,
                                          int check_orientation, int32_t* d_matches12, orbx_tri_match_result* d_res);
/* The same for one pair in host memory, through the batched path as a batch of one: KF1 (n1 features, fv_n1 FeatureVector pairs,
 * mask1 nullable, pose1 [12]), then KF2; median_depth2 <= 0 or not a number = no gate asked for (+infinity is passed on and is
 * flagged as the batch form flags it); matches12 holds n1 entries.  A
 * FeatureVector that names a feature the keyframe does not have: ORBX_E_BADARG.  More than ORBX_BOW_MAX_FEATURES features or
 * pairs: ORBX_E_CAPACITY.  Synchronous. */
int orbx_match_triangulation(orbx_ctx* ctx, const orbx_keypoint* kps_un1, const uint8_t* desc1, int n1, const uint32_t* fv_node1,
                             const uint32_t* fv_feat1, int fv_n1, const uint8_t* mask1, const float* pose1,
                             const orbx_keypoint* kps_un2, const uint8_t* desc2, int n2, const uint32_t* fv_node2,
                             const uint32_t* fv_feat2, int fv_n2, const uint8_t* mask2, const float* pose2, const float* K,
                             float median_depth2, int check_orientation, int32_t* matches12, orbx_tri_match_result* res);

/* orbx_triangulate_matches*: the body of CreateNewMapPoints' loop behind the matcher, for each i with j = matches12[i] >= 0 (j
 * not below KF2's count, or an octave outside [0, nlevels): ORBX_TRI_BAD_INPUT, the entry is not followed or counted):
 *   1. xn = ((x - cx) * invfx, (y - cy) * invfy, 1) for both, invfx = 1.0f / fx; ray = Rwc * xn; cos = (float)(ray1 . ray2 /
 *      (|ray1| * |ray2|)) in f64; kept iff cos > 0 && cos < 0.9998f (the monocular branch), else n_low_parallax.
 *   2. A's four rows are xn.x * T.row(2) - T.row(0) and xn.y * T.row(2) - T.row(1) for both cameras (T = [R | t], f32); x3D = the
 *      right singular vector of A's smallest singular value (the f64 one-sided Jacobi of orbx_check_rt), rounded to f32;
 *      x3D[3] == 0 (or a value that is no number): n_w_zero; otherwise x3D = x3D[0..2] / x3D[3].
 *   3. z = (float)(R.row(2) . x3D + tz) with the dot product in f64; z1 <= 0: n_behind_1; z2 <= 0: n_behind_2.
 *   4. per view x, y like z; invz = 1.0f / z; u = (fx * x) * invz + cx, v likewise; errX * errX + errY * errY >
 *      5.991f * sigma2[octave]: n_reproj_1, then n_reproj_2.
 *   5. dist1 = |x3D - Ow1| (cv::norm: f64 inside), dist2 likewise; either 0: n_zero_dist.  ratioDist = dist2 / dist1, ratioOctave =
 *      scale[octave1] / scale[octave2], ratioFactor = 1.5f * scaleFactor; ratioDist * ratioFactor < ratioOctave || ratioDist >
 *      ratioOctave * ratioFactor: n_scale.
 *   6. a kept match is a map point at KF1's feature i: d_points[i] = x3D, d_point_mask[i] = 1, d_point_normal[i] =
 *      ((x3D - Ow1) / dist1 + (x3D - Ow2) / dist2) / 2.0f (UpdateNormalAndDepth with two observations), d_point_dist[i] =
 *      (mfMinDistance, mfMaxDistance) = (max / scale[nlevels - 1], max = dist1 * scale[octave1]): KF1 is the reference keyframe.
 *      Every other entry of the row: mask 0 and zeros.
 * All four arrays are [n_pairs][capacity], indexed by KF1's feature, so pair p's row is a point set for
 * orbx_match_keyframe_projection* / orbx_pose_optimize* with KF1 as the keyframe.  With two observations
 * ComputeDistinctiveDescriptors picks KF1's descriptor: that is the consumers' d_point_desc32 == NULL convention, and no
 * descriptor array is written.
 * Documented deviations from ORB-SLAM2: cv::SVD on a CV_32F matrix is the project's f64 Jacobi, as in orbx_check_rt (no OpenCV
 * to pin against); x3D / x3D[3] is an f32 division; the normal's mean is taken in f32 in the order above; deviation 6 above.
 * A non-finite pose sets ORBX_TRI_NONFINITE and makes no point; a keyframe paired with itself has parallel rays and makes none. */
typedef struct orbx_tri_result {
  int32_t status;    /* 0, or a bitmask of ORBX_TRI_BAD_INPUT / ORBX_TRI_NONFINITE */
  int32_t n_matches; /* entries of matches12 that are followed */
  int32_t n_points;  /* ... that became map points */
  int32_t n_low_parallax, n_w_zero, n_behind_1, n_behind_2, n_reproj_1, n_reproj_2, n_zero_dist, n_scale; /* one per gate */
} orbx_tri_result;

/* Batched, device-resident, stream-ordered on the context stream; d_matches12 is orbx_match_triangulation_batch_device's (or any
 * matches12 in that layout).  The same refusals as that call.  Several workgroups per pair, one launch. */
int orbx_triangulate_matches_batch_device(orbx_ctx* ctx, int n_frames, int n_pairs, const int32_t* h_kf1, const int32_t* h_kf2,
                                          const orbx_keypoint* d_kps_un, const int32_t* d_n, int capacity, const float* d_pose,
                                          const float* K, const int32_t* d_matches12, float* d_points, uint8_t* d_point_mask,
                                          float* d_point_normal, float* d_point_dist, orbx_tri_result* d_res);
/* The same for one pair in host memory: points [n1][3], point_mask [n1], point_normal [n1][3], point_dist [n1][2].  Synchronous. */
int orbx_triangulate_matches(orbx_ctx* ctx, const orbx_keypoint* kps_un1, int n1, const float* pose1, const orbx_keypoint* kps_un2,
                             int n2, const float* pose2, const float* K, const int32_t* matches12, float* points, uint8_t* point_mask,
                             float* point_normal, float* point_dist, orbx_tri_result* res);

/* ---- measurement hooks (bench.py; HIP events on the ctx stream) ---------------------------- */
#define ORBX_STAGE_PYRAMID 0
#define ORBX_STAGE_FAST 1
#define ORBX_STAGE_SELECT 2 /* quadtree selection incl. its transfers */
#define ORBX_STAGE_DESCRIBE 3
#define ORBX_STAGE_MATCH 4
#define ORBX_STAGE_COUNT 5
/* enable: record hipEvents around every stage; accumulated device ms and launch counts since the
 * last reset are returned by orbx_profile_get (arrays of ORBX_STAGE_COUNT). */
int orbx_profile_enable(orbx_ctx* ctx, int on);
/* the same for a subset of the stages (bit s = ORBX_STAGE_s): every bracketed stage costs two event records on its stream */
int orbx_profile_stages(orbx_ctx* ctx, unsigned stage_mask);
int orbx_profile_reset(orbx_ctx* ctx);
int orbx_profile_get(orbx_ctx* ctx, double* ms, int64_t* launches);

/* ---- several MI355X from one host process ---------------------------------------- */
/* One orbx_ctx per device; a batch is cut into contiguous even-sized blocks, one per device (consecutive pairs (2k, 2k + 1)
 * never straddle devices); the only exchange is an ncclAllGather of the per-frame keypoint counts over xGMI.  RCCL is loaded
 * with dlopen when a context with more than one device is created (ORBX_E_RCCL if that fails); device ids must be distinct.
 * ORBX_MULTI_FORCE_RCCL=1 in the environment makes a ONE-device context go through RCCL as well (dlopen, ncclCommInitAll(1),
 * grouped ncclAllGather on the collective stream, ncclCommDestroy): the way to exercise these code paths on a one-GPU box.
 * If a device fails to queue its block of a batch, the batches issued before it are still completed as documented below
 * (blocks waited for, counts gathered into their counts_all) before the call returns the error; only the partly issued batch
 * is dropped. */
typedef struct orbx_multi orbx_multi;
int orbx_multi_create(const orbx_params* params, int n_devices, const int* device_ids, int max_width, int max_height,
                      int max_batch_per_device, orbx_multi** out);
void orbx_multi_destroy(orbx_multi* m);
int orbx_multi_size(const orbx_multi* m);
orbx_ctx* orbx_multi_ctx(orbx_multi* m, int r); /* device r's context, for every other call of this header */
const char* orbx_multi_last_error(const orbx_multi* m);
/* the block [*lo, *hi) of a batch of n_frames that device r of n_devices owns */
int orbx_multi_shard_range(int n_frames, int n_devices, int r, int* lo, int* hi);
/* d_*[r] = device r's arrays for ITS block (frames already resident in its HBM; layout of orbx_extract_match_batch_device).
 * Every device extracts its block and matches the block's consecutive pairs; counts_all (host, n_frames entries) receives the
 * all-gathered keypoint counts in global frame order (every device holds the same copy). */
int orbx_multi_extract_match_batch_device(orbx_multi* m, int n_frames, const uint8_t* const* d_imgs, int width, int height, int stride,
                                          size_t frame_stride_bytes, orbx_keypoint* const* d_kps, uint8_t* const* d_desc32, int capacity,
                                          int32_t* const* d_n_out, const orbx_bounds* bounds, int window_size, float nnratio,
                                          int check_orientation, int32_t* const* d_matches12, int32_t* const* d_nmatches,
                                          int32_t* counts_all);

/* The throughput form (what bench.py does with one process per GPU, for a C / C++ host): one issuing host thread per device, the
 * blocks of a batch issued stream-ordered on every device's context, several batches in flight.
 *   orbx_multi_set_pipeline_depth: orbx_set_pipeline_depth(depth) on every device's context (whole blocks on `depth` lanes;
 *     0 = two half blocks on two streams); at most max(depth, 2) batches are in flight;
 *   orbx_multi_extract_match_batch_device_async: returns once every device has queued its block; a call that would exceed the
 *     batches in flight first completes the oldest one (whose error, if any, it returns);
 *   orbx_multi_wait_one: completes the oldest batch -- waits for its blocks, all-gathers its counts on the collective streams
 *     (RCCL; the devices meanwhile run the batches issued after it) and fills ITS counts_all; orbx_multi_wait: all of them.
 * Batches in flight together need different output arrays (and counts_all arrays); the contexts returned by orbx_multi_ctx must
 * not be used directly while batches are in flight.  orbx_multi_extract_match_batch_device == the async call + orbx_multi_wait. */
int orbx_multi_set_pipeline_depth(orbx_multi* m, int depth);
int orbx_multi_extract_match_batch_device_async(orbx_multi* m, int n_frames, const uint8_t* const* d_imgs, int width, int height,
                                                int stride, size_t frame_stride_bytes, orbx_keypoint* const* d_kps,
                                                uint8_t* const* d_desc32, int capacity, int32_t* const* d_n_out,
                                                const orbx_bounds* bounds, int window_size, float nnratio, int check_orientation,
                                                int32_t* const* d_matches12, int32_t* const* d_nmatches, int32_t* counts_all);
int orbx_multi_wait_one(orbx_multi* m);
int orbx_multi_wait(orbx_multi* m);

/* ---- test hooks (used by tests/ only; stable but not part of the reference surface) -------- */
/* candidates of (frame, level) of the last extract call, as produced by the FAST kernel, sorted
 * into the reference's order (cell row, cell col, y, x): xyr = (x, y, response) triples relative to
 * (minBorderX, minBorderY) like vToDistributeKeys (cpp:1134-1137).  Returns the count. */
int orbx_debug_candidates(orbx_ctx* ctx, int frame, int level, float* xyr, int cap);
/* The selection units (frame, level) of the context's last batch: counts[level] = keypoints the unit selected (negative: it
 * failed), redone[level] (nullable) = 1 if the many-workgroup kernels could not take the unit (a bucket of keys overflowed its slot)
 * and its workgroup redid it with the one-workgroup code -- results are the same, only the time differs. */
int orbx_debug_selection_units(orbx_ctx* ctx, int frame, int32_t* counts, int32_t* redone);
/* The quadtree selection alone, DistributeOctTree (cpp:698-1011), on the device (the kernels the pipeline uses).  Candidates must be given in row-major (y, x)
 * order with integer coordinates in [0, 4095] relative to (min_x, min_y) and integer responses in [0, 255].
 * variant 0 = LDS-resident kernel (redoing a unit that does not fit on global scratch), variant 1 = global-scratch kernel
 * only, variant 2 = the smaller LDS instance (<= 1024 candidates) and variant 3 = the smallest one (<= 512 candidates, quota
 * <= 128) that the pipeline picks per pyramid level when the previous batch allows; variant 4 = the 2048-candidate LDS instance
 * with 64-bit sort keys (variants 0, 2, 3 use 32-bit keys whenever the rectangle's quadtree path codes fit 21 bits); variant 5 =
 * the many-workgroup kernels the pipeline takes for levels with large units (a workgroup per bucket of keys sorts, one per unit
 * does the tree arithmetic; a unit they cannot take falls to the global-scratch kernel), variant 6 = the same without that
 * fallback (ORBX_E_CAPACITY instead). */
int orbx_debug_distribute_device(orbx_ctx* ctx, const float* xyr, int n, int min_x, int max_x, int min_y, int max_y,
                                 int n_features, int variant, float* out_xyr, int cap);
/* The device's literal replay of libstdc++ std::sort with the reference's compareNodes (cpp:684-696, 912) on n
 * (count, UL.x, id) int32 triples, in place. */
int orbx_debug_std_sort(orbx_ctx* ctx, int32_t* triples, int n);
/* The (cos, sin) pair the descriptor kernel uses for a keypoint angle in degrees (f64 evaluation rounded to f32,
 * cpp:173-174), for n angles; host pointers. */
int orbx_debug_sincos(orbx_ctx* ctx, const float* angle_deg, int n, float* cos_out, float* sin_out);

/* How the context's last extraction batch was issued (the kernels behind one entry point depend on batch size, frame size,
 * alignment and the previous batch's statistics): info8 = { [0] pyramid: 1 = k_pyramid_bands (one launch, large batches), 2 = k_pyramid_tiles
 * (one launch, small batches), 0 = one resize launch per level; [1] row bands (tiles) per frame of that kernel; [2] FAST: 1 = k_fast_wave, 0 = k_fast; [3] selection: candidate
 * capacity of the smallest LDS instance a pyramid level of the batch ran on (2048 / 1024 / 512; 0 = a level expected units beyond
 * the LDS layout and went to the global-scratch kernel); [4] bit 0: the batch was cut into two
 * halves on two streams, bit 1: the descriptor kernel took the selection's staging lists itself (small launches: no k_sel_compact),
 * bit 2: the descriptor kernel ran its pair form, two keypoints per wave (the launches on k_sel_compact's list); [5] frames per kernel launch; [6] 1 = the wide matcher kernels went with the batch; [7] lane the batch
 * went to (1-based; 0 = the context itself) }. */
int orbx_debug_last_launch(const orbx_ctx* ctx, int32_t* info8);
/* Host only, no device needed: how k_pyramid_bands' 512 threads split over a row of `groups` (1 .. 1024) groups of four output
 * pixels, as the host hands it to the kernel with every launch -- info5 = { [0] groups per thread G (2 only when two_groups != 0,
 * i.e. in a launch of the two-group instances), [1] thread-columns ngt, [2] thread-rows per pass rpp, [3] ceil(2^19 / ngt),
 * [4] ceil(2^19 / rpp) }: the kernel computes x / d as (x * ceil(2^19 / d)) >> 19 and divides nothing. */
int orbx_debug_pyr_cols(int groups, int two_groups, uint32_t* info5);
/* Host only, no device needed: the cell records k_fast_wave reads (one 64-byte record of sixteen dwords per FAST cell, in the
 * order (level, cell row, cell column); csrc/orbx_device.h, FastCell) as a context with these parameters and `max_batch` frames
 * builds them for frames of width x height pixels whose level-0 rows lie `stride0` bytes apart.  records (nullable) receives
 * min(cells, cap) records of 16 dwords; info4 = { [0] cells of a frame over all levels, [1] which instance takes the geometry:
 * 0 = none (k_fast runs, and the records are zero), 1 = tile rows of 64 bytes, 2 = of 48 bytes, [2] bytes of the tile in the
 * kernel's dynamic LDS, [3] bytes of that LDS in all }. */
int orbx_debug_fast_cells(const orbx_params* params, int width, int height, int stride0, int max_batch, uint32_t* records, int cap,
                          int32_t* info4);
/* Which matcher kernels did the work (cumulative since orbx_create, for the context itself -- a lane has its own): info4 = { [0] blocks
 * of 256 queries whose candidate lists k_match_bf_mfma built on the matrix cores (a brute-force block of a launch with at least 256
 * such blocks; everything else is listed by k_match_wide_lists on the vector ALU), [1..3] reserved (0) }.  Waits for the context's
 * batches in flight.  Tests take the difference around a call to see that the matrix path ran (or, under the knob match_no_mfma,
 * did not). */
int orbx_debug_match_counters(orbx_ctx* ctx, uint32_t* info4);
/* Diagnostic knobs (process-wide; the library itself reads NO environment variable): a named integer that makes the launches that
 * follow take a particular kernel or launch shape -- e.g. "fast_wg_max_cells" = 0 sends the FAST cells of small batches through
 * k_fast_wave, "no_split" = 1 keeps a synchronous call on one stream.  None changes a result; tests use them to run one input
 * through every kernel, the profiling tools to look at a kernel alone.  The names are listed in csrc/orbx_knobs.h; the Python
 * loader forwards ORBX_<NAME> environment variables here.  value == LLONG_MIN unsets a knob.  ORBX_E_BADARG: unknown name. */
int orbx_debug_set(const char* key, long long value);
/* Host only, no device needed: the quadtree path codes (root << 32 | 16 quadrant digits of ExtractorNode::DivideNode,
 * Features/ORBextractor.cpp:617-676, 747) of n points (xs[i], ys[i]) of a width x height candidate region, from the per-level
 * x / y tables the selection kernels look up and by walking the 16 splits per point; the two agree for every point. */
int orbx_debug_path_codes(int width, int height, int n, const int32_t* xs, const int32_t* ys, uint64_t* from_tables,
                          uint64_t* from_walk);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H_ */
