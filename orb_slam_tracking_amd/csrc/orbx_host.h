// orbx_host.h — what the host .cpp files of liborbx share: the error check, the kernel launchers (orbx_launch.h), what one module
// needs of another's private types, and the small helpers of the entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

#include "orbx_buf.h"
#include "orbx_device.h"
#include "orbx_launch.h"

namespace orbx {

// What the modules need of a context (orbx_ctx is private to orbx_api.cpp, which defines these).
int ctxDevice(const orbx_ctx* c);
hipStream_t ctxStream(const orbx_ctx* c);
// the context's device made current and every batch issued with the _async calls waited for (they may still be writing the inputs)
int ctxDrain(orbx_ctx* c);
void ctxSetError(orbx_ctx* c, const char* msg);
const float* ctxInvSigma2(const orbx_ctx* c, int* nlevels);
const float* ctxScale(const orbx_ctx* c, int* nlevels);  // mvScaleFactor
const float* ctxSigma2(const orbx_ctx* c, int* nlevels);  // mvLevelSigma2
InitScratch* ctxInit(orbx_ctx* c);
MatchBowScratch* ctxMatchBow(orbx_ctx* c);
BaScratch* ctxBa(orbx_ctx* c);
PoseScratch* ctxPose(orbx_ctx* c);
PnpScratch* ctxPnp(orbx_ctx* c);
Sim3Scratch* ctxSim3(orbx_ctx* c);
Sim3OptScratch* ctxSim3Opt(orbx_ctx* c);
TriScratch* ctxTri(orbx_ctx* c);

// ... and of a vocabulary (orbx_vocabulary is private to orbx_bow.cpp): the context it was made on, and the descent alone over
// a batch; *nodes the vocabulary's breadth-first nodes, *fin [n_frames][capacity] the breadth-first index each feature ends at
// (the vocabulary's scratch: valid until its next call)
orbx_ctx* vocCtx(const orbx_vocabulary* v);
int vocDescend(orbx_ctx* ctx, orbx_vocabulary* voc, int n_frames, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
               const BowNode** nodes, const uint32_t** fin);

// A failed HIP call ends the enclosing function with ORBX_E_HIP and, when there is a context (the enclosing function's `ctx`),
// leaves the call and its error in the context's error string.
#define HIPCHK(expr)                                                                                    \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) {                                                                             \
      char buf_[512];                                                                                   \
      snprintf(buf_, sizeof buf_, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
      if (ctx) orbx::ctxSetError(ctx, buf_);                                                            \
      return ORBX_E_HIP;                                                                                \
    }                                                                                                   \
  } while (0)

// every first[p] in [0, nFirst) and every second[p] in [0, nSecond)
inline bool pairsInRange(const int32_t* first, const int32_t* second, int nPairs, int nFirst, int nSecond) {
  for (int p = 0; p < nPairs; p++)
    if (first[p] < 0 || first[p] >= nFirst || second[p] < 0 || second[p] >= nSecond) return false;
  return true;
}
inline bool pairsInRange(const int32_t* first, const int32_t* second, int nPairs, int nFrames) {
  return pairsInRange(first, second, nPairs, nFrames, nFrames);
}

// the row-major camera matrix K[9] as the kernels take it
inline void intrinsics(const float* K, double* fx, double* fy, double* cx, double* cy) {
  *fx = (double)K[0];
  *fy = (double)K[4];
  *cx = (double)K[2];
  *cy = (double)K[5];
}

// `count` elements host -> device / device -> host behind the work on `st`; nothing for a count of 0.  (up's destination may be
// a kernel argument, which points to const.)
template <class T>
hipError_t up(const T* dst, const T* src, size_t count, hipStream_t st) {
  return count ? hipMemcpyAsync(const_cast<T*>(dst), src, count * sizeof(T), hipMemcpyHostToDevice, st) : hipSuccess;
}
template <class T>
hipError_t down(T* dst, const T* src, size_t count, hipStream_t st) {
  return count ? hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, st) : hipSuccess;
}

}  // namespace orbx
