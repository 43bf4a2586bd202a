// orbx_host.h — what the host .cpp files of liborbx share: the error check, the kernel launchers (orbx_launch.h), what one module
// needs of another's private types, and the two steps the entry points have in common: HeldUploads, the upload of a batch call's
// index lists and tables, and Staged, the staging of a single-problem call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

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
DeviceBuf<uint8_t>& ctxIo(orbx_ctx* c);  // the one staging block of the context's single-problem calls (Staged, below)
InitScratch* ctxInit(orbx_ctx* c);
MatchBowScratch* ctxMatchBow(orbx_ctx* c);
BaScratch* ctxBa(orbx_ctx* c);
PoseScratch* ctxPose(orbx_ctx* c);
PnpScratch* ctxPnp(orbx_ctx* c);
Sim3Scratch* ctxSim3(orbx_ctx* c);
Sim3OptScratch* ctxSim3Opt(orbx_ctx* c);
TriScratch* ctxTri(orbx_ctx* c);
LbaScratch* ctxLba(orbx_ctx* c);
MapScratch* ctxMap(orbx_ctx* c);

// ... and of a vocabulary (orbx_vocabulary is private to orbx_bow.cpp): the context it was made on, and the descent alone over
// a batch; *nodes the vocabulary's breadth-first nodes, *fin [n_frames][capacity] the breadth-first index each feature ends at
// (the vocabulary's scratch: valid until its next call)
orbx_ctx* vocCtx(const orbx_vocabulary* v);
int vocDescend(orbx_ctx* ctx, orbx_vocabulary* voc, int n_frames, const uint8_t* d_desc32, const int32_t* d_n, int capacity,
               const BowNode** nodes, const uint32_t** fin);

// A HIP call's result as a code of the library: ORBX_OK, or ORBX_E_HIP with the call and its error left in the context's error
// string when there is a context.
inline int hipCode(orbx_ctx* ctx, hipError_t e, const char* file, int line, const char* expr) {
  if (e == hipSuccess) return ORBX_OK;
  char buf[512];
  snprintf(buf, sizeof buf, "%s:%d: %s -> %s", file, line, expr, hipGetErrorString(e));
  if (ctx) ctxSetError(ctx, buf);
  return ORBX_E_HIP;
}
// ... of `expr`, for the enclosing function's `ctx`; HIPCHK ends the enclosing function with it when the call failed.
#define HIPRC(expr) orbx::hipCode(ctx, (expr), __FILE__, __LINE__, #expr)
#define HIPCHK(expr)                                 \
  do {                                               \
    if (HIPRC(expr) != ORBX_OK) return ORBX_E_HIP;   \
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

// The held-upload step of a batch call.  What such a call reads from host memory -- its index lists, a sigma table, a RANSAC
// table -- it keeps in HeldArrays, and each goes up only when it differs from what the last call brought: a pipeline that works
// on the same pairs batch after batch uploads once.  An array that differs is replaced, host copy and all, and a copy queued by
// an earlier call may still be reading that host copy, so the call first waits for the stream: once, however many of its arrays
// differ (what is queued after the wait reads only what this call has put in place).  A call that waits here is the documented
// exception to "returns once queued" (include/orbx.h).  (The extraction pipeline's matcher in orbx_api.cpp keeps its pair list
// in a HeldArray too, but its batches run on more than this stream: it waits for all of them itself.)
//   HeldUploads hold(st);
//   HIPCHK(hold(s->problems, {h_frame, h_point_set}, n_problems));
//   HIPCHK(hold(s->sigma, {sig}, nLevels));
class HeldUploads {
 public:
  explicit HeldUploads(hipStream_t st) : st_(st) {}
  template <class T>
  hipError_t operator()(HeldArray<T>& held, typename HeldArray<T>::Columns columns, size_t n) {
    if (held.holds(columns, n)) return hipSuccess;
    if (!waited_) {
      const hipError_t e = hipStreamSynchronize(st_);
      if (e != hipSuccess) return e;
      waited_ = true;
    }
    return held.replace(st_, columns, n);
  }

 private:
  hipStream_t st_;
  bool waited_ = false;
};

// The staging of a synchronous single-problem call: one problem from host memory laid out as a batch of one in a device block,
// the batch entry run on it, the results copied back, the stream waited for.  The call names each array once, in the block's
// order (a Layout's: every array 256-byte aligned), and says with the name what happens to it:
//   Staged io(ctxIo(ctx), st);
//   auto dK = io.in(kps_un, n, cap);          // room for cap elements, the first n uploaded (n == 0 or no source: nothing)
//   auto dMask = io.optIn(mask, n, cap);      // ... and a null kernel argument when the caller brings none
//   auto dM = io.inout(matches, n, cap);      // uploaded before the call, downloaded after it
//   auto dR = io.out(res, 1, 1);              // downloaded after it (no destination: nothing); optOut: null argument then
//   auto dT = io.room<int32_t>(cap);          // device-only
//   io.in(dK, cap, kps_un2, n2);              // a second frame of an array [2][cap]: at an element offset (out likewise)
//   HIPCHK(io.open(Staged::Zeroed));          // the block grown, filled where the call says so, the uploads queued
//   r = orbx_x_batch_device(ctx, ..., io[dK], io[dMask], ...);
//   return io.close(ctx, r);                  // refused: the stream waited for, r.  Else the downloads, the wait, ORBX_OK
// Both ends wait for the stream whenever copies may be queued, also when open() fails half-way and when the batch entry
// refuses: the queued uploads read the caller's arrays and the wrapper's own variables (its counts, its index lists).  After
// close() a call whose downloads depend on a count it has just received names them with out() and closes again.
//
// One block serves every single-problem call of a context, ctxIo().  That is sound because each of them is synchronous -- the
// stream is idle when it returns, so no two blocks are ever live at once -- and because none calls another: every wrapper in
// orbx_pose.cpp, orbx_ba.cpp, orbx_match_bow.cpp, orbx_match_proj.cpp and orbx_init.cpp goes to its own batch entry (or, for
// orbx_check_homography / _fundamental / orbx_check_rt, to the launcher) and to nothing else, and no batch entry stages.  A
// wrapper that ever needs another's result takes both regions from one Staged.  The single pair of orbx_find_models /
// orbx_initialize stages behind the work area of its batch entry, in that arena (`behind`); a vocabulary and a database stage in
// a block of their own, which lives as long as they do.
class Staged {
 public:
  enum Fill { AsLeft, Zeroed };  // AsLeft: what no upload writes keeps what an earlier call left there
  template <class T>
  struct Slot {
    size_t off;
    bool absent;
  };

  Staged(DeviceBuf<uint8_t>& block, hipStream_t st, size_t behind = 0) : block_(block), st_(st), behind_(behind) {}

  template <class T>
  Slot<T> room(size_t cap) {
    const size_t off = layout_.size();
    layout_.take<T>(cap);
    return {off, false};
  }
  template <class T>
  Slot<T> in(const T* src, size_t n, size_t cap) {
    const Slot<T> s = room<T>(cap);
    in(s, 0, src, n);
    return s;
  }
  template <class T>
  Slot<T> optIn(const T* src, size_t n, size_t cap) {
    Slot<T> s = in(src, n, cap);
    s.absent = !src;
    return s;
  }
  template <class T>
  Slot<T> out(T* dst, size_t n, size_t cap) {
    const Slot<T> s = room<T>(cap);
    out(s, 0, dst, n);
    return s;
  }
  template <class T>
  Slot<T> optOut(T* dst, size_t n, size_t cap) {
    Slot<T> s = out(dst, n, cap);
    s.absent = !dst;
    return s;
  }
  template <class T>
  Slot<T> inout(T* host, size_t n, size_t cap) {
    const Slot<T> s = in((const T*)host, n, cap);
    out(s, 0, host, n);
    return s;
  }
  template <class T>
  void in(Slot<T> s, size_t at, const T* src, size_t n) {
    if (src && n) ops_.push_back({Up, 0, s.off + at * sizeof(T), n * sizeof(T), const_cast<T*>(src)});
  }
  template <class T>
  void out(Slot<T> s, size_t at, T* dst, size_t n) {
    if (dst && n) ops_.push_back({Down, 0, s.off + at * sizeof(T), n * sizeof(T), dst});
  }
  // the array's first `count` elements set to `byte` before the uploads
  template <class T>
  void fill(Slot<T> s, int byte, size_t count) {
    ops_.push_back({Set, byte, s.off, count * sizeof(T), nullptr});
  }

  hipError_t open(Fill fill = AsLeft) {
    const size_t bytes = layout_.size();
    hipError_t e = block_.grow(behind_ + bytes, st_);  // (waits for st when a live block is replaced)
    if (e != hipSuccess) return e;
    base_ = block_ + behind_;
    if (fill == Zeroed) e = hipMemsetAsync(base_, 0, bytes, st_);
    for (const Op& o : ops_)
      if (o.kind == Set && e == hipSuccess) e = hipMemsetAsync(base_ + o.off, o.byte, o.bytes, st_);
    for (const Op& o : ops_)
      if (o.kind == Up && e == hipSuccess) e = hipMemcpyAsync(base_ + o.off, o.host, o.bytes, hipMemcpyHostToDevice, st_);
    if (e != hipSuccess) (void)hipStreamSynchronize(st_);
    return e;
  }
  template <class T>
  T* operator[](Slot<T> s) const {
    return s.absent ? nullptr : reinterpret_cast<T*>(base_ + s.off);
  }
  int close(orbx_ctx* ctx, int r) {
    for (const Op& o : ops_)
      if (o.kind == Down && r == ORBX_OK) r = HIPRC(hipMemcpyAsync(o.host, base_ + o.off, o.bytes, hipMemcpyDeviceToHost, st_));
    ops_.clear();
    if (r != ORBX_OK) {
      (void)hipStreamSynchronize(st_);  // (the code and the message are those of what failed first)
      return r;
    }
    return HIPRC(hipStreamSynchronize(st_));
  }

 private:
  enum Kind { Set, Up, Down };
  struct Op {
    Kind kind;
    int byte;
    size_t off, bytes;
    void* host;
  };
  DeviceBuf<uint8_t>& block_;
  hipStream_t st_;
  size_t behind_;
  Layout layout_;
  uint8_t* base_ = nullptr;
  std::vector<Op> ops_;
};

}  // namespace orbx
