// orbx_buf.h — owners of the library's device and page-locked host memory, and the one description of a block's layout.
// Every host .cpp of the library except orbx_multi.cpp allocates and frees through these types only.  The scratch structs at the
// end are what a context keeps across calls for the modules that live in their own .cpp: held arrays and work areas.  The
// staging of the single-problem calls is no part of them: a context has one block for all of it (ctxIo() in orbx_host.h, which
// declares the accessors and Staged, the helper that lays a call's staging out).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

namespace orbx {

template <class T>
constexpr T alignUp(T v, T a) {
  return (v + a - 1) / a * a;
}

// Device memory that only grows; freed by its destructor or reset().  grow() replaces a smaller buffer: whoever may still use
// it must have been drained first (by the caller, or through the stream argument).  After a failed allocation the buffer is
// empty with size 0, so the next call retries.  Reads as a T* wherever one is expected.
template <class T>
class DeviceBuf {
 public:
  DeviceBuf() = default;
  DeviceBuf(DeviceBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  DeviceBuf& operator=(DeviceBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  ~DeviceBuf() { reset(); }
  operator T*() const { return p_; }
  size_t bytes() const { return bytes_; }
  hipError_t grow(size_t bytes) {
    if (bytes <= bytes_) return hipSuccess;
    reset();
    const hipError_t e = hipMalloc((void**)&p_, bytes);
    if (e != hipSuccess) {
      p_ = nullptr;
      return e;
    }
    bytes_ = bytes;
    return hipSuccess;
  }
  // ... and synchronises `st` first when a live buffer is about to be freed (work queued on it may still use the buffer)
  hipError_t grow(size_t bytes, hipStream_t st) {
    if (bytes > bytes_ && p_) {
      const hipError_t e = hipStreamSynchronize(st);
      if (e != hipSuccess) return e;
    }
    return grow(bytes);
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

// Page-locked host memory (hipHostMalloc), grown like DeviceBuf; grown `mapped`, dev() is its device view.
template <class T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept
      : p_(std::exchange(o.p_, nullptr)), dev_(std::exchange(o.dev_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      dev_ = std::exchange(o.dev_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  ~PinnedBuf() { reset(); }
  operator T*() const { return p_; }
  T* dev() const { return dev_; }
  size_t bytes() const { return bytes_; }
  hipError_t grow(size_t bytes, bool mapped = false) {
    if (bytes <= bytes_) return hipSuccess;
    reset();
    hipError_t e = hipHostMalloc((void**)&p_, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
      p_ = nullptr;
      return e;
    }
    bytes_ = bytes;
    if (mapped && (e = hipHostGetDevicePointer((void**)&dev_, p_, 0)) != hipSuccess) reset();
    return e;
  }
  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    dev_ = nullptr;
    bytes_ = 0;
  }

 private:
  T* p_ = nullptr;
  T* dev_ = nullptr;
  size_t bytes_ = 0;
};

// A block's arrays in order, each starting 256-byte aligned.  A block is described once, as code that takes its arrays from a
// Layout: run over a Layout without a base it only counts (size()), run over the block's base it hands out the pointers.
class Layout {
 public:
  Layout() = default;
  explicit Layout(void* base) : base_((uintptr_t)base) {}
  template <class T>
  T* take(size_t n) {
    T* p = reinterpret_cast<T*>(base_ + off_);
    off_ += alignUp(n * sizeof(T), (size_t)256);
    return p;
  }
  size_t size() const { return off_; }

 private:
  uintptr_t base_ = 0;
  size_t off_ = 0;
};

// A device array and the host copy its last upload read.  The copy command reads the host copy when it runs, which may be after
// the call that queued it has returned, so the copy stays put until the next replace(); and an array that holds() the values a
// call brings is not uploaded again.  Between "holds() says no" and replace() the caller drains whatever may still read either
// copy (HeldUploads in orbx_host.h is that step).  A call brings its values as columns of n entries each, held one after the
// other: a pair list is its two columns, a table is one.  Reads as a T* (the device array) wherever one is expected.
template <class T>
class HeldArray {
 public:
  using Columns = std::initializer_list<const T*>;
  operator T*() const { return dev_; }
  bool holds(Columns columns, size_t n) const {
    if (host_.size() != columns.size() * n) return false;
    const T* held = host_.data();
    for (const T* c : columns) {
      if (n && std::memcmp(held, c, n * sizeof(T)) != 0) return false;
      held += n;
    }
    return true;
  }
  // From the first step to the queued copy the array holds nothing, and again after a copy command that failed: no later call
  // skips an upload the device never received.
  hipError_t replace(hipStream_t st, Columns columns, size_t n) {
    host_.clear();
    hipError_t e = dev_.grow(columns.size() * n * sizeof(T));
    if (e != hipSuccess) return e;
    for (const T* c : columns) host_.insert(host_.end(), c, c + n);
    e = hipMemcpyAsync(dev_, host_.data(), host_.size() * sizeof(T), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) host_.clear();
    return e;
  }
  void forget() { host_.clear(); }  // (the work the upload was queued with has been abandoned)

 private:
  DeviceBuf<T> dev_;
  std::vector<T> host_;
};

// What a context keeps for the Initializer (orbx_init.cpp).
struct InitScratch {
  DeviceBuf<uint8_t> dInit;  // arena of orbx_find_models* / orbx_initialize*: the work area, a single pair's staging behind it
  HeldArray<int32_t> pairs;  // their pair list [2][n_pairs]
};

// What a context keeps for orbx_match_bow* (orbx_match_bow.cpp) and the matchers by projection (orbx_match_proj.cpp): the index
// lists of the last call of each.
struct MatchBowScratch {
  HeldArray<int32_t> pairs;        // [2][n_pairs] of orbx_match_bow*
  HeldArray<int32_t> projPairs;    // [3][n_pairs] (last, current, point set) of orbx_match_projection*
  HeldArray<int32_t> localPairs;   // [2][n_pairs] (frame, map set) of orbx_match_local_map*
  HeldArray<int32_t> kfProjPairs;  // [3][n_pairs] (keyframe, current, point set) of orbx_match_keyframe_projection*
  HeldArray<int32_t> sim3Pairs;    // [4][n_pairs] (KF1, KF2, set 1, set 2) of orbx_match_sim3*
  HeldArray<int32_t> scwPairs;     // [2][n_pairs] (current keyframe, map set) of orbx_match_scw*
  HeldArray<int32_t> composeKf2;   // [n_pairs] (matched keyframe) of orbx_sim3_compose_scw*
  HeldArray<int32_t> fusePairs;    // [2][n_pairs] (keyframe, map set) of orbx_fuse*
  HeldArray<int32_t> fuseScwPairs; // [2][n_pairs] (keyframe, map set) of orbx_fuse_scw*
};

// What a context keeps for orbx_match_triangulation* and orbx_triangulate_matches* (orbx_match_bow.cpp).
struct TriScratch {
  HeldArray<int32_t> pairs;  // the pair list [2][n_pairs] (KF1s, KF2s) of the last call of either: the chain uploads it once
};

// What a context keeps for orbx_bundle_adjust* (orbx_ba.cpp).
struct BaScratch {
  DeviceBuf<uint8_t> dWork;  // the per-point blocks of every pair: sized from n_pairs x capacity
  HeldArray<int32_t> pairs;  // the pair list [2][n_pairs] of the last call
  HeldArray<float> sigma;    // inv_sigma2 of the last call
};

// What a context keeps for orbx_pose_optimize* (orbx_pose.cpp).
struct PoseScratch {
  HeldArray<int32_t> problems;  // the problem list [2][n_problems] of the last call
  HeldArray<float> sigma;       // inv_sigma2 of the last call
};

// What a context keeps for orbx_pnp_solve* (orbx_pose.cpp).
struct PnpScratch {
  HeldArray<int32_t> problems;  // the problem list [2][n_problems] of the last call
  HeldArray<float> sigma2;      // sigma2 of the last call
  HeldArray<int32_t> table;     // N -> (mRansacMinInliers, mRansacMaxIts) for N in [0, capacity] of the last call
  std::vector<int32_t> hTable;  // ... as computed on the host for `key`: the parameters it was computed from
  double keyProbability = 0;
  float keyEpsilon = 0;
  int keyMinInliers = 0, keyMaxIterations = 0;
  DeviceBuf<uint8_t> dWork;     // the correspondences, the hypotheses and the per-problem values of a call
};

// What a context keeps for orbx_sim3_solve* (orbx_pose.cpp).
struct Sim3Scratch {
  HeldArray<int32_t> problems;  // the lists [4][n_problems] (KF1, KF2, set 1, set 2) of the last call
  HeldArray<float> sigma2;      // sigma2 of the last call
  HeldArray<int32_t> table;     // N -> mRansacMaxIts for N in [0, capacity] of the last call
  std::vector<int32_t> hTable;  // ... as computed on the host for `key`: the parameters it was computed from
  double keyProbability = 0;
  int keyMinInliers = 0, keyMaxIterations = 0;
  DeviceBuf<uint8_t> dWork;     // the correspondences, the hypotheses and the per-problem values of a call
};

// What a context keeps for orbx_optimize_sim3* (orbx_pose.cpp).
struct Sim3OptScratch {
  HeldArray<int32_t> problems;  // the lists [4][n_problems] (KF1, KF2, set 1, set 2) of the last call
  HeldArray<float> sigma;       // inv_sigma2 of the last call
};

// What a context keeps for orbx_local_ba* (orbx_ba.cpp).
struct LbaScratch {
  HeldArray<int32_t> problems;  // [5][n_problems] (first entry, entries, free entries, map set, workspace offset / 256) of the last call
  HeldArray<int32_t> entries;   // the entry list [n_entries] (frames) of the last call
  HeldArray<float> sigma;       // inv_sigma2 of the last call
  DeviceBuf<uint8_t> dWork;     // the problems' workspaces: graph, per-vertex and per-edge blocks, poses, reduced systems
};

// What a context keeps for orbx_map_update* (orbx_ba.cpp).
struct MapScratch {
  HeldArray<int32_t> problems;  // [5][n_problems] (first entry, entries, free entries, map set, workspace offset / 256) of the last call
  HeldArray<int32_t> entries;   // the entry list [n_entries] (frames) of the last call
  HeldArray<float> scale;       // mvScaleFactor
  DeviceBuf<uint8_t> dWork;     // the problems' workspaces: MapWork of orbx_device.h
};

// What a context keeps for orbx_stereo_match* (orbx_api.cpp).
struct StereoScratch {
  HeldArray<int32_t> rigs;  // [2][n_rigs] (left frame, right frame) of the last call
  HeldArray<uint8_t> levels;  // the last extract call's levels, StereoLevel of orbx_device.h [nlevels]
  DeviceBuf<int32_t> dWs;   // [n_rigs][STEREO_WS] the rigs' counters
  DeviceBuf<int32_t> dSad;  // [n_rigs][capacity] the kept SADs when the caller takes none
};

}  // namespace orbx
