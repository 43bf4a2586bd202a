// orbx_buf.h — owners of the library's device and page-locked host memory, and the one description of a staging block.
// orbx_api.cpp, orbx_bow.cpp, orbx_ba.cpp and orbx_pose.cpp allocate and free through these types only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
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

// A staging block's arrays in order, each starting 256-byte aligned.  A block is described once, as code that takes its arrays
// from a Layout: run over a Layout without a base it only counts (size()), run over the block's base it hands out the pointers.
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

// What a context keeps for orbx_match_bow* (orbx_match_bow.cpp; the context owns it, orbx_api.cpp).
struct MatchBowScratch {
  DeviceBuf<int32_t> dPairs;    // the pair list [2][n_pairs] of the last call
  std::vector<int32_t> hPairs;  // (kept alive behind the asynchronous upload)
  DeviceBuf<uint8_t> dIo;       // staging of orbx_match_bow
};

// What a context keeps for orbx_bundle_adjust* (orbx_ba.cpp; the context owns it, orbx_api.cpp).
struct BaScratch {
  DeviceBuf<uint8_t> dWork;     // the per-point blocks of every pair: sized from n_pairs x capacity
  DeviceBuf<int32_t> dPairs;    // the pair list [2][n_pairs] of the last call
  std::vector<int32_t> hPairs;  // (kept alive behind the asynchronous upload)
  DeviceBuf<float> dSigma;      // inv_sigma2 of the last call
  std::vector<float> hSigma;
  DeviceBuf<uint8_t> dIo;       // staging of orbx_bundle_adjust
};

// What a context keeps for orbx_pose_optimize* (orbx_pose.cpp; the context owns it, orbx_api.cpp).
struct PoseScratch {
  DeviceBuf<int32_t> dProblems;    // the problem list [2][n_problems] of the last call
  std::vector<int32_t> hProblems;  // (kept alive behind the asynchronous upload)
  DeviceBuf<float> dSigma;         // inv_sigma2 of the last call
  std::vector<float> hSigma;
  DeviceBuf<uint8_t> dIo;          // staging of orbx_pose_optimize
};

}  // namespace orbx
