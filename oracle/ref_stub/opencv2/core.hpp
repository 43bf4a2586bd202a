// Stand-in for the slice of OpenCV's core module that the reference's bag-of-words, matcher and frame-grid sources name
// (oracle/Makefile, target `ref`).  TEST INFRASTRUCTURE only: it lets those sources compile unmodified into
// oracle/_ref/libref.so without OpenCV.  cv::Mat is a minimal refcounted 2-D buffer: `create` fills a new buffer with a
// poison byte (OpenCV does not zero what it allocates), so a dependence on uninitialised data shows up in the results.
// Everything the tests must never reach (FileStorage / FileNode, reshape, convertTo) throws.
#ifndef ORBX_REF_STUB_OPENCV2_CORE_HPP
#define ORBX_REF_STUB_OPENCV2_CORE_HPP

#include <algorithm>
#include <cassert>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

[[noreturn]] inline void refStubUnreachable(const char* what) {
  throw std::logic_error(std::string("OpenCV stand-in: ") + what + " is not available to the reference harness");
}

class Mat {
 public:
  static const unsigned char kPoison = 0xA5;

  int rows = 0, cols = 0;

  Mat() {}
  Mat(int r, int c, int type) { create(r, c, type); }

  void create(int r, int c, int type) {
    if (r < 0 || c < 0) throw std::invalid_argument("cv::Mat stand-in: negative size");
    if (buf_ && rows == r && cols == c && type_ == type && offset_ == 0 && (size_t)r * c * elemSize(type) == buf_->size())
      return;  // OpenCV's create keeps a buffer of the same size and type
    buf_ = std::make_shared<std::vector<unsigned char>>((size_t)r * c * elemSize(type), kPoison);
    rows = r;
    cols = c;
    type_ = type;
    offset_ = 0;
    step_ = (size_t)c * elemSize(type);
  }

  static Mat zeros(int r, int c, int type) {
    Mat m(r, c, type);
    std::fill(m.buf_->begin(), m.buf_->end(), (unsigned char)0);
    return m;
  }

  Mat clone() const {
    Mat m;
    copyTo(m);
    return m;
  }

  void copyTo(Mat& m) const {
    if (empty()) {
      m.release();
      return;
    }
    Mat out(rows, cols, type_);
    for (int i = 0; i < rows; i++) std::memcpy(out.ptr<unsigned char>(i), ptr<unsigned char>(i), step_);
    m = out;
  }

  Mat row(int i) const {
    if (i < 0 || i >= rows) throw std::out_of_range("cv::Mat stand-in: row out of range");
    Mat m(*this);
    m.rows = 1;
    m.offset_ = offset_ + (size_t)i * step_;
    return m;
  }

  void release() {
    buf_.reset();
    rows = cols = 0;
    offset_ = step_ = 0;
  }

  bool empty() const { return !buf_ || rows == 0 || cols == 0; }
  int type() const { return type_; }

  template <typename T>
  T* ptr(int i = 0) {
    return reinterpret_cast<T*>(base(i));
  }
  template <typename T>
  const T* ptr(int i = 0) const {
    return reinterpret_cast<const T*>(const_cast<Mat*>(this)->base(i));
  }
  template <typename T>
  T& at(int i, int j) {
    return ptr<T>(i)[j];
  }
  template <typename T>
  const T& at(int i, int j) const {
    return ptr<T>(i)[j];
  }
  // one index: the i-th element of a single row or column, as OpenCV reads a vector
  template <typename T>
  T& at(int i) {
    return rows == 1 ? at<T>(0, i) : at<T>(i, 0);
  }
  template <typename T>
  const T& at(int i) const {
    return rows == 1 ? at<T>(0, i) : at<T>(i, 0);
  }

  Mat reshape(int) const { refStubUnreachable("Mat::reshape"); }
  void convertTo(Mat&, int) const { refStubUnreachable("Mat::convertTo"); }

 private:
  static size_t elemSize(int type) {
    if (type == CV_8U) return 1;
    if (type == CV_32F) return 4;
    throw std::invalid_argument("cv::Mat stand-in: only CV_8U and CV_32F");
  }
  unsigned char* base(int i) {
    if (!buf_) return nullptr;
    if (i < 0 || i >= rows) throw std::out_of_range("cv::Mat stand-in: row out of range");
    return buf_->data() + offset_ + (size_t)i * step_;
  }

  std::shared_ptr<std::vector<unsigned char>> buf_;
  int type_ = CV_8U;
  size_t offset_ = 0, step_ = 0;
};

class FileNode {
 public:
  FileNode operator[](const std::string&) const { refStubUnreachable("FileNode"); }
  FileNode operator[](const char*) const { refStubUnreachable("FileNode"); }
  FileNode operator[](int) const { refStubUnreachable("FileNode"); }
  size_t size() const { refStubUnreachable("FileNode"); }
  explicit operator int() const { refStubUnreachable("FileNode"); }
  explicit operator double() const { refStubUnreachable("FileNode"); }
  explicit operator std::string() const { refStubUnreachable("FileNode"); }
};

class FileStorage {
 public:
  enum Mode { READ = 0, WRITE = 1 };
  FileStorage(const std::string&, int) { refStubUnreachable("FileStorage"); }
  bool isOpened() const { refStubUnreachable("FileStorage"); }
  FileNode operator[](const std::string&) const { refStubUnreachable("FileStorage"); }
};

template <typename T>
FileStorage& operator<<(FileStorage&, const T&) {
  refStubUnreachable("FileStorage");
}

}  // namespace cv

#endif
