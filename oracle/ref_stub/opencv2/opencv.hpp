// Stand-in for <opencv2/opencv.hpp> (see core.hpp next to it): the point and keypoint types, the array proxies of
// ORBextractor::operator()'s signature, and undistortPoints, which throws.  TEST INFRASTRUCTURE only.
#ifndef ORBX_REF_STUB_OPENCV2_OPENCV_HPP
#define ORBX_REF_STUB_OPENCV2_OPENCV_HPP

#include <list>

#include "core.hpp"

namespace cv {

template <typename T>
struct Point_ {
  T x = 0, y = 0;
  Point_() {}
  Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<float> Point2f;

struct KeyPoint {
  Point2f pt;
  float size = 0, angle = -1, response = 0;
  int octave = 0, class_id = -1;
};

class _InputArray {
 public:
  _InputArray(const Mat& m) : m_(&m) {}

 private:
  const Mat* m_;
};
class _OutputArray {
 public:
  _OutputArray(Mat& m) : m_(&m) {}

 private:
  Mat* m_;
};
typedef const _InputArray& InputArray;
typedef const _OutputArray& OutputArray;

inline void undistortPoints(InputArray, OutputArray, InputArray, InputArray, InputArray, InputArray) {
  refStubUnreachable("undistortPoints");
}

}  // namespace cv

#endif
