// orbx_stereo_math.inc — the arithmetic of Frame::ComputeStereoMatches and Frame::UnprojectStereo (include/orbx.h, "stereo: matching
// left and right", rules 2-13), stated once: the device kernels (orbx_stereo_kernel.hip) and the CPU restatement
// (tests/cpp/stereo_ref.cpp) both compile this file.  f32 without contraction (-ffp-contract=off) and a correctly rounded divide
// on both sides.  Define ORBX_STEREO_FN (__device__, or nothing) before including; <math.h> / <cmath> must be in scope.
#ifndef ORBX_STEREO_FN
#define ORBX_STEREO_FN
#endif

namespace orbx_stereo {

constexpr int kWin = 5;       // w: half width of the correlation window
constexpr int kShift = 5;     // L: half range of the shifts
constexpr int kThOrb = 75;    // (TH_HIGH + TH_LOW) / 2
constexpr int kThHigh = 100;  // TH_HIGH
constexpr int kBadInput = 2, kNonFinite = 4;  // ORBX_STEREO_BAD_INPUT, ORBX_STEREO_NONFINITE

// the counters of orbx_stereo_result in the record's order, as the kernels and the restatement index them
enum Counter {
  cStatus, cMatches, cWithCandidates, cOrbMatched, cWindowRefused, cOutOfLevel, cEdge, cDeltaRefused, cDisparityRefused, cClamped,
  cBeforeMedian, cMedianSad, cThDist, cRemovedByMedian, cCount
};

ORBX_STEREO_FN inline bool finite32(float v) { return v - v == 0.0f; }

// rule 2: the rows [*minr, *maxr] a right keypoint is a candidate of, clipped to [0, rows0); an empty band has *minr > *maxr
ORBX_STEREO_FN inline void rowBand(float y, float scaleOct, int rows0, int* minr, int* maxr) {
  const float r = 2.0f * scaleOct;
  float hi = ceilf(y + r), lo = floorf(y - r);
  const float top = (float)(rows0 - 1);
  if (!(hi >= 0.0f) || !(lo <= top)) {
    *minr = 1;
    *maxr = 0;
    return;
  }
  if (lo < 0.0f) lo = 0.0f;
  if (hi > top) hi = top;
  *minr = (int)lo;
  *maxr = (int)hi;
}

// rule 4: the row of a left keypoint, or -1 when (int)y lies outside [0, rows0) (deviation 3)
ORBX_STEREO_FN inline int leftRow(float y, int rows0) { return (y > -1.0f && y < (float)rows0) ? (int)y : -1; }

// rule 5, on a right keypoint's band, octave and x
ORBX_STEREO_FN inline bool isCandidate(int row, int octL, float minU, float maxU, int minr, int maxr, int octR, float xR) {
  return row >= minr && row <= maxr && octR >= octL - 1 && octR <= octL + 1 && xR >= minU && xR <= maxU;
}

// rule 7: a coordinate at the keypoint's level, rounded half away from zero; kept as a float until the window tests have bounded it
ORBX_STEREO_FN inline float levelCoord(float v, float invScale) { return roundf(v * invScale); }

// rule 8, as the design writes it
ORBX_STEREO_FN inline bool windowRefused(float su0, int cols) {
  return su0 + (float)(kShift - kWin) < 0.0f || su0 + (float)(kShift + kWin + 1) >= (float)cols;
}
// deviation 1: the left window or the right strip would leave the level
ORBX_STEREO_FN inline bool outOfLevel(float su, float sv, float su0, int cols, int rows) {
  return !(sv - (float)kWin >= 0.0f && sv + (float)kWin < (float)rows && su - (float)kWin >= 0.0f && su + (float)kWin < (float)cols &&
           su0 - (float)(kShift + kWin) >= 0.0f && su0 + (float)(kShift + kWin) < (float)cols);
}

// rule 9: one pixel's term of a SAD, each side with its window's centre subtracted
ORBX_STEREO_FN inline int sadTerm(int l, int lc, int r, int rc) {
  const int d = (l - lc) - (r - rc);
  return d < 0 ? -d : d;
}

// rule 10
ORBX_STEREO_FN inline float parabolaDelta(int s1, int s2, int s3) {
  const float d1 = (float)s1, d2 = (float)s2, d3 = (float)s3;
  return (d1 - d3) / (2.0f * ((d1 + d3) - 2.0f * d2));
}
ORBX_STEREO_FN inline bool deltaRefused(float delta) { return delta < -1.0f || delta > 1.0f; }

// rule 11: false = refused by the disparity gate
ORBX_STEREO_FN inline bool disparity(float xL, float scaleO, float su0, int inc, float delta, float maxD, float bf, float* uR,
                                     float* depth, int* clamped) {
  float bestuR = scaleO * ((su0 + (float)inc) + delta);
  float disp = xL - bestuR;
  if (!(disp >= 0.0f && disp < maxD)) return false;
  *clamped = 0;
  if (disp <= 0.0f) {
    disp = 0.01f;
    bestuR = (float)((double)xL - 0.01);
    *clamped = 1;
  }
  *depth = bf / disp;
  *uR = bestuR;
  return true;
}

// rule 12
ORBX_STEREO_FN inline float medianThreshold(int median) { return (1.5f * 1.4f) * (float)median; }

// rule 13: pose = Rwc row-major then Ow, or null for camera coordinates
ORBX_STEREO_FN inline void unproject(float u, float v, float z, float cx, float cy, float invfx, float invfy, const float* pose,
                                     float* out) {
  const float x = ((u - cx) * z) * invfx, y = ((v - cy) * z) * invfy;
  if (!pose) {
    out[0] = x;
    out[1] = y;
    out[2] = z;
    return;
  }
  for (int k = 0; k < 3; k++) out[k] = ((pose[3 * k] * x + pose[3 * k + 1] * y) + pose[3 * k + 2] * z) + pose[9 + k];
}

}  // namespace orbx_stereo
