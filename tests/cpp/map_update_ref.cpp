// map_update_ref.cpp — CPU restatement of the map-point update behind the local bundle adjustment (include/orbx.h, "local
// mapping: updating the map points"), TEST INFRASTRUCTURE: built by tests/map_update_ref_lib.py with g++ -O2 -ffp-contract=off.
// The float arithmetic is orb_slam_tracking_amd/csrc/orbx_map_math.inc over orbx_tri_math.inc, the includes the device kernels
// compile too.  This file restates on its own the walk: one problem, sequentially -- the checks, the erasures, each point's
// observers in ascending entry, the bad rule, the reference keyframe, the median of a row of Hamming distances by a histogram
// of 257 bins, the writes behind all checks.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbx.h"

#define ORBX_TRI_FN
#define __device__
#include "../../orb_slam_tracking_amd/csrc/orbx_tri_math.inc"
#include "../../orb_slam_tracking_amd/csrc/orbx_map_math.inc"

using namespace orbx_map;

namespace {

struct Obs {
  int entry, feature;
};

int hamming(const uint8_t* x, const uint8_t* y) {
  int d = 0;
  for (int k = 0; k < 8; k++) {
    uint32_t a, b;
    std::memcpy(&a, x + 4 * k, 4);
    std::memcpy(&b, y + 4 * k, 4);
    d += popc32(a ^ b);
  }
  return d;
}

}  // namespace

extern "C" {

// One problem.  kps [frames][cap], desc [frames][cap][32], n [frames]; entry e names frame frameOf[e]; pose [nE][12], rows
// [nE][cap] (in and out), outlier [nE][cap] or null; the map set's arrays; maskOut may be mask.
void mapr_update(const orbx_keypoint* kps, const uint8_t* desc, const int32_t* n, const int32_t* frameOf, int nE, int nF,
                 const float* pose, int32_t* rows, const uint8_t* outlier, int cap, const float* mapPts, const uint8_t* mask,
                 uint8_t* maskOut, int32_t* mapRef, int mapN, int mapCap, const float* scale, int nLevels, int what, float* normals,
                 float* dist, uint8_t* mapDesc, int32_t* mapObs, orbx_map_result* res) {
  orbx_map_result out;
  std::memset(&out, 0, sizeof out);
  int status = 0;
  auto flagged = [&]() {
    out.status = status;
    *res = out;
  };
  if (mapN < 0 || mapN > mapCap) status |= ST_BAD;
  if (status) return flagged();
  // the entries
  std::vector<float> ow((size_t)nE * 3 + 1, 0.0f);
  for (int e = 0; e < nE; e++) {
    const int f = frameOf[e];
    if (n[f] < 0 || n[f] > cap) status |= ST_BAD;
    for (int e2 = 0; e2 < e; e2++)
      if (frameOf[e2] == f) status |= ST_BAD;
    bool fin = true;
    for (int c = 0; c < 12; c++) fin = fin && orbx_tri::isFinite(pose[(size_t)e * 12 + c]);
    if (!fin)
      status |= ST_NONFINITE;
    else
      orbx_tri::cameraCentre(pose + (size_t)e * 12, &ow[(size_t)e * 3]);
  }
  if (status) return flagged();
  // the vertices
  std::vector<char> vertex((size_t)mapN + 1, 0), lost((size_t)mapN + 1, 0), bad((size_t)mapN + 1, 0);
  for (int e = 0; e < nE; e++)
    for (int f = 0; f < n[frameOf[e]]; f++) {
      const int r = rows[(size_t)e * cap + f];
      if (r >= mapN)
        status |= ST_BAD;
      else if (r >= 0 && e < nF && (!mask || mask[r]))
        vertex[(size_t)r] = 1;
    }
  if (status) return flagged();
  // the observers of every vertex, ascending entry; a second feature of one entry on one vertex is garbage
  std::vector<std::vector<Obs>> obs((size_t)mapN + 1);
  std::vector<int> lastEntry((size_t)mapN + 1, -1);
  for (int e = 0; e < nE; e++)
    for (int f = 0; f < n[frameOf[e]]; f++) {
      const int r = rows[(size_t)e * cap + f];
      if (r < 0 || !vertex[(size_t)r]) continue;
      if (lastEntry[(size_t)r] == e) status |= ST_BAD;
      lastEntry[(size_t)r] = e;
      if (outlier && outlier[(size_t)e * cap + f])
        lost[(size_t)r] = 1;
      else
        obs[(size_t)r].push_back(Obs{e, f});
    }
  if (status) return flagged();
  // per vertex: the bad rule, the reference keyframe, the checks
  std::vector<int> refAt((size_t)mapN + 1, -1);
  for (int m = 0; m < mapN; m++) {
    if (!vertex[(size_t)m]) continue;
    out.n_points++;
    const float* X = mapPts + (size_t)m * 3;
    if (!finite3(X)) {
      status |= ST_NONFINITE;
      continue;
    }
    const std::vector<Obs>& o = obs[(size_t)m];
    const int N = (int)o.size();
    if (N > out.max_observers) out.max_observers = N;
    if ((lost[(size_t)m] && N <= 2) || N == 0) {
      bad[(size_t)m] = 1;
      out.n_bad_points++;
      continue;
    }
    const int refFrame = mapRef ? mapRef[m] : -1;
    int at = -1;
    for (int k = 0; k < N; k++)
      if (refFrame >= 0 && frameOf[o[(size_t)k].entry] == refFrame) at = k;
    if (at < 0) at = 0;
    refAt[(size_t)m] = at;
    const int fr = frameOf[o[(size_t)at].entry];
    const int oct = kps[(size_t)fr * cap + o[(size_t)at].feature].octave;
    if (oct < 0 || oct >= nLevels) status |= ST_BAD;
    for (int k = 0; k < N; k++) {
      float t[3];
      if (!normalTerm(X, &ow[(size_t)o[(size_t)k].entry * 3], t)) status |= ST_NONFINITE;
    }
    out.n_observations += N;
    if (refFrame >= 0 && fr != refFrame) out.n_ref_moved++;
  }
  if (status) {
    std::memset(&out, 0, sizeof out);
    return flagged();
  }

  // ---- the writes ----
  for (int e = 0; e < nE; e++)
    for (int f = 0; f < n[frameOf[e]]; f++) {
      int32_t& r = rows[(size_t)e * cap + f];
      if (r < 0 || !vertex[(size_t)r]) continue;
      if (outlier && outlier[(size_t)e * cap + f]) {
        r = -1;
        out.n_erased++;
      } else if (bad[(size_t)r]) {
        r = -1;
        out.n_cleared++;
      }
    }
  for (int m = 0; m < mapN; m++) {
    if (!vertex[(size_t)m]) continue;
    if (bad[(size_t)m]) {
      maskOut[m] = 0;
      mapObs[m] = 0;
      continue;
    }
    const std::vector<Obs>& o = obs[(size_t)m];
    const int N = (int)o.size();
    maskOut[m] = mask ? mask[m] : (uint8_t)1;
    mapObs[m] = N;
    const Obs ref = o[(size_t)refAt[(size_t)m]];
    if (mapRef) mapRef[m] = frameOf[ref.entry];
    const float* X = mapPts + (size_t)m * 3;
    if (what & WHAT_NORMALS) {
      float sum[3] = {0.0f, 0.0f, 0.0f};
      for (int k = 0; k < N; k++) {
        float t[3];
        normalTerm(X, &ow[(size_t)o[(size_t)k].entry * 3], t);
        normalAdd(sum, t);
      }
      normalFinish(sum, N, normals + (size_t)m * 3);
      const int oct = kps[(size_t)frameOf[ref.entry] * cap + ref.feature].octave;
      distances(X, &ow[(size_t)ref.entry * 3], scale[oct], scale[nLevels - 1], dist + (size_t)m * 2);
    }
    if (what & WHAT_DESCRIPTORS) {
      auto D = [&](int k) { return desc + ((size_t)frameOf[o[(size_t)k].entry] * cap + o[(size_t)k].feature) * 32; };
      int bestMedian = 0x7fffffff, best = 0;
      for (int a = 0; a < N; a++) {
        int hist[257] = {0};
        for (int b = 0; b < N; b++) hist[hamming(D(a), D(b))]++;
        int v = 0, below = hist[0];
        while (below <= (N - 1) / 2) below += hist[++v];  // the element at index (N - 1) / 2 of the sorted row
        if (v < bestMedian) {
          bestMedian = v;
          best = a;
        }
      }
      std::memcpy(mapDesc + (size_t)m * 32, D(best), 32);
    }
  }
  out.status = 0;
  out.n_free = nF;
  *res = out;
}

}  // extern "C"
