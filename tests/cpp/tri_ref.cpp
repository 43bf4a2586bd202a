// tri_ref.cpp — CPU restatement of LocalMapping::CreateNewMapPoints as include/orbx.h states it ("growing the map"):
// ORBmatcher::SearchForTriangulation and the triangulation of its matches.  TEST INFRASTRUCTURE only; compiled on first use by
// tests/tri_ref_lib.py with g++ -O2 -ffp-contract=off.  The arithmetic is orb_slam_tracking_amd/csrc/orbx_tri_math.inc, the
// include the device kernels compile too; this file restates on its own the walk around it, as ORB-SLAM2 writes it: std::map
// FeatureVectors, one KF1 feature after the other, the running bestDist with its non-strict test, the vector of taken KF2
// features, the rotation histogram as lists, the gates in their order.
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

#include "../../include/orbx.h"

#define __device__
#define ORBX_TRI_FN
#include "../../orb_slam_tracking_amd/csrc/orbx_tri_math.inc"

using namespace orbx_tri;

namespace {

const int TH_LOW = 50;
const int HISTO_LENGTH = 30;

typedef std::map<uint32_t, std::vector<uint32_t>> FeatureVector;

// the device form's rule for a malformed vector: an entry that names no feature of the keyframe is skipped
FeatureVector featureVector(const uint32_t* node, const uint32_t* feat, int fvN, int n) {
  FeatureVector fv;
  for (int i = 0; i < fvN; i++)
    if (feat[i] < (uint32_t)n) fv[node[i]].push_back(feat[i]);
  return fv;
}

int distance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

// ORBmatcher::ComputeThreeMaxima
void computeThreeMaxima(const std::vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  for (int i = 0; i < L; i++) {
    const int s = (int)histo[i].size();
    if (s > max1) {
      max3 = max2; max2 = max1; max1 = s;
      ind3 = ind2; ind2 = ind1; ind1 = i;
    } else if (s > max2) {
      max3 = max2; max2 = s;
      ind3 = ind2; ind2 = i;
    } else if (s > max3) {
      max3 = s;
      ind3 = i;
    }
  }
  if (max2 < 0.1f * static_cast<float>(max1)) {
    ind2 = -1;
    ind3 = -1;
  } else if (max3 < 0.1f * static_cast<float>(max1)) {
    ind3 = -1;
  }
}

int clampCount(int v, int cap, bool* clamped) {
  const int c = v < 0 ? 0 : (v > cap ? cap : v);
  if (c != v) *clamped = true;
  return c;
}

}  // namespace

// One pair.  n1 / n2 / fvn1 / fvn2 are clamped to cap (as the batch call's counts to the capacity).  useMedian == 0: no gate.
// matches12 holds cap entries, all of them written.
extern "C" void trr_search_for_triangulation(const orbx_keypoint* kps1, const uint8_t* desc1, int n1, const uint32_t* node1,
                                             const uint32_t* feat1, int fvn1, const uint8_t* mask1, const float* pose1,
                                             const orbx_keypoint* kps2, const uint8_t* desc2, int n2, const uint32_t* node2,
                                             const uint32_t* feat2, int fvn2, const uint8_t* mask2, const float* pose2, const float* K,
                                             int useMedian, float median2, const float* scale, const float* sigma2, int nLevels,
                                             int checkOrientation, int cap, int32_t* matches12, orbx_tri_match_result* res) {
  bool clamped = false;
  n1 = clampCount(n1, cap, &clamped);
  n2 = clampCount(n2, cap, &clamped);
  fvn1 = clampCount(fvn1, cap, &clamped);
  fvn2 = clampCount(fvn2, cap, &clamped);
  for (int i = 0; i < cap; i++) matches12[i] = -1;
  orbx_tri_match_result r = {};
  bool badMedian = false;
  PairGeom g;
  pairGeometry(pose1, pose2, K[0], K[4], K[2], K[5], &g);
  if (g.nonfinite) r.status |= ORBX_TRI_NONFINITE;
  else if (g.baseline == 0.0f) {
    r.status |= ORBX_TRI_ZERO_BASELINE;
    for (int k = 0; k < 9; k++) g.F12[k] = 0.0f;
    g.ex = g.ey = 0.0f;
  } else if (useMedian) {
    if (!(median2 > 0.0f) || !isFinite(median2)) badMedian = true;  // (garbage: flagged, no gate)
    else if (g.baseline / median2 < 0.01f) r.status |= ORBX_TRI_LOW_BASELINE;
  }
  r.baseline = g.baseline;
  r.ex = g.ex;
  r.ey = g.ey;
  for (int k = 0; k < 9; k++) r.F12[k] = g.F12[k];
  if (r.status == 0) {
    const FeatureVector fv1 = featureVector(node1, feat1, fvn1, n1), fv2 = featureVector(node2, feat2, fvn2, n2);
    std::vector<bool> vbMatched2(n2, false);
    std::vector<int> rotHist[HISTO_LENGTH];
    const float factor = HISTO_LENGTH / 360.0f;
    bool badOctave = false;
    for (const auto& kv : fv1) {
      const auto it = fv2.find(kv.first);
      if (it == fv2.end()) continue;
      for (uint32_t idx1 : kv.second) {
        if (mask1 && mask1[idx1] != 0) continue;  // (pKF1->GetMapPoint(idx1): already a map point)
        r.n_queries++;
        const orbx_keypoint& kp1 = kps1[idx1];
        float abc[3];
        epipolarLine(g.F12, kp1.x, kp1.y, abc);
        int bestDist = TH_LOW, bestIdx2 = -1;
        bool any = false;
        for (uint32_t idx2 : it->second) {
          if (vbMatched2[idx2] || (mask2 && mask2[idx2] != 0)) continue;
          const int dist = distance(desc1 + (size_t)idx1 * 32, desc2 + (size_t)idx2 * 32);
          if (dist > TH_LOW) continue;
          // (deviation 3: the counters see every candidate at dist <= TH_LOW; the walk below is ORB-SLAM2's)
          any = true;
          const orbx_keypoint& kp2 = kps2[idx2];
          if (kp2.octave < 0 || kp2.octave >= nLevels) {
            badOctave = true;
            continue;
          }
          const int verdict = candidateTest(g.ex, g.ey, abc, kp2.x, kp2.y, 100.0f * scale[kp2.octave], 3.84f * sigma2[kp2.octave]);
          if (verdict == 1) r.n_epipole_rejected++;
          if (verdict == 2) r.n_epiline_rejected++;
          if (dist > bestDist) continue;
          if (verdict != 0) continue;
          bestIdx2 = (int)idx2;
          bestDist = dist;
        }
        if (any) r.n_with_candidates++;
        if (bestIdx2 >= 0) {
          matches12[idx1] = bestIdx2;
          vbMatched2[bestIdx2] = true;
          r.nmatches++;
          if (checkOrientation) {
            float rot = kp1.angle - kps2[bestIdx2].angle;
            if (rot < 0.0f) rot += 360.0f;
            int bin = (int)roundf(rot * factor);
            if (bin == HISTO_LENGTH) bin = 0;
            if (bin >= 0 && bin < HISTO_LENGTH) rotHist[bin].push_back((int)idx1);
          }
        }
      }
    }
    if (badOctave) r.status |= ORBX_TRI_BAD_INPUT;
    if (checkOrientation) {
      int ind1 = -1, ind2 = -1, ind3 = -1;
      computeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
      for (int i = 0; i < HISTO_LENGTH; i++) {
        if (i == ind1 || i == ind2 || i == ind3) continue;
        for (int idx1 : rotHist[i]) {
          matches12[idx1] = -1;
          r.nmatches--;
          r.n_rot_removed++;
        }
      }
    }
  }
  if (clamped || badMedian) r.status |= ORBX_TRI_BAD_INPUT;
  *res = r;
}

// triangulate() of orbx_tri_math.inc on its own, for the inputs no keyframe pair produces (the camera centres are arguments): the
// outcome code; pt [8] = X, normal, minDist, maxDist
extern "C" int trr_triangulate_one(const float* pose1, const float* pose2, const float* Ow1, const float* Ow2, const float* K,
                                   const float* xy1, const float* xy2, float th1, float th2, float s1, float s2, float ratioFactor,
                                   float sLast, float* pt) {
  TriPoint p = {};
  const int o = triangulate(pose1, pose2, Ow1, Ow2, K[0], K[4], K[2], K[5], xy1[0], xy1[1], xy2[0], xy2[1], th1, th2, s1, s2, ratioFactor,
                            sLast, &p);
  for (int k = 0; k < 3; k++) {
    pt[k] = p.X[k];
    pt[3 + k] = p.normal[k];
  }
  pt[6] = p.minDist;
  pt[7] = p.maxDist;
  return o;
}

// One pair; every output holds cap entries; outcome (nullable) [cap]: 0 = no match followed, else the TRI_* code of the match;
// x3d (nullable) [cap][3]: the point of every match that reached the depth tests, kept or not.
extern "C" void trr_triangulate_matches(const orbx_keypoint* kps1, int n1, const float* pose1, const orbx_keypoint* kps2, int n2,
                                        const float* pose2, const float* K, const float* scale, const float* sigma2, int nLevels,
                                        float scaleFactor, const int32_t* matches12, int cap, float* points, uint8_t* pointMask,
                                        float* pointNormal, float* pointDist, orbx_tri_result* res, int32_t* outcome, float* x3d) {
  bool clamped = false;
  n1 = clampCount(n1, cap, &clamped);
  n2 = clampCount(n2, cap, &clamped);
  orbx_tri_result r = {};
  if (clamped) r.status |= ORBX_TRI_BAD_INPUT;
  for (int i = 0; i < cap; i++) {
    pointMask[i] = 0;
    for (int k = 0; k < 3; k++) points[3 * i + k] = pointNormal[3 * i + k] = 0.0f;
    pointDist[2 * i] = pointDist[2 * i + 1] = 0.0f;
    if (outcome) outcome[i] = 0;
    if (x3d) x3d[3 * i] = x3d[3 * i + 1] = x3d[3 * i + 2] = 0.0f;
  }
  bool finite = true;
  for (int k = 0; k < 12; k++) finite = finite && isFinite(pose1[k]) && isFinite(pose2[k]);
  if (!finite) r.status |= ORBX_TRI_NONFINITE;
  float Ow1[3], Ow2[3];
  if (finite) {
    cameraCentre(pose1, Ow1);
    cameraCentre(pose2, Ow2);
  }
  int32_t* counter[TRI_SCALE + 1] = {nullptr, &r.n_points, &r.n_low_parallax, &r.n_w_zero, &r.n_behind_1, &r.n_behind_2,
                                     &r.n_reproj_1, &r.n_reproj_2, &r.n_zero_dist, &r.n_scale};
  for (int i = 0; finite && i < n1; i++) {
    const int j = matches12[i];
    if (j < 0) continue;
    if (j >= n2 || kps1[i].octave < 0 || kps1[i].octave >= nLevels || kps2[j].octave < 0 || kps2[j].octave >= nLevels) {
      r.status |= ORBX_TRI_BAD_INPUT;
      continue;
    }
    const orbx_keypoint &kp1 = kps1[i], &kp2 = kps2[j];
    TriPoint pt = {};
    const int o = triangulate(pose1, pose2, Ow1, Ow2, K[0], K[4], K[2], K[5], kp1.x, kp1.y, kp2.x, kp2.y, 5.991f * sigma2[kp1.octave],
                              5.991f * sigma2[kp2.octave], scale[kp1.octave], scale[kp2.octave], 1.5f * scaleFactor, scale[nLevels - 1],
                              &pt);
    r.n_matches++;
    (*counter[o])++;
    if (outcome) outcome[i] = o;
    if (x3d && o != TRI_LOW_PARALLAX && o != TRI_W_ZERO)
      for (int k = 0; k < 3; k++) x3d[3 * i + k] = pt.X[k];
    if (o == TRI_KEPT) {
      pointMask[i] = 1;
      for (int k = 0; k < 3; k++) {
        points[3 * i + k] = pt.X[k];
        pointNormal[3 * i + k] = pt.normal[k];
      }
      pointDist[2 * i] = pt.minDist;
      pointDist[2 * i + 1] = pt.maxDist;
    }
  }
  *res = r;
}
