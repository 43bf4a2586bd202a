// match_kfproj_ref.cpp — CPU restatement of the relocalisation overload ORBmatcher::SearchByProjection(Frame& CurrentFrame,
// KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist) as include/orbx.h states it ("matching a keyframe's points by
// projection") -- the literal sequential loops, with the frame grid of SlamTypes/Frame.cpp as vectors per cell, nothing shared
// with the library.  TEST INFRASTRUCTURE only; compiled on first use by tests/match_kfproj_ref_lib.py with g++ -O2
// -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

const int HISTO_LENGTH = 30;
const int GRID_COLS = 64, GRID_ROWS = 48;
const int BAD_INPUT = 2, NONFINITE = 4;

struct KeyPoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
};

// Frame's grid (Frame.cpp:46-47, :71-77, :89-99) and GetFeaturesInArea (:163-206)
struct Grid {
  std::vector<int> cell[GRID_COLS][GRID_ROWS];
  float minX, minY, wInv, hInv;
  const KeyPoint* kps;

  Grid(const KeyPoint* k, int n, const int32_t* b) : kps(k) {
    minX = static_cast<float>(b[0]);
    minY = static_cast<float>(b[2]);
    wInv = static_cast<float>(GRID_COLS) / static_cast<float>(b[1] - b[0]);
    hInv = static_cast<float>(GRID_ROWS) / static_cast<float>(b[3] - b[2]);
    for (int i = 0; i < n; i++) {
      const float px = roundf((k[i].x - minX) * wInv), py = roundf((k[i].y - minY) * hInv);
      if (!(px >= 0.0f && px < GRID_COLS && py >= 0.0f && py < GRID_ROWS)) continue;  // (also a coordinate that is no number)
      cell[(int)px][(int)py].push_back(i);
    }
  }

  std::vector<int> area(float x, float y, float r, int minLevel, int maxLevel) const {
    std::vector<int> out;
    const float lox = floorf((x - minX - r) * wInv), hix = ceilf((x - minX + r) * wInv);
    const float loy = floorf((y - minY - r) * hInv), hiy = ceilf((y - minY + r) * hInv);
    // (compared as floats: the same cells as the reference's ints wherever its conversion is defined)
    if (lox >= GRID_COLS) return out;
    const int x0 = lox < 0.0f ? 0 : (int)lox;
    if (hix < 0.0f) return out;
    const int x1 = hix > GRID_COLS - 1 ? GRID_COLS - 1 : (int)hix;
    if (loy >= GRID_ROWS) return out;
    const int y0 = loy < 0.0f ? 0 : (int)loy;
    if (hiy < 0.0f) return out;
    const int y1 = hiy > GRID_ROWS - 1 ? GRID_ROWS - 1 : (int)hiy;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = x0; ix <= x1; ix++)
      for (int iy = y0; iy <= y1; iy++)
        for (int j : cell[ix][iy]) {
          const KeyPoint& kp = kps[j];
          if (bCheckLevels) {
            if (kp.octave < minLevel) continue;
            if (maxLevel >= 0)
              if (kp.octave > maxLevel) continue;
          }
          const float dx = kp.x - x, dy = kp.y - y;
          if (fabsf(dx) < r && fabsf(dy) < r) out.push_back(j);
        }
    return out;
  }
};

int distance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

bool finiteAll(const float* p, int n) {
  for (int k = 0; k < n; k++)
    if (!std::isfinite(p[k])) return false;
  return true;
}

// rule 5 over the candidates `cand` that `skip` does not hold: the first smallest, -1 when none is within orbDist
int pick(const std::vector<int>& cand, const std::vector<char>& skip, const uint8_t* dMP, const uint8_t* desc, int orbDist, int* best) {
  int bestDist = 256, bestIdx = -1;
  for (int idx : cand) {
    if (skip[idx]) continue;
    const int dist = distance(dMP, desc + 32 * (size_t)idx);
    if (dist < bestDist) {
      bestDist = dist;
      bestIdx = idx;
    }
  }
  if (best) *best = bestDist;
  return bestDist <= orbDist ? bestIdx : -1;
}

// ComputeThreeMaxima (Features/ORBmatcher.cpp:152-183) on the bins' sizes
void threeMaxima(const std::vector<int>* histo, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  for (int i = 0; i < HISTO_LENGTH; i++) {
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
  if (max2 < 0.1f * (float)max1) {
    ind2 = -1;
    ind3 = -1;
  } else if (max3 < 0.1f * (float)max1) {
    ind3 = -1;
  }
}

}  // namespace

extern "C" int kpr_features_in_area(const KeyPoint* kps, int n, const int32_t* bounds, float x, float y, float r, int minLevel,
                                    int maxLevel, int32_t* out) {
  const Grid g(kps, n, bounds);
  const std::vector<int> c = g.area(x, y, r, minLevel, maxLevel);
  for (size_t k = 0; k < c.size(); k++) out[k] = c[k];
  return (int)c.size();
}

// One pair.  The keyframe: kpsK [nK] (its angles), descK [nK][32], points [nK][3], dists [nK][2], mask nullable, pointDesc
// nullable [nK][32].  The current frame: kpsC / descC [nC].  pose [12] (R row-major, then t), K [9], bounds [4], scale [nLevels].
// matches [nC] in and out, outlier nullable [nC].  res [13] in the order of orbx_kfproj_result (rounds 0).  Per point (each
// nullable): proj [nK][6] = u, v, the window's radius, the level, zc < 0, and the stage (0 not a point of rule 2 or dropped,
// 2 out of the image, 3 distance, 5 searched); outcome [nK] = the feature it took (-1 none), alone [nK] = the one it takes with
// only the entry's matches taken; best [nK] = bestDist of its turn.
extern "C" void kpr_search_by_projection(const KeyPoint* kpsK, const uint8_t* descK, int nK, const KeyPoint* kpsC, const uint8_t* descC,
                                         int nC, const float* points, const float* dists, const uint8_t* mask, const uint8_t* pointDesc,
                                         const float* pose, const float* K, const int32_t* bounds, const float* scale, int nLevels,
                                         float th, int orbDist, int checkOri, int32_t* matches, const uint8_t* outlier, int32_t* res,
                                         float* proj, int32_t* outcome, int32_t* alone, int32_t* best) {
  enum { STATUS, NMATCHES, POINTS, FOUND, BEHIND_KEPT, OUT_IMAGE, OUT_DISTANCE, WITH_CAND, OVER_DIST, DISPLACED, ROT_REMOVED, CLEARED,
         ROUNDS, FIELDS };
  for (int c = 0; c < FIELDS; c++) res[c] = 0;
  const Grid grid(kpsC, nC, bounds);
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const float* R = pose;
  const float* t = pose + 9;
  const float minX = static_cast<float>(bounds[0]), maxX = static_cast<float>(bounds[1]);
  const float minY = static_cast<float>(bounds[2]), maxY = static_cast<float>(bounds[3]);
  const bool poseOk = finiteAll(pose, 12);
  if (!poseOk) res[STATUS] |= NONFINITE;
  // rule 1
  std::vector<char> found(nK > 0 ? nK : 1, 0), taken(nC > 0 ? nC : 1, 0);
  for (int j = 0; j < nC; j++) {
    const int i = matches[j];
    if (i < 0) continue;
    if (i >= nK) {
      res[STATUS] |= BAD_INPUT;
      taken[j] = 1;
      continue;
    }
    found[i] = 1;
    if (outlier && outlier[j] != 0) {
      matches[j] = -1;
      res[CLEARED]++;
    } else {
      taken[j] = 1;
    }
  }
  const std::vector<char> takenOnEntry = taken;
  std::vector<int> rotHist[HISTO_LENGTH];
  const float factor = HISTO_LENGTH / 360.0f;  // (the corrected factor of matching through the FeatureVector)
  float Ow[3];
  for (int k = 0; k < 3; k++) Ow[k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
  for (int i = 0; i < nK; i++) {
    if (proj) for (int k = 0; k < 6; k++) proj[6 * i + k] = 0.0f;
    if (outcome) outcome[i] = -1;
    if (alone) alone[i] = -1;
    if (best) best[i] = 256;
    if (found[i]) {
      res[FOUND]++;
      continue;
    }
    if (mask && mask[i] == 0) continue;
    res[POINTS]++;
    if (!poseOk) continue;
    // rule 2
    const float* P = points + 3 * (size_t)i;
    const float minDist = dists[2 * (size_t)i], maxDist = dists[2 * (size_t)i + 1];
    if (!finiteAll(P, 3) || !std::isfinite(minDist) || !std::isfinite(maxDist)) {
      res[STATUS] |= NONFINITE;
      continue;
    }
    const float PcX = ((R[0] * P[0] + R[1] * P[1]) + R[2] * P[2]) + t[0];
    const float PcY = ((R[3] * P[0] + R[4] * P[1]) + R[5] * P[2]) + t[1];
    const float PcZ = ((R[6] * P[0] + R[7] * P[1]) + R[8] * P[2]) + t[2];
    const float invz = 1.0f / PcZ;
    const float u = (fx * PcX) * invz + cx;
    const float v = (fy * PcY) * invz + cy;
    if (proj) { proj[6 * i + 4] = PcZ < 0.0f ? 1.0f : 0.0f; proj[6 * i + 5] = 2.0f; }
    if (!std::isfinite(u) || !std::isfinite(v) || u < minX || u > maxX || v < minY || v > maxY) {
      res[OUT_IMAGE]++;
      continue;
    }
    const bool behind = PcZ < 0.0f;
    // rule 3
    const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
    const float dist3D = static_cast<float>(std::sqrt(((double)PO[0] * PO[0] + (double)PO[1] * PO[1]) + (double)PO[2] * PO[2]));
    if (proj) { proj[6 * i] = u; proj[6 * i + 1] = v; proj[6 * i + 5] = 3.0f; }
    if (dist3D < 0.8f * minDist || dist3D > 1.2f * maxDist) {
      if (behind) res[BEHIND_KEPT]++;
      res[OUT_DISTANCE]++;
      continue;
    }
    const float ratio = maxDist / dist3D;
    if (ratio != ratio) {
      res[STATUS] |= NONFINITE;
      if (proj) proj[6 * i + 5] = 0.0f;
      continue;
    }
    if (behind) res[BEHIND_KEPT]++;
    int level = 0;
    for (int n = 0; n < nLevels - 1; n++)
      if (ratio > scale[n]) level++;
    // rule 4
    const float radius = th * scale[level];
    if (proj) { proj[6 * i + 2] = radius; proj[6 * i + 3] = (float)level; proj[6 * i + 5] = 5.0f; }
    const std::vector<int> cand = grid.area(u, v, radius, level - 1, level + 1);
    if (cand.empty()) continue;
    res[WITH_CAND]++;
    // rules 5 and 6
    const uint8_t* dMP = pointDesc ? pointDesc + 32 * (size_t)i : descK + 32 * (size_t)i;
    const int got = pick(cand, taken, dMP, descC, orbDist, best ? best + i : nullptr);
    const int free = pick(cand, takenOnEntry, dMP, descC, orbDist, nullptr);
    if (got < 0) res[OVER_DIST]++;
    if (got != free) res[DISPLACED]++;
    if (outcome) outcome[i] = got;
    if (alone) alone[i] = free;
    if (got >= 0) {
      matches[got] = i;
      taken[got] = 1;
      res[NMATCHES]++;
      if (checkOri) {
        float rot = kpsK[i].angle - kpsC[got].angle;
        if (rot < 0.0f) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == HISTO_LENGTH) bin = 0;
        if (bin >= 0 && bin < HISTO_LENGTH) rotHist[bin].push_back(got);  // (where the design asserts, the match joins no bin)
      }
    }
  }
  // rule 7
  if (checkOri) {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    threeMaxima(rotHist, ind1, ind2, ind3);
    for (int b = 0; b < HISTO_LENGTH; b++) {
      if (b == ind1 || b == ind2 || b == ind3) continue;
      for (int j : rotHist[b]) {
        matches[j] = -1;
        res[NMATCHES]--;
        res[ROT_REMOVED]++;
      }
    }
  }
}
