// match_proj_ref.cpp — CPU restatement of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono = true) as
// include/orbx.h states it ("matching by projection"): the literal sequential loop over the last frame's features with the frame
// grid of SlamTypes/Frame.cpp as vectors per cell, nothing shared with the library.  TEST INFRASTRUCTURE only; compiled on first
// use by tests/match_proj_ref_lib.py with g++ -O2 -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

const int TH_HIGH = 100;
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

  // the candidates with the number of the cell each came from (its place in the walk: cell x outer, cell y inner)
  void area(float x, float y, float r, int minLevel, int maxLevel, std::vector<int>* out, std::vector<int>* outCell) const {
    out->clear();
    if (outCell) outCell->clear();
    const float lox = floorf((x - minX - r) * wInv), hix = ceilf((x - minX + r) * wInv);
    const float loy = floorf((y - minY - r) * hInv), hiy = ceilf((y - minY + r) * hInv);
    // (compared as floats: the same cells as the reference's ints wherever its conversion is defined)
    if (lox >= GRID_COLS) return;
    const int x0 = lox < 0.0f ? 0 : (int)lox;
    if (hix < 0.0f) return;
    const int x1 = hix > GRID_COLS - 1 ? GRID_COLS - 1 : (int)hix;
    if (loy >= GRID_ROWS) return;
    const int y0 = loy < 0.0f ? 0 : (int)loy;
    if (hiy < 0.0f) return;
    const int y1 = hiy > GRID_ROWS - 1 ? GRID_ROWS - 1 : (int)hiy;
    const bool checkLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = x0; ix <= x1; ix++)
      for (int iy = y0; iy <= y1; iy++)
        for (int j : cell[ix][iy]) {
          const KeyPoint& kp = kps[j];
          if (checkLevels && !(kp.octave >= minLevel && kp.octave <= maxLevel)) continue;
          const float dx = kp.x - x, dy = kp.y - y;
          if (fabsf(dx) < r && fabsf(dy) < r) {
            out->push_back(j);
            if (outCell) outCell->push_back(ix * GRID_ROWS + iy);
          }
        }
  }
};

int distance(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

// Features/ORBmatcher.cpp:152-183
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

bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

}  // namespace

// GetFeaturesInArea on a frame of these keypoints: the candidate list in order; returns its length
extern "C" int mpr_features_in_area(const KeyPoint* kps, int n, const int32_t* bounds, float x, float y, float r, int minLevel,
                                    int maxLevel, int32_t* out) {
  const Grid g(kps, n, bounds);
  std::vector<int> c;
  g.area(x, y, r, minLevel, maxLevel, &c, nullptr);
  for (size_t k = 0; k < c.size(); k++) out[k] = c[k];
  return (int)c.size();
}

// One pair.  points [nL][3], mask / pointDesc / lastOutlier nullable, pose [12] (R row-major, then t), K [9], bounds [4],
// scale [nLevels].  matchesCur [nC]; res [8] = status, nmatches, n_points, n_in_image, n_with_candidates, n_displaced,
// n_rot_removed, 0.  Per feature of L (each nullable): proj [nL][4] = u, v, r and the stage reached (0 = skipped by step 2,
// 1 = by step 3, 2 = it has a window); freePick [nL] = the candidate it takes with nothing taken (-1 none); outcome [nL] = the
// one it took (before the histogram); takenAhead [nL] = the taken candidates of its window that rank before its outcome (for an
// outcome of none: those within TH_HIGH).
extern "C" void mpr_search_by_projection(const KeyPoint* kpsL, const uint8_t* descL, int nL, const KeyPoint* kpsC,
                                         const uint8_t* descC, int nC, const float* points, const uint8_t* mask,
                                         const uint8_t* pointDesc, const uint8_t* lastOutlier, const float* pose, const float* K,
                                         const int32_t* bounds, const float* scale, int nLevels, float th, int checkOrientation,
                                         int32_t* matchesCur, int32_t* res, float* proj, int32_t* freePick, int32_t* outcome,
                                         int32_t* takenAhead) {
  const Grid grid(kpsC, nC, bounds);
  for (int j = 0; j < nC; j++) matchesCur[j] = -1;
  for (int c = 0; c < 8; c++) res[c] = 0;
  std::vector<int> rotHist[HISTO_LENGTH];
  const float factor = HISTO_LENGTH / 360.0f;
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const float* R = pose;
  const float* t = pose + 9;
  const float minX = static_cast<float>(bounds[0]), maxX = static_cast<float>(bounds[1]);
  const float minY = static_cast<float>(bounds[2]), maxY = static_cast<float>(bounds[3]);
  for (int k = 0; k < 12; k++)
    if (!std::isfinite(pose[k])) res[0] |= NONFINITE;
  int nmatches = 0;
  std::vector<int> cand, candCell;
  for (int i = 0; i < nL; i++) {
    if (proj) proj[4 * i] = proj[4 * i + 1] = proj[4 * i + 2] = proj[4 * i + 3] = 0.0f;
    if (freePick) freePick[i] = -1;
    if (outcome) outcome[i] = -1;
    if (takenAhead) takenAhead[i] = 0;
    // step 2
    if (mask && mask[i] == 0) continue;
    if (lastOutlier && lastOutlier[i] != 0) continue;
    const int o = kpsL[i].octave;
    if (o < 0 || o >= nLevels) {
      res[0] |= BAD_INPUT;
      continue;
    }
    res[2]++;
    // step 3
    const float* X = points + 3 * (size_t)i;
    if (!finite3(X)) res[0] |= NONFINITE;
    const float xc = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + t[0];
    const float yc = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + t[1];
    const float zc = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + t[2];
    const float invz = 1.0f / zc;
    if (proj) proj[4 * i + 3] = 1.0f;
    if (invz < 0) continue;
    const float u = (fx * xc) * invz + cx;
    const float v = (fy * yc) * invz + cy;
    if (!std::isfinite(u) || !std::isfinite(v)) continue;
    if (u < minX || u > maxX) continue;
    if (v < minY || v > maxY) continue;
    res[3]++;
    // step 4
    const float radius = th * scale[o];
    if (proj) { proj[4 * i] = u; proj[4 * i + 1] = v; proj[4 * i + 2] = radius; proj[4 * i + 3] = 2.0f; }
    grid.area(u, v, radius, o - 1, o + 1, &cand, &candCell);
    if (cand.empty()) continue;
    res[4]++;
    // step 5
    const uint8_t* dMP = pointDesc ? pointDesc + 32 * (size_t)i : descL + 32 * (size_t)i;
    int bestDist = 256, bestIdx2 = -1, freeDist = 256, freeIdx = -1;
    size_t bestAt = cand.size();
    for (size_t k = 0; k < cand.size(); k++) {
      const int i2 = cand[k];
      const int dist = distance(dMP, descC + 32 * (size_t)i2);
      if (dist < freeDist) { freeDist = dist; freeIdx = i2; }
      if (matchesCur[i2] >= 0) continue;
      if (dist < bestDist) { bestDist = dist; bestIdx2 = i2; bestAt = k; }
    }
    if (freeDist > TH_HIGH) freeIdx = -1;
    const int got = bestDist <= TH_HIGH ? bestIdx2 : -1;
    if (got != freeIdx) res[5]++;
    int ahead = 0;
    for (size_t k = 0; k < cand.size(); k++) {
      if (matchesCur[cand[k]] < 0) continue;
      const int dist = distance(dMP, descC + 32 * (size_t)cand[k]);
      if (got >= 0 ? (dist < bestDist || (dist == bestDist && k < bestAt)) : dist <= TH_HIGH) ahead++;
    }
    if (freePick) freePick[i] = freeIdx;
    if (outcome) outcome[i] = got;
    if (takenAhead) takenAhead[i] = ahead;
    // step 6
    if (bestDist <= TH_HIGH) {
      matchesCur[bestIdx2] = i;
      nmatches++;
      if (checkOrientation) {
        float rot = kpsL[i].angle - kpsC[bestIdx2].angle;
        if (rot < 0.0f) rot += 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == HISTO_LENGTH) bin = 0;
        if (bin >= 0 && bin < HISTO_LENGTH) rotHist[bin].push_back(bestIdx2);
      }
    }
  }
  // step 7
  if (checkOrientation) {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    computeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
    for (int i = 0; i < HISTO_LENGTH; i++) {
      if (i == ind1 || i == ind2 || i == ind3) continue;
      for (int j : rotHist[i]) {
        matchesCur[j] = -1;
        nmatches--;
        res[6]++;
      }
    }
  }
  res[1] = nmatches;
}
