// match_local_ref.cpp — CPU restatement of Tracking::SearchLocalPoints as include/orbx.h states it ("matching the local map by
// projection"): the points the frame has, Frame::isInFrustum, MapPoint::PredictScale in table form and
// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) -- the literal sequential loops, with the frame grid of
// SlamTypes/Frame.cpp as vectors per cell, nothing shared with the library.  TEST INFRASTRUCTURE only; compiled on first use by
// tests/match_local_ref_lib.py with g++ -O2 -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

const int TH_HIGH = 100;
const int GRID_COLS = 64, GRID_ROWS = 48;
const int BAD_INPUT = 2, NONFINITE = 4;
const uint8_t NOT_IN_VIEW = 0xFF, SEEN = 0xFE;

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

int predictScale(float ratio, const float* scale, int nLevels) {
  int level = 0;
  for (int n = 0; n < nLevels - 1; n++)
    if (ratio > scale[n]) level++;
  return level;
}

// steps 5 and 6 over the candidates `cand` that `skip` does not hold: the feature or -1; why = 1 over TH_HIGH, 2 the ratio test.
// best [4] = bestDist, bestDist2, bestLevel, bestLevel2
int pick(const std::vector<int>& cand, const std::vector<char>& skip, const uint8_t* dMP, const uint8_t* desc, const KeyPoint* kps,
         float nnratio, int* why, int32_t* best) {
  int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
  for (int idx : cand) {
    if (skip[idx]) continue;
    const int dist = distance(dMP, desc + 32 * (size_t)idx);
    if (dist < bestDist) {
      bestDist2 = bestDist;
      bestDist = dist;
      bestLevel2 = bestLevel;
      bestLevel = kps[idx].octave;
      bestIdx = idx;
    } else if (dist < bestDist2) {
      bestLevel2 = kps[idx].octave;
      bestDist2 = dist;
    }
  }
  if (best) { best[0] = bestDist; best[1] = bestDist2; best[2] = bestLevel; best[3] = bestLevel2; }
  *why = 1;
  if (bestDist <= TH_HIGH) {
    *why = 2;
    if (bestLevel == bestLevel2 && static_cast<float>(bestDist) > nnratio * static_cast<float>(bestDist2)) return -1;
    *why = 0;
    return bestIdx;
  }
  return -1;
}

}  // namespace

extern "C" int mlr_features_in_area(const KeyPoint* kps, int n, const int32_t* bounds, float x, float y, float r, int minLevel,
                                    int maxLevel, int32_t* out) {
  const Grid g(kps, n, bounds);
  const std::vector<int> c = g.area(x, y, r, minLevel, maxLevel);
  for (size_t k = 0; k < c.size(); k++) out[k] = c[k];
  return (int)c.size();
}

// the table PredictScale for n ratios
extern "C" void mlr_predict_scale(const float* ratio, int n, const float* scale, int nLevels, int32_t* out) {
  for (int k = 0; k < n; k++) out[k] = predictScale(ratio[k], scale, nLevels);
}

// One pair.  kps / desc [nF]; the map: points [nM][3], normals [nM][3], dists [nM][2], mapDesc [nM][32], mask nullable; pose
// [12] (R row-major, then t), K [9], bounds [4], scale [nLevels].  matches [nF] in and out, outlier nullable.  res [15] in the
// order of orbx_local_result (rounds 0); view [nM] nullable.  Per point (each nullable): proj [nM][6] = u, v, the window's
// radius, the level, viewCos and the stage (0 not a point of step 2 or dropped, 1 behind, 2 out of the image, 3 distance, 4
// angle, 5 in view); outcome [nM] = the feature it took (-1 none), alone [nM] = the one it takes with only the entry's matches
// taken; best [nM][4] = bestDist, bestDist2, bestLevel, bestLevel2 of its turn.
extern "C" void mlr_search_local_points(const KeyPoint* kps, const uint8_t* desc, int nF, int nM, const float* points,
                                        const float* normals, const float* dists, const uint8_t* mapDesc, const uint8_t* mask,
                                        const float* pose, const float* K, const int32_t* bounds, const float* scale, int nLevels,
                                        float th, float nnratio, int32_t* matches, const uint8_t* outlier, int32_t* res,
                                        uint8_t* view, float* proj, int32_t* outcome, int32_t* alone, int32_t* best) {
  enum { STATUS, NMATCHES, POINTS, N_SEEN, BEHIND, OUT_IMAGE, OUT_DISTANCE, OUT_ANGLE, IN_VIEW, WITH_CAND, OVER_TH, RATIO, DISPLACED,
         CLEARED, ROUNDS, FIELDS };
  for (int c = 0; c < FIELDS; c++) res[c] = 0;
  const Grid grid(kps, nF, bounds);
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const float* R = pose;
  const float* t = pose + 9;
  const float minX = static_cast<float>(bounds[0]), maxX = static_cast<float>(bounds[1]);
  const float minY = static_cast<float>(bounds[2]), maxY = static_cast<float>(bounds[3]);
  const bool poseOk = finiteAll(pose, 12);
  if (!poseOk) res[STATUS] |= NONFINITE;
  // step 1
  std::vector<char> seen(nM > 0 ? nM : 1, 0), taken(nF > 0 ? nF : 1, 0);
  for (int j = 0; j < nF; j++) {
    const int i = matches[j];
    if (i < 0) continue;
    if (i >= nM) {
      res[STATUS] |= BAD_INPUT;
      taken[j] = 1;
      continue;
    }
    seen[i] = 1;
    if (outlier && outlier[j] != 0) {
      matches[j] = -1;
      res[CLEARED]++;
    } else {
      taken[j] = 1;
    }
  }
  const std::vector<char> takenOnEntry = taken;
  float Ow[3];
  for (int k = 0; k < 3; k++) Ow[k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
  for (int i = 0; i < nM; i++) {
    if (proj) for (int k = 0; k < 6; k++) proj[6 * i + k] = 0.0f;
    if (outcome) outcome[i] = -1;
    if (alone) alone[i] = -1;
    if (best) { best[4 * i] = best[4 * i + 1] = 256; best[4 * i + 2] = best[4 * i + 3] = -1; }
    if (view) view[i] = seen[i] ? SEEN : NOT_IN_VIEW;
    if (seen[i]) {
      res[N_SEEN]++;
      continue;
    }
    if (mask && mask[i] == 0) continue;
    res[POINTS]++;
    if (!poseOk) continue;
    // step 2
    const float* P = points + 3 * (size_t)i;
    const float* N = normals + 3 * (size_t)i;
    const float minDist = dists[2 * (size_t)i], maxDist = dists[2 * (size_t)i + 1];
    if (!finiteAll(P, 3) || !finiteAll(N, 3) || !std::isfinite(minDist) || !std::isfinite(maxDist)) {
      res[STATUS] |= NONFINITE;
      continue;
    }
    const float PcX = ((R[0] * P[0] + R[1] * P[1]) + R[2] * P[2]) + t[0];
    const float PcY = ((R[3] * P[0] + R[4] * P[1]) + R[5] * P[2]) + t[1];
    const float PcZ = ((R[6] * P[0] + R[7] * P[1]) + R[8] * P[2]) + t[2];
    if (proj) proj[6 * i + 5] = 1.0f;
    if (PcZ < 0.0f) {
      res[BEHIND]++;
      continue;
    }
    const float invz = 1.0f / PcZ;
    const float u = (fx * PcX) * invz + cx;
    const float v = (fy * PcY) * invz + cy;
    if (proj) proj[6 * i + 5] = 2.0f;
    if (!std::isfinite(u) || !std::isfinite(v) || u < minX || u > maxX || v < minY || v > maxY) {
      res[OUT_IMAGE]++;
      continue;
    }
    const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
    const float dist = static_cast<float>(std::sqrt(((double)PO[0] * PO[0] + (double)PO[1] * PO[1]) + (double)PO[2] * PO[2]));
    if (proj) proj[6 * i + 5] = 3.0f;
    if (dist < 0.8f * minDist || dist > 1.2f * maxDist) {
      res[OUT_DISTANCE]++;
      continue;
    }
    const float viewCos = static_cast<float>((((double)PO[0] * N[0] + (double)PO[1] * N[1]) + (double)PO[2] * N[2]) / (double)dist);
    if (proj) { proj[6 * i + 4] = viewCos; proj[6 * i + 5] = 4.0f; }
    if (viewCos < 0.5f) {
      res[OUT_ANGLE]++;
      continue;
    }
    // step 3
    const float ratio = maxDist / dist;
    if (ratio != ratio) {
      res[STATUS] |= NONFINITE;
      if (proj) proj[6 * i + 5] = 0.0f;
      continue;
    }
    const int level = predictScale(ratio, scale, nLevels);
    res[IN_VIEW]++;
    if (view) view[i] = (uint8_t)level;
    // step 4
    float r = viewCos > 0.998f ? 2.5f : 4.0f;
    if (th != 1.0f) r *= th;
    const float radius = r * scale[level];
    if (proj) { proj[6 * i] = u; proj[6 * i + 1] = v; proj[6 * i + 2] = radius; proj[6 * i + 3] = (float)level; proj[6 * i + 5] = 5.0f; }
    const std::vector<int> cand = grid.area(u, v, radius, level - 1, level);
    if (cand.empty()) continue;
    res[WITH_CAND]++;
    // steps 5 and 6
    const uint8_t* dMP = mapDesc + 32 * (size_t)i;
    int why, whyAlone;
    const int got = pick(cand, taken, dMP, desc, kps, nnratio, &why, best ? best + 4 * i : nullptr);
    const int free = pick(cand, takenOnEntry, dMP, desc, kps, nnratio, &whyAlone, nullptr);
    if (why == 1) res[OVER_TH]++;
    if (why == 2) res[RATIO]++;
    if (got != free) res[DISPLACED]++;
    if (outcome) outcome[i] = got;
    if (alone) alone[i] = free;
    if (got >= 0) {
      matches[got] = i;
      taken[got] = 1;
      res[NMATCHES]++;
    }
  }
}
