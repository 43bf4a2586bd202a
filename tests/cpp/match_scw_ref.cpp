// match_scw_ref.cpp — CPU restatement of the loop-closing overload ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
// and of the composition Scw = S12 * Tmw in front of it, as include/orbx.h states them ("loop closing: matching the loop's points
// under Scw"): the literal sequential loops, with the frame grid of SlamTypes/Frame.cpp as vectors per cell, nothing shared with
// the library.  TEST INFRASTRUCTURE only; compiled on first use by tests/match_scw_ref_lib.py with g++ -O2 -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

const int GRID_COLS = 64, GRID_ROWS = 48;
const int BAD_INPUT = 2, NONFINITE = 4;
const int TAKEN_UNMAPPED = -2;

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

// rule 7 over the candidates `cand` that `skip` does not hold: the feature or -1; *bestDist as the loop leaves it
int pick(const std::vector<int>& cand, const std::vector<char>& skip, const uint8_t* dMP, const uint8_t* desc, int thLow, int* best) {
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
  return (bestIdx >= 0 && bestDist <= thLow) ? bestIdx : -1;
}

}  // namespace

extern "C" int msr_features_in_area(const KeyPoint* kps, int n, const int32_t* bounds, float x, float y, float r, int minLevel,
                                    int maxLevel, int32_t* out) {
  const Grid g(kps, n, bounds);
  const std::vector<int> c = g.area(x, y, r, minLevel, maxLevel);
  for (size_t k = 0; k < c.size(); k++) out[k] = c[k];
  return (int)c.size();
}

// Scw = S12 * Tmw: pose2 [12] (Rmw row-major, tmw), sim3 [13] (R12 row-major, t12, s12) -> scw [12]
extern "C" void msr_compose_scw(const float* pose2, const float* sim3, float* scw) {
  const float s12 = sim3[12];
  if (!finiteAll(pose2, 12) || !finiteAll(sim3, 13) || !(s12 > 0.0f)) {
    for (int k = 0; k < 12; k++) scw[k] = 0.0f;
    return;
  }
  const double s = s12;
  for (int r = 0; r < 3; r++) {
    const double a = sim3[3 * r], b = sim3[3 * r + 1], c = sim3[3 * r + 2];
    for (int col = 0; col < 3; col++) {
      const double m = (a * (double)pose2[col] + b * (double)pose2[3 + col]) + c * (double)pose2[6 + col];
      scw[3 * r + col] = static_cast<float>(s * m);
    }
    const double q = (a * (double)pose2[9] + b * (double)pose2[10]) + c * (double)pose2[11];
    scw[9 + r] = static_cast<float>(s * q + (double)sim3[9 + r]);
  }
}

// One pair.  kps / desc [nF]; the map: points [nM][3], normals [nM][3], dists [nM][2], mapDesc [nM][32], mask nullable; scw [12]
// (sR row-major, then t), K [9], bounds [4], scale [nLevels].  matches [nF] in and out; table [nTable] nullable.  res [14] in the
// order of orbx_scw_result (rounds 0).  Per point (each nullable): stage [nM] (0 found or masked out, 1 dropped, 2 behind, 3 out
// of the image, 4 distance, 5 angle, 6 searched); proj [nM][4] = u, v, the window's radius, the level of a searched point;
// outcome [nM] = the feature it took (-1 none), alone [nM] = the one it takes with only the entry's matches taken; best [nM] =
// bestDist of its turn (256 without an untaken candidate).
extern "C" void msr_search_scw(const KeyPoint* kps, const uint8_t* desc, int nF, int nM, const float* points, const float* normals,
                               const float* dists, const uint8_t* mapDesc, const uint8_t* mask, const float* scw, const float* K,
                               const int32_t* bounds, const float* scale, int nLevels, float th, int thLow, int32_t* matches,
                               const int32_t* table, int nTable, int32_t* res, int32_t* stage, float* proj, int32_t* outcome,
                               int32_t* alone, int32_t* best) {
  enum { STATUS, NMATCHES, TOTAL, POINTS, FOUND, UNMAPPED, BEHIND, OUT_IMAGE, OUT_DISTANCE, OUT_ANGLE, WITH_CAND, OVER_DIST, DISPLACED,
         ROUNDS, FIELDS };
  for (int c = 0; c < FIELDS; c++) res[c] = 0;
  const Grid grid(kps, nF, bounds);
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const float minX = static_cast<float>(bounds[0]), maxX = static_cast<float>(bounds[1]);
  const float minY = static_cast<float>(bounds[2]), maxY = static_cast<float>(bounds[3]);
  // rule 1
  bool simOk = finiteAll(scw, 12);
  const float scw2 = (scw[0] * scw[0] + scw[1] * scw[1]) + scw[2] * scw[2];
  const float s = static_cast<float>(std::sqrt(static_cast<double>(scw2)));
  simOk = simOk && s > 0.0f && std::isfinite(s);
  float R[9], t[3], Ow[3];
  for (int k = 0; k < 9; k++) R[k] = scw[k] / s;
  for (int k = 0; k < 3; k++) t[k] = scw[9 + k] / s;
  simOk = simOk && finiteAll(R, 9) && finiteAll(t, 3);
  if (!simOk) res[STATUS] |= NONFINITE;
  for (int k = 0; k < 3; k++) Ow[k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
  // rule 2
  std::vector<char> found(nM > 0 ? nM : 1, 0), taken(nF > 0 ? nF : 1, 0);
  for (int j = 0; j < nF; j++) {
    int i = matches[j];
    if (i == TAKEN_UNMAPPED) {
      taken[j] = 1;
      res[UNMAPPED]++;
      continue;
    }
    if (i < 0) continue;
    taken[j] = 1;
    if (table) {
      if (i >= nTable) {
        res[STATUS] |= BAD_INPUT;
        continue;
      }
      i = table[i];
      if (i < 0) {
        matches[j] = TAKEN_UNMAPPED;
        res[UNMAPPED]++;
        continue;
      }
    }
    if (i >= nM) {
      res[STATUS] |= BAD_INPUT;
      continue;
    }
    matches[j] = i;
    found[i] = 1;
  }
  const std::vector<char> takenOnEntry = taken;
  for (int i = 0; i < nM; i++) {
    if (stage) stage[i] = 0;
    if (proj) for (int k = 0; k < 4; k++) proj[4 * i + k] = 0.0f;
    if (outcome) outcome[i] = -1;
    if (alone) alone[i] = -1;
    if (best) best[i] = 256;
    if (found[i]) {
      res[FOUND]++;
      continue;
    }
    if (mask && mask[i] == 0) continue;
    res[POINTS]++;
    if (stage) stage[i] = 1;
    if (!simOk) continue;
    // rule 3
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
    if (PcZ < 0.0f) {
      res[BEHIND]++;
      if (stage) stage[i] = 2;
      continue;
    }
    const float invz = 1.0f / PcZ;
    const float x = PcX * invz, y = PcY * invz;
    const float u = fx * x + cx;
    const float v = fy * y + cy;
    if (!(u >= minX && u < maxX && v >= minY && v < maxY)) {  // KeyFrame::IsInImage
      res[OUT_IMAGE]++;
      if (stage) stage[i] = 3;
      continue;
    }
    // rule 4
    const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
    const float dist = static_cast<float>(std::sqrt(((double)PO[0] * PO[0] + (double)PO[1] * PO[1]) + (double)PO[2] * PO[2]));
    if (dist < 0.8f * minDist || dist > 1.2f * maxDist) {
      res[OUT_DISTANCE]++;
      if (stage) stage[i] = 4;
      continue;
    }
    // rule 5
    const double dot = ((double)PO[0] * N[0] + (double)PO[1] * N[1]) + (double)PO[2] * N[2];
    if (dot < 0.5 * dist) {
      res[OUT_ANGLE]++;
      if (stage) stage[i] = 5;
      continue;
    }
    // rule 6
    const float ratio = maxDist / dist;
    if (ratio != ratio) {
      res[STATUS] |= NONFINITE;
      continue;
    }
    const int level = predictScale(ratio, scale, nLevels);
    const float radius = th * scale[level];
    if (stage) stage[i] = 6;
    if (proj) { proj[4 * i] = u; proj[4 * i + 1] = v; proj[4 * i + 2] = radius; proj[4 * i + 3] = (float)level; }
    std::vector<int> cand;
    for (int j : grid.area(u, v, radius, -1, -1)) {
      const int kpLevel = kps[j].octave;
      if (kpLevel < level - 1 || kpLevel > level) continue;
      cand.push_back(j);
    }
    if (cand.empty()) continue;
    res[WITH_CAND]++;
    // rule 7
    const uint8_t* dMP = mapDesc + 32 * (size_t)i;
    const int got = pick(cand, taken, dMP, desc, thLow, best ? best + i : nullptr);
    const int free = pick(cand, takenOnEntry, dMP, desc, thLow, nullptr);
    if (got < 0) res[OVER_DIST]++;
    if (got != free) res[DISPLACED]++;
    if (outcome) outcome[i] = got;
    if (alone) alone[i] = free;
    if (got >= 0) {
      matches[got] = i;
      taken[got] = 1;
      res[NMATCHES]++;
    }
  }
  // rule 8
  for (int j = 0; j < nF; j++)
    if (matches[j] >= 0 || matches[j] == TAKEN_UNMAPPED) res[TOTAL]++;
}
