// fuse_ref.cpp — CPU restatement of both overloads of ORBmatcher::Fuse as include/orbx.h states them ("fusing map points into a
// keyframe"): the literal sequential loop over the points with the literal state (the row, and a plain 64-bit count per feature),
// with the frame grid of SlamTypes/Frame.cpp as vectors per cell, nothing shared with the library.  TEST INFRASTRUCTURE only;
// compiled on first use by tests/fuse_ref_lib.py with g++ -O2 -ffp-contract=off.
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

const int GRID_COLS = 64, GRID_ROWS = 48;
const int BAD_INPUT = 2, NONFINITE = 4;
const int OCCUPIED_UNMAPPED = -2;
enum { NONE, ADD, KEEP_OCCUPANT, REPLACE_OCCUPANT, BAD_OCCUPANT };

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

// a count as R3 reads it
long long readObs(int raw, int32_t* status) {
  if (raw < 0) {
    *status |= BAD_INPUT;
    return 0;
  }
  if (raw > 65535) {
    *status |= BAD_INPUT;
    return 65535;
  }
  return raw;
}

}  // namespace

extern "C" int fr_features_in_area(const KeyPoint* kps, int n, const int32_t* bounds, float x, float y, float r, int minLevel,
                                   int maxLevel, int32_t* out) {
  const Grid g(kps, n, bounds);
  const std::vector<int> c = g.area(x, y, r, minLevel, maxLevel);
  for (size_t k = 0; k < c.size(); k++) out[k] = c[k];
  return (int)c.size();
}

// One pair, either form.  kps / desc [nF]; the map: points [nM][3], normals [nM][3], dists [nM][2], mapDesc [nM][32], mask nullable,
// mapObs [nM] (pose form); T [12]: Rcw row-major then tcw, or with scwForm sR row-major then t; K [9], bounds [4], scale and
// invSigma2 [nLevels].  matches [nF] in and out; occObs [nF] nullable.  idx / act / other [nM]; res [16] in the order of
// orbx_fuse_result (rounds 0).  Per point (each nullable): stage [nM] (0 in the keyframe or masked out, 1 dropped, 2 behind, 3 out
// of the image, 4 distance, 5 angle, 6 searched); proj [nM][4] = u, v, the window's radius, the level of a searched point.
extern "C" void fr_fuse(int scwForm, const KeyPoint* kps, const uint8_t* desc, int nF, int nM, const float* points, const float* normals,
                        const float* dists, const uint8_t* mapDesc, const uint8_t* mask, const int32_t* mapObs, const float* T,
                        const float* K, const int32_t* bounds, const float* scale, const float* invSigma2, int nLevels, float th,
                        int thLow, int32_t* matches, const int32_t* occObs, int32_t* idx, uint8_t* act, int32_t* other, int32_t* res,
                        int32_t* stage, float* proj) {
  enum { STATUS, FUSED, POINTS, IN_KF, BEHIND, OUT_IMAGE, OUT_DISTANCE, OUT_ANGLE, WITH_CAND, OVER_DIST, ADDED, KEPT, REPLACED, BAD_OCC,
         CHAINED, ROUNDS, FIELDS };
  for (int c = 0; c < FIELDS; c++) res[c] = 0;
  const Grid grid(kps, nF, bounds);
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const float minX = static_cast<float>(bounds[0]), maxX = static_cast<float>(bounds[1]);
  const float minY = static_cast<float>(bounds[2]), maxY = static_cast<float>(bounds[3]);
  // the pose
  float R[9], t[3], Ow[3];
  bool poseOk = finiteAll(T, 12);
  if (scwForm) {
    const float scw2 = (T[0] * T[0] + T[1] * T[1]) + T[2] * T[2];
    const float s = static_cast<float>(std::sqrt(static_cast<double>(scw2)));
    poseOk = poseOk && s > 0.0f && std::isfinite(s);
    for (int k = 0; k < 9; k++) R[k] = T[k] / s;
    for (int k = 0; k < 3; k++) t[k] = T[9 + k] / s;
    poseOk = poseOk && finiteAll(R, 9) && finiteAll(t, 3);
  } else {
    for (int k = 0; k < 9; k++) R[k] = T[k];
    for (int k = 0; k < 3; k++) t[k] = T[9 + k];
  }
  if (!poseOk) res[STATUS] |= NONFINITE;
  for (int k = 0; k < 3; k++) Ow[k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
  // rule 1: the entry
  std::vector<char> inKf(nM > 0 ? nM : 1, 0);
  for (int j = 0; j < nF; j++) {
    const int e = matches[j];
    if (e >= nM) res[STATUS] |= BAD_INPUT;
    else if (e >= 0) inKf[e] = 1;
    else if (!scwForm && e == OCCUPIED_UNMAPPED && !occObs) res[STATUS] |= BAD_INPUT;
  }
  // the sequential loop's state beside the row: the modelled count of a feature's occupant once this call has decided on it
  std::vector<long long> count(nF > 0 ? nF : 1, 0);
  std::vector<char> decided(nF > 0 ? nF : 1, 0);
  for (int i = 0; i < nM; i++) {
    idx[i] = -1;
    act[i] = NONE;
    other[i] = -1;
    if (stage) stage[i] = 0;
    if (proj) for (int k = 0; k < 4; k++) proj[4 * i + k] = 0.0f;
    if (inKf[i]) {
      res[IN_KF]++;
      continue;
    }
    if (mask && mask[i] == 0) continue;
    res[POINTS]++;
    if (stage) stage[i] = 1;
    if (!poseOk) continue;
    const float* P = points + 3 * (size_t)i;
    const float* N = normals + 3 * (size_t)i;
    const float minDist = dists[2 * (size_t)i], maxDist = dists[2 * (size_t)i + 1];
    if (!finiteAll(P, 3) || !finiteAll(N, 3) || !std::isfinite(minDist) || !std::isfinite(maxDist)) {
      res[STATUS] |= NONFINITE;
      continue;
    }
    // rule 2
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
    // rule 3
    const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
    const float dist = static_cast<float>(std::sqrt(((double)PO[0] * PO[0] + (double)PO[1] * PO[1]) + (double)PO[2] * PO[2]));
    if (dist < 0.8f * minDist || dist > 1.2f * maxDist) {
      res[OUT_DISTANCE]++;
      if (stage) stage[i] = 4;
      continue;
    }
    const double dot = ((double)PO[0] * N[0] + (double)PO[1] * N[1]) + (double)PO[2] * N[2];
    if (dot < 0.5 * dist) {
      res[OUT_ANGLE]++;
      if (stage) stage[i] = 5;
      continue;
    }
    // rule 4
    const float ratio = maxDist / dist;
    if (ratio != ratio) {
      res[STATUS] |= NONFINITE;
      continue;
    }
    const int level = predictScale(ratio, scale, nLevels);
    const float radius = th * scale[level];
    if (stage) stage[i] = 6;
    if (proj) { proj[4 * i] = u; proj[4 * i + 1] = v; proj[4 * i + 2] = radius; proj[4 * i + 3] = (float)level; }
    const std::vector<int> vIndices = grid.area(u, v, radius, -1, -1);
    if (vIndices.empty()) continue;
    res[WITH_CAND]++;
    // rules 4 to 6
    const uint8_t* dMP = mapDesc + 32 * (size_t)i;
    int bestDist = scwForm ? INT_MAX : 256, bestIdx = -1;
    for (int j : vIndices) {
      const KeyPoint& kp = kps[j];
      const int kpLevel = kp.octave;
      if (kpLevel < level - 1 || kpLevel > level) continue;
      if (!scwForm) {
        if (kpLevel < 0) continue;
        const float ex = u - kp.x, ey = v - kp.y;
        const float e2 = ex * ex + ey * ey;
        if (e2 * invSigma2[kpLevel] > 5.99) continue;
      }
      const int d = distance(dMP, desc + 32 * (size_t)j);
      if (d < bestDist) {
        bestDist = d;
        bestIdx = j;
      }
    }
    if (!(bestIdx >= 0 && bestDist <= thLow)) {
      res[OVER_DIST]++;
      continue;
    }
    // the resolution
    const int f = bestIdx;
    idx[i] = f;
    res[FUSED]++;
    const long long obs = scwForm ? 0 : readObs(mapObs[i], &res[STATUS]);
    const int occ = matches[f];
    if (occ < 0 && occ != OCCUPIED_UNMAPPED) {  // R1
      matches[f] = i;
      act[i] = ADD;
      res[ADDED]++;
      count[f] = obs + 1;
      decided[f] = 1;
      continue;
    }
    other[i] = occ;
    bool bad;
    if (occ >= nM) bad = true;
    else if (occ >= 0) bad = mask && mask[occ] == 0;
    else bad = scwForm ? (occObs && occObs[f] < 0) : (!occObs || occObs[f] < 0);
    if (bad) {  // R2
      act[i] = BAD_OCCUPANT;
      res[BAD_OCC]++;
      continue;
    }
    if (decided[f]) res[CHAINED]++;
    if (scwForm) {  // R4
      act[i] = KEEP_OCCUPANT;
      res[KEPT]++;
      decided[f] = 1;
      continue;
    }
    // R3
    if (!decided[f]) count[f] = readObs(occ >= 0 ? mapObs[occ] : occObs[f], &res[STATUS]);
    if (count[f] > obs) {
      act[i] = KEEP_OCCUPANT;
      res[KEPT]++;
    } else {
      act[i] = REPLACE_OCCUPANT;
      matches[f] = i;
      res[REPLACED]++;
    }
    count[f] = obs + count[f];
    decided[f] = 1;
  }
}
