// map_update_ref_main.cpp — a stand-alone program over tests/cpp/map_update_ref.cpp for the sanitizers (TEST INFRASTRUCTURE; built
// by tests/test_map_update_host.py with -fsanitize=address,undefined): the restatement over small synthetic windows, under each
// value of `what`, and over every garbage case of include/orbx.h, "local mapping: updating the map points", rule 7.  It checks
// the status of each run and that a flagged problem comes back as it went in; what it is for is that the sanitizers see every
// step run, also on garbage.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/orbx.h"

extern "C" void mapr_update(const orbx_keypoint* kps, const uint8_t* desc, const int32_t* n, const int32_t* frameOf, int nE, int nF,
                            const float* pose, int32_t* rows, const uint8_t* outlier, int cap, const float* mapPts, const uint8_t* mask,
                            uint8_t* maskOut, int32_t* mapRef, int mapN, int mapCap, const float* scale, int nLevels, int what,
                            float* normals, float* dist, uint8_t* mapDesc, int32_t* mapObs, orbx_map_result* res);

namespace {

constexpr int NLEVELS = 8;

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  double unit() { return next() / 2147483648.0; }
};

struct Window {
  int nE, nF, cap, mapN, mapCap;
  std::vector<orbx_keypoint> kps;
  std::vector<uint8_t> desc, outlier, mask;
  std::vector<int32_t> n, rows, frames, ref;
  std::vector<float> pose, pts;
};

struct Out {
  std::vector<int32_t> rows, ref, obs;
  std::vector<uint8_t> maskOut, desc;
  std::vector<float> normals, dist;
  orbx_map_result res;
};

// nE cameras on a baseline (identity rotations), nP points 4 to 8 deep, camera e sees point j when (e + j) % stride == 0 or e == j % nE
Window make(int nE, int nF, int nP, int stride, double erase, uint64_t seed) {
  Rng r{seed};
  Window w;
  w.nE = nE; w.nF = nF; w.cap = nP + 3; w.mapN = nP; w.mapCap = nP + 2;
  const size_t ne = (size_t)(nE ? nE : 1);
  w.kps.assign(ne * w.cap, orbx_keypoint{});
  w.desc.assign(ne * w.cap * 32, 0);
  w.outlier.assign(ne * w.cap, 0);
  w.n.assign(ne, 0);
  w.rows.assign(ne * w.cap, -1);
  w.frames.assign(ne, 0);
  w.pose.assign(ne * 12, 0.f);
  w.pts.assign((size_t)w.mapCap * 3, 0.f);
  w.mask.assign(w.mapCap, 0);
  w.ref.assign(w.mapCap, -1);
  for (int j = 0; j < nP; j++) {
    w.pts[j * 3] = (float)(4.0 * r.unit() - 2.0);
    w.pts[j * 3 + 1] = (float)(3.0 * r.unit() - 1.5);
    w.pts[j * 3 + 2] = (float)(4.0 + 4.0 * r.unit());
    w.mask[j] = j % 11 != 10;
    w.ref[j] = j % 3 == 0 ? -1 : (j % 3 == 1 ? j % (nE ? nE : 1) : nE + 3);
  }
  for (auto& b : w.desc) b = (uint8_t)r.next();
  for (int e = 0; e < nE; e++) {
    w.frames[e] = nE - 1 - e;  // (entries and frames differ)
    float* p = &w.pose[(size_t)e * 12];
    p[0] = p[4] = p[8] = 1.f;
    p[9] = -0.25f * e;
    int f = 0;
    const int fr = w.frames[e];
    for (int j = 0; j < nP; j++)
      if ((e + j) % stride == 0 || e == j % nE) {
        w.kps[(size_t)fr * w.cap + f].octave = (int)(r.next() % NLEVELS);
        if (r.unit() < erase) w.outlier[(size_t)e * w.cap + f] = 1;
        w.rows[(size_t)e * w.cap + f++] = j;
      }
    w.rows[(size_t)e * w.cap + f++] = -2;
    w.outlier[(size_t)e * w.cap + f - 1] = 1;  // (a byte on a feature that names nothing)
    w.n[fr] = f + 1;
  }
  return w;
}

Out run(const Window& w, int what, bool withOutlier, bool withRef, bool withMask) {
  Out o;
  o.rows = w.rows;
  o.ref = w.ref;
  o.maskOut = w.mask;
  o.obs.assign(w.mapCap, -7);
  o.desc.assign((size_t)w.mapCap * 32, 0xA5);
  o.normals.assign((size_t)w.mapCap * 3, -7.f);
  o.dist.assign((size_t)w.mapCap * 2, -7.f);
  float scale[NLEVELS];
  scale[0] = 1.f;
  for (int l = 1; l < NLEVELS; l++) scale[l] = scale[l - 1] * 1.2f;
  mapr_update(w.kps.data(), w.desc.data(), w.n.data(), w.frames.data(), w.nE, w.nF, w.pose.data(), o.rows.data(),
              withOutlier ? w.outlier.data() : nullptr, w.cap, w.pts.data(), withMask ? w.mask.data() : nullptr, o.maskOut.data(),
              withRef ? o.ref.data() : nullptr, w.mapN, w.mapCap, scale, NLEVELS, what, o.normals.data(), o.dist.data(), o.desc.data(),
              o.obs.data(), &o.res);
  return o;
}

bool untouched(const Window& w, const Out& o) {
  if (o.rows != w.rows || o.ref != w.ref || o.maskOut != w.mask) return false;
  for (int v : o.obs)
    if (v != -7) return false;
  for (uint8_t v : o.desc)
    if (v != 0xA5) return false;
  for (float v : o.normals)
    if (v != -7.f) return false;
  for (float v : o.dist)
    if (v != -7.f) return false;
  const int32_t* r = &o.res.status;
  for (int k = 1; k < 16; k++)
    if (r[k] != 0) return false;
  return true;
}

int fails = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    fails++;
  }
}

}  // namespace

int main() {
  // healthy windows, every `what`, with and without the optional arrays
  const int shapes[][4] = {{0, 0, 5, 2}, {1, 1, 1, 1}, {2, 1, 7, 2}, {4, 2, 40, 3}, {6, 6, 30, 2}, {70, 3, 12, 1}};
  long long points = 0, badPoints = 0;
  for (const auto& s : shapes)
    for (int what = 0; what < 4; what++)
      for (int opt = 0; opt < 8; opt++) {
        const Window w = make(s[0], s[1], s[2], s[3], 0.3, 17 + s[0] * 31 + s[2]);
        const Out o = run(w, what, opt & 1, opt & 2, opt & 4);
        expect(o.res.status == 0, "a healthy window is flagged");
        expect(o.res.n_free == s[1], "n_free");
        if (!(what & 1))
          for (float v : o.normals) expect(v == -7.f, "normals written without ORBX_MAP_NORMALS");
        if (!(what & 2))
          for (uint8_t v : o.desc) expect(v == 0xA5, "descriptors written without ORBX_MAP_DESCRIPTORS");
        if (!(opt & 1)) expect(o.res.n_erased == 0 && o.res.n_bad_points == 0, "erasures without outlier bytes");
        points += o.res.n_points;
        badPoints += o.res.n_bad_points;
      }
  expect(points > 0 && badPoints > 0, "the windows ran neither points nor bad points");

  // every garbage case
  const Window base = make(4, 2, 40, 3, 0.1, 99);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (int g = 0; g < 9; g++) {
    Window w = base;
    int want = ORBX_MAP_BAD_INPUT;
    // feature 0 of entry 0 names a masked point of a free entry: a vertex
    const int v = w.rows[0];
    switch (g) {
      case 0: w.n[w.frames[1]] = w.cap + 1; break;
      case 1: w.mapN = w.mapCap + 1; break;
      case 2: w.rows[(size_t)3 * w.cap] = w.mapN; break;
      case 3: w.rows[(size_t)w.n[w.frames[0]] - 1] = v; break;  // (a second feature of entry 0 on its first point)
      case 4: w.frames[2] = w.frames[0]; break;
      case 5:
        for (int e = 0; e < w.nE; e++)
          for (int f = 0; f < w.n[w.frames[e]]; f++)
            if (w.rows[(size_t)e * w.cap + f] == v) {
              w.kps[(size_t)w.frames[e] * w.cap + f].octave = NLEVELS;
              w.outlier[(size_t)e * w.cap + f] = 0;
            }
        break;
      case 6: w.pose[(size_t)3 * 12 + 10] = nan; want = ORBX_MAP_NONFINITE; break;
      case 7: w.pts[(size_t)v * 3 + 1] = inf; want = ORBX_MAP_NONFINITE; break;
      case 8:
        for (size_t k = 0; k < w.rows.size(); k++)
          if (w.rows[k] == v) w.outlier[k] = 0;  // (no erasure: the point is not bad, its lens are looked at)
        for (int c = 0; c < 3; c++) w.pts[(size_t)v * 3 + c] = c == 0 ? -w.pose[9] : 0.f;  // (at entry 0's centre: len 0)
        want = ORBX_MAP_NONFINITE;
        break;
    }
    const Out o = run(w, 3, true, true, true);
    if (o.res.status != want) std::printf("garbage case %d: status %d, expected %d\n", g, o.res.status, want);
    expect(o.res.status == want, "a garbage case's status");
    expect(untouched(w, o), "a flagged problem changed something");
  }
  std::printf("map_update_ref_main: %lld points, %lld bad, %d failures\n", points, badPoints, fails);
  return fails ? 1 : 0;
}
