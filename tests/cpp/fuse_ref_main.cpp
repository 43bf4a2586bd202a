// fuse_ref_main.cpp — a stand-alone program around tests/cpp/fuse_ref.cpp, TEST INFRASTRUCTURE: a generated world (a keyframe of
// 300 features, some outside the grid and one that is no number; a map set of 500 points around the camera, in front and behind,
// several of them on the same feature; a row with entries in the set, beyond the set, -2 and other negative values; counts
// outside their range) through both forms of the restatement, with and without the occupants' counts, then empty sides and a dead
// pose.  Built by tests/test_fuse_host.py with -fsanitize=address,undefined: the restatement's indexing under the sanitizers, in a
// process of its own.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct KeyPoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
};

extern "C" void fr_fuse(int scwForm, const KeyPoint* kps, const uint8_t* desc, int nF, int nM, const float* points, const float* normals,
                        const float* dists, const uint8_t* mapDesc, const uint8_t* mask, const int32_t* mapObs, const float* T,
                        const float* K, const int32_t* bounds, const float* scale, const float* invSigma2, int nLevels, float th,
                        int thLow, int32_t* matches, const int32_t* occObs, int32_t* idx, uint8_t* act, int32_t* other, int32_t* res,
                        int32_t* stage, float* proj);
extern "C" int fr_features_in_area(const KeyPoint* kps, int n, const int32_t* bounds, float x, float y, float r, int minLevel,
                                   int maxLevel, int32_t* out);

namespace {

uint32_t state = 24680u;
uint32_t next() {  // a small LCG: the world is the same on every run
  state = state * 1664525u + 1013904223u;
  return state >> 1;
}
double unit() { return (double)next() / 2147483648.0; }

}  // namespace

int main() {
  const int nF = 300, nM = 500, nLevels = 8;
  const int32_t bounds[4] = {-12, 655, -9, 490};
  const float K[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
  float scale[nLevels], inv[nLevels];
  scale[0] = 1.0f;
  for (int l = 1; l < nLevels; l++) scale[l] = scale[l - 1] * 1.2f;
  for (int l = 0; l < nLevels; l++) inv[l] = 1.0f / (scale[l] * scale[l]);
  const float pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  float scw[12], dead[12];
  for (int k = 0; k < 12; k++) { scw[k] = 1.3f * pose[k]; dead[k] = pose[k]; }
  dead[4] = NAN;

  std::vector<float> pts(3 * nM), nrm(3 * nM), dst(2 * nM);
  std::vector<uint8_t> mdesc(32 * nM), mask(nM), desc(32 * nF);
  std::vector<int32_t> obs(nM), occ(nF);
  std::vector<KeyPoint> kps(nF);
  std::memset(kps.data(), 0, sizeof(KeyPoint) * nF);
  for (int j = 0; j < nF; j++) {
    kps[j].x = (float)(unit() * 720 - 40);  // (some outside the grid)
    kps[j].y = (float)(unit() * 540 - 30);
    kps[j].octave = (int)(next() % nLevels) - (j % 50 == 0);  // (an octave of -1 here and there)
    for (int b = 0; b < 32; b++) desc[32 * j + b] = (uint8_t)(next() & 255);
    occ[j] = j % 6 == 0 ? -1 : (j % 31 == 0 ? 1 << 20 : (int)(next() % 10));
  }
  kps[7].x = NAN;
  for (int i = 0; i < nM; i++) {  // two of three points sit on a feature, so that features are picked more than once
    const int j = (int)(next() % nF), level = kps[j].octave < 0 ? 0 : kps[j].octave;
    const double z = (2 + 10 * unit()) * (i % 9 == 4 ? -1 : 1);
    const double u = i % 3 ? kps[j].x + unit() - 0.5 : unit() * 640, v = i % 3 ? kps[j].y + unit() - 0.5 : unit() * 480;
    const double x = (u - 320) / 500 * z, y = (v - 240) / 500 * z, d = std::sqrt(x * x + y * y + z * z);
    pts[3 * i] = (float)x; pts[3 * i + 1] = (float)y; pts[3 * i + 2] = (float)z;
    nrm[3 * i] = (float)(x / d); nrm[3 * i + 1] = (float)(y / d); nrm[3 * i + 2] = (float)(z / d * (i % 7 == 0 ? -1 : 1));
    dst[2 * i] = (float)(0.3 * d);
    dst[2 * i + 1] = (float)(d * std::pow(1.2, level) * 0.95 * (i % 13 == 0 ? 0.3 : 1.0));
    mask[i] = i % 10 != 0;
    obs[i] = i % 41 == 0 ? -5 : (i % 43 == 0 ? 100000 : (int)(next() % 12));
    for (int b = 0; b < 32; b++) {  // the feature's descriptor with a few bits flipped, or (every third point) an unrelated one
      const uint8_t flip = i % 3 ? (b < 4 ? (uint8_t)(next() & 3) : (uint8_t)0) : (uint8_t)(next() & 255);
      mdesc[32 * i + b] = (uint8_t)(desc[32 * j + b] ^ flip);
    }
  }
  pts[3 * 11] = NAN;
  std::vector<int32_t> entry(nF, -1);
  for (int j = 0; j < nF; j += 4) entry[j] = (int)(next() % (nM + 8));  // (some beyond the set)
  for (int j = 1; j < nF; j += 5) entry[j] = -2;
  entry[2] = -9;
  entry[8] = nM + 3;
  std::vector<int32_t> row(nF), res(16), stage(nM), idx(nM), other(nM), area(nF);
  std::vector<uint8_t> act(nM);
  std::vector<float> proj(4 * nM);
  int chained = 0;
  for (int pass = 0; pass < 4; pass++) {  // the pose form and the Scw form, with and without the occupants' counts
    const int form = pass & 1;
    row = entry;
    fr_fuse(form, kps.data(), desc.data(), nF, nM, pts.data(), nrm.data(), dst.data(), mdesc.data(), mask.data(), obs.data(), form ? scw : pose,
            K, bounds, scale, inv, nLevels, form ? 4.f : 3.f, 50, row.data(), pass < 2 ? occ.data() : nullptr, idx.data(), act.data(),
            other.data(), res.data(), stage.data(), proj.data());
    int fused = 0, searched = 0, changed = 0;
    for (int i = 0; i < nM; i++) {
      fused += idx[i] >= 0;
      searched += stage[i] == 6;
      if ((idx[i] >= 0) != (act[i] != 0) || idx[i] >= nF) return 1;
      if (stage[i] == 6) fr_features_in_area(kps.data(), nF, bounds, proj[4 * i], proj[4 * i + 1], proj[4 * i + 2], -1, -1, area.data());
    }
    for (int j = 0; j < nF; j++) changed += row[j] != entry[j];
    chained += res[14];
    if (res[1] != fused || res[1] != res[10] + res[11] + res[12] + res[13] || res[8] != res[1] + res[9] || res[8] > searched ||
        changed > res[10] + res[12] || !(res[0] & 2) || !(res[0] & 4) || res[1] == 0) {
      std::printf("pass %d: status %d, n_fused %d (recount %d), with candidates %d, over %d, searched %d, actions %d %d %d %d, changed %d\n",
                  pass, res[0], res[1], fused, res[8], res[9], searched, res[10], res[11], res[12], res[13], changed);
      return 1;
    }
  }
  if (chained == 0) return 1;
  // no features, no points, a dead pose
  fr_fuse(0, kps.data(), desc.data(), 0, nM, pts.data(), nrm.data(), dst.data(), mdesc.data(), nullptr, obs.data(), pose, K, bounds, scale, inv,
          nLevels, 3.f, 50, row.data(), nullptr, idx.data(), act.data(), other.data(), res.data(), nullptr, nullptr);
  if (res[1] != 0) return 1;
  fr_fuse(1, kps.data(), desc.data(), nF, 0, pts.data(), nrm.data(), dst.data(), mdesc.data(), nullptr, nullptr, scw, K, bounds, scale, inv,
          nLevels, 4.f, 256, row.data(), occ.data(), idx.data(), act.data(), other.data(), res.data(), nullptr, nullptr);
  if (res[1] != 0 || res[2] != 0) return 1;
  for (int form = 0; form < 2; form++) {
    row = entry;
    fr_fuse(form, kps.data(), desc.data(), nF, nM, pts.data(), nrm.data(), dst.data(), mdesc.data(), mask.data(), obs.data(), dead, K, bounds,
            scale, inv, nLevels, 3.f, 50, row.data(), occ.data(), idx.data(), act.data(), other.data(), res.data(), stage.data(), proj.data());
    if (!(res[0] & 4) || res[1] != 0 || row != entry) return 1;
  }
  std::printf("FUSE REF OK\n");
  return 0;
}
