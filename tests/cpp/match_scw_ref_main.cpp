// match_scw_ref_main.cpp — a stand-alone program around tests/cpp/match_scw_ref.cpp, TEST INFRASTRUCTURE: a generated world (a
// keyframe of 300 features, some outside the grid; a map set of 500 points around the camera, in front and behind; a row with
// entries through a table, entries beyond the table and beyond the set, and -2) through the restatement, and the composition on
// good and dead inputs.  Built by tests/test_match_scw_host.py with -fsanitize=address,undefined: the restatement's indexing
// under the sanitizers, in a process of its own.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct KeyPoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
};

extern "C" void msr_search_scw(const KeyPoint* kps, const uint8_t* desc, int nF, int nM, const float* points, const float* normals,
                               const float* dists, const uint8_t* mapDesc, const uint8_t* mask, const float* scw, const float* K,
                               const int32_t* bounds, const float* scale, int nLevels, float th, int thLow, int32_t* matches,
                               const int32_t* table, int nTable, int32_t* res, int32_t* stage, float* proj, int32_t* outcome,
                               int32_t* alone, int32_t* best);
extern "C" void msr_compose_scw(const float* pose2, const float* sim3, float* scw);
extern "C" int msr_features_in_area(const KeyPoint* kps, int n, const int32_t* bounds, float x, float y, float r, int minLevel,
                                    int maxLevel, int32_t* out);

namespace {

uint32_t state = 97531u;
uint32_t next() {  // a small LCG: the world is the same on every run
  state = state * 1664525u + 1013904223u;
  return state >> 1;
}
double unit() { return (double)next() / 2147483648.0; }

}  // namespace

int main() {
  const int nF = 300, nM = 500, nLevels = 8, nTable = 320;
  const int32_t bounds[4] = {-12, 655, -9, 490};
  const float K[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
  float scale[nLevels];
  scale[0] = 1.0f;
  for (int l = 1; l < nLevels; l++) scale[l] = scale[l - 1] * 1.2f;
  // Scw = S12 * Tmw: a small rotation about y and a scale of 1.3 on an identity pose
  const float c = std::cos(0.02f), s = std::sin(0.02f);
  const float pose2[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1f, -0.05f, 0.2f};
  float sim3[13] = {c, 0, s, 0, 1, 0, -s, 0, c, 0.3f, 0.1f, -0.2f, 1.3f}, scw[12], dead[12];
  msr_compose_scw(pose2, sim3, scw);
  const float norm = std::sqrt(scw[0] * scw[0] + scw[1] * scw[1] + scw[2] * scw[2]);
  if (std::fabs(norm - 1.3f) > 1e-5f) {
    std::printf("composition: scale %.9g\n", norm);
    return 1;
  }
  sim3[12] = 0.0f;
  msr_compose_scw(pose2, sim3, dead);
  for (int k = 0; k < 12; k++)
    if (dead[k] != 0.0f) return 1;

  std::vector<float> pts(3 * nM), nrm(3 * nM), dst(2 * nM);
  std::vector<uint8_t> mdesc(32 * nM), mask(nM), desc(32 * nF);
  std::vector<KeyPoint> kps(nF);
  std::memset(kps.data(), 0, sizeof(KeyPoint) * nF);
  for (int i = 0; i < nM; i++) {
    const double z = (2 + 10 * unit()) * (i % 9 == 4 ? -1 : 1), x = (unit() - 0.5) * 1.8 * z, y = (unit() - 0.5) * 1.4 * z;
    const double d = std::sqrt(x * x + y * y + z * z);
    pts[3 * i] = (float)x; pts[3 * i + 1] = (float)y; pts[3 * i + 2] = (float)z;
    nrm[3 * i] = (float)(x / d); nrm[3 * i + 1] = (float)(y / d); nrm[3 * i + 2] = (float)(z / d * (i % 7 == 0 ? -1 : 1));
    dst[2 * i] = (float)(0.3 * d);
    dst[2 * i + 1] = (float)(d * std::pow(1.2, (int)(next() % nLevels)) * 0.95 * (i % 13 == 0 ? 0.3 : 1.0));
    mask[i] = i % 10 != 0;
    for (int b = 0; b < 32; b++) mdesc[32 * i + b] = (uint8_t)(next() & 255);
  }
  for (int j = 0; j < nF; j++) {
    kps[j].x = (float)(unit() * 720 - 40);  // (some outside the grid)
    kps[j].y = (float)(unit() * 540 - 30);
    kps[j].octave = (int)(next() % nLevels);
    const int like = (int)(next() % nM);  // a third of the features resemble a map point
    for (int b = 0; b < 32; b++) desc[32 * j + b] = j % 3 == 0 ? mdesc[32 * like + b] : (uint8_t)(next() & 255);
  }
  kps[7].x = NAN;
  std::vector<int32_t> row(nF, -1), table(nTable);
  for (int f = 0; f < nTable; f++) table[f] = f % 5 == 0 ? -1 : (f % 17 == 0 ? nM + 3 : (int)(next() % nM));
  for (int j = 0; j < nF; j += 4) row[j] = (int)(next() % (nTable + 8));  // (some beyond the table)
  row[1] = -2;
  row[2] = -9;
  std::vector<int32_t> res(14), stage(nM), outcome(nM), alone(nM), best(nM), area(nF);
  std::vector<float> proj(4 * nM);
  for (int pass = 0; pass < 2; pass++) {  // with the table, then with the translated row as map indices
    msr_search_scw(kps.data(), desc.data(), nF, nM, pts.data(), nrm.data(), dst.data(), mdesc.data(), mask.data(), scw, K, bounds, scale,
                   nLevels, 10.f, 50, row.data(), pass == 0 ? table.data() : nullptr, pass == 0 ? nTable : 0, res.data(), stage.data(),
                   proj.data(), outcome.data(), alone.data(), best.data());
    int total = 0, searched = 0;
    for (int j = 0; j < nF; j++) total += row[j] >= 0 || row[j] == -2;
    for (int i = 0; i < nM; i++) {
      searched += stage[i] == 6;
      if (stage[i] == 6) msr_features_in_area(kps.data(), nF, bounds, proj[4 * i], proj[4 * i + 1], proj[4 * i + 2], -1, -1, area.data());
    }
    if (res[2] != total || res[10] != res[1] + res[11] || res[10] > searched || (pass == 0 && (res[5] == 0 || !(res[0] & 2)))) {
      std::printf("pass %d: status %d, nmatches %d, n_total %d (recount %d), n_unmapped %d, with candidates %d, over %d, searched %d\n", pass,
                  res[0], res[1], res[2], total, res[5], res[10], res[11], searched);
      return 1;
    }
  }
  // no features, no points, a dead similarity
  msr_search_scw(kps.data(), desc.data(), 0, nM, pts.data(), nrm.data(), dst.data(), mdesc.data(), nullptr, scw, K, bounds, scale, nLevels,
                 10.f, 50, row.data(), nullptr, 0, res.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
  msr_search_scw(kps.data(), desc.data(), nF, 0, pts.data(), nrm.data(), dst.data(), mdesc.data(), nullptr, scw, K, bounds, scale, nLevels,
                 10.f, 256, row.data(), nullptr, 0, res.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
  msr_search_scw(kps.data(), desc.data(), nF, nM, pts.data(), nrm.data(), dst.data(), mdesc.data(), mask.data(), dead, K, bounds, scale,
                 nLevels, 10.f, 50, row.data(), nullptr, 0, res.data(), stage.data(), proj.data(), outcome.data(), alone.data(), best.data());
  if (!(res[0] & 4) || res[1] != 0) return 1;
  std::printf("MATCH SCW REF OK\n");
  return 0;
}
