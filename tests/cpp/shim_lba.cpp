// Optimizer::LocalBundleAdjustment over include/orbx_shim.hpp, POD build: a synthetic window of 3 free and 2 fixed keyframes
// behind KeyFrameViews and 80 points behind a MapView -- cameras on a baseline, the free poses and the points off the truth,
// half a pixel of noise, three gross mismatches in one free keyframe -- through the shim and through the C ABI (orbx_local_ba); both must give the
// same poses, points, erasures and record.  Usage: shim_lba <seed>; prints RESULT <edges> <erased> <iterations 1> <iterations
// 2> <agree>.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }

int main(int argc, char** argv) {
  srand(argc > 1 ? atoi(argv[1]) : 0);
  const int nE = 5, nFree = 3, nP = 80;
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  const float K[9] = {517.25f, 0.f, 318.75f, 0.f, 388.5f, 255.5f, 0.f, 0.f, 1.f};
  std::vector<float> pos(3 * nP);
  std::vector<double> X(3 * nP);
  for (int j = 0; j < nP; j++) {
    X[3 * j] = uniform(-2, 2) - 0.5;
    X[3 * j + 1] = uniform(-1.5, 1.5);
    X[3 * j + 2] = uniform(4, 8);
    for (int c = 0; c < 3; c++) pos[3 * j + c] = (float)(X[3 * j + c] + uniform(-0.02, 0.02));
  }
  std::vector<std::vector<KeyPointT>> keys(nE);
  std::vector<std::vector<int>> rows(nE);
  std::vector<std::vector<float>> Tcw(nE, std::vector<float>(12, 0.f));
  for (int e = 0; e < nE; e++) {
    const double tx = -0.25 * e;
    Tcw[e][0] = Tcw[e][4] = Tcw[e][8] = 1.f;
    Tcw[e][9] = (float)(tx + (e < nFree ? uniform(-0.02, 0.02) : 0.0));
    Tcw[e][10] = (float)(e < nFree ? uniform(-0.02, 0.02) : 0.0);
    for (int j = e % 2; j < nP; j += 2) {
      KeyPointT k{};
      k.pt.x = (float)((X[3 * j] + tx) / X[3 * j + 2] * K[0] + K[2] + uniform(-0.5, 0.5));
      // (a mismatch along y: along the baseline a point's depth would absorb it)
      k.pt.y = (float)(X[3 * j + 1] / X[3 * j + 2] * K[4] + K[5] + uniform(-0.5, 0.5) + (j % 13 == 5 && e == 1 ? 25.0 : 0.0));
      k.octave = rand() % 8;
      keys[e].push_back(k);
      rows[e].push_back(j);
    }
    keys[e].push_back(KeyPointT{});
    rows[e].push_back(-1);
  }
  std::vector<KeyFrameView> kfs(nE);
  size_t cap = 1;
  for (int e = 0; e < nE; e++) {
    kfs[e].N = (int)keys[e].size();
    kfs[e].mvKeysUn = keys[e].data();
    kfs[e].mTcw = Tcw[e].data();
    cap = keys[e].size() > cap ? keys[e].size() : cap;
  }
  MapView map;
  map.N = nP;
  map.mWorldPos = pos.data();
  std::vector<float> vTcw, vPos;
  std::vector<std::pair<int, int>> erase;
  orbx_lba_result res;
  const int nErase = Optimizer::LocalBundleAdjustment(&extractor, kfs, nFree, rows, map, K, vTcw, vPos, erase, &res);

  // the same through the C ABI
  std::vector<orbx_keypoint> ck(nE * cap);
  std::vector<int32_t> cn(nE), crow(nE * cap, -1);
  std::vector<float> cpose(nE * 12), cpo(nE * 12), cpts(3 * nP);
  std::vector<uint8_t> col(nE * cap);
  for (int e = 0; e < nE; e++) {
    cn[e] = kfs[e].N;
    for (int i = 0; i < kfs[e].N; i++) {
      std::memcpy(&ck[e * cap + i], &keys[e][i], sizeof(orbx_keypoint));
      crow[e * cap + i] = rows[e][i];
    }
    std::memcpy(&cpose[e * 12], Tcw[e].data(), 12 * sizeof(float));
  }
  orbx_lba_result cres;
  const int r = orbx_local_ba(extractor.context(), nE, nFree, ck.data(), cn.data(), (int)cap, cpose.data(), crow.data(), nP, pos.data(),
                              nullptr, K, nullptr, 5, 10, cpo.data(), cpts.data(), col.data(), &cres);
  int nc = 0;
  bool agree = r == ORBX_OK && std::memcmp(&res, &cres, sizeof res) == 0 && std::memcmp(vTcw.data(), cpo.data(), cpo.size() * 4) == 0 &&
               std::memcmp(vPos.data(), cpts.data(), cpts.size() * 4) == 0;
  for (int e = 0; e < nE; e++)
    for (int i = 0; i < kfs[e].N; i++)
      if (col[e * cap + i]) {
        agree = agree && nc < nErase && erase[nc].first == e && erase[nc].second == i;
        nc++;
      }
  agree = agree && nc == nErase && res.n_erased == nErase;
  std::printf("RESULT %d %d %d %d %d\n", res.n_edges, nErase, res.iterations[0], res.iterations[1], agree ? 1 : 0);
  return agree ? 0 : 1;
}
