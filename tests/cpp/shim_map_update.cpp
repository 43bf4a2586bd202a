// LocalMapping::UpdateMapPoints over include/orbx_shim.hpp, POD build: a synthetic window of 3 free and 2 fixed keyframes behind
// KeyFrameViews and 60 points behind a MapView, a handful of (keyframe, feature) pairs to erase -- through the shim and through
// the C ABI (orbx_map_update); both must give the same rows, counts, normals, distances, descriptors, flags, reference keyframes
// and record.  Usage: shim_map_update <seed>; prints RESULT <points> <observations> <erased> <bad> <agree>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }

int main(int argc, char** argv) {
  srand(argc > 1 ? atoi(argv[1]) : 0);
  const int nE = 5, nFree = 3, nP = 60;
  ORBextractor extractor(1000, 1.2f, 8, 20, 7);
  std::vector<float> pos(3 * nP);
  for (int j = 0; j < nP; j++) {
    pos[3 * j] = (float)uniform(-2, 2);
    pos[3 * j + 1] = (float)uniform(-1.5, 1.5);
    pos[3 * j + 2] = (float)uniform(4, 8);
  }
  std::vector<std::vector<KeyPointT>> keys(nE);
  std::vector<std::vector<uint8_t>> desc(nE);
  std::vector<std::vector<int>> rows(nE);
  std::vector<float> Tcw(nE * 12, 0.f);
  std::vector<std::pair<int, int>> erase;
  for (int e = 0; e < nE; e++) {
    Tcw[e * 12] = Tcw[e * 12 + 4] = Tcw[e * 12 + 8] = 1.f;
    Tcw[e * 12 + 9] = -0.25f * e;
    for (int j = e % 2; j < nP; j += 2) {  // (a point has 3 or 2 observers)
      KeyPointT k{};
      k.octave = rand() % 8;
      if (j % 7 == 3 && e == 1) erase.push_back(std::make_pair(e, (int)keys[e].size()));
      keys[e].push_back(k);
      rows[e].push_back(j);
      for (int b = 0; b < 32; b++) desc[e].push_back((uint8_t)((j * 37 + b) ^ (rand() % 4 == 0 ? 1 << (rand() % 8) : 0)));
    }
    keys[e].push_back(KeyPointT{});
    rows[e].push_back(-1);
    for (int b = 0; b < 32; b++) desc[e].push_back((uint8_t)rand());
  }
  std::vector<KeyFrameView> kfs(nE);
  size_t cap = 1;
  for (int e = 0; e < nE; e++) {
    kfs[e].N = (int)keys[e].size();
    kfs[e].mvKeysUn = keys[e].data();
    kfs[e].mDescriptors = desc[e].data();
    cap = keys[e].size() > cap ? keys[e].size() : cap;
  }
  MapView map;
  map.N = nP;
  map.mWorldPos = pos.data();
  MapPointsUpdate up;
  std::vector<std::vector<int>> shimRows = rows;
  const int nPoints = LocalMapping::UpdateMapPoints(&extractor, kfs, nFree, Tcw, shimRows, erase, map, up);

  // the same through the C ABI
  std::vector<orbx_keypoint> ck(nE * cap);
  std::vector<uint8_t> cd(nE * cap * 32, 0), col(nE * cap, 0), cmask(nP, 1), cdesc(nP * 32, 0);
  std::vector<int32_t> cn(nE), crow(nE * cap, -1), cref(nP, -1), cobs(nP, 0);
  std::vector<float> cnrm(nP * 3, 0.f), cdist(nP * 2, 0.f);
  for (int e = 0; e < nE; e++) {
    cn[e] = kfs[e].N;
    for (int i = 0; i < kfs[e].N; i++) {
      std::memcpy(&ck[e * cap + i], &keys[e][i], sizeof(orbx_keypoint));
      crow[e * cap + i] = rows[e][i];
    }
    std::memcpy(&cd[e * cap * 32], desc[e].data(), desc[e].size());
  }
  for (const auto& kf_i : erase) col[kf_i.first * cap + kf_i.second] = 1;
  orbx_map_result cres;
  const int r = orbx_map_update(extractor.context(), nE, nFree, ck.data(), cd.data(), cn.data(), (int)cap, Tcw.data(), crow.data(), col.data(),
                                nP, pos.data(), nullptr, cmask.data(), cref.data(), ORBX_MAP_NORMALS | ORBX_MAP_DESCRIPTORS, cnrm.data(),
                                cdist.data(), cdesc.data(), cobs.data(), &cres);
  bool agree = r == ORBX_OK && std::memcmp(&up.result, &cres, sizeof cres) == 0 && up.mnObs == cobs && up.mnRefKF == cref &&
               up.mbGood == cmask && up.mDescriptor == cdesc && std::memcmp(up.mNormalVector.data(), cnrm.data(), cnrm.size() * 4) == 0 &&
               std::memcmp(up.mfMinMaxDistance.data(), cdist.data(), cdist.size() * 4) == 0 && nPoints == cres.n_points;
  for (int e = 0; e < nE; e++)
    for (int i = 0; i < kfs[e].N; i++) agree = agree && shimRows[e][i] == crow[e * cap + i];
  std::printf("RESULT %d %d %d %d %d\n", cres.n_points, cres.n_observations, cres.n_erased, cres.n_bad_points, agree ? 1 : 0);
  return agree ? 0 : 1;
}
