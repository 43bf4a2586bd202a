// A loop detector's call sequence over include/orbx_shim.hpp, POD build: an ORBextractor (the device context), an ORBVocabulary
// loaded from a text file, an ORBDatabase built from it; the frame's descriptors are added twice as two entries (once through
// their BowVector, once as features), a second vector made of the frame's first half is added, and the frame is queried.
// Usage: shim_database <vocabulary.txt> <descriptors.bin (N x 32 bytes)>; prints RESULT <entries> <results> and one line
// "<entry id> <score>" per result, best first.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "orbx_shim.hpp"

using namespace ORB_SLAM_Tracking;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[2], std::ios::binary);
  std::vector<uint8_t> desc((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  orbx::verbose() = false;
  try {
    ORBextractor extractor(1000, 1.2f, 8, 20, 7);
    ORBVocabulary voc(&extractor);
    voc.loadFromTextFile(argv[1]);
    ORBDatabase db(voc);
    DBoW2::BowVector mBowVec, half;
    voc.transform(desc.data(), (int)(desc.size() / 32), mBowVec);
    const DBoW2::EntryId e0 = db.add(mBowVec);
    const DBoW2::EntryId e1 = db.add(desc, &half);  // (half receives the same vector here)
    std::vector<uint8_t> front(desc.begin(), desc.begin() + (desc.size() / 64) * 32);
    const DBoW2::EntryId e2 = db.add(front, &half);
    if (e0 != 0 || e1 != 1 || e2 != 2 || db.size() != 3) return 3;
    DBoW2::QueryResults ret;
    db.query(mBowVec, ret, 4, -1);
    printf("RESULT %u %zu\n", db.size(), ret.size());
    for (const DBoW2::Result& r : ret) printf("%u %.17g\n", r.Id, r.Score);
    DBoW2::QueryResults again;
    db.query(desc, again, 4, 2);  // entries 0 and 1 only
    if (again.size() > 2) return 4;
    db.clear();
    if (db.size() != 0) return 5;
  } catch (const orbx::Error& e) {
    fprintf(stderr, "orbx error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
