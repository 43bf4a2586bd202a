// orbx_map_math.inc — the arithmetic of MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors (include/orbx.h,
// "local mapping: updating the map points") as plain f32 / f64 and integer operations, shared by orbx_map_kernel.hip (device) and
// tests/cpp/map_update_ref.cpp (the CPU restatement, g++ -ffp-contract=off): one source, so both sides take the same operations in
// the same order and agree bit for bit, as orbx_tri_math.inc does for CreateNewMapPoints, whose cameraCentre / norm3 this uses.
// What is NOT shared is the walk: who observes a point, in which order, which lane owns which observer, the selection of the
// median; each side writes that on its own.  The independent statement is numpy's (tests/map_update_ref_lib.py).
// f32 without contraction; only +, -, *, /, sqrt on doubles and comparisons.  The includer defines ORBX_TRI_FN as orbx_tri_math.inc
// asks for it and includes that file first.
namespace orbx_map {

constexpr int ST_BAD = 2, ST_NONFINITE = 4;  // ORBX_MAP_BAD_INPUT, ORBX_MAP_NONFINITE
constexpr int WHAT_NORMALS = 1, WHAT_DESCRIPTORS = 2;
// a slot of the inverse of the rows: -1 = the entry does not name the point, else the feature, + SLOT_ERASED when rule 2 erases it
constexpr int SLOT_ERASED = 0x40000000;
// a point's state word
constexpr int PT_VERTEX = 1, PT_LOST = 2, PT_BAD = 4;

ORBX_TRI_FN inline bool finite3(const float* v) { return orbx_tri::isFinite(v[0]) && orbx_tri::isFinite(v[1]) && orbx_tri::isFinite(v[2]); }

// one observer's term of the normal: d = P - Ow, len = |d| -> term = d / len.  false: len is 0 or no number (nothing usable)
ORBX_TRI_FN inline bool normalTerm(const float* P, const float* Ow, float* term) {
  const float d0 = P[0] - Ow[0], d1 = P[1] - Ow[1], d2 = P[2] - Ow[2];
  const float len = orbx_tri::norm3(d0, d1, d2);
  term[0] = d0 / len;
  term[1] = d1 / len;
  term[2] = d2 / len;
  return len > 0.0f && orbx_tri::isFinite(len);
}
// the running sum takes the observers' terms in ascending observer order, from +0.0f
ORBX_TRI_FN inline void normalAdd(float* sum, const float* term) {
  sum[0] = sum[0] + term[0];
  sum[1] = sum[1] + term[1];
  sum[2] = sum[2] + term[2];
}
ORBX_TRI_FN inline void normalFinish(const float* sum, int nObs, float* normal) {
  const float n = (float)nObs;
  normal[0] = sum[0] / n;
  normal[1] = sum[1] / n;
  normal[2] = sum[2] / n;
}
// mfMinDistance / mfMaxDistance from the reference keyframe: its centre, the scale of its feature's level, the last level's
ORBX_TRI_FN inline void distances(const float* P, const float* OwRef, float sRef, float sLast, float* minmax) {
  const float dist = orbx_tri::norm3(P[0] - OwRef[0], P[1] - OwRef[1], P[2] - OwRef[2]);
  const float mx = dist * sRef;
  minmax[0] = mx / sLast;
  minmax[1] = mx;
}

// popcount of a 32-bit word (the SWAR form of ORBmatcher::DescriptorDistance)
ORBX_TRI_FN inline int popc32(uint32_t v) {
  v = v - ((v >> 1) & 0x55555555u);
  v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
  return (int)((((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24);
}

}  // namespace orbx_map
