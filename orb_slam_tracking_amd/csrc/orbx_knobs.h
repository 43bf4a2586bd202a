// orbx_knobs.h — diagnostic knobs of liborbx (orbx_debug_set, include/orbx.h).  The shipped library reads no environment
// variable: tests, tools and experiments that want a particular kernel or launch shape set a named integer knob through the C ABI
// (the Python loader forwards ORBX_<NAME> environment variables to it, so the profiling scripts keep their command lines).
// None of the knobs changes a result: they choose among kernels / launch shapes that produce identical output.
#pragma once
#include <atomic>
#include <climits>

namespace orbx {

// X(enumerator, "name")
#define ORBX_KNOB_LIST(X)                                                                                                        \
  X(KNOB_NO_BANDS, "no_bands")                /* pyramid: never k_pyramid_bands */                                               \
  X(KNOB_PYR_BANDS, "pyr_bands")              /* bands per frame of k_pyramid_bands */                                           \
  X(KNOB_PYR_STRIPS, "pyr_strips")            /* column strips per band of k_pyramid_bands */                                    \
  X(KNOB_BANDS_MIN_FRAMES, "bands_min_frames") /* k_pyramid_bands from this many frames per stream */                            \
  X(KNOB_NO_SPLIT, "no_split")                /* synchronous calls: one stream instead of two half batches */                    \
  X(KNOB_LAT_TRACE, "lat_trace")              /* orbx_extract prints a host-side timeline to stderr */                           \
  X(KNOB_FAST_WG_MAX_CELLS, "fast_wg_max_cells") /* launches of up to this many cells take k_fast (default 5000) */              \
  X(KNOB_MATCH_NO_GENERAL, "match_no_general") /* the matcher's sequential fallback is skipped (pairs it would take stay pending) */ \
  X(KNOB_MATCH_NO_MFMA, "match_no_mfma")      /* brute-force matching on the vector ALU (xor / bcnt) instead of the matrix cores */ \
  X(KNOB_OCT_BIG_DEPTH, "oct_big_depth")      /* bucket depth of the many-workgroup selection (tests: a depth whose buckets overflow) */ \
  X(KNOB_OCT_BIG_NO_FALLBACK, "oct_big_no_fallback") /* k_octree_big does not redo a unit it cannot take: the unit fails (tests) */ \
  X(KNOB_MULTI_FORCE_RCCL, "multi_force_rccl") /* orbx_multi_create: a one-device context goes through RCCL as well */

enum Knob {
#define ORBX_KNOB_ENUM(e, n) e,
  ORBX_KNOB_LIST(ORBX_KNOB_ENUM)
#undef ORBX_KNOB_ENUM
  KNOB_COUNT
};
constexpr long long KNOB_UNSET = LLONG_MIN;
extern std::atomic<long long> g_knob[KNOB_COUNT];  // (orbx_api.cpp)

inline long long knob(Knob k, long long dflt) {
  const long long v = g_knob[k].load(std::memory_order_relaxed);
  return v == KNOB_UNSET ? dflt : v;
}
inline bool knobOn(Knob k) { return knob(k, 0) != 0; }

}  // namespace orbx
