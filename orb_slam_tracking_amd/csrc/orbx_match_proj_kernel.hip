// orbx_match_proj_kernel.hip — ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono = true) for a batch of
// (last frame L, current frame C) pairs (include/orbx.h, "matching by projection").  gfx950.
//
// One workgroup of MP_THREADS threads per pair, one launch per call.  The workgroup builds C's grid in LDS (orbx_match_grid.h: the
// cells' start table and the features' indices by cell: Frame::PosInGrid, Frame.cpp:89-99) and then gives every feature of L a
// thread: the thread projects the feature's map point and walks its window (Frame::GetFeaturesInArea, Frame.cpp:163-206) cell x
// outer, cell y inner.  The pose, the camera, the walk and the launcher are orbx_match_rounds.h's, shared with the other two
// projection kernels.  Inside a cell the indices lie in the order the fill's atomics left them, so a cell's best is taken as the
// smallest (distance, index) of the cell, and cells are compared with the reference's strict `dist < bestDist`: the first
// candidate with the smallest distance in the order (cell x, cell y, index), without a key that would have to hold all four (at
// 16384 features distance, cell and index need 35 bits).
//
// The sequential rule -- feature i does not see the candidates that features before it took -- is resolved in rounds, all
// unresolved features of L in parallel:
//   A. every unresolved i finds its pick: the best among its candidates that no FINAL match has taken.  No candidate left, or a
//      best above TH_HIGH: i is final without a match.  It also claims, with an LDS atomicMin of i into claim[j], EVERY untaken
//      candidate j of its window with distance <= TH_HIGH, not only its pick.
//   B. i becomes final on its pick j iff claim[j] == i; j is then taken.
// This equals the sequential walk.  Call a round's state "sound" when every final match is the sequential one and every final
// feature's sequential outcome is what it holds.  In a sound state the taken candidates are a subset of what the sequential walk
// has taken when it reaches an unresolved i (a final match of a LATER feature k > i on j would have needed claim[j] == k, but
// i claims every candidate it could still take, so j was no candidate i could take -- or i was already final).  So i chooses
// among a superset of its sequential choices, in the same order.  If its pick j is one the sequential walk gives to a smaller
// unresolved feature k, then j is an untaken candidate of k within TH_HIGH, k claims it, claim[j] <= k < i, and i waits.  If
// claim[j] == i, no smaller unresolved feature can take j, every final match is sequential, so at i's turn the sequential walk
// finds j free and everything that ranks before j in i's window taken (it is taken here already, by final = sequential
// matches): j is i's sequential match.  A feature with nothing left within TH_HIGH has nothing left sequentially either, since
// what is taken only grows.  The smallest unresolved feature holds the smallest claim on its pick, so every round resolves at
// least one feature and the loop ends; features in different parts of the image never meet, and the rounds needed are the
// longest chain of features that wait for one another (a handful on tracking data; one feature per round when every feature
// claims the same candidates).
// Integer arithmetic apart from the projection, the window and the rotation bin; no float atomics; the result does not depend on
// the order in which the atomics land.
//
// LDS, sized from the capacity by the launcher: 12304 bytes of cell starts, then per feature 4 bytes of claims, 2 of cell-ordered
// indices, 2 of picks and two bit sets -- 20.7 KB at capacity 1024 (17 of gfx950's 1280-byte pieces, seven workgroups per CU by
// LDS, four by waves), 144 KB at ORBX_BOW_MAX_FEATURES (one workgroup per CU).
#include <hip/hip_runtime.h>

#include "orbx_launch.h"
#include "orbx_match_hist.h"
#include "orbx_match_rounds.h"

namespace orbx {
namespace {

constexpr int MP_TH_HIGH = 100;  // ORBmatcher::TH_HIGH
constexpr int MP_FREE = 0x7fffffff;                      // claim[j]: nobody claims j
constexpr uint32_t MP_NO_PICK = 0x7fffu;                 // pick[i]: low 15 bits the candidate (< 16384) ...
constexpr uint32_t MP_DISPLACED = 0x8000u;               // ... bit 15: with nothing taken i would have taken another one
static_assert(BOW_MAX_FEATURES <= (int)MP_NO_PICK, "a pick is 15 bits");

__host__ __device__ constexpr size_t mpLdsBytes(int cap) {
  return (size_t)4 * (MP_START_WORDS + cap + 2 * mrBitWords(cap)) + (size_t)2 * 2 * ((cap + 1) & ~1);
}

// what the threads of a pair share about it
struct MpPair {
  const orbx_keypoint* kpsL;
  const orbx_keypoint* kpsC;
  const float* pts;
  const uint8_t* mask;
  const uint8_t* outl;
  MrPose pose;
  MpGrid g;
};

// steps 2 and 3 for feature i of L: 0 = skipped by step 2, 1 = by step 3, 2 = (u, v), the radius and the octave are set
__device__ __forceinline__ int mpProject(const MatchProjArgs& a, const MpPair& P, const float* __restrict__ scale, int i, float* u,
                                         float* v, float* r, int* o, int* status) {
  if (P.mask && P.mask[i] == 0) return 0;
  if (P.outl && P.outl[i] != 0) return 0;
  const int oct = P.kpsL[i].octave;
  if (oct < 0 || oct >= a.cam.nLevels) {
    *status |= ORBX_PROJ_BAD_INPUT;
    return 0;
  }
  const float X = P.pts[3 * (size_t)i], Y = P.pts[3 * (size_t)i + 1], Z = P.pts[3 * (size_t)i + 2];
  if (!(mpFinite(X) && mpFinite(Y) && mpFinite(Z))) *status |= ORBX_PROJ_NONFINITE;
  float xc, yc, zc;
  mrToCamera(P.pose, P.pts, i, &xc, &yc, &zc);
  const float invz = 1.0f / zc;
  if (invz < 0.0f) return 1;
  if (!mrToImage(a.cam, P.g, xc, yc, invz, u, v)) return 1;
  *r = a.cam.th * scale[oct];
  *o = oct;
  return 2;
}

__global__ __launch_bounds__(MP_THREADS) void k_match_proj(MatchProjArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t mpLds[];
  __shared__ float sScale[ORBX_MAX_LEVELS];
  __shared__ int hist[MATCH_HISTO_LENGTH];
  __shared__ int sKeep[3], sKeepV[3];
  __shared__ int sWave[MP_THREADS / 64];
  __shared__ int sCnt[8];  // status, nmatches, n_points, n_in_image, n_with_candidates, n_displaced, n_rot_removed, rounds
  __shared__ int sAny;
  const int pair = blockIdx.x, t = threadIdx.x;
  const int cap = a.cap, words = mrBitWords(cap);
  int* const cellStart = (int*)mpLds;                       // [MP_CELLS + 1]: cell c holds cellIdx[cellStart[c] .. cellStart[c + 1])
  int* const claim = cellStart + MP_START_WORDS;            // [cap] per feature of C: the smallest claimant; of a taken one: its match
  uint32_t* const taken = (uint32_t*)(claim + cap);         // [words] bits over C's features
  uint32_t* const pending = taken + words;                  // [words] bits over L's features: unresolved
  uint16_t* const cellIdx = (uint16_t*)(pending + words);   // [cap] C's features by cell
  uint16_t* const pick = cellIdx + ((cap + 1) & ~1);        // [cap] per feature of L

  const int fl = a.pairs[pair], fc = a.pairs[a.nPairs + pair], ps = a.pairs[2 * a.nPairs + pair];
  const int rawL = a.n[fl], rawC = a.n[fc];
  const int nL = mpClamp(rawL, cap), nC = mpClamp(rawC, cap);
  MpPair P;
  P.kpsL = a.kps + (size_t)fl * cap;
  P.kpsC = a.kps + (size_t)fc * cap;
  P.pts = a.points + (size_t)ps * cap * 3;
  P.mask = a.pointMask ? a.pointMask + (size_t)ps * cap : nullptr;
  P.outl = a.lastOutlier ? a.lastOutlier + (size_t)pair * cap : nullptr;
  int status = (rawL != nL || rawC != nC) ? ORBX_PROJ_BAD_INPUT : 0;
  if (!mrLoadPose(a.pose, pair, &P.pose)) status |= ORBX_PROJ_NONFINITE;
  if (t != 0) status = 0;  // (what all threads see alike is reported once)
  P.g = mpGridOf(a.cam.b);
  const uint4* __restrict__ descC = (const uint4*)a.desc + (size_t)fc * cap * 2;
  const uint4* __restrict__ descQ = a.pointDesc ? (const uint4*)a.pointDesc + (size_t)ps * cap * 2 : (const uint4*)a.desc + (size_t)fl * cap * 2;
  int* __restrict__ mC = a.matchesCur + (size_t)pair * cap;

  // ---- start state, and C's grid
  for (int c = t; c < MP_START_WORDS; c += MP_THREADS) cellStart[c] = 0;
  for (int k = t; k < 2 * words; k += MP_THREADS) taken[k] = 0;  // (taken and pending lie one behind the other)
  if (t < ORBX_MAX_LEVELS) sScale[t] = a.cam.scale[t];
  if (t < MATCH_HISTO_LENGTH) hist[t] = 0;
  if (t < 3) { sKeep[t] = -1; sKeepV[t] = 0; }
  if (t < 8) sCnt[t] = 0;
  if (t == 0) sAny = 0;
  __syncthreads();
  mpGridCount(P.g, P.kpsC, nC, cellStart);
  __syncthreads();
  mpGridFill(P.g, P.kpsC, nC, cellStart, cellIdx, sWave);
  // ---- steps 2 and 3 for every feature of L: those with a window are the unresolved ones of the first round
  int nPoints = 0, nInImage = 0, nWithCand = 0, nDisplaced = 0, nm = 0;
  for (int i = t; i < nL; i += MP_THREADS) {
    float u, v, r;
    int o;
    const int stage = mpProject(a, P, sScale, i, &u, &v, &r, &o, &status);
    nPoints += stage >= 1;
    if (stage == 2) {
      nInImage++;
      mrSetBit(pending, i);
      sAny = 1;
    }
  }
  __syncthreads();

  // ---- the rounds
  int rounds = 0;
  while (sAny) {  // (uniform: read behind a barrier, written again only behind the next one)
    for (int j = t; j < nC; j += MP_THREADS)
      if (!mrBit(taken, j)) claim[j] = MP_FREE;
    __syncthreads();
    if (t == 0) sAny = 0;
    // A. picks and claims
    for (int i = t; i < nL; i += MP_THREADS) {
      if (!mrBit(pending, i)) continue;
      float u, v, r;
      int o, ignored = 0;
      mpProject(a, P, sScale, i, &u, &v, &r, &o, &ignored);  // (the same arithmetic as above: stage 2 again)
      const uint4 q0 = descQ[(size_t)i * 2], q1 = descQ[(size_t)i * 2 + 1];
      int bestD = 256, bestJ = -1, bestCell = -1;  // among the untaken candidates
      int freeD = 256, freeJ = -1, freeCell = -1;  // among all of them
      int nCand = 0;
      mrWalk(P.g, P.kpsC, cellStart, cellIdx, u, v, r, o - 1, o + 1, [&](int j, int c) {
        nCand++;
        const int d = mpDistance(q0, q1, descC[(size_t)j * 2], descC[(size_t)j * 2 + 1]);
        if (d < freeD || (d == freeD && c == freeCell && j < freeJ)) { freeD = d; freeJ = j; freeCell = c; }
        if (mrBit(taken, j)) return;
        if (d < bestD || (d == bestD && c == bestCell && j < bestJ)) { bestD = d; bestJ = j; bestCell = c; }
        if (d <= MP_TH_HIGH) atomicMin(&claim[j], i);
      });
      if (rounds == 0) nWithCand += nCand > 0;
      const int got = bestD <= MP_TH_HIGH ? bestJ : -1, alone = freeD <= MP_TH_HIGH ? freeJ : -1;
      if (got < 0) {  // final without a match
        mrClearBit(pending, i);
        nDisplaced += alone >= 0;
      } else {
        pick[i] = (uint16_t)((uint32_t)got | (got != alone ? MP_DISPLACED : 0u));
      }
    }
    __syncthreads();
    // B. a pick whose smallest claimant is its feature is final
    for (int i = t; i < nL; i += MP_THREADS) {
      if (!mrBit(pending, i)) continue;
      const uint32_t pk = pick[i];
      const int j = (int)(pk & MP_NO_PICK);
      if (claim[j] == i) {
        mrSetBit(taken, j);
        mrClearBit(pending, i);
        nm++;
        nDisplaced += (pk & MP_DISPLACED) != 0;
      } else {
        sAny = 1;
      }
    }
    rounds++;
    __syncthreads();
  }

  // ---- steps 6 and 7: a taken feature's claim is its match
  if (a.checkOri) {  // (uniform)
    for (int j = t; j < nC; j += MP_THREADS)
      if (mrBit(taken, j)) {
        const int bin = matchRotBin(P.kpsL[claim[j]].angle, P.kpsC[j].angle);
        if (bin >= 0) atomicAdd(&hist[bin], 1);
      }
    __syncthreads();
    if (t < MATCH_HISTO_LENGTH) {
      const int v = hist[t], place = matchHistPlace(hist, t);
      if (v > 0 && place < 3) { sKeep[place] = t; sKeepV[place] = v; }
    }
    __syncthreads();
  }
  const int ind1 = sKeep[0];
  int ind2 = sKeep[1], ind3 = sKeep[2];
  matchDropMaxima(sKeepV[0], sKeepV[1], sKeepV[2], &ind2, &ind3);
  int dropped = 0;
  for (int j = t; j < nC; j += MP_THREADS) {
    int m = -1;
    if (mrBit(taken, j)) {
      m = claim[j];
      if (a.checkOri) {
        // a match's bin is a function of the match: recomputed here from the two angles instead of kept in a list per bin
        const int bin = matchRotBin(P.kpsL[m].angle, P.kpsC[j].angle);
        if (bin >= 0 && bin != ind1 && bin != ind2 && bin != ind3) {
          m = -1;
          dropped++;
        }
      }
    }
    mC[j] = m;
  }
  if (status) atomicOr(&sCnt[0], status);
  if (nm - dropped) atomicAdd(&sCnt[1], nm - dropped);
  if (nPoints) atomicAdd(&sCnt[2], nPoints);
  if (nInImage) atomicAdd(&sCnt[3], nInImage);
  if (nWithCand) atomicAdd(&sCnt[4], nWithCand);
  if (nDisplaced) atomicAdd(&sCnt[5], nDisplaced);
  if (dropped) atomicAdd(&sCnt[6], dropped);
  __syncthreads();
  if (t < 8) ((int32_t*)(a.res + pair))[t] = t == 7 ? rounds : sCnt[t];
}

}  // namespace

hipError_t launch_match_proj(hipStream_t st, const MatchProjArgs& a) {
  static_assert(sizeof(orbx_proj_result) == 32, "eight int32");
  static_assert(mpLdsBytes(BOW_MAX_FEATURES) + 512 <= 160 * 1024, "a workgroup's LDS at the largest capacity");
  static_assert(mpLdsBytes(1024) == 20752, "capacity 1024: seven workgroups per CU by LDS");
  return mrLaunch(k_match_proj, a.nPairs, mpLdsBytes(a.cap), st, a);
}

}  // namespace orbx
