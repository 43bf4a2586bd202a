// orbx_device.h — POD structures shared between the host pipeline and the HIP kernels of liborbx.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/orbx.h"

#define ORBX_MAX_LEVELS 16
#define ORBX_EDGE 19          // EDGE_THRESHOLD, Features/ORBextractor.cpp:90
#define ORBX_MIN_BORDER 16    // EDGE_THRESHOLD - 3, cpp:1056
#define ORBX_CELL_MAX 76      // widest/tallest FAST cell image: ceil(width/nCols) <= 70, +6 overlap
#define ORBX_GRID_COLS 64     // FRAME_GRID_COLS, SlamTypes/Frame.hpp:16
#define ORBX_GRID_ROWS 48     // FRAME_GRID_ROWS, SlamTypes/Frame.hpp:15

namespace orbx {

// geometry of one pyramid level for the current frame size
struct LevelGeom {
  int32_t w, h, stride;       // level image, row stride in bytes (level 0: caller's stride)
  int32_t nCols, nRows;       // FAST cell grid (cpp:1067-1075)
  int32_t wCell, hCell;
  int32_t maxBX, maxBY;       // maxBorderX/Y (cpp:1058-1059); minBorder = 16
  int32_t cellBase;           // index of this level's first cell in the flattened (level, row, col) list
  int32_t candCap;            // entries of one frame's candidate area on this level = cells * segCap
  int32_t quota;              // mnFeaturesPerLevel
  int32_t xtabOff, ytabOff;   // offsets into the resize tables (entries)
  int32_t patchSize;          // (int)(31 * scale), cpp:1165
  float scale;                // mvScaleFactor
  int64_t imgOff;             // byte offset of frame 0's image inside the pyramid buffer (levels >= 1)
  int64_t frameStride;        // bytes between consecutive frames of this level
  int64_t candOff;            // entry offset of frame 0's candidate area (frame stride = candCap, cell stride = segCap)
  int32_t resizeSpanOk;       // 1 if the taps of any 4 consecutive outputs span <= 8 source pixels (k_resize_dw usable)
  uint32_t colsInv24;         // ceil(2^24 / nCols): cell index / nCols == (index * colsInv24) >> 24 (k_fast)
  int32_t segCap;             // entries of one cell's candidate segment = worst case of its NMS survivors
  int32_t candMax;            // worst-case number of candidates of the level (sum over its cells)
};

struct Geom {
  int32_t nlevels;
  int32_t nCellsTotal;
  int32_t iniTh, minTh;
  int32_t selCap;             // per-frame capacity of the selected-keypoint list (== output capacity)
  int32_t frame0;             // first frame of this launch (a batch may be issued as several sub-batches / streams)
  LevelGeom L[ORBX_MAX_LEVELS];
};

// k_fast_wave: what one wave needs to know about its FAST cell, precomputed on the host (buildFastCells) so that the kernel's
// prologue is one scalar load instead of a level search and a dozen divisions / multiplications per wave.  Round 14: the record
// carries everything the wave used to derive from the cell, its level (LevelGeom, a second scalar load behind the first) and the
// tile stride TS (48 / 64) -- none of it changes between the calls of a context.  LDS addresses are relative to the start of the
// kernel's dynamic LDS, whose layout (fastWaveLds) is fixed by the geometry.  Whole dwords are what the kernel uses as they come;
// every packed field costs the wave one scalar instruction.
struct FastCell {          // 64 bytes, sixteen dwords
  uint64_t img;            // byte offset of the first staged dword (row iniY, column iniX & ~3) from frame 0's image: inside the
                           // caller's image (level 0) or inside the pyramid buffer (LevelGeom::imgOff folded in)
  uint32_t frameStride;    // bytes between the level's frames in the pyramid buffer (below 2^32, buildFastCells checks); 0 = level 0: the launch's own base / stride
  uint32_t stride;         // row stride of the level image in bytes
  uint64_t cand;           // byte offset of the cell's candidate segment of frame 0: 4 (LevelGeom::candOff + local cell * segCap)
  uint32_t candCap;        // bytes between the level's frames in the candidate area: 4 LevelGeom::candCap
  uint32_t oxy;            // candidate = (tile column | tile row << 12 | score << 24) + oxy: ox + (oy << 12) mod 2^32, relative to minBorder
  uint32_t dPos;           // sweep: a lane's step to its next quad, quad columns << 16 | LDS bytes
  uint32_t wrapK;          // ... and what a column at or beyond the row's end adds to get into the next tile row
  uint32_t selC0, selR0;   // v_perm_b32 selectors of the byte phase sh: centre / top / bottom pixels (0, 1); right compass pixels (0, 1)
  uint32_t lastThr;        // positions at or above: the row's last quad, (nqc - 1) << 16
  uint32_t aLast_kN;       // LDS address of the sweep's last item | (strength map - tile - xoff) << 16
  uint32_t quad;           // ceil(2^20 / nqc) | nqc << 21 | (nvLast > 1, > 2, > 3: one bit each) << 25 | (right compass pair one dword
                           // further: sh >= 2) << 28 | (sh + 1) << 29; nqc = quads per row (<= 15), nvLast = the last one's pixels inside
  uint32_t counts;         // full steps of 64 items (<= 13) | (64 - items of the last step) << 4 | segCap (< 2048) << 10 | rows ch
                           // (<= 64) << 21 | xoff << 28; ch == 0: the cell detects nothing (cpp:1088,1101), the whole record is zero
};
static_assert(sizeof(FastCell) == 64, "FastCell is loaded with one s_load_dwordx16");
// k_fast_wave's dynamic LDS for a geometry: 16 bytes | tile[tileBytes] | strength map[smapBytes] | survivor stack | corner list
#define ORBX_FW_RING 192   // survivor stack, entries (u16 LDS addresses)
#define ORBX_FW_CORN 256   // corner list, entries
struct FastWaveLds {
  int32_t tileBytes, smapBytes, total;
};
static inline FastWaveLds fastWaveLds(const Geom& g, int ts) {
  int ch = 7;  // tallest cell image of this geometry (cell + 6 px overlap, cpp:1094-1103)
  for (int l = 0; l < g.nlevels; l++) ch = std::max(ch, std::min(g.L[l].hCell + 6, ORBX_CELL_MAX));
  FastWaveLds r;
  r.tileBytes = ch * ts + 16;  // (+ 16: the quick reject's dword reads reach a few bytes beyond the last tile row)
  r.smapBytes = (ch - 6 + 2) * ts;
  r.total = 16 + r.tileBytes + r.smapBytes + ORBX_FW_RING * 2 + ORBX_FW_CORN * 2;
  return r;
}

// candidate entry written by the FAST kernel: x | y<<12 | score<<24, x/y relative to minBorder
#if defined(__HIPCC__)
#define ORBX_HD __host__ __device__
#else
#define ORBX_HD
#endif
ORBX_HD static inline uint32_t packCand(int x, int y, int score) { return (uint32_t)x | ((uint32_t)y << 12) | ((uint32_t)score << 24); }

// a keypoint chosen by the quadtree stage, input of the orientation/descriptor kernel
struct SelKp {
  uint16_t x, y;        // level coordinates (already + minBorder)
  uint8_t level, response;  // response = FAST score (<= 254)
  uint16_t pad;
};

// quadtree selection stage (orbx_octree_kernel.hip): per-level constants of DistributeOctTree
struct OctLevel {
  int32_t width, height;   // maxBorder - minBorder
  int32_t nIni;            // cpp:706
  float hX;                // cpp:709
  int32_t wCell, hCell, nCols;  // FAST cell grid: defines the reference's candidate order
  int32_t quota;
  int32_t cellBase, nCells, segCap;  // the level's cells in the per-frame cell-count array; entries per cell segment
  int32_t depthBits;       // splits after which every cell of the level is one pixel (DivideNode halves with ceil): the quadrant
                           // digits of a path code beyond this depth are all 0
  int32_t tabOff, tabW, tabH;  // the level's path-code tables inside OctLaunch::codeTab (dword offset, even): tabW pairs
                           // {x digits of the 16 DivideNode splits at bit 2 (15 - d), root} by x, then tabH words of y digits
                           // (bit 2 (15 - d) + 1) by y (octCodeTable on the host); tabW >= width, tabH >= height
  // Large units on many workgroups (k_octree_buckets + k_octree_big): the level's keys are cut into nIni * 4^bigD0 BUCKETS, one
  // per tree node of depth bigD0 (0 = not usable for this level).  bigD0 never exceeds the depth the quota guarantees the full
  // passes to reach (octBigPlan), so no list node ever spans two buckets.  A bucket's keys are sorted in LDS by one workgroup
  // and land in the bucket's own slot of bigCapB entries of the unit's key / score / divergence arrays.
  int32_t bigD0, bigBuckets, bigCapB;  // chosen per launch (octBigChoose): depth <= bigDMax, nIni << 2 bigD0 buckets, keys per slot
  int32_t bigDMax;         // deepest bucket depth the level allows (-1: none): the depth of the interval tables
  int32_t bigTabOff;       // dword offset in codeTab: first x of every (root, top bigDMax x digits) prefix [nIni << bigDMax, + 1 end],
                           // then first y of every top-bigDMax-y-digits prefix [(1 << bigDMax) + 1]; a coarser prefix owns the union
};
#define ORBX_OCTB_CAP 1024        // keys of one bucket (one wave's register sort in k_octree_buckets)
#define ORBX_OCTB_MAX_BUCKETS 1024
#define ORBX_OCTB_INFO 40         // ints of a bucket's record: count, first / last inner divergence, overflow, 18 + 18 histogram bins

// Small launches (the one-frame call): k_describe_patch reads the selection's per-level staging lists directly and does
// k_sel_compact's bookkeeping in one designated wave per frame, so that no compaction kernel sits on the call's critical path.
struct DescStage {
  const SelKp* selStage;
  const int* nselLevel;
  int* nsel;
  int* nselUser;
  int* hostNsel;
  int* hostErr;
  int* maxN;
  int* hostMaxN;
  int32_t selStride;
  int32_t selOff[ORBX_MAX_LEVELS];
};
#define ORBX_DESC_STAGED_MAX_UNITS 256  // units (frames x levels) up to which the descriptor kernel takes the staged lists (round 5:
                                        // 64 -> 256: 32 frames of eight levels per launch; synchronous 32-frame call 132.7 k -> 143.7 k frames/s)

struct OctLaunch {
  OctLevel lev[ORBX_MAX_LEVELS];
  int64_t candOff[ORBX_MAX_LEVELS];
  int64_t scrOff[ORBX_MAX_LEVELS];     // global-scratch placement (k_octree_global)
  int64_t scrStride[ORBX_MAX_LEVELS];
  int32_t candCap[ORBX_MAX_LEVELS];
  int32_t selOff[ORBX_MAX_LEVELS];     // offset of the level inside one frame's SelKp staging area
  int32_t scrNMax[ORBX_MAX_LEVELS];
  int32_t nlevels, selStride;          // SelKp staging entries per frame
  int32_t frame0, nCellsTotal;         // first frame of this launch; cells of one frame over all levels
  const uint32_t* codeTab;             // path-code tables of the levels (device memory), see OctLevel::tabOff
};

#define ORBX_OCT_MAX_CAND ((1 << 19) - 1)  // candidates per (frame, level) the selection stage can index
// what a unit reports for the next batch's launch choices (maxN[], hostMaxN[], the host's candHintL[]): its candidate count and, from
// k_octree_big, the fill of its fullest bucket; the reducers take the maximum of each field
// (round 5: and the bucket depth the unit ran with -- a fill says nothing without it: ADVICE r04.)  Bits 0..18 count, 19..27 the
// fill in units of four keys (rounded up), 28..30 the depth.
#define ORBX_OCT_FEEDBACK(n, fill, depth) ((int)(n) | ((((int)(fill) + 3) >> 2) << 19) | ((int)(depth) << 28))
#define ORBX_OCT_FB_COUNT(v) ((int)(v) & 0x7ffff)
#define ORBX_OCT_FB_FILL(v) ((((int)(v) >> 19) & 0x1ff) << 2)
#define ORBX_OCT_FB_DEPTH(v) (((int)(v) >> 28) & 7)
#define ORBX_OCT_FB_MAXF(a, b, F) (F(a) > F(b) ? F(a) : F(b))
#define ORBX_OCT_FB_MAX(a, b) ORBX_OCT_FEEDBACK(ORBX_OCT_FB_MAXF(a, b, ORBX_OCT_FB_COUNT), ORBX_OCT_FB_MAXF(a, b, ORBX_OCT_FB_FILL), ORBX_OCT_FB_MAXF(a, b, ORBX_OCT_FB_DEPTH))
#define ORBX_OCT_REDONE 0x40000000  // bit of a (frame, level) count in nselLevel[]: k_octree_big redid the unit in place with the one-workgroup code

#if defined(__HIPCC__)
// ---- bookkeeping of the selection stage shared by k_sel_compact and the staged form of k_describe_patch (small launches, which
//      run no k_sel_compact): ONE definition of what a unit's raw count means and of what is published per frame ----
// a unit's raw count in nselLevel[]: negative = the unit failed; ORBX_OCT_REDONE set = k_octree_big redid it in place (same result)
__device__ __forceinline__ int selUnitCount(int raw, bool* failed) {
  *failed = *failed || raw < 0;
  return raw < 0 ? 0 : (raw & ~ORBX_OCT_REDONE);
}
// a frame's totals: to the context's array (k_describe_patch's launch bound), the caller's array, the host's mapped mirror; a failed
// unit raises the host's error flag (ORBX_E_CAPACITY at the batch's wait)
__device__ __forceinline__ void selPublishFrame(int f, int total, bool failed, int* __restrict__ nsel, int* __restrict__ nselUser,
                                                int* __restrict__ hostNsel, int* __restrict__ hostErr) {
  nsel[f] = total;
  if (nselUser) nselUser[f] = total;
  if (hostNsel) hostNsel[f] = total;
  if (failed) *hostErr = 1;
}
// per-level maxima (field by field, ORBX_OCT_FEEDBACK) of the units' reports of frames [frame0, frame0 + nFrames), by ONE wave:
// lane = (frame % 4, level); the reports are reset for the next launch
__device__ __forceinline__ void selReduceReports(int lane, int frame0, int nFrames, int nlevels, int* __restrict__ maxN,
                                                 int* __restrict__ hostMaxN) {
  static_assert(ORBX_MAX_LEVELS <= 16, "sixteen lanes per frame");
  int m = 0;
  if ((lane & 15) < nlevels)
    for (int fr = lane >> 4; fr < nFrames; fr += 4) {
      const int idx = (frame0 + fr) * nlevels + (lane & 15);
      const int v = maxN[idx];
      m = ORBX_OCT_FB_MAX(m, v);
      maxN[idx] = 0;
    }
  { const int t = __shfl_xor(m, 16); m = ORBX_OCT_FB_MAX(m, t); }
  { const int t = __shfl_xor(m, 32); m = ORBX_OCT_FB_MAX(m, t); }
  if (lane < nlevels) hostMaxN[lane] = m;
}
#endif


// Bucket depth of a level for one launch of the many-workgroup selection (k_octree_buckets / k_octree_big): the coarsest depth
// that leaves a bucket at most 256 keys on average of the `hint` candidates a unit of that level had in the previous batch (a
// bucket is one wave's sort of up to ORBX_OCTB_CAP keys: four times that average before a dense corner of the frame overfills
// its slot and the unit falls to the one-workgroup kernel; a wave spends ~1200 instructions on a bucket before its first key, so
// many small buckets cost more than few full ones: 40 us against 13 for the 600 k keys of four 4K frames) -- or, without a hint,
// about 16 k pixels: 250 keys at 1.5 %.  nMax = the candidates the unit's scratch is sized for (OctLaunch::scrNMax):
// the buckets' slots share its key array.  bigBuckets == 0: no plan, the level keeps the one-workgroup kernel.
// fillPrev / dPrev (round 5): the fullest bucket of the previous batch's units of this level and the depth they ran with.
// A bucket of a coarser depth d holds at most fillPrev * 4^(dPrev - d) keys, one of a finer depth at most fillPrev: the depth is
// deepened until that bound leaves a quarter of the bucket's slot free.  (Before, the depth came from the count alone; a unit
// whose bucket overflowed reported the largest count, got the deepest depth for one batch, reported its true count from there and
// returned to the depth that overflowed: every second batch of a scene with one dense cluster went through the in-place redo.)
// *estFill = that bound for the chosen depth (0 = unknown): picks k_octree_buckets' LDS slot count.
inline void octBigChoose(OctLevel* O, int nMax, int hint, int fillPrev = 0, int dPrev = 0, int* estFill = nullptr) {
  O->bigD0 = 0; O->bigBuckets = 0; O->bigCapB = 0;
  if (estFill) *estFill = 0;
  if (O->bigDMax < 0) return;
  int d = 0;
  if (hint > 0) {
    while (d < O->bigDMax && (long long)hint > 256ll * ((long long)O->nIni << (2 * d))) d++;
  } else {
    const double rootArea = (double)(O->width / O->nIni + 1) * (double)O->height;
    while (d < O->bigDMax && rootArea / (double)(1ll << (2 * d)) > 16384.0) d++;
  }
  long long nPad = 1024;
  while (nPad < nMax) nPad <<= 1;
  auto capOf = [&](int dd) {
    const long long nb = (long long)O->nIni << (2 * dd);
    int cap = ORBX_OCTB_CAP;
    while (cap > 0 && (long long)cap * nb > nPad) cap >>= 1;
    return cap;
  };
  auto bound = [&](int dd) -> long long {
    if (fillPrev <= 0) return 0;
    return dd <= dPrev ? (long long)fillPrev << (2 * (dPrev - dd)) : (long long)fillPrev;
  };
  while (d < O->bigDMax && bound(d) * 4 > 3ll * capOf(d)) d++;
  const long long nb = (long long)O->nIni << (2 * d);
  const int cap = capOf(d);
  if (cap < 256 || nb > ORBX_OCTB_MAX_BUCKETS) return;
  O->bigD0 = d; O->bigBuckets = (int32_t)nb; O->bigCapB = cap;
  if (estFill) *estFill = (int)std::min<long long>(bound(d), 1 << 20);
}

// k_copy_out: the result arrays of a host-frame batch, copied by a kernel into the caller's page-locked (device-mapped) arrays:
// segment s = `rows` rows of `rowDwords` dwords, of which the first cnt[row] * mult are copied (cnt == nullptr: the whole row)
struct CopySeg {
  const uint32_t* src;
  uint32_t* dst;
  const int32_t* cnt;
  int32_t rows, rowDwords, mult, pad;
};
struct CopyOut {
  CopySeg s[6];
};

struct ResizeTab {
  int32_t ofs;    // source index
  int32_t coef;   // c0 | c1 << 16 (Q11)
};

// k_pyramid_tiles: what tile t of a frame produces of level l -- the rectangle it owns (written to the pyramid) and the rectangle it
// needs (owned pixels plus what its rectangles of the higher levels read), both in level-l pixel coordinates; level 0: the part of
// the caller's image the tile stages (host: buildPyrTiles).  The tile's resize taps follow in one blob per tile (PyrTileTap):
// per level 1 .. nlevels - 1 the x taps of the needed columns, then the y taps of the needed rows.
struct PyrTileRect {
  int16_t nx0, nx1, ny0, ny1;  // needed: computed into LDS
  int16_t ox0, ox1, oy0, oy1;  // owned: also stored to the pyramid
};
struct PyrTileTap {
  uint32_t pos;   // first source column (row) relative to the previous level's needed rectangle | (second - first) << 16
  uint32_t coef;  // c0 | c1 << 16 (Q11), as ResizeTab
};
#define ORBX_PYR_TILE_TAPS 768  // taps of one tile over all levels (capacity of the blob and of its LDS copy)

// k_pyramid_bands: rows [r0, r1) of level l that band b of a frame produces (host: computePyrBands)
#define ORBX_PYR_BANDS_MAX 32
#define ORBX_PYR_STRIPS_MAX 8
struct PyrBands {
  int32_t nBands, dual2;                                 // dual2: pixel 2 of some group needs the second dword pair
  int32_t safeFrom;                                      // frames >= safeFrom (batch index): nothing is known to follow their level 0
  int32_t maxRows;                                       // most rows any band has on any level (<= 256)
  int32_t xoff[ORBX_MAX_LEVELS], yoff[ORBX_MAX_LEVELS];  // the level's PyrXGroup / PyrYRow tables, in uint4 units from the table base
  // r0 | r1 << 16 (both below 32768): one dword, so that the kernel fetches the pair with a scalar load (16-bit fields of a
  // kernel argument under a runtime index are fetched by the vector unit, and what is computed from them stays there)
  uint32_t rows[ORBX_PYR_BANDS_MAX][ORBX_MAX_LEVELS];
  // column strips (round 5: few large frames -- four 3840x2160 frames are 128 workgroups of 32 bands, half the chip's CUs with one
  // workgroup each): strip s of a band produces the 4-pixel groups [g0, g1) of level l, its own share of the row plus the groups
  // its share of level l + 1 reads; workgroup = (band, strip).  One strip = the whole row (every 640x480 batch).
  int32_t nStrips;
  uint32_t grp[ORBX_PYR_STRIPS_MAX][ORBX_MAX_LEVELS];   // g0 | g1 << 16
  // round 13: how the workgroup's 512 threads split into thread-columns and thread-rows on level l of strip s depends on the launch
  // alone, so the host works it out (pyrColsOf) and the kernel divides nothing:
  //   cols[s][l][0] = ceil(2^19 / ngt) | (ngt - 1) << 20 | (G - 1) << 31      cols[s][l][1] = ceil(2^19 / rpp) | (rpp - 1) << 20
  // G groups per thread, ngt thread-columns, rpp thread-rows per pass (1 .. 512 each).  x / d == (x * ceil(2^19 / d)) >> 19 for
  // d <= 512 and x < 1024: the error term x (d ceil(2^19 / d) - 2^19) / (d 2^19) stays below 1 / d while x (d - 1) < 2^19, and
  // x * 2^19 < 2^32 (the kernel divides tid < 512 by ngt, and a band's rows + rpp - 1 < 768 by rpp)
  int32_t twoGroups;                                     // the two-group instances (GMAX = 2) take this launch
  uint32_t cols[ORBX_PYR_STRIPS_MAX][ORBX_MAX_LEVELS][2];
};
#define ORBX_PYR_INV_SHIFT 19
#define ORBX_PYR_THREADS 512   // threads per workgroup of k_pyramid_bands (PYR_T)
// groups per thread G, thread-columns ngt and thread-rows per pass rpp of a row of ng groups of 4 pixels: G (1 or 2) = whichever
// fills more of the workgroup's threads with whole rows; two only in the two-group instances
static inline void pyrColsOf(int ng, int twoGroups, uint32_t out[2]) {
  const int nThreads = ORBX_PYR_THREADS;
  ng = ng < 1 ? 1 : ng;
  const int ngt2 = (ng + 1) >> 1;
  const int use1 = ng <= nThreads ? ng * (nThreads / ng) : 0, use2 = ngt2 * (nThreads / ngt2);
  const int G = twoGroups && use2 > use1 ? 2 : 1;
  const int ngt = G == 2 ? ngt2 : ng;
  const int rpp = nThreads / ngt > 1 ? nThreads / ngt : 1;
  const uint32_t one = 1u << ORBX_PYR_INV_SHIFT;
  out[0] = (one + (uint32_t)ngt - 1u) / (uint32_t)ngt | (uint32_t)(ngt - 1) << 20 | (uint32_t)(G - 1) << 31;
  out[1] = (one + (uint32_t)rpp - 1u) / (uint32_t)rpp | (uint32_t)(rpp - 1) << 20;
}
// column constants of one group of 4 output pixels (host: appendPyrTables).  The group's taps lie in the 12 bytes of three
// dwords at byte offsets o[0] = (first tap & ~3), o[1], o[2] of a source row (o[1], o[2]: + 4, + 8, but never beyond the
// row's last dword, which can then only supply bytes of weight 0).
struct PyrXGroup {
  uint32_t o[3];
  uint32_t sel[6];   // v_perm_b32 selectors (bytes k, k + 1 as two u16 halves): pixel 0, 1, 2 in dwords (0, 1); pixel 2 in dwords
                     // (1, 2); pixel 3 in (0, 1); pixel 3 in (1, 2).  Of a pixel's two, the one that does not apply is 0x0c0c0c0c (zero)
  uint32_t cf[4];    // Q11 tap pair times 16: (c0 << 4) | (c1 << 4) << 16
  uint32_t pad[3];
};
static_assert(sizeof(PyrXGroup) == 64, "PyrXGroup is read as four uint4");
struct PyrYRow {     // one output row: byte offsets of its two source rows (already clamped), Q11 weights << 8
  uint32_t off0, off1, wy0, wy1;
};

// k_check_model: CheckHomography (kind 0) / CheckFundamental (kind 1) over nModels hypotheses
// Hypothesis m belongs to pair p = m / perPair, whose N is pairN[p], whose matches are first / second + p * stride, whose
// keypoints are k1 / k2 + frames[p] * stride / frames[nPairs + p] * stride, and whose inlier flags go to inliers + m * stride
// (one pair from host arrays: nPairs = 1, frames {0, 0}, stride = N)
struct ScoreArgs {
  const float* M21;   // [nModels][9] row-major H21 / F21
  const float* M12;   // [nModels][9] H12 (kind 0 only)
  const orbx_keypoint* k1;
  const orbx_keypoint* k2;
  const int32_t* first;   // mvMatches12[i].first / .second
  const int32_t* second;
  int32_t kind;
  float invSigmaSquare;
  float* scores;      // [nModels]
  uint8_t* inliers;   // [nModels][stride]
  const int32_t* pairN;
  const int32_t* frames;  // [2][nPairs]
  int32_t perPair, stride, nPairs;
};

// k_check_rt: CheckRT (Initializer.cpp:569-713) over nModels (R21, t21) hypotheses.  Model m is candidate m % perPair of pair
// p = m / perPair, with pairNInl[p] points at pts / book + p * stride (none when m % perPair >= pairNSol[p]); good / p3d / cosBuf
// of model m at m * stride, n1 = stride (one pair from host arrays: perPair = pairNSol[0] = nModels, stride = n1)
struct CheckRtArgs {
  const float* R21;      // [nModels][9]
  const float* t21;      // [nModels][3]
  const float* pts;      // [nPairs][stride][4] (u1, v1, u2, v2) of the inlier matches, in match order
  const int32_t* book;   // [nPairs][stride] keypoint of frame 1 the i-th triangulated point is booked under (the reference's quirk)
  float K[9];
  float th2;
  uint8_t* good;         // [nModels][stride]
  float* p3d;            // [nModels][stride][3]
  float* cosBuf;         // [nModels][stride] scratch: cosines of the counted points
  int32_t* nGood;        // [nModels]
  float* parallax;       // [nModels]
  const int32_t* pairNInl;
  const int32_t* pairNSol;
  int32_t perPair, stride;
};


// k_init_*: the RANSAC stage of Initializer::Initialize (Initializer.cpp:19-111) over nPairs pairs x nIter hypotheses
struct InitArgs {
  const orbx_keypoint* kps;  // [frames][cap] mvKeysUn
  const int32_t* nKps;       // [frames]
  const int32_t* m12;        // [nPairs][cap] the matcher's vnMatches12
  const int32_t* sets;       // [nPairs][nIter][8] mvSets
  const int32_t* frames;     // [2][nPairs] first frames, then second frames
  int32_t nPairs, nIter, cap;
  int32_t* N;                // [nPairs] |mvMatches12|
  int32_t* scoreN;           // [nPairs] N, or 0 for a pair whose matches cannot be used (nothing is scored)
  int32_t* pstat;            // [nPairs] ORBX_INIT_* bits found by k_init_prep
  int32_t* first;            // [nPairs][cap] mvMatches12 (first, second)
  int32_t* second;
  float* H21;                // [nPairs * nIter][9]
  float* H12;
  float* F21;
  uint8_t* flags;            // [2][nPairs * nIter] INIT_FLAG_* of the H, then the F hypotheses
  const float* scoresH;      // [nPairs * nIter] (k_check_model)
  const float* scoresF;
  const uint8_t* inlH;       // [nPairs * nIter][cap]
  const uint8_t* inlF;
  orbx_hf_result* res;       // [nPairs]
  uint8_t* inlOut;           // nullable [nPairs][2][cap]: the kept hypotheses' inlier flags (H, then F)
  // reconstruction (orbx_initialize*): k_init_select also decomposes the chosen model and lists its inliers for CheckRT
  int32_t reconstruct;
  float K[9];
  float minParallax;
  int32_t minTriangulated;
  float* R4;                 // [nPairs * 4][9] candidates
  float* t4;                 // [nPairs * 4][3]
  int32_t* nSol;             // [nPairs]
  int32_t* nInl;             // [nPairs]
  float* pts;                // [nPairs][cap][4] (u1, v1, u2, v2) of the chosen model's inliers, in match order
  int32_t* book;             // [nPairs][cap] the i-th inlier's keypoint of frame 1 = mvMatches12[i].first (CheckRT's quirk)
  const int32_t* nGood;      // [nPairs * 4] (k_check_rt)
  const float* parallax;
  const uint8_t* good;       // [nPairs * 4][cap]
  const float* p3d4;         // [nPairs * 4][cap][3]
  orbx_init_result* ires;    // [nPairs]
  float* p3dOut;             // nullable [nPairs][cap][3]
  uint8_t* triOut;           // nullable [nPairs][cap]
};
constexpr int INIT_FLAG_H_DEGENERATE = 1, INIT_FLAG_F_DEGENERATE = 2, INIT_FLAG_BAD_SET = 4;

// camera of cv::undistortPoints in the doubles OpenCV converts mK / mDistCoef (CV_32F, Settings.hpp:32,39) to
struct CamD {
  double fx, fy, cx, cy, ifx, ify;  // ifx = 1./fx, ify = 1./fy
  double k0, k1, k2, k3;            // k1 k2 p1 p2 of the reference = OpenCV's k[0..3]
  int32_t distorted, pad_;          // mDistCoef.at<float>(0) != 0 (Frame.cpp:103,138)
};

// ---- SearchForInitialization scratch (ints per pair; one place for the host allocation and the launches) ----
// matchGeneral needs 4 * capacity; the wide path (k_match_wide_*) a header, one record per eligible train, the query index
// list, the per-query candidate counts and MW_CP list entries per query, all for min(capacity, MW_CAP) queries / trains.
constexpr int MW_CAP = 4096;  // octave-0 queries / eligible trains per pair the wide path takes
constexpr int MW_CP = 128;    // candidates listed per query (a fuller window hands the pair to k_match)
constexpr int MW_CXS = 80;    // behind the top rows and the queries' column order: start slot of every grid column's trains (65 used)
constexpr int MW_TOPK = 4;   // four spare rows behind every query's list (round 3 kept the best candidates there; the lists are sorted in place now)
constexpr int MW_HDR = 16;    // [0] nQ, [1] nT, [2] 1 = too large for the wide path, [3] != 0 = a list overflowed, [4..7] bounding box of the eligible trains (float bits: min x, max x, min y, max y), [8] 1 = trains stored by grid column (matchWidePrep)
inline int matchWideCap(int capacity) { return capacity < MW_CAP ? capacity : MW_CAP; }
inline long long matchScratchStride(int capacity) {
  const long long capl = matchWideCap(capacity);
  long long s = (long long)capacity * 4;
  const long long wide = MW_HDR + capl * (4 + 1 + 1) + capl * (MW_CP + MW_TOPK) + capl + MW_CXS;  // ... + query order by column + column starts
  if (s < wide) s = wide;
  return (s + 3) & ~3LL;  // the train records are uint4
}

// ---- DBoW2 TemplatedVocabulary::transform / L1Scoring::score (orbx_bow_kernel.hip) ----
// One vocabulary node in breadth-first order: a node's children are the contiguous range [first, first + nChild).
struct BowNode {
  int32_t first;   // breadth-first index of the first child (0 when nChild == 0)
  int32_t nChild;  // 0 = isLeaf() (DBoW2: "has no children", not the file's leaf flag)
  uint32_t word;   // word id (0 for a node the file does not flag as a leaf, as the reference's Node())
  uint32_t id;     // the loader's node id (root 0, then the file's lines 1, 2, ...)
  double weight;
};
static_assert(sizeof(BowNode) == 24, "BowNode layout");
constexpr int BOW_MAX_FEATURES = 16384;  // keypoints per frame (ORBX_E_CAPACITY above)
constexpr int BOW_LDS_NODES = 1152;      // breadth-first prefix of descriptors k_bow_descend stages in LDS (36 KB: levels 0-3 at k = 10)
constexpr int BOW_DESCEND_THREADS = 512;
constexpr int BOW_ASSEMBLE_THREADS = 1024;
constexpr int BOW_SCORE_WAVES = 4;  // pairs (one wave each) per k_bow_score_l1 workgroup
struct BowArgs {
  const BowNode* nodes;   // [nNodes + 1] breadth-first
  const uint32_t* desc;   // [nNodes + 1][8] breadth-first, 32-byte aligned
  int32_t nStaged;        // breadth-first nodes whose descriptors k_bow_descend stages in LDS
  int32_t nidLevel;       // L - levelsup
  const uint8_t* fdesc;   // [nFrames][cap][32]
  const int32_t* n;       // [nFrames] (clamped to [0, cap])
  int32_t cap, nFrames;
  uint32_t* fin;          // scratch [nFrames][cap]: breadth-first index of the node the descent ended at
  uint32_t* nid;          // scratch [nFrames][cap]: node id at depth nidLevel (FeatureVector)
  int32_t weighting;      // 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY
  int32_t norm;           // 0 none (DOT_PRODUCT), 1 L1, 2 L2
  int32_t hasWords;       // 0: the vocabulary is empty(), both vectors are empty
  uint32_t* bowWord;      // [nFrames][cap]
  double* bowValue;       // [nFrames][cap]
  int32_t* bowN;          // [nFrames]
  uint32_t* fvNode;       // nullable [nFrames][cap]
  uint32_t* fvFeat;       // nullable [nFrames][cap]
  int32_t* fvN;           // nullable [nFrames]
  uint32_t* featWord;     // nullable [nFrames][cap]
};
struct BowScoreArgs {
  const uint32_t* word;   // [frames][cap]
  const double* value;    // [frames][cap]
  const int32_t* n;       // [frames] (clamped to [0, cap])
  int32_t cap, nPairs;
  const int32_t* pairs;   // [2][nPairs] first frames, then second frames
  double* score;          // [nPairs]
};

// ---- ORBmatcher::SearchByBoW (orbx_match_bow_kernel.hip): one workgroup per (keyframe, frame) pair ----
constexpr int MB_WAVES = 4;  // waves of k_match_bow: the pair's common nodes go to them in turn
constexpr int MB_THREADS = 64 * MB_WAVES;
struct MatchBowArgs {
  const orbx_keypoint* kps;  // [nFrames][cap] (only angle is read)
  const uint8_t* desc;       // [nFrames][cap][32], 16-byte aligned
  const int32_t* n;          // [nFrames] (clamped to [0, cap])
  const uint32_t* fvNode;    // [nFrames][cap] the FeatureVectors as orbx_bow_transform_batch_device writes them
  const uint32_t* fvFeat;    // [nFrames][cap]
  const int32_t* fvN;        // [nFrames] (clamped to [0, cap])
  const uint8_t* mask;       // nullable [nFrames][cap]: 0 = the keyframe's feature has no map point
  const int32_t* pairs;      // [2][nPairs] keyframes, then frames
  int32_t cap, nPairs, checkOri;
  float nnratio;
  int32_t* matchesF;         // [nPairs][cap]
  int32_t* nmatches;         // [nPairs]
};

// ---- ORBmatcher::SearchByProjection (orbx_match_proj_kernel.hip): one workgroup per (last frame, current frame) pair ----
constexpr int MP_THREADS = 512;
// what the three projection matchers take alike: the camera, the search radius factor, the image bounds and the pyramid's scales
struct MatchCamArgs {
  float fx, fy, cx, cy, th;
  orbx_bounds b;
  int32_t nLevels;
  float scale[ORBX_MAX_LEVELS];  // the context's mvScaleFactor
};
struct MatchProjArgs {
  const orbx_keypoint* kps;    // [nFrames][cap] undistorted
  const uint8_t* desc;         // [nFrames][cap][32], 16-byte aligned
  const int32_t* n;            // [nFrames] (clamped to [0, cap])
  const float* points;         // [nSets][cap][3]
  const uint8_t* pointMask;    // nullable [nSets][cap]
  const uint8_t* pointDesc;    // nullable [nSets][cap][32], 16-byte aligned
  const uint8_t* lastOutlier;  // nullable [nPairs][cap]
  const float* pose;           // [nPairs][12]
  const int32_t* pairs;        // [3][nPairs] last frames, current frames, point sets
  int32_t cap, nPairs, checkOri;
  MatchCamArgs cam;
  int32_t* matchesCur;         // [nPairs][cap]
  orbx_proj_result* res;       // [nPairs]
};

// ---- ORBmatcher::SearchByProjection(Frame, local map points) (orbx_match_local_kernel.hip): one workgroup of MP_THREADS per
// (frame, map set) pair ----
struct MatchLocalArgs {
  const orbx_keypoint* kps;   // [nFrames][cap] undistorted
  const uint8_t* desc;        // [nFrames][cap][32], 16-byte aligned
  const int32_t* n;           // [nFrames] (clamped to [0, cap])
  const int32_t* mapN;        // [nSets] (clamped to [0, mapCap])
  const float* mapPoints;     // [nSets][mapCap][3]
  const float* mapNormals;    // [nSets][mapCap][3]
  const float* mapDist;       // [nSets][mapCap][2] mfMinDistance, mfMaxDistance
  const uint8_t* mapDesc;     // [nSets][mapCap][32], 16-byte aligned
  const uint8_t* mapMask;     // nullable [nSets][mapCap]
  const uint8_t* outlier;     // nullable [nPairs][cap]
  const float* pose;          // [nPairs][12]
  const int32_t* pairs;       // [2][nPairs] frames, map sets
  int32_t cap, mapCap, nPairs;
  float nnratio;
  MatchCamArgs cam;
  int32_t* matches;           // [nPairs][cap] in and out
  uint8_t* pointView;         // nullable [nPairs][mapCap]
  orbx_local_result* res;     // [nPairs]
};

// ---- ORBmatcher::SearchByProjection(Frame, KeyFrame, sAlreadyFound, th, ORBdist) (orbx_match_kfproj_kernel.hip): one workgroup of
// MP_THREADS per (keyframe, current frame) pair ----
struct MatchKfProjArgs {
  const orbx_keypoint* kps;   // [nFrames][cap] undistorted
  const uint8_t* desc;        // [nFrames][cap][32], 16-byte aligned
  const int32_t* n;           // [nFrames] (clamped to [0, cap])
  const float* points;        // [nSets][cap][3] the keyframe's map points, per feature
  const uint8_t* pointMask;   // nullable [nSets][cap]
  const uint8_t* pointDesc;   // nullable [nSets][cap][32], 16-byte aligned
  const float* pointDist;     // [nSets][cap][2] mfMinDistance, mfMaxDistance
  const uint8_t* outlier;     // nullable [nPairs][cap]
  const float* pose;          // [nPairs][12]
  const int32_t* pairs;       // [3][nPairs] keyframes, current frames, point sets
  int32_t cap, nPairs, orbDist, checkOri;
  MatchCamArgs cam;
  int32_t* matches;           // [nPairs][cap] in and out
  orbx_kfproj_result* res;    // [nPairs]
};

// ---- ORBmatcher::SearchByProjection(KeyFrame, Scw, loop map points, vpMatched, th) (orbx_match_scw_kernel.hip): one workgroup
// of MP_THREADS per (current keyframe, map set) pair; and the composition Scw = S12 * Tmw in front of it, a lane per pair ----
struct MatchScwArgs {
  const orbx_keypoint* kps;   // [nFrames][cap] undistorted
  const uint8_t* desc;        // [nFrames][cap][32], 16-byte aligned
  const int32_t* n;           // [nFrames] (clamped to [0, cap])
  const int32_t* mapN;        // [nSets] (clamped to [0, mapCap])
  const float* mapPoints;     // [nSets][mapCap][3]
  const float* mapNormals;    // [nSets][mapCap][3]
  const float* mapDist;       // [nSets][mapCap][2] mfMinDistance, mfMaxDistance
  const uint8_t* mapDesc;     // [nSets][mapCap][32], 16-byte aligned
  const uint8_t* mapMask;     // nullable [nSets][mapCap]
  const float* scw;           // [nPairs][12] sR row-major, then t
  const int32_t* kf2ToMap;    // nullable [nPairs][cap]: the matched keyframe's feature -> an index into the map set, or negative
  const int32_t* pairs;       // [2][nPairs] current keyframes, map sets
  int32_t cap, mapCap, nPairs, thLow;
  MatchCamArgs cam;
  int32_t* matches;           // [nPairs][cap] in and out
  orbx_scw_result* res;       // [nPairs]
};
struct Sim3ComposeArgs {
  const float* pose;          // [nFrames][12] Tcw per frame
  const float* sim3;          // [nPairs][13] R12 row-major, t12, s12
  const int32_t* kf2;         // [nPairs] the matched keyframes
  int32_t nPairs;
  float* scw;                 // [nPairs][12]
};

// ---- ORBmatcher::Fuse, both overloads (orbx_match_fuse_kernel.hip): one workgroup of MP_THREADS per (keyframe, map set) pair ----
struct MatchFuseArgs {
  const orbx_keypoint* kps;   // [nFrames][cap] undistorted
  const uint8_t* desc;        // [nFrames][cap][32], 16-byte aligned
  const int32_t* n;           // [nFrames] (clamped to [0, cap])
  const int32_t* mapN;        // [nSets] (clamped to [0, mapCap])
  const float* mapPoints;     // [nSets][mapCap][3]
  const float* mapNormals;    // [nSets][mapCap][3]
  const float* mapDist;       // [nSets][mapCap][2] mfMinDistance, mfMaxDistance
  const uint8_t* mapDesc;     // [nSets][mapCap][32], 16-byte aligned
  const uint8_t* mapMask;     // nullable [nSets][mapCap]
  const int32_t* mapObs;      // [nSets][mapCap] Observations(); the pose form only (null in the Scw form)
  const float* pose;          // [nPairs][12]: Rcw row-major, then tcw (pose form); sR row-major, then t (Scw form)
  const int32_t* pairs;       // [2][nPairs] keyframes, map sets
  int32_t cap, mapCap, nPairs, thLow;
  MatchCamArgs cam;
  float invSigma2[ORBX_MAX_LEVELS];  // the context's mvInvLevelSigma2 (the pose form's chi-square gate)
  int32_t* matches;           // [nPairs][cap] in and out
  const int32_t* occObs;      // nullable [nPairs][cap]
  int32_t* fuseIdx;           // [nPairs][mapCap]
  uint8_t* fuseAct;           // [nPairs][mapCap]
  int32_t* fuseOther;         // [nPairs][mapCap]
  orbx_fuse_result* res;      // [nPairs]
};

// ---- ORBmatcher::SearchBySim3 (orbx_match_sim3_kernel.hip): one workgroup of MP_THREADS per (KF1, KF2) pair ----
struct MatchSim3Args {
  const orbx_keypoint* kps;   // [nFrames][cap] undistorted
  const uint8_t* desc;        // [nFrames][cap][32], 16-byte aligned
  const int32_t* n;           // [nFrames] (clamped to [0, cap])
  const float* points;        // [nSets][cap][3] a keyframe's map points, per feature
  const uint8_t* pointMask;   // nullable [nSets][cap]
  const uint8_t* pointDesc;   // nullable [nSets][cap][32], 16-byte aligned
  const float* pointDist;     // [nSets][cap][2] mfMinDistance, mfMaxDistance
  const float* pose;          // [nFrames][12] Tcw per frame
  const float* sim3;          // [nPairs][13] R12 row-major, t12, s12
  const int32_t* pairs;       // [4][nPairs] KF1s, KF2s, KF1s' point sets, KF2s' point sets
  int32_t cap, nPairs, orbDist;
  MatchCamArgs cam;
  int32_t* matches;           // [nPairs][cap] in and out, indexed by KF1's feature
  orbx_msim3_result* res;     // [nPairs]
};

// ---- LocalMapping::CreateNewMapPoints (orbx_match_tri_kernel.hip): SearchForTriangulation, one workgroup of MB_THREADS per
// (KF1, KF2) pair as k_match_bow; then the triangulation, TT_THREADS features of a pair per workgroup ----
constexpr int TT_THREADS = 256;
struct TriCamArgs {
  float fx, fy, cx, cy, scaleFactor;
  int32_t nLevels;
  float scale[ORBX_MAX_LEVELS];   // the context's mvScaleFactor
  float sigma2[ORBX_MAX_LEVELS];  // the context's mvLevelSigma2
};
struct MatchTriArgs {
  const orbx_keypoint* kps;  // [nFrames][cap] undistorted
  const uint8_t* desc;       // [nFrames][cap][32], 16-byte aligned
  const int32_t* n;          // [nFrames] (clamped to [0, cap])
  const uint32_t* fvNode;    // [nFrames][cap]
  const uint32_t* fvFeat;    // [nFrames][cap]
  const int32_t* fvN;        // [nFrames] (clamped to [0, cap])
  const uint8_t* mask;       // nullable [nFrames][cap]: != 0 = the feature has a map point
  const float* pose;         // [nFrames][12]
  const float* medianDepth;  // nullable [nFrames]
  const int32_t* pairs;      // [2][nPairs] KF1s, then KF2s
  int32_t cap, nPairs, checkOri;
  TriCamArgs cam;
  int32_t* matches12;          // [nPairs][cap]
  orbx_tri_match_result* res;  // [nPairs]
};
struct TriangulateArgs {
  const orbx_keypoint* kps;  // [nFrames][cap] undistorted
  const int32_t* n;          // [nFrames] (clamped to [0, cap])
  const float* pose;         // [nFrames][12]
  const int32_t* pairs;      // [2][nPairs] KF1s, then KF2s
  const int32_t* matches12;  // [nPairs][cap]
  int32_t cap, nPairs;
  TriCamArgs cam;
  float* points;           // [nPairs][cap][3]
  uint8_t* pointMask;      // [nPairs][cap]
  float* pointNormal;      // [nPairs][cap][3]
  float* pointDist;        // [nPairs][cap][2]
  orbx_tri_result* res;    // [nPairs], zero on entry: the workgroups of a pair add to it
};

// ---- DBoW2 TemplatedDatabase (orbx_db_kernel.hip): a CSR inverted file, batched add and query ----
constexpr int DB_THREADS = 256;       // threads of the database kernels
constexpr int DB_WAVES = DB_THREADS / 64;  // waves of k_db_accumulate: each owns a sub-slice of the workgroup's entries
constexpr int DB_SLICE_MAX = 2048;    // entries of one k_db_accumulate workgroup (the default), and the most keys sorted in LDS
constexpr int DB_MAX_RESULTS = 256;   // ORBX_DB_MAX_RESULTS
constexpr int DB_MERGE_MAX = 8;       // lists one k_db_merge workgroup merges (the default): DB_MERGE_MAX * DB_MAX_RESULTS keys
static_assert(DB_MERGE_MAX * DB_MAX_RESULTS <= DB_SLICE_MAX, "a merge sorts its lists in the LDS of one slice");
constexpr int DB_SCAN_THREADS = 1024;
struct DbAddArgs {
  const uint32_t* word;     // [nFrames][cap] the batch's BowVectors (orbx_bow_transform_batch_device's layout)
  const double* value;      // [nFrames][cap]
  const int32_t* n;         // [nFrames] (clamped to [0, cap])
  int32_t cap, nFrames;
  uint32_t nWords, firstId; // the vocabulary's words; the entry id of frame 0
  uint32_t oldTotal;        // postings in the old file
  uint32_t* cnt;            // [nWords] zero before k_db_count, zero again after k_db_scatter
  const uint32_t* oldRow;   // [nWords + 1]
  const uint32_t* oldEntry;
  const double* oldValue;
  uint32_t* newRow;         // [nWords + 1]
  uint32_t* newEntry;
  double* newValue;
  uint32_t* tmpWord;        // the batch's postings grouped by word, in arrival order within a word
  uint32_t* tmpFrame;
  double* tmpValue;
};
struct DbQueryArgs {
  const uint32_t* word;     // [nQueries][cap]
  const double* value;
  const int32_t* n;
  int32_t cap, nQueries;
  uint32_t nWords;
  const uint32_t* row;      // the inverted file
  const uint32_t* entry;
  const double* pvalue;
  int32_t scoring, binary;  // binary: DOT_PRODUCT's term is 1 (BINARY weighting)
  int32_t minCommon;        // common words an entry needs to be listed (1, or MIN_COMMON_WORDS)
  int32_t descending;       // best first = the largest sum (BHATTACHARYYA, DOT_PRODUCT)
  int32_t limit;            // entries [0, limit) take part (max_id)
  int32_t perSlice, nSlices, maxResults;
  double* listRaw;          // [nQueries][nSlices][maxResults] every slice's best: the sums ...
  uint32_t* listId;         // ... and the entry ids
  int32_t* listN;           // [nQueries][nSlices]
};
struct DbMergeArgs {
  int32_t nQueries, nIn, nOut, perMerge, maxResults, scoring, descending;
  const double* inRaw;      // [nQueries][nIn][maxResults]
  const uint32_t* inId;
  const int32_t* inN;       // [nQueries][nIn]
  double* outRaw;           // [nQueries][nOut][maxResults] (not the last round)
  uint32_t* outId;
  int32_t* outN;
  int32_t* resEntry;        // the last round (nOut == 1): [nQueries][maxResults] entry ids, final scores, counts
  double* resScore;
  int32_t* resN;
};

// ---- DBoW2 TemplatedVocabulary::create (orbx_voc_train_kernel.hip): one tree level at a time ----
constexpr int VT_THREADS = 256;   // threads of the training kernels, and the features of one block of the level's block table
constexpr int VT_CHUNK = 4096;    // features one workgroup of k_vt_count counts (a node with more has global counters)
constexpr int VT_SEED_LDS = 4096; // the largest node the one-workgroup seeding takes (its distances live in LDS)
constexpr int VT_KMAX = 20;
constexpr int VT_DF_THREADS = 1024;
enum { VT_RUNNING = 0, VT_CONVERGED = 1, VT_CAPPED = 2, VT_TRIVIAL = 3 };
struct VtNode {      // a node being split at this level
  uint64_t key;      // of the node's draws (root 0, child i of K: 21 K + i + 1)
  int32_t start, n;  // its features: perm[start, start + n), ascending original order
  int32_t nC;        // centres
  int32_t state, rounds, changed;
  int32_t form;      // 0: seeded by one workgroup (and the trivial case n <= k), 1: grid-wide seeding
  int32_t blk0;      // the node's first block in the block table
  int32_t multi;     // index of its global bit counters (more than one chunk of k_vt_count), -1: none
  int32_t seedDone, draws, pad;
};
static_assert(sizeof(VtNode) == 56, "VtNode layout");
struct VtArgs {
  const uint32_t* feat;   // descriptors [slots][8]; a feature is named by its slot (document * capacity + index)
  uint32_t* perm;         // [N] slots, every node's features contiguous
  uint32_t* permOut;      // [N] the regrouped order
  uint8_t* assoc;         // [N] cluster of the feature at a position
  int32_t* minDist;       // [N] grid-wide seeding: distance to the nearest centre, by position
  VtNode* nodes;          // [nNodes]
  uint32_t* centres;      // [nNodes][k][8]
  int32_t nNodes, k, maxRounds, nBlk;
  uint64_t seed;
  const int32_t* blkNode;   // [nBlk] block table: node and first position of blocks of VT_THREADS positions
  const int32_t* blkStart;  // [nBlk]
  uint32_t* blkSum;         // [nBlk] seeding: the block's distance sum
  int32_t* blkHist;         // [nBlk][k] regrouping: members per cluster, then their exclusive prefix within the node
  int32_t* nodeHist;        // [nNodes][k] members per cluster
  int32_t* childBase;       // [nNodes][k] first position of each cluster's group
  const int32_t* list;      // node indices a launch runs over (small nodes, large nodes, multi-chunk nodes)
  int32_t nList, nChunk;
  const int32_t* chNode;    // [nChunk] chunk table of k_vt_count: node, first position
  const int32_t* chStart;
  uint32_t* gCnt;           // [multi][k][256 + 1] global bit counters and the group size (zero between rounds)
  int32_t* stats;           // [8] orbx_vocabulary_train's statistics; [8] nodes still running after this round
};

// k_ba: the two-view bundle adjustment (include/orbx.h, "behind the Initializer: two-view bundle adjustment"), a workgroup per pair
constexpr int BA_THREADS = 256;     // lanes of the workgroup = the stride of the points over the lanes
constexpr int BA_WS_DOUBLES = 33;   // per point: estimate 3, its backup 3, Hll 6, bl 3, Hpl 18
constexpr int BA_WS_FLOATS = 6;     // per point: u1 v1 u2 v2, inv_sigma2 of the two keypoints' octaves
struct BaArgs {
  const orbx_keypoint* kps;      // [frames][cap] mvKeysUn
  const int32_t* nKps;           // [frames]
  const int32_t* m12;            // [nPairs][cap]
  const int32_t* frames;         // [2][nPairs] first frames, then second frames
  const orbx_init_result* ires;  // [nPairs]
  const float* p3d;              // [nPairs][cap][3]
  const uint8_t* tri;            // [nPairs][cap]
  const float* invSigma2;        // [nLevels] (device)
  orbx_ba_result* res;           // [nPairs]
  float* p3dOut;                 // [nPairs][cap][3], may be p3d
  double* ws;                    // [nPairs][BA_WS_DOUBLES][cap]
  float* wf;                     // [nPairs][BA_WS_FLOATS][cap]
  int32_t* widx;                 // [nPairs][cap] the point vertex's keypoint of frame 1
  double fx, fy, cx, cy, delta;
  int32_t nPairs, cap, nLevels, nIterations, minPoints, normalize;
};

// k_pose: Optimizer::PoseOptimization (include/orbx.h, "behind SearchByBoW: pose optimisation"), a wave per problem
constexpr int POSE_WAVES = 4;  // problems per workgroup; the waves share nothing
constexpr int POSE_THREADS = 64 * POSE_WAVES;
constexpr int POSE_CACHE = 6;  // edges per lane a wave keeps in LDS (384 per problem when they are spread evenly); 12 KB per wave
struct PoseArgs {
  const orbx_keypoint* kps;   // [frames][cap] mvKeysUn
  const int32_t* nKps;        // [frames]
  const int32_t* problems;    // [2][nProblems] frames, then point sets
  const int32_t* match;       // nullable [nProblems][cap]
  const float* points;        // [sets][cap][3]
  const uint8_t* mask;        // nullable [sets][cap]
  const float* pose0;         // [nProblems][12]
  const float* invSigma2;     // [nLevels] (device)
  orbx_pose_result* res;      // [nProblems]
  uint8_t* outlier;           // [nProblems][cap]
  double fx, fy, cx, cy, delta;
  int32_t nProblems, cap, nLevels, nIterations;
};

// k_pnp_*: PnPsolver (include/orbx.h, "behind SearchByBoW: PnP RANSAC"): prep and refine a wave per problem, the hypotheses a
// lane per (problem, iteration)
constexpr int PNP_CORR_BYTES = 32;   // orbx_pnp::Corr
constexpr int PNP_HYP_BYTES = 112;   // orbx_pnp::Hyp
constexpr int PNP_MAX_CAPACITY = 16384;  // ORBX_BOW_MAX_FEATURES: sizes the inlier bit sets in LDS
struct PnpArgs {
  const orbx_keypoint* kps;   // [frames][cap] mvKeysUn
  const int32_t* nKps;        // [frames]
  const int32_t* problems;    // [2][nProblems] frames, then point sets
  const int32_t* match;       // nullable [nProblems][cap]
  const float* points;        // [sets][cap][3]
  const uint8_t* mask;        // nullable [sets][cap]
  const float* sigma2;        // [nLevels] (device)
  const int32_t* table;       // [cap + 1][2] (device): mRansacMinInliers, mRansacMaxIts of N
  const int32_t* draws;       // [nProblems][nIter][4]
  orbx_pnp_result* res;       // [nProblems]
  float* pose;                // [nProblems][12]
  int32_t* matchInliers;      // [nProblems][cap]
  uint8_t* inliers;           // nullable [nProblems][cap]
  uint8_t* corr;              // workspace [nProblems][cap] Corr: the correspondences, ascending feature
  int32_t* corrOf;            // workspace [nProblems][cap]: feature j's correspondence, or -1
  int32_t* meta;              // workspace [nProblems][4]: orbx_pnp::Meta
  uint8_t* hyp;               // workspace [nProblems][nIter] Hyp
  double fu, fv, uc, vc;
  float th2;
  int32_t nProblems, cap, nLevels, nIter;
};

// k_sim3_*: Sim3Solver (include/orbx.h, "loop closing: Sim3 RANSAC"): prep and resolve a wave per problem, the hypotheses a lane
// per (problem, iteration)
constexpr int SIM3_CORR_BYTES = 56;  // orbx_sim3::Corr
constexpr int SIM3_HYP_BYTES = 64;   // orbx_sim3::Hyp
constexpr int SIM3_MAX_CAPACITY = 16384;  // ORBX_BOW_MAX_FEATURES
constexpr long long SIM3_MAX_HYPOTHESES = 2147483647LL - 63;  // n_problems * n_iter: (lanes + 63) / 64 workgroups of one wave
struct Sim3Args {
  const orbx_keypoint* kps;   // [frames][cap] mvKeysUn
  const int32_t* nKps;        // [frames]
  const int32_t* problems;    // [4][nProblems] KF1s, KF2s, KF1s' point sets, KF2s' point sets
  const int32_t* match;       // [nProblems][cap]: the feature of KF2 matched to KF1's feature, or -1
  const float* points;        // [sets][cap][3]
  const uint8_t* mask;        // nullable [sets][cap]
  const float* pose;          // [frames][12] Tcw
  const float* sigma2;        // [nLevels] (device)
  const int32_t* table;       // [cap + 1] (device): mRansacMaxIts of N
  const int32_t* draws;       // [nProblems][nIter][3]
  orbx_sim3_result* res;      // [nProblems]
  float* sim3;                // [nProblems][13]
  int32_t* matchInliers;      // [nProblems][cap]
  uint8_t* inliers;           // nullable [nProblems][cap]
  uint8_t* corr;              // workspace [nProblems][cap] Corr: the correspondences, ascending feature of KF1
  int32_t* corrOf;            // workspace [nProblems][cap]: feature i1's correspondence, or -1
  int32_t* meta;              // workspace [nProblems][4]: orbx_sim3::Meta
  uint8_t* hyp;               // workspace [nProblems][nIter] Hyp
  float fx, fy, cx, cy, th2;
  int32_t nProblems, cap, nLevels, nIter, minInliers, fixScale;
};

// k_sim3_optimize: Optimizer::OptimizeSim3 (include/orbx.h, "loop closing: Sim3 optimisation"), a wave per problem
constexpr int SIM3OPT_WAVES = 4;  // problems per workgroup; the waves share nothing
constexpr int SIM3OPT_THREADS = 64 * SIM3OPT_WAVES;
constexpr int SIM3OPT_MAX_CAPACITY = 16384;  // ORBX_BOW_MAX_FEATURES
struct Sim3OptArgs {
  const orbx_keypoint* kps;   // [frames][cap] mvKeysUn
  const int32_t* nKps;        // [frames]
  const int32_t* problems;    // [4][nProblems] KF1s, KF2s, KF1s' point sets, KF2s' point sets
  int32_t* row;               // [nProblems][cap] in and out: the feature of KF2 matched to KF1's feature, or -1
  const float* points;        // [sets][cap][3]
  const uint8_t* mask;        // nullable [sets][cap]
  const float* pose;          // [frames][12] Tcw
  const float* sim3;          // [nProblems][13] R12 row-major, t12, s12
  const float* invSigma2;     // [nLevels] (device)
  orbx_sim3opt_result* res;   // [nProblems]
  float* sim3Out;             // [nProblems][13], may be sim3
  double fx, fy, cx, cy, delta, th2;
  int32_t nProblems, cap, nLevels, nIterations, nMoreIterations, fixScale;
};
// k_lba: Optimizer::LocalBundleAdjustment (include/orbx.h, "local mapping: local bundle adjustment"), a workgroup per problem
constexpr int LBA_THREADS = 256;
struct LbaArgs {
  const orbx_keypoint* kps;   // [frames][cap] mvKeysUn
  const int32_t* nKps;        // [frames]
  const float* pose;          // [frames][12]
  const int32_t* rows;        // [nEntries][cap]
  const int32_t* problems;    // [5][nProblems]: first entry, entries, free entries, map set, workspace offset / 256
  const int32_t* entryFrame;  // [nEntries]
  const int32_t* mapN;        // [mapSets]
  const float* mapPts;        // [mapSets][mapCap][3]
  const uint8_t* mapMask;     // [mapSets][mapCap] or null
  const float* invSigma2;     // [nLevels] (device)
  float* poseOut;             // [nEntries][12]
  float* mapOut;              // [mapSets][mapCap][3], may be mapPts
  uint8_t* outlier;           // [nEntries][cap]
  orbx_lba_result* res;       // [nProblems]
  uint8_t* ws;                // the problems' workspaces
  double fx, fy, cx, cy, delta;
  int32_t nProblems, cap, mapCap, nLevels, nIterations, nMoreIterations;
  int32_t ldsMaxFree;         // problems with at most this many free keyframes keep the packed factor in LDS
  uint32_t ldsBytes;          // dynamic LDS of the launch: the largest such factor
};
// k_map_build, k_map_points: the map points behind a local bundle adjustment (include/orbx.h, "local mapping: updating the map
// points")
constexpr int MAP_THREADS = 512;  // k_map_build: one workgroup per problem
constexpr int MAP_WAVES = 4;      // k_map_points: waves per workgroup, one point per wave at a time
constexpr int MAP_CHUNK = 64;     // k_map_points: points per workgroup
// A problem's part of the workspace, every array 256-byte aligned: the one description the host sizes it by and the kernels
// find their arrays by (base 0 only counts).
struct MapWork {
  int32_t* state;   // [mapCap] PT_VERTEX | PT_LOST | PT_BAD (csrc/orbx_map_math.inc)
  int32_t* cnt;     // [mapCap] observers left behind the erasures
  int32_t* refEnt;  // [mapCap] the reference keyframe's entry
  int32_t* slot;    // [mapCap][nE] the inverse of the rows: the feature of entry e that names the point, or -1
  int32_t* list;    // [mapCap][nE] the point's observers (entries), ascending, cnt of them
  float* ow;        // [nE][3] the entries' camera centres
  int32_t* flag;    // [1] the problem's status, for k_map_points
};
ORBX_HD inline size_t mapWorkLayout(int mapCap, int nE, uintptr_t base, MapWork* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const uintptr_t p = base + off;
    off += (bytes + 255) / 256 * 256;
    return p;
  };
  const size_t mc = (size_t)mapCap, ne = (size_t)nE;
  w->state = (int32_t*)take(mc * 4);
  w->cnt = (int32_t*)take(mc * 4);
  w->refEnt = (int32_t*)take(mc * 4);
  w->slot = (int32_t*)take(mc * ne * 4);
  w->list = (int32_t*)take(mc * ne * 4);
  w->ow = (float*)take(ne * 12);
  w->flag = (int32_t*)take(4);
  return off;
}
struct MapArgs {
  const orbx_keypoint* kps;   // [frames][cap] mvKeysUn
  const uint8_t* desc;        // [frames][cap][32]
  const int32_t* nKps;        // [frames]
  const float* entryPose;     // [nEntries][12]
  int32_t* rows;              // [nEntries][cap], in and out
  const uint8_t* outlier;     // [nEntries][cap] or null
  const int32_t* problems;    // [5][nProblems]: first entry, entries, free entries, map set, workspace offset / 256
  const int32_t* entryFrame;  // [nEntries]
  const int32_t* mapN;        // [mapSets]
  const float* mapPts;        // [mapSets][mapCap][3]
  const uint8_t* mapMask;     // [mapSets][mapCap] or null
  uint8_t* mapMaskOut;       // [mapSets][mapCap]
  int32_t* mapRef;            // [mapSets][mapCap] or null
  const float* scale;         // [nLevels] (device) mvScaleFactor
  float* mapNormals;          // [mapSets][mapCap][3]
  float* mapDist;             // [mapSets][mapCap][2]
  uint8_t* mapDesc;           // [mapSets][mapCap][32]
  int32_t* mapObs;            // [mapSets][mapCap]
  orbx_map_result* res;       // [nProblems]
  uint8_t* ws;                // the problems' workspaces
  int32_t nProblems, cap, mapCap, nLevels, what;
};
// k_stereo_match, k_stereo_filter: Frame::ComputeStereoMatches for rigs of one extract batch (include/orbx.h, "stereo: matching left
// and right")
constexpr int STEREO_THREADS = 256;                            // both kernels
constexpr int STEREO_WAVES = STEREO_THREADS / 64;              // k_stereo_match: one left keypoint per wave at a time
constexpr int STEREO_PER_WAVE = 8;                             // ... and this many one after the other
constexpr int STEREO_BLOCK = STEREO_WAVES * STEREO_PER_WAVE;   // left keypoints per workgroup
constexpr int STEREO_CHUNK = 2048;                             // right keypoints whose records are in LDS at a time
constexpr int STEREO_WS = 16;                                  // int32 words of a rig's counters (orbx_stereo_math.inc's Counter)
struct StereoLevel {  // a pyramid level as the correlation reads it (40 bytes, no padding: held by memcmp)
  int64_t imgOff;       // levels >= 1: byte offset of frame 0's image inside the pyramid buffer; level 0: 0
  int64_t frameStride;  // bytes between consecutive frames (level 0: the caller's)
  int32_t cols, rows, stride, pad;
  float scale, invScale;
};
struct StereoArgs {
  const orbx_keypoint* kps;  // [frames][cap] mvKeys
  const uint8_t* desc;       // [frames][cap][32], 16-byte aligned
  const int32_t* nKps;       // [frames]
  const int32_t* rigs;       // [2][nRigs]: left frame, right frame
  const uint8_t* img0;       // level 0 of frame 0: the last extract call's frames, read in place
  const uint8_t* pyr;        // levels >= 1
  const StereoLevel* lev;    // [nLevels] (device)
  float* uRight;             // [nRigs][cap]
  float* depth;              // [nRigs][cap]
  int32_t* matchRight;       // [nRigs][cap] or null
  int32_t* sad;              // [nRigs][cap]: the caller's, or the context's own
  int32_t* ws;               // [nRigs][STEREO_WS], zero before k_stereo_match
  const orbx_keypoint* kpsUn;  // [frames][cap] or null: k_stereo_filter's (u, v)
  const float* poseWc;       // [nRigs][12] or null
  float* points;             // [nRigs][cap][3] or null
  uint8_t* pointMask;        // [nRigs][cap] or null
  orbx_stereo_result* res;   // [nRigs]
  float bf, maxD, cx, cy, invfx, invfy;
  int32_t nRigs, cap, nLevels;
};
}  // namespace orbx
