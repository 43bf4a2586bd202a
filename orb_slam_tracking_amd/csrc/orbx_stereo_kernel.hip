// orbx_stereo_kernel.hip — Frame::ComputeStereoMatches and Frame::UnprojectStereo for rigs (left frame, right frame) of one extract
// batch (include/orbx.h, "stereo: matching left and right"), on the keypoints, descriptors and pyramid the extraction left in HBM.
//
//   k_stereo_match   grid (rigs, blocks of 32 left keypoints),   the right frame's records (row band as two int16, x, octave) built
//                    4 waves per workgroup                      once per workgroup into LDS, 2048 at a time; a wave per left
//                                                               keypoint, eight one after the other: every record of the chunk
//                                                               tested (lane = record), the survivors compacted through a ballot
//                                                               into a list of the wave, a lane per survivor popcounts its 32
//                                                               bytes against the left descriptor, the wave's minimum of
//                                                               d << 16 | iR is rule 6; then the correlation on the same wave
//                                                               (lane = 4 row + q, the shifts q, q + 4, q + 8), the parabola
//                                                               and the disparity gate
//   k_stereo_filter  workgroup per rig                           the median of the kept SADs by selection on counts (two passes
//                                                               of a 256-bin LDS histogram), the removals, the unprojection, the
//                                                               record
//
// The arithmetic is csrc/orbx_stereo_math.inc, shared with the CPU restatement.  Integer atomics only (counters and histogram
// bins: order-independent); f32 without contraction.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/orbx.h"
#include "orbx_launch.h"

#define ORBX_STEREO_FN __device__
#include "orbx_stereo_math.inc"

namespace orbx {
using namespace orbx_stereo;

namespace {

struct Rec {  // a right keypoint as the search reads it
  float x;
  uint32_t band;  // minr | maxr << 16, both int16; an empty band has minr > maxr
  int32_t oct;
};

struct MatchShared {
  Rec rec[STEREO_CHUNK];
  uint32_t best[STEREO_WAVES][STEREO_PER_WAVE];  // per left keypoint of the workgroup: the smallest d << 16 | iR so far
  uint16_t list[STEREO_WAVES][128];              // per wave: the survivors waiting for a full round of 64
  int32_t count[cCount];                         // the workgroup's part of the rig's counters
};

__device__ inline int clampCount(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

__device__ inline uint32_t waveMin(uint32_t v) {
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
    v = o < v ? o : v;
  }
  return v;
}

// a lane's descriptor against the left one (eight dwords, uniform over the wave)
__device__ inline int hamming(const uint8_t* desc, const uint32_t (&left)[8]) {
  const uint4* p = (const uint4*)desc;
  const uint4 a = p[0], b = p[1];
  return __popc(a.x ^ left[0]) + __popc(a.y ^ left[1]) + __popc(a.z ^ left[2]) + __popc(a.w ^ left[3]) + __popc(b.x ^ left[4]) +
         __popc(b.y ^ left[5]) + __popc(b.z ^ left[6]) + __popc(b.w ^ left[7]);
}

__device__ inline const uint8_t* levelImage(const StereoArgs& a, const StereoLevel& lv, int o, int frame) {
  return (o == 0 ? a.img0 : a.pyr + lv.imgOff) + (long long)frame * lv.frameStride;
}

}  // namespace

__global__ __launch_bounds__(STEREO_THREADS) void k_stereo_match(const StereoArgs a) {
  __shared__ MatchShared s;
  const int rig = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fL = a.rigs[rig], fR = a.rigs[a.nRigs + rig], cap = a.cap;
  const int nLraw = a.nKps[fL], nRraw = a.nKps[fR];
  const int nL = clampCount(nLraw, cap), nR = clampCount(nRraw, cap);
  const int i0 = blockIdx.y * STEREO_BLOCK;
  const bool first = blockIdx.y == 0;  // the workgroup that flags the rig's counts and its right keypoints
  if (i0 >= nL && !first) return;
  const int rows0 = a.lev[0].rows, nLevels = a.nLevels;
  const orbx_keypoint* keysL = a.kps + (size_t)fL * cap;
  const orbx_keypoint* keysR = a.kps + (size_t)fR * cap;
  const uint8_t* dL = a.desc + (size_t)fL * cap * 32;
  const uint8_t* dR = a.desc + (size_t)fR * cap * 32;
  if (tid < cCount) s.count[tid] = 0;
  if (tid < STEREO_BLOCK) s.best[tid / STEREO_PER_WAVE][tid % STEREO_PER_WAVE] = 0xffffffffu;
  __syncthreads();
  if (first && tid == 0 && (nLraw != nL || nRraw != nR)) atomicOr(&s.count[cStatus], kBadInput);

  for (int c0 = 0; c0 < nR; c0 += STEREO_CHUNK) {
    const int cn = min(STEREO_CHUNK, nR - c0);
    if (c0) __syncthreads();  // (the waves are done with the chunk before)
    for (int j = tid; j < cn; j += STEREO_THREADS) {
      const orbx_keypoint k = keysR[c0 + j];
      Rec r;
      r.x = k.x;
      r.band = 1u;  // minr 1, maxr 0: no row
      r.oct = -4;   // (no left octave is within one of it)
      int bits = 0;
      if (k.octave < 0 || k.octave >= nLevels)
        bits = kBadInput;
      else if (!finite32(k.x) || !finite32(k.y))
        bits = kNonFinite;
      else {
        int minr, maxr;
        rowBand(k.y, a.lev[k.octave].scale, rows0, &minr, &maxr);
        r.band = (uint32_t)(minr & 0xffff) | (uint32_t)maxr << 16;
        r.oct = k.octave;
      }
      if (bits && first) atomicOr(&s.count[cStatus], bits);
      s.rec[j] = r;
    }
    __syncthreads();

    for (int q = 0; q < STEREO_PER_WAVE; q++) {
      const int iL = i0 + wave * STEREO_PER_WAVE + q;
      if (iL >= nL) break;
      const orbx_keypoint k = keysL[iL];  // (uniform over the wave)
      if (k.octave < 0 || k.octave >= nLevels || !finite32(k.x) || !finite32(k.y)) continue;
      const int row = leftRow(k.y, rows0);
      const float maxU = k.x, minU = k.x - a.maxD;
      if (row < 0 || maxU < 0.0f) continue;
      uint32_t left[8];
      for (int w = 0; w < 8; w++) left[w] = ((const uint32_t*)(dL + (size_t)iL * 32))[w];
      uint32_t key = 0xffffffffu;
      int waiting = 0;
      uint16_t* list = s.list[wave];
      for (int j0 = 0; j0 < cn; j0 += 64) {
        const int j = j0 + lane;
        bool pass = false;
        if (j < cn) {
          const Rec r = s.rec[j];
          pass = isCandidate(row, k.octave, minU, maxU, (int)(int16_t)(r.band & 0xffffu), (int)(int16_t)(r.band >> 16), r.oct, r.x);
        }
        const unsigned long long m = __ballot(pass);
        if (m == 0) continue;
        if (pass) list[waiting + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)j;
        waiting += __popcll(m);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (waiting >= 64) {  // a full round: a lane per survivor
          const int iR = c0 + list[lane];
          const uint32_t cand = (uint32_t)hamming(dR + (size_t)iR * 32, left) << 16 | (uint32_t)iR;
          key = cand < key ? cand : key;
          const int rest = waiting - 64;
          const uint16_t moved = lane < rest ? list[64 + lane] : (uint16_t)0;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          if (lane < rest) list[lane] = moved;
          waiting = rest;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
      }
      if (lane < waiting) {
        const int iR = c0 + list[lane];
        const uint32_t cand = (uint32_t)hamming(dR + (size_t)iR * 32, left) << 16 | (uint32_t)iR;
        key = cand < key ? cand : key;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      key = waveMin(key);
      if (lane == 0 && key < s.best[wave][q]) s.best[wave][q] = key;  // (the wave's own word)
    }
  }
  __syncthreads();

  // steps 6-11 for the wave's keypoints, every lane with the same values until the correlation
  for (int q = 0; q < STEREO_PER_WAVE; q++) {
    const int iL = i0 + wave * STEREO_PER_WAVE + q;
    if (iL >= nL) break;
    const size_t at = (size_t)rig * cap + iL;
    const orbx_keypoint k = keysL[iL];
    float uR = -1.0f, depth = -1.0f;
    int matchR = -1, sadBest = -1, bits = 0;
    int cnt = -1;  // the counter this keypoint ends in
    do {
      if (k.octave < 0 || k.octave >= nLevels) { bits = kBadInput; break; }
      if (!finite32(k.x) || !finite32(k.y)) { bits = kNonFinite; break; }
      if (leftRow(k.y, rows0) < 0) { bits = kBadInput; break; }
      if (k.x < 0.0f) break;
      const uint32_t key = s.best[wave][q];
      if (key == 0xffffffffu) break;
      if (lane == 0) atomicAdd(&s.count[cWithCandidates], 1);
      if ((int)(key >> 16) >= kThOrb) break;
      if (lane == 0) atomicAdd(&s.count[cOrbMatched], 1);
      const int iR = (int)(key & 0xffffu), o = k.octave;
      const StereoLevel lv = a.lev[o];
      const float fsu = levelCoord(k.x, lv.invScale), fsv = levelCoord(k.y, lv.invScale), fsu0 = levelCoord(keysR[iR].x, lv.invScale);
      if (windowRefused(fsu0, lv.cols)) { cnt = cWindowRefused; break; }
      if (outOfLevel(fsu, fsv, fsu0, lv.cols, lv.rows)) { cnt = cOutOfLevel; break; }
      const int su = (int)fsu, sv = (int)fsv, su0 = (int)fsu0;
      const uint8_t* IL = levelImage(a, lv, o, fL);
      const uint8_t* IR = levelImage(a, lv, o, fR);
      // lane = 4 row + part: the row's 11 left bytes and the 19 right bytes of its shifts part, part + 4, part + 8
      const int wrow = lane >> 2, part = lane & 3;
      int sum[3] = {0, 0, 0};
      const int lc = IL[(long long)sv * lv.stride + su];
      if (wrow < 2 * kWin + 1) {
        const uint8_t* pl = IL + (long long)(sv - kWin + wrow) * lv.stride + (su - kWin);
        const uint8_t* pr = IR + (long long)(sv - kWin + wrow) * lv.stride + (su0 - kShift - kWin + part);
        const uint8_t* pc = IR + (long long)sv * lv.stride + (su0 - kShift + part);
        int l[2 * kWin + 1], r[2 * kWin + 9];
#pragma unroll
        for (int x = 0; x < 2 * kWin + 1; x++) l[x] = pl[x];
#pragma unroll
        for (int x = 0; x < 2 * kWin + 9; x++) r[x] = (x < 2 * kWin + 5 || part < 3) ? pr[x] : 0;  // (part 3 has two shifts: nothing beyond the strip)
#pragma unroll
        for (int t = 0; t < 3; t++) {
          if (part + 4 * t <= 2 * kShift) {
            const int rc = pc[4 * t];
#pragma unroll
            for (int x = 0; x < 2 * kWin + 1; x++) sum[t] += sadTerm(l[x], lc, r[4 * t + x], rc);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 3; t++)
        for (int m = 4; m <= 32; m <<= 1) sum[t] += __shfl_xor(sum[t], m);
      int sad[2 * kShift + 1];
#pragma unroll
      for (int inc = 0; inc <= 2 * kShift; inc++) sad[inc] = __shfl(sum[inc >> 2], inc & 3);
      int best = 0;
#pragma unroll
      for (int inc = 1; inc <= 2 * kShift; inc++)
        if (sad[inc] < sad[best]) best = inc;
      if (best == 0 || best == 2 * kShift) { cnt = cEdge; break; }
      int s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
      for (int inc = 1; inc < 2 * kShift; inc++)
        if (inc == best) { s1 = sad[inc - 1]; s2 = sad[inc]; s3 = sad[inc + 1]; }
      const float delta = parabolaDelta(s1, s2, s3);
      if (deltaRefused(delta)) { cnt = cDeltaRefused; break; }
      int clamped = 0;
      if (!disparity(k.x, lv.scale, fsu0, best - kShift, delta, a.maxD, a.bf, &uR, &depth, &clamped)) {
        uR = depth = -1.0f;
        cnt = cDisparityRefused;
        break;
      }
      matchR = iR;
      sadBest = s2;
      cnt = cBeforeMedian;
      if (clamped && lane == 0) atomicAdd(&s.count[cClamped], 1);
    } while (false);
    if (lane == 0) {
      if (bits) atomicOr(&s.count[cStatus], bits);
      if (cnt >= 0) atomicAdd(&s.count[cnt], 1);
      a.uRight[at] = uR;
      a.depth[at] = depth;
      a.sad[at] = sadBest;
      if (a.matchRight) a.matchRight[at] = matchR;
    }
  }
  __syncthreads();
  if (tid < cCount && s.count[tid]) {
    int32_t* ws = a.ws + (size_t)rig * STEREO_WS;
    if (tid == cStatus)
      atomicOr(&ws[tid], s.count[tid]);
    else
      atomicAdd(&ws[tid], s.count[tid]);
  }
}

__global__ __launch_bounds__(STEREO_THREADS) void k_stereo_filter(const StereoArgs a) {
  __shared__ int32_t hist[256];
  __shared__ int32_t pick[2];  // the bin that holds the rank, the rank inside it
  __shared__ int32_t removed;
  const int rig = blockIdx.x, tid = threadIdx.x, cap = a.cap;
  const int fL = a.rigs[rig];
  const int n = clampCount(a.nKps[fL], cap);
  const int32_t* ws = a.ws + (size_t)rig * STEREO_WS;
  const int M = ws[cBeforeMedian];
  int32_t* sad = a.sad + (size_t)rig * cap;
  int median = 0;
  if (tid == 0) removed = 0;
  if (M > 0) {
    int rank = M / 2;
    for (int pass = 0; pass < 2; pass++) {
      hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < n; i += STEREO_THREADS) {
        const int v = sad[i];
        if (v >= 0 && (pass == 0 || (v >> 8) == median)) atomicAdd(&hist[pass == 0 ? v >> 8 : v & 255], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int b = 0, below = 0;
        while (b < 255 && below + hist[b] <= rank) below += hist[b++];
        pick[0] = b;
        pick[1] = rank - below;
      }
      __syncthreads();
      median = pass == 0 ? pick[0] : (median << 8 | pick[0]);
      rank = pick[1];
      __syncthreads();
    }
  } else {
    __syncthreads();
  }
  const float thDist = medianThreshold(median);
  float* uRight = a.uRight + (size_t)rig * cap;
  float* depth = a.depth + (size_t)rig * cap;
  const orbx_keypoint* uv = (a.kpsUn ? a.kpsUn : a.kps) + (size_t)fL * cap;
  int gone = 0;
  for (int i = tid; i < n; i += STEREO_THREADS) {
    const int v = sad[i];
    float z = depth[i];
    if (M > 0 && v >= 0 && (float)v >= thDist) {
      gone++;
      uRight[i] = -1.0f;
      depth[i] = z = -1.0f;
      sad[i] = -1;
      if (a.matchRight) a.matchRight[(size_t)rig * cap + i] = -1;
    }
    if (a.points) {
      float p[3] = {0.0f, 0.0f, 0.0f};
      if (z > 0.0f) unproject(uv[i].x, uv[i].y, z, a.cx, a.cy, a.invfx, a.invfy, a.poseWc ? a.poseWc + (size_t)rig * 12 : nullptr, p);
      float* out = a.points + ((size_t)rig * cap + i) * 3;
      out[0] = p[0];
      out[1] = p[1];
      out[2] = p[2];
    }
    if (a.pointMask) a.pointMask[(size_t)rig * cap + i] = z > 0.0f;
  }
  if (gone) atomicAdd(&removed, gone);
  __syncthreads();
  if (tid == 0) {
    orbx_stereo_result r{};
    r.status = ws[cStatus];
    r.n_matches = M - removed;
    r.n_with_candidates = ws[cWithCandidates];
    r.n_orb_matched = ws[cOrbMatched];
    r.n_window_refused = ws[cWindowRefused];
    r.n_out_of_level = ws[cOutOfLevel];
    r.n_edge = ws[cEdge];
    r.n_delta_refused = ws[cDeltaRefused];
    r.n_disparity_refused = ws[cDisparityRefused];
    r.n_clamped = ws[cClamped];
    r.n_before_median = M;
    r.median_sad = median;
    r.th_dist = thDist;
    r.n_removed_by_median = removed;
    a.res[rig] = r;
  }
}

hipError_t launch_stereo(hipStream_t st, const StereoArgs& a) {
  if (a.nRigs <= 0) return hipSuccess;
  const hipError_t e = hipMemsetAsync(a.ws, 0, (size_t)a.nRigs * STEREO_WS * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_stereo_match, dim3((unsigned)a.nRigs, (unsigned)((a.cap + STEREO_BLOCK - 1) / STEREO_BLOCK)), dim3(STEREO_THREADS),
                     0, st, a);
  hipLaunchKernelGGL(k_stereo_filter, dim3((unsigned)a.nRigs), dim3(STEREO_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
