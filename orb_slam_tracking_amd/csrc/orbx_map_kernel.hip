// orbx_map_kernel.hip — the map points behind a local bundle adjustment (include/orbx.h, "local mapping: updating the map
// points"): vToErase applied to the rows, MapPoint::Observations(), UpdateNormalAndDepth and ComputeDistinctiveDescriptors for
// the points of a batch of local windows, written where the matchers read them.
//
//   k_map_build    workgroup (512 lanes) per problem          the checks of the device data; the inverse of the rows in the
//                                                             workspace (per point a slot per entry, claimed by an integer
//                                                             compare-and-swap, so two features of one keyframe on one point
//                                                             show); per point its observers in ascending entry, their count,
//                                                             the bad flag, the reference keyframe, every len; then, for a
//                                                             problem without a flag only, the writes: rows, mask, counts,
//                                                             reference frames, the record
//   k_map_points   grid (problems x chunks of 64 points),      a wave per point, lane a = observer a: the descriptors gathered
//                  4 waves per workgroup                      into LDS, the lane's row of Hamming distances, its median by
//                                                             selection on counts (nine halving steps over [0, 256]), the
//                                                             wave's smallest (median, a); the normal summed in observer
//                                                             order through lane broadcasts, the distances of the reference
//
// The float arithmetic is csrc/orbx_map_math.inc over orbx_tri_math.inc, shared with the CPU restatement.  Up to 64 observers a
// lane keeps its row of distances in LDS ([other][lane], 2 bytes each); beyond, lane l owns observers l, l + 64, ... and
// recomputes a distance whenever it needs it: both give the same bytes.  A flagged problem leaves its status in the workspace
// and k_map_points returns at once for it.  f32 without contraction (-ffp-contract=off); integer atomics only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/orbx.h"
#include "orbx_launch.h"

#define ORBX_TRI_FN __device__
#include "orbx_tri_math.inc"
#include "orbx_map_math.inc"

namespace orbx {
using namespace orbx_map;

namespace {

struct BuildShared {
  int status, nPoints, nObs, nErased, nBad, nCleared, nRefMoved, maxObs;
};

// a word other lanes of the workgroup change with atomics: read where they land
__device__ int ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the lanes' status bits gathered: every lane gets the union
__device__ int gather(BuildShared& s, int bits) {
  if (bits) atomicOr(&s.status, bits);
  __syncthreads();
  return s.status;
}

struct Problem {
  int first, nE, nF, set, mapN;
  MapWork w;
  const int32_t* frameOf;
};
__device__ Problem problemOf(const MapArgs& a, int p) {
  Problem q;
  const int P = a.nProblems;
  q.first = a.problems[p];
  q.nE = a.problems[P + p];
  q.nF = a.problems[2 * P + p];
  q.set = a.problems[3 * P + p];
  mapWorkLayout(a.mapCap, q.nE, (uintptr_t)(a.ws + (size_t)a.problems[4 * P + p] * 256), &q.w);
  q.mapN = a.mapN[q.set];
  q.frameOf = a.entryFrame + q.first;
  return q;
}

__global__ __launch_bounds__(MAP_THREADS) void k_map_build(const MapArgs a) {
  __shared__ BuildShared s;
  const int p = blockIdx.x, tid = threadIdx.x;
  const Problem q = problemOf(a, p);
  const MapWork& w = q.w;
  const int nE = q.nE, mapN = q.mapN, cap = a.cap;
  int32_t* rows = a.rows + (size_t)q.first * cap;
  const uint8_t* outlier = a.outlier ? a.outlier + (size_t)q.first * cap : nullptr;
  const float* pose = a.entryPose + (size_t)q.first * 12;
  const size_t setAt = (size_t)q.set * a.mapCap;
  const float* mapPts = a.mapPts + setAt * 3;
  const uint8_t* mask = a.mapMask ? a.mapMask + setAt : nullptr;
  int32_t* mapRef = a.mapRef ? a.mapRef + setAt : nullptr;

  if (tid == 0) {
    s.status = (mapN < 0 || mapN > a.mapCap) ? ST_BAD : 0;
    s.nPoints = s.nObs = s.nErased = s.nBad = s.nCleared = s.nRefMoved = s.maxObs = 0;
  }
  __syncthreads();
  int status = s.status;

  // ---- the entries: counts inside the capacity, no frame twice, finite poses; the camera centres ----
  if (!status) {
    int bits = 0;
    for (int e = tid; e < nE; e += MAP_THREADS) {
      const int f = q.frameOf[e], n = a.nKps[f];
      if (n < 0 || n > cap) bits |= ST_BAD;
      for (int e2 = 0; e2 < e; e2++)
        if (q.frameOf[e2] == f) bits |= ST_BAD;
      bool fin = true;
      for (int c = 0; c < 12; c++) fin = fin && orbx_tri::isFinite(pose[(size_t)e * 12 + c]);
      if (!fin)
        bits |= ST_NONFINITE;
      else
        orbx_tri::cameraCentre(pose + (size_t)e * 12, w.ow + (size_t)e * 3);
    }
    status = gather(s, bits);
  }
  // ---- the vertices: named by a free entry, below map_n, mask byte set ----
  if (!status) {
    for (int m = tid; m < mapN; m += MAP_THREADS) {
      w.state[m] = 0;
      w.cnt[m] = 0;
    }
    for (size_t k = tid; k < (size_t)mapN * nE; k += MAP_THREADS) w.slot[k] = -1;
    __syncthreads();
    int bits = 0;
    for (int e = 0; e < nE; e++) {
      const int n = a.nKps[q.frameOf[e]];
      for (int f = tid; f < n; f += MAP_THREADS) {
        const int r = rows[(size_t)e * cap + f];
        if (r >= mapN)
          bits |= ST_BAD;
        else if (r >= 0 && e < q.nF && (!mask || mask[r] != 0))
          atomicOr(&w.state[r], PT_VERTEX);
      }
    }
    status = gather(s, bits);
  }
  // ---- the inverse of the rows: a slot per (vertex, entry); the erasures marked, not yet applied ----
  if (!status) {
    int bits = 0;
    for (int e = 0; e < nE; e++) {
      const int n = a.nKps[q.frameOf[e]];
      for (int f = tid; f < n; f += MAP_THREADS) {
        const int r = rows[(size_t)e * cap + f];
        if (r < 0 || !(ld(&w.state[r]) & PT_VERTEX)) continue;
        const bool erased = outlier && outlier[(size_t)e * cap + f] != 0;
        if (atomicCAS(&w.slot[(size_t)r * nE + e], -1, erased ? (f | SLOT_ERASED) : f) != -1) bits |= ST_BAD;
        if (erased) atomicOr(&w.state[r], PT_LOST);
      }
    }
    status = gather(s, bits);
  }
  // ---- per vertex: its observers in ascending entry, the bad flag, the reference keyframe, every len ----
  if (!status) {
    int bits = 0, nPoints = 0, nObs = 0, nBad = 0, nMoved = 0, maxObs = 0;
    for (int m = tid; m < mapN; m += MAP_THREADS) {
      const int st = ld(&w.state[m]);
      if (!(st & PT_VERTEX)) continue;
      nPoints++;
      const float* X = mapPts + (size_t)m * 3;
      if (!finite3(X)) {
        bits |= ST_NONFINITE;
        continue;
      }
      const int32_t* slot = w.slot + (size_t)m * nE;
      int32_t* list = w.list + (size_t)m * nE;
      const int refFrame = mapRef ? mapRef[m] : -1;
      int n = 0, refE = -1, firstE = -1;
      for (int e = 0; e < nE; e++) {
        const int sl = ld(&slot[e]);
        if (sl < 0 || (sl & SLOT_ERASED)) continue;
        if (n == 0) firstE = e;
        list[n++] = e;
        if (refFrame >= 0 && q.frameOf[e] == refFrame) refE = e;
      }
      w.cnt[m] = n;
      maxObs = n > maxObs ? n : maxObs;
      if (((st & PT_LOST) && n <= 2) || n == 0) {
        w.state[m] = st | PT_BAD;
        nBad++;
        continue;
      }
      if (refE < 0) refE = firstE;  // no reference yet, or it is gone: the first observer
      w.refEnt[m] = refE;
      const int fr = q.frameOf[refE];
      const int oct = a.kps[(size_t)fr * cap + ld(&slot[refE])].octave;
      if (oct < 0 || oct >= a.nLevels) bits |= ST_BAD;
      for (int k = 0; k < n; k++) {
        float t[3];
        if (!normalTerm(X, w.ow + (size_t)list[k] * 3, t)) bits |= ST_NONFINITE;
      }
      nObs += n;
      if (refFrame >= 0 && fr != refFrame) nMoved++;
    }
    if (nPoints) atomicAdd(&s.nPoints, nPoints);
    if (nObs) atomicAdd(&s.nObs, nObs);
    if (nBad) atomicAdd(&s.nBad, nBad);
    if (nMoved) atomicAdd(&s.nRefMoved, nMoved);
    if (maxObs) atomicMax(&s.maxObs, maxObs);
    status = gather(s, bits);
  }
  if (tid == 0) *w.flag = status;
  orbx_map_result* out = a.res + p;
  if (status) {  // flagged: nothing of the caller's is touched but the record
    if (tid == 0) {
      orbx_map_result r{};
      r.status = status;
      *out = r;
    }
    return;
  }

  // ---- the writes ----
  int nErased = 0, nCleared = 0;
  for (int e = 0; e < nE; e++) {
    const int n = a.nKps[q.frameOf[e]];
    for (int f = tid; f < n; f += MAP_THREADS) {
      const int r = rows[(size_t)e * cap + f];
      if (r < 0) continue;
      const int st = ld(&w.state[r]);
      if (!(st & PT_VERTEX)) continue;
      if (outlier && outlier[(size_t)e * cap + f] != 0) {
        rows[(size_t)e * cap + f] = -1;
        nErased++;
      } else if (st & PT_BAD) {
        rows[(size_t)e * cap + f] = -1;
        nCleared++;
      }
    }
  }
  if (nErased) atomicAdd(&s.nErased, nErased);
  if (nCleared) atomicAdd(&s.nCleared, nCleared);
  uint8_t* maskOut = a.mapMaskOut + setAt;
  int32_t* mapObs = a.mapObs + setAt;
  for (int m = tid; m < mapN; m += MAP_THREADS) {
    const int st = w.state[m];
    if (!(st & PT_VERTEX)) continue;
    if (st & PT_BAD) {
      maskOut[m] = 0;
      mapObs[m] = 0;
      continue;
    }
    maskOut[m] = mask ? mask[m] : (uint8_t)1;
    mapObs[m] = w.cnt[m];
    if (mapRef) {
      const int fr = q.frameOf[w.refEnt[m]];
      if (mapRef[m] != fr) mapRef[m] = fr;
    }
  }
  __syncthreads();
  if (tid == 0) {
    orbx_map_result r{};
    r.status = 0;
    r.n_points = s.nPoints;
    r.n_observations = s.nObs;
    r.n_erased = s.nErased;
    r.n_bad_points = s.nBad;
    r.n_cleared = s.nCleared;
    r.n_ref_moved = s.nRefMoved;
    r.max_observers = s.maxObs;
    r.n_free = q.nF;
    *out = r;
  }
}

__device__ int hamming(const uint32_t* x, const uint32_t* y) {
  int d = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) d += __popc(x[k] ^ y[k]);
  return d;
}

__global__ __launch_bounds__(MAP_WAVES * 64) void k_map_points(const MapArgs a) {
  __shared__ uint32_t ldsDesc[MAP_WAVES][64][8];     // the first 64 observers' descriptors
  __shared__ uint16_t ldsDist[MAP_WAVES][64][64];    // [other][lane]: the lane's row of distances, up to 64 observers
  const int chunks = (a.mapCap + MAP_CHUNK - 1) / MAP_CHUNK;
  const int p = blockIdx.x / chunks, chunk = blockIdx.x % chunks, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Problem q = problemOf(a, p);
  const MapWork& w = q.w;
  if (*w.flag) return;
  const int nE = q.nE, mapN = q.mapN, cap = a.cap;
  const size_t setAt = (size_t)q.set * a.mapCap;
  const float* mapPts = a.mapPts + setAt * 3;

  for (int i = wave; i < MAP_CHUNK; i += MAP_WAVES) {
    const int m = chunk * MAP_CHUNK + i;
    if (m >= mapN) break;
    const int st = w.state[m];
    if (!(st & PT_VERTEX) || (st & PT_BAD)) continue;
    const int N = w.cnt[m];
    const int32_t* list = w.list + (size_t)m * nE;
    const int32_t* slot = w.slot + (size_t)m * nE;
    // observer b's descriptor in global memory
    auto descOf = [&](int b) {
      const int e = list[b];
      return reinterpret_cast<const uint32_t*>(a.desc + ((size_t)q.frameOf[e] * cap + slot[e]) * 32);
    };

    if (a.what & WHAT_DESCRIPTORS) {
      if (lane < N) {
        const uint32_t* src = descOf(lane);
#pragma unroll
        for (int k = 0; k < 8; k++) ldsDesc[wave][lane][k] = src[k];
      }
      __builtin_amdgcn_wave_barrier();
      const int need = (N - 1) / 2 + 1;  // the median is the smallest v with at least `need` of the row <= v
      unsigned long long best = ~0ull;
      if (N <= 64) {
        uint32_t mine[8];
#pragma unroll
        for (int k = 0; k < 8; k++) mine[k] = ldsDesc[wave][lane < N ? lane : 0][k];
        for (int b = 0; b < N; b++) ldsDist[wave][b][lane] = (uint16_t)hamming(mine, ldsDesc[wave][b]);
        __builtin_amdgcn_wave_barrier();
        int lo = 0, hi = 256;
        for (int step = 0; step < 9; step++) {
          const int mid = (lo + hi) >> 1;
          int c = 0;
          for (int b = 0; b < N; b++) c += (int)ldsDist[wave][b][lane] <= mid ? 1 : 0;
          if (c >= need)
            hi = mid;
          else
            lo = mid + 1;
        }
        if (lane < N) best = ((unsigned long long)lo << 32) | (unsigned)lane;
      } else {
        for (int a0 = 0; a0 < N; a0 += 64) {
          const int aa = a0 + lane;
          uint32_t mine[8];
          const uint32_t* src = descOf(aa < N ? aa : 0);
#pragma unroll
          for (int k = 0; k < 8; k++) mine[k] = src[k];
          int lo = 0, hi = 256;
          for (int step = 0; step < 9; step++) {
            const int mid = (lo + hi) >> 1;
            int c = 0;
            for (int b = 0; b < N; b++) {
              uint32_t other[8];
              const uint32_t* o = b < 64 ? ldsDesc[wave][b] : descOf(b);
#pragma unroll
              for (int k = 0; k < 8; k++) other[k] = o[k];
              c += hamming(mine, other) <= mid ? 1 : 0;
            }
            if (c >= need)
              hi = mid;
            else
              lo = mid + 1;
          }
          const unsigned long long key = ((unsigned long long)lo << 32) | (unsigned)aa;
          if (aa < N && key < best) best = key;
        }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o < best ? o : best;
      }
      const int win = (int)(best & 0xffffffffull);
      if (lane < 8) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(a.mapDesc + (setAt + m) * 32);
        dst[lane] = win < 64 ? ldsDesc[wave][win][lane] : descOf(win)[lane];
      }
      __builtin_amdgcn_wave_barrier();
    }

    if (a.what & WHAT_NORMALS) {
      const float X[3] = {mapPts[(size_t)m * 3], mapPts[(size_t)m * 3 + 1], mapPts[(size_t)m * 3 + 2]};
      float sum[3] = {0.0f, 0.0f, 0.0f};
      for (int a0 = 0; a0 < N; a0 += 64) {
        const int aa = a0 + lane;
        float t[3] = {0.0f, 0.0f, 0.0f};
        if (aa < N) normalTerm(X, w.ow + (size_t)list[aa] * 3, t);
        const int here = N - a0 < 64 ? N - a0 : 64;
        for (int k = 0; k < here; k++) {  // ascending observer, every lane the same sum
          const float tk[3] = {__shfl(t[0], k, 64), __shfl(t[1], k, 64), __shfl(t[2], k, 64)};
          normalAdd(sum, tk);
        }
      }
      if (lane == 0) {
        float nrm[3], mm[2];
        normalFinish(sum, N, nrm);
        const int refE = w.refEnt[m];
        const int oct = a.kps[(size_t)q.frameOf[refE] * cap + slot[refE]].octave;
        distances(X, w.ow + (size_t)refE * 3, a.scale[oct], a.scale[a.nLevels - 1], mm);
        float* dn = a.mapNormals + (setAt + m) * 3;
        dn[0] = nrm[0];
        dn[1] = nrm[1];
        dn[2] = nrm[2];
        float* dd = a.mapDist + (setAt + m) * 2;
        dd[0] = mm[0];
        dd[1] = mm[1];
      }
    }
  }
}

}  // namespace

hipError_t launch_map_update(hipStream_t st, const MapArgs& a) {
  hipLaunchKernelGGL(k_map_build, dim3(a.nProblems), dim3(MAP_THREADS), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.what == 0) return e;
  hipLaunchKernelGGL(k_map_points, dim3((unsigned)((a.mapCap + MAP_CHUNK - 1) / MAP_CHUNK) * (unsigned)a.nProblems), dim3(MAP_WAVES * 64), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
