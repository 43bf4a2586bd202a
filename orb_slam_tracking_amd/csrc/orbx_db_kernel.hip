// orbx_db_kernel.hip — DBoW2's TemplatedDatabase on the device (Thirdparty/DBoW2/include/DBoW2/TemplatedDatabase.h:433-464 add,
// :566-1113 query): a CSR inverted file (row_start [words + 1], entry ids u32, values f64, every row in ascending entry id),
// batched add and batched query.
//
//   add    k_db_count       lane per BowVector slot   new postings per word (integer atomics)
//          k_db_scan_tiles  workgroup per 1024 words  row_start of the new file: the scan of old length + new count within a tile,
//          k_db_scan_offsets                          then every tile moved behind the tiles before it
//          k_db_move        lane per old posting      the old rows to their new offsets
//          k_db_scatter     lane per BowVector slot   the batch's postings grouped by word (arrival order within a word)
//          k_db_place       lane per new posting      ... each to its rank by frame within the word's tail: ascending entry id
//   query  k_db_accumulate  workgroup per (query, slice of entry ids)   each wave owns a sub-slice with f64 sums and counters
//                           in LDS and walks the query's words in ascending order; the slice's listed entries sorted by
//                           (sum, entry id), its best max_results written
//          k_db_merge       workgroup per (query, group of lists)       the lists sorted together, the best max_results kept;
//                           the last round applies the final score
//
// No float atomics: an entry's sum is one sequential f64 chain over its common words in ascending word order, from the first
// term (not from 0 +), in the owning wave's program order.  Arithmetic without contraction (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orbx_bow_terms.h"
#include "orbx_launch.h"

namespace orbx {

namespace {

// the BowVector slot of a lane: frame f, index i; false beyond the batch, the frame's count or the vocabulary's words (a word id
// that is no word is skipped, never indexed with)
__device__ __forceinline__ bool addSlot(const DbAddArgs& a, int* f, uint32_t* w, size_t* o) {
  const long long g = (long long)blockIdx.x * DB_THREADS + threadIdx.x;
  *f = (int)(g / a.cap);
  const int i = (int)(g - (long long)*f * a.cap);
  if (*f >= a.nFrames || i >= clampN(a.n, *f, a.cap)) return false;
  *o = (size_t)*f * a.cap + i;
  *w = a.word[*o];
  return *w < a.nWords;
}

}  // namespace

__global__ __launch_bounds__(DB_THREADS) void k_db_count(DbAddArgs a) {
  int f;
  uint32_t w;
  size_t o;
  if (addSlot(a, &f, &w, &o)) atomicAdd(&a.cnt[w], 1u);
}

// the scan of old length + new count over the words, in tiles of DB_SCAN_THREADS words: every tile scanned on its own ...
__global__ __launch_bounds__(DB_SCAN_THREADS) void k_db_scan_tiles(DbAddArgs a, uint32_t* tileSum) {
  __shared__ uint32_t scan[DB_SCAN_THREADS];
  const uint32_t t = threadIdx.x, w = blockIdx.x * DB_SCAN_THREADS + t;
  const uint32_t len = w < a.nWords ? a.oldRow[w + 1] - a.oldRow[w] + a.cnt[w] : 0;
  scan[t] = len;
  __syncthreads();
  for (uint32_t d = 1; d < DB_SCAN_THREADS; d <<= 1) {
    const uint32_t add = t >= d ? scan[t - d] : 0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  if (w < a.nWords) a.newRow[w] = scan[t] - len;
  if (t == DB_SCAN_THREADS - 1) tileSum[blockIdx.x] = scan[t];
}

// ... then moved behind the tiles before it; the last tile ends the file (newRow[nWords], the file's new length)
__global__ __launch_bounds__(DB_SCAN_THREADS) void k_db_scan_offsets(DbAddArgs a, const uint32_t* tileSum) {
  __shared__ uint32_t red[DB_SCAN_THREADS];
  const uint32_t t = threadIdx.x, w = blockIdx.x * DB_SCAN_THREADS + t;
  uint32_t sum = 0;
  for (uint32_t i = t; i < blockIdx.x; i += DB_SCAN_THREADS) sum += tileSum[i];
  red[t] = sum;
  __syncthreads();
  for (uint32_t d = DB_SCAN_THREADS / 2; d > 0; d >>= 1) {
    if (t < d) red[t] += red[t + d];
    __syncthreads();
  }
  const uint32_t off = red[0];
  if (w < a.nWords) a.newRow[w] += off;
  if (blockIdx.x == gridDim.x - 1 && t == 0) a.newRow[a.nWords] = off + tileSum[blockIdx.x];
}

__global__ __launch_bounds__(DB_THREADS) void k_db_move(DbAddArgs a) {
  const uint32_t p = blockIdx.x * DB_THREADS + threadIdx.x;
  if (p >= a.oldTotal) return;
  uint32_t lo = 0, hi = a.nWords;  // the posting's word: the last w with oldRow[w] <= p (the rows before it that are empty start there too)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.oldRow[mid] <= p) lo = mid;
    else hi = mid;
  }
  const uint32_t dst = a.newRow[lo] + (p - a.oldRow[lo]);
  a.newEntry[dst] = a.oldEntry[p];
  a.newValue[dst] = a.oldValue[p];
}

__global__ __launch_bounds__(DB_THREADS) void k_db_scatter(DbAddArgs a) {
  int f;
  uint32_t w;
  size_t o;
  if (!addSlot(a, &f, &w, &o)) return;
  const uint32_t slot = atomicSub(&a.cnt[w], 1u) - 1u;        // in [0, the word's new postings)
  const uint32_t t = a.newRow[w] - a.oldRow[w] + slot;        // the new postings of the words before w, then the slot
  a.tmpWord[t] = w;
  a.tmpFrame[t] = (uint32_t)f;
  a.tmpValue[t] = a.value[o];
}

// posting j of the grouped batch goes behind its word's old row, at its rank by frame among the word's new postings (a frame
// that names a word twice, which transform never writes, keeps both postings: equal frames rank by position)
__global__ __launch_bounds__(DB_THREADS) void k_db_place(DbAddArgs a, uint32_t nNew) {
  const uint32_t j = blockIdx.x * DB_THREADS + threadIdx.x;
  if (j >= nNew) return;
  const uint32_t w = a.tmpWord[j], f = a.tmpFrame[j];
  const uint32_t t0 = a.newRow[w] - a.oldRow[w], t1 = a.newRow[w + 1] - a.oldRow[w + 1];
  uint32_t rank = 0;
  for (uint32_t k = t0; k < t1; k++) {
    const uint32_t fk = a.tmpFrame[k];
    rank += fk < f || (fk == f && k < j);
  }
  const uint32_t dst = a.newRow[w] + (a.oldRow[w + 1] - a.oldRow[w]) + rank;
  a.newEntry[dst] = a.firstId + f;
  a.newValue[dst] = a.tmpValue[j];
}

namespace {

// A sum as a key that sorts best first in ascending order: the f64 order (-0 and +0 equal), inverted for the scorings whose
// best is the largest.  Equal keys are ordered by the tag behind them (the entry id: deviation 1 of the database).
__device__ __forceinline__ uint64_t dbKey(double raw, int descending) {
  if (raw == 0.0) raw = 0.0;  // -0 -> +0
  const uint64_t b = (uint64_t)__double_as_longlong(raw);
  const uint64_t k = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  return descending ? ~k : k;
}

// ascending bitonic sort of the pairs (key, tag)[0, P) in LDS, P a power of two; every thread of the workgroup takes part
__device__ void dbSort(uint64_t* key, uint64_t* tag, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += DB_THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t kx = key[i], ky = key[ixj], tx = tag[i], ty = tag[ixj];
          const bool gt = kx > ky || (kx == ky && tx > ty);
          if (gt == ((i & k) == 0)) {
            key[i] = ky;
            key[ixj] = kx;
            tag[i] = ty;
            tag[ixj] = tx;
          }
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace

__global__ __launch_bounds__(DB_THREADS) void k_db_accumulate(DbQueryArgs a) {
  __shared__ double acc[DB_SLICE_MAX];
  __shared__ uint64_t key[DB_SLICE_MAX];
  __shared__ uint64_t tag[DB_SLICE_MAX];
  __shared__ uint32_t cnt[DB_SLICE_MAX];
  __shared__ int sListed;
  const int q = blockIdx.x / a.nSlices, sl = blockIdx.x - q * a.nSlices;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int lo = sl * a.perSlice, hi = min(lo + a.perSlice, a.limit), S = hi - lo;  // (nSlices covers [0, limit): S >= 1)
  for (int i = t; i < S; i += DB_THREADS) cnt[i] = 0;
  if (t == 0) sListed = 0;
  __syncthreads();

  const int sub = (a.perSlice + DB_WAVES - 1) / DB_WAVES;
  const int wlo = lo + wave * sub, whi = min(wlo + sub, hi);  // this wave's entries: nobody else touches their acc / cnt
  if (wlo < whi) {
    const int n = clampN(a.n, q, a.cap);
    const uint32_t* qw = a.word + (size_t)q * a.cap;
    const double* qv = a.value + (size_t)q * a.cap;
    for (int b = 0; b < n; b += 64) {
      // the next 64 words together: lane i finds the part [s, e) of its word's row that lies in the wave's entries
      const int i = b + lane;
      uint32_t s = 0, e = 0;
      double v = 0.0;
      if (i < n) {
        const uint32_t w = qw[i];
        if (w < a.nWords) {
          v = qv[i];
          const uint32_t r1 = a.row[w + 1];
          uint32_t l = a.row[w], h = r1;
          while (l < h) {  // rows ascend in entry id: the first posting >= wlo
            const uint32_t mid = l + (h - l) / 2;
            if (a.entry[mid] < (uint32_t)wlo) l = mid + 1;
            else h = mid;
          }
          s = l;
          h = min(r1, s + (uint32_t)(whi - wlo));  // an entry appears once per row: at most whi - wlo postings follow
          while (l < h) {
            const uint32_t mid = l + (h - l) / 2;
            if (a.entry[mid] < (uint32_t)whi) l = mid + 1;
            else h = mid;
          }
          e = l;
        }
      }
      // ... then word by word in ascending order; within a word the lanes meet at different entries
      for (uint64_t mask = __ballot(e > s); mask; mask &= mask - 1) {
        const int j = __builtin_ctzll(mask);
        const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)s, j), ej = (uint32_t)__builtin_amdgcn_readlane((int)e, j);
        const double qj = readlaneF64(v, j);
        for (uint32_t p = sj + lane; p < ej; p += 64) {
          const uint32_t k = a.entry[p] - (uint32_t)lo;
          const double term = bowTerm(a.scoring, a.binary, qj, a.pvalue[p]);
          const uint32_t c = cnt[k];
          acc[k] = c ? acc[k] + term : term;  // the chain starts from the first term
          cnt[k] = c + 1;
        }
        // the next word's lanes read what these wrote: the wave's own program order, kept by the compiler behind this fence
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  __syncthreads();

  int P = 1;
  while (P < S) P <<= 1;
  int mine = 0;
  for (int i = t; i < P; i += DB_THREADS) {
    const bool listed = i < S && cnt[i] >= (uint32_t)a.minCommon;
    key[i] = listed ? dbKey(acc[i], a.descending) : ~0ull;
    tag[i] = listed ? (uint64_t)i : ~0ull;  // (entry id - lo: the same order)
    mine += listed;
  }
  if (mine) atomicAdd(&sListed, mine);
  __syncthreads();
  const int m = min(sListed, a.maxResults);
  if (sListed > 0) dbSort(key, tag, P);
  const size_t list = (size_t)q * a.nSlices + sl;
  for (int i = t; i < m; i += DB_THREADS) {
    const uint32_t k = (uint32_t)tag[i];
    a.listRaw[list * a.maxResults + i] = acc[k];
    a.listId[list * a.maxResults + i] = (uint32_t)lo + k;
  }
  if (t == 0) a.listN[list] = m;
}

__global__ __launch_bounds__(DB_THREADS) void k_db_merge(DbMergeArgs a) {
  __shared__ double raw[DB_SLICE_MAX];
  __shared__ uint64_t key[DB_SLICE_MAX];
  __shared__ uint64_t tag[DB_SLICE_MAX];
  __shared__ int sTotal;
  const int q = blockIdx.x / a.nOut, o = blockIdx.x - q * a.nOut, t = threadIdx.x;
  const int l0 = o * a.perMerge, nl = min(a.perMerge, a.nIn - l0), R = a.maxResults;
  const size_t in = (size_t)q * a.nIn + l0;
  if (t == 0) sTotal = 0;
  __syncthreads();
  int P = 1;
  while (P < nl * R) P <<= 1;  // <= DB_MERGE_MAX * DB_MAX_RESULTS
  int mine = 0;
  for (int x = t; x < P; x += DB_THREADS) {
    const int l = x / R, i = x - l * R;
    const bool have = l < nl && i < a.inN[in + l];
    uint64_t k = ~0ull, g = ~0ull;
    if (have) {
      const double r = a.inRaw[(in + l) * R + i];
      raw[x] = r;
      k = dbKey(r, a.descending);
      g = ((uint64_t)a.inId[(in + l) * R + i] << 32) | (uint32_t)x;  // the entry id orders equal keys; x finds the sum again
    }
    key[x] = k;
    tag[x] = g;
    mine += have;
  }
  if (mine) atomicAdd(&sTotal, mine);
  __syncthreads();
  const int m = min(sTotal, R);
  if (sTotal > 0) dbSort(key, tag, P);
  if (a.nOut == 1 && a.resN) {
    for (int i = t; i < m; i += DB_THREADS) {
      a.resEntry[(size_t)q * R + i] = (int32_t)(tag[i] >> 32);
      a.resScore[(size_t)q * R + i] = dbFinalScore(a.scoring, raw[(uint32_t)tag[i]]);
    }
    if (t == 0) a.resN[q] = m;
  } else {
    const size_t out = (size_t)q * a.nOut + o;
    for (int i = t; i < m; i += DB_THREADS) {
      a.outRaw[out * R + i] = raw[(uint32_t)tag[i]];
      a.outId[out * R + i] = (uint32_t)(tag[i] >> 32);
    }
    if (t == 0) a.outN[out] = m;
  }
}

namespace {
inline unsigned dbBlocks(long long lanes) { return (unsigned)((lanes + DB_THREADS - 1) / DB_THREADS); }
}  // namespace

// the new file's row starts from the old file and the batch (a.cnt zero on entry); the file's new length is newRow[nWords]
// (tileSum: one u32 per tile of DB_SCAN_THREADS words; nWords >= 1)
hipError_t launch_db_add_count(hipStream_t st, const DbAddArgs& a, uint32_t* tileSum) {
  hipLaunchKernelGGL(k_db_count, dim3(dbBlocks((long long)a.nFrames * a.cap)), dim3(DB_THREADS), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned tiles = (a.nWords + DB_SCAN_THREADS - 1) / DB_SCAN_THREADS;
  hipLaunchKernelGGL(k_db_scan_tiles, dim3(tiles), dim3(DB_SCAN_THREADS), 0, st, a, tileSum);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_db_scan_offsets, dim3(tiles), dim3(DB_SCAN_THREADS), 0, st, a, (const uint32_t*)tileSum);
  return hipGetLastError();
}

// the old rows moved and the batch's nNew postings placed behind them
hipError_t launch_db_add_fill(hipStream_t st, const DbAddArgs& a, uint32_t nNew) {
  hipError_t e = hipSuccess;
  if (a.oldTotal) {
    hipLaunchKernelGGL(k_db_move, dim3(dbBlocks(a.oldTotal)), dim3(DB_THREADS), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (nNew) {
    hipLaunchKernelGGL(k_db_scatter, dim3(dbBlocks((long long)a.nFrames * a.cap)), dim3(DB_THREADS), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_db_place, dim3(dbBlocks(nNew)), dim3(DB_THREADS), 0, st, a, nNew);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_db_accumulate(hipStream_t st, const DbQueryArgs& a) {
  hipLaunchKernelGGL(k_db_accumulate, dim3((unsigned)a.nQueries * a.nSlices), dim3(DB_THREADS), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_db_merge(hipStream_t st, const DbMergeArgs& a) {
  hipLaunchKernelGGL(k_db_merge, dim3((unsigned)a.nQueries * a.nOut), dim3(DB_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace orbx
