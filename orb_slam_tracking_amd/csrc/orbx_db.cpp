// orbx_db.cpp — host side of the database (include/orbx.h, "database"): DBoW2's TemplatedDatabase (TemplatedDatabase.h:433-464,
// :566-1113) as a CSR inverted file on the device, its argument checks, the two copies of the file an add moves between, and the
// C entry points.  The kernels are in orbx_db_kernel.hip.  Device memory is owned through orbx_buf.h's types only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>

#include "orbx_host.h"

using namespace orbx;

static_assert(ORBX_DB_MAX_RESULTS == DB_MAX_RESULTS, "orbx.h and orbx_device.h");

struct orbx_database {
  orbx_ctx* ctx = nullptr;
  int device = 0;
  int nWords = 0, scoring = 0, weighting = 0;
  int nEntries = 0;
  uint32_t nPost = 0;
  int cur = 0;  // the copy that holds the file; an add writes the other one, then they change places
  DeviceBuf<uint32_t> dRow[2];    // [nWords + 1]
  DeviceBuf<uint32_t> dEntry[2];  // [postings]
  DeviceBuf<double> dValue[2];
  DeviceBuf<uint32_t> dCnt;       // [nWords]
  DeviceBuf<uint32_t> dTiles;     // the scan's sum per tile of DB_SCAN_THREADS words
  DeviceBuf<uint32_t> dTmp;       // an add's grouped postings: words, frames [2][new postings]
  DeviceBuf<double> dTmpValue;
  DeviceBuf<uint8_t> dLists;      // a query's lists between its kernels
  DeviceBuf<uint8_t> dIo;         // staging of orbx_database_add / orbx_database_query
};

namespace {

// orbx_debug_database_shape
std::atomic<int> g_perSlice{DB_SLICE_MAX}, g_perMerge{DB_MERGE_MAX};

// the checks every entry point with a context and a database shares; ctx == NULL: no device
int checkDb(orbx_ctx* ctx, const orbx_database* db) {
  if (!db) return ORBX_E_BADARG;
  if (!ctx) return ORBX_E_HIP;
  if (db->ctx != ctx) {
    ctxSetError(ctx, "the database belongs to another context");
    return ORBX_E_BADARG;
  }
  return ORBX_OK;
}

int checkBatch(orbx_ctx* ctx, int n, const void* w, const void* v, const void* cnt, int capacity) {
  if (n < 0 || capacity < 1 || !w || !v || !cnt) return ORBX_E_BADARG;
  if (capacity > ORBX_BOW_MAX_FEATURES) {
    if (ctx) ctxSetError(ctx, "database: capacity above ORBX_BOW_MAX_FEATURES");
    return ORBX_E_CAPACITY;
  }
  return ORBX_OK;
}

// deviation 5: a host BowVector's words are strictly ascending word ids of the vocabulary
int checkVector(orbx_ctx* ctx, const orbx_database* db, const uint32_t* word, const double* value, int n) {
  if (n < 0 || (n > 0 && (!word || !value))) return ORBX_E_BADARG;
  if (n > ORBX_BOW_MAX_FEATURES) return ORBX_E_CAPACITY;
  for (int i = 0; i < n; i++)
    if (word[i] >= (uint32_t)db->nWords || (i > 0 && word[i] <= word[i - 1])) {
      ctxSetError(ctx, "database: a word id outside the vocabulary, or words not strictly ascending");
      return ORBX_E_BADARG;
    }
  return ORBX_OK;
}

void freeDb(orbx_database* db) {
  if (hipSetDevice(db->device) == hipSuccess) delete db;
}

}  // namespace

extern "C" {

int orbx_debug_database_shape(int entries_per_slice, int lists_per_merge) {
  if (entries_per_slice > DB_SLICE_MAX || entries_per_slice == 0 || lists_per_merge > DB_MERGE_MAX ||
      (lists_per_merge >= 0 && lists_per_merge < 2))
    return ORBX_E_BADARG;
  g_perSlice.store(entries_per_slice < 0 ? DB_SLICE_MAX : entries_per_slice);
  g_perMerge.store(lists_per_merge < 0 ? DB_MERGE_MAX : lists_per_merge);
  return ORBX_OK;
}

int orbx_database_create(orbx_ctx* ctx, const orbx_vocabulary* voc, orbx_database** out) {
  if (!out) return ORBX_E_BADARG;
  *out = nullptr;
  if (!voc) return ORBX_E_BADARG;
  if (!ctx) return ORBX_E_HIP;  // no device context
  if (vocCtx(voc) != ctx) {
    ctxSetError(ctx, "the vocabulary belongs to another context");
    return ORBX_E_BADARG;
  }
  int32_t info[6];
  orbx_vocabulary_info(voc, info);
  if (info[2] == ORBX_BOW_KL) {
    ctxSetError(ctx, "database: KL scoring is not offered");
    return ORBX_E_BADARG;
  }
  int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  orbx_database* db = new orbx_database();
  db->ctx = ctx;
  db->device = ctxDevice(ctx);
  db->scoring = info[2];
  db->weighting = info[3];
  db->nWords = info[5];
  auto body = [&]() -> int {
    const size_t rows = ((size_t)db->nWords + 1) * 4;
    for (int i = 0; i < 2; i++) HIPCHK(db->dRow[i].grow(rows));
    HIPCHK(db->dCnt.grow(rows));
    HIPCHK(db->dTiles.grow(((size_t)db->nWords / DB_SCAN_THREADS + 1) * 4));
    HIPCHK(hipMemsetAsync(db->dRow[0], 0, rows, ctxStream(ctx)));
    return ORBX_OK;
  };
  r = body();
  if (r != ORBX_OK) {
    freeDb(db);
    return r;
  }
  *out = db;
  return ORBX_OK;
}

void orbx_database_destroy(orbx_database* db) {
  if (!db) return;
  if (hipSetDevice(db->device) == hipSuccess) (void)hipStreamSynchronize(ctxStream(db->ctx));  // queued calls still read the file
  freeDb(db);
}

int orbx_database_clear(orbx_database* db) {
  if (!db) return ORBX_E_BADARG;
  orbx_ctx* ctx = db->ctx;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  HIPCHK(hipMemsetAsync(db->dRow[db->cur], 0, ((size_t)db->nWords + 1) * 4, ctxStream(ctx)));
  db->nEntries = 0;
  db->nPost = 0;
  return ORBX_OK;
}

int orbx_database_size(const orbx_database* db) { return db ? db->nEntries : ORBX_E_BADARG; }

int orbx_database_add_batch_device(orbx_ctx* ctx, orbx_database* db, int n_frames, const uint32_t* d_bow_word,
                                   const double* d_bow_value, const int32_t* d_bow_n, int capacity, int32_t* first_entry_id) {
  int r = checkBatch(ctx, n_frames, d_bow_word, d_bow_value, d_bow_n, capacity);
  if (r == ORBX_OK && !first_entry_id) r = ORBX_E_BADARG;
  if (r == ORBX_OK) r = checkDb(ctx, db);
  if (r != ORBX_OK) return r;
  const long long slots = (long long)n_frames * capacity;
  if ((long long)db->nEntries + n_frames > 0x7fffffffLL || (long long)db->nPost + slots > 0xffffffffLL) {
    ctxSetError(ctx, "database: more than 2^31 - 1 entries or 2^32 - 1 postings");
    return ORBX_E_CAPACITY;
  }
  *first_entry_id = db->nEntries;
  if (n_frames == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  hipStream_t st = ctxStream(ctx);
  const int cur = db->cur, nxt = 1 - cur;
  DbAddArgs a{};
  a.word = d_bow_word;
  a.value = d_bow_value;
  a.n = d_bow_n;
  a.cap = capacity;
  a.nFrames = n_frames;
  a.nWords = (uint32_t)db->nWords;
  a.firstId = (uint32_t)db->nEntries;
  a.oldTotal = db->nPost;
  a.cnt = db->dCnt;
  a.oldRow = db->dRow[cur];
  a.oldEntry = db->dEntry[cur];
  a.oldValue = db->dValue[cur];
  a.newRow = db->dRow[nxt];
  if (db->nWords > 0) {
    HIPCHK(hipMemsetAsync(db->dCnt, 0, (size_t)db->nWords * 4, st));
    HIPCHK(launch_db_add_count(st, a, db->dTiles));
    // the file's new length sizes its arrays: one small readback per add, behind which the stream is idle
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, db->dRow[nxt] + db->nWords, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint32_t nNew = total - db->nPost;
    if (total > 0) {
      const size_t have = db->dEntry[nxt].bytes() / 4;  // grown by half at least, so that a sequence of adds allocates rarely
      const size_t want = total <= have ? have : std::max<size_t>(total, have + have / 2);
      HIPCHK(db->dEntry[nxt].grow(want * 4));
      HIPCHK(db->dValue[nxt].grow(want * 8));
    }
    if (nNew > 0) {
      HIPCHK(db->dTmp.grow((size_t)nNew * 8));
      HIPCHK(db->dTmpValue.grow((size_t)nNew * 8));
    }
    a.newEntry = db->dEntry[nxt];
    a.newValue = db->dValue[nxt];
    a.tmpWord = db->dTmp;
    a.tmpFrame = db->dTmp + nNew;
    a.tmpValue = db->dTmpValue;
    HIPCHK(launch_db_add_fill(st, a, nNew));
    db->cur = nxt;
    db->nPost = total;
  }
  db->nEntries += n_frames;
  return ORBX_OK;
}

int orbx_database_query_batch_device(orbx_ctx* ctx, orbx_database* db, int n_queries, const uint32_t* d_bow_word,
                                     const double* d_bow_value, const int32_t* d_bow_n, int capacity, int max_results, int max_id,
                                     int32_t* d_res_entry, double* d_res_score, int32_t* d_res_n) {
  int r = checkBatch(ctx, n_queries, d_bow_word, d_bow_value, d_bow_n, capacity);
  if (r == ORBX_OK && (!d_res_entry || !d_res_score || !d_res_n)) r = ORBX_E_BADARG;
  if (r == ORBX_OK) r = checkDb(ctx, db);
  if (r != ORBX_OK) return r;
  if (max_results < 1 || max_results > ORBX_DB_MAX_RESULTS) {
    ctxSetError(ctx, "database query: max_results outside [1, ORBX_DB_MAX_RESULTS]");
    return ORBX_E_CAPACITY;
  }
  if (n_queries == 0) return ORBX_OK;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  hipStream_t st = ctxStream(ctx);
  // (int)entry_id < max_id || max_id == -1
  const int limit = max_id == -1 ? db->nEntries : std::min(std::max(max_id, 0), db->nEntries);
  if (limit == 0 || db->nPost == 0) {
    HIPCHK(hipMemsetAsync(d_res_n, 0, (size_t)n_queries * 4, st));
    return ORBX_OK;
  }
  const int perSlice = g_perSlice.load(), perMerge = g_perMerge.load(), R = max_results;
  const int nSlices = (limit + perSlice - 1) / perSlice;
  if ((long long)n_queries * nSlices > 0x7fffffffLL) return ORBX_E_CAPACITY;
  const size_t listsA = (size_t)n_queries * nSlices, listsB = (size_t)n_queries * ((nSlices + perMerge - 1) / perMerge);
  double *rawA, *rawB;
  uint32_t *idA, *idB;
  int32_t *nA, *nB;
  auto scratch = [&](Layout L) {
    rawA = L.take<double>(listsA * R);
    rawB = L.take<double>(listsB * R);
    idA = L.take<uint32_t>(listsA * R);
    idB = L.take<uint32_t>(listsB * R);
    nA = L.take<int32_t>(listsA);
    nB = L.take<int32_t>(listsB);
    return L.size();
  };
  HIPCHK(db->dLists.grow(scratch(Layout()), st));
  scratch(Layout(db->dLists));
  const bool descending = db->scoring == ORBX_BOW_BHATTACHARYYA || db->scoring == ORBX_BOW_DOT_PRODUCT;
  DbQueryArgs a{};
  a.word = d_bow_word;
  a.value = d_bow_value;
  a.n = d_bow_n;
  a.cap = capacity;
  a.nQueries = n_queries;
  a.nWords = (uint32_t)db->nWords;
  a.row = db->dRow[db->cur];
  a.entry = db->dEntry[db->cur];
  a.pvalue = db->dValue[db->cur];
  a.scoring = db->scoring;
  a.binary = db->weighting == ORBX_BOW_BINARY;
  a.minCommon = (db->scoring == ORBX_BOW_CHI_SQUARE || db->scoring == ORBX_BOW_BHATTACHARYYA) ? 5 : 1;  // MIN_COMMON_WORDS
  a.descending = descending;
  a.limit = limit;
  a.perSlice = perSlice;
  a.nSlices = nSlices;
  a.maxResults = R;
  a.listRaw = rawA;
  a.listId = idA;
  a.listN = nA;
  HIPCHK(launch_db_accumulate(st, a));
  for (int nIn = nSlices;;) {  // at least one round: the last one writes the results
    DbMergeArgs m{};
    m.nQueries = n_queries;
    m.nIn = nIn;
    m.nOut = (nIn + perMerge - 1) / perMerge;
    m.perMerge = perMerge;
    m.maxResults = R;
    m.scoring = db->scoring;
    m.descending = descending;
    m.inRaw = rawA;
    m.inId = idA;
    m.inN = nA;
    if (m.nOut == 1) {
      m.resEntry = d_res_entry;
      m.resScore = d_res_score;
      m.resN = d_res_n;
    } else {
      m.outRaw = rawB;
      m.outId = idB;
      m.outN = nB;
    }
    HIPCHK(launch_db_merge(st, m));
    if (m.nOut == 1) break;
    std::swap(rawA, rawB);
    std::swap(idA, idB);
    std::swap(nA, nB);
    nIn = m.nOut;
  }
  return ORBX_OK;
}

int orbx_database_add(orbx_ctx* ctx, orbx_database* db, const uint32_t* word, const double* value, int n, int32_t* entry_id) {
  if (!entry_id) return ORBX_E_BADARG;
  int r = checkDb(ctx, db);
  if (r == ORBX_OK) r = checkVector(ctx, db, word, value, n);
  if (r != ORBX_OK) return r;
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const int cap = std::max(n, 1);
  const int32_t hn = n;
  Staged io(db->dIo, ctxStream(ctx));  // the vector's words and values, its count
  auto dW = io.in(word, n, cap);
  auto dV = io.in(value, n, cap);
  auto dN = io.in(&hn, 1, 1);
  HIPCHK(io.open());
  r = orbx_database_add_batch_device(ctx, db, 1, io[dW], io[dV], io[dN], cap, entry_id);
  return io.close(ctx, r);
}

int orbx_database_query(orbx_ctx* ctx, orbx_database* db, const uint32_t* word, const double* value, int n, int max_results,
                        int max_id, int32_t* res_entry, double* res_score, int32_t* res_n) {
  if (!res_entry || !res_score || !res_n) return ORBX_E_BADARG;
  int r = checkDb(ctx, db);
  if (r == ORBX_OK) r = checkVector(ctx, db, word, value, n);
  if (r != ORBX_OK) return r;
  if (max_results < 1 || max_results > ORBX_DB_MAX_RESULTS) {
    ctxSetError(ctx, "database query: max_results outside [1, ORBX_DB_MAX_RESULTS]");
    return ORBX_E_CAPACITY;
  }
  r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  const int cap = std::max(n, 1);
  const int32_t hn = n;
  int32_t got = 0;
  Staged io(db->dIo, ctxStream(ctx));  // the vector's words and values, its count and the result count, the results
  auto dW = io.in(word, n, cap);
  auto dV = io.in(value, n, cap);
  auto dN = io.in(&hn, 1, 2);
  io.out(dN, 1, &got, 1);
  auto dE = io.room<int32_t>(max_results);
  auto dS = io.room<double>(max_results);
  HIPCHK(io.open());
  r = orbx_database_query_batch_device(ctx, db, 1, io[dW], io[dV], io[dN], cap, max_results, max_id, io[dE], io[dS], io[dN] + 1);
  r = io.close(ctx, r);
  if (r != ORBX_OK) return r;
  *res_n = got;
  if (!got) return ORBX_OK;
  io.out(dE, 0, res_entry, got);
  io.out(dS, 0, res_score, got);
  return io.close(ctx, ORBX_OK);
}

int64_t orbx_database_get_inverted_file(orbx_database* db, uint32_t* row_start, uint32_t* post_entry, double* post_value,
                                        int64_t capacity) {
  if (!db) return ORBX_E_BADARG;
  if (!row_start && !post_entry && !post_value) return (int64_t)db->nPost;
  if (!row_start || !post_entry || !post_value) return ORBX_E_BADARG;
  if (capacity < (int64_t)db->nPost) return ORBX_E_CAPACITY;
  orbx_ctx* ctx = db->ctx;
  const int r = ctxDrain(ctx);
  if (r != ORBX_OK) return r;
  hipStream_t st = ctxStream(ctx);
  HIPCHK(hipMemcpyAsync(row_start, db->dRow[db->cur], ((size_t)db->nWords + 1) * 4, hipMemcpyDeviceToHost, st));
  if (db->nPost) {
    HIPCHK(hipMemcpyAsync(post_entry, db->dEntry[db->cur], (size_t)db->nPost * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(post_value, db->dValue[db->cur], (size_t)db->nPost * 8, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return (int64_t)db->nPost;
}

}  // extern "C"
