// CPU restatement of the database as include/orbx.h ("database") specifies it: DBoW2's TemplatedDatabase add and query
// (TemplatedDatabase.h:433-464, :566-1113) over an inverted file whose rows are std::maps from entry id to value.  Written from
// the specification, for the tests only; compiled with -ffp-contract=off (tests/db_ref_lib.py).  The result list is sorted with
// a total order on (sum, entry id): deviation 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace {

struct Db {
  int scoring = 0;  // 0 L1, 1 L2, 2 chi-square, 4 Bhattacharyya, 5 dot product
  bool binary = false;
  uint32_t entries = 0;
  std::vector<std::map<uint32_t, double>> rows;  // per word: entry id -> value
};

double term(const Db& db, double q, double d) {
  switch (db.scoring) {
    case 0: return std::fabs(q - d) - std::fabs(q) - std::fabs(d);
    case 1: return -q * d;
    case 2: return q + d != 0.0 ? -q * d / (q + d) : 0.0;
    case 4: return std::sqrt(q * d);
    default: return db.binary ? 1.0 : q * d;
  }
}

double finalScore(const Db& db, double sum) {
  switch (db.scoring) {
    case 0: return -sum / 2.0;
    case 1: return sum <= -1.0 ? 1.0 : 1.0 - std::sqrt(1.0 + sum);
    case 2: return -2. * sum;
    default: return sum;
  }
}

struct Hit {
  double sum;
  uint32_t id;
};

}  // namespace

extern "C" {

void* dr_create(int n_words, int scoring, int binary) {
  Db* db = new Db();
  db->scoring = scoring;
  db->binary = binary != 0;
  db->rows.resize((size_t)n_words);
  return db;
}

void dr_free(void* h) { delete static_cast<Db*>(h); }

void dr_clear(void* h) {
  Db* db = static_cast<Db*>(h);
  for (auto& r : db->rows) r.clear();
  db->entries = 0;
}

int dr_size(void* h) { return (int)static_cast<Db*>(h)->entries; }

int dr_add(void* h, const uint32_t* word, const double* value, int n) {
  Db* db = static_cast<Db*>(h);
  const uint32_t id = db->entries++;
  for (int i = 0; i < n; i++) db->rows[word[i]].emplace_hint(db->rows[word[i]].end(), id, value[i]);
  return (int)id;
}

// the whole list when max_results <= 0; out_entry / out_score hold max_results entries, or size() of them
int dr_query(void* h, const uint32_t* word, const double* value, int n, int max_results, int max_id, int32_t* out_entry,
             double* out_score) {
  const Db* db = static_cast<const Db*>(h);
  std::map<uint32_t, std::pair<double, int>> sums;  // entry id -> (sum, common words)
  for (int i = 0; i < n; i++) {  // the query's words ascend
    for (const auto& post : db->rows[word[i]]) {
      if (!((int)post.first < max_id || max_id == -1)) continue;
      const double t = term(*db, value[i], post.second);
      auto it = sums.find(post.first);
      if (it == sums.end()) {
        sums.emplace(post.first, std::make_pair(t, 1));  // the chain starts from the first term
      } else {
        it->second.first += t;
        it->second.second += 1;
      }
    }
  }
  const int minCommon = (db->scoring == 2 || db->scoring == 4) ? 5 : 1;
  const bool descending = db->scoring == 4 || db->scoring == 5;
  std::vector<Hit> hits;
  for (const auto& s : sums)
    if (s.second.second >= minCommon) hits.push_back(Hit{s.second.first, s.first});
  std::sort(hits.begin(), hits.end(), [descending](const Hit& a, const Hit& b) {
    if (a.sum != b.sum) return descending ? a.sum > b.sum : a.sum < b.sum;
    return a.id < b.id;
  });
  if (max_results > 0 && (int)hits.size() > max_results) hits.resize((size_t)max_results);
  for (size_t i = 0; i < hits.size(); i++) {
    out_entry[i] = (int32_t)hits[i].id;
    out_score[i] = finalScore(*db, hits[i].sum);
  }
  return (int)hits.size();
}

// row_start [words + 1], the postings word by word; with NULL arrays only the count
long long dr_inverted_file(void* h, uint32_t* row_start, uint32_t* post_entry, double* post_value) {
  const Db* db = static_cast<const Db*>(h);
  long long n = 0;
  for (size_t w = 0; w < db->rows.size(); w++) {
    if (row_start) row_start[w] = (uint32_t)n;
    for (const auto& post : db->rows[w]) {
      if (post_entry) post_entry[n] = post.first;
      if (post_value) post_value[n] = post.second;
      n++;
    }
  }
  if (row_start) row_start[db->rows.size()] = (uint32_t)n;
  return n;
}

}  // extern "C"
