"""Rate of the database (orbx_database_add_batch_device, orbx_database_query_batch_device) against scoring every pair and against
its CPU restatement.

  python tools/db_rate.py --gpu   device, wall time to a device synchronisation, median of --reps calls, for databases of 1,000
                                  and 10,000 entries (frames of 1000 descriptors, the full k = 10, L = 6 vocabulary of
                                  tests/bow_ref_lib.py, L1 scoring) built in batches of 256: the add call on the empty database
                                  and the one that completes it; the query call for 1 and 64 queries with max_results 10; and,
                                  as the baseline, orbx_bow_score_batch_device over the same (query, entry) pairs, which ranks
                                  nothing
  python tools/db_rate.py --cpu   CPU: tests/cpp/db_ref.cpp (g++ -O2, std::map rows) on one core, add per entry and query

One JSON line per measurement (--out appends them to a file as well).  The kernel breakdown comes from a rocprofv3 --kernel-trace
--stats run of the --gpu mode."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_DESC, BATCH, N_QUERIES, MAX_RESULTS = 1000, 256, 64, 10
SIZES = (1000, 10000)


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _bow_vectors(n_frames):
    """The BowVectors of n_frames frames of N_DESC descriptors near the vocabulary's nodes, transformed on the device in batches:
    (extractor, vocabulary, d_word, d_value, d_n) with the vectors left in device memory, capacity N_DESC."""
    import torch
    import bow_ref_lib as R
    import orb_slam_tracking_amd as pkg
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    seed = np.concatenate([z[k] for k in z.files if k.endswith("/desc")])
    voc_ref = R.full_vocabulary(seed, k=10, L=6, seed=7)
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1)
    voc = pkg.Vocabulary.from_arrays(e, *voc_ref.arrays())
    d_w = torch.zeros(n_frames * N_DESC, dtype=torch.int32, device="cuda")
    d_v = torch.zeros(n_frames * N_DESC, dtype=torch.float64, device="cuda")
    d_n = torch.zeros(n_frames, dtype=torch.int32, device="cuda")
    for f0 in range(0, n_frames, 1024):
        nb = min(1024, n_frames - f0)
        feats = R.features_near(voc_ref, nb * N_DESC, 2024 + f0)
        d_d = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
        d_c = torch.full((nb,), N_DESC, dtype=torch.int32, device="cuda")
        voc.transform_batch_device(nb, d_d, d_c, d_w[f0 * N_DESC:], d_v[f0 * N_DESC:], d_n[f0:], capacity=N_DESC)
        torch.cuda.synchronize()
    return e, voc, d_w, d_v, d_n


def _rows(d_w, d_v, d_n, f0, nb):
    return d_w[f0 * N_DESC:(f0 + nb) * N_DESC], d_v[f0 * N_DESC:(f0 + nb) * N_DESC], d_n[f0:f0 + nb]


def _median_us(ts):
    return round(float(np.median(ts)) * 1e6, 1)


def run_gpu(reps, out, sizes):
    import torch
    import orb_slam_tracking_amd as pkg
    n_max = max(sizes)
    e, voc, d_w, d_v, d_n = _bow_vectors(n_max + N_QUERIES)  # the entries, then the queries
    sync = torch.cuda.synchronize
    words = round(float(d_n.float().mean()), 1)
    db = pkg.Database(voc)
    for n in sizes:
        first, last = [], []
        for _ in range(reps + 2):  # the database built again every time: its first and its last add are timed
            db.clear()
            sync()
            for f0 in range(0, n, BATCH):
                nb = min(BATCH, n - f0)
                t0 = time.perf_counter()
                db.add_batch_device(nb, *_rows(d_w, d_v, d_n, f0, nb), capacity=N_DESC)
                sync()
                dt = time.perf_counter() - t0
                if f0 == 0:
                    first.append(dt)
                if f0 + nb == n:
                    last.append(dt)
        postings = len(db.inverted_file()[1])
        _emit({"what": "database_add_batch_device", "entries": n, "batch": BATCH, "last_batch": n - (n - 1) // BATCH * BATCH,
               "mean_words": words, "postings": postings, "us_first_add": _median_us(first[2:]), "us_last_add": _median_us(last[2:]),
               "reps": reps}, out)
        for nq in (1, N_QUERIES):
            r_e = torch.zeros(nq * MAX_RESULTS, dtype=torch.int32, device="cuda")
            r_s = torch.zeros(nq * MAX_RESULTS, dtype=torch.float64, device="cuda")
            r_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
            q = _rows(d_w, d_v, d_n, n_max, nq)
            ts = []
            for i in range(reps + 3):
                t0 = time.perf_counter()
                db.query_batch_device(nq, *q, r_e, r_s, r_n, max_results=MAX_RESULTS, capacity=N_DESC)
                sync()
                ts.append(time.perf_counter() - t0)
            _emit({"what": "database_query_batch_device", "entries": n, "queries": nq, "max_results": MAX_RESULTS,
                   "us_per_call": _median_us(ts[3:]), "us_per_query": round(_median_us(ts[3:]) / nq, 2),
                   "listed_of_first_query": int(r_n[0]), "reps": reps}, out)
            # the baseline: the L1 score of every (query, entry) pair, unranked
            f1 = np.repeat(np.arange(n_max, n_max + nq, dtype=np.int32), n)
            f2 = np.tile(np.arange(n, dtype=np.int32), nq)
            d_s = torch.zeros(nq * n, dtype=torch.float64, device="cuda")
            ts = []
            for i in range(reps + 3):
                t0 = time.perf_counter()
                voc.score_pairs_device(n_max + N_QUERIES, f1, f2, d_w, d_v, d_n, d_s, capacity=N_DESC)
                sync()
                ts.append(time.perf_counter() - t0)
            _emit({"what": "bow_score_batch_device_all_pairs", "entries": n, "queries": nq, "pairs": nq * n,
                   "us_per_call": _median_us(ts[3:]), "us_per_query": round(_median_us(ts[3:]) / nq, 2), "reps": reps}, out)
    db.close()
    voc.close()
    e.close()


def run_cpu(out, sizes):
    """The restatement on one core over the same BowVectors (transformed on the device, copied to the host)."""
    import db_ref_lib as D
    n_max = max(sizes)
    e, voc, d_w, d_v, d_n = _bow_vectors(n_max + N_QUERIES)
    hn = d_n.cpu().numpy()
    hw = d_w.cpu().numpy().view(np.uint32).reshape(-1, N_DESC)
    hv = d_v.cpu().numpy().reshape(-1, N_DESC)
    n_words = voc.n_words
    voc.close()
    e.close()
    for n in sizes:
        ref = D.Database(n_words, 0)
        t0 = time.perf_counter()
        for f in range(n):
            ref.add(hw[f, :hn[f]], hv[f, :hn[f]])
        t_add = time.perf_counter() - t0
        ts = []
        for q in range(n_max, n_max + 8):
            t0 = time.perf_counter()
            ref.query(hw[q, :hn[q]], hv[q, :hn[q]], max_results=MAX_RESULTS)
            ts.append(time.perf_counter() - t0)
        _emit({"what": "db_ref_cpu_one_core", "entries": n, "us_per_add": round(t_add / n * 1e6, 1), "us_per_query": _median_us(ts),
               "max_results": MAX_RESULTS}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.gpu:
        run_gpu(a.reps, a.out, a.sizes)
    if a.cpu:
        run_cpu(a.out, a.sizes)


if __name__ == "__main__":
    main()
