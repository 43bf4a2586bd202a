"""Rate of the RANSAC stage of Initializer::Initialize (orbx_find_models_batch_device) against its CPU restatement.

  python tools/init_rate.py --gpu   device: wall time of the batched calls (to a device synchronisation) for 1, 16 and 128 pairs of synth frames
                                    (extracted and matched on the device), 200 iterations, median of --reps calls
  python tools/init_rate.py --cpu   CPU: tests/cpp/init_ref.cpp (g++ -O2, oracle scoring) per pair on one core and on all cores

One JSON line per measurement.  The kernel breakdown comes from a rocprofv3 --kernel-trace --stats run of the --gpu mode."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, ITERS = 640, 480, 200


def _sets_for(m12_rows, n_iter, sample_sets):
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(0)
    out = np.zeros((len(m12_rows), n_iter, 8), np.int32)
    for p, row in enumerate(m12_rows):
        N = int((row >= 0).sum())
        if N >= 8:
            out[p] = sample_sets(N, n_iter, libc.rand)
    return out


def _cpu_pairs(n_pairs):
    """Host data of n_pairs synth pairs: the oracle's extraction and matching (equal to the device's)."""
    import oracle_lib as O
    from orb_slam_tracking_amd import synth
    ex = O.Extractor(1000, 1.2, 8, 20, 7)
    pairs = []
    for k in range(n_pairs):
        a, b = synth.synth_pair(W, H, 1000 + k)
        _, ka, da = ex(a)
        _, kb, db = ex(b)
        _, m12, _ = O.match_init(ka, da, kb, db, (0, W, 0, H), 100, 0.9, True)
        pairs.append((ka, kb, m12))
    return pairs


def _cpu_one(args):
    import init_ref_lib as R
    ka, kb, m12, sets = args
    R.find_models(ka, kb, m12, sets)


def run_cpu(n_pairs, reps):
    import multiprocessing as mp
    import init_ref_lib as R
    from orb_slam_tracking_amd import sample_sets
    pairs = _cpu_pairs(n_pairs)
    sets = _sets_for([m for _, _, m in pairs], ITERS, sample_sets)
    jobs = [(ka, kb, m12, sets[p]) for p, (ka, kb, m12) in enumerate(pairs)]
    R.lib()
    best = 1e30
    for _ in range(reps):
        t0 = time.perf_counter()
        for j in jobs:
            _cpu_one(j)
        best = min(best, time.perf_counter() - t0)
    print(json.dumps({"what": "init_ref_cpu_one_core", "pairs": n_pairs, "iters": ITERS, "us_per_pair": round(best / n_pairs * 1e6, 1)}))
    ncpu = os.cpu_count() or 1
    with mp.get_context("fork").Pool(ncpu) as pool:
        pool.map(_cpu_one, jobs[:ncpu])  # warm-up: every worker compiles / loads its libraries
        best = 1e30
        for _ in range(reps):
            t0 = time.perf_counter()
            pool.map(_cpu_one, jobs, chunksize=max(1, len(jobs) // (4 * ncpu)))
            best = min(best, time.perf_counter() - t0)
    print(json.dumps({"what": "init_ref_cpu_all_cores", "cores": ncpu, "pairs": n_pairs, "iters": ITERS,
                      "us_per_pair": round(best / n_pairs * 1e6, 1)}))


def run_gpu(reps):
    import torch
    import orb_slam_tracking_amd as pkg
    from orb_slam_tracking_amd import synth
    P = 128
    B = 2 * P
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B)
    cap = e.capacity
    d_img = torch.from_numpy(synth.synth_frames(B, W, H)).cuda()
    d_k = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    d_d = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_m = torch.zeros(P * cap, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")
    first, second = np.arange(0, B, 2, dtype=np.int32), np.arange(1, B, 2, dtype=np.int32)
    e.extract_match_batch_device(d_img, B, W, H, W, W * H, d_k, d_d, d_n, first, second, (0, W, 0, H), d_m, d_nm)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()
    m12 = d_m.cpu().numpy().reshape(P, cap)
    sets = _sets_for([m12[p, :n[first[p]]] for p in range(P)], ITERS, pkg.sample_sets)
    d_sets = torch.from_numpy(sets).cuda()
    d_res = torch.zeros(P * pkg.HF_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    Ns = [int((m12[p, :n[first[p]]] >= 0).sum()) for p in range(P)]
    K = np.array([[520.0, 0, 320], [0, 520, 240], [0, 0, 1]], np.float32)
    d_ires = torch.zeros(P * pkg.INIT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_p3d = torch.zeros(P * cap * 3, dtype=torch.float32, device="cuda")
    d_tri = torch.zeros(P * cap, dtype=torch.uint8, device="cuda")
    calls = {
        "find_models_batch_device": lambda k: e.find_models_batch_device(B, first[:k], second[:k], d_k, d_n, d_m[:k * cap], d_sets[:k],
                                                                         d_res[:k * pkg.HF_RESULT_DTYPE.itemsize]),
        "initialize_batch_device": lambda k: e.initialize_batch_device(B, first[:k], second[:k], d_k, d_n, d_m[:k * cap], d_sets[:k], K,
                                                                       d_ires[:k * pkg.INIT_RESULT_DTYPE.itemsize], d_p3d[:k * cap * 3],
                                                                       d_tri[:k * cap]),
    }
    for what, call in calls.items():
        for np_ in (1, 16, 128):
            for _ in range(3):
                call(np_)
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call(np_)
                torch.cuda.synchronize()  # (the call is stream-ordered: wait for its results)
                ts.append(time.perf_counter() - t0)
            med = float(np.median(ts))
            print(json.dumps({"what": what, "pairs": np_, "iters": ITERS, "mean_matches": round(float(np.mean(Ns[:np_])), 1),
                              "us_per_call": round(med * 1e6, 1), "us_per_pair": round(med / np_ * 1e6, 2), "reps": reps}))
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.cpu:
        run_cpu(a.cpu_pairs, 3)
    if a.gpu:
        run_gpu(a.reps)


if __name__ == "__main__":
    main()
