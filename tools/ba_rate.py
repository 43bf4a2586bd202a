"""Rate of the two-view bundle adjustment (orbx_bundle_adjust_batch_device) against its CPU restatement on one core.

  python tools/ba_rate.py [--reps 20] [--out profiles/ba_rate.jsonl]

Two workloads, each initialized on the device (200 RANSAC iterations) and then adjusted behind it for 1, 16 and 128 pairs, 20
iterations: wall time of the call to a device synchronisation, median of --reps calls.
  two_view   synthetic two-view scenes with depth (tests/ba_ref_lib.init_scene, 500 keypoints): scenes are drawn until 128 of them
             are accepted by the device Initializer, so every timed pair runs the Levenberg-Marquardt loop;
  bench      the bench workload's synthetic frame pairs, extracted and matched on the device.  They are shifted planes, which the
             Initializer refuses: their pairs leave the kernel as ORBX_BA_SKIPPED.  No rate is reported for a batch in which no
             pair was optimised, only that fact.
The CPU figure is tests/cpp/ba_ref.cpp (g++ -O2) on the downloaded intermediates of the two_view pairs, compared byte for byte
with the device's results on the way.  One JSON line per measurement, written to --out as well."""
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

W, H, ITERS, BA_ITERS, MIN_POINTS = 640, 480, 200, 20, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_rate.jsonl"))
    a = ap.parse_args()
    import torch
    import ba_ref_lib as R
    import orb_slam_tracking_amd as pkg
    from orb_slam_tracking_amd import synth
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    P = 128
    K = np.array([[520.0, 0, 320], [0, 520, 240], [0, 0, 1]], np.float32)
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=2 * P)
    table = e.GetInverseScaleSigmaSquares()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731

    def timed(what, k_list, call, res, extra):
        for k in k_list:
            r = res[:k]
            ran = r["iterations"] > 0
            if not ran.any():
                emit(dict({"what": what, "pairs": k, "pairs_optimised": 0,
                           "note": "the Initializer accepted none of these pairs: nothing to time"}, **extra))
                continue
            for _ in range(3):
                call(k)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call(k)
                torch.cuda.synchronize()  # (the call is stream-ordered: wait for its results)
                ts.append(time.perf_counter() - t0)
            med = float(np.median(ts))
            emit(dict({"what": what, "pairs": k, "pairs_optimised": int(ran.sum()), "mean_points": round(float(r["n_points"][ran].mean()), 1),
                       "mean_iterations": round(float(r["iterations"][ran].mean()), 1),
                       "mean_lm_trials": round(float(r["lm_trials"][ran].mean()), 1), "us_per_call": round(med * 1e6, 1),
                       "us_per_pair": round(med / k * 1e6, 2), "reps": a.reps}, **extra))

    def adjust(B_, first, second, d_k, d_n, d_m, d_ir, d_p3d, d_tri, Kc, cap, d_res, d_out, k):
        e.bundle_adjust_batch_device(B_, first[:k], second[:k], d_k, d_n, d_m[:k * cap * 4], d_ir[:k * pkg.INIT_RESULT_DTYPE.itemsize],
                                     d_p3d[:k * cap * 12], d_tri[:k * cap], Kc, d_res[:k * pkg.BA_RESULT_DTYPE.itemsize],
                                     d_out[:k * cap * 12], n_iterations=BA_ITERS, min_points=MIN_POINTS, capacity=cap)

    # ---- two_view: scenes the Initializer accepts ----
    chunk, seed, kept = 256, 0, []
    while len(kept) < P and seed < 16 * chunk:
        scenes = [R.init_scene(s) for s in range(seed, seed + chunk)]
        seed += chunk
        cap = len(scenes[0][1])
        Kt = scenes[0][0]
        kps = np.stack([k for s in scenes for k in (s[1], s[3])])
        n = np.array([c for s in scenes for c in (s[2], s[4])], np.int32)
        m12, sets = np.stack([s[5] for s in scenes]), np.stack([s[6] for s in scenes])
        first, second = np.arange(0, 2 * chunk, 2, dtype=np.int32), np.arange(1, 2 * chunk, 2, dtype=np.int32)
        d_ir = torch.zeros(chunk * pkg.INIT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_p3d = torch.zeros(chunk * cap * 12, dtype=torch.uint8, device="cuda")
        d_tri = torch.zeros(chunk * cap, dtype=torch.uint8, device="cuda")
        e.initialize_batch_device(2 * chunk, first, second, dev(kps), dev(n), dev(m12), dev(sets), Kt, d_ir, d_p3d, d_tri, capacity=cap,
                                  n_iter=ITERS)
        torch.cuda.synchronize()
        ir = d_ir.cpu().numpy().view(R.INIT_RESULT_DTYPE)
        p3d, tri = d_p3d.cpu().numpy().view(np.float32).reshape(chunk, cap, 3), d_tri.cpu().numpy().reshape(chunk, cap)
        for p in np.flatnonzero(ir["status"] == 0):
            kept.append(R.Pair(kps[2 * p].copy(), n[2 * p], kps[2 * p + 1].copy(), n[2 * p + 1], m12[p].copy(), ir[p:p + 1].copy(),
                               p3d[p].copy(), tri[p].copy(), Kt.reshape(9)))
    emit({"what": "two_view_scenes", "drawn": seed, "accepted_by_the_initializer": len(kept)})
    kept = kept[:P]
    if kept:
        Pk, cap = len(kept), kept[0].cap
        first, second = np.arange(0, 2 * Pk, 2, dtype=np.int32), np.arange(1, 2 * Pk, 2, dtype=np.int32)
        d_k = dev(np.stack([k for w in kept for k in (w.k1, w.k2)]))
        d_n = dev(np.array([c for w in kept for c in (w.n1, w.n2)], np.int32))
        d_m, d_ir = dev(np.stack([w.m12 for w in kept])), dev(np.concatenate([w.init for w in kept]))
        d_p3d, d_tri = dev(np.stack([w.p3d for w in kept])), dev(np.stack([w.tri for w in kept]))
        d_res = torch.zeros(Pk * pkg.BA_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros(Pk * cap * 12, dtype=torch.uint8, device="cuda")
        call = lambda k: adjust(2 * Pk, first, second, d_k, d_n, d_m, d_ir, d_p3d, d_tri, kept[0].K, cap, d_res, d_out, k)  # noqa: E731
        call(Pk)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(pkg.BA_RESULT_DTYPE).copy()
        timed("bundle_adjust_batch_device", [k for k in (1, 16, 128) if k <= Pk], call, res, {"workload": "two_view"})
        # the restatement on one core, on the same pairs
        R.lib()
        best = 1e30
        for rep in range(3):
            t0 = time.perf_counter()
            out = [R.bundle_adjust(w, BA_ITERS, MIN_POINTS, True, inv_sigma2=table) for w in kept]
            best = min(best, time.perf_counter() - t0)
        same = all(out[p][0].tobytes() == res[p].tobytes() for p in range(Pk))
        emit({"what": "ba_ref_cpu_one_core", "workload": "two_view", "pairs": Pk, "us_per_pair": round(best / Pk * 1e6, 1),
              "equal_to_the_device": bool(same)})

    # ---- bench: the bench workload's pairs ----
    B = 2 * P
    cap = e.capacity
    d_img = torch.from_numpy(synth.synth_frames(B, W, H)).cuda()
    d_k = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    d_d = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_m = torch.zeros(P * cap * 4, dtype=torch.uint8, device="cuda")
    d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")
    first, second = np.arange(0, B, 2, dtype=np.int32), np.arange(1, B, 2, dtype=np.int32)
    e.extract_match_batch_device(d_img, B, W, H, W, W * H, d_k, d_d, d_n, first, second, (0, W, 0, H), d_m, d_nm)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()
    m12 = d_m.cpu().numpy().view(np.int32).reshape(P, cap)
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(0)
    sets = np.zeros((P, ITERS, 8), np.int32)
    nm = []
    for p in range(P):
        N = int((m12[p, :n[first[p]]] >= 0).sum())
        nm.append(N)
        if N >= 8:
            sets[p] = pkg.sample_sets(N, ITERS, libc.rand)
    d_ir = torch.zeros(P * pkg.INIT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_p3d = torch.zeros(P * cap * 12, dtype=torch.uint8, device="cuda")
    d_tri = torch.zeros(P * cap, dtype=torch.uint8, device="cuda")
    e.initialize_batch_device(B, first, second, d_k, d_n, d_m, dev(sets), K, d_ir, d_p3d, d_tri, n_iter=ITERS)
    d_res = torch.zeros(P * pkg.BA_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(P * cap * 12, dtype=torch.uint8, device="cuda")
    call = lambda k: adjust(B, first, second, d_k, d_n, d_m, d_ir, d_p3d, d_tri, K, cap, d_res, d_out, k)  # noqa: E731
    call(P)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(pkg.BA_RESULT_DTYPE).copy()
    ist = d_ir.cpu().numpy().view(R.INIT_RESULT_DTYPE)["status"]
    timed("bundle_adjust_batch_device", (1, 16, 128), call, res,
          {"workload": "bench", "mean_matches": round(float(np.mean(nm)), 1), "initialized_of_128": int((ist == 0).sum())})
    e.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
