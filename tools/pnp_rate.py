"""Rate of PnPsolver on the device (orbx_pnp_solve_batch_device) against its CPU restatement on one core.

  python tools/pnp_rate.py [--reps 20] [--out profiles/pnp_rate.jsonl]

Frames of 1000 features with about 200 correspondences each (tests/pnp_ref_lib.make_world: a fifth of them gross mismatches,
0.5 sigma of pixel noise), the reference's parameters (0.99, 10, 300, 4, 0.5, 5.991) and n_iter = 35, as 1, 64 and 640 problems
per call: wall time of the call to a device synchronisation, median of --reps calls.  64 distinct worlds are made; the 640
problems name them in turn with draws of their own.  Reported with the distribution of found_it and n_refines.  The CPU figure
is tests/cpp/pnp_ref.cpp (g++ -O2, the literal sequential loop, which stops at found_it) on the first 64 problems, compared byte
for byte with the device's results on the way.  One JSON line per measurement, written to --out as well."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DISTINCT, N_ITER, FEATURES, CORRESPONDENCES = 64, 35, 1000, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_rate.jsonl"))
    a = ap.parse_args()
    import torch
    import pnp_ref_lib as Q
    import orb_slam_tracking_amd as pkg
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def hist(v):
        u, c = np.unique(v, return_counts=True)
        return {str(int(k)): int(n) for k, n in zip(u, c)}

    e = pkg.ORBextractor(1000, 1.2, Q.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    worlds = [Q.make_world(CORRESPONDENCES, 1900 + s, cap=FEATURES, outliers=CORRESPONDENCES // 5, noise=0.5,
                           extra=FEATURES - CORRESPONDENCES) for s in range(DISTINCT)]
    cap = worlds[0].cap
    d_k, d_n = dev(np.stack([w.kps for w in worlds])), dev(np.array([w.n for w in worlds], np.int32))
    d_p, d_mask = dev(np.stack([w.points for w in worlds])), dev(np.stack([w.mask for w in worlds]))
    all_draws = np.stack([Q.make_draws(N_ITER, 1900 + p) for p in range(640)])
    first = None
    for P in (1, 64, 640):
        idx = (np.arange(P) % DISTINCT).astype(np.int32)
        d_draws = dev(all_draws[:P])
        d_res = torch.zeros(P * pkg.PNP_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_pose, d_row = torch.zeros(P * 12, dtype=torch.float32, device="cuda"), torch.zeros(P * cap, dtype=torch.int32, device="cuda")
        call = lambda: e.pnp_solve_batch_device(DISTINCT, idx, idx, d_k, d_n, None, DISTINCT, d_p, d_mask, worlds[0].K, d_draws,  # noqa: E731
                                                d_res, d_pose, d_row, None, n_iter=N_ITER, capacity=cap)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()  # (the call is stream-ordered: wait for its results)
            ts.append(time.perf_counter() - t0)
        med = float(np.median(ts))
        r = d_res.cpu().numpy().view(pkg.PNP_RESULT_DTYPE).copy()
        if P == DISTINCT:
            first = r
        emit({"what": "pnp_solve_batch_device", "features": FEATURES, "correspondences": CORRESPONDENCES, "n_iter": N_ITER, "problems": P,
              "us_per_call": round(med * 1e6, 1), "us_per_problem": round(med / P * 1e6, 2), "found_it": hist(r["found_it"]),
              "n_refines": hist(r["n_refines"]), "mean_inliers": round(float(r["n_inliers"].mean()), 1),
              "all_refined": bool((r["refined"] == 1).all()), "reps": a.reps})
    # the restatement on one core, on the first 64 problems
    Q.lib()
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        out = [Q.solve(worlds[p], all_draws[p], 0) for p in range(DISTINCT)]
        best = min(best, time.perf_counter() - t0)
    same = all(out[p][0].tobytes() == first[p].tobytes() for p in range(DISTINCT))
    emit({"what": "pnp_ref_cpu_one_core", "correspondences": CORRESPONDENCES, "problems": DISTINCT, "us_per_problem": round(best / DISTINCT * 1e6, 1),
          "equal_to_the_device": bool(same)})
    e.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
