"""Rate of Optimizer::PoseOptimization on the device (orbx_pose_optimize_batch_device) against its CPU restatement on one core.

  python tools/pose_rate.py [--reps 20] [--out profiles/pose_rate.jsonl]

Worlds of 200 and of 1000 correspondences (tests/pose_ref_lib.make_world: a tenth of them gross mismatches, 0.5 sigma of pixel
noise, a start pose 2 degrees and 5 % off), 10 iterations per round, as 1, 64 and 1024 problems per call: wall time of the call
to a device synchronisation, median of --reps calls.  64 distinct worlds are made per size; the 1024 problems name them in turn
(a frame and a point set may appear in any number of problems).  The CPU figure is tests/cpp/pose_ref.cpp (g++ -O2) on the same
64 worlds, compared byte for byte with the device's results on the way.  One JSON line per measurement, written to --out as
well."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DISTINCT, ITERATIONS = 64, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_rate.jsonl"))
    a = ap.parse_args()
    import torch
    import pose_ref_lib as R
    import orb_slam_tracking_amd as pkg
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    e = pkg.ORBextractor(1000, 1.2, R.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    table = e.GetInverseScaleSigmaSquares()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    for n in (200, 1000):
        worlds = [R.make_world(n, 900 + s, outliers=n // 10) for s in range(DISTINCT)]
        cap = worlds[0].cap
        d_k, d_n = dev(np.stack([w.kps for w in worlds])), dev(np.array([w.n for w in worlds], np.int32))
        d_p, d_mask = dev(np.stack([w.points for w in worlds])), dev(np.stack([w.mask for w in worlds]))
        res = None
        for P in (1, 64, 1024):
            idx = (np.arange(P) % DISTINCT).astype(np.int32)
            d_pose = dev(np.stack([worlds[i].pose0 for i in idx]))
            d_res = torch.zeros(P * pkg.POSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(P * cap, dtype=torch.uint8, device="cuda")
            call = lambda: e.pose_optimize_batch_device(DISTINCT, idx, idx, d_k, d_n, None, DISTINCT, d_p, d_mask, d_pose,  # noqa: E731
                                                        worlds[0].K, d_res, d_out, n_iterations=ITERATIONS, capacity=cap)
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
            r = d_res.cpu().numpy().view(pkg.POSE_RESULT_DTYPE).copy()
            if P == DISTINCT:
                res = r
            emit({"what": "pose_optimize_batch_device", "correspondences": n, "problems": P, "us_per_call": round(med * 1e6, 1),
                  "us_per_problem": round(med / P * 1e6, 2), "mean_iterations": round(float(r["iterations"].sum(axis=1).mean()), 1),
                  "mean_lm_trials": round(float(r["lm_trials"].mean()), 1), "mean_bad": round(float(r["n_bad"].mean()), 1),
                  "all_status_0": bool((r["status"] == 0).all()), "reps": a.reps})
        # the restatement on one core, on the same worlds
        R.lib()
        best = 1e30
        for _ in range(3):
            t0 = time.perf_counter()
            out = [R.pose_optimize(w, ITERATIONS, inv_sigma2=table) for w in worlds]
            best = min(best, time.perf_counter() - t0)
        same = all(out[p][0].tobytes() == res[p].tobytes() for p in range(DISTINCT))
        emit({"what": "pose_ref_cpu_one_core", "correspondences": n, "problems": DISTINCT, "us_per_problem": round(best / DISTINCT * 1e6, 1),
              "equal_to_the_device": bool(same)})
    e.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
