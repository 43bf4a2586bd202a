"""Rate of Sim3Solver on the device (orbx_sim3_solve_batch_device) against its CPU restatement on one core.

  python tools/sim3_rate.py [--gpu] [--cpu] [--reps 20] [--n-iter 300] [--out profiles/sim3_rate.jsonl]

Keyframe pairs of 1000 features with about 200 correspondences each (tests/sim3_ref_lib.make_world: a fifth of them gross
mismatches, 0.5 sigma of noise), LoopClosing's parameters (0.99, 20, 300, th2 9.210) and n_iter draws per problem, as 1, 64 and
640 problems per call: wall time of the call to a device synchronisation, median of --reps calls.  64 distinct worlds are made;
the 640 problems name them in turn with draws of their own.  Reported with the distribution of found_it.  --cpu: the
restatement tests/cpp/sim3_ref.cpp (g++ -O2, the literal sequential loop, which stops at found_it -- the device computes all
n_iter hypotheses) on the first 64 problems, compared byte for byte with the device's results when both ran.  Neither flag =
both.  Then ORBmatcher::SearchBySim3 (orbx_match_sim3_batch_device) the same way: pairs of 1000-feature keyframes with 400 common
points, half of them already in the row (the solver's inliers), the other half for the matcher to find (tests/sim3_ref_lib.
make_match_world), th 7.5 and TH_HIGH; the CPU figure is the restatement's two loops and the agreement loop.  One JSON line per
measurement, written to --out as well."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DISTINCT, FEATURES, CORRESPONDENCES = 64, 1000, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-iter", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_rate.jsonl"))
    a = ap.parse_args()
    if not a.gpu and not a.cpu:
        a.gpu = a.cpu = True
    import sim3_ref_lib as S
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def hist(v):
        edges = [-1, 0, 1, 2, 5, 10, 35, 100, 300]
        return {"%d..%d" % (lo, hi - 1): int(((v >= lo) & (v < hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])}

    worlds = [S.make_world(CORRESPONDENCES, 1900 + s, cap=FEATURES, outliers=CORRESPONDENCES // 5, noise=0.5,
                           extra=FEATURES - CORRESPONDENCES) for s in range(DISTINCT)]
    cap = worlds[0].cap
    all_draws = np.stack([S.make_draws(a.n_iter, 1900 + p) for p in range(640)])
    first = mfirst = None
    if a.gpu:
        import torch
        import orb_slam_tracking_amd as pkg
        e = pkg.ORBextractor(1000, 1.2, S.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
        inter = lambda a1, a2: np.stack([x for w in worlds for x in (a1(w), a2(w))])  # noqa: E731  keyframe / set 2 p, 2 p + 1
        d_k, d_n = dev(inter(lambda w: w.kps1, lambda w: w.kps2)), dev(np.array([n for w in worlds for n in (w.n1, w.n2)], np.int32))
        d_p, d_mask = dev(inter(lambda w: w.points1, lambda w: w.points2)), dev(inter(lambda w: w.mask1, lambda w: w.mask2))
        d_pose, d_m = dev(inter(lambda w: w.pose1, lambda w: w.pose2)), None
        for P in (1, 64, 640):
            idx = (2 * (np.arange(P) % DISTINCT)).astype(np.int32)
            d_m = dev(np.stack([worlds[p % DISTINCT].match for p in range(P)]))
            d_draws = dev(all_draws[:P])
            d_res = torch.zeros(P * pkg.SIM3_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            d_sim, d_row = torch.zeros(P * 13, dtype=torch.float32, device="cuda"), torch.zeros(P * cap, dtype=torch.int32, device="cuda")
            call = lambda: e.sim3_solve_batch_device(2 * DISTINCT, idx, idx + 1, idx, idx + 1, d_k, d_n, d_m, 2 * DISTINCT, d_p,  # noqa: E731
                                                     d_mask, d_pose, worlds[0].K, d_draws, d_res, d_sim, d_row, None, n_iter=a.n_iter,
                                                     capacity=cap)
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
            r = d_res.cpu().numpy().view(pkg.SIM3_RESULT_DTYPE).copy()
            if P == DISTINCT:
                first = r
            emit({"what": "sim3_solve_batch_device", "features": FEATURES, "correspondences": CORRESPONDENCES, "n_iter": a.n_iter,
                  "problems": P, "us_per_call": round(med * 1e6, 1), "us_per_problem": round(med / P * 1e6, 2),
                  "found_it": hist(r["found_it"]), "mean_inliers": round(float(r["n_inliers"].mean()), 1),
                  "all_found": bool((r["found_it"] >= 0).all()), "reps": a.reps})
        # ---- the matcher
        mworlds = [S.make_match_world(400, 2900 + s, cap=FEATURES, extra=FEATURES - 400, matched=0.5, noise_bits=20) for s in range(DISTINCT)]
        both = lambda f: np.stack([f(w, s) for w in mworlds for s in (0, 1)])  # noqa: E731
        m_k, m_d, m_n = dev(both(lambda w, s: w.kps[s])), dev(both(lambda w, s: w.desc[s])), dev(np.array([w.n[s] for w in mworlds for s in (0, 1)], np.int32))
        m_p, m_q = dev(both(lambda w, s: w.points[s])), dev(both(lambda w, s: w.dist[s]))
        m_mask, m_pose = dev(both(lambda w, s: w.mask[s])), dev(both(lambda w, s: w.pose[s]))
        mfirst = None
        for P in (1, 64, 640):
            idx = (2 * (np.arange(P) % DISTINCT)).astype(np.int32)
            rows0 = dev(np.stack([mworlds[p % DISTINCT].match for p in range(P)]))
            d_row = torch.zeros(P * cap * 4, dtype=torch.uint8, device="cuda")
            d_sim = dev(np.stack([mworlds[p % DISTINCT].sim for p in range(P)]))
            d_res = torch.zeros(P * pkg.MSIM3_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

            def call():
                d_row.copy_(rows0)  # (the row is in and out: every call starts from the solver's)
                e.match_sim3_pairs_device(2 * DISTINCT, idx, idx + 1, idx, idx + 1, m_k, m_d, m_n, 2 * DISTINCT, m_p, m_mask, m_q, m_pose,
                                          d_sim, mworlds[0].K, mworlds[0].bounds, d_row, d_res, capacity=cap)
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            med = float(np.median(ts))
            r = d_res.cpu().numpy().view(pkg.MSIM3_RESULT_DTYPE).copy()
            if P == DISTINCT:
                mfirst = (r, d_row.cpu().numpy().view(np.int32).reshape(P, cap).copy())
            emit({"what": "match_sim3_pairs_device", "features": FEATURES, "points_searched_per_direction": round(float(r["n_points_12"].mean()), 1),
                  "pairs": P, "us_per_call": round(med * 1e6, 1), "us_per_pair": round(med / P * 1e6, 2),
                  "mean_found": round(float(r["n_found"].mean()), 1), "includes": "the copy of the entry rows", "reps": a.reps})
        e.close()
    if a.cpu:
        S.lib()
        best = 1e30
        for _ in range(3):
            t0 = time.perf_counter()
            out = [S.solve(worlds[p], all_draws[p], 0) for p in range(DISTINCT)]
            best = min(best, time.perf_counter() - t0)
        rec = {"what": "sim3_ref_cpu_one_core", "correspondences": CORRESPONDENCES, "n_iter": a.n_iter, "problems": DISTINCT,
               "us_per_problem": round(best / DISTINCT * 1e6, 1),
               "mean_its_run": round(float(np.mean([o[0]["its_run"] for o in out])), 1)}
        if first is not None:
            rec["equal_to_the_device"] = bool(all(out[p][0].tobytes() == first[p].tobytes() for p in range(DISTINCT)))
        emit(rec)
        mworlds = [S.make_match_world(400, 2900 + s, cap=FEATURES, extra=FEATURES - 400, matched=0.5, noise_bits=20) for s in range(DISTINCT)]
        best = 1e30
        for _ in range(3):
            t0 = time.perf_counter()
            mout = [S.search_by_sim3(w) for w in mworlds]
            best = min(best, time.perf_counter() - t0)
        rec = {"what": "search_by_sim3_ref_cpu_one_core", "pairs": DISTINCT, "us_per_pair": round(best / DISTINCT * 1e6, 1),
               "mean_found": round(float(np.mean([o["res"]["n_found"] for o in mout])), 1)}
        if a.gpu and mfirst is not None:
            rec["equal_to_the_device"] = bool(all(mout[p]["res"].tobytes() == mfirst[0][p].tobytes() and
                                                  mout[p]["matches"].tobytes() == mfirst[1][p].tobytes() for p in range(DISTINCT)))
        emit(rec)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
