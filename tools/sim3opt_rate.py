"""Rate of Optimizer::OptimizeSim3 on the device (orbx_optimize_sim3_batch_device) against its CPU restatement on one core.

  python tools/sim3opt_rate.py [--gpu] [--cpu] [--reps 50] [--out profiles/sim3opt_rate.jsonl]

tools/sim3_rate.py's matcher worlds: pairs of 1000-feature keyframes with 400 common points, half of them in the row (the
solver's inliers) and the other half found by SearchBySim3 (here: its CPU restatement, run once while the inputs are made), so
about 200 + 199 correspondences; a tenth of them are then made gross mismatches (a cyclic shift among them) so that both rounds
and the 10-iteration branch run; the start is the world's similarity with 1 % more scale and t 1 % longer.  LoopClosing's
th2 = 10 and 5 / 10 iterations, as 1, 64 and 640 problems per call: wall time of the call to a device synchronisation, median
of --reps calls (the row is in and out: every call starts from a copy of the entry rows, which is inside the time).  64
distinct worlds are made; the 640 problems name them in turn.  Reported with the distribution of iterations and n_bad.  Then
the three-call chain compute_sim3_optimized_pairs_device (solver with 300 draws, matcher, optimiser) on the same keyframes from
the matcher worlds' own rows.  --cpu: the restatement tests/cpp/sim3opt_ref.cpp (g++ -O2, once per linearisation) on the 64
distinct problems, compared byte for byte with the device's results when both ran.  Neither flag = both.  One JSON line per
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

DISTINCT, FEATURES = 64, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3opt_rate.jsonl"))
    a = ap.parse_args()
    if not a.gpu and not a.cpu:
        a.gpu = a.cpu = True
    import sim3_ref_lib as R
    import sim3opt_ref_lib as S
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def hist(v, edges):
        return {"%d..%d" % (lo, hi - 1): int(((v >= lo) & (v < hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])}

    mworlds = [R.make_match_world(400, 2900 + s, cap=FEATURES, extra=FEATURES - 400, matched=0.5, noise_bits=20) for s in range(DISTINCT)]
    worlds = []
    for s, mw in enumerate(mworlds):
        row = R.search_by_sim3(mw)["matches"].copy()
        rng = np.random.default_rng(3900 + s)
        have = np.flatnonzero(row >= 0)
        bad = np.sort(rng.choice(have, len(have) // 10, replace=False))
        row[bad] = row[np.roll(bad, 1)]
        sim = mw.sim.copy()
        sim[9:12] *= np.float32(1.01)
        sim[12] *= np.float32(1.01)
        worlds.append(S.World(mw.kps[0], mw.n[0], mw.kps[1], mw.n[1], row, mw.points[0], mw.mask[0], mw.points[1], mw.mask[1], mw.pose[0],
                              mw.pose[1], sim, mw.K))
    cap = FEATURES
    first = None
    if a.gpu:
        import torch
        import orb_slam_tracking_amd as pkg
        e = pkg.ORBextractor(1000, 1.2, S.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
        both = lambda f: np.stack([f(w, s) for w in mworlds for s in (0, 1)])  # noqa: E731  keyframe / set 2 p, 2 p + 1
        m_k, m_d, m_n = dev(both(lambda w, s: w.kps[s])), dev(both(lambda w, s: w.desc[s])), dev(np.array([w.n[s] for w in mworlds for s in (0, 1)], np.int32))
        m_p, m_q = dev(both(lambda w, s: w.points[s])), dev(both(lambda w, s: w.dist[s]))
        m_mask, m_pose = dev(both(lambda w, s: w.mask[s])), dev(both(lambda w, s: w.pose[s]))

        def timed(call):
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()  # (the call is stream-ordered: wait for its results)
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts))

        for P in (1, 64, 640):
            idx = (2 * (np.arange(P) % DISTINCT)).astype(np.int32)
            rows0 = dev(np.stack([worlds[p % DISTINCT].match for p in range(P)]))
            sims0 = dev(np.stack([worlds[p % DISTINCT].sim for p in range(P)]))
            d_row, d_out = torch.zeros(P * cap * 4, dtype=torch.uint8, device="cuda"), torch.zeros(P * 52, dtype=torch.uint8, device="cuda")
            d_res = torch.zeros(P * pkg.SIM3OPT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

            def call():
                d_row.copy_(rows0)  # (the row is in and out: every call starts from the matcher's)
                e.optimize_sim3_pairs_device(2 * DISTINCT, idx, idx + 1, idx, idx + 1, m_k, m_n, d_row, 2 * DISTINCT, m_p, m_mask, m_pose,
                                             sims0, worlds[0].K, d_res, d_out, capacity=cap)
            med = timed(call)
            r = d_res.cpu().numpy().view(pkg.SIM3OPT_RESULT_DTYPE).copy()
            if P == DISTINCT:
                first = (r, d_out.cpu().numpy().copy(), d_row.cpu().numpy().view(np.int32).reshape(P, cap).copy())
            emit({"what": "optimize_sim3_pairs_device", "features": FEATURES, "correspondences": round(float(r["n_correspondences"].mean()), 1),
                  "problems": P, "us_per_call": round(med * 1e6, 1), "us_per_problem": round(med / P * 1e6, 2),
                  "iterations_round_1": hist(r["iterations"][:, 0], [0, 1, 2, 3, 4, 5, 6]),
                  "iterations_round_2": hist(r["iterations"][:, 1], [0, 1, 2, 3, 4, 5, 6, 8, 11]),
                  "n_bad": hist(r["n_bad"], [0, 1, 30, 38, 42, 50, 1000]), "mean_lm_trials": round(float(r["lm_trials"].mean()), 1),
                  "mean_inliers": round(float(r["n_inliers"].mean()), 1), "all_ok": bool((r["status"] == 0).all()),
                  "includes": "the copy of the entry rows", "reps": a.reps})
        # ---- the three-call chain from the matcher worlds' own rows
        for P in (1, 64, 640):
            idx = (2 * (np.arange(P) % DISTINCT)).astype(np.int32)
            d_m = dev(np.stack([mworlds[p % DISTINCT].match for p in range(P)]))
            d_draws = dev(np.stack([R.make_draws(300, 1900 + p) for p in range(P)]))
            z = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")  # noqa: E731
            d_sres, d_sim, d_row = z(P * pkg.SIM3_RESULT_DTYPE.itemsize), z(P * 52), z(P * cap * 4)
            d_mres, d_ores = z(P * pkg.MSIM3_RESULT_DTYPE.itemsize), z(P * pkg.SIM3OPT_RESULT_DTYPE.itemsize)
            call = lambda: e.compute_sim3_optimized_pairs_device(2 * DISTINCT, idx, idx + 1, idx, idx + 1, m_k, m_d, m_n, d_m,  # noqa: E731
                                                                 2 * DISTINCT, m_p, m_mask, m_q, m_pose, mworlds[0].K, mworlds[0].bounds,
                                                                 d_draws, d_sres, d_sim, d_row, d_mres, d_ores, capacity=cap)
            med = timed(call)
            r = d_ores.cpu().numpy().view(pkg.SIM3OPT_RESULT_DTYPE)
            emit({"what": "compute_sim3_optimized_pairs_device", "features": FEATURES, "n_iter": 300, "pairs": P,
                  "us_per_call": round(med * 1e6, 1), "us_per_pair": round(med / P * 1e6, 2),
                  "mean_correspondences": round(float(r["n_correspondences"].mean()), 1), "mean_inliers": round(float(r["n_inliers"].mean()), 1),
                  "loops_closed": int((r["n_inliers"] >= 20).sum()), "reps": a.reps})
        e.close()
    if a.cpu:
        S.lib()
        best = 1e30
        for _ in range(3):
            t0 = time.perf_counter()
            out = [S.optimize(w) for w in worlds]
            best = min(best, time.perf_counter() - t0)
        rec = {"what": "sim3opt_ref_cpu_one_core", "problems": DISTINCT, "us_per_problem": round(best / DISTINCT * 1e6, 1),
               "mean_correspondences": round(float(np.mean([o[0]["n_correspondences"] for o in out])), 1),
               "mean_lm_trials": round(float(np.mean([o[0]["lm_trials"] for o in out])), 1)}
        if first is not None:
            rec["equal_to_the_device"] = bool(all(out[p][0].tobytes() == first[0][p].tobytes() and out[p][2].tobytes() == first[2][p].tobytes()
                                                  for p in range(DISTINCT)))
        emit(rec)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
