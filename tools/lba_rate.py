"""Rate of the local bundle adjustment (orbx_local_ba_batch_device) and of its CPU restatement on one core.

  python tools/lba_rate.py --gpu [--reps 5] [--out profiles/lba_rate.jsonl]
  python tools/lba_rate.py --cpu [--out profiles/lba_rate.jsonl]

Two windows (tests/lba_ref_lib.make_world, half a pixel of noise per level sigma, a tenth of the edges gross mismatches):
  local   10 free + 10 fixed keyframes of 1000 features each, 2000 points with 5 or 6 observations each;
  wide    40 free + 10 fixed keyframes of 1000 features each, 5000 points.
--gpu: wall time of the call to a device synchronisation, median of --reps calls behind three warm-up calls, at 1, 64 and 640
problems (wide: 1 and 64); a batch repeats DISTINCT worlds (eight seeds), each problem with its own keyframes, rows and map set;
the results of the distinct worlds are compared byte for byte with the restatement on the way, and the distribution of
iterations, trials and n_level1 over them is reported; a window whose free keyframes fit the LDS-resident factor (at most 29) is
timed on both paths, the factor in LDS (the default) and in the workspace (orbx_debug_local_ba_lds_max_free(0)).  --cpu: tests/cpp/lba_ref.cpp (g++ -O2) per problem on one core.  One
JSON line per measurement, appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOWS = {"local": dict(n_free=10, n_fixed=10, n_points=2000, counts=(1, 64, 640)),
           "wide": dict(n_free=40, n_fixed=10, n_points=5000, counts=(1, 64))}
DISTINCT = 8


def worlds_of(name, L, distinct=DISTINCT):
    w = WINDOWS[name]
    nE = w["n_free"] + w["n_fixed"]
    out = []
    for seed in range(distinct):
        obs = 5 + seed % 2
        seen = w["n_points"] * obs // nE  # features with a point per keyframe, about
        extra = max((1000 - int(1.16 * seen) - 2) // 2, 0)  # (the keyframes' shares of the points vary by a few per cent)
        out.append(L.make_world(w["n_free"], w["n_fixed"], w["n_points"], 900 + seed, cap=1000, map_cap=w["n_points"] + 8,
                                outliers=w["n_points"] * obs // 10, obs_per_point=obs, extra=extra))
    return out


def distribution(res):
    return {k: [int(v) for v in np.asarray(res[k]).reshape(len(res), -1).sum(axis=1)] for k in ("iterations", "lm_trials", "n_level1")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", default="local,wide")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_rate.jsonl"))
    a = ap.parse_args()
    if a.gpu == a.cpu:
        ap.error("one of --gpu and --cpu")
    import lba_ref_lib as L
    L.lib()  # (compiled before anything is timed)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for name in a.windows.split(","):
        ws = worlds_of(name, L)
        shape = dict(window=name, n_free=ws[0].n_free, n_fixed=ws[0].n_entries - ws[0].n_free, capacity=ws[0].cap,
                     features_per_keyframe=int(np.mean([w.n.mean() for w in ws])))
        refs = []
        t_cpu = []
        L.local_ba(ws[0])  # (warm-up)
        for w in ws[:DISTINCT if a.gpu else 4]:
            t0 = time.perf_counter()
            refs.append(L.local_ba(w))
            t_cpu.append(time.perf_counter() - t0)
        r = np.array([x[0] for x in refs])
        if a.cpu:
            emit(dict(shape, what="cpu_restatement_one_core", problems=len(refs), ms_per_problem=[round(1e3 * t, 2) for t in t_cpu],
                      median_ms=round(1e3 * float(np.median(t_cpu)), 2), points=[int(v) for v in r["n_points"]],
                      edges=[int(v) for v in r["n_edges"]], **distribution(r)))
            continue
        import torch
        import orb_slam_tracking_amd as pkg
        e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
        nE, cap, mcap = ws[0].n_entries, ws[0].cap, ws[0].map_cap
        modes = ("lds", "workspace") if ws[0].n_free <= 29 else ("workspace",)
        for P, mode in [(P, m) for P in WINDOWS[name]["counts"] for m in modes]:
            pkg.debug_local_ba_lds_max_free(-1 if mode == "lds" else 0)
            pick = [p % DISTINCT for p in range(P)]
            kps = np.concatenate([ws[k].kps for k in pick])
            n = np.concatenate([ws[k].n for k in pick])
            pose = np.concatenate([ws[k].pose for k in pick])
            rows = np.concatenate([ws[k].rows for k in pick])
            first = (np.arange(P) * nE).astype(np.int32)
            count, n_free, mset = np.full(P, nE, np.int32), np.full(P, ws[0].n_free, np.int32), np.arange(P, dtype=np.int32)
            frames = np.arange(P * nE, dtype=np.int32)
            d_k, d_n, d_pose, d_rows = dev(kps), dev(n), dev(pose), dev(rows)
            d_mn = dev(np.array([ws[k].map_n for k in pick], np.int32))
            d_mp, d_mm = dev(np.stack([ws[k].map_pts for k in pick])), dev(np.stack([ws[k].map_mask for k in pick]))
            d_po = torch.zeros(P * nE * 48, dtype=torch.uint8, device="cuda")
            d_mo = torch.zeros(P * mcap * 12, dtype=torch.uint8, device="cuda")
            d_ol = torch.zeros(P * nE * cap, dtype=torch.uint8, device="cuda")
            d_res = torch.zeros(P * pkg.LBA_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

            def call():
                e.local_ba_problems_device(P * nE, first, count, n_free, mset, frames, d_k, d_n, d_pose, d_rows, P, mcap, d_mn, d_mp, d_mm,
                                           ws[0].K, d_po, d_ol, d_res, d_mo, capacity=cap)
                torch.cuda.synchronize()
            times = []
            for i in range(3 + a.reps):
                t0 = time.perf_counter()
                call()
                if i >= 3:
                    times.append(time.perf_counter() - t0)
            res = d_res.cpu().numpy().view(pkg.LBA_RESULT_DTYPE)
            po = d_po.cpu().numpy().view(np.float32).reshape(P, nE, 12)
            mo = d_mo.cpu().numpy().view(np.float32).reshape(P, mcap, 3)
            ol = d_ol.cpu().numpy().reshape(P, nE, cap)
            same = all(res[p].tobytes() == refs[pick[p]][0].tobytes() and po[p].tobytes() == refs[pick[p]][1].tobytes() and
                       mo[p].tobytes() == refs[pick[p]][2].tobytes() and ol[p].tobytes() == refs[pick[p]][3].tobytes() for p in range(P))
            med = float(np.median(times))
            emit(dict(shape, what="orbx_local_ba_batch_device", factor=mode, problems=P, reps=a.reps, us_per_call=round(1e6 * med, 1),
                      us_per_problem=round(1e6 * med / P, 1), us_min=round(1e6 * min(times), 1), us_max=round(1e6 * max(times), 1),
                      equals_restatement=bool(same), points=[int(v) for v in res["n_points"][:DISTINCT]],
                      edges=[int(v) for v in res["n_edges"][:DISTINCT]], **distribution(res[:DISTINCT])))
            del d_k, d_n, d_pose, d_rows, d_mn, d_mp, d_mm, d_po, d_mo, d_ol, d_res
        pkg.debug_local_ba_lds_max_free(-1)
        e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
