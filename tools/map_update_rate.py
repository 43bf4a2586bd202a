"""Rate of the map-point update behind the local bundle adjustment (orbx_map_update_batch_device) and of its CPU restatement on
one core.

  python tools/map_update_rate.py --gpu [--reps 5] [--out profiles/map_update_rate.jsonl]
  python tools/map_update_rate.py --cpu [--out profiles/map_update_rate.jsonl]

The window is tools/lba_rate.py's local one: 10 free + 10 fixed keyframes of 1000 features each, 2000 points with 5 or 6
observations each (tests/lba_ref_lib.make_world), as tests/map_update_ref_lib.from_lba dresses it: a descriptor per observation
(the point's own with up to 24 bits turned), a tenth of the vertices' observations to erase, reference keyframes of every kind.
what = ORBX_MAP_NORMALS | ORBX_MAP_DESCRIPTORS.
--gpu: wall time of the call to a device synchronisation, median of --reps calls behind three warm-up calls, at 1, 64 and 640
problems; a batch repeats DISTINCT worlds (eight seeds), each problem with its own keyframes, rows and map set; the rows and
reference frames, which the call rewrites, are put back before every call (outside the timed span), and EVERY timed batch is
compared byte for byte with the restatement.  --cpu: tests/cpp/map_update_ref.cpp (g++ -O2) per problem on one core.  One JSON
line per measurement, appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

COUNTS = (1, 64, 640)
DISTINCT = 8
WHAT = 3
SETS = ("mask_out", "ref", "obs", "desc", "normals", "dist")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_update_rate.jsonl"))
    a = ap.parse_args()
    if a.gpu == a.cpu:
        ap.error("one of --gpu and --cpu")
    import lba_ref_lib as L
    import map_update_ref_lib as U
    from lba_rate import worlds_of
    U.lib()  # (compiled before anything is timed)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    ws = [U.from_lba(lw, 900 + k, erase=0.1) for k, lw in enumerate(worlds_of("local", L))]
    ws = [w.padded(w.cap, w.map_cap) for w in ws]
    nE, cap, mcap = ws[0].n_entries, ws[0].cap, ws[0].map_cap
    shape = dict(window="local", n_free=ws[0].n_free, n_fixed=nE - ws[0].n_free, capacity=cap, map_capacity=mcap, what=WHAT,
                 features_per_keyframe=int(np.mean([w.n.mean() for w in ws])))
    scale = U.scale_table(8, 1.2)
    refs, t_cpu = [], []
    U.update(ws[0], WHAT, scale, in_place=False)  # (warm-up)
    for w in ws:
        into = U.blank_outputs(w)
        into["mask_out"][:] = U.FILL
        t0 = time.perf_counter()
        refs.append(U.update(w, WHAT, scale, into=into))
        t_cpu.append(time.perf_counter() - t0)
    r = np.array([x["res"] for x in refs])
    counters = {k: [int(v) for v in r[k]] for k in ("n_points", "n_observations", "n_erased", "n_bad_points", "n_ref_moved", "max_observers")}
    if a.cpu:
        emit(dict(shape, measurement="cpu_restatement_one_core", problems=len(refs), ms_per_problem=[round(1e3 * t, 3) for t in t_cpu],
                  median_ms=round(1e3 * float(np.median(t_cpu)), 3), **counters))
    else:
        import torch
        import orb_slam_tracking_amd as pkg
        e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2)
        assert np.array(e.GetScaleFactors(), np.float32).tobytes() == scale.tobytes()
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
        for P in COUNTS:
            pick = [p % DISTINCT for p in range(P)]
            cat = lambda f: np.concatenate([f(ws[k]) for k in pick])  # noqa: E731
            first = (np.arange(P) * nE).astype(np.int32)
            count, n_free, mset = np.full(P, nE, np.int32), np.full(P, ws[0].n_free, np.int32), np.arange(P, dtype=np.int32)
            frames = np.arange(P * nE, dtype=np.int32)
            # (a world's reference frames are its own keyframes' indices: in the batch they move with the world's first frame)
            ref = np.stack([np.where(ws[k].map_ref >= 0, ws[k].map_ref + p * nE, ws[k].map_ref) for p, k in enumerate(pick)]).astype(np.int32)
            d_k, d_d, d_n, d_pose = dev(cat(lambda w: w.kps)), dev(cat(lambda w: w.desc)), dev(cat(lambda w: w.n)), dev(cat(lambda w: w.pose))
            d_rows0, d_ol, d_ref0 = dev(cat(lambda w: w.rows)), dev(cat(lambda w: w.outlier)), dev(ref)
            d_rows, d_ref = d_rows0.clone(), d_ref0.clone()
            d_mn = dev(np.array([ws[k].map_n for k in pick], np.int32))
            d_mp, d_mm = dev(np.stack([ws[k].map_pts for k in pick])), dev(np.stack([ws[k].map_mask for k in pick]))
            fill = lambda nbytes: torch.full((nbytes,), U.FILL, dtype=torch.uint8, device="cuda")  # noqa: E731
            d_mo, d_obs, d_desc, d_nrm, d_dist = fill(P * mcap), fill(P * mcap * 4), fill(P * mcap * 32), fill(P * mcap * 12), fill(P * mcap * 8)
            d_res = fill(P * pkg.MAP_RESULT_DTYPE.itemsize)
            want = {k: np.stack([refs[j][k] for j in pick]).tobytes() for k in SETS if k != "ref"}
            want["rows"] = np.concatenate([refs[j]["rows"] for j in pick]).tobytes()
            want["ref"] = np.stack([np.where(refs[k]["ref"] >= 0, refs[k]["ref"] + p * nE, refs[k]["ref"])
                                    for p, k in enumerate(pick)]).astype(np.int32).tobytes()
            want["res"] = np.array([refs[j]["res"] for j in pick]).tobytes()
            got = dict(mask_out=d_mo, ref=d_ref, obs=d_obs, desc=d_desc, normals=d_nrm, dist=d_dist, rows=d_rows, res=d_res)
            times, same = [], True
            for i in range(3 + a.reps):
                d_rows.copy_(d_rows0)
                d_ref.copy_(d_ref0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.map_update_problems_device(P * nE, first, count, n_free, mset, frames, d_k, d_d, d_n, d_pose, d_rows, d_ol, P, mcap, d_mn,
                                             d_mp, d_mm, d_obs, d_res, d_nrm, d_dist, d_desc, d_ref, d_mo, what=WHAT, capacity=cap)
                torch.cuda.synchronize()
                if i >= 3:
                    times.append(time.perf_counter() - t0)
                    same = same and all(got[k].cpu().numpy().tobytes() == want[k] for k in want)
            med = float(np.median(times))
            emit(dict(shape, measurement="orbx_map_update_batch_device", problems=P, reps=a.reps, us_per_call=round(1e6 * med, 1),
                      us_per_problem=round(1e6 * med / P, 2), us_min=round(1e6 * min(times), 1), us_max=round(1e6 * max(times), 1),
                      equals_restatement=bool(same), **{k: v[:min(P, DISTINCT)] for k, v in counters.items()}))
            del d_k, d_d, d_n, d_pose, d_rows0, d_rows, d_ol, d_ref0, d_ref, d_mn, d_mp, d_mm, d_mo, d_obs, d_desc, d_nrm, d_dist, d_res, got
        e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
