"""Rate of the loop-closing SearchByProjection under Scw on the device (orbx_match_scw_batch_device) against its CPU restatement.

  python tools/match_scw_rate.py --gpu   device, wall time to a device synchronisation, median of --reps calls, for 1, 64 and 640
                                         pairs of a 1000-feature keyframe and a map set of 4000 points.  There are --distinct
                                         (64) different scenes; pair p uses keyframe and map set p % distinct and a row of its own.
                                         About a quarter of a map set is in view (tests/match_local_ref_lib.py's make_map: the
                                         rest projects outside the image, lies behind the camera, fails the distance or the angle
                                         test) under Scw = 1.3 * pose; the keyframe shows the points in view within a pixel of
                                         their projection (the predicted level or one below, 0 to about 30 descriptor bits
                                         flipped) among unrelated features, and about 400 of them are in the row on entry as the
                                         matched keyframe's features, translated through d_kf2_to_map (a twentieth of those have
                                         no point in the set); th = 10, th_low = 50.  Every call starts from the same entry rows
                                         (a device copy inside the timed region, timed alone as well).  Also the distribution of
                                         the kernel's `rounds`.
  python tools/match_scw_rate.py --cpu   tests/cpp/match_scw_ref.cpp (g++ -O2) on one core over the first 16 of the same pairs

One JSON line per measurement (--out appends them to a file as well)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_FEAT, N_MAP, TH, TH_LOW, SCALE = 1000, 4000, 10.0, 50, 1.3
SIZES = (1, 64, 640)
BOUNDS = (0, 640, 0, 480)


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _median_us(ts):
    return round(float(np.median(ts)) * 1e6, 1)


def _pair(seed):
    """-> match_scw_ref_lib.World of N_FEAT features, N_MAP points and a table of N_FEAT entries."""
    import match_local_ref_lib as ML
    import match_scw_ref_lib as L
    rng = np.random.default_rng(seed)
    K, pose = L.camera(), L.pose_of(seed)
    scw = L.scaled(pose, SCALE)
    ok, R, t, _ = L.decompose_numpy(scw)
    pts, normals, dists, mdesc, mask = ML.make_map(N_MAP, seed + 1, np.r_[R, t].astype(np.float32), K, BOUNDS, in_view=0.25)
    none_k, none_d = np.zeros(0, L.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
    e = L.search_scw(L.World(none_k, none_d, pts, normals, dists, mdesc, mask, scw, K, BOUNDS, TH, TH_LOW))
    shown = np.flatnonzero(e["stage"] == L.STAGES.index("searched"))
    shown = rng.permutation(shown)[:N_FEAT - 40]
    n = len(shown)
    proj = e["proj"]
    k = np.zeros(N_FEAT, L.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 640, N_FEAT), rng.uniform(0, 480, N_FEAT)
    k["octave"] = np.minimum(rng.geometric(0.35, N_FEAT) - 1, L.NLEVELS - 1)
    k["angle"], k["size"] = rng.uniform(0.0, 360.0, N_FEAT).astype(np.float32), 31.0
    d = rng.integers(0, 256, (N_FEAT, 32), dtype=np.uint8)
    k["x"][:n], k["y"][:n] = proj[shown, 0] + rng.uniform(-1, 1, n), proj[shown, 1] + rng.uniform(-1, 1, n)
    k["octave"][:n] = np.maximum(proj[shown, 3].astype(np.int64) - rng.integers(0, 2, n), 0)
    d[:n] = mdesc[shown] ^ np.packbits(rng.random((n, 256)) < rng.uniform(0.0, 0.12, (n, 1)), axis=1)
    entry = np.full(N_FEAT, -1, np.int32)
    has = rng.random(n) < 400.0 / max(n, 1)
    entry[:n][has] = shown[has]
    perm = rng.permutation(N_FEAT)
    entry = entry[perm]
    # the row as the optimiser leaves it: the matched keyframe's features, a permutation of [0, N_FEAT)
    f2 = rng.permutation(N_FEAT)
    table = np.full(N_FEAT, -1, np.int32)
    table[f2] = np.where(rng.random(N_FEAT) < 0.05, -1, entry)
    row = np.where(entry >= 0, f2, -1).astype(np.int32)
    return L.World(k[perm], d[perm], pts, normals, dists, mdesc, mask, scw, K, BOUNDS, TH, TH_LOW, row, table)


def run_gpu(reps, out, sizes, distinct):
    import torch
    import orb_slam_tracking_amd as pkg
    P, cap, mcap = max(sizes), N_FEAT, N_MAP
    D = min(distinct, P)
    worlds = [_pair(1000 + p) for p in range(D)]
    stack = lambda f: np.stack([getattr(w, f) for w in worlds])  # noqa: E731
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    d_k, d_d, d_p, d_nr, d_ds, d_md, d_mask = (up(stack(f)) for f in ("kps", "desc", "points", "normals", "dists", "map_desc", "mask"))
    which = np.arange(P) % D
    d_scw, d_table = up(stack("scw")[which]), up(stack("table")[which])
    d_entry = up(stack("matches")[which]).view(torch.int32)
    d_n = torch.full((D,), N_FEAT, dtype=torch.int32, device="cuda")
    d_mn = torch.full((D,), N_MAP, dtype=torch.int32, device="cuda")
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1)
    for n in sizes:
        idx = (np.arange(n) % D).astype(np.int32)
        d_match = torch.zeros(n * cap, dtype=torch.int32, device="cuda")
        d_res = torch.zeros(n * len(pkg.SCW_RESULT_FIELDS), dtype=torch.int32, device="cuda")

        def call():
            e.match_scw_pairs_device(D, idx, idx, d_k, d_d, d_n, D, mcap, d_mn, d_p, d_nr, d_ds, d_md, d_mask, d_scw, worlds[0].K, BOUNDS,
                                     d_match, d_res, th=TH, th_low=TH_LOW, d_kf2_to_map=d_table, capacity=cap)
        ts, tc = [], []
        for _ in range(reps + 3):
            t0 = time.perf_counter()
            d_match.copy_(d_entry[:n * cap])
            call()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            d_match.copy_(d_entry[:n * cap])
            torch.cuda.synchronize()
            tc.append(time.perf_counter() - t0)
        d_match.copy_(d_entry[:n * cap])
        call()
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(pkg.SCW_RESULT_DTYPE)
        want = worlds[0].expected()
        assert d_match.cpu().numpy()[:N_FEAT].tobytes() == want["matches"].tobytes(), "the first pair differs from the restatement"
        rounds = np.bincount(res["rounds"])
        mean = lambda f: round(float(res[f].mean()), 1)  # noqa: E731
        _emit({"what": "match_scw_batch_device", "pairs": n, "distinct_scenes": min(D, n), "features": N_FEAT, "map_points": N_MAP, "th": TH,
               "th_low": TH_LOW, "us_per_call": _median_us(ts[3:]), "us_per_pair": round(_median_us(ts[3:]) / n, 2),
               "us_entry_copy_alone": _median_us(tc[3:]), "mean_matches": mean("nmatches"), "mean_total": mean("n_total"),
               "mean_found": mean("n_found"), "mean_unmapped": mean("n_unmapped"), "mean_points": mean("n_points"),
               "mean_with_candidates": mean("n_with_candidates"), "mean_over_dist": mean("n_over_dist"),
               "mean_displaced": round(float(res["n_displaced"].mean()), 2),
               "rounds": {str(r): int(c) for r, c in enumerate(rounds) if c}, "reps": reps}, out)
    e.close()


def run_cpu(out, n_pairs=16):
    """The restatement on one core over the first pairs."""
    import match_scw_ref_lib as L
    worlds = [_pair(1000 + p) for p in range(n_pairs)]
    L.search_scw(worlds[0])
    ts, nms, tot = [], [], []
    for w in worlds:
        t0 = time.perf_counter()
        r = L.search_scw(w)
        ts.append(time.perf_counter() - t0)
        nms.append(r["res"]["nmatches"])
        tot.append(r["res"]["n_total"])
    _emit({"what": "match_scw_ref_cpu_one_core", "pairs": n_pairs, "features": N_FEAT, "map_points": N_MAP, "th": TH,
           "us_per_pair": _median_us(ts), "mean_matches": round(float(np.mean(nms)), 1), "mean_total": round(float(np.mean(tot)), 1)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.gpu:
        run_gpu(a.reps, a.out, a.sizes, a.distinct)
    if a.cpu:
        run_cpu(a.out)


if __name__ == "__main__":
    main()
