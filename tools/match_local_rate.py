"""Rate of Tracking::SearchLocalPoints on the device (orbx_match_local_map_batch_device) against its CPU restatement.

  python tools/match_local_rate.py --gpu   device, wall time to a device synchronisation, median of --reps calls, for 1, 64 and 640
                                           pairs of a 1000-feature frame and a 4000-point local map: every pair its own frame and
                                           map.  About a quarter of the map is in view (tests/match_local_ref_lib.py's make_map:
                                           the rest projects outside the image, lies behind the camera, fails the distance or the
                                           angle test); the frame shows the points in view within a pixel of their projection (the
                                           predicted level or one below, 0 to about 30 descriptor bits flipped) among unrelated
                                           features, and already has half of them on entry (a tenth of those flagged outliers);
                                           th = 1, nnratio = 0.8.  Every call starts from the same entry rows (a device copy inside
                                           the timed region, timed alone as well).  Also the distribution of the kernel's `rounds`.
  python tools/match_local_rate.py --cpu   tests/cpp/match_local_ref.cpp (g++ -O2) on one core over the first 16 of the same pairs

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

N_FEAT, N_MAP, TH, NNRATIO = 1000, 4000, 1.0, 0.8
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
    """-> match_local_ref_lib.World of N_FEAT features and N_MAP points."""
    import match_local_ref_lib as L
    rng = np.random.default_rng(seed)
    K, pose = L.camera(), L.pose_of(seed)
    pts, normals, dists, mdesc, mask = L.make_map(N_MAP, seed + 1, pose, K, BOUNDS, in_view=0.25)
    none_k, none_d = L._none_frame()
    proj = L.search_local_points(L.World(none_k, none_d, pts, normals, dists, mdesc, mask, pose, K, BOUNDS, TH, NNRATIO))["proj"]
    shown = np.flatnonzero(proj[:, 5] == 5.0)
    shown = rng.permutation(shown)[:N_FEAT - 40]
    n = len(shown)
    k = np.zeros(N_FEAT, L.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 640, N_FEAT), rng.uniform(0, 480, N_FEAT)
    k["octave"] = np.minimum(rng.geometric(0.35, N_FEAT) - 1, L.NLEVELS - 1)
    k["angle"], k["size"] = rng.uniform(0.0, 360.0, N_FEAT).astype(np.float32), 31.0
    d = rng.integers(0, 256, (N_FEAT, 32), dtype=np.uint8)
    k["x"][:n], k["y"][:n] = proj[shown, 0] + rng.uniform(-1, 1, n), proj[shown, 1] + rng.uniform(-1, 1, n)
    k["octave"][:n] = np.maximum(proj[shown, 3].astype(np.int64) - rng.integers(0, 2, n), 0)
    d[:n] = mdesc[shown] ^ np.packbits(rng.random((n, 256)) < rng.uniform(0.0, 0.12, (n, 1)), axis=1)
    entry = np.full(N_FEAT, -1, np.int32)
    has = rng.random(n) < 0.5
    entry[:n][has] = shown[has]
    outlier = ((entry >= 0) & (rng.random(N_FEAT) < 0.1)).astype(np.uint8)
    perm = rng.permutation(N_FEAT)
    return L.World(k[perm], d[perm], pts, normals, dists, mdesc, mask, pose, K, BOUNDS, TH, NNRATIO, entry[perm], outlier[perm])


def run_gpu(reps, out, sizes):
    import torch
    import orb_slam_tracking_amd as pkg
    P, cap, mcap = max(sizes), N_FEAT, N_MAP
    worlds = [_pair(1000 + p) for p in range(P)]
    stack = lambda f: np.stack([getattr(w, f) for w in worlds])  # noqa: E731
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    d_k, d_d, d_p, d_nr, d_ds, d_md, d_mask, d_pose, d_out = (up(stack(f)) for f in
                                                                ("kps", "desc", "points", "normals", "dists", "map_desc", "mask", "pose", "outlier"))
    d_entry = up(stack("matches")).view(torch.int32)
    d_n = torch.full((P,), N_FEAT, dtype=torch.int32, device="cuda")
    d_mn = torch.full((P,), N_MAP, dtype=torch.int32, device="cuda")
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1)
    for n in sizes:
        idx = np.arange(n, dtype=np.int32)
        d_match = torch.zeros(n * cap, dtype=torch.int32, device="cuda")
        d_view = torch.zeros(n * mcap, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros(n * len(pkg.LOCAL_RESULT_FIELDS), dtype=torch.int32, device="cuda")
        ts, tc = [], []
        for _ in range(reps + 3):
            t0 = time.perf_counter()
            d_match.copy_(d_entry[:n * cap])
            e.match_local_map_pairs_device(P, idx, idx, d_k, d_d, d_n, P, mcap, d_mn, d_p, d_nr, d_ds, d_md, d_mask, d_pose, worlds[0].K,
                                           BOUNDS, d_match, d_res, th=TH, nnratio=NNRATIO, d_outlier=d_out, d_point_view=d_view, capacity=cap)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            d_match.copy_(d_entry[:n * cap])
            torch.cuda.synchronize()
            tc.append(time.perf_counter() - t0)
            d_match.copy_(d_entry[:n * cap])
        e.match_local_map_pairs_device(P, idx, idx, d_k, d_d, d_n, P, mcap, d_mn, d_p, d_nr, d_ds, d_md, d_mask, d_pose, worlds[0].K, BOUNDS,
                                       d_match, d_res, th=TH, nnratio=NNRATIO, d_outlier=d_out, d_point_view=d_view, capacity=cap)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(pkg.LOCAL_RESULT_DTYPE)
        want = worlds[0].expected()
        assert d_match.cpu().numpy()[:N_FEAT].tobytes() == want["matches"].tobytes(), "the first pair differs from the restatement"
        assert d_view.cpu().numpy()[:N_MAP].tobytes() == want["view"].tobytes(), "the first pair's point_view differs from the restatement"
        rounds = np.bincount(res["rounds"])
        mean = lambda f: round(float(res[f].mean()), 1)  # noqa: E731
        _emit({"what": "match_local_map_batch_device", "pairs": n, "features": N_FEAT, "map_points": N_MAP, "th": TH, "nnratio": NNRATIO,
               "us_per_call": _median_us(ts[3:]), "us_per_pair": round(_median_us(ts[3:]) / n, 2), "us_entry_copy_alone": _median_us(tc[3:]),
               "mean_matches": mean("nmatches"), "mean_in_view": mean("n_in_view"), "mean_seen": mean("n_seen"),
               "mean_with_candidates": mean("n_with_candidates"), "mean_ratio_rejected": mean("n_ratio_rejected"),
               "mean_displaced": round(float(res["n_displaced"].mean()), 2),
               "rounds": {str(r): int(c) for r, c in enumerate(rounds) if c}, "reps": reps}, out)
    e.close()


def run_cpu(out, n_pairs=16):
    """The restatement on one core over the first pairs."""
    import match_local_ref_lib as L
    worlds = [_pair(1000 + p) for p in range(n_pairs)]
    L.search_local_points(worlds[0])
    ts, nms, inv = [], [], []
    for w in worlds:
        t0 = time.perf_counter()
        r = L.search_local_points(w)
        ts.append(time.perf_counter() - t0)
        nms.append(r["res"]["nmatches"])
        inv.append(r["res"]["n_in_view"])
    _emit({"what": "match_local_ref_cpu_one_core", "pairs": n_pairs, "features": N_FEAT, "map_points": N_MAP, "th": TH,
           "us_per_pair": _median_us(ts), "mean_matches": round(float(np.mean(nms)), 1), "mean_in_view": round(float(np.mean(inv)), 1)}, out)


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
        run_cpu(a.out)


if __name__ == "__main__":
    main()
