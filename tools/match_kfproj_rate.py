"""Rate of the relocalisation SearchByProjection on the device (orbx_match_keyframe_projection_batch_device) against its CPU
restatement.

  python tools/match_kfproj_rate.py --gpu   device, wall time to a device synchronisation, median of --reps calls, for 1, 64 and 640
                                            pairs of a 1000-feature frame against a 1000-feature keyframe: every pair its own frame
                                            and keyframe.  About four fifths of the keyframe's points project into the image and pass
                                            the distance test; the frame shows them within a pixel of their projection (the predicted
                                            level or one below, 0 to about 30 descriptor bits flipped, the keyframe's angle turned by
                                            30 degrees) among unrelated features, and already has about half of the keyframe's points
                                            on entry (a tenth of those flagged outliers); th = 10, ORBdist = 100, orientation check on.
                                            Every call starts from the same entry rows (a device copy inside the timed region, timed
                                            alone as well).  Also the distribution of the kernel's `rounds`.
  python tools/match_kfproj_rate.py --cpu   tests/cpp/match_kfproj_ref.cpp (g++ -O2) on one core over the first 16 of the same pairs

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

N_FEAT, TH, ORB_DIST = 1000, 10.0, 100
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
    """-> match_kfproj_ref_lib.World of N_FEAT features on both sides."""
    import match_kfproj_ref_lib as L
    rng = np.random.default_rng(seed)
    n = N_FEAT
    K, pose = L.camera(), L.pose_of(seed)
    kk = L._keypoints(n, rng)
    kk["angle"] = rng.integers(0, 360, n).astype(np.float32)
    dk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    uv = np.stack([rng.uniform(-30, 670, n), rng.uniform(-25, 505, n)], 1)
    depth = rng.uniform(2.0, 10.0, n)
    depth[rng.random(n) < 0.04] *= -1.0
    pts = L.points_seen_at(pose, K, uv, depth)
    dist, dists = L._distances(pts, pose, np.minimum(rng.geometric(0.35, n) - 1, L.NLEVELS - 1), rng)
    dists[:, 1] = np.where(rng.random(n) < 0.05, dist / 1.3, dists[:, 1])
    mask = (rng.random(n) < 0.95).astype(np.uint8)
    none_k, none_d = L._none_frame()
    proj = L.search_by_projection(L.World(kk, dk, none_k, none_d, pts, dists, None, pose, K, BOUNDS, TH, ORB_DIST))["proj"]
    shown = rng.permutation(np.flatnonzero(proj[:, 5] == 5.0))[:n - 40]
    s = len(shown)
    k = L._keypoints(n, rng)
    k["octave"] = np.minimum(rng.geometric(0.35, n) - 1, L.NLEVELS - 1)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    k["x"][:s], k["y"][:s] = proj[shown, 0] + rng.uniform(-1, 1, s), proj[shown, 1] + rng.uniform(-1, 1, s)
    k["octave"][:s] = np.maximum(proj[shown, 3].astype(np.int64) - rng.integers(0, 2, s), 0)
    k["angle"][:s] = (kk["angle"][shown] + 330.0) % 360.0
    d[:s] = dk[shown] ^ np.packbits(rng.random((s, 256)) < rng.uniform(0.0, 0.12, (s, 1)), axis=1)
    entry = np.full(n, -1, np.int32)
    has = rng.random(s) < 0.62
    entry[:s][has] = shown[has]
    outlier = ((entry >= 0) & (rng.random(n) < 0.1)).astype(np.uint8)
    perm = rng.permutation(n)
    return L.World(kk, dk, k[perm], d[perm], pts, dists, mask, pose, K, BOUNDS, TH, ORB_DIST, True, None, entry[perm], outlier[perm])


def run_gpu(reps, out, sizes):
    import torch
    import orb_slam_tracking_amd as pkg
    P, cap = max(sizes), N_FEAT
    worlds = [_pair(1000 + p) for p in range(P)]
    stack = lambda f: np.stack([getattr(w, f) for w in worlds])  # noqa: E731
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    # frames 0 .. P - 1 are the keyframes, P .. 2P - 1 the current frames
    d_k = up(np.concatenate([stack("kps_k"), stack("kps_c")]))
    d_d = up(np.concatenate([stack("desc_k"), stack("desc_c")]))
    d_p, d_ds, d_mask, d_pose, d_out = (up(stack(f)) for f in ("points", "dists", "mask", "pose", "outlier"))
    d_entry = up(stack("matches")).view(torch.int32)
    d_n = torch.full((2 * P,), N_FEAT, dtype=torch.int32, device="cuda")
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1)
    for n in sizes:
        kf = np.arange(n, dtype=np.int32)
        cur = kf + P
        d_match = torch.zeros(n * cap, dtype=torch.int32, device="cuda")
        d_res = torch.zeros(n * len(pkg.KFPROJ_RESULT_FIELDS), dtype=torch.int32, device="cuda")

        def call():
            e.match_keyframe_projection_pairs_device(2 * P, kf, cur, kf, d_k, d_d, d_n, P, d_p, d_mask, d_ds, d_pose, worlds[0].K, BOUNDS,
                                                     d_match, d_res, th=TH, ORBdist=ORB_DIST, checkOri=True, d_outlier=d_out, capacity=cap)
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
        res = d_res.cpu().numpy().view(pkg.KFPROJ_RESULT_DTYPE)
        want = worlds[0].expected()
        assert d_match.cpu().numpy()[:N_FEAT].tobytes() == want["matches"].tobytes(), "the first pair differs from the restatement"
        rounds = np.bincount(res["rounds"])
        mean = lambda f: round(float(res[f].mean()), 1)  # noqa: E731
        searched = res["n_points"] - res["n_out_image"] - res["n_out_distance"]
        _emit({"what": "match_keyframe_projection_batch_device", "pairs": n, "features": N_FEAT, "th": TH, "orb_dist": ORB_DIST,
               "us_per_call": _median_us(ts[3:]), "us_per_pair": round(_median_us(ts[3:]) / n, 2), "us_entry_copy_alone": _median_us(tc[3:]),
               "mean_matches": mean("nmatches"), "mean_found": mean("n_found"), "mean_searched": round(float(searched.mean()), 1),
               "mean_with_candidates": mean("n_with_candidates"), "mean_over_dist": mean("n_over_dist"),
               "mean_rot_removed": mean("n_rot_removed"), "mean_displaced": round(float(res["n_displaced"].mean()), 2),
               "rounds": {str(r): int(c) for r, c in enumerate(rounds) if c}, "reps": reps}, out)
    e.close()


def run_cpu(out, n_pairs=16):
    """The restatement on one core over the first pairs."""
    import match_kfproj_ref_lib as L
    worlds = [_pair(1000 + p) for p in range(n_pairs)]
    L.search_by_projection(worlds[0])
    ts, nms, found = [], [], []
    for w in worlds:
        t0 = time.perf_counter()
        r = L.search_by_projection(w)
        ts.append(time.perf_counter() - t0)
        nms.append(r["res"]["nmatches"])
        found.append(r["res"]["n_found"])
    _emit({"what": "match_kfproj_ref_cpu_one_core", "pairs": n_pairs, "features": N_FEAT, "th": TH, "orb_dist": ORB_DIST,
           "us_per_pair": _median_us(ts), "mean_matches": round(float(np.mean(nms)), 1), "mean_found": round(float(np.mean(found)), 1)}, out)


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
