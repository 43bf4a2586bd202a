"""Rate of ORBmatcher::SearchByProjection on the device (orbx_match_projection_batch_device) against its CPU restatement.

  python tools/match_proj_rate.py --gpu   device, wall time to a device synchronisation, median of --reps calls, for 1, 64 and 640
                                          pairs of 1000-feature frames: every pair its own two frames and point set.  The current
                                          frame shows four fifths of the last frame's map points within two pixels of their
                                          projection (octave off by at most one, 0 to about 30 descriptor bits flipped, the angle
                                          turned by 40 degrees plus noise) among unrelated features; th = 15, orientation check on.
                                          Also the distribution of the kernel's `rounds` over the pairs.
  python tools/match_proj_rate.py --cpu   tests/cpp/match_proj_ref.cpp (g++ -O2) on one core over the first 16 of the same pairs

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

N_FEAT, TH = 1000, 15.0
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
    """-> match_proj_ref_lib.World of N_FEAT + N_FEAT features."""
    import match_proj_ref_lib as M
    rng = np.random.default_rng(seed)
    n = N_FEAT
    K, pose = M.camera(), M.pose_of(seed)
    kl = np.zeros(n, M.KEYPOINT_DTYPE)
    kl["x"], kl["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
    kl["angle"] = rng.uniform(0.0, 360.0, n).astype(np.float32)
    kl["octave"] = np.minimum(rng.geometric(0.35, n) - 1, M.NLEVELS - 1)  # (most features on the lower levels, as an extractor leaves them)
    kl["size"] = 31.0
    dl = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    uv = np.stack([rng.uniform(-20, 660, n), rng.uniform(-20, 500, n)], 1)
    pts = M.points_seen_at(pose, K, uv, rng.uniform(2.0, 10.0, n))
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    kc, dc = kl.copy(), dl.copy()
    kc["x"], kc["y"] = uv[:, 0] + rng.uniform(-2, 2, n), uv[:, 1] + rng.uniform(-2, 2, n)
    kc["octave"] = np.clip(kl["octave"] + rng.integers(-1, 2, n), 0, M.NLEVELS - 1)
    kc["angle"] = np.mod(kl["angle"] - np.float32(40.0) + rng.normal(0.0, 9.0, n).astype(np.float32), np.float32(360.0))
    kc["angle"][kc["angle"] >= 360.0] = 0.0
    dc ^= np.packbits(rng.random((n, 256)) < rng.uniform(0.0, 0.12, (n, 1)), axis=1)
    gone = rng.random(n) < 0.2  # an unrelated feature somewhere else
    kc["x"][gone], kc["y"][gone] = rng.uniform(0, 640, int(gone.sum())), rng.uniform(0, 480, int(gone.sum()))
    dc[gone] = rng.integers(0, 256, (int(gone.sum()), 32), dtype=np.uint8)
    perm = rng.permutation(n)
    return M.World(kl, dl, kc[perm], dc[perm], pts, mask, pose, K, BOUNDS, TH, True)


def run_gpu(reps, out, sizes):
    import torch
    import orb_slam_tracking_amd as pkg
    P, cap = max(sizes), N_FEAT
    worlds = [_pair(1000 + p) for p in range(P)]
    kps = np.zeros((2 * P, cap), pkg.KEYPOINT_DTYPE)
    desc = np.zeros((2 * P, cap, 32), np.uint8)
    pts, mask, pose = np.zeros((P, cap, 3), np.float32), np.zeros((P, cap), np.uint8), np.zeros((P, 12), np.float32)
    for p, w in enumerate(worlds):
        kps[2 * p], kps[2 * p + 1], desc[2 * p], desc[2 * p + 1] = w.kps_l, w.kps_c, w.desc_l, w.desc_c
        pts[p], mask[p], pose[p] = w.points, w.mask, w.pose
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    d_k, d_d, d_p, d_m, d_pose = up(kps), up(desc), up(pts), up(mask), up(pose)
    d_n = torch.full((2 * P,), N_FEAT, dtype=torch.int32, device="cuda")
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1)
    for n in sizes:
        last, cur, pset = np.arange(0, 2 * n, 2, dtype=np.int32), np.arange(1, 2 * n, 2, dtype=np.int32), np.arange(n, dtype=np.int32)
        d_match = torch.zeros(n * cap, dtype=torch.int32, device="cuda")
        d_res = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
        ts = []
        for _ in range(reps + 3):
            t0 = time.perf_counter()
            e.match_projection_pairs_device(2 * P, last, cur, pset, d_k, d_d, d_n, P, d_p, d_m, d_pose, worlds[0].K, BOUNDS, d_match, d_res,
                                            th=TH, checkOri=True, capacity=cap)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res = d_res.cpu().numpy().view(pkg.PROJ_RESULT_DTYPE)
        want = worlds[0].expected()
        assert d_match.cpu().numpy()[:N_FEAT].tobytes() == want["matches"].tobytes(), "the first pair differs from the restatement"
        rounds = np.bincount(res["rounds"])
        _emit({"what": "match_projection_batch_device", "pairs": n, "features": N_FEAT, "th": TH, "us_per_call": _median_us(ts[3:]),
               "us_per_pair": round(_median_us(ts[3:]) / n, 2), "mean_matches": round(float(res["nmatches"].mean()), 1),
               "mean_in_image": round(float(res["n_in_image"].mean()), 1), "mean_displaced": round(float(res["n_displaced"].mean()), 2),
               "rounds": {str(r): int(c) for r, c in enumerate(rounds) if c}, "reps": reps}, out)
    e.close()


def run_cpu(out, n_pairs=16):
    """The restatement on one core over the first pairs."""
    import match_proj_ref_lib as M
    worlds = [_pair(1000 + p) for p in range(n_pairs)]
    M.search_by_projection(worlds[0])
    ts, nms = [], []
    for w in worlds:
        t0 = time.perf_counter()
        r = M.search_by_projection(w)
        ts.append(time.perf_counter() - t0)
        nms.append(r["res"]["nmatches"])
    _emit({"what": "match_proj_ref_cpu_one_core", "pairs": n_pairs, "features": N_FEAT, "th": TH, "us_per_pair": _median_us(ts),
           "mean_matches": round(float(np.mean(nms)), 1)}, out)


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
