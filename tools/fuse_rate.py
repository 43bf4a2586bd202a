"""Rate of ORBmatcher::Fuse on the device (orbx_fuse_batch_device, orbx_fuse_scw_batch_device) against its CPU restatement, and of
orbx_match_scw_batch_device on the same sizes in the same session.

  python tools/fuse_rate.py --gpu   device, wall time to a device synchronisation, median of --reps calls, for 1, 64 and 640 pairs
                                    of a 1000-feature keyframe and a map set of 4000 points, both forms.  The scenes are those of
                                    tools/match_scw_rate.py (--distinct of them; pair p uses keyframe and map set p % distinct and
                                    a row of its own): about a quarter of a map set in view, the keyframe showing the points in
                                    view within a pixel of their projection, about 400 of them in the row on entry.  For Fuse the
                                    row holds map indices, a tenth of the other features hold a point that is not in the set
                                    (with 0 to 9 observations, a fifth of them bad), the points have 1 to 12 observations; th = 3
                                    (pose form, under the decomposed pose) and 4 (Scw form), th_low = 50.  Every call starts from
                                    the same entry rows (a device copy inside the timed region, timed alone as well).  Also the
                                    distribution of `rounds` and of the four actions, and the Scw matcher (th = 10, through its
                                    table) on the same keyframes and map sets.
  python tools/fuse_rate.py --cpu   tests/cpp/fuse_ref.cpp (g++ -O2) on one core over the first 16 of the same pairs, both forms

One JSON line per measurement (--out appends them to a file as well)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from match_scw_rate import BOUNDS, N_FEAT, N_MAP, SIZES, TH_LOW, _emit, _median_us, _pair  # noqa: E402

TH = {"pose": 3.0, "scw": 4.0}
ACTIONS = ("n_added", "n_kept_occupant", "n_replaced_occupant", "n_bad_occupant")
_scenes = {}


def _fuse_pair(seed, form):
    """The Scw matcher's scene `seed` as a Fuse pair -> (fuse_ref_lib.World, the matcher's World)."""
    import fuse_ref_lib as L
    import match_scw_ref_lib as S
    if seed not in _scenes:
        _scenes[seed] = _pair(seed)
    sw = _scenes[seed]
    rng = np.random.default_rng(seed + 5)
    row = np.where(sw.matches >= 0, sw.table[np.maximum(sw.matches, 0)], -1).astype(np.int32)  # (map indices; -1 where unmapped)
    free = np.flatnonzero(row < 0)
    row[free[rng.random(len(free)) < 0.1]] = L.UNMAPPED
    occ = np.where(rng.random(N_FEAT) < 0.2, -1, rng.integers(0, 10, N_FEAT)).astype(np.int32)
    obs = rng.integers(1, 13, N_MAP).astype(np.int32)
    if form == "pose":
        ok, R, t, _ = S.decompose_numpy(sw.scw)
        T = np.r_[R, t].astype(np.float32)
    else:
        T = sw.scw
    return L.World(form, sw.kps, sw.desc, sw.points, sw.normals, sw.dists, sw.map_desc, sw.mask, obs, T, sw.K, BOUNDS, TH[form], TH_LOW, row,
                   occ), sw


def run_gpu(reps, out, sizes, distinct):
    import torch
    import orb_slam_tracking_amd as pkg
    import fuse_ref_lib as L
    P, cap, mcap = max(sizes), N_FEAT, N_MAP
    D = min(distinct, P)
    made = {form: [_fuse_pair(1000 + p, form) for p in range(D)] for form in L.FORMS}
    scenes = [s for _, s in made["scw"]]
    stack = lambda ws, f: np.stack([getattr(w, f) for w in ws])  # noqa: E731
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    d_k, d_d, d_p, d_nr, d_ds, d_md, d_mask = (up(stack(scenes, f)) for f in ("kps", "desc", "points", "normals", "dists", "map_desc", "mask"))
    which = np.arange(P) % D
    d_n = torch.full((D,), N_FEAT, dtype=torch.int32, device="cuda")
    d_mn = torch.full((D,), N_MAP, dtype=torch.int32, device="cuda")
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1)
    fuser = pkg.MapFuser(e)
    K = scenes[0].K

    def timed(n, d_match, d_entry, call):
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
        return _median_us(ts[3:]), _median_us(tc[3:])

    for form in L.FORMS:
        worlds = [w for w, _ in made[form]]
        d_T, d_occ = up(stack(worlds, "T")[which]), up(stack(worlds, "occ_obs")[which])
        d_obs = up(stack(worlds, "obs"))
        d_entry = up(stack(worlds, "matches")[which]).view(torch.int32)
        for n in sizes:
            idx = (np.arange(n) % D).astype(np.int32)
            d_match = torch.zeros(n * cap, dtype=torch.int32, device="cuda")
            d_idx, d_other = (torch.zeros(n * mcap, dtype=torch.int32, device="cuda") for _ in range(2))
            d_act = torch.zeros(n * mcap, dtype=torch.uint8, device="cuda")
            d_res = torch.zeros(n * len(pkg.FUSE_RESULT_FIELDS), dtype=torch.int32, device="cuda")
            head = (D, idx, idx, d_k, d_d, d_n, D, mcap, d_mn, d_p, d_nr, d_ds, d_md, d_mask)
            tail = (d_T, K, BOUNDS, d_match, d_occ, d_idx, d_act, d_other, d_res)
            if form == "pose":
                call = lambda: fuser.fuse_pairs_device(*head, d_obs, *tail, th=TH[form], th_low=TH_LOW, capacity=cap)  # noqa: E731
            else:
                call = lambda: fuser.fuse_scw_pairs_device(*head, *tail, th=TH[form], th_low=TH_LOW, capacity=cap)  # noqa: E731
            us, us_copy = timed(n, d_match, d_entry, call)
            res = d_res.cpu().numpy().view(pkg.FUSE_RESULT_DTYPE)
            want = worlds[0].expected()
            assert d_match.cpu().numpy()[:N_FEAT].tobytes() == want["matches"].tobytes(), "the first pair differs from the restatement"
            assert d_act.cpu().numpy()[:N_MAP].tobytes() == want["act"].tobytes(), "the first pair differs from the restatement"
            mean = lambda f: round(float(res[f].mean()), 1)  # noqa: E731
            _emit({"what": "fuse%s_batch_device" % ("_scw" if form == "scw" else ""), "pairs": n, "distinct_scenes": min(D, n),
                   "features": N_FEAT, "map_points": N_MAP, "th": TH[form], "th_low": TH_LOW, "us_per_call": us,
                   "us_per_pair": round(us / n, 2), "us_entry_copy_alone": us_copy, "mean_fused": mean("n_fused"),
                   "mean_points": mean("n_points"), "mean_in_kf": mean("n_in_kf"), "mean_with_candidates": mean("n_with_candidates"),
                   "mean_over_dist": mean("n_over_dist"), "mean_chained": round(float(res["n_chained"].mean()), 2),
                   "actions": {a: int(res[a].sum()) for a in ACTIONS},
                   "rounds": {str(r): int(c) for r, c in enumerate(np.bincount(res["rounds"])) if c}, "reps": reps}, out)
    # the Scw matcher on the same keyframes and map sets, in the same session
    d_scw, d_table = up(stack(scenes, "scw")[which]), up(stack(scenes, "table")[which])
    d_entry = up(stack(scenes, "matches")[which]).view(torch.int32)
    for n in sizes:
        idx = (np.arange(n) % D).astype(np.int32)
        d_match = torch.zeros(n * cap, dtype=torch.int32, device="cuda")
        d_res = torch.zeros(n * len(pkg.SCW_RESULT_FIELDS), dtype=torch.int32, device="cuda")
        us, us_copy = timed(n, d_match, d_entry, lambda: e.match_scw_pairs_device(
            D, idx, idx, d_k, d_d, d_n, D, mcap, d_mn, d_p, d_nr, d_ds, d_md, d_mask, d_scw, K, BOUNDS, d_match, d_res, th=10.0, th_low=TH_LOW,
            d_kf2_to_map=d_table, capacity=cap))
        res = d_res.cpu().numpy().view(pkg.SCW_RESULT_DTYPE)
        _emit({"what": "match_scw_batch_device", "pairs": n, "distinct_scenes": min(D, n), "features": N_FEAT, "map_points": N_MAP, "th": 10.0,
               "th_low": TH_LOW, "us_per_call": us, "us_per_pair": round(us / n, 2), "us_entry_copy_alone": us_copy,
               "mean_matches": round(float(res["nmatches"].mean()), 1),
               "rounds": {str(r): int(c) for r, c in enumerate(np.bincount(res["rounds"])) if c}, "reps": reps}, out)
    e.close()


def run_cpu(out, n_pairs=16):
    """The restatement on one core over the first pairs, both forms."""
    import fuse_ref_lib as L
    for form in L.FORMS:
        worlds = [_fuse_pair(1000 + p, form)[0] for p in range(n_pairs)]
        L.fuse(worlds[0])
        ts, fused = [], []
        for w in worlds:
            t0 = time.perf_counter()
            r = L.fuse(w)
            ts.append(time.perf_counter() - t0)
            fused.append(r["res"]["n_fused"])
        _emit({"what": "fuse%s_ref_cpu_one_core" % ("_scw" if form == "scw" else ""), "pairs": n_pairs, "features": N_FEAT,
               "map_points": N_MAP, "th": TH[form], "us_per_pair": _median_us(ts), "mean_fused": round(float(np.mean(fused)), 1)}, out)


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
