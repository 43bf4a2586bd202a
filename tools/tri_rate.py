"""Rate of LocalMapping::CreateNewMapPoints on the device (orbx_match_triangulation_batch_device, orbx_triangulate_matches_batch_device
and the two chained) against its CPU restatement.

  python tools/tri_rate.py --gpu   device, wall time to a device synchronisation, median of --reps calls, for 1, 64 and 640 pairs of
                                   1000-feature keyframes, every pair its own two keyframes (tests/tri_ref_lib.make_world: 850 points
                                   seen by both, KF2's copies with pixel noise of 0.35 of the level's scale and up to 23 descriptor bits
                                   flipped, 100 near copies of descriptors elsewhere in their node, 50 features of their own per
                                   keyframe, FeatureVectors of 100 nodes, orientation check on, no mask, no median gate): each call
                                   alone, then the chain.  The first pair's rows are compared with the restatement.
  python tools/tri_rate.py --cpu   tests/cpp/tri_ref.cpp (g++ -O2) on one core over the first 16 of the same pairs

One JSON line per measurement (--out appends them to a file as well; default profiles/tri_rate.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_FEAT = 1000
SIZES = (1, 64, 640)


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _median_us(ts):
    return round(float(np.median(ts)) * 1e6, 1)


def _pair(seed):
    import tri_ref_lib as L
    w = L.make_world(seed, n_points=850, n_nodes=100, n_distract=100, n_random=50)
    assert w.kf1.n <= N_FEAT and w.kf2.n <= N_FEAT
    return w


def run_gpu(reps, out, sizes):
    import torch
    import orb_slam_tracking_amd as pkg
    import tri_ref_lib as L
    P, cap = max(sizes), N_FEAT
    worlds = [_pair(5000 + p) for p in range(P)]
    F = 2 * P  # frames 0 .. P - 1 are the KF1s, P .. 2P - 1 the KF2s
    kps, desc = np.zeros((F, cap), L.KEYPOINT_DTYPE), np.zeros((F, cap, 32), np.uint8)
    node, feat = np.zeros((F, cap), np.uint32), np.zeros((F, cap), np.uint32)
    n, fvn, pose = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros((F, 12), np.float32)
    for p, w in enumerate(worlds):
        for f, k in ((p, w.kf1), (P + p, w.kf2)):
            kps[f, :k.n], desc[f, :k.n], n[f], pose[f] = k.kps, k.desc, k.n, k.pose
            node[f, :len(k.fv_node)], feat[f, :len(k.fv_feat)], fvn[f] = k.fv_node, k.fv_feat, len(k.fv_node)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    d_k, d_d, d_node, d_feat, d_n, d_fvn, d_pose = (up(a) for a in (kps, desc, node, feat, n, fvn, pose))
    K = worlds[0].K
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1)
    for q in sizes:
        kf1 = np.arange(q, dtype=np.int32)
        kf2 = kf1 + P
        d_m = torch.zeros(q * cap, dtype=torch.int32, device="cuda")
        d_mres = torch.zeros(q * pkg.TRI_MATCH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_p, d_nrm = (torch.zeros(q * cap * 3, dtype=torch.float32, device="cuda") for _ in range(2))
        d_msk = torch.zeros(q * cap, dtype=torch.uint8, device="cuda")
        d_dst = torch.zeros(q * cap * 2, dtype=torch.float32, device="cuda")
        d_tres = torch.zeros(q * pkg.TRI_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

        def match():
            e.match_triangulation_pairs_device(F, kf1, kf2, d_k, d_d, d_n, d_node, d_feat, d_fvn, d_pose, K, d_m, d_mres, capacity=cap)

        def tri():
            e.triangulate_matches_pairs_device(F, kf1, kf2, d_k, d_n, d_pose, K, d_m, d_p, d_msk, d_nrm, d_dst, d_tres, capacity=cap)

        def chain():
            e.create_new_map_points_pairs_device(F, kf1, kf2, d_k, d_d, d_n, d_node, d_feat, d_fvn, d_pose, K, d_m, d_mres, d_p, d_msk,
                                                 d_nrm, d_dst, d_tres, capacity=cap)
        times = {}
        for name, call in (("match_triangulation", match), ("triangulate_matches", tri), ("create_new_map_points", chain)):
            ts = []
            for _ in range(reps + 3):
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            times[name] = _median_us(ts[3:])
        mres = d_mres.cpu().numpy().view(pkg.TRI_MATCH_RESULT_DTYPE)
        tres = d_tres.cpu().numpy().view(pkg.TRI_RESULT_DTYPE)
        want = worlds[0].expected()
        assert d_m.cpu().numpy()[:worlds[0].kf1.n].tobytes() == want["match"]["matches12"][:worlds[0].kf1.n].tobytes(), "the first pair differs"
        assert d_p.cpu().numpy()[:3 * worlds[0].kf1.n].tobytes() == want["tri"]["points"][:worlds[0].kf1.n].tobytes(), "the first pair differs"
        for name, us in times.items():
            _emit({"what": name + "_batch_device" if name != "create_new_map_points" else "create_new_map_points (both calls chained)",
                   "pairs": q, "features": N_FEAT, "us_per_call": us, "us_per_pair": round(us / q, 2),
                   "mean_queries": round(float(mres["n_queries"].mean()), 1), "mean_matches": round(float(mres["nmatches"].mean()), 1),
                   "mean_epiline_rejected": round(float(mres["n_epiline_rejected"].mean()), 1),
                   "mean_rot_removed": round(float(mres["n_rot_removed"].mean()), 1),
                   "mean_points": round(float(tres["n_points"].mean()), 1), "reps": reps}, out)
    e.close()


def run_cpu(out, n_pairs=16):
    """The restatement on one core over the first pairs."""
    import tri_ref_lib as L
    worlds = [_pair(5000 + p) for p in range(n_pairs)]
    L.search(worlds[0])
    tm, tt, nm, npt = [], [], [], []
    for w in worlds:
        t0 = time.perf_counter()
        m = L.search(w, cap=N_FEAT)
        t1 = time.perf_counter()
        t = L.triangulate(w, m["matches12"], cap=N_FEAT)
        t2 = time.perf_counter()
        tm.append(t1 - t0)
        tt.append(t2 - t1)
        nm.append(int(m["res"]["nmatches"]))
        npt.append(int(t["res"]["n_points"]))
    _emit({"what": "tri_ref_cpu_one_core", "pairs": n_pairs, "features": N_FEAT, "us_per_pair_match": _median_us(tm),
           "us_per_pair_triangulate": _median_us(tt), "us_per_pair_chain": _median_us(np.array(tm) + np.array(tt)),
           "mean_matches": round(float(np.mean(nm)), 1), "mean_points": round(float(np.mean(npt)), 1)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tri_rate.jsonl"))
    a = ap.parse_args()
    if a.gpu:
        run_gpu(a.reps, a.out, a.sizes)
    if a.cpu:
        run_cpu(a.out)


if __name__ == "__main__":
    main()
