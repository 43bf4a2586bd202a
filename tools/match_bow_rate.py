"""Rate of ORBmatcher::SearchByBoW on the device (orbx_match_bow_batch_device) against its CPU restatement and, as context, against
the brute-force form of the initialization matcher.

  python tools/match_bow_rate.py --gpu   device, wall time to a device synchronisation, median of --reps calls, for 1, 64 and 640
                                         pairs of 1000-feature frames (the full k = 10, L = 6 vocabulary of tests/bow_ref_lib.py at
                                         levelsup 4; every frame is a permuted, perturbed copy of its keyframe with a third of
                                         the features replaced, as in tests/match_bow_ref_lib.py); and orbx_match_init_batch_device
                                         on the same pairs with a window that covers the whole image (every keypoint of octave 0
                                         against every other: the only device route to descriptor matches between two frames
                                         before this one -- it answers a different question)
  python tools/match_bow_rate.py --cpu   tests/cpp/match_bow_ref.cpp (g++ -O2, std::map of vectors) on one core over the same pairs

One JSON line per measurement (--out appends them to a file as well).  The kernel breakdown comes from a rocprofv3 --kernel-trace
--stats run of the --gpu mode."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_DESC, LEVELSUP, NNRATIO = 1000, 4, 0.6
SIZES = (1, 64, 640)
W, H = 640, 480


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _median_us(ts):
    return round(float(np.median(ts)) * 1e6, 1)


def _frames(voc_ref, n_pairs, seed=31):
    """Keyframes 0 .. n_pairs - 1 and their frames n_pairs .. 2 n_pairs - 1: (kps, desc) as numpy, N_DESC features each."""
    import bow_ref_lib as R
    import match_bow_ref_lib as M
    rng = np.random.default_rng(seed)
    n = n_pairs * N_DESC
    kd = R.features_near(voc_ref, n, seed, ands=4).reshape(n_pairs, N_DESC, 32)
    ka = rng.uniform(0.0, 360.0, (n_pairs, N_DESC)).astype(np.float32)
    perm = np.argsort(rng.random((n_pairs, N_DESC)), axis=1)
    fd = np.take_along_axis(kd, perm[:, :, None], axis=1).copy()
    fa = np.take_along_axis(ka, perm, axis=1)
    flips = rng.integers(0, 13, (n_pairs, N_DESC))
    rows, cols = np.indices((n_pairs, N_DESC))
    for r in range(12):  # 0 to 12 bit flips per descriptor
        byte, bit = rng.integers(0, 32, flips.shape), rng.integers(0, 8, flips.shape)
        fd[rows, cols, byte] ^= np.where(r < flips, 1 << bit, 0).astype(np.uint8)
    unrelated = rng.random((n_pairs, N_DESC)) < 1.0 / 3.0
    fd[unrelated] = rng.integers(0, 256, (int(unrelated.sum()), 32), dtype=np.uint8)
    fa = np.mod(fa - np.float32(40.0) + rng.normal(0.0, 14.0, fa.shape).astype(np.float32), np.float32(360.0)).astype(np.float32)
    fa[fa >= 360.0] = 0.0
    kps = np.zeros((2 * n_pairs, N_DESC), M.KEYPOINT_DTYPE)
    kps["angle"] = np.concatenate([ka, fa])
    kps["x"], kps["y"] = rng.uniform(16, W - 16, kps.shape), rng.uniform(16, H - 16, kps.shape)
    kps["size"] = 31.0
    return kps, np.concatenate([kd, fd])


def _world(n_pairs):
    """-> (extractor, vocabulary, device arrays of 2 n_pairs frames with their FeatureVectors, host copies)."""
    import torch
    import bow_ref_lib as R
    import orb_slam_tracking_amd as pkg
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    seed = np.concatenate([z[k] for k in z.files if k.endswith("/desc")])
    voc_ref = R.full_vocabulary(seed, k=10, L=6, seed=7)
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=1)
    voc = pkg.Vocabulary.from_arrays(e, *voc_ref.arrays())
    kps, desc = _frames(voc_ref, n_pairs)
    nf = 2 * n_pairs
    z32 = lambda m: torch.zeros(m, dtype=torch.int32, device="cuda")  # noqa: E731
    d = dict(kps=torch.from_numpy(kps.view(np.uint8).reshape(-1)).cuda(), desc=torch.from_numpy(desc.reshape(-1)).cuda(),
             n=torch.full((nf,), N_DESC, dtype=torch.int32, device="cuda"), fv_node=z32(nf * N_DESC), fv_feat=z32(nf * N_DESC), fv_n=z32(nf))
    voc.transform_batch_device(nf, d["desc"], d["n"], z32(nf * N_DESC), torch.zeros(nf * N_DESC, dtype=torch.float64, device="cuda"),
                               z32(nf), d["fv_node"], d["fv_feat"], d["fv_n"], levelsup=LEVELSUP, capacity=N_DESC)
    torch.cuda.synchronize()
    return e, voc, d, kps, desc


def run_gpu(reps, out, sizes):
    import torch
    n_max = max(sizes)
    e, voc, d, _, _ = _world(n_max)
    sync = torch.cuda.synchronize
    fvn = d["fv_n"].cpu().numpy()
    node = d["fv_node"].cpu().numpy().reshape(-1, N_DESC)
    nodes = round(float(np.mean([len(np.unique(node[f, :fvn[f]])) for f in range(min(64, 2 * n_max))])), 1)
    for n in sizes:
        kf, f = np.arange(n, dtype=np.int32), np.arange(n_max, n_max + n, dtype=np.int32)
        m, nm = torch.zeros(n * N_DESC, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        ts = []
        for i in range(reps + 3):
            t0 = time.perf_counter()
            e.match_bow_pairs_device(2 * n_max, kf, f, d["kps"], d["desc"], d["n"], d["fv_node"], d["fv_feat"], d["fv_n"], m, nm,
                                     nnratio=NNRATIO, checkOri=True, capacity=N_DESC)
            sync()
            ts.append(time.perf_counter() - t0)
        _emit({"what": "match_bow_batch_device", "pairs": n, "features": N_DESC, "levelsup": LEVELSUP, "mean_nodes_per_frame": nodes,
               "us_per_call": _median_us(ts[3:]), "us_per_pair": round(_median_us(ts[3:]) / n, 2),
               "mean_matches": round(float(nm.float().mean()), 1), "reps": reps}, out)
        st = torch.zeros(n * 3, dtype=torch.int32, device="cuda")
        ts = []
        for i in range(reps + 3):  # context: the initialization matcher with a window over the whole image
            t0 = time.perf_counter()
            e.match_pairs_device(kf, f, d["kps"], d["desc"], d["n"], (0, W, 0, H), m, nm, st, windowSize=2 * W, nnratio=NNRATIO,
                                 checkOri=True, capacity=N_DESC)
            sync()
            ts.append(time.perf_counter() - t0)
        _emit({"what": "match_init_batch_device_whole_image_window", "pairs": n, "features": N_DESC,
               "us_per_call": _median_us(ts[3:]), "us_per_pair": round(_median_us(ts[3:]) / n, 2),
               "mean_matches": round(float(nm.float().mean()), 1), "reps": reps}, out)
    voc.close()
    e.close()


def run_cpu(out, n_pairs=16):
    """The restatement on one core over the first pairs (FeatureVectors transformed on the device, copied to the host)."""
    import match_bow_ref_lib as M
    e, voc, d, kps, desc = _world(n_pairs)
    fvn = d["fv_n"].cpu().numpy()
    node = d["fv_node"].cpu().numpy().view(np.uint32).reshape(-1, N_DESC)
    feat = d["fv_feat"].cpu().numpy().view(np.uint32).reshape(-1, N_DESC)
    voc.close()
    e.close()
    side = lambda f: (kps["angle"][f], desc[f], node[f, :fvn[f]], feat[f, :fvn[f]])  # noqa: E731
    M.search_by_bow(side(0), side(n_pairs), None, NNRATIO, True)
    ts, nms = [], []
    for p in range(n_pairs):
        t0 = time.perf_counter()
        _, nm, _ = M.search_by_bow(side(p), side(n_pairs + p), None, NNRATIO, True)
        ts.append(time.perf_counter() - t0)
        nms.append(nm)
    _emit({"what": "match_bow_ref_cpu_one_core", "pairs": n_pairs, "features": N_DESC, "levelsup": LEVELSUP,
           "us_per_pair": _median_us(ts), "mean_matches": round(float(np.mean(nms)), 1)}, out)


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
