"""Rate of the bag-of-words path (orbx_bow_transform_batch_device, orbx_bow_score_batch_device) against its CPU restatement.

  python tools/bow_rate.py --gpu   device: wall time of the batched calls (to a device synchronisation), median of --reps calls:
                                   transform of 1, 32 and 256 frames x 1000 descriptors with a full k = 10, L = 6 vocabulary
                                   (1,111,110 nodes, tests/bow_ref_lib.py's fixture), with and without the FeatureVector;
                                   L1 score of 128 pairs and of 256 x 256 pairs
  python tools/bow_rate.py --cpu   CPU: tests/cpp/bow_ref.cpp (g++ -O2, std::map vectors as DBoW2 keeps them) per frame on one core

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

N_DESC = 1000


def _vocab_and_frames(n_frames):
    import bow_ref_lib as R
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    seed = np.concatenate([z[k] for k in z.files if k.endswith("/desc")])
    voc = R.full_vocabulary(seed, k=10, L=6, seed=7)
    feats = R.features_near(voc, n_frames * N_DESC, 2024).reshape(n_frames, N_DESC, 32)
    return voc, feats


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def run_cpu(n_frames, out):
    voc, feats = _vocab_and_frames(n_frames)
    voc.transform(feats[0], 4)
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        for f in range(n_frames):
            voc.transform(feats[f], 4)
        best = min(best, time.perf_counter() - t0)
    _emit({"what": "bow_ref_cpu_one_core", "frames": n_frames, "descriptors": N_DESC, "us_per_frame": round(best / n_frames * 1e6, 1)},
          out)


def _median_us(call, reps, sync):
    for _ in range(3):
        call()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        sync()  # (the calls are stream-ordered: wait for their results)
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e6, 1)


def run_gpu(reps, out):
    import torch
    import orb_slam_tracking_amd as pkg
    B, cap = 256, N_DESC
    voc_ref, feats = _vocab_and_frames(B)
    e = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=1)
    voc = pkg.Vocabulary.from_arrays(e, *voc_ref.arrays())
    d_d = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
    d_n = torch.full((B,), N_DESC, dtype=torch.int32, device="cuda")
    z = lambda dt: torch.zeros(B * cap, dtype=dt, device="cuda")  # noqa: E731
    bw, bv, fn, ff, fw = z(torch.int32), z(torch.float64), z(torch.int32), z(torch.int32), z(torch.int32)
    bn, fvn = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    sync = torch.cuda.synchronize
    for nf in (1, 32, 256):
        for fv in (True, False):
            kw = dict(d_fv_node=fn, d_fv_feat=ff, d_fv_n=fvn) if fv else {}
            us = _median_us(lambda: voc.transform_batch_device(nf, d_d, d_n, bw, bv, bn, levelsup=4, capacity=cap, **kw), reps, sync)
            _emit({"what": "bow_transform_batch_device", "frames": nf, "descriptors": N_DESC, "feature_vector": fv,
                   "vocabulary": "k10_L6", "us_per_call": us, "us_per_frame": round(us / nf, 2), "reps": reps}, out)
    voc.transform_batch_device(B, d_d, d_n, bw, bv, bn, levelsup=4, capacity=cap)
    sync()
    rng = np.random.default_rng(3)
    first, second = rng.integers(0, B, 128).astype(np.int32), rng.integers(0, B, 128).astype(np.int32)
    allf, alls = np.repeat(np.arange(B, dtype=np.int32), B), np.tile(np.arange(B, dtype=np.int32), B)
    d_s = torch.zeros(B * B, dtype=torch.float64, device="cuda")
    for what, f1, f2 in (("128 pairs", first, second), ("256 x 256", allf, alls)):
        us = _median_us(lambda: voc.score_pairs_device(B, f1, f2, bw, bv, bn, d_s, capacity=cap), reps, sync)
        _emit({"what": "bow_score_batch_device", "pairs": len(f1), "case": what, "mean_words": round(float(bn.float().mean()), 1),
               "us_per_call": us, "us_per_pair": round(us / len(f1), 3), "reps": reps}, out)
    voc.close()
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cpu:
        run_cpu(a.cpu_frames, a.out)
    if a.gpu:
        run_gpu(a.reps, a.out)


if __name__ == "__main__":
    main()
