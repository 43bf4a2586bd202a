"""Rate of vocabulary training on the device (orbx_vocabulary_train_device) against its CPU restatement.

  python tools/voc_train_rate.py --gpu   extracts the descriptors of 256 and 2048 bench-workload frames (640x480, 1000 features,
                                         orb_slam_tracking_amd.synth) on the device, leaves them there, and times a k = 10, L = 6
                                         training over them (TF_IDF, with the words of the training features): wall time of the
                                         synchronous call, best of --reps
  python tools/voc_train_rate.py --cpu   tests/cpp/voc_train_ref.cpp (g++ -O2) on one core over the descriptors of --cpu-frames of
                                         the same frames (the extraction still runs on the device)

One JSON line per measurement (--out appends them to a file as well; profiles/voc_train_rate.jsonl keeps a run).  The kernel
breakdown comes from a rocprofv3 --kernel-trace --stats run of the --gpu mode."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, CAP, BATCH = 640, 480, 1000, 256
K, L, SEED = 10, 6, 1


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _extract(pkg, ext, n_frames):
    """Descriptors of the bench workload's frames, extracted batch by batch into one device-resident array."""
    import torch
    from orb_slam_tracking_amd import synth
    d_desc = torch.zeros((n_frames, CAP, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(n_frames, dtype=torch.int32, device="cuda")
    d_kps = torch.zeros((BATCH, CAP, 28), dtype=torch.uint8, device="cuda")
    for lo in range(0, n_frames, BATCH):
        m = min(BATCH, n_frames - lo)
        frames = torch.from_numpy(synth.synth_frames(m, W, H, seed0=1000 + lo // 2)).cuda()
        ext.extract_batch_device(frames, m, W, H, W, W * H, d_kps, d_desc[lo:lo + m], d_n[lo:lo + m], capacity=CAP)
        torch.cuda.synchronize()
    return d_desc, d_n


def run(gpu_frames, cpu_frames, reps, out):
    import torch
    import orb_slam_tracking_amd as pkg
    ext = pkg.ORBextractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=BATCH)
    for nf in gpu_frames:
        d_desc, d_n = _extract(pkg, ext, nf)
        d_fw = torch.zeros((nf, CAP), dtype=torch.int32, device="cuda")
        best, stats = 1e30, None
        for _ in range(reps + 1):  # (the first call also allocates)
            t0 = time.perf_counter()
            v = pkg.Vocabulary.train(ext, None, K, L, 0, 0, SEED, d_desc=d_desc, d_n=d_n, n_docs=nf, capacity=CAP, d_feat_word=d_fw)
            best = min(best, time.perf_counter() - t0)
            stats = v.train_stats
            v.close()
        feats = int(d_n.clamp(0, CAP).sum())
        _emit({"what": "voc_train_device", "frames": nf, "features": feats, "k": K, "L": L, "seconds": round(best, 4),
               "features_per_s": round(feats / best), "stats": stats, "reps": reps}, out)
    if cpu_frames:
        import voc_train_ref_lib as T
        d_desc, d_n = _extract(pkg, ext, cpu_frames)
        desc, n = d_desc.cpu().numpy(), d_n.cpu().numpy()
        docs = [desc[f, :min(int(n[f]), CAP)] for f in range(cpu_frames)]
        t0 = time.perf_counter()
        tr = T.train(docs, K, L, 0, SEED)
        dt = time.perf_counter() - t0
        feats = int(sum(len(d) for d in docs))
        _emit({"what": "voc_train_ref_cpu_one_core", "frames": cpu_frames, "features": feats, "k": K, "L": L, "seconds": round(dt, 3),
               "features_per_s": round(feats / dt), "stats": tr.stats}, out)
    ext.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--gpu-frames", type=int, nargs="*", default=[256, 2048])
    ap.add_argument("--cpu-frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a.gpu_frames if a.gpu else [], a.cpu_frames if a.cpu else 0, a.reps, a.out)


if __name__ == "__main__":
    main()
