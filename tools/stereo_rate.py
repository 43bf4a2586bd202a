"""Rate of Frame::ComputeStereoMatches on the device (orbx_stereo_match_batch_device) and of its CPU restatement on one core.

  python tools/stereo_rate.py --gpu [--reps 5] [--out profiles/stereo_rate.jsonl]
  python tools/stereo_rate.py --cpu [--out profiles/stereo_rate.jsonl]

A rig is a pair of 640 x 480 frames of one scene, synth.synth_pair(640, 480, seed, shift=(d, 0)) with its independent noise, the
second frame as the left view (its features lie d columns further right), 1000 features, 8 levels at 1.2, bf / b = 80.
--gpu: the frames of a batch of 1, 64 and 128 rigs are extracted on the device as ONE batch (every rig its own two frames in it;
four distinct scenes repeat), then the wall time of the stereo call to a device synchronisation, median of --reps calls behind
three warm-up calls; EVERY timed batch is compared byte for byte with the restatement (all four arrays and the records).
--cpu: tests/cpp/stereo_ref.cpp (g++ -O2) per rig on one core, over the CPU oracle's keypoints and pyramids.  One JSON line per
measurement, appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COUNTS = (1, 64, 128)
SCENES = ((41, 9), (42, 14), (43, 20), (44, 27))  # (seed, d)
W, H, NFEATURES, BF, B = 640, 480, 1000, 80.0, 1.0
ARRAYS = ("u_right", "depth", "match_right", "sad")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_rate.jsonl"))
    a = ap.parse_args()
    if a.gpu == a.cpu:
        ap.error("one of --gpu and --cpu")
    import stereo_ref_lib as S
    from orb_slam_tracking_amd import synth
    S.lib()  # (compiled before anything is timed)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    worlds = []
    for seed, d in SCENES:
        right, left = synth.synth_pair(W, H, seed, shift=(d, 0))
        worlds.append(S.World("rate_%d" % seed, S.Scene("rate_%d" % seed, left, right, nfeatures=NFEATURES), bf=BF, b=B))
    shape = dict(width=W, height=H, nfeatures=NFEATURES, bf=BF, b=B, scenes=[list(s) for s in SCENES])
    worlds[0].expected()
    worlds[0]._expected = None  # (warm-up)
    t_cpu = []
    for w in worlds:
        w.scene.oracle()
        t0 = time.perf_counter()
        w.expected()
        t_cpu.append(time.perf_counter() - t0)
    recs = np.array([w.expected()["record"] for w in worlds])
    counters = {k: [int(v) for v in recs[k]] for k in ("n_with_candidates", "n_orb_matched", "n_before_median", "n_matches", "median_sad")}
    counters["n_left"] = [w.nL for w in worlds]
    counters["n_right"] = [w.nR for w in worlds]
    if a.cpu:
        emit(dict(shape, measurement="cpu_restatement_one_core", rigs=len(worlds), ms_per_rig=[round(1e3 * t, 3) for t in t_cpu],
                  median_ms=round(1e3 * float(np.median(t_cpu)), 3), **counters))
    else:
        import torch
        import orb_slam_tracking_amd as pkg
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
        fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
        for P in COUNTS:
            e = pkg.ORBextractor(NFEATURES, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=2 * P)
            cap, nf = e.capacity, 2 * P
            pick = [p % len(worlds) for p in range(P)]
            frames = np.stack([im for k in pick for im in (worlds[k].scene.left, worlds[k].scene.right)])
            d_imgs, d_kps, d_desc, d_n = dev(frames), fill(nf * cap * 28), fill(nf * cap * 32), fill(nf * 4)
            e.extract_batch_device(d_imgs, nf, W, H, W, W * H, d_kps, d_desc, d_n)
            torch.cuda.synchronize()
            n = d_n.cpu().numpy().view(np.int32)
            assert all(n[2 * p] == worlds[k].nL and n[2 * p + 1] == worlds[k].nR for p, k in enumerate(pick)), "the device's counts differ from the oracle's"
            left, right = np.arange(0, nf, 2, dtype=np.int32), np.arange(1, nf, 2, dtype=np.int32)
            outs = {k: fill(P * cap * 4) for k in ARRAYS}
            d_res = fill(P * 64)
            want = {k: [worlds[j].expected()[k].tobytes() for j in pick] for k in ARRAYS}
            want_res = np.array([worlds[j].expected()["record"] for j in pick]).tobytes()
            times, same = [], True
            for i in range(3 + a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.stereo_match_rigs_device(nf, left, right, d_kps, d_desc, d_n, BF, B, outs["u_right"], outs["depth"], d_res,
                                           d_match_right=outs["match_right"], d_sad=outs["sad"])
                torch.cuda.synchronize()
                if i >= 3:
                    times.append(time.perf_counter() - t0)
                    same = same and d_res.cpu().numpy().tobytes() == want_res
                    for k in ARRAYS:
                        got = outs[k].cpu().numpy().reshape(P, cap * 4)
                        same = same and all(got[p, :4 * worlds[j].nL].tobytes() == want[k][p] for p, j in enumerate(pick))
            med = float(np.median(times))
            emit(dict(shape, measurement="orbx_stereo_match_batch_device", rigs=P, reps=a.reps, capacity=cap, us_per_call=round(1e6 * med, 1),
                      us_per_rig=round(1e6 * med / P, 2), us_min=round(1e6 * min(times), 1), us_max=round(1e6 * max(times), 1),
                      equals_restatement=bool(same), **{k: v[:min(P, len(worlds))] for k, v in counters.items()}))
            del d_imgs, d_kps, d_desc, d_n, outs, d_res
            e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
