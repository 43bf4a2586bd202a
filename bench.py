#!/usr/bin/env python3
"""bench.py — frames/sec of the ORB extract + initialization-match hot path on MI355X.

One step = one pass of the hot path over one batch of synthetic 640x480 frames that are already resident in HBM:
  orbx_extract_match_batch_device_async: extraction of B frames -> SearchForInitialization of the B/2 consecutive pairs
  (window 100, ratio 0.9), issued stream-ordered, whole batches on four lanes of the context (orbx_set_pipeline_depth:
  at most four batches in flight; every batch is complete when the clock stops)  ->  (N > 1) RCCL all_gather of the
  per-frame keypoint counts.
Frames are sharded per rank (weak scaling: B frames per GPU), one process per GPU.  The steps rotate through four distinct
input sets (315 MB per GPU, more than the 256 MB Infinity Cache), so no step finds its input cache-resident.
Prints ONE JSON line on rank 0 (see the task contract): metric / value / roofline / cpu_baseline.
`python bench.py --gpus N` with N > 1 starts its own N ranks (torch.distributed.run, one process per GPU, RCCL) when it is not
already running under a launcher; after the timed regions rank 0 compares one complete output set with the CPU oracle
("checked": true -- outside every timed region).

The --steps timed steps run as back-to-back regions (--regions, five by default, each of at least 100 steps: fewer regions when
--steps is small); `value` and `ms_per_step` come from the median region's time per step, and `spread` carries min / max / the
first region and all of them in order.  --dump-outputs DIR writes what the last timed step computed as .npy files (dump_outputs).
The roofline of the dominant kernel is the VALU one: these kernels are bound by vector-instruction issue,
not by HBM.
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PARAMS = (1000, 1.2, 8, 20, 7)  # BASELINE "canonical" preset: 1000 features, 8 levels
W, H = 640, 480
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec
# VALU issue capacity of the chip: 256 CUs x 4 SIMDs x 2.4 GHz SIMD-cycles per second.  A wave64 vector instruction holds
# its SIMD's issue port for 2 cycles (add / sub / logic / shift / mov / fma) or 4 cycles (min / max / compare / cndmask /
# cvt / every three-operand integer op / packed 16-bit / dot4 / dot2): tools/microbench/valu_rate.hip, measured on gfx950.
VALU_PEAK_SIMD_CYCLES = 256 * 4 * 2.4e9
KERNEL_OF = {"pyramid": "k_pyramid_bands", "fast": "k_fast_wave", "describe": "k_describe_patch"}
PMC_WORKLOAD = "bench: 256 frames 640x480 / 1000 features per launch"


def level_sizes(w, h, nlevels=8, sf=1.2):
    out, s = [], np.float32(1.0)
    for _ in range(nlevels):
        inv = np.float32(1.0) / s
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
        s = np.float32(np.float64(s) * np.float64(np.float32(sf)))
    return out


def algorithmic_bytes(w, h, n_kp):
    """Per-frame algorithmic bytes of each stage (SURVEY.md 8(d) stage-streaming model)."""
    P = [a * b for a, b in level_sizes(w, h)]
    sp = sum(P)
    return {
        "pyramid": (sp - P[-1]) + (sp - P[0]),          # level reads + level writes
        "fast": sp,                                      # every level pixel read once
        "describe": 2 * sp + n_kp * (749 + 512) + n_kp * 60,  # blur read+write of the model, disc + samples, outputs
        "total": 5 * sp - P[0] - P[-1] + 1321 * n_kp,
    }


def load_pmc():
    """The committed counter profile of this round (profiles/r*_pmc.json, made by tools/pmc_to_json.py from rocprofv3 --pmc
    passes of this very command): per kernel and per frame, VALU wave-instructions, VALU issue cycles and HBM bytes."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc.json")))
    # the newest file collected from THIS workload (tools/pmc_to_json.py records it; files of rounds 1-3 carry no workload and are
    # the bench workload's): a counter file of another configuration must never become the source of `frac`
    for f in reversed(files):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if d.get("workload", PMC_WORKLOAD) == PMC_WORKLOAD:
            return d, os.path.basename(f)
    return None, None


def config_roofline(cfg, w, h, stage_ms, launch, n_kp):
    """The roofline object of one of the other BASELINE configurations (other_configs.<cfg>.roofline): the
    dominant stage of the SYNCHRONOUS call (live stage events), its kernel, the launch duration (a synchronous call of >= 16 frames is
    two half batches: two launches per stage), and against it the VALU issue cycles and the HBM bytes per launch from the committed
    counter passes of that configuration (profiles/r*_<cfg>_pmc.json, tools/prof_config.sh) and the algorithmic bytes of the stage."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s_pmc.json" % cfg)))
    pmc = json.load(open(files[-1])) if files else None
    dom = max(("pyramid", "fast", "describe"), key=lambda s_: stage_ms[s_])
    kname = KERNEL_OF[dom]
    nl = 2 if launch.get("split") else 1
    ms = stage_ms[dom] / nl
    fpl = launch.get("frames_per_launch") or 0
    roof = {"bound": "valu", "kernel": kname, "stage": dom, "unit": "T SIMD-issue-cycles/s", "peak": VALU_PEAK_SIMD_CYCLES / 1e12,
            "avg_launch_ms": ms, "launches_per_call": nl, "frames_per_launch": fpl, "pmc_file": os.path.basename(files[-1]) if files else None,
            "pmc_stale": None if not pmc else (pmc.get("kernel_sources_sha16") != kernel_sources_sha16()),
            "achieved": None, "frac": None, "traffic": None}
    pk = None
    for k_, v_ in ((pmc or {}).get("per_launch") or {}).items():
        if k_.startswith(kname):
            pk = v_
    ab = algorithmic_bytes(w, h, n_kp)[dom] * fpl
    if pk and ms > 0 and pmc.get("frames_per_launch") == fpl:
        roof["achieved"] = pk["valu_issue_cycles"] / (ms * 1e-3) / 1e12
        roof["frac"] = roof["achieved"] / roof["peak"]
        roof["traffic"] = pk["fetch_bytes"] + pk["write_bytes"]
        roof["in_the_profile"] = {"avg_launch_ms": pk["avg_us"] / 1e3, "frac": pk["valu_issue_cycles"] / (pk["avg_us"] * 1e-6) / VALU_PEAK_SIMD_CYCLES}
    roof["hbm"] = {"algorithmic_bytes_per_launch": ab, "algorithmic_frac": ab / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS if ms > 0 else None,
                   "counter_frac": roof["traffic"] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS if roof["traffic"] and ms > 0 else None, "peak_GBs": HBM_PEAK_GBS}
    return roof


def bf_roofline(bf):
    """The matrix-core view of the 2000 x 2000 brute-force match: descriptor pairs per second of the whole call (live) and of
    k_match_bf_mfma alone (its average launch in the committed rocprofv3 stats of the same call) against the int8 rate, 16
    v_mfma_i32_32x32x32_i8 of 32 cycles per 2048 pairs on 1024 SIMDs at 2.4 GHz = 9.8 T pairs/s."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_c5_pmc.json")))
    pmc = json.load(open(files[-1])) if files else None
    roof = {"bound": "mfma", "kernel": "k_match_bf_mfma", "unit": "T descriptor pairs/s", "peak": 9.8,
            "achieved": bf["descriptor_pairs_per_s"] / 1e12, "frac": bf["descriptor_pairs_per_s"] / 9.8e12,
            "what": "the whole match call (prep, lists on the matrix cores, sort, resolve), live",
            "pmc_file": os.path.basename(files[-1]) if files else None,
            "pmc_stale": None if not pmc else (pmc.get("kernel_sources_sha16") != kernel_sources_sha16())}
    pk = ((pmc or {}).get("per_launch_bf_match") or {}).get("k_match_bf_mfma")
    if pk:
        pairs = bf["sets_per_call"] * bf["descriptors"][0] * bf["descriptors"][1]
        roof["kernel_alone_in_the_profile"] = {"avg_launch_us": pk["avg_us"], "pairs_per_launch": pairs,
                                               "frac": pairs / (pk["avg_us"] * 1e-6) / 9.8e12,
                                               "traffic": pk["fetch_bytes"] + pk["write_bytes"]}
    return roof


def kernel_sources_sha16():
    """Hash of the device + host sources liborbx.so is built from: tools/pmc_to_json.py records it in profiles/r*_pmc.json, and the
    roofline object says whether the counters were collected from the code under test (`pmc_stale`)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "orb_slam_tracking_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".inc", ".h", ".cpp")):
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


def self_launch(n):
    """`python bench.py --gpus N` outside a launcher: N fresh ranks through torch.distributed.run (this process has not touched the
    GPU and never will), rank 0's JSON line relayed, exit code = the children's."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this pool
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


def oracle_check(frames, got, cores):
    """Not timed: one complete output set (host copies of k / d / n / m / nm) of the last batch against the CPU oracle -- every
    frame's count, keypoint bytes and descriptor bytes, every pair's nmatches and matches12.  Returns (ok, what)."""
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    B, cap = len(frames), 1000
    threads = max(1, min(cores, 16))
    bad = []

    def work(t):
        oe = O.Extractor(*PARAMS)
        for p_ in range(t, B // 2, threads):
            a, b = oe(frames[2 * p_]), oe(frames[2 * p_ + 1])
            nm, m12, _ = O.match_init(a[1], a[2], b[1], b[2], (0, W, 0, H), 100, 0.9, True)
            for f, (_, ko, do) in ((2 * p_, a), (2 * p_ + 1, b)):
                n = int(got["n"][f])
                if n != len(ko) or got["k"][f * cap * 28:(f * cap + n) * 28].tobytes() != ko.tobytes() or \
                        got["d"][f * cap * 32:(f * cap + n) * 32].tobytes() != do.tobytes():
                    bad.append("frame %d" % f)
            if int(got["nm"][p_]) != nm or not np.array_equal(got["m"][p_ * cap:p_ * cap + len(m12)], m12):
                bad.append("pair %d" % p_)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))
    return (not bad), ("%d frames (count, keypoint bytes, descriptor bytes) and %d pairs (nmatches, matches12) of the last batch equal "
                       "the CPU oracle" % (B, B // 2) if not bad else "MISMATCH: " + ", ".join(sorted(bad)[:8]))


MIN_REGION_STEPS = 100
DUMP_LIMIT_BYTES = 64_000_000
DUMP_SEED = 20240611


def region_steps(steps, regions):
    """The `steps` timed steps split into back-to-back regions: at most `regions`, each of at least MIN_REGION_STEPS steps (one
    region when there are fewer), as even as they can be.  The sum is exactly `steps`."""
    n = max(1, min(max(regions, 1), steps // MIN_REGION_STEPS))
    return [steps // n + (1 if i < steps % n else 0) for i in range(n)]


def dump_outputs(out_dir, got, B, cap=1000, limit=DUMP_LIMIT_BYTES):
    """Writes the output set of one batch -- what a caller of orbx_extract_match_batch_device_async receives: keypoints,
    descriptors and counts per frame, matches12 and nmatches per consecutive pair -- as float32 / float64 .npy files under
    `out_dir`.  Slots past a frame's count (keypoints, descriptors, matches12) hold no result and are written as zeros (-1 for
    matches12), so that two builds compare output for output.  When the whole batch exceeds `limit` bytes, a fixed seeded sample
    of its pairs is written (both frames of each); frame_index / pair_index name the frames and pairs written."""
    from orb_slam_tracking_amd import KEYPOINT_DTYPE
    P = B // 2
    per_pair = 2 * (cap * 7 * 4 + cap * 32 * 4 + 8 + 8) + cap * 4 + 8 + 8
    if P * per_pair <= limit:
        pairs = np.arange(P)
    else:
        pairs = np.sort(np.random.default_rng(DUMP_SEED).choice(P, size=max(1, limit // per_pair), replace=False))
    fr = np.stack([2 * pairs, 2 * pairs + 1], 1).ravel()
    n = np.asarray(got["n"], np.int32)[:B]
    kp = np.frombuffer(np.ascontiguousarray(got["k"]).tobytes()[:B * cap * 28], KEYPOINT_DTYPE).reshape(B, cap)[fr]
    keypoints = np.stack([kp[f].astype(np.float32) for f in KEYPOINT_DTYPE.names], -1)  # x y size angle response octave class_id
    desc = np.asarray(got["d"], np.uint8)[:B * cap * 32].reshape(B, cap, 32)[fr].astype(np.float32)
    m12 = np.asarray(got["m"], np.int32)[:P * cap].reshape(P, cap)[pairs].astype(np.float32)
    valid = np.arange(cap)[None, :] < n[fr][:, None]
    keypoints[~valid] = 0
    desc[~valid] = 0
    m12[~(np.arange(cap)[None, :] < n[2 * pairs][:, None])] = -1
    arrays = {"keypoints": keypoints, "descriptors": desc, "n_keypoints": n[fr].astype(np.float64), "matches12": m12,
              "nmatches": np.asarray(got["nm"], np.int32)[:P][pairs].astype(np.float64),
              "frame_index": fr.astype(np.float64), "pair_index": pairs.astype(np.float64)}
    assert sum(a.nbytes for a in arrays.values()) <= limit
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(arrays)


def cpu_share():
    """Host cores this process may really use: cgroup quota if set, else the affinity mask; capped at 64."""
    n = len(os.sched_getaffinity(0))
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(float(q) / float(p) + 0.5)))
    except Exception:
        pass
    return max(1, min(n, 64))


class Runner:
    """The stream-ordered call sequence that is timed: one step = orbx_extract_match_batch_device_async on `B` resident frames and
    their B / 2 consecutive pairs, `nout` batches in flight on as many output sets.  N > 1 (or --force-collective): the all_gather
    of batch k's counts (RCCL over xGMI) is issued asynchronously from a snapshot of the counts once batch k has been waited for,
    i.e. it runs under the kernels of batch k + 1; it is waited for before the next one is issued and before the clock stops."""

    @staticmethod
    def make_outs(B, nout, dev, cap=1000):
        """One set of output arrays per batch in flight: the batches are issued stream-ordered, and batches in flight together must not
        share their outputs."""
        import torch
        return [dict(k=torch.zeros(B * cap * 28, dtype=torch.uint8, device=dev), d=torch.zeros(B * cap * 32, dtype=torch.uint8, device=dev),
                     n=torch.zeros(B, dtype=torch.int32, device=dev), m=torch.zeros((B // 2) * cap, dtype=torch.int32, device=dev),
                     nm=torch.zeros(B // 2, dtype=torch.int32, device=dev)) for _ in range(nout)]

    def __init__(self, ext, d_imgs, B, nout, world, coll, cdev, dev, dist, cap=1000, outs=None):
        import torch
        self.ext, self.d_imgs, self.B, self.nout, self.world, self.coll, self.dist, self.cap = ext, d_imgs, B, nout, world, coll, dist, cap
        self.outs = outs if outs is not None else Runner.make_outs(B, nout, dev, cap)
        self.first = np.arange(0, B, 2, dtype=np.int32)
        self.second = self.first + 1
        self.counts_all = torch.zeros(B * world, dtype=torch.int32, device=cdev)
        self.snaps = [torch.zeros(B, dtype=torch.int32, device=cdev) for _ in range(2)]
        self.pending = None
        self.nstep = 0
        self.ngathered = 0      # batches whose counts have been gathered
        self.ngather_calls = 0

    def finish_gather(self):
        if self.pending is not None:
            self.pending.wait()
            self.pending = None

    def gather_counts(self, k):
        self.finish_gather()
        snap = self.snaps[k & 1]
        snap.copy_(self.outs[k % self.nout]["n"])  # batch k has been waited for: its counts are final.  (The copy runs on torch's
        # stream; the binding orders the context's streams behind it before the next batch rewrites that array: orbx_order_after.)
        self.pending = self.dist.all_gather_into_tensor(self.counts_all, snap, async_op=True)
        self.ngather_calls += 1

    def step(self):
        # one call = the whole hot path of the batch: extraction of B frames and SearchForInitialization of the B / 2
        # consecutive pairs, issued behind the previous batches (at most `nout` in flight)
        k, B = self.nstep, self.B
        o = self.outs[k % self.nout]
        self.ext.extract_match_batch_device_async(self.d_imgs[k % len(self.d_imgs)], B, W, H, W, W * H, o["k"], o["d"], o["n"], self.first,
                                                  self.second, (0, W, 0, H), o["m"], o["nm"], None, 100, 0.9, True, self.cap)
        self.nstep = k + 1
        if self.coll and k + 1 - self.ngathered >= self.nout:  # as many in flight as there are output sets: wait for the oldest
            self.ext.wait_one()                                    # (batch ngathered) and gather its counts
            self.gather_counts(self.ngathered)
            self.ngathered += 1

    def barrier(self):
        import torch
        self.ext.wait()  # every batch issued so far is complete
        while self.coll and self.ngathered < self.nstep:  # the counts of the last batches (the earlier ones were gathered in step())
            self.gather_counts(self.ngathered)
            self.ngathered += 1
        self.finish_gather()
        torch.cuda.synchronize()
        if self.world > 1:
            self.dist.barrier()
        torch.cuda.synchronize()

    def timed_region(self, steps, cdev):
        """Exactly `steps` steps between two barriers, the maximum over the ranks (the task contract's protocol)."""
        import torch
        self.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        self.barrier()
        dt = time.perf_counter() - t0
        if self.world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=cdev)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    def release(self):
        self.d_imgs = None
        self.outs = None


class Skipped(Exception):
    """A side measurement that was not asked for (a flag, N > 1): recorded in the line, not a failure."""


def run_side(out, name, fn, failures):
    """One of the figures behind the headline (single_frame, host_pipeline, other_configs).  It never keeps the JSON line from being
    printed -- but a figure that CRASHES is a failure of the run, not a footnote: its error goes into the line
    and into `failures`, which makes `all_checked` false and the exit code non-zero (final_status)."""
    try:
        out[name] = fn()
    except Skipped as ex:
        out[name] = {"skipped": str(ex)[:300]}
    except Exception as ex:
        out[name] = {"error": "%s: %s" % (type(ex).__name__, str(ex)[:300])}
        failures.append(name)
    return out[name]


def final_status(check_ok, failures):
    """(all_checked, exit code) of the run: a mismatch against the oracle anywhere, or a side measurement that raised, is exit 3."""
    ok = (bool(check_ok) if check_ok is not None else False) and not failures
    bad = check_ok is False or bool(failures)
    return ok, (3 if bad else 0)


def main():
    exit_code = 0
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps in all, split over the timed regions")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="frames per GPU per step")
    ap.add_argument("--regions", type=int, default=5, help="back-to-back timed regions the --steps steps are split into (fewer when a "
                    "region would hold less than %d steps); `value` is the median region's rate" % MIN_REGION_STEPS)
    ap.add_argument("--depth", type=int, default=4, help="pipeline depth of the stream-ordered call (orbx_set_pipeline_depth): whole "
                    "batches on this many lanes; 0 = the two-half-batches mode")
    ap.add_argument("--prime", type=int, default=16, help="untimed batches right after the context is created (initialisation of "
                    "every lane), before the W warmup steps")
    ap.add_argument("--input-sets", type=int, default=4, help="distinct input sets the steps rotate through (default 4 = 315 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-single-frame", action="store_true", help="skip the one-frame-per-call figure (profiling passes: keeps every launch of a kernel the same size)")
    ap.add_argument("--cpu-reps", type=int, default=30, help="timed repetitions per thread of the CPU baseline (>= 30 by protocol)")
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"),
                    help="torch.distributed backend for N > 1 (nccl = RCCL over xGMI; gloo only to rehearse the N > 1 path)")
    ap.add_argument("--one-device", action="store_true", help="rehearsal: every rank uses cuda:0 (with --backend gloo)")
    ap.add_argument("--no-check", action="store_true", help="skip the oracle comparison of the last batch (after the timed regions)")
    ap.add_argument("--force-collective", action="store_true", help="N = 1: initialise the nccl (RCCL) process group with one rank and "
                    "all_gather the keypoint counts every step, as the N > 1 runs do (exercises the RCCL path on a one-GPU box)")
    ap.add_argument("--no-host-pipeline", action="store_true", help="skip the host-frame pipeline figure (orbx_extract_match_batch_host_async)")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the BASELINE configurations 3 and 5 and the 2000 x 2000 "
                    "brute-force match that follow the headline (N = 1, outside its timed regions)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed "
                    "(rank 0's batch: keypoints, descriptors, counts, matches12, nmatches) as DIR/<name>.npy, float32 / float64, at "
                    "most 64 MB (a fixed seeded sample of pairs beyond that)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # before torch is imported or anything touches the GPU: start the ranks as fresh child processes (never an exec)
        raise SystemExit(self_launch(args.gpus))

    import torch
    import torch.distributed as dist
    import orb_slam_tracking_amd as orbx
    from orb_slam_tracking_amd import sharding, synth

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE is %d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    if args.one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    coll = world > 1 or args.force_collective  # the counts are all-gathered every step
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
    elif args.force_collective:
        import socket
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.backend == "nccl":  # a one-rank RCCL communicator: ncclCommInitRank, all_gather, destroy -- on one GPU
            dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=dev)
        else:
            dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    cdev = dev if args.backend == "nccl" else torch.device("cpu")  # where the collectives' tensors live

    B = args.batch
    cap = 1000
    # this rank's shard of the global batch (frame i -> rank i // B, contiguous blocks; pairs never straddle ranks)
    lo, hi = sharding.shard_range(B * world, world, rank)
    # four input sets: the frames, and their vertical / horizontal / both mirror images (pairs stay pairs of one scene); a fifth
    # (experiments: a rotation length that no lane count divides) is the first in reverse order.  tests/test_gpu_headline.py runs
    # exactly these sets through exactly this call sequence against the oracle.
    host_sets = synth.bench_input_sets(hi - lo, W, H, 1000 + lo // 2, args.input_sets)
    frames = host_sets[0]
    nsets = len(host_sets)
    # pipeline depth: whole batches on `depth` lanes of the context (orbx_set_pipeline_depth); 0 = two half batches on two streams
    depth = args.depth
    nout = max(2, depth)

    # (the caller's arrays first, the context behind them -- the order of rounds 1 - 5.  Round 6's first refactoring created the context
    # first: the same kernels then ran 1 % slower in the headline, and the configurations measured AFTER it, on fresh allocations in
    # the holes the headline had left, 8 - 14 % slower on their lanes -- tools/exp_bench_flow.sh; where the driver's allocations fall
    # matters on this part)
    d_sets = [torch.from_numpy(s).to(dev) for s in host_sets]
    d_outs = Runner.make_outs(B, nout, dev, cap)
    ext = orbx.ORBextractor(*PARAMS, max_width=W, max_height=H, max_batch=B, device=local_rank)
    if depth > 0:
        ext.set_pipeline_depth(depth)
    run = Runner(ext, d_sets, B, nout, world, coll, cdev, dev, dist if coll else None, cap, outs=d_outs)
    del d_sets, d_outs
    step, barrier = run.step, run.barrier

    # context initialisation, before the contract's W warmup steps: every lane runs its first batches (tables, selection-instance
    # hint, matcher expectation, clocks) -- the driver's W = 5 would otherwise end before the fourth lane has seen its second batch
    for _ in range(args.prime):
        step()
    barrier()

    # warmup: every stage bracketed by events -> per-stage device times and the dominant kernel
    ext.profile_enable(True)
    stage_steps = args.warmup
    for i in range(args.warmup):
        if i == 1:  # the first warmup step (cold caches, clocks ramping) stays out of the stage table when there are more
            barrier()
            stage_steps = args.warmup - 1
        if i <= 1:
            ext.profile_reset()
        step()
    barrier()
    stage_prof = ext.profile_get() if args.warmup > 0 else None
    if stage_prof is not None:
        dom = max(("pyramid", "fast", "describe"), key=lambda s: stage_prof[s][0])
        ext.profile_stages([dom])  # timed steps: events around the dominant kernel only (each pair costs stream time)
    ext.profile_reset()

    # exactly --steps timed steps, as back-to-back regions; `value` is the MEDIAN region's rate.  On this pool the GPU pauses for
    # ~10 ms about every 100 ms whatever runs on it (tools/hiccup.py; a plain torch matmul loop shows the same), so one short
    # region is hit with probability ~1/4 and then reads 35 % low; the median of several regions is not.
    reg_steps = region_steps(args.steps, args.regions)
    dt_first = run.timed_region(reg_steps[0], cdev)
    prof = ext.profile_get()             # (events of the first region)
    region_dts = [dt_first] + [run.timed_region(n_, cdev) for n_ in reg_steps[1:]]
    step_s = float(np.median([t / n_ for t, n_ in zip(region_dts, reg_steps)]))  # seconds per step, median region
    ext.profile_enable(False)
    if stage_prof is None:
        stage_prof, stage_steps = prof, reg_steps[0]
    last = run.nstep - 1
    d_n, d_nm = run.outs[last % nout]["n"], run.outs[last % nout]["nm"]
    gathered_ok = None
    if coll:  # the last all_gather's result: every rank's block holds the counts of that rank's last batch
        ca = run.counts_all.cpu().numpy()
        gathered_ok = bool(run.ngather_calls > 0 and (ca > 0).all() and np.array_equal(ca[lo:hi], d_n.cpu().numpy()))

    # not timed: the last batch's complete output set against the CPU oracle -- every rank its own shard, the
    # verdict reduced to rank 0; a mismatch makes the process exit non-zero behind the JSON line
    got = None
    if args.dump_outputs and rank == 0:  # (not timed) what the last timed step computed, before anything else runs on the outputs
        got = {k_: v.cpu().numpy() for k_, v in run.outs[last % nout].items()}
        dumped = dump_outputs(args.dump_outputs, got, B, cap)
    check_ok, check_what = None, "skipped (--no-check)"
    if not args.no_check:
        got = got if got is not None else {k_: v.cpu().numpy() for k_, v in run.outs[last % nout].items()}
        try:  # (a rank whose checker cannot run must still reach the all_reduce below: ADVICE r04)
            check_ok, check_what = oracle_check(host_sets[last % nsets], got, max(1, cpu_share() // max(world, 1)))
        except Exception as ex:
            check_ok, check_what = False, "the checker failed on rank %d: %s" % (rank, str(ex)[:200])
        if world > 1:
            t = torch.tensor([1 if check_ok else 0], dtype=torch.int32, device=cdev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            if check_ok and int(t.item()) == 0:
                check_ok, check_what = False, "MISMATCH on another rank"
            elif check_ok:
                check_what = "every rank: " + check_what
    # N > 1: BASELINE config 4 AS WRITTEN beside the weak-scaling `value` -- ONE batch of 256 frames over the N ranks, 256 / N frames
    # (and their pairs) per rank and step, same protocol (barrier, exactly --steps steps, barrier, the maximum over the ranks; the
    # median of three regions), counts all-gathered every step
    c4w = None
    B4 = max(2, (256 // world) // 2 * 2)
    if world > 1 and B4 > B:  # (a rehearsal with small --batch: this rank holds fewer frames than its share of the 256)
        c4w = {"skipped": "--batch %d is less than this configuration's %d frames per rank" % (B, B4), "gathered_counts_ok": True}
    elif world > 1:
        run4 = Runner(ext, [t[:B4] for t in run.d_imgs], B4, nout, world, coll, cdev, dev, dist, cap)
        for _ in range(2 * nout):
            run4.step()
        dt4 = sorted(run4.timed_region(args.steps, cdev) for _ in range(3))[1]
        ca4 = run4.counts_all.cpu().numpy()
        lo4, hi4 = sharding.shard_range(B4 * world, world, rank)
        ok4 = bool(run4.ngather_calls > 0 and (ca4 > 0).all() and
                   np.array_equal(ca4[lo4:hi4], run4.outs[(run4.nstep - 1) % nout]["n"].cpu().numpy()))
        t = torch.tensor([1 if ok4 else 0], dtype=torch.int32, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        c4w = {"workload": "ONE batch of %d frames 640x480 / 1000 features over %d ranks: %d frames + %d consecutive-pair matches per rank "
                           "and step, counts all-gathered" % (B4 * world, world, B4, B4 // 2),
               "frames_per_step": B4 * world, "frames_per_rank": B4, "frames_per_s": B4 * world * args.steps / dt4,
               "ms_per_step": dt4 / args.steps * 1e3, "steps": args.steps, "scaling": "strong (the batch is fixed, the ranks share it)",
               "gathered_counts_ok": bool(int(t.item()) == 1)}
        run4.release()
    if rank == 0:
        n_kp = float(d_n.float().mean().item())
        nm_mean = float(d_nm.float().mean().item())
        ab = algorithmic_bytes(W, H, n_kp)
        # dominant kernel = stage with the largest device time per step (warmup steps, every stage bracketed by events);
        # its launch duration below is measured over the first timed region (events on the context's own streams)
        dev_ms = {s: stage_prof[s][0] / stage_steps for s in ("pyramid", "fast", "describe", "match")}
        kern = max(("pyramid", "fast", "describe"), key=lambda s: dev_ms[s])
        launches = max(prof[kern][1], 1)
        avg_launch_ms = prof[kern][0] / launches
        frames_per_launch = B * reg_steps[0] / launches
        kname = KERNEL_OF[kern]
        pmc, pmc_file = load_pmc()
        pk = (pmc or {}).get("per_frame", {}).get(kname)
        secs = avg_launch_ms * 1e-3
        roof = {"bound": "valu", "kernel": kname, "unit": "T SIMD-issue-cycles/s", "peak": VALU_PEAK_SIMD_CYCLES / 1e12,
                "avg_launch_ms": avg_launch_ms, "frames_per_launch": frames_per_launch,
                "formula": "achieved = VALU issue cycles per frame [4 x (SQ_ACTIVE_INST_VALU - SQ_ACTIVE_INST_VALU2), %s] x frames per "
                           "launch / launch duration [HIP events, live]; peak = 256 CUs x 4 SIMDs x 2.4 GHz" % (pmc_file or "no PMC file")}
        roof["pmc_file"] = pmc_file
        roof["pmc_stale"] = None if not pmc else (pmc.get("kernel_sources_sha16") != kernel_sources_sha16())
        if pk and secs > 0:
            roof["achieved"] = pk["valu_issue_cycles"] * frames_per_launch / secs / 1e12
            roof["frac"] = roof["achieved"] / roof["peak"]
            roof["valu_wave_instr_per_s"] = pk["valu_instr"] * frames_per_launch / secs
            roof["traffic"] = (pk["fetch_bytes"] + pk["write_bytes"]) * frames_per_launch  # HBM bytes per launch, counters
            # the kernel alone on the chip (the PMC file's --stats pass with ORBX_NO_SPLIT=1): in the timed steps above it
            # shares the chip with the other half-batch chain's kernels, so its live share is about half of this
            if "avg_launch_us_single_stream" in pk:
                roof["single_stream"] = {"avg_launch_ms": pk["avg_launch_us_single_stream"] / 1e3, "frames_per_launch": pmc["frames_per_launch"],
                                         "frac": pk.get("valu_frac_single_stream")}
            # the whole step: VALU issue cycles of every kernel of the path per frame x frames / step time / peak
            tot_cycles = sum(v["valu_issue_cycles"] for v in pmc["per_frame"].values())
            roof["step_valu_frac"] = tot_cycles * B / step_s / VALU_PEAK_SIMD_CYCLES
        else:
            roof["achieved"] = roof["frac"] = roof["traffic"] = None
        # secondary: the HBM view of the same launch (algorithmic bytes of SURVEY 8(d) and counter bytes against 8 TB/s)
        bytes_per_launch = ab[kern] * frames_per_launch
        roof["hbm"] = {"algorithmic_bytes_per_launch": bytes_per_launch, "algorithmic_GBs": bytes_per_launch / secs / 1e9 if secs > 0 else None,
                       "algorithmic_frac": bytes_per_launch / secs / 1e9 / HBM_PEAK_GBS if secs > 0 else None,
                       "counter_GBs": roof["traffic"] / secs / 1e9 if roof.get("traffic") and secs > 0 else None,
                       "counter_frac": roof["traffic"] / secs / 1e9 / HBM_PEAK_GBS if roof.get("traffic") and secs > 0 else None,
                       "peak_GBs": HBM_PEAK_GBS,
                       "whole_path_algorithmic_GBs": ab["total"] * B * world / step_s / 1e9}
        # the other extraction kernels, from the warmup steps' events (same formulas), for comparison
        others = {}
        for s2 in ("pyramid", "fast", "describe"):
            if s2 == kern or stage_prof[s2][1] == 0:
                continue
            l2 = stage_prof[s2][1]
            ms2 = stage_prof[s2][0] / l2
            fpl = B * stage_steps / l2
            p2 = (pmc or {}).get("per_frame", {}).get(KERNEL_OF[s2])
            ent = {"avg_launch_ms": ms2, "hbm_algorithmic_frac": ab[s2] * fpl / (ms2 * 1e-3) / 1e9 / HBM_PEAK_GBS if ms2 > 0 else None}
            if p2 and ms2 > 0:
                ent["valu_frac"] = p2["valu_issue_cycles"] * fpl / (ms2 * 1e-3) / VALU_PEAK_SIMD_CYCLES
                ent["hbm_counter_frac"] = (p2["fetch_bytes"] + p2["write_bytes"]) * fpl / (ms2 * 1e-3) / 1e9 / HBM_PEAK_GBS
            others[KERNEL_OF[s2]] = ent
        rates = sorted(B * world * n_ / t for t, n_ in zip(region_dts, reg_steps))
        out = {
            "metric": "frames/sec (extract+match, 1000 feat, 640x480)",
            "value": B * world / step_s,
            "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": step_s * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8", "data": "synthetic",
            "config": {"workload": "640x480 gray frames, 1000 features, 8 levels, FAST 20/7; %d frames per GPU per step resident in "
                                   "HBM (4 input sets rotating, 315 MB per GPU), %d consecutive-pair SearchForInitialization "
                                   "(window 100, ratio 0.9)" % (B, B // 2),
                       "frames_per_gpu": B, "pairs_per_gpu": B // 2, "mean_keypoints": n_kp, "mean_nmatches": nm_mean,
                       "pipeline_depth": depth, "prime_steps": args.prime,
                       "rccl_ranks": (dist.get_world_size() if coll and args.backend == "nccl" else (0 if world > 1 else 1)),
                       "collective": ({"backend": args.backend, "world_size": dist.get_world_size(), "all_gathers": run.ngather_calls,
                                       "gathered_counts_ok": gathered_ok} if coll else None),
                       "parallelism": "frames sharded per GPU (%d ranks), RCCL all_gather of keypoint counts" % world},
            "spread": {"regions": len(region_dts), "steps_per_region": reg_steps, "median": float(np.median(rates)),
                       "min": rates[0], "max": rates[-1], "first_region": B * world * reg_steps[0] / dt_first,
                       "note": "`value` is the median region (the --steps timed steps split into back-to-back regions); the GPUs of "
                               "this pool pause ~10 ms every ~100 ms, which a single short region either catches or not",
                       "in_order": [round(B * world * n_ / t) for t, n_ in zip(region_dts, reg_steps)]},
            "roofline": roof,
            "roofline_other_kernels": others,
            "stage_ms_per_step": {s: stage_prof[s][0] / stage_steps for s in stage_prof},
            "stage_ms_source": "warmup steps, every stage bracketed by HIP events (sums over the lanes / half-batch streams); the "
                               "timed steps bracket only the dominant kernel",
        }
        if args.dump_outputs:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        out["checked"] = bool(check_ok) if check_ok is not None else False
        out["check"] = check_what
        if c4w is not None:
            out["config4_as_written"] = c4w
            if not c4w["gathered_counts_ok"]:
                check_ok = False
        failures = []  # side measurements that raised (run_side)
        # second figure: the call the reference actually makes -- one frame per call through the host API
        # (Frame.cpp:58-60: host image in, keypoints + descriptors back on the host), and one SearchForInitialization per call
        def single_frame():
            if args.no_single_frame or world > 1:
                raise Skipped("--no-single-frame" if args.no_single_frame else "N > 1: an N = 1 figure")
            e1 = orbx.ORBextractor(*PARAMS, max_width=W, max_height=H, max_batch=1, device=local_rank)
            fa, fb = orbx.Frame(frames[0], 0.0, e1), orbx.Frame(frames[1], 1.0, e1)
            mt = orbx.ORBmatcher(0.9, True)
            for _ in range(10):
                e1(frames[0]); mt.SearchForInitialization(fa, fb, 100)
            nrep = 200
            t0 = time.perf_counter()
            for _ in range(nrep):
                e1(frames[0])
            t1 = time.perf_counter()
            for _ in range(nrep):
                mt.SearchForInitialization(fa, fb, 100)
            t2 = time.perf_counter()
            sf = {"extract_ms_per_frame": (t1 - t0) / nrep * 1e3, "match_ms_per_pair": (t2 - t1) / nrep * 1e3,
                  "frames_per_s_extract_only": nrep / (t1 - t0),
                  "note": "synchronous host-buffer calls, one 640x480 frame (orbx_extract) / one pair (orbx_match_init) per call, "
                          "through the ctypes binding; cpp_shim: the same two calls as the reference makes them "
                          "(Frame.cpp:58-60, demo_initialization.cpp:105-108) through include/orbx_shim.hpp from C++ "
                          "(tests/cpp/shim_latency.cpp, medians of 300 calls)"}
            e1.close()
            # the drop-in call from C++: g++ builds the small harness against liborbx.so
            import subprocess
            import tempfile
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from test_host import build_shim_latency
            with tempfile.TemporaryDirectory() as td:
                exe = build_shim_latency(orbx.lib_path(), td)
                pa, pb = os.path.join(td, "a.raw"), os.path.join(td, "b.raw")
                frames[0].tofile(pa)
                frames[1].tofile(pb)
                r = subprocess.run([exe, str(W), str(H), pa, pb, "1000", "20", "7", "300"], stdout=subprocess.PIPE,
                                   stderr=subprocess.PIPE, text=True, timeout=120)
                if r.returncode != 0:
                    raise RuntimeError("shim_latency exited %d: %s" % (r.returncode, r.stderr[-200:]))
                sf["cpp_shim"] = json.loads(r.stdout.strip().splitlines()[-1])
            return sf
        run_side(out, "single_frame", single_frame, failures)
        # third figure (SURVEY 8(e) "report host-side time separately"): the same workload with the frames in HOST
        # memory -- what the reference's call site hands over (Frame.cpp:58-60) -- through the stream-ordered host call: page-locked
        # input sets, results into page-locked arrays, `depth` batches in flight; beside it the box's own H2D rate (the same
        # 78.6 MB through hipMemcpyAsync).  Never `value`.
        hp_state = {"ok": None}

        def host_pipeline():
            if world > 1 or args.no_host_pipeline or args.no_other_configs:  # (the profiling passes run neither)
                raise Skipped("N > 1" if world > 1 else "--no-host-pipeline / --no-other-configs")
            hp_depth = max(depth, 2)
            if hp_depth != depth:
                ext.set_pipeline_depth(hp_depth)
            h_sets = [torch.from_numpy(s).pin_memory() for s in host_sets]
            h_outs = [dict(k=torch.zeros(B * cap * 28, dtype=torch.uint8).pin_memory(), d=torch.zeros(B * cap * 32, dtype=torch.uint8).pin_memory(),
                           n=torch.zeros(B, dtype=torch.int32).pin_memory(), m=torch.zeros((B // 2) * cap, dtype=torch.int32).pin_memory(),
                           nm=torch.zeros(B // 2, dtype=torch.int32).pin_memory()) for _ in range(hp_depth)]
            dst = torch.empty_like(run.d_imgs[0])
            e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(3):
                dst.copy_(h_sets[0], non_blocking=True)
            torch.cuda.synchronize()
            ncopy = 20
            e0.record()
            for i in range(ncopy):
                dst.copy_(h_sets[i % nsets], non_blocking=True)
            e1_.record()
            torch.cuda.synchronize()
            h2d_peak = ncopy * B * W * H / (e0.elapsed_time(e1_) * 1e-3) / 1e9

            def hstep(i):
                o = h_outs[i % hp_depth]
                ext.extract_match_batch_host_async(h_sets[i % nsets], B, W, H, W, W * H, o["k"], o["d"], o["n"], run.first, run.second,
                                                   (0, W, 0, H), o["m"], o["nm"], None, 100, 0.9, True, cap)
            for i in range(2 * hp_depth):
                hstep(i)
            ext.wait()
            nh = max(80, 8 * hp_depth)
            ths = []
            for _ in range(3):  # (three regions of ~0.1 s, the median: this pool's GPUs pause ~10 ms every ~100 ms)
                t0 = time.perf_counter()
                for i in range(nh):
                    hstep(i)
                ext.wait()
                ths.append(time.perf_counter() - t0)
            th = sorted(ths)[1]
            hp_ok, hp_what = None, "skipped (--no-check)"
            if not args.no_check:
                lasth = nh - 1
                hp_ok, hp_what = oracle_check(host_sets[lasth % nsets], {k_: v.numpy() for k_, v in h_outs[lasth % hp_depth].items()}, cpu_share())
            fps = nh * B / th
            res = {"frames_per_s": fps, "ms_per_batch": th / nh * 1e3, "h2d_GBs": fps * W * H / 1e9,
                                    "d2h_GBs": fps * (cap * 60 + 4 + (cap * 4 + 4) / 2) / 1e9,
                                    "measured_pcie_h2d_peak_GBs": h2d_peak, "frac_of_measured_pcie_peak": fps * W * H / 1e9 / h2d_peak,
                                    "batches_in_flight": hp_depth, "checked": bool(hp_ok) if hp_ok is not None else False, "check": hp_what,
                                    "note": "orbx_extract_match_batch_host_async: %d page-locked 640x480 frames up, the kernels, every "
                                            "result array (15.5 MB) back per batch, stream-ordered on %d lanes; peak = the same frames "
                                            "through hipMemcpyAsync alone on this box" % (B, hp_depth)}
            del h_sets, h_outs, dst
            hp_state["ok"] = hp_ok
            return res
        run_side(out, "host_pipeline", host_pipeline, failures)
        if hp_state["ok"] is False:
            check_ok = False
        # BASELINE configurations 3 and 5 and config 5's 2000 x 2000 brute-force match: rates of the same
        # library right behind the headline (before the CPU legs: a GPU that has idled through them starts its next kernels at low
        # clocks), outside the timed regions, each compared with the CPU oracle on one pair (not timed)
        def other_configs():
            if world > 1 or args.no_other_configs:
                raise Skipped("N > 1" if world > 1 else "--no-other-configs")
            ext.close()
            run.release()
            torch.cuda.empty_cache()
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_config as BC
            oc = {}
            for cfg in ("c3", "c5"):
                r = BC.measure(cfg, steps=20, depth=3, device=local_rank)
                oc[cfg] = {"workload": "%d frames %dx%d / %d features + %d consecutive-pair matches (window %d) per call" % (
                               r["batch"], r["frame"][0], r["frame"][1], r["nfeatures"], r["batch"] // 2, r["window"]),
                           "frames_per_s_synchronous": r["sync"]["frames_per_s"], "frames_per_s_on_lanes": r["lanes"]["frames_per_s"],
                           "lanes": r["lanes"]["depth"], "ms_per_batch_synchronous": r["sync"]["ms_per_batch"],
                           "stage_ms": r["sync"]["stage_ms"], "dominant_stage": r["sync"]["dominant_stage"],
                           "hbm_algorithmic_frac_synchronous": r["sync"]["algorithmic_frac_of_8TBs"],
                           "hbm_algorithmic_frac_on_lanes": r["lanes"]["algorithmic_frac_of_8TBs"],
                           "mean_keypoints": r["sync"]["mean_keypoints"], "mean_nmatches": r["sync"]["mean_nmatches"],
                           "roofline": config_roofline(cfg, r["frame"][0], r["frame"][1], r["sync"]["stage_ms"], r["sync"]["launch"],
                                                       r["sync"]["mean_keypoints"]),
                           "checked": BC.check(cfg, device=local_rank)}
            # BASELINE config 4 as written: 256 frames over 8 GPUs = 32 frames + 16 pairs per GPU and step (the
            # headline's weak scaling keeps 256 frames PER GPU)
            # (three lanes: 32-frame batches do 324 k frames/s on three, 300 k on four, 315 k on five, 293 k on six -- round 6)
            r4 = BC.measure("c2", steps=200, depth=3, batch=32, modes=("sync", "lanes"), device=local_rank)
            oc["c4_per_gpu"] = {"workload": "32 frames 640x480 / 1000 features + 16 consecutive-pair matches per call: one GPU's share of "
                                            "BASELINE config 4's 256-frame batch over 8 GPUs",
                                "frames_per_s_synchronous": r4["sync"]["frames_per_s"], "frames_per_s_on_lanes": r4["lanes"]["frames_per_s"],
                                "lanes": r4["lanes"]["depth"], "ms_per_batch_synchronous": r4["sync"]["ms_per_batch"],
                                "ms_per_batch_on_lanes": 32e3 / r4["lanes"]["frames_per_s"], "stage_ms": r4["sync"]["stage_ms"],
                                "checked": BC.check("c2", device=local_rank)}
            bf, bf_data = BC.measure_bf(steps=20, device=local_rank)
            oc["bf_2000x2000"] = {"us_per_2000x2000": bf["ms_per_2000x2000"] * 1e3, "descriptor_pairs_per_s": bf["descriptor_pairs_per_s"],
                                  "frac_of_4.9T_popcount_bound": bf["frac_of_4.9T_pairs_per_s"],
                                  "frac_of_3.3T_bcnt_issue_bound": bf["frac_of_3.3T_pairs_per_s"],
                                  "frac_of_9.8T_mfma_i8_bound": bf["frac_of_9.8T_mfma_i8_pairs_per_s"], "sets_per_call": bf["sets_per_call"],
                                  "nmatches": bf["nmatches"], "checked": BC.check_bf(bf_data)}
            # the call BASELINE config 5 literally names: ONE 2000 x 2000 match per call, its result waited for (too few blocks for
            # the matrix-core kernel: the vector form), and sixteen per call
            bf1, bf1_data = BC.measure_bf(steps=100, device=local_rank, sets=1, sync_each=True)
            bf16, _ = BC.measure_bf(steps=20, device=local_rank, sets=16)
            oc["bf_2000x2000"]["roofline"] = bf_roofline(bf)
            oc["bf_2000x2000"]["single_call_us"] = bf1["ms_per_call"] * 1e3
            oc["bf_2000x2000"]["single_call_device_us"] = bf1["device_ms_per_call"] * 1e3
            oc["bf_2000x2000"]["us_per_2000x2000_at_16_per_call"] = bf16["ms_per_2000x2000"] * 1e3
            oc["bf_2000x2000"]["checked"] = bool(oc["bf_2000x2000"]["checked"] and BC.check_bf(bf1_data))
            return oc
        oc_ = run_side(out, "other_configs", other_configs, failures)
        if "error" not in oc_ and "skipped" not in oc_ and not all(v["checked"] for v in oc_.values()):
            check_ok = False
        if not args.no_cpu_baseline and world == 1:  # (the CPU baseline is an N = 1 figure: rank 0's host cores, one GPU beside it)
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import oracle_lib as O
            cores = cpu_share()
            sample = frames[:2 * min(cores, 16)] if len(frames) >= 2 * min(cores, 16) else frames
            reps = max(args.cpu_reps, 30)

            def stats(r):  # r: [threads, reps, 3] seconds
                tot = r[:, :, 0].ravel() * 1e3
                return {"ms_per_pair_median": float(np.median(tot)), "p10": float(np.percentile(tot, 10)), "p90": float(np.percentile(tot, 90)),
                        "extract_only_ms_median": float(np.median(r[:, :, 1]) * 1e3), "match_only_ms_median": float(np.median(r[:, :, 2]) * 1e3),
                        "frames_per_s": float(r.shape[0] * 2.0 / np.median(r[:, :, 0]))}
            one = stats(O.bench_protocol(PARAMS, sample, 100, 0.9, 1, 5, reps, False))
            allc = stats(O.bench_protocol(PARAMS, sample, 100, 0.9, cores, 5, reps, False))
            try:
                alln = stats(O.bench_protocol(PARAMS, sample, 100, 0.9, cores, 5, reps, True))
            except Exception as e:  # no compiler on the host: the generic build stands alone
                alln = {"error": str(e)[:200]}
            out["cpu_baseline"] = {"value": allc["frames_per_s"], "unit": "frames/s", "cores": cores, "kind": "port",
                                   "sample": "oracle restatement (scalar C++, -O3, one frame pair per pinned thread): per thread 5 warm-ups + "
                                             "%d timed repetitions of extract A + extract B + SearchForInitialization on its own pair of the "
                                             "same 640x480 frames (SURVEY 8(d) protocol); value = threads x 2 frames / median repetition"
                                             % reps,
                                   "all_cores": allc, "one_core": one, "all_cores_march_native": alln}
            out["speedup_vs_cpu_all_cores"] = out["value"] / out["cpu_baseline"]["value"]
        # (the exit code mirrors this field: `checked` is the headline batch alone; a side measurement that raised makes
        # it false as well)
        out["all_checked"], exit_code = final_status(check_ok, failures)
        out["side_failures"] = failures
        print(json.dumps(out))
    if coll:
        dist.destroy_process_group()
    if rank == 0 and exit_code:
        raise SystemExit(exit_code)  # (the line above says what differed or failed)
    if check_ok is False:
        raise SystemExit(3)


if __name__ == "__main__":
    main()
