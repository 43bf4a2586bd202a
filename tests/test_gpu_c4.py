"""BASELINE.json config 4 ("batch of 256 synthetic 640x480 frames sharded per-frame across 8 MI355X, RCCL gather of
keypoints") exercised at its size: 8 contiguous blocks of 32 frames (sharding.shard_range), every block through the fused
device call, the counts through sharding.gather_counts -- on one GPU (all eight blocks), with two ranks sharing the GPU
(gloo), and over RCCL when the box has more than one GPU.  All 256 frames and all 128 pairs are compared with the oracle."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = (1000, 1.2, 8, 20, 7)
W, H, N_FRAMES, CAP, B = 640, 480, 256, 1000, 32


@pytest.fixture(scope="module")
def c4_oracle(oracle):
    """The oracle's results for the 256 frames and the 128 consecutive pairs (a few seconds of CPU)."""
    from orb_slam_tracking_amd import synth
    oe = oracle.Extractor(*PARAMS)
    frames = [synth.synth(W, H, 1000 + i) for i in range(N_FRAMES)]
    ext = [oe(f) for f in frames]
    pairs = [oracle.match_init(ext[2 * p][1], ext[2 * p][2], ext[2 * p + 1][1], ext[2 * p + 1][2], (0, W, 0, H), 100, 0.9, True)
             for p in range(N_FRAMES // 2)]
    return ext, pairs


def _check(files, c4_oracle, orbx):
    ext, pairs = c4_oracle
    counts_exp = np.array([len(e[1]) for e in ext], np.int32)
    seen = set()
    for fn in files:
        z = np.load(fn)
        assert np.array_equal(z["counts_all"], counts_exp), "gathered keypoint counts differ from the oracle (%s)" % fn
        for b in z["blocks"]:
            seen.add(int(b))
            n = z["n%d" % b]
            kk = z["k%d" % b].view(orbx.KEYPOINT_DTYPE).reshape(B, CAP)
            dd = z["d%d" % b].reshape(B, CAP, 32)
            mm = z["m%d" % b].reshape(B // 2, CAP)
            nm = z["nm%d" % b]
            for f in range(B):
                g = b * B + f
                _, ko, do = ext[g]
                assert n[f] == len(ko)
                assert kk[f, :n[f]].tobytes() == ko.tobytes() and np.array_equal(dd[f, :n[f]], do), ("frame", g)
            for p in range(B // 2):
                onm, om12, _ = pairs[b * (B // 2) + p]
                assert nm[p] == onm and np.array_equal(mm[p, :len(om12)], om12), ("pair", b * (B // 2) + p)
    assert seen == set(range(8))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(cmd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=e, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout


def test_config4_one_gpu_all_blocks(orbx, c4_oracle, tmp_path):
    out = str(tmp_path / "c4.npz")
    _run([sys.executable, os.path.join(ROOT, "tests", "c4_worker.py"), "--backend", "none", "--out", out])
    _check([out], c4_oracle, orbx)


def test_config4_two_ranks_sharing_the_gpu_gloo(orbx, c4_oracle, tmp_path):
    """N > 1 on a one-GPU box: two processes (fresh children, started by the launcher before anything touches the GPU), each
    with its own context on cuda:0 and four of the eight blocks; the collective is gloo here."""
    out = str(tmp_path / "c4g.npz")
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "c4_worker.py"), "--backend", "gloo", "--one-device",
          "--out", out])
    _check([out, out + ".rank1.npz"], c4_oracle, orbx)


def test_config4_rccl(orbx, c4_oracle, tmp_path):
    """The configuration as BASELINE.json states it: one rank per GPU, RCCL all_gather of the counts over xGMI.  Needs more
    than one GPU; uses all of them up to 8 (a power of two)."""
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("RCCL needs more than one GPU: this box has %d (the driver's multi-GPU run covers N = 2, 4, 8)" % n)
    world = 8 if n >= 8 else 4 if n >= 4 else 2
    out = str(tmp_path / "c4r.npz")
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
          "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "c4_worker.py"), "--backend", "nccl", "--out", out],
         env={"HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    _check([out] + ["%s.rank%d.npz" % (out, r) for r in range(1, world)], c4_oracle, orbx)


def _bench_line(out):
    import json
    lines = [ln for ln in out.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, out[-3000:]
    return json.loads(lines[0])


def test_bench_starts_its_own_ranks(orbx):
    """`python bench.py --gpus 2`, started plainly (no launcher, as the driver starts it): bench.py spawns its ranks itself before
    anything touches the GPU.  Rehearsal on the one-GPU box: gloo, both ranks on cuda:0.  The line says n_gpus 2, the counts were
    all-gathered and equal the ranks' own, and the last batch equals the oracle."""
    out = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--one-device", "--steps", "5",
                "--warmup", "2", "--prime", "4", "--regions", "1", "--no-cpu-baseline", "--no-single-frame"])
    d = _bench_line(out)
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["scaling"] == "weak" and d["value"] > 0
    assert d["checked"] is True, d["check"]
    c = d["config"]["collective"]
    assert c["world_size"] == 2 and c["all_gathers"] >= 5 and c["gathered_counts_ok"] is True
    assert d["config"]["rccl_ranks"] == 0  # gloo rehearsal: RCCL did not run, and the line says so


def test_bench_four_ranks_config4_as_written(orbx):
    """The launcher, the shard ranges and the all-gather at world size 4 (gloo rehearsal, every rank on cuda:0, small batches), and
    the N > 1 line's second figure: BASELINE config 4 AS WRITTEN -- one batch of 256 frames over the ranks, 64 per rank and step --
    beside the weak-scaling `value`.  (VERDICT r05 item 7 asked for 8 children on the one GPU; this pool's process guard allows six
    processes on a card, and the test process is one of them: four fresh children is what a one-GPU box can hold.)"""
    out = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--backend", "gloo", "--one-device", "--batch", "64",
                "--steps", "4", "--warmup", "2", "--prime", "4", "--regions", "1", "--no-cpu-baseline", "--no-single-frame"])
    d = _bench_line(out)
    assert d["n_gpus"] == 4 and d["steps"] == 4 and d["scaling"] == "weak" and d["value"] > 0
    assert d["checked"] is True and d["all_checked"] is True and d["side_failures"] == [], d["check"]
    c = d["config"]["collective"]
    assert c["world_size"] == 4 and c["all_gathers"] >= 4 and c["gathered_counts_ok"] is True
    c4 = d["config4_as_written"]
    assert c4["frames_per_step"] == 256 and c4["frames_per_rank"] == 64 and c4["gathered_counts_ok"] is True and c4["frames_per_s"] > 0


def test_bench_rccl_ranks(orbx):
    """The same over RCCL, one rank per GPU, whenever the box has more than one."""
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("RCCL needs more than one GPU: this box has %d (the driver's multi-GPU run covers N = 2, 4, 8)" % n)
    world = 8 if n >= 8 else 4 if n >= 4 else 2
    out = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "20", "--warmup", "3", "--regions", "1",
                "--no-cpu-baseline", "--no-single-frame"])
    d = _bench_line(out)
    assert d["n_gpus"] == world and d["checked"] is True and d["config"]["rccl_ranks"] == world
    assert d["config"]["collective"]["gathered_counts_ok"] is True


def _multi_run(orbx, devices, n_frames, c4_oracle):
    """orbx_multi_* (the C ABI a C++ host uses) on `devices`: blocks resident per device, fused extract + match per block, counts
    all-gathered (RCCL when more than one device); everything against the oracle."""
    import ctypes
    import torch
    from orb_slam_tracking_amd import synth
    torch.cuda.init()  # torch's bundled HIP runtime first: a process that initialises the system's copy (liborbx.so) before it
    # leaves torch without devices (two libamdhip64 builds, one process); the other GPU tests get this order from their fixtures
    L = orbx.lib()
    ext, pairs = c4_oracle
    p = orbx._Params(*PARAMS)
    h = ctypes.c_void_p(0)
    devs = (ctypes.c_int * len(devices))(*devices)
    nd = len(devices)
    per = -(-(-(-n_frames // 2) // nd)) * 2  # block size = shard_range's
    r = L.orbx_multi_create(ctypes.byref(p), nd, devs, W, H, per, ctypes.byref(h))
    assert r == 0, r
    try:
        assert L.orbx_multi_size(h) == nd and L.orbx_multi_ctx(h, 0)
        vp = ctypes.c_void_p
        arrs = {k: [] for k in "ikdnmq"}
        blocks = []
        for i, dv in enumerate(devices):
            lo, hi = ctypes.c_int(0), ctypes.c_int(0)
            L.orbx_multi_shard_range(n_frames, nd, i, ctypes.byref(lo), ctypes.byref(hi))
            blocks.append((lo.value, hi.value))
            nb = max(hi.value - lo.value, 1)
            dev = torch.device("cuda", dv)
            fr = np.stack([synth.synth(W, H, 1000 + g) for g in range(lo.value, hi.value)]) if hi.value > lo.value else np.zeros((1, H, W), np.uint8)
            arrs["i"].append(torch.from_numpy(fr).to(dev))
            arrs["k"].append(torch.zeros(nb * CAP * 28, dtype=torch.uint8, device=dev))
            arrs["d"].append(torch.zeros(nb * CAP * 32, dtype=torch.uint8, device=dev))
            arrs["n"].append(torch.zeros(nb, dtype=torch.int32, device=dev))
            arrs["m"].append(torch.zeros(max(nb // 2, 1) * CAP, dtype=torch.int32, device=dev))
            arrs["q"].append(torch.zeros(max(nb // 2, 1), dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        ptrs = {k: (vp * nd)(*[t.data_ptr() for t in v]) for k, v in arrs.items()}
        b = orbx._Bounds(0, W, 0, H)
        counts = np.full(n_frames, -7, np.int32)
        r = L.orbx_multi_extract_match_batch_device(h, n_frames, ptrs["i"], W, H, W, W * H, ptrs["k"], ptrs["d"], CAP, ptrs["n"], ctypes.byref(b),
                                                    100, 0.9, 1, ptrs["m"], ptrs["q"], counts.ctypes.data)
        assert r == 0, (r, L.orbx_multi_last_error(h))
        assert np.array_equal(counts, np.array([len(ext[g][1]) for g in range(n_frames)], np.int32))
        for i, (lo, hi) in enumerate(blocks):
            nb = hi - lo
            if nb == 0:
                continue
            n = arrs["n"][i].cpu().numpy()
            kk = arrs["k"][i].cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(nb, CAP)
            dd = arrs["d"][i].cpu().numpy().reshape(nb, CAP, 32)
            mm = arrs["m"][i].cpu().numpy().reshape(-1, CAP)
            nm = arrs["q"][i].cpu().numpy()
            for f in range(nb):
                _, ko, do = ext[lo + f]
                assert n[f] == len(ko) and kk[f, :n[f]].tobytes() == ko.tobytes() and np.array_equal(dd[f, :n[f]], do)
            for pp in range(nb // 2):
                onm, om12, _ = pairs[(lo // 2) + pp]
                assert nm[pp] == onm and np.array_equal(mm[pp, :len(om12)], om12)
    finally:
        L.orbx_multi_destroy(h)


def test_multi_c_abi_one_device(orbx, c4_oracle):
    """orbx_multi_create / orbx_multi_extract_match_batch_device with one device: the same entry points a C++ host uses for
    eight (no collective needed for one; duplicate device ids are refused)."""
    import ctypes
    import torch
    torch.cuda.init()
    _multi_run(orbx, [0], 64, c4_oracle)
    _multi_run(orbx, [0], 7, c4_oracle)  # odd count: the last frame has no partner
    L = orbx.lib()
    p = orbx._Params(*PARAMS)
    h = ctypes.c_void_p(0)
    assert L.orbx_multi_create(ctypes.byref(p), 2, (ctypes.c_int * 2)(0, 0), W, H, 32, ctypes.byref(h)) == orbx.E_BADARG


def _multi_async_run(orbx, devices, c4_oracle, depth, nbatch=5, n_frames=64):
    """orbx_multi_*_async: `nbatch` batches of `n_frames` frames (batch j = frames [j * n_frames, (j + 1) * n_frames) of config 4),
    as many in flight as the lanes take, every batch's blocks, pairs and gathered counts against the oracle."""
    import ctypes
    import torch
    from orb_slam_tracking_amd import synth
    ext, pairs = c4_oracle
    L = orbx.lib()
    p = orbx._Params(*PARAMS)
    h = ctypes.c_void_p(0)
    nd = len(devices)
    devs = (ctypes.c_int * nd)(*devices)
    per = -(-(-(-n_frames // 2) // nd)) * 2
    assert L.orbx_multi_create(ctypes.byref(p), nd, devs, W, H, per, ctypes.byref(h)) == 0
    try:
        assert L.orbx_multi_set_pipeline_depth(h, depth) == 0
        nfl = max(depth, 2)  # batches in flight -> output sets
        vp = ctypes.c_void_p
        blocks = []
        for i in range(nd):
            lo, hi = ctypes.c_int(0), ctypes.c_int(0)
            L.orbx_multi_shard_range(n_frames, nd, i, ctypes.byref(lo), ctypes.byref(hi))
            blocks.append((lo.value, hi.value))
        imgs = []  # [batch][device]
        for j in range(nbatch):
            imgs.append([torch.from_numpy(np.stack([synth.synth(W, H, 1000 + j * n_frames + g) for g in range(lo, hi)])).to(torch.device("cuda", dv))
                         for dv, (lo, hi) in zip(devices, blocks)])
        sets = []
        for _ in range(nfl):
            a = {k: [] for k in "kdnmq"}
            for dv, (lo, hi) in zip(devices, blocks):
                nb, dev = hi - lo, torch.device("cuda", dv)
                a["k"].append(torch.zeros(nb * CAP * 28, dtype=torch.uint8, device=dev))
                a["d"].append(torch.zeros(nb * CAP * 32, dtype=torch.uint8, device=dev))
                a["n"].append(torch.zeros(nb, dtype=torch.int32, device=dev))
                a["m"].append(torch.zeros(max(nb // 2, 1) * CAP, dtype=torch.int32, device=dev))
                a["q"].append(torch.zeros(max(nb // 2, 1), dtype=torch.int32, device=dev))
            a["counts"] = np.full(n_frames, -7, np.int32)
            a["ptrs"] = {k: (vp * nd)(*[t.data_ptr() for t in a[k]]) for k in "kdnmq"}
            sets.append(a)
        torch.cuda.synchronize()
        b = orbx._Bounds(0, W, 0, H)

        def check(j, a):
            g0 = j * n_frames
            assert np.array_equal(a["counts"], np.array([len(ext[g0 + g][1]) for g in range(n_frames)], np.int32)), j
            for i, (lo, hi) in enumerate(blocks):
                nb = hi - lo
                n = a["n"][i].cpu().numpy()
                kk = a["k"][i].cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(nb, CAP)
                dd = a["d"][i].cpu().numpy().reshape(nb, CAP, 32)
                mm = a["m"][i].cpu().numpy().reshape(-1, CAP)
                nm = a["q"][i].cpu().numpy()
                for f in range(nb):
                    _, ko, do = ext[g0 + lo + f]
                    assert n[f] == len(ko) and kk[f, :n[f]].tobytes() == ko.tobytes() and np.array_equal(dd[f, :n[f]], do), (j, i, f)
                for pp in range(nb // 2):
                    onm, om12, _ = pairs[(g0 + lo) // 2 + pp]
                    assert nm[pp] == onm and np.array_equal(mm[pp, :len(om12)], om12), (j, i, pp)
        for j in range(nbatch):
            a = sets[j % nfl]
            if j >= nfl:  # the set is about to be reused: its batch is the oldest in flight
                assert L.orbx_multi_wait_one(h) == 0, L.orbx_multi_last_error(h)
                check(j - nfl, a)
                a["counts"][:] = -7
            ip = (vp * nd)(*[t.data_ptr() for t in imgs[j]])
            r = L.orbx_multi_extract_match_batch_device_async(h, n_frames, ip, W, H, W, W * H, a["ptrs"]["k"], a["ptrs"]["d"], CAP, a["ptrs"]["n"],
                                                              ctypes.byref(b), 100, 0.9, 1, a["ptrs"]["m"], a["ptrs"]["q"], a["counts"].ctypes.data)
            assert r == 0, (r, L.orbx_multi_last_error(h))
        assert L.orbx_multi_wait(h) == 0, L.orbx_multi_last_error(h)
        for j in range(max(nbatch - nfl, 0), nbatch):
            check(j, sets[j % nfl])
    finally:
        L.orbx_multi_destroy(h)


@pytest.mark.parametrize("depth", [0, 3])
def test_multi_c_abi_async_one_device(orbx, c4_oracle, depth):
    """The throughput form of the C ABI's multi-device host (issuing thread per device, batches in flight, counts of batch k gathered
    while batch k + 1 runs) on one device: every batch equals the oracle, in the two-half-batches mode and on three lanes."""
    import torch
    torch.cuda.init()
    _multi_async_run(orbx, [0], c4_oracle, depth, nbatch=4, n_frames=64)


def test_multi_c_abi_forced_rccl_one_device(orbx, c4_oracle, monkeypatch):
    """Diagnostic knob multi_force_rccl = 1 (orbx_debug_set): a ONE-device orbx_multi context goes through RCCL -- dlopen(librccl.so), ncclCommInitAll(1), a
    grouped ncclAllGather of the counts on the collective stream per batch, ncclCommDestroy -- so these code paths run on a
    one-GPU box too (they used to see their first execution on the driver's 8-GPU node).  The synchronous form and the
    stream-ordered form (three lanes, batches in flight) must both give the oracle's counts, blocks and pairs."""
    import torch
    torch.cuda.init()
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    with orbx.knobs(multi_force_rccl=1):
        _multi_run(orbx, [0], 64, c4_oracle)
        assert "librccl" in open("/proc/self/maps").read(), "RCCL was not loaded: the forced path did not run"
        _multi_async_run(orbx, [0], c4_oracle, 3, nbatch=4, n_frames=64)
        _multi_async_run(orbx, [0], c4_oracle, 0, nbatch=3, n_frames=64)


def test_bench_force_collective_one_rank(orbx):
    """`bench.py --gpus 1 --force-collective`: the nccl (RCCL) process group with ONE rank, the counts all-gathered every step as the
    N > 1 runs do -- the line says backend nccl, one RCCL rank, gathered counts equal the rank's own."""
    out = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-collective", "--steps", "5", "--warmup", "2",
                "--prime", "4", "--regions", "1", "--no-cpu-baseline", "--no-single-frame", "--no-other-configs"],
               env={"HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    d = _bench_line(out)
    c = d["config"]["collective"]
    assert d["n_gpus"] == 1 and d["checked"] is True, d["check"]
    assert c["backend"] == "nccl" and c["world_size"] == 1 and c["all_gathers"] >= 5 and c["gathered_counts_ok"] is True
    assert d["config"]["rccl_ranks"] == 1


def test_multi_c_abi_async_rccl(orbx, c4_oracle):
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("RCCL needs more than one GPU: this box has %d" % n)
    world = 8 if n >= 8 else 4 if n >= 4 else 2
    _multi_async_run(orbx, list(range(world)), c4_oracle, 3, nbatch=4, n_frames=64)


def test_multi_c_abi_rccl(orbx, c4_oracle):
    """More than one GPU: ncclCommInitAll + ncclAllGather of the counts inside liborbx.so (librccl.so through dlopen)."""
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("needs more than one GPU (this box has %d)" % n)
    _multi_run(orbx, list(range(min(n, 8))), N_FRAMES, c4_oracle)
