"""The local bundle adjustment's part of the Python package against include/orbx.h, without a device: the layout of RECORDS_LBA by
the probe of tests/test_abi_host.py, the byte-size guard of ORBextractor.local_ba_problems_device, the chain helper's calls, every
refusal the C entry points make without a context, and the C++ shim program's build."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_abi_host import CAP, FRAMES_UN_NODESC, MCAP, NF, NS, P, POSE, K3, Recorder, prototypes, run_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 2  # entries


def test_lba_record_layout_matches_the_header(orbx, tmp_path):
    """orbx_lba_result against its C struct, as test_record_layouts_match_the_header does it for RECORDS, which keeps its 19."""
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler on this machine")
    from orb_slam_tracking_amd._records import RECORDS, RECORDS_LBA
    assert len(RECORDS) == 19 and list(RECORDS_LBA) == ["orbx_lba_result"] and "orbx_lba_result" not in RECORDS
    cls, dtype = RECORDS_LBA["orbx_lba_result"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "orbx.h"', "int main(void) {",
             '  printf("orbx_lba_result %zu 0\\n", sizeof(orbx_lba_result));']
    for f in dtype.names:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(orbx_lba_result, %s), sizeof(((orbx_lba_result*)0)->%s));' % (f, f, f))
    lines += ['  printf("max_free %d 0\\n", ORBX_LBA_MAX_FREE);', '  printf("bad %d %d\\n", ORBX_LBA_BAD_INPUT, ORBX_LBA_NONFINITE);',
              "  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe"), str(src)], check=True)
    seen = {}
    for ln in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split("\n"):
        if ln:
            key, a, b = ln.split()
            seen[key] = (int(a), int(b))
    assert dtype.itemsize == seen["orbx_lba_result"][0] == ctypes.sizeof(cls) == 128
    end = 0
    for f, (cname, _) in zip(dtype.names, cls._fields_):
        off, size = seen[f]
        assert (dtype.fields[f][1], dtype.fields[f][0].itemsize) == (off, size), f
        assert cname in (f, f + "_") and (getattr(cls, cname).offset, getattr(cls, cname).size) == (off, size), f
        assert off == end, "%s: a gap, or a field of the struct the record table lacks" % f
        end = off + size
    assert end == dtype.itemsize
    assert orbx.LBA_RESULT_DTYPE is dtype and orbx.LbaResult is cls
    assert (orbx.LBA_MAX_FREE, orbx.LBA_BAD_INPUT, orbx.LBA_NONFINITE) == (seen["max_free"][0],) + seen["bad"]
    import lba_ref_lib
    assert lba_ref_lib.LBA_RESULT_DTYPE == dtype  # (the test library states the record on its own)


@pytest.fixture
def fake(orbx):
    rec = Recorder()
    ext = object.__new__(orbx.ORBextractor)
    ext._L, ext._h, ext.capacity, ext.nlevels, ext.nfeatures, ext.order_with_torch = rec, ctypes.c_void_p(0), CAP, 8, 8, True
    return {"ext": ext, "rec": rec, "orbx": orbx}


ARRAYS = FRAMES_UN_NODESC + [("d_pose", "d_pose", NF * POSE), ("d_rows", "d_rows", E * CAP * 4), ("d_map_n", "d_map_n", NS * 4),
                             ("d_map_points", "d_map_points", NS * MCAP * 12), ("d_map_mask", "d_map_mask", NS * MCAP, True),
                             ("d_pose_out", "d_pose_out", E * POSE), ("d_obs_outlier", "d_obs_outlier", E * CAP), ("d_res", "d_res", P * 128),
                             ("d_map_points_out", "d_map_points_out", NS * MCAP * 12, "d_map_points")]
SCALARS = dict(n_frames=NF, first=[0], count=[E], n_free=[1], map_set=[1], entry_frame=[1, 0], n_map_sets=NS, map_capacity=MCAP, K=K3)


def test_device_call_guards_every_array(fake):
    """With every array at exactly the size the header documents one C call is made and each array arrives at its parameter's
    position; the optional arrays left out arrive as null (the mask) or as the array they stand for (the points, in place); any
    one array one byte short is a ValueError before the call."""
    run_case(fake, "local_ba_problems_device", "orbx_local_ba_batch_device", SCALARS, ARRAYS, prototypes(),
             fake["ext"].local_ba_problems_device)
    name, args = fake["rec"].calls[-1] if fake["rec"].calls else (None, None)
    assert name is None  # (the last case of run_case was refused before the call)


def test_the_host_lists_arrive_in_the_headers_order(fake):
    bufs = {a[0]: np.zeros(a[2], np.uint8) for a in ARRAYS}
    fake["ext"].local_ba_problems_device(**SCALARS, **bufs, n_iterations=3, n_more_iterations=4)
    (name, args), = fake["rec"].calls
    pos = {n: i for i, (_, n) in enumerate(prototypes()[name][1])}
    assert args[pos["n_problems"]] == 1 and args[pos["n_entries"]] == E and args[pos["capacity"]] == CAP
    assert (args[pos["n_iterations"]], args[pos["n_more_iterations"]]) == (3, 4) and args[pos["inv_sigma2"]].value is None
    for host, want in (("h_first", [0]), ("h_count", [E]), ("h_n_free", [1]), ("h_map_set", [1]), ("h_entry_frame", [1, 0])):
        got = np.ctypeslib.as_array(ctypes.cast(args[pos[host]], ctypes.POINTER(ctypes.c_int32)), (len(want),))
        assert list(got) == want, host
    with pytest.raises(fake["orbx"].OrbxError):
        fake["ext"].local_ba_problems_device(**dict(SCALARS, count=[E, E]), **bufs)


def test_the_chain_queues_its_three_calls_and_nothing_else(fake):
    """MapFuser.fuse_local_ba_device: CreateNewMapPoints' two calls, Fuse, the local bundle adjustment, in this order on the one
    stream, no copy and no wait between them."""
    from test_abi_host import CASES
    from test_fuse_abi_host import CASES as FUSE_CASES, SCALARS as FUSE_SCALARS
    orbx = fake["orbx"]
    fuser = orbx.MapFuser(fake["ext"])
    z = lambda arrays: {a[0]: np.zeros(a[2], np.uint8) for a in arrays}  # noqa: E731
    create = dict(CASES["match_triangulation_pairs_device"][2])
    create.update({k: v for k, v in z(CASES["match_triangulation_pairs_device"][3]).items() if k != "d_res"})
    create.update({k: v for k, v in z(CASES["triangulate_matches_pairs_device"][3]).items() if k not in create})
    create["d_match_res"] = np.zeros(P * 76, np.uint8)
    fuse = dict(FUSE_SCALARS, **z(FUSE_CASES["fuse_pairs_device"][1]))
    lba = dict(SCALARS, **z(ARRAYS))
    fuser.fuse_local_ba_device(create, fuse, lba)
    assert [c[0] for c in fake["rec"].calls] == ["orbx_match_triangulation_batch_device", "orbx_triangulate_matches_batch_device",
                                                 "orbx_fuse_batch_device", "orbx_local_ba_batch_device"]


def test_every_refusal_without_a_context(orbx):
    """The C entry points judge their arguments before anything touches a device: ORBX_E_BADARG / ORBX_E_CAPACITY for each
    documented refusal, ORBX_E_HIP for well-formed arguments without a context."""
    lib = orbx.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    cap, mcap = 8, 4
    kps, n, pose, rows = np.zeros((2, cap), orbx.KEYPOINT_DTYPE), np.zeros(2, np.int32), np.zeros((2, 12), np.float32), np.full((2, cap), -1, np.int32)
    mn, pts, K = np.zeros(1, np.int32), np.zeros((mcap, 3), np.float32), np.eye(3, dtype=np.float32).reshape(9)
    po, ol, res = np.zeros((2, 12), np.float32), np.zeros((2, cap), np.uint8), np.zeros(1, orbx.LBA_RESULT_DTYPE)

    def call(n_frames=2, n_problems=1, first=0, count=2, n_free=1, mset=0, n_entries=2, frames=(0, 1), cap=cap, n_sets=1, mcap=mcap, n_it=5,
             n_more=10, **null):
        a = dict(kps=kps, n=n, pose=pose, rows=rows, mn=mn, pts=pts, K=K, po=po, mo=pts, ol=ol, res=res)
        a.update(null)
        hf, hc, hn, hs = (np.array([v], np.int32) for v in (first, count, n_free, mset))
        he = np.array(frames, np.int32)
        return lib.orbx_local_ba_batch_device(None, n_frames, n_problems, p(hf), p(hc), p(hn), p(hs), n_entries, p(he), p(a["kps"]), p(a["n"]),
                                              cap, p(a["pose"]), p(a["rows"]), n_sets, mcap, p(a["mn"]), p(a["pts"]), None, p(a["K"]), None,
                                              n_it, n_more, p(a["po"]), p(a["mo"]), p(a["ol"]), p(a["res"]))
    bad, full, hip = orbx.E_BADARG, orbx.E_CAPACITY, orbx.E_HIP
    assert call() == hip and call(n_problems=0) == hip
    for name in ("kps", "n", "pose", "rows", "mn", "pts", "K", "po", "mo", "ol", "res"):
        assert call(**{name: None}) == bad, name
    assert call(n_frames=-1) == bad and call(n_problems=-1) == bad and call(n_entries=-1) == bad and call(n_sets=-1) == bad
    assert call(cap=0) == bad and call(mcap=0) == bad and call(n_it=-1) == bad and call(n_more=-1) == bad
    assert call(first=1) == bad and call(first=-1) == bad and call(count=3) == bad and call(count=-1) == bad
    assert call(n_free=3) == bad and call(n_free=-1) == bad and call(mset=1) == bad and call(mset=-1) == bad
    assert call(frames=(0, 2)) == bad and call(frames=(-1, 1)) == bad
    assert call(cap=orbx.BOW_MAX_FEATURES + 1) == full and call(mcap=orbx.BOW_MAX_FEATURES + 1) == full
    # more free keyframes than ORBX_LBA_MAX_FREE
    many = orbx.LBA_MAX_FREE + 1
    assert call(n_frames=many, count=many, n_free=many, n_entries=many, frames=tuple(range(many))) == bad
    assert call(n_frames=many, count=many, n_free=many - 1, n_entries=many, frames=tuple(range(many))) == hip

    def one(n_entries=2, n_free=1, cap=cap, map_n=mcap, n_it=5, n_more=10, **null):
        a = dict(kps=kps, n=n, pose=pose, rows=rows, pts=pts, K=K, po=po, mo=pts, ol=ol)
        a.update(null)
        r = orbx.LbaResult()
        return lib.orbx_local_ba(None, n_entries, n_free, p(a["kps"]), p(a["n"]), cap, p(a["pose"]), p(a["rows"]), map_n, p(a["pts"]), None,
                                 p(a["K"]), None, n_it, n_more, p(a["po"]), p(a["mo"]), p(a["ol"]), ctypes.byref(r) if null.get("res", 1) else None)
    assert one() == hip and one(n_entries=0, n_free=0, kps=None, n=None, pose=None, rows=None, po=None, ol=None) == hip
    for name in ("kps", "n", "pose", "rows", "pts", "K", "po", "mo", "ol", "res"):
        assert one(**{name: None}) == bad, name
    assert one(n_free=3) == bad and one(n_free=-1) == bad and one(n_entries=-1) == bad and one(cap=0) == bad and one(map_n=-1) == bad
    assert one(n_it=-1) == bad and one(n_more=-1) == bad
    assert one(n_entries=many, n_free=many) == bad
    assert one(cap=orbx.BOW_MAX_FEATURES + 1) == full and one(map_n=orbx.BOW_MAX_FEATURES + 1) == full


def test_python_forms_refuse_mismatched_arrays(orbx):
    ext = object.__new__(orbx.ORBextractor)
    ext._L, ext._h, ext.capacity, ext.nlevels = Recorder(), ctypes.c_void_p(0), CAP, 8
    kps = np.zeros((2, CAP), orbx.KEYPOINT_DTYPE)
    with pytest.raises(orbx.OrbxError):
        ext.local_ba(kps, [1], np.zeros((2, 12)), np.zeros((2, CAP)), 1, np.zeros((3, 3)), None, K3)
    with pytest.raises(orbx.OrbxError):
        ext.local_ba(kps, [1, 1], np.zeros((2, 12)), np.zeros((2, CAP)), 1, np.zeros((3, 3)), [1, 1], K3)
    with pytest.raises(orbx.OrbxError):
        ext.local_ba(kps[0], [1, 1], np.zeros((2, 12)), np.zeros((2, CAP)), 1, np.zeros((3, 3)), None, K3)


def test_shim_lba_compiles(orbx, tmp_path):
    """tests/cpp/shim_lba.cpp -- Optimizer::LocalBundleAdjustment of include/orbx_shim.hpp -- builds against the C ABI alone
    (tests/test_gpu_lba.py runs it)."""
    libdir = os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_lba.cpp"),
           "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", os.path.join(str(tmp_path), "shim_lba")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout


def test_the_lds_switch_takes_its_range_only(orbx):
    """orbx_debug_local_ba_lds_max_free: [-1, 29]; 29 is the largest count whose packed factor (8 * 174 * 173 / 2 bytes) fits in
    the 160 KiB of LDS beside the kernel's own."""
    lib = orbx.lib()
    assert lib.orbx_debug_local_ba_lds_max_free(30) == orbx.E_BADARG and lib.orbx_debug_local_ba_lds_max_free(-2) == orbx.E_BADARG
    assert lib.orbx_debug_local_ba_lds_max_free(0) == 0 and lib.orbx_debug_local_ba_lds_max_free(29) == 0
    with pytest.raises(orbx.OrbxError):
        orbx.debug_local_ba_lds_max_free(64)
    orbx.debug_local_ba_lds_max_free(-1)
