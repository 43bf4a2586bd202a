"""The map-point update's part of the Python package against include/orbx.h, without a device: the layout of RECORDS_MAP by the
probe of tests/test_abi_host.py, the byte-size guard of ORBextractor.map_update_problems_device, the order of its host lists, the
chain helper's calls, every refusal the C entry points make without a context, and the C++ shim program's build."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_abi_host import CAP, FRAMES_UN, MCAP, NF, NS, P, POSE, Recorder, prototypes, run_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 2  # entries


def test_map_record_layout_matches_the_header(orbx, tmp_path):
    """orbx_map_result against its C struct: 64 bytes, 16 int32, no gaps; RECORDS keeps its 19."""
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler on this machine")
    from orb_slam_tracking_amd._records import RECORDS, RECORDS_MAP
    assert len(RECORDS) == 19 and list(RECORDS_MAP) == ["orbx_map_result"] and "orbx_map_result" not in RECORDS
    cls, dtype = RECORDS_MAP["orbx_map_result"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "orbx.h"', "int main(void) {",
             '  printf("orbx_map_result %zu 0\\n", sizeof(orbx_map_result));']
    for f in dtype.names:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(orbx_map_result, %s), sizeof(((orbx_map_result*)0)->%s));' % (f, f, f))
    lines += ['  printf("what %d %d\\n", ORBX_MAP_NORMALS, ORBX_MAP_DESCRIPTORS);',
              '  printf("bad %d %d\\n", ORBX_MAP_BAD_INPUT, ORBX_MAP_NONFINITE);', "  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe"), str(src)], check=True)
    seen = {}
    for ln in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split("\n"):
        if ln:
            key, a, b = ln.split()
            seen[key] = (int(a), int(b))
    assert dtype.itemsize == seen["orbx_map_result"][0] == ctypes.sizeof(cls) == 64
    end = 0
    for f, (cname, _) in zip(dtype.names, cls._fields_):
        off, size = seen[f]
        assert (dtype.fields[f][1], dtype.fields[f][0].itemsize) == (off, size), f
        assert cname == f and (getattr(cls, cname).offset, getattr(cls, cname).size) == (off, size), f
        assert off == end, "%s: a gap, or a field of the struct the record table lacks" % f
        end = off + size
    assert end == dtype.itemsize and len(dtype.names) == 10 and dtype["reserved"].shape == (7,)
    assert orbx.MAP_RESULT_DTYPE is dtype and orbx.MapResult is cls and tuple(dtype.names[:-1]) == orbx.MAP_RESULT_FIELDS
    assert (orbx.MAP_NORMALS, orbx.MAP_DESCRIPTORS) == seen["what"] and (orbx.MAP_BAD_INPUT, orbx.MAP_NONFINITE) == seen["bad"]
    import map_update_ref_lib
    assert map_update_ref_lib.MAP_RESULT_DTYPE == dtype  # (the test library states the record on its own)


@pytest.fixture
def fake(orbx):
    rec = Recorder()
    ext = object.__new__(orbx.ORBextractor)
    ext._L, ext._h, ext.capacity, ext.nlevels, ext.nfeatures, ext.order_with_torch = rec, ctypes.c_void_p(0), CAP, 8, 8, True
    return {"ext": ext, "rec": rec, "orbx": orbx}


ARRAYS = FRAMES_UN + [("d_entry_pose", "d_entry_pose", E * POSE), ("d_rows", "d_rows", E * CAP * 4),
                      ("d_obs_outlier", "d_obs_outlier", E * CAP, True), ("d_map_n", "d_map_n", NS * 4),
                      ("d_map_points", "d_map_points", NS * MCAP * 12), ("d_map_mask", "d_map_mask", NS * MCAP, True),
                      ("d_map_mask_out", "d_map_mask_out", NS * MCAP, "d_map_mask"), ("d_map_ref", "d_map_ref", NS * MCAP * 4, True),
                      ("d_map_normals", "d_map_normals", NS * MCAP * 12, True), ("d_map_dist", "d_map_dist", NS * MCAP * 8, True),
                      ("d_map_desc", "d_map_desc32", NS * MCAP * 32, True), ("d_map_obs", "d_map_obs", NS * MCAP * 4),
                      ("d_res", "d_res", P * 64)]
SCALARS = dict(n_frames=NF, first=[0], count=[E], n_free=[1], map_set=[1], entry_frame=[1, 0], n_map_sets=NS, map_capacity=MCAP)


def test_device_call_guards_every_array(fake):
    """With every array at exactly the size the header documents one C call is made and each array arrives at its parameter's
    position; the optional arrays left out arrive as null or as the array they stand for (the mask, in place); any one array one
    byte short is a ValueError before the call."""
    run_case(fake, "map_update_problems_device", "orbx_map_update_batch_device", SCALARS, ARRAYS, prototypes(),
             fake["ext"].map_update_problems_device)
    assert not fake["rec"].calls  # (the last case of run_case was refused before the call)


def test_the_host_lists_arrive_in_the_headers_order(fake):
    bufs = {a[0]: np.zeros(a[2], np.uint8) for a in ARRAYS}
    fake["ext"].map_update_problems_device(**SCALARS, **bufs, what=2)
    (name, args), = fake["rec"].calls
    pos = {n: i for i, (_, n) in enumerate(prototypes()[name][1])}
    assert args[pos["n_problems"]] == 1 and args[pos["n_entries"]] == E and args[pos["capacity"]] == CAP and args[pos["what"]] == 2
    assert args[pos["n_map_sets"]] == NS and args[pos["map_capacity"]] == MCAP and args[pos["n_frames"]] == NF
    for host, want in (("h_first", [0]), ("h_count", [E]), ("h_n_free", [1]), ("h_map_set", [1]), ("h_entry_frame", [1, 0])):
        got = np.ctypeslib.as_array(ctypes.cast(args[pos[host]], ctypes.POINTER(ctypes.c_int32)), (len(want),))
        assert list(got) == want, host
    del fake["rec"].calls[:]
    fake["ext"].map_update_problems_device(**SCALARS, **bufs)
    assert fake["rec"].calls[0][1][pos["what"]] == 3  # (the default: both)
    with pytest.raises(fake["orbx"].OrbxError):
        fake["ext"].map_update_problems_device(**dict(SCALARS, count=[E, E]), **bufs)


def test_the_chain_queues_its_five_calls_and_nothing_else(fake):
    """MapFuser.fuse_local_ba_update_device: CreateNewMapPoints' two calls, Fuse, the local bundle adjustment, the update, in this
    order on the one stream, no copy and no wait between them."""
    from test_abi_host import CASES
    from test_fuse_abi_host import CASES as FUSE_CASES, SCALARS as FUSE_SCALARS
    from test_lba_abi_host import ARRAYS as LBA_ARRAYS, SCALARS as LBA_SCALARS
    orbx = fake["orbx"]
    fuser = orbx.MapFuser(fake["ext"])
    z = lambda arrays: {a[0]: np.zeros(a[2], np.uint8) for a in arrays}  # noqa: E731
    create = dict(CASES["match_triangulation_pairs_device"][2])
    create.update({k: v for k, v in z(CASES["match_triangulation_pairs_device"][3]).items() if k != "d_res"})
    create.update({k: v for k, v in z(CASES["triangulate_matches_pairs_device"][3]).items() if k not in create})
    create["d_match_res"] = np.zeros(P * 76, np.uint8)
    fuse = dict(FUSE_SCALARS, **z(FUSE_CASES["fuse_pairs_device"][1]))
    lba = dict(LBA_SCALARS, **z(LBA_ARRAYS))
    fuser.fuse_local_ba_update_device(create, fuse, lba, dict(SCALARS, **z(ARRAYS)))
    assert [c[0] for c in fake["rec"].calls] == ["orbx_match_triangulation_batch_device", "orbx_triangulate_matches_batch_device",
                                                 "orbx_fuse_batch_device", "orbx_local_ba_batch_device", "orbx_map_update_batch_device"]


def test_every_refusal_without_a_context(orbx):
    """The C entry points judge their arguments before anything touches a device: ORBX_E_BADARG / ORBX_E_CAPACITY for each
    documented refusal, ORBX_E_HIP for well-formed arguments without a context."""
    lib = orbx.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    cap, mcap = 8, 4
    a0 = dict(kps=np.zeros((2, cap), orbx.KEYPOINT_DTYPE), desc=np.zeros((2, cap, 32), np.uint8), n=np.zeros(2, np.int32),
              pose=np.zeros((2, 12), np.float32), rows=np.full((2, cap), -1, np.int32), ol=np.zeros((2, cap), np.uint8),
              mn=np.zeros(1, np.int32), pts=np.zeros((mcap, 3), np.float32), mask=np.ones(mcap, np.uint8), mo=np.ones(mcap, np.uint8),
              ref=np.zeros(mcap, np.int32), nrm=np.zeros((mcap, 3), np.float32), dist=np.zeros((mcap, 2), np.float32),
              md=np.zeros((mcap, 32), np.uint8), obs=np.zeros(mcap, np.int32), res=np.zeros(1, orbx.MAP_RESULT_DTYPE))

    def call(n_frames=2, n_problems=1, first=0, count=2, n_free=1, mset=0, n_entries=2, frames=(0, 1), cap=cap, n_sets=1, mcap=mcap, what=3,
             **null):
        a = dict(a0)
        a.update(null)
        hf, hc, hn, hs = (np.array([v], np.int32) for v in (first, count, n_free, mset))
        he = np.array(frames, np.int32)
        return lib.orbx_map_update_batch_device(None, n_frames, n_problems, p(hf), p(hc), p(hn), p(hs), n_entries, p(he), p(a["kps"]),
                                                p(a["desc"]), p(a["n"]), cap, p(a["pose"]), p(a["rows"]), p(a["ol"]), n_sets, mcap,
                                                p(a["mn"]), p(a["pts"]), p(a["mask"]), p(a["mo"]), p(a["ref"]), what, p(a["nrm"]),
                                                p(a["dist"]), p(a["md"]), p(a["obs"]), p(a["res"]))
    bad, full, hip = orbx.E_BADARG, orbx.E_CAPACITY, orbx.E_HIP
    assert call() == hip and call(n_problems=0) == hip
    for name in ("kps", "n", "pose", "rows", "mn", "pts", "mo", "obs", "res"):  # required whatever `what` says
        for what in (0, 3):
            assert call(what=what, **{name: None}) == bad, name
    for name in ("ol", "mask", "ref"):  # optional
        assert call(**{name: None}) == hip, name
    # what `what` needs
    assert call(what=4) == bad and call(what=-1) == bad
    for name, bit in (("nrm", 1), ("dist", 1), ("desc", 2), ("md", 2)):
        assert call(what=bit, **{name: None}) == bad and call(what=3, **{name: None}) == bad, name
        assert call(what=3 - bit, **{name: None}) == hip and call(what=0, **{name: None}) == hip, name
    assert call(n_frames=-1) == bad and call(n_problems=-1) == bad and call(n_entries=-1) == bad and call(n_sets=-1) == bad
    assert call(cap=0) == bad and call(mcap=0) == bad
    assert call(first=1) == bad and call(first=-1) == bad and call(count=3) == bad and call(count=-1) == bad
    assert call(n_free=3) == bad and call(n_free=-1) == bad and call(mset=1) == bad and call(mset=-1) == bad
    assert call(frames=(0, 2)) == bad and call(frames=(-1, 1)) == bad
    assert call(cap=orbx.BOW_MAX_FEATURES + 1) == full and call(mcap=orbx.BOW_MAX_FEATURES + 1) == full
    # the order: an argument out of range before the capacity, the capacity before the missing context
    assert call(cap=orbx.BOW_MAX_FEATURES + 1, n_free=3) == bad
    # n_free has no bound but count: more free keyframes than the local bundle adjustment takes
    many = orbx.LBA_MAX_FREE + 6
    assert call(n_frames=many, count=many, n_free=many, n_entries=many, frames=tuple(range(many))) == hip

    def one(n_entries=2, n_free=1, cap=cap, map_n=mcap, what=3, **null):
        a = dict(a0)
        a.update(null)
        r = orbx.MapResult()
        return lib.orbx_map_update(None, n_entries, n_free, p(a["kps"]), p(a["desc"]), p(a["n"]), cap, p(a["pose"]), p(a["rows"]), p(a["ol"]),
                                   map_n, p(a["pts"]), p(a["mask"]), p(a["mo"]), p(a["ref"]), what, p(a["nrm"]), p(a["dist"]), p(a["md"]),
                                   p(a["obs"]), ctypes.byref(r) if null.get("res", 1) is not None else None)
    assert one() == hip and one(n_entries=0, n_free=0, kps=None, desc=None, n=None, pose=None, rows=None, ol=None) == hip
    assert one(map_n=0, pts=None, mask=None, mo=None, ref=None, nrm=None, dist=None, md=None, obs=None) == hip
    for name in ("kps", "desc", "n", "pose", "rows", "pts", "mo", "nrm", "dist", "md", "obs", "res"):
        assert one(**{name: None}) == bad, name
    for name in ("ol", "mask", "ref"):
        assert one(**{name: None}) == hip, name
    assert one(what=0, desc=None, nrm=None, dist=None, md=None) == hip and one(what=4) == bad and one(what=-1) == bad
    assert one(n_free=3) == bad and one(n_free=-1) == bad and one(n_entries=-1) == bad and one(cap=0) == bad and one(map_n=-1) == bad
    assert one(cap=orbx.BOW_MAX_FEATURES + 1) == full and one(map_n=orbx.BOW_MAX_FEATURES + 1) == full


def test_python_host_form_refuses_mismatched_arrays(orbx):
    ext = object.__new__(orbx.ORBextractor)
    ext._L, ext._h, ext.capacity, ext.nlevels = Recorder(), ctypes.c_void_p(0), CAP, 8
    kps, desc = np.zeros((2, CAP), orbx.KEYPOINT_DTYPE), np.zeros((2, CAP, 32), np.uint8)
    ok = dict(keys_un=kps, desc=desc, n=[1, 1], poses=np.zeros((2, 12)), rows=np.zeros((2, CAP)), n_free=1, map_points=np.zeros((3, 3)))
    ext.map_update(**ok)
    assert [c[0] for c in ext._L.calls] == ["orbx_map_update"]
    for wrong in (dict(n=[1]), dict(keys_un=kps[0]), dict(map_mask=[1, 1]), dict(desc=desc[:1]), dict(obs_outlier=np.zeros((1, CAP))),
                  dict(map_ref=[0, 0]), dict(map_normals=np.zeros((2, 3))), dict(map_obs=[1])):
        with pytest.raises(orbx.OrbxError):
            ext.map_update(**dict(ok, **wrong))


def test_shim_map_update_compiles(orbx, tmp_path):
    """tests/cpp/shim_map_update.cpp -- LocalMapping::UpdateMapPoints of include/orbx_shim.hpp -- builds against the C ABI alone
    (tests/test_gpu_map_update.py runs it)."""
    libdir = os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "shim_map_update.cpp"), "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o",
           os.path.join(str(tmp_path), "shim_map_update")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
