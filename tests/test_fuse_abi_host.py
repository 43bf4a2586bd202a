"""The Fuse part of the Python package against include/orbx.h, without a device: the layout of RECORDS_FUSE by the probe of
tests/test_abi_host.py, and its byte-size guard applied to the two device methods of MapFuser."""
import ctypes
import os
import shutil
import subprocess

import pytest

from test_abi_host import CAP, FRAMES_UN, MAP_SETS, MCAP, NF, NS, P, POSE, ROW, BOUNDS, K3, Recorder, prototypes, run_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuse_record_layout_matches_the_header(orbx, tmp_path):
    """orbx_fuse_result against its C struct, as test_record_layouts_match_the_header does it for RECORDS, which keeps its 19."""
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler on this machine")
    from orb_slam_tracking_amd._records import RECORDS, RECORDS_FUSE
    assert len(RECORDS) == 19 and list(RECORDS_FUSE) == ["orbx_fuse_result"] and "orbx_fuse_result" not in RECORDS
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "orbx.h"', "int main(void) {"]
    for c_name, (_, dtype) in RECORDS_FUSE.items():
        lines.append('  printf("%s %%zu 0\\n", sizeof(%s));' % (c_name, c_name))
        for f in dtype.names:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (c_name, f, c_name, f, c_name, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe"), str(src)], check=True)
    seen = {}
    for ln in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split("\n"):
        if ln:
            key, a, b = ln.split()
            seen[key] = (int(a), int(b))
    for c_name, (cls, dtype) in RECORDS_FUSE.items():
        assert dtype.itemsize == seen[c_name][0] == ctypes.sizeof(cls) == 64, c_name
        end = 0
        for f, (cname, _) in zip(dtype.names, cls._fields_):
            off, size = seen["%s.%s" % (c_name, f)]
            assert (dtype.fields[f][1], dtype.fields[f][0].itemsize) == (off, size), "%s.%s (dtype)" % (c_name, f)
            assert cname == f and (getattr(cls, cname).offset, getattr(cls, cname).size) == (off, size), "%s.%s (ctypes)" % (c_name, f)
            assert off == end, "%s.%s: a gap, or a field of the struct the record table lacks" % (c_name, f)
            end = off + size
        assert end == dtype.itemsize
    assert orbx.FUSE_RESULT_DTYPE is RECORDS_FUSE["orbx_fuse_result"][1] and orbx.FuseResult is RECORDS_FUSE["orbx_fuse_result"][0]
    assert (orbx.FUSE_BAD_INPUT, orbx.FUSE_NONFINITE, orbx.FUSE_OCCUPIED_UNMAPPED) == (2, 4, -2)
    assert (orbx.FUSE_NONE, orbx.FUSE_ADD, orbx.FUSE_KEEP_OCCUPANT, orbx.FUSE_REPLACE_OCCUPANT, orbx.FUSE_BAD_OCCUPANT) == (0, 1, 2, 3, 4)


@pytest.fixture
def fake(orbx):
    """A MapFuser over a context-less ORBextractor over a Recorder."""
    rec = Recorder()
    ext = object.__new__(orbx.ORBextractor)
    ext._L, ext._h, ext.capacity, ext.nlevels, ext.nfeatures, ext.order_with_torch = rec, ctypes.c_void_p(0), CAP, 8, 8, True
    return {"fuser": orbx.MapFuser(ext), "rec": rec, "orbx": orbx}


OUT = [("d_matches", "d_matches", ROW), ("d_occ_obs", "d_occ_obs", ROW, True), ("d_fuse_idx", "d_fuse_idx", P * MCAP * 4),
       ("d_fuse_act", "d_fuse_act", P * MCAP), ("d_fuse_other", "d_fuse_other", P * MCAP * 4), ("d_res", "d_res", P * 64)]
SCALARS = dict(n_frames=NF, kf=[0], map_set=[1], n_map_sets=NS, map_capacity=MCAP, K=K3, bounds=BOUNDS)
CASES = {
    "fuse_pairs_device": ("orbx_fuse_batch_device",
                          FRAMES_UN + MAP_SETS + [("d_map_obs", "d_map_obs", NS * MCAP * 4), ("d_pose", "d_pose", P * POSE)] + OUT),
    "fuse_scw_pairs_device": ("orbx_fuse_scw_batch_device", FRAMES_UN + MAP_SETS + [("d_scw", "d_scw", P * POSE)] + OUT),
}


@pytest.mark.parametrize("method", sorted(CASES))
def test_device_call_guards_every_array(fake, method):
    """With every array at exactly the size the header documents one C call is made and each array arrives at its parameter's
    position; optional arrays left out arrive as null; any one array one byte short is a ValueError before the call."""
    fn, arrays = CASES[method]
    run_case(fake, method, fn, SCALARS, arrays, prototypes(), getattr(fake["fuser"], method))


def test_every_device_method_of_the_fuser_is_in_the_table(orbx):
    for name in vars(orbx.MapFuser):
        if name.endswith(("_batch_device", "_pairs_device")) and not name.startswith("_"):
            assert name in CASES, name
    assert set(CASES) <= set(vars(orbx.MapFuser))
