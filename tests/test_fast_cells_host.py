"""k_fast_wave's cell records from the host (round 14), without a GPU: every field of every record of orbx_debug_fast_cells against
a plain Python restatement of what the parent kernel derived per wave from its cell, its level and the tile stride
(tests/fast_cells_lib.py), on the benchmark's frame sizes and on small frames on which every byte phase sh, every nvLast, a cell of
at most 64 items, a cell without rows and a geometry on the 64-byte tile occur -- asserted from the records themselves."""
import ctypes

import numpy as np
import pytest

import fast_cells_lib as F

CASES = [(n, p, w, h, (w + 3) & ~3, 8) for n, p, w, h in F.BIG + F.SMALL] + [
    ("vga_padded_rows_big_batch", F.PARAMS, 640, 480, 1024, 8192),   # 64-bit image and candidate offsets
    ("max_frame_dim", (2000, 1.2, 8, 20, 7), 4096, 4096, 4096, 64),
]


@pytest.fixture(scope="module")
def decoded(orbx):
    out = {}
    for name, params, w, h, stride0, batch in CASES:
        rec, info = F.records_of(orbx, params, w, h, stride0, batch)
        levels, TS, exp = F.expected_cells(params, w, h, stride0, batch)
        out[name] = (rec, info, levels, TS, exp, [F.decode(r) for r in rec])
    return out


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_every_field_equals_the_kernels_formulas(decoded, name):
    rec, info, levels, TS, exp, dec = decoded[name]
    tile, smap, total = F.lds_layout(levels, TS) if TS else (0, 0, 0)
    assert info == [len(exp), {0: 0, 64: 1, 48: 2}[TS], tile, total]
    assert len(rec) == len(exp) and TS in (48, 64)
    for i, (e, d) in enumerate(zip(exp, dec)):
        if e is None:
            assert not rec[i].any(), (name, i)   # rows == 0, and nothing else either
            continue
        at = (name, i, e["level"], e["ci"], e["cj"])
        assert d["spare"] == 0, at
        # where the cell image and the candidate segment lie
        assert (d["img"], d["frameStride"], d["stride"]) == (e["img"], e["frameStride"], e["stride"]), at
        assert (d["frameStride"] == 0) == (e["level"] == 0), at
        assert (d["cand"], d["candCap"], d["segCap"]) == (4 * e["cand"], 4 * e["candCap"], e["segCap"]), at   # (the record: bytes)
        assert d["oxy"] == (e["ox"] + (e["oy"] << 12)) & F.M32, at
        assert 0 <= e["oy"] < 4096 and e["ox"] + e["xoff"] + 3 >= 0 and e["ox"] + e["xoff"] + 3 + e["iw"] <= 4096, at
        # the cell image and the sweep
        assert (d["ch"], d["xoff"]) == (e["ch"], e["xoff"]), at
        assert (d["nqc"], d["inv"], d["nItems"], d["nvLast"]) == (e["nqc"], e["inv"], e["nItems"], e["nvLast"]), at
        assert d["inside"] == (1 << (e["nvLast"] - 1)) - 1, at            # bit j - 1: pixel j of a row's last quad is inside
        assert 0 <= d["nFull"] == (e["nItems"] - 1) // 64 and 1 <= 64 - d["tailShift"] <= 64, at
        assert (d["dPos"], d["wrapK"], d["lastThr"]) == (e["dPos"], e["wrapK"], e["lastThr"]), at
        assert (d["aLast"], d["kN"]) == (e["aLast"], e["kN"]), at
        assert d["sh1"] == e["sh"] + 1 and 16 + d["xoff"] - d["sh1"] == e["pos0s"] and 16 + d["xoff"] == e["eIdle"], at
        assert (d["selC0"], d["selR0"], d["rOff4"]) == (e["selC0"], e["selR0"], e["rOff4"]), at
        # what the kernel rebuilds in the rare scan path
        assert d["nvLast"] + 4 * (d["nqc"] - 1) == e["iw"] and d["ch"] - 6 == e["ih"], at
        # the last item's reads (dwords up to a + 6 TS + 8) stay inside the tile's bytes, and the 3 x 3 strength-map block of its
        # last pixel (e = a + sh + 1 + 3, bytes up to e + kN + 2 TS + 2) inside the strength map
        assert d["aLast"] + 6 * TS + 12 <= 16 + tile, at
        assert d["aLast"] + d["sh1"] + 3 + d["kN"] + 2 * TS + 2 < 16 + tile + smap, at


def test_the_listed_cases_occur(decoded):
    """From the records: all four byte phases, all four nvLast, a cell of at most 64 items, a cell without rows, a geometry on
    the 64-byte tile (a cell image wider than 12 dwords), both instances, and offsets beyond 32 bits."""
    small = [n for n, *_ in F.SMALL]
    live = [d for n in small for d in decoded[n][5] if d["ch"]]
    assert {d["sh1"] - 1 for d in live} == {0, 1, 2, 3}
    assert {d["nvLast"] for d in live} == {1, 2, 3, 4}
    assert {(d["sh1"] - 1, d["rOff4"]) for d in live} == {(0, 0), (1, 0), (2, 4), (3, 4)}
    assert any(d["nItems"] <= 64 and d["nFull"] == 0 for d in live) and any(d["nFull"] >= 2 for d in live)
    assert any(d["ch"] == 0 for d in decoded["no_rows"][5]) and any(d["ch"] for d in decoded["no_rows"][5])
    assert decoded["tile64"][3] == 64 and decoded["tile64"][1][1] == 1
    assert any((d["xoff"] + e["iw"] + 6 + 3) >> 2 > 12 for e, d in zip(decoded["tile64"][4], decoded["tile64"][5]) if e)
    assert all(decoded[n][3] == 48 and decoded[n][1][1] == 2 for n in ("vga", "wvga", "hd"))
    assert decoded["vga"][1][2:] == [2752, 6208]   # the benchmark's geometry: 6,208 bytes of LDS, five pieces of 1,280
    big = decoded["vga_padded_rows_big_batch"][5]
    assert max(d["img"] for d in big) >= 1 << 32 and max(d["cand"] for d in big) >= 1 << 32


def test_refusals(orbx):
    L = orbx.lib()
    info = np.zeros(4, np.int32)
    p = orbx._Params(1000, 1.2, 8, 20, 7)
    rec = np.zeros((4, 16), np.uint32)
    assert L.orbx_debug_fast_cells(None, 640, 480, 640, 1, None, 0, info.ctypes.data) == orbx.E_BADARG
    assert L.orbx_debug_fast_cells(ctypes.byref(p), 640, 480, 640, 1, None, 0, None) == orbx.E_BADARG
    assert L.orbx_debug_fast_cells(ctypes.byref(p), 640, 480, 639, 1, None, 0, info.ctypes.data) == orbx.E_BADARG
    assert L.orbx_debug_fast_cells(ctypes.byref(p), 640, 480, 640, 0, None, 0, info.ctypes.data) == orbx.E_BADARG
    assert L.orbx_debug_fast_cells(ctypes.byref(p), 640, 480, 640, 1, None, 4, info.ctypes.data) == orbx.E_BADARG
    assert L.orbx_debug_fast_cells(ctypes.byref(p), 60, 60, 60, 1, None, 0, info.ctypes.data) < 0          # too small for a cell
    assert L.orbx_debug_fast_cells(ctypes.byref(p), 640, 480, 640, 1, rec.ctypes.data, 4, info.ctypes.data) == 0
    assert info[0] > 4 and rec[3].any()                                                                    # cap cuts the copy
    # a geometry k_fast_wave does not take (one cell of 69 columns): no instance, no records
    q = orbx._Params(300, 1.2, 1, 20, 7)
    assert L.orbx_debug_fast_cells(ctypes.byref(q), 101, 101, 104, 1, rec.ctypes.data, 1, info.ctypes.data) == 0
    assert list(info) == [1, 0, 0, 0] and not rec[0].any()
