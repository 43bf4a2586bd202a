"""What the two round-14 test files of k_fast_wave share: a plain Python restatement of the host geometry (buildGeometry) and of what
the kernel derived per wave from its cell, its level and the tile stride before the host took that over (the parent kernel's own
formulas), the decoder of the 64-byte cell record, and the geometries of the cases.  No GPU: numpy and ctypes only."""
import ctypes

import numpy as np

f32 = np.float32
EDGE, MIN_BORDER, CELL_MAX = 19, 16, 76   # ORBX_EDGE, ORBX_MIN_BORDER, ORBX_CELL_MAX
FW_RING, FW_CORN = 192, 256               # ORBX_FW_RING, ORBX_FW_CORN
M32 = (1 << 32) - 1

# (name, (features, scale, levels, iniTh, minTh), width, height): the small ones were searched for what the docstrings of the tests
# list -- every byte phase sh, every nvLast, a cell of at most 64 items, a cell without rows, a geometry on the 64-byte tile
PARAMS = (1000, 1.2, 8, 20, 7)
BIG = [("vga", PARAMS, 640, 480), ("wvga", PARAMS, 752, 480), ("hd", PARAMS, 1920, 1080)]
SMALL = [("phases_a", (500, 1.2, 4, 20, 7), 316, 236), ("phases_b", (500, 1.2, 3, 20, 7), 299, 203),
         # (a cell of few items or of none is the last of a row of ~31 cells whose widths, rounded up, use the row up: 1120 columns)
         ("few_items", (300, 1.2, 1, 20, 7), 1120, 80), ("no_rows", (300, 1.2, 1, 20, 7), 1118, 80),
         ("tile64", (300, 1.2, 2, 20, 7), 84, 84)]


def _round(v):
    return int(np.rint(v))   # cvRound: half to even


def _align(v, a):
    return (v + a - 1) // a * a


def geometry(params, w, h, stride0, max_batch):
    """buildGeometry: per level the image, the cell grid and where its frames and candidates lie."""
    _, scale_factor, nlevels, _, _ = params
    sf = float(f32(scale_factor))
    scale = [f32(1)]
    for _ in range(1, nlevels):
        scale.append(f32(float(scale[-1]) * sf))
    levels, cell_base, pyr_off, cand_off = [], 0, 0, 0
    for l in range(nlevels):
        inv = f32(1) / scale[l]
        L = dict(w=_round(f32(w) * inv), h=_round(f32(h) * inv))
        L["maxBX"], L["maxBY"] = L["w"] - EDGE + 3, L["h"] - EDGE + 3
        width, height = f32(L["maxBX"] - MIN_BORDER), f32(L["maxBY"] - MIN_BORDER)
        assert width >= 35 and height >= 35, "the geometry is too small for this many levels"
        L["nCols"], L["nRows"] = int(width / f32(35)), int(height / f32(35))
        L["wCell"], L["hCell"] = int(np.ceil(width / f32(L["nCols"]))), int(np.ceil(height / f32(L["nRows"])))
        L["cellBase"] = cell_base
        cell_base += L["nCols"] * L["nRows"]
        L["segCap"] = _align(max(((L["wCell"] + 1) // 2) * ((L["hCell"] + 1) // 2), 1), 4)
        L["candCap"] = L["nCols"] * L["nRows"] * L["segCap"]
        L["candOff"] = cand_off
        cand_off += L["candCap"] * max_batch
        if l == 0:
            L["stride"], L["imgOff"], L["frameStride"] = stride0, 0, 0
        else:
            L["stride"] = _align(L["w"], 64)
            L["imgOff"], L["frameStride"] = pyr_off, L["stride"] * L["h"]
            pyr_off += L["frameStride"] * max_batch
        levels.append(L)
    return levels, cell_base


def cell_rect(L, ci, cj):
    """ComputeKeyPointsOctTree's cell image (cpp:1078-1103): (iniX, iniY, cw, ch), ch == 0 when the cell detects nothing."""
    iniY, iniX = MIN_BORDER + ci * L["hCell"], MIN_BORDER + cj * L["wCell"]
    if iniY >= L["maxBY"] - 3 or iniX >= L["maxBX"] - 6:
        return iniX, iniY, 0, 0
    maxY, maxX = min(iniY + L["hCell"] + 6, L["maxBY"]), min(iniX + L["wCell"] + 6, L["maxBX"])
    if maxX - iniX < 7 or maxY - iniY < 7:
        return iniX, iniY, 0, 0
    return iniX, iniY, maxX - iniX, maxY - iniY


def tile_stride(levels):
    """0 = k_fast_wave cannot take the geometry, else the bytes of a tile row: 48 when every cell image is at most 12 dwords wide."""
    ok, narrow = True, True
    for L in levels:
        for ci in range(L["nRows"]):
            for cj in range(L["nCols"]):
                iniX, _, cw, ch = cell_rect(L, ci, cj)
                if ch == 0:
                    continue
                nw = (iniX + cw - (iniX & ~3) + 3) >> 2
                ok &= nw <= 16 and ch <= 64
                narrow &= nw <= 12
    return 0 if not ok else 48 if narrow else 64


def lds_layout(levels, TS):
    """launch_fast: tile bytes, strength-map bytes, all of the kernel's dynamic LDS."""
    ch = max([7] + [min(L["hCell"] + 6, CELL_MAX) for L in levels])
    tile, smap = ch * TS + 16, (ch - 6 + 2) * TS
    return tile, smap, 16 + tile + smap + 2 * FW_RING + 2 * FW_CORN


def expected_cells(params, w, h, stride0, max_batch):
    """Per cell, in record order, what the parent kernel computed in its prologue (names as there); LDS addresses relative to the
    start of the dynamic LDS (tileAddr = 16).  None for a cell without rows."""
    levels, n_cells = geometry(params, w, h, stride0, max_batch)
    TS = tile_stride(levels)
    out = []
    if TS == 0:
        return levels, TS, [None] * n_cells
    tile_bytes, _, _ = lds_layout(levels, TS)
    tileAddr = 16
    smapAddr = tileAddr + tile_bytes
    for l, L in enumerate(levels):
        for ci in range(L["nRows"]):
            for cj in range(L["nCols"]):
                iniX, iniY, cw, ch = cell_rect(L, ci, cj)
                if ch == 0:
                    out.append(None)
                    continue
                local = ci * L["nCols"] + cj
                ax0 = iniX & ~3
                xoff = iniX - ax0
                iw, ih = cw - 6, ch - 6
                e = dict(level=l, ci=ci, cj=cj, ch=ch, iw=iw, ih=ih, xoff=xoff, stride=L["stride"], segCap=L["segCap"],
                         candCap=L["candCap"], frameStride=L["frameStride"])
                e["img"] = (0 if l == 0 else L["imgOff"]) + iniY * L["stride"] + ax0
                e["cand"] = L["candOff"] + local * L["segCap"]
                e["ox"], e["oy"] = cj * L["wCell"] - xoff, ci * L["hCell"]
                e["kN"] = smapAddr - tileAddr - xoff
                e["eIdle"] = tileAddr + xoff
                nqc = (iw + 3) >> 2
                e["nqc"], e["nItems"] = nqc, nqc * ih
                e["inv"] = ((1 << 20) + nqc - 1) // nqc                      # c_inv20.v[nqc]
                dqy = (64 * e["inv"]) >> 20
                dqc = 64 - dqy * nqc
                sh = (xoff + 3) & 3
                e["sh"] = sh
                e["pos0s"] = tileAddr + xoff + 3 - sh - 4                    # the scalar part of pos0
                e["dPos"] = (dqc << 16) | (dqy * TS + 4 * dqc)
                e["wrapK"] = ((TS - 4 * nqc) - (nqc << 16)) & M32
                e["lastThr"] = (nqc - 1) << 16
                e["nvLast"] = iw - 4 * (nqc - 1)
                e["aLast"] = tileAddr + (ih - 1) * TS + xoff + 3 - sh + 4 * (nqc - 1) - 4
                e["selC0"] = 0x0c000c00 + sh * 0x00010001 + 0x00010000
                rNear = sh <= 1
                e["rOff4"] = 0 if rNear else 4
                e["selR0"] = 0x0c000c00 + (sh + 3 if rNear else sh - 1) * 0x00010001 + 0x00010000
                out.append(e)
    assert len(out) == n_cells
    return levels, TS, out


RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3))


def fast_corners(img, th):
    """FAST-9 at threshold th: a mask of the pixels whose ring of radius 3 holds nine contiguous pixels all brighter than the
    centre + th or all darker than the centre - th (what k_fast_wave enters into a cell's corner list)."""
    h, w = img.shape
    c = img[3:h - 3, 3:w - 3].astype(np.int32)
    ring = [img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int32) for dx, dy in RING]
    out = np.zeros((h, w), bool)
    for side in ([r > c + th for r in ring], [r < c - th for r in ring]):
        b = np.stack(side + side[:8])
        for s in range(16):
            out[3:h - 3, 3:w - 3] |= b[s:s + 9].all(0)
    return out


def decode(rec):
    """The sixteen dwords of a record (csrc/orbx_device.h, FastCell) as the kernel reads them."""
    r = [int(v) for v in rec]
    quad, counts = r[14], r[15]
    inside = (quad >> 25) & 7
    d = dict(img=r[0] | r[1] << 32, frameStride=r[2], stride=r[3], cand=r[4] | r[5] << 32, candCap=r[6], oxy=r[7], dPos=r[8],
             wrapK=r[9], selC0=r[10], selR0=r[11], lastThr=r[12], aLast=r[13] & 0xffff, kN=r[13] >> 16,
             inv=quad & 0x1fffff, nqc=(quad >> 21) & 15, inside=inside, nvLast=1 + bin(inside).count("1"),
             rOff4=((quad >> 28) & 1) * 4, sh1=quad >> 29,
             nFull=counts & 15, tailShift=(counts >> 4) & 63, segCap=(counts >> 10) & 0x7ff, ch=(counts >> 21) & 0x7f,
             xoff=(counts >> 28) & 3, spare=counts >> 30)
    d["nItems"] = 64 * d["nFull"] + 64 - d["tailShift"]
    return d


def records_of(orbx, params, w, h, stride0, max_batch):
    """orbx_debug_fast_cells: (records [cells][16] uint32, info4)."""
    p = orbx._Params(int(params[0]), float(params[1]), int(params[2]), int(params[3]), int(params[4]))
    info = np.zeros(4, np.int32)
    L = orbx.lib()
    assert L.orbx_debug_fast_cells(ctypes.byref(p), w, h, stride0, max_batch, None, 0, info.ctypes.data) == 0
    rec = np.zeros((int(info[0]), 16), np.uint32)
    assert L.orbx_debug_fast_cells(ctypes.byref(p), w, h, stride0, max_batch, rec.ctypes.data, len(rec), info.ctypes.data) == 0
    return rec, [int(v) for v in info]
