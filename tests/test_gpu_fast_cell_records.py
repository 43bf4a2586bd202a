"""k_fast_wave on the host's 64-byte cell records (round 14): counts, keypoint bytes and descriptor bytes of small batches against the
CPU oracle, bit for bit, with the frames sent through k_fast_wave by the knob fast_wg_max_cells = 0.

Cases (at most four frames of at most 320 x 240 each): the geometries of tests/test_fast_cells_host.py that fit -- every byte phase
sh, every nvLast, both tile strides -- on a textured and a noise frame; and four frames of 160 x 128 that take the kernel's other
paths: uniform noise (more than 256 corners in a cell: the strength map is scanned instead of the corner list), a flat frame (no
pixel passes the quick reject even at minThFAST: the second sweep is skipped), lone pixels in the last detected row of every
level-0 cell (only the peeled last step of those sweeps lists anything) and a textured frame.  Each property is asserted on the
frame itself, in numpy, before the device is asked."""
import numpy as np
import pytest

import fast_cells_lib as F

pytestmark = pytest.mark.gpu

PATHS = ("paths", (500, 1.2, 2, 20, 7), 160, 128)
CASES = [c for c in F.SMALL if c[2] <= 320 and c[3] <= 240] + [PATHS]
_REF = {}


def _textured(w, h, seed):
    from orb_slam_tracking_amd import synth
    return synth.synth_frames(1, w, h, seed)[0]


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def _last_rows(params, w, h):
    """Ground 100 with one lone pixel of +100 in the last detected row of every level-0 cell that detects anything."""
    levels, _ = F.geometry(params, w, h, (w + 3) & ~3, 4)
    L = levels[0]
    img = np.full((h, w), 100, np.uint8)
    for ci in range(L["nRows"]):
        for cj in range(L["nCols"]):
            x, y, cw, ch = F.cell_rect(L, ci, cj)
            if ch:
                img[y + ch - 4, x + 3 + (7 * (ci + cj)) % (cw - 6)] = 200
    return img


def frames_of(case):
    name, params, w, h = case
    if name == "paths":
        return np.stack([_noise(w, h, 11), np.full((h, w), 100, np.uint8), _last_rows(params, w, h), _textured(w, h, 6400)])
    return np.stack([_textured(w, h, 6400), _noise(w, h, 12)])


def reference(oracle, case):
    """The case's frames and the oracle's (keypoints, descriptors) per frame: computed once, shared, never changed."""
    if case[0] not in _REF:
        frames = frames_of(case)
        oe = oracle.Extractor(*case[1])
        outs = []
        for f in frames:
            _, k, d = oe(f)
            outs.append((k.copy(), d.copy()))
        _REF[case[0]] = (frames, outs)
    return _REF[case[0]]


def _quick_reject(img):
    """d = max(min(max(T, B), max(L, R)) - v, v - max(min(T, B), min(L, R))) per pixel (0 in the 3-pixel border): the kernel lists
    a pixel at a threshold iff d is above it."""
    h, w = img.shape
    v = img[3:h - 3, 3:w - 3].astype(np.int32)
    T, B = img[0:h - 6, 3:w - 3].astype(np.int32), img[6:h, 3:w - 3].astype(np.int32)
    Lf, R = img[3:h - 3, 0:w - 6].astype(np.int32), img[3:h - 3, 6:w].astype(np.int32)
    mx = np.minimum(np.maximum(T, B), np.maximum(Lf, R))
    mn = np.maximum(np.minimum(T, B), np.minimum(Lf, R))
    d = np.zeros((h, w), np.int32)
    d[3:h - 3, 3:w - 3] = np.maximum(mx - v, v - mn)
    return d


def test_the_frames_take_the_paths(orbx):
    """On the frames alone: which path of the kernel each frame of `paths` takes at level 0, from the records and numpy."""
    name, params, w, h = PATHS
    ini, mn = params[3], params[4]
    noise, flat, last, _ = frames_of(PATHS)
    rec, info = F.records_of(orbx, params, w, h, (w + 3) & ~3, 4)
    levels, TS, exp = F.expected_cells(params, w, h, (w + 3) & ~3, 4)
    assert info[1] == 1 and TS == 64   # (cells of 43 columns: 13 dwords; the 48-byte instance takes the cases of F.SMALL)
    L = levels[0]
    cells = [(F.cell_rect(L, ci, cj), F.decode(rec[ci * L["nCols"] + cj])) for ci in range(L["nRows"]) for cj in range(L["nCols"])]
    det = lambda a, r: a[r[1] + 3:r[1] + r[3] - 3, r[0] + 3:r[0] + r[2] - 3]   # a cell's detected area
    # noise: every level-0 cell holds more corners at iniThFAST than the corner list does (256)
    corners = F.fast_corners(noise, ini)
    assert min(int(det(corners, r).sum()) for r, d in cells) > F.FW_CORN
    # (and so does a level-0 cell of the noise frame of the first case, which the 48-byte instance takes)
    _, p48, w48, h48 = CASES[0]
    L48 = F.geometry(p48, w48, h48, (w48 + 3) & ~3, 2)[0][0]
    assert F.tile_stride(F.geometry(p48, w48, h48, (w48 + 3) & ~3, 2)[0]) == 48
    c48 = F.fast_corners(frames_of(CASES[0])[1], p48[3])
    assert max(int(det(c48, F.cell_rect(L48, ci, cj)).sum()) for ci in range(L48["nRows"]) for cj in range(L48["nCols"])) > F.FW_CORN
    # flat: no d above minThFAST anywhere
    assert int(_quick_reject(flat).max()) <= mn
    # last rows: a corner in every cell (no second sweep), and every listed pixel's item lies in the last step of its cell's sweep
    d20 = _quick_reject(last) > ini
    corners = F.fast_corners(last, ini)
    for r, d in cells:
        ys, xs = np.nonzero(det(d20, r))
        assert len(ys) >= 1 and int(det(corners, r).sum()) >= 1, r
        assert d["nFull"] >= 1 and int((ys * d["nqc"] + (xs >> 2)).min()) >= 64 * d["nFull"], (r, d["nFull"])


def _extract_device(orbx, e, frames, cap):
    """The frames through extract_batch_device from a buffer whose rows are a multiple of four bytes apart (k_fast_wave asks for
    dword-aligned level-0 rows)."""
    import torch
    B, h, w = frames.shape
    stride = (w + 3) & ~3
    buf = np.zeros((B, h, stride), np.uint8)
    buf[:, :, :w] = frames
    d_img = torch.from_numpy(buf).cuda()
    d_k = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    d_d = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_img, B, w, h, stride, stride * h, d_k, d_d, d_n, cap)
    return (d_n.cpu().numpy(), d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap), d_d.cpu().numpy().reshape(B, cap, 32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_output_equals_the_oracle(orbx, oracle, case):
    name, params, w, h = case
    frames, outs = reference(oracle, case)
    assert len(frames) <= 4 and w <= 320 and h <= 240
    with orbx.knobs(fast_wg_max_cells=0):
        e = orbx.ORBextractor(*params, max_width=w, max_height=h, max_batch=len(frames))
        try:
            n, kk, dd = _extract_device(orbx, e, frames, params[0])
            assert e.debug_last_launch()["fast_wave"] == 1
            for f, (ko, do) in enumerate(outs):
                print(name, "frame", f, "keypoints", int(n[f]), "oracle", len(ko))
                assert n[f] == len(ko), (name, f, n[f], len(ko))
                assert kk[f, :n[f]].tobytes() == ko.tobytes(), (name, f)
                assert np.array_equal(dd[f, :n[f]], do), (name, f)
        finally:
            e.close()
    if name == "paths":
        assert len(outs[0][0]) > 100 and len(outs[1][0]) == 0 and len(outs[2][0]) >= 1
