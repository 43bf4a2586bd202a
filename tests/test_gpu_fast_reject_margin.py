"""The quick reject of k_fast_wave decides from one value per pixel, d = max(max side - v, v - min side) over the four compass
pixels, compared with the threshold (d > th), and skips a cell's second sweep when no d of the first one was above minThFAST.
Candidate lists and extractor output against the CPU oracle, bit for bit, on cells built around exactly those margins, through
k_fast_wave (knob fast_wg_max_cells = 0) and through k_fast.

Frames of 128 rows (every cell image of both levels fits k_fast_wave's tile) and 160, 158 and 155 columns (rows 160 bytes apart,
so level 0 stays dword-aligned), 2 levels, iniThFAST 20,
minThFAST 7: level 0 is 3 x 2 cells of 43, 42 and 41 detected columns, i.e. a last quad of 3, 2 and 1 pixels.  On flat ground:
  cell (0, 0)  lone pixels and 9-pixel arcs whose contrast is iniTh - 1, iniTh, iniTh + 1, bright and dark, and lone pixels of
               iniTh + 1 in the row's last three columns
  cell (0, 1)  the same around minTh (nothing in the cell reaches iniTh: the cell is swept again at minTh)
  cell (0, 2)  one lone pixel of minTh + 1, bright: the only near-corner, one above the bound that skips the second sweep
  cell (1, 0)  one lone pixel of minTh, dark: exactly at that bound, no candidate
  cell (1, 1)  one lone pixel of minTh + 1, dark
  cell (1, 2)  one lone pixel of iniTh + 1 beside lone pixels of minTh + 1: the cell is not swept again, they stay out
Frame B = 255 - A rotated by 180 degrees: every sign swapped, the features cut by other cells.  Each case of frame A is asserted
on the oracle's candidates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, STRIDE, NLEVELS = 128, 160, 2
WIDTHS = (160, 158, 155)
INI, MIN = 20, 7
PARAMS = (500, 1.2, NLEVELS, INI, MIN)
MB = 16   # first column / row of a level's first cell image; candidate rows are relative to it
D0 = MB + 3  # first detected column / row
G = 100   # the ground
# ring of radius 3, k = 0 .. 15 (dx, dy)
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3))
SLOT = (5, 14, 23, 32)  # cell-local columns / rows of the feature slots


def geometry(w):
    """(nCols, wCell, nRows, hCell) of level 0 (cpp:1094-1100)."""
    wd, ht = (w - 19 + 3) - MB, (H - 19 + 3) - MB
    nc, nr = int(np.float32(wd) / np.float32(35)), int(np.float32(ht) / np.float32(35))
    return nc, -(-wd // nc), nr, -(-ht // nr)


def build_frame(w):
    """The frame and its features: (cell row, cell column, x, y, contrast, sign, kind) with kind 'lone' or 'arc'."""
    nc, wc, nr, hc = geometry(w)
    assert (nc, nr) == (3, 2)
    img = np.full((H, w), G, np.uint8)
    feats = []

    def lone(ci, cj, lx, ly, a, s):
        x, y = D0 + cj * wc + lx, D0 + ci * hc + ly
        img[y, x] = G + s * a
        feats.append((ci, cj, x, y, a, s, "lone"))

    def arc(ci, cj, lx, ly, a, s, k0):
        x, y = D0 + cj * wc + lx, D0 + ci * hc + ly
        for k in range(k0, k0 + 9):
            dx, dy = RING[k % 16]
            img[y + dy, x + dx] = G + s * a
        feats.append((ci, cj, x, y, a, -s, "arc"))  # (a bright arc makes the centre the dark one)

    for cj, th in ((0, INI), (1, MIN)):
        n = 0
        for a in (th - 1, th, th + 1):
            for s in (1, -1):
                lone(0, cj, SLOT[n % 4], SLOT[n // 4], a, s)
                n += 1
                arc(0, cj, SLOT[n % 4], SLOT[n // 4], a, s, 3 * n)
                n += 1
        for k in range(3):  # the last three columns of the cell's rows
            lone(0, cj, wc - 1 - k, SLOT[3] + 2 + 4 * k, th + 1, 1 if k & 1 else -1)
    lone(0, 2, SLOT[1], SLOT[1], MIN + 1, 1)
    lone(1, 0, SLOT[2], SLOT[1], MIN, -1)
    lone(1, 1, SLOT[1], SLOT[2], MIN + 1, -1)
    lone(1, 2, SLOT[0], SLOT[0], INI + 1, 1)
    lone(1, 2, SLOT[2], SLOT[0], MIN + 1, 1)
    lone(1, 2, SLOT[0], SLOT[2], MIN + 1, -1)
    return img, feats


_REF = {}


def reference(oracle, w):
    """Frames A and B, the oracle's candidates per frame and level, its extractor output per frame, and A's features."""
    if w not in _REF:
        a, feats = build_frame(w)
        b = np.ascontiguousarray(255 - a[::-1, ::-1])
        oe = oracle.Extractor(*PARAMS)
        cands, outs = [], []
        for f in (a, b):
            _, k, d = oe(f)
            outs.append((k.copy(), d.copy()))
            cands.append([oe.level_candidates(l).copy() for l in range(NLEVELS)])
        _REF[w] = (a, b, cands, outs, feats, [oe.level_size(l) for l in range(NLEVELS)])
    return _REF[w]


def _response_at(c, x, y):
    """Response of the level-0 candidate at pixel (x, y), or None."""
    hit = c[(c[:, 0] == x - MB) & (c[:, 1] == y - MB)]
    return None if len(hit) == 0 else int(hit[0, 2])


def test_oracle_holds_every_case(oracle):
    """What the frames are for, on the oracle's candidates alone (rows are (x - 16, y - 16, response), response = strength - 1)."""
    last_quads = set()
    for w in WIDTHS:
        a, b, cands, outs, feats, sizes = reference(oracle, w)
        nc, wc, nr, hc = geometry(w)
        c0, cb = cands[0][0], cands[1][0]
        nv = wc - 4 * ((wc + 3) // 4 - 1)  # pixels of a row's last quad (k_fast_wave: nvLast)
        last_quads.add(nv)
        cell_of = lambda c: (np.floor_divide(c[:, 1] - 3, hc).astype(int), np.floor_divide(c[:, 0] - 3, wc).astype(int))
        ci, cj = cell_of(c0)
        in_last_quad = 0
        for (fi, fj, x, y, av, s, kind) in feats:
            r = _response_at(c0, x, y)
            th = MIN if (fi, fj) in ((0, 1), (0, 2), (1, 0), (1, 1)) else INI  # the threshold that decides in the feature's cell
            print(w, (fi, fj), kind, "contrast", av, "sign", s, "at", (x, y), "threshold", th, "response", r)
            # the centre's compass pixels differ from it by exactly av: a corner iff av > th, of strength av
            assert (r == av - 1) if av > th else (r is None), (w, fi, fj, kind, av, s, r)
            if kind == "lone" and r is not None and (x - D0) - fj * wc >= 4 * ((wc + 3) // 4 - 1):
                in_last_quad += 1
        assert in_last_quad >= min(nv, 3) * 2, (w, nv, in_last_quad)  # corners in every column of the last quad, both passes
        # both sides at each margin, around iniTh and around minTh
        for (fi, fj, th) in ((0, 0, INI), (0, 1, MIN)):
            got = {(av - th, s, kind) for (gi, gj, x, y, av, s, kind) in feats if (gi, gj) == (fi, fj)}
            assert got >= {(m, s, k) for m in (-1, 0, 1) for s in (1, -1) for k in ("lone", "arc")}, (w, fi, fj)
        # the cells around the bound that skips the second sweep: one candidate, none, one; and the cell that is not swept again
        count = lambda i, j: int(((ci == i) & (cj == j)).sum())
        assert (count(0, 2), count(1, 0), count(1, 1), count(1, 2)) == (1, 0, 1, 1), (w, count(0, 2), count(1, 0), count(1, 1), count(1, 2))
        assert count(0, 0) >= 7 and count(0, 1) >= 7  # two lone pixels, two arcs, three in the last columns
        assert int(c0[(ci == 0) & (cj == 0), 2].min()) == INI and int(c0[(ci == 0) & (cj == 1), 2].min()) == MIN
        # frame B (its cells cut the mirrored features differently: the detected area is not symmetric) has corners of both passes too
        assert set(cb[:, 2].astype(int).tolist()) >= {MIN, INI}
        for f in range(2):
            assert len(outs[f][0]) > 10 and len(cands[f][1]) > 0
    assert last_quads >= {1, 2, 3}, last_quads


def _extract_device(orbx, e, frames, w):
    """The frames through extract_batch_device from a buffer whose rows are STRIDE bytes apart."""
    import torch
    B, cap = len(frames), PARAMS[0]
    buf = np.zeros((B, H, STRIDE), np.uint8)
    buf[:, :, :w] = frames
    d_img = torch.from_numpy(buf).cuda()
    d_k = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    d_d = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_img, B, w, H, STRIDE, STRIDE * H, d_k, d_d, d_n, cap)
    n = d_n.cpu().numpy()
    kk = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap)
    dd = d_d.cpu().numpy().reshape(B, cap, 32)
    return n, kk, dd


@pytest.mark.parametrize("kernel", ["k_fast", "k_fast_wave"])
@pytest.mark.parametrize("w", WIDTHS)
def test_candidates_and_output_equal_the_oracle(orbx, oracle, w, kernel):
    a, b, cands, outs, feats, sizes = reference(oracle, w)
    with orbx.knobs(fast_wg_max_cells=0 if kernel == "k_fast_wave" else None):
        e = orbx.ORBextractor(*PARAMS, max_width=w, max_height=H, max_batch=2)
        try:
            n, kk, dd = _extract_device(orbx, e, np.stack([a, b]), w)
            assert e.debug_last_launch()["fast_wave"] == int(kernel == "k_fast_wave")
            for f in range(2):
                for l in range(NLEVELS):
                    assert e.level_size(l) == sizes[l]
                    assert np.array_equal(e.debug_candidates(f, l), cands[f][l]), (w, kernel, f, l)
                ko, do = outs[f]
                assert n[f] == len(ko), (w, kernel, f, n[f], len(ko))
                assert kk[f, :n[f]].tobytes() == ko.tobytes(), (w, kernel, f)
                assert np.array_equal(dd[f, :n[f]], do), (w, kernel, f)
        finally:
            e.close()
