"""GPU parity of the packed f16 arc strength (fastStrengthBiased in k_fast and k_fast_wave): the FAST candidates of every level
against the oracle's, bit for bit, on frames built to reach what the packed network could get wrong -- strength at the top of the
range on both signs, strength exactly at and one above iniThFAST, the second pass around minThFAST, cells with more than 64
survivors (full flushes) and with more than 256 corners (the strength map is scanned), narrow last cells -- each case asserted on
the oracle to really occur.  One 640 x 480 frame and a batch of two, through both kernels, three threshold pairs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 640, 480
NLEVELS = 8
MB = 16           # first detected column / row of a level (EDGE_THRESHOLD - 3)
WC, HC = 36, 38   # FAST cells of level 0 at 640 x 480: ceil(608 / 17), ceil(448 / 12)
PAIRS = ((20, 7), (7, 7), (40, 5))
# rows of level-0 cells per region
ROWS_EXTREME, ROW_DENSE, ROWS_RAMP, ROWS_FLAT = (0, 3), 3, (4, 7), (7, 10)


def _y(ci):
    return MB + ci * HC


def build_frame(ini, mn):
    rng = np.random.default_rng(1000 * ini + mn)
    img = np.full((H, W), 100, np.uint8)
    # -- 0 / 255 blocks: lone pixels, 2 x 2 and 3 x 3 blocks, bright on black (left half) and black on white (right half)
    y0, y1 = 0, _y(ROWS_EXTREME[1])
    img[y0:y1, : W // 2] = 0
    img[y0:y1, W // 2:] = 255
    for y in range(6, y1 - 8, 9):
        for x in range(6, W - 8, 9):
            if abs(x - W // 2) < 8:
                continue
            s = 1 + ((x // 9 + y // 9) % 3)
            img[y:y + s, x:x + s] = 255 if x < W // 2 else 0
    # -- dense cells: 3 x 3 blocks (200, centre 255) on black; period 6 in cells 0 .. 2 (> 256 corners per cell), period 12 in
    #    cells 3 .. 5 (> 64, <= 256)
    yd0, yd1 = _y(ROW_DENSE), _y(ROW_DENSE + 1) + 6
    img[yd0:yd1, MB:MB + 6 * WC + 6] = 0
    for (c0, c1, period) in ((0, 3, 6), (3, 6, 12)):
        for y in range(yd0, yd1 - 3, period):
            for x in range(MB + c0 * WC + (6 if c0 else 0), MB + c1 * WC + (6 if c1 == 6 else 0) - 3, period):
                img[y:y + 3, x:x + 3] = 200
                img[y + 1, x + 1] = 255
    # -- ramp of one grey level per 8 columns; lone pixels in the middle of a plateau (their ring stays on it) whose contrast,
    #    hence strength, is exactly iniTh (bands of 72 columns: 0, 2, ..) or iniTh + 1 as well (bands 1, 3, ..)
    yr0, yr1 = _y(ROWS_RAMP[0]) + 6, _y(ROWS_RAMP[1])
    ramp = (60 + np.arange(W) // 8).astype(np.uint8)
    img[yr0:yr1, :] = ramp[None, :]
    n = 0
    for y in range(yr0 + 4, yr1 - 4, 8):
        for x in range(3, W - 8, 8):
            if (x // 8 + y // 8) % 3:
                continue
            n += 1
            a = ini + (n & 1 if (x // 72) & 1 else 0)
            img[y, x] = int(ramp[x]) + (a if n & 2 else -a)
    # -- flat ground with noise of amplitude 6, 7, 8 around minThFAST = 7: dense uniform noise in [0, a] or sparse lone pixels of
    #    contrast +-a, one kind per band of 36 columns
    yf0, yf1 = _y(ROWS_FLAT[0]) + 6, _y(ROWS_FLAT[1])
    for b, x0 in enumerate(range(0, W, WC)):
        a = 6 + b % 3
        x1 = min(x0 + WC, W)
        if (b // 3) & 1:
            img[yf0:yf1, x0:x1] = 100 + rng.integers(0, a + 1, (yf1 - yf0, x1 - x0))
        else:
            for _ in range(10):
                y, x = int(rng.integers(yf0 + 4, yf1 - 4)), int(rng.integers(x0 + 4, max(x1 - 4, x0 + 5)))
                img[y, x] = 100 + (a if rng.integers(0, 2) else -a)
    # -- strong lone pixels along the right and the bottom border: the narrow last cells of every level
    for y in range(_y(ROWS_FLAT[1]) + 8, H - 4, 7):
        for x in range(10 + (y % 3), W - 4, 11):
            img[y, x] = 255 if (x + y) & 1 else 0
    for y in range(_y(ROW_DENSE), H - 4, 9):
        for x in range(W - 46, W - 4, 7):
            img[y:y + 2, x - 2:x + 3] = 100
            img[y, x] = 255 if (x + y) & 1 else 0
    return img


_REF = {}


def reference(oracle, pair):
    """Frames A and B = 255 - A rotated by 180 degrees (every sign swapped, every cell somewhere else) and the oracle's
    candidates per level, computed once per threshold pair."""
    if pair not in _REF:
        a = build_frame(*pair)
        b = np.ascontiguousarray(255 - a[::-1, ::-1])
        oe = oracle.Extractor(1000, 1.2, NLEVELS, *pair)
        cands = []
        for f in (a, b):
            oe(f)
            cands.append([oe.level_candidates(l).copy() for l in range(NLEVELS)])
        sizes = [oe.level_size(l) for l in range(NLEVELS)]
        _REF[pair] = (a, b, cands, sizes)
    return _REF[pair]


def last_cells(w, h):
    """(nCols, wCell, detected width of the last column's cells, nRows, hCell, detected height of the last row's) of a level."""
    wd, ht = (w - 19 + 3) - MB, (h - 19 + 3) - MB
    nc, nr = int(np.float32(wd) / np.float32(35)), int(np.float32(ht) / np.float32(35))
    wc, hc = -(-wd // nc), -(-ht // nr)
    return nc, wc, wd - (nc - 1) * wc - 6, nr, hc, ht - (nr - 1) * hc - 6


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "ini%d_min%d" % p)
def test_frames_hold_every_case(oracle, pair):
    """What the frames are for, asserted on the oracle alone (level 0 of frame A; candidate rows are (x - 16, y - 16, response),
    response = strength - 1)."""
    import oracle_lib as O
    ini, mn = pair
    a, b, cands, sizes = reference(oracle, pair)
    c0 = cands[0][0]
    x, y, r = c0[:, 0], c0[:, 1], c0[:, 2]
    rows = lambda r0, r1: (y >= r0 * HC + 3) & (y < r1 * HC + 3)
    top = rows(*ROWS_EXTREME)
    print(pair, "level-0 candidates", len(c0), "max response", r.max())
    # strength 255 on both signs
    assert r.max() == 254
    assert (top & (r == 254) & (x < W // 2 - 40)).sum() > 20 and (top & (r == 254) & (x > W // 2 + 40)).sum() > 20
    assert (cands[1][0][:, 2] == 254).sum() > 40
    # strength exactly iniTh + 1 is a corner; strength exactly iniTh only where the whole cell fell back to minTh < iniTh
    rr = rows(*ROWS_RAMP)
    n_at, n_above = int((rr & (r == ini - 1)).sum()), int((rr & (r == ini)).sum())
    print(pair, "ramp: strength == iniTh", n_at, "== iniTh + 1", n_above)
    assert n_above > 10
    assert (n_at > 10) if mn < ini else (n_at == 0)
    # the second pass: corners below iniTh in the flat rows
    fr = rows(*ROWS_FLAT) & (x < W - 64)
    n2 = int((fr & (r < ini)).sum())
    print(pair, "flat: second-pass corners", n2, "responses", sorted(set(r[fr].astype(int).tolist())))
    assert (n2 > 10) if mn < ini else (n2 == 0)
    if mn < ini:
        assert set(r[fr & (r < ini)].astype(int).tolist()) >= {k for k in (5, 6, 7) if mn <= k < ini}  # strengths 6, 7, 8 above minTh
    # more than 256 corners in one cell (the strength map is scanned), and more than 64 but at most 256 (full flushes, corner list)
    for cj, lo, hi in ((0, 257, 10**6), (1, 257, 10**6), (3, 65, 256), (4, 65, 256)):
        cell = a[_y(ROW_DENSE):_y(ROW_DENSE + 1) + 6, MB + cj * WC:MB + (cj + 1) * WC + 6]
        nc = len(O.fast(cell, ini, nms=False))
        print(pair, "dense cell", cj, "corners", nc)
        assert lo <= nc <= hi, (cj, nc)
        assert ((y >= ROW_DENSE * HC + 3) & (y < (ROW_DENSE + 1) * HC + 3) & (x >= cj * WC + 3) & (x < (cj + 1) * WC + 3)).sum() > 5
    # last cells narrower than the others, with candidates in them (640 x 480 offers 26 of 36 columns and 24 of 38 rows at level 0;
    # the ragged geometries with cells of a few pixels are test_gpu_parity.py's)
    ncol = nrow = 0
    for l in range(NLEVELS):
        nc, wc, lastw, nr, hc, lasth = last_cells(*sizes[l])
        cl = cands[0][l]
        in_col, in_row = int((cl[:, 0] >= (nc - 1) * wc + 3).sum()), int((cl[:, 1] >= (nr - 1) * hc + 3).sum())
        print(pair, "level", l, sizes[l], "last column", lastw, "of", wc, "candidates", in_col, "| last row", lasth, "of", hc, "candidates", in_row)
        ncol += int(4 * lastw <= 3 * wc and in_col > 0)
        nrow += int(4 * lasth <= 3 * hc and in_row > 0)
    assert ncol >= 2 and nrow >= 2


@pytest.mark.parametrize("kernel", ["k_fast", "k_fast_wave"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "ini%d_min%d" % p)
def test_candidates_equal_the_oracle(orbx, oracle, pair, kernel):
    a, b, cands, sizes = reference(oracle, pair)
    with orbx.knobs(fast_wg_max_cells=0 if kernel == "k_fast_wave" else None):
        e = orbx.ORBextractor(1000, 1.2, NLEVELS, *pair, max_width=W, max_height=H, max_batch=2)
        try:
            e(a)
            assert e.debug_last_launch()["fast_wave"] == int(kernel == "k_fast_wave")
            for l in range(NLEVELS):
                assert e.level_size(l) == sizes[l]
                assert np.array_equal(e.debug_candidates(0, l), cands[0][l]), (pair, kernel, "single", l)
            e.extract_batch(np.stack([a, b]))
            assert e.debug_last_launch()["fast_wave"] == int(kernel == "k_fast_wave")
            for f in range(2):
                for l in range(NLEVELS):
                    assert np.array_equal(e.debug_candidates(f, l), cands[f][l]), (pair, kernel, "batch", f, l)
        finally:
            e.close()
