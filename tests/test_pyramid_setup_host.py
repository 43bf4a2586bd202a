"""k_pyramid_bands' per-level set-up from the host (round 13), without a GPU: the multiply-shift reciprocals are exact wherever the
kernel uses them, the thread split equals the parent kernel's own formulas, and the frames of tests/test_gpu_pyramid_masks_setup.py
are ones on which a dropped low-byte mask would show."""
import numpy as np
import pytest

import pyr_setup_lib as P


def _cols(orbx, ng, two_groups):
    info = np.zeros(5, np.uint32)
    assert orbx.lib().orbx_debug_pyr_cols(int(ng), int(two_groups), info.ctypes.data) == 0, (ng, two_groups)
    return [int(v) for v in info]


def test_reciprocals_are_exact(orbx):
    """tid // ngt for every ngt in 1 .. 512 and tid in 0 .. 511, and (rows + rpp - 1) // rpp for every rpp the split can give
    and every sum below 768 (at most 256 rows per band, rpp <= 512): the 32-bit product does not overflow either."""
    tid = np.arange(P.PYR_T, dtype=np.uint64)
    x = np.arange(768, dtype=np.uint64)
    rpps = set()
    for ngt in range(1, P.PYR_T + 1):
        G, n, rpp, inv, inv_rpp = _cols(orbx, ngt, 0)
        assert (G, n, rpp) == (1, ngt, max(P.PYR_T // ngt, 1))
        assert inv == -(-(1 << P.INV_SHIFT) // ngt) and inv < 1 << 20
        assert int((tid * inv).max()) < 1 << 32
        assert np.array_equal((tid * inv) >> P.INV_SHIFT, tid // ngt), ngt
        assert inv_rpp == -(-(1 << P.INV_SHIFT) // rpp) and int((x * inv_rpp).max()) < 1 << 32
        assert np.array_equal((x * inv_rpp) >> P.INV_SHIFT, x // rpp), rpp
        rpps.add(rpp)
    assert {1, 2, 3, 512} <= rpps


def test_refusals(orbx):
    info = np.zeros(5, np.uint32)
    L = orbx.lib()
    for ng, two in ((0, 0), (513, 0), (1025, 1), (-1, 1)):
        assert L.orbx_debug_pyr_cols(ng, two, info.ctypes.data) == orbx.E_BADARG, (ng, two)
    assert L.orbx_debug_pyr_cols(8, 0, None) == orbx.E_BADARG
    assert L.orbx_debug_pyr_cols(1024, 1, info.ctypes.data) == 0 and list(info[:3]) == [2, 512, 1]


GEOMETRIES = [(p, w, h, K, S) for _, p, w, h, K, S in P.CASES] + [
    ((300, 1.2, 3, 20, 7), 2600, 160, 3, 1),      # the two-group instances
    ((1000, 1.2, 8, 20, 7), 640, 480, 3, 1),
    ((1000, 1.2, 8, 20, 7), 1920, 1080, 16, 1), ((1000, 1.2, 8, 20, 7), 1920, 1080, 8, 4),
    ((1000, 1.2, 8, 20, 7), 3840, 2160, 32, 1), ((1000, 1.2, 8, 20, 7), 3840, 2160, 32, 4), ((1000, 1.2, 8, 20, 7), 3840, 2160, 24, 8),
]


@pytest.mark.parametrize("params,w,h,K,S", GEOMETRIES)
def test_split_equals_the_parents_formulas(orbx, params, w, h, K, S):
    """G, ngt and rpp of every (strip, level) of a launch, from the host, against the parent kernel's loadCols formulas."""
    levels, r, g, two = P.launch_of(params, w, h, K, S)
    seen_two = False
    for s in range(len(g)):
        for l in range(1, params[2]):
            ng = g[s][l][1] - g[s][l][0]
            G, ngt, rpp = P.split_of(ng, two)
            assert tuple(_cols(orbx, ng, two)[:3]) == (G, ngt, rpp), (s, l, ng)
            seen_two |= G == 2
    assert seen_two == two or (two and S > 1)   # (a launch of the two-group instances has a level that takes two groups)
    if (w, S) in ((2600, 1), (1920, 1), (3840, 1)):
        assert two
    if w <= 640 or (w, S) == (3840, 8):
        assert not two


def test_a_dropped_mask_would_show():
    """The vertical step with and without the low-byte mask on 16 t, in numpy, over the GPU test's frames and scale-1.2 geometries:
    some output bytes differ, so the byte comparison on the device sees a mask that went missing; and the extremes the operand
    ranges are stated for occur -- a pixel of 255 under a (2048, 0) tap pair, 16 t at its maximum 255 * 2048 * 16, and low bytes
    of 16 t other than zero."""
    for name, params, w, h, K, S in P.CASES[:4:2]:
        levels = P.model.geometry(w, h, params[1], params[2])
        differ = full = low = 0
        top = 0
        for src in P.frames_of(w, h):
            for l in range(1, params[2]):
                dw, dh = levels[l]["w"], levels[l]["h"]
                with_mask, t16, (c0, c1) = P.resize_level(src, dw, dh, True)
                without, _, _ = P.resize_level(src, dw, dh, False)
                differ += int((with_mask != without).sum())
                top = max(top, int(t16.max()))
                low += int(((t16 & 0xff) != 0).sum())
                whole = (c0 == 2048) & (c1 == 0)
                if whole.any():
                    xo = P.taps(dw, src.shape[1])[0]
                    full += int((src[:, xo[whole]] == 255).sum())
                assert int(t16.max()) < 1 << 24 and int(c0.max()) << 8 <= 1 << 19
                src = with_mask
        assert differ > 100 and low > 1000, (name, differ, low)
        assert full > 0 and top == 255 * 2048 * 16, (name, full, top)
