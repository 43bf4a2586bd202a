"""What the two round-13 test files of k_pyramid_bands share: the frames, the cases, a numpy restatement of the kernel's resize
arithmetic with and without the low-byte mask, and the thread split of a launch as the kernel derives it from the host's record.
No GPU, no library: everything here is numpy on top of tools/pyr_row_model.py's replay of the host geometry."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import pyr_row_model as model
finally:
    sys.path.pop(0)

PYR_T = model.PYR_T
WAVE = model.WAVE
BANDS_MAX = model.BANDS_MAX
INV_SHIFT = 19   # ORBX_PYR_INV_SHIFT (orbx_device.h)

# (name, extractor parameters (features, scale, levels, iniTh, minTh), width, height, bands K, strips S): the GPU test's cases
CASES = [
    ("scale1.2_3bands_a", (300, 1.2, 8, 20, 7), 324, 243, 3, 1),
    ("scale1.2_maxbands_a", (300, 1.2, 8, 20, 7), 324, 243, BANDS_MAX, 1),
    ("scale1.2_3bands_b", (300, 1.2, 8, 20, 7), 322, 245, 3, 1),
    ("scale1.2_maxbands_b", (300, 1.2, 8, 20, 7), 322, 245, BANDS_MAX, 1),
    ("scale2_none_shares", (300, 2.0, 3, 20, 7), 488, 364, 3, 1),
    ("scale2_dual2", (300, 2.0, 3, 20, 7), 486, 363, 3, 1),
    ("scale1.5_half_share", (300, 1.5, 4, 20, 7), 486, 363, 3, 1),
    ("scale1.01_all_share", (300, 1.01, 3, 20, 7), 486, 363, 3, 1),
    ("one_row_and_odd_runs", (300, 1.2, 8, 20, 7), 322, 245, 7, 1),
]


def frames_of(w, h):
    """The four frames of a batch: textured, flat 255, a 0 / 255 checkerboard, flat 0 -- the last one is the frame behind which
    nothing is known to follow, so the flat 0 frame takes level 1 through the clamped loop and the others through the 12-byte loads
    (the textured frame takes its turn at the clamped loop in the batch `frames_of(w, h)[::-1]`)."""
    from orb_slam_tracking_amd import synth
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([synth.synth_frames(1, w, h, 6400)[0], np.full((h, w), 255, np.uint8),
                     (((xx + yy) & 1) * 255).astype(np.uint8), np.zeros((h, w), np.uint8)])


def taps(n_dst, n_src, pad_to=1, clamp_fraction=True):
    """cv::resize INTER_LINEAR's table of one axis as buildGeometry computes it: first source index, Q11 pair (c0, c1)."""
    f32 = np.float32
    scale = 1.0 / (n_dst / n_src)
    n = (n_dst + pad_to - 1) // pad_to * pad_to
    ofs, c0, c1 = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        d = min(i, n_dst - 1)
        fx = f32((d + 0.5) * scale - 0.5)
        sx = int(np.floor(fx))
        fx = f32(fx - f32(sx))
        if clamp_fraction:
            if sx < 0:
                fx, sx = f32(0), 0
            if sx >= n_src - 1:
                fx, sx = f32(0), n_src - 1
        ofs[i], c0[i], c1[i] = sx, int(np.rint(f32(f32(1) - fx) * f32(2048))), int(np.rint(fx * f32(2048)))
    return ofs, c0, c1


def resize_level(src, dw, dh, masked=True):
    """One level of the chain as k_pyramid_bands computes it.  Horizontal: t = p0 c0 + p1 c1 (the kernel holds 16 t).  Vertical, as the
    kernel has it: (wy << 8) * (16 t & ~0xff) >> 32 per source row == wy * (t >> 4) >> 16; with masked=False the low byte of 16 t
    stays in the product: wy * t >> 20.  Returns the level, 16 t of every (source row, output column), and the x pairs."""
    sh, sw = src.shape
    xo, xc0, xc1 = taps(dw, sw)
    yo, yc0, yc1 = taps(dh, sh, clamp_fraction=False)   # (the y table keeps its fraction; the rows are clamped instead)
    s = src.astype(np.int64)
    t = s[:, xo] * xc0 + s[:, np.minimum(xo + 1, sw - 1)] * xc1
    r0, r1 = np.clip(yo, 0, sh - 1), np.clip(yo + 1, 0, sh - 1)
    if masked:
        u = ((yc0[:, None] * (t[r0] >> 4)) >> 16) + ((yc1[:, None] * (t[r1] >> 4)) >> 16)
    else:
        u = ((yc0[:, None] * t[r0]) >> 20) + ((yc1[:, None] * t[r1]) >> 20)
    return ((u + 2) >> 2).astype(np.uint8), 16 * t, (xc0, xc1)


def split_of(ng, two_groups):
    """The parent kernel's loadCols formulas: groups per thread G, thread-columns ngt, thread-rows per pass rpp."""
    return model.columns(ng, 2 if two_groups else 1)


def runs_of(r0, r1, ng, two_groups):
    """Per thread of the workgroup the run [run0, run1) of the band's rows [r0, r1) (round 12's map, divisions and all)."""
    _, ngt, rpp = split_of(ng, two_groups)
    Lr = ((r1 - r0 + rpp - 1) // rpp + 1) & ~1
    out = []
    for tid in range(PYR_T):
        rsub = tid // ngt
        a = r0 + rsub * Lr
        out.append((a, min(r1, a + Lr) if rsub < rpp else a))
    return out


def launch_of(params, w, h, K, S):
    """(levels, bands' rows r[b][l], strips' groups g[s][l], two_groups) of a launch, as the host computes them."""
    levels = model.geometry(w, h, params[1], params[2])
    r, g = model.bands(levels, K, S)
    return levels, r, g, model.two_groups(levels, g)
