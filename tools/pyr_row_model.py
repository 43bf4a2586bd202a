#!/usr/bin/env python3
"""CPU replay of k_pyramid_bands' thread -> row map: wave-steps and row interpolations per level and frame.

Replays, without a GPU, what the host and the kernel decide for a frame geometry: the level sizes and cv::resize's x / y tables
(buildGeometry), the row bands and column strips (computePyrBands), a thread's column and thread-row (loadCols) and the row loop,
under the map of rounds 5 - 11 ("parent": thread-row rsub takes rows r0 + 2 rsub + 2 rpp k, three interpolations per step and a
fourth when some lane's pair does not share a source row; lanes without a row run the loop all the same) and under round 12's
("runs": one contiguous run per thread-row, the lower source row carried from step to step, idle lanes stay out).

  wave-step      = one trip of the row loop by one wave (64 threads) that has at least one lane in it
  interpolation  = one horizontal interpolation of a source row by a wave (hrow: 14 vector instructions per group), counted
                   per group a thread owns

The static listing of the one-group instance has 70 vector instructions per step outside hrow, so
  vector instructions per frame ~ 70 wave-steps + 14 interpolations
(640x480 / 1.2 / 8 levels / 3 bands, parent: 1518 wave-steps, 4967 interpolations, 175.8 k; SQ_INSTS_VALU: 175,567).

What the two weights leave out (found in round 12, when the new map measured 160,103 against 149.9 k): the vector instructions a
wave issues per level OUTSIDE the loop -- column constants, run bounds, the next level's row table: 71 in round 12's listing (54 in
the parent's), on 8 waves x bands x (levels - 1) wave-levels per frame = 11.9 k at the bench geometry.  The parent's figure agreed
with its counter to 0.1 % all the same: its idle waves' steps, counted at the full 112, skip both store blocks (about 55 of the
112, -5.9 k against the +9.1 k of the missing term); the remaining 3 k or so are an unexplained residual.
The last line printed for the new map adds the per-level term; it lands within 1 % of the counter.

usage: pyr_row_model.py [--width 640] [--height 480] [--scale 1.2] [--levels 8] [--bands 3] [--strips 1]
"""
import argparse
import math

import numpy as np

PYR_T = 512      # threads per workgroup (orbx_kernels.hip)
WAVE = 64
BANDS_MAX = 32   # ORBX_PYR_BANDS_MAX
STRIPS_MAX = 8   # ORBX_PYR_STRIPS_MAX
STEP_INSTS = 70  # vector instructions of a step outside hrow (instance <0,1>)
HROW_INSTS = 14
LEVEL_INSTS = 71  # vector instructions of a wave per level outside the loop (round 12's listing of <0,1>)
# Round 13's listing of <0,1> (one mask per interpolated row, no row copies, thread split from the host): a step without upper rows is
# 78 vector instructions = 50 + 2 x 14, and an upper row adds its interpolation and the address of its load, 15:
#   vector instructions per frame ~ 48 wave-steps + 15 interpolations + 40 busy wave-levels + 24 idle wave-levels
STEP_INSTS_R13 = 48
HROW_INSTS_R13 = 15
LEVEL_INSTS_R13 = 40       # a wave with a row on the level: column record, run bounds, the next level's row table
LEVEL_IDLE_INSTS_R13 = 24  # a wave without one: it skips the column record and the loop's set-up

f32 = np.float32


def _round_half_even(v):
    return int(np.rint(v))


def geometry(w, h, scale_factor, nlevels):
    """Level sizes and, per level >= 1, the source column of every output pixel (padded to 4) and the two clamped source rows of
    every output row, as buildGeometry / appendPyrTables compute them."""
    sf = float(f32(scale_factor))  # the parameter is a float, widened for the products
    scale = [f32(1)]
    for _ in range(1, nlevels):
        scale.append(f32(float(scale[-1]) * sf))
    levels = []
    for l in range(nlevels):
        inv = f32(1) / scale[l]
        levels.append(dict(w=_round_half_even(f32(w) * inv), h=_round_half_even(f32(h) * inv)))
    for l in range(1, nlevels):
        S, D = levels[l - 1], levels[l]
        sw, sh, dw, dh = S["w"], S["h"], D["w"], D["h"]
        scale_x, scale_y = 1.0 / (dw / sw), 1.0 / (dh / sh)
        xofs = []
        for dx in range((dw + 3) // 4 * 4):
            d = min(dx, dw - 1)
            sx = math.floor(f32((d + 0.5) * scale_x - 0.5))
            xofs.append(min(max(sx, 0), sw - 1))
        yofs = [math.floor(f32((dy + 0.5) * scale_y - 0.5)) for dy in range(dh)]
        D["xofs"], D["yofs"] = xofs, yofs
        D["rows"] = [(min(max(o, 0), sh - 1), min(max(o + 1, 0), sh - 1)) for o in yofs]
    return levels


def bands(levels, K, S):
    """computePyrBands: rows [r0, r1) per band and level, groups [g0, g1) per strip and level."""
    nl = len(levels)
    K = min(K, BANDS_MAX)
    S = max(1, min(S, STRIPS_MAX))
    while S > 1 and (levels[nl - 1]["w"] + 3) // 4 < 16 * S:
        S -= 1
    g = [[None] * nl for _ in range(S)]
    for s in range(S):
        need0 = need1 = 0
        for l in range(nl - 1, 0, -1):
            ng = (levels[l]["w"] + 3) // 4
            a, b = ng * s // S, ng * (s + 1) // S
            if l < nl - 1 and need1 > need0:
                a, b = min(a, need0), max(b, need1)
            g[s][l] = (a, b)
            need0 = need1 = 0
            if b > a and l >= 2:
                xo, ngs = levels[l]["xofs"], (levels[l - 1]["w"] + 3) // 4
                need0 = min(max((xo[4 * a] & ~3) // 4, 0), ngs - 1)
                need1 = min((xo[4 * (b - 1)] & ~3) // 4 + 3, ngs)
    r = [[None] * nl for _ in range(K)]
    for b in range(K):
        need0 = need1 = 0
        for l in range(nl - 1, 0, -1):
            h = levels[l]["h"]
            r0, r1 = b * h // K, (b + 1) * h // K
            if l < nl - 1 and need1 > need0:
                r0, r1 = min(r0, need0), max(r1, need1)
            r[b][l] = (r0, r1)
            need0 = need1 = 0
            if r1 > r0 and l >= 2:
                yo, sh = levels[l]["yofs"], levels[l - 1]["h"]
                need0 = min(max(yo[r0], 0), sh - 1)
                need1 = min(max(yo[r1 - 1] + 1, 0), sh - 1) + 1
    return r, g


def two_groups(levels, g):
    """launch_pyramid_bands: the two-group instances (GMAX = 2) unless every strip fits one group per thread."""
    nl = len(levels)
    one = all(g[s][l][1] - g[s][l][0] <= PYR_T for s in range(len(g)) for l in range(1, nl))
    return not (one and g[0][1][1] - g[0][1][0] <= PYR_T // 2)


def columns(ng, gmax):
    """loadCols: groups per thread G, thread-columns ngt, thread-rows per pass rpp."""
    ng = max(ng, 1)
    ngt2 = (ng + 1) >> 1
    use1 = ng * (PYR_T // ng) if ng <= PYR_T else 0
    use2 = ngt2 * (PYR_T // ngt2)
    G = 2 if gmax == 2 and use2 > use1 else 1
    ngt = ngt2 if G == 2 else ng
    return G, ngt, max(PYR_T // ngt, 1)


def level_parent(rows, r0, r1, ng, gmax):
    """Rounds 5 - 11: (wave-steps, interpolations) of one workgroup on one level."""
    G, ngt, rpp = columns(ng, gmax)
    steps = interps = 0
    for w0 in range(0, PYR_T, WAVE):
        rsubs = sorted({t // ngt for t in range(w0, w0 + WAVE)})
        k = 0
        while True:
            dys = [r0 + 2 * rs + 2 * rpp * k for rs in rsubs]
            if not any(dy < r1 for dy in dys):  # the loop bound does not look at the thread-row: idle lanes trip too
                break
            fourth = any(rs < rpp and dy + 1 < r1 and rows[dy + 1][0] != rows[dy][1] for rs, dy in zip(rsubs, dys))
            steps += 1
            interps += G * (3 + fourth)
            k += 1
    return steps, interps


def level_runs(rows, r0, r1, ng, gmax):
    """Round 12: contiguous runs; the carried row in the one-group instances."""
    G, ngt, rpp = columns(ng, gmax)
    carry = gmax == 1
    Lr = ((r1 - r0 + rpp - 1) // rpp + 1) & ~1
    steps = interps = 0
    for w0 in range(0, PYR_T, WAVE):
        runs = []
        for rs in sorted({t // ngt for t in range(w0, w0 + WAVE)}):
            a = r0 + rs * Lr
            b = min(r1, a + Lr) if rs < rpp else a
            if b > a:
                runs.append((a, b))
        car = {run: None for run in runs}
        k = 0
        while True:
            act = [(a, b) for a, b in runs if a + 2 * k < b]
            if not act:
                break
            upper0 = upper1 = False
            for run in act:
                dy = run[0] + 2 * k
                dy1 = dy + 1 if dy + 1 < run[1] else dy
                upper0 |= not carry or rows[dy][0] != car[run]
                upper1 |= dy1 != dy and rows[dy1][0] != rows[dy][1]
                car[run] = rows[dy1][1]
            steps += 1
            interps += G * (2 + upper0 + upper1)
            k += 1
    return steps, interps


def wave_level_counts(w, h, scale_factor, nlevels, K, S):
    """(busy, idle) wave-levels per frame under round 12's map: waves with and without a row on a level, over the frame's workgroups."""
    levels = geometry(w, h, scale_factor, nlevels)
    r, g = bands(levels, K, S)
    gmax = 2 if two_groups(levels, g) else 1
    busy = idle = 0
    for l in range(1, nlevels):
        for b in range(len(r)):
            for s in range(len(g)):
                _, ngt, rpp = columns(g[s][l][1] - g[s][l][0], gmax)
                r0, r1 = r[b][l]
                Lr = ((r1 - r0 + rpp - 1) // rpp + 1) & ~1
                for w0 in range(0, PYR_T, WAVE):
                    rows = any(rs < rpp and r0 + rs * Lr < r1 for rs in {t // ngt for t in range(w0, w0 + WAVE)})
                    busy, idle = busy + rows, idle + (not rows)
    return busy, idle


def model(w, h, scale_factor, nlevels, K, S, level_fn):
    """Per level >= 1: (wave-steps, interpolations) per frame, summed over the frame's workgroups."""
    levels = geometry(w, h, scale_factor, nlevels)
    r, g = bands(levels, K, S)
    gmax = 2 if two_groups(levels, g) else 1
    out = []
    for l in range(1, nlevels):
        st = it = 0
        for b in range(len(r)):
            for s in range(len(g)):
                a = level_fn(levels[l]["rows"], r[b][l][0], r[b][l][1], g[s][l][1] - g[s][l][0], gmax)
                st, it = st + a[0], it + a[1]
        out.append((st, it))
    return out, levels, gmax


def totals(per_level):
    return sum(a for a, _ in per_level), sum(b for _, b in per_level)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--scale", type=float, default=1.2)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--bands", type=int, default=3)
    ap.add_argument("--strips", type=int, default=1)
    a = ap.parse_args()
    args = (a.width, a.height, a.scale, a.levels, a.bands, a.strips)
    parent, levels, gmax = model(*args, level_parent)
    runs, _, _ = model(*args, level_runs)
    print("%dx%d, scale %g, %d levels, %d bands x %d strips, %s per thread" %
          (a.width, a.height, a.scale, a.levels, a.bands, a.strips, "two groups" if gmax == 2 else "one group"))
    print("level  size        parent: wave-steps  interpolations    runs: wave-steps  interpolations")
    for l in range(1, a.levels):
        print("%5d  %4dx%-4d %20d %15d %19d %15d" % (l, levels[l]["w"], levels[l]["h"], *parent[l - 1], *runs[l - 1]))
    for name, per in (("parent", parent), ("runs", runs)):
        st, it = totals(per)
        print("%-6s %d wave-steps, %d interpolations per frame; 70 x + 14 x = %.1f k vector instructions%s" %
              (name, st, it, (STEP_INSTS * st + HROW_INSTS * it) / 1e3, "" if gmax == 1 else " (one-group weights: indicative only)"))
    st, it = totals(runs)
    wave_levels = (PYR_T // WAVE) * min(a.bands, BANDS_MAX) * len(bands(levels, a.bands, a.strips)[1]) * (a.levels - 1)
    print("runs, with %d vector instructions per wave and level outside the loop (%d wave-levels): %.1f k" %
          (LEVEL_INSTS, wave_levels, (STEP_INSTS * st + HROW_INSTS * it + LEVEL_INSTS * wave_levels) / 1e3))
    busy, idle = wave_level_counts(*args)
    print("round 13's weights, %d x + %d x + %d x %d busy + %d x %d idle wave-levels: %.1f k%s" %
          (STEP_INSTS_R13, HROW_INSTS_R13, LEVEL_INSTS_R13, busy, LEVEL_IDLE_INSTS_R13, idle,
           (STEP_INSTS_R13 * st + HROW_INSTS_R13 * it + LEVEL_INSTS_R13 * busy + LEVEL_IDLE_INSTS_R13 * idle) / 1e3,
           "" if gmax == 1 else " (one-group weights: indicative only)"))


if __name__ == "__main__":
    main()
