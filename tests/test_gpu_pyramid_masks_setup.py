"""k_pyramid_bands after round 13 (one mask per interpolated row, no row copies, padded row table, thread split from the host): every
level of every frame equals the oracle's cv::resize chain byte for byte, on frames on which a missing mask would show
(tests/test_pyramid_setup_host.py) and in the situations the new code paths exist for.  Each situation is asserted on the CPU, from
the row map and the host formulas (tests/pyr_setup_lib.py), before the device is asked."""
import numpy as np
import pytest

import pyr_setup_lib as P


def _levels_equal_oracle(orbx, oracle, params, frames, K, S):
    """The frames as one batch through extract_batch_device under pyr_bands = K, pyr_strips = S: all levels >= 1 of all frames."""
    import torch
    B, h, w = frames.shape
    cap = params[0]
    stride = (w + 3) & ~3   # (k_pyramid_bands needs 4-byte aligned rows of level 0)
    padded = np.zeros((B, h, stride), np.uint8)
    padded[:, :, :w] = frames
    oe = oracle.Extractor(*params)
    e = orbx.ORBextractor(*params, max_width=w, max_height=h, max_batch=B)
    try:
        d_img = torch.from_numpy(padded).cuda()
        d_k = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
        d_d = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
        with orbx.knobs(bands_min_frames=1, pyr_bands=K, pyr_strips=S):
            e.extract_batch_device(d_img, B, w, h, stride, stride * h, d_k, d_d, d_n, cap)
            torch.cuda.synchronize()
        launch = e.debug_last_launch()
        assert launch["pyramid_banded"] == 1, (w, h, K, S, launch)
        for f in range(B):
            oe(np.ascontiguousarray(frames[f]), cap=cap)
            for l in range(1, params[2]):
                assert np.array_equal(e.image_pyramid(l, f), oe.level_image(l)), (w, h, params, K, S, f, l)
    finally:
        e.close()


def _thread_runs(params, w, h, K, S):
    """{(band, strip, level): per-thread runs} of a launch."""
    levels, r, g, two = P.launch_of(params, w, h, K, S)
    return {(b, s, l): P.runs_of(r[b][l][0], r[b][l][1], g[s][l][1] - g[s][l][0], two)
            for b in range(len(r)) for s in range(len(g)) for l in range(1, params[2])}, levels, two


def _pair_shares(levels, nlev):
    """Per adjacent row pair (dy, dy + 1) of every level: the lower source row of dy is the upper source row of dy + 1."""
    return [levels[l]["rows"][dy][1] == levels[l]["rows"][dy + 1][0] for l in range(1, nlev) for dy in range(levels[l]["h"] - 1)]


def _assert_situation(name, params, w, h, K, S):
    runs, levels, two = _thread_runs(params, w, h, K, S)
    lengths = [b - a for rr in runs.values() for a, b in rr]
    assert not two, name
    if name.startswith("scale1.2_maxbands"):
        # a whole wave without a row on a level on which the workgroup has rows: it skips that level's column record
        idle = [k for k, rr in runs.items() if any(b > a for a, b in rr) and
                any(all(b <= a for a, b in rr[w0:w0 + P.WAVE]) for w0 in range(0, P.PYR_T, P.WAVE))]
        assert idle, name
    if name == "one_row_and_odd_runs":
        # runs of exactly one row (no second row on the first step) and odd runs of three or more (none on the last step): the
        # second row's constants are then the padding entry of the staged row table
        assert 1 in lengths and any(n > 1 and n & 1 for n in lengths), sorted(set(lengths))
    shares = _pair_shares(levels, params[2])
    if name == "scale2_none_shares":
        assert not any(shares)
    if name == "scale1.01_all_share":
        assert sum(shares) > 0.98 * len(shares)
    if name.startswith("scale1.2"):
        assert 0.7 * len(shares) < sum(shares) < 0.9 * len(shares)
    # pixel 2 of some group of some level reads beyond the group's first two dwords (appendPyrTables' rule): the DUAL2 instances.
    # Scale 2 at an odd size has such groups.  Scale 1.5 has none at any width from 470 to 499 (pixel 2 starts at most 6 bytes into
    # the group's 12), so that case runs the plain instances on pairs of which every other one shares a row.
    dual2 = False
    for l in range(1, params[2]):
        xo, _, c1 = P.taps(levels[l]["w"], levels[l - 1]["w"], pad_to=4)
        dual2 |= any(xo[i + 2] + (c1[i + 2] != 0) - (xo[i] & ~3) > 7 for i in range(0, len(xo), 4))
    assert dual2 == (name == "scale2_dual2"), name
    if name == "scale1.5_half_share":
        assert 0.4 * len(shares) < sum(shares) < 0.6 * len(shares)


@pytest.mark.gpu
@pytest.mark.parametrize("name,params,w,h,K,S", P.CASES, ids=[c[0] for c in P.CASES])
def test_levels_equal_oracle(orbx, oracle, name, params, w, h, K, S):
    """Textured, flat 255, checkerboard and flat 0 frames in one batch (the last frame takes level 1 through the clamped loop)."""
    _assert_situation(name, params, w, h, K, S)
    _levels_equal_oracle(orbx, oracle, params, P.frames_of(w, h), K, S)


@pytest.mark.gpu
def test_clamped_loop_on_textured_and_checkerboard_frames(orbx, oracle):
    """The batch in reverse order and a batch of one: the frame behind which nothing is known to follow -- the one that takes level 1
    through the clamped single-dword loop -- is the textured one, then the checkerboard."""
    params, w, h = (300, 1.2, 8, 20, 7), 324, 243
    fr = P.frames_of(w, h)
    _levels_equal_oracle(orbx, oracle, params, fr[::-1], 3, 1)
    _levels_equal_oracle(orbx, oracle, params, fr[2:3], P.BANDS_MAX, 1)


@pytest.mark.gpu
def test_two_group_instances_at_the_smallest_height(orbx, oracle):
    """Level 1 is 542 groups wide: two groups per thread (masks and set-up as in the one-group instances, no carried row), at the
    smallest height the context accepts for that width."""
    params, w = (300, 1.2, 3, 20, 7), 2600
    for h in range(40, 200, 4):
        try:
            orbx.ORBextractor(*params, max_width=w, max_height=h, max_batch=1).close()
        except orbx.OrbxError as err:
            assert err.code == orbx.E_TOOSMALL, h
            continue
        break
    else:
        pytest.fail("no height up to 200 accepted")
    levels, r, g, two = P.launch_of(params, w, h, 3, 1)
    assert two and P.split_of(g[0][1][1] - g[0][1][0], two)[0] == 2
    from orb_slam_tracking_amd import synth
    fr = np.stack([synth.synth_frames(1, w, h, 6500)[0], np.full((h, w), 255, np.uint8)])
    _levels_equal_oracle(orbx, oracle, params, fr, 3, 1)
