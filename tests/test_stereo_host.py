"""Frame::ComputeStereoMatches without a device: the CPU restatement tests/cpp/stereo_ref.cpp (which shares
csrc/orbx_stereo_math.inc with the kernels) against the independently written numpy statement of tests/stereo_ref_lib.py on every
world, against ground truth, and world by world against what the rule it reaches says; three mutants of the restatement that the
worlds must tell apart."""
import os

import numpy as np
import pytest

import stereo_ref_lib as S

f32 = np.float32
_SEEN = {}  # counter -> the worlds in which it was non-zero (filled by test_restatement_equals_numpy_statement)


@pytest.fixture(scope="module")
def worlds(oracle):
    return S.worlds()


def rec(worlds, name):
    return worlds[name].expected()["record"]


def test_restatement_equals_numpy_statement(worlds):
    """All four arrays, the tail and every counter, byte for byte, on every world."""
    for name, w in worlds.items():
        e, n = w.expected(), S.numpy_statement(w)
        assert S.same(e, n) == [], name
        for f in S.RESULT_FIELDS:
            if e["record"][f] != 0:
                _SEEN.setdefault(f, []).append(name)
        assert list(e["record"]["reserved"]) == [0, 0]


def test_ground_truth(worlds):
    """right = left shifted by GT_D columns, noise-free.  At octave 0 the pyramid level is the image itself, so at the exact shift
    the two windows are the same bytes and SAD is 0; the best SAD is then 0 as well, and since the first smallest wins, d1 > d2
    and d3 >= d2, which bounds the parabola's delta by 0.5 in magnitude.  A kept octave-0 match therefore sits within half a
    pixel of the truth, and no tolerance beyond that 0.5 is needed: u_right - (su0 + inc) IS delta, exactly (scale[0] == 1)."""
    w = worlds["gt"]
    e, k = w.expected(), w.scene.oracle()["kL"]
    kept0 = (e["sad"] >= 0) & (k["octave"] == 0)
    assert kept0.sum() >= 30
    err = np.abs(k["x"][kept0].astype(np.float64) - e["u_right"][kept0] - S.GT_D)
    assert err.max() <= 0.5
    assert np.all(e["sad"][kept0] == 0)
    r = e["record"]
    assert r["n_removed_by_median"] > 0 and r["n_matches"] == r["n_before_median"] - r["n_removed_by_median"] == (e["sad"] >= 0).sum()
    assert np.array_equal(e["depth"] > 0, e["sad"] >= 0) and np.array_equal(e["u_right"] >= 0, e["sad"] >= 0)
    ok = e["depth"] > 0
    assert np.array_equal(e["depth"][ok], f32(w.bf) / (k["x"][ok] - e["u_right"][ok]))


def test_identical_images(worlds):
    r = rec(worlds, "same")
    assert r["median_sad"] == 0 and r["n_removed_by_median"] == r["n_before_median"] > 0 and r["n_matches"] == 0 and r["n_clamped"] > 0
    e = worlds["same"].expected()
    assert np.all(e["u_right"] == -1) and np.all(e["depth"] == -1) and np.all(e["match_right"] == -1) and np.all(e["sad"] == -1)


def test_empty_and_garbage_counts(worlds):
    for name in ("empty_left", "empty_right", "empty_both"):
        r = rec(worlds, name)
        assert all(r[f] == 0 for f in S.RESULT_FIELDS), name
    assert len(worlds["empty_left"].expected()["sad"]) == 0
    e = worlds["empty_right"].expected()
    assert len(e["sad"]) == worlds["empty_right"].nL and np.all(e["sad"] == -1)
    r = rec(worlds, "count_garbage")
    assert r["status"] == S.BAD_INPUT and r["n_with_candidates"] == 0  # (nR = -3 is clamped to no right keypoint)


def test_many_candidates_and_ties(worlds):
    """More candidates on a row than a wave has lanes: the best in the last chunk of 64 is found; of two at equal distance in
    different chunks the lower iR wins (rule 6)."""
    for n in (65, 129):
        e = worlds["many_%d" % n].expected()
        assert e["match_right"][0] == n - 1 and e["sad"][0] == 0, n
    assert worlds["tie_chunks"].expected()["match_right"][0] == 3


def test_distance_thresholds(worlds):
    """74 continues, 75 does not (thOrbDist); 99 and 100 are both candidates that match nothing (TH_HIGH only bounds bestDist)."""
    assert rec(worlds, "dist_74")["n_orb_matched"] == 2 and worlds["dist_74"].expected()["match_right"][0] == 0
    for d in (75, 99, 100):
        r = rec(worlds, "dist_%d" % d)
        assert r["n_with_candidates"] == 2 and r["n_orb_matched"] == 1, d  # (the anchor alone)
        assert worlds["dist_%d" % d].expected()["match_right"][0] == -1


def test_octaves(worlds):
    for oR, want in ((0, 0), (1, 1), (2, 1), (3, 1), (4, 0)):
        assert rec(worlds, "octave_2_%d" % oR)["n_with_candidates"] == want, oR


def test_x_range(worlds):
    for name, want in (("x_at_min", 1), ("x_below_min", 0), ("x_at_max", 1), ("x_above_max", 0)):
        assert rec(worlds, name)["n_with_candidates"] == want, name


def test_row_bands(worlds):
    """y_R + r an exact integer is the band's last row; y_L = 100.99 uses row 100; bands are clipped at row 0 and rows_0 - 1; a
    y_L in (-1, 0) truncates to row 0."""
    for name, want in (("band_exact", 1), ("band_frac", 1), ("band_miss", 0), ("band_below", 1), ("band_below_miss", 0), ("band_top", 1),
                       ("band_bottom", 1), ("band_negative_row", 1)):
        r = rec(worlds, name)
        assert r["n_with_candidates"] == want and r["status"] == 0, name


def test_window_and_level_bounds(worlds):
    assert rec(worlds, "window_refused")["n_window_refused"] == 1  # su0 + 11 == cols_o
    r = rec(worlds, "window_kept")                                 # su0 + 11 == cols_o - 1: the correlation runs
    assert r["n_window_refused"] == 0 and r["n_out_of_level"] == 0 and r["n_orb_matched"] == 1
    assert rec(worlds, "window_negative")["n_window_refused"] == 1
    assert rec(worlds, "strip_left")["n_out_of_level"] == 1 and rec(worlds, "strip_left")["n_window_refused"] == 0
    assert rec(worlds, "left_window_out")["n_out_of_level"] == 1
    r = rec(worlds, "huge_left")  # a huge finite x has no candidate (minU is as huge), a huge y has no row: neither is followed
    assert r["n_with_candidates"] == 1 and r["status"] == S.BAD_INPUT and r["n_matches"] == 1


def test_shifts(worlds):
    """The best shift at -5 or +5 is refused; at -4 and +4 it is kept, at the true column.  On the stripes SAD is 0 at -4, -1, 2
    and 5: the smallest inc wins."""
    for off in (-5, 5):
        r = rec(worlds, "shift_%+d" % off)
        assert r["n_edge"] == 1 and r["n_matches"] == 1, off
    x0 = float(worlds["shift_+4"].kL["x"][0])
    for off in (-4, 4):
        e = worlds["shift_%+d" % off].expected()
        assert e["record"]["n_edge"] == 0 and e["sad"][0] == 0 and abs(x0 - e["u_right"][0] - S.GT_D) <= 0.5, off
    e = worlds["sad_tie"].expected()
    assert e["sad"][0] == 0 and e["record"]["n_edge"] == 0 and round(float(e["u_right"][0])) == 119 - 4


def test_disparity(worlds):
    """disp == 0 is clamped to the exact bits of bf / 0.01f and (float)((double)x_L - 0.01); disp >= maxD is refused."""
    w = worlds["clamp"]
    e = w.expected()
    assert e["record"]["n_clamped"] == 1 and e["sad"][0] == 0
    assert e["depth"][0].tobytes() == (f32(w.bf) / f32(0.01)).tobytes()
    assert e["u_right"][0].tobytes() == f32(float(f32(205.0)) - 0.01).tobytes()
    assert rec(worlds, "disp_refused")["n_disparity_refused"] == 1
    e = worlds["disp_inside"].expected()
    assert e["record"]["n_disparity_refused"] == 0 and e["sad"][0] == 0


def test_median(worlds):
    """M = 1, M even, M odd: the element of rank M / 2; a match with (float)sad == thDist is removed (SADs 10, 21, 10: the median
    is 10 and (1.5f * 1.4f) * 10.0f rounds to 21.0f)."""
    e = worlds["median_equal"].expected()
    r = e["record"]
    assert r["n_before_median"] == 3 and r["median_sad"] == 10 and r["th_dist"] == f32(21.0) and r["n_removed_by_median"] == 1
    assert list(e["sad"]) == [10, -1, 10] and r["n_clamped"] == 3 and e["depth"][1] == -1 and e["match_right"][1] == -1
    r = rec(worlds, "median_1")
    assert r["n_before_median"] == 1 and r["n_matches"] == 1 and r["median_sad"] == worlds["median_1"].expected()["sad"][0] > 0
    for n in (4, 5):
        w = worlds["median_%d" % n]
        before = S.numpy_statement(S.World("x", w.scene, w.kL, w.dL, w.kR, w.dR))
        r = w.expected()["record"]
        assert r["n_before_median"] == n, n
        # the SADs before the filter: those kept, and those the filter removed, which are the ones at or above thDist
        sads = sorted(int(s) for s in _sads_before(w))
        assert r["median_sad"] == sads[n // 2] and r["th_dist"] == f32(f32(1.5) * f32(1.4)) * f32(sads[n // 2])
        assert r["n_removed_by_median"] == sum(f32(s) >= r["th_dist"] for s in sads)
        assert before["record"]["median_sad"] == r["median_sad"]


def _sads_before(w):
    """Each left keypoint's SAD before rule 12: every match alone (M = 1 removes nothing unless its SAD is 0)."""
    out = []
    for i in range(len(w.kL)):
        solo = S.numpy_statement(S.World("solo", w.scene, w.kL[i:i + 1], w.dL[i:i + 1], w.kR, w.dR))
        assert solo["record"]["n_before_median"] == 1
        out.append(solo["sad"][0] if solo["sad"][0] >= 0 else 0)
    return out


def test_flags(worlds):
    """A flagged keypoint is skipped, on either side, and the rest of the rig is unaffected."""
    clean = worlds["dist_74"].expected()  # the same match and anchor without the garbage (the descriptor distance plays no part)
    for name, bit in (("flag_octave_left", S.BAD_INPUT), ("flag_nan_left", S.NONFINITE), ("flag_inf_y_left", S.NONFINITE)):
        e = worlds[name].expected()
        assert e["record"]["status"] == bit and e["sad"][1] == -1 and e["record"]["n_matches"] == 2, name
        assert e["u_right"][[0, 2]].tobytes() == clean["u_right"].tobytes() and e["sad"][[0, 2]].tobytes() == clean["sad"].tobytes(), name
    for name, bit in (("flag_octave_right", S.BAD_INPUT), ("flag_nan_right", S.NONFINITE), ("flag_huge_right", 0)):
        e = worlds[name].expected()
        assert e["record"]["status"] == bit and list(e["match_right"]) == [1, 2], name
        assert e["u_right"].tobytes() == clean["u_right"].tobytes() and e["depth"].tobytes() == clean["depth"].tobytes(), name


def test_tail(worlds):
    """Frame::UnprojectStereo: camera coordinates, through a pose, and from undistorted keypoints that differ from the raw ones."""
    base, posed, un = (worlds[n].expected() for n in ("gt", "gt_pose", "gt_un"))
    ok = base["depth"] > 0
    assert ok.sum() > 100 and np.array_equal(base["mask"], ok.astype(np.uint8)) and np.all(base["points"][~ok] == 0)
    assert np.array_equal(base["points"][ok][:, 2], base["depth"][ok])
    k = worlds["gt"].kL
    assert np.allclose(base["points"][ok][:, 0], (k["x"][ok] - 160.0) * base["depth"][ok] / 260.0, rtol=1e-5)
    assert base["u_right"].tobytes() == posed["u_right"].tobytes() == un["u_right"].tobytes()
    R, t = S.POSE_WC[:9].reshape(3, 3), S.POSE_WC[9:]
    assert np.allclose(posed["points"][ok], base["points"][ok] @ R.T + t, rtol=1e-4, atol=1e-4)
    assert np.allclose(un["points"][ok][:, 0] - base["points"][ok][:, 0], 1.25 * base["depth"][ok] / 260.0, rtol=1e-3, atol=1e-4)


def test_second_geometry_and_stride(worlds):
    for name in ("pair15", "padded"):
        r = rec(worlds, name)
        assert r["n_matches"] > 50 and r["status"] == 0, name


MUTANTS = (("rule 6: <= for <", "cpp", "if (d < bestDist)", "if (d <= bestDist)"),
           ("rule 12: (M - 1) / 2 for M / 2", "cpp", "kept[M / 2]", "kept[(M - 1) / 2]"),
           ("rule 10: 2.0f * d2 dropped", "inc", "(d1 + d3) - 2.0f * d2", "(d1 + d3) - d2"))


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_worlds_tell_a_mutant_apart(worlds, tmp_path, mutant):
    """An altered copy of the restatement (or of the arithmetic it includes) must differ from the numpy statement on at least one
    world: the worlds can tell the rules apart."""
    _, where, old, new = mutant
    src, inc = open(S.SRC).read(), open(S.INC).read()
    assert (src if where == "cpp" else inc).count(old) == 1
    (tmp_path / "stereo_ref.cpp").write_text(src.replace(old, new) if where == "cpp" else src)
    (tmp_path / "orbx_stereo_math.inc").write_text(inc.replace(old, new) if where == "inc" else inc)
    L = S.build(str(tmp_path / "stereo_ref.cpp"), str(tmp_path))
    differing = []
    for name, w in worlds.items():
        o = w.scene.oracle()
        if S.same(S.restatement(w, o["pyrL"], o["pyrR"], L), S.numpy_statement(w)):
            differing.append(name)
    assert differing


def test_every_counter_was_reached(worlds):
    """Over all worlds together every counter of the record was non-zero at least once -- but n_delta_refused, which no input
    reaches: the best shift is the FIRST smallest SAD, so d1 > d2 and d3 >= d2, hence |d1 - d3| <= (d1 - d2) + (d3 - d2) and
    |delta| <= 0.5.  The design's test is kept for the design's sake; this asserts that it stayed 0 everywhere."""
    if not _SEEN:
        test_restatement_equals_numpy_statement(worlds)
    for f in S.RESULT_FIELDS:
        if f == "n_delta_refused":
            assert f not in _SEEN
        else:
            assert _SEEN.get(f), f
    assert os.path.exists(S.INC)
