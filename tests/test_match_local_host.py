"""Tracking::SearchLocalPoints (include/orbx.h, "matching the local map by projection") on the CPU: the restatement
tests/cpp/match_local_ref.cpp, which the device is compared with byte for byte (tests/test_gpu_match_local.py), is itself pinned
here -- its window search to the reference's own compiled Frame::GetFeaturesInArea (tests/ref_lib.py), the whole of it to a second
statement in numpy that has neither a grid nor the streaming update, its PredictScale to the logarithm's, every rule alone, a
hand-made case that separates the claim rule from its nearest wrong neighbour, and the generated worlds to the conditions the GPU
test relies on."""
import math

import numpy as np
import pytest

import match_local_ref_lib as L

GENERATED = ("main", "main_th5", "bounds", "w700", "contention")


@pytest.fixture(scope="module")
def ref():
    import ref_lib
    ref_lib.lib()
    return ref_lib


@pytest.mark.parametrize("name", GENERATED + ("order",))
def test_window_search_is_the_references(ref, name):
    """For every point in view the restatement's candidate list is the reference's GetFeaturesInArea(u, v, r * scale[level],
    level - 1, level), order included; level 0 (minLevel = -1) and the top level are among them."""
    w = L.world(name)
    proj = w.expected()["proj"]
    several, levels = 0, set()
    for i in np.flatnonzero(proj[:, 5] == 5.0):
        u, v, r = (float(x) for x in proj[i, :3])
        lv = int(proj[i, 3])
        want = ref.features_in_area(w.kps, w.bounds, u, v, r, lv - 1, lv)
        got = L.features_in_area(w.kps, w.bounds, u, v, r, lv - 1, lv)
        assert np.array_equal(got, want), (name, int(i))
        several += len(want) > 1
        if len(want):
            levels.add(lv)
    assert several > 0
    if name in ("main", "bounds", "w700"):
        assert {0, L.NLEVELS - 1} <= levels, levels


def test_pinned_worlds_cover_the_window_edges(ref):
    """Bounds that do not start at 0, features outside the grid, and features a hair inside and a hair outside the radius, which
    the reference includes and leaves out."""
    w = L.world("bounds")
    assert w.bounds[0] != 0 and w.bounds[2] != 0
    for name in ("main", "bounds"):
        w = L.world(name)
        e = w.expected()
        _, ok = ref.pos_in_grid(w.kps, w.bounds)
        assert (~ok).sum() >= 4
        inside = outside = 0
        for i, j, is_in in w.edge:
            if e["proj"][i, 5] != 5.0:  # (a point the frame has on entry is not searched)
                continue
            u, v, r = (float(x) for x in e["proj"][i, :3])
            lv = int(e["proj"][i, 3])
            got = ref.features_in_area(w.kps, w.bounds, u, v, r, lv - 1, lv)
            assert (j in got) == is_in, (name, i, j, is_in)
            inside, outside = inside + is_in, outside + (not is_in)
        assert inside >= 10 and outside >= 10


@pytest.mark.parametrize("name", L.WORLDS + L.WORLDS_2)
def test_restatement_equals_the_numpy_statement(name):
    """The streaming update of bestDist / bestDist2 over a grid walk equals "the two smallest under (distance, window position)"
    over a filter of all features."""
    w = L.world(name)
    e = w.expected()
    m, view, nm = L.search_local_points_numpy(w)
    assert np.array_equal(e["matches"], m) and np.array_equal(e["view"], view) and e["res"]["nmatches"] == nm, name
    assert e["res"]["rounds"] == 0  # (the sequential statement has none)


@pytest.mark.parametrize("name", list(L.rule_worlds()))
def test_rule_worlds_equal_the_numpy_statement(name):
    w = L.rule_worlds()[name]
    e = w.expected()
    m, view, nm = L.search_local_points_numpy(w)
    assert np.array_equal(e["matches"], m) and np.array_equal(e["view"], view) and e["res"]["nmatches"] == nm, name


def test_counters_add_up():
    for name in L.WORLDS:
        r = L.world(name).expected()["res"]
        assert r["n_points"] >= r["n_behind"] + r["n_out_image"] + r["n_out_distance"] + r["n_out_angle"] + r["n_in_view"], name
        if r["status"] == 0:
            assert r["n_points"] == r["n_behind"] + r["n_out_image"] + r["n_out_distance"] + r["n_out_angle"] + r["n_in_view"], name
        assert r["n_with_candidates"] == r["nmatches"] + r["n_over_th"] + r["n_ratio_rejected"], name


def test_predict_scale_table_equals_the_logarithm():
    """level = #{n in [0, nlevels - 1) : ratio > scale[n]} equals ceil(log(ratio) / log(1.2f)) clamped to [0, nlevels - 1] on 10^5
    random ratios farther than a relative 1e-5 from every table entry; at a table entry and one f32 step below it the level is
    the entry's index, one step above the next (clamped)."""
    scale = L.scale_table()
    rng = np.random.default_rng(3)
    ratios = np.exp(rng.uniform(math.log(0.3), math.log(8.0), 100000)).astype(np.float32)
    far = np.all(np.abs(ratios[:, None].astype(np.float64) / scale[None, :].astype(np.float64) - 1.0) > 1e-5, axis=1)
    assert far.sum() > 99000
    log_factor = math.log(float(np.float32(1.2)))
    want = np.clip(np.ceil(np.log(ratios.astype(np.float64)) / log_factor), 0, L.NLEVELS - 1).astype(np.int32)
    got = L.predict_scale(ratios, scale)
    assert np.array_equal(got[far], want[far])
    assert set(got.tolist()) == set(range(L.NLEVELS))
    top = L.NLEVELS - 1
    below = np.nextafter(scale, np.float32(0), dtype=np.float32)
    above = np.nextafter(scale, np.float32(99), dtype=np.float32)
    assert L.predict_scale(scale, scale).tolist() == list(range(L.NLEVELS))
    assert L.predict_scale(below, scale).tolist() == list(range(L.NLEVELS))
    assert L.predict_scale(above, scale).tolist() == [min(n + 1, top) for n in range(L.NLEVELS)]
    assert L.predict_scale([0.0, np.inf], scale).tolist() == [0, top]


def test_rules():
    R = L.rule_worlds()
    e = {k: w.expected() for k, w in R.items()}
    r = lambda k: e[k]["res"]  # noqa: E731
    m = lambda k: e[k]["matches"].tolist()  # noqa: E731
    view = lambda k: e[k]["view"].tolist()  # noqa: E731
    NIV, SEEN = L.NOT_IN_VIEW, L.SEEN
    assert m("all_four") == [0, 1, 2, 3] and r("all_four")["nmatches"] == 4
    assert m("mask") == [0, -1, 2, 3] and view("mask") == [0, NIV, 0, 0] and r("mask")["n_points"] == 3
    # a seen point is not searched; its feature stays taken: point 0 finds feature 0 taken
    assert m("seen_no_outlier_array") == [2, -1, -1, 1] and view("seen_no_outlier_array") == [0, SEEN, SEEN, 0]
    assert r("seen_no_outlier_array")["n_seen"] == 2 and r("seen_no_outlier_array")["n_over_th"] == 2
    # an outlier's entry is cleared and its feature is free (point 3 takes it), but its point stays seen
    assert m("seen_and_outlier") == [2, -1, -1, 3] and view("seen_and_outlier") == [0, SEEN, SEEN, 0]
    assert r("seen_and_outlier")["n_outliers_cleared"] == 1 and r("seen_and_outlier")["n_seen"] == 2 and r("seen_and_outlier")["nmatches"] == 1
    # entries beyond the map's count are kept, never followed, their features taken (the outlier flag of one changes nothing)
    assert m("bad_entry") == [0, 4, 2, 99] and r("bad_entry")["status"] == L.BAD_INPUT and r("bad_entry")["n_seen"] == 0
    assert r("bad_entry")["n_outliers_cleared"] == 0 and r("bad_entry")["n_over_th"] == 2
    assert m("behind_the_camera") == [0, -1, 2, -1] and r("behind_the_camera")["n_behind"] == 2
    # z = +0 and z = -0 are not behind the camera: their u is no number, which is outside the image
    z = R["zero_depth"]
    assert z.points[1, 2] == 0 and not np.signbit(z.points[1, 2]) and np.signbit(z.points[2, 2])
    assert r("zero_depth")["n_behind"] == 0 and r("zero_depth")["n_out_image"] == 2 and e["zero_depth"]["proj"][1:3, 5].tolist() == [2.0, 2.0]
    assert m("zero_depth") == [0, -1, -1, 3] and r("zero_depth")["status"] == 0
    on = e["on_the_bounds"]
    assert on["proj"][:2, 0].tolist() == [0.0, 640.0] and on["proj"][:, 5].tolist() == [5.0, 5.0, 2.0, 2.0]
    assert r("on_the_bounds")["n_out_image"] == 2 and r("on_the_bounds")["n_in_view"] == 2
    outside = R["on_the_bounds"].variant(bounds=(-1, 641, 0, 480)).expected()["proj"]
    assert -1e-3 < outside[2, 0] < 0.0 and 640.0 < outside[3, 0] < 640.001  # (the two that were outside, by less than 0.001 pixel)
    # dist == 0.8f * min and dist == 1.2f * max stay, one f32 step beyond is out
    assert e["distance_bounds"]["proj"][:, 5].tolist() == [5.0, 3.0, 5.0, 3.0] and r("distance_bounds")["n_out_distance"] == 2
    # viewCos == 0.5 stays, one step below is out; viewCos == 0.998 has the wide radius, one step above the narrow one
    vc = e["view_cos"]["proj"]
    assert vc[:, 4].tolist()[0] == 0.5 and vc[2, 4] == np.float32(0.998) and vc[3, 4] > np.float32(0.998)
    assert vc[:, 5].tolist() == [5.0, 4.0, 5.0, 5.0] and vc[[0, 2, 3], 2].tolist() == [4.0, 4.0, 2.5]
    assert r("view_cos")["n_out_angle"] == 1
    assert e["view_cos_th3"]["proj"][[0, 2, 3], 2].tolist() == [12.0, 12.0, 7.5]
    # th = 1 leaves the radius alone, th = 2 doubles it
    assert e["th_1"]["proj"][0, 2] == 4.0 and m("th_1") == [-1] and r("th_1")["n_with_candidates"] == 0
    assert e["th_2"]["proj"][0, 2] == 8.0 and m("th_2") == [0]
    assert m("distance_100_and_101") == [0, -1] and r("distance_100_and_101")["n_over_th"] == 1
    assert e["distance_100_and_101"]["best"][:, 0].tolist() == [100, 101]
    # the ratio test: 40 against 46 at equal levels is rejected at 0.8 and passes at 0.9; at different levels, or with no second
    # candidate (bestDist2 = 256, bestLevel2 = -1), it passes
    assert e["ratio_equal_levels"]["best"][0].tolist() == [40, 46, 1, 1]
    assert m("ratio_equal_levels") == [-1, -1] and r("ratio_equal_levels")["n_ratio_rejected"] == 1
    assert m("ratio_passes") == [0, -1] and r("ratio_passes")["n_ratio_rejected"] == 0
    assert e["ratio_different_levels"]["best"][0].tolist() == [40, 46, 1, 0] and m("ratio_different_levels") == [0, -1]
    assert e["ratio_second_at_256"]["best"][0].tolist() == [40, 256, 1, -1] and m("ratio_second_at_256") == [0]
    assert m("nonfinite_point") == [-1, -1, -1, 3] and r("nonfinite_point")["status"] == L.NONFINITE
    assert r("nonfinite_point")["n_points"] == 4 and r("nonfinite_point")["n_in_view"] == 1
    assert r("nonfinite_pose")["status"] == L.NONFINITE and r("nonfinite_pose")["nmatches"] == 0 and r("nonfinite_pose")["n_in_view"] == 0
    assert r("no_features")["n_in_view"] == 4 and r("no_features")["n_with_candidates"] == 0 and len(m("no_features")) == 0
    assert r("no_points") == dict.fromkeys(L.RESULT_FIELDS, 0) and m("no_points") == [-1] * 4


def test_hand_made_order_case():
    """0 -> A; 1 -> B, because its second-best A is taken (with A free the ratio test rejects it); 2 -> none."""
    w = L.world("order")
    e = w.expected()
    dist = lambda a, b: int(np.unpackbits(a ^ b).sum())  # noqa: E731
    A, B = w.desc
    d = w.map_desc
    assert [dist(d[0], A), dist(d[1], A), dist(d[1], B), dist(d[2], A), dist(d[2], B)] == [0, 46, 40, 65, 5]
    cands = [sorted(L.features_in_area(w.kps, w.bounds, *e["proj"][i, :3], -1, 0).tolist()) for i in range(3)]
    assert cands == [[0], [0, 1], [0, 1]]
    assert e["matches"].tolist() == [0, 1] and e["outcome"].tolist() == [0, 1, -1]
    assert e["best"].tolist() == [[0, 256, 0, -1], [40, 256, 0, -1], [256, 256, -1, -1]]
    # alone, point 1 is rejected by the ratio test and point 2 takes B: what "the lowest claimant of its pick wins" would give
    assert e["alone"].tolist() == [0, -1, 1] and e["res"]["n_displaced"] == 2 and e["res"]["n_ratio_rejected"] == 0


def test_conditions_on_the_generated_worlds():
    """What the GPU comparison relies on: the main world exercises every way out and every decision at least five times, the
    contention world displaces at least a third of its points, the large worlds have more points than threads."""
    r = L.world("main").expected()["res"]
    for f in ("n_seen", "n_behind", "n_out_image", "n_out_distance", "n_out_angle", "n_over_th", "n_ratio_rejected", "n_outliers_cleared"):
        assert r[f] >= 5, (f, r[f])
    assert r["nmatches"] >= 40 and r["status"] == 0
    assert set(L.world("main").expected()["view"].tolist()) >= set(range(L.NLEVELS)) | {L.NOT_IN_VIEW, L.SEEN}
    c = L.world("contention").expected()["res"]
    assert 3 * c["n_displaced"] >= c["n_in_view"] > 100 and c["nmatches"] > 100
    w7, w30 = L.world("w700"), L.world("w3000")
    assert 250 <= w7.n_f <= 512 < w7.n_m == 700 and w7.expected()["res"]["nmatches"] > 40
    assert 1024 < w30.n_f <= 2048 and w30.n_m == 3000 and w30.expected()["res"]["n_in_view"] > 512
    assert L.world("main_th5").th == 5.0 and L.world("main_th5").expected()["res"]["nmatches"] > 20


def test_cpp_shim_match_local_compiles_and_links(orbx, tmp_path):
    """tests/cpp/shim_match_local.cpp -- ORBmatcher::SearchByProjection(F, MapView, th) of include/orbx_shim.hpp on a Frame-like
    type and on a FrameView -- builds against the C ABI alone; without a device it fails loudly (tests/test_gpu_match_local.py
    runs it)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = os.path.join(str(tmp_path), "shim_match_local"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "shim_match_local.cpp"),
           "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert os.path.exists(exe)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        p = subprocess.run([exe, "1"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode != 0 and "RESULT" not in p.stdout
