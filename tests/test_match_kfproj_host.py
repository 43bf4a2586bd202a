"""The relocalisation overload ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (include/orbx.h,
"matching a keyframe's points by projection") on the CPU: the restatement tests/cpp/match_kfproj_ref.cpp, which the device is
compared with byte for byte (tests/test_gpu_match_kfproj.py), is itself pinned here -- its window search to the reference's own
compiled Frame::GetFeaturesInArea (tests/ref_lib.py), the whole of it to a second statement in numpy that has no grid and ranks
all candidates before it looks at what is taken, every rule alone, a hand-made case that separates the claim rule from its nearest
wrong neighbour, the generated worlds to the conditions the GPU test relies on, and the chain worlds to the paths they must take."""
import os
import subprocess

import numpy as np
import pytest

import match_kfproj_ref_lib as L

GENERATED = ("main", "main_th3", "bounds", "pdesc", "w700", "contention")


@pytest.fixture(scope="module")
def ref():
    import ref_lib
    ref_lib.lib()
    return ref_lib


@pytest.mark.parametrize("name", GENERATED + ("order",))
def test_window_search_is_the_references(ref, name):
    """For every searched point the restatement's candidate list is the reference's GetFeaturesInArea(u, v, th * scale[level],
    level - 1, level + 1), order included; level 0 (minLevel = -1) and the top level (maxLevel = nlevels) are among them."""
    w = L.world(name)
    proj = w.expected()["proj"]
    several, levels = 0, set()
    for i in np.flatnonzero(proj[:, 5] == 5.0):
        u, v, r = (float(x) for x in proj[i, :3])
        lv = int(proj[i, 3])
        want = ref.features_in_area(w.kps_c, w.bounds, u, v, r, lv - 1, lv + 1)
        got = L.features_in_area(w.kps_c, w.bounds, u, v, r, lv - 1, lv + 1)
        assert np.array_equal(got, want), (name, int(i))
        several += len(want) > 1
        if len(want):
            levels.add(lv)
    assert several > 0
    if name in ("main", "bounds", "w700"):
        assert {0, L.NLEVELS - 1} <= levels, levels


def test_pinned_worlds_cover_the_window_edges(ref):
    """Bounds that do not start at 0, features outside the grid, and features one f32 step inside and outside the radius, which
    the reference includes and leaves out."""
    w = L.world("bounds")
    assert w.bounds == (-12, 655, -9, 490)
    for name in ("main", "bounds"):
        w = L.world(name)
        e = w.expected()
        _, ok = ref.pos_in_grid(w.kps_c, w.bounds)
        assert (~ok).sum() >= 4
        inside = outside = 0
        for i, j, is_in in w.edge:
            if e["proj"][i, 5] != 5.0:  # (a point the frame has on entry is not searched)
                continue
            u, v, r = (float(x) for x in e["proj"][i, :3])
            lv = int(e["proj"][i, 3])
            got = ref.features_in_area(w.kps_c, w.bounds, u, v, r, lv - 1, lv + 1)
            assert (j in got) == is_in, (name, i, j, is_in)
            inside, outside = inside + is_in, outside + (not is_in)
        assert inside >= 10 and outside >= 10


@pytest.mark.parametrize("name", L.WORLDS + L.WORLDS_2)
def test_restatement_equals_the_numpy_statement(name):
    """The streaming `dist < bestDist` over a grid walk that skips what is taken equals "rank every candidate by (distance, window
    position), take the first untaken" over a filter of all features."""
    w = L.world(name)
    e = w.expected()
    m, nm = L.search_by_projection_numpy(w)
    assert np.array_equal(e["matches"], m) and e["res"]["nmatches"] == nm, name
    assert e["res"]["rounds"] == 0  # (the sequential statement has none)


@pytest.mark.parametrize("name", list(L.rule_worlds()))
def test_rule_worlds_equal_the_numpy_statement(name):
    w = L.rule_worlds()[name]
    e = w.expected()
    m, nm = L.search_by_projection_numpy(w)
    assert np.array_equal(e["matches"], m) and e["res"]["nmatches"] == nm, name


def test_counters_add_up():
    for name in L.WORLDS:
        e = L.world(name).expected()
        r = e["res"]
        searched = int((e["proj"][:, 5] == 5.0).sum())
        assert r["n_points"] >= r["n_out_image"] + r["n_out_distance"] + searched, name
        if r["status"] == 0:
            assert r["n_points"] == r["n_out_image"] + r["n_out_distance"] + searched, name
        assert r["n_with_candidates"] == r["nmatches"] + r["n_rot_removed"] + r["n_over_dist"], name
        assert r["n_with_candidates"] <= searched, name


def test_rules():
    R = L.rule_worlds()
    e = {k: w.expected() for k, w in R.items()}
    r = lambda k: e[k]["res"]  # noqa: E731
    m = lambda k: e[k]["matches"].tolist()  # noqa: E731
    stage = lambda k: e[k]["proj"][:, 5].tolist()  # noqa: E731
    assert m("all_four") == [0, 1, 2, 3] and r("all_four")["nmatches"] == 4
    assert m("mask") == [0, -1, 2, 3] and r("mask")["n_points"] == 3
    # a found point is not searched; its feature stays taken: point 3 finds feature 3 taken
    assert m("found_no_outlier_array") == [2, -1, -1, 1] and r("found_no_outlier_array")["n_found"] == 2
    assert r("found_no_outlier_array")["n_over_dist"] == 2 and r("found_no_outlier_array")["n_outliers_cleared"] == 0
    # the same row with the outlier array: the outlier's entry is cleared and its feature is free (point 3 takes it), but its
    # point 1 stays found
    assert m("found_and_outlier") == [2, -1, -1, 3] and stage("found_and_outlier") == [5.0, 0.0, 0.0, 5.0]
    assert r("found_and_outlier")["n_outliers_cleared"] == 1 and r("found_and_outlier")["n_found"] == 2 and r("found_and_outlier")["nmatches"] == 1
    assert np.array_equal(R["found_and_outlier"].matches, R["found_no_outlier_array"].matches) and R["found_no_outlier_array"].outlier is None
    # entries beyond the keyframe's count are kept, never followed, their features taken (the outlier flag of one changes nothing)
    assert m("bad_entry") == [0, 4, 2, 99] and r("bad_entry")["status"] == L.BAD_INPUT and r("bad_entry")["n_found"] == 0
    assert r("bad_entry")["n_outliers_cleared"] == 0 and r("bad_entry")["n_over_dist"] == 2
    # no depth test: the two points behind the camera project inside the bounds, ARE searched and take their features
    b = R["behind_the_camera"]
    assert b.points[1, 2] < 0 and b.points[3, 2] < 0 and e["behind_the_camera"]["proj"][:, 4].tolist() == [0.0, 1.0, 0.0, 1.0]
    assert m("behind_the_camera") == [0, 1, 2, 3] and r("behind_the_camera")["n_behind_kept"] == 2 and stage("behind_the_camera") == [5.0] * 4
    # z = +0 and z = -0: u is no number, which is outside the image
    z = R["zero_depth"]
    assert z.points[1, 2] == 0 and not np.signbit(z.points[1, 2]) and np.signbit(z.points[2, 2])
    assert r("zero_depth")["n_out_image"] == 2 and stage("zero_depth") == [5.0, 2.0, 2.0, 5.0] and r("zero_depth")["n_behind_kept"] == 0
    assert m("zero_depth") == [0, -1, -1, 3] and r("zero_depth")["status"] == 0
    on = e["on_the_bounds"]
    assert on["proj"][:2, 0].tolist() == [0.0, 640.0] and stage("on_the_bounds") == [5.0, 5.0, 2.0, 2.0]
    assert r("on_the_bounds")["n_out_image"] == 2
    outside = R["on_the_bounds"].variant(bounds=(-1, 641, 0, 480)).expected()["proj"]
    assert -1e-3 < outside[2, 0] < 0.0 and 640.0 < outside[3, 0] < 640.001  # (the two that were outside, by less than 0.001 pixel)
    # dist3D == 0.8f * min and dist3D == 1.2f * max stay, one f32 step beyond is out
    assert stage("distance_bounds") == [5.0, 3.0, 5.0, 3.0] and r("distance_bounds")["n_out_distance"] == 2
    # the level window [level - 1, level + 1]: octaves 1 and 5 around a point of level 3 are left out, 2 and 4 are candidates, and
    # the one at level + 1 (which matching the local map leaves out) is the match
    lw = R["level_window"]
    u, v, rad, lv = e["level_window"]["proj"][0, :4]
    assert lv == 3.0 and lw.kps_c["octave"].tolist() == [1, 2, 4, 5]
    assert sorted(L.features_in_area(lw.kps_c, lw.bounds, u, v, rad, 2, 4).tolist()) == [1, 2] and m("level_window") == [-1, -1, 0, -1]
    # orb_dist: candidates at 64, 65, 100 and 101 bits against 64 and against 100
    dist = lambda a, b: int(np.unpackbits(a ^ b).sum())  # noqa: E731
    w64 = R["orb_dist_64"]
    assert [dist(w64.desc_k[k], w64.desc_c[k]) for k in range(4)] == [64, 65, 100, 101]
    assert m("orb_dist_64") == [0, -1, -1, -1] and r("orb_dist_64")["n_over_dist"] == 3 and e["orb_dist_64"]["best"].tolist() == [64, 65, 100, 101]
    assert m("orb_dist_100") == [0, 1, 2, -1] and r("orb_dist_100")["n_over_dist"] == 1
    # orb_dist 0 takes an identical descriptor only; 256 takes everything but a candidate at 256, which is never below the start
    assert m("orb_dist_0") == [0, -1, 2, 3] and e["orb_dist_0"]["best"].tolist() == [0, 1, 0, 0]
    assert m("orb_dist_256") == [0, 1, 2, -1] and e["orb_dist_256"]["best"][3] == 256 and min(e["orb_dist_256"]["best"][:3]) > 100
    # the histogram: only new matches vote (with the entry's two, 270 degrees would be the second bin and 180 would go), the
    # entry's matches survive their losing bin
    assert m("histogram_new_matches_only") == [0, 1, 2, 3, 4, 5, 6, 7, 8, -1, 10, 11]
    assert r("histogram_new_matches_only")["n_rot_removed"] == 1 and r("histogram_new_matches_only")["nmatches"] == 9
    assert m("no_orientation") == list(range(12)) and r("no_orientation")["n_rot_removed"] == 0 and r("no_orientation")["nmatches"] == 10
    assert m("point_descriptors") == [0, 1, 2, 3] and m("frame_descriptors") == [-1] * 4 and r("frame_descriptors")["n_over_dist"] == 4
    assert m("nonfinite_point") == [-1, 1, -1, 3] and r("nonfinite_point")["status"] == L.NONFINITE and r("nonfinite_point")["n_points"] == 4
    assert r("nonfinite_pose")["status"] == L.NONFINITE and r("nonfinite_pose")["nmatches"] == 0 and r("nonfinite_pose")["n_with_candidates"] == 0
    assert r("no_features")["n_points"] == 4 and r("no_features")["n_with_candidates"] == 0 and len(m("no_features")) == 0
    assert r("no_points") == dict.fromkeys(L.RESULT_FIELDS, 0) and m("no_points") == [-1] * 4


def test_hand_made_order_case():
    """0 -> A, 1 -> B (its first choice A is taken), 2 -> none; "the lowest claimant of its first choice wins" would give B to
    point 2, whose first choice it is and which point 1 does not pick first."""
    w = L.world("order")
    e = w.expected()
    dist = lambda a, b: int(np.unpackbits(a ^ b).sum())  # noqa: E731
    A, B = w.desc_c
    d = w.desc_k
    assert [dist(d[0], A), dist(d[1], A), dist(d[1], B), dist(d[2], A), dist(d[2], B)] == [0, 1, 5, 8, 2]
    cands = [sorted(L.features_in_area(w.kps_c, w.bounds, *e["proj"][i, :3], -1, 1).tolist()) for i in range(3)]
    assert cands == [[0], [0, 1], [0, 1]]
    assert e["matches"].tolist() == [0, 1] and e["outcome"].tolist() == [0, 1, -1]
    # alone, point 1 takes A and point 2 takes B: first choices A, A, B
    assert e["alone"].tolist() == [0, 0, 1] and e["res"]["n_displaced"] == 2


def test_conditions_on_the_generated_worlds():
    """What the GPU comparison relies on: the main world (about 400 features against a 600-point keyframe) takes every way out,
    and matches, at least five times; the contention world (about 280 points in overlapping windows) displaces at least half
    of its searched points."""
    w = L.world("main")
    e = w.expected()
    r = e["res"]
    searched = int((e["proj"][:, 5] == 5.0).sum())
    assert w.n_k == 600 and 350 <= w.n_c <= 450
    masked = int(((w.mask == 0) & ~np.isin(np.arange(w.n_k), w.matches[w.matches >= 0])).sum())
    ways = dict(found=r["n_found"], masked=masked, behind_kept=r["n_behind_kept"], out_image=r["n_out_image"], out_distance=r["n_out_distance"],
                no_candidate=searched - r["n_with_candidates"], over_dist=r["n_over_dist"], displaced=r["n_displaced"],
                rot_removed=r["n_rot_removed"], outliers_cleared=r["n_outliers_cleared"], matched=r["nmatches"])
    for k, v in ways.items():
        assert v >= 5, (k, v)
    assert r["status"] == 0 and set(e["proj"][e["proj"][:, 5] == 5.0, 3].astype(int).tolist()) == set(range(L.NLEVELS))
    c = L.world("contention")
    ce = c.expected()
    cs = int((ce["proj"][:, 5] == 5.0).sum())
    assert 260 <= c.n_k <= 300 and cs == c.n_k and 2 * ce["res"]["n_displaced"] >= cs and ce["res"]["nmatches"] > 100
    w7 = L.world("w700")
    assert w7.n_k == 700 > 512 and w7.expected()["res"]["nmatches"] > 40
    t3 = L.world("main_th3")
    assert t3.th == 3.0 and t3.orb_dist == 64 and t3.outlier is None and t3.expected()["res"]["nmatches"] > 20
    assert L.world("pdesc").point_desc is not None and not L.world("pdesc").ori


def test_chain_worlds_take_their_paths():
    """The four candidates of the relocalisation chain (tests/test_gpu_match_kfproj.py runs them in one batch): one reaches 50
    inliers at the first pose call, one has fewer than 10, one needs both searches and ends at or above 50, one stops because
    nadditional + nGood < 50."""
    got = {name: L.relocalize_refine(*L.chain_world(name)) for name in L.CHAIN}
    for name, a in got.items():
        print(name, a["stage"], a["n_good"], a["trace"])
    assert got["enough_at_once"]["stage"] == 1 and got["enough_at_once"]["n_good"] >= 50
    assert got["dropped"]["stage"] == 1 and got["dropped"]["n_good"] < 10
    both = got["both_searches"]
    assert both["stage"] == 5 and both["n_good"] >= 50 and both["trace"][0] < 50 and 30 < both["trace"][2] < 50
    few = got["too_few_additional"]
    assert few["stage"] == 2 and 10 <= few["trace"][0] < 50 and few["trace"][0] + few["trace"][1] < 50


def test_cpp_shim_match_kfproj_compiles_and_links(orbx, tmp_path):
    """tests/cpp/shim_match_kfproj.cpp -- ORBmatcher::SearchByProjection(F, KeyFrameView, row, th, ORBdist) of
    include/orbx_shim.hpp on a Frame-like type and on a FrameView -- builds against the C ABI alone; without a device it fails
    loudly (tests/test_gpu_match_kfproj.py runs it)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = os.path.join(str(tmp_path), "shim_match_kfproj"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "shim_match_kfproj.cpp"),
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
