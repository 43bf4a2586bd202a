"""ORBmatcher::SearchByProjection (include/orbx.h, "matching by projection") on the CPU: the restatement
tests/cpp/match_proj_ref.cpp, which the device is compared with byte for byte (tests/test_gpu_match_proj.py), is itself pinned
here -- its window search to the reference's own compiled Frame::GetFeaturesInArea (tests/ref_lib.py), the whole of it to a second
statement in numpy that has no grid, to a world whose answer is known, to a hand-made case that separates the sequential rule from
its nearest wrong neighbour, and rule by rule."""
import numpy as np
import pytest

import match_proj_ref_lib as M

GENERATED = ("w300", "w300_noori", "w300_pdesc", "w310_bounds", "w40_th30", "contention")


@pytest.fixture(scope="module")
def ref():
    import ref_lib
    ref_lib.lib()
    return ref_lib


@pytest.mark.parametrize("name", GENERATED + ("truth", "order"))
def test_window_search_is_the_references(ref, name):
    """For every projected point the restatement's candidate list is the reference's GetFeaturesInArea(u, v, r, o - 1, o + 1),
    order included."""
    w = M.world(name)
    proj = w.expected()["proj"]
    seen = 0
    for i in np.flatnonzero(proj[:, 3] == 2.0):
        u, v, r = (float(x) for x in proj[i, :3])
        o = int(w.kps_l["octave"][i])
        want = ref.features_in_area(w.kps_c, w.bounds, u, v, r, o - 1, o + 1)
        got = M.features_in_area(w.kps_c, w.bounds, u, v, r, o - 1, o + 1)
        assert np.array_equal(got, want), (name, int(i))
        seen += len(want) > 1
    assert seen > 0


def test_pinned_worlds_cover_the_window_edges(ref):
    """What the pin above is worth: bounds that do not start at 0, octave 0 and the top octave, features outside the grid, and
    features a hair inside and a hair outside the radius, which the reference includes and leaves out."""
    w = M.world("w310_bounds")
    assert w.bounds[0] != 0 and w.bounds[2] != 0
    for name in ("w300", "w310_bounds"):
        w = M.world(name)
        e = w.expected()
        seen = e["proj"][:, 3] == 2.0
        assert {0, M.NLEVELS - 1} <= set(w.kps_l["octave"][seen].tolist())
        _, ok = ref.pos_in_grid(w.kps_c, w.bounds)
        assert (~ok).sum() >= 4
        inside = outside = 0
        for i, j, is_in in w.edge:
            u, v, r = (float(x) for x in e["proj"][i, :3])
            o = int(w.kps_l["octave"][i])
            got = ref.features_in_area(w.kps_c, w.bounds, u, v, r, o - 1, o + 1)
            assert (j in got) == is_in, (name, i, j, is_in)
            inside, outside = inside + is_in, outside + (not is_in)
        assert inside >= 10 and outside >= 10


@pytest.mark.parametrize("name", M.WORLDS + M.WORLDS_2)
def test_restatement_equals_the_numpy_statement(name):
    w = M.world(name)
    e = w.expected()
    m, nm = M.search_by_projection_numpy(w)
    assert np.array_equal(e["matches"], m) and e["res"]["nmatches"] == nm == int((e["matches"] >= 0).sum()), name
    if name.startswith("w") and w.n_l >= 280:
        assert nm >= w.n_l // 8, (name, nm)  # (a world that matches nothing would compare nothing)


@pytest.mark.parametrize("name", list(M.rule_worlds()))
def test_rule_worlds_equal_the_numpy_statement(name):
    w = M.rule_worlds()[name]
    e = w.expected()
    m, nm = M.search_by_projection_numpy(w)
    assert np.array_equal(e["matches"], m) and e["res"]["nmatches"] == nm, name


def test_truth_world():
    """Every visible point gets exactly its own feature, one rotation bin holds everything and nothing is removed."""
    w = M.world("truth")
    e = w.expected()
    assert w.visible.sum() > 200
    want = np.where(w.visible[w.truth], w.truth, -1)  # feature j of the current frame is the projection of point truth[j]
    assert np.array_equal(e["matches"], want)
    assert e["res"]["nmatches"] == int(w.visible.sum()) and e["res"]["n_rot_removed"] == 0 and e["res"]["n_displaced"] == 0


def test_hand_made_order_case():
    """0 -> A, 1 -> B, 2 -> none.  (The distances are 0 / 1, 5 / 8, 2: a table with d(2, A) = 50 beside d(1, A) = 1, d(1, B) = 5 and
    d(2, B) = 2 cannot exist -- the triangle inequality gives d(A, B) <= 6 and so d(2, A) <= 8 -- and 8 keeps every role: feature 2
    prefers B, and A is its worse, taken, candidate.)"""
    w = M.world("order")
    e = w.expected()
    dist = lambda a, b: int(np.unpackbits(a ^ b).sum())  # noqa: E731
    A, B = w.desc_c
    assert [dist(w.desc_l[0], A), dist(w.desc_l[1], A), dist(w.desc_l[1], B), dist(w.desc_l[2], A), dist(w.desc_l[2], B)] == [0, 1, 5, 8, 2]
    cands = [sorted(M.features_in_area(w.kps_c, w.bounds, *e["proj"][i, :3], -1, 1).tolist()) for i in range(3)]
    assert cands == [[0], [0, 1], [0, 1]]
    assert e["matches"].tolist() == [0, 1] and e["outcome"].tolist() == [0, 1, -1]
    assert e["free_pick"].tolist() == [0, 0, 1] and e["res"]["n_displaced"] == 2 and e["taken_ahead"].tolist() == [0, 1, 2]


def test_contention_world():
    w = M.world("contention")
    e = w.expected()
    assert e["res"]["n_displaced"] > 20
    matched = e["outcome"] >= 0
    assert (e["taken_ahead"][matched] >= 3).any()  # a feature that passed three taken candidates on the way to its pick
    starved = ~matched & (e["free_pick"] >= 0)
    assert starved.sum() > 10 and (e["taken_ahead"][starved] > 0).all()  # unmatched only because everything within 100 was taken


def test_rules():
    R = M.rule_worlds()
    e = {k: w.expected() for k, w in R.items()}
    r = lambda k: e[k]["res"]  # noqa: E731
    assert e["mask_and_outlier"]["matches"].tolist() == [0, -1, -1, 3] and r("mask_and_outlier")["n_points"] == 2
    assert e["behind_the_camera"]["matches"].tolist() == [0, -1, 2, -1]
    assert r("behind_the_camera")["n_points"] == 4 and r("behind_the_camera")["n_in_image"] == 2
    assert e["zero_depth"]["matches"].tolist() == [0, -1, 2, 3] and r("zero_depth")["status"] == 0
    on = e["on_the_bounds"]
    assert on["proj"][:2, 0].tolist() == [0.0, 640.0] and on["proj"][:, 3].tolist() == [2.0, 2.0, 1.0, 1.0]
    assert on["matches"].tolist() == [0, 1, -1, -1] and r("on_the_bounds")["n_in_image"] == 2
    outside = R["on_the_bounds"].variant(mask=np.array([0, 0, 1, 1], np.uint8), bounds=(-1, 641, 0, 480)).expected()["proj"]
    assert -1e-3 < outside[2, 0] < 0.0 and 640.0 < outside[3, 0] < 640.001  # (the two that were outside, by less than 0.001 pixel)
    assert e["distance_100_and_101"]["matches"].tolist() == [0, -1] and r("distance_100_and_101")["n_with_candidates"] == 2
    h3, h10 = e["histogram_three_bins"], e["histogram_tenth_rule"]
    assert h3["matches"].tolist() == list(range(9)) + [-1] and r("histogram_three_bins")["n_rot_removed"] == 1
    assert h10["matches"].tolist() == list(range(22)) + [-1, -1] and r("histogram_tenth_rule")["n_rot_removed"] == 2
    assert e["no_orientation"]["matches"].tolist() == list(range(10)) and r("no_orientation")["n_rot_removed"] == 0
    assert e["octave_out_of_table"]["matches"].tolist() == [0, -1, -1, 3]
    assert r("octave_out_of_table")["status"] == M.BAD_INPUT and r("octave_out_of_table")["n_points"] == 2
    assert e["nonfinite_point"]["matches"].tolist() == [0, -1, -1, 3] and r("nonfinite_point")["status"] == M.NONFINITE
    assert r("nonfinite_pose")["status"] == M.NONFINITE and r("nonfinite_pose")["nmatches"] == 0
    assert r("no_features") == dict.fromkeys(M.RESULT_FIELDS, 0) and len(e["no_features"]["matches"]) == 0
    assert e["point_descriptors"]["matches"].tolist() == [0, 1, 2, 3] and r("frame_descriptors")["nmatches"] == 0
    for k in R:
        assert r(k)["rounds"] == 0  # (the sequential statement has none)


def test_cpp_shim_match_proj_compiles_and_links(orbx, tmp_path):
    """tests/cpp/shim_match_proj.cpp -- ORBmatcher::SearchByProjection of include/orbx_shim.hpp on a Frame-like type and on
    FrameViews -- builds against the C ABI alone, as tests/test_host.py builds shim_demo.cpp; without a device it fails loudly
    (tests/test_gpu_match_proj.py runs it)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = os.path.join(str(tmp_path), "shim_match_proj"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "shim_match_proj.cpp"),
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
