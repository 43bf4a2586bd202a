"""The loop-closing overload ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) and the composition of Scw
(include/orbx.h, "loop closing: matching the loop's points under Scw") on the CPU: the restatement tests/cpp/match_scw_ref.cpp,
which the device is compared with byte for byte (tests/test_gpu_match_scw.py), is itself pinned here -- its window search to the
reference's own compiled Frame::GetFeaturesInArea (tests/ref_lib.py), the whole of it to a second statement in numpy that has no
grid and no claim rounds, every rule edge to the counter it aims at, the hand-made order case, the planted correspondences of a
world under a composed similarity, the composition to an f64 statement in numpy, the chain worlds to the paths they must take,
and the restatement runs under the sanitizers in a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import match_scw_ref_lib as L

GENERATED = ("main", "main_no_table", "bounds", "w513", "truth", "contention")
SEARCHED = L.STAGES.index("searched")


@pytest.fixture(scope="module")
def ref():
    import ref_lib
    ref_lib.lib()
    return ref_lib


@pytest.mark.parametrize("name", GENERATED + ("order",))
def test_window_search_is_the_references(ref, name):
    """For every searched point the restatement's candidate list is the reference's GetFeaturesInArea(u, v, th * scale[level])
    without level bounds, order included."""
    w = L.world(name)
    e = w.expected()
    several = 0
    for i in np.flatnonzero(e["stage"] == SEARCHED):
        u, v, r = (float(x) for x in e["proj"][i, :3])
        want = ref.features_in_area(w.kps, w.bounds, u, v, r, -1, -1)
        got = L.features_in_area(w.kps, w.bounds, u, v, r, -1, -1)
        assert np.array_equal(got, want), (name, int(i))
        several += len(want) > 1
    assert several > 0


def _same(w, name):
    e = w.expected()
    m, res = L.search_scw_numpy(w)
    assert m.tobytes() == e["matches"].tobytes(), name
    for f, v in res.items():
        if f != "n_displaced":  # (the numpy statement does not walk twice)
            assert e["res"][f] == v, (name, f, e["res"][f], v)


@pytest.mark.parametrize("name", L.WORLDS + L.WORLDS_2)
def test_restatement_equals_the_numpy_statement(name):
    _same(L.world(name), name)


@pytest.mark.parametrize("name", sorted(L.rule_worlds()))
def test_rule_worlds_equal_the_numpy_statement(name):
    _same(L.rule_worlds()[name], name)


@pytest.mark.parametrize("name", sorted(L.rule_worlds()))
def test_rule_worlds_take_their_branch(name):
    """The counters (and status bits) a rule world aims at, on the restatement: no world passes by missing its edge."""
    res = L.rule_worlds()[name].expected()["res"]
    aims = L.RULE_AIMS[name]
    assert aims
    for f, v in aims.items():
        if f == "status":
            assert res["status"] & v == v, (name, res)
        else:
            assert res[f] == v, (name, f, res)


def test_rule_edges_in_detail():
    """What the counters alone do not say: which point took which branch."""
    rw = L.rule_worlds()
    st = lambda n: [L.STAGES[s] for s in rw[n].expected()["stage"]]  # noqa: E731
    assert st("zero_and_negative_depth") == ["searched", "out_image", "searched", "behind"]
    assert st("on_the_bounds") == ["searched", "out_image", "searched", "out_image"]
    e = rw["on_the_bounds"].expected()
    assert e["proj"][0, 0] == 0.0 and e["proj"][2, 1] == 0.0  # (exactly on min_x and on min_y)
    assert st("distance_bounds") == ["searched", "out_distance", "searched", "out_distance"]
    assert st("angle_edge") == ["searched", "out_angle", "out_angle"]
    # the second normal is skipped only by the f64 comparison: its f32 cosine is 0.5 again
    w = rw["angle_edge"]
    dot = float(w.points[1, 0]) * float(w.normals[1, 0]) + float(w.points[1, 2]) * float(w.normals[1, 2])
    assert dot < 1.25 and np.float32(dot / 2.5) == np.float32(0.5)
    e = rw["octave_window"].expected()
    assert list(e["outcome"]) == [-1, 2] and e["res"]["n_with_candidates"] == 1
    assert len(L.features_in_area(rw["octave_window"].kps, L.BOUNDS, *e["proj"][0, :3])) == 2  # (both in the window, both refused)
    assert list(rw["distance_50_and_51"].expected()["best"]) == [50, 51]
    assert list(rw["distance_256"].expected()["best"]) == [256]
    assert list(rw["entry_minus_2"].expected()["matches"]) == [L.TAKEN_UNMAPPED, 1, 2, 3]
    assert list(rw["unmapped_translation"].expected()["matches"]) == [L.TAKEN_UNMAPPED, -1, 1, 3]
    assert list(rw["entry_beyond_the_set"].expected()["matches"]) == [0, 4, 2, 99]
    assert list(rw["table_beyond"].expected()["matches"]) == [4, 2, 2, 3]
    assert list(rw["masked_point_named"].expected()["matches"]) == [1, -1, 2, 3]
    assert list(rw["nonfinite_scw"].expected()["matches"]) == [3, -1, -1, -1]  # (the row as the entry pass left it)
    assert list(rw["zero_scw"].expected()["matches"]) == [-1] * 4


@pytest.mark.parametrize("name", L.WORLDS + L.WORLDS_2 + tuple(sorted(L.rule_worlds())))
def test_counters_add_up(name):
    w = L.world(name) if name in L.WORLDS + L.WORLDS_2 else L.rule_worlds()[name]
    e = w.expected()
    r, stage = e["res"], e["stage"]
    count = lambda s: int((stage == L.STAGES.index(s)).sum())  # noqa: E731
    assert r["n_points"] == r["n_behind"] + r["n_out_image"] + r["n_out_distance"] + r["n_out_angle"] + count("searched") + count("dropped")
    assert (r["n_behind"], r["n_out_image"], r["n_out_distance"], r["n_out_angle"]) == tuple(
        count(s) for s in ("behind", "out_image", "out_distance", "out_angle"))
    assert r["n_with_candidates"] == r["nmatches"] + r["n_over_dist"] <= count("searched")
    m = e["matches"]
    assert r["n_total"] == int(((m >= 0) | (m == L.TAKEN_UNMAPPED)).sum())
    assert r["n_unmapped"] == int((m == L.TAKEN_UNMAPPED).sum())
    assert r["nmatches"] == int((e["outcome"] >= 0).sum())
    assert r["n_displaced"] == int((e["outcome"] != e["alone"]).sum())
    if count("dropped") and not r["status"] & L.NONFINITE:
        raise AssertionError("a dropped point without the bit")


def test_hand_made_order_case():
    """The lower index wins the shared feature although the other point is nearer to it; the loser falls to its second candidate."""
    w = L.world("order")
    e = w.expected()
    assert list(e["outcome"]) == [0, 1] and list(e["alone"]) == [0, 0]
    assert list(e["best"]) == [10, 34] and e["res"]["n_displaced"] == 1
    assert list(e["matches"]) == [0, 1]


def test_conditions_on_the_generated_worlds():
    """What the GPU test relies on: sizes, a table with unmapped entries, contention, the append's second slice."""
    for name in ("main", "bounds", "w513", "w150@2", "w310_bounds@2"):
        w = L.world(name)
        r = w.expected()["res"]
        assert w.table is not None and r["n_unmapped"] > 0 and r["n_found"] > 10 and r["nmatches"] > 10 and r["n_over_dist"] > 0, name
        assert min(r["n_behind"], r["n_out_image"], r["n_out_distance"], r["n_out_angle"]) > 5, name
        assert r["status"] == 0
    assert L.world("main_no_table").table is None
    assert L.world("w513").n_m == 513
    assert len(L.world("w150@2").scale) == 5 and L.world("w150@2").K[0] != L.world("w150@2").K[4]
    r = L.world("contention").expected()["res"]
    assert r["n_displaced"] == 240 and r["nmatches"] == 160 and r["n_over_dist"] == 120


def test_planted_correspondences_are_found_under_the_composed_scw():
    w = L.world("truth")
    assert abs(float(w.sim3[12]) - 1.0) > 0.1
    assert w.scw.tobytes() == L.compose_scw(w.Tmw, w.sim3).tobytes()
    e = w.expected()
    on_entry = sum(w.matches[j] >= 0 for j, _ in w.planted)
    assert len(w.planted) > 100 and 20 < on_entry < len(w.planted) - 50
    for j, i in w.planted:
        assert e["matches"][j] == i, (j, i)
    assert e["res"]["n_total"] == len(w.planted) and e["res"]["nmatches"] == len(w.planted) - on_entry


def test_composition_equals_the_numpy_statement():
    rng = np.random.default_rng(3)
    for k in range(200):
        T2 = L.pose_of(1000 + k)
        T12 = L.pose_of(2000 + k)
        sim3 = np.r_[T12[:9], T12[9:] * np.float32(rng.uniform(0.5, 20)), np.float32(rng.uniform(0.2, 5.0))].astype(np.float32)
        assert L.compose_scw(T2, sim3).tobytes() == L.compose_scw_numpy(T2, sim3).tobytes(), k
    for bad in (12, 0, 10):
        s = sim3.copy()
        s[bad] = np.nan
        assert not L.compose_scw(T2, s).any() and not L.compose_scw_numpy(T2, s).any()
    for s12 in (0.0, -1.0, np.inf):
        s = sim3.copy()
        s[12] = s12
        assert not L.compose_scw(T2, s).any()
    P = T2.copy()
    P[4] = np.inf
    assert not L.compose_scw(P, sim3).any()


def test_composition_with_unit_scale_is_the_product_of_the_two_poses():
    """s12 = 1: Scw is Tcw of the matched keyframe composed with T12, [R12 Rmw | R12 tmw + t12]."""
    T2, T12 = L.pose_of(5), L.pose_of(6)
    sim3 = np.r_[T12, np.float32(1.0)].astype(np.float32)
    got = L.compose_scw(T2, sim3).astype(np.float64)
    R12, t12 = T12[:9].astype(np.float64).reshape(3, 3), T12[9:].astype(np.float64)
    Rm, tm = T2[:9].astype(np.float64).reshape(3, 3), T2[9:].astype(np.float64)
    want = np.r_[(R12 @ Rm).reshape(9), R12 @ tm + t12]
    assert np.abs(got - want).max() < 1e-6  # (f32 rounding of values below 2)
    ok, R, t, _ = L.decompose_numpy(L.compose_scw(T2, sim3))
    assert ok and np.abs(R.reshape(3, 3) @ R.reshape(3, 3).T - np.eye(3)).max() < 1e-6


def test_cpp_shim_match_scw_compiles_and_links(orbx, tmp_path):
    """tests/cpp/shim_match_scw.cpp -- ORBmatcher::SearchByProjection(KeyFrameView, Scw, MapView, vpMatched, th, K, bounds) of
    include/orbx_shim.hpp -- builds against the C ABI alone; without a device it fails loudly (tests/test_gpu_match_scw.py runs
    it)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = os.path.join(str(tmp_path), "shim_match_scw"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "shim_match_scw.cpp"),
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


def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/match_scw_ref_main.cpp links the restatement into a program of its own (a generated world with every kind of
    entry, empty sides, a dead similarity) built with -fsanitize=address,undefined: nothing sanitised is loaded into Python."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "match_scw_ref_main")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           L.SRC, os.path.join(root, "tests", "cpp", "match_scw_ref_main.cpp"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "MATCH SCW REF OK" in p.stdout, p.stdout


def test_chain_worlds_take_their_paths():
    """The three chain worlds of the GPU test on the four restatements: an accepted loop whose last step finds the neighbours'
    points, one without a similarity, and one the optimiser accepts whose nTotalMatches stays below 40."""
    got = {name: L.chain_world(name).expected() for name in L.CHAIN_WORLDS}
    assert [got[n]["accepted"] for n in L.CHAIN_WORLDS] == [True, False, False]
    a, b, c = (got[n] for n in L.CHAIN_WORLDS)
    assert a["opt"]["n_inliers"] >= 20 and a["scw_res"]["n_total"] >= 40 and a["scw_res"]["nmatches"] == L.chain_world("accepted").n_neighbours
    assert a["scw_res"]["n_unmapped"] == 5 and a["scw_res"]["status"] == 0
    assert b["opt"]["n_inliers"] < 20 and not b["scw"].any() and b["scw_res"]["status"] & L.NONFINITE
    assert c["opt"]["n_inliers"] >= 20 and 20 <= c["scw_res"]["n_total"] < 40 and c["scw_res"]["nmatches"] > 0
