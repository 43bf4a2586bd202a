"""Both overloads of ORBmatcher::Fuse (include/orbx.h, "fusing map points into a keyframe") on the CPU: the restatement
tests/cpp/fuse_ref.cpp, which the device is compared with byte for byte (tests/test_gpu_fuse.py), is itself pinned here -- its window
search to the reference's own compiled Frame::GetFeaturesInArea (tests/ref_lib.py), the whole of it to a second statement in numpy
that has no grid and resolves feature by feature, every rule edge to the counter it aims at, the hand-made order case written out,
and the restatement runs under the sanitizers in a program of its own.  Every test first asserts on the restatement's own counters
that its world does what it is for."""
import os
import subprocess

import numpy as np
import pytest

import fuse_ref_lib as L

NAMED = [(f, n) for f in L.FORMS for n in L.WORLDS + L.WORLDS_2]
RULES = sorted(L.rule_worlds())
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fuses(w):
    """What a generated world is for: it searches, fuses and leaves points over th_low."""
    r = w.expected()["res"]
    assert r["n_fused"] > 0 and r["n_with_candidates"] >= r["n_fused"], r
    return r


def contends(w):
    r = w.expected()["res"]
    for f in ("n_added", "n_kept_occupant", "n_bad_occupant", "n_chained", "n_over_dist") + (("n_replaced_occupant",) if w.form == "pose" else ()):
        assert r[f] > 0, (f, r)
    return r


@pytest.fixture(scope="module")
def ref():
    import ref_lib
    ref_lib.lib()
    return ref_lib


@pytest.mark.parametrize("form,name", NAMED)
def test_window_search_is_the_references(ref, form, name):
    """For every searched point the restatement's candidate list is the reference's GetFeaturesInArea(u, v, th * scale[level])
    without level bounds, order included."""
    w = L.world(form, name)
    fuses(w)
    e = w.expected()
    searched = np.flatnonzero(e["stage"] == L.SEARCHED)
    assert len(searched) > 0
    some = 0
    for i in searched:
        u, v, r = (float(x) for x in e["proj"][i, :3])
        want = ref.features_in_area(w.kps, w.bounds, u, v, r, -1, -1)
        got = L.features_in_area(w.kps, w.bounds, u, v, r, -1, -1)
        assert np.array_equal(got, want), (form, name, int(i))
        some += len(want) > 0
    assert some > 0


def _same(w, what):
    e = w.expected()
    row, idx, act, other, res = L.fuse_numpy(w)
    assert row.tobytes() == e["matches"].tobytes(), what
    assert idx.tobytes() == e["idx"].tobytes() and act.tobytes() == e["act"].tobytes() and other.tobytes() == e["other"].tobytes(), what
    for f, v in res.items():
        assert e["res"][f] == v, (what, f, e["res"][f], v)
    assert e["res"]["rounds"] == 0


@pytest.mark.parametrize("form,name", NAMED)
def test_restatement_equals_the_numpy_statement(form, name):
    w = L.world(form, name)
    contends(w) if name == "contention" else fuses(w)
    _same(w, (form, name))


@pytest.mark.parametrize("key", RULES)
def test_rule_worlds_equal_the_numpy_statement(key):
    _same(L.rule_worlds()[key], key)


@pytest.mark.parametrize("key", RULES)
def test_rule_worlds_take_their_branch(key):
    """The counters (and status bits) a rule world aims at, on the restatement: no world passes by missing its edge."""
    res = L.rule_worlds()[key].expected()["res"]
    aims = L.RULE_AIMS[key]
    assert aims
    for f, v in aims.items():
        if f == "status":
            assert (res["status"] & v == v) if v else res["status"] == 0, (key, res)
        else:
            assert res[f] == v, (key, f, res)


@pytest.mark.parametrize("form", L.FORMS)
def test_rule_edges_in_detail(form):
    """What the counters alone do not say: which point took which branch."""
    rw = {n: w for (f, n), w in L.rule_worlds().items() if f == form}
    pose = form == "pose"
    st = lambda n: [L.STAGES[s] for s in rw[n].expected()["stage"]]  # noqa: E731
    act = lambda n: list(rw[n].expected()["act"])  # noqa: E731
    assert st("zero_and_negative_depth") == ["searched", "out_image", "searched", "behind"]
    assert st("on_the_bounds") == ["searched", "out_image", "searched", "out_image"]
    e = rw["on_the_bounds"].expected()
    assert e["proj"][0, 0] == 0.0 and e["proj"][2, 1] == 0.0  # (exactly on min_x and on min_y)
    assert st("distance_bounds") == ["searched", "out_distance", "searched", "out_distance"]
    assert st("angle_edge") == ["searched", "out_angle", "out_angle"]
    w = rw["angle_edge"]  # the second normal is skipped only by the f64 comparison: its f32 cosine is 0.5 again
    dot = float(w.points[1, 0]) * float(w.normals[1, 0]) + float(w.points[1, 2]) * float(w.normals[1, 2])
    assert dot < 1.25 and np.float32(dot / 2.5) == np.float32(0.5)
    e = rw["octave_window"].expected()
    assert list(e["idx"]) == [-1, 2]
    assert len(L.features_in_area(rw["octave_window"].kps, L.BOUNDS, *e["proj"][0, :3])) == 2  # (both in the window, both refused)
    e, w = rw["chi_square_edge"].expected(), rw["chi_square_edge"]
    chi = [float(np.float32((e["proj"][i, 0] - w.kps["x"][i]) ** 2)) for i in range(2)]
    assert chi[0] < 5.99 < chi[1] and list(e["idx"]) == ([0, -1] if pose else [0, 1])
    assert act("distance_50_and_51") == [L.ADD, L.NONE]
    assert act("distance_256") == ([L.NONE] if pose else [L.ADD])
    e = rw["obs_equal_and_greater"].expected()
    assert list(e["act"]) == ([L.REPLACE, L.KEEP, 0, 0] if pose else [L.KEEP, L.KEEP, 0, 0]) and list(e["other"]) == [2, 3, -1, -1]
    assert list(e["matches"]) == ([0, 3, -1, -1] if pose else [2, 3, -1, -1])
    e = rw["bad_occupant_stays"].expected()
    assert list(e["act"]) == [L.BAD, L.BAD, 0, 0] and list(e["other"]) == [3, 3, -1, -1] and list(e["matches"]) == [3]
    e = rw["unmapped_with_counts"].expected()
    assert list(e["act"]) == ([L.REPLACE, L.KEEP, L.BAD, L.ADD] if pose else [L.KEEP, L.KEEP, L.BAD, L.ADD])
    assert list(e["matches"]) == ([0, L.UNMAPPED, L.UNMAPPED, 3] if pose else [L.UNMAPPED] * 3 + [3])
    assert list(e["other"]) == [L.UNMAPPED] * 3 + [-1]
    e = rw["unmapped_without_counts"].expected()
    assert list(e["act"]) == ([L.BAD] * 3 + [L.ADD] if pose else [L.KEEP] * 3 + [L.ADD])
    e = rw["entry_beyond_the_set"].expected()
    assert list(e["act"]) == [L.ADD, L.BAD, L.ADD, L.BAD] and list(e["matches"]) == [0, 4, 2, 99] and list(e["other"]) == [-1, 4, -1, 99]
    e = rw["counts_out_of_range"].expected()
    assert list(e["act"]) == ([L.REPLACE, L.REPLACE, L.KEEP, L.ADD] if pose else [L.KEEP] * 3 + [L.ADD])
    assert list(rw["masked_point_named"].expected()["act"]) == [L.BAD, 0, L.ADD, L.ADD]  # (feature 0 holds the masked-out point 1)
    e = rw["nonfinite_pose"].expected()
    assert list(e["matches"]) == [1, -1, -1, -1] and not e["act"].any()
    assert list(rw["nonfinite_point"].expected()["act"]) == [0, 0, 0, L.ADD]


@pytest.mark.parametrize("key", [(f, n) for f, n in NAMED] + RULES)
def test_counters_add_up(key):
    w = L.world(*key) if key in NAMED else L.rule_worlds()[key]
    e = w.expected()
    r, stage, act = e["res"], e["stage"], e["act"]
    count = lambda s: int((stage == L.STAGES.index(s)).sum())  # noqa: E731
    assert r["n_fused"] == r["n_added"] + r["n_kept_occupant"] + r["n_replaced_occupant"] + r["n_bad_occupant"] == int((e["idx"] >= 0).sum())
    assert r["n_points"] == r["n_behind"] + r["n_out_image"] + r["n_out_distance"] + r["n_out_angle"] + count("searched") + count("dropped")
    assert (r["n_behind"], r["n_out_image"], r["n_out_distance"], r["n_out_angle"]) == tuple(
        count(s) for s in ("behind", "out_image", "out_distance", "out_angle"))
    assert r["n_with_candidates"] == r["n_fused"] + r["n_over_dist"] <= count("searched")
    assert (r["n_added"], r["n_kept_occupant"], r["n_replaced_occupant"], r["n_bad_occupant"]) == tuple(
        int((act == a).sum()) for a in (L.ADD, L.KEEP, L.REPLACE, L.BAD))
    # the row on exit is the entry plus the ADD / REPLACE decisions, the last one on a feature standing
    row = w.matches.copy()
    for i in np.flatnonzero((act == L.ADD) | (act == L.REPLACE)):
        row[e["idx"][i]] = i
    assert row.tobytes() == e["matches"].tobytes()
    assert (e["other"][act == L.ADD] == -1).all() and (e["other"][act == L.NONE] == -1).all()
    if w.form == "scw":
        assert r["n_replaced_occupant"] == 0
    if count("dropped") and not r["status"] & L.NONFINITE:
        raise AssertionError("a dropped point without the bit")


@pytest.mark.parametrize("form", L.FORMS)
def test_hand_made_order_case(form):
    """Three points with 4, 9 and 2 observations on one free feature, every output written out by hand."""
    w = L.world(form, "order")
    e = w.expected()
    assert list(e["idx"]) == [0, 0, 0]
    if form == "pose":  # added (count 5); 5 <= 9: replaces point 0 (count 14); 14 > 2: point 1 stays
        assert list(e["act"]) == [L.ADD, L.REPLACE, L.KEEP] and list(e["other"]) == [-1, 0, 1] and list(e["matches"]) == [1]
        want = dict(n_fused=3, n_added=1, n_replaced_occupant=1, n_kept_occupant=1, n_bad_occupant=0, n_chained=2)
    else:  # added; both later points get point 0 as the point to be replaced by
        assert list(e["act"]) == [L.ADD, L.KEEP, L.KEEP] and list(e["other"]) == [-1, 0, 0] and list(e["matches"]) == [0]
        want = dict(n_fused=3, n_added=1, n_replaced_occupant=0, n_kept_occupant=2, n_bad_occupant=0, n_chained=2)
    want.update(status=0, n_points=3, n_in_kf=0, n_with_candidates=3, n_over_dist=0, n_behind=0, n_out_image=0, n_out_distance=0, n_out_angle=0,
                rounds=0)
    assert e["res"] == want


def test_conditions_on_the_generated_worlds():
    """What the GPU test relies on: sizes, every kind of entry, contention with every action inside one chain."""
    for form in L.FORMS:
        for name in ("main", "w513", "w150@2"):
            w = L.world(form, name)
            r = fuses(w)
            assert r["n_in_kf"] > 5 and r["n_added"] > 5 and r["n_over_dist"] > 0 and r["status"] == 0, (form, name, r)
            assert min(r["n_behind"], r["n_out_image"], r["n_out_distance"], r["n_out_angle"]) > 5, (form, name)
            assert (w.matches == L.UNMAPPED).sum() > 5 and (w.occ_obs < 0).any()
        assert 350 <= L.world(form, "main").n_f <= 500 and L.world(form, "main").n_m == 600
        assert L.world(form, "w513").n_m == 513 and (L.world(form, "tiny").n_f, L.world(form, "tiny").n_m) == (2, 2)
        w2 = L.world(form, "w150@2")
        assert len(w2.scale) == 5 and w2.K[0] != w2.K[4] and w2.inv_sigma2.tobytes() == L.inv_sigma2_table(5, L.SCALE_FACTOR_2).tobytes()
        w = L.world(form, "contention")
        contends(w)
        e = w.expected()
        assert len(w.clusters) == 40 and all(3 <= len(p) <= 7 for _, _, p in w.clusters)
        for kind, f, pts in w.clusters:  # every point of a cluster picks the cluster's feature
            assert (e["idx"][pts] == f).all(), (kind, f)
        assert {k for k, _, _ in w.clusters} == set(L.CLUSTER_KINDS)
        if form == "pose":  # one chain that draws an addition, a kept and a replaced occupant
            assert any({L.ADD, L.KEEP, L.REPLACE} <= set(e["act"][pts]) for _, _, pts in w.clusters)
    # the two forms differ where they should: the gate and the counts
    assert L.world("pose", "main").expected()["res"]["n_fused"] < L.world("scw", "main").expected()["res"]["n_fused"]


def test_cpp_shim_fuse_compiles_and_links(orbx, tmp_path):
    """tests/cpp/shim_fuse.cpp -- both ORBmatcher::Fuse overloads of include/orbx_shim.hpp -- builds against the C ABI alone, as does
    an existing shim program against the MapView that gained a member; without a device it fails loudly (tests/test_gpu_fuse.py
    runs it)."""
    libdir = os.path.dirname(orbx.lib_path())
    for prog in ("shim_fuse", "shim_match_scw"):
        exe = os.path.join(str(tmp_path), prog)
        cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", prog + ".cpp"),
               "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        p = subprocess.run([os.path.join(str(tmp_path), "shim_fuse"), "1"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode != 0 and "RESULT" not in p.stdout


def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/fuse_ref_main.cpp links the restatement into a program of its own (a generated world with every kind of entry and
    count, both forms, empty sides, a dead pose) built with -fsanitize=address,undefined: nothing sanitised is loaded into Python."""
    exe = str(tmp_path / "fuse_ref_main")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           L.SRC, os.path.join(ROOT, "tests", "cpp", "fuse_ref_main.cpp"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "FUSE REF OK" in p.stdout, p.stdout
