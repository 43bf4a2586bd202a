"""The CPU restatement of the local bundle adjustment (tests/cpp/lba_ref.cpp over csrc/orbx_lba_math.inc; include/orbx.h, "local
mapping: local bundle adjustment") against what does not share its code: an independent numpy statement of the first
Levenberg-Marquardt step, the two-view restatement on a world both can run, properties that need no tolerance, ground truth,
and a stand-alone program under the sanitizers.  tests/test_gpu_lba.py then holds the device to the restatement bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import ba_ref_lib as B
import lba_ref_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = ("window", "truth", "far", "lonely", "idle", "nofixed", "rejecting", "losing")
# Measured on the development machine: the largest relative difference (max |a - b| / max |b| per vector, test_ba_host._rel)
# between the restatement's first step and the numpy statement's over WORLDS and "second", in xp, xl, chi2_initial and lambda
# (the largest: truth, xp, 1.20e-5).  The numerical derivatives (central differences, h = 1e-6) dominate it, so the tests assert
# 100 times this value.
STEP_MEASURED = 1.2e-5
# Measured likewise: the distance to the truth behind the adjustment of "truth" (no pixel noise; f32 keypoints, poses and points
# and 15 iterations set the floor): the points' largest error (from 0.099 at the start) and the free poses' largest translation
# error (from 0.0216).
TRUTH_POINTS_MEASURED = 9.4e-4
TRUTH_POSES_MEASURED = 1.04e-4


def kw_of(name):
    return dict(inv_sigma2=L.inv_sigma2_of("second"), nlevels=L.NLEVELS_2) if name == "second" else {}


@pytest.fixture(scope="module")
def results():
    """{world: (result, poses, points, outlier, counters)} of the restatement, computed once and left unchanged."""
    return {name: L.local_ba(L.world(name), **kw_of(name)) for name in WORLDS + ("second",)}


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def test_first_step_agrees_with_the_numpy_statement():
    """The graph from the rows, the Schur elimination over several free poses, the dense Cholesky solve, the Jacobians and
    Huber's weights against numerically differentiated residuals and one dense solve of the full (6 F + 3 P) damped normal
    equations."""
    worst = 0.0
    for name in WORLDS + ("second",):
        w = L.world(name)
        a, b = L.first_step(w, **kw_of(name)), L.first_step_numpy(w, **kw_of(name))
        assert a is not None and list(a["pidx"]) == list(b["pidx"]) and list(a["free"]) == list(b["free"]), name
        figures = [_rel(a["xp"], b["xp"]), _rel(a["xl"], b["xl"]), _rel(a["chi2_initial"], b["chi2_initial"]), _rel(a["lam"], b["lam"])]
        print(name, figures)
        worst = max(worst, *figures)
    print("worst", worst)
    assert worst <= 100 * STEP_MEASURED


def test_first_step_agrees_with_the_two_view_restatement():
    """One free and one fixed keyframe at the identity with the two-view world's points: the same first step as
    ba_ref_lib.first_step up to the order of the sums and Huber's delta, sqrt(5.991) here against sqrt(5.99) there, which moves
    the weight of an edge in the outlier branch by 1e-4 of itself (measured: 3.7e-5 in lambda, the largest of the four)."""
    pair = B.world("general")
    a, b = L.first_step(L.two_view_world(pair)), B.first_step(pair)
    assert list(a["pidx"]) == list(b["idx"]) and list(a["free"]) == [0]
    figures = [_rel(a["xp"][0], b["xp"]), _rel(a["xl"], b["xl"]), _rel(a["chi2_initial"], b["chi2_initial"]), _rel(a["lam"], b["lam"])]
    print(figures)
    assert max(figures) <= 100 * STEP_MEASURED


def test_chi2_never_grows_within_a_round_and_rotations_are_rotations(results):
    for name, (r, po, _, _, _) in results.items():
        w = L.world(name)
        for k in range(2):
            assert r["chi2_final"][k] <= r["chi2_initial"][k], (name, k)
        # unit quaternions: the rotation matrices written from them are orthonormal to f32 rounding (nine entries rounded to 2^-24
        # relative, three products per entry of R R^T: below 2^-21)
        for e in range(w.n_free):
            R = po[e, :9].reshape(3, 3).astype(np.float64)
            assert np.abs(R @ R.T - np.eye(3)).max() < 2.0 ** -21 and np.linalg.det(R) > 0, (name, e)


def test_fixed_poses_come_back_bit_for_bit(results):
    for name, (_, po, _, _, _) in results.items():
        w = L.world(name)
        assert po[w.n_free:].tobytes() == w.pose[w.n_free:].tobytes(), name


def test_no_iterations_return_the_inputs_and_classify():
    w = L.world("window")
    r, po, pts, outlier, _ = L.local_ba(w, 0, 0)
    assert r["status"] == 0 and r["iterations"].sum() == 0 and r["lm_trials"].sum() == 0
    assert pts.tobytes() == w.map_pts.tobytes() and po[:, 9:].tobytes() == w.pose[:, 9:].tobytes()
    assert np.abs(po[:, :9] - w.pose[:, :9]).max() < 2.0 ** -20  # (through the normalised quaternion: a few f32 roundings)
    assert r["n_level1"] > 0 and outlier.sum() == r["n_erased"] >= r["n_level1"]


def test_a_vertex_without_an_active_edge_keeps_its_bits():
    """losing: some points lose every edge between the rounds.  Round 2 must leave exactly those as round 1 left them; the
    others move."""
    w = L.world("losing")
    full, _, pts_full, _, _ = L.local_ba(w, 5, 10)
    _, _, pts_one, _, _ = L.local_ba(w, 5, 0)
    vertices = L.graph(w)[0]
    kept = (pts_full[vertices].view(np.uint32) == pts_one[vertices].view(np.uint32)).all(axis=1)
    lost = full["n_points"] - full["n_active_points"][1]
    assert lost > 0 and int(kept.sum()) == lost
    # ... and a free keyframe that observes nothing keeps its pose's bits up to the quaternion's round trip: it is not in the system
    w = L.world("idle")
    r, po, _, _, _ = L.local_ba(w)
    r0, po0, _, _, _ = L.local_ba(w, 0, 0)
    idle = w.n_free - 1
    assert r["n_active_free"][0] == w.n_free - 1 and po[idle].tobytes() == po0[idle].tobytes()
    assert po[0].tobytes() != po0[0].tobytes()


def test_the_worlds_run_every_branch(results):
    r = {name: v[0] for name, v in results.items()}
    assert r["rejecting"]["rejected_trials"].sum() > 0  # a rejected trial
    assert any(2 in v["stop_reason"] for v in r.values())  # the _nBad rule
    assert any(0 in v["stop_reason"] for v in r.values())  # every iteration ran
    assert r["window"]["n_level1"] > 0 and r["window"]["n_erased"] > 0  # level-1 edges
    assert r["losing"]["n_active_points"][1] < r["losing"]["n_active_points"][0]  # a point that loses all its edges
    assert r["idle"]["n_active_free"][0] == r["idle"]["n_free"] - 1  # a free keyframe with no observation
    assert L.world("nofixed").n_entries == L.world("nofixed").n_free and r["nofixed"]["iterations"][0] > 0  # no fixed keyframe
    # a point seen by fixed keyframes and one free keyframe only; points only fixed keyframes see are no vertices
    w = L.world("lonely")
    vertices, edges, _, _ = L.graph(w)
    free_obs = np.bincount(edges[edges[:, 0] < w.n_free, 2], minlength=len(vertices))
    fixed_obs = np.bincount(edges[edges[:, 0] >= w.n_free, 2], minlength=len(vertices))
    assert ((free_obs == 1) & (fixed_obs == w.n_entries - w.n_free)).sum() >= 10
    assert r["lonely"]["n_points"] == len(vertices) == 64 and r["lonely"]["n_edges"] == len(edges)
    # a failed solve: under a table of zeros every pivot is 0
    z = L.local_ba(L.world("window"), inv_sigma2=L.zero_table())[0]
    assert z["status"] == 0 and list(z["solver_failures"]) == [10, 10] and list(z["stop_reason"]) == [1, 1] and list(z["iterations"]) == [1, 1]
    for name, v in r.items():
        assert v["status"] == 0 and v["n_edges"] == len(L.graph(L.world(name), **kw_of(name))[1]), name


def edge_chi2(w, po, pts, **kw):
    """chi2 of every edge at the f32 outputs, in numpy."""
    vertices, edges, obs, wt = L.graph(w, **kw)
    R, t = L.pose_matrices(po)
    X = pts[vertices].astype(np.float64)
    Kd = w.K.reshape(3, 3).astype(np.float64)
    Y = np.einsum("mij,mj->mi", R[edges[:, 0]], X[edges[:, 2]]) + t[edges[:, 0]]
    e = obs - np.c_[Y[:, 0] / Y[:, 2] * Kd[0, 0] + Kd[0, 2], Y[:, 1] / Y[:, 2] * Kd[1, 1] + Kd[1, 2]]
    return wt * (e ** 2).sum(axis=1), Y[:, 2]


def test_ground_truth(results):
    """truth: no pixel noise, perturbed free poses and points, two fixed keyframes: the adjustment finds the scene."""
    w = L.world("truth")
    r, po, pts, outlier, _ = results["truth"]
    X = w.truth["X"]
    vertices = L.graph(w)[0]
    before = np.abs(w.map_pts[vertices] - X[vertices]).max()
    after = np.abs(pts[vertices] - X[vertices]).max()
    tb = max(np.abs(w.pose[e, 9:] - w.truth["t"][e]).max() for e in range(w.n_free))
    ta = max(np.abs(po[e, 9:] - w.truth["t"][e]).max() for e in range(w.n_free))
    print("points", before, after, "poses", tb, ta)
    assert after < before and ta < tb
    assert after <= 100 * TRUTH_POINTS_MEASURED and ta <= 100 * TRUTH_POSES_MEASURED
    # the discrete outcome is not at the mercy of a rounding: no edge within 1e-3 of the threshold, every depth clearly positive
    chi2, depth = edge_chi2(w, po, pts)
    assert np.abs(chi2 - 5.991).min() > 1e-3 and depth.min() > 1.0
    assert r["n_erased"] == 0 and not outlier.any() and r["n_level1"] == 0


@pytest.mark.parametrize("name", ["window", "far", "losing", "second"])
def test_the_classification_against_numpy(results, name):
    """The worlds with level-1 edges: chi2 of every edge recomputed in numpy at the f32 outputs.  No edge lies within 1e-3 of
    5.991 and every depth is clearly positive, so the discrete outcome is not at the mercy of a rounding.  Round 2's last trial
    was accepted in these worlds, so the errors the classification reads are those of the final estimates: every edge above the
    threshold is erased, every edge kept is below it, and the erased edges below it -- level-1 edges, which keep round 1's error
    (rule 3) -- are no more than n_level1."""
    w = L.world(name)
    r, po, pts, outlier, _ = results[name]
    chi2, depth = edge_chi2(w, po, pts, **kw_of(name))
    edges = L.graph(w, **kw_of(name))[1]
    erased = outlier[edges[:, 0], edges[:, 1]] != 0
    assert r["rejected_trials"][1] == 0 and r["n_level1"] > 0
    assert np.abs(chi2 - 5.991).min() > 1e-3 and depth.min() > 1.0
    assert erased[chi2 > 5.991].all() and (chi2[~erased] < 5.991).all()
    assert 0 <= int((erased & (chi2 < 5.991)).sum()) <= r["n_level1"]
    assert int(erased.sum()) == r["n_erased"] == int(outlier.sum()) >= r["n_level1"]


def test_sanitized_stand_alone_program(tmp_path):
    """tests/cpp/lba_ref_main.cpp: the restatement over small windows and every garbage case under AddressSanitizer and
    UndefinedBehaviorSanitizer, as a program of its own (nothing sanitised is loaded into Python)."""
    exe = L.build(flags=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"),
                  exe_main=os.path.join(ROOT, "tests", "cpp", "lba_ref_main.cpp"))
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and "all fine" in p.stdout, p.stdout[-4000:]
