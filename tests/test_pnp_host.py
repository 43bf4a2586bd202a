"""PnPsolver (include/orbx.h, "behind SearchByBoW: PnP RANSAC") without a GPU: the C ABI's refusals and the Python mirror,
SetRansacParameters' table against a direct evaluation, the sampler against a literal swap-and-pop on a real list, and what the
CPU restatement tests/cpp/pnp_ref.cpp is worth -- against ground truth with conditions that need no measured tolerance, against
an independently written numpy EPnP, its prefix resolution against its literal loop byte for byte, and worlds that each assert
from the result's own counters that they take their branch.  tests/test_gpu_pnp.py compares the device with this restatement
bit for bit.

One branch that one might look for cannot exist: best_it < found_it.  Refine depends on the best alone, and the best
is refined at the iteration it becomes best; a later qualifying iteration that leaves the best unchanged would run the same
Refine over the same set, which failed.  test_found_it_is_the_best_it asserts the equality over every world here instead."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pnp_ref_lib as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def draws_for(picks, N):
    """rand() values that make the sampler pick the correspondences `picks` (four distinct indices below N), in this order."""
    avail, out = list(range(N)), []
    for idx in picks:
        pos, size = avail.index(idx), len(avail)
        r = -(-pos * (Q.RAND_MAX + 1) // size)  # the smallest r with (int)(r / 2^31 * size) == pos
        out.append(r)
        avail[pos] = avail[-1]
        avail.pop()
    assert Q.list_sampler(out, N) == list(picks)
    return out


# name -> (world, draws): made once, solved once per mode
def _worlds():
    W = {}
    W["clean"] = (Q.make_world(200, 1, outliers=40, noise=0.0), Q.make_draws(35, 1))
    W["clean_matched"] = (Q.make_world(150, 2, outliers=30, noise=0.0, matched=True), Q.make_draws(35, 2))
    W["noisy"] = (Q.make_world(200, 2, outliers=40, noise=0.5), Q.make_draws(35, 1))
    W["noisy_b"] = (Q.make_world(120, 4, outliers=30, noise=0.5), Q.make_draws(35, 4))
    W["unrefined"] = (Q.make_world(20, 100, outliers=10, noise=0.0), Q.make_draws(35, 0))
    W["second_try"] = (Q.make_world(40, 210, outliers=16, noise=1.0), Q.make_draws(60, 1))
    W["second_try_b"] = (Q.make_world(40, 228, outliers=16, noise=1.0), Q.make_draws(60, 2))
    W["planar"] = (Q.planar_world(80, 5), Q.make_draws(35, 5))
    for k, n in enumerate((3, 4, 9, 10, 11, 20)):
        # (N = 10 runs one iteration: the draws are chosen so that its four points give a pose all ten agree with)
        W["n%d" % n] = (Q.make_world(n, 60 + k, noise=0.0), Q.make_draws(35, 1 if n == 10 else 60 + k))
    for seed in range(300, 306):
        W["mixed%d" % seed] = (Q.make_world(50, seed, outliers=10, noise=0.5), Q.make_draws(35, seed - 300))
    # four features matched to one map point, then four collinear points, in front of ordinary draws
    w = Q.same_point_world(60, 7)
    d = Q.make_draws(35, 7)
    d[0] = draws_for([0, 1, 2, 3], w.n if w.match is None else len(w.edges()[0]))
    d[3] = draws_for([5, 2, 4, 0], len(w.edges()[0]))
    W["same_point"] = (w, d)
    w = Q.make_world(60, 8, noise=0.0, extra=0)
    jj, ii = w.edges()
    line = np.array([[0.5 * k, 0.25 * k, 6.0 + k] for k in range(4)], np.float32)  # exactly representable, exactly collinear
    w.points[ii[:4]] = line
    d = Q.make_draws(35, 8)
    d[1] = draws_for([0, 1, 2, 3], len(jj))
    W["collinear"] = (w, d)
    # the second setting (pose_ref_lib: K_ANISO, 5 levels of 1.37, a true pose rolled by 89 degrees), solved under SIGMA2_2
    two = dict(motion=Q.MOTION_2, **Q.SECOND)
    W["clean@2"] = (Q.make_world(90, 401, outliers=18, noise=0.0, **two), Q.make_draws(35, 1))
    W["clean_matched@2"] = (Q.make_world(70, 402, outliers=14, noise=0.0, matched=True, **two), Q.make_draws(35, 2))
    W["noisy@2"] = (Q.make_world(100, 403, outliers=20, noise=0.5, **two), Q.make_draws(35, 1))
    for seed in range(410, 413):
        W["mixed%d@2" % seed] = (Q.make_world(50, seed, outliers=10, noise=0.5, **two), Q.make_draws(35, seed - 410))
    return W


SIGMA2_2 = Q.sigma2_table(Q.NLEVELS_2, Q.SCALE_FACTOR_2)


def _sigma2(name):
    """The sigma2 table a world is solved under: the second setting's for the names that end in @2."""
    return SIGMA2_2 if name.endswith("@2") else None


def _of(setting, names):
    return names if setting == "first" else tuple(n + "@2" for n in names)


@pytest.fixture(scope="module")
def worlds():
    return _worlds()


@pytest.fixture(scope="module")
def results(worlds):
    """name -> (literal loop's outputs, prefix resolution's outputs)"""
    return {name: (Q.solve(w, d, 0, _sigma2(name)), Q.solve(w, d, 1, _sigma2(name))) for name, (w, d) in worlds.items()}


# ---- ABI ----

def test_python_mirror(orbx):
    assert ctypes.sizeof(orbx.PnpResult) == orbx.PNP_RESULT_DTYPE.itemsize == Q.PNP_RESULT_DTYPE.itemsize == 200
    assert Q.lib().pnr_result_size() == 200  # the header's struct
    assert orbx.PNP_RESULT_DTYPE == Q.PNP_RESULT_DTYPE
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for name, value in (("BAD_INPUT", 2), ("NONFINITE", 4), ("FEW_POINTS", 8), ("BAD_DRAWS", 16), ("NO_POSE", 32)):
        assert "#define ORBX_PNP_%s %d " % (name, value) in hdr
        assert getattr(orbx, "PNP_" + name) == getattr(Q, name) == value
    assert "#define ORBX_PNP_RAND_MAX %d\n" % Q.RAND_MAX in hdr and orbx.PNP_RAND_MAX == Q.RAND_MAX
    assert callable(orbx.ORBextractor.pnp_solve_batch_device) and callable(orbx.ORBextractor.pnp_solve)
    assert callable(orbx.PnPsolver.iterate) and callable(orbx.PnPsolver.find) and callable(orbx.PnPsolver.SetRansacParameters)
    vals = iter(range(100, 200))
    d = orbx.sample_pnp_draws(lambda: next(vals), 3)
    assert d.dtype == np.int32 and d.tolist() == [[100, 101, 102, 103], [104, 105, 106, 107], [108, 109, 110, 111]]


def test_refusals_without_a_context(orbx):
    """The pose call's list, then the parameters' ranges; ctx == NULL with well-formed arguments is ORBX_E_HIP: all decided
    before a device is touched (there is none here)."""
    L = orbx.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    frame, sets = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    neg, beyond = np.array([0, -1], np.int32), np.array([2, 0], np.int32)
    K = np.eye(3, dtype=np.float32)
    d = ctypes.c_void_p(4096)  # (a device pointer the call never follows)

    def batch(n_frames=2, n_problems=2, f=p(frame), s=p(sets), kps=d, n=d, cap=16, m=d, n_sets=2, pts=d, mask=d, K=p(K), sig=None,
              prob=0.99, mi=10, mx=300, eps=0.5, th2=5.991, it=35, draws=d, out=d, pose=d, row=d, flags=d):
        return L.orbx_pnp_solve_batch_device(None, n_frames, n_problems, f, s, kps, n, cap, m, n_sets, pts, mask, K, sig, prob, mi, mx,
                                             eps, th2, it, draws, out, pose, row, flags)
    assert batch() == orbx.E_HIP
    assert batch(m=None, mask=None, flags=None) == orbx.E_HIP  # (all optional)
    assert batch(n_problems=0, f=None, s=None) == orbx.E_HIP  # (ORBX_OK with a context)
    for bad in (dict(n_frames=-1), dict(n_problems=-1), dict(n_sets=-1), dict(cap=0), dict(cap=-2), dict(f=None), dict(s=None),
                dict(kps=None), dict(n=None), dict(pts=None), dict(K=None), dict(out=None), dict(pose=None), dict(row=None),
                dict(draws=None), dict(it=0), dict(it=-1), dict(n_frames=1), dict(n_sets=1), dict(f=p(neg)), dict(s=p(neg)),
                dict(f=p(beyond)), dict(s=p(beyond)), dict(prob=0.0), dict(prob=1.0), dict(prob=float("nan")), dict(eps=0.0),
                dict(eps=1.0), dict(mi=3), dict(mx=0), dict(th2=0.0), dict(th2=-1.0), dict(th2=float("nan")), dict(th2=float("inf"))):
        assert batch(**bad) == orbx.E_BADARG, bad
    assert batch(cap=16385) == orbx.E_CAPACITY
    assert batch(cap=16384) == orbx.E_HIP

    k, pts, flags = np.zeros(4, orbx.KEYPOINT_DTYPE), np.zeros((4, 3), np.float32), np.zeros(4, np.uint8)
    draws, res = np.zeros((35, 4), np.int32), orbx.PnpResult()

    def host(k=p(k), n=4, pts=p(pts), mask=None, K=p(K), prob=0.99, mi=10, mx=300, eps=0.5, th2=5.991, it=35, draws=p(draws),
             res=ctypes.byref(res), flags=p(flags)):
        return L.orbx_pnp_solve(None, k, n, pts, mask, K, None, prob, mi, mx, eps, th2, it, draws, res, flags)
    assert host() == orbx.E_HIP
    assert host(n=0, k=None, pts=None, flags=None) == orbx.E_HIP
    for bad in (dict(n=-1), dict(k=None), dict(pts=None), dict(K=None), dict(it=0), dict(draws=None), dict(res=None),
                dict(flags=None), dict(mi=3), dict(eps=1.5), dict(prob=-0.1), dict(mx=0), dict(th2=0.0)):
        assert host(**bad) == orbx.E_BADARG, bad
    assert host(n=16385) == orbx.E_CAPACITY
    t = np.zeros((4, 2), np.int32)
    assert L.orbx_pnp_ransac_table(0.99, 10, 300, 0.5, 3, None) == orbx.E_BADARG
    assert L.orbx_pnp_ransac_table(0.99, 10, 300, 0.5, -1, p(t)) == orbx.E_BADARG
    assert L.orbx_pnp_ransac_table(0.99, 3, 300, 0.5, 3, p(t)) == orbx.E_BADARG


# ---- SetRansacParameters ----

@pytest.mark.parametrize("prm", [dict(), dict(min_inliers=15, epsilon=0.4), dict(probability=0.999, max_iterations=20, epsilon=0.3),
                                 dict(min_inliers=4, epsilon=0.9)])
def test_ransac_table_against_a_direct_evaluation(orbx, prm):
    """N = 0 .. 45: N == minInliers gives one iteration, N in (minInliers, minInliers / epsilon) raises epsilon to minInliers / N,
    beyond that nMinInliers = (int)(N * epsilon) grows with N and the iteration count stays."""
    kw = dict(probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5)
    kw.update(prm)
    t = np.full((46, 2), -1, np.int32)
    assert orbx.lib().orbx_pnp_ransac_table(kw["probability"], kw["min_inliers"], kw["max_iterations"], kw["epsilon"], 45,
                                            ctypes.c_void_p(t.ctypes.data)) == 0
    ref = Q.ransac_table(45, **kw)
    assert t.tolist() == ref.tolist()
    mi = kw["min_inliers"]
    assert tuple(t[mi]) == (mi, 1)
    assert (t[:mi + 1, 0] == mi).all() and (t[:, 1] >= 1).all() and (t[:, 1] <= kw["max_iterations"]).all()
    if not prm:  # the reference's parameters
        assert t[11].tolist() == [10, 4] and t[15].tolist() == [10, 14] and t[20].tolist() == [10, 35]
        assert t[21].tolist() == [10, 35] and t[30].tolist() == [15, 35] and t[45].tolist() == [22, 35]
        assert (np.diff(t[10:21, 1]) >= 0).all()


# ---- the sampler ----

def test_sampler_against_a_literal_swap_and_pop():
    rng = np.random.default_rng(17)
    top = Q.RAND_MAX
    cases = [([0, 0, 0, 0], 50), ([top, top, top, top], 50), ([0, 0, 0, 0], 4), ([top, top, top, top], 4), ([0, top, 0, top], 5),
             ([top, 0, top, 0], 5), ([top // 2] * 4, 7)]
    cases += [(list(rng.integers(0, top + 1, 4)), int(n)) for n in (4, 4, 4, 5, 5, 6, 7, 10, 64, 65, 200, 1000, 16384) for _ in range(8)]
    for draws, N in cases:
        got = Q.sample(draws, N)
        assert got == Q.list_sampler(draws, N), (draws, N)
        assert len(set(got)) == 4 and all(0 <= g < N for g in got)
    assert Q.sample([0, 0, 0, 0], 50) == [0, 49, 48, 47]  # 0, then the last three entries
    assert Q.sample([top] * 4, 50) == [49, 48, 47, 46]
    assert sorted(Q.sample([0, 0, 0, 0], 4)) == [0, 1, 2, 3]
    for k in range(4):
        d = [5, 6, 7, 8]
        d[k] = -1
        assert Q.sample(d, 50) is None


# ---- against truth ----

def test_noise_free_worlds_return_exactly_the_clean_set(worlds, results, setting="first"):
    for name in _of(setting, ("clean", "clean_matched")):
        w, _ = worlds[name]
        r, pose, row, inl = results[name][0]
        assert r["status"] == 0 and r["refined"] == 1 and r["found_it"] >= 0
        assert np.array_equal(np.flatnonzero(inl), w.truth["clean"]), name
        assert r["n_inliers"] == len(w.truth["clean"])
        j, e2 = Q.error2(w, r["R"], r["t"], w.truth["clean"])
        assert (e2 < Q.max_error(w, j, sigma2=_sigma2(name))).all()
        jb, eb = Q.error2(w, r["R"], r["t"], w.truth["bad"])
        assert (eb > Q.max_error(w, jb, sigma2=_sigma2(name))).all()
        # the row is the pose call's d_match for the inliers
        jj, ii = w.edges()
        want = np.full(w.cap, -1, np.int32)
        keep = np.isin(jj, w.truth["clean"])
        want[jj[keep]] = ii[keep]
        assert np.array_equal(row, want)
        assert pose.tobytes() == r["Tcw"].tobytes() == np.r_[r["R"].reshape(9), r["t"]].astype(np.float32).tobytes()


def test_every_returned_inlier_passes_when_recomputed(worlds, results, setting="first"):
    """On worlds with 0.5 sigma of noise: error2 < maxError in numpy at the returned pose, but for points within 1e-4 relative of
    the threshold (at most 2 %)."""
    first = ("noisy", "noisy_b", "second_try", "mixed300", "mixed303")
    for name in (first if setting == "first" else ("noisy@2", "mixed410@2", "mixed411@2", "mixed412@2")):
        w, _ = worlds[name]
        r, _, _, inl = results[name][0]
        assert r["status"] == 0 and r["n_inliers"] == inl.sum() > 0
        j, e2 = Q.error2(w, r["R"], r["t"], np.flatnonzero(inl))
        th = Q.max_error(w, j, sigma2=_sigma2(name)).astype(np.float64)
        near = np.abs(e2 - th) <= 1e-4 * th
        print(name, "inliers", len(j), "within 1e-4 of the threshold", int(near.sum()))
        assert near.mean() <= 0.02, name
        assert (e2[~near] < th[~near]).all(), name
        jo, eo = Q.error2(w, r["R"], r["t"], np.setdiff1d(w.edges()[0], np.flatnonzero(inl)))
        tho = Q.max_error(w, jo, sigma2=_sigma2(name)).astype(np.float64)
        far = np.abs(eo - tho) > 1e-4 * tho
        assert (eo[far] >= tho[far]).all(), name


# ---- against the numpy statement ----

NUMPY_WORLDS = ("clean", "clean_matched", "noisy", "noisy_b", "mixed300", "mixed301", "mixed302", "mixed303", "mixed304", "mixed305")
NUMPY_WORLDS_2 = ("clean@2", "clean_matched@2", "noisy@2", "mixed410@2", "mixed411@2", "mixed412@2")


def test_refine_agrees_with_the_numpy_statement(worlds, results, setting="first"):
    """compute_pose over the returned inlier set against epnp_numpy over the same set, under the control points' signs that
    come closest (with noise EPnP depends on them beyond rounding, and they are the eigen-solver's to choose)."""
    worst = [0.0, 0.0]
    for name in (NUMPY_WORLDS if setting == "first" else NUMPY_WORLDS_2):
        w, _ = worlds[name]
        inl = results[name][0][3]
        assert inl.sum() >= 20
        c, R, t = Q.epnp(w, inl, _sigma2(name))
        assert c in (1, 2, 3)
        da, dt = Q.closest_numpy(w, inl, R, t)
        print(name, "angle", da, "translation", dt)
        worst = [max(worst[0], da), max(worst[1], dt)]
    print("largest: angle %.3g rad, relative translation %.3g" % tuple(worst))
    limit = (Q.NUMPY_ANGLE_LIMIT, Q.NUMPY_TRANS_LIMIT) if setting == "first" else (Q.NUMPY_ANGLE_LIMIT_2, Q.NUMPY_TRANS_LIMIT_2)
    assert worst[0] <= limit[0] and worst[1] <= limit[1]


def test_the_second_setting_against_the_truth_and_numpy(worlds, results):
    """The clean set, the recomputed inliers and Refine against epnp_numpy under the second setting (the worlds named @2: K_ANISO,
    5 levels of 1.37, a true pose rolled by 89 degrees)."""
    test_noise_free_worlds_return_exactly_the_clean_set(worlds, results, "second")
    test_every_returned_inlier_passes_when_recomputed(worlds, results, "second")
    test_refine_agrees_with_the_numpy_statement(worlds, results, "second")


# ---- the prefix resolution ----

def test_prefix_resolution_equals_the_literal_loop(results):
    for name, (a, b) in results.items():
        assert a[0].tobytes() == b[0].tobytes(), (name, a[0], b[0])
        for x, y in zip(a[1:], b[1:]):
            assert x.tobytes() == y.tobytes(), name


def test_found_it_is_the_best_it(results):
    n = 0
    for name, (a, _) in results.items():
        r = a[0]
        if r["refined"]:
            assert r["found_it"] == r["best_it"] == r["its_run"] - 1, name
            n += 1
        else:
            assert r["found_it"] == -1
    assert n >= 10


# ---- branch worlds ----

def test_unrefined(worlds, results):
    w, d = worlds["unrefined"]
    r, pose, row, inl = results["unrefined"][0]
    assert (r["n_correspondences"], r["min_inliers"], r["max_its"]) == (20, 10, 35)
    assert r["status"] == 0 and r["refined"] == 0 and r["found_it"] == -1 and r["its_run"] == 35 and r["best_it"] >= 0
    assert r["n_refines"] == 1 and r["n_best_inliers"] == r["n_inliers"] == 10  # Refine yields 10, which is not > 10
    assert np.array_equal(np.flatnonzero(inl), w.truth["clean"])
    assert np.isfinite(pose).all() and pose.any()


def test_second_try(results):
    for name in ("second_try", "second_try_b"):
        r = results[name][0][0]
        assert r["refined"] == 1 and r["n_refines"] >= 2 and r["n_inliers"] > r["min_inliers"], name


def test_degenerate_draws_are_counted_and_not_followed(worlds, results):
    for name in ("same_point", "collinear"):
        r, pose, row, inl = results[name][0]
        assert r["n_degenerate"] > 0, name
        assert r["status"] == 0 and r["refined"] == 1 and r["found_it"] > 0, name
        assert np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all() and np.isfinite(pose).all()
    # the solver with only the degenerate draw: no pose, zeros, an all -1 row
    w, d = worlds["same_point"]
    r, pose, row, inl = Q.solve(w, d[:1], 0)
    assert r["n_degenerate"] == 1 and r["status"] == Q.NO_POSE and r["its_run"] == 1 and r["best_it"] == -1
    assert not pose.any() and (row == -1).all() and not inl.any() and not r["R"].any() and r["beta_choice"] == 0


def test_planar_points_give_a_finite_pose_or_none(worlds, results):
    w, _ = worlds["planar"]
    r, pose, row, inl = results["planar"][0]
    assert np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all()
    if r["status"] & Q.NO_POSE:
        assert not pose.any() and (row == -1).all()
    else:
        j, e2 = Q.error2(w, r["R"], r["t"], np.flatnonzero(inl))
        th = Q.max_error(w, j).astype(np.float64)
        assert (e2 < th * (1 + 1e-4)).all() and r["n_inliers"] >= r["min_inliers"]


def test_small_counts(worlds, results):
    for n in (3, 4, 9):
        r, pose, row, inl = results["n%d" % n][0]
        assert r["status"] == Q.FEW_POINTS | Q.NO_POSE and r["n_correspondences"] == n and r["its_run"] == 0, n
        assert not pose.any() and (row == -1).all() and not inl.any()
    r = results["n10"][0][0]
    assert (r["min_inliers"], r["max_its"], r["its_run"]) == (10, 1, 1)  # one iteration; Refine's 10 is not > 10
    assert r["status"] == 0 and r["refined"] == 0 and r["n_inliers"] == 10 and r["n_refines"] == 1
    r = results["n11"][0][0]
    assert (r["min_inliers"], r["max_its"]) == (10, 4) and r["refined"] == 1 and r["n_inliers"] == 11 and r["found_it"] == 0
    r = results["n20"][0][0]
    assert (r["min_inliers"], r["max_its"]) == (10, 35) and r["refined"] == 1 and r["n_inliers"] == 20


def test_every_beta_choice_is_taken(results):
    seen = {int(a[0]["beta_choice"]) for a, _ in results.values()}
    assert {1, 2, 3} <= seen, seen


def bad(w, what):
    q = w.copy()
    jj, ii = w.edges()
    j, i = int(jj[0]), int(ii[0])
    if what == "count":
        q.n = q.cap + 1
    elif what == "negative_count":
        q.n = -1
    elif what == "match":
        if q.match is None:
            q.match = np.full(q.cap, -1, np.int32)
            q.match[:q.n] = np.arange(q.n)
        q.match[j] = q.cap
    elif what == "octave":
        q.kps["octave"][j] = Q.NLEVELS
    elif what == "negative_octave":
        q.kps["octave"][j] = -1
    elif what == "nan":
        q.points[i, 0] = np.nan
    elif what == "inf_keypoint":
        q.kps["x"][j] = np.inf
    return q


GARBAGE = (("count", Q.BAD_INPUT), ("negative_count", Q.BAD_INPUT), ("match", Q.BAD_INPUT), ("octave", Q.BAD_INPUT),
           ("negative_octave", Q.BAD_INPUT), ("nan", Q.NONFINITE), ("inf_keypoint", Q.NONFINITE))


def test_every_garbage_kind(worlds):
    w, d = worlds["clean"]
    for what, bit in GARBAGE:
        for mode in (0, 1):
            r, pose, row, inl = Q.solve(bad(w, what), d, mode)
            assert r["status"] == bit | Q.NO_POSE, what
            assert not pose.any() and (row == -1).all() and not inl.any() and not r["R"].any() and not r["t"].any()
            assert r["n_correspondences"] == 0 and r["its_run"] == 0 and r["found_it"] == -1 and r["best_it"] == -1
    # a draw out of range skips its hypothesis and sets its bit; the others go on
    d2 = d.copy()
    d2[0, 2] = -5
    r, pose, row, inl = Q.solve(w, d2, 0)
    assert r["status"] == Q.BAD_DRAWS and r["refined"] == 1 and r["found_it"] >= 1
    d3 = d.copy()
    d3[34, 0] = -1  # (behind found_it: never drawn)
    assert Q.solve(w, d3, 0)[0]["status"] == 0


def build_shim_pnp(orbx, out_dir):
    """Compiles tests/cpp/shim_pnp.cpp: PnPsolver of the C++ shim next to the C ABI."""
    exe = os.path.join(str(out_dir), "shim_pnp")
    libdir = os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "shim_pnp.cpp"), "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return exe


def test_shim_pnp_compiles(orbx, tmp_path):
    build_shim_pnp(orbx, tmp_path)
