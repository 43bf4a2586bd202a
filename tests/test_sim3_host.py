"""CPU-only checks of Sim3Solver (include/orbx.h, "loop closing: Sim3 RANSAC"): what the CPU restatement tests/cpp/sim3_ref.cpp
-- which the device must equal bit for bit (tests/test_gpu_sim3.py) -- is worth.  Ground-truth worlds with a known similarity
between the two camera frames; an independent numpy f64 statement (Horn through numpy.linalg.eigh, the inlier test spelled out
again); rule 6 (the literal loop against the after-the-fact resolution, the last of equals, the strict > minInliers); degenerate
triples; the RANSAC table, the sampler, every garbage kind, the refusals and the Python mirror."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pose_ref_lib as P
import sim3_ref_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24  # the unit roundoff of f32


# ---- the worlds the host and the GPU test share: name -> (world, draws, parameters) ----

def _spread_triple(w, tries=400, seed=0):
    """Among `tries` random triples of clean correspondences, the one whose triangles (in both cameras) have the largest
    smallest altitude -> (triple of correspondence indices, that altitude in camera 1, in camera 2)."""
    rng = np.random.default_rng(seed)
    _, _, Y1, Y2 = S.camera_points_numpy(w)
    clean = np.setdiff1d(np.arange(len(Y1)), w.truth["bad"])

    def altitude(T):
        a, b, c = T
        area2 = np.linalg.norm(np.cross(b - a, c - a))
        return area2 / max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b))
    best = None
    for _ in range(tries):
        tr = rng.choice(clean, 3, replace=False)
        h1, h2 = altitude(Y1[tr]), altitude(Y2[tr])
        if best is None or min(h1, h2) > min(best[1], best[2]):
            best = (tr, h1, h2)
    return best


def _coincident_world():
    """Three correspondences of KF2 name one position: Pr2 = 0, den = 0, s12 = 0 / 0."""
    w = S.make_world(80, 31, outliers=10, noise=0.3)
    i1, i2 = w.edges()
    w.points2[i2[1]] = w.points2[i2[0]]
    w.points2[i2[2]] = w.points2[i2[0]]
    d = S.make_draws(60, 31)
    d[0] = S.draws_for((0, 1, 2), len(i1))
    return w, d


def _collinear_world():
    """Three correspondences on one line in both cameras: the rotation about the line is free, the hypothesis finite and useless."""
    w = S.make_world(80, 32, outliers=10, noise=0.3)
    i1, i2 = w.edges()
    T1, T2 = w.pose1.astype(np.float64), w.pose2.astype(np.float64)
    R1, t1, R2, t2 = T1[:9].reshape(3, 3), T1[9:], T2[:9].reshape(3, 3), T2[9:]
    tr = w.truth
    for k, lam in enumerate((0.0, 0.25, 1.0)):
        Y2 = np.array([-1.0, 0.5, 8.0]) + lam * np.array([2.0, -1.0, 3.0])
        Y1 = tr["s"] * tr["R"] @ Y2 + tr["t"]
        w.points2[i2[k]] = ((Y2 - t2) @ R2).astype(np.float32)
        w.points1[i1[k]] = ((Y1 - t1) @ R1).astype(np.float32)
    d = S.make_draws(60, 32)
    d[0] = S.draws_for((0, 1, 2), len(i1))
    return w, d


def _equals_world():
    """25 correspondences, exactly 20 of them clean and exact, for minInliers = 20: every clean triple counts 20 inliers, which
    is not > 20, so nothing ends the solver and the best is the LAST of the equals.  (mRansacMaxIts of N = 25 is 7.)"""
    return S.make_world(25, 33, outliers=5, noise=0.0), S.make_draws(30, 33)


_cache = {}


def _worlds():
    if _cache:
        return _cache
    W = _cache
    W["clean"] = (S.make_world(200, 1, outliers=40, noise=0.5), S.make_draws(300, 1), {})
    W["truth"] = (S.make_world(120, 2), S.make_draws(40, 2), {})
    W["truth_far"] = (S.make_world(150, 3, s=0.6, rot=(-0.2, 0.15, 0.3), t=(-0.5, 0.3, 1.0)), S.make_draws(40, 3), {})
    W["fix_scale"] = (S.make_world(120, 4, s=1.0), S.make_draws(40, 4), dict(fix_scale=1))
    W["fix_scale_noisy"] = (S.make_world(150, 5, s=1.0, outliers=30, noise=0.5), S.make_draws(300, 5), dict(fix_scale=1))
    W["hard"] = (S.make_world(90, 6, outliers=60, noise=0.3), S.make_draws(300, 6), {})
    W["hopeless"] = (S.make_world(60, 7, outliers=60), S.make_draws(300, 7), {})
    W["identity"] = (S.make_world(100, 8, s=1.0, rot=(0, 0, 0), t=(0, 0, 0)), S.make_draws(40, 8), {})
    W["no_mask"] = (S.make_world(100, 9, outliers=20, noise=0.5, extra=0, use_mask=False), S.make_draws(300, 9), {})
    W["coincident"] = _coincident_world() + ({},)
    W["collinear"] = _collinear_world() + ({},)
    W["equals"] = _equals_world() + ({},)
    W["equals_19"] = _equals_world() + (dict(min_inliers=19),)
    W["exactly_min"] = (S.make_world(20, 10), S.make_draws(30, 10), {})
    W["below_min"] = (S.make_world(19, 11), S.make_draws(30, 11), {})
    W["three"] = (S.make_world(3, 12), S.make_draws(30, 12), dict(min_inliers=3))
    W["empty"] = (S.make_world(0, 13, cap=8), S.make_draws(30, 13), {})
    # the second setting (pose_ref_lib: K_ANISO, 5 levels of 1.37), camera 1 rolled by 89 degrees against camera 2
    two = dict(rot=S.ROLL, **S.SECOND)
    W["truth@2"] = (S.make_world(80, 102, **two), S.make_draws(40, 2), dict(sigma2=SIGMA2_2))
    W["clean@2"] = (S.make_world(120, 101, outliers=24, noise=0.5, **two), S.make_draws(300, 1), dict(sigma2=SIGMA2_2))
    W["fix_scale_noisy@2"] = (S.make_world(100, 105, s=1.0, outliers=20, noise=0.5, **two), S.make_draws(300, 5),
                              dict(fix_scale=1, sigma2=SIGMA2_2))
    return W


SIGMA2_2 = S.sigma2_table(S.NLEVELS_2, S.SCALE_FACTOR_2)


@pytest.fixture(scope="module")
def worlds():
    return _worlds()


@pytest.fixture(scope="module")
def results(worlds):
    """name -> (the literal loop's answer, the after-the-fact resolution's answer)."""
    return {name: (S.solve(w, d, 0, **prm), S.solve(w, d, 1, **prm)) for name, (w, d, prm) in worlds.items()}


# ---- ABI ----

def test_python_mirror(orbx):
    assert ctypes.sizeof(orbx.Sim3Result) == orbx.SIM3_RESULT_DTYPE.itemsize == S.SIM3_RESULT_DTYPE.itemsize == 96
    assert S.lib().s3r_result_size() == 96  # the header's struct
    assert orbx.SIM3_RESULT_DTYPE == S.SIM3_RESULT_DTYPE
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for name, value in (("BAD_INPUT", 2), ("NONFINITE", 4), ("FEW_POINTS", 8), ("BAD_DRAWS", 16), ("NO_RESULT", 32)):
        assert "#define ORBX_SIM3_%s %d " % (name, value) in hdr
        assert getattr(orbx, "SIM3_" + name) == getattr(S, name) == value
    assert "[from-knowledge], PARITY UNPINNED" in hdr[hdr.index("loop closing: Sim3 RANSAC"):hdr.index("#define ORBX_SIM3_BAD_INPUT")]
    assert callable(orbx.ORBextractor.sim3_solve_batch_device) and callable(orbx.ORBextractor.sim3_solve)
    assert callable(orbx.Sim3Solver.iterate) and callable(orbx.Sim3Solver.find) and callable(orbx.Sim3Solver.SetRansacParameters)
    L = ctypes.CDLL(orbx.lib_path())
    for sym in ("orbx_sim3_ransac_table", "orbx_sim3_solve_batch_device", "orbx_sim3_solve"):
        assert hasattr(L, sym), sym
    vals = iter(range(100, 200))
    d = orbx.sample_sim3_draws(lambda: next(vals), 3)
    assert d.dtype == np.int32 and d.tolist() == [[100, 101, 102], [103, 104, 105], [106, 107, 108]]


def test_refusals_without_a_context(orbx):
    """The lists, then the parameters' ranges; ctx == NULL with well-formed arguments is ORBX_E_HIP: all decided before a device
    is touched (there is none here)."""
    L = orbx.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    a, b = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    neg, beyond = np.array([0, -1], np.int32), np.array([2, 0], np.int32)
    K = np.eye(3, dtype=np.float32)
    d = ctypes.c_void_p(4096)  # (a device pointer the call never follows)

    def batch(n_frames=2, n_problems=2, k1=p(a), k2=p(b), s1=p(a), s2=p(b), kps=d, n=d, cap=16, m=d, n_sets=2, pts=d, mask=d, pose=d,
              K=p(K), sig=None, fix=0, prob=0.99, mi=20, mx=300, th2=9.21, it=35, draws=d, out=d, sim=d, row=d, flags=d):
        return L.orbx_sim3_solve_batch_device(None, n_frames, n_problems, k1, k2, s1, s2, kps, n, cap, m, n_sets, pts, mask, pose, K,
                                              sig, fix, prob, mi, mx, th2, it, draws, out, sim, row, flags)
    assert batch() == orbx.E_HIP
    assert batch(mask=None, flags=None, fix=1, mi=3) == orbx.E_HIP  # (all optional; the smallest minInliers)
    assert batch(n_problems=0, k1=None, k2=None, s1=None, s2=None) == orbx.E_HIP  # (ORBX_OK with a context)
    for bad in (dict(n_frames=-1), dict(n_problems=-1), dict(n_sets=-1), dict(cap=0), dict(cap=-2), dict(k1=None), dict(k2=None),
                dict(s1=None), dict(s2=None), dict(kps=None), dict(n=None), dict(m=None), dict(pts=None), dict(pose=None),
                dict(K=None), dict(out=None), dict(sim=None), dict(row=None), dict(draws=None), dict(it=0), dict(it=-1),
                dict(n_frames=1), dict(n_sets=1), dict(k1=p(neg)), dict(k2=p(neg)), dict(s1=p(neg)), dict(s2=p(neg)),
                dict(k1=p(beyond)), dict(k2=p(beyond)), dict(s1=p(beyond)), dict(s2=p(beyond)), dict(prob=0.0), dict(prob=1.0),
                dict(prob=float("nan")), dict(mi=2), dict(mx=0), dict(th2=0.0), dict(th2=-1.0), dict(th2=float("nan")),
                dict(th2=float("inf")), dict(fix=2), dict(fix=-1)):
        assert batch(**bad) == orbx.E_BADARG, bad
    assert batch(cap=16385) == orbx.E_CAPACITY
    assert batch(cap=16384) == orbx.E_HIP
    assert batch(it=2 ** 30) == orbx.E_CAPACITY and batch(it=2 ** 30 - 32) == orbx.E_HIP  # 2 problems: a lane per hypothesis, below 2^31 - 63

    k, pts, pose = np.zeros(4, orbx.KEYPOINT_DTYPE), np.zeros((4, 3), np.float32), np.zeros(12, np.float32)
    m, flags, row, sim = np.zeros(4, np.uint8), np.zeros(4, np.uint8), np.zeros(4, np.int32), np.zeros(13, np.float32)
    draws, res = np.zeros((35, 3), np.int32), orbx.Sim3Result()

    def host(k1=p(k), n1=4, p1=p(pts), m1=None, T1=p(pose), k2=p(k), n2=4, p2=p(pts), m2=None, T2=p(pose), match=p(row), K=p(K), fix=0,
             prob=0.99, mi=20, mx=300, th2=9.21, it=35, draws=p(draws), res=ctypes.byref(res), sim=p(sim), out=p(row), flags=p(flags)):
        return L.orbx_sim3_solve(None, k1, n1, p1, m1, T1, k2, n2, p2, m2, T2, match, K, None, fix, prob, mi, mx, th2, it, draws, res,
                                 sim, out, flags)
    assert host() == orbx.E_HIP
    assert host(m1=p(m), m2=p(m), flags=None) == orbx.E_HIP
    assert host(n1=0, k1=None, p1=None, match=None, out=None) == orbx.E_HIP and host(n2=0, k2=None, p2=None) == orbx.E_HIP
    for bad in (dict(n1=-1), dict(n2=-1), dict(k1=None), dict(k2=None), dict(p1=None), dict(p2=None), dict(T1=None), dict(T2=None),
                dict(match=None), dict(K=None), dict(it=0), dict(draws=None), dict(res=None), dict(sim=None), dict(out=None),
                dict(m1=p(m)), dict(m2=p(m)), dict(mi=2), dict(prob=-0.1), dict(mx=0), dict(th2=0.0), dict(fix=3)):
        assert host(**bad) == orbx.E_BADARG, bad
    assert host(n1=16385) == orbx.E_CAPACITY and host(n2=16385) == orbx.E_CAPACITY
    t = np.zeros(4, np.int32)
    assert L.orbx_sim3_ransac_table(0.99, 20, 300, 3, None) == orbx.E_BADARG
    assert L.orbx_sim3_ransac_table(0.99, 20, 300, -1, p(t)) == orbx.E_BADARG
    assert L.orbx_sim3_ransac_table(0.99, 2, 300, 3, p(t)) == orbx.E_BADARG


# ---- SetRansacParameters, the sampler ----

@pytest.mark.parametrize("prm", [dict(), dict(min_inliers=6), dict(probability=0.999, max_iterations=20), dict(min_inliers=3)])
def test_ransac_table_against_a_direct_evaluation(orbx, prm):
    """N = 0 .. 120: below minInliers the solver never iterates (max_iterations), N == minInliers gives one iteration, beyond it
    epsilon = minInliers / N falls and the count grows to max_iterations; minInliers itself never moves."""
    kw = dict(probability=0.99, min_inliers=20, max_iterations=300)
    kw.update(prm)
    t = np.full(121, -1, np.int32)
    assert orbx.lib().orbx_sim3_ransac_table(kw["probability"], kw["min_inliers"], kw["max_iterations"], 120,
                                             ctypes.c_void_p(t.ctypes.data)) == 0
    assert t.tolist() == S.ransac_table(120, **kw).tolist()
    mi = kw["min_inliers"]
    assert t[mi] == 1 and (t[:mi] == kw["max_iterations"]).all() and (np.diff(t[mi:]) >= 0).all()
    assert (t >= 1).all() and (t <= kw["max_iterations"]).all()
    if not prm:  # LoopClosing's parameters, by hand: N = 25: epsilon = 0.8, log(0.01) / log(1 - 0.512) = 6.42 -> 7
        assert t[25] == 7 and t[40] == 35 and t[120] == 300


def test_sampler_against_a_literal_swap_and_pop():
    rng = np.random.default_rng(17)
    for N in (3, 4, 5, 7, 64, 200, 16384):
        for _ in range(200):
            d = rng.integers(0, S.RAND_MAX + 1, 3).astype(np.int32)
            assert S.sample(d, N) == S.list_sampler(d, N), (N, d)
        edge = np.array([S.RAND_MAX, S.RAND_MAX, S.RAND_MAX], np.int32)  # the last entry three times over
        assert S.sample(edge, N) == S.list_sampler(edge, N) == [N - 1, N - 2, N - 3]
        assert S.sample(np.zeros(3, np.int32), N) == S.list_sampler([0, 0, 0], N)
        tr = [int(v) for v in rng.choice(N, 3, replace=False)]
        assert S.sample(S.draws_for(tr, N), N) == tr
    assert S.sample(np.array([5, -1, 7], np.int32), 10) is None


# ---- ground truth ----

@pytest.mark.parametrize("name", ["truth", "truth_far", "fix_scale", "identity", "truth@2"])
def test_noise_free_worlds_return_the_clean_set_and_the_true_similarity(worlds, name):
    """A noise-free world solved from a well-spread triple: every correspondence is an inlier, and s12, R12, t12 equal the truth
    to a tolerance DERIVED from the f32 inputs (not tuned against the code):

    delta, the error of a camera-frame coordinate: the stored points and poses are f32 (relative error U = 2^-24 each) and
    Rcw * X + tcw is evaluated in f32 (three products, three sums, each of magnitude <= 3 B where B bounds every coordinate and
    translation): <= 3 * 2 * U * B of input rounding + 6 * U * 3 B of operation rounding = 24 U B.
    To first order a displacement delta of a triangle's vertices turns its fitted frame by <= 2 delta / h (h the smallest
    altitude), changes its size by <= 2 delta / r relative (r the root of the summed squared distances from the centroid), and
    moves the centroid by <= delta; both triangles contribute (camera 1's over its own h and r).  The translation inherits
    |s O2| times the rotation and scale errors.  A factor 4 covers the constants of the first-order bounds, and one U of the
    value is added for the final rounding to f32."""
    w, _, prm = worlds[name]
    tr, h1, h2 = _spread_triple(w)
    i1, i2, Y1, Y2 = S.camera_points_numpy(w)
    d = S.draws_for(tr, len(i1)).reshape(1, 3)
    res, sim, row, inl = S.solve(w, d, 0, **prm)
    assert res["status"] == 0 and res["found_it"] == 0 and res["n_inliers"] == len(i1) == w.truth["slots1"].size
    assert np.array_equal(np.flatnonzero(inl), w.truth["slots1"]) and np.array_equal(row[w.truth["slots1"]], w.truth["slots2"])
    assert (row[np.setdiff1d(np.arange(w.cap), w.truth["slots1"])] == -1).all()
    B = max(np.abs(w.points1[i1]).max(), np.abs(w.points2[i2]).max(), np.abs(Y1).max(), np.abs(Y2).max(),
            np.abs(w.pose1[9:]).max(), np.abs(w.pose2[9:]).max())
    delta = 24 * U * B
    r1 = np.sqrt(((Y1[tr] - Y1[tr].mean(0)) ** 2).sum())
    r2 = np.sqrt(((Y2[tr] - Y2[tr].mean(0)) ** 2).sum())
    t = w.truth
    rot_tol = 4 * (2 * delta / h1 + 2 * delta / h2) + U
    scale_tol = (4 * (2 * delta / r1 + 2 * delta / r2) if not prm.get("fix_scale") else 0.0) + U
    t_tol = 4 * (2 * delta + t["s"] * np.linalg.norm(Y2[tr].mean(0)) * (rot_tol + scale_tol)) + U * np.abs(t["t"]).max()
    rot, scale, trans = S.sim_difference(sim[12], sim[:9].reshape(3, 3), sim[9:12], t["s"], t["R"], t["t"])
    print("%s: rotation %.3g (tol %.3g), scale %.3g (tol %.3g), translation %.3g (tol %.3g)" %
          (name, rot, rot_tol, scale, scale_tol, trans, t_tol))
    assert rot <= rot_tol and scale <= scale_tol and trans <= t_tol
    assert rot_tol < 1e-4 and scale_tol < 1e-4 and t_tol < 2e-2  # (the bound itself says something; |O2| is about 12 units)
    if prm.get("fix_scale"):
        assert sim[12] == 1.0
    assert np.allclose(res["R12"].reshape(9), sim[:9], rtol=0, atol=0) and res["s12"] == sim[12] and (res["t12"] == sim[9:12]).all()


def test_noisy_worlds_keep_the_clean_and_drop_the_gross(worlds, results):
    for name in ("clean", "fix_scale_noisy", "hard", "no_mask", "clean@2", "fix_scale_noisy@2"):
        w = worlds[name][0]
        res, sim, row, inl = results[name][0]
        assert res["status"] == 0 and res["found_it"] >= 0 and res["n_inliers"] > 20, name
        i1, _ = w.edges()
        gross = i1[w.truth["bad"]]
        assert not inl[gross].any(), name  # more than a unit off in 3D: hundreds of pixels
        assert inl.sum() == res["n_inliers"] and set(np.flatnonzero(inl)) <= set(i1)
        assert np.array_equal(row[inl != 0], w.match[inl != 0]) and (row[inl == 0] == -1).all()
        rot, scale, _ = S.sim_difference(sim[12], sim[:9].reshape(3, 3), sim[9:12], w.truth["s"], w.truth["R"], w.truth["t"])
        assert rot < 0.05 and scale < 0.05, (name, rot, scale)  # (a RANSAC hypothesis from three noisy points: coarse)
    res = results["hopeless"][0][0]
    assert res["status"] == S.NO_RESULT and res["found_it"] == -1 and res["its_run"] == res["max_its"] == S.ransac_entry(60) == 123


# ---- the independent numpy statement ----

BAND = 1e-3  # relative half-width of the excluded band around a bound.  The f32 evaluation of rule 5 carries pixel coordinates of
# up to 640 with a few U each (about 2e-4 px) and the similarity rounded to f32 (U * 20 units * 520 / 4 px per unit: another 2e-4
# px); the bounds are at d = 3 px and more, so err = d^2 is off by at most 2 * 4e-4 / 3 = 3e-4 relative.


@pytest.mark.parametrize("name", ["clean", "truth", "fix_scale_noisy", "hard", "no_mask", "identity", "collinear", "truth@2", "clean@2",
                                  "fix_scale_noisy@2"])
def test_inlier_decisions_agree_with_the_numpy_statement(worlds, results, name):
    """The winning hypothesis again in numpy f64 from the raw inputs: the sampler as a list, Horn through eigh, the two
    reprojections.  Every inlier decision agrees away from the thresholds; the band excludes at most 1 % of the world's
    correspondences (checked: the worlds are seeded so)."""
    w, d, prm = worlds[name]
    res, sim, row, inl = results[name][0]
    assert res["found_it"] >= 0
    i1, i2, Y1, Y2 = S.camera_points_numpy(w)
    tr = S.list_sampler(d[res["found_it"]], len(i1))
    s, R, t = S.horn_numpy(Y1[tr], Y2[tr], bool(prm.get("fix_scale")))
    rot, scale, trans = S.sim_difference(sim[12], sim[:9].reshape(3, 3), sim[9:12], s, R, t)
    e1, e2 = S.errors_numpy(Y1, Y2, s, R, t, w.K)
    sig = (S.sigma2_table() if prm.get("sigma2") is None else prm["sigma2"]).astype(np.float64)
    b1, b2 = 9.210 * sig[w.kps1["octave"][i1]], 9.210 * sig[w.kps2["octave"][i2]]
    near = (np.abs(e1 / b1 - 1) < BAND) | (np.abs(e2 / b2 - 1) < BAND)
    assert near.sum() <= 0.01 * len(i1), (name, int(near.sum()))
    mine = (e1 < b1) & (e2 < b2)
    assert np.array_equal(mine[~near], inl[i1][~near] != 0), name
    print("%s: numpy against the restatement: rotation %.3g, scale %.3g, translation %.3g; %d of %d in the band" %
          (name, rot, scale, trans, int(near.sum()), len(i1)))


def test_horn_agrees_with_numpy_on_random_triples():
    """The shared arithmetic's Horn on f64 triples against numpy.linalg.eigh's: well-spread triangles, so both are conditioned
    and differ by rounding alone (1e-10 is 1e5 roundoffs: the altitude of these triangles is above 0.1 against coordinates of 10)."""
    rng = np.random.default_rng(5)
    done = 0
    while done < 200:
        P2 = rng.uniform(-10, 10, (3, 3))
        a, b, c = P2
        if np.linalg.norm(np.cross(b - a, c - a)) / max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b)) < 0.1:
            continue
        done += 1
        R, t, s = P.rotvec(rng.uniform(-2, 2, 3)), rng.uniform(-5, 5, 3), rng.uniform(0.2, 5)
        P1 = s * P2 @ R.T + t + rng.normal(0, 0.05, (3, 3))
        for fix in (False, True):
            got, ref = S.horn(P1, P2, fix), S.horn_numpy(P1, P2, fix)
            rot, scale, trans = S.sim_difference(got[0], got[1], got[2], *ref)
            assert rot < 1e-10 and scale < 1e-10 and trans < 1e-9, (done, fix, rot, scale, trans)
            assert abs(np.linalg.det(got[1]) - 1) < 1e-12


# ---- rule 6 ----

def test_prefix_resolution_equals_the_literal_loop(results):
    for name, (loop, after) in results.items():
        for a, b in zip(loop, after):
            assert a.tobytes() == b.tobytes(), name


def test_every_result_is_consistent_with_its_hypotheses(worlds, results):
    """Rule 6 once more, in Python, over the counts of every hypothesis taken on its own."""
    for name, (w, d, prm) in worlds.items():
        res = results[name][0][0]
        mi = prm.get("min_inliers", 20)
        if res["status"] & (S.FEW_POINTS | S.BAD_INPUT | S.NONFINITE):
            assert res["its_run"] == 0 and res["found_it"] == -1 and res["best_it"] == -1
            continue
        N, counts, flags, sims = S.hypotheses(w, d, sigma2=prm.get("sigma2"), fix_scale=prm.get("fix_scale", 0))
        assert N == res["n_correspondences"]
        best, best_count, found = -1, 0, -1
        n_its = min(len(d), res["max_its"])
        for it in range(n_its):
            if flags[it] == 0 and counts[it] >= best_count:
                best, best_count = it, int(counts[it])
                if counts[it] > mi:
                    found = it
                    break
        assert (res["found_it"], res["best_it"], res["n_best_inliers"]) == (found, best, best_count), name
        assert res["its_run"] == (found + 1 if found >= 0 else n_its)
        assert res["n_degenerate"] == int((flags[:res["its_run"]] & S.HYP_DEGENERATE != 0).sum())
        if found >= 0:
            assert res["n_inliers"] == counts[found] and results[name][0][1].tobytes() == sims[found].tobytes()


def test_of_equal_hypotheses_the_later_is_the_best(worlds, results):
    w, d, _ = worlds["equals"]
    res = results["equals"][0][0]
    N, counts, flags, _ = S.hypotheses(w, d)
    assert N == 25 and res["max_its"] == 7 and res["its_run"] == 7
    top = np.flatnonzero(counts[:7] == 20)
    assert len(top) >= 2 and counts[:7].max() == 20  # several hypotheses explain exactly the 20 clean ones
    assert res["best_it"] == top[-1] != top[0] and res["n_best_inliers"] == 20
    # exactly minInliers inliers do not end the solver ...
    assert res["found_it"] == -1 and res["status"] == S.NO_RESULT and res["n_inliers"] == 0
    assert not results["equals"][0][1].any() and (results["equals"][0][2] == -1).all() and not results["equals"][0][3].any()
    # ... minInliers + 1 do, at the first of them
    res19 = results["equals_19"][0][0]
    assert res19["found_it"] == top[0] and res19["its_run"] == top[0] + 1 and res19["n_inliers"] == 20 and res19["status"] == 0


def test_small_counts(results):
    one = results["exactly_min"][0][0]
    assert one["n_correspondences"] == 20 and one["max_its"] == 1 and one["its_run"] == 1  # N == minInliers: one iteration
    assert one["found_it"] == -1 and one["best_it"] == 0 and one["n_best_inliers"] == 20 and one["status"] == S.NO_RESULT
    few = results["below_min"][0][0]
    assert few["n_correspondences"] == 19 and few["status"] == S.FEW_POINTS | S.NO_RESULT and few["its_run"] == 0
    assert few["max_its"] == 300
    three = results["three"][0][0]  # minInliers = 3 = N: one iteration, three inliers, not more than three
    assert three["max_its"] == 1 and three["n_best_inliers"] == 3 and three["found_it"] == -1
    empty = results["empty"][0][0]
    assert empty["n_correspondences"] == 0 and empty["status"] == S.FEW_POINTS | S.NO_RESULT


# ---- degenerate triples ----

def test_coincident_points_are_counted_and_not_followed(worlds, results):
    w, d, _ = worlds["coincident"]
    _, counts, flags, sims = S.hypotheses(w, d[:1])
    assert flags[0] == S.HYP_DEGENERATE and counts[0] == 0 and not sims[0].any()
    res = results["coincident"][0][0]
    assert res["n_degenerate"] >= 1 and res["found_it"] > 0 and res["status"] == 0 and np.isfinite(res["R12"]).all()
    i1, i2, Y1, Y2 = S.camera_points_numpy(w)
    s, R, t = S.horn(Y1[:3], Y2[:3])
    assert not np.isfinite(s)  # den = 0


def test_collinear_points_give_a_finite_useless_hypothesis(worlds, results):
    w, d, _ = worlds["collinear"]
    N, counts, flags, sims = S.hypotheses(w, d[:1])
    assert flags[0] == 0 and np.isfinite(sims[0]).all() and counts[0] < 20
    assert results["collinear"][0][0]["found_it"] > 0


def test_identity_rotation_is_finite(worlds, results):
    res, sim, _, _ = results["identity"][0]
    assert res["status"] == 0 and np.isfinite(sim).all() and abs(sim[12] - 1) < 1e-5
    assert np.abs(sim[:9].reshape(3, 3) - np.eye(3)).max() < 1e-5 and np.abs(sim[9:12]).max() < 1e-4
    Y = np.array([[1.0, 2, 8], [-2, 1, 9], [0.5, -1, 12]])
    s, R, t = S.horn(Y, Y)  # exactly the identity: the reference's atan2 + Rodrigues divides 0 / 0 here
    assert abs(s - 1) < 1e-15 and np.abs(R - np.eye(3)).max() < 1e-15 and np.abs(t).max() < 1e-14


def test_the_largest_signed_eigenvalue_wins():
    """Symmetric 4x4 matrices whose most negative eigenvalue has the larger magnitude: the Jacobi returns the largest SIGNED
    one, with numpy.linalg.eigh's vector.  Then Horn on a mirrored triple (P1 a reflection of P2), the worst a triple can do.
    WHY no solver world has |lambda_min| > lambda_max: N's eigenvalues are sigma1 +- sigma2 +- sigma3 with an even number of
    minus signs and their negatives with an odd number, sigma the singular values of M (signed by det M); three points are
    coplanar about their centroid, so M = Pr2 Pr1^T has rank <= 2, sigma3 = 0 and the spectrum is {+-(sigma1 + sigma2), +-(sigma1
    - sigma2)}: symmetric for EVERY triple, lambda_min = -lambda_max exactly (checked below on random triples).  A routine that
    orders by magnitude therefore ties on every hypothesis the solver ever makes and may return the reflection's quaternion --
    the case is not rare but universal, and every world of this file runs it; the strict case exists only for general matrices,
    which the direct check covers."""
    rng = np.random.default_rng(9)
    for k in range(100):
        Q, _ = np.linalg.qr(rng.normal(0, 1, (4, 4)))
        lam = np.array([rng.uniform(0.1, 2), rng.uniform(-1, 0.1), rng.uniform(-3, -1), rng.uniform(-9, -4)])
        if k % 2:
            lam = lam - lam.sum() / 4  # traceless, as Horn's N
        A = (Q * lam) @ Q.T
        A = (A + A.T) / 2
        top, q = S.eig_top(A)
        ref_lam, ref_vec = np.linalg.eigh(A)
        assert abs(ref_lam[0]) > abs(ref_lam[-1]) or k % 2
        assert abs(top - ref_lam[-1]) < 1e-12 and min(np.abs(q - ref_vec[:, -1]).max(), np.abs(q + ref_vec[:, -1]).max()) < 1e-10
    P2 = np.array([[1.0, 2, 8], [-2, 1, 9], [0.5, -1, 12]])
    P1 = P2 * np.array([1.0, 1.0, -1.0])  # mirrored in z
    for _ in range(50):  # the symmetric spectrum of any triple
        A, B = rng.normal(0, 3, (3, 3)), rng.normal(0, 3, (3, 3))
        M = (B - B.mean(0)).T @ (A - A.mean(0))
        Nm = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                       [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                       [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]], [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
        lam = np.linalg.eigvalsh(Nm + np.triu(Nm, 1).T)
        assert np.allclose(lam, -lam[::-1], rtol=0, atol=1e-9 * np.abs(lam).max())
        top, q = S.eig_top(Nm + np.triu(Nm, 1).T)
        assert abs(top - lam[-1]) < 1e-9 * np.abs(lam).max() and top > 0
    s, R, t = S.horn(P1, P2)
    s2, R2, t2 = S.horn_numpy(P1, P2)
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.isfinite([s, *t]).all()
    assert S.sim_difference(s, R, t, s2, R2, t2)[0] < 1e-10 and abs(s - s2) < 1e-10


def test_every_returned_inlier_passes_when_recomputed(worlds, results):
    for name, (w, d, prm) in worlds.items():
        res, sim, row, inl = results[name][0]
        if res["found_it"] < 0:
            continue
        e = S.errors(w, sim, sigma2=prm.get("sigma2"))
        assert np.array_equal(e["inlier"], inl[e["i1"]] != 0), name
        ok = (e["err"][:, 0] < e["err"][:, 2]) & (e["err"][:, 1] < e["err"][:, 3])
        assert np.array_equal(ok, e["inlier"]) and ok.sum() == res["n_inliers"], name


# ---- garbage ----

def bad(w, what):
    """The world with one kind of garbage in it."""
    q = w.copy()
    i1, i2 = w.edges()
    if what == "count":
        q.n1 = q.cap + 1
    elif what == "negative_count":
        q.n1 = -1
    elif what == "count2":
        q.n2 = q.cap + 1
    elif what == "negative_count2":
        q.n2 = -3
    elif what == "match":
        q.match[i1[5]] = q.n2  # the first index KF2 does not have
    elif what == "match_far":
        q.match[i1[5]] = 2 ** 30
    elif what == "octave1":
        q.kps1["octave"][i1[7]] = S.NLEVELS
    elif what == "octave2":
        q.kps2["octave"][i2[7]] = -1
    elif what == "nan_point1":
        q.points1[i1[3], 1] = np.nan
    elif what == "inf_point2":
        q.points2[i2[3], 2] = np.inf
    elif what == "nan_pose1":
        q.pose1[4] = np.nan
    elif what == "inf_pose2":
        q.pose2[11] = -np.inf
    elif what == "nan_keypoint":
        q.kps2["x"][i2[9]] = np.nan
    else:
        raise KeyError(what)
    return q


GARBAGE = (("count", S.BAD_INPUT), ("negative_count", S.BAD_INPUT), ("count2", S.BAD_INPUT), ("negative_count2", S.BAD_INPUT),
           ("match", S.BAD_INPUT), ("match_far", S.BAD_INPUT), ("octave1", S.BAD_INPUT), ("octave2", S.BAD_INPUT),
           ("nan_point1", S.NONFINITE), ("inf_point2", S.NONFINITE), ("nan_pose1", S.NONFINITE), ("inf_pose2", S.NONFINITE),
           ("nan_keypoint", S.NONFINITE))


def test_every_garbage_kind(worlds):
    w, d, _ = worlds["clean"]
    for what, bit in GARBAGE:
        for mode in (0, 1):
            res, sim, row, inl = S.solve(bad(w, what), d, mode)
            assert res["status"] == bit | S.NO_RESULT, what
            assert res["n_correspondences"] == 0 and res["its_run"] == 0 and res["found_it"] == -1 and res["best_it"] == -1
            assert not sim.any() and (row == -1).all() and not inl.any() and res["s12"] == 0 and not res["R12"].any()
    # garbage that is not followed is not garbage: the same entries on features without a correspondence
    q = w.copy()
    free = np.setdiff1d(np.arange(w.n1), w.edges()[0])
    q.points1[free[0]] = np.nan
    q.kps1["octave"][free[0]] = 99
    assert S.solve(q, d, 0)[0].tobytes() == S.solve(w, d, 0)[0].tobytes()
    d2 = d.copy()
    d2[0, 2] = -5
    res = S.solve(w, d2, 0)[0]
    assert res["status"] == S.BAD_DRAWS and res["found_it"] >= 1


# ---- the stand-alone program ----

def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/sim3_ref_main.cpp links the restatement into a program of its own (two worlds, both forms of iterate) built
    with -fsanitize=address,undefined: nothing sanitised is loaded into Python."""
    exe = str(tmp_path / "sim3_ref_main")
    cmd = S.compile_command(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  os.path.join(ROOT, "tests", "cpp", "sim3_ref_main.cpp")))
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "SIM3 REF OK" in p.stdout, p.stdout


# ---- the C++ shim ----

def build_shim_sim3(orbx, out_dir):
    """Compiles tests/cpp/shim_sim3.cpp: Sim3Solver of the C++ shim next to the C ABI."""
    exe = os.path.join(str(out_dir), "shim_sim3")
    libdir = os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "shim_sim3.cpp"), "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return exe


def test_shim_sim3_compiles(orbx, tmp_path):
    build_shim_sim3(orbx, tmp_path)


# ======== ORBmatcher::SearchBySim3 (include/orbx.h, "loop closing: matching under a similarity") ========

K512 = np.array([[512.0, 0, 320.0], [0, 512.0, 240.0], [0, 0, 1]], np.float32)  # u = 512 x / z + 320 is exact for the cases below
ZEROS, ONES = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)


def bits(k):
    """A descriptor with the first k bits set."""
    return np.packbits(np.arange(256) < k)


def pixel(X, K=K512):
    """Where the f32 rule puts X (identity poses and similarity)."""
    f = np.float32
    X = np.asarray(X, f)
    iz = f(1) / X[2]
    return f(K[0, 0] * f(X[0] * iz) + K[0, 2]), f(K[1, 1] * f(X[1] * iz) + K[1, 2])


def one_way(points, feats, th=7.5, orb_dist=100, pdesc=None, **kw):
    """A hand-made pair under the identity: KF1 holds `points` = (X, descriptor, min, max) on features of its own, KF2 the features
    `feats` = (u, v, octave, descriptor) WITHOUT points, so only direction 1 -> 2 searches -> (world, the restatement's answer)."""
    w = S.MWorld(max(len(points), len(feats), 1), K=K512, pdesc=pdesc is not None)
    for k, (X, d, lo, hi) in enumerate(points):
        u, v = pixel(X) if X[2] > 0 else (0.0, 0.0)
        i = w.feature(0, u, v, 0, d)
        w.point(0, i, X, lo, hi, pdesc=None if pdesc is None else pdesc[k])
    for u, v, o, d in feats:
        w.feature(1, u, v, o, d)
    return w, S.search_by_sim3(w, th, orb_dist, **kw)


def _match_worlds():
    """name -> (world, th, orb_dist): the worlds the GPU test runs too."""
    if "m" in _cache:
        return _cache["m"]
    W = {}
    W["truth"] = (S.make_match_world(300, 1), 7.5, 100)
    W["truth_noisy"] = (S.make_match_world(250, 2, noise_bits=30, s=0.7, rot=(-0.1, 0.08, 0.15), t=(-0.3, 0.2, 0.6)), 7.5, 100)
    W["truth_pdesc"] = (S.make_match_world(200, 3, pdesc=True, noise_bits=10), 7.5, 100)
    W["truth_tight"] = (S.make_match_world(300, 4, noise_bits=60), 3.0, 50)
    W["w1500"] = (S.make_match_world(1300, 5, extra=200, noise_bits=20), 7.5, 100)
    W["empty1"] = (_emptied(S.make_match_world(100, 6), 0), 7.5, 100)
    W["empty2"] = (_emptied(S.make_match_world(100, 6), 1), 7.5, 100)
    # the second setting: K_ANISO, 5 levels of 1.37 (the world carries its scale table), KF1 rolled by 89 degrees against KF2
    W["truth@2"] = (S.make_match_world(150, 101, rot=S.ROLL, **S.SECOND), 7.5, 100)
    W["truth_noisy@2"] = (S.make_match_world(120, 102, noise_bits=30, s=0.7, rot=S.ROLL, t=(-0.3, 0.2, 0.6), **S.SECOND), 7.5, 100)
    W["disagree"] = (_disagree_world(), 7.5, 100)
    W["two_on_one"] = (_two_on_one_world(), 7.5, 100)
    W["behind_and_out"] = (_behind_world(), 7.5, 100)
    _cache["m"] = W
    return W


def _emptied(w, side):
    w.n[side] = 0
    return w


def _disagree_world():
    """Identity similarity.  KF1's point A (descriptor 0 bits) lies at pixel p; KF2 has feature b there with 10 bits.  KF2's
    point on b projects to p too, where KF1 has A (10 bits from b) and, 2 px away, C (11 bits set: 1 bit from b).  A picks b, b
    picks C: no agreement for A; C (a point too) picks b as well and b picks C back: kept."""
    w = S.MWorld(4, K=K512)
    X = np.array([1.0, 0.5, 8.0], np.float32)
    u, v = pixel(X)
    a = w.feature(0, u, v, 0, bits(0))
    c = w.feature(0, u + 2, v, 0, bits(11))
    b = w.feature(1, u, v, 0, bits(10))
    w.point(0, a, X, 0.1, None)
    w.point(0, c, X, 0.1, None)  # (its point projects to p as well)
    w.point(1, b, X, 0.1, None)
    w.truth = dict(a=a, b=b, c=c)
    return w


def _two_on_one_world():
    """Two points of KF1 at one pixel (descriptors 3 and 5 bits) pick KF2's only feature there (0 bits); it picks the nearer."""
    w = S.MWorld(4, K=K512)
    X = np.array([-1.0, 0.25, 8.0], np.float32)
    u, v = pixel(X)
    p, q = w.feature(0, u, v, 0, bits(5)), w.feature(0, u + 1, v, 0, bits(3))
    j = w.feature(1, u, v, 0, bits(0))
    w.point(0, p, X, 0.1, None)
    w.point(0, q, X, 0.1, None)
    w.point(1, j, X, 0.1, None)
    w.truth = dict(p=p, q=q, j=j)
    return w


def _behind_world():
    """A truth world turned so that many points fall behind KF2's camera or outside its image under a wrong similarity."""
    w = S.make_match_world(200, 7)
    w.sim[9:12] = (3.0, -2.0, -9.0)
    return w


def test_msim3_python_mirror(orbx):
    assert ctypes.sizeof(orbx.MatchSim3Result) == orbx.MSIM3_RESULT_DTYPE.itemsize == S.MSIM3_RESULT_DTYPE.itemsize == 64
    S.search_by_sim3(S.MWorld(1))
    assert S.lib().s3r_msim3_result_size() == 64 and orbx.MSIM3_RESULT_DTYPE == S.MSIM3_RESULT_DTYPE
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    assert "#define ORBX_MSIM3_BAD_INPUT 2 " in hdr and "#define ORBX_MSIM3_NONFINITE 4 " in hdr
    assert orbx.MSIM3_BAD_INPUT == S.MSIM3_BAD_INPUT == 2 and orbx.MSIM3_NONFINITE == S.MSIM3_NONFINITE == 4
    L = ctypes.CDLL(orbx.lib_path())
    assert hasattr(L, "orbx_match_sim3_batch_device") and hasattr(L, "orbx_match_sim3")
    for name in ("match_sim3_pairs_device", "match_sim3", "compute_sim3_pairs_device"):
        assert callable(getattr(orbx.ORBextractor, name))
    assert callable(orbx.ORBmatcher.SearchBySim3)


def test_msim3_refusals_without_a_context(orbx):
    L = orbx.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    a, b = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    neg, beyond = np.array([0, -1], np.int32), np.array([2, 0], np.int32)
    K = np.eye(3, dtype=np.float32)
    d = ctypes.c_void_p(4096)
    bd = lambda *v: ctypes.byref(orbx._Bounds(*v))  # noqa: E731

    def batch(n_frames=2, n_pairs=2, k1=p(a), k2=p(b), s1=p(a), s2=p(b), kps=d, desc=d, n=d, cap=16, n_sets=2, pts=d, mask=d, pdesc=d,
              dist=d, pose=d, sim=d, K=p(K), bounds=bd(0, 640, 0, 480), th=7.5, od=100, m=d, out=d):
        return L.orbx_match_sim3_batch_device(None, n_frames, n_pairs, k1, k2, s1, s2, kps, desc, n, cap, n_sets, pts, mask, pdesc, dist,
                                              pose, sim, K, bounds, th, od, m, out)
    assert batch() == orbx.E_HIP and batch(mask=None, pdesc=None, od=0) == orbx.E_HIP and batch(od=256) == orbx.E_HIP
    assert batch(n_pairs=0, k1=None, k2=None, s1=None, s2=None) == orbx.E_HIP
    for bad_ in (dict(n_frames=-1), dict(n_pairs=-1), dict(n_sets=-1), dict(cap=0), dict(k1=None), dict(k2=None), dict(s1=None),
                 dict(s2=None), dict(kps=None), dict(desc=None), dict(n=None), dict(pts=None), dict(dist=None), dict(pose=None),
                 dict(sim=None), dict(K=None), dict(bounds=None), dict(m=None), dict(out=None), dict(n_frames=1), dict(n_sets=1),
                 dict(k1=p(neg)), dict(k2=p(beyond)), dict(s1=p(beyond)), dict(s2=p(neg)), dict(th=0.0), dict(th=float("nan")),
                 dict(od=-1), dict(od=257), dict(bounds=bd(0, 0, 0, 480)), dict(bounds=bd(0, 640, 480, 0))):
        assert batch(**bad_) == orbx.E_BADARG, bad_
    assert batch(cap=16385) == orbx.E_CAPACITY and batch(cap=16384) == orbx.E_HIP
    k, dd, pts, q = np.zeros(4, orbx.KEYPOINT_DTYPE), np.zeros((4, 32), np.uint8), np.zeros((4, 3), np.float32), np.zeros((4, 2), np.float32)
    pose, sim, m, msk, res = np.zeros(12, np.float32), np.zeros(13, np.float32), np.zeros(4, np.int32), np.zeros(4, np.uint8), orbx.MatchSim3Result()

    def host(n1=4, n2=4, k1=p(k), m1=None, m2=None, pd1=None, pd2=None, T1=p(pose), sim=p(sim), row=p(m), th=7.5, od=100, res=ctypes.byref(res)):
        return L.orbx_match_sim3(None, k1, p(dd), n1, p(pts), m1, pd1, p(q), T1, p(k), p(dd), n2, p(pts), m2, pd2, p(q), p(pose), sim, p(K),
                                 bd(0, 640, 0, 480), th, od, row, res)
    assert host() == orbx.E_HIP and host(m1=p(msk), m2=p(msk), pd1=p(dd), pd2=p(dd)) == orbx.E_HIP
    for bad_ in (dict(n1=-1), dict(n2=-1), dict(k1=None), dict(m1=p(msk)), dict(pd2=p(dd)), dict(T1=None), dict(sim=None), dict(row=None),
                 dict(res=None), dict(th=-1.0), dict(od=300)):
        assert host(**bad_) == orbx.E_BADARG, bad_
    assert host(n1=16385) == orbx.E_CAPACITY


@pytest.mark.parametrize("name", ["truth", "truth_noisy", "truth_pdesc", "w1500", "truth@2", "truth_noisy@2"])
def test_truth_worlds_give_every_unmatched_point_its_partner(name):
    w, th, od = _match_worlds()[name]
    e = S.search_by_sim3(w, th, od)
    t = w.truth
    new = ~t["have"]
    # visible: searched in both directions (inside the other image and its distance range)
    vis = new & (e["proj1"][t["slots1"], 4] == 5.0) & (e["proj2"][t["slots2"], 4] == 5.0)
    for side, sl in ((0, t["slots1"]), (1, t["slots2"])):  # (Frame::PosInGrid rounds: a feature in the last half cell is in no cell)
        vis &= (w.kps[side]["x"][sl] < 634.9) & (w.kps[side]["y"][sl] < 474.9)
    assert e["res"]["status"] == 0 and e["res"]["n_found"] == vis.sum() >= 0.95 * new.sum()
    assert new.sum() == e["res"]["n_points_12"] == e["res"]["n_points_21"]
    assert np.array_equal(e["matches"][t["slots1"][vis | ~new]], t["slots2"][vis | ~new])  # the old entries as they were, the new ones the partners
    assert np.array_equal(e["vn1"][t["slots1"][vis]], t["slots2"][vis]) and np.array_equal(e["vn2"][t["slots2"][vis]], t["slots1"][vis])
    assert (e["vn1"][t["slots1"][~new]] == -1).all() and (e["vn2"][t["slots2"][~new]] == -1).all()  # already matched: skipped on both sides
    rest = np.setdiff1d(np.arange(w.cap), t["slots1"][vis | ~new])
    assert (e["matches"][rest] == -1).all()
    new = vis
    # the predicted levels are the features' octaves (the worlds' distances are made for it)
    assert np.array_equal(e["proj1"][t["slots1"][new], 3].astype(int), t["lev"][new])


def test_candidate_lists_equal_the_reference_grid():
    """The restatement's KeyFrame::GetFeaturesInArea against the reference's own compiled Frame::GetFeaturesInArea without level
    bounds (tests/ref_lib.py), order included, at the projections of three worlds."""
    import ref_lib
    ref_lib.lib()
    several = 0
    for name in ("truth", "truth_noisy", "w1500"):
        w, th, od = _match_worlds()[name]
        e = S.search_by_sim3(w, th, od)
        for side, proj in ((1, e["proj1"]), (0, e["proj2"])):  # direction 1 -> 2 searches KF2's grid
            for i in np.flatnonzero(proj[:, 4] == 5.0)[:150]:
                u, v, r = (float(x) for x in proj[i, :3])
                want = ref_lib.features_in_area(w.kps[side][:w.n[side]], w.bounds, u, v, r)
                got = S.features_in_area_nolevels(w.kps[side][:w.n[side]], w.bounds, u, v, r)
                assert np.array_equal(got, want), (name, side, int(i))
                several += len(want) > 1
    assert several >= 20


def test_disagreement_is_left_out_and_counted():
    w, th, od = _match_worlds()["disagree"]
    e = S.search_by_sim3(w, th, od)
    t = w.truth
    assert e["vn1"][t["a"]] == t["b"] and e["vn1"][t["c"]] == t["b"] and e["vn2"][t["b"]] == t["c"]
    assert e["matches"][t["a"]] == -1 and e["matches"][t["c"]] == t["b"]
    assert e["res"]["n_found"] == 1 and e["res"]["n_one_sided"] == 1


def test_two_points_on_one_feature_keep_the_one_it_picks_back():
    w, th, od = _match_worlds()["two_on_one"]
    e = S.search_by_sim3(w, th, od)
    t = w.truth
    assert e["vn1"][t["p"]] == t["j"] == e["vn1"][t["q"]] and e["vn2"][t["j"]] == t["q"]
    assert e["matches"][t["p"]] == -1 and e["matches"][t["q"]] == t["j"] and e["res"]["n_found"] == 1 and e["res"]["n_one_sided"] == 1


def test_already_matched_entries_are_skipped_and_never_overwritten():
    w = _two_on_one_world()
    t = w.truth
    w.match[t["p"]] = t["j"]  # the farther point already holds the feature
    e = S.search_by_sim3(w)
    assert e["matches"][t["p"]] == t["j"] and e["matches"][t["q"]] == -1
    assert e["vn1"][t["p"]] == -1 and e["vn2"][t["j"]] == -1 and e["vn1"][t["q"]] == t["j"]  # q still picks it; nobody picks back
    assert e["res"]["n_points_12"] == 1 and e["res"]["n_points_21"] == 0 and e["res"]["n_one_sided"] == 1
    w.match[t["p"]] = 99  # an entry beyond KF2's count: flagged, kept, followed nowhere
    e = S.search_by_sim3(w)
    assert e["res"]["status"] == S.MSIM3_BAD_INPUT and e["matches"][t["p"]] == 99 and e["matches"][t["q"]] == t["j"]


def test_depth_zero_and_behind():
    feats = [(320.0, 240.0, 0, ZEROS)]
    w, e = one_way([((0.0, 0.0, 8.0), ZEROS, 0.1, None), ((0.0, 0.0, 0.0), ZEROS, 0.1, None), ((0.0, 0.0, -8.0), ZEROS, 0.1, None),
                    ((1.0, 0.0, -0.0), ZEROS, 0.1, None)], feats)
    assert e["vn1"][:4].tolist() == [0, -1, -1, -1]
    assert e["proj1"][:4, 4].tolist() == [5.0, 2.0, 1.0, 2.0]  # z == 0 (and -0) is not "behind": it fails IsInImage
    assert e["res"]["n_behind_12"] == 1 and e["res"]["n_out_image_12"] == 2 and e["res"]["n_points_12"] == 4


def test_image_bounds_are_closed_below_and_open_above():
    pts = [((-5.0, 0.0, 8.0), ZEROS, 0.1, None), ((5.0, 0.0, 8.0), ZEROS, 0.1, None), ((0.0, -3.75, 8.0), ZEROS, 0.1, None),
           ((0.0, 3.75, 8.0), ZEROS, 0.1, None)]
    assert [pixel(p[0]) for p in pts] == [(0.0, 240.0), (640.0, 240.0), (320.0, 0.0), (320.0, 480.0)]
    feats = [(0.0, 240.0, 0, ZEROS), (639.0, 240.0, 0, ZEROS), (320.0, 0.0, 0, ZEROS), (320.0, 479.0, 0, ZEROS)]
    w, e = one_way(pts, feats)
    assert e["proj1"][:4, 4].tolist() == [5.0, 2.0, 5.0, 2.0] and e["vn1"][:4].tolist() == [0, -1, 2, -1]
    assert e["res"]["n_out_image_12"] == 2


def test_distance_limits_are_inside():
    f = np.float32
    X = (0.0, 0.0, 8.0)  # dist3D = 8 exactly
    lo = f(10.0)
    assert f(f(0.8) * lo) == f(8.0)  # on the lower limit: dist3D < 0.8f * min is false
    lo_out = lo
    while f(f(0.8) * lo_out) <= f(8.0):
        lo_out = np.nextafter(lo_out, f(np.inf))
    hi = f(8.0 / 1.2)
    while f(f(1.2) * hi) < f(8.0):
        hi = np.nextafter(hi, f(np.inf))
    assert f(f(1.2) * hi) == f(8.0)  # on the upper limit: dist3D > 1.2f * max is false
    hi_out = np.nextafter(hi, f(-np.inf))
    assert f(f(1.2) * hi_out) < f(8.0)
    pts = [(X, ZEROS, lo, 7.0), (X, ZEROS, lo_out, 7.0), (X, ZEROS, 0.1, hi), (X, ZEROS, 0.1, hi_out)]
    w, e = one_way(pts, [(320.0, 240.0, 0, ZEROS)])
    assert e["proj1"][:4, 4].tolist() == [5.0, 3.0, 5.0, 3.0] and e["res"]["n_out_distance_12"] == 2
    assert e["proj1"][2, 3] == 0.0 and e["vn1"][:4].tolist() == [0, -1, 0, -1]  # max / dist = 0.83: level 0


def test_octave_window_is_level_minus_one_to_level():
    X = (0.0, 0.0, 8.0)
    sc = S.scale_table()
    feats = [(320.0, 240.0, o, bits(o)) for o in (4, 3, 2, 1, 0)]  # the better descriptors lie outside the window
    # level 3: max / dist in (1.2^2, 1.2^3]
    w, e = one_way([(X, bits(4), 0.1, float(8 * sc[3] * 0.95))], feats)
    assert e["proj1"][0, 3] == 3.0 and e["vn1"][0] == 1 and abs(e["proj1"][0, 2] - 7.5 * sc[3]) < 1e-5  # octaves 2 and 3: 3 is nearer
    w, e = one_way([(X, bits(3), 0.1, float(8 * sc[3] * 0.95))], [f for f in feats if f[2] not in (2, 3)])
    assert e["vn1"][0] == -1 and e["res"]["n_with_candidates_12"] == 0  # octaves 4, 1, 0 are outside
    # level 0: octave 0 only
    w, e = one_way([(X, bits(4), 0.1, 7.0)], feats)
    assert e["proj1"][0, 3] == 0.0 and e["vn1"][0] == 4
    w, e = one_way([(X, bits(4), 0.1, 7.0)], feats[:4])
    assert e["vn1"][0] == -1
    # the largest level: the table stops at nlevels - 1
    w, e = one_way([(X, bits(7), 0.1, 8000.0)], [(320.0, 240.0, 7, ZEROS), (320.0, 240.0, 6, bits(1))])
    assert e["proj1"][0, 3] == 7.0 and e["vn1"][0] == 1


def test_orb_dist_is_inclusive_and_256_can_win():
    X = (0.0, 0.0, 8.0)
    w, e = one_way([(X, ZEROS, 0.1, 7.0)], [(320.0, 240.0, 0, bits(100))], orb_dist=100)
    assert e["vn1"][0] == 0 and e["res"]["n_over_dist_12"] == 0
    w, e = one_way([(X, ZEROS, 0.1, 7.0)], [(320.0, 240.0, 0, bits(101))], orb_dist=100)
    assert e["vn1"][0] == -1 and e["res"]["n_over_dist_12"] == 1 and e["res"]["n_with_candidates_12"] == 1
    w, e = one_way([(X, ZEROS, 0.1, 7.0)], [(320.0, 240.0, 0, ONES)], orb_dist=256)
    assert e["vn1"][0] == 0  # bestDist starts at INT_MAX
    w, e = one_way([(X, ZEROS, 0.1, 7.0)], [(320.0, 240.0, 0, ONES)], orb_dist=255)
    assert e["vn1"][0] == -1
    # the first of equal distances, in the grid's order: the lower index inside a cell
    w, e = one_way([(X, ZEROS, 0.1, 7.0)], [(320.5, 240.0, 0, bits(7)), (320.0, 240.0, 0, bits(7))])
    assert e["vn1"][0] == 0


def test_point_descriptors_replace_the_features_own():
    X = (0.0, 0.0, 8.0)
    feats = [(320.0, 240.0, 0, bits(0)), (321.0, 240.0, 0, bits(200))]
    w, e = one_way([(X, bits(0), 0.1, 7.0)], feats, orb_dist=256)
    assert e["vn1"][0] == 0  # the feature's own descriptor
    w, e = one_way([(X, bits(0), 0.1, 7.0)], feats, orb_dist=256, pdesc=[bits(190)])
    assert e["vn1"][0] == 1  # the point's


def test_msim3_garbage_is_flagged_and_dropped():
    w, th, od = _match_worlds()["truth"]
    base = S.search_by_sim3(w)
    i = w.truth["slots1"][~w.truth["have"]][0]
    for kind in ("point", "dist"):
        q = w.copy()
        if kind == "point":
            q.points[0][i, 1] = np.nan
        else:
            q.dist[0][i, 1] = np.inf
        e = S.search_by_sim3(q)
        assert e["res"]["status"] == S.MSIM3_NONFINITE and e["matches"][i] == -1 and e["res"]["n_found"] == base["res"]["n_found"] - 1
    for kind in ("s0", "sneg", "snan", "rnan", "pose"):
        q = w.copy()
        if kind == "pose":
            q.pose[1][3] = np.nan
        elif kind == "rnan":
            q.sim[4] = np.inf
        else:
            q.sim[12] = dict(s0=0.0, sneg=-1.3, snan=np.nan)[kind]
        e = S.search_by_sim3(q)
        assert e["res"]["status"] == S.MSIM3_NONFINITE and np.array_equal(e["matches"], w.match), kind
        assert e["res"]["n_points_12"] == 0 and e["res"]["n_found"] == 0
    q = w.copy()
    q.n[1] = q.cap + 5
    assert S.search_by_sim3(q)["res"]["status"] & S.MSIM3_BAD_INPUT
    e = S.search_by_sim3(_match_worlds()["behind_and_out"][0])
    r = e["res"]
    assert r["n_behind_21"] >= 10 and r["n_out_image_21"] >= 10 and r["n_out_distance_12"] >= 10 and r["n_over_dist_12"] >= 10 and r["status"] == 0, r
