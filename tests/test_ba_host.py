"""The two-view bundle adjustment without a GPU (include/orbx.h, "behind the Initializer: two-view bundle adjustment"): the CPU
restatement tests/cpp/ba_ref.cpp, which the device must equal bit for bit (tests/test_gpu_ba.py), is itself checked here --
against an independent numpy statement of the first Levenberg-Marquardt step, against properties that need no tolerance, against
ground truth on a synthetic scene -- and its counters show that the shared worlds run every branch.  Then the ABI's refusals and
the C++ shim's build."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import ba_ref_lib as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_WORLDS = ("general", "rejecting", "huber", "mirrored", "few")
ALL_WORLDS = STEP_WORLDS + ("converged",)

# Measured on the development machine (x86-64, glibc): the largest |sinCos(x) - libm| over 300 001 angles in [1e-5, pi].  The
# test asserts twice this value.
SINCOS_MEASURED = 1.1102230246251565e-16
# Measured likewise: the largest relative difference (max |a - b| / max |b| per vector) between the restatement's first step and
# the numpy statement's over STEP_WORLDS, in xp, xl, chi2_initial and lambda.  The numerical derivatives (central differences,
# h = 1e-6) dominate it, so the test asserts 100 times this value.
STEP_MEASURED = 4.3e-6
# The same measurement over the pairs of the second setting (ba_ref_lib.SECOND_WORLDS: K_ANISO, 5 levels of 1.37, frame 2 rolled
# by 89 degrees; the largest: few, 1.02e-5), under the same margin of 100.
STEP_MEASURED_2 = 1.02e-5


@pytest.fixture(scope="module")
def results():
    """{(world, n_iterations): (result, points, counters)} of the restatement, computed once and left unchanged."""
    out = {}
    for name in ALL_WORLDS:
        for it in (20, 3):
            out[name, it] = B.bundle_adjust(B.world(name), it, 100, False)
    return out


def test_sin_cos_stay_close_to_libm():
    xs = np.r_[np.linspace(1e-5, math.pi, 200001), np.random.default_rng(0).uniform(1e-5, math.pi, 100000)]
    worst = 0.0
    for x in xs:
        s, c = B.sincos(float(x))
        worst = max(worst, abs(s - math.sin(x)), abs(c - math.cos(x)))
    print("largest distance from libm:", worst)
    assert worst <= 2 * SINCOS_MEASURED
    # the quadrants beyond pi and the edge of the domain
    for x in (4.0, 5.5, 100.0, 524287.5):
        s, c = B.sincos(x)
        assert abs(s - math.sin(x)) < 1e-10 and abs(c - math.cos(x)) < 1e-10, x
    for x in (-1.0, 524288.0, float("inf"), float("nan")):
        s, c = B.sincos(x)
        assert math.isnan(s) and math.isnan(c), x


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def test_first_step_agrees_with_the_numpy_statement(setting="first"):
    """The Schur elimination, the Jacobians and Huber's weights against numerically differentiated residuals and one dense solve
    of the full (6 + 3n) damped normal equations."""
    worst, sig = 0.0, B.inv_sigma2_of(setting)
    for name in (STEP_WORLDS if setting == "first" else tuple(B.SECOND_WORLDS)):
        w = B.world(name, setting)
        a, b = B.first_step(w, sig), B.first_step_numpy(w, sig)
        assert a is not None, name
        assert np.array_equal(a["idx"], B.pair_graph(w)[0])
        d = max(_rel(a["xp"], b["xp"]), _rel(a["xl"], b["xl"]), _rel([a["chi2_initial"]], [b["chi2_initial"]]), _rel([a["lam"]], [b["lam"]]))
        print(name, "largest relative difference:", d)
        worst = max(worst, d)
    assert worst <= 100 * (STEP_MEASURED if setting == "first" else STEP_MEASURED_2)


def test_chi2_never_grows_and_the_quaternion_is_a_unit(results):
    for key, (r, _, _) in results.items():
        assert r["chi2_final"] <= r["chi2_initial"], key
        assert abs(float(np.sqrt((r["q"] ** 2).sum())) - 1.0) <= 2.0 ** -52, key
        assert r["q"][3] >= 0, key
        assert r["iterations"] >= 1 and r["lm_trials"] >= r["iterations"], key


def test_no_iteration_is_the_round_trip_of_the_inputs():
    w = B.world("general")
    r, p, c = B.bundle_adjust(w, 0, 100, False)
    assert r["status"] == 0 and r["iterations"] == 0 and r["lm_trials"] == 0 and r["n_points"] == 300
    assert p.tobytes() == w.p3d.tobytes()
    assert r["t21"].tobytes() == w.init["t21"][0].tobytes() and np.array_equal(r["t"], w.init["t21"][0].astype(np.float64))
    # the rotation goes through a normalised quaternion: each entry within a few f32 roundings of the input's
    assert np.abs(r["R21"] - w.init["R21"][0]).max() <= 4 * 2.0 ** -24
    assert r["chi2_initial"] == 0 and r["chi2_final"] == 0 and c == dict.fromkeys(B.COUNTERS, 0)


def _untouched(r, p, w, status):
    assert r["status"] == status
    assert p.tobytes() == w.p3d.tobytes()
    assert r["R21"].tobytes() == w.init["R21"][0].tobytes() and r["t21"].tobytes() == w.init["t21"][0].tobytes()
    for f in ("n_points", "iterations", "lm_trials", "rejected_trials", "solver_failures", "stop_reason", "chi2_initial", "chi2_final",
              "lambda", "median_depth"):
        assert r[f] == 0, f
    assert not r["q"].any() and not r["t"].any()


def test_a_skipped_pair_keeps_its_inputs():
    w = B.skipped(B.world("general"), status=B.NEGATIVE_DEPTH)
    r, p, _ = B.bundle_adjust(w, 20, 100, True)
    _untouched(r, p, w, B.SKIPPED)


def _angle(Ra, Rb):
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(Ra.T @ Rb) - 1) / 2))))


def _dir(a, b):
    return math.degrees(math.acos(max(-1.0, min(1.0, float(a @ b) / float(np.linalg.norm(a) * np.linalg.norm(b))))))


def test_general_scene_moves_towards_the_truth(setting="first"):
    w = B.world("truth", setting)
    r, _, _ = B.bundle_adjust(w, 20, 100, False, B.inv_sigma2_of(setting))
    T = w.truth
    Rin, tin = w.init["R21"][0].astype(np.float64), w.init["t21"][0].astype(np.float64)
    assert _angle(r["R21"].astype(np.float64), T["R"]) < _angle(Rin, T["R"])
    assert _dir(r["t21"].astype(np.float64), T["t"]) < _dir(tin, T["t"])
    # the robust chi2 at the true pose with the true points: any minimiser must end below it
    sig = (B.inv_sigma2_table() if setting == "first" else B.inv_sigma2_of(setting)).astype(np.float64)
    truth_chi2, _, _ = B.robust_chi2(T["R"], T["t"], T["X"], T["obs1"], T["obs2"], sig[T["octs"][:, 0]], sig[T["octs"][:, 1]],
                                     w.K.reshape(3, 3).astype(np.float64), float(np.float32(np.sqrt(5.99))))
    print("chi2 at the truth:", truth_chi2, "final:", r["chi2_final"])
    assert r["chi2_final"] < truth_chi2


def test_the_second_setting_against_numpy_and_the_truth():
    """The first step and the general scene under the second setting (ba_ref_lib.SECOND_WORLDS: K_ANISO, 5 levels of 1.37,
    frame 2 rolled by 89 degrees)."""
    test_first_step_agrees_with_the_numpy_statement("second")
    test_general_scene_moves_towards_the_truth("second")


def test_a_table_of_zeros_fails_every_solve():
    """general under a table of zeros: Hpp = 0 and lambda = 1e-5 * 0 = 0, every point's 3x3 block is 0 and the first of them has
    no inverse, so each of the ten trials of the only iteration is a failed solve (stop reason 1).  Status 0, a finite result,
    and the refined points are the input points times the normalisation only.  world("no_weight") under top_level_off_table()
    is the same problem (every edge at a level that weighs nothing) and gives the same bytes."""
    g, idx = B.world("general"), B.pair_graph(B.world("general"))[0]
    rest = np.setdiff1d(np.arange(g.cap), idx)
    for normalize in (False, True):
        r, p, c = B.bundle_adjust(g, 20, 100, normalize, inv_sigma2=B.zero_table())
        assert r["status"] == 0 and r["n_points"] == 300
        assert r["solver_failures"] == r["lm_trials"] == r["rejected_trials"] == 10 and r["iterations"] == 1 and r["stop_reason"] == 1
        assert r["chi2_initial"] == 0 and r["chi2_final"] == 0 and r["lambda"] == 0
        assert c == dict(accepted=0, rejected=10, huber_outliers=0, small_theta=0)
        assert all(np.isfinite(r[f]).all() for f in ("q", "t", "R21", "t21", "median_depth")) and np.isfinite(p).all()
        assert r["median_depth"] == np.sort(g.p3d[idx, 2])[(len(idx) - 1) // 2]
        scale = np.float32(1.0) / r["median_depth"] if normalize else np.float32(1.0)
        assert np.array_equal(p[idx], g.p3d[idx] * scale) and p[rest].tobytes() == g.p3d[rest].tobytes()
        assert np.array_equal(r["t21"], g.init["t21"][0] * scale) and np.abs(r["R21"] - g.init["R21"][0]).max() <= 4 * 2.0 ** -24
        r2, p2, c2 = B.bundle_adjust(B.world("no_weight"), 20, 100, normalize, inv_sigma2=B.top_level_off_table())
        assert r2.tobytes() == r.tobytes() and p2.tobytes() == p.tobytes() and c2 == c
    # the other pairs of tests/test_gpu_ba.py's call keep weighted edges under that table and solve
    for name in ("rejecting", "general"):
        r = B.bundle_adjust(B.world(name), inv_sigma2=B.top_level_off_table())[0]
        assert r["status"] == 0 and r["solver_failures"] == 0 and r["iterations"] > 1, name


def test_a_table_with_one_weight_keeps_every_solve():
    """A mixed pair: weight 1 at level 3, 0 elsewhere, so three quarters of the points have two edges that weigh nothing and a
    3x3 block of zeros.  Found on the restatement: neither NONFINITE nor a failed solve.  Some edge weighs, so lambda = 1e-5 *
    max |diag H| > 0, and the damping makes such a point's block lambda * I with the determinant lambda^3: pointDinv never divides
    by 0.  Status 0, solver_failures == 0, the weightless points get a zero step (their b and their Hpl are 0) and come back bit
    for bit; every point with a weighted edge moves."""
    g, table = B.world("general"), B.one_level_table(3)
    r, p, c = B.bundle_adjust(g, 20, 100, False, inv_sigma2=table)
    assert r["status"] == 0 and r["solver_failures"] == 0 and c["accepted"] > 0 and r["lambda"] > 0
    assert r["chi2_final"] < r["chi2_initial"] and np.isfinite(p).all()
    idx = B.pair_graph(g)[0]
    weighs = (g.k1["octave"][idx] == 3) | (g.k2["octave"][g.m12[idx]] == 3)
    assert 50 <= weighs.sum() <= len(idx) - 150
    assert p[idx[~weighs]].tobytes() == g.p3d[idx[~weighs]].tobytes()
    assert (p[idx[weighs]] != g.p3d[idx[weighs]]).any(axis=1).all()


def test_the_worlds_run_every_branch(results):
    """What the GPU comparison relies on: each branch of the optimisation is taken by at least one of the shared worlds.  None
    of them has a failed solve; that branch is test_a_table_of_zeros_fails_every_solve's."""
    cnt = {k: v[2] for k, v in results.items()}
    res = {k: v[0] for k, v in results.items()}
    assert cnt["rejecting", 20]["rejected"] > 0 and res["rejecting", 20]["rejected_trials"] == cnt["rejecting", 20]["rejected"]
    assert cnt["huber", 20]["huber_outliers"] > 0
    assert cnt["converged", 20]["small_theta"] > 0
    assert all(c["accepted"] > 0 for c in cnt.values())
    assert res["general", 20]["stop_reason"] == 2 and res["general", 20]["iterations"] < 20  # _nBad >= 3
    assert res["general", 3]["stop_reason"] == 0 and res["general", 3]["iterations"] == 3   # all iterations used
    assert res["huber", 20]["stop_reason"] == 0 and res["huber", 20]["iterations"] == 20
    assert res["rejecting", 20]["lm_trials"] == cnt["rejecting", 20]["accepted"] + cnt["rejecting", 20]["rejected"]
    assert all(r["solver_failures"] == 0 for r in res.values())


def test_few_points_and_negative_depth_on_and_off():
    few, mirrored, general = B.world("few"), B.world("mirrored"), B.world("general")
    assert B.bundle_adjust(few, 20, 100, True)[0]["status"] == B.FEW_POINTS
    assert B.bundle_adjust(few, 20, 40, True)[0]["status"] == 0
    assert B.bundle_adjust(few, 20, 41, True)[0]["status"] == B.FEW_POINTS
    r, p, _ = B.bundle_adjust(mirrored, 20, 100, True)
    assert r["status"] == B.NEGATIVE_DEPTH and r["median_depth"] < 0
    r2, p2, _ = B.bundle_adjust(mirrored, 20, 100, False)
    assert p.tobytes() == p2.tobytes() and r["t21"].tobytes() == r2["t21"].tobytes()  # no normalisation under a status bit
    r, p, _ = B.bundle_adjust(general, 20, 100, True)
    r2, p2, _ = B.bundle_adjust(general, 20, 100, False)
    assert r["status"] == 0 and r["median_depth"] > 0 and r["median_depth"] == r2["median_depth"]
    inv = np.float32(1.0) / r["median_depth"]
    assert np.array_equal(r["t21"], r2["t21"] * inv)
    idx = B.pair_graph(general)[0]
    assert np.array_equal(p[idx], p2[idx] * inv)
    rest = np.setdiff1d(np.arange(general.cap), idx)
    assert p[rest].tobytes() == general.p3d[rest].tobytes()  # not a vertex: not touched
    # the median is the element (n - 1) / 2 of the sorted depths
    assert r2["median_depth"] == np.sort(p2[idx, 2])[(len(idx) - 1) // 2]


def _first_vertex(w):
    return int(B.pair_graph(w)[0][0])


def test_bad_inputs_are_reported_and_not_followed():
    g = B.world("general")
    i = _first_vertex(g)
    w = g.padded(g.cap); w.m12[i] = w.n2
    _untouched(*B.bundle_adjust(w)[:2], w, B.BAD_INPUT)
    w = g.padded(g.cap); w.m12[3] = 2 ** 31 - 1
    _untouched(*B.bundle_adjust(w)[:2], w, B.BAD_INPUT)
    for octave in (-1, B.NLEVELS, 2 ** 30):
        w = g.padded(g.cap); w.k1["octave"][i] = octave
        _untouched(*B.bundle_adjust(w)[:2], w, B.BAD_INPUT)
        w = g.padded(g.cap); w.k2["octave"][w.m12[i]] = octave
        _untouched(*B.bundle_adjust(w)[:2], w, B.BAD_INPUT)
    for n1, n2 in ((g.cap + 1, g.n2), (g.n1, g.cap + 1), (-1, g.n2), (g.n1, -5)):
        w = g.padded(g.cap); w.n1, w.n2 = n1, n2
        _untouched(*B.bundle_adjust(w)[:2], w, B.BAD_INPUT)
    # an octave out of range on a keypoint that is no vertex's is nobody's business
    w = g.padded(g.cap)
    free = np.setdiff1d(np.arange(w.n1), B.pair_graph(g)[0])
    w.k1["octave"][free[-1]] = 99
    assert B.bundle_adjust(w)[0]["status"] == 0
    # non-finite inputs
    for v in (np.nan, np.inf):
        w = g.padded(g.cap); w.p3d[i, 1] = v
        r, p, _ = B.bundle_adjust(w)
        assert r["status"] == B.NONFINITE and r["iterations"] == 0 and p.tobytes() == w.p3d.tobytes()
        w = g.padded(g.cap); w.init["t21"][0, 2] = v
        r, p, _ = B.bundle_adjust(w)
        assert r["status"] == B.NONFINITE and r["iterations"] == 0 and p.tobytes() == w.p3d.tobytes()
    # a point in the first camera's plane (z = 0): finite inputs, a non-finite result
    w = g.padded(g.cap); w.p3d[i, 2] = 0.0
    r, p, _ = B.bundle_adjust(w)
    assert r["status"] == B.NONFINITE and p.tobytes() == w.p3d.tobytes() and r["chi2_final"] == 0


def test_no_points_runs_nothing():
    w = B.make_pair(0, 9, cap=4)
    r, p, _ = B.bundle_adjust(w, 20, 100, True)
    assert r["status"] == B.FEW_POINTS and r["n_points"] == 0 and r["iterations"] == 0 and r["median_depth"] == 0
    assert B.bundle_adjust(w, 20, 0, True)[0]["status"] == 0


def test_refusals_without_a_context(orbx):
    """Null pointers, negative counts, capacity < 1, a negative iteration count and a pair index outside [0, n_frames) are
    ORBX_E_BADARG, a capacity of 2^20 is ORBX_E_CAPACITY, ctx == NULL with well-formed arguments is ORBX_E_HIP: all decided
    before a device is touched (there is none here)."""
    L = orbx.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    first, second = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    neg, beyond = np.array([0, -1], np.int32), np.array([2, 0], np.int32)
    K = np.eye(3, dtype=np.float32)
    d = ctypes.c_void_p(4096)  # (a device pointer the call never follows)

    def batch(n_frames=2, n_pairs=2, f=p(first), s=p(second), kps=d, n=d, cap=16, m=d, ir=d, p3d=d, tri=d, K=p(K), sig=None, it=20, out=d,
              p3d_out=d):
        return L.orbx_bundle_adjust_batch_device(None, n_frames, n_pairs, f, s, kps, n, cap, m, ir, p3d, tri, K, sig, it, 100, 1, out, p3d_out)
    assert batch() == orbx.E_HIP
    assert batch(n_pairs=0, f=None, s=None) == orbx.E_HIP  # (ORBX_OK with a context)
    for bad in (dict(n_frames=-1), dict(n_pairs=-1), dict(cap=0), dict(cap=-2), dict(f=None), dict(s=None), dict(kps=None), dict(n=None),
                dict(m=None), dict(ir=None), dict(p3d=None), dict(tri=None), dict(K=None), dict(out=None), dict(p3d_out=None), dict(it=-1),
                dict(n_frames=1), dict(f=p(neg)), dict(s=p(beyond))):
        assert batch(**bad) == orbx.E_BADARG, bad
    assert batch(cap=1 << 20) == orbx.E_CAPACITY
    assert batch(cap=(1 << 20) - 1) == orbx.E_HIP

    k = np.zeros(4, orbx.KEYPOINT_DTYPE)
    m, tri, pts = np.full(4, -1, np.int32), np.zeros(4, np.uint8), np.zeros((4, 3), np.float32)
    ir, res = orbx.InitResult(), orbx.BAResult()

    def host(k1=p(k), n1=4, k2=p(k), n2=4, m=p(m), ir=ctypes.byref(ir), pts=p(pts), tri=p(tri), K=p(K), it=20, res=ctypes.byref(res),
             out=p(pts)):
        return L.orbx_bundle_adjust(None, k1, n1, k2, n2, m, ir, pts, tri, K, None, it, 100, 1, res, out)
    assert host() == orbx.E_HIP
    assert host(n1=0, n2=0, k1=None, k2=None, m=None, pts=None, tri=None, out=None) == orbx.E_HIP
    for bad in (dict(n1=-1), dict(n2=-1), dict(k1=None), dict(k2=None), dict(m=None), dict(ir=None), dict(pts=None), dict(tri=None),
                dict(K=None), dict(it=-1), dict(res=None), dict(out=None)):
        assert host(**bad) == orbx.E_BADARG, bad
    assert host(n1=1 << 20) == orbx.E_CAPACITY


def test_python_mirror_and_extent_guard(orbx):
    assert ctypes.sizeof(orbx.BAResult) == orbx.BA_RESULT_DTYPE.itemsize == B.BA_RESULT_DTYPE.itemsize == 168
    assert orbx.BA_RESULT_DTYPE == B.BA_RESULT_DTYPE
    assert (orbx.BA_SKIPPED, orbx.BA_BAD_INPUT, orbx.BA_NONFINITE, orbx.BA_FEW_POINTS, orbx.BA_NEGATIVE_DEPTH) == (1, 2, 4, 8, 16)
    first, second = np.array([0], np.int32), np.array([1], np.int32)
    cap = 8
    ok = dict(kps=np.zeros(2 * cap * 28, np.uint8), n=np.zeros(2, np.int32), m=np.zeros(cap, np.int32), ir=np.zeros(184, np.uint8),
              p3d=np.zeros(cap * 3, np.float32), tri=np.zeros(cap, np.uint8), res=np.zeros(168, np.uint8), out=np.zeros(cap * 3, np.float32))
    for short in ("kps", "n", "m", "ir", "p3d", "tri", "res", "out"):
        a = dict(ok)
        a[short] = a[short][:-1]
        with pytest.raises(ValueError):
            orbx._need_batch(None, 2, 0, 0, 0, 0, a["kps"], None, a["n"], cap, first, second, a["m"], None, None, init_res=a["ir"],
                             p3d=a["p3d"], triangulated=a["tri"], ba_res=a["res"], p3d_out=a["out"])
    orbx._need_batch(None, 2, 0, 0, 0, 0, ok["kps"], None, ok["n"], cap, first, second, ok["m"], None, None, init_res=ok["ir"],
                     p3d=ok["p3d"], triangulated=ok["tri"], ba_res=ok["res"], p3d_out=ok["out"])


def build_shim_ba(orbx, out_dir):
    """Compiles tests/cpp/shim_ba.cpp: Optimizer::BundleAdjustmentTwoView of the C++ shim next to the C ABI."""
    exe = os.path.join(str(out_dir), "shim_ba")
    libdir = os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "shim_ba.cpp"), "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return exe


def test_shim_ba_compiles(orbx, tmp_path):
    build_shim_ba(orbx, tmp_path)
