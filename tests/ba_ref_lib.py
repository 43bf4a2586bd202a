"""ctypes wrapper around tests/cpp/ba_ref.cpp -- the CPU restatement of the two-view bundle adjustment (include/orbx.h, "behind the
Initializer: two-view bundle adjustment") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary
directory, as tests/match_bow_ref_lib.py compiles its source; a second, independently written numpy statement of the first
Levenberg-Marquardt step (numerically differentiated residuals, the full damped normal equations, numpy.linalg.solve); and the
worlds (synthetic two-view scenes) that tests/test_ba_host.py and tests/test_gpu_ba.py share.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

from pose_ref_lib import K_ANISO, MOTION_2, NLEVELS_2, ROLL, SCALE_FACTOR_2, SECOND, SETTINGS  # noqa: F401 (the second setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ba_ref.cpp")
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
_INIT_INTS = ("status", "model", "n_matches", "best_it_h", "best_it_f", "n_inliers_h", "n_inliers_f", "n_solutions", "best_solution",
              "best_good", "second_good", "reserved")
INIT_RESULT_DTYPE = np.dtype([(n, "<i4") for n in _INIT_INTS] + [(n, "<f4") for n in ("score_h", "score_f", "rh", "parallax")] +
                             [("R21", "<f4", (3, 3)), ("t21", "<f4", 3), ("H21", "<f4", (3, 3)), ("F21", "<f4", (3, 3))])
BA_INTS = ("status", "n_points", "iterations", "lm_trials", "rejected_trials", "solver_failures", "stop_reason", "reserved")
BA_RESULT_DTYPE = np.dtype([(n, "<i4") for n in BA_INTS] + [(n, "<f8") for n in ("chi2_initial", "chi2_final", "lambda")] +
                           [("q", "<f8", 4), ("t", "<f8", 3), ("R21", "<f4", (3, 3)), ("t21", "<f4", 3), ("median_depth", "<f4"),
                            ("reserved2", "<f4")])
assert INIT_RESULT_DTYPE.itemsize == 184 and BA_RESULT_DTYPE.itemsize == 168
SKIPPED, BAD_INPUT, NONFINITE, FEW_POINTS, NEGATIVE_DEPTH = 1, 2, 4, 8, 16
COUNTERS = ("accepted", "rejected", "huber_outliers", "small_theta")
NLEVELS = 8
_L = None


def build(src=SRC) -> ctypes.CDLL:
    """Compiles a restatement source (lib(): the committed one; tests/test_camera_mutants_host.py: an altered copy) and binds it."""
    d = tempfile.mkdtemp(prefix="ba_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libba_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", src, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("ba_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.bar_bundle_adjust.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.bar_bundle_adjust.restype = None
    L.bar_first_step.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.bar_sincos.argtypes = [f64, ctypes.POINTER(f64), ctypes.POINTER(f64)]
    L.bar_sincos.restype = None
    L.bar_huber_delta.restype = f64
    return L


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        _L = build()
    return _L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def inv_sigma2_table(nlevels: int = NLEVELS, scale_factor: float = 1.2) -> np.ndarray:
    """mvInvLevelSigma2 as ORBextractor's constructor computes it (f32)."""
    f32 = np.float32
    scale, out = f32(1.0), np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        scale = f32(scale * f32(scale_factor))
        out[i] = f32(1.0) / f32(scale * scale)
    return out


class Pair:
    """One pair's inputs in the batch layout (arrays of `cap` entries), plus what is known about the scene."""

    def __init__(self, k1, n1, k2, n2, m12, init, p3d, tri, K, truth=None):
        self.k1, self.n1, self.k2, self.n2, self.m12, self.init, self.p3d, self.tri, self.K, self.truth = \
            k1, int(n1), k2, int(n2), m12, init, p3d, tri, K, truth
        self.cap = len(k1)

    def padded(self, cap):
        """The same pair in arrays of a larger capacity."""
        def grow(a, fill=0):
            out = np.full((cap,) + a.shape[1:], fill, a.dtype) if a.dtype != KEYPOINT_DTYPE else np.zeros(cap, a.dtype)
            out[:len(a)] = a
            return out
        return Pair(grow(self.k1), self.n1, grow(self.k2), self.n2, grow(self.m12, -1), self.init.copy(), grow(self.p3d), grow(self.tri),
                    self.K, self.truth)


def sincos(x: float):
    s, c = ctypes.c_double(0), ctypes.c_double(0)
    lib().bar_sincos(float(x), ctypes.byref(s), ctypes.byref(c))
    return s.value, c.value


def bundle_adjust(pair: Pair, n_iterations=20, min_points=100, normalize=True, inv_sigma2=None, nlevels=NLEVELS):
    """The restatement for one pair -> (BA_RESULT_DTYPE record, refined p3d [cap, 3] float32, {counter: value})."""
    sig = np.ascontiguousarray(inv_sigma2_table(nlevels) if inv_sigma2 is None else inv_sigma2, np.float32)
    out, p3d_out, cnt = np.zeros(1, BA_RESULT_DTYPE), np.zeros((pair.cap, 3), np.float32), np.zeros(4, np.int64)
    lib().bar_bundle_adjust(_p(pair.k1), pair.n1, _p(pair.k2), pair.n2, pair.cap, _p(pair.m12), _p(pair.init), _p(pair.p3d), _p(pair.tri),
                            _p(pair.K), _p(sig), len(sig), int(n_iterations), int(min_points), int(bool(normalize)), _p(out), _p(p3d_out),
                            _p(cnt))
    return out[0].copy(), p3d_out, dict(zip(COUNTERS, (int(c) for c in cnt)))


def first_step(pair: Pair, inv_sigma2=None, nlevels=NLEVELS):
    """The restatement's first trial of iteration 0 -> dict(idx, q, t, lambda, chi2_initial, xp [6], xl [n, 3]) or None."""
    sig = np.ascontiguousarray(inv_sigma2_table(nlevels) if inv_sigma2 is None else inv_sigma2, np.float32)
    idx, pose = np.zeros(pair.cap, np.int32), np.zeros(7)
    lam, chi2, xp, xl = np.zeros(1), np.zeros(1), np.zeros(6), np.zeros((pair.cap, 3))
    n = lib().bar_first_step(_p(pair.k1), pair.n1, _p(pair.k2), pair.n2, pair.cap, _p(pair.m12), _p(pair.init), _p(pair.p3d),
                             _p(pair.tri), _p(pair.K), _p(sig), len(sig), _p(idx), _p(pose), _p(lam), _p(chi2), _p(xp), _p(xl))
    if n < 0:
        return None
    return dict(idx=idx[:n].copy(), q=pose[:4].copy(), t=pose[4:].copy(), lam=float(lam[0]), chi2_initial=float(chi2[0]), xp=xp,
                xl=xl[:n].copy())


# ---- the second statement: numpy, rotation matrices, numerical derivatives, one dense solve; nothing shared with the C++ ----

def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def se3_exp(u):
    """(omega, upsilon) -> (R, t) by Rodrigues' formulas."""
    w, v = np.asarray(u[:3], np.float64), np.asarray(u[3:], np.float64)
    th = float(np.linalg.norm(w))
    W = _skew(w)
    if th < 1e-9:
        return np.eye(3) + W, v + 0.5 * W @ v
    A, B, C = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) + A * W + B * W @ W, (np.eye(3) + B * W + C * W @ W) @ v


def _residuals(R, t, X, obs1, obs2, K):
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    Y = X @ R.T + t
    e1 = obs1 - np.c_[X[:, 0] / X[:, 2] * fx + cx, X[:, 1] / X[:, 2] * fy + cy]
    e2 = obs2 - np.c_[Y[:, 0] / Y[:, 2] * fx + cx, Y[:, 1] / Y[:, 2] * fy + cy]
    return e1, e2


def robust_chi2(R, t, X, obs1, obs2, w1, w2, K, delta):
    """Sum of Huber's rho over both edges of every point -> (chi2, weights rho' of the two edge sets)."""
    e1, e2 = _residuals(R, t, X, obs1, obs2, K)
    total, rho1 = 0.0, []
    for e, w in ((e1, w1), (e2, w2)):
        c = w * (e ** 2).sum(axis=1)
        out = c > delta * delta
        total += float(np.where(out, 2 * np.sqrt(np.where(out, c, 1.0)) * delta - delta * delta, c).sum())
        rho1.append(np.where(out, delta / np.sqrt(np.where(out, c, 1.0)), 1.0))
    return total, rho1[0], rho1[1]


def pair_graph(pair: Pair, inv_sigma2=None, nlevels=NLEVELS):
    """The graph of a pair as plain arrays: (idx, X [n, 3] f64, obs1, obs2, w1, w2, R, t, K f64)."""
    sig = (inv_sigma2_table(nlevels) if inv_sigma2 is None else np.asarray(inv_sigma2, np.float32)).astype(np.float64)
    idx = np.array([i for i in range(pair.n1) if pair.m12[i] >= 0 and pair.tri[i]], np.int64)
    m = pair.m12[idx]
    a, b = pair.k1[idx], pair.k2[m]
    X = pair.p3d[idx].astype(np.float64)
    obs1 = np.c_[a["x"], a["y"]].astype(np.float64)
    obs2 = np.c_[b["x"], b["y"]].astype(np.float64)
    return (idx, X, obs1, obs2, sig[a["octave"]], sig[b["octave"]], pair.init["R21"][0].astype(np.float64),
            pair.init["t21"][0].astype(np.float64), pair.K.reshape(3, 3).astype(np.float64))


def first_step_numpy(pair: Pair, inv_sigma2=None, nlevels=NLEVELS, h=1e-6):
    """The first damped Gauss-Newton step on the full (6 + 3n) system -> dict(lam, chi2_initial, xp, xl)."""
    idx, X, obs1, obs2, w1, w2, R, t, K = pair_graph(pair, inv_sigma2, nlevels)
    n = len(idx)
    delta = float(np.float32(np.sqrt(5.99)))
    chi2, r1, r2 = robust_chi2(R, t, X, obs1, obs2, w1, w2, K, delta)
    W = np.r_[np.repeat(r1 * w1, 2), np.repeat(r2 * w2, 2)]  # per residual row: edges of frame 1, then of frame 2

    def res(u, dX):
        dR, dt = se3_exp(u)
        e1, e2 = _residuals(dR @ R, dR @ t + dt, X + dX, obs1, obs2, K)
        return np.r_[e1.reshape(-1), e2.reshape(-1)]

    e0 = res(np.zeros(6), np.zeros_like(X))
    J = np.zeros((4 * n, 6 + 3 * n))
    for k in range(6):
        u = np.zeros(6)
        u[k] = h
        J[:, k] = (res(u, np.zeros_like(X)) - res(-u, np.zeros_like(X))) / (2 * h)
    for c in range(3):  # the points are independent: one perturbation per coordinate serves them all
        dX = np.zeros_like(X)
        dX[:, c] = h
        d = (res(np.zeros(6), dX) - res(np.zeros(6), -dX)) / (2 * h)
        for j in range(n):
            rows = [2 * j, 2 * j + 1, 2 * n + 2 * j, 2 * n + 2 * j + 1]
            J[rows, 6 + 3 * j + c] = d[rows]
    H = J.T @ (W[:, None] * J)
    b = -J.T @ (W * e0)
    lam = 1e-5 * float(np.abs(np.diag(H)).max())
    x = np.linalg.solve(H + lam * np.eye(len(H)), b)
    return dict(lam=lam, chi2_initial=chi2, xp=x[:6], xl=x[6:].reshape(n, 3))


# ---- the worlds the host and the GPU test share ----

K0 = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1]], np.float32)


def rotvec(w):
    return se3_exp(np.r_[np.asarray(w, np.float64), 0, 0, 0])[0]


def make_pair(n, seed=0, cap=None, noise=0.5, outliers=0, twist=(0.004, -0.003, 0.002, 0.01, -0.008, 0.006), point_noise=0.02,
              pose_scale=1.0, mirrored=False, extra=5, nlevels=NLEVELS, motion=((0.02, -0.05, 0.01), (-0.3, 0.02, 0.05)), K=K0,
              scale_factor=1.2):
    """A general scene of n triangulated matches seen from two frames: the true (R, t) and points, pixel noise (in units of the
    keypoint's level sigma), `outliers` gross mismatches, input points off by point_noise, and the input pose = the true one moved by
    the twist, its translation then multiplied by pose_scale.  Frame 1 holds `extra` keypoints without a match and `extra` matched but
    not triangulated ones in between; frame 2 is permuted.  mirrored: points and translation negated (every depth negative)."""
    rng = np.random.default_rng(1000 + seed)
    Rt, tt = rotvec(motion[0]), np.array(motion[1], np.float64)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 8, n)]
    Kd = np.asarray(K, np.float64).reshape(3, 3)
    octs = rng.integers(0, nlevels, (n, 2))
    sigma = scale_factor ** octs

    def proj(P):
        return np.c_[P[:, 0] / P[:, 2] * Kd[0, 0] + Kd[0, 2], P[:, 1] / P[:, 2] * Kd[1, 1] + Kd[1, 2]]
    o1 = proj(X) + rng.normal(0, 1, (n, 2)) * noise * sigma[:, :1]
    o2 = proj(X @ Rt.T + tt) + rng.normal(0, 1, (n, 2)) * noise * sigma[:, 1:]
    bad = rng.choice(n, outliers, replace=False) if outliers else np.zeros(0, np.int64)
    o2[bad] += rng.choice([-1.0, 1.0], (len(bad), 2)) * rng.uniform(20, 40, (len(bad), 2))
    n1 = n + 2 * extra if n else 0
    n2 = n + extra if n else 0
    cap = int(cap or max(n1, n2, 1))
    assert cap >= max(n1, n2)
    k1, k2 = np.zeros(cap, KEYPOINT_DTYPE), np.zeros(cap, KEYPOINT_DTYPE)
    m12, tri, p3d = np.full(cap, -1, np.int32), np.zeros(cap, np.uint8), np.zeros((cap, 3), np.float32)
    slots1 = np.sort(rng.permutation(n1)[:n]) if n else np.zeros(0, np.int64)  # where the n real matches sit in frame 1
    slots2 = rng.permutation(n2)[:n] if n else np.zeros(0, np.int64)
    k1["x"][:n1], k1["y"][:n1] = rng.uniform(0, 640, n1), rng.uniform(0, 480, n1)
    k2["x"][:n2], k2["y"][:n2] = rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)
    k1["octave"][:n1], k2["octave"][:n2] = rng.integers(0, nlevels, n1), rng.integers(0, nlevels, n2)
    k1["x"][slots1], k1["y"][slots1], k1["octave"][slots1] = o1[:, 0], o1[:, 1], octs[:, 0]
    k2["x"][slots2], k2["y"][slots2], k2["octave"][slots2] = o2[:, 0], o2[:, 1], octs[:, 1]
    m12[slots1], tri[slots1] = slots2, 1
    sign = -1.0 if mirrored else 1.0
    p3d[slots1] = sign * (X + rng.normal(0, point_noise, (n, 3)))
    others = np.setdiff1d(np.arange(n1), slots1)
    free2 = np.setdiff1d(np.arange(n2), slots2)
    for j, i in enumerate(others[:extra]):  # matched, not triangulated (their points are left over from another candidate)
        m12[i] = free2[j]
        p3d[i] = rng.normal(0, 1, 3)
    dR, dt = se3_exp(np.asarray(twist, np.float64))
    Rin, tin = dR @ Rt, (dR @ tt + dt) * pose_scale
    init = np.zeros(1, INIT_RESULT_DTYPE)
    init["model"], init["R21"][0], init["t21"][0] = 1, Rin, sign * tin
    truth = dict(R=Rt, t=sign * tt, X=sign * X, slots1=slots1, obs1=o1, obs2=o2, octs=octs)
    return Pair(k1, n1, k2, n2, m12, init, p3d, tri, np.asarray(K, np.float32).reshape(9).copy(), truth)


def skipped(pair: Pair, status=16) -> Pair:
    q = pair.padded(pair.cap)
    q.init["status"] = status
    return q


def feed_back(pair: Pair, res, p3d_out) -> Pair:
    """The pair with a result as its input: a converged pose (steps below theta = 1e-5)."""
    q = pair.padded(pair.cap)
    q.init["R21"][0], q.init["t21"][0] = res["R21"], res["t21"]
    q.p3d = np.ascontiguousarray(p3d_out, np.float32).copy()
    return q


def init_scene(seed, n=500, n_iter=200):
    """Inputs for the device Initializer that it can accept: tests/oracle_lib.two_view_case -- points 4 to 20 units deep, a rotation
    of 2 to 8 degrees per axis, a unit baseline, 0.3 px of noise, a tenth of the keypoints unmatched -- as arrays of one capacity,
    and mvSets drawn with glibc's rand() seeded with `seed`.  About one seed in ten initialises (CheckRT's kept quirks make most
    scenes AMBIGUOUS); 3, 11 and 29 do.  -> (K [3, 3] f32, k1 [cap], n1, k2 [cap], n2, m12 [cap], sets [n_iter, 8])"""
    import ctypes as C
    import oracle_lib as O
    from orb_slam_tracking_amd import sample_sets
    K, _, _, a, b, m, _ = O.two_view_case(seed=seed, n=n, outliers=0.0, noise=0.3)
    cap = max(len(a), len(b))
    k1, k2, m12 = np.zeros(cap, KEYPOINT_DTYPE), np.zeros(cap, KEYPOINT_DTYPE), np.full(cap, -1, np.int32)
    k1[:len(a)], k2[:len(b)], m12[:len(a)] = a.astype(KEYPOINT_DTYPE), b.astype(KEYPOINT_DTYPE), m
    libc = C.CDLL("libc.so.6")
    libc.srand(int(seed))
    sets = sample_sets(int((m >= 0).sum()), n_iter, libc.rand)
    return K.astype(np.float32), k1, len(a), k2, len(b), m12, sets


def zero_table():
    return np.zeros(NLEVELS, np.float32)


def top_level_off_table():
    """The usual table with the weight of the last level set to 0: the table world("no_weight") is meant for."""
    t = inv_sigma2_table()
    t[NLEVELS - 1] = 0
    return t


def one_level_table(level=3):
    """Weight 1 at one level, 0 elsewhere."""
    t = zero_table()
    t[level] = 1
    return t


def inv_sigma2_of(setting_name: str):
    """The inv_sigma2 table of a setting's pyramid: None (the default table) for the first."""
    return None if setting_name == "first" else inv_sigma2_table(NLEVELS_2, SCALE_FACTOR_2)


# frame 2 rolled by 89 degrees against frame 1 (pose_ref_lib.ROLL), the baseline as in the first setting
MOTION_ROLL = (ROLL, (-0.3, 0.02, 0.05))
# the named pairs that exist under the second setting as well (world(name, "second")): smaller, with seeds of their own
SECOND_WORLDS = {"general": lambda: make_pair(120, 101, motion=MOTION_ROLL, **SECOND),
                 "huber": lambda: make_pair(110, 103, outliers=8, motion=MOTION_ROLL, **SECOND),
                 "few": lambda: make_pair(40, 105, motion=MOTION_ROLL, **SECOND),
                 "truth": lambda: make_pair(150, 111, noise=0.2, twist=(0.02, -0.015, 0.01, 0.05, -0.04, 0.03), motion=MOTION_ROLL, **SECOND)}
_worlds = {}


def world(name: str, setting_name: str = "first") -> Pair:
    """Named pairs, made once.  setting_name "second": the pair of that name in SECOND_WORLDS (K_ANISO, 5 levels of 1.37, frame 2
    rolled by 89 degrees), for the table inv_sigma2_of("second").

    general: converges; rejecting: the input translation 30 times too long and gross
    mismatches (rejected trials); huber:
    gross mismatches; converged: general's result fed back (the small-theta branch); mirrored: negative depths; few: 40 points; truth: little pixel noise, an input pose
    1.5 degrees and 11 degrees (translation direction) off; no_weight: general with every keypoint at the last level, for
    top_level_off_table() -- every edge weighs nothing, as under a table of zeros, in a call whose other pairs keep their weights
    (a call has one table)."""
    if setting_name != "first":
        if (name, setting_name) not in _worlds:
            _worlds[name, setting_name] = SECOND_WORLDS[name]()
        return _worlds[name, setting_name]
    if name not in _worlds:
        if name == "general":
            w = make_pair(300, 1)
        elif name == "rejecting":
            w = make_pair(120, 2, outliers=10, pose_scale=30.0)
        elif name == "huber":
            w = make_pair(200, 3, outliers=12)
        elif name == "converged":
            g = world("general")
            r, p, _ = bundle_adjust(g, 20, 100, False)
            w = feed_back(g, r, p)
        elif name == "mirrored":
            w = make_pair(150, 4, mirrored=True)
        elif name == "few":
            w = make_pair(40, 5)
        elif name == "truth":
            w = make_pair(300, 11, noise=0.2, twist=(0.02, -0.015, 0.01, 0.05, -0.04, 0.03))
        elif name == "no_weight":
            g = world("general")
            w = g.padded(g.cap)
            w.k1["octave"][:], w.k2["octave"][:] = NLEVELS - 1, NLEVELS - 1
        else:
            raise KeyError(name)
        _worlds[name] = w
    return _worlds[name]
