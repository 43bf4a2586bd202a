"""ctypes wrapper around tests/cpp/sim3opt_ref.cpp -- the CPU restatement of Optimizer::OptimizeSim3 (include/orbx.h, "loop
closing: Sim3 optimisation") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary directory, as
tests/sim3_ref_lib.py compiles its source; a second, independently written numpy statement (the similarity as a 4x4 matrix, its
exponential by the Taylor series of the generator, numerically differentiated residuals with a step of its own, Huber weights,
numpy.linalg.solve; nothing shared with the C++); and the worlds that tests/test_sim3opt_host.py and tests/test_gpu_sim3opt.py
share.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import pose_ref_lib as P
from pose_ref_lib import K_ANISO, MOTION_2, NLEVELS_2, ROLL, SCALE_FACTOR_2, SECOND, SETTINGS  # noqa: F401 (the second setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim3opt_ref.cpp")
MAIN_SRC = os.path.join(ROOT, "tests", "cpp", "sim3opt_ref_main.cpp")
KEYPOINT_DTYPE = P.KEYPOINT_DTYPE
SIM3OPT_RESULT_DTYPE = np.dtype(
    [(n, "<i4") for n in ("status", "n_correspondences", "n_bad", "n_inliers", "rounds")] + [("iterations", "<i4", 2)] +
    [(n, "<i4") for n in ("lm_trials", "rejected_trials", "solver_failures")] + [("stop_reason", "<i4", 2)] +
    [(n, "<i4") for n in ("small_theta", "small_sigma", "small_both", "reserved")] +
    [(n, "<f8") for n in ("chi2_initial", "chi2_final", "lambda")] + [("q", "<f8", 4), ("t", "<f8", 3), ("s", "<f8")] +
    [("s12", "<f4"), ("R12", "<f4", (3, 3)), ("t12", "<f4", 3), ("reserved_f", "<f4")])
assert SIM3OPT_RESULT_DTYPE.itemsize == 208
BAD_INPUT, NONFINITE = 2, 4
COUNTERS = ("accepted", "rejected", "huber_outliers", "ended_on_rejected", "fail12_only", "fail21_only", "fail_both", "unused")
NLEVELS = P.NLEVELS
K0 = P.K0
TH2 = 10.0  # LoopClosing passes 10
WAVE = 64
_L = None


def compile_command(out, extra=(), src=SRC):
    return ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", *extra, src, "-o", out]


def build(src=SRC) -> ctypes.CDLL:
    """Compiles a restatement source (lib(): the committed one; the camera mutant: an altered copy) and binds it."""
    d = tempfile.mkdtemp(prefix="sim3opt_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libsim3opt_ref.so")
    p = subprocess.run(compile_command(so, ("-fPIC", "-shared"), src), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("sim3opt_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, f32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    world = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.s3o_optimize.argtypes = world + [i32, f32, i32, i32, i32, vp, vp, vp]
    L.s3o_optimize.restype = None
    L.s3o_first_step.argtypes = world + [i32, f32, i32, vp, vp, vp, vp, vp, vp]
    L.s3o_exp.argtypes, L.s3o_exp.restype = [f64], f64
    L.s3o_sim3_exp.argtypes = [vp, vp]
    L.s3o_oplus.argtypes, L.s3o_oplus.restype = [vp, i32, vp], None
    L.s3o_huber_delta.argtypes, L.s3o_huber_delta.restype = [f32], f64
    L.s3o_exp_breakpoints.argtypes, L.s3o_exp_breakpoints.restype = [vp], None
    return L


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        _L = build()
    return _L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


# ---- worlds ----

class World:
    """One problem's inputs as rows of `cap` entries: the two keyframes (kps1, n1, points1, mask1, pose1 / ...2), the match row,
    the start similarity sim [13] (R12 row-major, t12, s12) and K, plus what is known about the scene."""

    def __init__(self, kps1, n1, kps2, n2, match, points1, mask1, points2, mask2, pose1, pose2, sim, K, truth=None):
        self.kps1, self.n1, self.kps2, self.n2, self.match = kps1, int(n1), kps2, int(n2), match
        self.points1, self.mask1, self.points2, self.mask2, self.pose1, self.pose2, self.sim, self.K, self.truth = \
            points1, mask1, points2, mask2, pose1, pose2, sim, K, truth
        self.cap = len(kps1)

    def copy(self):
        c = lambda a: None if a is None else a.copy()  # noqa: E731
        return World(self.kps1.copy(), self.n1, self.kps2.copy(), self.n2, self.match.copy(), self.points1.copy(), c(self.mask1),
                     self.points2.copy(), c(self.mask2), self.pose1.copy(), self.pose2.copy(), self.sim.copy(), self.K, self.truth)

    def edges(self, match=None):
        """(features i1, features i2) of the correspondences, ascending i1."""
        match = self.match if match is None else match
        i1 = np.arange(max(min(self.n1, self.cap), 0))
        i2 = match[:len(i1)].astype(np.int64)
        ok = (i2 >= 0) & (i2 < self.n2)
        if self.mask1 is not None:
            ok &= (self.mask1[i1] != 0) & (self.mask2[np.where(ok, i2, 0)] != 0)
        return i1[ok], i2[ok]


def sim_row(s, R, t):
    return np.r_[np.asarray(R, np.float64).reshape(9), t, s].astype(np.float32)


def make_world(n, seed=0, cap=None, noise=0.0, outliers=0, extra=5, s=1.3, rot=(0.05, -0.08, 0.03), t=(0.3, -0.2, 0.4),
               use_mask=True, nlevels=NLEVELS, K=K0, scale_factor=1.2, start=(1.5, 1.03, 1.04), on_axis=False):
    """Two keyframes with n correspondences.  The points lie 4 to 20 units in front of camera 2 (Y2); camera 1 sees them at Y1 =
    s R Y2 + t, the true similarity between the camera frames.  Each keyframe stores its points in a world frame of its own
    pose and has a keypoint at the point's projection plus pixel noise (`noise` in units of the keypoint's level sigma).
    `outliers` of the correspondences name the feature of another one (gross mismatches: a cyclic shift among them).  Each
    keyframe holds `extra` more features: without a point, with a point but no match, and matched to an entry that is no point.
    start = (degrees, factor of t, factor of s) by which the start similarity is off the truth (s is kept with s == 1: a
    fix_scale world); None: the truth rounded to f32.  on_axis: every point on both optical axes (R = I, t along z)."""
    rng = np.random.default_rng(35000 + seed)
    Rt, tt, st = P.rotvec(rot), np.array(t, np.float64), float(s)
    Kd = np.asarray(K, np.float64).reshape(3, 3)
    z = rng.uniform(4, 20, n)
    Y2 = np.c_[rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.3, 0.3, n) * z, z]
    if on_axis:
        Rt, tt = np.eye(3), np.array([0.0, 0.0, float(t[2])])
        Y2 = np.c_[np.zeros(n), np.zeros(n), z]
    Y1 = st * Y2 @ Rt.T + tt
    oct1, oct2 = rng.integers(0, nlevels, n), rng.integers(0, nlevels, n)
    R1, t1 = P.rotvec((0.2, -0.1, 0.05)), np.array([0.5, -1.0, 2.0])
    R2, t2 = P.rotvec((-0.1, 0.3, 0.1)), np.array([-1.5, 0.4, 1.0])
    X1w, X2w = (Y1 - t1) @ R1, (Y2 - t2) @ R2
    nf = n + extra if n else 0
    cap = int(cap or max(nf, 1))
    assert cap >= nf
    kps1, kps2 = np.zeros(cap, KEYPOINT_DTYPE), np.zeros(cap, KEYPOINT_DTYPE)
    for k in (kps1, kps2):
        k["x"][:nf], k["y"][:nf], k["octave"][:nf] = rng.uniform(0, 640, nf), rng.uniform(0, 480, nf), rng.integers(0, nlevels, nf)
    slots1 = np.sort(rng.permutation(nf)[:n]) if n else np.zeros(0, np.int64)
    slots2 = rng.permutation(nf)[:n] if n else np.zeros(0, np.int64)
    proj = lambda Y: np.c_[Y[:, 0] / Y[:, 2] * Kd[0, 0] + Kd[0, 2], Y[:, 1] / Y[:, 2] * Kd[1, 1] + Kd[1, 2]]  # noqa: E731
    if n:
        uv1 = proj(Y1) + rng.normal(0, 1, (n, 2)) * noise * (scale_factor ** oct1)[:, None]
        uv2 = proj(Y2) + rng.normal(0, 1, (n, 2)) * noise * (scale_factor ** oct2)[:, None]
        kps1["x"][slots1], kps1["y"][slots1], kps1["octave"][slots1] = uv1[:, 0], uv1[:, 1], oct1
        kps2["x"][slots2], kps2["y"][slots2], kps2["octave"][slots2] = uv2[:, 0], uv2[:, 1], oct2
    points1 = rng.normal(0, 1, (cap, 3)).astype(np.float32)  # (entries that are no point hold leftovers)
    points2 = rng.normal(0, 1, (cap, 3)).astype(np.float32)
    mask1, mask2 = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    match = np.full(cap, -1, np.int32)
    match[slots1] = slots2
    bad = np.sort(rng.choice(n, outliers, replace=False)) if outliers else np.zeros(0, np.int64)
    if len(bad):
        assert len(bad) >= 2
        match[slots1[bad]] = slots2[np.roll(bad, 1)]
    points1[slots1], points2[slots2] = X1w, X2w
    mask1[slots1], mask2[slots2] = 1, 1
    free1, free2 = np.setdiff1d(np.arange(nf), slots1), np.setdiff1d(np.arange(nf), slots2)
    if use_mask and len(free1) >= 3 and len(free2) >= 2:
        match[free1[0]] = free2[0]                       # matched, neither side a point
        match[free1[1]], mask1[free1[1]] = free2[1], 1   # a point of KF1 matched to an entry of KF2 that is no point
        mask1[free1[2]] = 1                              # a point of KF1 without a match
    if not use_mask:
        assert extra == 0
        mask1 = mask2 = None
    pose1, pose2 = np.r_[R1.reshape(9), t1].astype(np.float32), np.r_[R2.reshape(9), t2].astype(np.float32)
    if start is None:
        sim = sim_row(st, Rt, tt)
    else:
        axis = rng.normal(0, 1, 3)
        dR = P.rotvec(axis / np.linalg.norm(axis) * np.radians(start[0]))
        sim = sim_row(st * start[2] if st != 1.0 else 1.0, dR @ Rt, (dR @ tt) * start[1])
    clean = np.setdiff1d(np.arange(n), bad)
    truth = dict(s=st, R=Rt, t=tt, slots1=slots1, slots2=slots2, bad=slots1[bad], clean=slots1[clean])
    return World(kps1, nf, kps2, nf, match, points1, mask1, points2, mask2, pose1, pose2, sim,
                 np.asarray(K, np.float32).reshape(9).copy(), truth)


def inv_sigma2_of(setting_name: str):
    return P.inv_sigma2_of(setting_name)


def nlevels_of(setting_name: str):
    return NLEVELS if setting_name == "first" else NLEVELS_2


_worlds = {}
# name -> (arguments of make_world under the first setting, under the second).  "@2" names the second: K_ANISO, 5 levels of
# 1.37 and the 89-degree roll.
_SECOND = dict(rot=ROLL, t=MOTION_2[1], **SECOND)
WORLDS = {
    "clean": dict(n=200, seed=1, noise=0.3, outliers=20),            # both rounds, the 10-iteration branch
    "nobad": dict(n=120, seed=2, noise=0.05),                         # nBad == 0: 5 more iterations
    "truth13": dict(n=150, seed=3, s=1.3),                            # noise-free, scale 1.3
    "truth06": dict(n=150, seed=4, s=0.6),                            # noise-free, scale 0.6
    "fixed": dict(n=150, seed=5, s=1.0),                              # for fix_scale = 1
    "far": dict(n=160, seed=6, noise=0.4, outliers=40, start=(6.0, 1.15, 1.2)),  # rejected trials
    "noisy": dict(n=180, seed=7, noise=0.8, outliers=18, start=(3.0, 1.05, 1.08)),
    "mixed": dict(n=300, seed=8, noise=0.3, outliers=30),
    "big": dict(n=640, seed=9, noise=0.3, outliers=64, cap=1024),     # lanes walk ten entries and more
    "nomask": dict(n=90, seed=10, noise=0.3, outliers=9, extra=0, use_mask=False),
    "axis": dict(n=40, seed=11, on_axis=True, start=None, extra=0),   # H is singular: failed 7x7 solves
}


def world(name: str) -> World:
    """Named worlds, made once; "name@2" is the world of that name under the second setting."""
    if name not in _worlds:
        base, second = name.split("@")[0], name.endswith("@2")
        kw = dict(WORLDS[base])
        if second:
            kw.update(_SECOND, seed=kw["seed"] + 100)
        n = kw.pop("n")
        _worlds[name] = make_world(n, **kw)
    return _worlds[name]


def setting_of(name: str) -> str:
    return "second" if name.endswith("@2") else "first"


def sized_world(n, seed, setting_name="first", **kw):
    """A world of exactly n correspondences with a tenth of them mismatched (none below 20), for the lane and wave edges."""
    args = dict(noise=0.3, outliers=(n // 10 if n >= 20 else 0))
    args.update(kw)
    if setting_name != "first":
        args.update(_SECOND)
    return make_world(n, seed, **args)


# ---- the restatement ----

def _world_args(w: World, row, sig):
    return (_p(w.kps1), w.n1, _p(w.kps2), w.n2, w.cap, _p(row), _p(w.points1), _p(w.mask1), _p(w.points2), _p(w.mask2),
            _p(w.pose1), _p(w.pose2), _p(w.K), _p(sig), len(sig), _p(w.sim))


def _sig(inv_sigma2, nlevels):
    return np.ascontiguousarray(P.inv_sigma2_table(nlevels) if inv_sigma2 is None else inv_sigma2, np.float32)


def optimize(w: World, inv_sigma2=None, nlevels=NLEVELS, fix_scale=0, th2=TH2, n_iterations=5, n_more_iterations=10, per_edge=0):
    """The restatement for one problem -> (SIM3OPT_RESULT_DTYPE record, sim_out [13] f32, row [cap] i32, {counter: value}).
    per_edge: the fourteen perturbed estimates computed again for every edge, as g2o does."""
    sig = _sig(inv_sigma2, nlevels)
    res, sim, row = np.zeros(1, SIM3OPT_RESULT_DTYPE), np.zeros(13, np.float32), w.match.copy()
    cnt = np.zeros(len(COUNTERS), np.int64)
    lib().s3o_optimize(*_world_args(w, row, sig), int(fix_scale), np.float32(th2), int(n_iterations), int(n_more_iterations),
                       int(per_edge), _p(res), _p(sim), _p(cnt))
    return res[0].copy(), sim, row, dict(zip(COUNTERS, (int(c) for c in cnt)))


def optimize_named(name, **kw):
    s = setting_of(name)
    return optimize(world(name), inv_sigma2=inv_sigma2_of(s), nlevels=nlevels_of(s), **kw)


def first_step(w: World, inv_sigma2=None, nlevels=NLEVELS, fix_scale=0, th2=TH2, per_edge=0, L=None):
    """The restatement's first trial step -> dict(q, t, s, lam, chi2_initial, H [7, 7], b [7], x [7], n) or None."""
    sig = _sig(inv_sigma2, nlevels)
    sim8, lam, chi2, H, b, x = np.zeros(8), np.zeros(1), np.zeros(1), np.zeros((7, 7)), np.zeros(7), np.zeros(7)
    row = w.match.copy()
    n = (L or lib()).s3o_first_step(*_world_args(w, row, sig), int(fix_scale), np.float32(th2), int(per_edge), _p(sim8),
                                    _p(lam), _p(chi2), _p(H), _p(b), _p(x))
    if n < 0:
        return None
    return dict(q=sim8[:4].copy(), t=sim8[4:7].copy(), s=float(sim8[7]), lam=float(lam[0]), chi2_initial=float(chi2[0]), H=H, b=b,
                x=x, n=n)


def exp(x: float) -> float:
    return float(lib().s3o_exp(float(x)))


def exp_breakpoints():
    out = np.zeros(4)
    lib().s3o_exp_breakpoints(_p(out))
    return [float(v) for v in out]


def sim3_exp(update):
    """Sim3(update) of the restatement -> (q [4], t [3], s, branch bits: 1 = theta < 1e-5, 2 = |sigma| < 1e-5)."""
    u, out = np.ascontiguousarray(update, np.float64), np.zeros(8)
    br = lib().s3o_sim3_exp(_p(u), _p(out))
    return out[:4].copy(), out[4:7].copy(), float(out[7]), int(br)


def oplus(update, est8, fix_scale=0):
    u, e = np.ascontiguousarray(update, np.float64), np.ascontiguousarray(est8, np.float64).copy()
    lib().s3o_oplus(_p(u), int(fix_scale), _p(e))
    return e


# ---- the second statement: numpy f64, 4x4 matrices, numerical derivatives, one dense solve; nothing shared with the C++ ----

def generator(u):
    """The 4x4 generator of the similarity group for update = (omega, upsilon, sigma)."""
    w, v, sg = np.asarray(u[:3], np.float64), np.asarray(u[3:6], np.float64), float(u[6])
    G = np.zeros((4, 4))
    G[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + sg * np.eye(3)
    G[:3, 3] = v
    return G


def expm_taylor(G, terms=60):
    """exp of a small 4x4 matrix by scaling, its Taylor series and squaring."""
    k = max(0, int(np.ceil(np.log2(max(np.abs(G).sum(1).max(), 1e-300)))) + 4)
    A, out, term = G / 2.0 ** k, np.eye(4), np.eye(4)
    for i in range(1, terms):
        term = term @ A / i
        out = out + term
    for _ in range(k):
        out = out @ out
    return out


def sim_matrix(s, R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * np.asarray(R, np.float64), t
    return M


def quat_matrix_raw(q):
    """Quaterniond::toRotationMatrix of a quaternion as it is (x, y, z, w)."""
    return P.quat_to_matrix(q)


def rotate_raw(q, X):
    """Eigen's q * v for a quaternion that may not be a unit one, on rows of X: v + 2 w (u x v) + 2 u x (u x v)."""
    u, w = np.asarray(q[:3], np.float64), float(q[3])
    uv = np.cross(u, X)
    return X + 2 * w * uv + 2 * np.cross(u, uv)


def graph(w: World, inv_sigma2=None, nlevels=NLEVELS, match=None):
    """The graph as plain f64 arrays: dict(i1, i2, P1c, P2c, obs1, obs2, w1, w2, K) with the camera-frame points taken in f64 from
    the f32 inputs."""
    sig = (P.inv_sigma2_table(nlevels) if inv_sigma2 is None else np.asarray(inv_sigma2, np.float32)).astype(np.float64)
    i1, i2 = w.edges(match)
    T1, T2 = w.pose1.astype(np.float64), w.pose2.astype(np.float64)
    k1, k2 = w.kps1[i1], w.kps2[i2]
    return dict(i1=i1, i2=i2, P1c=w.points1[i1].astype(np.float64) @ T1[:9].reshape(3, 3).T + T1[9:],
                P2c=w.points2[i2].astype(np.float64) @ T2[:9].reshape(3, 3).T + T2[9:],
                obs1=np.c_[k1["x"], k1["y"]].astype(np.float64), obs2=np.c_[k2["x"], k2["y"]].astype(np.float64),
                w1=sig[k1["octave"]], w2=sig[k2["octave"]], K=w.K.reshape(3, 3).astype(np.float64))


def _project(K, Y):
    return np.c_[K[0, 0] * Y[:, 0] / Y[:, 2] + K[0, 2], K[1, 1] * Y[:, 1] / Y[:, 2] + K[1, 2]]


def residuals_numpy(M, g):
    """(e12 [n, 2], e21 [n, 2]) under the 4x4 similarity M (camera 2 -> camera 1)."""
    Mi = np.linalg.inv(M)
    return (g["obs1"] - _project(g["K"], g["P2c"] @ M[:3, :3].T + M[:3, 3]),
            g["obs2"] - _project(g["K"], g["P1c"] @ Mi[:3, :3].T + Mi[:3, 3]))


def chi2_numpy(M, g):
    e12, e21 = residuals_numpy(M, g)
    return g["w1"] * (e12 ** 2).sum(1), g["w2"] * (e21 ** 2).sum(1)


def first_step_numpy(w: World, inv_sigma2=None, nlevels=NLEVELS, fix_scale=0, th2=TH2, h=1e-6):
    """The first damped step -> dict(lam, chi2_initial, x [7]): central differences with this statement's own h, its own Huber
    weights, numpy.linalg.solve.  The start is the f32 row read as a matrix."""
    g = graph(w, inv_sigma2, nlevels)
    sim = w.sim.astype(np.float64)
    M0 = sim_matrix(sim[12], sim[:9].reshape(3, 3), sim[9:12])
    delta = float(np.float32(np.sqrt(np.float64(np.float32(th2)))))
    dof = 6 if fix_scale else 7

    def res(u):
        e12, e21 = residuals_numpy(expm_taylor(generator(u)) @ M0, g)
        return np.c_[e12, e21].reshape(-1)  # per correspondence: e12 (2), e21 (2)

    c12, c21 = chi2_numpy(M0, g)
    c = np.c_[c12, c21].reshape(-1)
    out = c > delta * delta
    root = np.sqrt(np.where(out, c, 1.0))
    chi2 = float(np.where(out, 2 * root * delta - delta * delta, c).sum())
    rho1 = np.where(out, delta / root, 1.0)
    W = np.repeat(rho1 * np.c_[g["w1"], g["w2"]].reshape(-1), 2)
    J = np.zeros((len(W), 7))
    for k in range(dof):
        u = np.zeros(7)
        u[k] = h
        J[:, k] = (res(u) - res(-u)) / (2 * h)
    H, b = J.T @ (W[:, None] * J), -J.T @ (W * res(np.zeros(7)))
    lam = 1e-5 * float(np.abs(np.diag(H)).max())
    x = np.zeros(7)
    x[:dof] = np.linalg.solve((H + lam * np.eye(7))[:dof, :dof], b[:dof])
    return dict(lam=lam, chi2_initial=chi2, x=x, H=H, b=b)


def sim_difference(s1, R1, t1, s2, R2, t2):
    """(rotation angle in radians as |R1 - R2|_F / sqrt(2), |s1 / s2 - 1|, |t1 - t2|)."""
    return (float(np.linalg.norm(np.asarray(R1, np.float64) - R2) / np.sqrt(2)), abs(float(s1) / float(s2) - 1.0),
            float(np.linalg.norm(np.asarray(t1, np.float64) - t2)))
