"""ctypes wrapper around tests/cpp/pose_ref.cpp -- the CPU restatement of Optimizer::PoseOptimization (include/orbx.h, "behind
SearchByBoW: pose optimisation") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary directory, as
tests/ba_ref_lib.py compiles its source; a second, independently written numpy statement (numerically differentiated residuals,
the damped 6x6 normal equations, numpy.linalg.solve, and a Gauss-Newton run to convergence); and the worlds (a frame seen from a
true pose, fixed map points, gross mismatches, a start pose that is off) that tests/test_pose_host.py and tests/test_gpu_pose.py
share.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pose_ref.cpp")
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
POSE_RESULT_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_correspondences", "n_bad", "n_inliers", "rounds")] +
                             [("iterations", "<i4", 4)] + [(n, "<i4") for n in ("lm_trials", "rejected_trials", "solver_failures")] +
                             [("stop_reason", "<i4", 4)] + [(n, "<f8") for n in ("chi2_initial", "chi2_final", "lambda")] +
                             [("q", "<f8", 4), ("t", "<f8", 3), ("R", "<f4", (3, 3)), ("tcw", "<f4", 3)])
assert POSE_RESULT_DTYPE.itemsize == 192
BAD_INPUT, NONFINITE, FEW_POINTS = 2, 4, 8
COUNTERS = ("accepted", "rejected", "huber_outliers", "small_theta", "ended_on_rejected", "stale_differs")
NLEVELS = 8
_L = None


def build(src=SRC) -> ctypes.CDLL:
    """Compiles a restatement source (lib(): the committed one; tests/test_camera_mutants_host.py: an altered copy) and binds it."""
    d = tempfile.mkdtemp(prefix="pose_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libpose_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", src, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("pose_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.por_pose_optimize.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    L.por_pose_optimize.restype = None
    L.por_first_step.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.por_huber_delta.restype = ctypes.c_double
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


class World:
    """One problem's inputs as rows of `cap` entries (kps, n, match or None, points, mask or None, pose0 [12], K [9]) plus what
    is known about the scene."""

    def __init__(self, kps, n, match, points, mask, pose0, K, truth=None):
        self.kps, self.n, self.match, self.points, self.mask, self.pose0, self.K, self.truth = \
            kps, int(n), match, points, mask, pose0, K, truth
        self.cap = len(kps)

    def copy(self):
        c = lambda a: None if a is None else a.copy()  # noqa: E731
        return World(self.kps.copy(), self.n, c(self.match), self.points.copy(), c(self.mask), self.pose0.copy(), self.K, self.truth)

    def padded(self, cap):
        """The same problem in rows of a larger capacity."""
        def grow(a, fill=0):
            if a is None:
                return None
            out = np.zeros(cap, a.dtype) if a.dtype == KEYPOINT_DTYPE else np.full((cap,) + a.shape[1:], fill, a.dtype)
            out[:len(a)] = a
            return out
        mask = self.mask
        if mask is None and cap > self.cap:  # (entries beyond the old capacity are no points)
            mask = np.ones(self.cap, np.uint8)
        return World(grow(self.kps), self.n, grow(self.match, -1), grow(self.points), grow(mask), self.pose0.copy(), self.K, self.truth)

    def edges(self):
        """(features j, their points' indices i) of the graph, ascending j."""
        j = np.arange(self.n)
        i = j.copy() if self.match is None else self.match[:self.n].astype(np.int64)
        ok = i >= 0
        if self.mask is not None:
            ok &= self.mask[np.where(ok, i, 0)] != 0
        return j[ok], i[ok]


def pose_optimize(w: World, n_iterations=10, inv_sigma2=None, nlevels=NLEVELS):
    """The restatement for one problem -> (POSE_RESULT_DTYPE record, flags [cap] uint8, flags behind each round [4, cap],
    {counter: value})."""
    sig = np.ascontiguousarray(inv_sigma2_table(nlevels) if inv_sigma2 is None else inv_sigma2, np.float32)
    out, flags, rounds = np.zeros(1, POSE_RESULT_DTYPE), np.zeros(w.cap, np.uint8), np.zeros((4, w.cap), np.uint8)
    cnt = np.zeros(len(COUNTERS), np.int64)
    lib().por_pose_optimize(_p(w.kps), w.n, w.cap, _p(w.match), _p(w.points), _p(w.mask), _p(w.pose0), _p(w.K), _p(sig), len(sig),
                            int(n_iterations), _p(out), _p(flags), _p(rounds), _p(cnt))
    return out[0].copy(), flags, rounds, dict(zip(COUNTERS, (int(c) for c in cnt)))


def first_step(w: World, inv_sigma2=None, nlevels=NLEVELS):
    """The restatement's first trial step of round 0 -> dict(q, t, lam, chi2_initial, xp [6]) or None."""
    sig = np.ascontiguousarray(inv_sigma2_table(nlevels) if inv_sigma2 is None else inv_sigma2, np.float32)
    pose, lam, chi2, xp = np.zeros(7), np.zeros(1), np.zeros(1), np.zeros(6)
    n = lib().por_first_step(_p(w.kps), w.n, w.cap, _p(w.match), _p(w.points), _p(w.mask), _p(w.pose0), _p(w.K), _p(sig), len(sig),
                             _p(pose), _p(lam), _p(chi2), _p(xp))
    if n < 0:
        return None
    return dict(q=pose[:4].copy(), t=pose[4:].copy(), lam=float(lam[0]), chi2_initial=float(chi2[0]), xp=xp, n=n)


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


def rotvec(w):
    return se3_exp(np.r_[np.asarray(w, np.float64), 0, 0, 0])[0]


def graph(w: World, inv_sigma2=None, nlevels=NLEVELS):
    """The graph as plain f64 arrays: (features j, X [n, 3], obs [n, 2], weights [n], R, t, K)."""
    sig = (inv_sigma2_table(nlevels) if inv_sigma2 is None else np.asarray(inv_sigma2, np.float32)).astype(np.float64)
    j, i = w.edges()
    k = w.kps[j]
    return (j, w.points[i].astype(np.float64), np.c_[k["x"], k["y"]].astype(np.float64), sig[k["octave"]],
            w.pose0[:9].reshape(3, 3).astype(np.float64), w.pose0[9:].astype(np.float64), w.K.reshape(3, 3).astype(np.float64))


def residuals(R, t, X, obs, K):
    Y = X @ R.T + t
    return obs - np.c_[Y[:, 0] / Y[:, 2] * K[0, 0] + K[0, 2], Y[:, 1] / Y[:, 2] * K[1, 1] + K[1, 2]]


def plain_chi2(R, t, X, obs, wt, K):
    return wt * (residuals(R, t, X, obs, K) ** 2).sum(axis=1)


def _normal_equations(R, t, X, obs, wt, K, delta, h=1e-6):
    """chi2 (Huber's rho summed; delta None = plain), H and b of the 6-dof system by central differences."""
    def res(u):
        dR, dt = se3_exp(u)
        return residuals(dR @ R, dR @ t + dt, X, obs, K).reshape(-1)
    c = plain_chi2(R, t, X, obs, wt, K)
    if delta is None:
        chi2, rho1 = float(c.sum()), np.ones_like(c)
    else:
        out = c > delta * delta
        root = np.sqrt(np.where(out, c, 1.0))
        chi2 = float(np.where(out, 2 * root * delta - delta * delta, c).sum())
        rho1 = np.where(out, delta / root, 1.0)
    W = np.repeat(rho1 * wt, 2)
    J = np.zeros((2 * len(X), 6))
    for k in range(6):
        u = np.zeros(6)
        u[k] = h
        J[:, k] = (res(u) - res(-u)) / (2 * h)
    return chi2, J.T @ (W[:, None] * J), -J.T @ (W * res(np.zeros(6)))


def first_step_numpy(w: World, inv_sigma2=None, nlevels=NLEVELS):
    """The first damped step of round 0 -> dict(lam, chi2_initial, xp)."""
    _, X, obs, wt, R, t, K = graph(w, inv_sigma2, nlevels)
    chi2, H, b = _normal_equations(R, t, X, obs, wt, K, float(np.float32(np.sqrt(5.991))))
    lam = 1e-5 * float(np.abs(np.diag(H)).max())
    return dict(lam=lam, chi2_initial=chi2, xp=np.linalg.solve(H + lam * np.eye(6), b))


def gauss_newton_numpy(w: World, keep, inv_sigma2=None, nlevels=NLEVELS, steps=30):
    """Undamped Gauss-Newton without a robust kernel over the features `keep` (bool per feature of the frame), from the world's
    start pose (its f32 rotation made orthonormal by an SVD), until the step is below 1e-13 -> (R, t)."""
    j, X, obs, wt, R, t, K = graph(w, inv_sigma2, nlevels)
    U, _, Vt = np.linalg.svd(R)
    R = U @ Vt
    sel = keep[j]
    X, obs, wt = X[sel], obs[sel], wt[sel]
    for _ in range(steps):
        _, H, b = _normal_equations(R, t, X, obs, wt, K, None)
        x = np.linalg.solve(H, b)
        dR, dt = se3_exp(x)
        R, t = dR @ R, dR @ t + dt
        if np.abs(x).max() < 1e-13:
            break
    return R, t


def quat_to_matrix(q):
    x, y, z, s = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s)],
                     [2 * (x * y + z * s), 1 - 2 * (x * x + z * z), 2 * (y * z - x * s)],
                     [2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)]], np.float64)


# ---- the worlds the host and the GPU test share ----

K0 = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1]], np.float32)
SCALE_FACTOR = 1.2

# The second setting of the back-end worlds (this library's and those of ba_, pnp_, sim3_, tri_, match_proj_, match_local_ and
# match_kfproj_ref_lib, which import it).  Under the first one -- fx == fy, a pyramid of 8 levels of 1.2, motions of a few degrees
# -- a v-projection that reads fx, a table length or a scale factor taken from a constant, and an x row written where a y row
# belongs all leave every comparison unchanged.  K_ANISO: focal lengths a third apart and a principal point off the centre, all
# four exact in f32.  The pyramid: 5 levels of 1.37, as the front-end tests use.  The motion: a roll of 89 degrees about the
# optical axis with some 3 degrees about the other two (a rotation vector), so that the camera's x and y axes change roles.
K_ANISO = np.array([[517.25, 0, 318.75], [0, 388.5, 255.5], [0, 0, 1]], np.float32)
SCALE_FACTOR_2, NLEVELS_2 = 1.37, 5
ROLL = (0.06, -0.05, 1.55)
MOTION_2 = (ROLL, (0.4, -0.1, 0.3))
SECOND = dict(K=K_ANISO, scale_factor=SCALE_FACTOR_2, nlevels=NLEVELS_2)
SETTINGS = ("first", "second")


def make_world(n, seed=0, cap=None, noise=0.5, outliers=0, angle_deg=2.0, scale=1.05, extra=5, matched=False, use_mask=True,
               nlevels=NLEVELS, motion=((0.03, -0.06, 0.02), (0.4, -0.1, 0.3)), identity_start=False, K=K0,
               scale_factor=SCALE_FACTOR):
    """A frame of n correspondences: map points 4 to 20 units deep seen from the true pose (R, t) = motion, pixel noise (in units
    of the keypoint's level sigma), mixed octaves, `outliers` gross mismatches more than 20 px off, and a start pose `angle_deg`
    off in rotation with its translation multiplied by `scale`.  The frame holds `extra` more features without a map point in
    between.  matched: the points sit in a permuted point set of their own (with `extra` unused entries) and the frame's
    features name them through a match row, the layout of SearchByBoW's output; otherwise feature j's point is entry j.
    identity_start: the start pose is the identity rotation with the true translation."""
    rng = np.random.default_rng(5000 + seed)
    Rt, tt = rotvec(motion[0]), np.array(motion[1], np.float64)
    Kd = np.asarray(K, np.float64).reshape(3, 3)
    z = rng.uniform(4, 20, n)
    Y = np.c_[rng.uniform(-0.55, 0.55, n) * z, rng.uniform(-0.4, 0.4, n) * z, z]  # in the camera's frame, inside the image
    X = (Y - tt) @ Rt  # Rt^T (Y - t)
    octs = rng.integers(0, nlevels, n)
    obs = np.c_[Y[:, 0] / Y[:, 2] * Kd[0, 0] + Kd[0, 2], Y[:, 1] / Y[:, 2] * Kd[1, 1] + Kd[1, 2]]
    obs = obs + rng.normal(0, 1, (n, 2)) * noise * (scale_factor ** octs)[:, None]
    bad = np.sort(rng.choice(n, outliers, replace=False)) if outliers else np.zeros(0, np.int64)
    obs[bad] += rng.choice([-1.0, 1.0], (len(bad), 2)) * rng.uniform(20, 40, (len(bad), 2)) * (scale_factor ** octs[bad])[:, None]
    nf = n + extra if n else 0
    cap = int(cap or max(nf, 1))
    assert cap >= nf
    kps = np.zeros(cap, KEYPOINT_DTYPE)
    slots = np.sort(rng.permutation(nf)[:n]) if n else np.zeros(0, np.int64)  # where the n correspondences sit in the frame
    kps["x"][:nf], kps["y"][:nf], kps["octave"][:nf] = rng.uniform(0, 640, nf), rng.uniform(0, 480, nf), rng.integers(0, nlevels, nf)
    kps["x"][slots], kps["y"][slots], kps["octave"][slots] = obs[:, 0], obs[:, 1], octs
    points = rng.normal(0, 1, (cap, 3)).astype(np.float32)  # (entries that are no point hold leftovers)
    mask = np.zeros(cap, np.uint8)
    match = None
    if matched:
        where = rng.permutation(nf)[:n] if n else np.zeros(0, np.int64)
        match = np.full(cap, -1, np.int32)
        match[slots] = where
        free = np.setdiff1d(np.arange(nf), where)
        others = np.setdiff1d(np.arange(nf), slots)
        if len(free) and len(others):  # a feature matched to an entry that is no map point
            match[others[0]] = free[0]
    else:
        where = slots
    points[where] = X
    mask[where] = 1
    if not use_mask:
        assert not matched and extra == 0
        mask = None
    if identity_start:
        R0, t0 = np.eye(3), tt
    else:
        axis = rng.normal(0, 1, 3)
        dR = rotvec(axis / np.linalg.norm(axis) * np.radians(angle_deg))
        R0, t0 = dR @ Rt, (dR @ tt) * scale
    pose0 = np.r_[R0.reshape(9), t0].astype(np.float32)
    truth = dict(R=Rt, t=tt, slots=slots, bad=slots[bad], clean=np.setdiff1d(slots, slots[bad]))
    return World(kps, nf, match, points, mask, pose0, np.asarray(K, np.float32).reshape(9).copy(), truth)


def feed_back(w: World, res) -> World:
    """The world with a result as its start pose: a start at the optimum (steps below theta = 1e-5, trials that cannot improve)."""
    q = w.copy()
    q.pose0 = np.r_[res["R"].reshape(9), res["tcw"]].astype(np.float32)
    return q


WAVE, LANE_CACHE = 64, 6  # k_pose: feature j is lane j % 64's, and a lane keeps its first six edges in LDS
BIG_CAP = 1024            # the capacity of the worlds that leave that cache


def lane_layout(w: World):
    """From the edges alone: (features of the edges behind their lane's cache [ascending], edges per lane [64], lanes with a
    feature without an edge in front of their sixth edge, lanes with one behind their seventh edge)."""
    j, _ = w.edges()
    behind, per_lane, hole_front, hole_behind = [], np.zeros(WAVE, np.int64), [], []
    for lane in range(WAVE):
        mine = j[j % WAVE == lane]
        per_lane[lane] = len(mine)
        behind.extend(mine[LANE_CACHE:])
        holes = np.setdiff1d(np.arange(lane, w.n, WAVE), mine)
        if len(mine) >= LANE_CACHE and (holes < mine[LANE_CACHE - 1]).any():
            hole_front.append(lane)
        if len(mine) > LANE_CACHE and (holes > mine[LANE_CACHE]).any():
            hole_behind.append(lane)
    return np.sort(np.array(behind, np.int64)), per_lane, hole_front, hole_behind


def scattered(dense: World, at, nf, seed, cap=BIG_CAP, dead=()):
    """A dense world (make_world(..., extra=0): feature j's point is entry j) as a match-row world of nf features: edge k sits
    on feature at[k] (ascending) and names a permuted entry of a masked point set; the features `dead` are matched to entries
    with mask == 0; every other feature has match -1."""
    rng = np.random.default_rng(7000 + seed)
    at, dead = np.asarray(at, np.int64), np.asarray(dead, np.int64)
    m = len(at)
    assert dense.match is None and dense.n == m and (np.diff(at) > 0).all() and at[-1] < nf <= cap and not np.intersect1d(at, dead).size
    kps = np.zeros(cap, KEYPOINT_DTYPE)
    kps["x"][:nf], kps["y"][:nf], kps["octave"][:nf] = rng.uniform(0, 640, nf), rng.uniform(0, 480, nf), rng.integers(0, NLEVELS, nf)
    kps[at] = dense.kps[:m]
    entries = rng.permutation(cap)
    where, off = entries[:m], entries[m:m + len(dead)]
    points = rng.normal(0, 1, (cap, 3)).astype(np.float32)  # (entries that are no point hold leftovers)
    points[where] = dense.points[:m]
    mask = np.zeros(cap, np.uint8)
    mask[where] = 1
    match = np.full(cap, -1, np.int32)
    match[at], match[dead] = where, off
    t = dense.truth
    truth = dict(R=t["R"], t=t["t"], slots=at, bad=at[t["bad"]], clean=at[t["clean"]])
    return World(kps, nf, match, points, mask, dense.pose0.copy(), dense.K, truth)


def weight_lost_world(n_gross, n_exact, seed, cap=None):
    """n_gross correspondences at octave 0 that are all gross mismatches (20 to 40 px off in both coordinates) and n_exact
    without noise at octave 1, for the table level0_table(): 1 at level 0 and 0 elsewhere.  Round 0 optimises over the weighted
    edges and flags them; the exact edges weigh nothing, so their chi2 is 0 and they stay active for ever.  From the round in
    which no weighted edge is active any more Hpp = 0, lambda re-initialises to 1e-5 * 0 = 0 and every 6x6 solve fails at its
    first pivot."""
    n = n_gross + n_exact
    w = make_world(n, seed, cap=cap, noise=0.0)
    rng = np.random.default_rng(9000 + seed)
    slots = w.truth["slots"]
    gross = np.sort(rng.choice(n, n_gross, replace=False))
    w.kps["octave"][slots] = 1
    w.kps["octave"][slots[gross]] = 0
    off = rng.choice([-1.0, 1.0], (n_gross, 2)) * rng.uniform(20, 40, (n_gross, 2))
    w.kps["x"][slots[gross]] += off[:, 0].astype(np.float32)
    w.kps["y"][slots[gross]] += off[:, 1].astype(np.float32)
    w.truth = dict(w.truth, bad=slots[gross], clean=np.setdiff1d(slots, slots[gross]))
    return w


def zero_table():
    return np.zeros(NLEVELS, np.float32)


def level0_table():
    t = np.zeros(NLEVELS, np.float32)
    t[0] = 1
    return t


# the inv_sigma2 table a named world is meant for (every other world: the default table)
TABLES = {"no_weight": zero_table, "no_weight_big": zero_table, "weight_lost": level0_table, "weight_lost_big": level0_table}


def table_of(name):
    return TABLES[name]() if name in TABLES else None


def inv_sigma2_of(setting_name: str):
    """The inv_sigma2 table of a setting's pyramid: None (the default table) for the first."""
    return None if setting_name == "first" else inv_sigma2_table(NLEVELS_2, SCALE_FACTOR_2)


# the named worlds that exist under the second setting as well (world(name, "second")): smaller, with seeds of their own
SECOND_WORLDS = {"clean": lambda: make_world(100, 101, outliers=10, motion=MOTION_2, **SECOND),
                 "matched": lambda: make_world(80, 102, outliers=8, matched=True, motion=MOTION_2, **SECOND),
                 "far": lambda: make_world(90, 103, outliers=30, angle_deg=25.0, scale=1.6, motion=MOTION_2, **SECOND),
                 "noisy": lambda: make_world(120, 104, outliers=20, noise=1.2, angle_deg=4.0, motion=MOTION_2, **SECOND),
                 "truth": lambda: make_world(150, 108, noise=0.2, outliers=15, motion=MOTION_2, **SECOND)}
_worlds = {}


def world(name: str, setting_name: str = "first") -> World:
    """Named worlds, made once.  setting_name "second": the world of that name in SECOND_WORLDS (K_ANISO, 5 levels of 1.37, the
    true pose rolled by 89 degrees), for the table inv_sigma2_of("second").

    clean: 200 correspondences, 20 mismatches; matched: the same kind through a match row; far: a
    start 25 degrees and 60 % off with a third mismatches (rejected trials); noisy: 1.2 sigma of pixel noise (features that
    change sides between rounds); converged: clean's result fed back; nine: 9 correspondences (one round); three: 3; two: 2
    (FEW_POINTS); truth: little noise.

    Worlds of capacity 1024 in which lanes hold more than the six edges k_pose caches (lane_layout): cache_edge: 385
    correspondences in 390 features, so a few lanes hold a seventh edge; cache_full: 700 correspondences with 1.2 sigma of
    noise, 90 mismatches and a start 4 degrees off (flags behind the cache that change sides between rounds); cache_skewed: a
    match-row world of 1000 features whose 24 correspondences all sit on the features of two lanes, 16 on lane 5's and 8 on every
    other one of lane 37's, so that 62 lanes hold none (a lane has at most 16 features at this capacity); cache_holes: a
    match-row world of 640 features of which about a quarter have no point -- match -1, or a match to an entry with mask == 0 --
    in front of, between and behind the edges.

    Worlds whose 6x6 solves fail, each for the table table_of(name): no_weight: clean under a table of zeros (Hpp = 0, lambda =
    0: every solve fails); no_weight_big: the same with 700 correspondences; weight_lost (weight_lost_world: 100 gross mismatches
    at level 0, 20 exact correspondences at level 1) and weight_lost_big (420 and 40): failures behind accepted trials, with flags
    set."""
    if setting_name != "first":
        if (name, setting_name) not in _worlds:
            _worlds[name, setting_name] = SECOND_WORLDS[name]()
        return _worlds[name, setting_name]
    if name not in _worlds:
        if name == "clean":
            w = make_world(200, 1, outliers=20)
        elif name == "matched":
            w = make_world(150, 2, outliers=15, matched=True)
        elif name == "far":
            w = make_world(120, 3, outliers=40, angle_deg=25.0, scale=1.6)
        elif name == "noisy":
            w = make_world(180, 4, outliers=30, noise=1.2, angle_deg=4.0)
        elif name == "converged":
            c = world("clean")
            w = feed_back(c, pose_optimize(c)[0])
        elif name == "nine":
            w = make_world(9, 5, outliers=1)
        elif name == "three":
            w = make_world(3, 6)
        elif name == "two":
            w = make_world(2, 7)
        elif name == "truth":
            w = make_world(300, 8, noise=0.2, outliers=30)
        elif name == "cache_edge":
            w = make_world(385, 74, cap=BIG_CAP, outliers=40)  # (three mismatches behind the cache)
        elif name == "cache_full":
            w = make_world(700, 770, cap=BIG_CAP, outliers=90, noise=1.2, angle_deg=4.0)
        elif name == "cache_skewed":
            at = np.sort(np.r_[np.arange(5, 1000, WAVE), np.arange(37, 1000, 2 * WAVE)])
            w = scattered(make_world(len(at), 71, outliers=6, extra=0), at, 1000, 71)
        elif name == "cache_holes":
            rng = np.random.default_rng(72)
            kind = rng.choice(3, 640, p=[0.74, 0.13, 0.13])  # an edge, match -1, a match to an entry with mask == 0
            at = np.flatnonzero(kind == 0)
            w = scattered(make_world(len(at), 72, outliers=50, extra=0), at, 640, 72, dead=np.flatnonzero(kind == 2))
        elif name == "no_weight":
            w = world("clean")
        elif name == "no_weight_big":
            w = make_world(700, 73, cap=BIG_CAP, outliers=70)
        elif name == "weight_lost":
            w = weight_lost_world(100, 20, 74)
        elif name == "weight_lost_big":
            w = weight_lost_world(420, 40, 75, cap=BIG_CAP)
        else:
            raise KeyError(name)
        _worlds[name] = w
    return _worlds[name]
