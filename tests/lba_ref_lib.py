"""ctypes wrapper around tests/cpp/lba_ref.cpp -- the CPU restatement of the local bundle adjustment (include/orbx.h, "local
mapping: local bundle adjustment") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary directory,
as tests/ba_ref_lib.py compiles its source; a second, independently written numpy statement of the first Levenberg-Marquardt step
(numerically differentiated residuals, the full damped (6 F + 3 P) normal equations, numpy.linalg.solve); and the worlds
(synthetic local windows) that tests/test_lba_host.py and tests/test_gpu_lba.py share.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

from ba_ref_lib import K0, KEYPOINT_DTYPE, NLEVELS, inv_sigma2_table, rotvec, se3_exp
from pose_ref_lib import K_ANISO, NLEVELS_2, SCALE_FACTOR_2, SECOND  # noqa: F401 (the second setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lba_ref.cpp")
LBA_INTS = ("status", "n_points", "n_edges", "n_free")
LBA_PAIRS = ("iterations", "lm_trials", "rejected_trials", "solver_failures", "stop_reason", "n_active_points", "n_active_free")
LBA_RESULT_DTYPE = np.dtype([(n, "<i4") for n in LBA_INTS] + [(n, "<i4", 2) for n in LBA_PAIRS] +
                            [("n_level1", "<i4"), ("n_erased", "<i4")] +
                            [(n, "<f8", 2) for n in ("chi2_initial", "chi2_final", "lambda")])
assert LBA_RESULT_DTYPE.itemsize == 128
BAD_INPUT, NONFINITE = 2, 4
MAX_FREE = 64
COUNTERS = ("accepted", "rejected", "huber_outliers", "small_theta")
_L = None


def build(src=SRC, flags=("-O2",), exe_main=None):
    """Compiles the restatement: a shared object, or with exe_main (a source with its own main) a program -> its path."""
    d = tempfile.mkdtemp(prefix="lba_ref_")
    atexit.register(shutil.rmtree, d, True)
    out = os.path.join(d, "lba_ref_main" if exe_main else "liblba_ref.so")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", *flags]
    cmd += [exe_main, src, "-o", out] if exe_main else ["-fPIC", "-shared", src, "-o", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("lba_ref.cpp does not compile:\n" + p.stdout)
    return out


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        L = ctypes.CDLL(build())
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        head = [vp, vp, vp, vp, i32, i32, vp, i32, vp, vp, i32, i32, vp, vp, i32]
        L.lbar_local_ba.argtypes = head + [i32, i32, vp, vp, vp, vp, vp]
        L.lbar_local_ba.restype = None
        L.lbar_first_step.argtypes = head + [vp, vp, vp, vp, vp, vp, vp]
        L.lbar_huber_delta.restype = ctypes.c_double
        _L = L
    return _L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class World:
    """One problem in the batch layout: entry e is keyframe e.  kps [nE, cap], n [nE], pose [nE, 12], rows [nE, cap], map_pts
    [map_cap, 3], map_mask [map_cap] (or None), map_n, n_free, K [9]; truth: what is known about the scene."""

    def __init__(self, kps, n, pose, rows, map_pts, map_mask, map_n, n_free, K, truth=None, frames=None):
        self.kps, self.n, self.pose, self.rows, self.map_pts, self.map_mask, self.map_n, self.n_free, self.K, self.truth = \
            kps, n, pose, rows, map_pts, map_mask, int(map_n), int(n_free), K, truth
        self.n_entries, self.cap, self.map_cap = kps.shape[0], kps.shape[1], map_pts.shape[0]
        # the entry list: entry e names frame frames[e] of kps / n / pose (default: itself); rows stay per entry
        self.frames = np.arange(max(self.n_entries, 1), dtype=np.int32) if frames is None else np.ascontiguousarray(frames, np.int32)

    def copy(self):
        return World(self.kps.copy(), self.n.copy(), self.pose.copy(), self.rows.copy(), self.map_pts.copy(),
                     None if self.map_mask is None else self.map_mask.copy(), self.map_n, self.n_free, self.K, self.truth, self.frames.copy())

    def padded(self, cap, map_cap):
        """The same problem in arrays of larger capacities."""
        kps, rows = np.zeros((self.n_entries, cap), KEYPOINT_DTYPE), np.full((self.n_entries, cap), -1, np.int32)
        kps[:, :self.cap], rows[:, :self.cap] = self.kps, self.rows
        pts, mask = np.zeros((map_cap, 3), np.float32), np.zeros(map_cap, np.uint8)
        pts[:self.map_cap] = self.map_pts
        mask[:self.map_cap] = 1 if self.map_mask is None else self.map_mask
        return World(kps, self.n.copy(), self.pose.copy(), rows, pts, mask, self.map_n, self.n_free, self.K, self.truth, self.frames.copy())


def local_ba(w: World, n_iterations=5, n_more_iterations=10, inv_sigma2=None, nlevels=NLEVELS):
    """The restatement for one problem -> (LBA_RESULT_DTYPE record, pose_out [nE, 12], map_out [map_cap, 3], outlier [nE, cap],
    {counter: value})."""
    sig = np.ascontiguousarray(inv_sigma2_table(nlevels) if inv_sigma2 is None else inv_sigma2, np.float32)
    nE = w.n_entries
    frames = w.frames
    res, pose_out = np.zeros(1, LBA_RESULT_DTYPE), np.zeros((max(nE, 1), 12), np.float32)
    map_out, outlier, cnt = np.zeros((w.map_cap, 3), np.float32), np.zeros((max(nE, 1), w.cap), np.uint8), np.zeros(4, np.int64)
    lib().lbar_local_ba(_p(w.kps), _p(w.n), _p(w.pose), _p(frames), nE, w.n_free, _p(w.rows), w.cap, _p(w.map_pts), _p(w.map_mask),
                        w.map_n, w.map_cap, _p(w.K), _p(sig), len(sig), int(n_iterations), int(n_more_iterations), _p(pose_out),
                        _p(map_out), _p(outlier), _p(res), _p(cnt))
    return res[0].copy(), pose_out[:nE], map_out, outlier[:nE], dict(zip(COUNTERS, (int(c) for c in cnt)))


def first_step(w: World, inv_sigma2=None, nlevels=NLEVELS):
    """The restatement's first trial of iteration 0 of round 1 -> dict(pidx, free, lam, chi2_initial, xp [nA, 6], xl [n, 3]) or
    None."""
    sig = np.ascontiguousarray(inv_sigma2_table(nlevels) if inv_sigma2 is None else inv_sigma2, np.float32)
    frames = w.frames
    pidx, act, nA = np.zeros(w.map_cap, np.int32), np.zeros(MAX_FREE, np.int32), np.zeros(1, np.int32)
    xp, xl, lam, chi2 = np.zeros(6 * MAX_FREE), np.zeros((w.map_cap, 3)), np.zeros(1), np.zeros(1)
    n = lib().lbar_first_step(_p(w.kps), _p(w.n), _p(w.pose), _p(frames), w.n_entries, w.n_free, _p(w.rows), w.cap, _p(w.map_pts),
                              _p(w.map_mask), w.map_n, w.map_cap, _p(w.K), _p(sig), len(sig), _p(pidx), _p(act), _p(nA), _p(xp),
                              _p(xl), _p(lam), _p(chi2))
    if n < 0:
        return None
    a = int(nA[0])
    return dict(pidx=pidx[:n].copy(), free=act[:a].copy(), lam=float(lam[0]), chi2_initial=float(chi2[0]),
                xp=xp[:6 * a].reshape(a, 6).copy(), xl=xl[:n].copy())


# ---- the second statement: numpy, rotation matrices, numerical derivatives, one dense solve; nothing shared with the C++ ----

def graph(w: World, inv_sigma2=None, nlevels=NLEVELS):
    """The graph as plain arrays: (vertices: map indices ascending; edges: rows of (entry, feature, vertex number); u v [M, 2];
    weights [M])."""
    sig = (inv_sigma2_table(nlevels) if inv_sigma2 is None else np.asarray(inv_sigma2, np.float32)).astype(np.float64)
    usable = np.zeros(w.map_cap, bool)
    usable[:w.map_n] = True if w.map_mask is None else w.map_mask[:w.map_n] != 0
    seen_free = np.zeros(w.map_cap, bool)
    for e in range(w.n_free):
        r = w.rows[e, :w.n[e]]
        seen_free[r[r >= 0]] = True
    vertices = np.flatnonzero(usable & seen_free)
    number = np.full(w.map_cap, -1, np.int64)
    number[vertices] = np.arange(len(vertices))
    edges = [(e, f, number[w.rows[e, f]]) for e in range(w.n_entries) for f in range(w.n[e])
             if w.rows[e, f] >= 0 and number[w.rows[e, f]] >= 0]
    edges = np.array(edges, np.int64).reshape(-1, 3)
    kp = w.kps[edges[:, 0], edges[:, 1]]
    return vertices, edges, np.c_[kp["x"], kp["y"]].astype(np.float64), sig[kp["octave"]]


def pose_matrices(pose12):
    p = np.asarray(pose12, np.float64).reshape(-1, 12)
    return p[:, :9].reshape(-1, 3, 3).copy(), p[:, 9:].copy()


def first_step_numpy(w: World, inv_sigma2=None, nlevels=NLEVELS, h=1e-6):
    """The first damped Gauss-Newton step on the full (6 F + 3 P) system -> dict(pidx, free, lam, chi2_initial, xp, xl)."""
    vertices, edges, obs, wt = graph(w, inv_sigma2, nlevels)
    R0, t0 = pose_matrices(w.pose)
    X0 = w.map_pts[vertices].astype(np.float64)
    Kd = w.K.reshape(3, 3).astype(np.float64)
    free = np.array(sorted(set(int(e) for e in edges[:, 0] if e < w.n_free)), np.int64)
    col = {int(e): 6 * a for a, e in enumerate(free)}
    F, P, M = len(free), len(vertices), len(edges)
    delta = float(np.float32(np.sqrt(5.991)))

    def res(R, t, X):
        Y = np.einsum("mij,mj->mi", R[edges[:, 0]], X[edges[:, 2]]) + t[edges[:, 0]]
        return obs - np.c_[Y[:, 0] / Y[:, 2] * Kd[0, 0] + Kd[0, 2], Y[:, 1] / Y[:, 2] * Kd[1, 1] + Kd[1, 2]]

    e0 = res(R0, t0, X0)
    c = wt * (e0 ** 2).sum(axis=1)
    out = c > delta * delta
    chi2 = float(np.where(out, 2 * np.sqrt(np.where(out, c, 1.0)) * delta - delta * delta, c).sum())
    rho1 = np.where(out, delta / np.sqrt(np.where(out, c, 1.0)), 1.0)
    W = np.repeat(rho1 * wt, 2)
    J = np.zeros((2 * M, 6 * F + 3 * P))
    for e in free:
        mine = np.repeat(edges[:, 0] == e, 2)
        for k in range(6):
            d = []
            for sign in (1.0, -1.0):
                u = np.zeros(6)
                u[k] = sign * h
                dR, dt = se3_exp(u)
                R, t = R0.copy(), t0.copy()
                R[e], t[e] = dR @ R0[e], dR @ t0[e] + dt
                d.append(res(R, t, X0).reshape(-1))
            J[mine, col[int(e)] + k] = ((d[0] - d[1]) / (2 * h))[mine]
    for k in range(3):  # the points are independent: one perturbation per coordinate serves them all
        dX = np.zeros_like(X0)
        dX[:, k] = h
        d = ((res(R0, t0, X0 + dX) - res(R0, t0, X0 - dX)) / (2 * h)).reshape(-1)
        rows = np.arange(2 * M)
        J[rows, 6 * F + 3 * np.repeat(edges[:, 2], 2) + k] = d
    H = J.T @ (W[:, None] * J)
    b = -J.T @ (W * e0.reshape(-1))
    lam = 1e-5 * float(np.abs(np.diag(H)).max())
    x = np.linalg.solve(H + lam * np.eye(len(H)), b)
    return dict(pidx=vertices, free=free, lam=lam, chi2_initial=chi2, xp=x[:6 * F].reshape(F, 6), xl=x[6 * F:].reshape(P, 3))


# ---- the worlds the host and the GPU test share ----

def make_world(n_free, n_fixed, n_points, seed=0, cap=None, map_cap=None, noise=0.5, outliers=0, obs_per_point=4,
               twist_scale=1.0, point_noise=0.02, extra=3, nlevels=NLEVELS, K=K0, scale_factor=1.2, dense=None, lonely=0,
               fixed_only=0, idle_free=0, masked=2, pose_scale=1.0):
    """A window of n_free + n_fixed keyframes on a baseline that see n_points points 4 to 8 units deep, obs_per_point keyframes
    per point.  Pixel noise in units of the level's sigma; `outliers` gross mismatches; the free poses start off the truth by a
    twist (twist_scale), the points by point_noise; the fixed poses are the true ones.  Each keyframe also holds `extra` features
    without a point (-1), `extra` unmapped ones (-2) and, with masked > 0, `masked` that name a point whose mask byte is 0.
    dense: (entry, count): that keyframe sees the first `count` points.  lonely: points seen by exactly one free keyframe and all
    fixed ones; fixed_only: points only fixed keyframes see (no vertices); idle_free: the last idle_free free keyframes observe
    nothing; pose_scale: the free poses' input translations multiplied by it."""
    rng = np.random.default_rng(5000 + seed)
    nE = n_free + n_fixed
    Kd = np.asarray(K, np.float64).reshape(3, 3)
    Rt = [rotvec(rng.normal(0, 0.03, 3)) for _ in range(nE)]
    tt = [np.array([-0.25 * e, 0.0, 0.0]) + rng.normal(0, 0.03, 3) for e in range(nE)]
    X = np.c_[rng.uniform(-2, 2, n_points) - 0.12 * nE, rng.uniform(-1.5, 1.5, n_points), rng.uniform(4, 8, n_points)]
    seeing = [[] for _ in range(nE)]
    busy_free = n_free - idle_free
    pool = [e for e in range(nE) if e < busy_free or e >= n_free]
    for j in range(n_points):
        if j < lonely and busy_free > 0:
            who = [int(rng.integers(0, busy_free))] + list(range(n_free, nE))
        elif j < lonely + fixed_only and n_fixed > 0:
            who = list(range(n_free, nE))
        else:
            who = list(rng.choice(pool, min(obs_per_point, len(pool)), replace=False)) if pool else []
        for e in who:
            seeing[int(e)].append(j)
    if dense is not None:
        seeing[dense[0]] = sorted(set(seeing[dense[0]]) | set(range(min(dense[1], n_points))))
    n = np.array([len(sv) + 2 * extra + masked for sv in seeing], np.int32)
    cap = int(cap or max(int(n.max()) if nE else 1, 1))
    n_spare = masked
    map_n = n_points + n_spare
    map_cap = int(map_cap or max(map_n + 2, 1))
    assert cap >= (n.max() if nE else 0) and map_cap >= map_n
    kps, rows = np.zeros((nE, cap), KEYPOINT_DTYPE), np.full((nE, cap), -1, np.int32)
    pose = np.zeros((nE, 12), np.float32)
    bad_left = outliers
    for e in range(nE):
        ne = int(n[e])
        kps["x"][e, :ne], kps["y"][e, :ne] = rng.uniform(0, 640, ne), rng.uniform(0, 480, ne)
        kps["octave"][e, :ne] = rng.integers(0, nlevels, ne)
        slots = rng.permutation(ne)
        pts = np.array(seeing[e], np.int64)
        if len(pts):
            Y = X[pts] @ Rt[e].T + tt[e]
            octs = kps["octave"][e, slots[:len(pts)]]
            uv = np.c_[Y[:, 0] / Y[:, 2] * Kd[0, 0] + Kd[0, 2], Y[:, 1] / Y[:, 2] * Kd[1, 1] + Kd[1, 2]]
            uv += rng.normal(0, 1, uv.shape) * noise * (scale_factor ** octs)[:, None]
            nb = min(bad_left, len(pts) // 8)
            if nb:
                which = rng.choice(len(pts), nb, replace=False)
                uv[which] += rng.choice([-1.0, 1.0], (nb, 2)) * rng.uniform(20, 40, (nb, 2))
                bad_left -= nb
            kps["x"][e, slots[:len(pts)]], kps["y"][e, slots[:len(pts)]] = uv[:, 0], uv[:, 1]
            rows[e, slots[:len(pts)]] = pts
        rest = slots[len(pts):]
        if len(rest):
            rows[e, rest[:extra]] = -2
            for k in range(masked):
                rows[e, rest[2 * extra + k]] = n_points + k  # (a point whose mask byte is 0)
        if e < n_free:
            dR, dt = se3_exp(rng.normal(0, 1, 6) * twist_scale * np.array([0.004, 0.004, 0.004, 0.01, 0.01, 0.01]))
            Rin, tin = dR @ Rt[e], (dR @ tt[e] + dt) * pose_scale
        else:
            Rin, tin = Rt[e], tt[e]
        pose[e] = np.r_[Rin.reshape(9), tin]
    map_pts, mask = np.zeros((map_cap, 3), np.float32), np.zeros(map_cap, np.uint8)
    map_pts[:n_points] = X + rng.normal(0, point_noise, X.shape)
    map_pts[n_points:] = rng.normal(0, 1, (map_cap - n_points, 3))
    mask[:n_points] = 1
    truth = dict(R=Rt, t=tt, X=X)
    return World(kps, n, pose, rows, map_pts, mask, map_n, n_free, np.asarray(K, np.float32).reshape(9).copy(), truth)


def zero_table(nlevels=NLEVELS):
    return np.zeros(nlevels, np.float32)


def inv_sigma2_of(setting_name: str):
    return None if setting_name == "first" else inv_sigma2_table(NLEVELS_2, SCALE_FACTOR_2)


_worlds = {}


def world(name: str) -> World:
    """Named worlds, made once.
    window: 4 free + 3 fixed keyframes, 120 points, gross mismatches (level-1 edges, rejected trials are likely);
    truth: no pixel noise, 3 free + 2 fixed, perturbed poses and points;
    far: the free poses start 12 times further off, with mismatches (rejected trials);
    lonely: points seen by one free keyframe and the fixed ones only, and points only fixed keyframes see;
    idle: a free keyframe without an observation; nofixed: no fixed keyframe at all;
    rejecting: the free poses' translations three times too long, no fixed keyframe (a rejected trial);
    losing: two observations per point and many mismatches, so that some points lose every edge between the rounds;
    two_view: one free and one fixed keyframe (the fixed one at the identity: see two_view_world);
    second: the window under K_ANISO and 5 levels of 1.37."""
    if name not in _worlds:
        if name == "window":
            w = make_world(4, 3, 120, 1, outliers=10)
        elif name == "truth":
            w = make_world(3, 2, 90, 2, noise=0.0, twist_scale=2.0, point_noise=0.03)
        elif name == "far":
            w = make_world(3, 2, 80, 3, outliers=8, twist_scale=12.0)
        elif name == "lonely":
            w = make_world(3, 3, 70, 4, lonely=10, fixed_only=6)
        elif name == "idle":
            w = make_world(4, 2, 60, 5, idle_free=1)
        elif name == "nofixed":
            w = make_world(4, 0, 80, 6)
        elif name == "losing":
            w = make_world(2, 1, 60, 7, outliers=30, obs_per_point=2)
        elif name == "rejecting":
            w = make_world(3, 0, 80, 102, outliers=8, pose_scale=3)
        elif name == "second":
            w = make_world(4, 3, 100, 8, outliers=8, **SECOND)
        else:
            raise KeyError(name)
        _worlds[name] = w
    return _worlds[name]


def two_view_world(pair) -> World:
    """A ba_ref_lib.Pair as a local window: entry 0 = frame 2 (free, at the Initializer's pose), entry 1 = frame 1 (fixed, the
    identity), the map set = the pair's points with the triangulated matches as the mask."""
    cap = pair.cap
    kps = np.stack([pair.k2, pair.k1])
    n = np.array([pair.n2, pair.n1], np.int32)
    rows = np.full((2, cap), -1, np.int32)
    idx = np.array([i for i in range(pair.n1) if pair.m12[i] >= 0 and pair.tri[i]], np.int64)
    rows[1, idx] = idx
    rows[0, pair.m12[idx]] = idx
    pose = np.zeros((2, 12), np.float32)
    pose[0] = np.r_[pair.init["R21"][0].reshape(9), pair.init["t21"][0]]
    pose[1] = np.r_[np.eye(3).reshape(9), np.zeros(3)]
    mask = np.zeros(cap, np.uint8)
    mask[idx] = 1
    return World(kps, n, pose, rows, pair.p3d.copy(), mask, pair.n1, 1, pair.K.copy())
