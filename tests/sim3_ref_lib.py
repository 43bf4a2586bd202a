"""ctypes wrapper around tests/cpp/sim3_ref.cpp -- the CPU restatement of Sim3Solver (include/orbx.h, "loop closing: Sim3
RANSAC") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary directory, as tests/tri_ref_lib.py
compiles its source; SetRansacParameters' table evaluated directly in Python; a literal swap-and-pop sampler on a real list; a
second, independently written numpy statement (Horn through numpy.linalg.eigh, the inlier test spelled out again in f64, nothing
shared with the C++); and the worlds that tests/test_sim3_host.py and tests/test_gpu_sim3.py share.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

import pose_ref_lib as P
from pnp_ref_lib import sigma2_table
from pose_ref_lib import K_ANISO, MOTION_2, NLEVELS_2, ROLL, SCALE_FACTOR_2, SECOND, SETTINGS  # noqa: F401 (the second setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim3_ref.cpp")
KEYPOINT_DTYPE = P.KEYPOINT_DTYPE
SIM3_INTS = ("status", "n_correspondences", "max_its", "its_run", "found_it", "best_it", "n_inliers", "n_best_inliers", "n_degenerate")
SIM3_RESULT_DTYPE = np.dtype([(n, "<i4") for n in SIM3_INTS] + [("reserved", "<i4", 2), ("s12", "<f4"), ("R12", "<f4", (3, 3)),
                                                                 ("t12", "<f4", 3)])
assert SIM3_RESULT_DTYPE.itemsize == 96
BAD_INPUT, NONFINITE, FEW_POINTS, BAD_DRAWS, NO_RESULT = 2, 4, 8, 16, 32
HYP_DEGENERATE, HYP_BAD_DRAWS = 1, 2
RAND_MAX = 2147483647
NLEVELS = P.NLEVELS
K0 = P.K0
# LoopClosing's SetRansacParameters(0.99, 20, 300) and Sim3Solver's th = sqrt(9.210)
PARAMS = dict(probability=0.99, min_inliers=20, max_iterations=300, th2=9.210, fix_scale=0)
_L = None


def compile_command(out, extra=(), src=SRC):
    return ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", *extra, src, "-o", out]


def build(src=SRC) -> ctypes.CDLL:
    """Compiles a restatement source (lib(): the committed one; tests/test_camera_mutants_host.py: an altered copy) and binds it."""
    d = tempfile.mkdtemp(prefix="sim3_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libsim3_ref.so")
    p = subprocess.run(compile_command(so, ("-fPIC", "-shared"), src), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("sim3_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    world = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.s3r_solve.argtypes = world + [vp, i32, i32, f32, i32, vp, i32, vp, vp, vp, vp]
    L.s3r_solve.restype = None
    L.s3r_hypotheses.argtypes = world + [i32, f32, i32, vp, vp, vp, vp]
    L.s3r_errors.argtypes = world + [f32, vp, vp, vp, vp, vp, vp]
    L.s3r_sample.argtypes = [vp, i32, vp]
    L.s3r_horn.argtypes = [vp, vp, i32, vp, vp, vp]
    L.s3r_horn.restype = None
    L.s3r_eig_top.argtypes = [vp, vp]
    L.s3r_eig_top.restype = ctypes.c_double
    return L


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        _L = build()
    return _L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


# ---- SetRansacParameters, the sampler ----

def ransac_entry(N, probability=0.99, min_inliers=20, max_iterations=300):
    """SetRansacParameters for one N, evaluated directly with the design's expression types -> mRansacMaxIts.  N < min_inliers
    (bNoMore before anything iterates; the design takes log of a negative number there) is given max_iterations."""
    if N < min_inliers:
        return int(max_iterations)
    if N == min_inliers:
        its = 1
    else:
        eps = np.float32(min_inliers) / np.float32(N)
        its = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3)))
    return max(1, min(its, int(max_iterations)))


_tables = {}


def ransac_table(n_max, probability=0.99, min_inliers=20, max_iterations=300, **_) -> np.ndarray:
    """[n_max + 1] int32, made once per parameter set."""
    key = (n_max, probability, min_inliers, max_iterations)
    if key not in _tables:
        _tables[key] = np.array([ransac_entry(N, *key[1:]) for N in range(n_max + 1)], np.int32)
    return _tables[key]


def list_sampler(draws, N):
    """The literal sampler: vAvailableIndices as a real list, RandomInt on the draws, swap with the last and pop."""
    avail = list(range(N))
    out = []
    for r in draws:
        randi = int((float(r) / (float(RAND_MAX) + 1.0)) * len(avail))
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


def sample(draws, N):
    """The restatement's sampler -> the three picks, or None for a draw out of range."""
    d, sel = np.ascontiguousarray(draws, np.int32), np.zeros(3, np.int32)
    return [int(v) for v in sel] if lib().s3r_sample(_p(d), int(N), _p(sel)) else None


def draws_for(triple, N):
    """Three rand() values that make the sampler pick the correspondences `triple` out of N, in that order."""
    avail, out = list(range(N)), []
    for c in triple:
        pos, size = avail.index(c), len(avail)
        r = -(-pos * (RAND_MAX + 1) // size)  # the smallest r with (int)(r / 2^31 * size) == pos
        while int((float(r) / (float(RAND_MAX) + 1.0)) * size) < pos:
            r += 1
        assert int((float(r) / (float(RAND_MAX) + 1.0)) * size) == pos and r <= RAND_MAX
        out.append(r)
        avail[pos] = avail[-1]
        avail.pop()
    return np.array(out, np.int32)


def make_draws(n_iter, seed=0):
    """rand() values for n_iter hypotheses."""
    return np.random.default_rng(41000 + seed).integers(0, RAND_MAX + 1, (n_iter, 3)).astype(np.int32)


# ---- worlds ----

class World:
    """One problem's inputs as rows of `cap` entries: the two keyframes (kps1, n1, points1, mask1, pose1 / ...2), the match row
    and K, plus what is known about the scene."""

    def __init__(self, kps1, n1, kps2, n2, match, points1, mask1, points2, mask2, pose1, pose2, K, truth=None):
        self.kps1, self.n1, self.kps2, self.n2, self.match = kps1, int(n1), kps2, int(n2), match
        self.points1, self.mask1, self.points2, self.mask2, self.pose1, self.pose2, self.K, self.truth = \
            points1, mask1, points2, mask2, pose1, pose2, K, truth
        self.cap = len(kps1)

    def copy(self):
        c = lambda a: None if a is None else a.copy()  # noqa: E731
        return World(self.kps1.copy(), self.n1, self.kps2.copy(), self.n2, self.match.copy(), self.points1.copy(), c(self.mask1),
                     self.points2.copy(), c(self.mask2), self.pose1.copy(), self.pose2.copy(), self.K, self.truth)

    def edges(self):
        """(features i1, features i2) of the correspondences, ascending i1."""
        i1 = np.arange(max(min(self.n1, self.cap), 0))
        i2 = self.match[:len(i1)].astype(np.int64)
        ok = (i2 >= 0) & (i2 < self.n2)
        if self.mask1 is not None:
            ok &= (self.mask1[i1] != 0) & (self.mask2[np.where(ok, i2, 0)] != 0)
        return i1[ok], i2[ok]


def make_world(n, seed=0, cap=None, noise=0.0, outliers=0, extra=5, s=1.3, rot=(0.05, -0.08, 0.03), t=(0.3, -0.2, 0.4),
               use_mask=True, nlevels=NLEVELS, same_depth=None, K=K0, scale_factor=1.2):
    """Two keyframes with n correspondences.  The points lie 4 to 20 units in front of camera 2 (Y2); camera 1 sees them at Y1 =
    s R Y2 + t, the true similarity between the camera frames (s != 1: a monocular map that drifted in scale; s = 1 for a
    fix_scale world).  Each keyframe stores its points in a world frame of its own pose.  noise: standard deviation of the error
    of KF2's points, in pixels of image 2 at the point's depth and level (in units of the level's sigma); `outliers` of the
    correspondences name a wrong point (gross mismatches).  Each keyframe holds `extra` more features: without a point, with a
    point but no match, and matched to an entry that is no point."""
    rng = np.random.default_rng(15000 + seed)
    Rt, tt, st = P.rotvec(rot), np.array(t, np.float64), float(s)
    Kd = np.asarray(K, np.float64).reshape(3, 3)
    z = rng.uniform(4, 20, n) if same_depth is None else np.full(n, float(same_depth))
    Y2 = np.c_[rng.uniform(-0.45, 0.45, n) * z, rng.uniform(-0.32, 0.32, n) * z, z]
    Y1 = st * Y2 @ Rt.T + tt
    oct1, oct2 = rng.integers(0, nlevels, n), rng.integers(0, nlevels, n)
    Y2n = Y2 + rng.normal(0, 1, (n, 3)) * (noise * (scale_factor ** oct2) * z / Kd[0, 0])[:, None]
    bad = np.sort(rng.choice(n, outliers, replace=False)) if outliers else np.zeros(0, np.int64)
    Y2n[bad] += rng.choice([-1.0, 1.0], (len(bad), 3)) * rng.uniform(1.0, 3.0, (len(bad), 3))
    R1, t1 = P.rotvec((0.2, -0.1, 0.05)), np.array([0.5, -1.0, 2.0])
    R2, t2 = P.rotvec((-0.1, 0.3, 0.1)), np.array([-1.5, 0.4, 1.0])
    X1w, X2w = (Y1 - t1) @ R1, (Y2n - t2) @ R2
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
        kps1["x"][slots1], kps1["y"][slots1], kps1["octave"][slots1] = proj(Y1)[:, 0], proj(Y1)[:, 1], oct1
        kps2["x"][slots2], kps2["y"][slots2], kps2["octave"][slots2] = proj(Y2)[:, 0], proj(Y2)[:, 1], oct2
    points1 = rng.normal(0, 1, (cap, 3)).astype(np.float32)  # (entries that are no point hold leftovers)
    points2 = rng.normal(0, 1, (cap, 3)).astype(np.float32)
    mask1, mask2 = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    match = np.full(cap, -1, np.int32)
    match[slots1] = slots2
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
    truth = dict(s=st, R=Rt, t=tt, slots1=slots1, slots2=slots2, bad=bad, Y1=Y1, Y2=Y2)
    return World(kps1, nf, kps2, nf, match, points1, mask1, points2, mask2, pose1, pose2, np.asarray(K, np.float32).reshape(9).copy(), truth)


# ---- the restatement ----

def _world_args(w: World, sig):
    return (_p(w.kps1), w.n1, _p(w.kps2), w.n2, w.cap, _p(w.match), _p(w.points1), _p(w.mask1), _p(w.points2), _p(w.mask2),
            _p(w.pose1), _p(w.pose2), _p(w.K), _p(sig), len(sig))


def _sig(sigma2, nlevels):
    return np.ascontiguousarray(sigma2_table(nlevels) if sigma2 is None else sigma2, np.float32)


def solve(w: World, draws, mode=0, sigma2=None, nlevels=NLEVELS, **params):
    """The restatement for one problem -> (SIM3_RESULT_DTYPE record, sim3 [13] f32, row [cap] i32, inliers [cap] u8).  mode 0:
    the literal sequential loop; mode 1: all hypotheses, then rule 6 in iteration order."""
    prm = dict(PARAMS, **params)
    sig = _sig(sigma2, nlevels)
    table = np.ascontiguousarray(ransac_table(w.cap, **prm))
    draws = np.ascontiguousarray(draws, np.int32).reshape(-1, 3)
    res, sim = np.zeros(1, SIM3_RESULT_DTYPE), np.zeros(13, np.float32)
    row, inl = np.zeros(w.cap, np.int32), np.zeros(w.cap, np.uint8)
    lib().s3r_solve(*_world_args(w, sig), _p(table), int(prm["fix_scale"]), int(prm["min_inliers"]), np.float32(prm["th2"]),
                    len(draws), _p(draws), int(mode), _p(res), _p(sim), _p(row), _p(inl))
    return res[0].copy(), sim, row, inl


def hypotheses(w: World, draws, sigma2=None, nlevels=NLEVELS, fix_scale=0, th2=9.210):
    """Every hypothesis on its own -> (N, counts [n_iter], flags [n_iter], sims [n_iter, 13]); N = -1: refused."""
    sig = _sig(sigma2, nlevels)
    draws = np.ascontiguousarray(draws, np.int32).reshape(-1, 3)
    counts, flags, sims = np.zeros(len(draws), np.int32), np.zeros(len(draws), np.int32), np.zeros((len(draws), 13), np.float32)
    N = lib().s3r_hypotheses(*_world_args(w, sig), int(fix_scale), np.float32(th2), len(draws), _p(draws), _p(counts), _p(flags),
                             _p(sims))
    return N, counts, flags, sims


def errors(w: World, sim, sigma2=None, nlevels=NLEVELS, th2=9.210):
    """The constructor's arrays and rule 5's f32 errors under sim [13] -> dict(i1, i2, err [N, 4] = err1, err2, maxErr1,
    maxErr2, X1 [N, 3], X2 [N, 3], inlier [N])."""
    sig = _sig(sigma2, nlevels)
    sim = np.ascontiguousarray(sim, np.float32)
    i1, i2, err = np.zeros(w.cap, np.int32), np.zeros(w.cap, np.int32), np.zeros((w.cap, 4), np.float32)
    X, inl = np.zeros((w.cap, 6), np.float32), np.zeros(w.cap, np.uint8)
    N = lib().s3r_errors(*_world_args(w, sig), np.float32(th2), _p(sim), _p(i1), _p(i2), _p(err), _p(X), _p(inl))
    assert N >= 0
    return dict(i1=i1[:N], i2=i2[:N], err=err[:N], X1=X[:N, :3], X2=X[:N, 3:], inlier=inl[:N] != 0)


def horn(P1, P2, fix_scale=False):
    """The restatement's Horn on a triple: P1, P2 [3 points, 3] -> (s, R, t)."""
    A, B = np.ascontiguousarray(P1, np.float64), np.ascontiguousarray(P2, np.float64)
    R, t, s = np.zeros(9), np.zeros(3), np.zeros(1)
    lib().s3r_horn(_p(A), _p(B), int(fix_scale), _p(R), _p(t), _p(s))
    return float(s[0]), R.reshape(3, 3), t


def eig_top(N):
    """The restatement's 4x4 Jacobi -> (largest signed eigenvalue, its eigenvector)."""
    A, q = np.ascontiguousarray(N, np.float64), np.zeros(4)
    lam = lib().s3r_eig_top(_p(A), _p(q))
    return float(lam), q


# ---- the second statement: numpy f64; nothing shared with the C++ ----

def camera_points_numpy(w: World):
    """(i1, i2, Y1 [N, 3], Y2 [N, 3]): the correspondences' points in their camera frames, f64 from the f32 inputs."""
    i1, i2 = w.edges()
    T1, T2 = w.pose1.astype(np.float64), w.pose2.astype(np.float64)
    Y1 = w.points1[i1].astype(np.float64) @ T1[:9].reshape(3, 3).T + T1[9:]
    Y2 = w.points2[i2].astype(np.float64) @ T2[:9].reshape(3, 3).T + T2[9:]
    return i1, i2, Y1, Y2


def horn_numpy(P1, P2, fix_scale=False):
    """Horn 1987 through numpy.linalg.eigh: P1, P2 [k points, 3] -> (s, R, t) with P1 ~ s R P2 + t."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    O1, O2 = P1.mean(0), P2.mean(0)
    A, B = (P1 - O1).T, (P2 - O2).T  # 3 x k
    M = B @ A.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    lam, vec = np.linalg.eigh(N)
    qw, qx, qy, qz = vec[:, -1] / np.linalg.norm(vec[:, -1])
    R = P.quat_to_matrix((qx, qy, qz, qw))
    P3 = R @ B
    s = 1.0 if fix_scale else float((A * P3).sum() / (P3 * P3).sum())
    return s, R, O1 - s * R @ O2


def errors_numpy(Y1, Y2, s, R, t, K):
    """The squared pixel distances of rule 5 in f64 -> (err1 [N], err2 [N])."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    proj = lambda Y: np.c_[K[0, 0] * Y[:, 0] / Y[:, 2] + K[0, 2], K[1, 1] * Y[:, 1] / Y[:, 2] + K[1, 2]]  # noqa: E731
    in1 = proj(s * Y2 @ R.T + t)
    in2 = proj((Y1 - t) @ R / s)
    return ((proj(Y1) - in1) ** 2).sum(1), ((in2 - proj(Y2)) ** 2).sum(1)


def sim_difference(s1, R1, t1, s2, R2, t2):
    """(rotation angle in radians as |R1 - R2|_F / sqrt(2), |s1 / s2 - 1|, |t1 - t2|)."""
    return (float(np.linalg.norm(np.asarray(R1, np.float64) - R2) / np.sqrt(2)), abs(float(s1) / float(s2) - 1.0),
            float(np.linalg.norm(np.asarray(t1, np.float64) - t2)))


# ======== ORBmatcher::SearchBySim3 ("loop closing: matching under a similarity") ========

MSIM3_FIELDS = ("status", "n_found", "n_points_12", "n_behind_12", "n_out_image_12", "n_out_distance_12", "n_with_candidates_12",
                "n_over_dist_12", "n_points_21", "n_behind_21", "n_out_image_21", "n_out_distance_21", "n_with_candidates_21",
                "n_over_dist_21", "n_one_sided", "reserved")
MSIM3_RESULT_DTYPE = np.dtype([(n, "<i4") for n in MSIM3_FIELDS])
MSIM3_BAD_INPUT, MSIM3_NONFINITE = 2, 4
BOUNDS = (0, 640, 0, 480)
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
IDENTITY_SIM = np.r_[IDENTITY, 1].astype(np.float32)


def scale_table(nlevels=NLEVELS, scale_factor=1.2):
    """mvScaleFactor as ORBextractor's constructor computes it (f32)."""
    out = np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        out[i] = np.float32(out[i - 1] * np.float32(scale_factor))
    return out


class MWorld:
    """One pair for SearchBySim3, rows of `cap` entries per keyframe: kps, desc [cap, 32], n, points, mask (or None), pdesc (or
    None), dist [cap, 2], pose [12]; the row `match` [cap], sim [13], K [9], bounds."""

    def __init__(self, cap, K=None, bounds=BOUNDS, masks=True, pdesc=False):
        z = lambda *s, dt=np.float32: np.zeros((cap,) + s, dt)  # noqa: E731
        self.cap, self.K, self.bounds = cap, np.ascontiguousarray(K0 if K is None else K, np.float32).reshape(9), tuple(bounds)
        self.kps, self.desc, self.n = [np.zeros(cap, KEYPOINT_DTYPE) for _ in range(2)], [z(32, dt=np.uint8) for _ in range(2)], [0, 0]
        self.points, self.dist = [z(3), z(3)], [z(2), z(2)]
        self.mask = [z(dt=np.uint8), z(dt=np.uint8)] if masks else None
        self.pdesc = [z(32, dt=np.uint8), z(32, dt=np.uint8)] if pdesc else None
        self.pose, self.sim, self.match = [IDENTITY.copy(), IDENTITY.copy()], IDENTITY_SIM.copy(), np.full(cap, -1, np.int32)
        self.truth = {}
        self.scale = None  # (mvScaleFactor when it is not the default table)

    def copy(self):
        import copy
        return copy.deepcopy(self)

    def feature(self, side, u, v, octave, desc):
        """Appends a feature to keyframe `side` -> its index."""
        i = self.n[side]
        self.kps[side]["x"][i], self.kps[side]["y"][i], self.kps[side]["octave"][i], self.desc[side][i] = u, v, octave, desc
        self.n[side] = i + 1
        return i

    def point(self, side, i, X, min_d=0.1, max_d=1000.0, pdesc=None):
        if max_d is None:  # level 0 under the identity: max / dist3D = 0.95
            max_d = 0.95 * float(np.linalg.norm(np.asarray(X, np.float64)))
        self.points[side][i], self.dist[side][i] = X, (min_d, max_d)
        if self.mask is not None:
            self.mask[side][i] = 1
        if pdesc is not None:
            self.pdesc[side][i] = pdesc


def search_by_sim3(w: MWorld, th=7.5, orb_dist=100, scale=None):
    """The restatement for one pair -> dict(matches [cap], res (MSIM3_RESULT_DTYPE record), vn1, vn2 [cap], proj1, proj2 [cap,
    5] = u, v, radius, level, stage).  Counts outside [0, cap] are clamped and flagged here, as the device does."""
    if scale is None:
        scale = scale_table() if w.scale is None else w.scale
    sc = np.ascontiguousarray(scale, np.float32)
    n = [max(0, min(int(v), w.cap)) for v in w.n]
    m, res = w.match.copy(), np.zeros(1, MSIM3_RESULT_DTYPE)
    vn1, vn2 = np.full(w.cap, -1, np.int32), np.full(w.cap, -1, np.int32)
    pr1, pr2 = np.zeros((w.cap, 5), np.float32), np.zeros((w.cap, 5), np.float32)
    b = np.array(w.bounds, np.int32)
    L = lib()
    if not hasattr(L, "_msim3"):
        vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        side = [vp, vp, i32, vp, vp, vp, vp, vp]
        L.s3r_search_by_sim3.argtypes = side + side + [vp, vp, vp, vp, i32, f32, i32, vp, vp, vp, vp, vp, vp]
        L.s3r_search_by_sim3.restype = None
        L.s3r_features_in_area.argtypes = [vp, i32, vp, f32, f32, f32, vp]
        L._msim3 = True
    args = []
    for s in (0, 1):
        args += [_p(w.kps[s]), _p(w.desc[s]), n[s], _p(w.points[s]), _p(w.mask[s]) if w.mask else None,
                 _p(w.pdesc[s]) if w.pdesc else None, _p(w.dist[s]), _p(w.pose[s])]
    L.s3r_search_by_sim3(*args, _p(w.sim), _p(w.K), _p(b), _p(sc), len(sc), np.float32(th), int(orb_dist), _p(m), _p(res), _p(vn1),
                         _p(vn2), _p(pr1), _p(pr2))
    if n != [int(v) for v in w.n]:
        res["status"] |= MSIM3_BAD_INPUT
    return dict(matches=m, res=res[0].copy(), vn1=vn1, vn2=vn2, proj1=pr1, proj2=pr2)


def features_in_area_nolevels(kps, bounds, x, y, r):
    """The restatement's KeyFrame::GetFeaturesInArea (no level bounds) -> indices in its order."""
    search_by_sim3(MWorld(1))  # (binds the symbols)
    k, b = np.ascontiguousarray(kps, KEYPOINT_DTYPE), np.array(bounds, np.int32)
    out = np.zeros(max(len(k), 1), np.int32)
    n = lib().s3r_features_in_area(_p(k), len(k), _p(b), np.float32(x), np.float32(y), np.float32(r), _p(out))
    return out[:n].copy()


def project(K, Y):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return np.c_[K[0, 0] * Y[:, 0] / Y[:, 2] + K[0, 2], K[1, 1] * Y[:, 1] / Y[:, 2] + K[1, 2]]


def make_match_world(n, seed=0, cap=None, extra=20, matched=0.4, s=1.3, rot=(0.03, -0.05, 0.02), t=(0.2, -0.1, 0.3), pdesc=False,
                     noise_bits=0, K=None, scale_factor=1.2, nlevels=NLEVELS):
    """A truth world: n physical points seen by both keyframes, Y1 = s R Y2 + t between the camera frames; each keyframe has a
    feature at the point's projection (exact descriptor copies, `noise_bits` flipped in KF2's) and the point in its own map;
    the distances are set so that PredictScale returns the features' octave.  A fraction `matched` of the pairs is already in
    the row (the solver's inliers); `extra` features per keyframe have no point.  KF2 holds its features in a permuted order."""
    rng = np.random.default_rng(25000 + seed)
    Rt, tt, st = P.rotvec(rot), np.array(t, np.float64), float(s)
    z = rng.uniform(4, 20, n)
    Y2 = np.c_[rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.3, 0.3, n) * z, z]
    Y1 = st * Y2 @ Rt.T + tt
    nf = n + extra
    cap = int(cap or nf)
    w = MWorld(cap, K=K, pdesc=pdesc)
    if (scale_factor, nlevels) != (1.2, NLEVELS):
        w.scale = scale_table(nlevels, scale_factor)
    R1, t1 = P.rotvec((0.2, -0.1, 0.05)), np.array([0.5, -1.0, 2.0])
    R2, t2 = P.rotvec((-0.1, 0.3, 0.1)), np.array([-1.5, 0.4, 1.0])
    w.pose = [np.r_[R1.reshape(9), t1].astype(np.float32), np.r_[R2.reshape(9), t2].astype(np.float32)]
    w.sim = np.r_[Rt.reshape(9), tt, st].astype(np.float32)
    X = [(Y1 - t1) @ R1, (Y2 - t2) @ R2]
    uv = [project(w.K, Y1), project(w.K, Y2)]
    lev = rng.integers(0, nlevels, n)
    desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    slots = [np.sort(rng.permutation(nf)[:n]), rng.permutation(nf)[:n]]
    sc = scale_table(nlevels, scale_factor).astype(np.float64)
    for side, other_depth in ((0, np.linalg.norm(Y2, axis=1)), (1, np.linalg.norm(Y1, axis=1))):
        k = w.kps[side]
        k["x"][:nf], k["y"][:nf], k["octave"][:nf] = rng.uniform(0, 640, nf), rng.uniform(0, 480, nf), rng.integers(0, nlevels, nf)
        w.desc[side][:nf] = rng.integers(0, 256, (nf, 32))
        sl = slots[side]
        k["x"][sl], k["y"][sl], k["octave"][sl] = uv[side][:, 0], uv[side][:, 1], lev
        d = desc.copy()
        if side == 1 and noise_bits:
            for row in d:
                for bit in rng.choice(256, noise_bits, replace=False):
                    row[bit // 8] ^= 1 << (bit % 8)
        if pdesc:  # the points carry the descriptors; the features of KF1 / the points' own features hold something else
            w.pdesc[side][sl] = d
            w.desc[side][sl] = d if side == 1 else rng.integers(0, 256, (n, 32))
        else:
            w.desc[side][sl] = d
        w.points[side][sl] = X[side]
        max_d = other_depth * sc[lev] * 0.95  # the distance in the OTHER camera decides the level there
        w.dist[side][sl] = np.c_[0.3 * other_depth, max_d]
        w.mask[side][sl] = 1
        w.n[side] = nf
    if pdesc:  # both directions compare a point's descriptor with the other keyframe's FEATURES: those hold the copies
        w.desc[0][slots[0]] = desc
    have = rng.random(n) < matched
    w.match[slots[0][have]] = slots[1][have]
    w.truth = dict(slots1=slots[0], slots2=slots[1], have=have, lev=lev)
    return w
