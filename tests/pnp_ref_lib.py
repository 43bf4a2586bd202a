"""ctypes wrapper around tests/cpp/pnp_ref.cpp -- the CPU restatement of PnPsolver (include/orbx.h, "behind SearchByBoW: PnP
RANSAC") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary directory, as tests/pose_ref_lib.py
compiles its source; SetRansacParameters' table evaluated directly in Python; a literal swap-and-pop sampler on a real list; a
second, independently written numpy EPnP (numpy.linalg.eigh / svd / lstsq, nothing shared with the C++); and the worlds that
tests/test_pnp_host.py and tests/test_gpu_pnp.py share (pose_ref_lib.make_world's scenes).  TEST INFRASTRUCTURE only."""
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
from pose_ref_lib import K_ANISO, MOTION_2, NLEVELS_2, SCALE_FACTOR_2, SECOND, SETTINGS  # noqa: F401 (the second setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pnp_ref.cpp")
KEYPOINT_DTYPE = P.KEYPOINT_DTYPE
PNP_INTS = ("status", "n_correspondences", "min_inliers", "max_its", "its_run", "found_it", "best_it", "refined", "n_inliers",
            "n_best_inliers", "n_refines", "n_degenerate", "beta_choice", "reserved")
PNP_RESULT_DTYPE = np.dtype([(n, "<i4") for n in PNP_INTS] + [("R", "<f8", (3, 3)), ("t", "<f8", 3), ("Tcw", "<f4", 12)])
assert PNP_RESULT_DTYPE.itemsize == 200
BAD_INPUT, NONFINITE, FEW_POINTS, BAD_DRAWS, NO_POSE = 2, 4, 8, 16, 32
RAND_MAX = 2147483647
NLEVELS = P.NLEVELS
# the reference's SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
PARAMS = dict(probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5, th2=5.991)
_L = None


def build(src=SRC) -> ctypes.CDLL:
    """Compiles a restatement source (lib(): the committed one; tests/test_camera_mutants_host.py: an altered copy) and binds it."""
    d = tempfile.mkdtemp(prefix="pnp_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libpnp_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", src, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("pnp_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.pnr_solve.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, f32, i32, vp, i32, vp, vp, vp, vp]
    L.pnr_solve.restype = None
    L.pnr_sample.argtypes = [vp, i32, vp]
    L.pnr_epnp.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    return L


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        _L = build()
    return _L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def sigma2_table(nlevels: int = NLEVELS, scale_factor: float = 1.2) -> np.ndarray:
    """mvLevelSigma2 as ORBextractor's constructor computes it (f32)."""
    f32 = np.float32
    scale, out = f32(1.0), np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        scale = f32(scale * f32(scale_factor))
        out[i] = f32(scale * scale)
    return out


def ransac_entry(N, probability=0.99, min_inliers=10, max_iterations=300, epsilon=0.5):
    """SetRansacParameters for one N, evaluated directly with the reference's expression types -> (mRansacMinInliers,
    mRansacMaxIts).  N < mRansacMinInliers (bNoMore before anything iterates; the reference takes log of a negative number there,
    and divides by N = 0) is given max_iterations."""
    f32 = np.float32
    eps = f32(epsilon)
    n_min = max(int(f32(N) * eps), int(min_inliers), 4)
    nd = max(int(N), 1)
    if eps < f32(n_min) / f32(nd):
        eps = f32(n_min) / f32(nd)
    if n_min == nd:
        its = 1
    elif nd < n_min:
        its = max_iterations
    else:
        its = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3)))
    return n_min, max(1, min(its, int(max_iterations)))


_tables = {}


def ransac_table(n_max, **kw) -> np.ndarray:
    """[n_max + 1, 2] int32, made once per parameter set."""
    key = (n_max,) + tuple(sorted((k, v) for k, v in kw.items() if k != "th2"))
    if key not in _tables:
        _tables[key] = np.array([ransac_entry(N, **dict(key[1:])) for N in range(n_max + 1)], np.int32)
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
    """The restatement's sampler -> the four picks, or None for a draw out of range."""
    d, sel = np.ascontiguousarray(draws, np.int32), np.zeros(4, np.int32)
    return list(sel) if lib().pnr_sample(_p(d), int(N), _p(sel)) else None


def make_draws(n_iter, seed=0):
    """rand() values for n_iter hypotheses."""
    return np.random.default_rng(31000 + seed).integers(0, RAND_MAX + 1, (n_iter, 4)).astype(np.int32)


def solve(w: P.World, draws, mode=0, sigma2=None, nlevels=NLEVELS, **params):
    """The restatement for one problem -> (PNP_RESULT_DTYPE record, pose [12] f32, row [cap] i32, inliers [cap] u8).  mode 0:
    the literal sequential loop; mode 1: all hypotheses, then the distinct bests in order."""
    prm = dict(PARAMS, **params)
    sig = np.ascontiguousarray(sigma2_table(nlevels) if sigma2 is None else sigma2, np.float32)
    table = np.ascontiguousarray(ransac_table(w.cap, **prm))
    draws = np.ascontiguousarray(draws, np.int32)
    res, pose = np.zeros(1, PNP_RESULT_DTYPE), np.zeros(12, np.float32)
    row, inl = np.zeros(w.cap, np.int32), np.zeros(w.cap, np.uint8)
    lib().pnr_solve(_p(w.kps), w.n, w.cap, _p(w.match), _p(w.points), _p(w.mask), _p(w.K), _p(sig), len(sig), _p(table),
                    np.float32(prm["th2"]), len(draws), _p(draws), int(mode), _p(res), _p(pose), _p(row), _p(inl))
    return res[0].copy(), pose, row, inl


def epnp(w: P.World, use, sigma2=None, nlevels=NLEVELS):
    """The restatement's compute_pose over the features flagged in use [cap] -> (choice, R, t); choice 0 / -1: none."""
    sig = np.ascontiguousarray(sigma2_table(nlevels) if sigma2 is None else sigma2, np.float32)
    use = np.ascontiguousarray(use, np.uint8)
    R, t = np.zeros(9), np.zeros(3)
    c = lib().pnr_epnp(_p(w.kps), w.n, w.cap, _p(w.match), _p(w.points), _p(w.mask), _p(w.K), _p(sig), len(sig), _p(use), _p(R), _p(t))
    return c, R.reshape(3, 3), t


def max_error(w: P.World, j, th2=5.991, sigma2=None):
    return ((sigma2_table() if sigma2 is None else sigma2)[w.kps["octave"][j]] * np.float32(th2)).astype(np.float32)


def error2(w: P.World, R, t, j=None):
    """CheckInliers' error2 (in f64) of the features j (default: every correspondence) at the pose (R, t) -> (j, error2)."""
    jj, ii = w.edges()
    if j is not None:
        keep = np.isin(jj, j)
        jj, ii = jj[keep], ii[keep]
    K = w.K.reshape(3, 3).astype(np.float64)
    Y = w.points[ii].astype(np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    ue, ve = K[0, 2] + K[0, 0] * Y[:, 0] / Y[:, 2], K[1, 2] + K[1, 1] * Y[:, 1] / Y[:, 2]
    return jj, (w.kps["x"][jj] - ue) ** 2 + (w.kps["y"][jj] - ve) ** 2


# ---- the second statement: EPnP in numpy; nothing shared with the C++ ----

def _rt_numpy(X, obs, K, alphas, ccs):
    pcs = alphas @ ccs
    if pcs[0, 2] < 0:
        ccs, pcs = -ccs, -pcs
    pc0, pw0 = pcs.mean(0), X.mean(0)
    U, _, Vt = np.linalg.svd((pcs - pc0).T @ (X - pw0))
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R[2] = -R[2]
    t = pc0 - R @ pw0
    Y = X @ R.T + t
    proj = np.c_[K[0, 2] + K[0, 0] * Y[:, 0] / Y[:, 2], K[1, 2] + K[1, 1] * Y[:, 1] / Y[:, 2]]
    return R, t, float(np.sqrt(((obs - proj) ** 2).sum(1)).mean())


def epnp_numpy(w: P.World, use, signs=(1, 1, 1)):
    """EPnP over the features flagged in use -> (R, t, choice).  signs: of the three eigenvectors the control points are built
    from.  With noise EPnP's answer depends on them beyond rounding, and an eigen-solver is free to choose them."""
    jj, ii = w.edges()
    keep = np.asarray(use)[jj] != 0
    jj, ii = jj[keep], ii[keep]
    X = w.points[ii].astype(np.float64)
    obs = np.c_[w.kps["x"][jj], w.kps["y"][jj]].astype(np.float64)
    K = w.K.reshape(3, 3).astype(np.float64)
    n = len(X)
    c0 = X.mean(0)
    lam, vec = np.linalg.eigh((X - c0).T @ (X - c0))
    cws = np.vstack([c0] + [c0 + sg * np.sqrt(max(lam[k], 0) / n) * vec[:, k] for sg, k in zip(signs, (2, 1, 0))])
    a123 = np.linalg.solve((cws[1:] - cws[0]).T, (X - c0).T).T
    alphas = np.c_[1 - a123.sum(1), a123]
    M = np.zeros((2 * n, 12))
    for i in range(4):
        M[0::2, 3 * i] = alphas[:, i] * K[0, 0]
        M[0::2, 3 * i + 2] = alphas[:, i] * (K[0, 2] - obs[:, 0])
        M[1::2, 3 * i + 1] = alphas[:, i] * K[1, 1]
        M[1::2, 3 * i + 2] = alphas[:, i] * (K[1, 2] - obs[:, 1])
    # (the right singular vectors of M itself: M^T M squares the condition number, and LAPACK's eigh then loses the small end)
    _, _, Vt = np.linalg.svd(M)
    v = [Vt[11 - k].reshape(4, 3) for k in range(4)]  # descending singular values: v[0] is ut's row 11
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = [[v[i][a] - v[i][b] for a, b in pairs] for i in range(4)]
    order = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3)]
    L = np.array([[(1 if a == b else 2) * dv[a][r] @ dv[b][r] for a, b in order] for r in range(6)])
    rho = np.array([((cws[a] - cws[b]) ** 2).sum() for a, b in pairs])

    def start(cols):
        x = np.linalg.lstsq(L[:, cols], rho, rcond=None)[0]
        b = np.zeros(4)
        if len(cols) == 4:
            s = -1.0 if x[0] < 0 else 1.0
            b[0] = np.sqrt(s * x[0])
            b[1:] = s * x[1:] / b[0]
        else:
            s = -1.0 if x[0] < 0 else 1.0
            b[0] = np.sqrt(s * x[0])
            b[1] = np.sqrt(s * x[2]) if s * x[2] > 0 else 0.0
            if x[1] < 0:
                b[0] = -b[0]
            if len(cols) == 5:
                b[2] = x[3] / b[0]
        return b

    best = None
    for choice, cols in enumerate(([0, 1, 3, 6], [0, 1, 2], [0, 1, 2, 3, 4]), 1):
        b = start(cols)
        for _ in range(5):
            bb = np.array([b[a] * b[c] for a, c in order])
            J = np.zeros((6, 4))
            for k, (a, c) in enumerate(order):
                J[:, a] += L[:, k] * b[c]
                J[:, c] += L[:, k] * b[a]
            b = b + np.linalg.lstsq(J, rho - L @ bb, rcond=None)[0]
        ccs = sum(b[i] * v[i] for i in range(4))
        R, t, err = _rt_numpy(X, obs, K, alphas, ccs)
        if best is None or err < best[3]:
            best = (R, t, choice, err)
    return best[0], best[1], best[2]


def closest_numpy(w: P.World, use, R, t):
    """epnp_numpy under the signs that come closest to the pose (R, t) -> (angle, relative translation) of the difference."""
    best = None
    for k in range(8):
        R2, t2, _ = epnp_numpy(w, use, tuple(-1.0 if k >> b & 1 else 1.0 for b in range(3)))
        d = pose_difference(R, t, R2, t2)
        if best is None or d[0] + d[1] < best[0] + best[1]:
            best = d
    return best


def pose_difference(R1, t1, R2, t2):
    """(rotation angle between the two in radians, as |R1 - R2|_F / sqrt(2): exact for small angles, where arccos of the trace
    loses half the digits; |t1 - t2| / |t2|)."""
    return (float(np.linalg.norm(np.asarray(R1) - np.asarray(R2)) / np.sqrt(2)),
            float(np.linalg.norm(np.asarray(t1) - t2) / np.linalg.norm(t2)))


# The restatement's Refine against epnp_numpy over the same inlier sets, on the worlds of test_pnp_host.NUMPY_WORLDS, under the
# control points' signs that come closest.  Measured on the development machine (x86-64, glibc, numpy on OpenBLAS): the largest
# rotation difference 2.52e-15 rad, the largest relative translation difference 6.84e-14.  The limits are ten times that, room
# for another libm or LAPACK: the two statements differ by rounding and by eigen-solver only.
NUMPY_ANGLE_MEASURED, NUMPY_ANGLE_LIMIT = 2.52e-15, 2.52e-14  # radians
NUMPY_TRANS_MEASURED, NUMPY_TRANS_LIMIT = 6.84e-14, 6.84e-13  # relative
# The same measurement on test_pnp_host.NUMPY_WORLDS_2, the worlds of the second setting (the largest of both: mixed411@2; the
# other five stay below 2.5e-15 rad and 8.8e-14), with the same margin of ten.
NUMPY_ANGLE_MEASURED_2, NUMPY_ANGLE_LIMIT_2 = 1.68e-14, 1.68e-13  # radians
NUMPY_TRANS_MEASURED_2, NUMPY_TRANS_LIMIT_2 = 1.89e-13, 1.89e-12  # relative


# ---- worlds ----

def make_world(n, seed=0, **kw):
    """pose_ref_lib.make_world's scene; the start pose it carries is not used."""
    return P.make_world(n, seed, **kw)


def planar_world(n, seed=0, cap=None, **kw):
    """Every map point in the plane z = 0 of the world frame."""
    w = P.make_world(n, seed, cap=cap, noise=0.0, **kw)
    rng = np.random.default_rng(12000 + seed)
    R, t = w.truth["R"], w.truth["t"]
    K = w.K.reshape(3, 3).astype(np.float64)
    jj, ii = w.edges()
    X = np.c_[rng.uniform(-3, 3, len(ii)), rng.uniform(-2, 2, len(ii)), np.zeros(len(ii))]
    Xw = (X + np.array([0, 0, 8.0]) - t) @ R  # the plane 8 units in front of the camera, slanted by R
    Y = Xw @ R.T + t
    w.points[ii] = Xw.astype(np.float32)
    Y = w.points[ii].astype(np.float64) @ R.T + t
    w.kps["x"][jj] = (Y[:, 0] / Y[:, 2] * K[0, 0] + K[0, 2]).astype(np.float32)
    w.kps["y"][jj] = (Y[:, 1] / Y[:, 2] * K[1, 1] + K[1, 2]).astype(np.float32)
    return w


def same_point_world(n, seed=0, copies=6, cap=None):
    """`copies` features of the frame matched to one map point (a match-row world): draws that pick four of them give EPnP four
    equal points."""
    w = P.make_world(n, seed, cap=cap, noise=0.0, matched=True)
    jj, ii = w.edges()
    w.match[jj[:copies]] = ii[0]
    return w
