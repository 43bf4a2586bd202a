"""ctypes wrapper around tests/cpp/init_ref.cpp -- the CPU restatement of the RANSAC stage of Initializer::Initialize
(orbx_find_models), compiled on first use with g++ -O2 -ffp-contract=off into a private temporary directory.  Scoring goes
through the oracle's CheckHomography / CheckFundamental (oracle/liborbx_oracle.so).  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "init_ref.cpp")
KP = oracle_lib.KP
_L = None


def lib() -> ctypes.CDLL:
    global _L
    if _L is not None:
        return _L
    d = tempfile.mkdtemp(prefix="init_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libinit_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", SRC, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("init_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.ir_eigen_inverse.argtypes = [vp, vp]
    L.ir_eigen_inverse.restype = None
    L.ir_jacobi_smallest.argtypes = [i32, vp, vp]
    L.ir_solve_h.argtypes = [vp, vp, vp, vp, vp]
    L.ir_solve_f.argtypes = [vp, vp, vp, vp]
    L.ir_find_models.argtypes = [vp, i32, vp, i32, vp, i32, vp, f32, vp, vp, vp, vp, vp, vp, vp]
    L.ir_find_models.restype = None
    L.ir_sample_sets.argtypes = [ctypes.c_uint, i32, i32, vp]
    L.ir_sample_sets.restype = None
    L.ir_reconstruct_rules.argtypes = [i32, vp, vp, i32, f32, i32, vp, vp]
    _L = L
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def solve_h(src, dst):
    """-> (ok, H as f64 [3, 3] scaled to H22 = 1, H21 f32, H12 f32)."""
    src, dst = np.ascontiguousarray(src, np.float32).reshape(8, 2), np.ascontiguousarray(dst, np.float32).reshape(8, 2)
    Md, H21, H12 = np.zeros(9), np.zeros(9, np.float32), np.zeros(9, np.float32)
    ok = lib().ir_solve_h(_p(src), _p(dst), _p(Md), _p(H21), _p(H12))
    return bool(ok), Md.reshape(3, 3), H21.reshape(3, 3), H12.reshape(3, 3)


def solve_f(src, dst):
    """-> (ok, F as f64 [3, 3], F21 f32)."""
    src, dst = np.ascontiguousarray(src, np.float32).reshape(8, 2), np.ascontiguousarray(dst, np.float32).reshape(8, 2)
    Md, F21 = np.zeros(9), np.zeros(9, np.float32)
    ok = lib().ir_solve_f(_p(src), _p(dst), _p(Md), _p(F21))
    return bool(ok), Md.reshape(3, 3), F21.reshape(3, 3)


def eigen_inverse(m):
    m = np.ascontiguousarray(m, np.float32).reshape(9)
    r = np.zeros(9, np.float32)
    lib().ir_eigen_inverse(_p(m), _p(r))
    return r.reshape(3, 3)


def jacobi_smallest(A):
    A = np.ascontiguousarray(A, np.float64)
    v = np.zeros(len(A))
    tiny = lib().ir_jacobi_smallest(len(A), _p(A), _p(v))
    return v, tiny


def find_models(k1, k2, matches12, sets, sigma=1.0):
    """The restated stage for one pair -> (result dict with the fields of orbx_hf_result, inliers [2, N] bool,
    models [3, n_iter, 3, 3] (H21, H12, F21), scores [2, n_iter])."""
    k1, k2 = np.ascontiguousarray(k1, KP), np.ascontiguousarray(k2, KP)
    m12 = np.ascontiguousarray(matches12, np.int32)
    sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
    n_iter = len(sets)
    O = oracle_lib.lib()
    ri, rf = np.zeros(8, np.int32), np.zeros(30, np.float32)
    inl = np.zeros((2, max(len(k1), 1)), np.uint8)
    models = np.zeros((3, n_iter, 3, 3), np.float32)
    scores = np.zeros((2, n_iter), np.float32)
    chkH = ctypes.cast(O.orbo_check_homography, ctypes.c_void_p)
    chkF = ctypes.cast(O.orbo_check_fundamental, ctypes.c_void_p)
    lib().ir_find_models(_p(k1), len(k1), _p(k2), len(k2), _p(m12), n_iter, _p(sets), float(sigma), chkH, chkF, _p(ri), _p(rf),
                         _p(inl), _p(models), _p(scores))
    names = ("status", "model", "n_matches", "best_it_h", "best_it_f", "n_inliers_h", "n_inliers_f")
    res = {n: int(ri[i]) for i, n in enumerate(names)}
    res.update(score_h=np.float32(rf[0]), score_f=np.float32(rf[1]), rh=np.float32(rf[2]), H21=rf[3:12].reshape(3, 3),
               H12=rf[12:21].reshape(3, 3), F21=rf[21:30].reshape(3, 3))
    inl2 = np.zeros((2, len(k1)), np.uint8) if len(k1) == 0 else inl[:, :len(k1)]
    return res, inl2[:, :res["n_matches"]].astype(bool), models, scores


def sample_sets_cpp(seed, n_matches, n_iter):
    """mvSets drawn by the reference's own loop (Initializer.cpp:50-63) after srand(seed)."""
    out = np.zeros((n_iter, 8), np.int32)
    lib().ir_sample_sets(seed, n_matches, n_iter, _p(out))
    return out


def exact_homography_case(seed):
    """8 correspondences under a projective H whose images are exact in f32: dyadic entries, points chosen so that the third
    coordinate is a power of two.  -> (H f64, src [8, 2] f32, dst [8, 2] f32)."""
    rng = np.random.default_rng(seed)
    H = np.array([[1.25, 0.125, 16], [-0.25, 1.5, 8], [1 / 512, 1 / 1024, 1.0]])
    H[:2, :2] += rng.integers(-4, 5, (2, 2)) / 64
    w = rng.choice([0.5, 1, 2, 4], 8)
    y = rng.integers(-200, 200, 8) * 2.0
    x = 512 * (w - 1) - y / 2
    src = np.c_[x, y]
    p = np.c_[src, np.ones(8)] @ H.T
    dst = p[:, :2] / p[:, 2:]
    assert np.array_equal(dst.astype(np.float32).astype(np.float64), dst)
    return H, src.astype(np.float32), dst.astype(np.float32)


def exact_fundamental_case(seed):
    """8 correspondences of a rectified stereo pair (y2 == y1, x2 = x1 - disparity, all exact in f32): F = [e]x with
    e = (1, 0, 0), i.e. F ~ [[0, 0, 0], [0, 0, -1], [0, 1, 0]].  -> (F f64 unit norm, src, dst)."""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(0, 640, 8).astype(np.float32)
    y1 = rng.uniform(0, 480, 8).astype(np.float32)
    d = rng.uniform(5, 300, 8).astype(np.float32)  # a wide range of depths: a well-conditioned 8-point system
    F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0.0]]) / np.sqrt(2)
    return F, np.c_[x1, y1], np.c_[(x1 - d).astype(np.float32), y1]


def decompose_essential(F, K):
    """cv::decomposeEssentialMat(K^T F K) as restated -> (R [4, 3, 3], t [4, 3]) in the order of Initializer.cpp:458-466."""
    L = lib()
    L.ir_decompose_essential.argtypes = [ctypes.c_void_p] * 4
    F, K = np.ascontiguousarray(F, np.float32).reshape(9), np.ascontiguousarray(K, np.float32).reshape(9)
    R, t = np.zeros((4, 9), np.float32), np.zeros((4, 3), np.float32)
    n = L.ir_decompose_essential(_p(F), _p(K), _p(R), _p(t))
    return R[:n].reshape(-1, 3, 3), t[:n]


def decompose_homography(H, K):
    """cv::decomposeHomographyMat(H, K) as restated -> (R [n, 3, 3], t/d [n, 3], normal [n, 3])."""
    L = lib()
    L.ir_decompose_homography.argtypes = [ctypes.c_void_p] * 5
    H, K = np.ascontiguousarray(H, np.float32).reshape(9), np.ascontiguousarray(K, np.float32).reshape(9)
    R, t, nrm = np.zeros((4, 9), np.float32), np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    n = L.ir_decompose_homography(_p(H), _p(K), _p(R), _p(t), _p(nrm))
    return R[:n].reshape(-1, 3, 3), t[:n], nrm[:n]


_INIT_INTS = ("status", "model", "n_matches", "best_it_h", "best_it_f", "n_inliers_h", "n_inliers_f", "n_solutions", "best_solution",
              "best_good", "second_good")


def initialize(k1, k2, matches12, sets, K, sigma=1.0, min_parallax=1.0, min_triangulated=50):
    """The restated Initializer::Initialize for one pair -> (result dict with orbx_init_result's fields, p3d [n1, 3], tri [n1])."""
    k1, k2 = np.ascontiguousarray(k1, KP), np.ascontiguousarray(k2, KP)
    m12 = np.ascontiguousarray(matches12, np.int32)
    sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
    Kf = np.ascontiguousarray(K, np.float32).reshape(9)
    O = oracle_lib.lib()
    L = lib()
    L.ir_initialize.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 7
    L.ir_initialize.restype = None
    ri, rf = np.zeros(12, np.int32), np.zeros(34, np.float32)
    p3d, tri = np.zeros((max(len(k1), 1), 3), np.float32), np.zeros(max(len(k1), 1), np.uint8)
    fp = [ctypes.cast(getattr(O, n), ctypes.c_void_p) for n in ("orbo_check_homography", "orbo_check_fundamental", "orbo_check_rt")]
    L.ir_initialize(_p(k1), len(k1), _p(k2), len(k2), _p(m12), len(sets), _p(sets), _p(Kf), float(sigma), float(min_parallax),
                    int(min_triangulated), *fp, _p(ri), _p(rf), _p(p3d), _p(tri))
    res = {n: int(ri[i]) for i, n in enumerate(_INIT_INTS)}
    res.update(score_h=np.float32(rf[0]), score_f=np.float32(rf[1]), rh=np.float32(rf[2]), parallax=np.float32(rf[3]),
               R21=rf[4:13].reshape(3, 3), t21=rf[13:16].copy(), H21=rf[16:25].reshape(3, 3), F21=rf[25:34].reshape(3, 3))
    return res, p3d[:len(k1)], tri[:len(k1)].astype(bool)


def planar_case(seed=0, n=400, noise=0.3, outliers=0.1):
    """A planar scene: points on the plane n.X = d in front of camera 1, camera 2 = (R, t).  -> (K, R, t, n, d, k1, k2, matches12)."""
    rng = np.random.default_rng(seed)
    K = np.array([[609.2855, 0, 351.4274], [0, 609.3422, 237.7324], [0, 0, 1.0]])
    ang = np.deg2rad(rng.uniform(2, 6, 3)) * rng.choice([-1, 1], 3)
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    t = rng.normal(0, 1, 3); t /= np.linalg.norm(t)
    nrm = np.array([0.15, -0.1, -1.0]); nrm /= np.linalg.norm(nrm)
    d = 8.0
    xy = np.stack([rng.uniform(-5, 5, n), rng.uniform(-4, 4, n)], 1)
    z = (d + nrm[0] * xy[:, 0] + nrm[1] * xy[:, 1]) / -nrm[2]   # n.X = -d with n_z < 0 -> points at depth ~ d
    X = np.c_[xy, z]
    p1 = (K @ X.T).T; p1 = p1[:, :2] / p1[:, 2:]
    X2 = (R @ X.T).T + t
    p2 = (K @ X2.T).T; p2 = p2[:, :2] / p2[:, 2:]
    k1, k2 = np.zeros(n, KP), np.zeros(n, KP)
    k1["x"], k1["y"] = (p1[:, 0] + rng.normal(0, noise, n)).astype(np.float32), (p1[:, 1] + rng.normal(0, noise, n)).astype(np.float32)
    k2["x"], k2["y"] = (p2[:, 0] + rng.normal(0, noise, n)).astype(np.float32), (p2[:, 1] + rng.normal(0, noise, n)).astype(np.float32)
    m12 = np.arange(n, dtype=np.int32)
    wrong = rng.random(n) < outliers
    m12[wrong] = rng.integers(0, n, wrong.sum())
    return K, R, t, nrm, d, k1, k2, m12, X


def reconstruct_rules(n_good, parallax, n_inliers, min_parallax=1.0, min_triangulated=50):
    """orbx_init_decomp.inc's reconstructRules as compiled into the restatement -> (status bits, bestIdx, bestGood, secondGood,
    bestParallax f32); one entry of n_good / parallax per candidate (0, 1 or 4 of them)."""
    ng, par = np.ascontiguousarray(n_good, np.int32), np.ascontiguousarray(parallax, np.float32)
    io, bp = np.zeros(3, np.int32), np.zeros(1, np.float32)
    st = lib().ir_reconstruct_rules(len(ng), _p(ng), _p(par), int(n_inliers), float(min_parallax), int(min_triangulated), _p(io), _p(bp))
    return int(st), int(io[0]), int(io[1]), int(io[2]), bp[0]


def rotation_case(seed=3, n=500):
    """A pure rotation: frame 1 of oracle_lib.two_view_case(seed, n), frame 2 its exact image under K R K^-1 (rounded to f32), every
    keypoint matched.  -> (K, R, k1, k2, matches12)."""
    K, Rm, _, k1, *_ = oracle_lib.two_view_case(seed=seed, n=n)
    H = K @ Rm @ np.linalg.inv(K)
    p = np.c_[k1["x"], k1["y"], np.ones(len(k1))] @ H.T
    k2 = k1.copy()
    k2["x"], k2["y"] = (p[:, 0] / p[:, 2]).astype(np.float32), (p[:, 1] / p[:, 2]).astype(np.float32)
    return K, Rm, k1, k2, np.arange(len(k1), dtype=np.int32)


def doubled(k1, k2, m12, seed, n_iter=200):
    """Every keypoint twice: frames k1 ++ k1 and k2 ++ k2, matches m12 ++ (m12 + len(k2)) with holes kept, so that position c of
    mvMatches12 (N/2 of them) has a copy at c + N/2.  mvSets are built, not drawn: four distinct positions and their copies, the eight
    indices permuted (seeded numpy generator).  Eight distinct indices over four distinct points: the homography solver is exact on
    them, the 8-point F sees a rank-4 system -- degenerate (two eigenvalues under DBL_EPSILON) or an arbitrary null vector that fits
    little else -- so SH > SF and the pair takes ReconstructHF's homography route.  -> (k1d, k2d, m12d, sets [n_iter, 8])."""
    m12 = np.asarray(m12, np.int32)
    k1d, k2d = np.concatenate([k1, k1]), np.concatenate([k2, k2])
    m12d = np.concatenate([m12, np.where(m12 >= 0, m12 + len(k2), -1)]).astype(np.int32)
    half = int((m12 >= 0).sum())
    rng = np.random.default_rng(seed)
    sets = np.zeros((n_iter, 8), np.int32)
    for it in range(n_iter):
        c = rng.choice(half, 4, replace=False)
        sets[it] = rng.permutation(np.concatenate([c, c + half]))
    return k1d, k2d, m12d, sets


# ---- the worlds of the Initializer's tests ---------------------------------------------------------------------------------------
# (name, generator, its arguments, doubled, seed, keep, n_iter).  generator: "planar" = planar_case, "two_view" =
# oracle_lib.two_view_case, "rotation" = rotation_case.  doubled: the pair goes through doubled() with `seed` for its numpy generator
# (ReconstructHF's homography route); otherwise mvSets are drawn as the reference draws them after srand(seed).  keep: only the first
# `keep` matches of the generator's matches12 stay (before doubling), which sets N = |mvMatches12| around the wave of 64.
# Every world has at most 250 positions (500 keypoints per frame once doubled) but f_rotation: it is the scene of
# test_pure_rotation_is_low_parallax unchanged, 500 positions, not doubled, so 500 keypoints per frame as well.
# tests/test_initializer_host.py::test_init_worlds_reach_every_branch asserts on the CPU what each of them reaches.
INIT_WORLDS = (
    # the homography route
    ("h_accept_i0", "planar", dict(seed=11, n=60, noise=0.3, outliers=0.0), True, 11, None, 200),
    ("h_accept_i1", "planar", dict(seed=3, n=30, noise=0.3, outliers=0.0), True, 3, None, 200),
    ("h_ambiguous_i2", "planar", dict(seed=1, n=30, noise=0.3, outliers=0.0), True, 1, None, 200),
    ("h_low_parallax", "planar", dict(seed=0, n=30, noise=0.3, outliers=0.0), True, 0, None, 200),
    ("h_few_triangulated", "planar", dict(seed=11, n=30, noise=1.0, outliers=0.0), True, 11, None, 200),
    ("h_few_inliers", "planar", dict(seed=11, n=30, noise=2.0, outliers=0.5), True, 11, None, 200),
    ("h_40", "planar", dict(seed=3, n=30, noise=1.0, outliers=0.3), True, 3, None, 200),
    ("h_56", "planar", dict(seed=6, n=30, noise=0.3, outliers=0.3), True, 6, None, 200),
    ("h_n128", "planar", dict(seed=11, n=64, noise=0.3, outliers=0.0), True, 11, None, 200),
    ("h_rotation", "rotation", dict(seed=0, n=30), True, 0, None, 200),
    ("tiny", "planar", dict(seed=11, n=60, noise=0.3, outliers=0.0), True, 5, 4, 3),
    # the fundamental route
    ("f_accept_n63", "two_view", dict(seed=3, n=70, outliers=0.0, noise=0.3), False, 0, None, 200),
    ("f_accept_200", "two_view", dict(seed=3, n=200, outliers=0.0, noise=0.3), False, 0, None, 200),
    ("f_n64", "two_view", dict(seed=3, n=200, outliers=0.0, noise=0.3), False, 0, 64, 200),
    ("f_n65", "two_view", dict(seed=3, n=200, outliers=0.0, noise=0.3), False, 0, 65, 200),
    ("f_ambiguous", "two_view", dict(seed=1, n=130, outliers=0.0, noise=0.3), False, 0, None, 200),
    ("f_low_parallax", "two_view", dict(seed=7, n=60, outliers=0.0, noise=0.3), False, 0, None, 200),
    ("f_few_triangulated", "two_view", dict(seed=3, n=60, outliers=0.2, noise=0.5), False, 0, None, 200),
    ("f_few_inliers", "two_view", dict(seed=3, n=250, outliers=0.2, noise=0.5), False, 0, None, 200),
    ("f_no_good_point", "planar", dict(seed=3, n=130, noise=0.3, outliers=0.0), False, 0, None, 200),
    ("f_104", "planar", dict(seed=0, n=60, noise=0.3, outliers=0.0), False, 0, None, 200),
    ("f_120", "planar", dict(seed=0, n=60, noise=0.3, outliers=0.3), False, 0, None, 200),
    ("f_rotation", "rotation", dict(seed=3, n=500), False, 0, None, 200),
)
_WORLDS = {}


def init_world(name):
    """The world `name` of INIT_WORLDS -> dict(K f32 [3, 3], k1, k2, m12, sets, doubled, truth); truth = (R, t, plane normal, plane
    distance) with None where the generator has none.  Built once and shared: do not write into it."""
    if name in _WORLDS:
        return _WORLDS[name]
    _, gen, args, dbl, seed, keep, n_iter = next(w for w in INIT_WORLDS if w[0] == name)
    if gen == "planar":
        K, Rm, t, nrm, d, k1, k2, m12, _ = planar_case(**args)
    elif gen == "two_view":
        K, Rm, t, k1, k2, m12, _ = oracle_lib.two_view_case(**args)
        nrm = d = None
    else:
        K, Rm, k1, k2, m12 = rotation_case(**args)
        t = nrm = d = None
    m12 = m12.astype(np.int32).copy()
    if keep is not None:
        m12[np.nonzero(m12 >= 0)[0][keep:]] = -1
    if dbl:
        k1, k2, m12, sets = doubled(k1, k2, m12, seed, n_iter)
    else:
        sets = sample_sets_cpp(seed, int((m12 >= 0).sum()), n_iter)
    w = dict(name=name, K=np.ascontiguousarray(K, np.float32), k1=k1, k2=k2, m12=m12, sets=sets, doubled=dbl, truth=(Rm, t, nrm, d))
    _WORLDS[name] = w
    return w


_REFS = {}


def init_reference(name):
    """The restatement's answer for the world `name` -> (result dict, p3d, tri), computed once and shared: do not write into it."""
    if name not in _REFS:
        w = init_world(name)
        _REFS[name] = initialize(w["k1"], w["k2"], w["m12"], w["sets"], w["K"])
    return _REFS[name]
