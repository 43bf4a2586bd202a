"""ctypes wrapper around tests/cpp/tri_ref.cpp -- the CPU restatement of LocalMapping::CreateNewMapPoints (include/orbx.h, "growing
the map": ORBmatcher::SearchForTriangulation and the triangulation of its matches) -- compiled on first use with g++ -O2
-ffp-contract=off into a private temporary directory, as tests/match_kfproj_ref_lib.py compiles its source; a second, independently
written numpy statement in f64 (the matcher by brute force over the node-equal pairs, the triangulation with np.linalg.svd); and the
worlds (two keyframes that see the same 3D points) that tests/test_tri_host.py and tests/test_gpu_tri.py share.  TEST INFRASTRUCTURE
only."""
from __future__ import annotations

import atexit
import ctypes
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

import match_proj_ref_lib as M
from pose_ref_lib import K_ANISO, NLEVELS_2, SCALE_FACTOR_2, SECOND, SETTINGS  # noqa: F401 (the second setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tri_ref.cpp")
KEYPOINT_DTYPE = M.KEYPOINT_DTYPE
MATCH_COUNTERS = ("status", "nmatches", "n_queries", "n_with_candidates", "n_epipole_rejected", "n_epiline_rejected", "n_rot_removed")
MATCH_RESULT_DTYPE = np.dtype([(n, "<i4") for n in MATCH_COUNTERS] + [("baseline", "<f4"), ("ex", "<f4"), ("ey", "<f4"), ("F12", "<f4", (9,))])
TRI_FIELDS = ("status", "n_matches", "n_points", "n_low_parallax", "n_w_zero", "n_behind_1", "n_behind_2", "n_reproj_1", "n_reproj_2",
              "n_zero_dist", "n_scale")
TRI_RESULT_DTYPE = np.dtype([(n, "<i4") for n in TRI_FIELDS])
BAD_INPUT, NONFINITE, LOW_BASELINE, ZERO_BASELINE = 2, 4, 8, 16
KEPT, LOW_PARALLAX, W_ZERO, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE = range(1, 10)
OUTCOME_FIELD = {KEPT: "n_points", LOW_PARALLAX: "n_low_parallax", W_ZERO: "n_w_zero", BEHIND_1: "n_behind_1", BEHIND_2: "n_behind_2",
                 REPROJ_1: "n_reproj_1", REPROJ_2: "n_reproj_2", ZERO_DIST: "n_zero_dist", SCALE: "n_scale"}
NLEVELS = M.NLEVELS
SCALE_FACTOR = 1.2
TH_LOW = 50
# a tested quantity within this relative distance of its threshold is "within rounding" for the f64 statement: the f32 chain behind
# F12 (three products with one rounding each, then a difference of terms of the size of a pixel coordinate) carries a relative
# error of up to some 1e-5 into a line's coefficients, 6e-3 px into a distance of 2 px, 6e-3 relative into its square
MARGIN = 1e-2
# ... and for the triangulation's gates, whose quantities come from x3D (f32, some 1e-6 of its norm from the f64 point): 1e-4 px in
# a reprojection of 2.4 px, 1e-6 in a ratio of distances
TRI_MARGIN = 1e-3
f32 = np.float32
_L = None


def build(src=SRC) -> ctypes.CDLL:
    """Compiles a restatement source (lib(): the committed one; tests/test_camera_mutants_host.py: an altered copy) and binds it."""
    d = tempfile.mkdtemp(prefix="tri_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libtri_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", src, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("tri_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.trr_search_for_triangulation.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, fl, vp, vp, i32,
                                               i32, i32, vp, vp]
    L.trr_search_for_triangulation.restype = None
    L.trr_triangulate_matches.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, fl, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.trr_triangulate_matches.restype = None
    L.trr_triangulate_one.argtypes = [vp, vp, vp, vp, vp, vp, vp, fl, fl, fl, fl, fl, fl, vp]
    return L


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        _L = build()
    return _L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


scale_table = M.scale_table


def sigma2_table(nlevels: int = NLEVELS, scale_factor: float = SCALE_FACTOR) -> np.ndarray:
    """mvLevelSigma2 as ORBextractor's constructor computes it (f32)."""
    s = scale_table(nlevels, scale_factor)
    return (s * s).astype(np.float32)


def pose12(R, C) -> np.ndarray:
    """Tcw [12] of a camera with rotation Rcw and centre C (f64 in, f32 out)."""
    R = np.asarray(R, np.float64)
    return np.r_[R.reshape(9), -R @ np.asarray(C, np.float64)].astype(np.float32)


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


class KeyFrame:
    """kps (undistorted), desc [n, 32], the FeatureVector (node, feat: ascending by node, then feature), mask (None or [n], != 0 =
    the feature has a map point), pose [12]."""

    def __init__(self, kps, desc, fv_node, fv_feat, pose, mask=None):
        self.kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE).reshape(-1)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.fv_node = np.ascontiguousarray(fv_node, np.uint32).reshape(-1)
        self.fv_feat = np.ascontiguousarray(fv_feat, np.uint32).reshape(-1)
        self.pose = np.ascontiguousarray(pose, np.float32).reshape(12)
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        self.n = len(self.kps)
        assert len(self.desc) == self.n and len(self.fv_node) == len(self.fv_feat)
        assert self.mask is None or len(self.mask) == self.n

    @classmethod
    def from_nodes(cls, kps, desc, nodes, pose, mask=None):
        """... with one node per feature (a negative node: the feature is in no FeatureVector entry)."""
        nodes = np.asarray(nodes, np.int64)
        feat = np.flatnonzero(nodes >= 0)
        order = np.lexsort((feat, nodes[feat]))
        return cls(kps, desc, nodes[feat][order], feat[order], pose, mask)


class World:
    """One pair (kf1, kf2), K [9], the orientation switch, the median depth of kf2's scene (None = no gate); truth (optional):
    {kf1 feature: (kf2 feature, X)}."""

    def __init__(self, kf1, kf2, K, ori=True, median=None, truth=None, scale_factor=SCALE_FACTOR, nlevels=NLEVELS):
        self.kf1, self.kf2 = kf1, kf2
        self.K = np.ascontiguousarray(K, np.float32).reshape(9)
        self.ori, self.median, self.truth = bool(ori), median, truth or {}
        self.scale, self.sigma2 = scale_table(nlevels, scale_factor), sigma2_table(nlevels, scale_factor)
        self.scale_factor, self.nlevels = float(f32(scale_factor)), nlevels
        self._expected = None

    def expected(self):
        """The restatement's answer for the chain (the matcher, then the triangulation of its rows), computed once."""
        if self._expected is None:
            m = search(self)
            t = triangulate(self, m["matches12"])
            self._expected = dict(match=m, tri=t)
        return self._expected


def search(w: World, cap=None, n1=None, n2=None, fvn1=None, fvn2=None):
    """The restatement's SearchForTriangulation -> dict(matches12 [cap], res: MATCH_RESULT_DTYPE record)."""
    a, b = w.kf1, w.kf2
    cap = int(cap if cap is not None else max(a.n, b.n, len(a.fv_node), len(b.fv_node), 1))
    m = np.full(cap, -7, np.int32)
    res = np.zeros(1, MATCH_RESULT_DTYPE)
    lib().trr_search_for_triangulation(_p(a.kps), _p(a.desc), a.n if n1 is None else n1, _p(a.fv_node), _p(a.fv_feat),
                                       len(a.fv_node) if fvn1 is None else fvn1, _p(a.mask), _p(a.pose), _p(b.kps), _p(b.desc),
                                       b.n if n2 is None else n2, _p(b.fv_node), _p(b.fv_feat), len(b.fv_node) if fvn2 is None else fvn2,
                                       _p(b.mask), _p(b.pose), _p(w.K), int(w.median is not None),
                                       float(w.median if w.median is not None else 0.0), _p(w.scale), _p(w.sigma2), w.nlevels,
                                       int(w.ori), cap, _p(m), _p(res))
    return dict(matches12=m, res=res[0])


def triangulate(w: World, matches12, cap=None, n1=None, n2=None):
    """The restatement's triangulation of matches12 -> dict(points, mask, normal, dist, res, outcome, x3d), arrays of cap rows."""
    a, b = w.kf1, w.kf2
    m = np.ascontiguousarray(matches12, np.int32)
    cap = int(cap if cap is not None else len(m))
    assert len(m) >= cap >= 1
    pts, msk, nrm, dst = np.zeros((cap, 3), f32), np.zeros(cap, np.uint8), np.zeros((cap, 3), f32), np.zeros((cap, 2), f32)
    out, x3d = np.zeros(cap, np.int32), np.zeros((cap, 3), f32)
    res = np.zeros(1, TRI_RESULT_DTYPE)
    lib().trr_triangulate_matches(_p(a.kps), a.n if n1 is None else n1, _p(a.pose), _p(b.kps), b.n if n2 is None else n2, _p(b.pose),
                                  _p(w.K), _p(w.scale), _p(w.sigma2), w.nlevels, w.scale_factor, _p(m), cap, _p(pts), _p(msk), _p(nrm),
                                  _p(dst), _p(res), _p(out), _p(x3d))
    return dict(points=pts, mask=msk, normal=nrm, dist=dst, res=res[0], outcome=out, x3d=x3d)


def triangulate_one(pose1, pose2, Ow1, Ow2, K, xy1, xy2, octave1=0, octave2=0):
    """triangulate() of orbx_tri_math.inc for one match with the camera centres given by the caller -> (outcome, X [3])."""
    a = [np.ascontiguousarray(v, np.float32) for v in (pose1, pose2, Ow1, Ow2, K, xy1, xy2)]
    sc, s2 = scale_table(), sigma2_table()
    pt = np.zeros(8, np.float32)
    o = lib().trr_triangulate_one(*[_p(v) for v in a], float(f32(5.991) * s2[octave1]), float(f32(5.991) * s2[octave2]), float(sc[octave1]),
                                  float(sc[octave2]), float(f32(1.5) * f32(SCALE_FACTOR)), float(sc[-1]), _p(pt))
    return int(o), pt[:3].copy()


# ---- the second statement: numpy, f64 ----

_ONES = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def _Rt(pose):
    p = np.asarray(pose, np.float64)
    return p[:9].reshape(3, 3), p[9:]


def geometry_numpy(w: World):
    """-> (F12 [3, 3], epipole (ex, ey), baseline), f64 from the f32 inputs, with np.linalg.inv for K."""
    R1, t1 = _Rt(w.kf1.pose)
    R2, t2 = _Rt(w.kf2.pose)
    K = np.asarray(w.K, np.float64).reshape(3, 3)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Kinv = np.linalg.inv(K)
    F12 = Kinv.T @ tx @ R12 @ Kinv
    O1, O2 = -R1.T @ t1, -R2.T @ t2
    with np.errstate(all="ignore"):
        C2 = K @ (R2 @ O1 + t2)
        e = C2[:2] / C2[2]
    return F12, e, float(np.linalg.norm(O2 - O1))


def search_numpy(w: World, given=None):
    """SearchForTriangulation by brute force over the node-equal pairs -> dict(matches12 [n1], res {counter: value}, borderline
    [(i, j)], candidates: the number of (i, j) tested).  A candidate pair whose epipole distance or line distance lies within MARGIN
    of its threshold is borderline: its verdict is taken from `given` {(i, j): 0 | 1 | 2} (the other statement's), which is how the
    comparison leaves it out; without `given` it gets this statement's own."""
    a, b = w.kf1, w.kf2
    F, e, _ = geometry_numpy(w)
    sc, s2 = w.scale.astype(np.float64), w.sigma2.astype(np.float64)
    m12 = np.full(a.n, -1, np.int64)
    res = dict.fromkeys(MATCH_COUNTERS, 0)
    borderline, n_cand = [], 0
    node_of_1 = {}
    for nd, ft in zip(a.fv_node.tolist(), a.fv_feat.tolist()):
        if ft < a.n:
            node_of_1.setdefault(nd, []).append(ft)
    node_of_2 = {}
    for nd, ft in zip(b.fv_node.tolist(), b.fv_feat.tolist()):
        if ft < b.n:
            node_of_2.setdefault(nd, []).append(ft)
    taken = np.zeros(b.n, bool)
    x1s = np.stack([a.kps["x"], a.kps["y"], np.ones(a.n)], 1).astype(np.float64) if a.n else np.zeros((0, 3))
    bad = False
    for nd in sorted(set(node_of_1) & set(node_of_2)):
        js = np.array(sorted(node_of_2[nd]), np.int64)
        for i in sorted(node_of_1[nd]):
            if a.mask is not None and a.mask[i]:
                continue
            res["n_queries"] += 1
            free = js[~taken[js]]
            if b.mask is not None:
                free = free[b.mask[free] == 0]
            if not len(free):
                continue
            d = _ONES[b.desc[free] ^ a.desc[i][None, :]].sum(axis=1, dtype=np.int64)
            near = d <= TH_LOW
            free, d = free[near], d[near]
            if not len(free):
                continue
            res["n_with_candidates"] += 1
            line = x1s[i] @ F
            best = None
            for j, dj in zip(free.tolist(), d.tolist()):
                o = int(b.kps["octave"][j])
                if o < 0 or o >= w.nlevels:
                    bad = True
                    continue
                n_cand += 1
                x2, y2 = float(b.kps["x"][j]), float(b.kps["y"][j])
                with np.errstate(all="ignore"):
                    de = (e[0] - x2) ** 2 + (e[1] - y2) ** 2
                    den = line[0] ** 2 + line[1] ** 2
                    dl = (line[0] * x2 + line[1] * y2 + line[2]) ** 2 / den if den > 0 else np.inf
                te, tl = 100.0 * sc[o], 3.84 * s2[o]
                verdict = 1 if de < te else (0 if dl < tl else 2)
                near_e = abs(de - te) <= MARGIN * te
                near_l = not de < te * (1 - MARGIN) and abs(dl - tl) <= MARGIN * tl
                if near_e or near_l:
                    borderline.append((i, j))
                    if given is not None:
                        verdict = given[(i, j)]
                if verdict == 1:
                    res["n_epipole_rejected"] += 1
                elif verdict == 2:
                    res["n_epiline_rejected"] += 1
                elif best is None or dj <= best[0]:  # (ascending j: among equals the last)
                    best = (dj, j)
            if best is not None:
                m12[i] = best[1]
                taken[best[1]] = True
    if w.ori:
        ii = np.flatnonzero(m12 >= 0)
        bins = np.full(a.n, -1, np.int64)
        for i in ii:
            r = f32(a.kps["angle"][i]) - f32(b.kps["angle"][m12[i]])
            if r < 0:
                r = f32(r + f32(360.0))
            x = float(f32(r * f32(f32(30) / f32(360.0))))
            if math.isfinite(x):
                k = int(M._round_half_away(x))
                k = 0 if k == 30 else k
                bins[i] = k if 0 <= k < 30 else -1
        size = np.bincount(bins[bins >= 0], minlength=30)
        top = sorted((k for k in range(30) if size[k] > 0), key=lambda k: (-size[k], k))[:3]
        keep = top[:1]
        if len(top) > 1 and not f32(size[top[1]]) < f32(f32(0.1) * f32(size[top[0]])):
            keep = top[:2]
            if len(top) > 2 and not f32(size[top[2]]) < f32(f32(0.1) * f32(size[top[0]])):
                keep = top[:3]
        for i in ii:
            if bins[i] >= 0 and bins[i] not in keep:
                m12[i] = -1
                res["n_rot_removed"] += 1
    res["nmatches"] = int((m12 >= 0).sum())
    res["status"] = BAD_INPUT if bad else 0
    return dict(matches12=m12.astype(np.int32), res=res, borderline=borderline, candidates=n_cand)


def verdicts(w: World, pairs):
    """The restatement's verdict (0 passes, 1 epipole, 2 line) for single (i, j) pairs: each as a world of its own with only these
    two features, in one node, without the orientation test."""
    out = {}
    for i, j in pairs:
        a = KeyFrame(w.kf1.kps[i:i + 1], np.zeros((1, 32), np.uint8), [1], [0], w.kf1.pose)
        b = KeyFrame(w.kf2.kps[j:j + 1], np.zeros((1, 32), np.uint8), [1], [0], w.kf2.pose)
        r = search(World(a, b, w.K, ori=False, nlevels=w.nlevels, scale_factor=w.scale_factor))["res"]
        out[(i, j)] = 1 if r["n_epipole_rejected"] else (2 if r["n_epiline_rejected"] else 0)
    return out


def triangulate_numpy(w: World, matches12):
    """The triangulation with np.linalg.svd in f64 -> dict(outcome [n1], points [n1, 3], normal, dist, borderline [i]): a match one
    of whose tested quantities lies within TRI_MARGIN of its threshold is borderline and carries outcome -1."""
    a, b = w.kf1, w.kf2
    R1, t1 = _Rt(a.pose)
    R2, t2 = _Rt(b.pose)
    fx, fy, cx, cy = (float(w.K[k]) for k in (0, 4, 2, 5))
    O1, O2 = -R1.T @ t1, -R2.T @ t2
    T1, T2 = np.c_[R1, t1], np.c_[R2, t2]
    sc, s2 = w.scale.astype(np.float64), w.sigma2.astype(np.float64)
    n1 = a.n
    outcome, pts = np.zeros(n1, np.int64), np.zeros((n1, 3))
    nrm, dst = np.zeros((n1, 3)), np.zeros((n1, 2))
    borderline = []

    def near(v, th):
        return abs(v - th) <= TRI_MARGIN * abs(th)

    for i in range(n1):
        j = int(matches12[i])
        if j < 0:
            continue
        o1, o2 = int(a.kps["octave"][i]), int(b.kps["octave"][j])
        x1, y1, x2, y2 = (float(v) for v in (a.kps["x"][i], a.kps["y"][i], b.kps["x"][j], b.kps["y"][j]))
        xn1 = np.array([(x1 - cx) / fx, (y1 - cy) / fy, 1.0])
        xn2 = np.array([(x2 - cx) / fx, (y2 - cy) / fy, 1.0])
        r1, r2 = R1.T @ xn1, R2.T @ xn2
        cos = float(r1 @ r2 / (np.linalg.norm(r1) * np.linalg.norm(r2)))
        edge = abs(cos - 0.9998) < 1e-6 or abs(cos) < 1e-6  # (f64 from f32 rays on both sides: some 1e-7 apart)
        code = 0
        if not (0 < cos < float(f32(0.9998))):
            code = LOW_PARALLAX
        else:
            A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
            X = np.linalg.svd(A)[2][3]
            if X[3] == 0:
                code = W_ZERO
            else:
                X = X[:3] / X[3]
                pts[i] = X
                c1, c2 = R1 @ X + t1, R2 @ X + t2
                d1, d2 = float(np.linalg.norm(X - O1)), float(np.linalg.norm(X - O2))
                # depths: a sign is "within rounding" when the depth is tiny against the distance
                edge = edge or abs(c1[2]) < 1e-4 * d1 or abs(c2[2]) < 1e-4 * d2
                if c1[2] <= 0:
                    code = BEHIND_1
                elif c2[2] <= 0:
                    code = BEHIND_2
                else:
                    e1 = (fx * c1[0] / c1[2] + cx - x1) ** 2 + (fy * c1[1] / c1[2] + cy - y1) ** 2
                    e2 = (fx * c2[0] / c2[2] + cx - x2) ** 2 + (fy * c2[1] / c2[2] + cy - y2) ** 2
                    th1, th2 = 5.991 * s2[o1], 5.991 * s2[o2]
                    edge = edge or near(e1, th1)
                    if e1 > th1:
                        code = REPROJ_1
                    else:
                        edge = edge or near(e2, th2)
                        if e2 > th2:
                            code = REPROJ_2
                        elif d1 == 0 or d2 == 0:
                            code = ZERO_DIST
                        else:
                            rd, ro, rf = d2 / d1, sc[o1] / sc[o2], 1.5 * float(f32(w.scale_factor))
                            edge = edge or near(rd * rf, ro) or near(rd, ro * rf)
                            if rd * rf < ro or rd > ro * rf:
                                code = SCALE
                            else:
                                code = KEPT
                                nrm[i] = ((X - O1) / d1 + (X - O2) / d2) / 2
                                dst[i] = (d1 * sc[o1] / sc[w.nlevels - 1], d1 * sc[o1])
        if edge:
            borderline.append(i)
            code = -1
        outcome[i] = code
    return dict(outcome=outcome, points=pts, normal=nrm, dist=dst, borderline=borderline)


# ---- worlds ----

K_DEFAULT = np.array([520.0, 0, 320.0, 0, 520.0, 240.0, 0, 0, 1], np.float32)
K_POW2 = np.array([512.0, 0, 256.0, 0, 512.0, 256.0, 0, 0, 1], np.float32)  # (cx, cy powers of two: the hand-made worlds' exact zeros)
WIDTH, HEIGHT = 640, 480


def keypoints(x, y, octave, angle, nlevels=NLEVELS, scale_factor=SCALE_FACTOR):
    k = np.zeros(len(x), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = x, y, octave, angle
    k["size"] = 31.0 * scale_table(nlevels, scale_factor)[np.clip(octave, 0, nlevels - 1)]
    k["response"], k["class_id"] = 1.0, -1
    return k


def flip(desc, rng, n_bits):
    """desc [32] with n_bits distinct bits flipped."""
    out = desc.copy()
    for bit in rng.choice(256, n_bits, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def make_world(seed, n_points=220, n_nodes=48, noise=0.35, n_distract=40, n_random=30, centre2=(0.6, 0.05, 0.1), rot2=((0.1, 1.0, 0.2), 4.0),
               depth=(4.0, 12.0), ori=True, masked=0.0, median=None, big_node=0, octave_jitter=0.1, octave_spread=1, K=K_DEFAULT, angle_outliers=0.08,
               scale_factor=SCALE_FACTOR, nlevels=NLEVELS, rot1=((0.3, -0.2, 1.0), 1.5)):
    """Two keyframes that see n_points 3D points (KF2's copies carry pixel noise of `noise` * the level's scale and a few flipped
    descriptor bits), n_distract KF2 features that copy a KF1 feature's descriptor at a random place of its node, n_random
    features of their own in each keyframe; every feature in a random order.  big_node > 0 puts that many of the points under one
    node.  masked: the share of features of either keyframe that already have a map point."""
    rng = np.random.default_rng(seed)
    sc = scale_table(nlevels, scale_factor).astype(np.float64)
    Kd = np.asarray(K, np.float64).reshape(3, 3)
    R1, C1 = rot(*rot1), np.array([0.02, -0.01, 0.03])
    R2, C2 = rot(*rot2), np.asarray(centre2, np.float64)
    pose1, pose2 = pose12(R1, C1), pose12(R2, C2)
    f1, f2 = [], []  # (x, y, octave, angle, desc, node, point id or -1)
    pid = 0
    tries = 0
    while pid < n_points and tries < 50 * n_points:
        tries += 1
        u, v, z = rng.uniform(10, WIDTH - 10), rng.uniform(10, HEIGHT - 10), rng.uniform(*depth)
        X = R1.T @ (np.linalg.inv(Kd) @ np.array([u, v, 1.0]) * z) + C1
        c2 = R2 @ (X - C2)
        if c2[2] <= 0.5:
            continue
        p2 = Kd @ c2
        u2, v2 = p2[0] / p2[2], p2[1] / p2[2]
        if not (10 < u2 < WIDTH - 10 and 10 < v2 < HEIGHT - 10):
            continue
        o1 = int(min(nlevels - 1, rng.geometric(0.35) - 1))
        o2 = int(np.clip(o1 + (rng.integers(-octave_spread, octave_spread + 1) if rng.random() < octave_jitter else 0), 0, nlevels - 1))
        ang = rng.uniform(0, 360)
        ang2 = rng.uniform(0, 360) if rng.random() < angle_outliers else (ang - 12.0 + rng.normal(0, 2.0)) % 360.0
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        node = 1000 + 7 * (0 if pid < big_node else 1 + pid % n_nodes)
        f1.append((u + rng.normal(0, 0.3 * noise), v + rng.normal(0, 0.3 * noise), o1, ang, d, node, pid, X))
        f2.append((u2 + rng.normal(0, noise * sc[o2]), v2 + rng.normal(0, noise * sc[o2]), o2, ang2, flip(d, rng, int(rng.integers(0, 24))),
                   node, pid, X))
        pid += 1
    for _ in range(n_distract):  # a near copy of a KF1 descriptor somewhere else in KF2, under the same node
        src = f1[int(rng.integers(0, len(f1)))]
        f2.append((rng.uniform(10, WIDTH - 10), rng.uniform(10, HEIGHT - 10), src[2], rng.uniform(0, 360),
                   flip(src[4], rng, int(rng.integers(20, 45))), src[5], -1, None))
    for f in (f1, f2):
        for _ in range(n_random):
            f.append((rng.uniform(10, WIDTH - 10), rng.uniform(10, HEIGHT - 10), int(rng.integers(0, nlevels)), rng.uniform(0, 360),
                      rng.integers(0, 256, 32, dtype=np.uint8), 1000 + 7 * int(rng.integers(0, n_nodes + 6)), -1, None))
    kfs, index = [], []
    for f, pose in ((f1, pose1), (f2, pose2)):
        order = rng.permutation(len(f))
        f = [f[k] for k in order]
        kps = keypoints(np.array([e[0] for e in f], f32), np.array([e[1] for e in f], f32), np.array([e[2] for e in f], np.int32),
                        np.array([e[3] for e in f], f32), nlevels, scale_factor)
        mask = (rng.random(len(f)) < masked).astype(np.uint8) if masked > 0 else None
        kfs.append(KeyFrame.from_nodes(kps, np.stack([e[4] for e in f]), [e[5] for e in f], pose, mask))
        index.append({e[6]: (k, e[7]) for k, e in enumerate(f) if e[6] >= 0})
    truth = {i: (index[1][p][0], X) for p, (i, X) in index[0].items()}
    return World(kfs[0], kfs[1], K, ori=ori, median=median, truth=truth, scale_factor=scale_factor, nlevels=nlevels)


_WORLDS = {}
WORLDS = ("small_nodes", "big_node", "forward", "masked", "noise_free", "dense", "mixed")


# the second setting: K_ANISO, 5 levels of 1.37, KF2 rolled by 89 degrees against KF1; the same seven kinds, smaller
WORLDS_2 = tuple(n + "@2" for n in WORLDS)
ROLL_2 = ((0.04, -0.03, 1.0), 89.0)


def world(name):
    """The committed worlds, built once.  name@2: the world of that kind under the second setting (WORLDS_2).  small_nodes: 48 nodes of a handful of features (more nodes than the kernel has waves);
    big_node: one node of some 100 KF2 features (the chunked path) among the small ones; forward: KF2 ahead of KF1, the epipole
    inside the image; masked: a third of either keyframe's features already have map points; noise_free: exact projections
    (the ground-truth world); dense: 600 points, more than 256 matches per pair; mixed: near points, pixel noise of a level's scale
    and octaves up to five levels apart between the views, so that the line test, the reprojection gates and the scale gate all
    reject some."""
    if name not in _WORLDS and name.endswith("@2"):
        two = dict(rot2=ROLL_2, **SECOND)
        _WORLDS[name] = {
            "small_nodes@2": lambda: make_world(111, n_points=120, n_nodes=70, n_distract=20, n_random=15, **two),
            "big_node@2": lambda: make_world(112, n_points=150, big_node=90, n_distract=20, n_random=15, **two),
            "forward@2": lambda: make_world(113, n_points=120, n_distract=20, n_random=15, centre2=(0.03, -0.02, 1.2), depth=(4.0, 10.0), **two),
            "masked@2": lambda: make_world(114, n_points=120, n_distract=20, n_random=15, masked=0.33, **two),
            "noise_free@2": lambda: make_world(115, n_points=120, noise=0.0, n_distract=10, n_random=15, octave_jitter=0.0, depth=(2.0, 4.0),
                                               centre2=(1.0, 0.1, 0.1), **two),
            "dense@2": lambda: make_world(116, n_points=330, n_nodes=90, n_distract=30, **two),
            "mixed@2": lambda: make_world(124, n_points=150, n_distract=20, n_random=15, noise=1.0, depth=(1.5, 6.0), octave_jitter=0.5,
                                          octave_spread=4, centre2=(0.5, 0.1, 0.3), **two),
        }[name]()
    if name not in _WORLDS:
        _WORLDS[name] = {
            "small_nodes": lambda: make_world(11),
            "big_node": lambda: make_world(12, n_points=230, big_node=90, n_distract=30),
            "forward": lambda: make_world(13, centre2=(0.03, -0.02, 1.2), rot2=((0, 1, 0), 0.5), depth=(4.0, 10.0)),
            "masked": lambda: make_world(14, masked=0.33),
            "noise_free": lambda: make_world(15, noise=0.0, n_distract=10, octave_jitter=0.0, depth=(2.0, 4.0), centre2=(1.0, 0.1, 0.1)),
            "dense": lambda: make_world(16, n_points=600, n_nodes=90, n_distract=60),
            "mixed": lambda: make_world(24, noise=1.0, depth=(1.5, 6.0), octave_jitter=0.5, octave_spread=5, centre2=(0.5, 0.1, 0.3)),
        }[name]()
    return _WORLDS[name]


def hand_desc(bits):
    """A descriptor with the given bit positions set: the distance of two of them is the size of the symmetric difference."""
    d = np.zeros(32, np.uint8)
    for bit in bits:
        d[bit >> 3] |= np.uint8(1 << (bit & 7))
    return d


def hand_world(feats1, feats2, centre2=(0.0, 0.0, 1.0), ori=False, median=None, K=K_POW2, mask1=None, mask2=None):
    """A hand-made pair: KF1 at the origin, KF2 at centre2, both without rotation; feats = [(x, y, octave, angle, desc, node)]."""
    kfs = []
    for feats, C, mask in ((feats1, (0, 0, 0), mask1), (feats2, centre2, mask2)):
        kps = keypoints(np.array([f[0] for f in feats], f32), np.array([f[1] for f in feats], f32),
                        np.array([f[2] for f in feats], np.int32), np.array([f[3] for f in feats], f32))
        desc = np.stack([f[4] for f in feats]) if feats else np.zeros((0, 32), np.uint8)
        kfs.append(KeyFrame.from_nodes(kps, desc, [f[5] for f in feats], pose12(np.eye(3), C), mask))
    return World(kfs[0], kfs[1], K, ori=ori, median=median)


def project(K, C, X):
    """The pixel of X seen from an unrotated camera at C."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    p = K @ (np.asarray(X, np.float64) - np.asarray(C, np.float64))
    return p[0] / p[2], p[1] / p[2]
