"""ctypes wrapper around tests/cpp/match_proj_ref.cpp -- the CPU restatement of ORBmatcher::SearchByProjection(CurrentFrame,
LastFrame, th, bMono=True) (include/orbx.h, "matching by projection") -- compiled on first use with g++ -O2 -ffp-contract=off
into a private temporary directory, as tests/pose_ref_lib.py compiles its source; a second, independently written numpy
statement without a grid; and the worlds (a last frame's map points seen from a predicted pose, a current frame around their
projections) that tests/test_match_proj_host.py and tests/test_gpu_match_proj.py share.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

from pose_ref_lib import K_ANISO, NLEVELS_2, SCALE_FACTOR_2, SECOND, SETTINGS  # noqa: F401 (the second setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "match_proj_ref.cpp")
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
RESULT_FIELDS = ("status", "nmatches", "n_points", "n_in_image", "n_with_candidates", "n_displaced", "n_rot_removed", "rounds")
COMPARED_FIELDS = RESULT_FIELDS[:-1]  # (rounds is the device's own count)
BAD_INPUT, NONFINITE = 2, 4
NLEVELS = 8
TH_HIGH = 100
BOUNDS = (0, 640, 0, 480)
f32 = np.float32
_L = None


def build(src=SRC) -> ctypes.CDLL:
    """Compiles a restatement source (lib(): the committed one; tests/test_camera_mutants_host.py: an altered copy) and binds it."""
    d = tempfile.mkdtemp(prefix="match_proj_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libmatch_proj_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", src, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("match_proj_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.mpr_features_in_area.argtypes = [vp, i32, vp, fl, fl, fl, i32, i32, vp]
    L.mpr_search_by_projection.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, fl, i32, vp, vp, vp, vp, vp, vp]
    L.mpr_search_by_projection.restype = None
    return L


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        _L = build()
    return _L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def scale_table(nlevels: int = NLEVELS, scale_factor: float = 1.2) -> np.ndarray:
    """mvScaleFactor as ORBextractor's constructor computes it (f32)."""
    out = np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        out[i] = f32(out[i - 1] * f32(scale_factor))
    return out


class World:
    """One pair: the last frame (kps_l, desc_l), its map points (points [n_l, 3], mask, point_desc or None, outlier or None), the
    current frame (kps_c, desc_c), its predicted pose [12], K [9], the bounds, th and the orientation switch."""

    def __init__(self, kps_l, desc_l, kps_c, desc_c, points, mask, pose, K, bounds=BOUNDS, th=15.0, ori=True, point_desc=None,
                 outlier=None, scale=None, truth=None):
        self.kps_l, self.kps_c = np.ascontiguousarray(kps_l, KEYPOINT_DTYPE), np.ascontiguousarray(kps_c, KEYPOINT_DTYPE)
        self.desc_l = np.ascontiguousarray(desc_l, np.uint8).reshape(-1, 32)
        self.desc_c = np.ascontiguousarray(desc_c, np.uint8).reshape(-1, 32)
        self.points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.point_desc = None if point_desc is None else np.ascontiguousarray(point_desc, np.uint8).reshape(-1, 32)
        self.outlier = None if outlier is None else np.ascontiguousarray(outlier, np.uint8)
        self.pose, self.K = np.ascontiguousarray(pose, np.float32).reshape(12), np.ascontiguousarray(K, np.float32).reshape(9)
        self.bounds, self.th, self.ori = tuple(int(b) for b in bounds), float(th), bool(ori)
        self.scale = scale_table() if scale is None else np.ascontiguousarray(scale, np.float32)
        self.truth = truth
        self.n_l, self.n_c = len(self.kps_l), len(self.kps_c)
        assert len(self.desc_l) == self.n_l == len(self.points) and len(self.desc_c) == self.n_c
        self._expected = None

    def variant(self, **kw):
        """The same pair with some inputs replaced (a fresh World: nothing cached is shared)."""
        a = dict(kps_l=self.kps_l.copy(), desc_l=self.desc_l, kps_c=self.kps_c.copy(), desc_c=self.desc_c, points=self.points.copy(),
                 mask=self.mask, pose=self.pose, K=self.K, bounds=self.bounds, th=self.th, ori=self.ori, point_desc=self.point_desc,
                 outlier=self.outlier, scale=self.scale, truth=self.truth)
        a.update(kw)
        return World(**a)

    def expected(self):
        """The restatement's answer, computed once and left unchanged."""
        if self._expected is None:
            self._expected = search_by_projection(self)
        return self._expected


def features_in_area(kps, bounds, x, y, r, min_level, max_level):
    """The restatement's GetFeaturesInArea -> int32 indices in its order."""
    k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    b = np.ascontiguousarray(bounds, np.int32)
    out = np.zeros(max(len(k), 1), np.int32)
    n = lib().mpr_features_in_area(_p(k), len(k), _p(b), float(x), float(y), float(r), int(min_level), int(max_level), _p(out))
    return out[:n].copy()


def search_by_projection(w: World):
    """The restatement -> dict(matches [n_c] int32, res {field: value}, proj [n_l, 4] (u, v, r, stage), free_pick [n_l],
    outcome [n_l], taken_ahead [n_l])."""
    m, res = np.full(max(w.n_c, 1), -7, np.int32), np.zeros(8, np.int32)
    nl = max(w.n_l, 1)
    proj, free, out, ahead = np.zeros((nl, 4), np.float32), np.zeros(nl, np.int32), np.zeros(nl, np.int32), np.zeros(nl, np.int32)
    b = np.ascontiguousarray(w.bounds, np.int32)
    lib().mpr_search_by_projection(_p(w.kps_l), _p(w.desc_l), w.n_l, _p(w.kps_c), _p(w.desc_c), w.n_c, _p(w.points), _p(w.mask),
                                   _p(w.point_desc), _p(w.outlier), _p(w.pose), _p(w.K), _p(b), _p(w.scale), len(w.scale), w.th,
                                   int(w.ori), _p(m), _p(res), _p(proj), _p(free), _p(out), _p(ahead))
    return dict(matches=m[:w.n_c].copy(), res=dict(zip(RESULT_FIELDS, (int(v) for v in res))), proj=proj[:w.n_l],
                free_pick=free[:w.n_l], outcome=out[:w.n_l], taken_ahead=ahead[:w.n_l])


# ---- the second statement: numpy, no grid -- every feature of C is tested against the window's cell range ----

def _round_half_away(v):
    v = np.asarray(v, np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), -np.floor(-v + 0.5))


def project_numpy(w: World, i):
    """Steps 2 and 3 for feature i -> (stage, u, v) in f32 arithmetic, one operation at a time."""
    if w.mask is not None and w.mask[i] == 0:
        return 0, None, None
    if w.outlier is not None and w.outlier[i] != 0:
        return 0, None, None
    o = int(w.kps_l["octave"][i])
    if o < 0 or o >= len(w.scale):
        return 0, None, None
    R, t, X = w.pose[:9], w.pose[9:], w.points[i]
    with np.errstate(all="ignore"):
        c = [f32(f32(f32(f32(R[3 * k] * X[0]) + f32(R[3 * k + 1] * X[1])) + f32(R[3 * k + 2] * X[2])) + t[k]) for k in range(3)]
        invz = f32(f32(1.0) / c[2])
        if invz < 0:
            return 1, None, None
        u = f32(f32(f32(w.K[0] * c[0]) * invz) + w.K[2])
        v = f32(f32(f32(w.K[4] * c[1]) * invz) + w.K[5])
    if not (math.isfinite(u) and math.isfinite(v)):
        return 1, None, None
    if u < w.bounds[0] or u > w.bounds[1] or v < w.bounds[2] or v > w.bounds[3]:
        return 1, None, None
    return 2, u, v


def window_numpy(kps, bounds, u, v, r, lo, hi):
    """The candidates of a window, by filtering all features: cell in the window's range, level, strict radius; sorted by
    (cell x, cell y, index)."""
    x, y, octv = kps["x"], kps["y"], kps["octave"]
    with np.errstate(all="ignore"):
        minx, miny = f32(bounds[0]), f32(bounds[2])
        winv, hinv = f32(64) / f32(bounds[1] - bounds[0]), f32(48) / f32(bounds[3] - bounds[2])
        px, py = _round_half_away((x - minx) * winv), _round_half_away((y - miny) * hinv)
        x0 = max(0.0, math.floor(float(f32(f32(f32(u - minx) - r) * winv))))
        x1 = min(63.0, math.ceil(float(f32(f32(f32(u - minx) + r) * winv))))
        y0 = max(0.0, math.floor(float(f32(f32(f32(v - miny) - r) * hinv))))
        y1 = min(47.0, math.ceil(float(f32(f32(f32(v - miny) + r) * hinv))))
        ok = (px >= 0) & (px < 64) & (py >= 0) & (py < 48) & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        ok &= (octv >= lo) & (octv <= hi) & (np.abs(x - u) < r) & (np.abs(y - v) < r)
    idx = np.flatnonzero(ok)
    return idx[np.lexsort((idx, py[idx], px[idx]))].astype(np.int32)


def search_by_projection_numpy(w: World):
    """-> (matches [n_c], nmatches)."""
    ones = np.array([bin(v).count("1") for v in range(256)], np.uint8)
    matches = np.full(w.n_c, -1, np.int32)
    bins = np.full(w.n_c, -1, np.int64)
    q = w.desc_l if w.point_desc is None else w.point_desc
    for i in range(w.n_l):
        stage, u, v = project_numpy(w, i)
        if stage != 2:
            continue
        o = int(w.kps_l["octave"][i])
        cand = window_numpy(w.kps_c, w.bounds, u, v, f32(f32(w.th) * w.scale[o]), o - 1, o + 1)
        cand = cand[matches[cand] < 0]
        if not len(cand):
            continue
        d = ones[w.desc_c[cand] ^ q[i][None, :]].sum(axis=1, dtype=np.int64)
        k = int(np.argmin(d))  # (the first smallest)
        if d[k] > TH_HIGH:
            continue
        j = int(cand[k])
        matches[j] = i
        rot = f32(w.kps_l["angle"][i]) - f32(w.kps_c["angle"][j])
        if rot < 0:
            rot = f32(rot + f32(360.0))
        x = float(f32(rot * f32(f32(30) / f32(360.0))))
        if math.isfinite(x):
            b = int(_round_half_away(x))
            b = 0 if b == 30 else b
            bins[j] = b if 0 <= b < 30 else -1
    if w.ori:
        size = np.bincount(bins[bins >= 0], minlength=30)
        order = [b for b in sorted(range(30), key=lambda b: (-size[b], b)) if size[b] > 0][:3]
        top = [int(size[b]) for b in order] + [0, 0, 0]
        keep = order + [-1, -1, -1]
        if f32(top[1]) < f32(0.1) * f32(top[0]):
            keep[1] = keep[2] = -1
        elif f32(top[2]) < f32(0.1) * f32(top[0]):
            keep[2] = -1
        lose = (bins >= 0) & ~np.isin(bins, [b for b in keep[:3] if b >= 0])
        matches[lose] = -1
    return matches, int((matches >= 0).sum())


# ---- the worlds the host and the GPU test share ----

def camera(bounds=BOUNDS):
    return np.array([500.0, 0, (bounds[0] + bounds[1]) / 2.0, 0, 500.0, (bounds[2] + bounds[3]) / 2.0, 0, 0, 1], np.float32)


def pose_of(seed, roll_deg=0.0):
    """A small motion: a rotation of a few degrees about a random axis (f64 Rodrigues, stored f32) and a translation.  roll_deg:
    that rotation applied behind a roll about the optical axis (the second setting: 89 degrees)."""
    rng = np.random.default_rng(seed)
    wv = rng.normal(size=3)
    wv *= np.deg2rad(rng.uniform(1.0, 4.0)) / np.linalg.norm(wv)
    th = np.linalg.norm(wv)
    k = wv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx
    if roll_deg:
        c, s = math.cos(math.radians(roll_deg)), math.sin(math.radians(roll_deg))
        R = R @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    return np.r_[R.reshape(9), rng.uniform(-0.2, 0.2, 3)].astype(np.float32)


def points_seen_at(pose, K, uv, depth):
    """World points whose projection with `pose` lands (up to f32 rounding) at the pixels uv with these depths."""
    R, t = pose[:9].reshape(3, 3).astype(np.float64), pose[9:].astype(np.float64)
    xc = np.stack([(uv[:, 0] - K[2]) / K[0] * depth, (uv[:, 1] - K[5]) / K[4] * depth, depth], axis=1)
    return ((xc - t) @ R).astype(np.float32)  # R^T (xc - t)


def _keypoints(n, rng, octave=None, nlevels=NLEVELS):
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
    k["angle"] = rng.uniform(0.0, 360.0, n).astype(np.float32)
    k["octave"] = rng.integers(0, nlevels, n) if octave is None else octave
    k["size"], k["class_id"] = 31.0, -1
    return k


def _flip(desc, nbits, rng):
    d = desc.copy()
    for b in rng.choice(256, size=int(nbits), replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def make_world(n, seed, bounds=BOUNDS, th=15.0, ori=True, n_extra=None, with_point_desc=False, with_outlier=True, edge_cases=True,
               K=None, scale_factor=1.2, nlevels=NLEVELS, roll_deg=0.0):
    """n features in the last frame.  Their map points project all over the bounds and a margin around them, a tenth behind the
    camera; the current frame holds, in random order, for three quarters of the points a feature near the projection (0 to 3.5
    window radii away per axis, the octave off by 0, 1 or, rarely, 2; the descriptor the point's with 0 to 60 bits flipped; the
    angle the last frame's minus 40 degrees plus noise wide enough that bins lose), n_extra unrelated features, and features
    outside the grid.  With edge_cases a few features sit a hair inside and a hair outside the radius of a projection."""
    rng = np.random.default_rng(seed)
    K, pose = camera(bounds) if K is None else np.asarray(K, np.float32).reshape(9), pose_of(seed + 1, roll_deg)
    kl = _keypoints(n, rng, nlevels=nlevels)
    if n >= 2:
        kl["octave"][0], kl["octave"][1] = 0, nlevels - 1
    dl = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    w_, h_ = bounds[1] - bounds[0], bounds[3] - bounds[2]
    uv = np.stack([rng.uniform(bounds[0] - 0.06 * w_, bounds[1] + 0.06 * w_, n), rng.uniform(bounds[2] - 0.06 * h_, bounds[3] + 0.06 * h_, n)], 1)
    depth = rng.uniform(2.0, 10.0, n)
    depth[rng.random(n) < 0.1] *= -1.0
    pts = points_seen_at(pose, K, uv, depth)
    mask = (rng.random(n) < 0.85).astype(np.uint8)
    outlier = (rng.random(n) < 0.05).astype(np.uint8) if with_outlier else None
    pdesc = np.stack([_flip(d, rng.integers(0, 9), rng) for d in dl]) if with_point_desc and n else None
    scale = scale_table(nlevels, scale_factor)
    # where the restatement projects them (the current frame plays no part in steps 2 and 3)
    none_k, none_d = np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
    proj = search_by_projection(World(kl, dl, none_k, none_d, pts, None, pose, K, bounds, th, ori, scale=scale))["proj"]
    feats, descs, truth = [], [], []
    src = dl if pdesc is None else pdesc
    for i in range(n):
        if proj[i, 3] != 2.0 or rng.random() > 0.75:
            continue
        u, v, r = proj[i, 0], proj[i, 1], proj[i, 2]
        k = np.zeros(1, KEYPOINT_DTYPE)
        k["x"], k["y"] = f32(u + r * rng.uniform(-1.0, 1.0) * rng.choice([0.2, 0.9, 3.5])), f32(v + r * rng.uniform(-1.0, 1.0) * 0.6)
        k["octave"] = int(kl["octave"][i]) + int(rng.choice([0, 0, 0, 1, -1, 1, -1, 2, -2]))
        k["angle"] = f32((float(kl["angle"][i]) - 40.0 + rng.normal(0.0, 9.0)) % 360.0)
        feats.append(k)
        descs.append(_flip(src[i], rng.integers(0, 61), rng))
        truth.append(i)
    edge = []
    if edge_cases:
        live = (proj[:, 3] == 2.0) & (mask != 0) & ((outlier == 0) if outlier is not None else True)
        live &= (proj[:, 0] - proj[:, 2] > bounds[0]) & (proj[:, 0] + proj[:, 2] < bounds[1])  # (the window's sides lie in the grid)
        for i in np.flatnonzero(live)[:12]:
            u, v, r = proj[i, 0], proj[i, 1], proj[i, 2]
            for side, inside in ((1, True), (1, False), (-1, True), (-1, False)):
                # the largest x with |x - u| < r in f32, and the next one
                x = f32(u + side * r)
                while not abs(f32(x - u)) < r:
                    x = np.nextafter(x, f32(u), dtype=np.float32)
                if not inside:
                    x = np.nextafter(x, f32(u + side * 1e9), dtype=np.float32)
                k = np.zeros(1, KEYPOINT_DTYPE)
                k["x"], k["y"], k["octave"], k["angle"] = x, v, kl["octave"][i], f32((float(kl["angle"][i]) - 40.0) % 360.0)
                feats.append(k)
                descs.append(_flip(src[i], 20 + len(edge) % 7, rng))
                truth.append(-1)
                edge.append((int(i), len(feats) - 1, inside))
    n_extra = n // 4 if n_extra is None else n_extra
    extra = _keypoints(n_extra, rng, nlevels=nlevels)
    extra["x"], extra["y"] = rng.uniform(bounds[0], bounds[1], n_extra), rng.uniform(bounds[2], bounds[3], n_extra)
    far = _keypoints(min(6, n), rng, nlevels=nlevels)  # outside the grid: beyond the bounds by more than a cell, and one that is no number
    far["x"] = np.array([bounds[0] - 40.0, bounds[1] + 40.0, 100.0, 200.0, np.nan, bounds[1] + 4.0], np.float32)[:len(far)]
    far["y"] = np.array([100.0, 100.0, bounds[2] - 40.0, bounds[3] + 40.0, 50.0, bounds[3] + 4.0], np.float32)[:len(far)]
    kc = np.concatenate(feats + [extra, far]) if feats or n_extra or len(far) else np.zeros(0, KEYPOINT_DTYPE)
    dc = np.concatenate([np.array(descs, np.uint8).reshape(-1, 32), rng.integers(0, 256, (n_extra + len(far), 32), dtype=np.uint8)])
    truth = np.array(truth + [-1] * (n_extra + len(far)), np.int64)
    perm = rng.permutation(len(kc))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    edge = [(i, int(inv[j]), inside) for i, j, inside in edge]
    w = World(kl, dl, kc[perm], dc[perm], pts, mask, pose, K, bounds, th, ori, pdesc, outlier, scale, truth=truth[perm])
    w.edge = edge
    return w


def truth_world(n=300, seed=5):
    """The current frame's features ARE the projections of the last frame's points (in random order), their descriptors exact
    copies among random 256-bit descriptors, every angle shifted by the same 36 degrees (angles are multiples of a quarter
    degree, so the difference is exact): one bin, nothing removed; every visible point must get exactly its feature."""
    rng = np.random.default_rng(seed)
    K, pose = camera(), pose_of(seed + 1)
    kl = _keypoints(n, rng)
    kl["angle"] = (rng.integers(0, 1440, n) * 0.25).astype(np.float32)
    dl = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    uv = np.stack([rng.uniform(-30, 670, n), rng.uniform(-30, 510, n)], 1)
    pts = points_seen_at(pose, K, uv, rng.uniform(2.0, 10.0, n))
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    none_k, none_d = np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
    proj = search_by_projection(World(kl, dl, none_k, none_d, pts, None, pose, K))["proj"]
    kc = kl.copy()
    kc["x"], kc["y"] = np.where(proj[:, 3] == 2.0, proj[:, 0], uv[:, 0]), np.where(proj[:, 3] == 2.0, proj[:, 1], uv[:, 1])
    kc["angle"] = ((kl["angle"].astype(np.float64) - 36.0) % 360.0).astype(np.float32)
    perm = rng.permutation(n)
    w = World(kl, dl, kc[perm], dl[perm], pts, mask, pose, K, truth=perm.copy())
    # (PosInGrid leaves the last half cell of the bounds out of the grid: a feature there is nobody's candidate)
    in_grid = (_round_half_away(kc["x"] * f32(64.0 / 640.0)) < 64) & (_round_half_away(kc["y"] * f32(48.0 / 480.0)) < 48)
    w.visible = (proj[:, 3] == 2.0) & (mask != 0) & in_grid
    return w


def order_world():
    """Three features of the last frame (0, 1, 2) whose windows share the candidates A = feature 0 and B = feature 1 of the
    current frame, with d(0, A) = 0, d(1, A) = 1, d(1, B) = 5, d(2, B) = 2, d(2, A) = 8, and B outside feature 0's window.  The
    sequential answer is 0 -> A, 1 -> B, 2 -> none; "the lowest claimant of its first choice wins" gives 2 -> B.  (d(2, A) = 8 is
    the largest value the triangle inequality leaves with the other four: d(A, B) <= d(1, A) + d(1, B) = 6.)"""
    rng = np.random.default_rng(11)
    K = camera()
    pose = np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32)
    A = rng.integers(0, 256, 32, dtype=np.uint8)

    def x(d, bits):
        d = d.copy()
        for b in bits:
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        return d
    B = x(A, range(6))
    dl = np.stack([A, x(A, [0]), x(B, [100, 101])])
    kl = np.zeros(3, KEYPOINT_DTYPE)
    kl["octave"], kl["angle"] = 0, 10.0
    kc = np.zeros(2, KEYPOINT_DTYPE)
    kc["x"], kc["y"], kc["octave"], kc["angle"] = [300.0, 310.0], [200.0, 200.0], 0, 10.0
    uv = np.array([[290.0, 200.0], [305.0, 200.0], [306.0, 201.0]])  # window radius 15: feature 0 reaches A (10) but not B (20)
    pts = points_seen_at(pose, K, uv, np.full(3, 4.0))
    return World(kl, dl, kc, np.stack([A, B]), pts, None, pose, K, truth=np.array([0, 1]))


def contention_world(n_clusters=40, seed=21):
    """Clusters: seven map points that project within a few pixels of each other, with descriptors a few bits from a common
    one, over four features of the current frame with such descriptors under all their windows: what a feature gets depends on
    what the features before it took, three of the seven find everything taken, and later ones skip several taken candidates."""
    rng = np.random.default_rng(seed)
    K, pose = camera(), pose_of(seed + 1)
    uv, dl, kc_xy, dc, octs = [], [], [], [], []
    for c in range(n_clusters):
        centre = np.array([rng.uniform(40, 600), rng.uniform(40, 440)])
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        o = int(rng.integers(0, 3))
        for _ in range(7):
            uv.append(centre + rng.uniform(-3, 3, 2))
            dl.append(_flip(base, rng.integers(0, 5), rng))
            octs.append(o)
        for _ in range(4):
            kc_xy.append((centre + rng.uniform(-5, 5, 2), o))
            dc.append(_flip(base, rng.integers(0, 5), rng))
    n = len(uv)
    order = rng.permutation(n)
    uv, dl, octs = np.array(uv)[order], np.array(dl, np.uint8)[order], np.array(octs)[order]
    kl = _keypoints(n, rng, octs)
    pts = points_seen_at(pose, K, uv, rng.uniform(2.0, 10.0, n))
    kc = _keypoints(len(kc_xy), rng, np.array([o for _, o in kc_xy]))
    kc["x"], kc["y"] = [p[0] for p, _ in kc_xy], [p[1] for p, _ in kc_xy]
    perm = rng.permutation(len(kc))
    return World(kl, dl, kc[perm], np.array(dc, np.uint8)[perm], pts, None, pose, K, ori=False)


# the second setting: K_ANISO, 5 levels of 1.37, the pose rolled by 89 degrees; 150 features, and 310 under the offset bounds
WORLDS_2 = ("w150@2", "w310_bounds@2")
TWO = dict(roll_deg=89.0, **SECOND)
WORLDS = ("w300", "w300_noori", "w300_pdesc", "w310_bounds", "w1500", "w40_th30", "truth", "order", "contention", "empty_l", "empty_c")
_worlds = {}


def world(name: str) -> World:
    if name not in _worlds:
        none_k, none_d = np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
        if name == "w300":
            w = make_world(300, 1)
        elif name == "w150@2":
            w = make_world(150, 101, **TWO)
        elif name == "w310_bounds@2":
            w = make_world(310, 104, bounds=(-12, 655, -9, 490), **TWO)
        elif name == "w300_noori":
            w = make_world(300, 2, ori=False)
        elif name == "w300_pdesc":
            w = make_world(280, 3, with_point_desc=True)
        elif name == "w310_bounds":
            w = make_world(310, 4, bounds=(-12, 655, -9, 490))
        elif name == "w1500":
            w = make_world(1500, 6, edge_cases=False)
        elif name == "w40_th30":
            w = make_world(40, 7, th=30.0)
        elif name == "truth":
            w = truth_world()
        elif name == "order":
            w = order_world()
        elif name == "contention":
            w = contention_world()
        elif name == "empty_l":
            b = make_world(50, 8)
            w = World(none_k, none_d, b.kps_c, b.desc_c, np.zeros((0, 3), np.float32), None, b.pose, b.K)
        elif name == "empty_c":
            b = make_world(50, 9)
            w = World(b.kps_l, b.desc_l, none_k, none_d, b.points, b.mask, b.pose, b.K)
        else:
            raise KeyError(name)
        _worlds[name] = w
    return _worlds[name]


_rules = {}


def rule_worlds():
    """Small worlds, each built around one rule of the statement -> {name: World} (built once)."""
    out = _rules
    if out:
        return out
    K = camera()
    eye = np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32)
    rng = np.random.default_rng(77)
    d = rng.integers(0, 256, (8, 32), dtype=np.uint8)

    def pair(uv, depth, cxy, desc_l, desc_c, **kw):
        n, m = len(uv), len(cxy)
        kl, kc = np.zeros(n, KEYPOINT_DTYPE), np.zeros(m, KEYPOINT_DTYPE)
        kl["angle"] = kw.pop("ang_l", 10.0)
        kc["angle"] = kw.pop("ang_c", 10.0)
        kl["octave"] = kw.pop("oct_l", 0)
        kc["octave"] = kw.pop("oct_c", 0)
        kc["x"], kc["y"] = [c[0] for c in cxy], [c[1] for c in cxy]
        pts = points_seen_at(eye, K, np.asarray(uv, np.float64).reshape(-1, 2), np.asarray(depth, np.float64))
        return World(kl, desc_l, kc, desc_c, pts, kw.pop("mask", None), eye, K, **kw)
    spots = [(100.0 + 60 * k, 100.0) for k in range(4)]
    out["mask_and_outlier"] = pair(spots, [4.0] * 4, spots, d[:4], d[:4], mask=np.array([1, 0, 1, 1], np.uint8),
                                   outlier=np.array([0, 0, 1, 0], np.uint8))
    out["behind_the_camera"] = pair(spots, [4.0, -4.0, 4.0, -1e-3], spots, d[:4], d[:4])
    zero_depth = pair(spots, [4.0] * 4, spots, d[:4], d[:4])
    zero_depth.points[1, 2] = 0.0
    out["zero_depth"] = zero_depth.variant()
    # u exactly on min_x and on max_x (cx = 320 and fx = 500 with X = -+1.28, Z = 2 give 0 and 640 exactly), and just outside
    on = pair(spots, [2.0] * 4, [(0.0, 240.0), (630.0, 240.0), (2.0, 240.0), (634.0, 240.0)], d[:4], d[[0, 1, 0, 1]])
    on.points[:] = [[-1.28, 0, 2], [1.28, 0, 2], [f32(-1.2800005), 0, 2], [f32(1.2800005), 0, 2]]
    out["on_the_bounds"] = on.variant()
    out["distance_100_and_101"] = pair(spots[:2], [4.0] * 2, spots[:2], d[:2], np.stack([_flip(d[0], 100, rng), _flip(d[1], 101, rng)]))
    # six matches at rotation 0, two at 90 degrees, one at 180: 0.1 * 6 keeps the second bin (2) and the third (1); with twenty
    # at rotation 0 the third goes (1 < 2.0) and the second stays (2 >= 2.0)
    for name, n0 in (("histogram_three_bins", 6), ("histogram_tenth_rule", 20)):
        n = n0 + 4
        sp = [(40.0 + 45 * (k % 13), 60.0 + 90 * (k // 13)) for k in range(n)]
        dd = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ang_c = np.array([10.0] * n0 + [280.0, 280.0, 190.0, 100.0], np.float32)  # rot 0 ... 90 90 180 270
        out[name] = pair(sp, [4.0] * n, sp, dd, dd, ang_c=ang_c)
    out["no_orientation"] = out["histogram_three_bins"].variant(ori=False)
    out["octave_out_of_table"] = pair(spots, [4.0] * 4, spots, d[:4], d[:4], oct_l=np.array([0, NLEVELS, -1, NLEVELS - 1]),
                                      oct_c=np.array([0, 0, 0, NLEVELS - 1]))
    nonfinite = pair(spots, [4.0] * 4, spots, d[:4], d[:4])
    nonfinite.points[1, 0], nonfinite.points[2, 2] = np.nan, np.inf
    out["nonfinite_point"] = nonfinite.variant()
    out["nonfinite_pose"] = pair(spots, [4.0] * 4, spots, d[:4], d[:4]).variant(pose=np.r_[eye[:9], [np.nan, 0, 0]].astype(np.float32))
    out["no_features"] = pair([], [], [], d[:0], d[:0])
    out["point_descriptors"] = pair(spots, [4.0] * 4, spots, d[4:8], d[:4], point_desc=d[:4])
    out["frame_descriptors"] = pair(spots, [4.0] * 4, spots, d[4:8], d[:4])
    return out
