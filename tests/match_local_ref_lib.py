"""ctypes wrapper around tests/cpp/match_local_ref.cpp -- the CPU restatement of Tracking::SearchLocalPoints (include/orbx.h,
"matching the local map by projection") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary
directory, as tests/match_proj_ref_lib.py compiles its source; a second, independently written numpy statement without a grid and
without the streaming update; and the worlds (a local map seen from a pose, a frame around the projections of the points in view)
that tests/test_match_local_host.py and tests/test_gpu_match_local.py share.  TEST INFRASTRUCTURE only."""
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
SRC = os.path.join(ROOT, "tests", "cpp", "match_local_ref.cpp")
KEYPOINT_DTYPE = M.KEYPOINT_DTYPE
RESULT_FIELDS = ("status", "nmatches", "n_points", "n_seen", "n_behind", "n_out_image", "n_out_distance", "n_out_angle", "n_in_view",
                 "n_with_candidates", "n_over_th", "n_ratio_rejected", "n_displaced", "n_outliers_cleared", "rounds")
COMPARED_FIELDS = RESULT_FIELDS[:-1]  # (rounds is the device's own count)
BAD_INPUT, NONFINITE = 2, 4
NOT_IN_VIEW, SEEN = 0xFF, 0xFE
NLEVELS = M.NLEVELS
TH_HIGH = 100
BOUNDS = M.BOUNDS
f32 = np.float32
_L = None


def build(src=SRC) -> ctypes.CDLL:
    """Compiles a restatement source (lib(): the committed one; tests/test_camera_mutants_host.py: an altered copy) and binds it."""
    d = tempfile.mkdtemp(prefix="match_local_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libmatch_local_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", src, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("match_local_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.mlr_features_in_area.argtypes = [vp, i32, vp, fl, fl, fl, i32, i32, vp]
    L.mlr_predict_scale.argtypes = [vp, i32, vp, i32, vp]
    L.mlr_predict_scale.restype = None
    L.mlr_search_local_points.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, fl, fl, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mlr_search_local_points.restype = None
    return L


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        _L = build()
    return _L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


scale_table = M.scale_table


class World:
    """One pair: the frame (kps, desc), the map (points, normals [n_m, 3], dists [n_m, 2] = min, max, map_desc, mask or None), the
    pose [12], K [9], the bounds, th, nnratio, the matches the frame has on entry [n_f] and its outlier flags (or None)."""

    def __init__(self, kps, desc, points, normals, dists, map_desc, mask, pose, K, bounds=BOUNDS, th=1.0, nnratio=0.8, matches=None,
                 outlier=None, scale=None):
        self.kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self.dists = np.ascontiguousarray(dists, np.float32).reshape(-1, 2)
        self.map_desc = np.ascontiguousarray(map_desc, np.uint8).reshape(-1, 32)
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.pose, self.K = np.ascontiguousarray(pose, np.float32).reshape(12), np.ascontiguousarray(K, np.float32).reshape(9)
        self.bounds, self.th, self.nnratio = tuple(int(b) for b in bounds), float(th), float(nnratio)
        self.n_f, self.n_m = len(self.kps), len(self.points)
        self.matches = np.full(self.n_f, -1, np.int32) if matches is None else np.ascontiguousarray(matches, np.int32)
        self.outlier = None if outlier is None else np.ascontiguousarray(outlier, np.uint8)
        self.scale = scale_table() if scale is None else np.ascontiguousarray(scale, np.float32)
        assert len(self.desc) == self.n_f == len(self.matches)
        assert len(self.normals) == len(self.dists) == len(self.map_desc) == self.n_m
        self._expected = None

    def variant(self, **kw):
        """The same pair with some inputs replaced (a fresh World: nothing cached is shared)."""
        a = dict(kps=self.kps.copy(), desc=self.desc, points=self.points.copy(), normals=self.normals.copy(), dists=self.dists.copy(),
                 map_desc=self.map_desc, mask=self.mask, pose=self.pose, K=self.K, bounds=self.bounds, th=self.th, nnratio=self.nnratio,
                 matches=self.matches.copy(), outlier=self.outlier, scale=self.scale)
        a.update(kw)
        return World(**a)

    def expected(self):
        """The restatement's answer, computed once and left unchanged."""
        if self._expected is None:
            self._expected = search_local_points(self)
        return self._expected


def features_in_area(kps, bounds, x, y, r, min_level, max_level):
    """The restatement's GetFeaturesInArea -> int32 indices in its order."""
    k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    b = np.ascontiguousarray(bounds, np.int32)
    out = np.zeros(max(len(k), 1), np.int32)
    n = lib().mlr_features_in_area(_p(k), len(k), _p(b), float(x), float(y), float(r), int(min_level), int(max_level), _p(out))
    return out[:n].copy()


def predict_scale(ratios, scale=None):
    """The restatement's table PredictScale for an array of f32 ratios -> int32 levels."""
    r = np.ascontiguousarray(ratios, np.float32).reshape(-1)
    s = scale_table() if scale is None else np.ascontiguousarray(scale, np.float32)
    out = np.zeros(max(len(r), 1), np.int32)
    lib().mlr_predict_scale(_p(r), len(r), _p(s), len(s), _p(out))
    return out[:len(r)]


def search_local_points(w: World):
    """The restatement -> dict(matches [n_f] int32, res {field: value}, view [n_m] uint8, proj [n_m, 6] (u, v, radius, level,
    viewCos, stage), outcome [n_m], alone [n_m], best [n_m, 4])."""
    m = np.full(max(w.n_f, 1), -1, np.int32)
    m[:w.n_f] = w.matches
    nm = max(w.n_m, 1)
    res, view = np.zeros(15, np.int32), np.zeros(nm, np.uint8)
    proj, out, alone, best = np.zeros((nm, 6), np.float32), np.zeros(nm, np.int32), np.zeros(nm, np.int32), np.zeros((nm, 4), np.int32)
    b = np.ascontiguousarray(w.bounds, np.int32)
    lib().mlr_search_local_points(_p(w.kps), _p(w.desc), w.n_f, w.n_m, _p(w.points), _p(w.normals), _p(w.dists), _p(w.map_desc),
                                  _p(w.mask), _p(w.pose), _p(w.K), _p(b), _p(w.scale), len(w.scale), w.th, w.nnratio, _p(m),
                                  _p(w.outlier), _p(res), _p(view), _p(proj), _p(out), _p(alone), _p(best))
    return dict(matches=m[:w.n_f].copy(), res=dict(zip(RESULT_FIELDS, (int(v) for v in res))), view=view[:w.n_m], proj=proj[:w.n_m],
                outcome=out[:w.n_m], alone=alone[:w.n_m], best=best[:w.n_m])


# ---- the second statement: numpy; no grid, no streaming update ----

def frustum_numpy(w: World, i):
    """Steps 2 and 3 for point i -> (stage, u, v, level, viewCos); stage as the restatement's proj column."""
    P, N, (mind, maxd) = w.points[i], w.normals[i], w.dists[i]
    if not (np.isfinite(P).all() and np.isfinite(N).all() and np.isfinite(mind) and np.isfinite(maxd) and np.isfinite(w.pose).all()):
        return 0, None, None, None, None
    R, t = w.pose[:9], w.pose[9:]
    with np.errstate(all="ignore"):
        c = [f32(f32(f32(f32(R[3 * k] * P[0]) + f32(R[3 * k + 1] * P[1])) + f32(R[3 * k + 2] * P[2])) + t[k]) for k in range(3)]
        if c[2] < 0:
            return 1, None, None, None, None
        invz = f32(f32(1.0) / c[2])
        u = f32(f32(f32(w.K[0] * c[0]) * invz) + w.K[2])
        v = f32(f32(f32(w.K[4] * c[1]) * invz) + w.K[5])
        if not (math.isfinite(u) and math.isfinite(v)) or u < w.bounds[0] or u > w.bounds[1] or v < w.bounds[2] or v > w.bounds[3]:
            return 2, None, None, None, None
        ow = [f32(-f32(f32(f32(R[k] * t[0]) + f32(R[3 + k] * t[1])) + f32(R[6 + k] * t[2]))) for k in range(3)]
        po = [float(f32(P[k] - ow[k])) for k in range(3)]
        dist = f32(math.sqrt((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2]))
        if dist < f32(f32(0.8) * mind) or dist > f32(f32(1.2) * maxd):
            return 3, None, None, None, None
        dot = (po[0] * float(N[0]) + po[1] * float(N[1])) + po[2] * float(N[2])
        view_cos = f32(dot / float(dist)) if dist != 0 else f32(np.nan)
        if view_cos < f32(0.5):
            return 4, None, None, None, view_cos
        ratio = f32(maxd / dist) if dist != 0 else f32(np.inf if maxd > 0 else np.nan)
        if math.isnan(ratio):
            return 0, None, None, None, None
        level = int((ratio > w.scale[:len(w.scale) - 1]).sum())
    return 5, u, v, level, view_cos


def search_local_points_numpy(w: World):
    """-> (matches [n_f], view [n_m], nmatches): per point the two smallest candidates under (distance, window position)."""
    ones = np.array([bin(v).count("1") for v in range(256)], np.uint8)
    matches = w.matches.copy()
    taken = np.zeros(w.n_f, bool)
    seen = np.zeros(w.n_m, bool)
    for j in np.flatnonzero(matches >= 0):
        i = matches[j]
        if i >= w.n_m:
            taken[j] = True
            continue
        seen[i] = True
        if w.outlier is not None and w.outlier[j]:
            matches[j] = -1
        else:
            taken[j] = True
    view = np.where(seen, SEEN, NOT_IN_VIEW).astype(np.uint8)
    nm = 0
    for i in range(w.n_m):
        if seen[i] or (w.mask is not None and w.mask[i] == 0):
            continue
        stage, u, v, level, view_cos = frustum_numpy(w, i)
        if stage != 5:
            continue
        view[i] = level
        r = f32(2.5) if view_cos > f32(0.998) else f32(4.0)
        if f32(w.th) != f32(1.0):
            r = f32(r * f32(w.th))
        cand = M.window_numpy(w.kps, w.bounds, u, v, f32(r * w.scale[level]), level - 1, level)  # (sorted by window position)
        cand = cand[~taken[cand]]
        if not len(cand):
            continue
        d = ones[w.desc[cand] ^ w.map_desc[i][None, :]].sum(axis=1, dtype=np.int64)
        order = np.lexsort((np.arange(len(cand)), d))[:2]
        d1, l1 = int(d[order[0]]), int(w.kps["octave"][cand[order[0]]])
        d2, l2 = (int(d[order[1]]), int(w.kps["octave"][cand[order[1]]])) if len(order) > 1 else (256, -1)
        if d1 > TH_HIGH or (l1 == l2 and f32(d1) > f32(f32(w.nnratio) * f32(d2))):
            continue
        j = int(cand[order[0]])
        matches[j] = i
        taken[j] = True
        nm += 1
    return matches, view, nm


# ---- the worlds the host and the GPU test share ----

camera, pose_of, points_seen_at = M.camera, M.pose_of, M.points_seen_at
_keypoints, _flip = M._keypoints, M._flip
EYE = np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32)


def _none_frame():
    return np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)


def make_map(n, seed, pose, K, bounds=BOUNDS, in_view=0.6, scale_factor=1.2, nlevels=NLEVELS):
    """n map points: projections all over the bounds and a margin that leaves about a fifth outside, 8% behind the camera; the
    normal the viewing direction turned by 0 to 3 degrees (viewCos > 0.998), 10 to 55 degrees or, for a seventh, 65 to 120
    degrees; the maximal distance such that every level of the table comes out, a tenth of the points nearer than 0.8 times the
    minimal or farther than 1.2 times the maximal distance; 90% of the mask set."""
    rng = np.random.default_rng(seed)
    scale = scale_table(nlevels, scale_factor)
    w_, h_ = bounds[1] - bounds[0], bounds[3] - bounds[2]
    m = 0.5 * (1.0 / math.sqrt(in_view + 0.2) - 1.0)
    uv = np.stack([rng.uniform(bounds[0] - m * w_, bounds[1] + m * w_, n), rng.uniform(bounds[2] - m * h_, bounds[3] + m * h_, n)], 1)
    depth = rng.uniform(2.0, 10.0, n)
    depth[rng.random(n) < 0.08] *= -1.0
    pts = points_seen_at(pose, K, uv, depth)
    R, t = pose[:9].reshape(3, 3).astype(np.float64), pose[9:].astype(np.float64)
    po = pts.astype(np.float64) - (-R.T @ t)
    dist = np.linalg.norm(po, axis=1)
    dirs = po / dist[:, None]
    kind = rng.choice(3, n, p=[0.4, 0.45, 0.15])
    ang = np.deg2rad(np.where(kind == 0, rng.uniform(0, 3, n), np.where(kind == 1, rng.uniform(10, 55, n), rng.uniform(65, 120, n))))
    perp = np.cross(dirs, rng.normal(size=(n, 3)))
    perp /= np.linalg.norm(perp, axis=1)[:, None]
    normals = np.cos(ang)[:, None] * dirs + np.sin(ang)[:, None] * perp
    level = rng.integers(0, nlevels + 1, n)  # (the last one is beyond the table: clamped)
    maxd = dist * np.where(level == 0, 1.0, scale[np.minimum(level, nlevels - 1)].astype(np.float64)) * rng.uniform(0.86, 0.99, n)
    maxd[level == nlevels] = dist[level == nlevels] * float(scale[-1]) * 1.3
    mind = maxd / float(scale[-1])
    far = rng.random(n)
    mind = np.where(far < 0.05, dist * 1.3, mind)
    maxd = np.where((far >= 0.05) & (far < 0.10), dist / 1.3, maxd)
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    mdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return pts, normals.astype(np.float32), np.stack([mind, maxd], 1).astype(np.float32), mdesc, mask


def make_world(n_m, seed, bounds=BOUNDS, th=1.0, nnratio=0.8, n_extra=None, edge_cases=True, in_view=0.6, have=0.3,
               K=None, scale_factor=1.2, nlevels=NLEVELS, roll_deg=0.0):
    """A map of n_m points (make_map) and a frame built around the projections of those in view: for three quarters of them a
    feature within 0.2, 0.9 or 1.5 window radii, its octave the predicted level or off by one or two, its descriptor the point's
    with 0 to 60 bits flipped (a tenth: 105 to 140, beyond TH_HIGH); for a quarter of those a second feature of the same octave
    with a descriptor as near (what the ratio test rejects); unrelated features; features outside the grid.  The frame already
    has a share `have` of the points its features show, and a few it has no window for; 15% of these entries are outliers."""
    rng = np.random.default_rng(seed)
    K, pose = camera(bounds) if K is None else np.asarray(K, np.float32).reshape(9), pose_of(seed + 1, roll_deg)
    scale = scale_table(nlevels, scale_factor)
    pts, normals, dists, mdesc, mask = make_map(n_m, seed + 2, pose, K, bounds, in_view, scale_factor, nlevels)
    none_k, none_d = _none_frame()
    proj = search_local_points(World(none_k, none_d, pts, normals, dists, mdesc, None, pose, K, bounds, th, nnratio, scale=scale))["proj"]
    feats, descs, shows = [], [], []

    def feature(x, y, octave, desc, shown):
        k = np.zeros(1, KEYPOINT_DTYPE)
        k["x"], k["y"], k["octave"], k["angle"], k["size"], k["class_id"] = x, y, octave, rng.uniform(0, 360), 31.0, -1
        feats.append(k)
        descs.append(desc)
        shows.append(shown)
    for i in range(n_m):
        if proj[i, 5] != 5.0 or rng.random() > 0.75:
            continue
        u, v, r, level = proj[i, 0], proj[i, 1], proj[i, 2], int(proj[i, 3])
        bits = int(rng.integers(105, 141)) if rng.random() < 0.1 else int(rng.integers(0, 61))
        octave = level + int(rng.choice([0, 0, 0, -1, -1, -1, 1, -2]))
        feature(f32(u + r * rng.uniform(-1.0, 1.0) * rng.choice([0.2, 0.9, 1.5])), f32(v + r * rng.uniform(-1.0, 1.0) * 0.6), octave,
                _flip(mdesc[i], bits, rng), i)
        if rng.random() < 0.25:
            feature(f32(u + r * rng.uniform(-0.5, 0.5)), f32(v + r * rng.uniform(-0.5, 0.5)), octave,
                    _flip(mdesc[i], min(bits + int(rng.integers(0, 8)), 200), rng), -1)
    edge = []
    if edge_cases:
        live = (proj[:, 5] == 5.0) & (mask != 0)
        # (the window's sides lie in the grid, whose last half cell PosInGrid leaves out)
        live &= (proj[:, 0] - proj[:, 2] > bounds[0]) & (proj[:, 0] + proj[:, 2] < bounds[1] - 6) & (proj[:, 1] < bounds[3] - 6)
        for i in np.flatnonzero(live)[:12]:
            u, v, r = proj[i, 0], proj[i, 1], proj[i, 2]
            for side, inside in ((1, True), (1, False), (-1, True), (-1, False)):
                x = f32(u + side * r)  # the largest x with |x - u| < r in f32, and the next one
                while not abs(f32(x - u)) < r:
                    x = np.nextafter(x, f32(u), dtype=np.float32)
                if not inside:
                    x = np.nextafter(x, f32(u + side * 1e9), dtype=np.float32)
                feature(x, v, int(proj[i, 3]), _flip(mdesc[i], 20 + len(edge) % 7, rng), -1)
                edge.append((int(i), len(feats) - 1, inside))
    n_extra = n_m // 8 if n_extra is None else n_extra
    extra = _keypoints(n_extra, rng, nlevels=nlevels)
    extra["x"], extra["y"] = rng.uniform(bounds[0], bounds[1], n_extra), rng.uniform(bounds[2], bounds[3], n_extra)
    far = _keypoints(6, rng, nlevels=nlevels)  # outside the grid: beyond the bounds by more than a cell, and one that is no number
    far["x"] = np.array([bounds[0] - 40.0, bounds[1] + 40.0, 100.0, 200.0, np.nan, bounds[1] + 4.0], np.float32)
    far["y"] = np.array([100.0, 100.0, bounds[2] - 40.0, bounds[3] + 40.0, 50.0, bounds[3] + 4.0], np.float32)
    kf = np.concatenate(feats + [extra, far])
    df = np.concatenate([np.array(descs, np.uint8).reshape(-1, 32), rng.integers(0, 256, (n_extra + 6, 32), dtype=np.uint8)])
    shows = np.array(shows + [-1] * (n_extra + 6), np.int64)
    # what the frame has on entry: some of the points its features show, and a few other points for unrelated features
    matches = np.where((shows >= 0) & (rng.random(len(kf)) < have), shows, -1).astype(np.int32)
    unrelated = np.flatnonzero(shows < 0)
    lucky = rng.choice(unrelated, size=min(len(unrelated), max(6, n_m // 50)), replace=False)
    matches[lucky] = rng.integers(0, n_m, len(lucky))
    outlier = ((matches >= 0) & (rng.random(len(kf)) < 0.15)).astype(np.uint8)
    perm = rng.permutation(len(kf))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    w = World(kf[perm], df[perm], pts, normals, dists, mdesc, mask, pose, K, bounds, th, nnratio, matches[perm], outlier[perm],
              scale=scale)
    w.edge = [(i, int(inv[j]), inside) for i, j, inside in edge]
    w.shows = shows[perm]  # per feature: the point it was built around, or -1
    return w


def contention_world(n_clusters=40, seed=21):
    """Clusters: seven map points of one level L >= 1 that project within a pixel of each other, their descriptors a few bits
    from a common one, over four features under all their windows whose descriptors lie 0, 12, 24 and 36 bits from it and whose
    octaves alternate between L and L - 1 (so that the ratio test, which compares equal levels only, lets them pass): the first
    four points take the features one after the other, the last three find everything taken -- six of seven are displaced."""
    rng = np.random.default_rng(seed)
    K, pose = camera(), pose_of(seed + 1)
    scale = scale_table()
    uv, md, lv, fxy, fo, fd = [], [], [], [], [], []
    for c in range(n_clusters):
        centre = np.array([rng.uniform(40, 600), rng.uniform(40, 440)])
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        L = int(rng.integers(1, NLEVELS))
        for _ in range(7):
            uv.append(centre + rng.uniform(-0.8, 0.8, 2))
            md.append(_flip(base, rng.integers(0, 4), rng))
            lv.append(L)
        far_bits = rng.permutation(256)
        for k in range(4):
            fxy.append(centre + rng.uniform(-1.2, 1.2, 2))
            fo.append(L - (k & 1))
            d = base.copy()
            for b in far_bits[:12 * k]:
                d[b >> 3] ^= np.uint8(1 << (b & 7))
            fd.append(d)
    n = len(uv)
    order = rng.permutation(n)
    uv, md, lv = np.array(uv)[order], np.array(md, np.uint8)[order], np.array(lv)[order]
    depth = rng.uniform(2.0, 10.0, n)
    pts = points_seen_at(pose, K, uv, depth)
    R, t = pose[:9].reshape(3, 3).astype(np.float64), pose[9:].astype(np.float64)
    po = pts.astype(np.float64) - (-R.T @ t)
    dist = np.linalg.norm(po, axis=1)
    maxd = dist * scale[lv].astype(np.float64) * 0.93
    kf = _keypoints(len(fxy), rng, np.array(fo))
    kf["x"], kf["y"] = [p[0] for p in fxy], [p[1] for p in fxy]
    perm = rng.permutation(len(kf))
    return World(kf[perm], np.array(fd, np.uint8)[perm], pts, (po / dist[:, None]).astype(np.float32),
                 np.stack([maxd / 4.0, maxd], 1).astype(np.float32), md, None, pose, K)


def _flip_bits(d, bits):
    d = d.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def axis_map(uv, depth, K, level=0, cos=1.0):
    """Points seen with the identity pose at the pixels uv: the normal the viewing direction (scaled by cos), the distances such
    that PredictScale gives `level`."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    depth = np.broadcast_to(np.asarray(depth, np.float64), (len(uv),))
    pts = points_seen_at(EYE, K, uv, depth) if len(uv) else np.zeros((0, 3), np.float32)
    dist = np.linalg.norm(pts.astype(np.float64), axis=1)
    s = scale_table()
    lv = np.broadcast_to(np.asarray(level), (len(uv),))
    maxd = dist * np.where(lv == 0, 0.95, s[lv].astype(np.float64) * 0.95)
    normals = pts.astype(np.float64) / np.maximum(dist, 1e-30)[:, None] * cos
    return pts, normals.astype(np.float32), np.stack([maxd / 4.0, maxd], 1).astype(np.float32)


def order_world():
    """Three points (0, 1, 2) of level 0 and two features A = 0 and B = 1 of octave 0, B outside point 0's window.  d(0, A) = 0;
    d(1, B) = 40 and d(1, A) = 46; d(2, B) = 5 and d(2, A) = 65 (d(A, B) = 60).  Sequentially 0 takes A; point 1 then sees B
    alone and takes it -- with A free its second-best would be A at the same level and 40 > 0.8 * 46 would reject it; point 2
    finds nothing.  "The lowest claimant of its pick wins" lets point 1 fail the ratio test in the first round and gives B to
    point 2."""
    rng = np.random.default_rng(11)
    K = camera()
    A = rng.integers(0, 256, 32, dtype=np.uint8)
    B = _flip_bits(A, range(60))
    md = np.stack([A, _flip_bits(A, list(range(33)) + list(range(100, 113))), _flip_bits(B, range(200, 205))])
    kf = np.zeros(2, KEYPOINT_DTYPE)
    kf["x"], kf["y"], kf["octave"] = [300.0, 303.0], [200.0, 200.0], 0
    uv = np.array([[297.0, 200.0], [301.5, 200.0], [302.0, 200.5]])  # radius 4 (level 0, th 1): point 0 reaches A (3) but not B (6)
    pts, normals, dists = axis_map(uv, 4.0, K, 0, cos=0.9)
    return World(kf, np.stack([A, B]), pts, normals, dists, md, None, EYE, K)


# the second setting: K_ANISO, 5 levels of 1.37, the pose rolled by 89 degrees; 150 features, and 310 under the offset bounds
WORLDS_2 = ("w150@2", "w310_bounds@2")
TWO = dict(roll_deg=89.0, **SECOND)
WORLDS = ("main", "main_th5", "bounds", "w700", "w3000", "contention", "order", "empty_frame", "empty_map")
_worlds = {}


def world(name: str) -> World:
    if name not in _worlds and name in WORLDS_2:
        _worlds[name] = make_world(150, 101, **TWO) if name == "w150@2" else make_world(310, 104, bounds=(-12, 655, -9, 490), **TWO)
    if name not in _worlds:
        none_k, none_d = _none_frame()
        if name == "main":
            w = make_world(600, 1)
        elif name == "main_th5":
            w = make_world(400, 2, th=5.0, nnratio=0.9)
        elif name == "bounds":
            w = make_world(420, 4, bounds=(-12, 655, -9, 490))
        elif name == "w700":  # about 300 features against 700 points: more than one point per thread
            w = make_world(700, 5, edge_cases=False, n_extra=20)
        elif name == "w3000":  # about 1500 features against 3000 points
            w = make_world(3000, 6, edge_cases=False, n_extra=300)
        elif name == "contention":
            w = contention_world()
        elif name == "order":
            w = order_world()
        elif name == "empty_frame":
            b = make_world(80, 8)
            w = World(none_k, none_d, b.points, b.normals, b.dists, b.map_desc, b.mask, b.pose, b.K)
        elif name == "empty_map":
            b = make_world(80, 9)
            w = World(b.kps, b.desc, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2)), none_d, None, b.pose, b.K,
                      matches=np.full(b.n_f, -1, np.int32))
        else:
            raise KeyError(name)
        _worlds[name] = w
    return _worlds[name]


_rules = {}


def rule_worlds():
    """Small worlds, each built around one rule of the statement -> {name: World} (built once).  Identity pose: the camera centre
    is the origin, a point (0, 0, Z) lies at distance Z exactly and projects onto (cx, cy) = (320, 240)."""
    out = _rules
    if out:
        return out
    K = camera()
    rng = np.random.default_rng(77)
    d = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    spots = [(100.0 + 60 * k, 100.0) for k in range(4)]
    nxt = lambda x, to: np.nextafter(f32(x), f32(to), dtype=np.float32)  # noqa: E731

    def frame(xy, desc, octave=0):
        k = np.zeros(len(xy), KEYPOINT_DTYPE)
        k["x"], k["y"], k["octave"] = [p[0] for p in xy], [p[1] for p in xy], octave
        return k, np.ascontiguousarray(desc, np.uint8)

    def four(**kw):
        """Four points over four features with the points' descriptors: everything matches unless a rule says no."""
        pts, nrm, dst = axis_map(spots, 4.0, K)
        a = dict(points=pts, normals=nrm, dists=dst, map_desc=d[:4], mask=None, pose=EYE, K=K)
        a["kps"], a["desc"] = frame(spots, d[:4])
        a.update(kw)
        return World(**a)
    out["all_four"] = four()
    out["mask"] = four(mask=np.array([1, 0, 1, 1], np.uint8))
    # feature 0 has point 2, feature 3 has point 1 and is an outlier: both points are seen; feature 3 is free again
    out["seen_and_outlier"] = four(matches=np.array([2, -1, -1, 1], np.int32), outlier=np.array([0, 0, 0, 1], np.uint8))
    out["seen_no_outlier_array"] = four(matches=np.array([2, -1, -1, 1], np.int32))
    out["bad_entry"] = four(matches=np.array([-1, 4, -5, 99], np.int32), outlier=np.array([0, 1, 0, 0], np.uint8))
    behind = four()
    behind.points[1, 2], behind.points[3, 2] = -4.0, -1e-3
    out["behind_the_camera"] = behind.variant()
    zero = four()
    zero.points[1] = [0.1, 0.0, 0.0]        # PcZ = +0: invz = +inf
    zero.points[2] = [-0.1, -0.1, -0.0]     # PcZ = -0 (with t = -0): not < 0, invz = -inf
    out["zero_depth"] = zero.variant(pose=np.r_[np.eye(3).reshape(9), [0.0, 0.0, -0.0]].astype(np.float32))
    # u exactly on min_x and on max_x (cx = 320 and fx = 500 with X = -+1.28, Z = 2 give 0 and 640 exactly), and just outside
    kb, db = frame([(0.0, 240.0), (630.0, 240.0), (2.0, 240.0), (634.0, 240.0)], d[[0, 1, 0, 1]])
    on = four(kps=kb, desc=db)
    on.points[:] = [[-1.28, 0, 2], [1.28, 0, 2], [f32(-1.2800005), 0, 2], [f32(1.2800005), 0, 2]]
    on.normals[:] = on.points
    on.dists[:] = [1.0, 2.2]
    out["on_the_bounds"] = on.variant()
    # the distance bounds: points on the optical axis at Z = 0.8f * min and 1.2f * max exactly, and one step beyond
    lo, hi = f32(f32(0.8) * f32(5.0)), f32(f32(1.2) * f32(3.0))
    ax = four()
    ax.points[:] = [[0, 0, lo], [0, 0, nxt(lo, 0)], [0, 0, hi], [0, 0, nxt(hi, 9)]]
    ax.normals[:] = [0, 0, 1]
    ax.dists[:] = [[5.0, 9.0], [5.0, 9.0], [1.0, 3.0], [1.0, 3.0]]
    out["distance_bounds"] = ax.variant()
    # viewCos: Z = 4 and a normal (0.8, 0, c) give (4 * c) / 4 = c exactly
    half, close = f32(0.5), f32(0.998)
    vc = four()
    vc.points[:] = [0, 0, 4]
    vc.normals[:] = [[0.8, 0, half], [0.8, 0, nxt(half, 0)], [0.05, 0, close], [0.05, 0, nxt(close, 1)]]
    vc.dists[:] = [1.0, 3.9]
    out["view_cos"] = vc.variant()
    out["view_cos_th3"] = vc.variant(th=3.0)
    # th: a feature 5 pixels from the projection is outside th = 1's window (4) and inside th = 2's (8)
    kt, dt_ = frame([(spots[0][0] + 5.0, 100.0)], d[:1])
    pts, nrm, dst = axis_map(spots[:1], 4.0, K, cos=0.9)
    out["th_1"] = World(kt, dt_, pts, nrm, dst, d[:1], None, EYE, K, th=1.0)
    out["th_2"] = out["th_1"].variant(th=2.0)
    k2, d2 = frame(spots[:2], np.stack([_flip(d[0], 100, rng), _flip(d[1], 101, rng)]))
    pts, nrm, dst = axis_map(spots[:2], 4.0, K)
    out["distance_100_and_101"] = World(k2, d2, pts, nrm, dst, d[:2], None, EYE, K)
    # the ratio test: one point, two features 1 pixel apart with distances 40 and 46 (40 > 0.8 * 46 = 36.8)
    pts, nrm, dst = axis_map(spots[:1], 4.0, K, level=1)
    two = [(spots[0][0] - 0.5, 100.0), (spots[0][0] + 0.5, 100.0)]
    dd = np.stack([_flip(d[0], 40, rng), _flip(d[0], 46, rng)])
    out["ratio_equal_levels"] = World(*frame(two, dd, 1), pts, nrm, dst, d[:1], None, EYE, K)
    out["ratio_different_levels"] = World(*frame(two, dd, np.array([1, 0])), pts, nrm, dst, d[:1], None, EYE, K)
    out["ratio_passes"] = out["ratio_equal_levels"].variant(nnratio=0.9)  # 40 > 0.9 * 46 = 41.4 is false
    out["ratio_second_at_256"] = World(*frame(two[:1], dd[:1], 1), pts, nrm, dst, d[:1], None, EYE, K)
    nf = four()
    nf.points[0, 0], nf.normals[1, 2], nf.dists[2, 0] = np.nan, np.inf, np.nan
    out["nonfinite_point"] = nf.variant()
    out["nonfinite_pose"] = four(pose=np.r_[EYE[:9], [np.nan, 0, 0]].astype(np.float32))
    out["no_features"] = four(kps=np.zeros(0, KEYPOINT_DTYPE), desc=np.zeros((0, 32), np.uint8))
    out["no_points"] = World(*frame(spots, d[:4]), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 32), np.uint8),
                             None, EYE, K)
    return out
