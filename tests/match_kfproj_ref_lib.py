"""ctypes wrapper around tests/cpp/match_kfproj_ref.cpp -- the CPU restatement of the relocalisation overload
ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (include/orbx.h, "matching a keyframe's points by
projection") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary directory, as
tests/match_local_ref_lib.py compiles its source; a second, independently written numpy statement without a grid; the worlds (a
keyframe's map points seen from the lost frame's pose, a current frame around their projections) that
tests/test_match_kfproj_host.py and tests/test_gpu_match_kfproj.py share; and the chain of restatements that is the tail of
Tracking::Relocalization.  TEST INFRASTRUCTURE only."""
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
SRC = os.path.join(ROOT, "tests", "cpp", "match_kfproj_ref.cpp")
KEYPOINT_DTYPE = M.KEYPOINT_DTYPE
RESULT_FIELDS = ("status", "nmatches", "n_points", "n_found", "n_behind_kept", "n_out_image", "n_out_distance", "n_with_candidates",
                 "n_over_dist", "n_displaced", "n_rot_removed", "n_outliers_cleared", "rounds")
COMPARED_FIELDS = RESULT_FIELDS[:-1]  # (rounds is the device's own count)
BAD_INPUT, NONFINITE = 2, 4
NLEVELS = M.NLEVELS
BOUNDS = M.BOUNDS
f32 = np.float32
_L = None


def build(src=SRC) -> ctypes.CDLL:
    """Compiles a restatement source (lib(): the committed one; tests/test_camera_mutants_host.py: an altered copy) and binds it."""
    d = tempfile.mkdtemp(prefix="match_kfproj_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libmatch_kfproj_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", src, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("match_kfproj_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.kpr_features_in_area.argtypes = [vp, i32, vp, fl, fl, fl, i32, i32, vp]
    L.kpr_search_by_projection.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, fl, i32, i32, vp, vp, vp, vp, vp,
                                           vp, vp]
    L.kpr_search_by_projection.restype = None
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
    """One pair: the keyframe (kps_k, desc_k; its map points: points [n_k, 3], dists [n_k, 2] = min, max, mask or None, point_desc
    or None), the current frame (kps_c, desc_c), its pose [12], K [9], the bounds, th, orb_dist, the orientation switch, the
    matches the current frame has on entry [n_c] and its outlier flags (or None)."""

    def __init__(self, kps_k, desc_k, kps_c, desc_c, points, dists, mask, pose, K, bounds=BOUNDS, th=10.0, orb_dist=100, ori=True,
                 point_desc=None, matches=None, outlier=None, scale=None):
        self.kps_k, self.kps_c = np.ascontiguousarray(kps_k, KEYPOINT_DTYPE), np.ascontiguousarray(kps_c, KEYPOINT_DTYPE)
        self.desc_k = np.ascontiguousarray(desc_k, np.uint8).reshape(-1, 32)
        self.desc_c = np.ascontiguousarray(desc_c, np.uint8).reshape(-1, 32)
        self.points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.dists = np.ascontiguousarray(dists, np.float32).reshape(-1, 2)
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.point_desc = None if point_desc is None else np.ascontiguousarray(point_desc, np.uint8).reshape(-1, 32)
        self.pose, self.K = np.ascontiguousarray(pose, np.float32).reshape(12), np.ascontiguousarray(K, np.float32).reshape(9)
        self.bounds, self.th, self.orb_dist, self.ori = tuple(int(b) for b in bounds), float(th), int(orb_dist), bool(ori)
        self.n_k, self.n_c = len(self.kps_k), len(self.kps_c)
        self.matches = np.full(self.n_c, -1, np.int32) if matches is None else np.ascontiguousarray(matches, np.int32)
        self.outlier = None if outlier is None else np.ascontiguousarray(outlier, np.uint8)
        self.scale = scale_table() if scale is None else np.ascontiguousarray(scale, np.float32)
        assert len(self.desc_k) == self.n_k == len(self.points) == len(self.dists)
        assert len(self.desc_c) == self.n_c == len(self.matches)
        self._expected = None

    def variant(self, **kw):
        """The same pair with some inputs replaced (a fresh World: nothing cached is shared)."""
        a = dict(kps_k=self.kps_k.copy(), desc_k=self.desc_k, kps_c=self.kps_c.copy(), desc_c=self.desc_c, points=self.points.copy(),
                 dists=self.dists.copy(), mask=self.mask, pose=self.pose, K=self.K, bounds=self.bounds, th=self.th, orb_dist=self.orb_dist,
                 ori=self.ori, point_desc=self.point_desc, matches=self.matches.copy(), outlier=self.outlier, scale=self.scale)
        a.update(kw)
        return World(**a)

    def query_desc(self):
        return self.desc_k if self.point_desc is None else self.point_desc

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
    n = lib().kpr_features_in_area(_p(k), len(k), _p(b), float(x), float(y), float(r), int(min_level), int(max_level), _p(out))
    return out[:n].copy()


def search_by_projection(w: World):
    """The restatement -> dict(matches [n_c] int32, res {field: value}, proj [n_k, 6] (u, v, radius, level, zc < 0, stage),
    outcome [n_k], alone [n_k], best [n_k])."""
    m = np.full(max(w.n_c, 1), -1, np.int32)
    m[:w.n_c] = w.matches
    nk = max(w.n_k, 1)
    res = np.zeros(len(RESULT_FIELDS), np.int32)
    proj, out, alone, best = np.zeros((nk, 6), np.float32), np.zeros(nk, np.int32), np.zeros(nk, np.int32), np.zeros(nk, np.int32)
    b = np.ascontiguousarray(w.bounds, np.int32)
    lib().kpr_search_by_projection(_p(w.kps_k), _p(w.desc_k), w.n_k, _p(w.kps_c), _p(w.desc_c), w.n_c, _p(w.points), _p(w.dists),
                                   _p(w.mask), _p(w.point_desc), _p(w.pose), _p(w.K), _p(b), _p(w.scale), len(w.scale), w.th,
                                   w.orb_dist, int(w.ori), _p(m), _p(w.outlier), _p(res), _p(proj), _p(out), _p(alone), _p(best))
    return dict(matches=m[:w.n_c].copy(), res=dict(zip(RESULT_FIELDS, (int(v) for v in res))), proj=proj[:w.n_k], outcome=out[:w.n_k],
                alone=alone[:w.n_k], best=best[:w.n_k])


# ---- the second statement: numpy; no grid; per point all candidates sorted by (distance, window position), the first untaken ----

def project_numpy(w: World, i):
    """Rules 2 and 3 for point i -> (stage, u, v, level); stage as the restatement's proj column."""
    P, (mind, maxd) = w.points[i], w.dists[i]
    if not (np.isfinite(P).all() and np.isfinite(mind) and np.isfinite(maxd) and np.isfinite(w.pose).all()):
        return 0, None, None, None
    R, t = w.pose[:9], w.pose[9:]
    with np.errstate(all="ignore"):
        c = [f32(f32(f32(f32(R[3 * k] * P[0]) + f32(R[3 * k + 1] * P[1])) + f32(R[3 * k + 2] * P[2])) + t[k]) for k in range(3)]
        invz = f32(f32(1.0) / c[2])
        u = f32(f32(f32(w.K[0] * c[0]) * invz) + w.K[2])
        v = f32(f32(f32(w.K[4] * c[1]) * invz) + w.K[5])
        if not (math.isfinite(u) and math.isfinite(v)) or u < w.bounds[0] or u > w.bounds[1] or v < w.bounds[2] or v > w.bounds[3]:
            return 2, None, None, None
        ow = [f32(-f32(f32(f32(R[k] * t[0]) + f32(R[3 + k] * t[1])) + f32(R[6 + k] * t[2]))) for k in range(3)]
        po = [float(f32(P[k] - ow[k])) for k in range(3)]
        dist = f32(math.sqrt((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2]))
        if dist < f32(f32(0.8) * mind) or dist > f32(f32(1.2) * maxd):
            return 3, None, None, None
        ratio = f32(maxd / dist) if dist != 0 else f32(np.inf if maxd > 0 else np.nan)
        if math.isnan(ratio):
            return 0, None, None, None
        level = int((ratio > w.scale[:len(w.scale) - 1]).sum())
    return 5, u, v, level


def search_by_projection_numpy(w: World):
    """-> (matches [n_c], nmatches)."""
    ones = np.array([bin(v).count("1") for v in range(256)], np.uint8)
    matches = w.matches.copy()
    taken = np.zeros(w.n_c, bool)
    found = np.zeros(w.n_k, bool)
    for j in np.flatnonzero(matches >= 0):
        i = matches[j]
        if i >= w.n_k:
            taken[j] = True
            continue
        found[i] = True
        if w.outlier is not None and w.outlier[j]:
            matches[j] = -1
        else:
            taken[j] = True
    q = w.query_desc()
    bins = np.full(w.n_c, -2, np.int64)  # -2: no new match; -1: a new match in no bin
    for i in range(w.n_k):
        if found[i] or (w.mask is not None and w.mask[i] == 0):
            continue
        stage, u, v, level = project_numpy(w, i)
        if stage != 5:
            continue
        cand = M.window_numpy(w.kps_c, w.bounds, u, v, f32(f32(w.th) * w.scale[level]), level - 1, level + 1)  # (by window position)
        if not len(cand):
            continue
        d = ones[w.desc_c[cand] ^ q[i][None, :]].sum(axis=1, dtype=np.int64)
        ranked = cand[np.lexsort((np.arange(len(cand)), d))]
        free = [int(j) for j in ranked if not taken[j]]
        if not free:
            continue
        j = free[0]
        if int(ones[w.desc_c[j] ^ q[i]].sum()) > min(w.orb_dist, 255):  # (a candidate at 256 is never below the start value)
            continue
        matches[j] = i
        taken[j] = True
        rot = f32(w.kps_k["angle"][i]) - f32(w.kps_c["angle"][j])
        if rot < 0:
            rot = f32(rot + f32(360.0))
        x = float(f32(rot * f32(f32(30) / f32(360.0))))
        bins[j] = -1
        if math.isfinite(x):
            b = int(M._round_half_away(x))
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
        bins[lose] = -2
    return matches, int((bins > -2).sum())


# ---- the worlds the host and the GPU test share ----

camera, pose_of, points_seen_at = M.camera, M.pose_of, M.points_seen_at
_keypoints, _flip = M._keypoints, M._flip
EYE = np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32)


def _none_frame():
    return np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)


def _distances(pts, pose, level, rng=None, scale_factor=1.2, nlevels=NLEVELS):
    """(min, max) distances such that the table PredictScale gives `level` (an entry nlevels is beyond the table: clamped)."""
    scale = scale_table(nlevels, scale_factor)
    R, t = pose[:9].reshape(3, 3).astype(np.float64), pose[9:].astype(np.float64)
    dist = np.linalg.norm(pts.astype(np.float64) - (-R.T @ t), axis=1)
    level = np.broadcast_to(np.asarray(level), dist.shape)
    jitter = 0.93 if rng is None else rng.uniform(0.86, 0.99, len(dist))
    maxd = dist * np.where(level == 0, 1.0, scale[np.minimum(level, nlevels - 1)].astype(np.float64)) * jitter
    maxd = np.where(level == nlevels, dist * float(scale[-1]) * 1.3, maxd)
    return dist, np.stack([maxd / float(scale[-1]), maxd], 1)


def make_world(n_k, seed, bounds=BOUNDS, th=10.0, orb_dist=100, ori=True, n_extra=None, edge_cases=True, have=0.3, with_point_desc=False,
               with_outlier=True, K=None, scale_factor=1.2, nlevels=NLEVELS, roll_deg=0.0):
    """A keyframe of n_k features with map points: projections all over the bounds and a margin that leaves about a fifth outside,
    8% behind the camera (they project inside all the same), every level of the table, a tenth nearer than 0.8 times the minimal
    or farther than 1.2 times the maximal distance, 90% of the mask set, 12% twins of an earlier point (the same position, a
    descriptor a few bits away: what displaces).  The current frame is built around the projections of the searched points: for
    three quarters a feature within 0.2, 0.9 or 1.5 window radii, its octave the level or off by one or two, its descriptor the
    point's with 0 to 60, 66 to 99 or 105 to 140 bits flipped, its angle the keyframe's minus 40 degrees plus noise wide enough
    that bins lose; unrelated features; features outside the grid.  The frame already has a share `have` of the points its
    features show, and a few for unrelated features; 15% of these entries are outliers."""
    rng = np.random.default_rng(seed)
    K, pose = camera(bounds) if K is None else np.asarray(K, np.float32).reshape(9), pose_of(seed + 1, roll_deg)
    scale = scale_table(nlevels, scale_factor)
    kk = _keypoints(n_k, rng, nlevels=nlevels)
    dk = rng.integers(0, 256, (n_k, 32), dtype=np.uint8)
    w_, h_ = bounds[1] - bounds[0], bounds[3] - bounds[2]
    uv = np.stack([rng.uniform(bounds[0] - 0.06 * w_, bounds[1] + 0.06 * w_, n_k), rng.uniform(bounds[2] - 0.06 * h_, bounds[3] + 0.06 * h_, n_k)], 1)
    depth = rng.uniform(2.0, 10.0, n_k)
    depth[rng.random(n_k) < 0.08] *= -1.0
    pts = points_seen_at(pose, K, uv, depth)
    dist, dists = _distances(pts, pose, rng.integers(0, nlevels + 1, n_k), rng, scale_factor, nlevels)
    far = rng.random(n_k)
    dists[:, 0] = np.where(far < 0.05, dist * 1.3, dists[:, 0])
    dists[:, 1] = np.where((far >= 0.05) & (far < 0.10), dist / 1.3, dists[:, 1])
    for i in np.flatnonzero(rng.random(n_k) < 0.12):
        if i > 0:
            src = int(rng.integers(0, i))
            pts[i], dists[i], dk[i], kk["angle"][i] = pts[src], dists[src], _flip(dk[src], rng.integers(0, 4), rng), kk["angle"][src]
    mask = (rng.random(n_k) < 0.9).astype(np.uint8)
    pdesc = np.stack([_flip(d, rng.integers(0, 9), rng) for d in dk]) if with_point_desc and n_k else None
    src_desc = dk if pdesc is None else pdesc
    none_k, none_d = _none_frame()
    proj = search_by_projection(World(kk, dk, none_k, none_d, pts, dists, None, pose, K, bounds, th, orb_dist, ori, scale=scale))["proj"]
    feats, descs, shows = [], [], []

    def feature(x, y, octave, desc, shown, angle):
        k = np.zeros(1, KEYPOINT_DTYPE)
        k["x"], k["y"], k["octave"], k["angle"], k["size"], k["class_id"] = x, y, octave, angle, 31.0, -1
        feats.append(k)
        descs.append(desc)
        shows.append(shown)
    for i in range(n_k):
        if proj[i, 5] != 5.0 or rng.random() > 0.75:
            continue
        u, v, r, level = proj[i, 0], proj[i, 1], proj[i, 2], int(proj[i, 3])
        kind = rng.random()
        bits = int(rng.integers(0, 61)) if kind < 0.7 else int(rng.integers(66, 100)) if kind < 0.85 else int(rng.integers(105, 141))
        octave = level + int(rng.choice([0, 0, 0, -1, 1, 1, -1, 2, -2]))
        feature(f32(u + r * rng.uniform(-1.0, 1.0) * rng.choice([0.2, 0.9, 1.5])), f32(v + r * rng.uniform(-1.0, 1.0) * 0.6), octave,
                _flip(src_desc[i], bits, rng), i, f32((float(kk["angle"][i]) - 40.0 + rng.normal(0.0, 9.0)) % 360.0))
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
                feature(x, v, int(proj[i, 3]), _flip(src_desc[i], 20 + len(edge) % 7, rng), -1, f32((float(kk["angle"][i]) - 40.0) % 360.0))
                edge.append((int(i), len(feats) - 1, inside))
    n_extra = n_k // 8 if n_extra is None else n_extra
    extra = _keypoints(n_extra, rng, nlevels=nlevels)
    extra["x"], extra["y"] = rng.uniform(bounds[0], bounds[1], n_extra), rng.uniform(bounds[2], bounds[3], n_extra)
    outside = _keypoints(6, rng, nlevels=nlevels)  # outside the grid: beyond the bounds by more than a cell, and one that is no number
    outside["x"] = np.array([bounds[0] - 40.0, bounds[1] + 40.0, 100.0, 200.0, np.nan, bounds[1] + 4.0], np.float32)
    outside["y"] = np.array([100.0, 100.0, bounds[2] - 40.0, bounds[3] + 40.0, 50.0, bounds[3] + 4.0], np.float32)
    kc = np.concatenate(feats + [extra, outside])
    dc = np.concatenate([np.array(descs, np.uint8).reshape(-1, 32), rng.integers(0, 256, (n_extra + 6, 32), dtype=np.uint8)])
    shows = np.array(shows + [-1] * (n_extra + 6), np.int64)
    matches = np.where((shows >= 0) & (rng.random(len(kc)) < have), shows, -1).astype(np.int32)
    unrelated = np.flatnonzero(shows < 0)
    if have > 0:
        lucky = rng.choice(unrelated, size=min(len(unrelated), max(6, n_k // 50)), replace=False)
        matches[lucky] = rng.integers(0, n_k, len(lucky))
    outlier = ((matches >= 0) & (rng.random(len(kc)) < 0.15)).astype(np.uint8) if with_outlier else None
    perm = rng.permutation(len(kc))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    w = World(kk, dk, kc[perm], dc[perm], pts, dists, mask, pose, K, bounds, th, orb_dist, ori, pdesc, matches[perm],
              None if outlier is None else outlier[perm], scale=scale)
    w.edge = [(i, int(inv[j]), inside) for i, j, inside in edge]
    w.shows = shows[perm]  # per feature: the point it was built around, or -1
    return w


def contention_world(n_clusters=40, seed=21):
    """Clusters: seven points of one level L >= 1 that project within a pixel of each other, their descriptors a few bits from a
    common one, over four features under all their windows whose descriptors lie 0, 12, 24 and 36 bits from it: the first four
    points take the features one after the other, the last three find everything taken -- six of seven are displaced."""
    rng = np.random.default_rng(seed)
    K, pose = camera(), pose_of(seed + 1)
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
    pts = points_seen_at(pose, K, uv, rng.uniform(2.0, 10.0, n))
    _, dists = _distances(pts, pose, lv)
    kk = _keypoints(n, rng)
    kc = _keypoints(len(fxy), rng, np.array(fo))
    kc["x"], kc["y"] = [p[0] for p in fxy], [p[1] for p in fxy]
    perm = rng.permutation(len(kc))
    return World(kk, md, kc[perm], np.array(fd, np.uint8)[perm], pts, dists, None, pose, K, ori=False)


def _flip_bits(d, bits):
    d = d.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def order_world():
    """Three points (0, 1, 2) of level 0 whose windows (th 15) share the candidates A = feature 0 and B = feature 1 of the current
    frame, with d(0, A) = 0, d(1, A) = 1, d(1, B) = 5, d(2, B) = 2, d(2, A) = 8, and B outside point 0's window.  The sequential
    answer is 0 -> A, 1 -> B, 2 -> none; "the lowest claimant of its first choice wins" gives 2 -> B."""
    rng = np.random.default_rng(11)
    K = camera()
    A = rng.integers(0, 256, 32, dtype=np.uint8)
    B = _flip_bits(A, range(6))
    dk = np.stack([A, _flip_bits(A, [0]), _flip_bits(B, [100, 101])])
    kk = np.zeros(3, KEYPOINT_DTYPE)
    kk["angle"] = 10.0
    kc = np.zeros(2, KEYPOINT_DTYPE)
    kc["x"], kc["y"], kc["octave"], kc["angle"] = [300.0, 310.0], [200.0, 200.0], 0, 10.0
    uv = np.array([[290.0, 200.0], [305.0, 200.0], [306.0, 201.0]])  # window radius 15: point 0 reaches A (10) but not B (20)
    pts = points_seen_at(EYE, K, uv, np.full(3, 4.0))
    _, dists = _distances(pts, EYE, 0)
    return World(kk, dk, kc, np.stack([A, B]), pts, dists, None, EYE, K, th=15.0)


# the second setting: K_ANISO, 5 levels of 1.37, the pose rolled by 89 degrees; 150 features, and 310 under the offset bounds
WORLDS_2 = ("w150@2", "w310_bounds@2")
TWO = dict(roll_deg=89.0, **SECOND)
WORLDS = ("main", "main_th3", "bounds", "pdesc", "w700", "contention", "order", "empty_frame", "empty_keyframe")
_worlds = {}


def world(name: str) -> World:
    if name not in _worlds and name in WORLDS_2:
        _worlds[name] = make_world(150, 101, **TWO) if name == "w150@2" else make_world(310, 104, bounds=(-12, 655, -9, 490), **TWO)
    if name not in _worlds:
        none_k, none_d = _none_frame()
        if name == "main":
            w = make_world(600, 1)
        elif name == "main_th3":
            w = make_world(400, 2, th=3.0, orb_dist=64, with_outlier=False)
        elif name == "bounds":
            w = make_world(420, 4, bounds=(-12, 655, -9, 490))
        elif name == "pdesc":
            w = make_world(300, 3, with_point_desc=True, ori=False)
        elif name == "w700":  # more than one point per thread, and more than one slice of the pass
            w = make_world(700, 5, edge_cases=False, n_extra=20)
        elif name == "contention":
            w = contention_world()
        elif name == "order":
            w = order_world()
        elif name == "empty_frame":
            b = make_world(80, 8)
            w = World(b.kps_k, b.desc_k, none_k, none_d, b.points, b.dists, b.mask, b.pose, b.K)
        elif name == "empty_keyframe":
            b = make_world(80, 9)
            w = World(none_k, none_d, b.kps_c, b.desc_c, np.zeros((0, 3)), np.zeros((0, 2)), None, b.pose, b.K)
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

    def frame(xy, desc, octave=0, angle=10.0):
        k = np.zeros(len(xy), KEYPOINT_DTYPE)
        k["x"], k["y"], k["octave"], k["angle"] = [p[0] for p in xy], [p[1] for p in xy], octave, angle
        return k, np.ascontiguousarray(desc, np.uint8)

    def pair(uv, cxy, desc_k, desc_c, level=0, depth=4.0, **kw):
        """Points seen at the pixels uv (windows of radius 10 * scale[level]) over the features cxy."""
        uv = np.asarray(uv, np.float64).reshape(-1, 2)
        pts = points_seen_at(EYE, K, uv, np.broadcast_to(np.asarray(depth, np.float64), (len(uv),))) if len(uv) else np.zeros((0, 3), np.float32)
        dists = _distances(pts, EYE, level)[1] if len(uv) else np.zeros((0, 2))
        kk, dk = frame([(0.0, 0.0)] * len(uv), desc_k, angle=kw.pop("ang_k", 10.0))
        kc, dc = frame(cxy, desc_c, kw.pop("oct_c", 0), kw.pop("ang_c", 10.0))
        return World(kk, dk, kc, dc, pts, dists, kw.pop("mask", None), kw.pop("pose", EYE), K, **kw)

    def four(**kw):
        """Four points over four features with the points' descriptors, 60 pixels apart: everything matches unless a rule says no."""
        return pair(spots, spots, d[:4], d[:4], **kw)
    out["all_four"] = four()
    out["mask"] = four(mask=np.array([1, 0, 1, 1], np.uint8))
    # feature 0 has point 2, feature 3 has point 1 and is an outlier: both points are found; feature 3 is free again
    out["found_and_outlier"] = four(matches=np.array([2, -1, -1, 1], np.int32), outlier=np.array([0, 0, 0, 1], np.uint8))
    out["found_no_outlier_array"] = four(matches=np.array([2, -1, -1, 1], np.int32))
    out["bad_entry"] = four(matches=np.array([-1, 4, -5, 99], np.int32), outlier=np.array([0, 1, 0, 0], np.uint8))
    out["behind_the_camera"] = pair(spots, spots, d[:4], d[:4], depth=[4.0, -4.0, 4.0, -1e-3])
    zero = four()
    zero.points[1] = [0.1, 0.0, 0.0]        # zc = +0: invz = +inf
    zero.points[2] = [-0.1, -0.1, -0.0]     # zc = -0 (with t = -0): invz = -inf
    out["zero_depth"] = zero.variant(pose=np.r_[np.eye(3).reshape(9), [0.0, 0.0, -0.0]].astype(np.float32))
    # u exactly on min_x and on max_x (cx = 320 and fx = 500 with X = -+1.28, Z = 2 give 0 and 640 exactly), and just outside
    on = pair(spots, [(0.0, 240.0), (630.0, 240.0), (2.0, 240.0), (634.0, 240.0)], d[:4], d[[0, 1, 0, 1]])
    on.points[:] = [[-1.28, 0, 2], [1.28, 0, 2], [f32(-1.2800005), 0, 2], [f32(1.2800005), 0, 2]]
    on.dists[:] = [1.0, 2.2]
    out["on_the_bounds"] = on.variant()
    # the distance bounds: points on the optical axis at Z = 0.8f * min and 1.2f * max exactly, and one step beyond
    lo, hi = f32(f32(0.8) * f32(5.0)), f32(f32(1.2) * f32(3.0))
    ax = four()
    ax.points[:] = [[0, 0, lo], [0, 0, nxt(lo, 0)], [0, 0, hi], [0, 0, nxt(hi, 9)]]
    ax.dists[:] = [[5.0, 9.0], [5.0, 9.0], [1.0, 3.0], [1.0, 3.0]]
    out["distance_bounds"] = ax.variant()
    # the level window: a point of level 3 over features of octaves 1, 2, 4 and 5 a pixel around its projection; the one at
    # level + 1 carries the point's descriptor
    lw = [(spots[0][0] - 1.0, 100.0), (spots[0][0] + 1.0, 100.0), (spots[0][0], 101.0), (spots[0][0], 99.0)]
    out["level_window"] = pair(spots[:1], lw, d[:1], np.stack([d[0], _flip(d[0], 30, rng), d[0], d[0]]), level=3,
                               oct_c=np.array([1, 2, 4, 5]))
    # orb_dist: candidates at 64, 65, 100 and 101 bits
    far = np.stack([_flip(d[k], b, rng) for k, b in enumerate((64, 65, 100, 101))])
    out["orb_dist_64"] = pair(spots, spots, d[:4], far, orb_dist=64)
    out["orb_dist_100"] = pair(spots, spots, d[:4], far, orb_dist=100)
    out["orb_dist_0"] = pair(spots, spots, d[:4], np.stack([d[0], _flip(d[1], 1, rng), d[2], d[3]]), orb_dist=0)
    out["orb_dist_256"] = pair(spots, spots, d[:4], np.stack([d[4], d[5], d[6], ~d[3]]), orb_dist=256)
    # the histogram: six new matches at rotation 0, two at 90 degrees, one at 180, one at 270 -- and two matches the frame has on
    # entry at 270 degrees, which would make that bin the second largest if they voted.  They do not: 270 loses to 180 (the same
    # size, the smaller bin), its NEW match goes, the entry's two stay
    n = 10
    sp = [(40.0 + 45 * (k % 13), 60.0 + 90 * (k // 13)) for k in range(n + 2)]
    dd = rng.integers(0, 256, (n + 2, 32), dtype=np.uint8)
    ang_c = np.array([10.0] * 6 + [280.0, 280.0, 190.0, 100.0, 100.0, 100.0], np.float32)  # rot 0 ... 90 90 180 270 | 270 270
    entry = np.array([-1] * n + [n, n + 1], np.int32)
    out["histogram_new_matches_only"] = pair(sp, sp, dd, dd, ang_c=ang_c, matches=entry)
    out["no_orientation"] = out["histogram_new_matches_only"].variant(ori=False)
    out["point_descriptors"] = pair(spots, spots, d[4:8], d[:4], point_desc=d[:4])
    out["frame_descriptors"] = pair(spots, spots, d[4:8], d[:4])
    nf = four()
    nf.points[0, 0], nf.dists[2, 0] = np.nan, np.nan
    out["nonfinite_point"] = nf.variant()
    out["nonfinite_pose"] = four(pose=np.r_[EYE[:9], [np.nan, 0, 0]].astype(np.float32))
    out["no_features"] = pair(spots, [], d[:4], d[:0])
    out["no_points"] = pair([], spots, d[:0], d[:4])
    return out


# ---- the tail of Tracking::Relocalization as a chain of restatements (pose_ref, match_kfproj_ref) ----

def relocalize_refine(w: World, pose0, row, cap):
    """Relocalization behind PnPsolver for one (lost frame, candidate keyframe) pair: `row` [n_c] holds the PnP inliers' points
    (indices into the keyframe), pose0 [12] the PnP pose -> dict(stage, n_good, pose [12], row [n_c], trace).  The stages are
    those of ORBextractor.relocalize_refine_pairs_device; ORBmatcher(0.9, true): the orientation check is on."""
    import pose_ref_lib as PR
    kps_row, pts_row, mask_row = np.zeros(cap, KEYPOINT_DTYPE), np.zeros((cap, 3), np.float32), np.zeros(cap, np.uint8)
    kps_row[:w.n_c], pts_row[:w.n_k] = w.kps_c, w.points
    mask_row[:w.n_k] = 1 if w.mask is None else w.mask
    row = np.ascontiguousarray(row, np.int32).copy()
    pose = np.ascontiguousarray(pose0, np.float32).copy()
    trace = []

    def optimise():
        full = np.full(cap, -1, np.int32)
        full[:w.n_c] = row
        p, flags, _, _ = PR.pose_optimize(PR.World(kps_row, w.n_c, full, pts_row, mask_row, pose.copy(), w.K))
        pose[:] = np.r_[np.asarray(p["R"], np.float32).reshape(9), np.asarray(p["tcw"], np.float32)]
        return int(p["n_inliers"]), flags[:w.n_c].astype(np.uint8)

    def search(th, orb_dist, outl):
        e = w.variant(pose=pose.copy(), matches=row.copy(), outlier=outl, th=th, orb_dist=orb_dist, ori=True).expected()
        row[:] = e["matches"]
        return e["res"]["nmatches"]
    good, flags = optimise()                                        # 1
    stage = 1
    trace.append(good)
    if good >= 10:
        if good >= 50:
            row[flags != 0] = -1
        else:
            extra = search(10.0, 100, flags)                        # 2
            stage = 2
            trace.append(extra)
            if extra + good >= 50:
                good, flags = optimise()                            # 3
                stage = 3
                trace.append(good)
                if 30 < good < 50:
                    extra = search(3.0, 64, None)                   # 4
                    stage = 4
                    trace.append(extra)
                    if good + extra >= 50:
                        good, flags = optimise()                    # 5
                        stage = 5
                        trace.append(good)
                        row[flags != 0] = -1
    return dict(stage=stage, n_good=good, pose=pose, row=row, trace=trace)


# ---- four candidate keyframes against one lost frame, built so that the chain above provably takes each of its paths ----

CHAIN = ("enough_at_once", "dropped", "both_searches", "too_few_additional")
CHAIN_CAP = 512
# per candidate, groups of keyframe points (count, rotation of their feature in degrees, kind): "in" = in the row on entry (a PnP
# inlier), its feature at the projection; "gross" = in the row on entry, its feature 30 pixels off; "good" = not in the row, a
# feature at the projection; "bad" = not in the row, a feature six level-scaled pixels off: inside the window of th 10, an outlier
# of the optimisation.  both_searches: 20 inliers; the first search adds 6 + 12 + 9 + 9 = 36 (the 8 at 180 degrees are the fourth
# bin and go), 56 >= 50; the optimisation keeps 20 + 6 + 9 + 9 = 44; the second search finds the 8 alone in their bin, 52 >= 50.
_CHAIN_PLAN = dict(enough_at_once=[(70, 0, "in")], dropped=[(8, 0, "in"), (3, 0, "gross")],
                   both_searches=[(20, 0, "in"), (6, 0, "good"), (12, 0, "bad"), (9, 90, "good"), (9, 270, "good"), (8, 180, "good")],
                   too_few_additional=[(15, 0, "in"), (10, 0, "good")])
_chain = {}


def chain_world(name: str):
    """-> (World with the start pose and the entry row, pose0 [12], row [n_c], capacity); the four share the lost frame."""
    if not _chain:
        rng = np.random.default_rng(303)
        K, pose = camera(), pose_of(304)
        scale = scale_table()
        none_k, none_d = _none_frame()
        feats, descs, per = [], [], {}
        for cand, groups in _CHAIN_PLAN.items():
            n = sum(g[0] for g in groups)
            uv = np.stack([rng.uniform(40, 600, n), rng.uniform(40, 440, n)], 1)
            pts = points_seen_at(pose, K, uv, rng.uniform(4.0, 10.0, n))
            _, dists = _distances(pts, pose, rng.integers(0, NLEVELS, n))
            kk = _keypoints(n, rng)
            kk["angle"] = (rng.integers(0, 1440, n) * 0.25).astype(np.float32)  # (quarter degrees: the rotations below are exact)
            dk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            proj = search_by_projection(World(kk, dk, none_k, none_d, pts, dists, None, pose, K))["proj"]
            assert np.all(proj[:, 5] == 5.0)
            entries, i = [], 0
            for count, rot, kind in groups:
                for _ in range(count):
                    lv = int(proj[i, 3])
                    off = 6.0 * float(scale[lv]) if kind == "bad" else 30.0 if kind == "gross" else 0.0
                    k = np.zeros(1, KEYPOINT_DTYPE)
                    k["x"], k["y"] = f32(proj[i, 0] + off + rng.normal(0.0, 0.2)), f32(proj[i, 1] + rng.normal(0.0, 0.2))
                    k["octave"], k["angle"], k["size"], k["class_id"] = lv, f32((float(kk["angle"][i]) - rot) % 360.0), 31.0, -1
                    if kind in ("in", "gross"):
                        entries.append((len(feats), i))
                    feats.append(k)
                    descs.append(_flip(dk[i], rng.integers(0, 20), rng))
                    i += 1
            per[cand] = (kk, dk, pts, dists, entries)
        extra = _keypoints(30, rng)
        kc = np.concatenate(feats + [extra])
        dc = np.concatenate([np.array(descs, np.uint8), rng.integers(0, 256, (30, 32), dtype=np.uint8)])
        perm = rng.permutation(len(kc))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        kc, dc = kc[perm], dc[perm]
        pose0 = pose.copy()
        pose0[9:] += np.array([0.01, -0.008, 0.012], np.float32)
        for cand, (kk, dk, pts, dists, entries) in per.items():
            row = np.full(len(kc), -1, np.int32)
            for j, i in entries:
                row[inv[j]] = i
            _chain[cand] = (World(kk, dk, kc, dc, pts, dists, None, pose0, K, matches=row), pose0.copy(), row, CHAIN_CAP)
    return _chain[name]
