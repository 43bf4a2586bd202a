"""ctypes wrapper around tests/cpp/match_scw_ref.cpp -- the CPU restatement of the loop-closing overload
ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) and of the composition Scw = S12 * Tmw (include/orbx.h, "loop
closing: matching the loop's points under Scw") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary
directory, as tests/match_kfproj_ref_lib.py compiles its source; a second, independently written numpy statement without a grid
and without claim rounds (a brute-force window over all features, a plain loop over the points); and the worlds that
tests/test_match_scw_host.py and tests/test_gpu_match_scw.py share.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

import match_local_ref_lib as ML
import match_proj_ref_lib as M
from pose_ref_lib import K_ANISO, NLEVELS_2, SCALE_FACTOR_2, SECOND  # noqa: F401 (the second setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "match_scw_ref.cpp")
KEYPOINT_DTYPE = M.KEYPOINT_DTYPE
RESULT_FIELDS = ("status", "nmatches", "n_total", "n_points", "n_found", "n_unmapped", "n_behind", "n_out_image", "n_out_distance",
                 "n_out_angle", "n_with_candidates", "n_over_dist", "n_displaced", "rounds")
COMPARED_FIELDS = RESULT_FIELDS[:-1]  # (rounds is the device's own count)
BAD_INPUT, NONFINITE, TAKEN_UNMAPPED = 2, 4, -2
STAGES = ("none", "dropped", "behind", "out_image", "out_distance", "out_angle", "searched")
NLEVELS = M.NLEVELS
TH_LOW = 50
BOUNDS = M.BOUNDS
NO_POINT = np.iinfo(np.int32).max  # a table entry that names no point of any set: never followed
f32 = np.float32
_L = None


def build(src=SRC) -> ctypes.CDLL:
    d = tempfile.mkdtemp(prefix="match_scw_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libmatch_scw_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", src, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("match_scw_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.msr_features_in_area.argtypes = [vp, i32, vp, fl, fl, fl, i32, i32, vp]
    L.msr_compose_scw.argtypes = [vp, vp, vp]
    L.msr_compose_scw.restype = None
    L.msr_search_scw.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, fl, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.msr_search_scw.restype = None
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
    """One pair: the current keyframe (kps, desc), the map set (points, normals [n_m, 3], dists [n_m, 2] = min, max, map_desc, mask
    or None), Scw [12] (sR row-major, then t), K [9], the bounds, th, th_low, the row on entry [n_f] and the table from the matched
    keyframe's features to the map set (or None: the row holds map indices)."""

    def __init__(self, kps, desc, points, normals, dists, map_desc, mask, scw, K, bounds=BOUNDS, th=10.0, th_low=TH_LOW, matches=None,
                 table=None, scale=None):
        self.kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self.dists = np.ascontiguousarray(dists, np.float32).reshape(-1, 2)
        self.map_desc = np.ascontiguousarray(map_desc, np.uint8).reshape(-1, 32)
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.scw, self.K = np.ascontiguousarray(scw, np.float32).reshape(12), np.ascontiguousarray(K, np.float32).reshape(9)
        self.bounds, self.th, self.th_low = tuple(int(b) for b in bounds), float(th), int(th_low)
        self.n_f, self.n_m = len(self.kps), len(self.points)
        self.matches = np.full(self.n_f, -1, np.int32) if matches is None else np.ascontiguousarray(matches, np.int32)
        self.table = None if table is None else np.ascontiguousarray(table, np.int32).reshape(-1)
        self.scale = scale_table() if scale is None else np.ascontiguousarray(scale, np.float32)
        assert len(self.desc) == self.n_f == len(self.matches)
        assert len(self.normals) == len(self.dists) == len(self.map_desc) == self.n_m
        self._expected = None

    @property
    def n_table(self):
        return 0 if self.table is None else len(self.table)

    def variant(self, **kw):
        """The same pair with some inputs replaced (a fresh World: nothing cached is shared)."""
        a = dict(kps=self.kps.copy(), desc=self.desc, points=self.points.copy(), normals=self.normals.copy(), dists=self.dists.copy(),
                 map_desc=self.map_desc, mask=self.mask, scw=self.scw.copy(), K=self.K, bounds=self.bounds, th=self.th,
                 th_low=self.th_low, matches=self.matches.copy(), table=self.table, scale=self.scale)
        a.update(kw)
        return World(**a)

    def expected(self):
        """The restatement's answer, computed once and left unchanged."""
        if self._expected is None:
            self._expected = search_scw(self)
        return self._expected


def features_in_area(kps, bounds, x, y, r, min_level=-1, max_level=-1):
    """The restatement's GetFeaturesInArea -> int32 indices in its order."""
    k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    b = np.ascontiguousarray(bounds, np.int32)
    out = np.zeros(max(len(k), 1), np.int32)
    n = lib().msr_features_in_area(_p(k), len(k), _p(b), float(x), float(y), float(r), int(min_level), int(max_level), _p(out))
    return out[:n].copy()


def compose_scw(pose2, sim3):
    """The restatement's Scw = S12 * Tmw -> [12] float32."""
    T2 = np.ascontiguousarray(pose2, np.float32).reshape(12)
    s = np.ascontiguousarray(sim3, np.float32).reshape(13)
    out = np.zeros(12, np.float32)
    lib().msr_compose_scw(_p(T2), _p(s), _p(out))
    return out


def search_scw(w: World):
    """The restatement -> dict(matches [n_f] int32, res {field: value}, stage [n_m], proj [n_m, 4] (u, v, radius, level), outcome
    [n_m], alone [n_m], best [n_m])."""
    m = np.full(max(w.n_f, 1), -1, np.int32)
    m[:w.n_f] = w.matches
    nm = max(w.n_m, 1)
    res, stage = np.zeros(14, np.int32), np.zeros(nm, np.int32)
    proj, out, alone, best = np.zeros((nm, 4), np.float32), np.zeros(nm, np.int32), np.zeros(nm, np.int32), np.zeros(nm, np.int32)
    b = np.ascontiguousarray(w.bounds, np.int32)
    lib().msr_search_scw(_p(w.kps), _p(w.desc), w.n_f, w.n_m, _p(w.points), _p(w.normals), _p(w.dists), _p(w.map_desc), _p(w.mask),
                         _p(w.scw), _p(w.K), _p(b), _p(w.scale), len(w.scale), w.th, w.th_low, _p(m), _p(w.table), w.n_table, _p(res),
                         _p(stage), _p(proj), _p(out), _p(alone), _p(best))
    return dict(matches=m[:w.n_f].copy(), res=dict(zip(RESULT_FIELDS, (int(v) for v in res))), stage=stage[:w.n_m], proj=proj[:w.n_m],
                outcome=out[:w.n_m], alone=alone[:w.n_m], best=best[:w.n_m])


# ---- the second statement: numpy; no grid, no claim rounds ----

def compose_scw_numpy(pose2, sim3):
    """Scw = S12 * Tmw in f64, one operation at a time in the rule's order."""
    T2, s = np.asarray(pose2, np.float32).reshape(12), np.asarray(sim3, np.float32).reshape(13)
    if not (np.isfinite(T2).all() and np.isfinite(s).all() and s[12] > 0):
        return np.zeros(12, np.float32)
    A, B = s[:9].astype(np.float64).reshape(3, 3), T2[:9].astype(np.float64).reshape(3, 3)
    tm, t12, s12 = T2[9:].astype(np.float64), s[9:12].astype(np.float64), float(s[12])
    out = np.zeros(12, np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                out[3 * r + c] = f32(s12 * ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]))
            out[9 + r] = f32(s12 * ((A[r, 0] * tm[0] + A[r, 1] * tm[1]) + A[r, 2] * tm[2]) + t12[r])
    return out


def decompose_numpy(scw):
    """Rule 1 -> (ok, R [9], t [3], Ow [3]) in f32 arithmetic, one operation at a time."""
    S = np.asarray(scw, np.float32)
    with np.errstate(all="ignore"):
        dot = f32(f32(f32(S[0] * S[0]) + f32(S[1] * S[1])) + f32(S[2] * S[2]))
        s = f32(math.sqrt(float(dot))) if dot >= 0 else f32(np.nan)
        ok = bool(np.isfinite(S).all() and np.isfinite(s) and s > 0)
        if not ok:
            return False, None, None, None
        R, t = (S[:9] / s).astype(np.float32), (S[9:] / s).astype(np.float32)
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            return False, None, None, None
        ow = [f32(-f32(f32(f32(R[k] * t[0]) + f32(R[3 + k] * t[1])) + f32(R[6 + k] * t[2]))) for k in range(3)]
    return True, R, t, ow


def point_numpy(w: World, i, R, t, ow):
    """Rules 3 to 6 for point i -> (stage name, u, v, level)."""
    P, N, (mind, maxd) = w.points[i], w.normals[i], w.dists[i]
    if not (np.isfinite(P).all() and np.isfinite(N).all() and np.isfinite(mind) and np.isfinite(maxd)):
        return "dropped", None, None, None
    with np.errstate(all="ignore"):
        c = [f32(f32(f32(f32(R[3 * k] * P[0]) + f32(R[3 * k + 1] * P[1])) + f32(R[3 * k + 2] * P[2])) + t[k]) for k in range(3)]
        if c[2] < 0:
            return "behind", None, None, None
        invz = f32(f32(1.0) / c[2])
        u = f32(f32(w.K[0] * f32(c[0] * invz)) + w.K[2])
        v = f32(f32(w.K[4] * f32(c[1] * invz)) + w.K[5])
        if not (u >= w.bounds[0] and u < w.bounds[1] and v >= w.bounds[2] and v < w.bounds[3]):
            return "out_image", None, None, None
        po = [float(f32(P[k] - ow[k])) for k in range(3)]
        dist = f32(math.sqrt((po[0] * po[0] + po[1] * po[1]) + po[2] * po[2]))
        if dist < f32(f32(0.8) * mind) or dist > f32(f32(1.2) * maxd):
            return "out_distance", None, None, None
        dot = (po[0] * float(N[0]) + po[1] * float(N[1])) + po[2] * float(N[2])
        if dot < 0.5 * float(dist):
            return "out_angle", None, None, None
        ratio = f32(maxd / dist) if dist != 0 else f32(np.inf if maxd > 0 else np.nan)
        if math.isnan(ratio):
            return "dropped", None, None, None
        level = int((ratio > w.scale[:len(w.scale) - 1]).sum())
    return "searched", u, v, level


def search_scw_numpy(w: World):
    """-> (matches [n_f], res {field: value} without n_displaced and rounds)."""
    ones = np.array([bin(v).count("1") for v in range(256)], np.uint8)
    matches = w.matches.copy()
    taken, found = np.zeros(w.n_f, bool), np.zeros(w.n_m, bool)
    res = dict.fromkeys(COMPARED_FIELDS, 0)
    for j in range(w.n_f):
        i = int(matches[j])
        if i == TAKEN_UNMAPPED:
            taken[j] = True
            res["n_unmapped"] += 1
        if i < 0:
            continue
        taken[j] = True
        if w.table is not None:
            if i >= len(w.table):
                res["status"] |= BAD_INPUT
                continue
            i = int(w.table[i])
            if i < 0:
                matches[j] = TAKEN_UNMAPPED
                res["n_unmapped"] += 1
                continue
        if i >= w.n_m:
            res["status"] |= BAD_INPUT
            continue
        matches[j], found[i] = i, True
    res["n_found"] = int(found.sum())
    ok, R, t, ow = decompose_numpy(w.scw)
    if not ok:
        res["status"] |= NONFINITE
    th_low = min(w.th_low, 255)
    for i in range(w.n_m):
        if found[i] or (w.mask is not None and w.mask[i] == 0):
            continue
        res["n_points"] += 1
        if not ok:
            continue
        stage, u, v, level = point_numpy(w, i, R, t, ow)
        if stage == "dropped":
            res["status"] |= NONFINITE
        elif stage != "searched":
            res["n_" + stage] += 1
        if stage != "searched":
            continue
        cand = M.window_numpy(w.kps, w.bounds, u, v, f32(f32(w.th) * w.scale[level]), level - 1, level)  # (sorted by window position)
        if not len(cand):
            continue
        res["n_with_candidates"] += 1
        cand = cand[~taken[cand]]
        d = ones[w.desc[cand] ^ w.map_desc[i][None, :]].sum(axis=1, dtype=np.int64)
        if not len(cand) or d.min() > th_low:
            res["n_over_dist"] += 1
            continue
        j = int(cand[int(np.argmin(d))])  # (the first smallest)
        matches[j], taken[j] = i, True
        res["nmatches"] += 1
    res["n_total"] = int(((matches >= 0) | (matches == TAKEN_UNMAPPED)).sum())
    return matches, res


# ---- the worlds the host and the GPU test share ----

camera, pose_of, points_seen_at = M.camera, M.pose_of, M.points_seen_at
_keypoints, _flip = M._keypoints, M._flip
EYE = ML.EYE


def scaled(pose, s):
    """Scw = s * [R | t] in f32: a similarity whose decomposition gives the pose back up to rounding."""
    return (np.asarray(pose, np.float32) * f32(s)).astype(np.float32)


def with_table(matches, n_m, rng, unmapped=0.1, spare=20):
    """The row `matches` (map indices) as the optimiser leaves it: entries become features of the matched keyframe, drawn without
    repetition, and the table gives the map index back -- or, for a share `unmapped`, -1.  The other entries of the table are
    map indices or -1 at random.  -> (row, table)."""
    has = np.flatnonzero(matches >= 0)
    n_table = len(matches) + spare
    table = np.where(rng.random(n_table) < 0.5, rng.integers(0, max(n_m, 1), n_table), -1).astype(np.int32)
    f2 = rng.permutation(n_table)[:len(has)]
    row = np.full(len(matches), -1, np.int32)
    row[has] = f2
    table[f2] = np.where(rng.random(len(has)) < unmapped, -1, matches[has])
    return row, table


def from_local(w, s=1.3, th=10.0, th_low=TH_LOW, table_seed=None):
    """A world of the local-map matcher (a map seen from a pose, a frame built around the projections of the points in view, a share
    of them already matched, a few entries for unrelated features) under Scw = s * pose; with table_seed the row goes through a
    table."""
    matches, table = w.matches, None
    if table_seed is not None:
        matches, table = with_table(w.matches, w.n_m, np.random.default_rng(table_seed))
    return World(w.kps, w.desc, w.points, w.normals, w.dists, w.map_desc, w.mask, scaled(w.pose, s), w.K, w.bounds, th, th_low, matches,
                 table, w.scale)


def make_world(n_m, seed, s=1.3, table=True, **kw):
    return from_local(ML.make_world(n_m, seed, **kw), s, table_seed=seed + 7 if table else None)


def truth_world(n_m=300, seed=31, s12=1.17, have=0.3):
    """A loop keyframe's and its neighbours' points (world frame), the matched keyframe's pose Tmw and a true similarity S12 with
    s12 != 1 from the matched keyframe's camera to the current one's; Scw is the restatement's composition.  The current keyframe
    has a feature exactly on the projection of every point in view (octave = the predicted level, the point's descriptor with 0 to
    30 bits flipped) and unrelated features with random descriptors; a share `have` of the planted correspondences is in the row
    already, through the table.  .planted: (feature, point) pairs; every one of them is to be found."""
    rng = np.random.default_rng(seed)
    K = camera()
    Tmw, T12 = pose_of(seed + 1), pose_of(seed + 2)
    sim3 = np.r_[T12[:9], T12[9:] * f32(3.0), f32(s12)].astype(np.float32)
    scw = compose_scw(Tmw, sim3)
    ok, R, t, _ = decompose_numpy(scw)
    assert ok
    pts, normals, dists, mdesc, _ = ML.make_map(n_m, seed + 3, np.r_[R, t].astype(np.float32), K)
    none_k, none_d = np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
    e = search_scw(World(none_k, none_d, pts, normals, dists, mdesc, None, scw, K))
    seen = np.flatnonzero(e["stage"] == STAGES.index("searched"))
    # (a feature in the grid's last half cell is in no cell: leave those points without one)
    seen = seen[(e["proj"][seen, 0] < BOUNDS[1] - 6) & (e["proj"][seen, 1] < BOUNDS[3] - 6)]
    kf = _keypoints(len(seen) + 40, rng)
    kf["x"][:len(seen)], kf["y"][:len(seen)] = e["proj"][seen, 0], e["proj"][seen, 1]
    kf["octave"][:len(seen)] = e["proj"][seen, 3].astype(np.int32)
    df = rng.integers(0, 256, (len(kf), 32), dtype=np.uint8)
    for k, i in enumerate(seen):
        df[k] = _flip(mdesc[i], int(rng.integers(0, 31)), rng)
    perm = rng.permutation(len(kf))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    planted = [(int(inv[k]), int(i)) for k, i in enumerate(seen)]
    matches = np.full(len(kf), -1, np.int32)
    for j, i in planted:
        if rng.random() < have:
            matches[j] = i
    row, table = with_table(matches, n_m, rng, unmapped=0.0)
    w = World(kf[perm], df[perm], pts, normals, dists, mdesc, None, scw, K, matches=row, table=table)
    w.planted, w.Tmw, w.sim3 = planted, Tmw, sim3
    return w


def contention_world(n_clusters=40, seed=21):
    """The local-map matcher's clusters under Scw: seven map points of one level that project within a pixel of each other, their
    descriptors a few bits from a common one, over four features under all their windows whose descriptors lie 0, 12, 24 and 36
    bits from it, all within th_low: the first four points take the features one after the other, the last three find everything
    taken -- rounds > 1 and six of seven are displaced."""
    return from_local(ML.contention_world(n_clusters, seed))


def order_world():
    """Two points (0, 1) of level 0 on neighbouring pixels and two features A = 0 and B = 1 of octave 0 under both windows.  d(0, A)
    = 10 and d(0, B) = 20; d(1, A) = 4 and d(1, B) = 34.  Sequentially point 0 takes A, its nearest, although A is nearer to point
    1; point 1 then falls to B, its second candidate.  "The nearest point wins the feature" would give A to point 1."""
    rng = np.random.default_rng(12)
    K = camera()
    p0 = rng.integers(0, 256, 32, dtype=np.uint8)
    A = ML._flip_bits(p0, range(10))
    B = ML._flip_bits(p0, range(100, 120))
    p1 = ML._flip_bits(A, range(200, 204))
    kf = np.zeros(2, KEYPOINT_DTYPE)
    kf["x"], kf["y"], kf["octave"] = [300.0, 303.0], [200.0, 200.0], 0
    pts, normals, dists = ML.axis_map(np.array([[301.0, 200.0], [302.0, 200.5]]), 4.0, K, 0, cos=0.9)
    return World(kf, np.stack([A, B]), pts, normals, dists, np.stack([p0, p1]), None, scaled(EYE, 2.0), K)


# the second setting: K_ANISO, 5 levels of 1.37, the pose rolled by 89 degrees
WORLDS_2 = ("w150@2", "w310_bounds@2")
TWO = dict(roll_deg=89.0, **SECOND)
WORLDS = ("main", "main_no_table", "bounds", "w513", "truth", "contention", "order")
_worlds = {}


def world(name: str) -> World:
    if name not in _worlds:
        if name == "w150@2":
            w = make_world(150, 101, **TWO)
        elif name == "w310_bounds@2":
            w = make_world(310, 104, bounds=(-12, 655, -9, 490), **TWO)
        elif name == "main":
            w = make_world(600, 1)
        elif name == "main_no_table":
            w = make_world(400, 2, s=0.8, table=False)
        elif name == "bounds":
            w = make_world(420, 4, bounds=(-12, 655, -9, 490))
        elif name == "w513":  # one point past a multiple of the workgroup's 512 threads: the append's second slice holds one point
            w = make_world(513, 5, edge_cases=False, n_extra=20)
        elif name == "truth":
            w = truth_world()
        elif name == "contention":
            w = contention_world()
        elif name == "order":
            w = order_world()
        else:
            raise KeyError(name)
        _worlds[name] = w
    return _worlds[name]


_rules = {}
# per rule world: the counters (or "status" bits) the world aims at, as the restatement has to report them
RULE_AIMS = {}


def rule_worlds():
    """Small worlds, each built around one rule edge of the statement -> {name: World} (built once); RULE_AIMS[name] holds what the
    restatement has to report for the world to have met its edge.  Scw = 2 * identity: Rcw = I and tcw = 0 exactly, the camera
    centre is the origin, a point (0, 0, Z) lies at distance Z exactly and projects onto (cx, cy) = (320, 240)."""
    out = _rules
    if out:
        return out
    K = camera()
    S2 = scaled(EYE, 2.0)
    rng = np.random.default_rng(78)
    d = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    spots = [(100.0 + 60 * k, 100.0) for k in range(4)]
    nxt = lambda x, to: np.nextafter(f32(x), f32(to), dtype=np.float32)  # noqa: E731

    def frame(xy, desc, octave=0):
        k = np.zeros(len(xy), KEYPOINT_DTYPE)
        k["x"], k["y"], k["octave"] = [p[0] for p in xy], [p[1] for p in xy], octave
        return k, np.ascontiguousarray(desc, np.uint8)

    def four(**kw):
        """Four points over four features with the points' descriptors: everything matches unless a rule says no."""
        pts, nrm, dst = ML.axis_map(spots, 4.0, K)
        a = dict(points=pts, normals=nrm, dists=dst, map_desc=d[:4], mask=None, scw=S2, K=K)
        a["kps"], a["desc"] = frame(spots, d[:4])
        a.update(kw)
        return World(**a)

    def add(name, w, **aims):
        out[name] = w
        RULE_AIMS[name] = aims
    add("all_four", four(), nmatches=4, n_total=4)
    # zc exactly 0 (goes on, fails the image test) and slightly negative (behind)
    z = four()
    z.points[1] = [0.1, 0.0, 0.0]
    z.points[3, 2] = -1e-3
    add("zero_and_negative_depth", z.variant(), n_behind=1, n_out_image=1, nmatches=2)
    # u on min_x (in) and on max_x (out), v likewise: fx = fy = 512 with X = -+1.25, Y = -+0.9375 and Z = 2 give 0, 640, 0, 480 exactly
    K512 = np.array([512.0, 0, 320.0, 0, 512.0, 240.0, 0, 0, 1], np.float32)
    kb, db = frame([(2.0, 240.0), (630.0, 240.0), (320.0, 2.0), (320.0, 470.0)], d[:4])
    on = four(kps=kb, desc=db, K=K512)
    on.points[:] = [[-1.25, 0, 2], [1.25, 0, 2], [0, -0.9375, 2], [0, 0.9375, 2]]
    on.normals[:] = on.points
    on.dists[:] = [1.0, 2.3]
    add("on_the_bounds", on.variant(), n_out_image=2, nmatches=2)
    # the distance bounds: points on the optical axis at Z = 0.8f * min and 1.2f * max exactly, and one step beyond
    lo, hi = f32(f32(0.8) * f32(5.0)), f32(f32(1.2) * f32(3.0))
    ka, da = frame([(318.0, 240.0), (322.0, 240.0)], d[[0, 2]], np.array([5, 0]))  # (points 0 and 2 come out at levels 5 and 0)
    ax = four(kps=ka, desc=da)
    ax.points[:] = [[0, 0, lo], [0, 0, nxt(lo, 0)], [0, 0, hi], [0, 0, nxt(hi, 9)]]
    ax.normals[:] = [0, 0, 1]
    ax.dists[:] = [[5.0, 9.0], [5.0, 9.0], [1.0, 3.0], [1.0, 3.0]]
    add("distance_bounds", ax.variant(), n_out_distance=2, nmatches=2)
    # the viewing angle, compared in f64: P = (1.5, 0, 2) lies at distance 2.5 exactly and N = (0.5, 0, 0.25) gives dot = 1.25 =
    # 0.5 * dist exactly (kept).  One ulp less in Nz gives dot = 1.25 - 3e-8, which (float)(dot / dist) rounds back to 0.5f: only
    # the f64 comparison skips it.  One ulp less in Nx is skipped either way.
    K256 = np.array([256.0, 0, 320.0, 0, 256.0, 240.0, 0, 0, 1], np.float32)
    kv, dv = frame([(512.0, 240.0)], d[:1])
    va = World(kv, dv, np.tile(f32([1.5, 0, 2]), (3, 1)), [[0.5, 0, 0.25], [0.5, 0, nxt(0.25, 0)], [nxt(0.5, 0), 0, 0.25]],
               np.tile(f32([1.0, 2.4]), (3, 1)), d[:3], None, S2, K256)
    add("angle_edge", va, n_out_angle=2, nmatches=1)
    # the octave window [level - 1, level]: level 2; octaves 3 and 0 are refused, 1 and 2 stay
    pts, nrm, dst = ML.axis_map(spots[:2], 4.0, K, level=2)
    ko, do = frame([spots[0], spots[0], spots[1], spots[1]], d[[0, 0, 1, 1]], np.array([3, 0, 1, 2]))
    add("octave_window", World(ko, do, pts, nrm, dst, d[:2], None, S2, K), n_with_candidates=1, nmatches=1)
    # bestDist == th_low and th_low + 1
    k2, d2 = frame(spots[:2], np.stack([_flip(d[0], TH_LOW, rng), _flip(d[1], TH_LOW + 1, rng)]))
    pts, nrm, dst = ML.axis_map(spots[:2], 4.0, K)
    add("distance_50_and_51", World(k2, d2, pts, nrm, dst, d[:2], None, S2, K), nmatches=1, n_over_dist=1)
    # a candidate at distance 256 under th_low = 256: `dist < bestDist` from 256 never picks it
    add("distance_256", World(*frame(spots[:1], ~d[:1]), pts[:1], nrm[:1], dst[:1], d[:1], None, S2, K, th_low=256), nmatches=0,
        n_over_dist=1)
    # the entry: -2 keeps its feature and finds nothing; another negative entry is free
    add("entry_minus_2", four(matches=np.array([TAKEN_UNMAPPED, -1, -7, -1], np.int32)), n_unmapped=1, nmatches=3, n_total=4,
        n_over_dist=1)
    # feature 0 has the matched keyframe's feature 1, which has no point in the set; feature 2 has feature 3 -> point 1
    add("unmapped_translation", four(matches=np.array([1, -1, 3, -1], np.int32), table=np.array([2, -1, 0, 1], np.int32)), n_unmapped=1,
        n_found=1, nmatches=1, n_total=3)
    add("entry_beyond_the_set", four(matches=np.array([-1, 4, -5, 99], np.int32)), status=BAD_INPUT, n_total=4, nmatches=2)
    # with the table: feature 0's entry is beyond the table, feature 1's translates to a point beyond the set
    add("table_beyond", four(matches=np.array([4, 2, -1, -1], np.int32), table=np.array([0, 1, 9, 3], np.int32)), status=BAD_INPUT,
        n_total=4, nmatches=2, n_found=0)
    # feature 0 names point 1, which the mask leaves out: the point is found whatever its mask
    add("masked_point_named", four(mask=np.array([1, 0, 1, 1], np.uint8), matches=np.array([1, -1, -1, -1], np.int32)), n_found=1,
        n_points=3)
    add("mask", four(mask=np.array([1, 0, 1, 1], np.uint8)), n_points=3, nmatches=3)
    bad = S2.copy()
    bad[10] = np.nan
    add("nonfinite_scw", four(scw=bad, matches=np.array([1, -1, -1, -1], np.int32), table=np.array([0, 3, 0, 0], np.int32)),
        status=NONFINITE, n_points=3, nmatches=0, n_total=1)
    add("zero_scw", four(scw=np.zeros(12, np.float32)), status=NONFINITE, n_points=4, nmatches=0)
    neg = S2.copy()
    neg[:3] = 0.0  # (the first row of sR is zero: scw == 0 although the matrix is not)
    add("zero_scale_row", four(scw=neg), status=NONFINITE, nmatches=0)
    nf = four()
    nf.points[0, 0], nf.normals[1, 2], nf.dists[2, 0] = np.nan, np.inf, np.nan
    add("nonfinite_point", nf.variant(), status=NONFINITE, nmatches=1)
    add("no_features", four(kps=np.zeros(0, KEYPOINT_DTYPE), desc=np.zeros((0, 32), np.uint8)), n_points=4, n_total=0)
    add("no_points", World(*frame(spots, d[:4]), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 32), np.uint8), None,
                           S2, K, matches=np.array([-1, TAKEN_UNMAPPED, -1, -1], np.int32)), n_points=0, n_total=1, n_unmapped=1)
    return out


# ---- the chain: Sim3Solver -> SearchBySim3 -> OptimizeSim3 -> Scw -> this matcher (LoopClosing::ComputeSim3 up to its decision) ----

CHAIN_WORLDS = ("accepted", "few_inliers", "few_total")
CHAIN_CAP = 512
_chains = {}


class ChainWorld:
    """A keyframe pair of tests/sim3_ref_lib.py (frame 0 the current keyframe, frame 1 the matched one; point set k is keyframe
    k's) at capacity CHAIN_CAP, the solver's draws, and the loop's map set: the matched keyframe's own map points, entry f the
    point of its feature f (normal towards the current camera, distances in map units so that PredictScale returns the octave of
    the current keyframe's feature, the matched keyframe's descriptor), with the table feature -> entry."""

    def __init__(self, mw, draws):
        import sim3_ref_lib as R
        self.mw, self.draws, cap = mw, draws, mw.cap
        ok, Rc, tc, ow = decompose_numpy(compose_scw(mw.pose[1], mw.sim))  # (the true similarity: where the points are seen from)
        assert ok
        t = mw.truth
        self.map_points, self.map_mask, self.map_desc = mw.points[1].copy(), mw.mask[1].copy(), mw.desc[1].copy()
        po = self.map_points.astype(np.float64) - np.array(ow, np.float64)
        dist = np.maximum(np.linalg.norm(po, axis=1), 1e-9)
        self.map_normals = (po / dist[:, None]).astype(np.float32)
        lev = np.zeros(cap, np.int64)
        lev[t["slots2"]] = t["lev"]
        maxd = dist * R.scale_table().astype(np.float64)[lev] * 0.95
        self.map_dist = np.c_[0.3 * dist, maxd].astype(np.float32)
        self.map_normals[self.map_mask == 0], self.map_dist[self.map_mask == 0] = 0, 0
        self.table = np.where(self.map_mask != 0, np.arange(cap), -1).astype(np.int32)
        gone = t["slots2"][:5]  # five of the matched keyframe's points are not in the loop's set: their features stay taken
        self.table[gone], self.map_mask[gone] = -1, 0
        # the neighbours' points: one in front of every feature of the current keyframe that has no point of its own
        n1, n2 = mw.n
        lone = np.setdiff1d(np.arange(n1), t["slots1"])
        self.map_n = n2 + len(lone)
        assert self.map_n <= cap
        rng = np.random.default_rng(len(lone))
        K, k1 = mw.K.astype(np.float64), mw.kps[0][lone]
        z = rng.uniform(4, 20, len(lone))
        pc = np.c_[(k1["x"] - K[2]) / K[0] * z, (k1["y"] - K[5]) / K[4] * z, z]
        Rm, tv = Rc.astype(np.float64).reshape(3, 3), tc.astype(np.float64)
        at = np.arange(n2, self.map_n)
        self.map_points[at] = (pc - tv) @ Rm
        self.map_normals[at] = (pc @ Rm) / np.linalg.norm(pc, axis=1)[:, None]
        d = np.linalg.norm(pc, axis=1)
        self.map_dist[at] = np.c_[0.3 * d, d * R.scale_table().astype(np.float64)[k1["octave"]] * 0.95]
        self.map_mask[at] = 1
        self.map_desc[at] = [_flip(x, 8, rng) for x in mw.desc[0][lone]]
        self.n_neighbours = len(lone)
        self._expected = None

    def expected(self):
        """The four restatements chained -> dict(sim3 record, msim3 record, opt record, sim [13], scw [12], row [cap], scw_res,
        accepted)."""
        if self._expected is None:
            import sim3_ref_lib as R
            import sim3opt_ref_lib as O
            mw = self.mw
            sw = R.World(mw.kps[0], mw.n[0], mw.kps[1], mw.n[1], mw.match, mw.points[0], mw.mask[0], mw.points[1], mw.mask[1],
                         mw.pose[0], mw.pose[1], mw.K)
            ref = R.solve(sw, self.draws, 0)
            q = mw.copy()
            q.match, q.sim = ref[2].copy(), ref[1].copy()
            mref = R.search_by_sim3(q)
            ow = O.World(mw.kps[0], mw.n[0], mw.kps[1], mw.n[1], mref["matches"].copy(), mw.points[0], mw.mask[0], mw.points[1],
                         mw.mask[1], mw.pose[0], mw.pose[1], ref[1].copy(), mw.K)
            opt, sim, row, _ = O.optimize(ow)
            scw = compose_scw(mw.pose[1], sim)
            n1, nm = mw.n[0], self.map_n
            w = World(mw.kps[0][:n1], mw.desc[0][:n1], self.map_points[:nm], self.map_normals[:nm], self.map_dist[:nm], self.map_desc[:nm],
                      self.map_mask[:nm], scw, mw.K, mw.bounds, matches=row[:n1], table=self.table)
            e = w.expected()
            out_row = row.copy()
            out_row[:n1] = e["matches"]
            self._expected = dict(sim3=ref[0], msim3=mref["res"], opt=opt, sim=sim, scw=scw, row=out_row, scw_res=e["res"],
                                  accepted=bool(opt["n_inliers"] >= 20 and e["res"]["n_total"] >= 40))
        return self._expected


def chain_world(name: str) -> ChainWorld:
    """accepted: 300 common points, a fifth of the solver's matches wrong.  few_inliers: every match of the row is wrong -- no
    similarity, nInliers 0.  few_total: 32 common points -- the optimiser keeps more than 20 of them, and the whole map set cannot
    bring nTotalMatches to 40."""
    if name not in _chains:
        import sim3_ref_lib as R
        # (padded_m lives in the GPU test module of the solver, which tests/test_gpu_sim3opt.py borrows it from as well; its home
        # would be sim3_ref_lib, an existing file this change leaves alone.  The module imports no torch at its top level, so
        # the host test that builds these worlds imports it without a device.)
        from test_gpu_sim3 import padded_m
        n, seed, matched = dict(accepted=(300, 81, 0.4), few_inliers=(120, 82, 0.4), few_total=(32, 83, 0.85))[name]
        mw = padded_m(R.make_match_world(n, seed, noise_bits=10, extra=4 if name == "few_total" else 20, matched=matched), CHAIN_CAP)
        rng = np.random.default_rng(seed)
        t = mw.truth
        have = np.flatnonzero(t["have"])
        wrong = have if name == "few_inliers" else rng.choice(have, len(have) // 5 if name == "accepted" else 0, replace=False)
        if len(wrong):
            mw.match[t["slots1"][wrong]] = np.roll(t["slots2"][wrong], 1)  # mismatches among points
        _chains[name] = ChainWorld(mw, R.make_draws(300, seed))
    return _chains[name]
