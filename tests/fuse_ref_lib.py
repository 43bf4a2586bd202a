"""ctypes wrapper around tests/cpp/fuse_ref.cpp -- the CPU restatement of both overloads of ORBmatcher::Fuse (include/orbx.h,
"fusing map points into a keyframe") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary directory,
as tests/match_scw_ref_lib.py compiles its source; a second, independently written numpy statement (a brute-force window over all
features, the picks first and then a plain loop per feature); and the worlds that tests/test_fuse_host.py and
tests/test_gpu_fuse.py share.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import match_local_ref_lib as ML
import match_proj_ref_lib as M
import match_scw_ref_lib as S
from pose_ref_lib import K_ANISO, NLEVELS_2, SCALE_FACTOR_2, SECOND, inv_sigma2_table  # noqa: F401 (the second setting)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fuse_ref.cpp")
KEYPOINT_DTYPE = M.KEYPOINT_DTYPE
RESULT_FIELDS = ("status", "n_fused", "n_points", "n_in_kf", "n_behind", "n_out_image", "n_out_distance", "n_out_angle",
                 "n_with_candidates", "n_over_dist", "n_added", "n_kept_occupant", "n_replaced_occupant", "n_bad_occupant", "n_chained",
                 "rounds")
COMPARED_FIELDS = RESULT_FIELDS[:-1]  # (rounds is the device's own count)
BAD_INPUT, NONFINITE, UNMAPPED = 2, 4, -2
NONE, ADD, KEEP, REPLACE, BAD = 0, 1, 2, 3, 4
STAGES = ("none", "dropped", "behind", "out_image", "out_distance", "out_angle", "searched")
SEARCHED = STAGES.index("searched")
NLEVELS, BOUNDS, TH_LOW = M.NLEVELS, M.BOUNDS, 50
f32 = np.float32
_L = None


def build(src=SRC) -> ctypes.CDLL:
    d = tempfile.mkdtemp(prefix="fuse_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libfuse_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", src, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("fuse_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.fr_features_in_area.argtypes = [vp, i32, vp, fl, fl, fl, i32, i32, vp]
    L.fr_fuse.argtypes = [i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, fl, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.fr_fuse.restype = None
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
    """One pair: the keyframe (kps, desc), the map set (points, normals [n_m, 3], dists [n_m, 2] = min, max, map_desc, mask or None,
    obs [n_m] = Observations()), T [12] (the pose, or with form "scw" the similarity), K [9], the bounds, th, th_low, the row on
    entry [n_f] and the unmapped occupants' counts [n_f] (or None)."""

    def __init__(self, form, kps, desc, points, normals, dists, map_desc, mask, obs, T, K, bounds=BOUNDS, th=None, th_low=TH_LOW,
                 matches=None, occ_obs=None, scale=None, inv_sigma2=None):
        assert form in ("pose", "scw")
        self.form = form
        self.kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self.dists = np.ascontiguousarray(dists, np.float32).reshape(-1, 2)
        self.map_desc = np.ascontiguousarray(map_desc, np.uint8).reshape(-1, 32)
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.n_f, self.n_m = len(self.kps), len(self.points)
        self.obs = np.ones(self.n_m, np.int32) if obs is None else np.ascontiguousarray(obs, np.int32)
        self.T, self.K = np.ascontiguousarray(T, np.float32).reshape(12), np.ascontiguousarray(K, np.float32).reshape(9)
        self.bounds, self.th_low = tuple(int(b) for b in bounds), int(th_low)
        self.th = float(th if th is not None else (3.0 if form == "pose" else 4.0))
        self.matches = np.full(self.n_f, -1, np.int32) if matches is None else np.ascontiguousarray(matches, np.int32)
        self.occ_obs = None if occ_obs is None else np.ascontiguousarray(occ_obs, np.int32)
        self.scale = scale_table() if scale is None else np.ascontiguousarray(scale, np.float32)
        self.inv_sigma2 = inv_sigma2_table() if inv_sigma2 is None else np.ascontiguousarray(inv_sigma2, np.float32)
        assert len(self.desc) == self.n_f == len(self.matches) and len(self.scale) == len(self.inv_sigma2)
        assert len(self.normals) == len(self.dists) == len(self.map_desc) == len(self.obs) == self.n_m
        self._expected = None

    @property
    def scw(self):  # (what the numpy statement of the Scw matcher's rule 1 reads)
        return self.T

    def variant(self, **kw):
        """The same pair with some inputs replaced (a fresh World: nothing cached is shared)."""
        a = dict(form=self.form, kps=self.kps.copy(), desc=self.desc, points=self.points.copy(), normals=self.normals.copy(),
                 dists=self.dists.copy(), map_desc=self.map_desc, mask=self.mask, obs=self.obs.copy(), T=self.T.copy(), K=self.K,
                 bounds=self.bounds, th=self.th, th_low=self.th_low, matches=self.matches.copy(), occ_obs=self.occ_obs, scale=self.scale,
                 inv_sigma2=self.inv_sigma2)
        a.update(kw)
        return World(**a)

    def expected(self):
        """The restatement's answer, computed once and left unchanged."""
        if self._expected is None:
            self._expected = fuse(self)
        return self._expected


def features_in_area(kps, bounds, x, y, r, min_level=-1, max_level=-1):
    """The restatement's GetFeaturesInArea -> int32 indices in its order."""
    k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    b = np.ascontiguousarray(bounds, np.int32)
    out = np.zeros(max(len(k), 1), np.int32)
    n = lib().fr_features_in_area(_p(k), len(k), _p(b), float(x), float(y), float(r), int(min_level), int(max_level), _p(out))
    return out[:n].copy()


def fuse(w: World):
    """The restatement -> dict(matches [n_f], idx, act, other [n_m], res {field: value}, stage [n_m], proj [n_m, 4] (u, v, radius,
    level))."""
    m = np.full(max(w.n_f, 1), -1, np.int32)
    m[:w.n_f] = w.matches
    nm = max(w.n_m, 1)
    res, stage, proj = np.zeros(16, np.int32), np.zeros(nm, np.int32), np.zeros((nm, 4), np.float32)
    idx, act, other = np.full(nm, -9, np.int32), np.full(nm, 9, np.uint8), np.full(nm, -9, np.int32)
    b = np.ascontiguousarray(w.bounds, np.int32)
    lib().fr_fuse(int(w.form == "scw"), _p(w.kps), _p(w.desc), w.n_f, w.n_m, _p(w.points), _p(w.normals), _p(w.dists), _p(w.map_desc),
                  _p(w.mask), _p(w.obs), _p(w.T), _p(w.K), _p(b), _p(w.scale), _p(w.inv_sigma2), len(w.scale), w.th, w.th_low, _p(m),
                  _p(w.occ_obs), _p(idx), _p(act), _p(other), _p(res), _p(stage), _p(proj))
    return dict(matches=m[:w.n_f].copy(), idx=idx[:w.n_m].copy(), act=act[:w.n_m].copy(), other=other[:w.n_m].copy(),
                res=dict(zip(RESULT_FIELDS, (int(v) for v in res))), stage=stage[:w.n_m], proj=proj[:w.n_m])


# ---- the second statement: numpy; no grid, the picks first, then one plain loop per feature ----

def _clamp_obs(v, res):
    v = int(v)
    if v < 0 or v > 65535:
        res["status"] |= BAD_INPUT
    return min(max(v, 0), 65535)


def fuse_numpy(w: World):
    """-> (matches [n_f], idx, act, other [n_m], res {field: value} without rounds)."""
    ones = np.array([bin(v).count("1") for v in range(256)], np.uint8)
    res = dict.fromkeys(COMPARED_FIELDS, 0)
    scw = w.form == "scw"
    row = w.matches.copy()
    named = row[(row >= 0) & (row < w.n_m)]
    in_kf = np.zeros(w.n_m, bool)
    in_kf[named] = True
    if (row >= w.n_m).any() or (not scw and w.occ_obs is None and (row == UNMAPPED).any()):
        res["status"] |= BAD_INPUT
    res["n_in_kf"] = int(in_kf.sum())
    if scw:
        ok, R, t, ow = S.decompose_numpy(w.T)
    else:
        ok = bool(np.isfinite(w.T).all())
        R, t = w.T[:9], w.T[9:]
        with np.errstate(all="ignore"):
            ow = [f32(-f32(f32(f32(R[k] * t[0]) + f32(R[3 + k] * t[1])) + f32(R[6 + k] * t[2]))) for k in range(3)]
    if not ok:
        res["status"] |= NONFINITE
    idx = np.full(w.n_m, -1, np.int32)
    for i in range(w.n_m):
        if in_kf[i] or (w.mask is not None and w.mask[i] == 0):
            continue
        res["n_points"] += 1
        if not ok:
            continue
        stage, u, v, level = S.point_numpy(w, i, R, t, ow)
        if stage == "dropped":
            res["status"] |= NONFINITE
        elif stage != "searched":
            res["n_" + stage] += 1
        if stage != "searched":
            continue
        cand = M.window_numpy(w.kps, w.bounds, u, v, f32(f32(w.th) * w.scale[level]), -2 ** 31, 2 ** 31 - 1)
        if not len(cand):
            continue
        res["n_with_candidates"] += 1
        octv = w.kps["octave"][cand]
        keep = (octv >= level - 1) & (octv <= level)
        if not scw:
            with np.errstate(all="ignore"):
                ex, ey = (u - w.kps["x"][cand]).astype(np.float32), (v - w.kps["y"][cand]).astype(np.float32)
                e2 = (ex * ex).astype(np.float32) + (ey * ey).astype(np.float32)
                chi = (e2.astype(np.float32) * w.inv_sigma2[np.clip(octv, 0, len(w.scale) - 1)]).astype(np.float32)
            keep &= (octv >= 0) & ~(chi.astype(np.float64) > 5.99)
        cand = cand[keep]
        d = ones[w.desc[cand] ^ w.map_desc[i][None, :]].sum(axis=1, dtype=np.int64)
        if not scw:
            cand, d = cand[d < 256], d[d < 256]
        if not len(cand) or d.min() > w.th_low:
            res["n_over_dist"] += 1
            continue
        idx[i] = int(cand[int(np.argmin(d))])  # (the first smallest)
    act, other = np.zeros(w.n_m, np.uint8), np.full(w.n_m, -1, np.int32)
    res["n_fused"] = int((idx >= 0).sum())
    if not scw:
        for i in np.flatnonzero(idx >= 0):
            _clamp_obs(w.obs[i], res)
    for f in np.unique(idx[idx >= 0]):
        pts = np.flatnonzero(idx == f)  # ascending
        occ = int(row[f])
        free = occ < 0 and occ != UNMAPPED
        if not free:
            if occ >= w.n_m:
                bad = True
            elif occ >= 0:
                bad = w.mask is not None and w.mask[occ] == 0
            elif scw:
                bad = w.occ_obs is not None and w.occ_obs[f] < 0
            else:
                bad = w.occ_obs is None or w.occ_obs[f] < 0
            if bad:
                act[pts], other[pts] = BAD, occ
                res["n_bad_occupant"] += len(pts)
                continue
        c = None
        for k, i in enumerate(pts):
            obs = 0 if scw else _clamp_obs(w.obs[i], dict(status=0))
            if free and k == 0:
                act[i], row[f], c = ADD, i, obs + 1
                res["n_added"] += 1
                continue
            res["n_chained"] += k > 0
            other[i] = row[f]
            if scw:
                act[i] = KEEP
                res["n_kept_occupant"] += 1
                continue
            if c is None:
                c = _clamp_obs(w.obs[occ] if occ >= 0 else w.occ_obs[f], res)
            if c > obs:
                act[i] = KEEP
                res["n_kept_occupant"] += 1
            else:
                act[i], row[f] = REPLACE, i
                res["n_replaced_occupant"] += 1
            c += obs
    return row, idx, act, other, res


# ---- the worlds the host and the GPU test share ----

camera, pose_of, points_seen_at = M.camera, M.pose_of, M.points_seen_at
_keypoints, _flip = M._keypoints, M._flip
EYE, scaled = ML.EYE, S.scaled


def from_local(lw, form, seed, s=1.3, th=None, th_low=TH_LOW, unmapped=0.15, inv_sigma2=None):
    """A world of the local-map matcher (a map seen from a pose, a keyframe built around the projections of the points in view, a
    share of them already in the row, a few entries for unrelated features) as a Fuse pair: observation counts of 1 to 12, a share
    `unmapped` of the row's entries turned into occupants that are not in the set (a fifth of those bad), and a point that is not
    in the set on some free features too."""
    rng = np.random.default_rng(seed)
    row = lw.matches.copy()
    has = np.flatnonzero(row >= 0)
    row[has[rng.random(len(has)) < unmapped]] = UNMAPPED
    free = np.flatnonzero(row == -1)
    row[free[rng.random(len(free)) < 0.2]] = UNMAPPED
    occ = np.where(rng.random(lw.n_f) < 0.2, -1, rng.integers(0, 13, lw.n_f)).astype(np.int32)
    obs = rng.integers(1, 13, lw.n_m).astype(np.int32)
    T = lw.pose if form == "pose" else scaled(lw.pose, s)
    return World(form, lw.kps, lw.desc, lw.points, lw.normals, lw.dists, lw.map_desc, lw.mask, obs, T, lw.K, lw.bounds, th, th_low, row, occ,
                 lw.scale, inv_sigma2)


def make_world(form, n_m, seed, **kw):
    two = kw.get("nlevels") == NLEVELS_2
    return from_local(ML.make_world(n_m, seed, have=0.15, **kw), form, seed + 11,
                      inv_sigma2=inv_sigma2_table(NLEVELS_2, SCALE_FACTOR_2) if two else None)


def tiny_world(form):
    """2 features / 2 points: point 0 over feature 0 (free: added), point 1 over feature 1, which holds an unmapped point with 3
    observations against the point's 2 (kept)."""
    K = camera()
    rng = np.random.default_rng(5)
    d = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    spots = [(200.0, 150.0), (400.0, 300.0)]
    kf = np.zeros(2, KEYPOINT_DTYPE)
    kf["x"], kf["y"] = [p[0] for p in spots], [p[1] for p in spots]
    pts, nrm, dst = ML.axis_map(spots, 4.0, K)
    T = EYE if form == "pose" else scaled(EYE, 2.0)
    return World(form, kf, d, pts, nrm, dst, d, None, [5, 2], T, K, matches=[-1, UNMAPPED], occ_obs=[0, 3])


CLUSTER_KINDS = ("free", "occupied", "masked_occupant", "unmapped", "bad_unmapped", "beyond")


def contention_world(form, n_clusters=40, seed=21):
    """Clusters in which 3 to 7 map points of one level project within half a pixel of ONE feature and pick it (a second feature
    under their windows is 100 bits away), plus one point per cluster whose descriptor is 70 to 90 bits from the feature's (over
    th_low).  The feature is, by cluster, free, held by a point of the set, held by a masked-out point, held by an unmapped point,
    by a bad unmapped point, or its entry lies beyond the set; observation counts of 1 to 9 against occupants with 3 to 8 draw
    keeps and replacements inside one chain.  .clusters: (kind, feature, [points in ascending index])."""
    rng = np.random.default_rng(seed)
    K, pose = camera(), pose_of(seed + 1)
    scale = scale_table()
    uv, md, lv, cl, fxy, fo, fd, kinds = [], [], [], [], [], [], [], []
    for c in range(n_clusters):
        centre = np.array([rng.uniform(40, 600), rng.uniform(40, 440)])
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        L = int(rng.integers(1, NLEVELS))
        kinds.append(CLUSTER_KINDS[c % len(CLUSTER_KINDS)] if c >= 12 else ("free", "occupied", "unmapped")[c % 3])
        for _ in range(int(rng.integers(3, 8))):
            uv.append(centre + rng.uniform(-0.5, 0.5, 2))
            md.append(_flip(base, int(rng.integers(0, 20)), rng))
            lv.append(L)
            cl.append(c)
        uv.append(centre + rng.uniform(-0.5, 0.5, 2))  # the point that finds nothing near enough
        md.append(_flip(base, int(rng.integers(70, 91)), rng))
        lv.append(L)
        cl.append(-1)
        fxy += [centre + rng.uniform(-0.3, 0.3, 2), centre + rng.uniform(-1.0, 1.0, 2)]
        fo += [L - (c & 1), L]
        fd += [base, _flip(base, 100, rng)]
    n = len(uv)
    order = rng.permutation(n)
    uv, md, lv, cl = np.array(uv)[order], np.array(md, np.uint8)[order], np.array(lv)[order], np.array(cl)[order]
    n_occ = n_clusters  # one occupant slot per cluster behind the searched points (used by "occupied" and "masked_occupant")
    depth = rng.uniform(2.0, 10.0, n + n_occ)
    uv_all = np.concatenate([uv, rng.uniform(50, 500, (n_occ, 2))])
    pts = points_seen_at(pose, K, uv_all, depth)
    R, t = pose[:9].reshape(3, 3).astype(np.float64), pose[9:].astype(np.float64)
    po = pts.astype(np.float64) - (-R.T @ t)
    dist = np.linalg.norm(po, axis=1)
    maxd = dist * scale[np.concatenate([lv, np.ones(n_occ, np.int64)])].astype(np.float64) * 0.93
    mdesc = np.concatenate([md, rng.integers(0, 256, (n_occ, 32), dtype=np.uint8)])
    mask = np.ones(n + n_occ, np.uint8)
    obs = np.concatenate([rng.integers(1, 10, n), rng.integers(3, 9, n_occ)]).astype(np.int32)
    kf = _keypoints(len(fxy), rng, np.array(fo))
    kf["x"], kf["y"] = [p[0] for p in fxy], [p[1] for p in fxy]
    perm = rng.permutation(len(kf))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    row, occ_obs, clusters = np.full(len(kf), -1, np.int32), np.full(len(kf), -1, np.int32), []
    for c, kind in enumerate(kinds):
        f = int(inv[2 * c])
        if kind in ("occupied", "masked_occupant"):
            row[f] = n + c
            mask[n + c] = kind == "occupied"
        elif kind in ("unmapped", "bad_unmapped"):
            row[f], occ_obs[f] = UNMAPPED, int(rng.integers(3, 9)) if kind == "unmapped" else -1
        elif kind == "beyond":
            row[f] = n + n_occ + 5
        clusters.append((kind, f, [int(i) for i in np.flatnonzero(cl == c)]))
    T = pose if form == "pose" else scaled(pose, 1.3)
    w = World(form, kf[perm], np.array(fd, np.uint8)[perm], pts, (po / dist[:, None]).astype(np.float32),
              np.stack([maxd / 4.0, maxd], 1).astype(np.float32), mdesc, mask, obs, T, K, matches=row, occ_obs=occ_obs)
    w.clusters = clusters
    return w


def order_world(form):
    """Three points (0, 1, 2) on one free feature, with 4, 9 and 2 observations.  Pose form: point 0 is added (count 5); point 1
    meets point 0 with 5 <= 9 and replaces it (count 14); point 2 meets point 1 with 14 > 2 and is replaced by it.  Scw form:
    point 0 is added; points 1 and 2 both get point 0 as the point to be replaced by."""
    K = camera()
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    kf = np.zeros(1, KEYPOINT_DTYPE)
    kf["x"], kf["y"] = 300.0, 200.0
    pts, nrm, dst = ML.axis_map([(300.2, 200.0), (300.0, 200.3), (299.7, 199.8)], 4.0, K)
    md = np.stack([_flip(base, 3, rng), _flip(base, 1, rng), _flip(base, 7, rng)])
    T = EYE if form == "pose" else scaled(EYE, 2.0)
    return World(form, kf, base[None], pts, nrm, dst, md, None, [4, 9, 2], T, K)


TWO = dict(roll_deg=89.0, **SECOND)
WORLDS = ("tiny", "main", "w513", "contention", "order")
WORLDS_2 = ("w150@2",)
FORMS = ("pose", "scw")
_worlds = {}


def world(form: str, name: str) -> World:
    key = (form, name)
    if key not in _worlds:
        if name == "tiny":
            w = tiny_world(form)
        elif name == "main":  # about 400 features / 600 points
            w = make_world(form, 600, 1)
        elif name == "w513":  # one point past a multiple of the workgroup's 512 threads: a second trip of the stride loop
            w = make_world(form, 513, 5, edge_cases=False, n_extra=20)
        elif name == "contention":
            w = contention_world(form)
        elif name == "order":
            w = order_world(form)
        elif name == "w150@2":
            w = make_world(form, 150, 101, **TWO)
        else:
            raise KeyError(name)
        _worlds[key] = w
    return _worlds[key]


_rules = {}
# per rule world: the counters (or "status" bits) the world aims at, as the restatement has to report them
RULE_AIMS = {}


def rule_worlds():
    """Small worlds, each built around one rule edge of the statement -> {(form, name): World} (built once); RULE_AIMS holds what
    the restatement has to report for the world to have met its edge.  The pose is the identity (Scw = 2 * identity): the camera
    centre is the origin, a point (0, 0, Z) lies at distance Z exactly and projects onto (cx, cy) = (320, 240)."""
    out = _rules
    if out:
        return out
    K = camera()
    rng = np.random.default_rng(78)
    d = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    spots = [(100.0 + 60 * k, 100.0) for k in range(4)]
    nxt = lambda x, to: np.nextafter(f32(x), f32(to), dtype=np.float32)  # noqa: E731

    def frame(xy, desc, octave=0):
        k = np.zeros(len(xy), KEYPOINT_DTYPE)
        k["x"], k["y"], k["octave"] = [p[0] for p in xy], [p[1] for p in xy], octave
        return k, np.ascontiguousarray(desc, np.uint8)

    for form in FORMS:
        T0 = EYE if form == "pose" else scaled(EYE, 2.0)

        def four(form=form, T0=T0, **kw):
            """Four points over four free features with the points' descriptors: every point is added unless a rule says no."""
            pts, nrm, dst = ML.axis_map(spots, 4.0, K)
            a = dict(form=form, points=pts, normals=nrm, dists=dst, map_desc=d[:4], mask=None, obs=[2, 3, 4, 5], T=T0, K=K)
            a["kps"], a["desc"] = frame(spots, d[:4])
            a.update(kw)
            return World(**a)

        def add(name, w, form=form, **aims):
            out[(form, name)] = w
            RULE_AIMS[(form, name)] = aims
        add("all_four", four(), n_fused=4, n_added=4)
        z = four()
        z.points[1] = [0.1, 0.0, 0.0]
        z.points[3, 2] = -1e-3
        add("zero_and_negative_depth", z.variant(), n_behind=1, n_out_image=1, n_added=2)
        # u on min_x (in) and on max_x (out), v likewise: fx = fy = 512 with X = -+1.25, Y = -+0.9375 and Z = 2 give 0, 640, 0, 480
        K512 = np.array([512.0, 0, 320.0, 0, 512.0, 240.0, 0, 0, 1], np.float32)
        kb, db = frame([(1.0, 240.0), (630.0, 240.0), (320.0, 1.0), (320.0, 470.0)], d[:4])
        on = four(kps=kb, desc=db, K=K512)
        on.points[:] = [[-1.25, 0, 2], [1.25, 0, 2], [0, -0.9375, 2], [0, 0.9375, 2]]
        on.normals[:] = on.points
        on.dists[:] = [1.0, 2.3]
        add("on_the_bounds", on.variant(), n_out_image=2, n_added=2)
        lo, hi = f32(f32(0.8) * f32(5.0)), f32(f32(1.2) * f32(3.0))
        ka, da = frame([(319.0, 240.0), (321.0, 240.0)], d[[0, 2]], np.array([5, 0]))  # (points 0 and 2 come out at levels 5 and 0)
        ax = four(kps=ka, desc=da)
        ax.points[:] = [[0, 0, lo], [0, 0, nxt(lo, 0)], [0, 0, hi], [0, 0, nxt(hi, 9)]]
        ax.normals[:] = [0, 0, 1]
        ax.dists[:] = [[5.0, 9.0], [5.0, 9.0], [1.0, 3.0], [1.0, 3.0]]
        add("distance_bounds", ax.variant(), n_out_distance=2, n_added=2)
        # the viewing angle in f64: P = (1.5, 0, 2) at distance 2.5 and N = (0.5, 0, 0.25) give dot = 1.25 = 0.5 * dist exactly (kept);
        # one ulp less in Nz gives 1.25 - 3e-8, whose f32 cosine is 0.5 again: only the f64 comparison skips it
        K256 = np.array([256.0, 0, 320.0, 0, 256.0, 240.0, 0, 0, 1], np.float32)
        kv, dv = frame([(512.0, 240.0)], d[:1])
        add("angle_edge", World(form, kv, dv, np.tile(f32([1.5, 0, 2]), (3, 1)), [[0.5, 0, 0.25], [0.5, 0, nxt(0.25, 0)], [nxt(0.5, 0), 0, 0.25]],
                                np.tile(f32([1.0, 2.4]), (3, 1)), d[:3], None, None, T0, K256), n_out_angle=2, n_added=1)
        # the octave window [level - 1, level] behind an unbounded GetFeaturesInArea: level 2; point 0 sees octaves 3 and 0 only
        # (candidates, none kept), point 1 sees octaves 1 and 2
        pts, nrm, dst = ML.axis_map(spots[:2], 4.0, K, level=2)
        ko, do = frame([spots[0], spots[0], spots[1], spots[1]], d[[0, 0, 1, 1]], np.array([3, 0, 1, 2]))
        add("octave_window", World(form, ko, do, pts, nrm, dst, d[:2], None, None, T0, K), n_with_candidates=2, n_over_dist=1, n_added=1)
        # the chi-square gate: octave 0, features 2.44 and 2.45 pixels to the right of the projections (e2 = 5.95 and 6.00)
        kc, dc = frame([(spots[0][0] + 2.44, spots[0][1]), (spots[1][0] + 2.45, spots[1][1])], d[:2])
        pts, nrm, dst = ML.axis_map(spots[:2], 4.0, K)
        add("chi_square_edge", World(form, kc, dc, pts, nrm, dst, d[:2], None, None, T0, K), n_with_candidates=2,
            n_added=1 if form == "pose" else 2, n_over_dist=1 if form == "pose" else 0)
        k2, d2 = frame(spots[:2], np.stack([_flip(d[0], TH_LOW, rng), _flip(d[1], TH_LOW + 1, rng)]))
        add("distance_50_and_51", World(form, k2, d2, pts, nrm, dst, d[:2], None, None, T0, K), n_added=1, n_over_dist=1)
        # a candidate at distance 256 under th_low = 256: the pose form's `dist < bestDist` from 256 never picks it, the Scw form does
        add("distance_256", World(form, *frame(spots[:1], ~d[:1]), pts[:1], nrm[:1], dst[:1], d[:1], None, None, T0, K, th_low=256),
            n_added=0 if form == "pose" else 1, n_over_dist=1 if form == "pose" else 0)
        # obs equal (the occupant is replaced) and greater by one (the point is replaced): points 0 and 1 meet points 2 and 3,
        # which features 0 and 1 hold (and which are therefore not searched)
        ob = four(obs=[4, 4, 4, 5], matches=np.array([2, 3, -1, -1], np.int32))
        add("obs_equal_and_greater", ob, n_in_kf=2, n_fused=2, n_replaced_occupant=1 if form == "pose" else 0,
            n_kept_occupant=1 if form == "pose" else 2)
        # a masked-out occupant stays bad for the next point: points 0 and 1 both over feature 0, which holds point 3
        kk, dk = frame([spots[0]], d[:1])
        pts2, nrm2, dst2 = ML.axis_map([spots[0], (spots[0][0] + 0.2, spots[0][1]), spots[2], spots[3]], 4.0, K)
        add("bad_occupant_stays", World(form, kk, dk, pts2, nrm2, dst2, d[[0, 0, 2, 3]], np.array([1, 1, 1, 0], np.uint8), None, T0, K,
                                        matches=np.array([3], np.int32)), n_bad_occupant=2, n_chained=0, n_in_kf=1)
        un = np.array([UNMAPPED, UNMAPPED, UNMAPPED, -1], np.int32)
        add("unmapped_with_counts", four(matches=un, occ_obs=np.array([2, 4, -1, 0], np.int32)), n_bad_occupant=1,
            n_replaced_occupant=1 if form == "pose" else 0, n_kept_occupant=1 if form == "pose" else 2, n_added=1)
        add("unmapped_without_counts", four(matches=un), n_added=1, n_bad_occupant=3 if form == "pose" else 0,
            n_kept_occupant=0 if form == "pose" else 3, status=BAD_INPUT if form == "pose" else 0)
        add("entry_beyond_the_set", four(matches=np.array([-1, 4, -5, 99], np.int32)), status=BAD_INPUT, n_added=2, n_bad_occupant=2)
        big = four(obs=[70000, -3, 4, 5], matches=np.array([UNMAPPED, UNMAPPED, UNMAPPED, -1], np.int32),
                   occ_obs=np.array([65535, 0, 1 << 20, 0], np.int32))
        add("counts_out_of_range", big, status=BAD_INPUT if form == "pose" else 0, n_replaced_occupant=2 if form == "pose" else 0,
            n_kept_occupant=1 if form == "pose" else 3)
        add("masked_point_named", four(mask=np.array([1, 0, 1, 1], np.uint8), matches=np.array([1, -1, -1, -1], np.int32)), n_in_kf=1,
            n_points=3)
        bad = T0.copy()
        bad[10] = np.nan
        add("nonfinite_pose", four(T=bad, matches=np.array([1, -1, -1, -1], np.int32)), status=NONFINITE, n_points=3, n_fused=0)
        if form == "scw":
            add("zero_scw", four(T=np.zeros(12, np.float32)), status=NONFINITE, n_points=4, n_fused=0)
        nf = four()
        nf.points[0, 0], nf.normals[1, 2], nf.dists[2, 0] = np.nan, np.inf, np.nan
        add("nonfinite_point", nf.variant(), status=NONFINITE, n_added=1)
        add("no_features", four(kps=np.zeros(0, KEYPOINT_DTYPE), desc=np.zeros((0, 32), np.uint8)), n_points=4, n_with_candidates=0)
        add("no_points", World(form, *frame(spots, d[:4]), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 32), np.uint8),
                               None, None, T0, K, matches=np.array([-1, UNMAPPED, -1, -1], np.int32), occ_obs=np.zeros(4, np.int32)),
            n_points=0, n_fused=0)
    return out
