"""ctypes wrapper around tests/cpp/map_update_ref.cpp -- the CPU restatement of the map-point update behind the local bundle
adjustment (include/orbx.h, "local mapping: updating the map points") -- compiled on first use with g++ -O2 -ffp-contract=off into
a private temporary directory, as tests/fuse_ref_lib.py compiles its source; a second, independently written numpy statement
(np.sort + index for the median, argmin for the pick, np.float32 scalar operations in the stated order with the norm in f64);
and the worlds that tests/test_map_update_host.py and tests/test_gpu_map_update.py share, built on lba_ref_lib's windows.  TEST
INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

import lba_ref_lib as L
from lba_ref_lib import KEYPOINT_DTYPE, NLEVELS, NLEVELS_2, SCALE_FACTOR_2, SECOND  # noqa: F401
from sim3_ref_lib import scale_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "map_update_ref.cpp")
MAIN_SRC = os.path.join(ROOT, "tests", "cpp", "map_update_ref_main.cpp")
COUNTERS = ("status", "n_points", "n_observations", "n_erased", "n_bad_points", "n_cleared", "n_ref_moved", "max_observers", "n_free")
MAP_RESULT_DTYPE = np.dtype([(n, "<i4") for n in COUNTERS] + [("reserved", "<i4", 7)])
assert MAP_RESULT_DTYPE.itemsize == 64
NORMALS, DESCRIPTORS, BAD_INPUT, NONFINITE = 1, 2, 2, 4
OUTPUTS = ("rows", "mask_out", "ref", "obs", "desc", "normals", "dist")
FILL = 0xA5  # what every output holds before a call: what is not written shows
_L = None


def build(src=SRC, flags=("-O2",), exe_main=None):
    """Compiles the restatement: a shared object, or with exe_main (a source with its own main) a program -> its path."""
    d = tempfile.mkdtemp(prefix="map_update_ref_")
    atexit.register(shutil.rmtree, d, True)
    out = os.path.join(d, "map_update_ref_main" if exe_main else "libmap_update_ref.so")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", *flags]
    cmd += [exe_main, src, "-o", out] if exe_main else ["-fPIC", "-shared", src, "-o", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("map_update_ref.cpp does not compile:\n" + p.stdout)
    return out


def lib() -> ctypes.CDLL:
    global _L
    if _L is None:
        Lb = ctypes.CDLL(build())
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        Lb.mapr_update.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp]
        Lb.mapr_update.restype = None
        _L = Lb
    return _L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class World:
    """One problem: entry e names frame frames[e] of kps [F, cap] / desc [F, cap, 32] / n [F]; pose [nE, 12] and rows [nE, cap]
    are per entry; outlier [nE, cap] or None; map_pts [map_cap, 3], map_mask [map_cap] or None, map_ref [map_cap] or None, map_n,
    n_free."""

    def __init__(self, kps, desc, n, pose, rows, outlier, map_pts, map_mask, map_ref, map_n, n_free, frames=None):
        self.kps, self.desc, self.n, self.pose, self.rows, self.outlier = kps, desc, n, pose, rows, outlier
        self.map_pts, self.map_mask, self.map_ref, self.map_n, self.n_free = map_pts, map_mask, map_ref, int(map_n), int(n_free)
        self.n_entries, self.cap, self.map_cap = rows.shape[0], kps.shape[1], map_pts.shape[0]
        self.frames = np.arange(max(self.n_entries, 1), dtype=np.int32) if frames is None else np.ascontiguousarray(frames, np.int32)

    def copy(self):
        c = lambda a: None if a is None else a.copy()  # noqa: E731
        w = World(self.kps.copy(), self.desc.copy(), self.n.copy(), self.pose.copy(), self.rows.copy(), c(self.outlier),
                  self.map_pts.copy(), c(self.map_mask), c(self.map_ref), self.map_n, self.n_free, self.frames.copy())
        w.n_entries = self.n_entries
        return w

    def padded(self, cap, map_cap):
        """The same problem in arrays of larger capacities, with a mask, a reference array and outlier bytes."""
        F, nE = self.kps.shape[0], self.n_entries
        kps, desc = np.zeros((F, cap), KEYPOINT_DTYPE), np.zeros((F, cap, 32), np.uint8)
        rows, outlier = np.full((max(nE, 1), cap), -1, np.int32), np.zeros((max(nE, 1), cap), np.uint8)
        kps[:, :self.cap], desc[:, :self.cap] = self.kps, self.desc
        rows[:nE, :self.cap] = self.rows[:nE]
        if self.outlier is not None:
            outlier[:nE, :self.cap] = self.outlier[:nE]
        pts, mask, ref = np.zeros((map_cap, 3), np.float32), np.zeros(map_cap, np.uint8), np.full(map_cap, -1, np.int32)
        pts[:self.map_cap] = self.map_pts
        mask[:self.map_cap] = 1 if self.map_mask is None else self.map_mask
        if self.map_ref is not None:
            ref[:self.map_cap] = self.map_ref
        pose = np.zeros((max(nE, 1), 12), np.float32)
        pose[:nE] = self.pose[:nE]
        w = World(kps, desc, self.n.copy(), pose, rows, outlier, pts, mask, ref, self.map_n, self.n_free, self.frames.copy())
        w.n_entries = nE
        return w


def blank_outputs(w: World):
    """The outputs as a caller may hold them before the call: rows, mask and ref are the inputs; the rest is FILL."""
    mc = w.map_cap
    f = lambda shape, dt: np.frombuffer(bytes([FILL]) * int(np.prod(shape) * np.dtype(dt).itemsize), dt).reshape(shape).copy()  # noqa: E731
    return dict(rows=w.rows.copy(), mask_out=f((mc,), np.uint8) if w.map_mask is None else w.map_mask.copy(),
                ref=None if w.map_ref is None else w.map_ref.copy(), obs=f((mc,), np.int32), desc=f((mc, 32), np.uint8),
                normals=f((mc, 3), np.float32), dist=f((mc, 2), np.float32))


def _scale(scale, nlevels):
    return np.ascontiguousarray(scale_table(nlevels) if scale is None else scale, np.float32)


def update(w: World, what=3, scale=None, nlevels=NLEVELS, in_place=True, into=None):
    """The restatement for one problem -> dict(OUTPUTS..., res).  in_place: mask_out starts as the mask (else as FILL).  into: the
    outputs as they stand (contiguous arrays, rewritten where the call writes) instead of blank ones."""
    sc = _scale(scale, nlevels)
    o = blank_outputs(w) if into is None else dict(into)
    if into is None and not in_place and w.map_mask is not None:
        o["mask_out"][:] = FILL
    res = np.zeros(1, MAP_RESULT_DTYPE)
    lib().mapr_update(_p(w.kps), _p(w.desc), _p(w.n), _p(w.frames), w.n_entries, w.n_free, _p(w.pose), _p(o["rows"]), _p(w.outlier), w.cap,
                      _p(w.map_pts), _p(w.map_mask), _p(o["mask_out"]), _p(o["ref"]), w.map_n, w.map_cap, _p(sc), len(sc), int(what),
                      _p(o["normals"]), _p(o["dist"]), _p(o["desc"]), _p(o["obs"]), _p(res))
    o["res"] = res[0].copy()
    return o


# ---- the second statement: numpy, nothing shared with the C++ ----

def _centre(pose12):
    R, t = pose12[:9].reshape(3, 3).astype(np.float64), pose12[9:].astype(np.float64)
    out = np.zeros(3, np.float32)
    for r in range(3):
        sd = 0.0
        for k in range(3):
            sd += R[k, r] * t[k]
        out[r] = np.float32(-1.0 * sd)
    return out


def _norm(d):
    x, y, z = (float(v) for v in d)
    return np.float32(np.sqrt((x * x + y * y) + z * z))


def update_numpy(w: World, what=3, scale=None, nlevels=NLEVELS, in_place=True):
    """The rules of include/orbx.h read off one after the other -> dict(OUTPUTS..., res)."""
    f32 = np.float32
    sc = _scale(scale, nlevels)
    o = blank_outputs(w)
    if not in_place and w.map_mask is not None:
        o["mask_out"][:] = FILL
    res = np.zeros(1, MAP_RESULT_DTYPE)[0]
    nE, frames = w.n_entries, w.frames

    def flagged(status):
        res["status"] = status
        o["res"] = res
        return o
    if not 0 <= w.map_n <= w.map_cap:
        return flagged(BAD_INPUT)
    status = 0
    cnt = [int(w.n[frames[e]]) for e in range(nE)]
    if any(c < 0 or c > w.cap for c in cnt) or len(set(int(frames[e]) for e in range(nE))) != nE:
        status |= BAD_INPUT
    if not np.isfinite(w.pose[:nE]).all():
        status |= NONFINITE
    if status:
        return flagged(status)
    named = [w.rows[e, :cnt[e]] for e in range(nE)]
    if any((r >= w.map_n).any() for r in named):
        return flagged(BAD_INPUT)
    usable = np.zeros(w.map_n, bool)
    usable[:] = True if w.map_mask is None else w.map_mask[:w.map_n] != 0
    vertex = np.zeros(w.map_n, bool)
    for e in range(w.n_free):
        vertex[named[e][named[e] >= 0]] = True
    vertex &= usable
    observers = {int(i): [] for i in np.flatnonzero(vertex)}
    lost = set()
    for e in range(nE):
        on = [(int(i), f) for f, i in enumerate(named[e]) if i >= 0 and vertex[i]]
        if len(set(i for i, _ in on)) != len(on):
            status |= BAD_INPUT
        for i, f in on:
            if w.outlier is not None and w.outlier[e, f]:
                lost.add(i)
            else:
                observers[i].append((e, f))
    if status:
        return flagged(status)
    with np.errstate(all="ignore"):
        centres = [_centre(w.pose[e]) for e in range(nE)]
        good, bad, moved = {}, [], 0
        for i, ob in observers.items():
            if not np.isfinite(w.map_pts[i]).all():
                status |= NONFINITE
                continue
            if (i in lost and len(ob) <= 2) or not ob:
                bad.append(i)
                continue
            want = -1 if w.map_ref is None else int(w.map_ref[i])
            at = next((k for k, (e, _) in enumerate(ob) if want >= 0 and frames[e] == want), 0)
            e, f = ob[at]
            if not 0 <= w.kps["octave"][frames[e], f] < len(sc):
                status |= BAD_INPUT
            lens = [_norm(w.map_pts[i] - centres[e2]) for e2, _ in ob]
            if not all(np.isfinite(v) and v > 0 for v in lens):
                status |= NONFINITE
            moved += int(want >= 0 and frames[e] != want)
            good[i] = (ob, at, lens)
    if status:
        return flagged(status)
    for e in range(nE):
        for f in range(cnt[e]):
            i = int(w.rows[e, f])
            if i >= 0 and vertex[i]:
                if w.outlier is not None and w.outlier[e, f]:
                    o["rows"][e, f] = -1
                    res["n_erased"] += 1
                elif i in bad:
                    o["rows"][e, f] = -1
                    res["n_cleared"] += 1
    for i in bad:
        o["mask_out"][i], o["obs"][i] = 0, 0
    for i, (ob, at, lens) in good.items():
        o["mask_out"][i] = 1 if w.map_mask is None else w.map_mask[i]
        o["obs"][i] = len(ob)
        if o["ref"] is not None:
            o["ref"][i] = frames[ob[at][0]]
        P = w.map_pts[i]
        if what & NORMALS:
            normal = np.zeros(3, f32)
            for (e, _), ln in zip(ob, lens):
                d = P - centres[e]
                for k in range(3):
                    normal[k] = f32(normal[k] + f32(d[k] / ln))
            for k in range(3):
                normal[k] = f32(normal[k] / f32(len(ob)))
            e, f = ob[at]
            mx = f32(_norm(P - centres[e]) * sc[w.kps["octave"][frames[e], f]])
            o["normals"][i], o["dist"][i] = normal, (f32(mx / sc[len(sc) - 1]), mx)
        if what & DESCRIPTORS:
            D = np.stack([w.desc[frames[e], f] for e, f in ob])
            dist = np.unpackbits(D[:, None, :] ^ D[None, :, :], axis=2).sum(axis=2)
            med = np.sort(dist, axis=1)[:, (len(ob) - 1) // 2]
            o["desc"][i] = D[int(np.argmin(med))]
    res["n_points"], res["n_bad_points"], res["n_ref_moved"], res["n_free"] = len(observers), len(bad), moved, w.n_free
    res["n_observations"] = sum(len(g[0]) for g in good.values())
    res["max_observers"] = max([len(ob) for ob in observers.values()] + [0])
    o["res"] = res
    return o


def same(a, b):
    """The names of the outputs in which two result dictionaries differ (bit for bit)."""
    bad = [k for k in OUTPUTS if (a[k] is None) != (b[k] is None) or (a[k] is not None and a[k].tobytes() != b[k].tobytes())]
    return bad + (["res"] if a["res"].tobytes() != b["res"].tobytes() else [])


# ---- the worlds ----

def from_lba(lw: L.World, seed=0, erase=0.0, ref="mixed", flips=24, use_ref=True, use_outlier=True) -> World:
    """A local window of lba_ref_lib as a problem of the update: every observation of a point gets the point's own random
    descriptor with up to `flips` bits turned (so that the medians differ), the other features random ones; `erase`: the share
    of the observations of vertices whose outlier byte is set (plus a few bytes on features that name nothing or no vertex);
    ref: 'none' (all -1), 'first', 'last' (the last observer's frame) or 'mixed' (by point index: -1, a frame that observes it,
    a frame that does not)."""
    rng = np.random.default_rng(7100 + seed)
    nE, cap, mc = lw.n_entries, lw.cap, lw.map_cap
    F = max(nE, 1)
    base = rng.integers(0, 256, (mc, 32), dtype=np.uint8)
    desc = rng.integers(0, 256, (F, cap, 32), dtype=np.uint8)
    outlier = np.zeros((F, cap), np.uint8) if use_outlier else None
    mask = np.ones(mc, bool) if lw.map_mask is None else lw.map_mask != 0
    vertex = np.zeros(mc, bool)
    for e in range(lw.n_free):
        r = lw.rows[e, :lw.n[lw.frames[e]]]
        vertex[r[(r >= 0) & (r < lw.map_n)]] = True
    vertex &= mask
    seen = [[] for _ in range(mc)]
    for e in range(nE):
        fr = lw.frames[e]
        for f in range(lw.n[fr]):
            i = lw.rows[e, f]
            if 0 <= i < lw.map_n:
                d = np.unpackbits(base[i])
                d[rng.choice(256, int(rng.integers(0, flips + 1)), replace=False)] ^= 1
                desc[fr, f] = np.packbits(d)
                seen[i].append(int(fr))
                if use_outlier and vertex[i] and rng.random() < erase:
                    outlier[e, f] = 1
            elif use_outlier and erase > 0 and rng.random() < 0.2:
                outlier[e, f] = 1  # (names nothing: ignored)
    map_ref = None
    if use_ref:
        map_ref = np.full(mc, -1, np.int32)
        for i in range(lw.map_n):
            if not seen[i] or ref == "none":
                continue
            kind = {"first": 1, "last": 2}.get(ref, i % 4)
            if kind == 1:
                map_ref[i] = seen[i][0]
            elif kind == 2:
                map_ref[i] = seen[i][-1]
            elif kind == 3:
                map_ref[i] = F + 5  # (a keyframe outside the window: gone)
    pose = np.stack([lw.pose[lw.frames[e]] for e in range(nE)]) if nE else np.zeros((1, 12), np.float32)
    rows = lw.rows.copy() if nE else np.full((1, cap), -1, np.int32)
    w = World(lw.kps.copy(), desc, lw.n.copy(), pose.astype(np.float32), rows, outlier, lw.map_pts.copy(),
              None if lw.map_mask is None else lw.map_mask.copy(), map_ref, lw.map_n, lw.n_free, lw.frames.copy())
    w.n_entries = nE
    return w


def make_world(n_free, n_fixed, n_points, seed=0, erase=0.1, ref="mixed", obs_per_point=4, **kw):
    kw.setdefault("outliers", 0)
    return from_lba(L.make_world(n_free, n_fixed, n_points, seed, obs_per_point=obs_per_point, **kw), seed, erase=erase, ref=ref)


def tiny(n_obs, n_free=None, seed=0, erase=(), ref=-1, fixed_only=False, desc=None, octaves=None):
    """One point (index 0) seen by feature 0 of each of n_obs keyframes on a baseline; a second point (index 1) that only the
    LAST keyframe names; erase: the entries whose observation of point 0 is an outlier; ref: d_map_ref[0]; n_free: default all;
    fixed_only: point 0 is named by fixed entries only (entry 0, the one free keyframe, names nothing of it); desc: [n_obs, 32]
    descriptors of the observations."""
    rng = np.random.default_rng(9000 + seed)
    nE = n_obs + (1 if fixed_only else 0)
    n_free = (1 if fixed_only else nE) if n_free is None else n_free
    cap, mc = 3, 4
    kps, d = np.zeros((nE, cap), KEYPOINT_DTYPE), rng.integers(0, 256, (nE, cap, 32), dtype=np.uint8)
    kps["octave"] = rng.integers(0, NLEVELS, (nE, cap)) if octaves is None else np.asarray(octaves).reshape(nE, 1)
    n = np.full(nE, cap, np.int32)
    rows, outlier = np.full((nE, cap), -1, np.int32), np.zeros((nE, cap), np.uint8)
    pose = np.zeros((nE, 12), np.float32)
    first = 1 if fixed_only else 0
    for e in range(nE):
        pose[e] = np.r_[L.rotvec(rng.normal(0, 0.05, 3)).reshape(9), [-0.3 * e, 0.02 * e, 0.01]]
        if e >= first:
            rows[e, 0] = 0
            if desc is not None:
                d[e, 0] = desc[e - first]
            if (e - first) in erase:
                outlier[e, 0] = 1
    rows[nE - 1, 1] = 1
    rows[0, 2] = -2
    pts = np.array([[0.3, -0.2, 5.0], [1.0, 0.5, 6.0], [0, 0, 1], [0, 0, 1]], np.float32)
    return World(kps, d, n, pose, rows, outlier, pts, np.array([1, 1, 0, 0], np.uint8), np.array([ref, -1, -1, -1], np.int32), 2, n_free)


def garbage(w: World, what: str) -> World:
    """Each garbage case of rule 7 on a copy."""
    q = w.copy()
    mask = np.ones(q.map_cap, bool) if q.map_mask is None else q.map_mask != 0
    e, f = [(e, f) for e in range(q.n_free) for f in range(q.n[q.frames[e]]) if 0 <= q.rows[e, f] < q.map_n and mask[q.rows[e, f]]][0]
    i = q.rows[e, f]
    if what == "count":
        q.n[q.frames[1]] = q.cap + 1
    elif what == "map_count":
        q.map_n = q.map_cap + 1
    elif what == "row":
        q.rows[q.n_entries - 1, 0] = q.map_n
    elif what == "duplicate":
        g = [g for g in range(q.n[q.frames[e]]) if g != f and q.rows[e, g] < 0][0]
        q.rows[e, g] = i
    elif what == "frame_twice":
        q.frames[2] = q.frames[0]
    elif what == "octave":  # every observation of the point: whichever is the reference
        for e2 in range(q.n_entries):
            for f2 in range(q.n[q.frames[e2]]):
                if q.rows[e2, f2] == i:
                    q.kps["octave"][q.frames[e2], f2] = 99
                    if q.outlier is not None:
                        q.outlier[e2, f2] = 0
    elif what == "nan_pose":
        q.pose[q.n_entries - 1, 10] = np.nan
    elif what == "inf_point":
        q.map_pts[i, 1] = np.inf
    elif what == "zero_len":  # the point at the camera centre of its observer
        q.pose[e] = np.r_[np.eye(3).reshape(9), np.zeros(3)]
        q.map_pts[i] = 0.0
        if q.outlier is not None:
            q.outlier[e, f] = 0
    else:
        raise KeyError(what)
    return q


GARBAGE = {"count": BAD_INPUT, "map_count": BAD_INPUT, "row": BAD_INPUT, "duplicate": BAD_INPUT, "frame_twice": BAD_INPUT,
           "octave": BAD_INPUT, "nan_pose": NONFINITE, "inf_point": NONFINITE, "zero_len": NONFINITE}

_worlds = {}


def world(name: str) -> World:
    """Named worlds, made once.
    window: 4 free + 3 fixed keyframes, 120 points, a tenth of the observations erased, mixed references;
    clean: no outlier array and no reference array at all;
    all_free: n_free == count (the form behind Fuse); all_erased: every observation of a vertex erased;
    second: the window under K_ANISO and 5 levels of 1.37."""
    if name not in _worlds:
        if name == "window":
            w = make_world(4, 3, 120, 1)
        elif name == "clean":
            w = from_lba(L.make_world(3, 2, 90, 2, outliers=0), 2, use_ref=False, use_outlier=False)
        elif name == "all_free":
            w = make_world(5, 0, 80, 3, erase=0.15)
        elif name == "all_erased":
            w = make_world(3, 2, 60, 4, erase=1.0)
        elif name == "second":
            w = make_world(4, 3, 100, 8, **SECOND)
        else:
            raise KeyError(name)
        _worlds[name] = w
    return _worlds[name]


def _bits(*sets):
    """Descriptors [len(sets), 32] with the given bit indices set."""
    d = np.zeros((len(sets), 256), np.uint8)
    for k, s in enumerate(sets):
        d[k, list(s)] = 1
    return np.packbits(d, axis=1, bitorder="little")


# Each rule world reports the counters it aims at; tests/test_map_update_host.py asserts them on the restatement's record
# before it compares the two statements, and looks at the outputs in detail.
RULE_AIMS = {
    "obs1": dict(n_points=2, max_observers=1, n_observations=2, n_bad_points=0),
    "obs2": dict(n_points=2, max_observers=2, n_observations=3, n_bad_points=0),
    "obs3": dict(n_points=2, max_observers=3, n_observations=4, n_bad_points=0),
    "obs4": dict(n_points=2, max_observers=4, n_observations=5),
    "obs5": dict(n_points=2, max_observers=5, n_observations=6),
    "tie": dict(n_points=2, max_observers=3),
    "fixed_only": dict(n_points=0, n_observations=0, n_free=1),
    "outlier_elsewhere": dict(n_points=1, n_erased=0, n_bad_points=0),
    "three_to_two": dict(n_erased=1, n_bad_points=1, n_cleared=2, n_observations=1),
    "four_to_three": dict(n_erased=1, n_bad_points=0, n_cleared=0, max_observers=3),
    "ref_erased": dict(n_erased=1, n_ref_moved=1, n_bad_points=0),
    "ref_kept": dict(n_ref_moved=0, n_erased=0),
    "ref_gone": dict(n_ref_moved=1),
    "ref_negative": dict(n_ref_moved=0),
    "ref_null": dict(n_ref_moved=0),
}


def rule_worlds():
    """name -> World, one per aim of RULE_AIMS."""
    out = {"obs%d" % k: tiny(k, seed=k) for k in (1, 2, 3, 4, 5)}
    # three rows with the median 4: d01 = 4, d12 = 4, d02 = 8
    out["tie"] = tiny(3, seed=6, desc=_bits((), (0, 1, 2, 3), (0, 1, 2, 3, 4, 5, 6, 7)))
    out["fixed_only"] = tiny(3, seed=7, fixed_only=True)
    w = tiny(3, seed=8, n_free=2)   # point 1 is named by the last keyframe only, which is fixed: no vertex
    w.outlier[2, 1] = 1
    w.outlier[0, 2] = 1             # (and a byte on a feature that names nothing)
    out["outlier_elsewhere"] = w
    out["three_to_two"] = tiny(3, seed=9, erase=(1,))
    out["four_to_three"] = tiny(4, seed=10, erase=(0,))
    out["ref_erased"] = tiny(4, seed=11, erase=(1,), ref=1)
    out["ref_kept"] = tiny(3, seed=12, ref=2)
    out["ref_gone"] = tiny(3, seed=13, ref=17)
    out["ref_negative"] = tiny(3, seed=14, ref=-1)
    w = tiny(3, seed=15)
    w.map_ref = None
    out["ref_null"] = w
    return out
