"""ctypes wrapper around tests/cpp/match_bow_ref.cpp -- the CPU restatement of ORBmatcher::SearchByBoW (include/orbx.h, "matching
through the FeatureVector") -- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary directory, as
tests/db_ref_lib.py compiles its source; a second, independently written numpy statement of the same rules; and the worlds
(frames, FeatureVectors, pairs) that tests/test_match_bow_host.py and tests/test_gpu_match_bow.py share.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

import bow_ref_lib as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "match_bow_ref.cpp")
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
COUNTERS = ("by_distance", "by_ratio", "changed_by_taken", "by_orientation")
_L = None


def lib() -> ctypes.CDLL:
    global _L
    if _L is not None:
        return _L
    d = tempfile.mkdtemp(prefix="match_bow_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libmatch_bow_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", SRC, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("match_bow_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.mbr_search_by_bow.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, ctypes.c_float, i32, vp, vp]
    _L = L
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _args(ang, desc, node, feat):
    a = np.ascontiguousarray(ang, np.float32).reshape(-1)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n, f = np.ascontiguousarray(node, np.uint32).reshape(-1), np.ascontiguousarray(feat, np.uint32).reshape(-1)
    assert len(a) == len(d) and len(n) == len(f)
    return a, d, n, f


def search_by_bow(kf, f, mask=None, nnratio=0.6, check_orientation=True):
    """The restatement.  kf, f = (angles [n], descriptors [n, 32], fv_node, fv_feat) -> (matches_f int32 [n_F], nmatches,
    {counter: value})."""
    ak, dk, nk, fk = _args(*kf)
    af, df, nf, ff = _args(*f)
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8).reshape(-1)
    assert m is None or len(m) == len(ak)
    out, cnt = np.full(max(len(af), 1), -7, np.int32), np.zeros(4, np.int64)
    nm = lib().mbr_search_by_bow(_p(ak), _p(dk), len(ak), _p(nk), _p(fk), len(nk), _p(af), _p(df), len(af), _p(nf), _p(ff), len(nf),
                                 _p(m), float(nnratio), int(bool(check_orientation)), _p(out), _p(cnt))
    return out[:len(af)].copy(), int(nm), dict(zip(COUNTERS, (int(c) for c in cnt)))


# ---- the second statement: numpy, per node one distance matrix, nothing shared with the C++ one ----

def search_by_bow_numpy(kf, f, mask=None, nnratio=0.6, check_orientation=True):
    """-> (matches_f, nmatches)."""
    ak, dk, nk, fk = _args(*kf)
    af, df, nf, ff = _args(*f)
    f32 = np.float32
    ones = np.array([bin(v).count("1") for v in range(256)], np.uint8)  # set bits of a byte
    ok_k, ok_f = fk < len(ak), ff < len(af)
    nk, fk, nf, ff = nk[ok_k], fk[ok_k], nf[ok_f], ff[ok_f]
    matches = np.full(len(af), -1, np.int32)
    bins = np.full(len(af), -1, np.int64)
    for node in np.intersect1d(nk, nf):
        rows, cols = np.sort(fk[nk == node]), np.sort(ff[nf == node])
        dist = ones[dk[rows][:, None, :] ^ df[cols][None, :, :]].sum(axis=2, dtype=np.int64)  # [rows, cols]
        free = np.ones(len(cols), bool)
        for r, i in enumerate(rows):
            if mask is not None and not mask[i]:
                continue
            d = np.sort(np.concatenate([dist[r][free], [256, 256]]), kind="stable")
            best1, best2 = int(d[0]), int(d[1])
            if best1 > 50 or not f32(best1) < f32(nnratio) * f32(best2):
                continue
            c = int(np.flatnonzero(free & (dist[r] == best1))[0])
            free[c] = False
            j = int(cols[c])
            matches[j] = i
            rot = f32(ak[i]) - f32(af[j])
            if rot < 0:
                rot = f32(rot + f32(360.0))
            x = float(f32(rot * f32(f32(30) / f32(360.0))))
            if math.isfinite(x):
                b = math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)  # roundf: halves away from zero
                b = 0 if b == 30 else b
                bins[j] = b if 0 <= b < 30 else -1
    if check_orientation:
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

CAP = 1024
COUNTS = (1000, 0, 1, 3, 40, 150)  # features per frame, in turn
N_KF = 12                          # frames 0 .. 11 are keyframes, frame 12 + g is the frame made from keyframe g
N_FRAMES = 2 * N_KF
# (keyframe, frame): every keyframe with its own frame; a frame with itself; the empty (1, 7, 13, 19) and the 1-feature (2, 8, 14,
# 20) frames on either side; a frame as the keyframe of its keyframe; frames reused across pairs
PAIRS = [(g, N_KF + g) for g in range(N_KF)] + [(0, 0), (0, 13), (1, 12), (0, 14), (2, 12), (12, 0), (18, 6), (5, 16), (4, 17),
                                                 (13, 1), (14, 14), (17, 5)]
BIG_PAIRS = [p for p, (a, b) in enumerate(PAIRS) if COUNTS[a % 6] == 1000 and COUNTS[b % 6] == 1000]  # 1000 x 1000 features
CONFIGS = [(ori, ratio, masked) for ori in (0, 1) for ratio in (0.6, 0.9) for masked in (False, True)]


def base_vocabularies(golden):
    return {"irregular": R.irregular_tree(3, k=4, L=5, n_nodes=300),
            "full1000": R.full_vocabulary(golden["canonical/dbow0/desc"], k=10, L=3)}


def levelsups(voc):
    """node = word; intermediate nodes; one node for the whole frame (the chunked path beyond 256 features on both sides)"""
    return (0, 2, voc.header[1])


def make_frames(voc, seed):
    """-> (kps [N_FRAMES, CAP] KEYPOINT_DTYPE, desc [N_FRAMES, CAP, 32], n [N_FRAMES], mask [N_FRAMES, CAP] uint8).  A keyframe's
    descriptors lie near the vocabulary's nodes, one in sixteen a near copy of another of its features (two candidates at almost
    the same distance: ratio rejections, and matches that depend on what was taken before).  Its frame: a permuted copy with 0 to
    12 bits flipped per descriptor, a third of the features replaced by unrelated ones, and the angles the keyframe's plus a
    common rotation plus noise wide enough that some bins lose."""
    rng = np.random.default_rng(seed)
    kps = np.zeros((N_FRAMES, CAP), KEYPOINT_DTYPE)
    desc, n = np.zeros((N_FRAMES, CAP, 32), np.uint8), np.zeros(N_FRAMES, np.int32)
    for g in range(N_KF):
        c = COUNTS[g % len(COUNTS)]
        n[g] = n[N_KF + g] = c
        if c == 0:
            continue
        d = R.features_near(voc, c, seed + 17 * g + 1, ands=4)
        for i in range(7, c, 16):  # near copies
            d[i] = d[i - 3]
            d[i, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        ang = rng.uniform(0.0, 360.0, c).astype(np.float32)
        perm = rng.permutation(c)
        d2, a2 = d[perm].copy(), ang[perm].copy()
        for i in range(c):
            for _ in range(int(rng.integers(0, 13))):
                d2[i, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        unrelated = rng.random(c) < 1.0 / 3.0
        d2[unrelated] = rng.integers(0, 256, (int(unrelated.sum()), 32), dtype=np.uint8)
        a2 = (a2 - np.float32(40.0 + 3.0 * g) + rng.normal(0.0, 14.0, c).astype(np.float32)).astype(np.float32)
        a2 = np.mod(a2, np.float32(360.0)).astype(np.float32)
        a2[a2 >= 360.0] = 0.0
        desc[g, :c], desc[N_KF + g, :c] = d, d2
        kps["angle"][g, :c], kps["angle"][N_KF + g, :c] = ang, a2
    kps["x"], kps["y"] = rng.uniform(0, 640, kps.shape), rng.uniform(0, 480, kps.shape)
    mask = (rng.random((N_FRAMES, CAP)) < 0.8).astype(np.uint8)
    return kps, desc, n, mask


def feature_vectors(voc, desc, n, levelsup):
    """The restatement's FeatureVectors (tests/bow_ref_lib.py; what the device's transform writes bit for bit) ->
    [(fv_node, fv_feat)] per frame."""
    out = []
    for f in range(len(n)):
        r = voc.transform(desc[f, :n[f]], levelsup)
        out.append((r["fv_node"].copy(), r["fv_feat"].copy()))
    return out


def reference_pair(kps, desc, n, fv, mask, pair, cfg, fn=search_by_bow):
    """One pair of a world through a statement (fn) under cfg = (check_orientation, nnratio, masked)."""
    a, b = pair
    ori, ratio, masked = cfg
    return fn((kps["angle"][a, :n[a]], desc[a, :n[a]], fv[a][0], fv[a][1]), (kps["angle"][b, :n[b]], desc[b, :n[b]], fv[b][0], fv[b][1]),
              mask[a, :n[a]] if masked else None, ratio, bool(ori))


WORLDS = [(name, li) for name in ("irregular", "full1000") for li in range(3)]  # (vocabulary, index into levelsups())
_vocs, _worlds = {}, {}


class World:
    """One vocabulary at one levelsup: the frames, their FeatureVectors from the restatement of the transform, and (computed once
    per configuration, then left unchanged) what the restatement of SearchByBoW gives for every pair of PAIRS."""

    def __init__(self, name, voc, levelsup):
        self.name, self.voc, self.levelsup = name, voc, int(levelsup)
        self.kps, self.desc, self.n, self.mask = make_frames(voc, 900)
        self.fv = feature_vectors(voc, self.desc, self.n, self.levelsup)
        self._expected = {}

    def expected(self, cfg):
        """-> [(matches_f, nmatches, counters)] per pair."""
        if cfg not in self._expected:
            self._expected[cfg] = [reference_pair(self.kps, self.desc, self.n, self.fv, self.mask, pair, cfg) for pair in PAIRS]
        return self._expected[cfg]


def world(name, levelsup_index) -> World:
    key = (name, levelsup_index)
    if key not in _worlds:
        if not _vocs:
            z = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
            _vocs.update(base_vocabularies({"canonical/dbow0/desc": z["canonical/dbow0/desc"]}))
        voc = _vocs[name]
        _worlds[key] = World(name, voc, levelsups(voc)[levelsup_index])
    return _worlds[key]
