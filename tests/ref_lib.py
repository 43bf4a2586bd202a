"""ctypes wrapper around oracle/_ref/libref.so: the reference's own DBoW2 (text loader, transform, the six scoring objects),
Frame::PosInGrid / GetFeaturesInArea and ORBmatcher::SearchForInitialization, compiled unmodified by `make -C oracle ref`
(run by __graft_entry__.build() where the reference tree exists) with oracle/ref_harness.cpp as their C API.  TEST
INFRASTRUCTURE only.  The library is required: without it every call raises with the command that builds it."""
from __future__ import annotations

import ctypes
import os

import numpy as np

import bow_ref_lib as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "oracle", "_ref", "libref.so")
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
               ("class_id", "<i4")])
E_EXCEPTION, E_THROWN, E_BADARG, E_CAPACITY = -1, -2, -3, -4
_L = None


class RefError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    global _L
    if _L is not None:
        return _L
    if not os.path.exists(LIB_PATH):
        raise RefError("%s is missing: build it with `make -C oracle ref REF_ROOT=<reference checkout>` (or __graft_entry__.build() "
                       "where the reference tree exists); the reference-pinned tests need the reference's compiled code" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.ref_last_error.argtypes = []
    L.ref_last_error.restype = ctypes.c_char_p
    L.ref_voc_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
    L.ref_voc_free.argtypes = [vp]
    L.ref_voc_free.restype = None
    L.ref_voc_info.argtypes = [vp, vp]
    L.ref_voc_nodes.argtypes = [vp, vp, vp, vp, vp, vp, i32]
    L.ref_transform.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32]
    L.ref_score.argtypes = [i32, vp, vp, i32, vp, vp, i32, vp]
    L.ref_pos_in_grid.argtypes = [vp, i32, vp, vp, vp]
    L.ref_features_in_area.argtypes = [vp, i32, vp, f32, f32, f32, i32, i32, vp, i32]
    L.ref_match_init.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, f32, i32, vp, vp, vp]
    _L = L
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _check(r, what):
    if r < 0:
        raise RefError("%s failed (%d): %s" % (what, r, lib().ref_last_error().decode(errors="replace")))
    return r


class Vocabulary:
    """TemplatedVocabulary<FORB> after loadFromTextFile(path).  info: (k, L, scoring, weighting, nodes without the root, words);
    nodes is -1 when the loader rejected the header and kept no tree."""

    def __init__(self, path):
        h = ctypes.c_void_p(0)
        _check(lib().ref_voc_load(os.fsencode(path), ctypes.byref(h)), "loadFromTextFile(%s)" % path)
        self._h = h
        info = np.zeros(6, np.int32)
        _check(lib().ref_voc_info(self._h, _p(info)), "vocabulary info")
        self.k, self.L, self.scoring, self.weighting, self.n_nodes, self.n_words = (int(v) for v in info)

    def nodes(self):
        """(parent, n_children, desc [n, 32], weight) of nodes 1..n, and word_node [words]: each word id's node id."""
        n, m = max(self.n_nodes, 0), max(self.n_nodes, self.n_words, 1)
        parent, nch = np.zeros(m, np.int32), np.zeros(m, np.int32)
        desc, weight, word_node = np.zeros((m, 32), np.uint8), np.zeros(m, np.float64), np.zeros(m, np.int32)
        _check(lib().ref_voc_nodes(self._h, _p(parent), _p(nch), _p(desc), _p(weight), _p(word_node), m), "vocabulary nodes")
        return parent[:n], nch[:n], desc[:n], weight[:n], word_node[:self.n_words]

    def transform(self, feats, levelsup=4, feature_vector=True, feat_word=True):
        """-> dict of bow_word, bow_value, and (feature_vector) fv_node, fv_feat, (feat_word) feat_word."""
        f = np.ascontiguousarray(feats, np.uint8).reshape(-1, 32)
        n = len(f)
        m = max(n, 1)
        bw, bv, bn = np.zeros(m, np.uint32), np.zeros(m, np.float64), ctypes.c_int32(0)
        fn, ff, fvn = np.zeros(m, np.uint32), np.zeros(m, np.uint32), ctypes.c_int32(0)
        fw = np.zeros(m, np.uint32)
        _check(lib().ref_transform(self._h, _p(f), n, int(levelsup), _p(bw), _p(bv), ctypes.byref(bn),
                                   _p(fn) if feature_vector else None, _p(ff) if feature_vector else None,
                                   ctypes.byref(fvn) if feature_vector else None, _p(fw) if feat_word else None, m), "transform")
        out = dict(bow_word=bw[:bn.value], bow_value=bv[:bn.value])
        if feature_vector:
            out.update(fv_node=fn[:fvn.value], fv_feat=ff[:fvn.value])
        if feat_word:
            out["feat_word"] = fw[:n]
        return out

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ref_voc_free(self._h)
            self._h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def score(scoring, w1, v1, w2, v2) -> float:
    """ScoringObject::score of the scoring type (0 L1, 1 L2, 2 chi-square, 3 KL, 4 Bhattacharyya, 5 dot product)."""
    w1, w2 = np.ascontiguousarray(w1, np.uint32), np.ascontiguousarray(w2, np.uint32)
    v1, v2 = np.ascontiguousarray(v1, np.float64), np.ascontiguousarray(v2, np.float64)
    out = np.zeros(1, np.float64)
    _check(lib().ref_score(int(scoring), _p(w1), _p(v1), len(w1), _p(w2), _p(v2), len(w2), _p(out)), "score")
    return float(out[0])


def pos_in_grid(kps, bounds):
    """Frame::PosInGrid per keypoint -> (pos [n, 2] int32, ok [n] bool)."""
    k = np.ascontiguousarray(kps, KP)
    b = np.ascontiguousarray(bounds, np.int32)
    pos, ok = np.zeros((max(len(k), 1), 2), np.int32), np.zeros(max(len(k), 1), np.int32)
    _check(lib().ref_pos_in_grid(_p(k), len(k), _p(b), _p(pos), _p(ok)), "PosInGrid")
    return pos[:len(k)], ok[:len(k)].astype(bool)


def features_in_area(kps, bounds, x, y, r, min_level=-1, max_level=-1):
    """Frame::GetFeaturesInArea on a frame of these (undistorted) keypoints -> int32 indices in the reference's order."""
    k = np.ascontiguousarray(kps, KP)
    b = np.ascontiguousarray(bounds, np.int32)
    out = np.zeros(max(len(k), 1), np.int32)
    n = _check(lib().ref_features_in_area(_p(k), len(k), _p(b), float(x), float(y), float(r), int(min_level), int(max_level), _p(out),
                                          len(out)), "GetFeaturesInArea")
    return out[:n].copy()


def match_init(k1, d1, k2, d2, bounds, window=100, nnratio=0.9, check_ori=True):
    """ORBmatcher(nnratio, check_ori).SearchForInitialization(F1, F2, vnMatches12, window) -> (nmatches, matches12, stats[3]),
    stats being the three counters the call prints; both frames share `bounds` (Frame's statics)."""
    k1, k2 = np.ascontiguousarray(k1, KP), np.ascontiguousarray(k2, KP)
    d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
    b = np.ascontiguousarray(bounds, np.int32)
    m = np.full(max(len(k1), 1), -1, np.int32)
    nm, st = np.zeros(1, np.int32), np.zeros(3, np.int32)
    _check(lib().ref_match_init(_p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), _p(b), int(window), float(nnratio), int(check_ori),
                                _p(m), _p(nm), _p(st)), "SearchForInitialization")
    return int(nm[0]), m[:len(k1)].copy(), st


# ---- bag-of-words helpers shared by tests/test_ref_pins.py (CPU) and tests/test_gpu_ref_pins.py --------------------------

def write_for_reference(path, voc, **kw):
    """The vocabulary as a text file the reference loads with defined behaviour: no trailing newline (deviation 1: a trailing empty
    line becomes a node with an uninitialised descriptor) and at most the k^(L+1) nodes the loader reserves (beyond them m_nodes
    reallocates under the m_words pointers into it).  k >= 2: k < 2 divides by zero in that reservation."""
    k, L = voc.header[:2]
    assert k >= 2 and len(voc.parent) + 1 <= (k ** (L + 1) - 1) // (k - 1)
    R.write_text(path, voc, trailing_newline=False, **kw)


def end_depths(voc, feats):
    """The depth of the node each feature's descent ends at (DBoW2's descent: smallest distance, first child on a tie, until a
    node without children)."""
    n = len(voc.parent)
    children = [[] for _ in range(n + 1)]
    depth = np.zeros(n + 1, np.int64)
    for i in range(n):
        children[int(voc.parent[i])].append(i + 1)
        depth[i + 1] = depth[int(voc.parent[i])] + 1
    bits = np.unpackbits(voc.desc, axis=1)
    out = []
    for f in np.unpackbits(np.asarray(feats, np.uint8).reshape(-1, 32), axis=1):
        cur = 0
        while children[cur]:
            ch = children[cur]
            cur = ch[int(np.argmin((bits[np.array(ch) - 1] != f).sum(axis=1)))]
        out.append(int(depth[cur]))
    return np.array(out, np.int64)


def same_transform(ref, mine, what, skip_fv_feats=()):
    assert np.array_equal(ref["bow_word"], mine["bow_word"]), what
    assert ref["bow_value"].tobytes() == np.asarray(mine["bow_value"], np.float64).tobytes(), what
    assert np.array_equal(ref["feat_word"], mine["feat_word"]), what
    keep_r = ~np.isin(ref["fv_feat"], list(skip_fv_feats))
    keep_m = ~np.isin(mine["fv_feat"], list(skip_fv_feats))
    assert np.array_equal(ref["fv_node"][keep_r], mine["fv_node"][keep_m]), what
    assert np.array_equal(ref["fv_feat"][keep_r], mine["fv_feat"][keep_m]), what


def shallow_features(voc, feats, levelsup):
    """Deviation 2: a feature whose descent ends above depth L - levelsup leaves the reference's nid unset (UB), so its
    FeatureVector entry is not compared; its BowVector contribution is."""
    nid_level = voc.header[1] - levelsup
    if nid_level <= 0:
        return ()
    return tuple(np.nonzero(end_depths(voc, feats) < nid_level)[0].tolist())



# ---- matcher fixtures shared by tests/test_ref_pins.py (CPU) and tests/test_gpu_ref_pins.py ---------------------------------

def golden_pairs(golden, widths):
    """(name, k1, d1, k2, d2, bounds) for the frame pairs of tests/golden/golden.npz, both presets; widths: image name -> width."""
    out = []
    for key in sorted(golden):
        if not key.endswith("/matches12"):
            continue
        preset, pair, _ = key.split("/")
        a, b = pair.split("-")
        out.append(("%s/%s" % (preset, pair), golden["%s/%s/kps" % (preset, a)], golden["%s/%s/desc" % (preset, a)],
                    golden["%s/%s/kps" % (preset, b)], golden["%s/%s/desc" % (preset, b)], (0, int(widths[b]), 0, 480)))
    return out


def _flip_bits(rng, d, max_flips):
    for i in range(len(d)):
        for bit in rng.integers(0, 256, int(rng.integers(0, max_flips + 1))):
            d[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    return d


def contention_pair(rng, n, n_protos, flips, w, h, level0_share, jitter):
    """The clustered pairs of tests/test_gpu_parity.py's contention cases: frame A from few prototypes with flipped bits (many
    near-duplicates), frame B a jittered permutation of most of A with more flipped bits, other octaves and angles."""
    protos = rng.integers(0, 256, (n_protos, 32), dtype=np.uint8)
    k1 = np.zeros(n, KP)
    k1["x"] = rng.uniform(0, w - 1, n).astype(np.float32)
    k1["y"] = rng.uniform(0, h - 1, n).astype(np.float32)
    k1["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k1["octave"] = np.where(rng.uniform(0, 1, n) < level0_share, 0, rng.integers(1, 8, n))
    d1 = _flip_bits(rng, protos[rng.integers(0, n_protos, n)].copy(), flips)
    perm = rng.permutation(n)[:n - 7]
    k2 = k1[perm].copy()
    k2["x"] = np.clip(k2["x"] + rng.uniform(-jitter, jitter, len(perm)), 0, w - 1).astype(np.float32)
    k2["y"] = np.clip(k2["y"] + rng.uniform(-jitter, jitter, len(perm)), 0, h - 1).astype(np.float32)
    k2["angle"] = ((k2["angle"] + 20 + rng.choice([0, 0, 0, 0, 90, 200], len(perm)) + rng.uniform(-3, 3, len(perm))) % 360)
    k2["octave"] = np.where(rng.uniform(0, 1, len(perm)) < 0.9, k2["octave"], rng.integers(0, 3, len(perm)))
    d2 = _flip_bits(rng, d1[perm].copy(), flips)
    return k1, d1, k2, d2


def contention_cases():
    """(name, k1, d1, k2, d2, bounds, window, nnratio, check_ori): a few of test_gpu_parity.py's contention shapes, smaller."""
    rng = np.random.default_rng(17)
    out = []
    for (n, npro, flips, win, w, h, share, ratio, ori) in ((1500, 1500, 20, 300, 1920, 1080, 0.7, 0.9, True),
                                                           (1800, 150, 8, 4096, 1920, 1080, 0.9, 0.9, True),
                                                           (1200, 400, 10, 60, 752, 480, 0.9, 0.9, True),
                                                           (1000, 1000, 25, 4096, 1280, 720, 0.9, 0.6, False)):
        k1, d1, k2, d2 = contention_pair(rng, n, npro, flips, w, h, share, min(win, 300) / 3)
        out.append(("contention-%d-%d-%d" % (n, npro, win), k1, d1, k2, d2, (0, w, 0, h), win, ratio, ori))
    return out


def edge_cases():
    """(name, k1, d1, k2, d2, bounds, window, nnratio, check_ori): test_gpu_parity.py's match edge cases -- empty frames,
    keypoints in the grid's last cells, the stolen match in a pruned bin, colliding descriptors."""
    out = []
    e = np.zeros(0, KP), np.zeros((0, 32), np.uint8)
    k = np.zeros(5, KP)
    k["x"], k["y"] = [10, 630, 320, 639.6, 0.2], [10, 470, 240, 479.7, 0.1]
    d = np.arange(5 * 32, dtype=np.uint8).reshape(5, 32)
    b = (0, 640, 0, 480)
    out += [("empty-f5", e[0], e[1], k, d, b, 100, 0.9, True), ("f5-empty", k, d, e[0], e[1], b, 100, 0.9, True),
            ("f5-f5", k, d, k, d, b, 100, 0.9, True)]
    rng = np.random.default_rng(11)
    k1, k2 = np.zeros(40, KP), np.zeros(40, KP)
    k1["x"], k1["y"] = rng.integers(50, 590, 40), rng.integers(50, 430, 40)
    k2["x"], k2["y"] = k1["x"], k1["y"]
    k1["angle"] = rng.integers(0, 360, 40)
    k2["angle"] = (k1["angle"] + rng.choice([0, 0, 0, 90, 200], 40)) % 360
    d1 = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    d2 = d1.copy()
    d2[5] = d2[6]
    d1[7] = d1[8]
    out += [("stolen-%d" % win, k1, d1, k2, d2, b, win, 0.9, True) for win in (30, 100, 700)]
    return out


def fuzz_case(seed):
    """A small random frame pair built to sit on the matcher's edges: keypoints on grid-cell and bound edges (and outside the
    bounds), a few octaves including -1, angle differences on the rotation histogram's bin edges and wrap, duplicated
    descriptors and descriptors at equal distances, windows and ratios of several sizes, bounds not starting at 0."""
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.choice([64, 130, 640, 752])), int(rng.choice([48, 97, 480]))
    x0, y0 = int(rng.choice([0, 0, -7, 5])), int(rng.choice([0, 0, 3, -2]))
    bounds = (x0, x0 + w, y0, y0 + h)
    n1, n2 = int(rng.integers(0, 50)), int(rng.integers(0, 50))

    def keys(n):
        k = np.zeros(n, KP)
        cw, ch = np.float32(w) / np.float32(64), np.float32(h) / np.float32(48)
        kind = rng.integers(0, 4, n)
        gx = (x0 + rng.integers(0, 65, n) * cw + rng.choice([0.0, -0.5, 0.5, 0.25], n) * cw).astype(np.float32)
        gy = (y0 + rng.integers(0, 49, n) * ch + rng.choice([0.0, -0.5, 0.5, 0.25], n) * ch).astype(np.float32)
        ex = np.array([x0, x0 + w, x0 + w - 1, np.nextafter(np.float32(x0 + w), np.float32(0)), x0 - 1], np.float32)
        ey = np.array([y0, y0 + h, y0 + h - 1, np.nextafter(np.float32(y0 + h), np.float32(0)), y0 - 1], np.float32)
        k["x"] = np.where(kind == 0, rng.uniform(x0, x0 + w, n), np.where(kind == 1, gx, ex[rng.integers(0, 5, n)]))
        k["y"] = np.where(kind == 0, rng.uniform(y0, y0 + h, n), np.where(kind == 2, gy, ey[rng.integers(0, 5, n)]))
        k["octave"] = rng.choice([0, 0, 0, 0, 1, 2, -1], n)
        k["angle"] = rng.choice([0.0, 6.0, 18.0, 354.0, 359.99], n) + rng.integers(0, 30, n) * 12.0
        k["angle"] = np.where(rng.random(n) < 0.3, rng.uniform(0, 360, n), k["angle"] % 360).astype(np.float32)
        return k

    def descs(n, base):
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        if len(base):
            take = rng.random(n) < 0.7
            d[take] = _flip_bits(rng, base[rng.integers(0, len(base), int(take.sum()))].copy(), 6)
        if n > 2:
            d[rng.integers(0, n, n // 4)] = d[rng.integers(0, n, n // 4)]  # duplicates: equal distances
        return d

    k1, k2 = keys(n1), keys(n2)
    protos = rng.integers(0, 256, (int(rng.integers(1, 6)), 32), dtype=np.uint8)
    d1, d2 = descs(n1, protos), descs(n2, protos)
    window = int(rng.choice([1, 5, 13, 40, 100, 1000]))
    ratio = float(rng.choice([0.6, 0.75, 0.9, 1.0]))
    return ("fuzz-%d" % seed, k1, d1, k2, d2, bounds, window, ratio, bool(rng.random() < 0.8))
