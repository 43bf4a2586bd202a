"""ctypes wrapper around tests/cpp/bow_ref.cpp -- the CPU restatement of DBoW2's text loader, transform and L1 score -- compiled
on first use with g++ -O2 -ffp-contract=off into a private temporary directory, and the deterministic vocabulary fixtures of the
bag-of-words tests (nothing is downloaded or read from elsewhere).  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bow_ref.cpp")
_L = None


def lib() -> ctypes.CDLL:
    global _L
    if _L is not None:
        return _L
    d = tempfile.mkdtemp(prefix="bow_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libbow_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", SRC, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("bow_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.br_voc_create.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.br_voc_create.restype = vp
    L.br_voc_free.argtypes = [vp]
    L.br_voc_free.restype = None
    L.br_transform.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.br_transform.restype = None
    L.br_score_l1.argtypes = [i32, vp, vp, i32, vp, vp]
    L.br_score_l1.restype = ctypes.c_double
    L.br_parse_text.argtypes = [ctypes.c_char_p, vp, vp, vp, vp, vp]
    _L = L
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


class Voc:
    """A vocabulary in the restatement: nodes 1..n in file order (parent, is_leaf, desc [n, 32], weight)."""

    def __init__(self, k, L, scoring, weighting, parent, is_leaf, desc, weight):
        self.header = (int(k), int(L), int(scoring), int(weighting))
        self.parent = np.ascontiguousarray(parent, np.int32)
        self.is_leaf = np.ascontiguousarray(is_leaf, np.int32)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.weight = np.ascontiguousarray(weight, np.float64)
        n = len(self.parent)
        self._h = lib().br_voc_create(*self.header, n, _p(self.parent), _p(self.is_leaf), _p(self.desc), _p(self.weight))

    def with_types(self, scoring, weighting) -> "Voc":
        return Voc(self.header[0], self.header[1], scoring, weighting, self.parent, self.is_leaf, self.desc, self.weight)

    def arrays(self):
        return self.header + (self.parent, self.is_leaf, self.desc, self.weight)

    def transform(self, feats, levelsup=4):
        """-> dict of bow_word, bow_value, fv_node, fv_feat, feat_word (numpy arrays)."""
        f = np.ascontiguousarray(feats, np.uint8).reshape(-1, 32)
        n = len(f)
        m = max(n, 1)
        bw, bv = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fn, ff, fw = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        bn, fvn = ctypes.c_int32(0), ctypes.c_int32(0)
        lib().br_transform(self._h, _p(f), n, int(levelsup), _p(bw), _p(bv), ctypes.byref(bn), _p(fn), _p(ff), ctypes.byref(fvn), _p(fw))
        return dict(bow_word=bw[:bn.value], bow_value=bv[:bn.value], fv_node=fn[:fvn.value], fv_feat=ff[:fvn.value], feat_word=fw[:n])

    def __del__(self):
        try:
            if self._h:
                lib().br_voc_free(self._h)
        except Exception:
            pass


def score_l1(w1, v1, w2, v2) -> float:
    w1, w2 = np.ascontiguousarray(w1, np.uint32), np.ascontiguousarray(w2, np.uint32)
    v1, v2 = np.ascontiguousarray(v1, np.float64), np.ascontiguousarray(v2, np.float64)
    return lib().br_score_l1(len(w1), _p(w1), _p(v1), len(w2), _p(w2), _p(v2))


def parse_text(path):
    """The restatement's loader: (header, parent, is_leaf, desc, weight), or None for a header outside the reference's ranges."""
    n = lib().br_parse_text(os.fsencode(path), None, None, None, None, None)
    if n < 0:
        return None
    m = max(n, 1)
    hdr, parent, leaf = np.zeros(4, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
    desc, weight = np.zeros((m, 32), np.uint8), np.zeros(m, np.float64)
    lib().br_parse_text(os.fsencode(path), _p(hdr), _p(parent), _p(leaf), _p(desc), _p(weight))
    return hdr, parent[:n], leaf[:n], desc[:n], weight[:n]


def write_text(path, voc: Voc, trailing_newline=True, exact=True, header_line=None):
    """saveToTextFile's format (:1626-1645): "k L  scoring weighting", then "parent flag d0 .. d31 weight" per node.  exact: the
    weights with 17 significant digits (round trip); else as an ostream writes a double by default (6 significant digits)."""
    k, L, sc, wt = voc.header
    lines = [header_line if header_line is not None else "%d %d  %d %d" % (k, L, sc, wt)]
    for i in range(len(voc.parent)):
        w = voc.weight[i]
        ws = repr(float(w)) if exact else "%g" % w
        lines.append("%d %d %s %s" % (voc.parent[i], voc.is_leaf[i], " ".join(str(int(b)) for b in voc.desc[i]), ws))
    text = "\n".join(lines) + ("\n" if trailing_newline else "")
    with open(path, "w") as f:
        f.write(text)


# ---- fixtures ------------------------------------------------------------------------------------------------------------

def _flip(rng, parent_desc, ands):
    """The parent's descriptors with random bits flipped, each with probability 2^-ands."""
    m = rng.integers(0, 256, parent_desc.shape, dtype=np.uint8)
    for _ in range(ands - 1):
        m &= rng.integers(0, 256, parent_desc.shape, dtype=np.uint8)
    return parent_desc ^ m


def full_vocabulary(seed_desc, k=10, L=6, seed=1, scoring=0, weighting=0) -> Voc:
    """A full k^L-leaf tree as DBoW2's create lays it out (each node's children numbered together, depth first): the root's
    children are descriptors from real frames, every child is its parent with random bit flips (fewer the deeper), leaves flagged 1
    with IDF-like f64 weights, some of them 0; inner nodes flagged 0 with weight 0."""
    rng = np.random.default_rng(seed)
    seed_desc = np.asarray(seed_desc, np.uint8).reshape(-1, 32)
    levels = [seed_desc[rng.choice(len(seed_desc), k, replace=False)]]  # breadth-first, level 1
    for d in range(2, L + 1):
        levels.append(_flip(rng, np.repeat(levels[-1], k, axis=0), ands=min(2 + d // 2, 5)))
    # number nodes as create does: the children of a node together, then recurse into each child in order
    n = sum(len(x) for x in levels)
    parent, leaf = np.zeros(n, np.int32), np.zeros(n, np.int32)
    desc, weight = np.zeros((n, 32), np.uint8), np.zeros(n, np.float64)
    nxt = 1
    stack = [(0, 0, 0)]  # (node id, depth, breadth-first index within its level)
    while stack:
        nid, depth, bi = stack.pop()
        if depth == L:
            continue
        ids = list(range(nxt, nxt + k))
        nxt += k
        lev = levels[depth]
        for j, cid in enumerate(ids):
            cb = bi * k + j
            parent[cid - 1] = nid
            desc[cid - 1] = lev[cb]
            if depth + 1 == L:
                leaf[cid - 1] = 1
        stack.extend((ids[j], depth + 1, bi * k + j) for j in reversed(range(k)))
    lv = leaf == 1
    w = np.log(rng.uniform(1.0, 3000.0, lv.sum()))
    w[rng.random(lv.sum()) < 0.03] = 0.0
    weight[lv] = w
    return Voc(k, L, scoring, weighting, parent, leaf, desc, weight)


def irregular_tree(seed, k=4, L=5, n_nodes=300, scoring=0, weighting=0) -> Voc:
    """1..k children per node, leaves at every depth, childless nodes flagged non-leaf, flagged leaves with children, sibling
    descriptors duplicated to force ties, weights with zeros and negatives."""
    rng = np.random.default_rng(seed)
    parent, depth, nch = [], [0], [0]
    desc = [rng.integers(0, 256, 32, dtype=np.uint8)]  # the root's (never read)
    while len(parent) < n_nodes:
        cand = [i for i in range(len(depth)) if depth[i] < L and nch[i] < k]
        if not cand:
            break
        p = int(cand[int(rng.integers(len(cand)))] if rng.random() < 0.7 else cand[0])
        nid = len(depth)
        parent.append(p)
        depth.append(depth[p] + 1)
        nch.append(0)
        nch[p] += 1
        sib = [i for i in range(1, nid) if parent[i - 1] == p]
        if sib and rng.random() < 0.2:
            desc.append(desc[sib[int(rng.integers(len(sib)))]].copy())
        else:
            desc.append(_flip(rng, desc[p], ands=2))
    n = len(parent)
    leaf = np.array([(1 if nch[i + 1] == 0 else 0) for i in range(n)], np.int32)
    flip = rng.random(n) < 0.15
    leaf[flip] = 1 - leaf[flip]  # childless nodes flagged 0, nodes with children flagged 1
    leaf[rng.random(n) < 0.05] = 2  # any flag > 0 is a leaf flag
    weight = rng.uniform(0.1, 5.0, n)
    weight[rng.random(n) < 0.1] = 0.0
    weight[rng.random(n) < 0.05] *= -1.0
    return Voc(k, L, scoring, weighting, np.array(parent, np.int32), leaf, np.array(desc[1:], np.uint8), weight)


def features_near(voc: Voc, n, seed, ands=3):
    """n descriptors near random nodes of the vocabulary (bit flips of theirs): they spread over many words with near-ties."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(voc.desc), n)
    return _flip(rng, voc.desc[pick], ands)
