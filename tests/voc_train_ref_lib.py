"""ctypes wrapper around tests/cpp/voc_train_ref.cpp -- the recursive CPU restatement of DBoW2's TemplatedVocabulary::create
with the three documented deviations (include/orbx.h, "training") -- compiled on first use with g++ -O2 -ffp-contract=off into a
private temporary directory, and the inputs the vocabulary-training tests share.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import collections
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "voc_train_ref.cpp")
STATS = ("nodes", "words", "kmeans_runs", "max_rounds_seen", "capped_runs", "emptied_clusters", "short_seedings", "trivial_nodes")
_L = None

Trained = collections.namedtuple("Trained", "parent is_leaf desc weight stats feat_node feat_word")
Trained.__doc__ = """create's result: nodes 1..n in id order (parent, is_leaf = no children, desc [n, 32], weight), stats (dict, STATS),
and per training feature the node of its final training group (feat_node) and the word its descent ends in (feat_word)."""


def lib() -> ctypes.CDLL:
    global _L
    if _L is not None:
        return _L
    d = tempfile.mkdtemp(prefix="voc_train_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libvoc_train_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", SRC, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("voc_train_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.vt_train.argtypes = [i32, i32, i32, ctypes.c_uint64, i32, i32, vp, vp]
    L.vt_get.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.vt_get.restype = None
    _L = L
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def train(docs, k, L, weighting=0, seed=0, max_rounds=100) -> Trained:
    arrs = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in docs]
    doc_n = np.array([len(a) for a in arrs] + [0], np.int32)
    cat = np.ascontiguousarray(np.concatenate(arrs + [np.zeros((1, 32), np.uint8)]))
    N = len(cat) - 1
    n = lib().vt_train(int(k), int(L), int(weighting), int(seed), int(max_rounds), len(arrs), _p(cat), _p(doc_n))
    m = max(n, 1)
    parent, leaf, desc, weight = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 32), np.uint8), np.zeros(m, np.float64)
    stats, fnode, fword = np.zeros(8, np.int32), np.zeros(N + 1, np.int32), np.zeros(N + 1, np.uint32)
    lib().vt_get(_p(parent), _p(leaf), _p(desc), _p(weight), _p(stats), _p(fnode), _p(fword))
    return Trained(parent[:n], leaf[:n], desc[:n], weight[:n], dict(zip(STATS, (int(x) for x in stats))), fnode[:N], fword[:N])


# ---- shared inputs -------------------------------------------------------------------------------------------------------

GOLDEN_K, GOLDEN_L, GOLDEN_SEED = 10, 3, 12345


def golden_docs(golden):
    """The eight descriptor sets of tests/golden/golden.npz as eight documents (9,993 features), in the file's order."""
    keys = ["canonical/%s/desc" % k for k in ("dbow0", "dbow1", "dbow2", "dbow3", "init0", "init1")] + \
           ["as_shipped/init0/desc", "as_shipped/init1/desc"]
    return [np.ascontiguousarray(golden[key], np.uint8).reshape(-1, 32) for key in keys]


@functools.lru_cache(maxsize=None)
def _golden_cached(weighting):
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    return train(golden_docs({k: z[k] for k in z.files}), GOLDEN_K, GOLDEN_L, weighting, GOLDEN_SEED)


def golden_trained(weighting=0) -> Trained:
    """The restatement's result on the golden input, computed once per weighting and shared (treat it as read-only)."""
    return _golden_cached(int(weighting))


def sweep_case(i):
    """Edge sweep, set i of 150: (docs, k, L, seed) -- 5 to 200 features in 1 to 4 documents, k 2-10, L 1-4, of three kinds: uniform
    random bytes; 1-5 distinct descriptors repeated; 4 bases with sparse bit flips."""
    rng = np.random.default_rng(7000 + i)
    n, k, L = int(rng.integers(5, 201)), int(rng.integers(2, 11)), int(rng.integers(1, 5))
    kind = i % 3
    if kind == 0:
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    elif kind == 1:
        base = rng.integers(0, 256, (int(rng.integers(1, 6)), 32), dtype=np.uint8)
        d = base[rng.integers(0, len(base), n)]
    else:
        base = rng.integers(0, 256, (4, 32), dtype=np.uint8)
        m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        for _ in range(4):
            m &= rng.integers(0, 256, (n, 32), dtype=np.uint8)
        d = base[rng.integers(0, 4, n)] ^ m
    cuts = np.sort(rng.integers(0, n + 1, int(rng.integers(0, 4))))
    docs = [np.ascontiguousarray(x) for x in np.split(d, cuts)]  # (documents may be empty)
    return docs, k, L, 100 + i


SWEEP = 150


def children_of(parent):
    """children[id] (ascending ids) for node ids 0..n from parent [n] of nodes 1..n."""
    ch = [[] for _ in range(len(parent) + 1)]
    for i, p in enumerate(parent):
        ch[int(p)].append(i + 1)
    return ch


def groups_of(tr, n_feat):
    """node id -> ascending features of its training group, from every feature's final node and the parents."""
    groups = {}
    par = np.concatenate([[0], tr.parent])  # parent of node id (root: itself)
    for f in range(n_feat):
        node = int(tr.feat_node[f])
        while True:
            groups.setdefault(node, []).append(f)
            if node == 0:
                break
            node = int(par[node])
    return groups


Split = collections.namedtuple("Split", "node level key group children")
Split.__doc__ = """A node that was split: its id (0: the root), the level of its children (1 for the root's), its key (deviation 1:
the root's is 0, child i of the node with key K has 21 K + i + 1), its group (ascending features, an array) and its children."""


def splits_of(tr, n_feat):
    """Every node of tr that has children, as a Split, in ascending id order (so a parent comes before its children)."""
    children, groups = children_of(tr.parent), groups_of(tr, n_feat)
    key, level, out = {0: 0}, {0: 1}, []
    for node, ch in enumerate(children):
        if not ch:
            continue
        out.append(Split(node, level[node], key[node], np.array(groups[node]), ch))
        for i, c in enumerate(ch):
            key[c], level[c] = 21 * key[node] + i + 1, level[node] + 1
    return out


# ---- the seeding, stated in numpy from include/orbx.h ("training", deviation 1) and initiateClustersKMpp (:846-925) -----------

_M64 = (1 << 64) - 1
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)


def _mix(z):  # the splitmix64 step
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw(seed, key, j):
    """Draw j of the node with this key: 31 bits."""
    return _mix((_mix((seed ^ _mix(key & _M64)) & _M64) + j) & _M64) >> 33


def seeds_numpy(feats, k, seed, key):
    """The indices into feats [n, 32] that k-means++ seeding picks for the node with this key, in order: k of them, or fewer where
    every feature coincides with a centre already chosen."""
    feats = np.asarray(feats, np.uint8).reshape(-1, 32)
    n, j = len(feats), 0
    picks = [int(draw(seed, key, j) / 2147483648.0 * n)]
    j += 1
    min_dist = POPCOUNT[feats ^ feats[picks[0]]].sum(axis=1)
    while len(picks) < k:
        d = POPCOUNT[feats ^ feats[picks[-1]]].sum(axis=1)
        min_dist = np.where((min_dist > 0) & (d < min_dist), d, min_dist)
        total = int(min_dist.sum())
        if total == 0:
            break
        cut = 0.0
        while cut == 0.0:
            cut = draw(seed, key, j) / 2147483647.0 * float(total)
            j += 1
        i = int(np.searchsorted(np.cumsum(min_dist).astype(np.float64), cut, side="left"))  # the first running sum >= the cut
        picks.append(min(i, n - 1))
    return picks


def seeded_tree_numpy(feats, k, L, seed):
    """(parent, desc) of the tree a training with max_rounds = 1 leaves, in create's numbering, from seeds_numpy alone: every
    k-means node's children are its seeds, a child's group the features nearest to it (the first among equals), a node of at most
    k features has one child per feature."""
    feats = np.asarray(feats, np.uint8).reshape(-1, 32)
    parent, desc = [], []

    def step(node, g, level, key):
        f = feats[g]
        if len(g) <= k:
            picks = list(range(len(g)))
            nearest = np.arange(len(g))
        else:
            picks = seeds_numpy(f, k, seed, key)
            nearest = np.argmin(POPCOUNT[f[:, None, :] ^ f[picks][None, :, :]].sum(axis=2), axis=1)
        first = len(parent) + 1
        for p in picks:
            parent.append(node)
            desc.append(f[p])
        for i in range(len(picks)):
            child = g[nearest == i]
            if level < L and len(child) > 1:
                step(first + i, child, level + 1, 21 * key + i + 1)

    if len(feats):
        step(0, np.arange(len(feats)), 1, 0)
    return np.array(parent, np.int32), np.array(desc, np.uint8).reshape(-1, 32)


# ---- inputs at the sizes where the device code changes paths -------------------------------------------------------------------

VT_THREADS, VT_CHUNK, VT_SEED_LDS, VT_KMAX = 256, 4096, 4096, 20  # csrc/orbx_device.h (test_voc_train_host.py pins them)
MAX_DOC = 16384  # ORBX_BOW_MAX_FEATURES: the largest document
TF_IDF, TF, IDF, BINARY = range(4)

Case = collections.namedtuple("Case", "label docs k L weighting seed grid_min")
Case.__doc__ = """One training input; grid_min is the value of orbx_debug_voc_train_seed_grid_min the device runs it under (None: the
default)."""

SIZE_CASES = ("root_above_65536", "edges_of_4096", "edges_of_256", "edge_of_65536", "emptied_in_chunks", "short_seeding_large",
              "wide_level", "k20", "deep", "many_documents")


def _around_bases(rng, n, n_bases, ands):
    import bow_ref_lib
    base = rng.integers(0, 256, (n_bases, 32), dtype=np.uint8)
    return bow_ref_lib._flip(rng, base[rng.integers(0, n_bases, n)], ands)


def _documents(d, size=MAX_DOC):
    return [np.ascontiguousarray(d[i:i + size]) for i in range(0, len(d), size)]


@functools.lru_cache(maxsize=None)
def size_case(name):
    """The Cases of one named input (treat them as read-only); the docstrings of test_size_cases_reach_their_paths and of
    DESIGN.md 4d say which path each drives."""
    rng = np.random.default_rng(9000 + SIZE_CASES.index(name))
    if name == "root_above_65536":
        return (Case("81920", _documents(_around_bases(rng, 5 * MAX_DOC, 30, 3)), 4, 2, IDF, 11, None),)
    if name == "edges_of_4096":
        return tuple(Case(str(n), [_around_bases(rng, n, 20, 3)], 6, 1, TF_IDF, 20 + n, None) for n in (4095, 4096, 4097))
    if name == "edges_of_256":
        return tuple(Case(str(n), [_around_bases(rng, n, 12, 3)], 5, 2, TF_IDF, 30 + n, 64) for n in (255, 256, 257, 512, 513))
    if name == "edge_of_65536":
        return tuple(Case(str(n), _documents(_around_bases(rng, n, 30, 3)), 3, 1, TF_IDF, 40 + n, None) for n in (65536, 65537))
    if name == "emptied_in_chunks":
        n = 5000
        base = rng.integers(0, 256, (4, 32), dtype=np.uint8)
        m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        for _ in range(4):
            m &= rng.integers(0, 256, (n, 32), dtype=np.uint8)
        return (Case("5000", [base[rng.integers(0, 4, n)] ^ m], 16, 1, TF_IDF, 51, None),)
    if name == "short_seeding_large":
        base = rng.integers(0, 256, (3, 32), dtype=np.uint8)
        return (Case("5000", [base[rng.integers(0, 3, 5000)]], 10, 3, TF_IDF, 61, None),)
    if name == "wide_level":
        d = rng.integers(0, 256, (12000, 32), dtype=np.uint8)
        return (Case("12000", [d[:5000], d[5000:]], 10, 4, TF_IDF, 71, None),)
    if name == "k20":
        return (Case("3000", [_around_bases(rng, 3000, 30, 6)], 20, 2, TF, 81, None),)
    if name == "deep":
        return (Case("3000", [rng.integers(0, 256, (3000, 32), dtype=np.uint8)], 2, 10, TF_IDF, 91, None),)
    if name == "many_documents":
        d = _around_bases(rng, 700 * 40, 50, 3)
        lens = rng.integers(0, 41, 700)
        lens[rng.integers(0, 700, 30)] = 0
        lens[:2] = (40, 0)
        docs = [np.ascontiguousarray(d[40 * i:40 * i + int(m)]) for i, m in enumerate(lens)]
        return tuple(Case(w, docs, 8, 3, wt, 101, None) for w, wt in (("idf", IDF), ("tf_idf", TF_IDF)))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def size_trained(name):
    """The restatement's results on size_case(name), in its order, computed once and shared (treat them as read-only)."""
    return tuple(train(c.docs, c.k, c.L, c.weighting, c.seed) for c in size_case(name))


def case_feats(docs):
    return np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in docs] + [np.zeros((0, 32), np.uint8)])


def mean_value(group):
    """FORB::meanValue of the rows of group [m, 32]."""
    if len(group) == 1:
        return group[0].copy()
    bits = np.unpackbits(group, axis=1).sum(axis=0)
    n2 = len(group) // 2 + len(group) % 2
    return np.packbits((bits >= n2).astype(np.uint8))
