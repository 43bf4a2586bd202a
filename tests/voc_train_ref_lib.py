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


def mean_value(group):
    """FORB::meanValue of the rows of group [m, 32]."""
    if len(group) == 1:
        return group[0].copy()
    bits = np.unpackbits(group, axis=1).sum(axis=0)
    n2 = len(group) // 2 + len(group) % 2
    return np.packbits((bits >= n2).astype(np.uint8))
