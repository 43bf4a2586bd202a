"""ctypes wrapper around tests/cpp/db_ref.cpp -- the CPU restatement of the database's add and query (include/orbx.h, "database")
-- compiled on first use with g++ -O2 -ffp-contract=off into a private temporary directory, as tests/bow_ref_lib.py compiles its
source.  TEST INFRASTRUCTURE only."""
from __future__ import annotations

import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "db_ref.cpp")
MIN_COMMON = {0: 1, 1: 1, 2: 5, 4: 5, 5: 1}  # common words an entry needs to be listed, by scoring type
SCORINGS = (0, 1, 2, 4, 5)
_L = None


def lib() -> ctypes.CDLL:
    global _L
    if _L is not None:
        return _L
    d = tempfile.mkdtemp(prefix="db_ref_")
    atexit.register(shutil.rmtree, d, True)
    so = os.path.join(d, "libdb_ref.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", SRC, "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("db_ref.cpp does not compile:\n" + p.stdout)
    L = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.dr_create.argtypes = [i32, i32, i32]
    L.dr_create.restype = vp
    L.dr_free.argtypes = [vp]
    L.dr_free.restype = None
    L.dr_clear.argtypes = [vp]
    L.dr_clear.restype = None
    L.dr_size.argtypes = [vp]
    L.dr_add.argtypes = [vp, vp, vp, i32]
    L.dr_query.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.dr_inverted_file.argtypes = [vp, vp, vp, vp]
    L.dr_inverted_file.restype = ctypes.c_longlong
    _L = L
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _vec(word, value):
    w, v = np.ascontiguousarray(word, np.uint32).reshape(-1), np.ascontiguousarray(value, np.float64).reshape(-1)
    assert len(w) == len(v)
    return w, v


class Database:
    """The restatement's database over a vocabulary of n_words words with the scoring type (and BINARY weighting or not)."""

    def __init__(self, n_words, scoring, binary=False):
        self.n_words, self.scoring = int(n_words), int(scoring)
        self._h = lib().dr_create(self.n_words, self.scoring, 1 if binary else 0)

    @property
    def size(self):
        return lib().dr_size(self._h)

    def clear(self):
        lib().dr_clear(self._h)

    def add(self, word, value) -> int:
        w, v = _vec(word, value)
        assert not len(w) or (int(w.max()) < self.n_words and np.all(np.diff(w.astype(np.int64)) > 0))
        return lib().dr_add(self._h, _p(w), _p(v), len(w))

    def query(self, word, value, max_results=1, max_id=-1):
        """-> (entry int32 [m], score float64 [m]); max_results <= 0: the whole list."""
        w, v = _vec(word, value)
        assert not len(w) or int(w.max()) < self.n_words
        m = max(self.size if max_results <= 0 else max_results, 1)
        e, s = np.zeros(m, np.int32), np.zeros(m, np.float64)
        n = lib().dr_query(self._h, _p(w), _p(v), len(w), int(max_results), int(max_id), _p(e), _p(s))
        return e[:n].copy(), s[:n].copy()

    def inverted_file(self):
        """-> (row_start uint32 [words + 1], post_entry uint32, post_value float64)."""
        n = lib().dr_inverted_file(self._h, None, None, None)
        rs, pe, pv = np.zeros(self.n_words + 1, np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64)
        lib().dr_inverted_file(self._h, _p(rs), _p(pe), _p(pv))
        return rs, pe[:n], pv[:n]

    def __del__(self):
        try:
            if self._h:
                lib().dr_free(self._h)
        except Exception:
            pass


def random_vectors(rng, n, n_words, max_words=24, norm=1, n_dup=6):
    """n BowVectors of 0 .. max_words words with positive values (norm 1: L1-normalised, 2: L2-normalised, 0: as drawn, which is
    what the vocabulary does for the scoring types), some of them exact duplicates of earlier ones."""
    out = []
    for i in range(n):
        if i >= 10 and i % (n // n_dup) == 3:
            out.append(out[int(rng.integers(0, i))])
            continue
        k = int(rng.integers(0, max_words + 1))
        w = np.sort(rng.choice(n_words, k, replace=False)).astype(np.uint32)
        v = rng.uniform(0.05, 3.0, k)
        if norm and k:
            v = v / (np.abs(v).sum() if norm == 1 else np.sqrt((v * v).sum()))
        out.append((w, v.astype(np.float64)))
    return out
