"""The database without a GPU: the CPU restatement of add and query (tests/cpp/db_ref.cpp, the yardstick of tests/test_gpu_database.py)
against the reference's own compiled scoring objects (oracle/_ref/libref.so through tests/ref_lib.py), and the new C ABI's
exports, refusals and shim program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import db_ref_lib as D
import ref_lib as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_WORDS, N_ENTRIES, N_QUERIES = 60, 300, 40


def _norm(scoring):
    return {0: 1, 1: 2, 2: 1, 4: 1, 5: 0}[scoring]  # mustNormalize of the scoring objects: L2 for L2_NORM, none for DOT_PRODUCT


@pytest.fixture(scope="module")
def filled():
    """scoring -> (restatement database of 300 entries, the entries, 40 queries): a 60-word vocabulary, vectors of 0-24 words with
    exact duplicates; a quarter of the queries are entries themselves."""
    F.lib()  # fails (does not skip) when oracle/_ref/libref.so is missing
    out = {}
    for scoring in D.SCORINGS:
        rng = np.random.default_rng(100 + scoring)
        entries = D.random_vectors(rng, N_ENTRIES, N_WORDS, norm=_norm(scoring))
        queries = D.random_vectors(rng, N_QUERIES, N_WORDS, norm=_norm(scoring))
        for i in range(0, N_QUERIES, 4):
            queries[i] = entries[int(rng.integers(0, N_ENTRIES))]
        db = D.Database(N_WORDS, scoring)
        for i, (w, v) in enumerate(entries):
            assert db.add(w, v) == i
        assert db.size == N_ENTRIES
        out[scoring] = (db, entries, queries)
    return out


def _common(a, b):
    return len(np.intersect1d(a[0], b[0]))


@pytest.mark.parametrize("scoring", D.SCORINGS)
def test_restatement_equals_reference_scoring_objects(filled, scoring):
    db, entries, queries = filled[scoring]
    compared = 0
    for q in queries:
        e, s = db.query(q[0], q[1], max_results=N_ENTRIES)
        listed = sorted(i for i in range(N_ENTRIES) if _common(q, entries[i]) >= D.MIN_COMMON[scoring])
        assert sorted(e.tolist()) == listed  # exactly the listed set, every entry once
        for i, sc in zip(e, s):
            want = F.score(scoring, q[0], q[1], entries[i][0], entries[i][1])
            assert np.float64(want).tobytes() == np.float64(sc).tobytes(), (scoring, int(i), want, sc)
            compared += 1
        assert np.all(s[:-1] >= s[1:])  # best first: every scoring object's score is the larger the better
        assert compared > 0 or not len(q[0])
    assert compared > N_QUERIES  # (the lists are not empty: something was compared)


@pytest.mark.parametrize("scoring", D.SCORINGS)
def test_max_results_and_max_id(filled, scoring):
    db, entries, queries = filled[scoring]
    ties = 0
    for q in queries:
        full_e, full_s = db.query(q[0], q[1], max_results=N_ENTRIES)
        e5, s5 = db.query(q[0], q[1], max_results=5)
        assert len(e5) == min(5, len(full_e))
        assert sorted(s5.tolist()) == sorted(full_s[:len(s5)].tolist())  # the best five as a multiset
        for a in range(len(full_e) - 1):
            if full_s[a] == full_s[a + 1] and _tied(scoring, full_s[a]):
                assert full_e[a] < full_e[a + 1]  # deviation 1: equal sums in ascending entry id
                ties += 1
        for max_id in (0, 1, 150, -1):
            e, s = db.query(q[0], q[1], max_results=N_ENTRIES, max_id=max_id)
            keep = full_e < max_id if max_id != -1 else np.ones(len(full_e), bool)
            assert np.array_equal(e, full_e[keep]) and s.tobytes() == full_s[keep].tobytes()
    assert ties > 0  # (the duplicates make ties)


def _tied(scoring, score):
    """Equal final scores of two neighbours mean equal SUMS, but for L2_NORM's clamp: every sum <= -1.0 scores 1.0."""
    return scoring != 1 or score != 1.0


def test_binary_weighting_dot_product_counts_common_words():
    rng = np.random.default_rng(7)
    entries = D.random_vectors(rng, 80, N_WORDS, norm=0)
    db = D.Database(N_WORDS, 5, binary=True)
    for w, v in entries:
        db.add(w, v)
    for q in D.random_vectors(rng, 10, N_WORDS, norm=0):
        e, s = db.query(q[0], q[1], max_results=80)
        for i, sc in zip(e, s):
            assert sc == float(_common(q, entries[i])) and sc >= 1.0
        assert np.all(s[:-1] >= s[1:])


def test_restatement_inverted_file_rows_ascend(filled):
    db, entries, _ = filled[0]
    rs, pe, pv = db.inverted_file()
    assert rs[0] == 0 and rs[-1] == len(pe) == sum(len(w) for w, _ in entries)
    for w in range(N_WORDS):
        row = pe[rs[w]:rs[w + 1]]
        assert np.all(np.diff(row.astype(np.int64)) > 0)
        for ent, val in zip(row, pv[rs[w]:rs[w + 1]]):
            ew, ev = entries[ent]
            assert ev[list(ew).index(w)] == val


# ---- the C ABI without a device ------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("orbx_database_create", "orbx_database_destroy", "orbx_database_clear", "orbx_database_size",
               "orbx_database_add_batch_device", "orbx_database_query_batch_device", "orbx_database_add", "orbx_database_query",
               "orbx_database_get_inverted_file", "orbx_debug_database_shape")


def test_database_symbols_exported_and_bound(orbx):
    L = ctypes.CDLL(orbx.lib_path())
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
    assert orbx.DB_MAX_RESULTS >= 128
    for m in ("add", "add_batch_device", "query", "query_batch_device", "size", "clear", "inverted_file", "close"):
        assert hasattr(orbx.Database, m), m


def test_database_refusals_without_a_context(orbx):
    """ctx == NULL with otherwise well-formed arguments is ORBX_E_HIP (no device, never a host computation); null pointers,
    negative counts and capacity < 1 are ORBX_E_BADARG, a capacity above ORBX_BOW_MAX_FEATURES ORBX_E_CAPACITY, whatever the
    context.  A handle is not looked into before the context is known to exist, so a placeholder stands for it here."""
    L = orbx.lib()
    h = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))  # a non-null handle (never dereferenced)
    w, v, n = np.zeros(8, np.uint32), np.zeros(8), np.zeros(1, np.int32)
    e, s, rn, first = np.zeros(4, np.int32), np.zeros(4), np.zeros(1, np.int32), ctypes.c_int32(0)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert L.orbx_database_create(None, fake, ctypes.byref(h)) == orbx.E_HIP and not h.value
    assert L.orbx_database_create(None, None, ctypes.byref(h)) == orbx.E_BADARG
    assert L.orbx_database_create(None, fake, None) == orbx.E_BADARG
    add = L.orbx_database_add_batch_device
    assert add(None, fake, 1, p(w), p(v), p(n), 8, ctypes.byref(first)) == orbx.E_HIP
    assert add(None, None, 1, p(w), p(v), p(n), 8, ctypes.byref(first)) == orbx.E_BADARG
    assert add(None, fake, -1, p(w), p(v), p(n), 8, ctypes.byref(first)) == orbx.E_BADARG
    assert add(None, fake, 1, None, p(v), p(n), 8, ctypes.byref(first)) == orbx.E_BADARG
    assert add(None, fake, 1, p(w), p(v), p(n), 0, ctypes.byref(first)) == orbx.E_BADARG
    assert add(None, fake, 1, p(w), p(v), p(n), 8, None) == orbx.E_BADARG
    assert add(None, fake, 1, p(w), p(v), p(n), orbx.BOW_MAX_FEATURES + 1, ctypes.byref(first)) == orbx.E_CAPACITY
    qry = L.orbx_database_query_batch_device
    assert qry(None, fake, 1, p(w), p(v), p(n), 8, 4, -1, p(e), p(s), p(rn)) == orbx.E_HIP
    assert qry(None, None, 1, p(w), p(v), p(n), 8, 4, -1, p(e), p(s), p(rn)) == orbx.E_BADARG
    assert qry(None, fake, -1, p(w), p(v), p(n), 8, 4, -1, p(e), p(s), p(rn)) == orbx.E_BADARG
    assert qry(None, fake, 1, p(w), p(v), None, 8, 4, -1, p(e), p(s), p(rn)) == orbx.E_BADARG
    assert qry(None, fake, 1, p(w), p(v), p(n), 0, 4, -1, p(e), p(s), p(rn)) == orbx.E_BADARG
    assert qry(None, fake, 1, p(w), p(v), p(n), 8, 4, -1, p(e), None, p(rn)) == orbx.E_BADARG
    assert qry(None, fake, 1, p(w), p(v), p(n), orbx.BOW_MAX_FEATURES + 1, 4, -1, p(e), p(s), p(rn)) == orbx.E_CAPACITY
    assert L.orbx_database_add(None, fake, p(w), p(v), 8, ctypes.byref(first)) == orbx.E_HIP
    assert L.orbx_database_add(None, None, p(w), p(v), 8, ctypes.byref(first)) == orbx.E_BADARG
    assert L.orbx_database_add(None, fake, p(w), p(v), 8, None) == orbx.E_BADARG
    assert L.orbx_database_query(None, fake, p(w), p(v), 8, 4, -1, p(e), p(s), p(rn)) == orbx.E_HIP
    assert L.orbx_database_query(None, fake, p(w), p(v), 8, 4, -1, None, p(s), p(rn)) == orbx.E_BADARG
    assert L.orbx_database_size(None) == orbx.E_BADARG and L.orbx_database_clear(None) == orbx.E_BADARG
    assert L.orbx_database_get_inverted_file(None, None, None, None, 0) == orbx.E_BADARG
    L.orbx_database_destroy(None)


def test_debug_database_shape_range(orbx):
    L = orbx.lib()
    try:
        for eps, lpm, want in ((32, 2, 0), (1, 8, 0), (2048, 2, 0), (0, 2, orbx.E_BADARG), (2049, 2, orbx.E_BADARG),
                               (32, 1, orbx.E_BADARG), (32, 9, orbx.E_BADARG), (32, 0, orbx.E_BADARG), (-1, -1, 0)):
            assert L.orbx_debug_database_shape(eps, lpm) == want, (eps, lpm)
    finally:
        orbx.debug_database_shape()


def test_database_source_allocates_only_through_the_buffer_types():
    """orbx_db.cpp, like orbx_api.cpp and orbx_bow.cpp: device memory through csrc/orbx_buf.h's owning types only."""
    import re
    src = open(os.path.join(ROOT, "orb_slam_tracking_amd", "csrc", "orbx_db.cpp"), errors="replace").read()
    assert not re.findall(r"\bhip(?:Host)?(?:Malloc|Free)\b", src)
    assert "DeviceBuf<" in src


def test_shim_database_compiles(orbx, tmp_path):
    exe = os.path.join(str(tmp_path), "shim_database")
    libdir = os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "shim_database.cpp"), "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
