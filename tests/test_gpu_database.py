"""The database on the device (orbx_database_*): the inverted file after every add and every query result equal the CPU restatement
(tests/cpp/db_ref.cpp) bit for bit -- entries, scores, counts and order -- and every returned score equals the reference's own
compiled ScoringObject::score for that pair (oracle/_ref/libref.so, tests/ref_lib.py)."""
import numpy as np
import pytest

import bow_ref_lib as R
import db_ref_lib as D
import ref_lib as F

pytestmark = pytest.mark.gpu

CAP = 1024
N_ENTRIES, N_UNSEEN = 96, 8
N_FRAMES = N_ENTRIES + N_UNSEEN + 1          # the entries, 8 unseen frames, an empty one: all of them are queries
COUNTS = (1000, 0, 1, 3, 40, 150)            # features per frame, in turn
BATCHES = (1, 7, 24, 64)                     # the adds: rows that already hold postings, an empty frame inside a batch
DUPLICATES = ((48, 18), (95, 5))             # frame 48 is frame 18 again (1000 features), frame 95 frame 5 (150)
SLICE = 2048                                 # the default entries_per_slice (orbx.DB_ENTRIES_PER_SLICE)
# (vocabulary, scoring, weighting): the five scorings on both vocabularies, and DOT_PRODUCT under BINARY weighting (term 1)
WORLDS = [(kind, s, 0) for kind in ("irregular", "full1000") for s in D.SCORINGS] + [("irregular", 5, 3)]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ext(orbx):
    F.lib()  # fails (does not skip) when oracle/_ref/libref.so is missing
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def base_vocs(golden):
    return {"irregular": R.irregular_tree(3, k=4, L=5, n_nodes=300),
            "full1000": R.full_vocabulary(golden["canonical/dbow0/desc"], k=10, L=3)}


def _frames(voc, seed):
    """[N_FRAMES, CAP, 32] descriptors near the vocabulary's nodes and their counts."""
    d, n = np.zeros((N_FRAMES, CAP, 32), np.uint8), np.zeros(N_FRAMES, np.int32)
    for f in range(N_FRAMES - 1):
        n[f] = COUNTS[f % len(COUNTS)]
        d[f, :n[f]] = R.features_near(voc, int(n[f]), seed + f)
    for f, g in DUPLICATES:
        d[f], n[f] = d[g], n[g]
    return d, n                                 # (the last frame stays empty)


class World:
    """One vocabulary with its types on the device, the BowVectors of N_FRAMES frames transformed there (device tensors and host
    copies), the device database and the restatement's, both filled with the first N_ENTRIES frames in BATCHES; what each add
    left behind is kept for the tests."""

    def __init__(self, orbx, torch, ext, base, scoring, weighting):
        self.scoring = scoring
        self.base = base.with_types(scoring, weighting)
        self.voc = orbx.Vocabulary.from_arrays(ext, *self.base.arrays())
        d, n = _frames(self.base, 500)
        z = lambda dt, m: torch.zeros(m, dtype=dt, device="cuda")  # noqa: E731
        self.d_word, self.d_value, self.d_n = z(torch.int32, N_FRAMES * CAP), z(torch.float64, N_FRAMES * CAP), z(torch.int32, N_FRAMES)
        self.voc.transform_batch_device(N_FRAMES, torch.from_numpy(d).cuda(), torch.from_numpy(n).cuda(), self.d_word, self.d_value,
                                        self.d_n, capacity=CAP)
        torch.cuda.synchronize()
        hn = self.d_n.cpu().numpy()
        hw = self.d_word.cpu().numpy().view(np.uint32).reshape(N_FRAMES, CAP)
        hv = self.d_value.cpu().numpy().reshape(N_FRAMES, CAP)
        self.vec = [(hw[f, :hn[f]].copy(), hv[f, :hn[f]].copy()) for f in range(N_FRAMES)]
        self.ref = D.Database(self.voc.n_words, scoring, binary=weighting == 3)
        self.db = orbx.Database(self.voc)
        self.after_add = []
        self.fill(self.db, self.ref, self.after_add)

    def rows(self, f0, nb):
        return self.d_word[f0 * CAP:(f0 + nb) * CAP], self.d_value[f0 * CAP:(f0 + nb) * CAP], self.d_n[f0:f0 + nb]

    def fill(self, db, ref, log=None):
        f0 = 0
        for nb in BATCHES:
            first = db.add_batch_device(nb, *self.rows(f0, nb), capacity=CAP)
            ids = [ref.add(*self.vec[f]) for f in range(f0, f0 + nb)] if ref is not None else None
            if log is not None:
                log.append((first, ids, db.size, ref.size, db.inverted_file(), ref.inverted_file()))
            f0 += nb
        assert f0 == N_ENTRIES

    def close(self):
        self.db.close()
        self.voc.close()


@pytest.fixture(scope="module")
def worlds(orbx, torch, ext, base_vocs):
    made = {}

    def get(kind, scoring, weighting):
        key = (kind, scoring, weighting)
        if key not in made:
            made[key] = World(orbx, torch, ext, base_vocs[kind], scoring, weighting)
        return made[key]
    yield get
    orbx.debug_database_shape()
    for w in made.values():
        w.close()


def _same_file(got, want):
    assert np.array_equal(got[0], want[0]), "row lengths differ"
    assert np.array_equal(got[1], want[1]), "entry ids differ"
    assert got[2].tobytes() == want[2].tobytes(), "values differ"


def _query_batch(torch, w, db, nq, max_results, max_id):
    """All nq first frames in one call -> (entry [nq, R], score [nq, R], n [nq]) as numpy."""
    e = torch.full((nq * max_results,), -7, dtype=torch.int32, device="cuda")
    s = torch.full((nq * max_results,), -7.0, dtype=torch.float64, device="cuda")
    n = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    db.query_batch_device(nq, *w.rows(0, nq), e, s, n, max_results=max_results, max_id=max_id, capacity=CAP)
    torch.cuda.synchronize()
    return e.cpu().numpy().reshape(nq, max_results), s.cpu().numpy().reshape(nq, max_results), n.cpu().numpy()


@pytest.mark.parametrize("kind,scoring,weighting", WORLDS)
def test_inverted_file_after_every_add(worlds, kind, scoring, weighting):
    w = worlds(kind, scoring, weighting)
    f0 = 0
    for nb, (first, ids, size, ref_size, got, want) in zip(BATCHES, w.after_add):
        assert first == f0 and ids == list(range(f0, f0 + nb)) and size == ref_size == f0 + nb
        _same_file(got, want)
        for r in range(len(got[0]) - 1):  # (the restatement's rows ascend by construction: so do these)
            assert np.all(np.diff(got[1][got[0][r]:got[0][r + 1]].astype(np.int64)) > 0)
        f0 += nb
    assert len(w.vec[1][0]) == 0 and len(w.vec[0][0]) > 20  # an empty vector got an id; a large frame holds many words
    assert got[0][-1] == len(got[1]) > 1000  # (the file is not small: rows of many postings were moved and extended)
    for f, g in DUPLICATES:
        assert np.array_equal(w.vec[f][0], w.vec[g][0]) and w.vec[f][1].tobytes() == w.vec[g][1].tobytes()


@pytest.mark.parametrize("kind,scoring,weighting", WORLDS)
def test_queries_equal_restatement_and_reference(orbx, torch, worlds, kind, scoring, weighting):
    """Default shape and orbx_debug_database_shape(32, 2) (three slices, two merge rounds over 96 entries); every frame as a
    query, in one batch and one by one; max_results 1, 4, 128 and max_id -1, 0, 33, 96."""
    w = worlds(kind, scoring, weighting)
    # the restatement's whole list once per (query, max_id); a cut list is its head (the final score is applied per entry)
    want = {mid: [w.ref.query(*w.vec[f], max_results=0, max_id=mid) for f in range(N_FRAMES)] for mid in (-1, 0, 33, 96)}
    for f in range(N_FRAMES):  # ... and the whole list directly against the reference's scoring objects
        e, s = want[-1][f]
        listed = [i for i in range(N_ENTRIES) if len(np.intersect1d(w.vec[f][0], w.vec[i][0])) >= D.MIN_COMMON[scoring]]
        assert sorted(e.tolist()) == listed
        if weighting != 3:  # (the reference's DotProductScoring::score has no BINARY form; its database's term 1 is restated)
            for i, sc in zip(e, s):
                ref = F.score(scoring, w.vec[f][0], w.vec[f][1], w.vec[i][0], w.vec[i][1])
                assert np.float64(ref).tobytes() == np.float64(sc).tobytes(), (f, int(i))
    try:
        for shape in ((32, 2), (-1, -1)):
            orbx.debug_database_shape(*shape)
            for max_results in (1, 4, 128):
                for max_id in (-1, 0, 33, 96):
                    be, bs, bn = _query_batch(torch, w, w.db, N_FRAMES, max_results, max_id)
                    for f in range(N_FRAMES):
                        we, ws = want[max_id][f]
                        we, ws = we[:max_results], ws[:max_results]
                        what = (shape, max_results, max_id, f)
                        assert bn[f] == len(we), what
                        assert np.array_equal(be[f, :bn[f]], we), what
                        assert bs[f, :bn[f]].tobytes() == ws.tobytes(), what
                        assert np.all(be[f, bn[f]:] == -7) and np.all(bs[f, bn[f]:] == -7.0), what  # nothing beyond the count
                        oe, os_ = w.db.query(*w.vec[f], max_results=max_results, max_id=max_id)  # one by one
                        assert np.array_equal(oe, we) and os_.tobytes() == ws.tobytes(), what
    finally:
        orbx.debug_database_shape()
    assert len(want[-1][0][0]) > 32 and len(want[-1][N_FRAMES - 1][0]) == 0  # long lists were cut; the empty query lists nothing


def test_more_entries_than_one_slice(orbx, torch, ext, worlds):
    """2 * 2048 + 3 = 4099 entries of 1-4 words through the device path in batches of 256 (the last of 3): the 64th and later
    frames of a batch, three slices of the default shape and their seams."""
    assert orbx.DB_ENTRIES_PER_SLICE == SLICE
    w = worlds("full1000", 0, 0)
    n_words, cap, total = w.voc.n_words, 4, 2 * SLICE + 3
    rng = np.random.default_rng(31)
    hw, hv, hn = np.zeros((total, cap), np.uint32), np.zeros((total, cap)), rng.integers(1, cap + 1, total).astype(np.int32)
    hn[[SLICE - 1, 7, total - 1]] = cap  # the three queries: four words each, so that every list below is cut
    for f in range(total):
        hw[f, :hn[f]] = np.sort(rng.choice(64, hn[f], replace=False)) * (n_words // 64)  # few distinct words: long rows
        v = rng.uniform(0.1, 1.0, hn[f])
        hv[f, :hn[f]] = v / v.sum()
    hw[SLICE], hv[SLICE], hn[SLICE] = hw[SLICE - 1], hv[SLICE - 1], hn[SLICE - 1]  # equal sums on both sides of a seam
    d_w, d_v, d_n = torch.from_numpy(hw.view(np.int32)).cuda(), torch.from_numpy(hv).cuda(), torch.from_numpy(hn).cuda()
    db, ref = orbx.Database(w.voc), D.Database(n_words, 0)
    for f0 in range(0, total, 256):
        nb = min(256, total - f0)
        assert db.add_batch_device(nb, d_w[f0:f0 + nb], d_v[f0:f0 + nb], d_n[f0:f0 + nb], capacity=cap) == f0
        for f in range(f0, f0 + nb):
            ref.add(hw[f, :hn[f]], hv[f, :hn[f]])
    assert db.size == ref.size == total
    _same_file(db.inverted_file(), ref.inverted_file())
    for f in (SLICE - 1, 7, total - 1):
        for max_results, max_id in ((128, -1), (orbx.DB_MAX_RESULTS, -1), (128, SLICE + 1), (3, 2 * SLICE)):
            e, s = db.query(hw[f, :hn[f]], hv[f, :hn[f]], max_results=max_results, max_id=max_id)
            we, ws = ref.query(hw[f, :hn[f]], hv[f, :hn[f]], max_results=max_results, max_id=max_id)
            assert len(we) == max_results  # (the rows are long: every list is cut)
            assert np.array_equal(e, we) and s.tobytes() == ws.tobytes(), (f, max_results, max_id)
    e, _ = db.query(hw[SLICE - 1, :hn[SLICE - 1]], hv[SLICE - 1, :hn[SLICE - 1]], max_results=2)
    assert e.tolist() == [SLICE - 1, SLICE]  # the tie across the seam, in ascending id
    db.close()


def test_clear_then_add_again(orbx, torch, worlds):
    w = worlds("irregular", 0, 0)
    db = orbx.Database(w.voc)
    w.fill(db, None)
    db.clear()
    assert db.size == 0 and len(db.inverted_file()[1]) == 0
    e, s, n = _query_batch(torch, w, db, N_FRAMES, 4, -1)
    assert np.all(n == 0)
    assert db.add_batch_device(3, *w.rows(40, 3), capacity=CAP) == 0  # ids restart at 0
    db.clear()
    w.fill(db, None)
    _same_file(db.inverted_file(), w.db.inverted_file())
    a, b = _query_batch(torch, w, db, N_FRAMES, 4, -1), _query_batch(torch, w, w.db, N_FRAMES, 4, -1)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    db.close()


def test_same_batch_twice_is_byte_identical(torch, worlds):
    w = worlds("full1000", 1, 0)
    a, b = _query_batch(torch, w, w.db, N_FRAMES, 128, -1), _query_batch(torch, w, w.db, N_FRAMES, 128, -1)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    e, s, n = a
    assert n.max() <= N_ENTRIES < 128
    for f in range(N_FRAMES):
        assert np.all(e[f, n[f]:] == -7) and np.all(s[f, n[f]:] == -7.0)  # the sentinels beyond the count


def test_refusals_launch_nothing(orbx, torch, ext, base_vocs, worlds):
    w = worlds("irregular", 0, 0)
    kl = orbx.Vocabulary.from_arrays(ext, *base_vocs["irregular"].with_types(3, 0).arrays())
    with pytest.raises(orbx.OrbxError) as err:
        orbx.Database(kl)
    assert err.value.code == orbx.E_BADARG
    kl.close()
    e = torch.full((4 * (orbx.DB_MAX_RESULTS + 1),), -7, dtype=torch.int32, device="cuda")
    s = torch.full((4 * (orbx.DB_MAX_RESULTS + 1),), -7.0, dtype=torch.float64, device="cuda")
    n = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    for max_results in (0, orbx.DB_MAX_RESULTS + 1):
        with pytest.raises(orbx.OrbxError) as err:
            w.db.query_batch_device(4, *w.rows(0, 4), e, s, n, max_results=max_results, capacity=CAP)
        assert err.value.code == orbx.E_CAPACITY
        with pytest.raises(orbx.OrbxError) as err:
            w.db.query(*w.vec[0], max_results=max_results)
        assert err.value.code == orbx.E_CAPACITY
    other = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    L = orbx.lib()
    first = np.zeros(1, np.int32)
    assert L.orbx_database_query_batch_device(other._h, w.db._h, 4, w.d_word.data_ptr(), w.d_value.data_ptr(), w.d_n.data_ptr(), CAP, 4,
                                              -1, e.data_ptr(), s.data_ptr(), n.data_ptr()) == orbx.E_BADARG
    assert L.orbx_database_add_batch_device(other._h, w.db._h, 4, w.d_word.data_ptr(), w.d_value.data_ptr(), w.d_n.data_ptr(), CAP,
                                            first.ctypes.data) == orbx.E_BADARG
    import ctypes
    h = ctypes.c_void_p(0)
    assert L.orbx_database_create(other._h, w.voc._h, ctypes.byref(h)) == orbx.E_BADARG and not h.value  # a vocabulary of another context
    other.close()
    with pytest.raises(ValueError):  # short buffers are refused by the binding
        w.db.query_batch_device(4, *w.rows(0, 4), e[:8], s, n, max_results=4, capacity=CAP)
    with pytest.raises(ValueError):
        w.db.query_batch_device(4, *w.rows(0, 3), e, s, n, max_results=4, capacity=CAP)
    with pytest.raises(ValueError):
        w.db.add_batch_device(4, *w.rows(0, 3), capacity=CAP)
    for bad_w in ([5, 5], [7, 3], [w.voc.n_words]):  # deviation 5: the host forms refuse what the reference indexes with
        with pytest.raises(orbx.OrbxError) as err:
            w.db.add(np.array(bad_w, np.uint32), np.ones(len(bad_w)))
        assert err.value.code == orbx.E_BADARG
        with pytest.raises(orbx.OrbxError) as err:
            w.db.query(np.array(bad_w, np.uint32), np.ones(len(bad_w)))
        assert err.value.code == orbx.E_BADARG
    torch.cuda.synchronize()
    assert w.db.size == N_ENTRIES
    assert np.all(e.cpu().numpy() == -7) and np.all(s.cpu().numpy() == -7.0) and np.all(n.cpu().numpy() == -7)
    _same_file(w.db.inverted_file(), w.ref.inverted_file())


def test_device_path_skips_a_word_id_that_is_no_word(orbx, torch, worlds):
    """Deviation 5 on the device path: a posting whose word id is not below the vocabulary's word count is skipped by add and by
    query, never indexed with."""
    w = worlds("irregular", 0, 0)
    nw = w.voc.n_words
    hw = np.array([[1, 3, nw, 0xffffffff], [2, 3, nw + 5, 0]], np.uint32)
    hv = np.array([[0.25, 0.25, 0.25, 0.25], [0.5, 0.25, 0.25, 0.0]])
    hn = np.array([4, 3], np.int32)
    d_w, d_v, d_n = torch.from_numpy(hw.view(np.int32)).cuda(), torch.from_numpy(hv).cuda(), torch.from_numpy(hn).cuda()
    db, ref = orbx.Database(w.voc), D.Database(nw, 0)
    assert db.add_batch_device(2, d_w, d_v, d_n, capacity=4) == 0
    ref.add(hw[0, :2], hv[0, :2])
    ref.add(hw[1, :2], hv[1, :2])
    _same_file(db.inverted_file(), ref.inverted_file())
    e = torch.full((2 * 4,), -7, dtype=torch.int32, device="cuda")
    s = torch.full((2 * 4,), -7.0, dtype=torch.float64, device="cuda")
    n = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    db.query_batch_device(2, d_w, d_v, d_n, e, s, n, max_results=4, capacity=4)
    torch.cuda.synchronize()
    for f in range(2):
        we, ws = ref.query(hw[f, :2], hv[f, :2], max_results=4)
        assert n[f].item() == len(we) and np.array_equal(e.cpu().numpy().reshape(2, 4)[f, :len(we)], we)
        assert s.cpu().numpy().reshape(2, 4)[f, :len(we)].tobytes() == ws.tobytes()
    db.close()


def test_shim_database_compiles_and_runs(orbx, base_vocs, tmp_path):
    """tests/cpp/shim_database.cpp, the reference's call sequence over include/orbx_shim.hpp's ORBDatabase: a frame added twice
    and its first half once, then queried -- the two copies tie at the top in ascending id, the half follows with the
    restatement's score."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = os.path.join(str(tmp_path), "shim_database"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
           os.path.join(root, "tests", "cpp", "shim_database.cpp"), "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    voc = base_vocs["full1000"]
    desc = R.features_near(voc, 400, 77)
    voc_path, desc_path = str(tmp_path / "voc.txt"), str(tmp_path / "desc.bin")
    R.write_text(voc_path, voc)
    desc.tofile(desc_path)
    p = subprocess.run([exe, voc_path, desc_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    lines = p.stdout.strip().splitlines()
    assert lines[0] == "RESULT 3 3"
    whole, half = voc.transform(desc, 0), voc.transform(desc[:200], 0)
    ref = D.Database(int((voc.is_leaf > 0).sum()), 0)
    for v in (whole, whole, half):
        ref.add(v["bow_word"], v["bow_value"])
    we, ws = ref.query(whole["bow_word"], whole["bow_value"], max_results=4)
    assert we.tolist() == [0, 1, 2]
    got = [ln.split() for ln in lines[1:]]
    assert [int(g[0]) for g in got] == we.tolist()
    assert np.array([float(g[1]) for g in got]).tobytes() == ws.tobytes()  # (%.17g round-trips an f64)


def test_vocabulary_of_several_scan_tiles(orbx, torch, ext, golden):
    """10,000 words: the row starts are scanned in ten tiles of 1,024 words, the last one partial; words in every tile, the first
    and the last word among them, added in three batches."""
    voc_ref = R.full_vocabulary(golden["canonical/dbow0/desc"], k=10, L=4)
    voc = orbx.Vocabulary.from_arrays(ext, *voc_ref.arrays())
    n_words, cap, total = voc.n_words, 32, 150
    assert n_words == 10000
    rng = np.random.default_rng(5)
    hw, hv, hn = np.zeros((total, cap), np.uint32), np.zeros((total, cap)), rng.integers(0, cap + 1, total).astype(np.int32)
    hn[[0, 60]] = cap
    for f in range(total):
        hw[f, :hn[f]] = np.sort(rng.choice(n_words, hn[f], replace=False))
        v = rng.uniform(0.1, 1.0, hn[f])
        hv[f, :hn[f]] = v / max(v.sum(), 1e-300)
    hw[0, 0], hw[0, cap - 1], hw[60, 0], hw[60, cap - 1] = 0, n_words - 1, 0, n_words - 1
    d_w, d_v, d_n = torch.from_numpy(hw.view(np.int32)).cuda(), torch.from_numpy(hv).cuda(), torch.from_numpy(hn).cuda()
    db, ref = orbx.Database(voc), D.Database(n_words, 0)
    for f0, nb in ((0, 1), (1, 49), (50, 100)):
        assert db.add_batch_device(nb, d_w[f0:f0 + nb], d_v[f0:f0 + nb], d_n[f0:f0 + nb], capacity=cap) == f0
        for f in range(f0, f0 + nb):
            ref.add(hw[f, :hn[f]], hv[f, :hn[f]])
        _same_file(db.inverted_file(), ref.inverted_file())
    for f in (0, 60, 99):
        e, s = db.query(hw[f, :hn[f]], hv[f, :hn[f]], max_results=16)
        we, ws = ref.query(hw[f, :hn[f]], hv[f, :hn[f]], max_results=16)
        assert len(we) > 0 and np.array_equal(e, we) and s.tobytes() == ws.tobytes()
    db.close()
    voc.close()
