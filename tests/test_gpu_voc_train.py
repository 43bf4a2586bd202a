"""DBoW2's TemplatedVocabulary::create on the device (orbx_vocabulary_train): every case equals the recursive CPU restatement
(tests/cpp/voc_train_ref.cpp) byte for byte -- parents, leaf flags, descriptors, the bytes of every weight, the statistics and each
training feature's word -- and the reference's compiled DBoW2 loads and transforms with what the device trained."""
import contextlib
import functools
import os
import subprocess

import numpy as np
import pytest

import bow_ref_lib as R
import ref_lib
import voc_train_ref_lib as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


def _same(v, tr, what=""):
    parent, leaf, desc, weight = v.nodes()
    assert np.array_equal(parent, tr.parent), what
    assert np.array_equal(leaf, tr.is_leaf), what
    assert np.array_equal(desc, tr.desc), what
    assert weight.tobytes() == tr.weight.tobytes(), what
    assert v.train_stats == tr.stats, (what, v.train_stats, tr.stats)
    assert (v.n_nodes, v.n_words) == (tr.stats["nodes"], tr.stats["words"]), what
    if v.train_feat_word is not None:
        assert np.array_equal(v.train_feat_word, tr.feat_word), what


@pytest.mark.parametrize("weighting", range(4))
def test_golden_frames_equal_the_restatement(orbx, ext, golden, weighting):
    v = orbx.Vocabulary.train(ext, T.golden_docs(golden), T.GOLDEN_K, T.GOLDEN_L, weighting, 0, T.GOLDEN_SEED, feat_word=True)
    _same(v, T.golden_trained(weighting))
    v.close()


def test_edge_sweep_equals_the_restatement(orbx, ext):
    for i in range(T.SWEEP):
        docs, k, L, seed = T.sweep_case(i)
        v = orbx.Vocabulary.train(ext, docs, k, L, i % 4, i % 6, seed, feat_word=True)
        _same(v, T.train(docs, k, L, i % 4, seed), "set %d" % i)
        v.close()


def test_round_limit_equals_the_restatement(orbx, ext):
    docs, k, L, seed = T.sweep_case(0)
    for max_rounds in (1, 2, 3):
        v = orbx.Vocabulary.train(ext, docs, k, L, 0, 0, seed, max_rounds=max_rounds, feat_word=True)
        assert v.train_stats["capped_runs"] >= 1
        _same(v, T.train(docs, k, L, 0, seed, max_rounds), "max_rounds %d" % max_rounds)
        v.close()


def test_grid_wide_seeding_equals_the_one_workgroup_form(orbx, ext):
    """About 600 features in three documents: with the switch at 64 features the root and the larger nodes of the next level are
    seeded by the grid-wide kernels (several blocks each), the rest by one workgroup; both equal the restatement."""
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (12, 32), dtype=np.uint8)
    d = R._flip(rng, base[rng.integers(0, 12, 613)], 3)
    docs = [d[:200], d[200:201], d[201:]]
    tr = T.train(docs, 5, 4, 0, 99)
    plain = orbx.Vocabulary.train(ext, docs, 5, 4, 0, 0, 99, feat_word=True)
    orbx.lib().orbx_debug_voc_train_seed_grid_min(64)
    try:
        grid = orbx.Vocabulary.train(ext, docs, 5, 4, 0, 0, 99, feat_word=True)
    finally:
        orbx.lib().orbx_debug_voc_train_seed_grid_min(-1)
    _same(plain, tr, "one workgroup")
    _same(grid, tr, "grid-wide")
    for a, b in zip(plain.nodes(), grid.nodes()):
        assert a.tobytes() == b.tobytes()
    plain.close()
    grid.close()


def test_larger_nodes_take_the_chunked_paths(orbx, ext):
    """20,000 features: the root is above the one-workgroup seeding's limit and has several count chunks (global counters)."""
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    d = R._flip(rng, base[rng.integers(0, 40, 20000)], 2)
    docs = [d[:7000], d[7000:7001], d[7001:]]
    v = orbx.Vocabulary.train(ext, docs, 6, 2, 0, 0, 3, feat_word=True)
    _same(v, T.train(docs, 6, 2, 0, 3))
    v.close()


@contextlib.contextmanager
def _seed_grid_min(orbx, value):
    """Inside the block, nodes above `value` features are seeded grid-wide (None: the default).  The switch is process-wide."""
    if value is None:
        yield
        return
    orbx.lib().orbx_debug_voc_train_seed_grid_min(value)
    try:
        yield
    finally:
        orbx.lib().orbx_debug_voc_train_seed_grid_min(-1)


@pytest.mark.parametrize("name", T.SIZE_CASES)
def test_size_case_equals_the_restatement(orbx, ext, name, tmp_path):
    """The inputs at which the kernels change paths (voc_train_ref_lib.size_case; tests/test_voc_train_host.py asserts that each
    reaches its path).  root_above_65536 also runs in the device form, and the reference's compiled transform of its training
    features through the saved file gives the device's words."""
    for c, tr in zip(T.size_case(name), T.size_trained(name)):
        with _seed_grid_min(orbx, c.grid_min):
            v = orbx.Vocabulary.train(ext, c.docs, c.k, c.L, c.weighting, 0, c.seed, feat_word=True)
        _same(v, tr, "%s %s" % (name, c.label))
        if name == "root_above_65536":
            import torch
            desc, n = np.stack(c.docs), np.full(len(c.docs), T.MAX_DOC, np.int32)
            assert desc.shape == (5, T.MAX_DOC, 32)
            d_desc, d_n = torch.from_numpy(desc).cuda(), torch.from_numpy(n).cuda()
            d_fw = torch.zeros((len(c.docs), T.MAX_DOC), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            d = orbx.Vocabulary.train(ext, None, c.k, c.L, c.weighting, 0, c.seed, d_desc=d_desc, d_n=d_n, n_docs=len(c.docs),
                                      capacity=T.MAX_DOC, d_feat_word=d_fw)
            _same(d, tr, "device form")
            assert np.array_equal(d_fw.cpu().numpy().view(np.uint32).reshape(-1), tr.feat_word)
            d.close()
            path = str(tmp_path / "device.txt")
            v.save_text(path, exact=True)
            text = open(path).read()
            assert text.endswith("\n")
            open(path, "w").write(text[:-1])  # (as in test_device_against_the_reference)
            rv = ref_lib.Vocabulary(path)
            off = 0
            for doc in c.docs:
                assert np.array_equal(rv.transform(doc, 4, feature_vector=False)["feat_word"], v.train_feat_word[off:off + len(doc)])
                off += len(doc)
            rv.close()
        v.close()


@functools.lru_cache(maxsize=None)
def _seed_input(which):
    """(docs, k, L, seed, grid_min) of test_seeds_equal_the_numpy_statement."""
    if which in ("300", "300_grid_wide"):
        rng = np.random.default_rng(300)
        base = rng.integers(0, 256, (12, 32), dtype=np.uint8)
        return [R._flip(rng, base[rng.integers(0, 12, 300)], 3)], 5, 1, 17, 0 if which == "300_grid_wide" else None
    name, label, L = {"4097": ("edges_of_4096", "4097", 1), "65537": ("edge_of_65536", "65537", 1),
                      "81920": ("root_above_65536", "81920", 1), "short": ("short_seeding_large", "5000", 1), "two_levels": ("root_above_65536", "81920", 2)}[which]
    c = [x for x in T.size_case(name) if x.label == label][0]
    return c.docs, c.k, L, c.seed, c.grid_min


@pytest.mark.parametrize("which", ["300", "300_grid_wide", "4097", "65537", "81920", "short", "two_levels"])
def test_seeds_equal_the_numpy_statement(orbx, ext, which):
    """A training stopped after its first round leaves the seeds as the children's descriptors.  They equal, in count and bytes,
    what voc_train_ref_lib.seeds_numpy -- written from the text of include/orbx.h, not from the restatement -- picks: by one
    workgroup (300), grid-wide (300 under the switch, 4097), with one and with two block sums per thread of k_vt_seed_pick (65537,
    81920), stopping short grid-wide (three distinct descriptors), and on the second level under every node's own key."""
    docs, k, L, seed, grid_min = _seed_input(which)
    feats = T.case_feats(docs)
    parent, desc = T.seeded_tree_numpy(feats, k, L, seed)
    with _seed_grid_min(orbx, grid_min):
        v = orbx.Vocabulary.train(ext, docs, k, L, 0, 0, seed, max_rounds=1)
    mine = v.nodes()
    assert v.n_nodes == len(parent) and np.array_equal(mine[0], parent) and np.array_equal(mine[2], desc)
    assert v.train_stats["capped_runs"] == v.train_stats["kmeans_runs"] >= 1 and v.train_stats["max_rounds_seen"] == 1
    if which == "short":
        assert len(parent) == 3 and v.train_stats["short_seedings"] == 1
    if which == "two_levels":
        assert len(parent) == k + k * k
    v.close()


@functools.lru_cache(maxsize=None)
def _sweep_trained(i):
    docs, k, L, seed = T.sweep_case(i)
    return T.train(docs, k, L, i % 4, seed)


@pytest.mark.parametrize("grid_min", [0, 16])
def test_edge_sweep_under_grid_wide_seeding(orbx, ext, grid_min):
    """The edge sweep with every k-means node (0), or every one above 16 features (a mixed level), seeded by the grid-wide
    kernels: down to n = k + 1, and with the seedings that stop short in k_vt_seed_pick."""
    short = 0
    with _seed_grid_min(orbx, grid_min):
        for i in range(T.SWEEP):
            docs, k, L, seed = T.sweep_case(i)
            v = orbx.Vocabulary.train(ext, docs, k, L, i % 4, i % 6, seed, feat_word=True)
            _same(v, _sweep_trained(i), "set %d" % i)
            short += _sweep_trained(i).stats["short_seedings"]
            v.close()
    assert short >= 1


def test_round_limit_in_a_chunked_node(orbx, ext):
    """5,000 features in one node (two count chunks, global counters): stopped after 1, 2 and 3 rounds."""
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (20, 32), dtype=np.uint8)
    docs = [R._flip(rng, base[rng.integers(0, 20, 5000)], 3)]
    assert len(docs[0]) > T.VT_CHUNK and T.train(docs, 6, 1, 0, 7).stats["max_rounds_seen"] > 3
    for max_rounds in (1, 2, 3):
        tr = T.train(docs, 6, 1, 0, 7, max_rounds)
        assert tr.stats["capped_runs"] == 1
        v = orbx.Vocabulary.train(ext, docs, 6, 1, 0, 0, 7, max_rounds=max_rounds, feat_word=True)
        _same(v, tr, "max_rounds %d" % max_rounds)
        v.close()


def test_trained_vocabulary_transforms_like_its_nodes(orbx, ext, golden):
    docs = T.golden_docs(golden)
    v = orbx.Vocabulary.train(ext, docs, T.GOLDEN_K, T.GOLDEN_L, 0, 0, T.GOLDEN_SEED)
    w = orbx.Vocabulary.from_arrays(ext, v.k, v.L, v.scoring, v.weighting, *v.nodes())
    for d in docs:
        for x, y in zip(v.transform(d, 2, feat_word=True), w.transform(d, 2, feat_word=True)):
            assert x.tobytes() == y.tobytes()
    a, b = v.transform(docs[0]), v.transform(docs[1])
    assert v.score(a.bow_word, a.bow_value, b.bow_word, b.bow_value) == w.score(a.bow_word, a.bow_value, b.bow_word, b.bow_value)
    v.close()
    w.close()


def test_device_against_the_reference(orbx, ext, golden, tmp_path):
    """save_text -> the reference's loadFromTextFile: the same nodes; its transform of the training frames gives the device's
    words.  (The file's trailing newline is cut: the reference reads it as one more node, bag-of-words deviation 1.)"""
    docs = T.golden_docs(golden)
    v = orbx.Vocabulary.train(ext, docs, T.GOLDEN_K, T.GOLDEN_L, 2, 0, T.GOLDEN_SEED, feat_word=True)
    path = str(tmp_path / "device.txt")
    v.save_text(path, exact=True)
    text = open(path).read()
    assert text.endswith("\n")
    open(path, "w").write(text[:-1])
    rv = ref_lib.Vocabulary(path)
    parent, nch, desc, weight, word_node = rv.nodes()
    mine = v.nodes()
    assert np.array_equal(parent, mine[0]) and np.array_equal(nch == 0, mine[1] == 1) and np.array_equal(desc, mine[2])
    assert weight.tobytes() == mine[3].tobytes()
    off = 0
    for d in docs:
        assert np.array_equal(rv.transform(d, 4, feature_vector=False)["feat_word"], v.train_feat_word[off:off + len(d)])
        off += len(d)
    rv.close()
    v.close()


def test_device_form_equals_host_form(orbx, ext, golden):
    import torch
    docs = T.golden_docs(golden)
    cap = max(len(d) for d in docs) + 5
    desc = np.zeros((len(docs), cap, 32), np.uint8)
    for f, d in enumerate(docs):
        desc[f, :len(d)] = d
    n = np.array([len(d) for d in docs], np.int32)
    n_in = n.copy()
    n_in[3] = cap + 100  # clamped to the capacity: slots beyond the document hold zeros, features like any other
    docs2 = [desc[f, :min(int(n_in[f]), cap)] for f in range(len(docs))]
    d_desc, d_n = torch.from_numpy(desc).cuda(), torch.from_numpy(n_in).cuda()
    d_fw = torch.zeros((len(docs), cap), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    v = orbx.Vocabulary.train(ext, None, 10, 3, 0, 0, 5, d_desc=d_desc, d_n=d_n, n_docs=len(docs), capacity=cap, d_feat_word=d_fw)
    h = orbx.Vocabulary.train(ext, docs2, 10, 3, 0, 0, 5, feat_word=True)
    for a, b in zip(v.nodes(), h.nodes()):
        assert a.tobytes() == b.tobytes()
    assert v.train_stats == h.train_stats
    fw = d_fw.cpu().numpy().view(np.uint32)
    assert np.array_equal(np.concatenate([fw[f, :len(docs2[f])] for f in range(len(docs))]), h.train_feat_word)
    v.close()
    h.close()


def test_no_features_gives_an_empty_vocabulary(orbx, ext):
    for docs in ([], [np.zeros((0, 32), np.uint8)] * 3):
        v = orbx.Vocabulary.train(ext, docs, 10, 3, 0, 0, 1, feat_word=True)
        assert (v.n_nodes, v.n_words) == (0, 0) and all(x == 0 for x in v.train_stats.values())
        assert len(v.transform(np.zeros((5, 32), np.uint8)).bow_word) == 0
        v.close()
    one = orbx.Vocabulary.train(ext, [np.full((1, 32), 7, np.uint8)], 10, 3, 2, 0, 1, feat_word=True)
    _same(one, T.train([np.full((1, 32), 7, np.uint8)], 10, 3, 2, 1))  # one feature: the trivial root, one word
    one.close()


def test_get_nodes_and_text_round_trip(orbx, ext, tmp_path):
    tree = R.irregular_tree(5, k=4, L=5, n_nodes=300, scoring=0, weighting=0)
    v = orbx.Vocabulary.from_arrays(ext, *tree.arrays())
    for a, b in zip(v.nodes(), tree.arrays()[4:]):
        assert a.tobytes() == b.tobytes()
    exact, short, want = (str(tmp_path / n) for n in ("exact.txt", "short.txt", "want.txt"))
    v.save_text(exact, exact=True)
    hdr, parent, leaf, desc, weight = orbx.Vocabulary.parse_text(exact)
    assert tuple(hdr) == tree.header
    for a, b in zip((parent, leaf, desc, weight), tree.arrays()[4:]):
        assert a.tobytes() == b.tobytes()
    v.save_text(short, exact=False)
    R.write_text(want, tree, exact=False)
    assert open(short).read() == open(want).read()
    v.close()


def test_shim_voc_train_compiles_and_runs(orbx, tmp_path):
    exe = os.path.join(str(tmp_path), "shim_voc_train")
    libdir = os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DORBX_WITH_OPENCV", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "tests", "cpp", "mock_opencv"), os.path.join(ROOT, "tests", "cpp", "shim_voc_train.cpp"), "-L", libdir,
           "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    out = str(tmp_path / "shim_voc.txt")
    p = subprocess.run([exe, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    assert "shim_voc_train ok" in p.stdout
    hdr, parent, leaf, desc, weight = orbx.Vocabulary.parse_text(out)
    assert tuple(hdr[:2]) == (4, 3) and len(parent) > 4
