"""Vocabulary training (orbx_vocabulary_train, include/orbx.h "training") without a device: the ABI's refusals, and the CPU
restatement the GPU tests compare against (tests/cpp/voc_train_ref.cpp) checked on its own -- against the reference's compiled
DBoW2 as far as oracle/_ref/libref.so reaches (its loader, its transform), against the fixed-point property of k-means stated
in numpy, and its k-means++ seeding against a numpy statement written from the header's text; and that the inputs of the size
edges (voc_train_ref_lib.size_case) reach the paths they are there for.  (save_text needs a vocabulary, which needs a device: its round trip is in
tests/test_gpu_voc_train.py.)"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import bow_ref_lib as R
import ref_lib
import voc_train_ref_lib as T


def test_abi_refusals_without_a_device(orbx):
    L = orbx.lib()
    d = np.zeros((4, 32), np.uint8)
    n = np.array([4], np.int32)
    stats = np.zeros(8, np.int32)
    h = ctypes.c_void_p(0)

    def host(k=10, L_=3, sc=0, wt=0, n_docs=1, desc=d, doc_n=n, out=ctypes.byref(h)):
        return L.orbx_vocabulary_train(None, k, L_, sc, wt, 1, 100, n_docs, desc.ctypes.data if desc is not None else None,
                                       doc_n.ctypes.data if doc_n is not None else None, out, stats.ctypes.data, None)

    def dev(k=10, L_=3, sc=0, wt=0, n_docs=1, cap=4, desc=1 << 20, dn=1 << 21, out=ctypes.byref(h)):
        return L.orbx_vocabulary_train_device(None, k, L_, sc, wt, 1, 100, n_docs, desc, dn, cap, out, stats.ctypes.data, None)

    for f in (host, dev):
        for bad in (dict(k=1), dict(k=21), dict(L_=0), dict(L_=11), dict(sc=-1), dict(sc=6), dict(wt=-1), dict(wt=4), dict(n_docs=-1),
                    dict(out=None)):
            assert f(**bad) == orbx.E_BADARG, (f.__name__, bad)
        assert f() == orbx.E_HIP and not h.value  # well-formed, but no context
    assert host(desc=None) == orbx.E_BADARG and host(doc_n=None) == orbx.E_BADARG
    assert host(doc_n=np.array([-1], np.int32)) == orbx.E_BADARG
    assert host(doc_n=np.array([orbx.BOW_MAX_FEATURES + 1], np.int32)) == orbx.E_CAPACITY
    assert dev(desc=None) == orbx.E_BADARG and dev(dn=None) == orbx.E_BADARG and dev(cap=0) == orbx.E_BADARG
    assert dev(cap=orbx.BOW_MAX_FEATURES + 1) == orbx.E_CAPACITY
    assert dev(n_docs=(1 << 30) // 4 + 1) == orbx.E_CAPACITY  # more slots than ORBX_VOC_TRAIN_MAX_SLOTS
    assert L.orbx_vocabulary_get_nodes(None, None, None, None, None, 0) == orbx.E_BADARG
    assert L.orbx_vocabulary_save_text(None, b"/nonexistent/x", 1) == orbx.E_BADARG


def _check_fixed_point(tr, docs, k, L):
    """For every node that was split and not stopped by the round limit: each child's descriptor is meanValue of its group (the
    trivial case: the feature itself, in order), and every feature's nearest child, the first among equals, is its group's."""
    feats = np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in docs] + [np.zeros((0, 32), np.uint8)])
    if len(feats) == 0:
        assert len(tr.parent) == 0
        return
    assert tr.stats["capped_runs"] == 0  # (no input of these tests runs into the limit of 100 rounds)
    children, groups = T.children_of(tr.parent), T.groups_of(tr, len(feats))
    seen_kmeans = seen_trivial = 0
    for node, ch in enumerate(children):
        if not ch:
            continue
        g = np.array(groups[node])
        if len(g) <= k:
            seen_trivial += 1
            assert len(ch) == len(g) and np.array_equal(tr.desc[np.array(ch) - 1], feats[g])
            assert all(groups[c] == [int(f)] for c, f in zip(ch, g))
            continue
        seen_kmeans += 1
        dist = T.POPCOUNT[feats[g][:, None, :] ^ tr.desc[np.array(ch) - 1][None, :, :]].sum(axis=2)  # (per byte, not per bit)
        nearest = np.array(ch)[np.argmin(dist, axis=1)]  # argmin: the first minimum
        for c in ch:
            mine = g[nearest == c]
            assert groups.get(c, []) == mine.tolist(), (node, c)
            if len(mine):
                assert np.array_equal(tr.desc[c - 1], T.mean_value(feats[mine])), (node, c)
    assert seen_kmeans == tr.stats["kmeans_runs"] and seen_trivial == tr.stats["trivial_nodes"]
    assert tr.stats["nodes"] == len(tr.parent) and tr.stats["words"] == int(tr.is_leaf.sum())


def test_restatement_against_the_reference_on_the_golden_frames(golden, tmp_path):
    docs = T.golden_docs(golden)
    assert sum(len(d) for d in docs) == 9993 and len(docs) == 8
    tr = T.golden_trained(2)  # IDF
    print("stats", tr.stats)
    assert tr.stats["nodes"] == 1110 and tr.stats["kmeans_runs"] == 111 and tr.stats["max_rounds_seen"] == 27
    assert (tr.stats["emptied_clusters"], tr.stats["short_seedings"], tr.stats["trivial_nodes"], tr.stats["capped_runs"]) == (0, 0, 0, 0)
    path = str(tmp_path / "trained.txt")
    ref_lib.write_for_reference(path, R.Voc(T.GOLDEN_K, T.GOLDEN_L, 0, 2, tr.parent, tr.is_leaf, tr.desc, tr.weight))
    rv = ref_lib.Vocabulary(path)
    parent, nch, desc, weight, word_node = rv.nodes()
    assert (rv.k, rv.L, rv.n_nodes, rv.n_words) == (T.GOLDEN_K, T.GOLDEN_L, len(tr.parent), int(tr.is_leaf.sum()))
    assert np.array_equal(parent, tr.parent) and np.array_equal(nch == 0, tr.is_leaf == 1) and np.array_equal(desc, tr.desc)
    assert weight.tobytes() == tr.weight.tobytes()
    assert np.array_equal(word_node, np.nonzero(tr.is_leaf)[0] + 1)  # createWords: word ids in node-id order
    # the reference's transform of every training feature ends in the leaf of its training group, except where a trivial node
    # holds duplicate descriptors (the first of them wins the descent); and its words give the IDF weights
    children = T.children_of(tr.parent)
    Ni = np.zeros(rv.n_words, np.int64)
    off = excluded = 0
    for d in docs:
        fw = rv.transform(d, 4, feature_vector=False)["feat_word"]
        assert np.array_equal(fw, tr.feat_word[off:off + len(d)])
        for i in range(len(d)):
            node = int(tr.feat_node[off + i])
            sib = children[int(tr.parent[node - 1])]
            if sum(np.array_equal(tr.desc[s - 1], tr.desc[node - 1]) for s in sib) > 1:
                excluded += 1
            else:
                assert int(word_node[fw[i]]) == node
        Ni[np.unique(fw)] += 1
        off += len(d)
    assert excluded == 0
    rv.close()
    words = np.nonzero(tr.is_leaf)[0]
    assert np.all(tr.weight[tr.is_leaf == 0] == 0)
    for w, node in enumerate(words):
        want = math.log(len(docs) / int(Ni[w])) if Ni[w] > 0 else 0.0
        assert np.float64(want).tobytes() == tr.weight[node].tobytes(), (w, node)
    for weighting in (1, 3):  # TF, BINARY: every word weighs 1
        t1 = T.golden_trained(weighting)
        assert np.array_equal(t1.desc, tr.desc) and np.array_equal(t1.weight, (t1.is_leaf == 1).astype(np.float64))


def test_fixed_point_on_the_golden_frames(golden):
    _check_fixed_point(T.golden_trained(2), T.golden_docs(golden), T.GOLDEN_K, T.GOLDEN_L)


def test_edge_sweep_exercises_the_deviations():
    emptied = short = trivial = 0
    for i in range(T.SWEEP):
        docs, k, L, seed = T.sweep_case(i)
        tr = T.train(docs, k, L, i % 4, seed)
        _check_fixed_point(tr, docs, k, L)
        n = sum(len(d) for d in docs)
        assert len(tr.feat_node) == n and np.all(tr.is_leaf[tr.feat_node - 1] == 1)
        emptied += tr.stats["emptied_clusters"] > 0
        short += tr.stats["short_seedings"] > 0
        trivial += tr.stats["trivial_nodes"] > 0
    print("sets with emptied clusters %d, short seedings %d, trivial nodes %d" % (emptied, short, trivial))
    assert emptied >= 1 and short >= 1 and trivial >= 1


def test_round_limit_and_seed():
    docs, k, L, seed = T.sweep_case(0)
    a, b = T.train(docs, k, L, 0, seed), T.train(docs, k, L, 0, seed + 1)
    assert a.stats["max_rounds_seen"] > 2
    assert not (np.array_equal(a.parent, b.parent) and np.array_equal(a.desc, b.desc))  # the seed matters
    c = T.train(docs, k, L, 0, seed, max_rounds=2)
    assert c.stats["capped_runs"] >= 1 and c.stats["max_rounds_seen"] == 2


# ---- the seeding against its numpy statement (voc_train_ref_lib.seeds_numpy, written from include/orbx.h) -------------------------


def _check_seeds(tr, feats, k, seed, what):
    """Of a training stopped after one round: every split node's children are, in count and bytes, the seeds the numpy statement
    picks from the node's group under the node's key (a node of at most k features: its features).  Returns the seedings that
    stopped short, counted from the statement's own output."""
    short = 0
    for s in T.splits_of(tr, len(feats)):
        f = feats[s.group]
        picks = list(range(len(f))) if len(f) <= k else T.seeds_numpy(f, k, seed, s.key)
        short += len(f) > k and len(picks) < k
        assert len(s.children) == len(picks), (what, s.node, s.key)
        assert np.array_equal(tr.desc[np.array(s.children) - 1], f[picks]), (what, s.node, s.key)
    return short


def test_seeding_equals_the_numpy_statement():
    ran = short = 0
    for i in range(T.SWEEP):
        docs, k, L, seed = T.sweep_case(i)
        feats = T.case_feats(docs)
        if len(feats) <= k:
            continue  # (the trivial root: nothing is seeded)
        tr = T.train(docs, k, 1, 0, seed, max_rounds=1)
        picks = T.seeds_numpy(feats, k, seed, 0)
        assert len(tr.parent) == len(picks) and np.array_equal(tr.desc, feats[picks]), "set %d" % i
        assert tr.stats["short_seedings"] == (len(picks) < k), "set %d" % i
        ran += 1
        short += len(picks) < k
    deeper = 0
    for i, L in [(j, 2) for j in range(14)] + [(20, 3), (22, 3), (24, 3)]:
        docs, k, _, seed = T.sweep_case(i)
        feats = T.case_feats(docs)
        if len(feats) <= k:
            continue
        tr = T.train(docs, k, L, 0, seed, max_rounds=1)
        short_here = _check_seeds(tr, feats, k, seed, "set %d, L %d" % (i, L))
        assert short_here == tr.stats["short_seedings"]
        parent, desc = T.seeded_tree_numpy(feats, k, L, seed)
        assert np.array_equal(parent, tr.parent) and np.array_equal(desc, tr.desc), "set %d, L %d" % (i, L)
        deeper += 1
    print("seeding: %d of %d sweep sets with n > k, %d of them stop short; %d sets with L 2 or 3" % (ran, T.SWEEP, short, deeper))
    assert ran >= T.SWEEP - 1 and short >= 1 and deeper >= 12


def test_size_constants_equal_the_device_header():
    text = open(os.path.join(T.ROOT, "orb_slam_tracking_amd", "csrc", "orbx_device.h")).read()
    for name in ("VT_THREADS", "VT_CHUNK", "VT_SEED_LDS", "VT_KMAX"):
        m = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert len(m) == 1 and int(m[0]) == getattr(T, name), name
    m = re.findall(r"#define\s+ORBX_BOW_MAX_FEATURES\s+(\d+)", open(os.path.join(T.ROOT, "include", "orbx.h")).read())
    assert len(m) == 1 and int(m[0]) == T.MAX_DOC


def _levels(tr, n_feat):
    """level -> the sizes of the groups that were split there (level 1: the root's), from the restatement's tree."""
    out = {}
    for s in T.splits_of(tr, n_feat):
        out.setdefault(s.level, []).append(len(s.group))
    return out


@pytest.mark.parametrize("name", T.SIZE_CASES)
def test_size_cases_reach_their_paths(name):
    """Each named input of voc_train_ref_lib.size_case meets, in the restatement's tree alone, the condition it exists for (the
    device's path at that size is in the comment), and is a fixed point of k-means."""
    cases, trained = T.size_case(name), T.size_trained(name)
    B, C, S = T.VT_THREADS, T.VT_CHUNK, T.VT_SEED_LDS
    for c, tr in zip(cases, trained):
        n = sum(len(d) for d in c.docs)
        lv = _levels(tr, n)
        kmeans = {level: [m for m in sizes if m > c.k] for level, sizes in lv.items()}
        print(name, c.label, "n %d k %d L %d" % (n, c.k, c.L), tr.stats, "k-means nodes per level",
              {level: len(v) for level, v in kmeans.items()})
        assert all(len(d) <= T.MAX_DOC for d in c.docs)
        assert tr.stats["capped_runs"] == 0
        if name == "root_above_65536":
            assert n > B * B  # k_vt_seed_pick: more than VT_THREADS blocks, two block sums per thread
            assert len([m for m in lv[2] if m > max(C, S)]) >= 2  # grid-wide seeding and global counters, several nodes at once
            assert max(len(d) for d in c.docs) == T.MAX_DOC and c.weighting == T.IDF  # k_vt_docfreq at the largest capacity
        elif name == "edges_of_4096":
            assert (C, S) == (4096, 4096) and n == int(c.label) and len(c.docs) == 1 and lv[1] == [n] and n > c.k
        elif name == "edges_of_256":
            assert B == 256 and n == int(c.label) and lv[1] == [n] and c.grid_min < B - 1 and c.L == 2
            assert any(m > c.grid_min for m in lv.get(2, []))  # a grid-seeded node that does not start at a block's edge
        elif name == "edge_of_65536":
            assert n == int(c.label) and lv[1] == [n] and n - B * B in (0, 1)
        elif name == "emptied_in_chunks":
            assert c.L == 1 and n > C and tr.stats["emptied_clusters"] >= 1  # vtMean's size == 0 from k_vt_centre_final
        elif name == "short_seeding_large":
            assert n > S and c.grid_min is None and tr.stats["short_seedings"] >= 1
            assert len(T.children_of(tr.parent)[0]) < c.k  # the root itself, above VT_SEED_LDS, was seeded short
        elif name == "wide_level":
            assert max(len(v) for v in kmeans.values()) > B  # k_vt_round's second workgroup
            assert [len(lv[level]) for level in (1, 2, 3, 4)] == [1, 10, 100, 1000]
        elif name == "k20":
            assert c.k == T.VT_KMAX and len(T.children_of(tr.parent)[0]) == T.VT_KMAX and any(m > c.k for m in lv[2])
        elif name == "deep":
            assert c.L == 10 and max(lv) == 10 and any(m > c.k for m in lv[10])  # keys up to 21^9 and beyond
        elif name == "many_documents":
            lens = [len(d) for d in c.docs]
            assert len(lens) >= 700 and lens.count(0) >= 10 and 32 < max(lens) <= 64  # k_vt_docfreq sorts 64 keys a document
            assert c.weighting in (T.IDF, T.TF_IDF)
            w = tr.weight[tr.is_leaf == 1]
            assert w.min() < math.log(len(lens) / 100.0) and len(np.unique(w)) > 20  # a word in more than 100 documents
        _check_fixed_point(tr, c.docs, c.k, c.L)
    assert {c.label for c in cases} == {"root_above_65536": {"81920"}, "edges_of_4096": {"4095", "4096", "4097"},
                                        "edges_of_256": {"255", "256", "257", "512", "513"}, "edge_of_65536": {"65536", "65537"},
                                        "many_documents": {"idf", "tf_idf"}}.get(name, {cases[0].label})
