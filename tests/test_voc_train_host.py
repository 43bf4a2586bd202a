"""Vocabulary training (orbx_vocabulary_train, include/orbx.h "training") without a device: the ABI's refusals, and the CPU
restatement the GPU tests compare against (tests/cpp/voc_train_ref.cpp) checked on its own -- against the reference's compiled
DBoW2 as far as oracle/_ref/libref.so reaches (its loader, its transform), and against the fixed-point property of k-means stated
in numpy.  (save_text needs a vocabulary, which needs a device: its round trip is in tests/test_gpu_voc_train.py.)"""
import ctypes
import math

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


def _groups(tr, n_feat):
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


def _check_fixed_point(tr, docs, k, L):
    """For every node that was split and not stopped by the round limit: each child's descriptor is meanValue of its group (the
    trivial case: the feature itself, in order), and every feature's nearest child, the first among equals, is its group's."""
    feats = np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in docs] + [np.zeros((0, 32), np.uint8)])
    if len(feats) == 0:
        assert len(tr.parent) == 0
        return
    assert tr.stats["capped_runs"] == 0  # (no input of these tests runs into the limit of 100 rounds)
    children, groups = T.children_of(tr.parent), _groups(tr, len(feats))
    bits = np.unpackbits(feats, axis=1).astype(np.int32)
    nbits = np.unpackbits(tr.desc, axis=1).astype(np.int32)
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
        dist = (bits[g][:, None, :] != nbits[np.array(ch) - 1][None, :, :]).sum(axis=2)
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
