"""The device against the reference's own compiled code (oracle/_ref/libref.so, tests/ref_lib.py), with no restatement in
between: DBoW2's loadFromTextFile + transform + L1Scoring::score vs Vocabulary.from_text + transform / score, and
ORBmatcher::SearchForInitialization vs the device matcher.  The exclusions of tests/test_ref_pins.py apply (files written without
a trailing newline, deviation 2's FeatureVector entries not compared)."""
import numpy as np
import pytest

import bow_ref_lib as R
import ref_lib as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext(orbx):
    F.lib()  # fails (does not skip) when oracle/_ref/libref.so is missing
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def full_voc(orbx, ext, golden, tmp_path_factory):
    """The full k = 10, L = 6 vocabulary (1,111,110 nodes) in the reference and on the device, loaded once from one file."""
    voc = R.full_vocabulary(golden["canonical/dbow0/desc"])
    path = str(tmp_path_factory.mktemp("refpins") / "full.txt")
    F.write_for_reference(path, voc)
    ref = F.Vocabulary(path)
    dev = orbx.Vocabulary.from_text(ext, path)
    yield voc, ref, dev
    dev.close()
    ref.close()


def _dev(res):
    return dict(bow_word=res.bow_word, bow_value=res.bow_value, fv_node=res.fv_node, fv_feat=res.fv_feat, feat_word=res.feat_word)


def test_full_vocabulary_vs_reference(golden, full_voc):
    voc, ref, dev = full_voc
    assert (dev.k, dev.L, dev.scoring, dev.weighting, dev.n_nodes, dev.n_words) == (ref.k, ref.L, ref.scoring, ref.weighting,
                                                                                   ref.n_nodes, ref.n_words)
    frames = [golden["canonical/%s/desc" % f] for f in ("dbow0", "dbow1", "dbow2", "dbow3", "init0")]
    vecs = []
    for i, d in enumerate(frames):
        for ls in ((0, 2, 4, 6, 7) if i < 2 else (4,)):
            r = ref.transform(d, ls)
            F.same_transform(r, _dev(dev.transform(d, ls, feat_word=True)), ("full", i, ls))  # a full tree has no shallow leaf
            if ls == 4:
                vecs.append(r)
    for a in vecs:
        for b in vecs:
            want = F.score(0, a["bow_word"], a["bow_value"], b["bow_word"], b["bow_value"])
            got = dev.score(a["bow_word"], a["bow_value"], b["bow_word"], b["bow_value"])
            assert np.float64(want).tobytes() == np.float64(got).tobytes()


@pytest.mark.parametrize("weighting", range(4))
def test_irregular_trees_vs_reference(orbx, ext, tmp_path, weighting):
    """Irregular trees (ties, childless non-leaf nodes, flagged leaves with children, zero and negative weights) with L1 and
    DOT_PRODUCT scoring, levelsup 0 .. L + 1, and the device's L1 score against the reference's."""
    for seed in range(2):
        for scoring in (0, 5, 1):
            voc = R.irregular_tree(seed, k=4, L=5, n_nodes=300, scoring=scoring, weighting=weighting)
            path = str(tmp_path / ("irr%d-%d.txt" % (seed, scoring)))
            F.write_for_reference(path, voc)
            ref, dev = F.Vocabulary(path), orbx.Vocabulary.from_text(ext, path)
            feats = np.concatenate([R.features_near(voc, 200, seed + 80), voc.desc[:16]])
            vecs = []
            for ls in range(0, 7):
                r = ref.transform(feats, ls)
                F.same_transform(r, _dev(dev.transform(feats, ls, feat_word=True)), (seed, scoring, weighting, ls),
                                 F.shallow_features(voc, feats, ls))
            if scoring == 0:
                for n, s in ((1, 1), (40, 2), (150, 3)):
                    vecs.append(ref.transform(R.features_near(voc, n, 90 + s), 4))
                for a in vecs:
                    for b in vecs:
                        want = F.score(0, a["bow_word"], a["bow_value"], b["bow_word"], b["bow_value"])
                        got = dev.score(a["bow_word"], a["bow_value"], b["bow_word"], b["bow_value"])
                        assert np.float64(want).tobytes() == np.float64(got).tobytes()
            dev.close()
            ref.close()


def _check_match(orbx, ext, case):
    name, k1, d1, k2, d2, bounds, window, ratio, ori = case
    want = F.match_init(k1, d1, k2, d2, bounds, window, ratio, ori)
    m = orbx.ORBmatcher(ratio, ori, extractor=ext)
    nm, m12 = m.SearchForInitialization(orbx.Frame.from_arrays(k1, d1, bounds), orbx.Frame.from_arrays(k2, d2, bounds), window)
    assert nm == want[0], name
    assert np.array_equal(m12, want[1]), name
    assert list(m.last_stats) == want[2].tolist(), name


def test_matches_golden_pairs_vs_reference(orbx, ext, golden, images):
    widths = {k: v.shape[1] for k, v in images.items()}
    for name, k1, d1, k2, d2, bounds in F.golden_pairs(golden, widths):
        _check_match(orbx, ext, (name, k1, d1, k2, d2, bounds, 100, 0.9, True))


def test_matches_edges_and_fuzz_vs_reference(orbx, ext):
    """The contention and edge cases, and a third of the CPU fuzz, whose keypoints include octave -1: GetFeaturesInArea skips
    its level check for a negative level, so such a query's candidates are the trains of every octave (the device sends its pair
    through the general loop)."""
    for case in F.contention_cases() + F.edge_cases() + [F.fuzz_case(s) for s in range(0, 300, 3)]:
        _check_match(orbx, ext, case)


def test_negative_octave_queries_vs_reference(orbx, ext):
    """Queries of octave -1 in pairs that the small kernel and the wide path would take, in the two-call API and the batched
    device-resident one.  The cases are chosen so that the octave filter matters: the reference's result changes when the
    octave -1 queries are read as octave 0."""
    rng = np.random.default_rng(29)
    cases = []
    for n, npro, win, w, h in ((120, 40, 60, 640, 480), (1500, 300, 100, 1280, 720), (2400, 2400, 300, 1920, 1080)):
        k1, d1, k2, d2 = F.contention_pair(rng, n, npro, 8, w, h, 0.6, win / 3)
        k1["octave"] = np.where(rng.random(n) < 0.3, -1, k1["octave"])
        cases.append(("negative-octave-%d" % n, k1, d1, k2, d2, (0, w, 0, h), win, 0.9, True))
    for case in cases:
        name, k1, d1, k2, d2, bounds, win, ratio, ori = case
        as0 = k1.copy()
        as0["octave"] = np.maximum(as0["octave"], 0)
        assert not np.array_equal(F.match_init(as0, d1, k2, d2, bounds, win, ratio, ori)[1],
                                  F.match_init(k1, d1, k2, d2, bounds, win, ratio, ori)[1]), name
        _check_match(orbx, ext, case)
    # the batched device-resident form: all three pairs in one call, in the bounds of the largest frame (one bounds per call)
    import torch
    cap, nf, bounds = 2400, 2 * len(cases), (0, 1920, 0, 1080)
    kps, desc, cnt = np.zeros((nf, cap), F.KP), np.zeros((nf, cap, 32), np.uint8), np.zeros(nf, np.int32)
    for p, c in enumerate(cases):
        for f, (k, d) in enumerate(((c[1], c[2]), (c[3], c[4]))):
            kps[2 * p + f, :len(k)], desc[2 * p + f, :len(d)], cnt[2 * p + f] = k, d, len(k)
    e = orbx.ORBextractor(cap, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=nf, device=0)
    d_k = torch.from_numpy(kps.view(np.uint8).reshape(-1)).cuda()
    d_d, d_n = torch.from_numpy(desc.reshape(-1)).cuda(), torch.from_numpy(cnt).cuda()
    P = len(cases)
    d_m = torch.zeros(P * cap, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")
    d_st = torch.zeros(P * 3, dtype=torch.int32, device="cuda")
    e.match_pairs_device(np.arange(0, nf, 2, dtype=np.int32), np.arange(1, nf, 2, dtype=np.int32), d_k, d_d, d_n, bounds, d_m, d_nm,
                         d_st, 100, 0.9, True, cap)
    mm, nm, st = d_m.cpu().numpy().reshape(P, cap), d_nm.cpu().numpy(), d_st.cpu().numpy().reshape(-1, 3)
    e.close()
    for p, c in enumerate(cases):
        want = F.match_init(c[1], c[2], c[3], c[4], bounds, 100, 0.9, True)
        assert nm[p] == want[0] and np.array_equal(mm[p, :len(c[1])], want[1]) and st[p].tolist() == want[2].tolist(), c[0]
