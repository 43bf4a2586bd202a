"""CPU tests pinned to the reference's own compiled code (oracle/_ref/libref.so, tests/ref_lib.py), not to a restatement of it:
  - the DBoW2 restatement (tests/cpp/bow_ref.cpp, which the device is tested against bit for bit) vs DBoW2's own transform and
    L1 score, bit for bit, for every weighting x scoring and levelsup 0 .. L + 1;
  - the library's host parser (orbx_vocabulary_parse_text) vs DBoW2's loadFromTextFile on the same files;
  - the CPU oracle's matcher and frame grid (oracle/orbx_oracle.cpp, which the device is tested against) vs the reference's
    ORBmatcher::SearchForInitialization, Frame::GetFeaturesInArea and Frame::PosInGrid.
Nothing here needs a GPU.  Where the reference's behaviour is undefined, the test does not compare; each exclusion is stated where
it is made."""
import math
import os

import numpy as np
import pytest

import bow_ref_lib as R
import ref_lib as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _ref_library():
    F.lib()  # fails (does not skip) with the command that builds it when oracle/_ref/libref.so is missing


# ---- bag of words: restatement vs reference -------------------------------------------------------------------------------

def check_restatement(tmp_path, voc, feats, levelsups, tag):
    path = str(tmp_path / ("%s.txt" % tag))
    F.write_for_reference(path, voc)
    ref = F.Vocabulary(path)
    assert (ref.k, ref.L, ref.scoring, ref.weighting) == tuple(voc.header)
    assert ref.n_nodes == len(voc.parent) and ref.n_words == int((voc.is_leaf > 0).sum())
    for ls in levelsups:
        r = ref.transform(feats, ls)
        m = voc.transform(feats, ls)
        F.same_transform(r, m, (tag, ls), F.shallow_features(voc, feats, ls))
        r2 = ref.transform(feats, ls, feature_vector=False, feat_word=False)  # the two-argument transform
        assert np.array_equal(r2["bow_word"], r["bow_word"]) and r2["bow_value"].tobytes() == r["bow_value"].tobytes()
    ref.close()


@pytest.mark.parametrize("weighting", range(4))
@pytest.mark.parametrize("scoring", range(6))
def test_restatement_vs_reference_irregular(tmp_path, scoring, weighting):
    """Irregular trees (ties in the descent, childless nodes flagged non-leaf, flagged leaves with children, zero and negative
    weights) for every weighting x scoring -- including DOT_PRODUCT's division by the number of words -- at levelsup 0 .. L + 1."""
    for seed in range(3):
        base = R.irregular_tree(seed, k=4, L=5, n_nodes=300)
        voc = base.with_types(scoring, weighting)
        feats = np.concatenate([R.features_near(voc, 150, seed + 50), voc.desc[:20], voc.desc[-10:]])
        check_restatement(tmp_path, voc, feats, range(0, voc.header[1] + 2), "irr%d-%d-%d" % (seed, scoring, weighting))


@pytest.mark.parametrize("weighting", range(4))
@pytest.mark.parametrize("scoring", range(6))
def test_restatement_vs_reference_full_small(tmp_path, golden, scoring, weighting):
    """Full k = 10, L = 3 trees built from real descriptors, every weighting x scoring, levelsup 0 .. L + 1."""
    voc = R.full_vocabulary(golden["canonical/dbow0/desc"], k=10, L=3, seed=5, scoring=scoring, weighting=weighting)
    feats = np.concatenate([golden["canonical/dbow1/desc"][:400], R.features_near(voc, 100, 9)])
    check_restatement(tmp_path, voc, feats, range(0, 5), "full3-%d-%d" % (scoring, weighting))


def test_restatement_vs_reference_full_vocabulary(tmp_path, golden):
    """The full k = 10, L = 6 vocabulary (1,111,110 nodes, the size of ORB-SLAM's ORBvoc.txt) with the golden descriptors."""
    voc = R.full_vocabulary(golden["canonical/dbow0/desc"])
    feats = np.concatenate([golden["canonical/dbow1/desc"], golden["canonical/dbow2/desc"][:300]])
    check_restatement(tmp_path, voc, feats, (0, 2, 4, 6, 7), "full6")


def test_l1_score_restatement_vs_reference(tmp_path):
    """L1Scoring::score of the reference vs the restatement's on transformed vectors (sparse overlaps, identical vectors, an
    empty vector), and the device's scoring choice: the other five scoring objects differ from L1 on the same vectors."""
    voc = R.irregular_tree(4, k=4, L=5, n_nodes=300)
    path = str(tmp_path / "l1.txt")
    F.write_for_reference(path, voc)
    ref = F.Vocabulary(path)
    vecs = [ref.transform(R.features_near(voc, n, 70 + i), 4) for i, n in enumerate((1, 5, 30, 120, 200, 0))]
    vecs.append(vecs[2])
    for a in vecs:
        for b in vecs:
            want = F.score(0, a["bow_word"], a["bow_value"], b["bow_word"], b["bow_value"])
            got = R.score_l1(a["bow_word"], a["bow_value"], b["bow_word"], b["bow_value"])
            assert np.float64(want).tobytes() == np.float64(got).tobytes()
    a, b = vecs[3], vecs[4]
    l1 = F.score(0, a["bow_word"], a["bow_value"], b["bow_word"], b["bow_value"])
    others = [F.score(s, a["bow_word"], a["bow_value"], b["bow_word"], b["bow_value"]) for s in range(1, 6)]
    assert all(math.isfinite(v) for v in others) and all(v != l1 for v in others)
    ref.close()


# ---- the library's text parser vs the reference loader --------------------------------------------------------------------

def small_tree():
    """A valid k = 3, L = 3 tree of 20 nodes (leaves at depth 1 .. 3)."""
    return R.irregular_tree(21, k=3, L=3, n_nodes=20)


def tree_lines(voc, weight_fmt=repr):
    k, L, sc, wt = voc.header
    lines = ["%d %d  %d %d" % (k, L, sc, wt)]
    for i in range(len(voc.parent)):
        lines.append("%d %d %s %s" % (voc.parent[i], voc.is_leaf[i], " ".join(str(int(b)) for b in voc.desc[i]),
                                      weight_fmt(float(voc.weight[i]))))
    return lines


def write_lines(path, lines, eol="\n"):
    with open(path, "w", newline="") as f:
        f.write(eol.join(lines))  # no trailing line: deviation 1


def parse_both(orbx, path):
    """(library parse, reference vocabulary) of one file; the library's result as (header, parent, is_leaf, desc, weight)."""
    return orbx.Vocabulary.parse_text(path), F.Vocabulary(path)


def same_parse(mine, ref):
    hdr, parent, leaf, desc, weight = mine
    assert tuple(hdr) == (ref.k, ref.L, ref.scoring, ref.weighting)
    rp, _, rd, rw, word_node = ref.nodes()
    assert ref.n_nodes == len(parent)
    assert np.array_equal(rp, parent)
    assert np.array_equal(word_node, np.nonzero(leaf > 0)[0] + 1)  # word ids in file order to the lines flagged > 0
    assert np.array_equal(rd, desc)
    assert rw.tobytes() == weight.tobytes()


@pytest.mark.parametrize("fmt", ["%.17g", "%g", "repr"])
def test_parser_vs_reference_weight_formats(orbx, tmp_path, fmt):
    """17 significant digits, 6 (what saveToTextFile writes: an ostream's default precision) and the shortest round trip."""
    f = repr if fmt == "repr" else (lambda w: fmt % w)
    path = str(tmp_path / "w.txt")
    write_lines(path, tree_lines(small_tree(), f))
    same_parse(*parse_both(orbx, path))


ACCEPTED_WEIGHTS = ["+.5", "5.", "-0", "1e-400", "4.9406564584124654e-324", "1E+2", "-.25e-1", "000123.5000", "+0e0",
                    "1.7976931348623157e308"]


@pytest.mark.parametrize("token", ACCEPTED_WEIGHTS)
def test_parser_vs_reference_weight_tokens(orbx, tmp_path, token):
    """Weight tokens both read: the library must give the reference's exact double (the sign of -0, the underflow of 1e-400 to
    0 and of the smallest denormal included)."""
    lines = tree_lines(small_tree())
    for i in (1, 7, len(lines) - 1):
        parts = lines[i].split(" ")
        parts[-1] = token
        lines[i] = " ".join(parts)
    path = str(tmp_path / "t.txt")
    write_lines(path, lines)
    same_parse(*parse_both(orbx, path))


# token -> what the reference loader (`ssnode >> weight`, libstdc++'s num_get) makes of it
REFUSED_WEIGHTS = {"inf": 0.0, "nan": 0.0, "-inf": 0.0, "infinity": 0.0, "0x1p3": 0.0, "1e400": 1.7976931348623157e308,
                   "-1e400": -1.7976931348623157e308, "1e5x": 1e5, "1e": 0.0, ".": 0.0}


@pytest.mark.parametrize("token", sorted(REFUSED_WEIGHTS))
def test_parser_refuses_weights_the_reference_misreads(orbx, tmp_path, token):
    """Deviation 3 (include/orbx.h): a weight token that is not one complete finite decimal number is refused (ORBX_E_BADARG).
    The reference reads these without an error it reports: no number (inf, nan, a lone exponent) as 0, a hexadecimal float as
    its leading 0, an overflow as +-DBL_MAX, a number with trailing characters as its prefix.  Pinned here as the reason."""
    lines = tree_lines(small_tree())
    parts = lines[5].split(" ")
    parts[-1] = token
    lines[5] = " ".join(parts)
    path = str(tmp_path / "bad.txt")
    write_lines(path, lines)
    with pytest.raises(orbx.OrbxError) as e:
        orbx.Vocabulary.parse_text(path)
    assert e.value.code == orbx.E_BADARG
    _, _, _, rw, _ = F.Vocabulary(path).nodes()
    assert rw[4] == REFUSED_WEIGHTS[token]


def test_parser_vs_reference_descriptor_tokens(orbx, tmp_path):
    """Descriptor elements: an explicit sign, values outside a byte (300 -> 44, -1 -> 255: int, then cast) and a leading zero
    (07 is decimal 7)."""
    lines = tree_lines(small_tree())
    for i, toks in ((1, ("+7", "300", "-1", "07")), (4, ("07", "-1", "+0", "256")), (len(lines) - 1, ("-255", "511", "+300", "0"))):
        parts = lines[i].split(" ")
        parts[2:6] = toks
        lines[i] = " ".join(parts)
    path = str(tmp_path / "d.txt")
    write_lines(path, lines)
    mine, ref = parse_both(orbx, path)
    same_parse(mine, ref)
    assert mine[3][0][:4].tolist() == [7, 44, 255, 7]


def test_parser_vs_reference_crlf_and_trailing_tokens(orbx, tmp_path):
    """CRLF line endings, and extra tokens after the weight (the reference reads 35 numbers and ignores the rest of the line)."""
    voc = small_tree()
    path = str(tmp_path / "crlf.txt")
    write_lines(path, tree_lines(voc), eol="\r\n")
    same_parse(*parse_both(orbx, path))
    lines = tree_lines(voc)
    lines = [lines[0] + " 7 x"] + [ln + (" 1 2 3" if i % 2 else " junk") for i, ln in enumerate(lines[1:])]
    path = str(tmp_path / "extra.txt")
    write_lines(path, lines)
    same_parse(*parse_both(orbx, path))


def test_parser_vs_reference_irregular_and_full(orbx, tmp_path, golden):
    """Whole vocabularies: irregular trees (flags 0, 1 and 2, zero and negative weights) and a full k = 10, L = 3 tree."""
    for i, voc in enumerate([R.irregular_tree(s, k=4, L=5, n_nodes=300) for s in range(3)] +
                            [R.full_vocabulary(golden["canonical/dbow0/desc"], k=10, L=3, seed=2)]):
        path = str(tmp_path / ("v%d.txt" % i))
        F.write_for_reference(path, voc, exact=bool(i % 2))
        same_parse(*parse_both(orbx, path))


# ---- matcher and frame grid: the CPU oracle vs the reference --------------------------------------------------------------

def _check_match(oracle, case):
    name, k1, d1, k2, d2, bounds, window, ratio, ori = case
    want = F.match_init(k1, d1, k2, d2, bounds, window, ratio, ori)
    got = oracle.match_init(k1, d1, k2, d2, bounds, window, ratio, ori)
    assert got[0] == want[0], name
    assert np.array_equal(got[1], want[1]), name
    assert got[2].tolist() == want[2].tolist(), name
    # the in-area candidate lists the matcher searches, in the reference's order, for F1's keypoints it does not skip
    for i in np.nonzero(np.asarray(k1["octave"]) <= 0)[0][:200]:
        lv = int(k1["octave"][i])
        r = F.features_in_area(k2, bounds, k1["x"][i], k1["y"][i], window, lv, lv)
        o = oracle.features_in_area(k2, bounds, float(k1["x"][i]), float(k1["y"][i]), float(window), lv, lv)
        assert np.array_equal(r, o), (name, int(i))
    return want[0]


def test_match_golden_pairs_vs_reference(oracle, golden, images):
    widths = {k: v.shape[1] for k, v in images.items()}
    pairs = F.golden_pairs(golden, widths)
    assert len(pairs) == 4
    total = 0
    for name, k1, d1, k2, d2, bounds in pairs:
        nm = _check_match(oracle, (name, k1, d1, k2, d2, bounds, 100, 0.9, True))
        assert nm == int(golden["%s/nmatches" % name])
        total += nm
    assert total >= 200


def test_match_contention_and_edge_cases_vs_reference(oracle):
    for case in F.contention_cases() + F.edge_cases():
        _check_match(oracle, case)


def test_match_fuzz_vs_reference(oracle):
    """300 small random pairs on the matcher's edges (ref_lib.fuzz_case); enough of them must produce matches, ratio and
    orientation rejections for the comparison to mean something."""
    total, stats = 0, np.zeros(3, np.int64)
    for seed in range(300):
        case = F.fuzz_case(seed)
        total += _check_match(oracle, case)
        stats += F.match_init(*case[1:])[2]
    assert total > 150 and (stats > 50).all(), (total, stats)


def test_pos_in_grid_vs_reference(oracle):
    """Frame::PosInGrid on cell edges, half cells, bound edges and outside the bounds, for bounds not starting at 0."""
    rng = np.random.default_rng(3)
    for bounds in ((0, 640, 0, 480), (-7, 633, 5, 470), (0, 752, 0, 480), (3, 67, -2, 46), (0, 1, 0, 1)):
        x0, x1, y0, y1 = bounds
        cw, ch = np.float32(x1 - x0) / np.float32(64), np.float32(y1 - y0) / np.float32(48)
        n = 4000
        k = np.zeros(n, F.KP)
        k["x"] = (x0 + rng.integers(-2, 67, n) * cw * rng.choice([1.0, 0.5, 0.25], n) + rng.choice([0, 0, 1e-3, -1e-3], n)).astype(np.float32)
        k["y"] = (y0 + rng.integers(-2, 51, n) * ch * rng.choice([1.0, 0.5, 0.25], n) + rng.choice([0, 0, 1e-3, -1e-3], n)).astype(np.float32)
        pos, ok = F.pos_in_grid(k, bounds)
        ox, oy, ook = oracle.pos_in_grid(k, bounds)
        assert np.array_equal(ook, ok), bounds
        assert np.array_equal(ox, pos[:, 0]) and np.array_equal(oy, pos[:, 1]), bounds
