"""Bag of words without a device: the CPU restatement (tests/cpp/bow_ref.cpp) against a plain-Python descent, the library's text
parser (orbx_vocabulary_parse_text) against the restatement's loader, the refused inputs (ORBX_E_BADARG), create without a
device (ORBX_E_HIP), and the C++ shim's ORBVocabulary compiling against liborbx."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bow_ref_lib as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _py_transform(voc, feats, levelsup):
    """DBoW2's transform in plain Python, straight from the semantics (a check on the restatement itself)."""
    n = len(voc.parent)
    children = {i: [] for i in range(n + 1)}
    for i in range(n):
        children[int(voc.parent[i])].append(i + 1)
    word, nw = {}, 0
    for i in range(n):
        if voc.is_leaf[i] > 0:
            word[i + 1], nw = nw, nw + 1
    k, L, scoring, weighting = voc.header
    bow, fv, fw = {}, {}, []
    for fi, f in enumerate(feats):
        cur, level, nid = 0, 0, (0 if L - levelsup <= 0 else None)
        while children[cur]:
            level += 1
            d = [bin(int.from_bytes(np.bitwise_xor(f, voc.desc[c - 1]).tobytes(), "little")).count("1") for c in children[cur]]
            cur = children[cur][d.index(min(d))]
            if level == L - levelsup:
                nid = cur
        if nid is None:
            nid = cur
        w = float(voc.weight[cur - 1]) if cur else 0.0
        fw.append(word.get(cur, 0))
        if nw == 0 or not w > 0:
            continue
        wid = word.get(cur, 0)
        if wid in bow:
            if weighting in (0, 1):
                bow[wid] += w
        else:
            bow[wid] = w
        fv.setdefault(nid, []).append(fi)
    if nw == 0:
        bow, fv = {}, {}
    if scoring == 5:
        if weighting in (0, 1) and bow:
            nd = float(len(bow))
            bow = {w: v / nd for w, v in bow.items()}
    else:
        norm = 0.0
        for w in sorted(bow):
            norm += abs(bow[w]) if scoring != 1 else bow[w] * bow[w]
        if scoring == 1:
            norm = float(np.sqrt(norm))
        if norm > 0:
            bow = {w: v / norm for w, v in bow.items()}
    ws = sorted(bow)
    fvp = [(nd, f) for nd in sorted(fv) for f in fv[nd]]
    return dict(bow_word=np.array(ws, np.uint32), bow_value=np.array([bow[w] for w in ws], np.float64),
                fv_node=np.array([p[0] for p in fvp], np.uint32), fv_feat=np.array([p[1] for p in fvp], np.uint32),
                feat_word=np.array(fw, np.uint32))


def _same(a, b):
    for key in ("bow_word", "fv_node", "fv_feat", "feat_word"):
        assert np.array_equal(np.asarray(a[key], np.uint32), np.asarray(b[key], np.uint32)), key
    assert np.asarray(a["bow_value"], np.float64).tobytes() == np.asarray(b["bow_value"], np.float64).tobytes()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_matches_plain_python_descent(seed):
    base = R.irregular_tree(seed, k=3, L=4, n_nodes=60)
    feats = R.features_near(base, 40, seed + 10)
    for scoring in range(6):
        for weighting in range(4):
            voc = base.with_types(scoring, weighting)
            for levelsup in (0, 2, 5):
                _same(voc.transform(feats, levelsup), _py_transform(voc, feats, levelsup))


def test_restatement_score_l1():
    w1, v1 = np.array([1, 3, 5, 9], np.uint32), np.array([0.1, 0.2, 0.3, 0.4])
    w2, v2 = np.array([3, 4, 9], np.uint32), np.array([0.5, 0.25, 0.25])
    s = 0.0
    for a, b in ((0.2, 0.5), (0.4, 0.25)):
        s += abs(a - b) - abs(a) - abs(b)
    assert R.score_l1(w1, v1, w2, v2) == -s / 2.0
    assert R.score_l1(w1, v1, w1, v1) == 1.0
    assert R.score_l1(w1, v1, np.array([2], np.uint32), np.array([1.0])) == 0.0


@pytest.mark.parametrize("trailing", [True, False])
@pytest.mark.parametrize("exact", [True, False])
def test_parse_text_matches_restatement(orbx, tmp_path, trailing, exact):
    voc = R.irregular_tree(5, k=4, L=5, n_nodes=200, scoring=2, weighting=1)
    path = str(tmp_path / "voc.txt")
    R.write_text(path, voc, trailing_newline=trailing, exact=exact)
    hdr, parent, leaf, desc, weight = orbx.Vocabulary.parse_text(path)
    rh, rp, rl, rd, rw = R.parse_text(path)
    assert list(hdr) == list(rh) == [4, 5, 2, 1]
    assert len(parent) == len(voc.parent) == len(rp)
    assert np.array_equal(parent, rp) and np.array_equal(leaf, rl) and np.array_equal(desc, rd)
    assert weight.tobytes() == rw.tobytes()
    if exact:
        assert weight.tobytes() == voc.weight.tobytes() and np.array_equal(desc, voc.desc)


def test_parse_text_descriptor_elements_cast_to_uint8(orbx, tmp_path):
    path = str(tmp_path / "v.txt")
    with open(path, "w") as f:
        f.write("2 1  0 0\n0 1 " + " ".join(["-1", "256", "300"] + ["7"] * 29) + " 0.5\n   \n0 1 " + " ".join(["1"] * 32) + " 1e-3\n\n")
    hdr, parent, leaf, desc, weight = orbx.Vocabulary.parse_text(path)
    assert len(parent) == 2 and list(desc[0][:3]) == [255, 0, 44] and weight[1] == 1e-3
    rh, rp, rl, rd, rw = R.parse_text(path)
    assert np.array_equal(desc, rd) and weight.tobytes() == rw.tobytes()


def _parse_code(orbx, path):
    n = ctypes.c_int32(0)
    return orbx.lib().orbx_vocabulary_parse_text(os.fsencode(path), None, ctypes.byref(n), None, None, None, None, 0)


@pytest.mark.parametrize("header", ["21 2  0 0", "3 0  0 0", "3 11  0 0", "3 2  6 0", "3 2  0 4", "3 2  -1 0", "3 2 0", "x 2 0 0"])
def test_bad_header_refused(orbx, tmp_path, header):
    voc = R.irregular_tree(1, k=3, L=2, n_nodes=8)
    path = str(tmp_path / "v.txt")
    R.write_text(path, voc, header_line=header)
    assert _parse_code(orbx, path) == orbx.E_BADARG


def _tree_file(tmp_path, lines, header="3 2  0 0"):
    path = str(tmp_path / "t.txt")
    with open(path, "w") as f:
        f.write(header + "\n" + "".join("%d %d %s 1.0\n" % (p, l, " ".join(["0"] * 32)) for p, l in lines))
    return path


@pytest.mark.parametrize("lines", [
    [(0, 1), (2, 1)],              # a parent id equal to the line's own
    [(0, 0), (5, 1)],              # a parent after the line
    [(0, 0), (-1, 1)],             # a negative parent
    [(0, 1)] * 4,                  # more than k = 3 children
    [(0, 0), (1, 0), (2, 1)],      # deeper than L = 2
])
def test_bad_tree_refused(orbx, tmp_path, lines):
    path = _tree_file(tmp_path, lines)
    assert _parse_code(orbx, path) == orbx.E_BADARG
    parent = np.array([p for p, _ in lines], np.int32)
    leaf = np.array([lf for _, lf in lines], np.int32)
    desc, weight = np.zeros((len(lines), 32), np.uint8), np.ones(len(lines))
    h = ctypes.c_void_p(0)
    assert orbx.lib().orbx_vocabulary_create(None, 3, 2, 0, 0, len(lines), parent.ctypes.data, leaf.ctypes.data, desc.ctypes.data,
                                             weight.ctypes.data, ctypes.byref(h)) == orbx.E_BADARG


def test_short_line_and_missing_file_refused(orbx, tmp_path):
    path = str(tmp_path / "s.txt")
    with open(path, "w") as f:
        f.write("3 2  0 0\n0 1 1 2 3\n")
    assert _parse_code(orbx, path) == orbx.E_BADARG
    assert _parse_code(orbx, str(tmp_path / "missing.txt")) == orbx.E_BADARG


def test_parse_text_capacity(orbx, tmp_path):
    voc = R.irregular_tree(2, k=3, L=3, n_nodes=20)
    path = str(tmp_path / "v.txt")
    R.write_text(path, voc)
    n = ctypes.c_int32(0)
    parent = np.zeros(5, np.int32)
    r = orbx.lib().orbx_vocabulary_parse_text(os.fsencode(path), None, ctypes.byref(n), parent.ctypes.data, None, None, None, 5)
    assert r == orbx.E_CAPACITY and n.value == len(voc.parent)


def test_create_without_device_is_e_hip(orbx):
    """No device context (orbx_create fails with ORBX_E_HIP without a GPU): a well-formed vocabulary returns ORBX_E_HIP, never a
    host computation."""
    voc = R.irregular_tree(3, k=3, L=3, n_nodes=20)
    k, L, sc, wt, parent, leaf, desc, weight = voc.arrays()
    h = ctypes.c_void_p(0)
    r = orbx.lib().orbx_vocabulary_create(None, k, L, sc, wt, len(parent), parent.ctypes.data, leaf.ctypes.data, desc.ctypes.data,
                                          weight.ctypes.data, ctypes.byref(h))
    assert r == orbx.E_HIP and not h.value


def test_shim_bow_compiles(orbx, tmp_path):
    exe = os.path.join(str(tmp_path), "shim_bow")
    libdir = os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "shim_bow.cpp"), "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
