"""ORBmatcher::SearchByBoW on the device (orbx_match_bow*): matches_f and nmatches of every pair equal the CPU restatement
(tests/cpp/match_bow_ref.cpp) bit for bit on the worlds of tests/match_bow_ref_lib.py -- two vocabularies, levelsup 0 (node =
word), 2 and L (one node of 1000 x 1000 features: the chunked path), orientation check off and on, nnratio 0.6 and 0.9, mask
absent and random -- for the batch, for every pair issued alone and for the host form; and the extract -> transform -> match
chain without a host copy."""
import os
import subprocess

import numpy as np
import pytest

import bow_ref_lib as R
import match_bow_ref_lib as M

pytestmark = pytest.mark.gpu

CAP, NF, NP = M.CAP, M.N_FRAMES, len(M.PAIRS)
KF_IDX = np.array([p[0] for p in M.PAIRS], np.int32)
F_IDX = np.array([p[1] for p in M.PAIRS], np.int32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    yield e
    e.close()


class DeviceWorld:
    """A world's frames in HBM and their FeatureVectors as the device's own transform wrote them there."""

    def __init__(self, orbx, torch, ext, w):
        self.w = w
        self.voc = orbx.Vocabulary.from_arrays(ext, *w.voc.arrays())
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
        self.kps, self.desc, self.mask = up(w.kps), up(w.desc), up(w.mask)
        self.n = torch.from_numpy(w.n).cuda()
        z = lambda dt, m: torch.zeros(m, dtype=dt, device="cuda")  # noqa: E731
        self.fv_node, self.fv_feat, self.fv_n = z(torch.int32, NF * CAP), z(torch.int32, NF * CAP), z(torch.int32, NF)
        self.voc.transform_batch_device(NF, self.desc, self.n, z(torch.int32, NF * CAP), z(torch.float64, NF * CAP), z(torch.int32, NF),
                                        self.fv_node, self.fv_feat, self.fv_n, levelsup=w.levelsup, capacity=CAP)
        torch.cuda.synchronize()

    def match(self, torch, ext, kf, f, cfg):
        """One call over the pairs (kf[p], f[p]) -> (matches_f [P, CAP] as numpy, nmatches [P]); the outputs start at -7."""
        ori, ratio, masked = cfg
        m = torch.full((len(kf) * CAP,), -7, dtype=torch.int32, device="cuda")
        nm = torch.full((len(kf),), -7, dtype=torch.int32, device="cuda")
        ext.match_bow_pairs_device(NF, kf, f, self.kps, self.desc, self.n, self.fv_node, self.fv_feat, self.fv_n, m, nm,
                                   d_kf_mask=self.mask if masked else None, nnratio=ratio, checkOri=bool(ori), capacity=CAP)
        torch.cuda.synchronize()
        return m.cpu().numpy().reshape(len(kf), CAP), nm.cpu().numpy()


@pytest.fixture(scope="module")
def worlds(orbx, torch, ext):
    made = {}

    def get(name, li):
        if (name, li) not in made:
            made[(name, li)] = DeviceWorld(orbx, torch, ext, M.world(name, li))
        return made[(name, li)]
    yield get
    for d in made.values():
        d.voc.close()


@pytest.mark.parametrize("name,li", M.WORLDS)
def test_feature_vectors_are_the_restatements(worlds, name, li):
    """What the matcher reads is what the CPU statements were given."""
    d = worlds(name, li)
    n = d.fv_n.cpu().numpy()
    node = d.fv_node.cpu().numpy().view(np.uint32).reshape(NF, CAP)
    feat = d.fv_feat.cpu().numpy().view(np.uint32).reshape(NF, CAP)
    for f in range(NF):
        assert n[f] == len(d.w.fv[f][0])
        assert np.array_equal(node[f, :n[f]], d.w.fv[f][0]) and np.array_equal(feat[f, :n[f]], d.w.fv[f][1])


@pytest.mark.parametrize("cfg", M.CONFIGS, ids=lambda c: "ori%d-r%.1f-%s" % (c[0], c[1], "mask" if c[2] else "all"))
@pytest.mark.parametrize("name,li", M.WORLDS)
def test_batch_equals_restatement(torch, ext, worlds, name, li, cfg):
    d = worlds(name, li)
    want = d.w.expected(cfg)
    got, nm = d.match(torch, ext, KF_IDX, F_IDX, cfg)
    again, nm2 = d.match(torch, ext, KF_IDX, F_IDX, cfg)
    assert got.tobytes() == again.tobytes() and nm.tobytes() == nm2.tobytes(), "two runs differ"
    for p, (a, b) in enumerate(M.PAIRS):
        nb = int(d.w.n[b])
        assert nm[p] == want[p][1], (M.PAIRS[p], int(nm[p]), want[p][1])
        assert np.array_equal(got[p, :nb], want[p][0]), M.PAIRS[p]
        assert np.all(got[p, nb:] == -7)  # (nothing is written beyond the frame's count)


@pytest.mark.parametrize("name,li", M.WORLDS)
def test_single_pairs_and_host_form_equal_the_batch(torch, ext, worlds, name, li):
    d, cfg = worlds(name, li), (1, 0.9, True)
    got, nm = d.match(torch, ext, KF_IDX, F_IDX, cfg)
    w = d.w
    for p, (a, b) in enumerate(M.PAIRS):
        nb = int(w.n[b])
        one, nm1 = d.match(torch, ext, KF_IDX[p:p + 1], F_IDX[p:p + 1], cfg)
        assert nm1[0] == nm[p] and np.array_equal(one[0, :nb], got[p, :nb]), M.PAIRS[p]
        hm, hnm = ext.match_bow(w.kps[a, :w.n[a]], w.desc[a, :w.n[a]], w.fv[a][0], w.fv[a][1], w.kps[b, :nb], w.desc[b, :nb],
                                w.fv[b][0], w.fv[b][1], kf_mask=w.mask[a, :w.n[a]], nnratio=cfg[1], checkOri=True)
        assert hnm == nm[p] and np.array_equal(hm, got[p, :nb]), M.PAIRS[p]


def test_pair_list_held_across_calls(orbx, torch):
    """The pair list lives on the device between calls with the host copy its upload read: call after call on one context of its
    own -- a first list, the same again (no upload), as many other pairs (replaced in place), one pair, three (the device array
    grows), the first list again -- every call equals the restatement.  Pairs of the small frames only."""
    cfg = (1, 0.9, True)
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    d = DeviceWorld(orbx, torch, e, M.world("irregular", 0))
    want = d.w.expected(cfg)
    try:
        two = [4, 5]  # (keyframe g, frame 12 + g) of 40 and of 150 features
        steps = (("two pairs", two), ("the same list", two), ("as many other pairs", [10, 11]), ("one pair", [3]),
                 ("three pairs", [5, 9, 10]), ("the first list again", two))
        assert not set(M.BIG_PAIRS) & {p for _, idx in steps for p in idx}
        # (a list left in place of its successor would be seen: the two lists of two expect different matches)
        assert any(not np.array_equal(want[p][0], want[q][0]) for p, q in zip(two, [10, 11]))
        for what, idx in steps:
            got, nm = d.match(torch, e, KF_IDX[idx], F_IDX[idx], cfg)
            for row, p in enumerate(idx):
                nb = int(d.w.n[M.PAIRS[p][1]])
                assert nm[row] == want[p][1] and np.array_equal(got[row, :nb], want[p][0]), (what, M.PAIRS[p])
                assert np.all(got[row, nb:] == -7), (what, M.PAIRS[p])
    finally:
        d.voc.close()
        e.close()


def test_refusals_with_a_context(orbx, torch, ext, worlds):
    d = worlds("irregular", 0)
    m, nm = torch.zeros(CAP, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    L, p = orbx.lib(), orbx._ptr

    def call(kf, f, cap):
        hk, hf = np.array([kf], np.int32), np.array([f], np.int32)  # (named: they must outlive the call)
        return L.orbx_match_bow_batch_device(ext._h, NF, 1, p(hk), p(hf), p(d.kps), p(d.desc), p(d.n), cap, p(d.fv_node), p(d.fv_feat),
                                             p(d.fv_n), None, 0.6, 1, p(m), p(nm))
    assert call(0, NF, CAP) == orbx.E_BADARG
    assert call(-1, 0, CAP) == orbx.E_BADARG
    assert call(0, 1, orbx.BOW_MAX_FEATURES + 1) == orbx.E_CAPACITY
    ext.match_bow_pairs_device(NF, np.zeros(0, np.int32), np.zeros(0, np.int32), d.kps, d.desc, d.n, d.fv_node, d.fv_feat, d.fv_n, m, nm,
                               capacity=CAP)  # no pairs: ORBX_OK
    w = d.w
    with pytest.raises(orbx.OrbxError) as e:  # the host form refuses a FeatureVector that names a feature the frame does not have
        ext.match_bow(w.kps[4, :40], w.desc[4, :40], w.fv[4][0], w.fv[4][1], w.kps[16, :20], w.desc[16, :20], w.fv[16][0], w.fv[16][1])
    assert e.value.code == orbx.E_BADARG


def test_device_form_skips_pairs_that_name_no_feature(torch, ext, worlds):
    """Counts lowered behind the transform: the FeatureVectors now name features the frames no longer have; the device form
    skips those pairs, as the restatement does."""
    d, w = worlds("full1000", 1), M.world("full1000", 1)
    n = w.n.copy()
    n[0], n[12] = 700, 650
    keep = d.n
    d.n = torch.from_numpy(n).cuda()
    try:
        got, nm = d.match(torch, ext, KF_IDX[:1], F_IDX[:1], (1, 0.9, False))
    finally:
        d.n = keep
    m, want_nm, _ = M.search_by_bow((w.kps["angle"][0, :700], w.desc[0, :700], w.fv[0][0], w.fv[0][1]),
                                    (w.kps["angle"][12, :650], w.desc[12, :650], w.fv[12][0], w.fv[12][1]), None, 0.9, True)
    assert nm[0] == want_nm and np.array_equal(got[0, :650], m) and want_nm > 50


def test_extract_transform_match_chain(orbx, torch, images, golden):
    """Two golden images, one a shifted copy of the other: extract_batch_device, transform_batch_device and
    match_bow_pairs_device on the same device arrays with no host copy in between; the arrays are downloaded once afterwards
    and fed to the restatement."""
    a = images["dbow0"]
    b = np.roll(a, (3, 5), axis=(0, 1))
    h, wd = a.shape
    cap, B = 1024, 2
    base = R.full_vocabulary(golden["canonical/dbow0/desc"], k=10, L=3)
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=wd, max_height=h, max_batch=B, device=0)
    voc = orbx.Vocabulary.from_arrays(e, *base.arrays())
    z = lambda dt, m: torch.zeros(m, dtype=dt, device="cuda")  # noqa: E731
    d_img = torch.from_numpy(np.stack([a, b])).cuda()
    d_k, d_d, d_n = z(torch.uint8, B * cap * 28), z(torch.uint8, B * cap * 32), z(torch.int32, B)
    fv_node, fv_feat, fv_n = z(torch.int32, B * cap), z(torch.int32, B * cap), z(torch.int32, B)
    m, nm = torch.full((2 * cap,), -7, dtype=torch.int32, device="cuda"), z(torch.int32, 2)
    e.extract_batch_device(d_img, B, wd, h, wd, wd * h, d_k, d_d, d_n, cap)
    voc.transform_batch_device(B, d_d, d_n, z(torch.int32, B * cap), z(torch.float64, B * cap), z(torch.int32, B), fv_node, fv_feat, fv_n,
                               levelsup=2, capacity=cap)
    e.match_bow_pairs_device(B, np.array([0, 1], np.int32), np.array([1, 0], np.int32), d_k, d_d, d_n, fv_node, fv_feat, fv_n, m, nm,
                             nnratio=0.7, checkOri=True, capacity=cap)
    torch.cuda.synchronize()
    kps = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap)
    desc, n = d_d.cpu().numpy().reshape(B, cap, 32), d_n.cpu().numpy()
    node, feat = fv_node.cpu().numpy().view(np.uint32).reshape(B, cap), fv_feat.cpu().numpy().view(np.uint32).reshape(B, cap)
    fvn, got, gnm = fv_n.cpu().numpy(), m.cpu().numpy().reshape(2, cap), nm.cpu().numpy()
    side = lambda f: (kps["angle"][f, :n[f]], desc[f, :n[f]], node[f, :fvn[f]], feat[f, :fvn[f]])  # noqa: E731
    for p, (x, y) in enumerate(((0, 1), (1, 0))):
        want, wnm, _ = M.search_by_bow(side(x), side(y), None, 0.7, True)
        assert gnm[p] == wnm and np.array_equal(got[p, :n[y]], want)
        assert wnm >= 50, wnm  # a shifted copy: the chain found real matches
    voc.close()
    e.close()


def test_shim_match_bow_compiles_and_runs(orbx, ext, tmp_path):
    """tests/cpp/shim_match_bow.cpp, a relocaliser's call sequence over include/orbx_shim.hpp's ORBmatcher::SearchByBoW (the
    -DORBX_WITH_OPENCV branch against the mock OpenCV headers): it returns what the C call returns."""
    exe, libdir = os.path.join(str(tmp_path), "shim_match_bow"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DORBX_WITH_OPENCV", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "tests", "cpp", "mock_opencv"), os.path.join(ROOT, "tests", "cpp", "shim_match_bow.cpp"), "-L", libdir,
           "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    w = M.world("full1000", 1)
    a, b = 5, 17  # 150 features each
    na, nb = int(w.n[a]), int(w.n[b])
    paths = {k: str(tmp_path / (k + ".bin")) for k in ("kd", "ka", "km", "fd", "fa")}
    w.desc[a, :na].tofile(paths["kd"])
    w.kps["angle"][a, :na].astype(np.float32).tofile(paths["ka"])
    w.mask[a, :na].tofile(paths["km"])
    w.desc[b, :nb].tofile(paths["fd"])
    w.kps["angle"][b, :nb].astype(np.float32).tofile(paths["fa"])
    voc_path = str(tmp_path / "voc.txt")
    R.write_text(voc_path, w.voc)
    p = subprocess.run([exe, voc_path, paths["kd"], paths["ka"], paths["km"], paths["fd"], paths["fa"], str(w.levelsup)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    lines = p.stdout.strip().splitlines()
    hm, hnm = ext.match_bow(w.kps[a, :na], w.desc[a, :na], w.fv[a][0], w.fv[a][1], w.kps[b, :nb], w.desc[b, :nb], w.fv[b][0], w.fv[b][1],
                            kf_mask=w.mask[a, :na], nnratio=0.6, checkOri=True)
    assert lines[0] == "RESULT %d" % hnm and hnm > 10
    assert [int(v) for v in lines[1].split()] == hm.tolist()
