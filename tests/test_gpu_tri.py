"""LocalMapping::CreateNewMapPoints on the device (orbx_match_triangulation*, orbx_triangulate_matches*): the match rows, every
field of both result records and every output array equal the CPU restatement (tests/cpp/tri_ref.cpp) byte for byte on the worlds
of tests/tri_ref_lib.py -- issued alone and chained, in one batch whose pairs share frames, on the hand-made order cases inside a
node that crosses a lane-chunk boundary, on the empty shapes and on garbage -- through the host forms, the Python classes and the
shim; and the output row is a point set the relocalisation SearchByProjection accepts as it is."""
import os
import subprocess

import numpy as np
import pytest

import match_kfproj_ref_lib as KP
import tri_ref_lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KPD = L.KEYPOINT_DTYPE


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    assert np.asarray(e.GetScaleFactors(), np.float32).tobytes() == L.scale_table().tobytes()
    assert np.asarray(e.GetScaleSigmaSquares(), np.float32).tobytes() == L.sigma2_table().tobytes()
    yield e
    e.close()


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


class Batch:
    """Keyframes and pairs in the device layout.  frames: [KeyFrame]; pairs: [(kf1, kf2)]; n / fv_n: the counts the device is told
    (default the true ones); median: [n_frames] or None."""

    def __init__(self, torch, frames, pairs, cap, n=None, fv_n=None, median=None, scale_factor=L.SCALE_FACTOR, nlevels=L.NLEVELS):
        self.scale_factor, self.nlevels = scale_factor, nlevels  # (the pyramid of the context the batch runs on: the restatement's tables)
        self.torch, self.frames, self.pairs, self.cap, self.F, self.P = torch, frames, pairs, cap, len(frames), len(pairs)
        F, P = self.F, self.P
        kps, desc = np.zeros((F, cap), KPD), np.zeros((F, cap, 32), np.uint8)
        node, feat = np.zeros((F, cap), np.uint32), np.zeros((F, cap), np.uint32)
        mask, pose = np.zeros((F, cap), np.uint8), np.zeros((F, 12), np.float32)
        for f, k in enumerate(frames):
            kps[f, :k.n], desc[f, :k.n], pose[f] = k.kps, k.desc, k.pose
            node[f, :len(k.fv_node)], feat[f, :len(k.fv_feat)] = k.fv_node, k.fv_feat
            if k.mask is not None:
                mask[f, :k.n] = k.mask
        self.n = np.array([k.n for k in frames], np.int32) if n is None else np.asarray(n, np.int32)
        self.fv_n = np.array([len(k.fv_node) for k in frames], np.int32) if fv_n is None else np.asarray(fv_n, np.int32)
        self.median = None if median is None else np.asarray(median, np.float32)
        self.d_kps, self.d_desc, self.d_node, self.d_feat, self.d_pose = (up(torch, a) for a in (kps, desc, node, feat, pose))
        self.d_n, self.d_fv_n = up(torch, self.n), up(torch, self.fv_n)
        self.d_mask = up(torch, mask) if any(k.mask is not None for k in frames) else None
        self.d_median = None if median is None else up(torch, self.median)
        self.kf1, self.kf2 = (np.array([p[k] for p in pairs], np.int32) for k in range(2))
        q = max(P, 1)
        self.m12 = torch.empty(q * cap, dtype=torch.int32, device="cuda")
        self.mres = torch.empty(q * L.MATCH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self.pts = torch.empty(q * cap * 3, dtype=torch.float32, device="cuda")
        self.msk = torch.empty(q * cap, dtype=torch.uint8, device="cuda")
        self.nrm = torch.empty(q * cap * 3, dtype=torch.float32, device="cuda")
        self.dst = torch.empty(q * cap * 2, dtype=torch.float32, device="cuda")
        self.tres = torch.empty(q * L.TRI_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

    def _poison(self, *arrays):
        for a in arrays:
            a.fill_(-7 if a.dtype != self.torch.uint8 else 0xA5)

    def match(self, ext, K, ori=True):
        self._poison(self.m12, self.mres)
        ext.match_triangulation_pairs_device(self.F, self.kf1, self.kf2, self.d_kps, self.d_desc, self.d_n, self.d_node, self.d_feat,
                                             self.d_fv_n, self.d_pose, K, self.m12, self.mres, d_mask=self.d_mask,
                                             d_median_depth=self.d_median, checkOri=ori, capacity=self.cap)
        return self.match_out()

    def match_out(self):
        self.torch.cuda.synchronize()
        return (self.m12.cpu().numpy().reshape(-1, self.cap)[:self.P],
                self.mres.cpu().numpy().view(L.MATCH_RESULT_DTYPE)[:self.P])

    def triangulate(self, ext, K, m12=None):
        if m12 is not None:
            self.m12.copy_(up(self.torch, np.ascontiguousarray(m12, np.int32)).view(self.torch.int32))
        self._poison(self.pts, self.msk, self.nrm, self.dst, self.tres)
        ext.triangulate_matches_pairs_device(self.F, self.kf1, self.kf2, self.d_kps, self.d_n, self.d_pose, K, self.m12, self.pts, self.msk,
                                             self.nrm, self.dst, self.tres, capacity=self.cap)
        return self.tri_out()

    def tri_out(self):
        self.torch.cuda.synchronize()
        c, P = self.cap, self.P
        return dict(points=self.pts.cpu().numpy().reshape(-1, c, 3)[:P], mask=self.msk.cpu().numpy().reshape(-1, c)[:P],
                    normal=self.nrm.cpu().numpy().reshape(-1, c, 3)[:P], dist=self.dst.cpu().numpy().reshape(-1, c, 2)[:P],
                    res=self.tres.cpu().numpy().view(L.TRI_RESULT_DTYPE)[:P])

    def chain(self, ext, K, ori=True):
        self._poison(self.m12, self.mres, self.pts, self.msk, self.nrm, self.dst, self.tres)
        ext.create_new_map_points_pairs_device(self.F, self.kf1, self.kf2, self.d_kps, self.d_desc, self.d_n, self.d_node, self.d_feat,
                                               self.d_fv_n, self.d_pose, K, self.m12, self.mres, self.pts, self.msk, self.nrm, self.dst,
                                               self.tres, d_mask=self.d_mask, d_median_depth=self.d_median, checkOri=ori,
                                               capacity=self.cap)
        return self.match_out(), self.tri_out()

    def world_of(self, p, K, ori=True):
        f1, f2 = self.pairs[p]
        return L.World(self.frames[f1], self.frames[f2], K, ori=ori, median=None if self.median is None else float(self.median[f2]),
                       scale_factor=self.scale_factor, nlevels=self.nlevels)

    def expect_match(self, p, K, ori=True):
        f1, f2 = self.pairs[p]
        return L.search(self.world_of(p, K, ori), cap=self.cap, n1=int(self.n[f1]), n2=int(self.n[f2]), fvn1=int(self.fv_n[f1]),
                        fvn2=int(self.fv_n[f2]))

    def expect_tri(self, p, K, m12):
        f1, f2 = self.pairs[p]
        return L.triangulate(self.world_of(p, K), m12, cap=self.cap, n1=int(self.n[f1]), n2=int(self.n[f2]))


def check_match(b, got, K, ori=True, what=""):
    rows, res = got
    out = []
    for p in range(b.P):
        e = b.expect_match(p, K, ori)
        print(what, p, "device", res[p], "restatement", e["res"])
        assert rows[p].tobytes() == e["matches12"].tobytes(), (what, p)
        assert res[p].tobytes() == e["res"].tobytes(), (what, p, res[p], e["res"])
        out.append(e)
    return out


def check_tri(b, got, K, rows, what=""):
    out = []
    for p in range(b.P):
        e = b.expect_tri(p, K, rows[p])
        print(what, p, "device", got["res"][p], "restatement", e["res"])
        assert got["res"][p].tobytes() == e["res"].tobytes(), (what, p, got["res"][p], e["res"])
        for f in ("mask", "points", "normal", "dist"):
            assert got[f][p].tobytes() == e[f].tobytes(), (what, p, f)
        assert np.isfinite(got["points"][p]).all() and np.isfinite(got["normal"][p]).all() and np.isfinite(got["dist"][p]).all()
        out.append(e)
    return out


# ---- the second setting (pose_ref_lib.SECOND): fx != fy, a context of 5 levels of 1.37 (both calls read the context's tables),
# KF2 rolled by 89 degrees ----

@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, L.SCALE_FACTOR_2, L.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    assert np.asarray(e.GetScaleFactors(), np.float32).tobytes() == L.scale_table(L.NLEVELS_2, L.SCALE_FACTOR_2).tobytes()
    assert np.asarray(e.GetScaleSigmaSquares(), np.float32).tobytes() == L.sigma2_table(L.NLEVELS_2, L.SCALE_FACTOR_2).tobytes()
    yield e
    e.close()


def second_setting_worlds():
    """Two pairs whose first keyframes hold 150 and 310 features: a quiet one, and one with near points, pixel noise of a level's
    scale and octaves up to four levels apart (every gate of the triangulation rejects some)."""
    two = dict(rot2=L.ROLL_2, **L.SECOND)
    return [L.make_world(211, n_points=120, n_random=30, n_distract=15, **two),
            L.make_world(212, n_points=280, n_random=30, n_distract=30, noise=1.0, depth=(1.5, 6.0), octave_jitter=0.5, octave_spread=4,
                         centre2=(0.5, 0.1, 0.3), **two)]


def test_second_setting_anisotropic_camera_and_five_levels(torch, ext2):
    """SearchForTriangulation and the triangulation on both pairs in one batch at the capacity of the largest count, each call
    alone and chained; then both host forms on the smaller pair."""
    ws = second_setting_worlds()
    K = ws[0].K
    assert ws[0].kf1.n == 150 and ws[1].kf1.n == 310 and K.tobytes() == L.K_ANISO.reshape(9).tobytes()
    cap = max(k.n for w in ws for k in (w.kf1, w.kf2))
    b = Batch(torch, [ws[0].kf1, ws[0].kf2, ws[1].kf1, ws[1].kf2], [(0, 1), (2, 3)], cap, scale_factor=L.SCALE_FACTOR_2, nlevels=L.NLEVELS_2)
    got = b.match(ext2, K)
    e = check_match(b, got, K, True, "second setting")
    tri = b.triangulate(ext2, K)
    t = check_tri(b, tri, K, got[0], "second setting")
    (rows2, res2), tri2 = b.chain(ext2, K)
    assert rows2.tobytes() == got[0].tobytes() and res2.tobytes() == got[1].tobytes()
    for f in tri:
        assert tri2[f].tobytes() == tri[f].tobytes(), f
    for p, w in enumerate(ws):  # not trivial: matches found, candidates rejected by the epipolar line, points kept
        assert e[p]["matches12"][:w.kf1.n].tobytes() == w.expected()["match"]["matches12"][:w.kf1.n].tobytes()
        assert got[1][p]["status"] == 0 and got[1][p]["nmatches"] > 0.7 * len(w.truth) and got[1][p]["n_epiline_rejected"] > 5
        assert tri["res"][p]["status"] == 0 and tri["res"][p]["n_points"] > 0.6 * len(w.truth)
    assert tri["res"][1]["n_matches"] - tri["res"][1]["n_points"] > 5  # (the second pair's gates reject)
    w, x = ws[0], ws[0].expected()
    T1, T2 = np.c_[w.kf1.pose[:9].reshape(3, 3), w.kf1.pose[9:]], np.c_[w.kf2.pose[:9].reshape(3, 3), w.kf2.pose[9:]]
    m12, res = ext2.match_triangulation(w.kf1.kps, w.kf1.desc, w.kf1.fv_node, w.kf1.fv_feat, T1, w.kf2.kps, w.kf2.desc, w.kf2.fv_node,
                                        w.kf2.fv_feat, T2, w.K)
    assert m12.tobytes() == x["match"]["matches12"][:w.kf1.n].tobytes() and bytes(res) == x["match"]["res"].tobytes()
    pts, msk, nrm, dst, tres = ext2.triangulate_matches(w.kf1.kps, T1, w.kf2.kps, T2, w.K, m12)
    tt, n1 = x["tri"], w.kf1.n
    assert bytes(tres) == tt["res"].tobytes() and msk.tobytes() == tt["mask"][:n1].tobytes() and pts.tobytes() == tt["points"][:n1].tobytes()
    assert nrm.tobytes() == tt["normal"][:n1].tobytes() and dst.tobytes() == tt["dist"][:n1].tobytes()


def batch_of(torch, w, cap):
    return Batch(torch, [w.kf1, w.kf2], [(0, 1)], cap, median=None if w.median is None else [0.0, w.median])


@pytest.mark.parametrize("name", L.WORLDS)
def test_world_equals_restatement(torch, ext, name):
    """Each call alone, then the chain: the same bytes; two runs agree.  dense: more than 256 matches (k_triangulate's workgroups
    past the first); big_node: the chunked path; small_nodes: more nodes than waves."""
    w = L.world(name)
    b = batch_of(torch, w, 704 if name == "dense" else 320)
    got = b.match(ext, w.K, w.ori)
    e = check_match(b, got, w.K, w.ori, name)
    assert e[0]["matches12"][:w.kf1.n].tobytes() == w.expected()["match"]["matches12"][:w.kf1.n].tobytes()
    tri = b.triangulate(ext, w.K)
    check_tri(b, tri, w.K, got[0], name)
    (rows2, res2), tri2 = b.chain(ext, w.K, w.ori)
    assert rows2.tobytes() == got[0].tobytes() and res2.tobytes() == got[1].tobytes(), "the chain's matcher differs from the call alone"
    for f in tri:
        assert tri2[f].tobytes() == tri[f].tobytes(), ("the chain differs from the two calls run apart", f)
    assert int(tri["res"][0]["n_points"]) > 0
    if name == "dense":
        assert int(got[1][0]["nmatches"]) > 256
    # without the orientation test
    check_match(b, b.match(ext, w.K, False), w.K, False, name + " no-ori")


H = L.hand_desc
C2 = (0.0, 0.0, 1.0)


def _both(X, desc2=(), node=5):
    (x1, y1), (x2, y2) = L.project(L.K_POW2, (0, 0, 0), X), L.project(L.K_POW2, C2, X)
    return (x1, y1, 0, 0.0, H([]), node), (x2, y2, 0, 0.0, H(desc2), node)


def _filler(k):
    """A KF2 feature of node 5 that no query comes near in Hamming distance."""
    return (40.0 + k, 30.0, 0, 0.0, H(range(60, 200)), 5)


def _padded(cands):
    """KF2's node 5 with the candidates at positions 62, 64, 70 and 71 (either side of the 64-lane chunk), fillers between."""
    at = dict(zip((62, 64, 70, 71), cands))
    return [at.get(k, _filler(k)) for k in range(80)]


def test_tie_and_taken_across_a_lane_chunk_boundary(torch, ext):
    s = lambda k: (0.5 * k, 0.0, 4.0 * k)  # noqa: E731  (points on KF1's ray through (320, 256))
    a, c1 = _both(s(1.0), desc2=[0, 1, 2, 3])
    _, c0 = _both(s(0.75), desc2=[4, 5, 6, 7])
    _, c2 = _both(s(1.5), desc2=[8, 9, 10, 11])
    _, c3 = _both(s(2.0), desc2=range(6))
    tie = L.hand_world([a], _padded([c0, c1, c2, c3]))
    b = batch_of(torch, tie, 96)
    got = b.match(ext, tie.K, False)
    check_match(b, got, tie.K, False, "tie")
    assert got[0][0, 0] == 70  # (62, 64 and 70 at distance 4: the last one, in the second chunk)
    _, j0 = _both(s(1.0), desc2=[0, 1])
    _, j1 = _both(s(1.5), desc2=range(8))
    taken = L.hand_world([a, a, a], _padded([j1, j0, _filler(70), _filler(71)]))
    b = batch_of(torch, taken, 96)
    got = b.match(ext, taken.K, False)
    check_match(b, got, taken.K, False, "taken")
    assert got[0][0, :3].tolist() == [64, 62, -1]
    # the same two cases in a node of four KF2 features: the path that keeps the node in registers, one feature per lane
    small = L.hand_world([a], [c0, c1, c2, c3])
    b = batch_of(torch, small, 8)
    got = b.match(ext, small.K, False)
    check_match(b, got, small.K, False, "tie, one per lane")
    assert got[0][0, 0] == 2
    small = L.hand_world([a, a, a], [j1, j0])
    b = batch_of(torch, small, 8)
    got = b.match(ext, small.K, False)
    check_match(b, got, small.K, False, "taken, one per lane")
    assert got[0][0, :3].tolist() == [1, 0, -1]


def _empty_kf(pose):
    return L.KeyFrame(np.zeros(0, KPD), np.zeros((0, 32), np.uint8), [], [], pose)


def test_empty_shapes(torch, ext):
    """0 features, 1 feature, an empty FeatureVector, no common node."""
    w = L.world("small_nodes")
    one = lambda k: L.KeyFrame(k.kps[:1], k.desc[:1], [5], [0], k.pose)  # noqa: E731
    no_fv = L.KeyFrame(w.kf2.kps, w.kf2.desc, [], [], w.kf2.pose)
    apart = L.KeyFrame(w.kf2.kps, w.kf2.desc, w.kf2.fv_node + 100000, w.kf2.fv_feat, w.kf2.pose)
    frames = [w.kf1, w.kf2, _empty_kf(w.kf1.pose), _empty_kf(w.kf2.pose), one(w.kf1), one(w.kf2), no_fv, apart]
    b = Batch(torch, frames, [(2, 3), (2, 1), (0, 3), (4, 5), (0, 6), (0, 7), (6, 1)], 320)
    (rows, res), tri = b.chain(ext, w.K)
    check_match(b, (rows, res), w.K, True, "empty")
    check_tri(b, tri, w.K, rows, "empty")
    assert not (rows[[0, 1, 2, 4, 5, 6]] >= 0).any()
    # no pairs at all: nothing is written
    z = Batch(torch, frames, [], 320)
    (rows, res), tri = z.chain(ext, w.K)
    assert len(rows) == 0 and (z.m12.cpu().numpy() == -7).all()


def test_pairs_that_share_frames_and_a_pair_with_itself(torch, ext):
    """A frame as KF1 in three pairs and as KF2 in another, plus a pair with itself: zero baseline, all rejected, nothing non-finite
    written (also when the triangulation is handed every feature matched to itself)."""
    s, g, f = L.world("small_nodes"), L.world("big_node"), L.world("forward")
    frames = [s.kf1, s.kf2, g.kf2, f.kf2]
    b = Batch(torch, frames, [(0, 1), (0, 2), (0, 3), (1, 0), (0, 0)], 320)
    (rows, res), tri = b.chain(ext, s.K)
    check_match(b, (rows, res), s.K, True, "shared")
    check_tri(b, tri, s.K, rows, "shared")
    assert int(res[4]["status"]) == L.ZERO_BASELINE and (rows[4] == -1).all() and np.isfinite(res[4]["F12"]).all()
    assert int(res[0]["nmatches"]) > 64 and int(res[3]["nmatches"]) > 64
    ident = rows.copy()
    ident[4, :s.kf1.n] = np.arange(s.kf1.n)
    tri = b.triangulate(ext, s.K, ident)
    check_tri(b, tri, s.K, ident, "identity")
    assert int(tri["res"][4]["n_matches"]) == s.kf1.n and int(tri["res"][4]["n_points"]) == 0 and not tri["mask"][4].any()


def test_garbage_is_flagged_and_not_followed(torch, ext):
    """A non-finite pose, counts beyond the capacity and below zero, an octave outside the pyramid, matches beyond KF2's count."""
    w = L.world("small_nodes")
    nan_pose = w.kf2.pose.copy()
    nan_pose[4] = np.inf
    broken = L.KeyFrame(w.kf2.kps, w.kf2.desc, w.kf2.fv_node, w.kf2.fv_feat, nan_pose)
    deep = w.kf2.kps.copy()
    deep["octave"][::3] = 11
    deep["octave"][1::7] = -1
    octaves = L.KeyFrame(deep, w.kf2.desc, w.kf2.fv_node, w.kf2.fv_feat, w.kf2.pose)
    frames = [w.kf1, w.kf2, broken, octaves]
    b = Batch(torch, frames, [(0, 2), (2, 0), (0, 3), (3, 0)], 320)
    (rows, res), tri = b.chain(ext, w.K)
    em = check_match(b, (rows, res), w.K, True, "garbage")
    check_tri(b, tri, w.K, rows, "garbage")
    assert int(res[0]["status"]) == L.NONFINITE and int(tri["res"][1]["status"]) == L.NONFINITE and not tri["mask"][:2].any()
    assert int(res[2]["status"]) == L.BAD_INPUT and int(em[2]["res"]["nmatches"]) > 0
    wild = rows.copy()
    wild[3, :5] = [400, 2 ** 30, w.kf1.n, 0, -5]
    tri = b.triangulate(ext, w.K, wild)
    check_tri(b, tri, w.K, wild, "wild matches")
    assert int(tri["res"][3]["status"]) & L.BAD_INPUT
    # counts the arrays do not hold: clamped to the capacity and flagged; the features that exist still match
    c = Batch(torch, [w.kf1, w.kf2], [(0, 1), (1, 0)], 320, n=[400, w.kf2.n])
    (rows, res), tri = c.chain(ext, w.K)
    check_match(c, (rows, res), w.K, True, "counts above")
    check_tri(c, tri, w.K, rows, "counts above")
    assert all(int(r["status"]) == L.BAD_INPUT for r in res) and all(int(r["status"]) == L.BAD_INPUT for r in tri["res"])
    assert rows[0][:w.kf1.n].tobytes() == w.expected()["match"]["matches12"][:w.kf1.n].tobytes()
    c = Batch(torch, [w.kf1, w.kf2], [(0, 1), (1, 0)], 320, n=[w.kf1.n, -4], fv_n=[-3, len(w.kf2.fv_node)])
    (rows, res), tri = c.chain(ext, w.K)
    check_match(c, (rows, res), w.K, True, "counts below")
    check_tri(c, tri, w.K, rows, "counts below")
    assert all(int(r["status"]) == L.BAD_INPUT for r in res) and not (rows >= 0).any()


def test_median_depth_gate(torch, ext):
    w = L.world("small_nodes")
    base = float(w.expected()["match"]["res"]["baseline"])
    b = Batch(torch, [w.kf1, w.kf2], [(0, 1), (1, 0)], 320, median=[base / 0.02, base / 0.005])
    got = b.match(ext, w.K)
    check_match(b, got, w.K, True, "median")
    assert int(got[1][0]["status"]) == L.LOW_BASELINE and (got[0][0] == -1).all() and int(got[1][1]["status"]) == 0 and int(got[1][1]["nmatches"]) > 0
    # medians that are no positive finite numbers: flagged, matched without the gate
    clean = got[0][1].copy()
    for bad in (0.0, -2.0, np.nan, np.inf):
        b = Batch(torch, [w.kf1, w.kf2], [(1, 0)], 320, median=[bad, 1.0])
        got = b.match(ext, w.K)
        check_match(b, got, w.K, True, "median %r" % bad)
        assert int(got[1][0]["status"]) == L.BAD_INPUT and got[0][0].tobytes() == clean.tobytes()


def test_output_row_is_a_point_set_for_the_keyframe_projection_matcher(torch, ext):
    """The chain's row, untouched on the device, as d_points / d_point_mask / d_point_dist of
    orbx_match_keyframe_projection_batch_device with KF1 as the keyframe and KF2 as the lost frame: accepted, and equal to that
    call's own restatement on the same arrays."""
    w = L.world("small_nodes")
    cap = 320
    b = batch_of(torch, w, cap)
    (rows, res), tri = b.chain(ext, w.K)
    assert int(tri["res"][0]["n_points"]) > 100
    matches = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    kres = torch.empty(len(KP.RESULT_FIELDS), dtype=torch.int32, device="cuda")
    pose2 = up(torch, w.kf2.pose)
    ext.match_keyframe_projection_pairs_device(2, [0], [1], [0], b.d_kps, b.d_desc, b.d_n, 1, b.pts, b.msk, b.dst, pose2, w.K, KP.BOUNDS,
                                               matches, kres, th=10.0, ORBdist=100, checkOri=True, capacity=cap)
    torch.cuda.synchronize()
    n1 = w.kf1.n
    kw = KP.World(w.kf1.kps, w.kf1.desc, w.kf2.kps, w.kf2.desc, tri["points"][0][:n1], tri["dist"][0][:n1], tri["mask"][0][:n1], w.kf2.pose,
                  w.K, th=10.0, orb_dist=100, ori=True)
    e = kw.expected()
    got = dict(zip(KP.RESULT_FIELDS, (int(v) for v in kres.cpu().numpy())))
    print("keyframe projection over the new points", got)
    assert matches.cpu().numpy()[:w.kf2.n].tobytes() == e["matches"].tobytes()
    for f in KP.COMPARED_FIELDS:
        assert got[f] == e["res"][f], f
    # the points project back onto the features they were made from
    m = matches.cpu().numpy()[:w.kf2.n]
    made = np.flatnonzero(tri["mask"][0][:n1])
    back = sum(1 for i in made if m[rows[0][i]] == i)
    assert got["status"] == 0 and back > 0.9 * len(made)


@pytest.mark.parametrize("li", [1, 2])
def test_feature_vectors_from_the_device_transform(orbx, torch, ext, li):
    """The path from the vocabulary into the matcher: the frames of tests/match_bow_ref_lib.py's full1000 world, their FeatureVectors
    written by Vocabulary.transform_batch_device at levelsup 2 (intermediate nodes) and at levelsup = L (one node per frame, of nearly all its 1000,
    150 or 40 features: the chunked path) and read by the matcher where they lie, under poses of this file's own; rows, records and points
    equal the restatement on the downloaded FeatureVectors."""
    import match_bow_ref_lib as M
    w = M.world("full1000", li)
    NF, CAP = M.N_FRAMES, M.CAP
    voc = orbx.Vocabulary.from_arrays(ext, *w.voc.arrays())
    z = lambda dt, m: torch.zeros(m, dtype=dt, device="cuda")  # noqa: E731
    kps = w.kps.copy()
    kps["octave"] = np.arange(CAP)[None, :] % L.NLEVELS
    d_kps, d_desc, d_n = up(torch, kps), up(torch, w.desc), torch.from_numpy(w.n).cuda()
    fv_node, fv_feat, fv_n = z(torch.int32, NF * CAP), z(torch.int32, NF * CAP), z(torch.int32, NF)
    voc.transform_batch_device(NF, d_desc, d_n, z(torch.int32, NF * CAP), z(torch.float64, NF * CAP), z(torch.int32, NF), fv_node, fv_feat,
                               fv_n, levelsup=w.levelsup, capacity=CAP)
    s = L.world("small_nodes")
    pose = np.stack([s.kf1.pose if f < M.N_KF else s.kf2.pose for f in range(NF)])
    pairs = [(0, 12), (5, 17), (4, 16), (12, 0), (5, 12), (1, 13), (2, 14)]  # 1000, 150, 40 features; mixed; empty; one feature
    kf1, kf2 = (np.array([p[k] for p in pairs], np.int32) for k in range(2))
    P = len(pairs)
    m12, mres = z(torch.int32, P * CAP), z(torch.uint8, P * L.MATCH_RESULT_DTYPE.itemsize)
    pts, msk, nrm, dst = z(torch.float32, P * CAP * 3), z(torch.uint8, P * CAP), z(torch.float32, P * CAP * 3), z(torch.float32, P * CAP * 2)
    tres = z(torch.uint8, P * L.TRI_RESULT_DTYPE.itemsize)
    ext.create_new_map_points_pairs_device(NF, kf1, kf2, d_kps, d_desc, d_n, fv_node, fv_feat, fv_n, up(torch, pose), s.K, m12, mres, pts, msk,
                                           nrm, dst, tres, capacity=CAP)
    torch.cuda.synchronize()
    voc.close()
    node, feat, fvn = fv_node.cpu().numpy().view(np.uint32).reshape(NF, CAP), fv_feat.cpu().numpy().view(np.uint32).reshape(NF, CAP), fv_n.cpu().numpy()
    frames = [L.KeyFrame(kps[f, :w.n[f]], w.desc[f, :w.n[f]], node[f, :fvn[f]], feat[f, :fvn[f]], pose[f]) for f in range(NF)]
    if li == 2:
        assert len(np.unique(frames[0].fv_node)) == 1 and len(frames[0].fv_node) > 900 and 130 < len(frames[5].fv_node) <= 150
    rows, res = m12.cpu().numpy().reshape(P, CAP), mres.cpu().numpy().view(L.MATCH_RESULT_DTYPE)
    got_t = dict(points=pts.cpu().numpy().reshape(P, CAP, 3), mask=msk.cpu().numpy().reshape(P, CAP), normal=nrm.cpu().numpy().reshape(P, CAP, 3),
                 dist=dst.cpu().numpy().reshape(P, CAP, 2), res=tres.cpu().numpy().view(L.TRI_RESULT_DTYPE))
    total = 0
    for p, (f1, f2) in enumerate(pairs):
        wd = L.World(frames[f1], frames[f2], s.K)
        e = L.search(wd, cap=CAP)
        print(li, p, "device", res[p], "restatement", e["res"])
        assert rows[p].tobytes() == e["matches12"].tobytes() and res[p].tobytes() == e["res"].tobytes(), (li, p)
        t = L.triangulate(wd, rows[p], cap=CAP)
        assert got_t["res"][p].tobytes() == t["res"].tobytes(), (li, p)
        for f in ("mask", "points", "normal", "dist"):
            assert got_t[f][p].tobytes() == t[f].tobytes(), (li, p, f)
        total += int(res[p]["n_with_candidates"])
    assert total > 500  # (the frames' descriptors are near copies: the geometric tests decide)


def test_host_forms_and_python_classes(orbx, ext):
    w = L.world("mixed")
    e = w.expected()
    T1, T2 = np.c_[w.kf1.pose[:9].reshape(3, 3), w.kf1.pose[9:]], np.c_[w.kf2.pose[:9].reshape(3, 3), w.kf2.pose[9:]]  # (Tcw, 3x4)
    m12, res = ext.match_triangulation(w.kf1.kps, w.kf1.desc, w.kf1.fv_node, w.kf1.fv_feat, T1, w.kf2.kps, w.kf2.desc, w.kf2.fv_node,
                                       w.kf2.fv_feat, T2, w.K)
    assert m12.tobytes() == e["match"]["matches12"][:w.kf1.n].tobytes()
    assert bytes(res) == e["match"]["res"].tobytes()
    pts, msk, nrm, dst, tres = ext.triangulate_matches(w.kf1.kps, T1, w.kf2.kps, T2, w.K, m12)
    t, n1 = e["tri"], w.kf1.n
    assert bytes(tres) == t["res"].tobytes() and msk.tobytes() == t["mask"][:n1].tobytes() and pts.tobytes() == t["points"][:n1].tobytes()
    assert nrm.tobytes() == t["normal"][:n1].tobytes() and dst.tobytes() == t["dist"][:n1].tobytes()
    # masks and the gate through the host form
    mw = L.world("masked")
    m12, res = ext.match_triangulation(mw.kf1.kps, mw.kf1.desc, mw.kf1.fv_node, mw.kf1.fv_feat, T1, mw.kf2.kps, mw.kf2.desc, mw.kf2.fv_node,
                                       mw.kf2.fv_feat, np.c_[mw.kf2.pose[:9].reshape(3, 3), mw.kf2.pose[9:]], mw.K, mask1=mw.kf1.mask,
                                       mask2=mw.kf2.mask)
    assert m12.tobytes() == mw.expected()["match"]["matches12"][:mw.kf1.n].tobytes() and bytes(res) == mw.expected()["match"]["res"].tobytes()
    _, res = ext.match_triangulation(w.kf1.kps, w.kf1.desc, w.kf1.fv_node, w.kf1.fv_feat, T1, w.kf2.kps, w.kf2.desc, w.kf2.fv_node,
                                     w.kf2.fv_feat, T2, w.K, median_depth2=1000.0)
    assert res.status == orbx.TRI_LOW_BASELINE
    # ORBmatcher.SearchForTriangulation over Frames with a FeatureVector
    frames = []
    for k in (w.kf1, w.kf2):
        fr = orbx.Frame.from_arrays(k.kps, k.desc, (0, 640, 0, 480))
        for nd, ft in zip(k.fv_node.tolist(), k.fv_feat.tolist()):
            fr.mFeatVec.setdefault(nd, []).append(ft)
        fr._bow_computed = True
        frames.append(fr)
    nm, pairs, res = orbx.ORBmatcher(0.6, True, extractor=ext).SearchForTriangulation(frames[0], frames[1], T1, T2, K=w.K.reshape(3, 3))
    want = e["match"]["matches12"][:n1]
    assert nm == int((want >= 0).sum()) and pairs[:, 0].tolist() == np.flatnonzero(want >= 0).tolist() and pairs[:, 1].tolist() == want[want >= 0].tolist()
    # the binding's size checks come before anything is issued
    with pytest.raises(ValueError):
        ext.match_triangulation_pairs_device(2, [0], [2], 0, 0, 0, 0, 0, 0, 0, w.K, 0, 0, capacity=8)


def test_shim_tri_runs(orbx, tmp_path):
    """tests/cpp/shim_tri.cpp: the shim's SearchForTriangulation / CreateNewMapPoints and the C calls give the same pairs and
    points; most pairs are the true ones and their points lie on the truth."""
    exe, libdir = os.path.join(str(tmp_path), "shim_tri"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_tri.cpp"),
           "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    last = p.stdout.strip().splitlines()[-1].split()
    npairs, right, npoints, worst, same = int(last[1]), int(last[2]), int(last[3]), float(last[4]), int(last[5])
    assert same == 1 and npairs > 150 and right > 0.95 * npairs and npoints > 0.9 * right and worst < 1e-3, p.stdout
