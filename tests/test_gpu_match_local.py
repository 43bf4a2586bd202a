"""Tracking::SearchLocalPoints on the device (orbx_match_local_map*): the match rows, d_point_view and every field of
orbx_local_result but `rounds` equal the CPU restatement (tests/cpp/match_local_ref.cpp) byte for byte on the worlds of
tests/match_local_ref_lib.py -- the generated ones, the contention world, the hand-made order case and the rule worlds -- issued
alone, at capacities equal to the counts and at the largest ones, in one batch whose pairs share frames and map sets, through the
host form, the Python classes and the shim, and chained behind SearchByProjection and PoseOptimization without a host pass."""
import os
import subprocess

import numpy as np
import pytest

import match_local_ref_lib as L
import match_proj_ref_lib as M
import pose_ref_lib as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP = L.KEYPOINT_DTYPE
NF = len(L.RESULT_FIELDS)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    assert np.asarray(e.GetScaleFactors(), np.float32).tobytes() == L.scale_table().tobytes()
    yield e
    e.close()


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


class Batch:
    """Frames, map sets and pairs in the device layout.  frames: [(kps, desc)]; sets: [(points, normals, dists, map_desc, mask |
    None)]; pairs: [(frame, set, pose [12], matches on entry, outlier | None)].  An array that no set / pair gives is passed as
    NULL."""

    def __init__(self, torch, frames, sets, pairs, cap, mcap, view=True):
        self.cap, self.mcap, self.P, self.F, self.S = cap, mcap, len(pairs), len(frames), len(sets)
        F, S, P = self.F, self.S, self.P
        kps, desc, n = np.zeros((F, cap), KP), np.zeros((F, cap, 32), np.uint8), np.zeros(F, np.int32)
        for f, (k, d) in enumerate(frames):
            n[f] = len(k)
            kps[f, :len(k)], desc[f, :len(k)] = k, d
        pts, nrm, dst = np.zeros((S, mcap, 3), np.float32), np.zeros((S, mcap, 3), np.float32), np.zeros((S, mcap, 2), np.float32)
        mdesc, mask, mn = np.zeros((S, mcap, 32), np.uint8), np.ones((S, mcap), np.uint8), np.zeros(S, np.int32)
        for s, (p, nr, ds, md, m) in enumerate(sets):
            mn[s] = len(p)
            pts[s, :len(p)], nrm[s, :len(p)], dst[s, :len(p)], mdesc[s, :len(p)] = p, nr, ds, md
            if m is not None:
                mask[s, :len(m)] = m
        pose, outl, entry = np.zeros((P, 12), np.float32), np.zeros((P, cap), np.uint8), np.full((P, cap), -7, np.int32)
        for p, (f, _, ps, me, o) in enumerate(pairs):
            pose[p] = ps
            entry[p, :len(me)] = me
            if o is not None:
                outl[p, :len(o)] = o
        self.kps, self.desc, self.n, self.mn, self.pts, self.nrm, self.dst, self.mdesc, self.pose = \
            (up(torch, a) for a in (kps, desc, n, mn, pts, nrm, dst, mdesc, pose))
        self.mask = up(torch, mask) if any(s[4] is not None for s in sets) else None
        self.outl = up(torch, outl) if any(p[4] is not None for p in pairs) else None
        self.entry = up(torch, entry).view(torch.int32)
        self.frame, self.set = (np.array([p[k] for p in pairs], np.int32) for k in range(2))
        self.matches = torch.empty(max(P, 1) * cap, dtype=torch.int32, device="cuda")
        self.view = torch.empty(max(P, 1) * mcap, dtype=torch.uint8, device="cuda") if view else None
        self.res = torch.empty(max(P, 1) * NF, dtype=torch.int32, device="cuda")

    def run(self, torch, ext, K, bounds, th, nnratio):
        self.matches[:self.P * self.cap].copy_(self.entry)
        self.res.fill_(-7)
        if self.view is not None:
            self.view.fill_(0x77)
        ext.match_local_map_pairs_device(self.F, self.frame, self.set, self.kps, self.desc, self.n, self.S, self.mcap, self.mn, self.pts,
                                         self.nrm, self.dst, self.mdesc, self.mask, self.pose, K, bounds, self.matches, self.res, th=th,
                                         nnratio=nnratio, d_outlier=self.outl, d_point_view=self.view, capacity=self.cap)
        torch.cuda.synchronize()
        view = None if self.view is None else self.view.cpu().numpy().reshape(-1, self.mcap)[:self.P]
        return self.matches.cpu().numpy().reshape(-1, self.cap)[:self.P], view, self.res.cpu().numpy().reshape(-1, NF)[:self.P]


def parts(w):
    return (w.kps, w.desc), (w.points, w.normals, w.dists, w.map_desc, w.mask), (0, 0, w.pose, w.matches, w.outlier)


def batch_of(torch, w, cap, mcap, view=True):
    f, s, p = parts(w)
    return Batch(torch, [f], [s], [p], cap, mcap, view)


def check_pair(got_row, got_view, got_res, w, what):
    e = w.expected()
    res = dict(zip(L.RESULT_FIELDS, (int(v) for v in got_res)))
    print(what, "device", res, "restatement", e["res"])
    assert got_row[:w.n_f].tobytes() == e["matches"].tobytes(), what
    assert np.all(got_row[w.n_f:] == -7), what  # (nothing is written beyond the frame's count)
    if got_view is not None:
        assert got_view[:w.n_m].tobytes() == e["view"].tobytes(), what
        assert np.all(got_view[w.n_m:] == 0x77), what
    for f in L.COMPARED_FIELDS:
        assert res[f] == e["res"][f], (what, f, res[f], e["res"][f])
    return res


def _caps(w):
    return (2048 if w.n_f > 1024 else 1024), (4096 if w.n_m > 1024 else 1024)


@pytest.mark.parametrize("name", L.WORLDS)
def test_world_equals_restatement(torch, ext, name):
    w = L.world(name)
    b = batch_of(torch, w, *_caps(w))
    m, v, r = b.run(torch, ext, w.K, w.bounds, w.th, w.nnratio)
    res = check_pair(m[0], v[0], r[0], w, name)
    m2, v2, r2 = b.run(torch, ext, w.K, w.bounds, w.th, w.nnratio)
    assert m.tobytes() == m2.tobytes() and v.tobytes() == v2.tobytes() and r.tobytes() == r2.tobytes(), "two runs differ"
    if name == "w700":
        assert w.n_m > 512 and res["rounds"] >= 1
    if name == "w3000":
        assert w.n_f > 1024 and w.n_m > 2048
    if name == "order":  # 0 alone, then 1, then 2: one point per round
        assert res["rounds"] == 3 and m[0, :2].tolist() == [0, 1]
    if name == "contention":
        assert 3 * res["n_displaced"] >= res["n_in_view"] and res["rounds"] >= 5
    if name == "empty_map":
        assert res["rounds"] == 0 and res["nmatches"] == 0
    if name == "empty_frame":  # (the points in view find no candidate in their first round)
        assert res["rounds"] == 1 and res["nmatches"] == 0 and res["n_in_view"] > 0


@pytest.mark.parametrize("name", list(L.rule_worlds()))
def test_rule_world_equals_restatement(torch, ext, name):
    w = L.rule_worlds()[name]
    m, v, r = batch_of(torch, w, 64, 32).run(torch, ext, w.K, w.bounds, w.th, w.nnratio)
    check_pair(m[0], v[0], r[0], w, name)


def _small_frame_large_map():
    """16 features against a map of 1500 points of which a few dozen are in view (the others that were get their normal turned
    away): twelve features lie on projections of points in view, eight of those points with an index >= 512; four features bring
    entry matches that name points with an index >= 512, two of them as outliers."""
    rng = np.random.default_rng(123)
    K, pose = L.camera(), L.pose_of(52)
    pts, normals, dists, mdesc, mask = L.make_map(1500, 53, pose, K)
    none_k, none_d = L._none_frame()
    proj = L.search_local_points(L.World(none_k, none_d, pts, normals, dists, mdesc, None, pose, K))["proj"]
    in_view = np.flatnonzero((proj[:, 5] == 5.0) & (mask != 0))
    low, high = in_view[in_view < 512][:12], in_view[in_view >= 512][:28]
    assert len(low) == 12 and len(high) == 28
    away = np.setdiff1d(np.flatnonzero(proj[:, 5] == 5.0), np.r_[low, high])
    normals[away] = -normals[away]
    shown = np.r_[high[:8], low[:4]]
    k = np.zeros(16, KP)
    k["x"], k["y"], k["octave"] = rng.uniform(50, 590, 16), rng.uniform(50, 430, 16), rng.integers(0, L.NLEVELS, 16)
    k["x"][:12], k["y"][:12], k["octave"][:12] = proj[shown, 0], proj[shown, 1], proj[shown, 3]
    k["angle"], k["size"], k["class_id"] = rng.uniform(0, 360, 16), 31.0, -1
    desc = rng.integers(0, 256, (16, 32), dtype=np.uint8)
    for f, i in enumerate(shown):
        desc[f] = L._flip(mdesc[i], int(rng.integers(0, 30)), rng)
    entry, outlier = np.full(16, -1, np.int32), np.zeros(16, np.uint8)
    entry[[8, 13, 10, 11]] = [high[8], high[9], high[10], 1499]  # (features 10 and 11 lie on projections: cleared, they can match anew)
    outlier[[10, 11]] = 1
    return L.World(k, desc, pts, normals, dists, mdesc, mask, pose, K, matches=entry, outlier=outlier)


def test_seen_bits_beyond_the_claims(torch, ext):
    """capacity 16 against map_capacity 2048: the "seen" bits of the entry pass need 64 words where the claims that later lie in
    the same LDS need 16, and the entry names points whose bits lie beyond claim[capacity]."""
    cap, mcap = 16, 2048
    w = _small_frame_large_map()
    e = w.expected()
    named, new = w.matches[w.matches >= 0], e["matches"][(e["matches"] >= 0) & (e["matches"] != w.matches)]
    print("restatement", e["res"], "entry", w.matches.tolist(), "row", e["matches"].tolist())
    assert (mcap + 31) // 32 > cap and w.n_f <= cap and 1400 <= w.n_m <= 1600
    assert 24 <= e["res"]["n_in_view"] <= 60
    assert e["res"]["n_seen"] > 0 and e["res"]["n_outliers_cleared"] > 0 and e["res"]["nmatches"] > 0
    assert len(named) and named.min() >= 512 and w.matches[w.outlier != 0].min() >= 512
    assert len(new) == e["res"]["nmatches"] and new.max() >= 512
    m, v, r = batch_of(torch, w, cap, mcap).run(torch, ext, w.K, w.bounds, w.th, w.nnratio)
    check_pair(m[0], v[0], r[0], w, "16 features, 1500 points")


@pytest.mark.parametrize("caps", ("exact", "largest"))
def test_capacities_and_counts(torch, orbx, ext, caps):
    """Capacities that are exactly the counts (nothing lies beyond the rows), and both at ORBX_BOW_MAX_FEATURES with counts far
    below (the kernel's LDS is sized from the capacities: 158 KB here); the second without d_point_view."""
    w = L.make_world(240, 31)
    cap, mcap = (w.n_f, w.n_m) if caps == "exact" else (orbx.BOW_MAX_FEATURES, orbx.BOW_MAX_FEATURES)
    assert orbx.BOW_MAX_FEATURES == 16384 and w.n_f != w.n_m
    m, v, r = batch_of(torch, w, cap, mcap, view=caps == "exact").run(torch, ext, w.K, w.bounds, w.th, w.nnratio)
    res = check_pair(m[0], None if v is None else v[0], r[0], w, caps)
    assert res["nmatches"] > 15


def test_batch_with_shared_frames_and_maps(torch, ext):
    """One call: frame 0 against map 0 under two poses (two answers) and against map 1; frame 1 against map 0; an empty frame and
    an empty map; pair 1 brings outlier flags and entry matches, the others' rows are fresh."""
    a, c = L.world("main"), L.world("main_th5")
    other = L.pose_of(99)
    none_k, none_d = L._none_frame()
    z3, z2 = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
    fresh_a, fresh_c = np.full(a.n_f, -1, np.int32), np.full(c.n_f, -1, np.int32)
    frames = [(a.kps, a.desc), (c.kps, c.desc), (none_k, none_d)]
    sets = [(a.points, a.normals, a.dists, a.map_desc, a.mask), (c.points, c.normals, c.dists, c.map_desc, c.mask), (z3, z3, z2, none_d, None)]
    pairs = [(0, 0, a.pose, fresh_a, None), (0, 0, other, a.matches, a.outlier), (0, 1, c.pose, fresh_a, None),
             (1, 0, a.pose, fresh_c, None), (2, 0, a.pose, np.zeros(0, np.int32), None), (1, 2, c.pose, fresh_c, None)]

    def world_of(f, s, pose, entry, outl):
        (k, d), (p, nr, ds, md, m) = frames[f], sets[s]
        return L.World(k, d, p, nr, ds, md, m, pose, a.K, a.bounds, a.th, a.nnratio, entry, outl)
    want = [world_of(*p) for p in pairs]
    b = Batch(torch, frames, sets, pairs, 1024, 1024)
    m, v, r = b.run(torch, ext, a.K, a.bounds, a.th, a.nnratio)
    got = [check_pair(m[p], v[p], r[p], want[p], "pair %d" % p) for p in range(len(pairs))]
    assert m[0, :a.n_f].tobytes() != m[1, :a.n_f].tobytes()  # (one frame, two poses: two answers)
    assert got[0]["nmatches"] > 40 and got[1]["n_seen"] > 5 and got[4]["nmatches"] == 0 and got[5]["n_points"] == 0
    # every pair issued alone gives its row of the batch
    for p in (0, 1, 3):
        one = Batch(torch, frames, sets, pairs[p:p + 1], 1024, 1024)
        m1, v1, r1 = one.run(torch, ext, a.K, a.bounds, a.th, a.nnratio)
        assert m1[0].tobytes() == m[p].tobytes() and v1[0].tobytes() == v[p].tobytes() and r1[0, :NF - 1].tobytes() == r[p, :NF - 1].tobytes(), p


# ---- the second setting (pose_ref_lib.SECOND): fx != fy, a context of 5 levels of 1.37 (the matcher reads the context's scale
# table), the pose rolled by 89 degrees ----

BOUNDS_2 = (-12, 655, -9, 490)


@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, L.SCALE_FACTOR_2, L.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    assert np.asarray(e.GetScaleFactors(), np.float32).tobytes() == L.scale_table(L.NLEVELS_2, L.SCALE_FACTOR_2).tobytes()
    yield e
    e.close()


def test_second_setting_anisotropic_camera_and_five_levels(orbx, torch, ext2):
    """The maps of 150 and 310 points under K_ANISO in one batch at the capacities of the largest counts, under the offset
    bounds (a call has one set of bounds: the smaller scene's restatement runs under them too); then the smaller scene alone
    at its own counts under the usual bounds, through the batch and the host form."""
    a, b = L.world("w150@2"), L.world("w310_bounds@2")
    assert a.n_m == 150 and b.n_m == 310 and b.bounds == BOUNDS_2 and len(a.scale) == L.NLEVELS_2
    a_off = a.variant(bounds=BOUNDS_2)
    fa, sa, _ = parts(a)
    fb, sb, _ = parts(b)
    pairs = [(0, 0, a.pose, a.matches, a.outlier), (1, 1, b.pose, b.matches, b.outlier)]
    m, v, r = Batch(torch, [fa, fb], [sa, sb], pairs, max(a.n_f, b.n_f), 310).run(torch, ext2, b.K, BOUNDS_2, b.th, b.nnratio)
    for p, w in enumerate((a_off, b)):
        res = check_pair(m[p], v[p], r[p], w, "pair %d" % p)
        # not trivial: matches found, points rejected outside the image, by distance and by angle, and by the ratio test
        assert res["status"] == 0 and res["nmatches"] >= 8 and res["n_out_image"] > 10 and res["n_out_distance"] > 10
        assert res["n_out_angle"] > 5 and res["n_in_view"] > 30 and res["n_ratio_rejected"] > 0
    m1, v1, r1 = batch_of(torch, a, a.n_f, a.n_m).run(torch, ext2, a.K, a.bounds, a.th, a.nnratio)
    check_pair(m1[0], v1[0], r1[0], a, "alone")
    e = a.expected()
    T = np.c_[a.pose[:9].reshape(3, 3), a.pose[9:]]
    mh, vh, rh = ext2.match_local_map(a.kps, a.desc, a.points, a.normals, a.dists, a.map_desc, a.mask, T, a.K, a.bounds, a.matches, a.th,
                                      a.nnratio, a.outlier)
    assert mh.tobytes() == e["matches"].tobytes() and vh.tobytes() == e["view"].tobytes()
    assert {f: x for f, x in rh.as_dict().items() if f != "rounds"} == {f: e["res"][f] for f in L.COMPARED_FIELDS}


def test_host_form_and_classes(orbx, torch, ext):
    for name in ("main", "main_th5", "order", "empty_frame", "empty_map"):
        w = L.world(name)
        e = w.expected()
        T = np.c_[w.pose[:9].reshape(3, 3), w.pose[9:]]
        m, view, res = ext.match_local_map(w.kps, w.desc, w.points, w.normals, w.dists, w.map_desc, w.mask, T, w.K, w.bounds, w.matches,
                                           w.th, w.nnratio, w.outlier)
        assert m.tobytes() == e["matches"].tobytes() and view.tobytes() == e["view"].tobytes(), name
        assert {f: v for f, v in res.as_dict().items() if f != "rounds"} == {f: e["res"][f] for f in L.COMPARED_FIELDS}, name
        F = orbx.Frame.from_arrays(w.kps, w.desc, w.bounds)
        nm, m2, view2, res2 = orbx.ORBmatcher(w.nnratio, True, extractor=ext).SearchLocalPoints(
            F, w.points, w.normals, w.dists, w.map_desc, w.mask, T, w.th, K=w.K.reshape(3, 3), matches=w.matches, outlier=w.outlier)
        assert nm == e["res"]["nmatches"] and m2.tobytes() == m.tobytes() and view2.tobytes() == view.tobytes() and bytes(res2) == bytes(res), name


def test_chain_behind_projection_and_pose_optimization(orbx, torch, ext):
    """match_projection -> gather (the last frame's feature -> its map point) -> pose_optimize -> match_local_map with that
    call's pose and d_outlier, on the same row -> pose_optimize, all on the device at map_capacity == capacity, equals
    match_proj_ref -> pose_ref -> match_local_ref -> pose_ref byte for byte."""
    cap = 1024
    base = L.make_world(500, 41, have=0.0)
    kc = base.kps.copy()
    kc["octave"] = np.clip(kc["octave"], 0, L.NLEVELS - 1)  # (the optimisation refuses an octave outside the table)
    w = base.variant(kps=kc, matches=np.full(base.n_f, -1, np.int32), outlier=None)
    # the last frame: 150 features that have map points the current frame shows; feature i's map point is last_map[i]
    shown = np.flatnonzero(base.shows >= 0)[:150]
    last_map = base.shows[shown].astype(np.int32)
    kl = kc[shown].copy()
    kl["x"], kl["y"] = np.random.default_rng(4).uniform(0, 480, (2, len(shown)))
    wp = M.World(kl, w.map_desc[last_map], kc, w.desc, w.points[last_map], None, w.pose, w.K, w.bounds, 15.0, True)
    # -- the restatements
    e1 = wp.expected()
    row = np.full(cap, -1, np.int32)
    row[:w.n_f] = np.where(e1["matches"] >= 0, last_map[np.maximum(e1["matches"], 0)], -1)
    assert e1["res"]["nmatches"] >= 60
    kps_row, pts_row, mask_row = np.zeros(cap, KP), np.zeros((cap, 3), np.float32), np.zeros(cap, np.uint8)
    kps_row[:w.n_f], pts_row[:w.n_m], mask_row[:w.n_m] = kc, w.points, w.mask
    p1, flags1, _, _ = PR.pose_optimize(PR.World(kps_row, w.n_f, row.copy(), pts_row, mask_row, w.pose.copy(), w.K))
    assert p1["status"] == 0 and flags1.sum() > 0
    pose1 = np.r_[p1["R"].reshape(9), p1["tcw"]].astype(np.float32)
    w2 = w.variant(pose=pose1, matches=row[:w.n_f].copy(), outlier=flags1[:w.n_f].copy())
    e2 = w2.expected()
    assert e2["res"]["nmatches"] >= 20 and e2["res"]["n_seen"] >= 60 and e2["res"]["n_outliers_cleared"] == int(flags1.sum())
    row2 = np.full(cap, -1, np.int32)
    row2[:w.n_f] = e2["matches"]
    p2, flags2, _, _ = PR.pose_optimize(PR.World(kps_row, w.n_f, row2.copy(), pts_row, mask_row, pose1.copy(), w.K))
    assert int((row2 >= 0).sum()) == e1["res"]["nmatches"] - int(flags1.sum()) + e2["res"]["nmatches"]
    assert p2["status"] == 0 and p2["n_correspondences"] == int((mask_row[row2[row2 >= 0]] != 0).sum())  # (a masked point is no edge)
    # -- the device: frames 0 (last) and 1 (current); point set 0 = the last frame's points, 1 = the map
    kps, desc, n = np.zeros((2, cap), KP), np.zeros((2, cap, 32), np.uint8), np.array([len(kl), w.n_f], np.int32)
    kps[0, :len(kl)], desc[0, :len(kl)], kps[1, :w.n_f], desc[1, :w.n_f] = kl, wp.desc_l, kc, w.desc
    pts = np.zeros((2, cap, 3), np.float32)
    pts[0, :len(kl)], pts[1] = wp.points, pts_row
    masks = np.zeros((2, cap), np.uint8)
    masks[0, :len(kl)], masks[1] = 1, mask_row
    nrm, dst, mdesc = np.zeros((1, cap, 3), np.float32), np.zeros((1, cap, 2), np.float32), np.zeros((1, cap, 32), np.uint8)
    nrm[0, :w.n_m], dst[0, :w.n_m], mdesc[0, :w.n_m] = w.normals, w.dists, w.map_desc
    d_kps, d_desc, d_n, d_pts, d_masks, d_nrm, d_dst, d_mdesc = (up(torch, a) for a in (kps, desc, n, pts, masks, nrm, dst, mdesc))
    d_mn, d_pose0 = up(torch, np.array([w.n_m], np.int32)), up(torch, w.pose)
    d_last_map = torch.from_numpy(np.r_[last_map, np.full(cap - len(last_map), -1, np.int32)]).cuda()
    d_cur = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    d_proj_res = torch.zeros(8, dtype=torch.int32, device="cuda")
    d_pres = torch.zeros(2 * orbx.POSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(2 * cap, dtype=torch.uint8, device="cuda")
    d_lres = torch.zeros(NF, dtype=torch.int32, device="cuda")
    one, zero = np.array([1], np.int32), np.array([0], np.int32)
    d_map_pts, d_map_mask = d_pts[cap * 12:], d_masks[cap:]
    ext.match_projection_pairs_device(2, zero, one, zero, d_kps, d_desc, d_n, 2, d_pts, d_masks, d_pose0, w.K, w.bounds, d_cur, d_proj_res,
                                      th=15.0, checkOri=True, capacity=cap)
    # the caller's gather: the last frame's feature -> its index in the map set (entries beyond the frame's count name nothing)
    # (the gather and the pose row below are torch's work: it starts behind what the context has queued)
    ext.order_before(torch.cuda.current_stream().cuda_stream)
    live = torch.arange(cap, device="cuda") < w.n_f
    d_row = torch.where(live & (d_cur >= 0), d_last_map[d_cur.clamp(0, cap - 1).long()], torch.full_like(d_cur, -1)).contiguous()
    ext.pose_optimize_batch_device(2, one, zero, d_kps, d_n, d_row, 1, d_map_pts, d_map_mask, d_pose0, w.K, d_pres[:192], d_out[:cap], capacity=cap)
    ext.order_before(torch.cuda.current_stream().cuda_stream)
    d_pose1 = d_pres[144:192].clone()  # (the record ends with R [9] and tcw [3] as f32: a pose row)
    ext.match_local_map_pairs_device(2, one, zero, d_kps, d_desc, d_n, 1, cap, d_mn, d_map_pts, d_nrm, d_dst, d_mdesc, d_map_mask, d_pose1,
                                     w.K, w.bounds, d_row, d_lres, th=w.th, nnratio=w.nnratio, d_outlier=d_out[:cap], capacity=cap)
    ext.pose_optimize_batch_device(2, one, zero, d_kps, d_n, d_row, 1, d_map_pts, d_map_mask, d_pose1, w.K, d_pres[192:], d_out[cap:], capacity=cap)
    torch.cuda.synchronize()
    res = d_pres.cpu().numpy().view(orbx.POSE_RESULT_DTYPE)
    assert d_pose1.cpu().numpy().tobytes() == pose1.tobytes()
    lres = dict(zip(L.RESULT_FIELDS, d_lres.cpu().numpy().tolist()))
    assert {f: lres[f] for f in L.COMPARED_FIELDS} == {f: e2["res"][f] for f in L.COMPARED_FIELDS}
    assert d_row.cpu().numpy().tobytes() == row2.tobytes()
    flags = d_out.cpu().numpy().reshape(2, cap)
    for k, (ref, rflags) in enumerate(((p1, flags1), (p2, flags2))):
        for f in orbx.POSE_RESULT_DTYPE.names:
            assert np.asarray(res[k][f]).tobytes() == np.asarray(ref[f]).tobytes(), (k, f, res[k][f], ref[f])
        assert flags[k].tobytes() == rflags.tobytes(), k


def test_refusals(orbx, torch, ext):
    w = L.world("order")
    b = batch_of(torch, w, 64, 32)
    lib, p = orbx.lib(), orbx._ptr
    K = np.ascontiguousarray(w.K, np.float32)
    b.matches.fill_(-1)
    b.res.fill_(-7)

    def call(frame=0, mset=0, cap=64, mcap=32, th=1.0, nnratio=0.8, bounds=(0, 640, 0, 480), ctx=ext._h, n_pairs=1, matches=b.matches):
        hf, hs = np.array([frame], np.int32), np.array([mset], np.int32)  # (named: they outlive the call)
        bb = orbx._Bounds(*bounds)
        return lib.orbx_match_local_map_batch_device(ctx, 1, n_pairs, p(hf), p(hs), p(b.kps), p(b.desc), p(b.n), cap, 1, mcap, p(b.mn),
                                                     p(b.pts), p(b.nrm), p(b.dst), p(b.mdesc), None, p(b.pose), p(K), orbx.ctypes.byref(bb),
                                                     th, nnratio, p(matches), None, None, p(b.res))
    assert call(n_pairs=0) == 0
    torch.cuda.synchronize()
    assert int(b.res[0]) == -7  # (nothing ran)
    bad, full = orbx.E_BADARG, orbx.E_CAPACITY
    assert call(frame=1) == bad and call(frame=-1) == bad and call(mset=1) == bad and call(matches=None) == bad
    assert call(th=0.0) == bad and call(th=-1.0) == bad and call(th=float("nan")) == bad and call(th=float("inf")) == bad
    assert call(nnratio=0.0) == bad and call(nnratio=1.0000001) == bad and call(nnratio=float("nan")) == bad and call(nnratio=-0.5) == bad
    assert call(bounds=(5, 5, 0, 480)) == bad and call(bounds=(0, 640, 10, 9)) == bad
    assert call(cap=orbx.BOW_MAX_FEATURES + 1) == full and call(mcap=orbx.BOW_MAX_FEATURES + 1) == full
    assert call(cap=0) == bad and call(mcap=0) == bad
    assert call(ctx=None) == orbx.E_HIP and call(ctx=None, nnratio=0.0) == bad  # (the arguments are judged first)
    torch.cuda.synchronize()
    assert int(b.res[0]) == -7 and bool((b.matches == -1).all())  # (no refusal touched the device)
    assert call(nnratio=1.0) == 0  # (the largest ratio)
    torch.cuda.synchronize()
    assert int(b.res[1]) == 2 and b.matches[:2].tolist() == [0, 1]
    # the binding's size checks come before anything is issued
    short = torch.zeros(10, dtype=torch.int32, device="cuda")
    args = lambda **kw: dict(dict(n_frames=1, frame=[0], map_set=[0], d_kps_un=b.kps, d_desc=b.desc, d_n=b.n, n_map_sets=1, map_capacity=32,  # noqa: E731
                                  d_map_n=b.mn, d_map_points=b.pts, d_map_normals=b.nrm, d_map_dist=b.dst, d_map_desc=b.mdesc, d_map_mask=None,
                                  d_pose=b.pose, K=K, bounds=w.bounds, d_matches=b.matches, d_res=b.res, capacity=64), **kw)
    for kw in (dict(d_matches=short), dict(d_res=short[:4]), dict(frame=[1]), dict(map_set=[2]),
               dict(d_outlier=torch.zeros(8, dtype=torch.uint8, device="cuda")), dict(d_point_view=torch.zeros(8, dtype=torch.uint8, device="cuda")),
               dict(d_map_normals=short)):
        with pytest.raises(ValueError):
            ext.match_local_map_pairs_device(**args(**kw))


def test_shim_match_local_runs(orbx, tmp_path):
    """tests/cpp/shim_match_local.cpp: the shim's two forms and the C call give the same rows, most new matches the true ones."""
    exe, libdir = os.path.join(str(tmp_path), "shim_match_local"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_match_local.cpp"),
           "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    nm, right, searched, same = (int(v) for v in p.stdout.strip().splitlines()[-1].split()[1:])
    assert same == 1 and searched > 50 and nm > 0.7 * searched and right > 0.9 * nm, p.stdout
