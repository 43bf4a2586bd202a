"""Both overloads of ORBmatcher::Fuse on the device (orbx_fuse*, orbx_fuse_scw*): the row, the three per-point outputs and every
field of orbx_fuse_result but `rounds` equal the CPU restatement (tests/cpp/fuse_ref.cpp) byte for byte on the worlds of
tests/fuse_ref_lib.py -- the named ones, the contention world, the hand-made order case and the rule worlds -- issued alone, at
capacities equal to the counts and at the largest ones, in one batch whose pairs share a keyframe and a map set, under the second
setting, through the host forms, the Python classes and the shim, and chained behind the Scw matcher on one row without a host
pass.  Every test first asserts on the restatement's counters that its world does what it is for."""
import os
import subprocess

import numpy as np
import pytest

import fuse_ref_lib as L
import match_scw_ref_lib as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP = L.KEYPOINT_DTYPE
NF = len(L.RESULT_FIELDS)
NAMED = [(f, n) for f in L.FORMS for n in L.WORLDS]
RULES = sorted(L.rule_worlds())


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    assert np.asarray(e.GetScaleFactors(), np.float32).tobytes() == L.scale_table().tobytes()
    assert np.asarray(e.GetInverseScaleSigmaSquares(), np.float32).tobytes() == L.inv_sigma2_table().tobytes()
    yield e
    e.close()


@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, L.SCALE_FACTOR_2, L.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    assert np.asarray(e.GetScaleFactors(), np.float32).tobytes() == L.scale_table(L.NLEVELS_2, L.SCALE_FACTOR_2).tobytes()
    assert np.asarray(e.GetInverseScaleSigmaSquares(), np.float32).tobytes() == L.inv_sigma2_table(L.NLEVELS_2, L.SCALE_FACTOR_2).tobytes()
    yield e
    e.close()


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Batch:
    """Keyframes, map sets and pairs of ONE form in the device layout.  frames: [(kps, desc)]; sets: [(points, normals, dists,
    map_desc, mask | None, obs)]; pairs: [(frame, set, T [12], row on entry, occ_obs | None)].  The mask is NULL when no set gives
    one, the occupants' counts when no pair gives them.  Everything beyond the counts is filled with -7 / 0xF9 before a run."""

    def __init__(self, torch, form, frames, sets, pairs, cap, mcap):
        self.form, self.cap, self.mcap, self.P, self.F, self.S = form, cap, mcap, len(pairs), len(frames), len(sets)
        F, S, P = self.F, self.S, self.P
        kps, desc, n = np.zeros((F, cap), KP), np.zeros((F, cap, 32), np.uint8), np.zeros(F, np.int32)
        for f, (k, d) in enumerate(frames):
            n[f] = len(k)
            kps[f, :len(k)], desc[f, :len(k)] = k, d
        pts, nrm, dst = np.zeros((S, mcap, 3), np.float32), np.zeros((S, mcap, 3), np.float32), np.zeros((S, mcap, 2), np.float32)
        mdesc, mask, mn = np.zeros((S, mcap, 32), np.uint8), np.ones((S, mcap), np.uint8), np.zeros(S, np.int32)
        obs = np.zeros((S, mcap), np.int32)
        for s, (p, nr, ds, md, m, ob) in enumerate(sets):
            mn[s] = len(p)
            pts[s, :len(p)], nrm[s, :len(p)], dst[s, :len(p)], mdesc[s, :len(p)], obs[s, :len(p)] = p, nr, ds, md, ob
            if m is not None:
                mask[s, :len(m)] = m
        T, entry, occ = np.zeros((P, 12), np.float32), np.full((P, cap), -7, np.int32), np.full((P, cap), -1, np.int32)
        counted = [p[4] is not None for p in pairs]
        assert all(counted) or not any(counted)
        for p, (_, _, t, me, oc) in enumerate(pairs):
            T[p] = t
            entry[p, :len(me)] = me
            if oc is not None:
                occ[p, :len(oc)] = oc
        self.kps, self.desc, self.n, self.mn, self.pts, self.nrm, self.dst, self.mdesc, self.obs, self.T = \
            (up(torch, a) for a in (kps, desc, n, mn, pts, nrm, dst, mdesc, obs, T))
        self.mask = up(torch, mask) if any(s[4] is not None for s in sets) else None
        self.occ = up(torch, occ) if any(counted) else None
        self.entry = up(torch, entry).view(torch.int32)
        self.frame, self.set = (np.array([p[k] for p in pairs], np.int32) for k in range(2))
        q = max(P, 1)
        self.matches = torch.empty(q * cap, dtype=torch.int32, device="cuda")
        self.idx = torch.empty(q * mcap, dtype=torch.int32, device="cuda")
        self.act = torch.empty(q * mcap, dtype=torch.uint8, device="cuda")
        self.other = torch.empty(q * mcap, dtype=torch.int32, device="cuda")
        self.res = torch.empty(q * NF, dtype=torch.int32, device="cuda")

    def run(self, torch, fuser, K, bounds, th, th_low):
        self.matches[:self.P * self.cap].copy_(self.entry)
        for a in (self.idx, self.other, self.res):
            a.fill_(-7)
        self.act.fill_(0xF9)
        a = (self.F, self.frame, self.set, self.kps, self.desc, self.n, self.S, self.mcap, self.mn, self.pts, self.nrm, self.dst, self.mdesc,
             self.mask)
        b = (self.T, K, bounds, self.matches, self.occ, self.idx, self.act, self.other, self.res)
        if self.form == "pose":
            fuser.fuse_pairs_device(*a, self.obs, *b, th=th, th_low=th_low, capacity=self.cap)
        else:
            fuser.fuse_scw_pairs_device(*a, *b, th=th, th_low=th_low, capacity=self.cap)
        torch.cuda.synchronize()
        rows = lambda t, w: t.cpu().numpy().reshape(-1, w)[:self.P]  # noqa: E731
        return rows(self.matches, self.cap), rows(self.idx, self.mcap), rows(self.act, self.mcap), rows(self.other, self.mcap), rows(self.res, NF)


def parts(w):
    return (w.kps, w.desc), (w.points, w.normals, w.dists, w.map_desc, w.mask, w.obs), (0, 0, w.T, w.matches, w.occ_obs)


def batch_of(torch, w, cap, mcap):
    f, s, p = parts(w)
    return Batch(torch, w.form, [f], [s], [p], cap, mcap)


def check_pair(out, p, w, what):
    row, idx, act, other, r = (o[p] for o in out)
    e = w.expected()
    res = dict(zip(L.RESULT_FIELDS, (int(v) for v in r)))
    print(what, "device", res, "restatement", e["res"])
    assert row[:w.n_f].tobytes() == e["matches"].tobytes(), what
    assert idx[:w.n_m].tobytes() == e["idx"].tobytes() and act[:w.n_m].tobytes() == e["act"].tobytes(), what
    assert other[:w.n_m].tobytes() == e["other"].tobytes(), what
    # nothing is written at and beyond the counts
    assert np.all(row[w.n_f:] == -7) and np.all(idx[w.n_m:] == -7) and np.all(other[w.n_m:] == -7) and np.all(act[w.n_m:] == 0xF9), what
    for f in L.COMPARED_FIELDS:
        assert res[f] == e["res"][f], (what, f, res[f], e["res"][f])
    return res


def longest_list(w):
    idx = w.expected()["idx"]
    return int(np.bincount(idx[idx >= 0]).max()) if (idx >= 0).any() else 0


@pytest.mark.parametrize("form,name", NAMED)
def test_world_equals_restatement(orbx, torch, ext, form, name):
    w = L.world(form, name)
    r = w.expected()["res"]
    assert r["n_fused"] > 0 and r["n_with_candidates"] >= r["n_fused"]
    if name == "contention":
        for f in ("n_added", "n_kept_occupant", "n_bad_occupant", "n_chained", "n_over_dist") + (("n_replaced_occupant",) if form == "pose" else ()):
            assert r[f] > 0, (f, r)
    b = batch_of(torch, w, 1024, 1024)
    fuser = orbx.MapFuser(ext)
    out = b.run(torch, fuser, w.K, w.bounds, w.th, w.th_low)
    res = check_pair(out, 0, w, (form, name))
    again = b.run(torch, fuser, w.K, w.bounds, w.th, w.th_low)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(out, again)), "two runs differ"
    assert res["rounds"] == longest_list(w)  # (the longest list of points on one feature)
    if name == "w513":
        assert w.n_m == 513
    if name == "order":
        assert res["rounds"] == 3
    if name == "contention":
        assert res["rounds"] == 7


@pytest.mark.parametrize("key", RULES)
def test_rule_world_equals_restatement(orbx, torch, ext, key):
    w = L.rule_worlds()[key]
    e = w.expected()["res"]
    for f, v in L.RULE_AIMS[key].items():
        assert ((e["status"] & v == v) if v else e["status"] == 0) if f == "status" else e[f] == v, (key, f, e)
    fuser = orbx.MapFuser(ext)
    out = batch_of(torch, w, max(w.n_f, 1), max(w.n_m, 1)).run(torch, fuser, w.K, w.bounds, w.th, w.th_low)
    check_pair(out, 0, w, key)
    out = batch_of(torch, w, 64, 32).run(torch, fuser, w.K, w.bounds, w.th, w.th_low)
    check_pair(out, 0, w, key + ("at 64 / 32",))


@pytest.mark.parametrize("form", L.FORMS)
@pytest.mark.parametrize("caps", ("exact", "largest"))
def test_capacities_and_counts(torch, orbx, ext, form, caps):
    """Capacities that are exactly the counts (nothing lies beyond the rows), and both at ORBX_BOW_MAX_FEATURES with counts far
    below (the kernel's LDS is sized from the capacities: 132 KB here, beyond the default limit of a launch)."""
    w = L.make_world(form, 100, 33, edge_cases=False, n_extra=10)
    assert w.expected()["res"]["n_fused"] > 5 and w.expected()["res"]["n_in_kf"] > 1
    cap, mcap = (w.n_f, w.n_m) if caps == "exact" else (orbx.BOW_MAX_FEATURES, orbx.BOW_MAX_FEATURES)
    assert orbx.BOW_MAX_FEATURES == 16384
    out = batch_of(torch, w, cap, mcap).run(torch, orbx.MapFuser(ext), w.K, w.bounds, w.th, w.th_low)
    check_pair(out, 0, w, (form, caps))


@pytest.mark.parametrize("form", L.FORMS)
def test_batch_with_a_shared_keyframe_and_map_set(orbx, torch, ext, form):
    """One call: keyframe 0 against map set 0 under two poses and two rows (two answers) and against map set 1; keyframe 1 against
    map set 0; a keyframe without features and an empty map set."""
    a, c = L.world(form, "main"), L.world(form, "contention")
    other = L.pose_of(99) if form == "pose" else L.scaled(L.pose_of(99), 0.7)
    none_k, none_d = np.zeros(0, KP), np.zeros((0, 32), np.uint8)
    z3, z2, z1 = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.int32)
    fresh_a, fresh_c = np.full(a.n_f, -1, np.int32), np.full(c.n_f, -1, np.int32)
    frames = [(a.kps, a.desc), (c.kps, c.desc), (none_k, none_d)]
    sets = [(a.points, a.normals, a.dists, a.map_desc, a.mask, a.obs), (c.points, c.normals, c.dists, c.map_desc, c.mask, c.obs),
            (z3, z3, z2, none_d, None, z1)]
    pairs = [(0, 0, a.T, a.matches, a.occ_obs), (0, 0, other, fresh_a, a.occ_obs), (0, 1, c.T, fresh_a, a.occ_obs),
             (1, 0, a.T, fresh_c, c.occ_obs), (2, 0, a.T, z1, z1), (1, 2, c.T, c.matches, c.occ_obs), (1, 1, c.T, c.matches, c.occ_obs)]

    def world_of(f, s, T, entry, occ):
        (k, d), (p, nr, ds, md, m, ob) = frames[f], sets[s]
        return L.World(form, k, d, p, nr, ds, md, m, ob, T, a.K, a.bounds, a.th, a.th_low, entry, occ)
    want = [world_of(*p) for p in pairs]
    assert want[0].expected()["res"]["n_fused"] > 40 and want[6].expected()["res"]["n_chained"] > 0
    fuser = orbx.MapFuser(ext)
    out = Batch(torch, form, frames, sets, pairs, 1024, 1024).run(torch, fuser, a.K, a.bounds, a.th, a.th_low)
    got = [check_pair(out, p, want[p], "pair %d" % p) for p in range(len(pairs))]
    assert out[0][0, :a.n_f].tobytes() != out[0][1, :a.n_f].tobytes()  # (one keyframe, two poses and rows: two answers)
    assert got[4]["n_fused"] == 0 and got[5]["n_points"] == 0 and got[6]["rounds"] == 7
    for p in (0, 1, 6):  # a pair issued alone gives its rows of the batch
        one = Batch(torch, form, frames, sets, pairs[p:p + 1], 1024, 1024).run(torch, fuser, a.K, a.bounds, a.th, a.th_low)
        assert all(x[0].tobytes() == y[p].tobytes() for x, y in zip(one, out)), p


@pytest.mark.parametrize("form", L.FORMS)
def test_second_setting_anisotropic_camera_and_five_levels(orbx, torch, ext2, form):
    w = L.world(form, "w150@2")
    r = w.expected()["res"]
    assert r["n_fused"] > 5 and r["status"] == 0 and r["n_out_image"] > 10 and r["n_out_angle"] > 5
    out = batch_of(torch, w, 256, 160).run(torch, orbx.MapFuser(ext2), w.K, w.bounds, w.th, w.th_low)
    check_pair(out, 0, w, (form, "w150@2"))


def _host(fuser, w):
    if w.form == "pose":
        return fuser.fuse(w.kps, w.desc, w.points, w.normals, w.dists, w.map_desc, w.mask, w.obs, w.T, w.K, w.bounds, w.matches, w.occ_obs,
                          w.th, w.th_low)
    return fuser.fuse_scw(w.kps, w.desc, w.points, w.normals, w.dists, w.map_desc, w.mask, w.T, w.K, w.bounds, w.matches, w.occ_obs, w.th,
                          w.th_low)


@pytest.mark.parametrize("form", L.FORMS)
def test_host_forms_and_classes(orbx, torch, ext, form):
    fuser = orbx.MapFuser(ext)
    names = [L.world(form, n) for n in ("main", "contention", "order", "tiny")]
    names += [L.rule_worlds()[(form, n)] for n in ("unmapped_without_counts", "no_features", "no_points", "counts_out_of_range")]
    assert names[0].expected()["res"]["n_fused"] > 40
    for w in names:
        e = w.expected()
        row, idx, act, other, res = _host(fuser, w)
        assert row.tobytes() == e["matches"].tobytes() and idx.tobytes() == e["idx"].tobytes()
        assert act.tobytes() == e["act"].tobytes() and other.tobytes() == e["other"].tobytes()
        assert {f: v for f, v in res.as_dict().items() if f != "rounds"} == {f: e["res"][f] for f in L.COMPARED_FIELDS}
        F = orbx.Frame.from_arrays(w.kps, w.desc, w.bounds)
        T44 = np.eye(4, dtype=np.float32)
        T44[:3, :3], T44[:3, 3] = w.T[:9].reshape(3, 3), w.T[9:]
        m = orbx.ORBmatcher(0.75, True, extractor=ext)
        if form == "pose":
            got = m.Fuse(F, w.points, w.normals, w.dists, w.map_desc, w.mask, w.obs, T44, w.th, K=w.K.reshape(3, 3), matches=w.matches,
                         occ_obs=w.occ_obs, th_low=w.th_low)
        else:
            got = m.FuseScw(F, T44, w.points, w.normals, w.dists, w.map_desc, w.mask, w.th, K=w.K.reshape(3, 3), matches=w.matches,
                            occ_obs=w.occ_obs, th_low=w.th_low)
        assert got[0] == e["res"]["n_fused"] and got[1].tobytes() == row.tobytes() and got[2].tobytes() == idx.tobytes()
        assert got[3].tobytes() == act.tobytes() and got[4].tobytes() == other.tobytes() and bytes(got[5]) == bytes(res)


def test_chain_behind_the_scw_matcher_on_one_row(orbx, torch, ext):
    """LoopClosing: match_scw_pairs_device, then fuse_scw_pairs_device on the same map set, under the same d_scw and into the same
    row, queued on the stream with no copy between them -- equal to the two restatements chained."""
    sw = S.world("contention")  # (seven points over four features: three of seven find everything taken, and Fuse has no such rule)
    se = sw.expected()
    assert se["res"]["nmatches"] > 10
    fw = L.World("scw", sw.kps, sw.desc, sw.points, sw.normals, sw.dists, sw.map_desc, sw.mask, None, sw.scw, sw.K, sw.bounds, 4.0, L.TH_LOW,
                 se["matches"])
    fe = fw.expected()
    assert fe["res"]["n_kept_occupant"] > 100 and fe["res"]["n_in_kf"] == se["res"]["nmatches"] == 160 and fe["res"]["n_added"] == 0
    b = batch_of(torch, fw, 1024, 1024)
    b.matches[:b.cap].copy_(up(torch, np.r_[sw.matches, np.full(b.cap - sw.n_f, -7, np.int32)]).view(torch.int32))
    for a in (b.idx, b.other, b.res):
        a.fill_(-7)
    b.act.fill_(0xF9)
    scw_res = torch.zeros(14, dtype=torch.int32, device="cuda")
    ext.match_scw_pairs_device(1, b.frame, b.set, b.kps, b.desc, b.n, 1, b.mcap, b.mn, b.pts, b.nrm, b.dst, b.mdesc, b.mask, b.T, sw.K, sw.bounds,
                               b.matches, scw_res, th=sw.th, th_low=sw.th_low, capacity=b.cap)
    orbx.MapFuser(ext).fuse_scw_pairs_device(1, b.frame, b.set, b.kps, b.desc, b.n, 1, b.mcap, b.mn, b.pts, b.nrm, b.dst, b.mdesc, b.mask, b.T,
                                             sw.K, sw.bounds, b.matches, None, b.idx, b.act, b.other, b.res, th=4.0, th_low=L.TH_LOW,
                                             capacity=b.cap)
    torch.cuda.synchronize()
    got = {f: int(v) for f, v in zip(S.RESULT_FIELDS, scw_res.cpu().numpy())}
    assert {f: got[f] for f in S.COMPARED_FIELDS} == {f: se["res"][f] for f in S.COMPARED_FIELDS}
    rows = lambda t, w: t.cpu().numpy().reshape(-1, w)[:1]  # noqa: E731
    check_pair((rows(b.matches, b.cap), rows(b.idx, b.mcap), rows(b.act, b.mcap), rows(b.other, b.mcap), rows(b.res, NF)), 0, fw, "chain")


def test_refusals(orbx, torch, ext):
    w = L.world("pose", "order")
    b = batch_of(torch, w, 64, 32)
    lib, p = orbx.lib(), orbx._ptr
    K = np.ascontiguousarray(w.K, np.float32)
    b.matches.fill_(-1)
    b.res.fill_(-7)

    def call(scw=False, frame=0, mset=0, cap=64, mcap=32, th=3.0, th_low=50, bounds=(0, 640, 0, 480), ctx=ext._h, n_pairs=1, matches=b.matches,
             T=b.T, obs=b.obs, idx=b.idx, act=b.act, other=b.other, res=b.res):
        hf, hs = np.array([frame], np.int32), np.array([mset], np.int32)  # (named: they outlive the call)
        bb = orbx._Bounds(*bounds)
        head = (ctx, 1, n_pairs, p(hf), p(hs), p(b.kps), p(b.desc), p(b.n), cap, 1, mcap, p(b.mn), p(b.pts), p(b.nrm), p(b.dst), p(b.mdesc), None)
        tail = (p(T), p(K), orbx.ctypes.byref(bb), th, th_low, p(matches), None, p(idx), p(act), p(other), p(res))
        return lib.orbx_fuse_scw_batch_device(*head, *tail) if scw else lib.orbx_fuse_batch_device(*head, p(obs), *tail)
    bad, full = orbx.E_BADARG, orbx.E_CAPACITY
    for scw in (False, True):
        assert call(scw, n_pairs=0) == 0
        assert call(scw, frame=1) == bad and call(scw, frame=-1) == bad and call(scw, mset=1) == bad and call(scw, matches=None) == bad
        assert call(scw, T=None) == bad and call(scw, idx=None) == bad and call(scw, act=None) == bad and call(scw, other=None) == bad
        assert call(scw, res=None) == bad
        assert call(scw, th=0.0) == bad and call(scw, th=-1.0) == bad and call(scw, th=float("nan")) == bad and call(scw, th=float("inf")) == bad
        assert call(scw, th_low=-1) == bad and call(scw, th_low=257) == bad
        assert call(scw, bounds=(5, 5, 0, 480)) == bad and call(scw, bounds=(0, 640, 10, 9)) == bad
        assert call(scw, cap=orbx.BOW_MAX_FEATURES + 1) == full and call(scw, mcap=orbx.BOW_MAX_FEATURES + 1) == full
        assert call(scw, cap=0) == bad and call(scw, mcap=0) == bad and call(scw, n_pairs=-1) == bad
        assert call(scw, ctx=None) == orbx.E_HIP and call(scw, ctx=None, th_low=300) == bad  # (the arguments are judged first)
    assert call(obs=None) == bad
    torch.cuda.synchronize()
    assert int(b.res[0]) == -7 and bool((b.matches == -1).all())  # (no refusal touched the device)
    assert call(th_low=256) == 0  # (the largest threshold)
    torch.cuda.synchronize()
    assert int(b.res[1]) == 3 and int(b.matches[0]) == 1
    # the binding's size checks come before anything is issued
    short = torch.zeros(10, dtype=torch.int32, device="cuda")
    fuser = orbx.MapFuser(ext)
    args = lambda **kw: dict(dict(n_frames=1, kf=[0], map_set=[0], d_kps_un=b.kps, d_desc=b.desc, d_n=b.n, n_map_sets=1, map_capacity=32,  # noqa: E731
                                  d_map_n=b.mn, d_map_points=b.pts, d_map_normals=b.nrm, d_map_dist=b.dst, d_map_desc=b.mdesc, d_map_mask=None,
                                  d_map_obs=b.obs, d_pose=b.T, K=K, bounds=w.bounds, d_matches=b.matches, d_occ_obs=None, d_fuse_idx=b.idx,
                                  d_fuse_act=b.act, d_fuse_other=b.other, d_res=b.res, capacity=64), **kw)
    for kw in (dict(d_matches=short), dict(d_res=short[:4]), dict(kf=[1]), dict(map_set=[2]), dict(d_occ_obs=short), dict(d_pose=short[:2]),
               dict(d_map_obs=short), dict(d_fuse_idx=short), dict(d_fuse_act=short[:2]), dict(d_fuse_other=short)):
        with pytest.raises(ValueError):
            fuser.fuse_pairs_device(**args(**kw))
    with pytest.raises(orbx.OrbxError):  # more points than ORBX_BOW_MAX_FEATURES
        n = orbx.BOW_MAX_FEATURES + 1
        fuser.fuse(w.kps, w.desc, np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 2)), np.zeros((n, 32), np.uint8), None, np.zeros(n), w.T, w.K,
                   w.bounds)
    with pytest.raises(orbx.OrbxError):  # the pose form needs the observation counts
        fuser.fuse(w.kps, w.desc, w.points, w.normals, w.dists, w.map_desc, None, None, w.T, w.K, w.bounds)


def test_shim_fuse_runs(orbx, tmp_path):
    """tests/cpp/shim_fuse.cpp: the shim and the C calls give the same rows, outputs and records; most points land on the feature
    that shows them."""
    exe, libdir = os.path.join(str(tmp_path), "shim_fuse"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_fuse.cpp"),
           "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    fused, right, fused_scw, replace, same = (int(v) for v in p.stdout.strip().splitlines()[-1].split()[1:])
    print(p.stdout.strip().splitlines()[-1])
    assert same == 1 and fused > 50 and right >= 0.9 * fused and fused_scw >= fused and replace > 10
