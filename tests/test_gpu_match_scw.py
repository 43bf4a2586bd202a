"""The loop-closing overload ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) on the device (orbx_match_scw*), the
composition of Scw (orbx_sim3_compose_scw*) and the chain compute_sim3_loop_pairs_device: the match rows, d_scw and every field of
orbx_scw_result but `rounds` equal the CPU restatement (tests/cpp/match_scw_ref.cpp) byte for byte on the worlds of
tests/match_scw_ref_lib.py -- the generated ones, the contention world, the hand-made order case and the rule worlds -- issued
alone, at capacities equal to the counts and at the largest ones, in one batch whose pairs share a keyframe and a map set, under
the second setting, through the host form, the Python classes and the shim, and chained behind the solver, SearchBySim3 and
OptimizeSim3 without a host pass."""
import os
import subprocess

import numpy as np
import pytest

import match_scw_ref_lib as L

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


@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, L.SCALE_FACTOR_2, L.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    assert np.asarray(e.GetScaleFactors(), np.float32).tobytes() == L.scale_table(L.NLEVELS_2, L.SCALE_FACTOR_2).tobytes()
    yield e
    e.close()


def up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Batch:
    """Keyframes, map sets and pairs in the device layout.  frames: [(kps, desc)]; sets: [(points, normals, dists, map_desc, mask |
    None)]; pairs: [(frame, set, scw [12], row on entry, table | None)].  A table is padded to the capacity with entries that name
    no point; the mask is NULL when no set gives one, the table when no pair gives one."""

    def __init__(self, torch, frames, sets, pairs, cap, mcap):
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
        scw, entry, table = np.zeros((P, 12), np.float32), np.full((P, cap), -7, np.int32), np.full((P, cap), L.NO_POINT, np.int32)
        self.tabled = [p[4] is not None for p in pairs]
        assert all(self.tabled) or not any(self.tabled)
        for p, (_, _, sc, me, tb) in enumerate(pairs):
            scw[p] = sc
            entry[p, :len(me)] = me
            if tb is not None:
                assert len(tb) <= cap
                table[p, :len(tb)] = tb
        self.kps, self.desc, self.n, self.mn, self.pts, self.nrm, self.dst, self.mdesc, self.scw = \
            (up(torch, a) for a in (kps, desc, n, mn, pts, nrm, dst, mdesc, scw))
        self.mask = up(torch, mask) if any(s[4] is not None for s in sets) else None
        self.table = up(torch, table) if any(self.tabled) else None
        self.entry = up(torch, entry).view(torch.int32)
        self.frame, self.set = (np.array([p[k] for p in pairs], np.int32) for k in range(2))
        self.matches = torch.empty(max(P, 1) * cap, dtype=torch.int32, device="cuda")
        self.res = torch.empty(max(P, 1) * NF, dtype=torch.int32, device="cuda")

    def run(self, torch, ext, K, bounds, th, th_low):
        self.matches[:self.P * self.cap].copy_(self.entry)
        self.res.fill_(-7)
        ext.match_scw_pairs_device(self.F, self.frame, self.set, self.kps, self.desc, self.n, self.S, self.mcap, self.mn, self.pts, self.nrm,
                                   self.dst, self.mdesc, self.mask, self.scw, K, bounds, self.matches, self.res, th=th, th_low=th_low,
                                   d_kf2_to_map=self.table, capacity=self.cap)
        torch.cuda.synchronize()
        return self.matches.cpu().numpy().reshape(-1, self.cap)[:self.P], self.res.cpu().numpy().reshape(-1, NF)[:self.P]


def parts(w):
    return (w.kps, w.desc), (w.points, w.normals, w.dists, w.map_desc, w.mask), (0, 0, w.scw, w.matches, w.table)


def cap_of(w, least=1):
    return max(w.n_f, w.n_table, least)


def batch_of(torch, w, cap, mcap):
    f, s, p = parts(w)
    return Batch(torch, [f], [s], [p], cap, mcap)


def check_pair(got_row, got_res, w, what):
    e = w.expected()
    res = dict(zip(L.RESULT_FIELDS, (int(v) for v in got_res)))
    print(what, "device", res, "restatement", e["res"])
    assert got_row[:w.n_f].tobytes() == e["matches"].tobytes(), what
    assert np.all(got_row[w.n_f:] == -7), what  # (nothing is written beyond the keyframe's count)
    for f in L.COMPARED_FIELDS:
        assert res[f] == e["res"][f], (what, f, res[f], e["res"][f])
    return res


@pytest.mark.parametrize("name", L.WORLDS)
def test_world_equals_restatement(torch, ext, name):
    w = L.world(name)
    b = batch_of(torch, w, 1024, 1024)
    m, r = b.run(torch, ext, w.K, w.bounds, w.th, w.th_low)
    res = check_pair(m[0], r[0], w, name)
    m2, r2 = b.run(torch, ext, w.K, w.bounds, w.th, w.th_low)
    assert m.tobytes() == m2.tobytes() and r.tobytes() == r2.tobytes(), "two runs differ"
    if name == "w513":  # (the append's second slice holds one point)
        assert w.n_m == 513 and res["rounds"] >= 1
    if name == "order":  # point 0 alone, then point 1: one point per round
        assert res["rounds"] == 2 and m[0, :2].tolist() == [0, 1]
    if name == "contention":
        assert res["n_displaced"] == 240 and res["rounds"] >= 4
    if name == "truth":
        assert all(m[0, j] == i for j, i in w.planted)


@pytest.mark.parametrize("name", sorted(L.rule_worlds()))
def test_rule_world_equals_restatement(torch, ext, name):
    w = L.rule_worlds()[name]
    m, r = batch_of(torch, w, cap_of(w, 4), max(w.n_m, 1)).run(torch, ext, w.K, w.bounds, w.th, w.th_low)
    res = check_pair(m[0], r[0], w, name)
    for f, v in L.RULE_AIMS[name].items():
        assert (res["status"] & v == v) if f == "status" else res[f] == v, (name, f, res)
    m, r = batch_of(torch, w, 64, 32).run(torch, ext, w.K, w.bounds, w.th, w.th_low)  # (a table padded with entries that name nothing)
    check_pair(m[0], r[0], w, name + " at 64 / 32")


@pytest.mark.parametrize("caps", ("exact", "largest"))
def test_capacities_and_counts(torch, orbx, ext, caps):
    """Capacities that are exactly the counts (nothing lies beyond the rows), and both at ORBX_BOW_MAX_FEATURES with counts far
    below (the kernel's LDS is sized from the capacities: 158 KB here, beyond the default limit of a launch)."""
    w = L.make_world(100, 33, edge_cases=False, n_extra=10)
    cap, mcap = (cap_of(w), w.n_m) if caps == "exact" else (orbx.BOW_MAX_FEATURES, orbx.BOW_MAX_FEATURES)
    assert orbx.BOW_MAX_FEATURES == 16384 and w.n_table > w.n_f
    m, r = batch_of(torch, w, cap, mcap).run(torch, ext, w.K, w.bounds, w.th, w.th_low)
    res = check_pair(m[0], r[0], w, caps)
    assert res["nmatches"] > 5 and res["n_found"] > 3


def test_batch_with_a_shared_keyframe_and_map_set(torch, ext):
    """One call: keyframe 0 against map set 0 under two similarities (two answers) and against map set 1; keyframe 1 against map
    set 0; a keyframe without features and an empty map set; every pair brings a table."""
    a, c = L.world("main"), L.world("bounds").variant(bounds=L.BOUNDS)
    other = L.scaled(L.pose_of(99), 0.7)
    none_k, none_d = np.zeros(0, KP), np.zeros((0, 32), np.uint8)
    z3, z2 = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
    fresh_a, fresh_c, no_table = np.full(a.n_f, -1, np.int32), np.full(c.n_f, -1, np.int32), np.zeros(0, np.int32)
    frames = [(a.kps, a.desc), (c.kps, c.desc), (none_k, none_d)]
    sets = [(a.points, a.normals, a.dists, a.map_desc, a.mask), (c.points, c.normals, c.dists, c.map_desc, c.mask), (z3, z3, z2, none_d, None)]
    pairs = [(0, 0, a.scw, a.matches, a.table), (0, 0, other, a.matches, a.table), (0, 1, c.scw, fresh_a, no_table),
             (1, 0, a.scw, fresh_c, no_table), (2, 0, a.scw, np.zeros(0, np.int32), no_table), (1, 2, c.scw, c.matches, c.table)]

    def world_of(f, s, scw, entry, table):
        (k, d), (p, nr, ds, md, m) = frames[f], sets[s]
        return L.World(k, d, p, nr, ds, md, m, scw, a.K, a.bounds, a.th, a.th_low, entry, table)
    want = [world_of(*p) for p in pairs]
    b = Batch(torch, frames, sets, pairs, 1024, 1024)
    m, r = b.run(torch, ext, a.K, a.bounds, a.th, a.th_low)
    got = [check_pair(m[p], r[p], want[p], "pair %d" % p) for p in range(len(pairs))]
    assert m[0, :a.n_f].tobytes() != m[1, :a.n_f].tobytes()  # (one keyframe, two similarities: two answers)
    assert got[0]["nmatches"] > 40 and got[0]["n_unmapped"] > 0 and got[4]["n_total"] == 0 and got[5]["n_points"] == 0
    for p in (0, 1, 3):  # every pair issued alone gives its row of the batch
        one = Batch(torch, frames, sets, pairs[p:p + 1], 1024, 1024)
        m1, r1 = one.run(torch, ext, a.K, a.bounds, a.th, a.th_low)
        assert m1[0].tobytes() == m[p].tobytes() and r1[0, :NF - 1].tobytes() == r[p, :NF - 1].tobytes(), p


def test_second_setting_anisotropic_camera_and_five_levels(torch, ext2):
    """The maps of 150 and 310 points under K_ANISO and five levels of 1.37 in one batch under the offset bounds (a call has one
    set of bounds: the smaller scene's restatement runs under them too), then the smaller one through the host form."""
    a, b = L.world("w150@2"), L.world("w310_bounds@2")
    a_off = a.variant(bounds=b.bounds)
    fa, sa, _ = parts(a)
    fb, sb, _ = parts(b)
    pairs = [(0, 0, a.scw, a.matches, a.table), (1, 1, b.scw, b.matches, b.table)]
    cap = max(cap_of(a), cap_of(b))
    m, r = Batch(torch, [fa, fb], [sa, sb], pairs, cap, 310).run(torch, ext2, b.K, b.bounds, b.th, b.th_low)
    for p, w in enumerate((a_off, b)):
        res = check_pair(m[p], r[p], w, "pair %d" % p)
        assert res["status"] == 0 and res["nmatches"] >= 8 and res["n_out_image"] > 10 and res["n_out_angle"] > 5
    e = a.expected()
    mh, rh = ext2.match_scw(a.kps, a.desc, a.points, a.normals, a.dists, a.map_desc, a.mask, a.scw, a.K, a.bounds, a.matches, a.th, a.th_low,
                            a.table)
    assert mh.tobytes() == e["matches"].tobytes()
    assert {f: x for f, x in rh.as_dict().items() if f != "rounds"} == {f: e["res"][f] for f in L.COMPARED_FIELDS}


def test_host_form_and_classes(orbx, torch, ext):
    names = [("world", n) for n in ("main", "main_no_table", "order")] + [("rule", n) for n in ("table_beyond", "no_features", "no_points")]
    for kind, name in names:
        w = L.world(name) if kind == "world" else L.rule_worlds()[name]
        e = w.expected()
        m, res = ext.match_scw(w.kps, w.desc, w.points, w.normals, w.dists, w.map_desc, w.mask, w.scw, w.K, w.bounds, w.matches, w.th,
                               w.th_low, w.table)
        assert m.tobytes() == e["matches"].tobytes(), name
        assert {f: v for f, v in res.as_dict().items() if f != "rounds"} == {f: e["res"][f] for f in L.COMPARED_FIELDS}, name
        F = orbx.Frame.from_arrays(w.kps, w.desc, w.bounds)
        S44 = np.eye(4, dtype=np.float32)
        S44[:3, :3], S44[:3, 3] = w.scw[:9].reshape(3, 3), w.scw[9:]
        nm, m2, res2 = orbx.ORBmatcher(0.75, True, extractor=ext).SearchByProjectionScw(
            F, S44, w.points, w.normals, w.dists, w.map_desc, w.mask, w.matches, w.th, K=w.K.reshape(3, 3), th_low=w.th_low,
            kf2_to_map=w.table)
        assert nm == e["res"]["nmatches"] and m2.tobytes() == m.tobytes() and bytes(res2) == bytes(res), name


def test_composition_equals_restatement(orbx, torch, ext):
    """orbx_sim3_compose_scw*: 70 pairs over 5 poses (more than one workgroup of lanes), some without a similarity."""
    rng = np.random.default_rng(8)
    poses = np.stack([L.pose_of(300 + k) for k in range(5)])
    kf2 = rng.integers(0, 5, 70).astype(np.int32)
    sims = np.stack([np.r_[L.pose_of(400 + k)[:9], rng.uniform(-5, 5, 3), rng.uniform(0.3, 4.0)] for k in range(70)]).astype(np.float32)
    sims[3] = 0.0            # a pair without a similarity
    sims[17, 12] = -1.0
    sims[40, 4] = np.nan
    sims[41, 12] = np.inf
    want = np.stack([L.compose_scw(poses[kf2[p]], sims[p]) for p in range(70)])
    assert not want[[3, 17, 40, 41]].any() and want[0].any()
    d_pose, d_sim = up(torch, poses), up(torch, sims)
    d_scw = torch.full((70 * 48,), 0xA5, dtype=torch.uint8, device="cuda")
    ext.sim3_compose_scw_pairs_device(5, kf2, d_pose, d_sim, d_scw)
    torch.cuda.synchronize()
    assert d_scw.cpu().numpy().tobytes() == want.tobytes()
    for p in (0, 3, 40):
        assert ext.sim3_compose_scw(poses[kf2[p]], sims[p]).tobytes() == want[p].tobytes()
        T44 = np.eye(4, dtype=np.float32)  # the pose as a matrix: R and t are taken apart, not read row by row
        T44[:3, :3], T44[:3, 3] = poses[kf2[p]][:9].reshape(3, 3), poses[kf2[p]][9:]
        assert ext.sim3_compose_scw(T44, sims[p]).tobytes() == ext.sim3_compose_scw(T44[:3], sims[p]).tobytes() == want[p].tobytes()
    with pytest.raises(orbx.OrbxError):
        ext.sim3_compose_scw_pairs_device(5, np.array([5], np.int32), d_pose, d_sim, d_scw)


def test_fixed_seed_slice_of_generated_worlds(torch, ext):
    """Eight generated worlds of 64 to 220 points under scales from 0.5 to 3, one batch, seeds fixed."""
    rng = np.random.default_rng(2024)
    worlds = [L.make_world(int(rng.integers(64, 221)), 500 + k, s=float(rng.uniform(0.5, 3.0)), edge_cases=k % 2 == 0, n_extra=12)
              for k in range(8)]
    frames, sets = [parts(w)[0] for w in worlds], [parts(w)[1] for w in worlds]
    pairs = [(k, k, w.scw, w.matches, w.table) for k, w in enumerate(worlds)]
    cap, mcap = max(cap_of(w) for w in worlds), max(w.n_m for w in worlds)
    m, r = Batch(torch, frames, sets, pairs, cap, mcap).run(torch, ext, worlds[0].K, L.BOUNDS, 10.0, L.TH_LOW)
    total = sum(check_pair(m[k], r[k], w, "seed %d" % (500 + k))["nmatches"] for k, w in enumerate(worlds))
    assert total > 50


@pytest.mark.parametrize("name", L.CHAIN_WORLDS)
def test_chain_equals_the_four_restatements(orbx, torch, ext, name):
    """compute_sim3_loop_pairs_device: the solver, SearchBySim3 and OptimizeSim3 leave d_sim3 and the row; the composition writes
    d_scw; this matcher translates the row through d_kf2_to_map and extends it -- no copy and no wait between them.  Equal to the
    four restatements chained, the decision included."""
    import sim3opt_ref_lib as O
    c = L.chain_world(name)
    mw, cap, e = c.mw, c.mw.cap, c.expected()
    d = lambda a: up(torch, a)  # noqa: E731
    col = lambda a: d(np.stack(a))  # noqa: E731
    z = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_sres, d_sim, d_row, d_mres = z(orbx.SIM3_RESULT_DTYPE.itemsize), z(52), z(cap * 4), z(orbx.MSIM3_RESULT_DTYPE.itemsize)
    d_ores, d_scw, d_scw_res = z(orbx.SIM3OPT_RESULT_DTYPE.itemsize), z(48), z(orbx.SCW_RESULT_DTYPE.itemsize)
    one, two = np.array([0], np.int32), np.array([1], np.int32)
    ext.compute_sim3_loop_pairs_device(2, one, two, one, two, col(mw.kps), col(mw.desc), d(np.array(mw.n, np.int32)), d(mw.match), 2,
                                       col(mw.points), col(mw.mask), col(mw.dist), col(mw.pose), mw.K, mw.bounds, d(c.draws), d_sres, d_sim,
                                       d_row, d_mres, d_ores, one, 1, cap, d(np.array([c.map_n], np.int32)), d(c.map_points),
                                       d(c.map_normals), d(c.map_dist), d(c.map_desc), d(c.map_mask), d(c.table), d_scw, d_scw_res,
                                       capacity=cap)
    # the decision straight behind the chain: nothing here waits for the device, the helper orders its own read-back
    accepted = ext.loop_accepted(d_ores, d_scw_res)
    assert accepted.tolist() == [e["accepted"]] == [name == "accepted"]
    torch.cuda.synchronize()
    ores = d_ores.cpu().numpy().view(orbx.SIM3OPT_RESULT_DTYPE)
    for f in O.SIM3OPT_RESULT_DTYPE.names:
        assert np.asarray(ores[0][f]).tobytes() == np.asarray(e["opt"][f]).tobytes(), (name, f)
    assert d_sim.cpu().numpy().tobytes() == e["sim"].tobytes()
    assert d_scw.cpu().numpy().tobytes() == e["scw"].tobytes()
    assert d_row.cpu().numpy().tobytes() == e["row"].tobytes()
    sres = d_scw_res.cpu().numpy().view(orbx.SCW_RESULT_DTYPE)
    got = {f: int(sres[0][f]) for f in L.COMPARED_FIELDS}
    print(name, "nInliers", int(ores[0]["n_inliers"]), got)
    assert got == {f: e["scw_res"][f] for f in L.COMPARED_FIELDS}
    assert orbx.loop_accepted(ores, sres).tolist() == ext.loop_accepted(ores, sres).tolist() == accepted.tolist()
    with pytest.raises(orbx.OrbxError):  # (the module function orders nothing: it takes host records only)
        orbx.loop_accepted(d_ores, d_scw_res)
    if name == "accepted":
        assert got["nmatches"] == c.n_neighbours and got["n_unmapped"] == 5 and got["n_total"] >= 40
    if name == "few_inliers":
        assert ores[0]["n_inliers"] < 20 and got["status"] & L.NONFINITE
    if name == "few_total":
        assert ores[0]["n_inliers"] >= 20 and got["n_total"] < 40 and got["nmatches"] > 0


def test_refusals(orbx, torch, ext):
    w = L.world("order")
    b = batch_of(torch, w, 64, 32)
    lib, p = orbx.lib(), orbx._ptr
    K = np.ascontiguousarray(w.K, np.float32)
    b.matches.fill_(-1)
    b.res.fill_(-7)

    def call(frame=0, mset=0, cap=64, mcap=32, th=10.0, th_low=50, bounds=(0, 640, 0, 480), ctx=ext._h, n_pairs=1, matches=b.matches,
             scw=b.scw):
        hf, hs = np.array([frame], np.int32), np.array([mset], np.int32)  # (named: they outlive the call)
        bb = orbx._Bounds(*bounds)
        return lib.orbx_match_scw_batch_device(ctx, 1, n_pairs, p(hf), p(hs), p(b.kps), p(b.desc), p(b.n), cap, 1, mcap, p(b.mn), p(b.pts),
                                               p(b.nrm), p(b.dst), p(b.mdesc), None, p(scw), p(K), orbx.ctypes.byref(bb), th, th_low,
                                               p(matches), None, p(b.res))
    assert call(n_pairs=0) == 0
    torch.cuda.synchronize()
    assert int(b.res[0]) == -7  # (nothing ran)
    bad, full = orbx.E_BADARG, orbx.E_CAPACITY
    assert call(frame=1) == bad and call(frame=-1) == bad and call(mset=1) == bad and call(matches=None) == bad and call(scw=None) == bad
    assert call(th=0.0) == bad and call(th=-1.0) == bad and call(th=float("nan")) == bad and call(th=float("inf")) == bad
    assert call(th_low=-1) == bad and call(th_low=257) == bad
    assert call(bounds=(5, 5, 0, 480)) == bad and call(bounds=(0, 640, 10, 9)) == bad
    assert call(cap=orbx.BOW_MAX_FEATURES + 1) == full and call(mcap=orbx.BOW_MAX_FEATURES + 1) == full
    assert call(cap=0) == bad and call(mcap=0) == bad and call(n_pairs=-1) == bad
    assert call(ctx=None) == orbx.E_HIP and call(ctx=None, th_low=300) == bad  # (the arguments are judged first)
    cl = lib.orbx_sim3_compose_scw_batch_device
    one, far = np.array([0], np.int32), np.array([1], np.int32)
    assert cl(ext._h, 1, 1, p(far), p(b.scw), p(b.scw), p(b.scw)) == bad and cl(ext._h, 1, 1, p(one), None, p(b.scw), p(b.scw)) == bad
    assert cl(None, 1, 1, p(one), p(b.scw), p(b.scw), p(b.scw)) == orbx.E_HIP and cl(ext._h, 1, 0, None, p(b.scw), p(b.scw), p(b.scw)) == 0
    torch.cuda.synchronize()
    assert int(b.res[0]) == -7 and bool((b.matches == -1).all())  # (no refusal touched the device)
    assert call(th_low=256) == 0  # (the largest threshold)
    torch.cuda.synchronize()
    assert int(b.res[1]) == 2 and b.matches[:2].tolist() == [0, 1]
    # the binding's size checks come before anything is issued
    short = torch.zeros(10, dtype=torch.int32, device="cuda")
    args = lambda **kw: dict(dict(n_frames=1, kf=[0], map_set=[0], d_kps_un=b.kps, d_desc=b.desc, d_n=b.n, n_map_sets=1, map_capacity=32,  # noqa: E731
                                  d_map_n=b.mn, d_map_points=b.pts, d_map_normals=b.nrm, d_map_dist=b.dst, d_map_desc=b.mdesc, d_map_mask=None,
                                  d_scw=b.scw, K=K, bounds=w.bounds, d_matches=b.matches, d_res=b.res, capacity=64), **kw)
    for kw in (dict(d_matches=short), dict(d_res=short[:4]), dict(kf=[1]), dict(map_set=[2]), dict(d_kf2_to_map=short), dict(d_scw=short[:2]),
               dict(d_map_normals=short)):
        with pytest.raises(ValueError):
            ext.match_scw_pairs_device(**args(**kw))
    with pytest.raises(orbx.OrbxError):  # more table entries than ORBX_BOW_MAX_FEATURES
        ext.match_scw(w.kps, w.desc, w.points, w.normals, w.dists, w.map_desc, None, w.scw, w.K, w.bounds,
                      kf2_to_map=np.zeros(orbx.BOW_MAX_FEATURES + 1, np.int32))


def test_shim_match_scw_runs(orbx, tmp_path):
    """tests/cpp/shim_match_scw.cpp: the shim and the C call give the same row and record, most new matches the true ones."""
    exe, libdir = os.path.join(str(tmp_path), "shim_match_scw"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_match_scw.cpp"),
           "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    nm, right, searched, total, same = (int(v) for v in p.stdout.strip().splitlines()[-1].split()[1:])
    print(p.stdout.strip().splitlines()[-1])
    assert same == 1 and nm > 50 and right >= 0.9 * nm and total >= nm and searched >= nm
