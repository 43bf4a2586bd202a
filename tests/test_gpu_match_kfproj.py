"""The relocalisation overload ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) on the device
(orbx_match_keyframe_projection*): the match rows and every field of orbx_kfproj_result but `rounds` equal the CPU restatement
(tests/cpp/match_kfproj_ref.cpp) byte for byte on the worlds of tests/match_kfproj_ref_lib.py -- the generated ones, the
contention world, the hand-made order case and the rule worlds -- issued alone, at a capacity equal to the counts and at the
largest one, in one batch whose pairs share frames, through the host form, the Python classes and the shim, and through the tail of
Relocalization (relocalize_refine_pairs_device) against the same chain of restatements."""
import os
import subprocess

import numpy as np
import pytest

import match_kfproj_ref_lib as L

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
    """Frames, point sets and pairs in the device layout.  frames: [(kps, desc)]; sets: [(points, dists, mask | None, point_desc |
    None)]; pairs: [(keyframe, current frame, point set, pose [12], matches on entry, outlier | None)].  An array that no set /
    pair gives is passed as NULL."""

    def __init__(self, torch, frames, sets, pairs, cap):
        self.cap, self.P, self.F, self.S = cap, len(pairs), len(frames), len(sets)
        F, S, P = self.F, self.S, self.P
        kps, desc, n = np.zeros((F, cap), KP), np.zeros((F, cap, 32), np.uint8), np.zeros(F, np.int32)
        for f, (k, d) in enumerate(frames):
            n[f] = len(k)
            kps[f, :len(k)], desc[f, :len(k)] = k, d
        pts, dst = np.zeros((S, cap, 3), np.float32), np.zeros((S, cap, 2), np.float32)
        pdesc, mask = np.zeros((S, cap, 32), np.uint8), np.ones((S, cap), np.uint8)
        for s, (p, ds, m, pd) in enumerate(sets):
            pts[s, :len(p)], dst[s, :len(p)] = p, ds
            if m is not None:
                mask[s, :len(m)] = m
            if pd is not None:
                pdesc[s, :len(pd)] = pd
        pose, outl, entry = np.zeros((P, 12), np.float32), np.zeros((P, cap), np.uint8), np.full((P, cap), -7, np.int32)
        for p, (_, _, _, ps, me, o) in enumerate(pairs):
            pose[p] = ps
            entry[p, :len(me)] = me
            if o is not None:
                outl[p, :len(o)] = o
        self.kps, self.desc, self.n, self.pts, self.dst, self.pose = (up(torch, a) for a in (kps, desc, n, pts, dst, pose))
        self.mask = up(torch, mask) if any(s[2] is not None for s in sets) else None
        self.pdesc = up(torch, pdesc) if any(s[3] is not None for s in sets) else None
        self.outl = up(torch, outl) if any(p[5] is not None for p in pairs) else None
        self.entry = up(torch, entry).view(torch.int32)
        self.kf, self.cur, self.set = (np.array([p[k] for p in pairs], np.int32) for k in range(3))
        self.matches = torch.empty(max(P, 1) * cap, dtype=torch.int32, device="cuda")
        self.res = torch.empty(max(P, 1) * NF, dtype=torch.int32, device="cuda")

    def run(self, torch, ext, K, bounds, th, orb_dist, ori):
        self.matches[:self.P * self.cap].copy_(self.entry)
        self.res.fill_(-7)
        ext.match_keyframe_projection_pairs_device(self.F, self.kf, self.cur, self.set, self.kps, self.desc, self.n, self.S, self.pts,
                                                   self.mask, self.dst, self.pose, K, bounds, self.matches, self.res, th=th,
                                                   ORBdist=orb_dist, checkOri=ori, d_point_desc=self.pdesc, d_outlier=self.outl,
                                                   capacity=self.cap)
        torch.cuda.synchronize()
        return self.matches.cpu().numpy().reshape(-1, self.cap)[:self.P], self.res.cpu().numpy().reshape(-1, NF)[:self.P]


def batch_of(torch, w, cap):
    return Batch(torch, [(w.kps_k, w.desc_k), (w.kps_c, w.desc_c)], [(w.points, w.dists, w.mask, w.point_desc)],
                 [(0, 1, 0, w.pose, w.matches, w.outlier)], cap)


def run_world(torch, ext, w, cap):
    return batch_of(torch, w, cap).run(torch, ext, w.K, w.bounds, w.th, w.orb_dist, w.ori)


def check_pair(got_row, got_res, w, what):
    e = w.expected()
    res = dict(zip(L.RESULT_FIELDS, (int(v) for v in got_res)))
    print(what, "device", res, "restatement", e["res"])
    assert got_row[:w.n_c].tobytes() == e["matches"].tobytes(), what
    assert np.all(got_row[w.n_c:] == -7), what  # (nothing is written beyond the frame's count)
    for f in L.COMPARED_FIELDS:
        assert res[f] == e["res"][f], (what, f, res[f], e["res"][f])
    return res


@pytest.mark.parametrize("name", L.WORLDS)
def test_world_equals_restatement(torch, ext, name):
    w = L.world(name)
    b = batch_of(torch, w, 1024)
    m, r = b.run(torch, ext, w.K, w.bounds, w.th, w.orb_dist, w.ori)
    res = check_pair(m[0], r[0], w, name)
    m2, r2 = b.run(torch, ext, w.K, w.bounds, w.th, w.orb_dist, w.ori)
    assert m.tobytes() == m2.tobytes() and r.tobytes() == r2.tobytes(), "two runs differ"
    if name == "w700":
        assert w.n_k > 512 and res["rounds"] >= 1
    if name == "order":  # the hand-made case: 0 and 2 cannot both be decided in the round in which 1 still waits for A
        assert res["rounds"] > 1 and m[0, :2].tolist() == [0, 1]
    if name == "contention":
        assert 2 * res["n_displaced"] >= res["n_points"] and res["rounds"] >= 4
    if name == "empty_keyframe":
        assert res["rounds"] == 0 and res["nmatches"] == 0
    if name == "empty_frame":  # (the searched points find no candidate in their first round)
        assert res["rounds"] == 1 and res["nmatches"] == 0 and res["n_points"] > 0


@pytest.mark.parametrize("name", list(L.rule_worlds()))
def test_rule_world_equals_restatement(torch, ext, name):
    w = L.rule_worlds()[name]
    m, r = run_world(torch, ext, w, 64)
    check_pair(m[0], r[0], w, name)


@pytest.mark.parametrize("caps", ("exact", "largest"))
def test_capacities_and_counts(torch, orbx, ext, caps):
    """A capacity that is exactly the larger count (nothing lies beyond the rows), and ORBX_BOW_MAX_FEATURES with counts far below
    (the kernel's LDS is sized from the capacity: 158 KB here)."""
    w = L.make_world(240, 31)
    cap = max(w.n_k, w.n_c) if caps == "exact" else orbx.BOW_MAX_FEATURES
    assert orbx.BOW_MAX_FEATURES == 16384 and w.n_k != w.n_c
    m, r = run_world(torch, ext, w, cap)
    res = check_pair(m[0], r[0], w, caps)
    assert res["nmatches"] > 15


def test_batch_with_shared_frames(torch, ext):
    """One call: the current frame 0 against three keyframes under three poses; a keyframe that is also a current frame; an empty
    frame on either side.  Pair 0 brings outlier flags and entry matches, the others' rows are fresh."""
    a, c, d = L.world("main"), L.world("bounds"), L.world("w700")
    none_k, none_d = L._none_frame()
    frames = [(a.kps_c, a.desc_c), (a.kps_k, a.desc_k), (c.kps_k, c.desc_k), (d.kps_k, d.desc_k), (none_k, none_d)]
    sets = [(a.points, a.dists, a.mask, None), (c.points, c.dists, c.mask, None), (d.points, d.dists, d.mask, None),
            (np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), None, None)]
    fresh = lambda n: np.full(n, -1, np.int32)  # noqa: E731
    pairs = [(1, 0, 0, a.pose, a.matches, a.outlier), (2, 0, 1, c.pose, fresh(a.n_c), None), (3, 0, 2, d.pose, fresh(a.n_c), None),
             (2, 1, 1, L.pose_of(99), fresh(a.n_k), None),  # frame 1, a keyframe above, is the current frame here
             (4, 0, 3, a.pose, fresh(a.n_c), None), (1, 4, 0, a.pose, np.zeros(0, np.int32), None)]

    def world_of(fk, fc, s, pose, entry, outl):
        (kk, dk), (kc, dc), (p, ds, m, pd) = frames[fk], frames[fc], sets[s]
        return L.World(kk, dk, kc, dc, p, ds, m, pose, a.K, a.bounds, a.th, a.orb_dist, a.ori, pd, entry, outl)
    want = [world_of(*p) for p in pairs]
    b = Batch(torch, frames, sets, pairs, 1024)
    m, r = b.run(torch, ext, a.K, a.bounds, a.th, a.orb_dist, a.ori)
    got = [check_pair(m[p], r[p], want[p], "pair %d" % p) for p in range(len(pairs))]
    assert got[0]["nmatches"] > 40 and got[0]["n_found"] > 5 and got[4]["n_points"] == 0 and got[5]["nmatches"] == 0 and got[5]["n_points"] > 0
    assert len({m[p, :a.n_c].tobytes() for p in range(3)}) == 3  # (one frame, three keyframes: three answers)
    # every pair issued alone gives its row of the batch
    for p in (0, 1, 3):
        one = Batch(torch, frames, sets, pairs[p:p + 1], 1024)
        m1, r1 = one.run(torch, ext, a.K, a.bounds, a.th, a.orb_dist, a.ori)
        assert m1[0].tobytes() == m[p].tobytes() and r1[0, :NF - 1].tobytes() == r[p, :NF - 1].tobytes(), p


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
    """The keyframes of 150 and 310 features under K_ANISO in one batch at the capacity of the largest count, under the offset
    bounds (a call has one set of bounds: the smaller scene's restatement runs under them too); then the smaller scene alone
    at its own largest count under the usual bounds, through the batch and the host form."""
    a, b = L.world("w150@2"), L.world("w310_bounds@2")
    assert a.n_k == 150 and b.n_k == 310 and b.bounds == BOUNDS_2 and len(a.scale) == L.NLEVELS_2
    a_off = a.variant(bounds=BOUNDS_2)
    frames = [(a.kps_k, a.desc_k), (a.kps_c, a.desc_c), (b.kps_k, b.desc_k), (b.kps_c, b.desc_c)]
    sets = [(a.points, a.dists, a.mask, None), (b.points, b.dists, b.mask, None)]
    pairs = [(0, 1, 0, a.pose, a.matches, a.outlier), (2, 3, 1, b.pose, b.matches, b.outlier)]
    cap = max(b.n_k, b.n_c)
    m, r = Batch(torch, frames, sets, pairs, cap).run(torch, ext2, b.K, BOUNDS_2, b.th, b.orb_dist, b.ori)
    for p, w in enumerate((a_off, b)):
        res = check_pair(m[p], r[p], w, "pair %d" % p)
        # not trivial: matches found, points rejected outside the image and by distance, windows with candidates
        assert res["status"] == 0 and res["nmatches"] > 20 and res["n_out_image"] > 10 and res["n_out_distance"] > 10
        assert res["n_with_candidates"] > 30
    m1, r1 = run_world(torch, ext2, a, max(a.n_k, a.n_c))
    check_pair(m1[0], r1[0], a, "alone")
    e = a.expected()
    T = np.c_[a.pose[:9].reshape(3, 3), a.pose[9:]]
    mh, rh = ext2.match_keyframe_projection(a.kps_k, a.desc_k, a.kps_c, a.desc_c, a.points, a.mask, a.dists, T, a.K, a.bounds, a.matches,
                                            a.th, a.orb_dist, a.ori, a.point_desc, a.outlier)
    assert mh.tobytes() == e["matches"].tobytes()
    assert {f: x for f, x in rh.as_dict().items() if f != "rounds"} == {f: e["res"][f] for f in L.COMPARED_FIELDS}


def test_host_form_and_classes(orbx, torch, ext):
    for name in ("main", "main_th3", "pdesc", "order", "empty_frame", "empty_keyframe"):
        w = L.world(name)
        e = w.expected()
        T = np.c_[w.pose[:9].reshape(3, 3), w.pose[9:]]
        m, res = ext.match_keyframe_projection(w.kps_k, w.desc_k, w.kps_c, w.desc_c, w.points, w.mask, w.dists, T, w.K, w.bounds, w.matches,
                                               w.th, w.orb_dist, w.ori, w.point_desc, w.outlier)
        assert m.tobytes() == e["matches"].tobytes(), name
        assert {f: v for f, v in res.as_dict().items() if f != "rounds"} == {f: e["res"][f] for f in L.COMPARED_FIELDS}, name
        C, KF = orbx.Frame.from_arrays(w.kps_c, w.desc_c, w.bounds), orbx.Frame.from_arrays(w.kps_k, w.desc_k, w.bounds)
        nm, m2, res2 = orbx.ORBmatcher(0.9, w.ori, extractor=ext).SearchByProjectionKeyFrame(
            C, KF, w.points, w.mask, w.dists, T, w.th, w.orb_dist, K=w.K.reshape(3, 3), matches=w.matches, outlier=w.outlier,
            point_desc=w.point_desc)
        assert nm == e["res"]["nmatches"] and m2.tobytes() == m.tobytes() and bytes(res2) == bytes(res), name


def test_relocalization_tail_equals_the_chain_of_restatements(orbx, torch, ext):
    """relocalize_refine_pairs_device on four candidate keyframes against one lost frame, in one batch: the stage each pair
    reaches, nGood, the pose and the row equal pose_ref -> match_kfproj_ref -> pose_ref -> match_kfproj_ref -> pose_ref byte for
    byte.  (tests/test_match_kfproj_host.py asserts that the CPU chain takes each of the four paths.)"""
    cap = L.CHAIN_CAP
    worlds = [L.chain_world(name) for name in L.CHAIN]
    want = [L.relocalize_refine(*cw) for cw in worlds]
    assert [a["stage"] for a in want] == [1, 1, 5, 2]
    w0 = worlds[0][0]
    frames = [(w0.kps_c, w0.desc_c)] + [(w.kps_k, w.desc_k) for w, _, _, _ in worlds]
    sets = [(w.points, w.dists, None, None) for w, _, _, _ in worlds]
    pairs = [(1 + k, 0, k, pose0, row, None) for k, (_, pose0, row, _) in enumerate(worlds)]
    b = Batch(torch, frames, sets, pairs, cap)
    rows = b.entry.clone()
    rows[rows == -7] = -1
    stage, n_good, pose, out = ext.relocalize_refine_pairs_device(b.F, b.kf, b.cur, b.set, b.kps, b.desc, b.n, b.S, b.pts, None, b.dst,
                                                                  b.pose, rows, w0.K, w0.bounds, capacity=cap)
    torch.cuda.synchronize()
    got_rows, got_pose = out.cpu().numpy().reshape(-1, cap), pose.cpu().numpy()
    for k, (name, a) in enumerate(zip(L.CHAIN, want)):
        print(name, "device", int(stage[k]), int(n_good[k]), "restatement", a["stage"], a["n_good"], a["trace"])
        assert int(stage[k]) == a["stage"] and int(n_good[k]) == a["n_good"], name
        assert got_pose[k].tobytes() == a["pose"].tobytes(), name
        assert got_rows[k, :w0.n_c].tobytes() == a["row"].tobytes() and np.all(got_rows[k, w0.n_c:] == -1), name


def test_refusals(orbx, torch, ext):
    w = L.world("order")
    b = batch_of(torch, w, 64)
    lib, p = orbx.lib(), orbx._ptr
    K = np.ascontiguousarray(w.K, np.float32)
    b.matches.fill_(-1)
    b.res.fill_(-7)

    def call(kf=0, cur=1, pset=0, cap=64, th=15.0, orb_dist=100, bounds=(0, 640, 0, 480), ctx=ext._h, n_pairs=1, matches=b.matches, dist=b.dst):
        hk, hc, hs = np.array([kf], np.int32), np.array([cur], np.int32), np.array([pset], np.int32)  # (named: they outlive the call)
        bb = orbx._Bounds(*bounds)
        return lib.orbx_match_keyframe_projection_batch_device(ctx, 2, n_pairs, p(hk), p(hc), p(hs), p(b.kps), p(b.desc), p(b.n), cap, 1,
                                                               p(b.pts), None, None, p(dist), p(b.pose), p(K), orbx.ctypes.byref(bb), th,
                                                               orb_dist, 1, p(matches), None, p(b.res))
    assert call(n_pairs=0) == 0
    torch.cuda.synchronize()
    assert int(b.res[0]) == -7  # (nothing ran)
    bad, full = orbx.E_BADARG, orbx.E_CAPACITY
    assert call(kf=2) == bad and call(cur=-1) == bad and call(pset=1) == bad and call(matches=None) == bad and call(dist=None) == bad
    assert call(th=0.0) == bad and call(th=-1.0) == bad and call(th=float("nan")) == bad and call(th=float("inf")) == bad
    assert call(orb_dist=-1) == bad and call(orb_dist=257) == bad
    assert call(bounds=(5, 5, 0, 480)) == bad and call(bounds=(0, 640, 10, 9)) == bad
    assert call(cap=orbx.BOW_MAX_FEATURES + 1) == full and call(cap=0) == bad and call(n_pairs=-1) == bad
    assert call(ctx=None) == orbx.E_HIP and call(ctx=None, orb_dist=300) == bad  # (the arguments are judged first)
    torch.cuda.synchronize()
    assert int(b.res[0]) == -7 and bool((b.matches == -1).all())  # (no refusal touched the device)
    assert call(orb_dist=256) == 0  # (the largest threshold)
    torch.cuda.synchronize()
    assert int(b.res[1]) == 2 and b.matches[:2].tolist() == [0, 1]
    # the binding's size checks come before anything is issued
    short = torch.zeros(10, dtype=torch.int32, device="cuda")
    args = lambda **kw: dict(dict(n_frames=2, kf=[0], cur=[1], point_set=[0], d_kps_un=b.kps, d_desc=b.desc, d_n=b.n, n_point_sets=1,  # noqa: E731
                                  d_points=b.pts, d_point_mask=None, d_point_dist=b.dst, d_pose=b.pose, K=K, bounds=w.bounds,
                                  d_matches=b.matches, d_res=b.res, capacity=64), **kw)
    for kw in (dict(d_matches=short), dict(d_res=short[:4]), dict(kf=[2]), dict(point_set=[1]), dict(d_point_dist=short),
               dict(d_outlier=torch.zeros(8, dtype=torch.uint8, device="cuda")), dict(d_point_desc=torch.zeros(8, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            ext.match_keyframe_projection_pairs_device(**args(**kw))


def test_shim_match_kfproj_runs(orbx, tmp_path):
    """tests/cpp/shim_match_kfproj.cpp: the shim's two forms and the C call give the same rows, most new matches the true ones."""
    exe, libdir = os.path.join(str(tmp_path), "shim_match_kfproj"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_match_kfproj.cpp"),
           "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    nm, right, searched, same = (int(v) for v in p.stdout.strip().splitlines()[-1].split()[1:])
    assert same == 1 and searched > 50 and nm > 0.7 * searched and right > 0.9 * nm, p.stdout
