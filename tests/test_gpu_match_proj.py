"""ORBmatcher::SearchByProjection on the device (orbx_match_projection*): the rows of matches_cur and every field of
orbx_proj_result but `rounds` equal the CPU restatement (tests/cpp/match_proj_ref.cpp) byte for byte on the worlds of
tests/match_proj_ref_lib.py -- the generated ones (300 features, 1500, other bounds, map-point descriptors, th 30), the truth
world, the hand-made order case, the contention world and the rule worlds -- issued alone, at a capacity above the counts, in
one batch whose pairs share frames, through the host form and the Python classes, and chained into PoseOptimization without a
host pass."""
import os
import subprocess

import numpy as np
import pytest

import match_proj_ref_lib as M
import pose_ref_lib as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP = M.KEYPOINT_DTYPE


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    assert np.asarray(e.GetScaleFactors(), np.float32).tobytes() == M.scale_table().tobytes()
    yield e
    e.close()


class Batch:
    """Frames, point sets and pairs in the device layout.  frames: [(kps, desc)]; sets: [(points, mask | None, point_desc |
    None)]; pairs: [(last, cur, set, pose [12], outlier | None)].  An array that no set / pair gives is passed as NULL."""

    def __init__(self, torch, frames, sets, pairs, cap):
        self.cap, self.P = cap, len(pairs)
        F, S, P = len(frames), len(sets), len(pairs)
        kps, desc, n = np.zeros((F, cap), KP), np.zeros((F, cap, 32), np.uint8), np.zeros(F, np.int32)
        for f, (k, d) in enumerate(frames):
            n[f] = len(k)
            kps[f, :len(k)], desc[f, :len(k)] = k, d
        pts, mask, pdesc = np.zeros((S, cap, 3), np.float32), np.ones((S, cap), np.uint8), np.zeros((S, cap, 32), np.uint8)
        for s, (p, m, pd) in enumerate(sets):
            pts[s, :len(p)] = p
            if m is not None:
                mask[s, :len(m)] = m
            if pd is not None:
                pdesc[s, :len(pd)] = pd
        pose, outl = np.zeros((P, 12), np.float32), np.zeros((P, cap), np.uint8)
        for p, (_, _, _, ps, o) in enumerate(pairs):
            pose[p] = ps
            if o is not None:
                outl[p, :len(o)] = o
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
        self.n_host, self.kps_host, self.pts_host, self.mask_host = n, kps, pts, mask
        self.kps, self.desc, self.n, self.pts, self.pose = up(kps), up(desc), up(n), up(pts), up(pose)
        self.mask = up(mask) if any(m is not None for _, m, _ in sets) else None
        self.pdesc = up(pdesc) if any(pd is not None for _, _, pd in sets) else None
        assert self.pdesc is None or all(pd is not None for _, _, pd in sets)
        self.outl = up(outl) if any(o is not None for *_, o in pairs) else None
        self.last, self.cur, self.set = (np.array([p[k] for p in pairs], np.int32) for k in range(3))
        self.F, self.S = F, S
        self.matches = torch.full((max(P, 1) * cap,), -7, dtype=torch.int32, device="cuda")
        self.res = torch.full((max(P, 1) * 8,), -7, dtype=torch.int32, device="cuda")

    def run(self, torch, ext, K, bounds, th, ori):
        self.matches.fill_(-7)
        self.res.fill_(-7)
        ext.match_projection_pairs_device(self.F, self.last, self.cur, self.set, self.kps, self.desc, self.n, self.S, self.pts, self.mask,
                                          self.pose, K, bounds, self.matches, self.res, th=th, checkOri=ori, d_point_desc=self.pdesc,
                                          d_last_outlier=self.outl, capacity=self.cap)
        torch.cuda.synchronize()
        return self.matches.cpu().numpy().reshape(-1, self.cap)[:self.P], self.res.cpu().numpy().reshape(-1, 8)[:self.P]


def batch_of(torch, w, cap):
    return Batch(torch, [(w.kps_l, w.desc_l), (w.kps_c, w.desc_c)], [(w.points, w.mask, w.point_desc)], [(0, 1, 0, w.pose, w.outlier)], cap)


def check_pair(got_row, got_res, w, what):
    e = w.expected()
    res = dict(zip(M.RESULT_FIELDS, (int(v) for v in got_res)))
    print(what, "device", res, "restatement", e["res"])
    assert got_row[:w.n_c].tobytes() == e["matches"].tobytes(), what
    assert np.all(got_row[w.n_c:] == -7), what  # (nothing is written beyond the frame's count)
    for f in M.COMPARED_FIELDS:
        assert res[f] == e["res"][f], (what, f, res[f], e["res"][f])
    return res


def _cap(w):
    return 2048 if max(w.n_l, w.n_c) > 1024 else 1024


@pytest.mark.parametrize("name", M.WORLDS)
def test_world_equals_restatement(torch, ext, name):
    w = M.world(name)
    b = batch_of(torch, w, _cap(w))
    m, r = b.run(torch, ext, w.K, w.bounds, w.th, w.ori)
    res = check_pair(m[0], r[0], w, name)
    m2, r2 = b.run(torch, ext, w.K, w.bounds, w.th, w.ori)
    assert m.tobytes() == m2.tobytes() and r.tobytes() == r2.tobytes(), "two runs differ"
    if name == "w1500":
        assert w.n_l > 1024 and w.n_c > 1024
    if name == "order":
        assert w.n_l == 3 and res["rounds"] == 3 and m[0, :2].tolist() == [0, 1]
    if name == "contention":
        assert res["n_displaced"] > 20 and res["rounds"] >= 3
    if name in ("empty_l", "empty_c"):  # (without a last frame nothing is unresolved; without a current one a round finds no candidate)
        assert res["rounds"] == (0 if name == "empty_l" else 1) and res["nmatches"] == 0


@pytest.mark.parametrize("name", list(M.rule_worlds()))
def test_rule_world_equals_restatement(torch, ext, name):
    w = M.rule_worlds()[name]
    m, r = batch_of(torch, w, 64).run(torch, ext, w.K, w.bounds, w.th, w.ori)
    check_pair(m[0], r[0], w, name)


@pytest.mark.parametrize("cap", (None, 16384), ids=("exact", "cap16384"))
def test_capacity_and_counts(torch, orbx, ext, cap):
    """A capacity that is exactly the larger count (nothing lies beyond the rows), and the largest one with counts far below it
    (the kernel's LDS is sized from the capacity: 144 KB here)."""
    w = M.make_world(240, 31)
    cap = cap or max(w.n_l, w.n_c)
    assert max(w.n_l, w.n_c) <= cap and orbx.BOW_MAX_FEATURES == 16384 and w.n_l != w.n_c
    m, r = batch_of(torch, w, cap).run(torch, ext, w.K, w.bounds, w.th, w.ori)
    res = check_pair(m[0], r[0], w, "cap %d" % cap)
    assert res["nmatches"] > 30


# ---- the second setting (pose_ref_lib.SECOND): fx != fy, a context of 5 levels of 1.37 (the matcher reads the context's scale
# table), the pose rolled by 89 degrees ----

BOUNDS_2 = (-12, 655, -9, 490)


@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, M.SCALE_FACTOR_2, M.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2, device=0)
    assert np.asarray(e.GetScaleFactors(), np.float32).tobytes() == M.scale_table(M.NLEVELS_2, M.SCALE_FACTOR_2).tobytes()
    yield e
    e.close()


def test_second_setting_anisotropic_camera_and_five_levels(orbx, torch, ext2):
    """The scenes of 150 and 310 features under K_ANISO in one batch at the capacity of the largest count, under the offset
    bounds (a call has one set of bounds: the smaller scene's restatement runs under them too); then the smaller scene alone
    at its own largest count under the usual bounds, through the batch and the host form."""
    a, b = M.world("w150@2"), M.world("w310_bounds@2")
    assert a.n_l == 150 and b.n_l == 310 and b.bounds == BOUNDS_2 and len(a.scale) == M.NLEVELS_2
    a_off = a.variant(bounds=BOUNDS_2)
    cap = max(b.n_l, b.n_c)
    frames = [(a.kps_l, a.desc_l), (a.kps_c, a.desc_c), (b.kps_l, b.desc_l), (b.kps_c, b.desc_c)]
    sets = [(a.points, a.mask, None), (b.points, b.mask, None)]
    pairs = [(0, 1, 0, a.pose, a.outlier), (2, 3, 1, b.pose, b.outlier)]
    m, r = Batch(torch, frames, sets, pairs, cap).run(torch, ext2, b.K, BOUNDS_2, b.th, b.ori)
    for p, w in enumerate((a_off, b)):
        res = check_pair(m[p], r[p], w, "pair %d" % p)
        # not trivial: matches found, points that project outside the image (or lie behind the camera), windows with candidates
        assert res["status"] == 0 and res["nmatches"] > 30 and res["n_points"] - res["n_in_image"] > 20 and res["n_with_candidates"] > 50
    m1, r1 = batch_of(torch, a, max(a.n_l, a.n_c)).run(torch, ext2, a.K, a.bounds, a.th, a.ori)
    check_pair(m1[0], r1[0], a, "alone")
    e = a.expected()
    T = np.c_[a.pose[:9].reshape(3, 3), a.pose[9:]]
    mh, rh = ext2.match_projection(a.kps_l, a.desc_l, a.kps_c, a.desc_c, a.points, a.mask, T, a.K, a.bounds, a.th, a.ori, last_outlier=a.outlier)
    assert mh.tobytes() == e["matches"].tobytes()
    assert {f: v for f, v in rh.as_dict().items() if f != "rounds"} == {f: e["res"][f] for f in M.COMPARED_FIELDS}


def test_batch_with_shared_frames(torch, ext):
    """One call: frame 1 is the current frame of pairs 0 and 1 (two poses, so two answers) and the last frame of pair 2, whose
    current frame is frame 0; pair 3 has an empty last frame, pair 4 an empty current frame; pair 1 brings outlier flags, the
    others' rows of the array are zero."""
    a = M.world("w300")
    rng = np.random.default_rng(5)
    other = M.pose_of(99)
    # frame 1's own map points for pair 2: the point of a feature that shows frame 0's feature i projects onto that feature
    uv2 = rng.uniform(0, 480, (a.n_c, 2))
    shown = a.truth >= 0
    uv2[shown] = np.stack([a.kps_l["x"], a.kps_l["y"]], 1)[a.truth[shown]]
    pts2 = M.points_seen_at(other, a.K, uv2, rng.uniform(2.0, 10.0, a.n_c))
    mask2 = (rng.random(a.n_c) < 0.8).astype(np.uint8)
    outl1 = (rng.random(a.n_l) < 0.3).astype(np.uint8)
    none_k, none_d = np.zeros(0, KP), np.zeros((0, 32), np.uint8)
    frames = [(a.kps_l, a.desc_l), (a.kps_c, a.desc_c), (none_k, none_d)]
    sets = [(a.points, a.mask, None), (pts2, mask2, None), (np.zeros((0, 3), np.float32), None, None)]
    pairs = [(0, 1, 0, a.pose, None), (0, 1, 0, other, outl1), (1, 0, 1, other, None), (2, 1, 2, a.pose, None), (0, 2, 0, a.pose, None)]
    want = [a.variant(outlier=None), a.variant(pose=other, outlier=outl1),
            M.World(a.kps_c, a.desc_c, a.kps_l, a.desc_l, pts2, mask2, other, a.K),
            M.World(none_k, none_d, a.kps_c, a.desc_c, np.zeros((0, 3), np.float32), None, a.pose, a.K),
            M.World(a.kps_l, a.desc_l, none_k, none_d, a.points, a.mask, a.pose, a.K)]
    b = Batch(torch, frames, sets, pairs, 1024)
    m, r = b.run(torch, ext, a.K, a.bounds, a.th, a.ori)
    got = [check_pair(m[p], r[p], want[p], "pair %d" % p) for p in range(5)]
    assert m[0, :a.n_c].tobytes() != m[1, :a.n_c].tobytes()  # (one current frame, two poses: two answers)
    assert got[0]["nmatches"] > 40 and got[2]["nmatches"] > 10 and got[3]["nmatches"] == 0 and got[4]["nmatches"] == 0
    # every pair issued alone gives its row of the batch
    for p in range(5):
        one = Batch(torch, frames, sets, pairs[p:p + 1], 1024)
        m1, r1 = one.run(torch, ext, a.K, a.bounds, a.th, a.ori)
        assert m1[0].tobytes() == m[p].tobytes() and r1[0, :7].tobytes() == r[p, :7].tobytes(), p


def test_chain_into_pose_optimization(orbx, torch, ext):
    """match_projection_pairs_device -> pose_optimize_batch_device on the device, the second reading the first's d_matches_cur
    where it lies, equals match_proj_ref -> pose_ref byte for byte."""
    worlds = []
    for n, seed in ((300, 41), (260, 42)):  # (the optimisation refuses an octave outside the table: the current frames' stay inside)
        w = M.make_world(n, seed, with_outlier=False)
        kc = w.kps_c.copy()
        kc["octave"] = np.clip(kc["octave"], 0, M.NLEVELS - 1)
        worlds.append(w.variant(kps_c=kc))
    cap = 1024
    frames, sets, pairs = [], [], []
    for k, w in enumerate(worlds):
        frames += [(w.kps_l, w.desc_l), (w.kps_c, w.desc_c)]
        sets.append((w.points, w.mask, None))
        pairs.append((2 * k, 2 * k + 1, k, w.pose, None))
    b = Batch(torch, frames, sets, pairs, cap)
    w0 = worlds[0]
    d_res = torch.zeros(len(pairs) * orbx.POSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(len(pairs) * cap, dtype=torch.uint8, device="cuda")
    ext.match_projection_pairs_device(b.F, b.last, b.cur, b.set, b.kps, b.desc, b.n, b.S, b.pts, b.mask, b.pose, w0.K, w0.bounds,
                                      b.matches, b.res, th=w0.th, checkOri=True, capacity=cap)
    ext.pose_optimize_batch_device(b.F, b.cur, b.set, b.kps, b.n, b.matches, b.S, b.pts, b.mask, b.pose, w0.K, d_res, d_out, capacity=cap)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(orbx.POSE_RESULT_DTYPE)
    flags = d_out.cpu().numpy().reshape(len(pairs), cap)
    for p, w in enumerate(worlds):
        e = w.expected()
        assert e["res"]["nmatches"] >= 60
        match = np.full(cap, -1, np.int32)
        match[:w.n_c] = e["matches"]
        ref, rflags, _, _ = PR.pose_optimize(PR.World(b.kps_host[2 * p + 1], w.n_c, match, b.pts_host[p], b.mask_host[p], w.pose, w.K))
        assert ref["status"] == 0 and ref["n_correspondences"] == e["res"]["nmatches"] and ref["rounds"] == 4
        for f in orbx.POSE_RESULT_DTYPE.names:
            assert np.asarray(res[p][f]).tobytes() == np.asarray(ref[f]).tobytes(), (p, f, res[p][f], ref[f])
        assert flags[p].tobytes() == rflags.tobytes(), p


def test_host_form_and_classes(orbx, torch, ext):
    for name in ("w300", "w300_pdesc", "order", "empty_l", "empty_c"):
        w = M.world(name)
        e = w.expected()
        T = np.c_[w.pose[:9].reshape(3, 3), w.pose[9:]]
        m, res = ext.match_projection(w.kps_l, w.desc_l, w.kps_c, w.desc_c, w.points, w.mask, T, w.K, w.bounds, w.th, w.ori,
                                      point_desc=w.point_desc, last_outlier=w.outlier)
        assert m.tobytes() == e["matches"].tobytes(), name
        assert {f: v for f, v in res.as_dict().items() if f != "rounds"} == {f: e["res"][f] for f in M.COMPARED_FIELDS}, name
        last = orbx.Frame.from_arrays(w.kps_l, w.desc_l, w.bounds)
        cur = orbx.Frame.from_arrays(w.kps_c, w.desc_c, w.bounds)
        nm, m2, res2 = orbx.ORBmatcher(0.9, w.ori, extractor=ext).SearchByProjection(cur, last, w.th, w.points, w.mask, T, w.K.reshape(3, 3),
                                                                                    point_desc=w.point_desc, last_outlier=w.outlier)
        assert nm == e["res"]["nmatches"] and m2.tobytes() == m.tobytes() and bytes(res2) == bytes(res), name


def test_refusals(orbx, torch, ext):
    w = M.world("w40_th30")
    b = batch_of(torch, w, 128)
    L, p = orbx.lib(), orbx._ptr
    K = np.ascontiguousarray(w.K, np.float32)

    def call(last=0, cur=1, pset=0, cap=128, th=15.0, bounds=(0, 640, 0, 480), ctx=ext._h, n_pairs=1):
        hl, hc, hs = np.array([last], np.int32), np.array([cur], np.int32), np.array([pset], np.int32)  # (named: they outlive the call)
        bb = orbx._Bounds(*bounds)
        return L.orbx_match_projection_batch_device(ctx, 2, n_pairs, p(hl), p(hc), p(hs), p(b.kps), p(b.desc), p(b.n), cap, 1, p(b.pts), None,
                                                    None, None, p(b.pose), p(K), orbx.ctypes.byref(bb), th, 1, p(b.matches), p(b.res))
    assert call() == 0 and call(n_pairs=0) == 0
    assert call(last=2) == orbx.E_BADARG and call(cur=-1) == orbx.E_BADARG and call(pset=1) == orbx.E_BADARG
    assert call(th=0.0) == orbx.E_BADARG and call(th=-1.0) == orbx.E_BADARG and call(th=float("nan")) == orbx.E_BADARG
    assert call(th=float("inf")) == orbx.E_BADARG
    assert call(bounds=(5, 5, 0, 480)) == orbx.E_BADARG and call(bounds=(0, 640, 10, 9)) == orbx.E_BADARG
    assert call(cap=orbx.BOW_MAX_FEATURES + 1) == orbx.E_CAPACITY and call(cap=0) == orbx.E_BADARG
    assert call(ctx=None) == orbx.E_HIP and call(ctx=None, th=0.0) == orbx.E_BADARG  # (the arguments are judged first)
    torch.cuda.synchronize()
    # the binding's size checks come before anything is issued
    short = torch.zeros(10, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ext.match_projection_pairs_device(2, [0], [1], [0], b.kps, b.desc, b.n, 1, b.pts, None, b.pose, K, w.bounds, short, b.res, capacity=128)
    with pytest.raises(ValueError):
        ext.match_projection_pairs_device(2, [0], [1], [0], b.kps, b.desc, b.n, 1, b.pts, None, b.pose, K, w.bounds, b.matches, short[:4],
                                          capacity=128)
    with pytest.raises(ValueError):
        ext.match_projection_pairs_device(2, [0], [2], [0], b.kps, b.desc, b.n, 1, b.pts, None, b.pose, K, w.bounds, b.matches, b.res, capacity=128)
    with pytest.raises(ValueError):
        ext.match_projection_pairs_device(2, [0], [1], [0], b.kps, b.desc, b.n, 1, b.pts, None, b.pose, K, w.bounds, b.matches, b.res,
                                          d_last_outlier=torch.zeros(8, dtype=torch.uint8, device="cuda"), capacity=128)


def test_shim_match_proj_runs(orbx, tmp_path):
    """tests/cpp/shim_match_proj.cpp: the shim's two forms and the C call give the same matches, most of them the true ones."""
    exe, libdir = os.path.join(str(tmp_path), "shim_match_proj"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_match_proj.cpp"),
           "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    nm, right, n_cur, same = (int(v) for v in p.stdout.strip().splitlines()[-1].split()[1:])
    assert same == 1 and n_cur > 100 and nm > 0.7 * n_cur and right > 0.9 * nm, p.stdout
