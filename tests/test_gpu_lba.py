"""The local bundle adjustment on the device (orbx_local_ba / orbx_local_ba_batch_device) equals the CPU restatement
tests/cpp/lba_ref.cpp BYTE FOR BYTE: every pose, every point of every map set, every outlier byte and every field of
orbx_lba_result, the bytes of its f64 included.  Both sides run the phases of csrc/orbx_lba_math.inc and fold the lanes' sums in
the order that file states (include/orbx.h, deviation 2).  What the restatement itself is worth is tests/test_lba_host.py's
business, which also shows that the named worlds run every branch.  The shapes are the smallest at which the kernel's
structure changes: free keyframes around the 64 lanes of the block-pair owners (11 keyframes are 66 block pairs) and at the
limit of 64 (the full 384 x 384 system), vertices around a wave and around the workgroup's 256 lanes, a keyframe with more
features than a wave / the workgroup has lanes."""
import numpy as np
import pytest

import lba_ref_lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, L.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, L.SCALE_FACTOR_2, L.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


def run_batch(orbx, ext, worlds, order=None, map_set=None, n_map_sets=None, in_place=False, reverse_frames=False, **kw):
    """The worlds as one device batch.  order: the sequence of the problems' runs in the entry list; map_set[p]: the set of
    problem p (default p); worlds that share a set must hold the same map arrays.  -> (results [P], pose_out per problem, map
    sets out [NS, map_cap, 3], outlier per problem, the map sets as given)"""
    import torch
    P = len(worlds)
    cap, mcap = max(w.cap for w in worlds), max(w.map_cap for w in worlds)
    ws = [w if (w.cap, w.map_cap) == (cap, mcap) and w.map_mask is not None else w.padded(cap, mcap) for w in worlds]
    order = list(range(P)) if order is None else list(order)
    map_set = list(range(P)) if map_set is None else list(map_set)
    NS = int(n_map_sets or max(map_set) + 1)
    E = sum(w.n_entries for w in ws)
    first, count, n_free = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    at = 0
    for p in order:
        first[p], count[p], n_free[p] = at, ws[p].n_entries, ws[p].n_free
        at += ws[p].n_entries
    NF = max(E, 1)
    entry_frame = np.arange(E, dtype=np.int32)[::-1].copy() if reverse_frames else np.arange(E, dtype=np.int32)
    kps, n, pose = np.zeros((NF, cap), orbx.KEYPOINT_DTYPE), np.zeros(NF, np.int32), np.zeros((NF, 12), np.float32)
    rows = np.full((max(E, 1), cap), -1, np.int32)
    base = entry_frame.copy()
    for p, w in enumerate(ws):
        for e in range(w.n_entries):  # (frame e of the world sits where entry e would point; entry e names the world's frames[e])
            f = base[first[p] + e]
            kps[f], n[f], pose[f] = w.kps[e], w.n[e], w.pose[e]
            rows[first[p] + e] = w.rows[e]
            entry_frame[first[p] + e] = base[first[p] + w.frames[e]]
    map_n, map_pts, map_mask = np.zeros(NS, np.int32), np.zeros((NS, mcap, 3), np.float32), np.zeros((NS, mcap), np.uint8)
    for p, w in enumerate(ws):
        map_n[map_set[p]], map_pts[map_set[p]], map_mask[map_set[p]] = w.map_n, w.map_pts, w.map_mask
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    fill = lambda nbytes: torch.full((max(nbytes, 1),), 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_k, d_n, d_pose, d_rows, d_mn, d_mp, d_mm = d(kps), d(n), d(pose), d(rows), d(map_n), d(map_pts), d(map_mask)
    d_po, d_ol, d_res = fill(max(E, 1) * 48), fill(max(E, 1) * cap), fill(P * orbx.LBA_RESULT_DTYPE.itemsize)
    d_mo = None if in_place else fill(NS * mcap * 12)
    ext.local_ba_problems_device(NF, first, count, n_free, map_set, entry_frame, d_k, d_n, d_pose, d_rows, NS, mcap, d_mn, d_mp, d_mm,
                                 worlds[0].K, d_po, d_ol, d_res, d_mo, capacity=cap, **kw)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(orbx.LBA_RESULT_DTYPE)
    po = d_po.cpu().numpy().view(np.float32).reshape(-1, 12)
    ol = d_ol.cpu().numpy().reshape(-1, cap)
    mo = (d_mp if in_place else d_mo).cpu().numpy().view(np.float32).reshape(NS, mcap, 3)
    return (res, [po[first[p]:first[p] + count[p]] for p in range(P)], mo, [ol[first[p]:first[p] + count[p]] for p in range(P)],
            map_pts, ws, map_set)


def check(orbx, ext, worlds, **kw):
    """Runs the batch and compares everything with the restatement, bit for bit."""
    ref_kw = {k: v for k, v in kw.items() if k in ("n_iterations", "n_more_iterations", "inv_sigma2")}
    if ext.nlevels != L.NLEVELS:
        ref_kw["nlevels"] = ext.nlevels
    res, po, mo, ol, map_in, ws, map_set = run_batch(orbx, ext, worlds, **kw)
    expect = map_in.copy()
    for p, w in enumerate(ws):
        r, rpo, rmo, rol, _ = L.local_ba(w, **ref_kw)
        for f in L.LBA_RESULT_DTYPE.names:
            assert np.asarray(res[p][f]).tobytes() == np.asarray(r[f]).tobytes(), ("problem %d" % p, f, res[p][f], r[f])
        assert po[p].tobytes() == rpo.tobytes(), "problem %d: poses" % p
        assert ol[p].tobytes() == rol.tobytes(), "problem %d: outlier bytes" % p
        changed = (rmo.view(np.uint32) != w.map_pts.view(np.uint32)).any(axis=1)
        expect[map_set[p]][changed] = rmo[changed]
    assert mo.tobytes() == expect.tobytes(), "map points"
    return res


@pytest.fixture(scope="module")
def sized():
    """Worlds by (free, fixed, points), padded to one shape so that any of them can share a batch."""
    made = {}

    def get(n_free, n_fixed, n_points, **kw):
        key = (n_free, n_fixed, n_points, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = make(n_free, n_fixed, n_points, **kw)
        return made[key]
    return get


def make(n_free, n_fixed, n_points, **kw):
    kw.setdefault("outliers", n_points // 12)
    kw.setdefault("obs_per_point", n_free + n_fixed if n_points < 10 else min(4, max(n_free + n_fixed, 1)))
    return L.make_world(n_free, n_fixed, n_points, 40 + n_free + 7 * n_fixed + n_points, **kw)


@pytest.mark.parametrize("n_free", [1, 2, 3, 11, 12, 29, 30, 64])
def test_free_keyframe_counts(orbx, ext, sized, n_free):
    """11 free keyframes are 66 block pairs, one past a wave; 29 is the largest problem whose packed factor lives in LDS (120,408
    bytes of dynamic LDS: past the 64 KiB a kernel gets unasked), 30 the smallest that keeps it in the workspace; 64 is the full
    384 x 384 system."""
    w = sized(n_free, 2, max(40, 5 * n_free))
    res = check(orbx, ext, [w])
    assert res[0]["status"] == 0 and res[0]["n_free"] == n_free and res[0]["n_active_free"][0] == n_free
    assert res[0]["iterations"][0] > 0 and res[0]["solver_failures"].sum() == 0


@pytest.mark.parametrize("n_free", [12, 29])
def test_the_workspace_path_at_sizes_the_lds_path_takes(orbx, ext, sized, n_free):
    """orbx_debug_local_ba_lds_max_free(0): the same problems with the packed factor in the workspace give the same bytes (the
    switch is restored behind the test)."""
    orbx.debug_local_ba_lds_max_free(0)
    try:
        res = check(orbx, ext, [sized(n_free, 2, max(40, 5 * n_free))])
    finally:
        orbx.debug_local_ba_lds_max_free(-1)
    assert res[0]["status"] == 0 and res[0]["iterations"][0] > 0 and res[0]["solver_failures"].sum() == 0


@pytest.mark.parametrize("n_points", [0, 1, 63, 64, 255, 256, 257])
def test_point_counts(orbx, ext, sized, n_points):
    w = sized(3, 2, n_points, masked=0 if n_points == 0 else 2)
    res = check(orbx, ext, [w])
    assert res[0]["status"] == 0 and res[0]["n_points"] == n_points
    if n_points >= 63:
        assert res[0]["iterations"][0] > 0 and res[0]["iterations"][1] > 0


@pytest.mark.parametrize("seen", [65, 257])
def test_a_dense_keyframe(orbx, ext, sized, seen):
    """One free keyframe with more observed features than a wave / the workgroup has lanes (the pose block's feature stride)."""
    w = sized(2, 2, seen + 3, dense=(0, seen), obs_per_point=3)
    assert (w.rows[0, :w.n[0]] >= 0).sum() >= seen
    res = check(orbx, ext, [w])
    assert res[0]["status"] == 0 and res[0]["iterations"][0] > 0


@pytest.mark.parametrize("n_fixed", [0, 1, 5])
def test_fixed_keyframe_counts(orbx, ext, sized, n_fixed):
    res = check(orbx, ext, [sized(3, n_fixed, 70)])
    assert res[0]["status"] == 0 and res[0]["iterations"][0] > 0


@pytest.mark.parametrize("in_place", [False, True])
def test_five_problems_diverging_workgroups(orbx, ext, sized, in_place):
    """Problems of different sizes whose workgroups differ in iterations and trials, the entry runs in another order than the
    problems, the frames in reverse."""
    worlds = [L.world("window"), sized(1, 2, 64), L.world("far"), sized(0, 2, 30), L.world("losing")]
    res = check(orbx, ext, worlds, order=[3, 0, 4, 2, 1], reverse_frames=True, in_place=in_place)
    assert list(res["status"]) == [0] * 5 and res[3]["iterations"].sum() == 0
    assert len({tuple(r["lm_trials"]) for r in res}) >= 4
    assert res[4]["n_active_points"][1] < res[4]["n_active_points"][0]


def blind(w):
    """The world with every keypoint at the last level: under top_off_table() every edge weighs nothing."""
    q = w.copy()
    q.kps["octave"][:] = L.NLEVELS - 1
    return q


def top_off_table():
    t = L.inv_sigma2_table()
    t[L.NLEVELS - 1] = 0
    return t


@pytest.mark.parametrize("in_place", [False, True])
def test_failed_solves_between_problems_that_solve(orbx, ext, sized, in_place):
    """Every edge of problem 1 weighs nothing under this table: ten failed solves per round, decided from LDS and taken by the
    whole workgroup, between two problems that solve."""
    worlds = [L.world("window"), blind(L.world("idle")), sized(3, 2, 257)]
    res = check(orbx, ext, worlds, inv_sigma2=top_off_table(), in_place=in_place)
    assert list(res["status"]) == [0, 0, 0]
    assert list(res[1]["solver_failures"]) == [10, 10] and list(res[1]["lm_trials"]) == [10, 10] and list(res[1]["stop_reason"]) == [1, 1]
    assert res[0]["solver_failures"].sum() == 0 and res[2]["solver_failures"].sum() == 0 and res[2]["iterations"][0] > 0


def merged(a, b):
    """Two worlds on ONE map set: b's points behind a's; disjoint keyframes, disjoint vertices."""
    cap = max(a.cap, b.cap)
    mcap = a.map_n + b.map_n + 3
    pts, mask = np.zeros((mcap, 3), np.float32), np.zeros(mcap, np.uint8)
    pts[:a.map_n], pts[a.map_n:a.map_n + b.map_n] = a.map_pts[:a.map_n], b.map_pts[:b.map_n]
    mask[:a.map_n], mask[a.map_n:a.map_n + b.map_n] = a.map_mask[:a.map_n], b.map_mask[:b.map_n]
    out = []
    for w, shift in ((a, 0), (b, a.map_n)):
        q = w.padded(cap, mcap)
        q.rows = np.where(q.rows >= 0, q.rows + shift, q.rows).astype(np.int32)
        q.map_pts, q.map_mask, q.map_n = pts, mask, a.map_n + b.map_n
        out.append(q)
    return out


@pytest.mark.parametrize("in_place", [False, True])
def test_two_problems_share_a_map_set(orbx, ext, sized, in_place):
    a, b = merged(L.world("truth"), L.world("lonely"))
    res = check(orbx, ext, [a, sized(2, 1, 63), b], map_set=[1, 0, 1], in_place=in_place)
    assert list(res["status"]) == [0, 0, 0] and res[0]["n_points"] > 0 and res[2]["n_points"] > 0


def garbage(w, what):
    q = w.copy()
    e, f = [(e, f) for e in range(q.n_free) for f in range(q.n[e]) if q.rows[e, f] >= 0 and q.map_mask[q.rows[e, f]]][0]
    if what == "count":
        q.n[1] = q.cap + 1
    elif what == "map_count":
        q.map_n = q.map_cap + 1
    elif what == "row":
        q.rows[e, f] = q.map_n
    elif what == "octave":
        q.kps["octave"][e, f] = L.NLEVELS
    elif what == "duplicate":
        g = [g for g in range(q.n[e]) if g != f and q.rows[e, g] < 0][0]
        q.rows[e, g] = q.rows[e, f]
    elif what == "frame_twice":
        q.frames[2] = q.frames[0]
    elif what == "nan_pose":
        q.pose[q.n_entries - 1, 10] = np.nan
    elif what == "inf_point":
        q.map_pts[q.rows[e, f], 1] = np.inf
    return q


@pytest.mark.parametrize("what", ["count", "map_count", "row", "octave", "duplicate", "frame_twice", "nan_pose", "inf_point"])
def test_each_garbage_flag_next_to_a_healthy_problem(orbx, ext, what):
    """A flagged problem copies its inputs through and its healthy neighbour is unaffected."""
    w = L.world("window").padded(L.world("window").cap, L.world("window").map_cap)
    bad = garbage(w, what)
    res = check(orbx, ext, [bad, w], order=[1, 0])
    want = L.NONFINITE if what in ("nan_pose", "inf_point") else L.BAD_INPUT
    assert res[0]["status"] == want and res[1]["status"] == 0 and res[1]["iterations"][0] > 0
    assert res[0]["n_points"] == 0 and res[0]["iterations"].sum() == 0


def test_null_table_is_the_contexts_and_the_lists_are_held(orbx, ext):
    """inv_sigma2 = None is the context's own table (the restatement is given ORBextractor's), and a second call with the same
    lists, then one with other lists, give what a first call gives."""
    w, v = L.world("window"), L.world("nofixed")
    table = np.array(ext.GetInverseScaleSigmaSquares(), np.float32)
    a = check(orbx, ext, [w, v], inv_sigma2=None)
    b = check(orbx, ext, [w, v], inv_sigma2=table)
    c = check(orbx, ext, [w, v], inv_sigma2=None)
    assert a.tobytes() == b.tobytes() == c.tobytes()
    check(orbx, ext, [v, w, v], order=[2, 0, 1])


def test_the_host_form_equals_a_batch_of_one(orbx, ext):
    for name in ("window", "lonely", "idle"):
        w = L.world(name)
        r, rpo, rmo, rol, _ = L.local_ba(w)
        res, po, pts, ol = ext.local_ba(w.kps, w.n, w.pose, w.rows, w.n_free, w.map_pts[:w.map_n], w.map_mask[:w.map_n], w.K)
        got = np.frombuffer(bytes(res), L.LBA_RESULT_DTYPE)[0]
        for f in L.LBA_RESULT_DTYPE.names:
            assert np.asarray(got[f]).tobytes() == np.asarray(r[f]).tobytes(), (name, f)
        assert po.tobytes() == rpo.tobytes() and ol.tobytes() == rol.tobytes() and pts.tobytes() == rmo[:w.map_n].tobytes(), name


def test_the_second_setting(orbx, ext2):
    """fx != fy and five levels of 1.37."""
    res = check(orbx, ext2, [L.world("second")], inv_sigma2=L.inv_sigma2_of("second"))
    assert res[0]["status"] == 0 and res[0]["iterations"][0] > 0 and res[0]["n_level1"] > 0


def test_no_iterations_only_classifies(orbx, ext):
    res = check(orbx, ext, [L.world("window")], n_iterations=0, n_more_iterations=0)
    assert res[0]["iterations"].sum() == 0 and res[0]["n_level1"] > 0 and res[0]["n_erased"] >= res[0]["n_level1"]


def test_refusals_touch_nothing_and_the_python_class(orbx, ext):
    """With a context: a refused call (more than ORBX_LBA_MAX_FREE free keyframes) leaves the outputs as they were; the
    Optimizer class gives the host form's answer."""
    import torch
    w = L.world("window")
    many = orbx.LBA_MAX_FREE + 1
    d_res = torch.full((128,), 0xA5, dtype=torch.uint8, device="cuda")
    some = torch.zeros(many * max(w.cap, 12) * 48, dtype=torch.uint8, device="cuda")
    with pytest.raises(orbx.OrbxError) as err:
        ext.local_ba_problems_device(many, [0], [many], [many], [0], np.arange(many), some, some, some, some, 1, 4, some, some, None, w.K,
                                     some, some, d_res, capacity=w.cap)
    assert err.value.code == orbx.E_BADARG and "ORBX_LBA_MAX_FREE" in str(err.value)
    torch.cuda.synchronize()
    assert bool((d_res == 0xA5).all())
    frames = []
    for e in range(w.n_entries):
        f = orbx.Frame.from_arrays(w.kps[e, :w.n[e]], np.zeros((w.n[e], 32), np.uint8), (0, 640, 0, 480))
        f.mvKeysUn, f.mpORBextractor = w.kps[e, :w.n[e]], ext
        frames.append((f, w.pose[e]))
    T, pts, erase, res = orbx.Optimizer.LocalBundleAdjustment(frames, w.n_free, [w.rows[e, :w.n[e]] for e in range(w.n_entries)],
                                                              w.map_pts[:w.map_n], w.map_mask[:w.map_n], K=w.K.reshape(3, 3))
    r, rpo, rmo, rol, _ = L.local_ba(w)
    assert np.frombuffer(bytes(res), L.LBA_RESULT_DTYPE)[0].tobytes() == r.tobytes()
    assert T[:, :3, :3].reshape(-1, 9).tobytes() == rpo[:, :9].tobytes() and T[:, :3, 3].tobytes() == rpo[:, 9:].tobytes()
    assert pts.tobytes() == rmo[:w.map_n].tobytes() and erase == [(int(e), int(f)) for e, f in zip(*np.nonzero(rol))] and len(erase) > 0


def test_shim_lba_runs(orbx, tmp_path):
    """tests/cpp/shim_lba.cpp: the shim and the C call give the same poses, points, erasures and record."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = os.path.join(str(tmp_path), "shim_lba"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "shim_lba.cpp"),
           "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    edges, erased, it1, it2, same = (int(v) for v in p.stdout.strip().splitlines()[-1].split()[1:])
    print(p.stdout.strip().splitlines()[-1])
    assert same == 1 and edges == 200 and erased > 0 and it1 > 0 and it2 > 0


def test_the_chain_equals_the_three_restatements_chained(orbx, ext):
    """MapFuser.fuse_local_ba_device on one scene: CreateNewMapPoints for the pair (kf1, kf2), its point set fused into kf2 and
    kf1 (kf2's row holds unmapped occupants, -2, some of which stay), the rows Fuse leaves adjusted with kf2 free and kf1 fixed --
    queued on the stream with no copy and no wait in between.  Every stage's output equals tri_ref, then fuse_ref on its points,
    then lba_ref on its rows, byte for byte."""
    import torch
    import fuse_ref_lib as FL
    import tri_ref_lib as TL
    w = TL.make_world(5)
    a, b = w.kf1, w.kf2
    cap = max(a.n, b.n, len(a.fv_node), len(b.fv_node))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    fill = lambda nbytes, byte=0xA5: torch.full((nbytes,), byte, dtype=torch.uint8, device="cuda")  # noqa: E731
    kps, desc = np.zeros((2, cap), orbx.KEYPOINT_DTYPE), np.zeros((2, cap, 32), np.uint8)
    node, feat = np.zeros((2, cap), np.uint32), np.zeros((2, cap), np.uint32)
    for f, k in enumerate((a, b)):  # frame 0 = kf1, frame 1 = kf2
        kps[f, :k.n], desc[f, :k.n] = k.kps, k.desc
        node[f, :len(k.fv_node)], feat[f, :len(k.fv_feat)] = k.fv_node, k.fv_feat
    n, fv_n, pose = np.array([a.n, b.n], np.int32), np.array([len(a.fv_node), len(b.fv_node)], np.int32), np.stack([a.pose, b.pose])
    d_kps, d_desc, d_n, d_pose = up(kps), up(desc), up(n), up(pose)
    # the fuse pairs = the adjustment's entries: (kf2, set 0) free, then (kf1, set 0) fixed
    kf = np.array([1, 0], np.int32)
    rows0 = np.full((2, cap), -1, np.int32)
    rows0[0, 0:b.n:7] = orbx.FUSE_OCCUPIED_UNMAPPED
    occ = np.zeros((2, cap), np.int32)
    occ[0, 0:b.n:14], occ[0, 7:b.n:14] = 5, 1  # (Observations() of the occupants: above / below the new points' 2)
    obs = np.full(cap, 2, np.int32)
    m12, mres, tres = fill(cap * 4), fill(TL.MATCH_RESULT_DTYPE.itemsize), fill(TL.TRI_RESULT_DTYPE.itemsize)
    pts, msk, nrm, dst = fill(cap * 12), fill(cap), fill(cap * 12), fill(cap * 8)
    d_rows, d_idx, d_act, d_other, d_fres = up(rows0), fill(2 * cap * 4), fill(2 * cap), fill(2 * cap * 4), fill(2 * orbx.FUSE_RESULT_DTYPE.itemsize)
    d_po, d_ol, d_res = fill(2 * 48), fill(2 * cap), fill(orbx.LBA_RESULT_DTYPE.itemsize)
    d_mn = up(np.array([a.n], np.int32))
    create = dict(n_frames=2, kf1=[0], kf2=[1], d_kps_un=d_kps, d_desc=d_desc, d_n=d_n, d_fv_node=up(node), d_fv_feat=up(feat), d_fv_n=up(fv_n),
                  d_pose=d_pose, K=w.K, d_matches12=m12, d_match_res=mres, d_points=pts, d_point_mask=msk, d_point_normal=nrm,
                  d_point_dist=dst, d_res=tres, capacity=cap)
    fuse = dict(n_frames=2, kf=kf, map_set=[0, 0], d_kps_un=d_kps, d_desc=d_desc, d_n=d_n, n_map_sets=1, map_capacity=cap, d_map_n=d_mn,
                d_map_points=pts, d_map_normals=nrm, d_map_dist=dst, d_map_desc=up(desc[0]), d_map_mask=msk, d_map_obs=up(obs),
                d_pose=up(pose[kf]), K=w.K, bounds=FL.BOUNDS, d_matches=d_rows, d_occ_obs=up(occ), d_fuse_idx=d_idx, d_fuse_act=d_act,
                d_fuse_other=d_other, d_res=d_fres, capacity=cap)
    lba = dict(n_frames=2, first=[0], count=[2], n_free=[1], map_set=[0], entry_frame=kf, d_kps_un=d_kps, d_n=d_n, d_pose=d_pose,
               d_rows=d_rows, n_map_sets=1, map_capacity=cap, d_map_n=d_mn, d_map_points=pts, d_map_mask=msk, K=w.K, d_pose_out=d_po,
               d_obs_outlier=d_ol, d_res=d_res, capacity=cap)
    orbx.MapFuser(ext).fuse_local_ba_device(create, fuse, lba)
    torch.cuda.synchronize()
    # 1. CreateNewMapPoints (the points are adjusted in place behind it: the mask, the normals and the records tell)
    m = TL.search(w, cap=cap)
    t = TL.triangulate(w, m["matches12"], cap=cap)
    assert m12.cpu().numpy().tobytes() == m["matches12"].tobytes() and mres.cpu().numpy().tobytes() == m["res"].tobytes()
    assert tres.cpu().numpy().tobytes() == t["res"].tobytes() and msk.cpu().numpy().tobytes() == t["mask"].tobytes()
    assert nrm.cpu().numpy().tobytes() == t["normal"].tobytes() and dst.cpu().numpy().tobytes() == t["dist"].tobytes()
    # 2. Fuse on the restatement's points
    rows = rows0.copy()
    got_rows = d_rows.cpu().numpy().view(np.int32).reshape(2, cap)
    got_fres = d_fres.cpu().numpy().view(orbx.FUSE_RESULT_DTYPE)
    for e, k in enumerate((b, a)):
        fw = FL.World("pose", k.kps, k.desc, t["points"][:a.n], t["normal"][:a.n], t["dist"][:a.n], a.desc, t["mask"][:a.n], obs[:a.n], k.pose,
                      w.K, matches=rows0[e, :k.n], occ_obs=occ[e, :k.n])
        f = FL.fuse(fw)
        rows[e, :k.n] = f["matches"]
        assert got_rows[e].tobytes() == rows[e].tobytes(), "the row Fuse leaves, entry %d" % e
        fields = [name for name in orbx.FUSE_RESULT_FIELDS if name != "rounds"]  # (rounds is the device's own count)
        assert [int(got_fres[e][name]) for name in fields] == [f["res"][name] for name in fields], e
    assert (rows[0] == orbx.FUSE_OCCUPIED_UNMAPPED).sum() > 0 and (rows[0] >= 0).sum() > 100 and (rows[1] >= 0).sum() > 100
    # 3. the local bundle adjustment on the restatement's rows
    lk = np.zeros((2, cap), L.KEYPOINT_DTYPE)
    lk[0, :b.n], lk[1, :a.n] = b.kps, a.kps
    lw = L.World(lk, np.array([b.n, a.n], np.int32), np.stack([b.pose, a.pose]), rows, t["points"].copy(), t["mask"].copy(), a.n, 1, w.K)
    r, rpo, rmo, rol, _ = L.local_ba(lw)
    assert d_res.cpu().numpy().tobytes() == r.tobytes() and r["status"] == 0 and r["n_points"] > 100 and r["iterations"][0] > 0
    assert d_po.cpu().numpy().tobytes() == rpo.tobytes() and d_ol.cpu().numpy().tobytes() == rol.tobytes()
    assert pts.cpu().numpy().tobytes() == rmo.tobytes() and rmo.tobytes() != t["points"].tobytes()
