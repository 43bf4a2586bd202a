"""The map-point update on the device (orbx_map_update / orbx_map_update_batch_device) equals the CPU restatement
tests/cpp/map_update_ref.cpp BYTE FOR BYTE: every row entry, every mask byte, reference frame, observation count, descriptor,
normal and distance of every map set -- the rows the call must not touch included, which hold a fill pattern -- and every field
of orbx_map_result.  What the restatement itself is worth is tests/test_map_update_host.py's business.  The shapes are the
smallest at which the kernels' structure changes: observers per point around the 64 lanes of a wave (the lane path's edges) and
beyond (the looped path), points per problem around a chunk of 64 and past one trip of the 512 lanes' stride loops."""
import os
import subprocess

import numpy as np
import pytest

import lba_ref_lib as L
import map_update_ref_lib as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("mask_out", "ref", "obs", "desc", "normals", "dist")


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, U.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, U.SCALE_FACTOR_2, U.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


def check(orbx, ext, worlds, order=None, map_set=None, in_place=True, what=3, null=()):
    """The worlds as one device batch against the restatement run problem by problem on the same arrays, bit for bit.  order:
    the sequence of the problems' runs in the entry list; map_set[p]: the set of problem p (default p); worlds that share a set
    hold the same map arrays and say with `owned` whose reference frames are whose.  null: the optional arrays left out
    ("outlier", "ref", "mask").  -> the records."""
    import torch
    P = len(worlds)
    cap, mcap = max(w.cap for w in worlds), max(w.map_cap for w in worlds)
    ws = [w.padded(cap, mcap) for w in worlds]
    order = list(range(P)) if order is None else list(order)
    map_set = list(range(P)) if map_set is None else list(map_set)
    NS = max(map_set) + 1
    first, count, n_free = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    at = 0
    for p in order:
        first[p], count[p], n_free[p] = at, ws[p].n_entries, ws[p].n_free
        at += ws[p].n_entries
    E = at
    NF, E1 = max(E, 1), max(E, 1)
    kps, desc, n = np.zeros((NF, cap), orbx.KEYPOINT_DTYPE), np.zeros((NF, cap, 32), np.uint8), np.zeros(NF, np.int32)
    pose, rows, outlier = np.zeros((E1, 12), np.float32), np.full((E1, cap), -1, np.int32), np.zeros((E1, cap), np.uint8)
    entry_frame = np.arange(E, dtype=np.int32)
    map_n, pts = np.zeros(NS, np.int32), np.zeros((NS, mcap, 3), np.float32)
    mask, ref = np.zeros((NS, mcap), np.uint8), np.full((NS, mcap), -1, np.int32)
    for p, (w, w0) in enumerate(zip(ws, worlds)):
        for e in range(w.n_entries):  # (local frame e sits at global frame first + e; entry e names the world's frames[e])
            f = first[p] + e
            kps[f], desc[f], n[f] = w.kps[e], w.desc[e], w.n[e]
            pose[f], rows[f], outlier[f] = w.pose[e], w.rows[e], w.outlier[e]
            entry_frame[f] = first[p] + w.frames[e]
        s = map_set[p]
        map_n[s], pts[s], mask[s] = w.map_n, w.map_pts, w.map_mask
        own = np.zeros(mcap, bool)
        own[:w0.map_cap] = getattr(w0, "owned", np.ones(w0.map_cap, bool))
        ref[s][own] = np.where(w.map_ref[own] >= 0, w.map_ref[own] + first[p], w.map_ref[own])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    fill = lambda nbytes: torch.full((max(nbytes, 1),), U.FILL, dtype=torch.uint8, device="cuda")  # noqa: E731
    host_fill = lambda shape, dt: np.frombuffer(bytes([U.FILL]) * int(np.prod(shape) * np.dtype(dt).itemsize), dt).reshape(shape).copy()  # noqa: E731
    d_rows, d_mask, d_ref = d(rows), (None if "mask" in null else d(mask)), (None if "ref" in null else d(ref))
    d_ol = None if "outlier" in null else d(outlier)
    d_mo = d_mask if in_place and d_mask is not None else fill(NS * mcap)
    d_obs, d_desc_out, d_nrm, d_dist = fill(NS * mcap * 4), fill(NS * mcap * 32), fill(NS * mcap * 12), fill(NS * mcap * 8)
    d_res = fill(P * orbx.MAP_RESULT_DTYPE.itemsize)
    ext.map_update_problems_device(NF, first, count, n_free, map_set, entry_frame, d(kps), d(desc), d(n), d(pose), d_rows, d_ol, NS, mcap,
                                   d(map_n), d(pts), d_mask, d_obs, d_res, d_nrm, d_dist, d_desc_out, d_ref, d_mo, what=what, capacity=cap)
    torch.cuda.synchronize()
    # the restatement, problem by problem, on the batch's own arrays
    exp = dict(mask_out=mask.copy() if in_place and d_mask is not None else host_fill((NS, mcap), np.uint8), ref=ref.copy(),
               obs=host_fill((NS, mcap), np.int32), desc=host_fill((NS, mcap, 32), np.uint8),
               normals=host_fill((NS, mcap, 3), np.float32), dist=host_fill((NS, mcap, 2), np.float32))
    exp_rows, res = rows.copy(), np.zeros(P, U.MAP_RESULT_DTYPE)
    scale = np.array(ext.GetScaleFactors(), np.float32)
    for p in range(P):
        s, sl = map_set[p], slice(first[p], first[p] + count[p])
        rw = U.World(kps, desc, n, pose[sl], rows[sl], None if "outlier" in null else outlier[sl], pts[s], None if "mask" in null else mask[s],
                     None, map_n[s], n_free[p], frames=entry_frame[sl] if count[p] else None)
        rw.n_entries = int(count[p])
        into = {k: exp[k][s] for k in SETS}
        into["rows"] = exp_rows[sl]
        if "ref" in null:
            into["ref"] = None
        res[p] = U.update(rw, what, scale, into=into)["res"]
    got_res = d_res.cpu().numpy().view(orbx.MAP_RESULT_DTYPE)
    for p in range(P):
        for f in U.MAP_RESULT_DTYPE.names:
            assert np.asarray(got_res[p][f]).tobytes() == np.asarray(res[p][f]).tobytes(), ("problem %d" % p, f, got_res[p], res[p])
    assert d_rows.cpu().numpy().tobytes() == exp_rows.tobytes(), "rows"
    got = dict(mask_out=d_mo, ref=d_ref, obs=d_obs, desc=d_desc_out, normals=d_nrm, dist=d_dist)
    for k in SETS:
        if got[k] is not None:
            assert got[k].cpu().numpy().tobytes() == exp[k].tobytes(), k
    return got_res


def observers(n_obs, erase=0.0, seed=0):
    """6 points that each of n_obs free keyframes observes (plus the spare masked ones)."""
    return U.from_lba(L.make_world(n_obs, 0, 6, 300 + n_obs + seed, obs_per_point=n_obs, outliers=0), n_obs + seed, erase=erase)


@pytest.mark.parametrize("n_obs", [1, 2, 3, 4, 63, 64, 65, 130])
def test_observers_per_point(orbx, ext, n_obs):
    """Exactly n_obs observers per point, then the same with a few erased: the lane path's edges and the looped path."""
    res = check(orbx, ext, [observers(n_obs), observers(n_obs, erase=0.03, seed=1)])
    assert list(res["status"]) == [0, 0] and res[0]["max_observers"] == n_obs and res[0]["n_points"] == 6
    assert res[0]["n_observations"] == 6 * n_obs and res[1]["n_erased"] > (0 if n_obs > 60 else -1)


@pytest.mark.parametrize("n_points", [0, 1, 63, 64, 65, 513])
def test_points_per_problem(orbx, ext, n_points):
    """The chunks of 64 points of the second launch and a second trip of the first one's 512-lane loops."""
    w = U.make_world(3, 2, n_points, 400 + n_points, obs_per_point=4, masked=0)
    res = check(orbx, ext, [w])
    assert res[0]["status"] == 0 and (n_points < 63 or res[0]["n_points"] >= n_points - 8) and w.map_n == n_points


def empty():
    return U.from_lba(L.make_world(0, 0, 0, 1), 1)


@pytest.mark.parametrize("in_place", [False, True])
def test_five_problems_diverging_in_one_call(orbx, ext, in_place):
    """Empty, flagged, all erased, large, n_free == count."""
    large = U.make_world(10, 10, 600, 77, obs_per_point=6)
    ws = [empty(), U.garbage(U.world("window"), "duplicate"), U.world("all_erased"), large, U.world("all_free")]
    res = check(orbx, ext, ws, order=[3, 0, 4, 1, 2], in_place=in_place)
    assert list(res["status"]) == [0, U.BAD_INPUT, 0, 0, 0] and res[0]["n_points"] == 0 and res[3]["n_points"] > 500
    assert res[2]["n_bad_points"] == res[2]["n_points"] > 0 and res[4]["n_free"] == ws[4].n_entries and res[3]["n_erased"] > 100


def merged(a, b):
    """Two worlds on ONE map set: b's points behind a's; disjoint keyframes, disjoint vertices."""
    cap, mcap = max(a.cap, b.cap), a.map_n + b.map_n + 3
    out = []
    pts, mask, ref = np.zeros((mcap, 3), np.float32), np.zeros(mcap, np.uint8), np.full(mcap, -1, np.int32)
    pts[:a.map_n], pts[a.map_n:a.map_n + b.map_n] = a.map_pts[:a.map_n], b.map_pts[:b.map_n]
    mask[:a.map_n], mask[a.map_n:a.map_n + b.map_n] = a.map_mask[:a.map_n], b.map_mask[:b.map_n]
    for w, shift in ((a, 0), (b, a.map_n)):
        q = w.padded(cap, mcap)
        q.rows = np.where(q.rows >= 0, q.rows + shift, q.rows).astype(np.int32)
        r = np.full(mcap, -1, np.int32)
        r[shift:shift + w.map_n] = w.map_ref[:w.map_n]
        q.owned = np.zeros(mcap, bool)
        q.owned[shift:shift + w.map_n] = True
        q.map_pts, q.map_mask, q.map_ref, q.map_n = pts, mask, r, a.map_n + b.map_n
        out.append(q)
    return out


@pytest.mark.parametrize("in_place", [False, True])
def test_two_problems_share_a_map_set(orbx, ext, in_place):
    a, b = merged(U.world("window"), U.world("all_free"))
    res = check(orbx, ext, [a, U.make_world(2, 1, 63, 5), b], map_set=[1, 0, 1], in_place=in_place)
    assert list(res["status"]) == [0, 0, 0] and res[0]["n_points"] > 50 and res[2]["n_points"] > 50


@pytest.mark.parametrize("what", sorted(U.GARBAGE))
def test_each_garbage_flag_next_to_a_healthy_problem(orbx, ext, what):
    """The flagged problem is untouched (its outputs keep the fill, its rows and mask their bits) and the neighbour is right."""
    w = U.world("window")
    res = check(orbx, ext, [U.garbage(w, what), w], order=[1, 0])
    assert res[0]["status"] == U.GARBAGE[what] and res[1]["status"] == 0 and res[1]["n_points"] > 50
    assert all(res[0][f] == 0 for f in U.COUNTERS[1:])


@pytest.mark.parametrize("what", [0, 1, 2, 3])
def test_what_and_the_optional_arrays(orbx, ext, what):
    """Each `what`; then without outlier bytes, without reference frames, without a mask (the output mask is then required and
    gets a 1 per good vertex)."""
    w = U.world("window")
    check(orbx, ext, [w, U.world("clean")], what=what)
    for null in (("outlier",), ("ref",), ("mask",), ("outlier", "ref", "mask")):
        res = check(orbx, ext, [w], what=what, null=null)
        assert res[0]["status"] == 0 and (res[0]["n_erased"] == 0) == ("outlier" in null)


def test_the_lists_are_held(orbx, ext):
    """A second call with the same lists, then one with other lists, give what a first call gives."""
    w, v = U.world("window"), U.world("all_free")
    a = check(orbx, ext, [w, v])
    b = check(orbx, ext, [w, v])
    assert a.tobytes() == b.tobytes()
    check(orbx, ext, [v, w, v], order=[2, 0, 1])


def test_the_host_form_equals_a_batch_of_one(orbx, ext):
    scale = np.array(ext.GetScaleFactors(), np.float32)
    for name in ("window", "all_free", "all_erased"):
        w = U.world(name).padded(U.world(name).cap, U.world(name).map_cap)
        N = w.map_n
        blank = U.blank_outputs(w)
        want = U.update(w, 3, scale)
        res, out = ext.map_update(w.kps, w.desc, w.n, w.pose, w.rows, w.n_free, w.map_pts[:N], w.map_mask[:N], w.outlier, w.map_ref[:N],
                                  blank["normals"][:N], blank["dist"][:N], blank["desc"][:N], blank["obs"][:N])
        assert bytes(res) == want["res"].tobytes(), name
        assert out["rows"].tobytes() == want["rows"].tobytes() and out["mask"].tobytes() == want["mask_out"][:N].tobytes(), name
        for k in ("ref", "obs", "normals", "dist", "desc"):
            assert out[k].tobytes() == want[k][:N].tobytes(), (name, k)
    # a flagged problem comes back as it went in
    bad = U.garbage(w, "inf_point")
    res, out = ext.map_update(bad.kps, bad.desc, bad.n, bad.pose, bad.rows, bad.n_free, bad.map_pts[:N], bad.map_mask[:N], bad.outlier,
                              bad.map_ref[:N], blank["normals"][:N], blank["dist"][:N], blank["desc"][:N], blank["obs"][:N])
    assert res.status == U.NONFINITE and out["rows"].tobytes() == bad.rows.tobytes() and out["obs"].tobytes() == blank["obs"][:N].tobytes()
    assert out["normals"].tobytes() == blank["normals"][:N].tobytes() and out["ref"].tobytes() == bad.map_ref[:N].tobytes()


def test_the_second_setting(orbx, ext2):
    """fx != fy and five levels of 1.37: the distances come from the other pyramid's table."""
    res = check(orbx, ext2, [U.world("second")])
    assert res[0]["status"] == 0 and res[0]["n_points"] > 50
    w = U.world("second").copy()
    w.kps["octave"][:] = np.minimum(w.kps["octave"], U.NLEVELS_2 - 1)
    top = w.copy()
    top.kps["octave"][:] = U.NLEVELS_2  # inside the first setting's table, outside this one's
    res = check(orbx, ext2, [top, w])
    assert res[0]["status"] == U.BAD_INPUT and res[1]["status"] == 0


def test_refusals_touch_nothing(orbx, ext):
    import torch
    d_res = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    some = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    for kw, code in ((dict(what=4), orbx.E_BADARG), (dict(n_free=[3]), orbx.E_BADARG), (dict(d_map_normals=None), orbx.E_BADARG)):
        a = dict(n_frames=2, first=[0], count=[2], n_free=[1], map_set=[0], entry_frame=[0, 1], d_kps_un=some, d_desc=some, d_n=some,
                 d_entry_pose=some, d_rows=some, d_obs_outlier=None, n_map_sets=1, map_capacity=4, d_map_n=some, d_map_points=some,
                 d_map_mask=some, d_map_obs=some, d_res=d_res, d_map_normals=some, d_map_dist=some, d_map_desc=some, capacity=8)
        a.update(kw)
        with pytest.raises(orbx.OrbxError) as err:
            ext.map_update_problems_device(**a)
        assert err.value.code == code
    torch.cuda.synchronize()
    assert bool((d_res == 0xA5).all())


def test_shim_map_update_runs(orbx, tmp_path):
    """tests/cpp/shim_map_update.cpp: the shim and the C call give the same rows, arrays and record."""
    exe, libdir = os.path.join(str(tmp_path), "shim_map_update"), os.path.dirname(orbx.lib_path())
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "shim_map_update.cpp"), "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    points, observations, erased, bad, same = (int(v) for v in p.stdout.strip().splitlines()[-1].split()[1:])
    print(p.stdout.strip().splitlines()[-1])
    assert same == 1 and points == 60 and erased == 5 and bad == 5 and observations == 30 * 3 + 25 * 2


def test_the_chain_equals_the_four_restatements_chained(orbx, ext):
    """MapFuser.fuse_local_ba_update_device on the scene of tests/test_gpu_lba.py's chain test: CreateNewMapPoints for (kf1,
    kf2), its point set fused into kf2 and kf1, the rows adjusted with kf2 free and kf1 fixed, then the erasures applied and the
    points' counts, normals, distances and descriptors written over Fuse's map arrays -- queued on the stream with no copy and
    no wait in between -- equals tri_ref, fuse_ref, lba_ref and map_update_ref chained.  The arrays then go unchanged into
    match_local_map_pairs_device, whose result equals match_local_ref on the restatement's arrays."""
    import torch
    import fuse_ref_lib as FL
    import match_local_ref_lib as ML
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
    kf = np.array([1, 0], np.int32)  # the fuse pairs = the adjustment's entries: (kf2, set 0) free, then (kf1, set 0) fixed
    rows0 = np.full((2, cap), -1, np.int32)
    rows0[0, 0:b.n:7] = orbx.FUSE_OCCUPIED_UNMAPPED
    occ = np.zeros((2, cap), np.int32)
    occ[0, 0:b.n:14], occ[0, 7:b.n:14] = 5, 1
    obs = np.full(cap, 2, np.int32)
    m12, mres, tres = fill(cap * 4), fill(TL.MATCH_RESULT_DTYPE.itemsize), fill(TL.TRI_RESULT_DTYPE.itemsize)
    pts, msk, nrm, dst = fill(cap * 12), fill(cap), fill(cap * 12), fill(cap * 8)
    d_rows, d_idx, d_act, d_other, d_fres = up(rows0), fill(2 * cap * 4), fill(2 * cap), fill(2 * cap * 4), fill(2 * orbx.FUSE_RESULT_DTYPE.itemsize)
    d_po, d_ol, d_res = fill(2 * 48), fill(2 * cap), fill(orbx.LBA_RESULT_DTYPE.itemsize)
    d_mn, d_mdesc, d_obs, d_ref = up(np.array([a.n], np.int32)), up(desc[0]), up(obs), up(np.full(cap, -1, np.int32))
    d_ures = fill(orbx.MAP_RESULT_DTYPE.itemsize)
    create = dict(n_frames=2, kf1=[0], kf2=[1], d_kps_un=d_kps, d_desc=d_desc, d_n=d_n, d_fv_node=up(node), d_fv_feat=up(feat), d_fv_n=up(fv_n),
                  d_pose=d_pose, K=w.K, d_matches12=m12, d_match_res=mres, d_points=pts, d_point_mask=msk, d_point_normal=nrm,
                  d_point_dist=dst, d_res=tres, capacity=cap)
    fuse = dict(n_frames=2, kf=kf, map_set=[0, 0], d_kps_un=d_kps, d_desc=d_desc, d_n=d_n, n_map_sets=1, map_capacity=cap, d_map_n=d_mn,
                d_map_points=pts, d_map_normals=nrm, d_map_dist=dst, d_map_desc=d_mdesc, d_map_mask=msk, d_map_obs=d_obs,
                d_pose=up(pose[kf]), K=w.K, bounds=FL.BOUNDS, d_matches=d_rows, d_occ_obs=up(occ), d_fuse_idx=d_idx, d_fuse_act=d_act,
                d_fuse_other=d_other, d_res=d_fres, capacity=cap)
    lba = dict(n_frames=2, first=[0], count=[2], n_free=[1], map_set=[0], entry_frame=kf, d_kps_un=d_kps, d_n=d_n, d_pose=d_pose,
               d_rows=d_rows, n_map_sets=1, map_capacity=cap, d_map_n=d_mn, d_map_points=pts, d_map_mask=msk, K=w.K, d_pose_out=d_po,
               d_obs_outlier=d_ol, d_res=d_res, capacity=cap)
    update = dict(n_frames=2, first=[0], count=[2], n_free=[1], map_set=[0], entry_frame=kf, d_kps_un=d_kps, d_desc=d_desc, d_n=d_n,
                  d_entry_pose=d_po, d_rows=d_rows, d_obs_outlier=d_ol, n_map_sets=1, map_capacity=cap, d_map_n=d_mn, d_map_points=pts,
                  d_map_mask=msk, d_map_obs=d_obs, d_res=d_ures, d_map_normals=nrm, d_map_dist=dst, d_map_desc=d_mdesc, d_map_ref=d_ref,
                  capacity=cap)
    orbx.MapFuser(ext).fuse_local_ba_update_device(create, fuse, lba, update)
    # ... and the tracker's next SearchLocalPoints for kf2 under its adjusted pose, on the arrays as they are
    d_lm, d_lres = up(np.full((1, cap), -1, np.int32)), fill(orbx.LOCAL_RESULT_DTYPE.itemsize)
    ext.match_local_map_pairs_device(2, [1], [0], d_kps, d_desc, d_n, 1, cap, d_mn, pts, nrm, dst, d_mdesc, msk, d_po, w.K, FL.BOUNDS,
                                     d_lm, d_lres, capacity=cap)
    torch.cuda.synchronize()
    # the restatements: CreateNewMapPoints, Fuse, the local bundle adjustment
    m = TL.search(w, cap=cap)
    t = TL.triangulate(w, m["matches12"], cap=cap)
    rows = rows0.copy()
    for e, k in enumerate((b, a)):
        fw = FL.World("pose", k.kps, k.desc, t["points"][:a.n], t["normal"][:a.n], t["dist"][:a.n], a.desc, t["mask"][:a.n], obs[:a.n], k.pose,
                      w.K, matches=rows0[e, :k.n], occ_obs=occ[e, :k.n])
        rows[e, :k.n] = FL.fuse(fw)["matches"]
    lk = np.zeros((2, cap), L.KEYPOINT_DTYPE)
    lk[0, :b.n], lk[1, :a.n] = b.kps, a.kps
    lw = L.World(lk, np.array([b.n, a.n], np.int32), np.stack([b.pose, a.pose]), rows, t["points"].copy(), t["mask"].copy(), a.n, 1, w.K)
    r, rpo, rmo, rol, _ = L.local_ba(lw)
    assert d_res.cpu().numpy().tobytes() == r.tobytes() and d_po.cpu().numpy().tobytes() == rpo.tobytes()
    assert d_ol.cpu().numpy().tobytes() == rol.tobytes() and pts.cpu().numpy().tobytes() == rmo.tobytes()
    # the update on the restatements' arrays
    uw = U.World(kps, desc, n, rpo, rows, rol, rmo, t["mask"], None, a.n, 1, frames=kf)
    into = dict(rows=rows.copy(), mask_out=t["mask"].copy(), ref=np.full(cap, -1, np.int32), obs=obs.copy(), desc=desc[0].copy(),
                normals=t["normal"].copy(), dist=t["dist"].copy())
    o = U.update(uw, 3, np.array(ext.GetScaleFactors(), np.float32), into=into)
    assert d_ures.cpu().numpy().tobytes() == o["res"].tobytes() and o["res"]["status"] == 0 and o["res"]["n_points"] > 100
    assert o["res"]["n_erased"] == r["n_erased"] and o["res"]["max_observers"] == 2
    assert d_rows.cpu().numpy().tobytes() == o["rows"].tobytes() and msk.cpu().numpy().tobytes() == o["mask_out"].tobytes()
    assert d_ref.cpu().numpy().tobytes() == o["ref"].tobytes() and d_obs.cpu().numpy().tobytes() == o["obs"].tobytes()
    assert nrm.cpu().numpy().tobytes() == o["normals"].tobytes() and dst.cpu().numpy().tobytes() == o["dist"].tobytes()
    assert d_mdesc.cpu().numpy().tobytes() == o["desc"].tobytes() and o["normals"].tobytes() != t["normal"].tobytes()
    # SearchLocalPoints on the restatement's arrays
    mw = ML.World(b.kps, b.desc, rmo[:a.n], o["normals"][:a.n], o["dist"][:a.n], o["desc"][:a.n], o["mask_out"][:a.n], rpo[0], w.K, FL.BOUNDS,
                  scale=np.array(ext.GetScaleFactors(), np.float32))
    want = ML.search_local_points(mw)
    got = d_lm.cpu().numpy().view(np.int32)
    got_res = d_lres.cpu().numpy().view(orbx.LOCAL_RESULT_DTYPE)[0]
    assert got[:b.n].tobytes() == want["matches"].tobytes() and (got[b.n:] == -1).all() and want["res"]["nmatches"] > 50
    assert [int(got_res[f]) for f in orbx.LOCAL_RESULT_FIELDS if f != "rounds"] == [want["res"][f] for f in orbx.LOCAL_RESULT_FIELDS if f != "rounds"]
