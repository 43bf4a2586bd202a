"""Frame::ComputeStereoMatches on the device (orbx_stereo_match_batch_device / orbx_extract_stereo) equals the CPU restatement
tests/cpp/stereo_ref.cpp BYTE FOR BYTE: u_right, depth, match_right, sad, the tail's points and mask and every field of
orbx_stereo_result, on every world of tests/test_stereo_host.py, which says what the restatement itself is worth.  Natural scenes
are extracted on the device as the two frames of one batch; a crafted world's hand-written keypoints are uploaded next to that
batch's resident pyramid, which is first compared with the oracle's."""
import os
import subprocess

import numpy as np
import pytest

import stereo_ref_lib as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
_RIGS = {}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def fill(nbytes):
    import torch
    return torch.full((max(int(nbytes), 1),), FILL, dtype=torch.uint8, device="cuda")


def host(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


class Rig:
    """A scene's two frames extracted on the device as one batch (frame 0 left, frame 1 right), kept with its extractor."""

    def __init__(self, orbx, sc, extra=()):
        self.sc = sc
        self.ext = orbx.ORBextractor(sc.nfeatures, sc.scale_factor, sc.nlevels, 20, 7, max_width=sc.w, max_height=sc.h, max_batch=2 + len(extra))
        frames = [sc.left, sc.right] + list(extra)
        self.nf = len(frames)
        buf = np.zeros((self.nf, sc.h, sc.stride), np.uint8)
        for f, im in enumerate(frames):
            buf[f, :, :sc.w] = im
        self.cap = self.ext.capacity
        self.d_imgs, self.d_kps, self.d_desc, self.d_n = dev(buf), fill(self.nf * self.cap * 28), fill(self.nf * self.cap * 32), fill(self.nf * 4)
        self.extract()

    def extract(self):
        import torch
        sc = self.sc
        self.ext.extract_batch_device(self.d_imgs, self.nf, sc.w, sc.h, sc.stride, sc.stride * sc.h, self.d_kps, self.d_desc, self.d_n)
        torch.cuda.synchronize()
        self.n = host(self.d_n, np.int32, (self.nf,)).copy()
        self.kps = host(self.d_kps, S.KEYPOINT_DTYPE, (self.nf, self.cap)).copy()
        self.desc = host(self.d_desc, np.uint8, (self.nf, self.cap, 32)).copy()

    def pyramid(self, frame):
        return [self.ext.image_pyramid(l, frame) for l in range(self.sc.nlevels)]


def rig_of(orbx, sc):
    """One batch per scene; the device's keypoints, descriptors and pyramid equal the oracle's, asserted once."""
    if sc.name not in _RIGS:
        r = Rig(orbx, sc)
        o = sc.oracle()
        for f, side in ((0, "L"), (1, "R")):
            n = int(r.n[f])
            assert n == len(o["k" + side]) and r.kps[f, :n].tobytes() == o["k" + side].tobytes() and np.array_equal(r.desc[f, :n], o["d" + side])
            for l, (a, b) in enumerate(zip(r.pyramid(f), o["pyr" + side])):
                assert np.array_equal(a, b), (sc.name, side, l)
        assert r.ext.GetScaleFactors().tobytes() == o["scale"].tobytes() and r.ext.GetInverseScaleFactors().tobytes() == o["inv_scale"].tobytes()
        _RIGS[sc.name] = r
    return _RIGS[sc.name]


def run(orbx, rig, w, cap=None, with_optional=True, left=0, right=1):
    """One world through stereo_match_rigs_device over the rig's resident pyramid -> the same dict the restatement returns, and
    the raw output rows (for what lies beyond the count)."""
    import torch
    cap = cap or w.cap
    nf = rig.nf
    kps, desc, n = np.zeros((nf, cap), S.KEYPOINT_DTYPE), np.zeros((nf, cap, 32), np.uint8), np.zeros(nf, np.int32)
    kps[left, :len(w.kL)], desc[left, :len(w.kL)], n[left] = w.kL, w.dL, w.nL
    kps[right, :len(w.kR)], desc[right, :len(w.kR)], n[right] = w.kR, w.dR, w.nR
    d_ur, d_z, d_mr, d_sad, d_res = fill(cap * 4), fill(cap * 4), fill(cap * 4), fill(cap * 4), fill(64)
    tail = w.K is not None
    d_pts, d_mask = (fill(cap * 12), fill(cap)) if tail else (None, None)
    k_un = None
    if tail and w.k_un is not None:
        k_un = np.zeros((nf, cap), S.KEYPOINT_DTYPE)
        k_un[left, :len(w.k_un)] = w.k_un
    rig.ext.stereo_match_rigs_device(nf, [left], [right], dev(kps), dev(desc), dev(n), w.bf, w.b, d_ur, d_z, d_res,
                                     d_match_right=d_mr if with_optional else None, d_sad=d_sad if with_optional else None,
                                     d_kps_un=None if k_un is None else dev(k_un), K=w.K, d_pose_wc=None if w.pose is None else dev(w.pose),
                                     d_points=d_pts, d_point_mask=d_mask, capacity=cap)
    torch.cuda.synchronize()
    raw = dict(u_right=host(d_ur, np.float32, (cap,)), depth=host(d_z, np.float32, (cap,)), match_right=host(d_mr, np.int32, (cap,)),
               sad=host(d_sad, np.int32, (cap,)), points=host(d_pts, np.float32, (cap, 3)) if tail else None,
               mask=host(d_mask, np.uint8, (cap,)) if tail else None)
    m = min(max(w.nL, 0), cap)
    out = {k: (None if v is None else v[:m]) for k, v in raw.items()}
    out["record"] = host(d_res, S.STEREO_RESULT_DTYPE, (1,))[0]
    return out, raw, m


@pytest.fixture(scope="module")
def worlds(oracle):
    return S.worlds()


def test_every_world_equals_the_restatement(orbx, worlds):
    """The restatement is fed the pyramid image_pyramid downloads (equal to the oracle's: rig_of asserts it), so its expected()
    over the oracle's pyramid is the same computation."""
    for name, w in worlds.items():
        rig = rig_of(orbx, w.scene)
        got, raw, m = run(orbx, rig, w)
        assert S.same(got, w.expected()) == [], name
        for k, v in raw.items():  # rows beyond the count keep the fill pattern
            assert v is None or np.all(np.ascontiguousarray(v[m:]).view(np.uint8) == FILL), (name, k)
    gt = worlds["gt"]
    fed = S.restatement(gt, rig_of(orbx, gt.scene).pyramid(0), rig_of(orbx, gt.scene).pyramid(1))
    assert S.same(fed, gt.expected()) == []


def test_optional_outputs_left_out(orbx, worlds):
    for name in ("gt", "same", "clamp"):
        w = worlds[name]
        got, _, _ = run(orbx, rig_of(orbx, w.scene), w, with_optional=False)
        e = w.expected()
        assert got["u_right"].tobytes() == e["u_right"].tobytes() and got["depth"].tobytes() == e["depth"].tobytes(), name
        assert got["record"].tobytes() == e["record"].tobytes(), name


def test_five_rigs_over_six_frames(orbx, oracle):
    """One call with 5 rigs over a batch of 6 frames: frame 2 is the left image of two rigs and the right image of a third, the
    rig order differs from the frame order, one rig is empty (its left frame's count is 0).  Equal to five single calls."""
    import torch
    gt, same_ = S.scene("gt"), S.scene("same")
    blank = np.full((gt.h, gt.w), 90, np.uint8)  # no corner: an empty frame
    rig = Rig(orbx, gt, extra=[same_.left, same_.right, gt.right, blank])  # frames: gtL gtR sameL sameR gtR blank
    assert rig.n[5] == 0 and rig.n[0] > 100
    left, right = [2, 0, 5, 2, 4], [3, 1, 0, 4, 2]
    cap, nf, P = rig.cap, rig.nf, 5

    def call(ls, rs):
        p = len(ls)
        outs = [fill(p * cap * 4) for _ in range(4)] + [fill(p * 64)]
        rig.ext.stereo_match_rigs_device(nf, ls, rs, rig.d_kps, rig.d_desc, rig.d_n, 40.0, 0.5, outs[0], outs[1], outs[4], d_match_right=outs[2],
                                         d_sad=outs[3])
        torch.cuda.synchronize()
        return [host(o, np.uint8, (p, -1)) for o in outs]
    batch = call(left, right)
    for p in range(P):
        one = call(left[p:p + 1], right[p:p + 1])
        for a, b in zip(batch, one):
            assert a[p].tobytes() == b[0].tobytes(), p
    recs = batch[4].view(S.STEREO_RESULT_DTYPE).reshape(P)
    assert recs[2]["n_with_candidates"] == 0 and recs[1]["n_matches"] > 100 and recs[0]["median_sad"] == 0
    # rig 1 is the ground-truth world
    w = S.worlds()["gt"]
    n = w.nL
    assert batch[0].view(np.float32).reshape(P, cap)[1, :n].tobytes() == w.expected()["u_right"].tobytes()
    assert recs[1].tobytes() == w.expected()["record"].tobytes()
    rig.ext.close()


def test_capacity_larger_than_any_count(orbx, worlds):
    w = worlds["gt"]
    got, raw, m = run(orbx, rig_of(orbx, w.scene), w, cap=w.cap + 77)
    assert S.same(got, w.expected()) == []
    for k, v in raw.items():
        assert np.all(np.ascontiguousarray(v[m:]).view(np.uint8) == FILL), k


def test_the_chain_to_the_next_frames_pose(orbx, oracle):
    """stereo_match_rigs_device with d_points, then match_projection_pairs_device and pose_optimize_batch_device on the next frame
    of the same scene, reading the point row as it is: the pose record equals the CPU restatements chained the same way."""
    import torch
    import match_proj_ref_lib as M
    import pose_ref_lib as P
    gt = S.scene("gt")
    wide = S._wide(S.GT_SEED, S.GT_W, S.GT_H, S.GT_D)
    nxt = np.ascontiguousarray(wide[:, 2:2 + S.GT_W])  # the left camera two columns on
    rig = Rig(orbx, gt, extra=[nxt])
    cap, nf, K = rig.cap, rig.nf, S.K_CAM
    d_ur, d_z, d_res, d_pts, d_mask = fill(cap * 4), fill(cap * 4), fill(64), fill(cap * 12), fill(cap)
    d_pose, d_m, d_pres = dev(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)), fill(cap * 4), fill(32)
    d_pose_res, d_out = fill(orbx.POSE_RESULT_DTYPE.itemsize), fill(cap)
    bounds = (0, gt.w, 0, gt.h)
    rig.ext.stereo_match_rigs_device(nf, [0], [1], rig.d_kps, rig.d_desc, rig.d_n, 40.0, 0.5, d_ur, d_z, d_res, K=K, d_points=d_pts, d_point_mask=d_mask)
    rig.ext.match_projection_pairs_device(nf, [0], [2], [0], rig.d_kps, rig.d_desc, rig.d_n, 1, d_pts, d_mask, d_pose, K, bounds, d_m, d_pres)
    rig.ext.pose_optimize_batch_device(nf, [2], [0], rig.d_kps, rig.d_n, d_m, 1, d_pts, d_mask, d_pose, K, d_pose_res, d_out)
    torch.cuda.synchronize()
    # the same chain on the CPU
    n0, n2 = int(rig.n[0]), int(rig.n[2])
    w = S.World("chain", gt, rig.kps[0, :n0], rig.desc[0, :n0], rig.kps[1, :rig.n[1]], rig.desc[1, :rig.n[1]], K=K)
    e = w.expected()
    assert host(d_pts, np.float32, (cap, 3))[:n0].tobytes() == e["points"].tobytes() and e["mask"].sum() > 100
    pose = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    mw = M.World(rig.kps[0, :n0], rig.desc[0, :n0], rig.kps[2, :n2], rig.desc[2, :n2], e["points"], e["mask"], pose, K.reshape(9), bounds=bounds)
    matches = M.search_by_projection(mw)["matches"]
    assert host(d_m, np.int32, (cap,))[:n2].tobytes() == matches.tobytes() and (matches >= 0).sum() > 50
    pts, mask, match = np.zeros((cap, 3), np.float32), np.zeros(cap, np.uint8), np.full(cap, -1, np.int32)
    pts[:n0], mask[:n0], match[:n2] = e["points"], e["mask"], matches
    ref, rflags, _, _ = P.pose_optimize(P.World(rig.kps[2].copy(), n2, match, pts, mask, pose, np.ascontiguousarray(K.reshape(9))))
    res = host(d_pose_res, orbx.POSE_RESULT_DTYPE, (1,))[0]
    for f in P.POSE_RESULT_DTYPE.names:
        assert np.asarray(res[f]).tobytes() == np.asarray(ref[f]).tobytes(), f
    assert host(d_out, np.uint8, (cap,))[:n2].tobytes() == rflags[:n2].tobytes() and res["n_inliers"] > 30
    rig.ext.close()


def test_repeating_the_call_gives_the_same_bytes(orbx, worlds):
    w = worlds["gt"]
    rig = rig_of(orbx, w.scene)
    runs = [run(orbx, rig, w)[1] for _ in range(3)]
    for r in runs[1:]:
        for k in r:
            assert r[k].tobytes() == runs[0][k].tobytes(), k


def test_host_forms_agree_with_the_batched_call(orbx, worlds, tmp_path):
    """extract_stereo, Frame.ComputeStereoMatches / UnprojectStereo and the shim program give the batched call's bytes."""
    w = worlds["gt"]
    sc, e = w.scene, w.expected()
    ext = orbx.ORBextractor(sc.nfeatures, sc.scale_factor, sc.nlevels, 20, 7, max_width=sc.w, max_height=sc.h, max_batch=2)
    (kl, dl), (kr, dr), ur, z, res = ext.extract_stereo(sc.left, sc.right, w.bf, w.b)
    assert kl.tobytes() == w.kL.tobytes() and np.array_equal(dr, w.dR) and len(kr) == len(w.kR)
    assert ur.tobytes() == e["u_right"].tobytes() and z.tobytes() == e["depth"].tobytes() and bytes(res) == e["record"].tobytes()
    fl, fr = orbx.Frame(sc.left, 0.0, ext), orbx.Frame(sc.right, 0.0, ext)
    r2 = fl.ComputeStereoMatches(fr, w.bf, w.b)
    assert fl.mvuRight.tobytes() == ur.tobytes() and fl.mvDepth.tobytes() == z.tobytes() and bytes(r2) == bytes(res)
    fl.stereo_camera = (S.K_CAM[0, 0], S.K_CAM[1, 1], S.K_CAM[0, 2], S.K_CAM[1, 2])
    i = int(np.flatnonzero(z > 0)[0])
    assert fl.UnprojectStereo(i).tobytes() == e["points"][i].tobytes() and fl.UnprojectStereo(int(np.flatnonzero(z < 0)[0])) is None
    assert fl.UnprojectStereo(i, S.POSE_WC).tobytes() == worlds["gt_pose"].expected()["points"][i].tobytes()
    ext.close()
    # the shim program: the two images in, mvuRight / mvDepth out as raw floats
    libdir = os.path.dirname(orbx.lib_path())
    exe = str(tmp_path / "shim_stereo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_stereo.cpp"), "-L", libdir, "-lorbx", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    (tmp_path / "left.raw").write_bytes(sc.left.tobytes())
    (tmp_path / "right.raw").write_bytes(sc.right.tobytes())
    subprocess.run([exe, str(tmp_path / "left.raw"), str(tmp_path / "right.raw"), str(sc.w), str(sc.h), str(sc.nfeatures), repr(w.bf), repr(w.b),
                    str(tmp_path / "out.raw")], check=True, timeout=120)
    out = np.fromfile(str(tmp_path / "out.raw"), np.float32)
    assert out[:len(ur)].tobytes() == ur.tobytes() and out[len(ur):].tobytes() == z.tobytes()


def test_state_refusals(orbx, worlds):
    """With a context: before any extract call, and with an n_frames that is not the last extract call's."""
    sc = S.scene("gt")
    ext = orbx.ORBextractor(sc.nfeatures, sc.scale_factor, sc.nlevels, 20, 7, max_width=sc.w, max_height=sc.h, max_batch=2)
    cap = ext.capacity
    args = lambda nf: (nf, [0], [1], fill(nf * cap * 28), fill(nf * cap * 32), dev(np.zeros(nf, np.int32)), 40.0, 0.5, fill(cap * 4),  # noqa: E731
                       fill(cap * 4), fill(64))
    with pytest.raises(orbx.OrbxError) as err:
        ext.stereo_match_rigs_device(*args(2))
    assert err.value.code == orbx.E_BADARG and "no extract call" in str(err.value)
    assert b"no extract call" in orbx.lib().orbx_last_error(ext._h)
    rig = Rig(orbx, sc)
    with pytest.raises(orbx.OrbxError) as err:
        rig.ext.stereo_match_rigs_device(*args(3))
    assert err.value.code == orbx.E_BADARG and "n_frames" in str(err.value)
    rig.ext.stereo_match_rigs_device(*args(2))  # (and with the right count it runs)
    import torch
    torch.cuda.synchronize()
    ext.close()
    rig.ext.close()
