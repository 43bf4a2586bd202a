"""k_describe_patch's angle chain (IC_Angle's moments -> fastAtan2 -> cos / sin) and its workgroups of three keypoints against the CPU
oracle, bit for bit: count, keypoint bytes (the angle among them), descriptor bytes.  Written for round 9's evaluation of the chain
once per workgroup (one wave evaluates with lane = keypoint, the others pick the results up; docs/history.md: parity-green here,
not faster, not kept); the cases are what ANY hand-over between the three waves of a workgroup can get wrong, and they hold the
kernel as it is -- one wave per keypoint, the blur's matrix products on two-dword operands (v_mfma_i32_16x16x32_i8) -- to the same
results.  On the smallest shapes that show them (322x243 frames):
  * a last workgroup with three, one and two live waves: 15, 16 and 14 keypoints per frame (nfeatures steers the count; eight levels
    with quotas of one and two keypoints at the top, so some workgroups hold three keypoints of three different levels), beside a
    frame without any keypoint in the same batch;
  * three keypoints of one workgroup within a few pixels of each other (500 keypoints on a textured frame);
  * a frame of single bright pixels, each with a faint 3x3 satellite that sets the patch's moments: every octant of fastAtan2, its
    special values (m10 = 0, m01 = 0, both 0, |m01| = |m10|) and workgroups whose three keypoints lie in three octants on both sides
    of the |m10| >= |m01| split, so that an evaluation with lane = keypoint runs both sides at once.  (IC_Angle cannot see a flat patch: a
    keypoint is a FAST corner.  Both moments are zero on a lone pixel, which is as flat as a patch around a corner gets.);
  * a window that crosses its level's left / right side (dword-by-dword staging) beside two that do not, in one workgroup;
  * both forms of the keypoint list (staged lists up to 256 (frame, level) units, k_sel_compact's list above), both libm readings,
    both Gaussian tap sets.
Every situation is asserted on the oracle's own output (test_oracle_coverage), so a change of a frame generator fails here and
does not silently thin the test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 322, 243
BIG = (500, 1.2, 4, 20, 7)
SMALL_NF = (15, 16, 14)  # keypoints per frame = 0, 1, 2 (mod 3)
VARIANTS = tuple((gv, lm) for gv in (0, 1) for lm in (1, 0))  # (Gaussian tap set, libm reading: 1 = FLOAT, 0 = DOUBLE)
# satellite offsets (du, dv): m10 = 54 du, m01 = 54 dv at level 0 -- the eight octants, then the special values
KINDS = ((10, 4), (4, 10), (-4, 10), (-10, 4), (-10, -4), (-4, -10), (4, -10), (10, -4),
         (0, 0), (0, 8), (0, -8), (8, 0), (-8, 0), (8, 8), (-8, -8), (-8, 8), (8, -8))


def _small(nf):
    return (nf, 1.2, 8, 20, 7)


def _dot_frame():
    rng = np.random.default_rng(0)
    img = np.full((H, W), 60, np.uint8)
    sites = [(x, y) for y in range(30, 200, 40) for x in [20] + list(range(60, 300, 40))]  # (x = 20: the window crosses the left side)
    for (x, y), kind in zip(sites, rng.permutation(len(sites)) % len(KINDS)):
        img[y, x] = 220  # a FAST corner on its own
        du, dv = KINDS[kind]
        if (du, dv) != (0, 0):
            img[y + dv - 1:y + dv + 2, x + du - 1:x + du + 2] = 66  # below minThFAST: no corner, only moments
    return img


def _info(oracle, oe, k):
    """Per keypoint of the frame the oracle extracted last: (level, x, y in level pixels, m10, m01, window crosses the level's left or
    right side).  The moments are the oracle's IC_Angle's on its own level image."""
    scale = oe.tables()["scale"]
    imgs = {}
    out = np.zeros((len(k), 6), np.int64)
    for i, kp in enumerate(k):
        l = int(kp["octave"])
        w, _ = oe.level_size(l)
        kx, ky = int(round(float(kp["x"]) / float(scale[l]))), int(round(float(kp["y"]) / float(scale[l])))
        if l not in imgs:
            imgs[l] = oe.level_image(l)
        a, m10, m01 = oracle.ic_angle(imgs[l], kx, ky)
        assert np.float32(a) == kp["angle"], (i, a, kp["angle"])
        ax = (kx - 21) & ~3  # first staged byte (k_describe_patch): 48 bytes from there must lie inside the level's rows
        out[i] = (l, kx, ky, m10, m01, not (ax >= 0 and ax + 48 <= w))
    return out


def _octant(m10, m01):
    """0 .. 7 counter-clockwise from the +m10 axis, -1 on a special value of fastAtan2."""
    if m10 == 0 or m01 == 0 or abs(m10) == abs(m01):
        return -1
    q = 0 if m10 > 0 and m01 > 0 else 1 if m10 < 0 and m01 > 0 else 2 if m10 < 0 else 3
    steep = abs(m01) > abs(m10)
    return 2 * q + int(steep if q in (0, 2) else not steep)


def _groups(n):
    """The workgroups of three consecutive keypoints of a frame's list."""
    return [slice(3 * g, 3 * g + 3) for g in range(n // 3)]


@pytest.fixture(scope="module")
def cases(oracle):
    """The frames and, per (Gaussian, libm) variant, the oracle's results (computed once, shared, left unchanged)."""
    from orb_slam_tracking_amd import synth
    frames = {"textured": synth.synth_frames(1, W, H, 4101)[0], "dots": _dot_frame(), "small": synth.synth_frames(1, W, H, 4200)[0],
              "empty": np.full((H, W), 128, np.uint8)}
    ref, info = {}, {}
    try:
        for v in VARIANTS:
            oracle.set_opencv_variant(v[0], 0)
            oracle.set_libm_variant(v[1])
            oe = oracle.Extractor(*BIG)
            for name in ("textured", "dots"):
                _, ko, do = oe(frames[name])
                ref[v, name] = (ko.copy(), do.copy())
                if v == VARIANTS[0]:
                    info[name] = _info(oracle, oe, ko)
            for nf in SMALL_NF:
                oe = oracle.Extractor(*_small(nf))
                _, ko, do = oe(frames["small"])
                ref[v, nf] = (ko.copy(), do.copy())
                if v == VARIANTS[0]:
                    info[nf] = _info(oracle, oe, ko)
                _, ko, do = oe(frames["empty"])
                ref[v, nf, "empty"] = (ko.copy(), do.copy())
    finally:
        oracle.set_opencv_variant(0, 0)
        oracle.set_libm_variant(oracle.LIBM_DEFAULT)
    return frames, ref, info


def test_oracle_coverage(cases):
    """What the frames are for, on the oracle's own output."""
    _, ref, info = cases
    for v in VARIANTS:
        for r, nf in enumerate(SMALL_NF):
            assert len(ref[v, nf][0]) == nf and nf % 3 == r and len(ref[v, nf, "empty"][0]) == 0   # three, one, two live waves at the end
        assert len(ref[v, "textured"][0]) == 500 and len(ref[v, "dots"][0]) > 100
        assert np.array_equal(ref[v, "dots"][0]["angle"], ref[VARIANTS[0], "dots"][0]["angle"])
    for nf in SMALL_NF:   # a workgroup whose three keypoints lie on three levels
        assert any(len(set(info[nf][g, 0])) == 3 for g in _groups(nf)), nf
    tex, dots = info["textured"], info["dots"]
    # three keypoints of one level within 4 pixels of each other in one workgroup
    assert any(len(set(tex[g, 0])) == 1 and np.ptp(tex[g, 1]) <= 4 and np.ptp(tex[g, 2]) <= 4 for g in _groups(len(tex)))
    # one window across the level's side, two inside, in one workgroup: both staging paths side by side
    assert any(tex[g, 5].sum() == 1 for g in _groups(len(tex))) and any(dots[g, 5].sum() == 1 for g in _groups(len(dots)))
    m10, m01 = dots[:, 3], dots[:, 4]
    oc = np.array([_octant(a, b) for a, b in zip(m10, m01)])
    assert set(oc.tolist()) == set(range(-1, 8))
    assert ((m10 == 0) & (m01 != 0)).any() and ((m01 == 0) & (m10 != 0)).any() and ((m10 == 0) & (m01 == 0)).any()
    assert ((abs(m10) == abs(m01)) & (m10 != 0)).any()
    for sx in (1, -1):  # the diagonal in every quadrant
        for sy in (1, -1):
            assert ((m10 * sx > 0) & (m01 * sy > 0) & (abs(m10) == abs(m01))).any(), (sx, sy)
    # three octants in one workgroup, on both sides of the |m10| >= |m01| split
    assert any((oc[g] >= 0).all() and len(set(oc[g])) == 3 and len(set((abs(m10[g]) >= abs(m01[g])).tolist())) == 2
               for g in _groups(len(dots)))


def _same(kg, dg, ko, do):
    assert len(kg) == len(ko), (len(kg), len(ko))
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        bad = np.nonzero(kg[f] != ko[f])[0]
        assert len(bad) == 0, (f, bad[:5], kg[f][bad[:5]], ko[f][bad[:5]])
    assert kg.tobytes() == ko.tobytes()
    bad = np.nonzero((dg != do).any(1))[0]
    assert len(bad) == 0, ("descriptors", bad[:5])


def _extract_device(orbx, e, buf, cap):
    import torch
    B = len(buf)
    d_img = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    d_k = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    d_d = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_img, B, W, H, W, W * H, d_k, d_d, d_n, cap)
    n = d_n.cpu().numpy()
    kk = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap)
    dd = d_d.cpu().numpy().reshape(B, cap, 32)
    return n, kk, dd


def _run(orbx, cases, params, names, keys, check, staged):
    """Extracts the batch `names` for every variant and compares the frames `check` with the oracle's results ref[v, *keys[i]]."""
    frames, ref, _ = cases
    buf = np.stack([frames[nm] for nm in names])
    e = orbx.ORBextractor(*params, max_width=W, max_height=H, max_batch=len(buf))
    try:
        with orbx.knobs(no_split=1):  # (one launch: batches of 16 frames and more go out as two half batches otherwise)
            for v in VARIANTS:
                e.set_opencv_variant(v[0], 0)
                e.set_libm_variant(v[1])
                n, kk, dd = _extract_device(orbx, e, buf, params[0])
                assert e.debug_last_launch()["staged_lists"] == staged
                for i in check:
                    ko, do = ref[(v,) + keys[i]]
                    assert n[i] == len(ko), (v, i, n[i], len(ko))
                    _same(kk[i, :n[i]], dd[i, :n[i]], ko, do)
    finally:
        e.set_opencv_variant(0, 0)
        e.set_libm_variant(e.LIBM_DEFAULT)
        e.close()


@pytest.mark.parametrize("nf", SMALL_NF)
def test_tail_staged_lists(orbx, cases, nf):
    """A frame of nf keypoints and a frame without any: 16 (frame, level) units, the kernel indexes the selection's staging lists."""
    _run(orbx, cases, _small(nf), ["small", "empty"], [(nf,), (nf, "empty")], (0, 1), 1)


@pytest.mark.parametrize("nf", SMALL_NF)
def test_tail_compacted_lists(orbx, cases, nf):
    """33 frames in one launch: 264 (frame, level) units go through k_sel_compact.  Even frames hold nf keypoints, odd ones none."""
    names = ["small" if i % 2 == 0 else "empty" for i in range(33)]
    _run(orbx, cases, _small(nf), names, [(nf,) if i % 2 == 0 else (nf, "empty") for i in range(33)], (0, 1, 31, 32), 0)


def test_octants_neighbours_staged_lists(orbx, cases):
    _run(orbx, cases, BIG, ["textured", "dots"], [("textured",), ("dots",)], (0, 1), 1)


def test_octants_neighbours_compacted_lists(orbx, cases):
    """65 frames of four levels in one launch: 260 units."""
    names = ["textured" if i % 2 == 0 else "dots" for i in range(65)]
    _run(orbx, cases, BIG, names, [(nm,) for nm in names], (0, 1, 63, 64), 0)
