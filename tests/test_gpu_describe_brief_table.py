"""k_describe_patch's steered-BRIEF loop (round 15): the byte address of a rotated sample point is one v_mad_u32_u24 on the float
bits of its rounded coordinates (the low 24 bits of 0x4B400000 + c times the column stride, plus the dword 0x4B400000 + r) and one
add of a per-wave scalar, mod 2^32; in the pair form keypoint B's slice is reached through immediate offsets, by the staging stores
too; and IC_Angle's two moments are summed in registers (DPP adds over rows of 16 lanes, row sums through SGPRs, each half of a
pair wave selecting its own) where each half added into two LDS words.  (The file's name is that of the round's plan: products k sin, k cos from a per-keypoint LDS table.  That form was built,
passed these tests and was not kept -- docs/history.md, round 15.)  Same arithmetic on the same bits: count, keypoint bytes and
descriptor bytes must equal the CPU oracle's, bit for bit, no tolerance.

322x243 frames, 4 levels, 500 features (test_gpu_describe_blur_chain.py's shape).  Frames: a textured frame, its three np.rot90
turns and its two mirror images, so that the keypoints' angles fall in all four quadrants (c and r of either sign: 0x400000 + c on
both sides of 0x400000, products of either sign and signed zeros); the two turns that change the frame's shape are a batch
of their own.  65 frames in one launch (260 (frame, level) units) go through k_sel_compact's list and the pair instances, 8 frames
through the staged lists and the one-keypoint-per-wave instances; both tap sets in each.  Every frame of every batch is compared.
The coverage (odd keypoint count: the last keypoint alone in its wave; a wave whose two keypoints lie on different levels; angles
in each quadrant) is asserted on the oracle's keypoints, so a frame generator that stops producing a case fails here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARAMS = (500, 1.2, 4, 20, 7)
W, H = 322, 243
VARIANTS = ((0, 0), (1, 0))
# (width, height) -> the frame kinds of that shape
BATCHES = {(W, H): ("textured", "rot180", "mirror_lr", "mirror_ud"), (H, W): ("rot90", "rot270")}


def _frames():
    from orb_slam_tracking_amd import synth
    t = synth.synth_frames(1, W, H, 4121)[0]  # (a seed whose frame the selection does not fill up to 500: odd counts occur)
    f = {"textured": t, "rot90": np.rot90(t, 1), "rot180": np.rot90(t, 2), "rot270": np.rot90(t, 3),
         "mirror_lr": t[:, ::-1], "mirror_ud": t[::-1, :]}
    return {k: np.ascontiguousarray(v) for k, v in f.items()}


@pytest.fixture(scope="module")
def cases(oracle):
    """The frames and, per Gaussian variant and frame kind, the oracle's keypoints and descriptors (computed once, shared)."""
    frames = _frames()
    oe = oracle.Extractor(*PARAMS)
    ref = {}
    try:
        for v in VARIANTS:
            oracle.set_opencv_variant(*v)
            for name, img in frames.items():
                _, ko, do = oe(img)
                ref[v, name] = (ko.copy(), do.copy())
    finally:
        oracle.set_opencv_variant(0, 0)
    for (w, h), names in BATCHES.items():
        for name in names:
            assert frames[name].shape == (h, w), name
    return frames, ref


def test_coverage(cases):
    """What the frames are for, on the oracle's keypoints."""
    _, ref = cases
    for v in VARIANTS:
        ang = []
        for shape, names in BATCHES.items():
            odd, split = False, False
            for name in names:
                ko = ref[v, name][0]
                n = len(ko)
                assert n > 100, (v, name, n)
                octv = ko["octave"]
                assert (np.diff(octv) >= 0).all(), (v, name)  # level-major: keypoints 2 j and 2 j + 1 share a wave of the pair form
                odd |= n % 2 == 1
                split |= bool((octv[0:n - 1:2] != octv[1:n:2]).any())
                ang.append(ko["angle"].astype(np.float64))
                print(v, name, n, "keypoints, per level", np.bincount(octv, minlength=PARAMS[2]))
            # in each batch, so that both launches of the pair instances meet both cases
            assert odd, (v, shape, "no frame with an odd keypoint count")
            assert split, (v, shape, "no pair of keypoints (2 j, 2 j + 1) on two levels")
        ang = np.concatenate(ang)
        assert (ang >= 0).all() and (ang <= 360).all()
        for q in range(4):
            assert ((ang > 90 * q + 1) & (ang < 90 * q + 89)).sum() > 20, (v, q)
        cs, sn = np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang))
        assert (cs < 0).any() and (sn < 0).any() and ((cs < 0) & (sn < 0)).any()


def _extract_device(orbx, e, buf):
    import torch
    B, h, w = buf.shape
    cap = PARAMS[0]
    d_img = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    d_k = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    d_d = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_img, B, w, h, w, w * h, d_k, d_d, d_n, cap)
    n = d_n.cpu().numpy()
    kk = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap)
    dd = d_d.cpu().numpy().reshape(B, cap, 32)
    return n, kk, dd


def _same(n, kg, dg, ko, do, what):
    assert n == len(ko), what + (n, len(ko))
    assert kg.dtype.itemsize == 28 and kg[:n].tobytes() == ko.tobytes(), what + ("keypoints",)
    bad = np.nonzero((dg[:n] != do).any(1))[0]
    assert len(bad) == 0, what + ("descriptors", bad[:5])


def _run(orbx, cases, shape, B, pairs):
    frames, ref = cases
    w, h = shape
    names = BATCHES[shape]
    which = [names[i % len(names)] for i in range(B)]
    buf = np.stack([frames[nm] for nm in which])
    e = orbx.ORBextractor(*PARAMS, max_width=w, max_height=h, max_batch=B)
    try:
        with orbx.knobs(no_split=1):  # (one launch: batches of 16 frames and more go out as two half batches otherwise)
            for v in VARIANTS:
                e.set_opencv_variant(*v)
                n, kk, dd = _extract_device(orbx, e, buf)
                last = e.debug_last_launch()
                assert last["staged_lists"] == (0 if pairs else 1) and last["describe_pairs"] == (1 if pairs else 0), last
                for i in range(B):
                    _same(n[i], kk[i], dd[i], *ref[v, which[i]], (v, i, which[i]))
    finally:
        e.set_opencv_variant(0, 0)
        e.close()


@pytest.mark.parametrize("shape", sorted(BATCHES), ids=lambda s: "%dx%d" % s)
def test_pair_instances(orbx, cases, shape):
    """65 frames in one launch: 260 (frame, level) units, k_sel_compact's list, two keypoints per wave."""
    _run(orbx, cases, shape, 65, True)


@pytest.mark.parametrize("shape", sorted(BATCHES), ids=lambda s: "%dx%d" % s)
def test_staged_instances(orbx, cases, shape):
    """8 frames: 32 (frame, level) units, one keypoint per wave on the selection's staging lists."""
    _run(orbx, cases, shape, 8, False)
