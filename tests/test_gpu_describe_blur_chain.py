"""k_describe_patch's vertical blur product takes the lo chain's result, shifted right by 8, as the accumulator of the hi chain:
Out' = V hi + ((V lo + CLO) >> 8), blurred byte = byte 1 of Out' (saturated at 0xffff for the taps that sum to 257), in place of
byte 2 of 256 (V hi) + (V lo + CLO).  Count, keypoint bytes and descriptor bytes against the CPU oracle, bit for bit.

322x243 frames, 4 levels, 500 features (test_gpu_describe_matrix_blur.py's shape: the smallest that reaches every byte shift of the
staged window and a window across a level's side).  Frames: flat 0, flat 255, random 0 / 255 blocks, a textured frame, and a frame
of bands of nine equal rows of noise -- inside a band all seven rows under a vertical tap window hold the same H, which is what
takes V lo to both ends of its range.  Both tap sets, the staged lists (one keypoint per wave) and k_sel_compact's list (two per
wave, more than 256 (frame, level) units).

The two-chain arithmetic is restated here in numpy (H, hi, lo, Lo, Hi) on the windows of the oracle's keypoints and checked
against the plain 7x7 sum and against the oracle's blurred levels; the coverage is asserted on that restatement, so a frame
generator that stops producing a case fails here and does not silently thin the test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARAMS = (500, 1.2, 4, 20, 7)
W, H = 322, 243
VARIANTS = ((0, 0), (1, 0))
TAPS = {0: np.array([18, 34, 48, 56, 48, 34, 18], np.int64), 1: np.array([18, 34, 49, 55, 49, 34, 18], np.int64)}
# blurred positions (row, column) of the 37x37 patch that the 512 rotated sample points can reach
DISC = np.array([[(r - 18) ** 2 + (c - 18) ** 2 <= 365 for c in range(37)] for r in range(37)])
NAMES = ("flat0", "flat255", "blocks", "textured", "bands")


def _block_frame(seed, cell):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 2, ((H + cell - 1) // cell, (W + cell - 1) // cell), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.kron(g, np.ones((cell, cell), np.uint8))[:H, :W])


def _band_frame(seed, rows):
    """Bands of `rows` equal rows of uniform noise."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, ((H + rows - 1) // rows, W), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(g, rows, axis=0)[:H])


def _frames():
    from orb_slam_tracking_amd import synth
    return {"flat0": np.zeros((H, W), np.uint8), "flat255": np.full((H, W), 255, np.uint8), "blocks": _block_frame(7, 12),
            "textured": synth.synth_frames(1, W, H, 4100)[0], "bands": _band_frame(11, 9)}


def two_chains(win, gv):
    """The kernel's arithmetic on windows [N, 43, 43] (rows ky - 21 .., columns kx - 21 ..): per blurred position [N, 37, 37] the
    lo chain's result Lo, the hi chain's Hi, and the blurred byte of the old and of the new form."""
    T = TAPS[gv]
    S = int(T.sum())
    CLO = 128 * S * S + 32768
    w = win.astype(np.int64)
    Hm = sum(T[j] * (w[:, :, j:j + 37] - 128) for j in range(7)) + 128          # [N, 43, 37]
    assert Hm.min() >= -32768 and Hm.max() <= 32767
    hi, lo = Hm >> 8, (Hm & 255) - 128                                           # signed byte 1; byte 0 - 128
    assert np.array_equal(256 * hi + lo + 128, Hm) and hi.min() >= -128 and hi.max() <= 127
    Lo = sum(T[k] * lo[:, k:k + 37, :] for k in range(7)) + CLO                  # [N, 37, 37]
    Hi = sum(T[k] * hi[:, k:k + 37, :] for k in range(7))
    assert Lo.min() >= 0
    old = np.minimum(256 * Hi + Lo, 0xffffff) >> 16
    new = np.minimum(Hi + (Lo >> 8), 0xffff) >> 8
    plain = sum(T[k] * sum(T[j] * w[:, k:k + 37, j:j + 37] for j in range(7)) for k in range(7))
    assert np.array_equal(old, np.minimum((plain + 32768) >> 16, 255))
    return Lo, Hi, old, new


def _windows(oe, k):
    """Per keypoint of the frame the oracle extracted last: its 43x43 window (REFLECT_101 at the level's sides) and the blurred
    37x37 patch around it from the oracle's blurred level; (level, byte shift of the staged window, window crosses a side)."""
    scale = oe.tables()["scale"]
    padded, blurred = {}, {}
    win, blr, info = np.zeros((len(k), 43, 43), np.uint8), np.zeros((len(k), 37, 37), np.uint8), np.zeros((len(k), 3), np.int64)
    for i, kp in enumerate(k):
        l = int(kp["octave"])
        w, _ = oe.level_size(l)
        kx, ky = int(round(float(kp["x"]) / float(scale[l]))), int(round(float(kp["y"]) / float(scale[l])))
        if l not in padded:
            padded[l] = np.pad(oe.level_image(l), 21, mode="reflect")
            blurred[l] = np.pad(oe.level_blurred(l), 21, mode="reflect")
        win[i] = padded[l][ky:ky + 43, kx:kx + 43]
        blr[i] = blurred[l][ky + 3:ky + 40, kx + 3:kx + 40]
        ax = (kx - 21) & ~3
        info[i] = (l, (kx - 21) & 3, not (ax >= 0 and ax + 48 <= w))
    return win, blr, info


@pytest.fixture(scope="module")
def cases(oracle):
    """The frames and, per Gaussian variant, the oracle's results and its keypoints' windows (computed once, shared, unchanged)."""
    frames = _frames()
    oe = oracle.Extractor(*PARAMS)
    oe.keep_blurred(True)
    ref, win = {}, {}
    try:
        for v in VARIANTS:
            oracle.set_opencv_variant(*v)
            for name in NAMES:
                _, ko, do = oe(frames[name])
                ref[v, name] = (ko.copy(), do.copy())
                win[v, name] = _windows(oe, ko)
    finally:
        oracle.set_opencv_variant(0, 0)
    return frames, ref, win


def test_restatement_and_coverage(cases):
    """The identity on every blurred position of every keypoint's patch, and what the frames are for."""
    _, ref, win = cases
    for v in VARIANTS:
        gv = v[0]
        S = int(TAPS[gv].sum())
        CLO = 128 * S * S + 32768
        lo8, carry, low, top = [], [], [], 0
        for name in NAMES:
            w, blr, info = win[v, name]
            assert (len(w) == 0) == name.startswith("flat"), (v, name, len(w))
            if len(w) == 0:
                continue
            Lo, Hi, old, new = two_chains(w, gv)
            assert np.array_equal(new, old), (v, name)
            assert np.array_equal(new[:, DISC], blr[:, DISC]), (v, name)  # the oracle's blurred level at the same positions
            assert new.max() <= 255
            lo8.append((Lo >> 8)[:, DISC].ravel())
            carry.append((((Hi & 255) + ((Lo >> 8) & 255)) >> 8)[:, DISC].ravel())
            low.append(((Hi + (Lo >> 8)) & 255)[:, DISC].ravel())
            top = max(top, int((Hi + (Lo >> 8))[:, DISC].max()))
            print(v, name, len(w), "keypoints; Lo >> 8 in", int(lo8[-1].min()), int(lo8[-1].max()), "max Out'", top)
        lo8, carry, low = np.concatenate(lo8), np.concatenate(carry), np.concatenate(low)
        # Lo >> 8 at both ends of its range: every lo of the seven rows at its smallest value, -128, and at its largest (to within
        # what the shift drops).  H's low byte is (sum of taps x pixels + 128) mod 256, a multiple of g = gcd(taps, 256): the
        # largest lo is 127 with the taps that sum to 257 and 126 with the others, which are all even
        g = int(np.gcd.reduce(np.append(TAPS[gv], 256)))
        assert g == (1 if gv else 2)
        lo_max = 256 - g - 128
        assert int(lo8.min()) == (CLO - 128 * S) >> 8 and int(lo8.max()) == (CLO + lo_max * S) >> 8, (v, int(lo8.min()), int(lo8.max()))
        # the addition of Lo >> 8 to Hi carries out of the low byte (the old form's carry into bit 16) and does not, and the sum
        # lands directly below and directly on a multiple of 256
        assert (carry == 1).any() and (carry == 0).any()
        assert (low == 255).any() and (low == 0).any()
        # the saturating case: only with the taps that sum to 257
        assert (top > 0xffff) == (gv == 1), (v, top)
    # the shapes' own purposes: every byte shift at level 0 and above, a window across a side, both on the texture and the bands
    for name in ("textured", "bands"):
        info = win[(0, 0), name][2]
        for s in range(4):
            assert ((info[:, 0] == 0) & (info[:, 1] == s)).any() and ((info[:, 0] > 0) & (info[:, 1] == s)).any(), (name, s)
        assert info[:, 2].any(), name


def _extract_device(orbx, e, buf):
    import torch
    B, cap = len(buf), PARAMS[0]
    d_img = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    d_k = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    d_d = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_img, B, W, H, W, W * H, d_k, d_d, d_n, cap)
    n = d_n.cpu().numpy()
    kk = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap)
    dd = d_d.cpu().numpy().reshape(B, cap, 32)
    return n, kk, dd


def _same(n, kg, dg, ko, do, what):
    assert n == len(ko), what + (n, len(ko))
    assert kg[:n].tobytes() == ko.tobytes(), what + ("keypoints",)
    bad = np.nonzero((dg[:n] != do).any(1))[0]
    assert len(bad) == 0, what + ("descriptors", bad[:5])


def test_staged_lists(orbx, cases):
    """B = 5: 20 (frame, level) units, one keypoint per wave on the selection's staging lists."""
    frames, ref, _ = cases
    e = orbx.ORBextractor(*PARAMS, max_width=W, max_height=H, max_batch=len(NAMES))
    try:
        for v in VARIANTS:
            e.set_opencv_variant(*v)
            n, kk, dd = _extract_device(orbx, e, np.stack([frames[nm] for nm in NAMES]))
            last = e.debug_last_launch()
            assert last["staged_lists"] == 1 and last["describe_pairs"] == 0
            for f, nm in enumerate(NAMES):
                _same(n[f], kk[f], dd[f], *ref[v, nm], (v, nm))
    finally:
        e.set_opencv_variant(0, 0)
        e.close()


def test_compacted_lists(orbx, cases):
    """B = 65 in one launch: 260 (frame, level) units go through k_sel_compact, two keypoints per wave.  The frames cycle through
    the five kinds, so flat frames (no keypoint) sit between the others; frames 0 .. 4 and 60 .. 64 are compared."""
    frames, ref, _ = cases
    which = [NAMES[i % len(NAMES)] for i in range(65)]
    buf = np.stack([frames[nm] for nm in which])
    e = orbx.ORBextractor(*PARAMS, max_width=W, max_height=H, max_batch=65)
    try:
        with orbx.knobs(no_split=1):  # (one launch of 65 frames: batches of 16 frames and more go out as two half batches otherwise)
            for v in VARIANTS:
                e.set_opencv_variant(*v)
                n, kk, dd = _extract_device(orbx, e, buf)
                last = e.debug_last_launch()
                assert last["staged_lists"] == 0 and last["describe_pairs"] == 1
                for i in list(range(5)) + list(range(60, 65)):
                    _same(n[i], kk[i], dd[i], *ref[v, which[i]], (v, i, which[i]))
    finally:
        e.set_opencv_variant(0, 0)
        e.close()
