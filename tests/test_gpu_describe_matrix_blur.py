"""k_describe_patch's 7x7 Gaussian on the matrix cores (v_mfma_i32_16x16x64_i8: H = (W - 128) G_s + 128, split into two int8
operands, Out = 256 V hi + V lo + const) against the CPU oracle, bit for bit: count, keypoint bytes, descriptor bytes.

The smallest shapes at which the blur can still go wrong: 322x243 frames, 4 levels.  Textured frames carry every byte shift of the
staged window ((kx - 21) & 3, which selects the horizontal tap fragment) at level 0 and above it, and windows that cross a level's
left / right side (the dword-by-dword staging); frames of random 0 / 255 blocks reach both ends of the int8 operand ranges and,
with the taps that sum to 257, the saturating sums.  Both Gaussian tap sets, both forms of the keypoint list (staged lists for up
to 256 (frame, level) units, k_sel_compact's list above), and a level 0 whose rows are not dword-aligned.  The coverage itself is
asserted on the oracle's output, so a change of the frame generator fails here and does not silently thin the test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARAMS = (500, 1.2, 4, 20, 7)
W, H = 322, 243
VARIANTS = ((0, 0), (1, 0))
# blurred positions (row, column) of the 37x37 patch that the 512 rotated sample points can reach
DISC = np.array([[(r - 18) ** 2 + (c - 18) ** 2 <= 365 for c in range(37)] for r in range(37)])


def _block_frame(seed, cell):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 2, ((H + cell - 1) // cell, (W + cell - 1) // cell), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.kron(g, np.ones((cell, cell), np.uint8))[:H, :W])


def _same(kg, dg, ko, do):
    assert len(kg) == len(ko), (len(kg), len(ko))
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        bad = np.nonzero(kg[f] != ko[f])[0]
        assert len(bad) == 0, (f, bad[:5], kg[f][bad[:5]], ko[f][bad[:5]])
    assert kg.tobytes() == ko.tobytes()
    bad = np.nonzero((dg != do).any(1))[0]
    assert len(bad) == 0, ("descriptors", bad[:5])


def _windows(oe, k):
    """Per keypoint of the frame the oracle extracted last: (level, byte shift of the staged window, window crosses the level's left
    or right side, 7x7 all-255 support inside the sampling disc), from the keypoint's level coordinates."""
    scale = oe.tables()["scale"]
    padded = {}
    out = np.zeros((len(k), 4), np.int64)
    for i, kp in enumerate(k):
        l = int(kp["octave"])
        w, _ = oe.level_size(l)
        kx, ky = int(round(float(kp["x"]) / float(scale[l]))), int(round(float(kp["y"]) / float(scale[l])))
        ax = (kx - 21) & ~3  # first staged byte (k_describe_patch): 48 bytes from there must lie inside the level's rows
        if l not in padded:
            padded[l] = np.pad(oe.level_image(l), 21, mode="reflect")
        win = padded[l][ky:ky + 43, kx:kx + 43]  # rows ky - 21 .. ky + 21, columns kx - 21 .. kx + 21
        full = np.lib.stride_tricks.sliding_window_view(win == 255, (7, 7)).all(axis=(2, 3))  # [37, 37]: support of blurred (r, c)
        out[i] = (l, (kx - 21) & 3, not (ax >= 0 and ax + 48 <= w), bool((full & DISC).any()))
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    """The frames and, per Gaussian variant, the oracle's results (computed once, shared, left unchanged)."""
    from orb_slam_tracking_amd import synth
    frames = {"textured": synth.synth_frames(2, W, H, 4100), "blocks": np.stack([_block_frame(7, 12), _block_frame(8, 9)]),
              "unaligned": synth.synth_frames(1, 321, H, 4101)}
    oe = oracle.Extractor(*PARAMS)
    ref, win = {}, {}
    try:
        for v in VARIANTS:
            oracle.set_opencv_variant(*v)
            for name, fr in frames.items():
                for f in range(len(fr)):
                    _, ko, do = oe(fr[f])
                    ref[v, name, f] = (ko.copy(), do.copy())
                    if v == (0, 0):
                        win[name, f] = _windows(oe, ko)
    finally:
        oracle.set_opencv_variant(0, 0)
    return frames, ref, win


def test_oracle_coverage(cases):
    """What the frames are for, on the oracle's own output."""
    _, ref, win = cases
    tex = np.concatenate([win["textured", 0], win["textured", 1]])
    blk = np.concatenate([win["blocks", 0], win["blocks", 1]])
    for s in range(4):
        assert ((tex[:, 0] == 0) & (tex[:, 1] == s)).sum() > 0 and ((tex[:, 0] > 0) & (tex[:, 1] == s)).sum() > 0, s
        assert ((blk[:, 0] > 0) & (blk[:, 1] == s)).sum() > 0, s
    assert tex[:, 2].sum() > 0 and blk[:, 2].sum() > 0   # windows that cross a level's side: the other staging path
    assert blk[:, 3].sum() > 0                          # a blurred byte of 255 * S * S: the top of both operand ranges
    assert win["unaligned", 0][:, 0].min() == 0         # level-0 keypoints on the unaligned frame
    for v in VARIANTS:
        assert sum(len(ref[v, "textured", f][0]) for f in range(2)) > 500 and sum(len(ref[v, "blocks", f][0]) for f in range(2)) > 300


def _extract_device(orbx, e, buf, w, stride):
    import torch
    B, cap = len(buf), PARAMS[0]
    d_img = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    d_k = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    d_d = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_img, B, w, H, stride, stride * H, d_k, d_d, d_n, cap)
    n = d_n.cpu().numpy()
    kk = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap)
    dd = d_d.cpu().numpy().reshape(B, cap, 32)
    return n, kk, dd


@pytest.mark.parametrize("name", ["textured", "blocks"])
def test_staged_lists(orbx, cases, name):
    """B = 2: 8 (frame, level) units, the descriptor kernel indexes the selection's staging lists itself."""
    frames, ref, _ = cases
    e = orbx.ORBextractor(*PARAMS, max_width=W, max_height=H, max_batch=2)
    try:
        for v in VARIANTS:
            e.set_opencv_variant(*v)
            n, kk, dd = _extract_device(orbx, e, frames[name], W, W)
            assert e.debug_last_launch()["staged_lists"] == 1
            for f in range(2):
                ko, do = ref[v, name, f]
                assert n[f] == len(ko), (v, f, n[f], len(ko))
                _same(kk[f, :n[f]], dd[f, :n[f]], ko, do)
    finally:
        e.set_opencv_variant(0, 0)
        e.close()


def test_compacted_lists(orbx, cases):
    """B = 65 in one launch: 260 (frame, level) units go through k_sel_compact.  Frames 0, 32 and 64 are a textured, the other
    textured and a block frame."""
    frames, ref, _ = cases
    four = [("textured", 0), ("textured", 1), ("blocks", 0), ("blocks", 1)]
    which = [four[(i + i // 32) % 4] for i in range(65)]
    assert [which[i] for i in (0, 32, 64)] == four[:3]
    buf = np.stack([frames[nm][f] for nm, f in which])
    e = orbx.ORBextractor(*PARAMS, max_width=W, max_height=H, max_batch=65)
    try:
        with orbx.knobs(no_split=1):  # (one launch of 65 frames: batches of 16 frames and more go out as two half batches otherwise)
            for v in VARIANTS:
                e.set_opencv_variant(*v)
                n, kk, dd = _extract_device(orbx, e, buf, W, W)
                assert e.debug_last_launch()["staged_lists"] == 0
                for i in (0, 32, 64):
                    ko, do = ref[(v,) + which[i]]
                    assert n[i] == len(ko), (v, i, n[i], len(ko))
                    _same(kk[i, :n[i]], dd[i, :n[i]], ko, do)
    finally:
        e.set_opencv_variant(0, 0)
        e.close()


def test_unaligned_level0(orbx, cases):
    """Width 321 with a byte-packed row stride: level 0 is staged dword by dword from bytes, in rows of the kernel's LDS stride."""
    frames, ref, _ = cases
    e = orbx.ORBextractor(*PARAMS, max_width=321, max_height=H, max_batch=1)
    try:
        for v in VARIANTS:
            e.set_opencv_variant(*v)
            n, kk, dd = _extract_device(orbx, e, frames["unaligned"], 321, 321)
            ko, do = ref[v, "unaligned", 0]
            assert n[0] == len(ko), (v, n[0], len(ko))
            _same(kk[0, :n[0]], dd[0, :n[0]], ko, do)
    finally:
        e.set_opencv_variant(0, 0)
        e.close()
