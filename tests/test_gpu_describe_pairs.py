"""k_describe_patch's pair form -- one wave describes keypoints 2 j and 2 j + 1 of a frame's level-major list: lanes 0..30 / 32..62 of
IC_Angle on the two windows, fastAtan2 and cos / sin once with lane = keypoint, staging, blur and steered BRIEF one keypoint after
the other -- against the CPU oracle, bit for bit: count, keypoint bytes (the angle among them), descriptor bytes.  The pair form runs
exactly where a launch takes k_sel_compact's list (more than 256 (frame, level) units); every case asserts
debug_last_launch()["describe_pairs"] and ["staged_lists"], so that it runs the form it names, and the same frames go through the
staged one-keypoint-per-wave form in a batch of two.  The cases are what a shared wave can get wrong, on 322x243 frames:
  * tails: frames of 0 .. 16 keypoints (single faint pixels: 0, 1, 2, 3 keypoints and every residue modulo the six keypoints of a
    workgroup, a dead half B wherever the count is odd) in one batch of 34 frames, beside flat frames;
  * a pair on two levels (geometry, image base, byte shift differ): eight levels with quotas of one and two keypoints at the top;
    every combination of the two byte shifts (s_A, s_B) in 0..3 x 0..3;
  * a window across its level's left / right side (dword-by-dword staging) in half A only, in half B only, in both;
  * the two halves in different octants of fastAtan2 and on both sides of the |m10| >= |m01| split; every special value (m10 = 0,
    m01 = 0, both 0, |m01| = |m10|) in half A, in half B, and special values in both halves of one pair;
  * the two keypoints of a pair within a few pixels of each other (500 keypoints on a textured frame: overlapping windows, so one half
    writing into the other's LDS slice shows);
  * both Gaussian tap sets, both libm readings.
Every situation is asserted on the oracle's own output (test_oracle_coverage), so a change of a frame generator fails here and does
not silently thin the test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 322, 243
BIG = (500, 1.2, 4, 20, 7)
TAILS = (100, 1.2, 8, 20, 7)
SMALL_NF = (15, 16, 14)
PER_GROUP = 6   # keypoints per workgroup of the pair form: three waves of two
VARIANTS = tuple((gv, lm) for gv in (0, 1) for lm in (1, 0))  # (Gaussian tap set, libm reading: 1 = FLOAT, 0 = DOUBLE)
# satellite offsets (du, dv): m10 = 54 du, m01 = 54 dv at level 0 -- the eight octants, then the special values
KINDS = ((10, 4), (4, 10), (-4, 10), (-10, 4), (-10, -4), (-4, -10), (4, -10), (10, -4),
         (0, 0), (0, 8), (0, -8), (8, 0), (-8, 0), (8, 8), (-8, -8), (-8, 8), (8, -8))
DOT_SEEDS = (0, 1, 2)
N_TAIL = 15     # tail frames: 0 .. 14 faint pixels, 0 .. 16 keypoints


def _small(nf):
    return (nf, 1.2, 8, 20, 7)


def _dot_frame(seed):
    """Single bright pixels (FAST corners on their own), each with a faint 3x3 satellite that sets the patch's moments.  The columns
    x = 20 and x = 300 put the window across the level's left and right side."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 60, np.uint8)
    sites = [(x, y) for y in range(30, 220, 36) for x in [20] + list(range(56, 290, 36)) + [300]]
    for (x, y), kind in zip(sites, rng.permutation(len(sites)) % len(KINDS)):
        img[y, x] = 220
        du, dv = KINDS[kind]
        if (du, dv) != (0, 0):
            img[y + dv - 1:y + dv + 2, x + du - 1:x + du + 2] = 66  # below minThFAST: no corner, only moments
    return img


def _tail_frame(n):
    """n single pixels 10 above a flat ground, spread over the frame (the selection keeps one corner per quadtree node): corners at
    level 0 for minThFAST = 7, most of them too faint after one resize."""
    sites = [(40 + 60 * c, 40 + 80 * r) for r in range(3) for c in range(5)]
    img = np.full((H, W), 60, np.uint8)
    for j in range(n):
        x, y = sites[(11 * j) % 15]
        img[y, x] = 70
    return img


def _info(oracle, oe, k):
    """Per keypoint of the frame the oracle extracted last: (level, x, y in level pixels, m10, m01, window crosses the level's left or
    right side, byte shift of the staged window).  The moments are the oracle's IC_Angle's on its own level image."""
    scale = oe.tables()["scale"]
    imgs = {}
    out = np.zeros((len(k), 7), np.int64)
    for i, kp in enumerate(k):
        l = int(kp["octave"])
        w, _ = oe.level_size(l)
        kx, ky = int(round(float(kp["x"]) / float(scale[l]))), int(round(float(kp["y"]) / float(scale[l])))
        if l not in imgs:
            imgs[l] = oe.level_image(l)
        a, m10, m01 = oracle.ic_angle(imgs[l], kx, ky)
        assert np.float32(a) == kp["angle"], (i, a, kp["angle"])
        ax = (kx - 21) & ~3  # first staged byte (k_describe_patch): 48 bytes from there must lie inside the level's rows
        out[i] = (l, kx, ky, m10, m01, not (ax >= 0 and ax + 48 <= w), (kx - 21) & 3)
    return out


def _octant(m10, m01):
    """0 .. 7 counter-clockwise from the +m10 axis, -1 on a special value of fastAtan2."""
    if m10 == 0 or m01 == 0 or abs(m10) == abs(m01):
        return -1
    q = 0 if m10 > 0 and m01 > 0 else 1 if m10 < 0 and m01 > 0 else 2 if m10 < 0 else 3
    steep = abs(m01) > abs(m10)
    return 2 * q + int(steep if q in (0, 2) else not steep)


def _special(m10, m01):
    """Which special value of fastAtan2: 0 none, 1 m10 = 0 only, 2 m01 = 0 only, 3 both 0, 4 |m01| = |m10| != 0."""
    if m10 == 0 and m01 == 0:
        return 3
    if m10 == 0:
        return 1
    if m01 == 0:
        return 2
    return 4 if abs(m10) == abs(m01) else 0


def _pairs(n):
    """The waves' pairs (A, B) of consecutive keypoints of a frame's list; a last keypoint on its own has no B."""
    return [(2 * j, 2 * j + 1) for j in range(n // 2)]


@pytest.fixture(scope="module")
def cases(oracle):
    """The frames and, per (Gaussian, libm) variant, the oracle's results (computed once, shared, left unchanged)."""
    from orb_slam_tracking_amd import synth
    frames = {"textured": synth.synth_frames(1, W, H, 4101)[0], "small": synth.synth_frames(1, W, H, 4200)[0],
              "empty": np.full((H, W), 128, np.uint8)}
    for sd in DOT_SEEDS:
        frames["dots%d" % sd] = _dot_frame(sd)
    for n in range(N_TAIL):
        frames["tail%d" % n] = _tail_frame(n)
    ref, info = {}, {}
    try:
        for v in VARIANTS:
            oracle.set_opencv_variant(v[0], 0)
            oracle.set_libm_variant(v[1])
            oe = oracle.Extractor(*BIG)
            for name in ["textured"] + ["dots%d" % sd for sd in DOT_SEEDS]:
                _, ko, do = oe(frames[name])
                ref[v, name] = (ko.copy(), do.copy())
                if v == VARIANTS[0]:
                    info[name] = _info(oracle, oe, ko)
            oe = oracle.Extractor(*TAILS)
            for name in ["tail%d" % n for n in range(N_TAIL)] + ["empty"]:
                _, ko, do = oe(frames[name])
                ref[v, "T", name] = (ko.copy(), do.copy())
            for nf in SMALL_NF:
                oe = oracle.Extractor(*_small(nf))
                _, ko, do = oe(frames["small"])
                ref[v, nf, "small"] = (ko.copy(), do.copy())
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
        counts = [len(ref[v, "T", "tail%d" % n][0]) for n in range(N_TAIL)]
        assert counts[:4] == [0, 1, 2, 3] and max(counts) > 2 * PER_GROUP, counts  # (odd counts: a dead half B)
        assert {c % PER_GROUP for c in counts} == set(range(PER_GROUP))  # every residue modulo the keypoints of a workgroup
        assert len(ref[v, "T", "empty"][0]) == 0
        for nf in SMALL_NF:
            assert len(ref[v, nf, "small"][0]) == nf and len(ref[v, nf, "empty"][0]) == 0
        assert len(ref[v, "textured"][0]) == 500
        for sd in DOT_SEEDS:
            assert len(ref[v, "dots%d" % sd][0]) > 100
            assert np.array_equal(ref[v, "dots%d" % sd][0]["angle"], ref[VARIANTS[0], "dots%d" % sd][0]["angle"])
    # a pair on two levels (different geometry and image base), also with different byte shifts
    for nf in SMALL_NF:
        t = info[nf]
        assert any(t[a, 0] != t[b, 0] for a, b in _pairs(len(t))), nf
    assert any(t[a, 0] != t[b, 0] and t[a, 6] != t[b, 6] for nf in SMALL_NF for t in [info[nf]] for a, b in _pairs(len(t)))
    tex = info["textured"]
    dots = [info["dots%d" % sd] for sd in DOT_SEEDS]
    everything = [tex] + dots
    # every combination of the two byte shifts
    assert {(int(t[a, 6]), int(t[b, 6])) for t in everything for a, b in _pairs(len(t))} == {(p, q) for p in range(4) for q in range(4)}
    # the two keypoints of a pair on one level within 4 pixels of each other: overlapping windows
    assert any(tex[a, 0] == tex[b, 0] and abs(tex[a, 1] - tex[b, 1]) <= 4 and abs(tex[a, 2] - tex[b, 2]) <= 4 for a, b in _pairs(len(tex)))
    # side-crossing windows: A only, B only, both
    cross = {(int(t[a, 5]), int(t[b, 5])) for t in everything for a, b in _pairs(len(t))}
    assert cross == {(0, 0), (1, 0), (0, 1), (1, 1)}, cross
    # angles: the two halves in different octants on both sides of the |m10| >= |m01| split, in both orders
    split = set()
    for t in dots:
        for a, b in _pairs(len(t)):
            oa, ob = _octant(t[a, 3], t[a, 4]), _octant(t[b, 3], t[b, 4])
            if oa >= 0 and ob >= 0 and oa != ob:
                split.add((bool(abs(t[a, 3]) >= abs(t[a, 4])), bool(abs(t[b, 3]) >= abs(t[b, 4]))))
    assert split == {(True, True), (True, False), (False, True), (False, False)}, split
    assert {_octant(a, b) for t in dots for a, b in t[:, 3:5]} == set(range(-1, 8))
    # every special value in half A and in half B; special values in both halves of one pair
    inA = {_special(t[a, 3], t[a, 4]) for t in dots for a, _ in _pairs(len(t))}
    inB = {_special(t[b, 3], t[b, 4]) for t in dots for _, b in _pairs(len(t))}
    assert inA == {0, 1, 2, 3, 4} and inB == {0, 1, 2, 3, 4}, (inA, inB)
    assert any(_special(t[a, 3], t[a, 4]) and _special(t[b, 3], t[b, 4]) for t in dots for a, b in _pairs(len(t)))
    assert any(_special(t[a, 3], t[a, 4]) and not _special(t[b, 3], t[b, 4]) for t in dots for a, b in _pairs(len(t)))
    assert any(not _special(t[a, 3], t[a, 4]) and _special(t[b, 3], t[b, 4]) for t in dots for a, b in _pairs(len(t)))
    # the diagonal in every quadrant
    m10 = np.concatenate([t[:, 3] for t in dots])
    m01 = np.concatenate([t[:, 4] for t in dots])
    for sx in (1, -1):
        for sy in (1, -1):
            assert ((m10 * sx > 0) & (m01 * sy > 0) & (abs(m10) == abs(m01))).any(), (sx, sy)


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
    # (0xa5 everywhere: a slot past a frame's count must come back untouched -- a dead half B stores nothing)
    d_k = torch.full((B * cap * 28,), 0xa5, dtype=torch.uint8, device="cuda")
    d_d = torch.full((B * cap * 32,), 0xa5, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_img, B, W, H, W, W * H, d_k, d_d, d_n, cap)
    n = d_n.cpu().numpy()
    kk = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap)
    dd = d_d.cpu().numpy().reshape(B, cap, 32)
    return n, kk, dd


def _run(orbx, cases, params, names, keys, check, pairs):
    """Extracts the batch `names` for every variant and compares the frames `check` with the oracle's results ref[v, *keys[i]].
    pairs = 1: the launch must take k_sel_compact's list and the pair form; 0: the staging lists, one keypoint per wave."""
    frames, ref, _ = cases
    buf = np.stack([frames[nm] for nm in names])
    cap = params[0]
    e = orbx.ORBextractor(*params, max_width=W, max_height=H, max_batch=len(buf))
    try:
        with orbx.knobs(no_split=1):  # (one launch: batches of 16 frames and more go out as two half batches otherwise)
            for v in VARIANTS:
                e.set_opencv_variant(v[0], 0)
                e.set_libm_variant(v[1])
                n, kk, dd = _extract_device(orbx, e, buf, cap)
                info = e.debug_last_launch()
                assert info["describe_pairs"] == pairs and info["staged_lists"] == 1 - pairs, info
                for i in check:
                    ko, do = ref[(v,) + keys[i]]
                    assert n[i] == len(ko), (v, i, n[i], len(ko))
                    _same(kk[i, :n[i]], dd[i, :n[i]], ko, do)
                    # nothing is stored past the frame's count (the slot of a dead half B first of all)
                    assert (kk[i, n[i]:].view(np.uint8) == 0xa5).all() and (dd[i, n[i]:] == 0xa5).all(), (v, i)
    finally:
        e.set_opencv_variant(0, 0)
        e.set_libm_variant(e.LIBM_DEFAULT)
        e.close()


def _tail_names():
    """34 frames: the tail frames, a flat frame after each, and the first four once more at the end."""
    names = []
    for n in range(N_TAIL):
        names += ["tail%d" % n, "empty"]
    return names + ["tail%d" % n for n in range(4)]


def test_tails_pairs(orbx, cases):
    """34 frames of eight levels in one launch: 272 (frame, level) units go through k_sel_compact; counts 0 .. 16."""
    names = _tail_names()
    assert len(names) * TAILS[2] > 256
    _run(orbx, cases, TAILS, names, [("T", nm) for nm in names], range(len(names)), 1)


def test_tails_staged(orbx, cases):
    """The same frames in staged launches (32 frames = 256 units at the most), one keypoint per wave: identical bytes."""
    names = _tail_names()[:32]
    _run(orbx, cases, TAILS, names, [("T", nm) for nm in names], range(len(names)), 0)


@pytest.mark.parametrize("nf", SMALL_NF)
def test_levels_pairs(orbx, cases, nf):
    """33 frames of eight levels with quotas of one and two keypoints at the top: pairs that straddle two levels."""
    names = ["small" if i % 2 == 0 else "empty" for i in range(33)]
    _run(orbx, cases, _small(nf), names, [(nf, nm) for nm in names], (0, 1, 31, 32), 1)


@pytest.mark.parametrize("nf", SMALL_NF)
def test_levels_staged(orbx, cases, nf):
    _run(orbx, cases, _small(nf), ["small", "empty"], [(nf, "small"), (nf, "empty")], (0, 1), 0)


def _big_names(n):
    cyc = ["textured"] + ["dots%d" % sd for sd in DOT_SEEDS]
    return [cyc[i % len(cyc)] for i in range(n)]


def test_angles_sides_neighbours_pairs(orbx, cases):
    """65 frames of four levels in one launch: 260 units.  The textured frame and the dot frames, first and last of each checked."""
    names = _big_names(65)
    _run(orbx, cases, BIG, names, [(nm,) for nm in names], (0, 1, 2, 3, 61, 62, 63, 64), 1)


def test_angles_sides_neighbours_staged(orbx, cases):
    names = _big_names(4)
    _run(orbx, cases, BIG, names, [(nm,) for nm in names], (0, 1, 2, 3), 0)
