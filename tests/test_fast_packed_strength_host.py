"""The packed f16 arc strength of k_fast / k_fast_wave (fastStrengthBiased, orbx_kernels.hip), restated with numpy.float16 and
integer halves, against the oracle's FAST strength: exact, no tolerance.  A register of the device network carries
(B + v - p_k, B - v + p_k) with B = 0x6500; read as f16 both halves are integers of the binade whose ulp is 1, so one network of
minimum3 / maximum3 serves the bright and the dark side at once.  Runs without a GPU."""
import itertools

import numpy as np
import pytest

import oracle_lib as O

B = 0x6500
LO, HI = 0x6401, 0x65FF
# ring pixel k at (dx, dy) from the centre, the kernels' order
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2),
        (-1, 3))
EDGE = (0, 1, 127, 128, 254, 255)
CENTRES = (0, 1, 128, 254, 255)


def packed_strength(v, ring):
    """v: (N,) centres, ring: (N, 16) ring pixels, both 0 .. 255.  Returns (strength, smallest half, largest half, smn, smx) of the
    packed form: v_pk_mad_i16 twice (16-bit wrap-around arithmetic), the minimum3 / minimum3 / maximum3 network on f16 pairs."""
    v = v.astype(np.uint16)[:, None]
    p = ring.astype(np.uint16)
    one, minus = np.uint16(1), np.uint16(0xFFFF)
    k_lo, k_hi = v * one + np.uint16(B), v * minus + np.uint16(B)          # K = v * (+1, -1) + (B, B)
    e_lo, e_hi = p * minus + k_lo, p * one + k_hi                          # e_k = p_k * (-1, +1) + K
    halves = np.stack([e_lo, e_hi])                                        # (2, N, 16) u16
    f = halves.view(np.float16)
    assert not np.isnan(f).any()
    idx = np.arange(16)
    mn3 = np.minimum(np.minimum(f, f[..., (idx + 1) & 15]), f[..., (idx + 2) & 15])
    arc = np.minimum(np.minimum(mn3, mn3[..., (idx + 3) & 15]), mn3[..., (idx + 6) & 15])
    r = arc.max(axis=-1)                                                   # (2, N) f16: (B + smn, B - smx)
    r16 = np.ascontiguousarray(r).view(np.uint16).astype(np.int32)
    assert np.array_equal(r16 - 0x6400, r.astype(np.int32) - 1024)         # the bit pattern 0x6400 + n IS the f16 value 1024 + n
    return r16.max(axis=0) - B, int(halves.min()), int(halves.max()), r16[0] - B, B - r16[1]


def oracle_strength(v, ring):
    """The oracle's strength of every (centre, ring): the rings are laid out as 7 x 7 patches of one image."""
    n = len(v)
    cols = 1024
    rows = (n + cols - 1) // cols
    img = np.zeros((rows * 7, cols * 7), np.uint8)
    cy, cx = (np.arange(n) // cols) * 7 + 3, (np.arange(n) % cols) * 7 + 3
    img[cy, cx] = v
    for k, (dx, dy) in enumerate(RING):
        img[cy + dy, cx + dx] = ring[:, k]
    L = O.lib()
    ptr, w, h, st = O._p(img), img.shape[1], img.shape[0], img.strides[0]
    fs = L.orbo_fast_strength
    out = np.empty(n, np.int32)
    for i, (x, y) in enumerate(zip(cx.tolist(), cy.tolist())):
        out[i] = fs(ptr, w, h, st, x, y)
    # (the library entry point is what oracle_lib.fast_strength calls; spot-check the wrapper itself)
    for i in range(0, n, max(1, n // 7)):
        assert O.fast_strength(img, int(cx[i]), int(cy[i])) == out[i]
    return out


def numpy_strength(v, ring):
    """The definition, in int32: max over the 16 arcs of 9 of min(v - p_k) and of min(p_k - v)."""
    d = v.astype(np.int32)[:, None] - ring.astype(np.int32)
    idx = np.arange(16)
    win = np.stack([d[:, (idx + j) & 15] for j in range(9)])               # (9, N, 16): arc starting at k
    return np.maximum(win.min(axis=0).max(axis=-1), (-win).min(axis=0).max(axis=-1))


def edge_rings():
    """Rings over EDGE, exhaustive per arc position: for every start of the arc, every arc length 8, 9 and 10 (an arc just
    short of nine pixels, one of exactly nine, a longer one), the arc filled with one edge value, ONE pixel of it replaced by
    every edge value in every place, the rest of the ring filled with every edge value, against every centre."""
    rings, cen = [], []
    for start in range(16):
        for n in (8, 9, 10):
            arc = [(start + j) & 15 for j in range(n)]
            for a, b, c in itertools.product(EDGE, EDGE, EDGE):
                base = np.full(16, b, np.uint8)
                base[arc] = a
                for odd in (arc if c != a else arc[:1]):
                    r = base.copy()
                    r[odd] = c
                    rings.append(r)
    rings = np.unique(np.array(rings, np.uint8), axis=0)
    for cv in CENTRES:
        cen.append(np.full(len(rings), cv, np.uint8))
    return np.concatenate(cen), np.tile(rings, (len(CENTRES), 1))


def two_valued_rings():
    """Every ring of {0, 255}^16 (all 65,536 arc shapes, at the top of the range on both sides) against centres 0, 128, 255."""
    masks = np.arange(1 << 16, dtype=np.uint32)
    rings = (((masks[:, None] >> np.arange(16)) & 1) * 255).astype(np.uint8)
    cen = np.concatenate([np.full(len(rings), cv, np.uint8) for cv in (0, 128, 255)])
    return cen, np.tile(rings, (3, 1))


def random_rings():
    rng = np.random.default_rng(8008)
    n = 100_000
    v = rng.integers(0, 256, n).astype(np.uint8)
    ring = rng.integers(0, 256, (n, 16)).astype(np.uint8)
    # a third of them near the centre value, a third with a planted arc of 9 .. 12 pixels: random bytes alone rarely hold an arc
    near = slice(n // 3, 2 * n // 3)
    ring[near] = np.clip(v[near, None].astype(np.int32) + rng.integers(-12, 13, (n // 3, 16)), 0, 255).astype(np.uint8)
    for i in range(2 * n // 3, n):
        s, ln = int(rng.integers(0, 16)), int(rng.integers(9, 13))
        sign = 1 if rng.integers(0, 2) else -1
        arc = [(s + j) & 15 for j in range(ln)]
        ring[i, arc] = np.clip(int(v[i]) + sign * rng.integers(1, 120, ln), 0, 255)
    return v, ring


@pytest.mark.parametrize("family", ["edge_values", "two_valued", "random"])
def test_packed_strength_equals_the_oracle(family):
    v, ring = {"edge_values": edge_rings, "two_valued": two_valued_rings, "random": random_rings}[family]()
    got, lo, hi, smn, smx = packed_strength(v, ring)
    print("%s: %d rings, halves 0x%04x .. 0x%04x, strength %d .. %d" % (family, len(v), lo, hi, got.min(), got.max()))
    assert LO <= lo and hi <= HI, (hex(lo), hex(hi))
    want = oracle_strength(v, ring)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), v[bad[:3]], ring[bad[:3]], got[bad[:3]], want[bad[:3]])
    assert np.array_equal(want, numpy_strength(v, ring))
    # the coverage this family owes
    d = v.astype(np.int32)[:, None] - ring.astype(np.int32)
    if family in ("edge_values", "two_valued"):
        assert lo == LO and hi == HI                                  # both ends of the range of a half are reached
        assert (smn == 255).any() and (smx == -255).any()             # strength 255 on the bright-centre and on the dark-centre side
        assert got.max() == 255
        # a ring with an arc of nine on one side AND compass pixels of the other sign (k = 0, 4, 8, 12: what the quick reject reads)
        compass = d[:, [0, 4, 8, 12]]
        assert ((smn > 0) & (compass < 0).any(axis=1)).any()
        assert ((smx < 0) & (compass > 0).any(axis=1)).any()
    if family == "random":
        assert len(v) == 100_000
        assert (got > 20).sum() > 5000 and (got <= 0).sum() > 5000 and ((got > 0) & (got <= 20)).sum() > 5000
        assert ((smn > 0) & (smn > -smx)).any() and ((smx < 0) & (-smx > smn)).any()
