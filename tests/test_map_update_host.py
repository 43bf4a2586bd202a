"""The CPU restatement of the map-point update behind the local bundle adjustment (tests/cpp/map_update_ref.cpp over
csrc/orbx_map_math.inc; include/orbx.h, "local mapping: updating the map points") against what does not share its code: an
independently written numpy statement, BIT FOR BIT in every output (every operation is an IEEE basic operation in a fixed order:
there is no tolerance); rule worlds that report the counter they aim at; CreateNewMapPoints' restatement on a pair both can run;
and a stand-alone program under the sanitizers.  tests/test_gpu_map_update.py then holds the device to the restatement."""
import subprocess

import numpy as np
import pytest

import map_update_ref_lib as U

NAMED = ("window", "clean", "all_free", "all_erased", "second")
RULES = sorted(U.RULE_AIMS)


def kw_of(name):
    return dict(scale=U.scale_table(U.NLEVELS_2, U.SCALE_FACTOR_2), nlevels=U.NLEVELS_2) if name == "second" else {}


def agree(w, **kw):
    a, b = U.update(w, **kw), U.update_numpy(w, **kw)
    assert U.same(a, b) == [], (U.same(a, b), a["res"], b["res"])
    return a


@pytest.mark.parametrize("name", NAMED)
@pytest.mark.parametrize("what", [0, 1, 2, 3])
def test_the_two_statements_agree_on_the_named_worlds(name, what):
    """... and `what` writes only what it names: the other arrays keep the fill."""
    w = U.world(name)
    a = agree(w, what=what, **kw_of(name))
    blank = U.blank_outputs(w)
    assert a["res"]["status"] == 0 and a["res"]["n_points"] > 20 and a["res"]["n_free"] == w.n_free
    live = a["res"]["n_observations"] > 0  # (all_erased: every vertex is bad, and for a bad one nothing of these is written)
    assert (a["normals"].tobytes() != blank["normals"].tobytes()) == (live and bool(what & U.NORMALS))
    assert (a["dist"].tobytes() != blank["dist"].tobytes()) == (live and bool(what & U.NORMALS))
    assert (a["desc"].tobytes() != blank["desc"].tobytes()) == (live and bool(what & U.DESCRIPTORS))
    assert a["obs"].tobytes() != blank["obs"].tobytes()
    full = U.update(w, what=3, **kw_of(name))
    for k in ("rows", "mask_out", "ref", "obs"):  # (what `what` does not govern does not depend on it)
        assert (a[k] is None and full[k] is None) or a[k].tobytes() == full[k].tobytes(), k


def test_the_named_worlds_do_what_they_are_for():
    r = {n: U.update(U.world(n), **kw_of(n))["res"] for n in NAMED}
    assert r["window"]["n_erased"] > 10 and r["window"]["n_bad_points"] > 0 and r["window"]["n_cleared"] > 0 and r["window"]["n_ref_moved"] > 0
    assert r["window"]["max_observers"] >= 4 and r["window"]["n_observations"] > 200
    assert r["clean"]["n_erased"] == 0 and r["clean"]["n_bad_points"] == 0 and r["clean"]["n_ref_moved"] == 0
    assert r["all_free"]["n_free"] == U.world("all_free").n_entries and r["all_free"]["n_bad_points"] > 0
    assert r["all_erased"]["n_bad_points"] == r["all_erased"]["n_points"] > 0 and r["all_erased"]["n_observations"] == 0
    assert r["second"]["n_points"] > 50


def test_not_in_place_leaves_the_mask_output_of_other_points_alone():
    w = U.world("window")
    a = agree(w, in_place=False)
    touched = a["mask_out"] != U.FILL
    assert touched.sum() == a["res"]["n_points"] and not touched[w.map_n:].any()


@pytest.mark.parametrize("key", RULES)
def test_rule_worlds_hit_their_aim_and_agree(key):
    w = U.rule_worlds()[key]
    a = agree(w)
    assert a["res"]["status"] == 0
    for f, v in U.RULE_AIMS[key].items():
        assert a["res"][f] == v, (key, f, a["res"])


def test_rule_worlds_in_detail():
    """What the counters alone do not say."""
    rw = U.rule_worlds()
    out = {k: U.update(w) for k, w in rw.items()}
    blank = U.blank_outputs(rw["obs3"])
    # N = 1 .. 5: the median index is 0, 0, 1, 1, 2; the pick is the numpy statement's, and point 0's count is N
    for n, idx in zip((1, 2, 3, 4, 5), (0, 0, 1, 1, 2)):
        w, o = rw["obs%d" % n], out["obs%d" % n]
        D = w.desc[:n, 0]
        dist = np.unpackbits(D[:, None] ^ D[None], axis=2).sum(axis=2)
        med = np.sort(dist, axis=1)[:, idx]
        assert (n - 1) // 2 == idx and o["obs"][0] == n and o["desc"][0].tobytes() == D[int(np.argmin(med))].tobytes(), n
        if n <= 2:  # (every median is the diagonal's zero: the first observer's descriptor)
            assert o["desc"][0].tobytes() == D[0].tobytes()
        assert o["obs"][1] == 1 and o["desc"][1].tobytes() == w.desc[n - 1, 1].tobytes()
        # the mean of unit vectors at most 0.25 rad apart (a baseline of 1.2 at depth 5) is at least cos(0.125) long
        assert np.cos(0.125) <= np.linalg.norm(o["normals"][0].astype(np.float64)) <= 1 + 1e-6
        assert 0 < o["dist"][0, 0] < o["dist"][0, 1]
    # equal medians: the first wins
    assert out["tie"]["desc"][0].tobytes() == rw["tie"].desc[0, 0].tobytes()
    # fixed entries only: nothing at all is touched
    assert U.same(out["fixed_only"], dict(U.blank_outputs(rw["fixed_only"]), res=out["fixed_only"]["res"])) == []
    # an outlier byte on a non-vertex or on nothing: the rows stay, point 1 is untouched
    o = out["outlier_elsewhere"]
    assert o["rows"].tobytes() == rw["outlier_elsewhere"].rows.tobytes() and o["obs"][1] == blank["obs"][1] and o["obs"][0] == 3
    # 3 -> 2: bad; every row entry cleared, the mask byte 0, the count 0, nothing else written; point 1 lives on
    o = out["three_to_two"]
    assert (o["rows"][:, 0] == -1).all() and o["mask_out"][0] == 0 and o["obs"][0] == 0 and o["ref"][0] == -1
    assert o["normals"][0].tobytes() == blank["normals"][0].tobytes() and o["desc"][0].tobytes() == blank["desc"][0].tobytes()
    assert o["mask_out"][1] == 1 and o["obs"][1] == 1 and o["rows"][2, 1] == 1
    # 4 -> 3: good; only the erased entry goes
    o = out["four_to_three"]
    assert list(o["rows"][:, 0]) == [-1, 0, 0, 0] and o["mask_out"][0] == 1 and o["obs"][0] == 3 and o["ref"][0] == 1
    # the reference keyframe
    assert list(out["ref_erased"]["rows"][:, 0]) == [0, -1, 0, 0] and out["ref_erased"]["ref"][0] == 0
    assert out["ref_kept"]["ref"][0] == 2 and out["ref_gone"]["ref"][0] == 0 and out["ref_negative"]["ref"][0] == 0
    assert out["ref_null"]["ref"] is None
    # ... decides the distances: the same world under another reference
    a, b = rw["ref_kept"].copy(), rw["ref_kept"].copy()
    a.kps["octave"][:, 0], b.kps["octave"][:, 0] = (0, 1, 2), (0, 1, 2)
    b.map_ref[0] = 0
    oa, ob = U.update(a), U.update(b)
    assert oa["normals"].tobytes() == ob["normals"].tobytes() and oa["dist"][0, 1] > ob["dist"][0, 1]


@pytest.mark.parametrize("what", sorted(U.GARBAGE))
def test_garbage_leaves_every_byte_as_it_was(what):
    base = U.world("window")
    w = U.garbage(base, what)
    a = agree(w)
    assert a["res"]["status"] == U.GARBAGE[what], (what, a["res"])
    assert all(a["res"][f] == 0 for f in U.COUNTERS[1:]) and not a["res"]["reserved"].any()
    assert U.same(a, dict(U.blank_outputs(w), res=a["res"])) == []
    assert U.update(base)["res"]["status"] == 0


def test_the_chain_property_on_the_cpu():
    """CreateNewMapPoints' restatement for a pair, fed in as a two-entry problem with rows built from matches12 and KF1 as the
    reference keyframe: the normals and distances are the bits its rule 6 wrote, the descriptors KF1's."""
    import tri_ref_lib as TL
    tw = TL.make_world(5)
    a, b = tw.kf1, tw.kf2
    cap = max(a.n, b.n)
    t = TL.triangulate(tw, TL.search(tw, cap=cap)["matches12"], cap=cap)
    m12, made = TL.search(tw, cap=cap)["matches12"], t["mask"][:a.n] != 0
    assert made.sum() > 100
    kps, desc = np.zeros((2, cap), U.KEYPOINT_DTYPE), np.zeros((2, cap, 32), np.uint8)
    kps[0, :a.n], kps[1, :b.n], desc[0, :a.n], desc[1, :b.n] = a.kps, b.kps, a.desc, b.desc
    rows = np.full((2, cap), -1, np.int32)
    idx = np.flatnonzero(made)
    rows[0, idx], rows[1, m12[idx]] = idx, idx
    w = U.World(kps, desc, np.array([a.n, b.n], np.int32), np.stack([a.pose, b.pose]).astype(np.float32), rows, None,
                t["points"][:cap].copy(), t["mask"][:cap].copy(), np.zeros(cap, np.int32), a.n, 2)
    o = agree(w, scale=U.scale_table(tw.nlevels, tw.scale_factor), nlevels=tw.nlevels)
    assert o["res"]["status"] == 0 and o["res"]["n_points"] == made.sum() and o["res"]["max_observers"] == 2
    assert o["normals"][idx].tobytes() == t["normal"][idx].tobytes() and o["dist"][idx].tobytes() == t["dist"][idx].tobytes()
    assert o["desc"][idx].tobytes() == a.desc[idx].tobytes() and (o["obs"][idx] == 2).all() and (o["ref"][idx] == 0).all()


def test_sanitized_stand_alone_program():
    """tests/cpp/map_update_ref_main.cpp: the restatement over small windows, every `what`, every optional array left out and
    every garbage case under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own (nothing sanitised is
    loaded into Python)."""
    exe = U.build(flags=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), exe_main=U.MAIN_SRC)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and " 0 failures" in p.stdout, p.stdout[-4000:]
