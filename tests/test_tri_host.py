"""LocalMapping::CreateNewMapPoints without a GPU (include/orbx.h, "growing the map"): the CPU restatement (tests/cpp/tri_ref.cpp)
against a second, independently written numpy statement in f64 on the worlds the GPU test uses, the recovery of ground truth, hand-built
cases with their exact outputs, and the C ABI's symbols and refusals, which are decided before anything touches a device.

Point bound.  The two statements' kept 3D points differ by at most 1.52e-6 of the point's norm over the committed worlds (largest
component difference / |X|; the restatement's Jacobi and LAPACK's SVD sum in different orders, and the restatement rounds x3D to f32);
REL_BOUND is that times 4.  The normals differ by at most 1.1e-7 (absolute: they are unit-sized) and the two distances by at most
1.82e-6 of their value; the same factor 4 applies."""
import ctypes

import numpy as np
import pytest

import tri_ref_lib as L

REL_BOUND = 4 * 1.52e-6
NORMAL_BOUND = 4 * 1.1e-7
DIST_BOUND = 4 * 1.82e-6
LEFT_OUT_CAP = 0.01  # of a world's candidate pairs / matches

H = L.hand_desc
K2 = L.K_POW2


# ---- 1. two statements, the same worlds ----

@pytest.mark.parametrize("name", L.WORLDS + L.WORLDS_2)
def test_restatement_equals_numpy_statement(name):
    w = L.world(name)
    e = w.expected()
    first = L.search_numpy(w)
    assert len(first["borderline"]) <= LEFT_OUT_CAP * max(first["candidates"], 1), (len(first["borderline"]), first["candidates"])
    s = L.search_numpy(w, L.verdicts(w, first["borderline"])) if first["borderline"] else first
    m = e["match"]
    print(name, "restatement", m["res"], "numpy", s["res"], "left out", len(first["borderline"]), "of", first["candidates"])
    assert np.array_equal(m["matches12"][:w.kf1.n], s["matches12"])
    assert np.all(m["matches12"][w.kf1.n:] == -1)
    for f in L.MATCH_COUNTERS:
        assert int(m["res"][f]) == s["res"][f], f
    assert int(m["res"]["nmatches"]) == int((m["matches12"] >= 0).sum()) > 0
    F, ep, base = L.geometry_numpy(w)
    assert np.abs(m["res"]["F12"].reshape(3, 3) - F).max() <= 1e-5 * np.abs(F).max()
    assert abs(m["res"]["baseline"] - base) <= 1e-6 * base and abs(m["res"]["ex"] - ep[0]) <= 1e-4 * abs(ep[0])

    t = e["tri"]
    n = L.triangulate_numpy(w, m["matches12"][:w.kf1.n])
    followed = int((m["matches12"] >= 0).sum())
    print(name, "restatement", t["res"], "left out", len(n["borderline"]), "of", followed)
    assert len(n["borderline"]) <= LEFT_OUT_CAP * followed
    sure = n["outcome"] >= 0
    assert np.array_equal(t["outcome"][:w.kf1.n][sure], n["outcome"][sure])
    assert int(t["res"]["n_matches"]) == followed and int(t["res"]["status"]) == 0
    for code, field in L.OUTCOME_FIELD.items():
        assert int(t["res"][field]) == int((t["outcome"] == code).sum()), field
    assert np.array_equal(t["mask"], (t["outcome"] == L.KEPT).astype(np.uint8))
    kept = np.flatnonzero((t["outcome"][:w.kf1.n] == L.KEPT) & (n["outcome"] == L.KEPT))
    assert len(kept) > 0
    rel = np.abs(t["points"][kept] - n["points"][kept]).max(axis=1) / np.linalg.norm(n["points"][kept], axis=1)
    dn = np.abs(t["normal"][kept] - n["normal"][kept]).max()
    dd = (np.abs(t["dist"][kept] - n["dist"][kept]) / n["dist"][kept]).max()
    print(name, "points", rel.max(), "normals", dn, "distances", dd)
    assert rel.max() <= REL_BOUND and dn <= NORMAL_BOUND and dd <= DIST_BOUND
    off = t["outcome"] != L.KEPT  # every other entry: zeros
    assert not t["points"][off].any() and not t["normal"][off].any() and not t["dist"][off].any()


def test_noise_free_world_recovers_ground_truth(name="noise_free"):
    w = L.world(name)
    e = w.expected()
    m, t = e["match"]["matches12"], e["tri"]
    right = [i for i, (j, _) in w.truth.items() if m[i] == j and t["outcome"][i] == L.KEPT]
    assert len(right) >= 0.8 * len(w.truth)
    X = np.array([w.truth[i][1] for i in right])
    rel = np.abs(t["points"][right] - X).max(axis=1) / np.linalg.norm(X, axis=1)
    print("ground truth", rel.max(), "over", len(right))
    assert rel.max() <= REL_BOUND
    # and no wrong match survives both calls on exact projections
    assert all(m[i] == w.truth[i][0] for i in np.flatnonzero(t["outcome"][:w.kf1.n] == L.KEPT) if i in w.truth)


def test_noise_free_world_of_the_second_setting_recovers_ground_truth():
    test_noise_free_world_recovers_ground_truth("noise_free@2")


def test_worlds_reach_every_path():
    """More common nodes than the kernel has waves; a node of 65-130 KF2 features (the chunked path beyond one per lane); more than
    64 and more than 256 matches per pair; the epipole inside the image; every gate but the two no input reaches alone."""
    def common(w):
        return set(w.kf1.fv_node.tolist()) & set(w.kf2.fv_node.tolist())
    assert len(common(L.world("small_nodes"))) > 16
    big = L.world("big_node")
    sizes = np.bincount(np.unique(big.kf2.fv_node, return_inverse=True)[1])
    assert 65 <= sizes.max() <= 130 and big.kf2.fv_node[np.argmax(sizes)] in common(big)
    assert 64 < int(L.world("small_nodes").expected()["match"]["res"]["nmatches"]) <= 256
    assert int(L.world("dense").expected()["match"]["res"]["nmatches"]) > 256
    fw = L.world("forward").expected()
    assert 0 < fw["match"]["res"]["ex"] < L.WIDTH and 0 < fw["match"]["res"]["ey"] < L.HEIGHT and fw["tri"]["res"]["n_low_parallax"] > 0
    mixed = L.world("mixed").expected()
    assert mixed["tri"]["res"]["n_scale"] > 0 and mixed["match"]["res"]["n_epiline_rejected"] > 0
    assert L.world("masked").expected()["match"]["res"]["n_queries"] < L.world("masked").kf1.n * 0.8


# ---- 2. hand-built cases: KF1 at the origin, KF2 one unit ahead of it, no rotation; the epipole is (256, 256) in both images and
# the epipolar lines are the rays from it ----

C2 = (0.0, 0.0, 1.0)


def both(X, octave=0, angle=0.0, desc1=(), desc2=(), node=5, C=C2):
    """The two features of a 3D point: ((x, y, octave, angle, desc, node) in KF1, the same in KF2)."""
    (x1, y1), (x2, y2) = L.project(K2, (0, 0, 0), X), L.project(K2, C, X)
    return (x1, y1, octave, angle, H(desc1), node), (x2, y2, octave, angle, H(desc2), node)


def along(s):
    """Points on KF1's ray through (320, 256): they share KF1's pixel and lie on one epipolar line of KF2."""
    return (0.5 * s, 0.0, 4.0 * s)


def test_equal_distances_the_last_passing_candidate_wins():
    a, c1 = both(along(1.0), desc2=[0, 1, 2, 3])
    _, c0 = both(along(0.75), desc2=[4, 5, 6, 7])
    _, c2 = both(along(1.5), desc2=[8, 9, 10, 11])
    _, c3 = both(along(2.0), desc2=range(6))
    w = L.hand_world([a], [c0, c1, c2, c3])
    r = L.search(w)
    assert r["matches12"].tolist()[:1] == [2] and int(r["res"]["nmatches"]) == 1  # (c0, c1, c2 at distance 4: the last; c3 at 6)
    assert L.search_numpy(w)["matches12"].tolist() == [2]
    # ... and a later candidate that fails the line test does not win: the third one moved 3 px off the line
    off = (c2[0], c2[1] + 3.0) + c2[2:]
    assert L.search(L.hand_world([a], [c0, c1, off, c3]))["matches12"].tolist()[:1] == [1]


def test_a_feature_taken_by_an_earlier_one_of_the_node():
    a, j0 = both(along(1.0), desc2=[0, 1])
    b = a
    _, j1 = both(along(1.5), desc2=range(8))
    w = L.hand_world([a, b], [j0, j1])
    assert L.search(w)["matches12"].tolist()[:2] == [0, 1]  # (both prefer j0; the first takes it)
    assert L.search_numpy(w)["matches12"].tolist() == [0, 1]
    # in different nodes nobody sees j1 from a's node: b gets nothing there
    b2 = b[:5] + (6,)
    assert L.search(L.hand_world([a, b2], [j0, j1]))["matches12"].tolist()[:2] == [0, -1]


def test_both_masks():
    a, j0 = both(along(1.0), desc2=[0, 1])
    _, j1 = both(along(1.5), desc2=range(8))
    r = L.search(L.hand_world([a], [j0, j1], mask1=[1]))
    assert r["matches12"].tolist()[:1] == [-1] and int(r["res"]["n_queries"]) == 0  # (a already has a map point)
    r = L.search(L.hand_world([a], [j0, j1], mask2=[1, 0]))
    assert r["matches12"].tolist()[:1] == [1] and int(r["res"]["n_queries"]) == 1   # (j0 has one: the next best)
    assert L.search(L.hand_world([a], [j0, j1], mask1=[0], mask2=[0, 0]))["matches12"].tolist()[:1] == [0]


def test_epipole_exclusion_inside_the_image():
    """KF2 ahead of KF1: the epipole (256, 256) lies in the image, and a candidate within sqrt(100 * scale[octave]) px of it is skipped
    although it lies on the line."""
    a = (260.0, 256.0, 0, 0.0, H([]), 5)
    near = (261.0, 256.0, 0, 0.0, H([]), 5)          # 5 px from the epipole: 25 < 100
    far0 = (268.0, 256.0, 0, 0.0, H([0]), 5)         # 12 px at level 0: 144 >= 100
    far3 = (268.0, 256.0, 3, 0.0, H([]), 5)          # 12 px at level 3: 144 < 172.8
    r = L.search(L.hand_world([a], [near]))
    assert r["matches12"].tolist()[:1] == [-1] and int(r["res"]["n_epipole_rejected"]) == 1 and int(r["res"]["n_with_candidates"]) == 1
    assert (float(r["res"]["ex"]), float(r["res"]["ey"])) == (256.0, 256.0)
    r = L.search(L.hand_world([a], [near, far3, far0]))
    assert r["matches12"].tolist()[:1] == [2] and int(r["res"]["n_epipole_rejected"]) == 2 and int(r["res"]["n_epiline_rejected"]) == 0


def test_epipolar_line_threshold_per_octave():
    """2.5 px off the line: 6.25 >= 3.84 * 1 at level 0, 6.25 < 3.84 * 2.0736 at level 2."""
    a, on = both(along(1.0))
    for octave, accepted in ((0, False), (1, True), (2, True)):
        cand = (on[0], on[1] + (2.5 if octave != 1 else 2.3), octave) + on[3:]  # (level 1: 5.29 < 3.84 * 1.44 = 5.53)
        r = L.search(L.hand_world([a], [cand]))
        assert (r["matches12"][0] == 0) == accepted and int(r["res"]["n_epiline_rejected"]) == (0 if accepted else 1), octave


def test_a_feature_on_the_epipole_has_no_line():
    """x1 on KF1's epipole: a = b = 0 exactly (cx, cy are powers of two), den == 0, every candidate is rejected."""
    a = (256.0, 256.0, 0, 0.0, H([]), 5)
    _, c = both(along(1.0))
    w = L.hand_world([a], [c, c])
    r = L.search(w)
    F = r["res"]["F12"]
    assert np.float32(np.float32(256.0 * F[0]) + np.float32(256.0 * F[3])) + F[6] == 0 and np.float32(np.float32(256.0 * F[1]) + np.float32(256.0 * F[4])) + F[7] == 0
    assert r["matches12"].tolist()[:1] == [-1] and int(r["res"]["n_epiline_rejected"]) == 2 and int(r["res"]["n_with_candidates"]) == 1


def test_rotation_bins_remove_the_outliers():
    f1, f2 = [], []
    for k in range(14):
        a, b = both((0.3 + 0.05 * k, 0.2, 4.0), node=10 + k, angle=100.0)
        turn = 88.0 if k < 12 else (280.0 if k == 12 else 10.0)  # twelve at 12 degrees (bin 1), one at 180 (bin 15), one at 90 (bin 8)
        f1.append(a)
        f2.append(b[:3] + (turn,) + b[4:])
    w = L.hand_world(f1, f2, ori=True)
    r = L.search(w)
    assert r["matches12"].tolist()[:14] == list(range(12)) + [-1, -1] and int(r["res"]["n_rot_removed"]) == 2 and int(r["res"]["nmatches"]) == 12
    assert L.search_numpy(w)["matches12"].tolist() == r["matches12"].tolist()[:14]
    w.ori = False
    assert L.search(w)["matches12"].tolist()[:14] == list(range(14))


def one_match(f1, f2, C=C2):
    w = L.hand_world([f1], [f2], centre2=C)
    t = L.triangulate(w, np.array([0], np.int32))
    return t, {f: int(t["res"][f]) for f in L.TRI_FIELDS}


def only(res, field):
    want = dict.fromkeys(L.TRI_FIELDS, 0)
    want["n_matches"] = 1
    want[field] = 1
    return res == want


def test_every_triangulation_gate_on_its_own():
    """One world per counter.  n_w_zero and n_zero_dist are reached by no pair of keyframes, up to rounding: x3D[3] == 0 needs
    parallel rays, which the parallax gate takes first, and a point at a camera centre has a depth of 0 up to the rounding of
    R.row(2) . Ow + tz, which the depth gates take first; they are asserted zero on every world here, and
    test_the_two_gates_no_keyframe_pair_reaches calls the function with inputs that do reach them."""
    X = (0.5, 0.0, 4.0)
    a, b = both(X)
    t, r = one_match(a, b)
    assert only(r, "n_points") and t["mask"].tolist() == [1]
    assert np.abs(t["points"][0] - np.array(X)).max() <= REL_BOUND * np.linalg.norm(X)
    d1, d2 = np.linalg.norm(X), np.linalg.norm(np.array(X) - np.array(C2))
    want_n = (np.array(X) / d1 + (np.array(X) - np.array(C2)) / d2) / 2
    assert np.abs(t["normal"][0] - want_n).max() <= NORMAL_BOUND
    s = L.scale_table()
    assert abs(t["dist"][0, 1] - d1) <= DIST_BOUND * d1 and abs(t["dist"][0, 0] - d1 / s[-1]) <= DIST_BOUND * d1 / s[-1]
    # a point at level 3 carries that level's scale in its distances
    t3, r3 = one_match(*both(X, octave=3))
    assert only(r3, "n_points") and abs(t3["dist"][0, 1] - d1 * s[3]) <= DIST_BOUND * d1 * s[3]

    _, r = one_match(*both((0.05, 0.0, 60.0)))
    assert only(r, "n_low_parallax")
    # sideways, the second ray turned away from the first: they meet behind both cameras
    side = (1.0, 0.0, 0.0)
    a = (256.0, 256.0, 0, 0.0, H([]), 5)
    b = (256.0 + 51.2, 256.0, 0, 0.0, H([]), 5)
    _, r = one_match(a, b, C=side)
    assert only(r, "n_behind_1")
    # a point between the two cameras: in front of KF1, behind KF2
    _, r = one_match(*both((0.1, 0.0, 0.5)))
    assert only(r, "n_behind_2")
    a, b = both(X)
    _, r = one_match((a[0], a[1] + 8.0) + a[2:], b)
    assert only(r, "n_reproj_1")
    a, b = both(X, octave=0)
    a7 = a[:2] + (7,) + a[3:]
    t, r = one_match(a7, (b[0], b[1] + 8.0) + b[2:])
    assert only(r, "n_reproj_2")  # (level 7 forgives KF1 its share of the 8 px, level 0 does not forgive KF2 its own)
    a, b = both(X)
    _, r = one_match(a, b[:2] + (7,) + b[3:])
    assert only(r, "n_scale")  # (the same distance seen at levels 0 and 7)
    _, r = one_match(a[:2] + (7,) + a[3:], b)
    assert only(r, "n_scale")


def test_the_two_gates_no_keyframe_pair_reaches():
    """triangulate() called on its own (the camera centres are its arguments).  A translation that is no number passes the parallax
    gate -- the rays come from the rotations alone -- and gives an x3D that is no number: the n_w_zero return.  A camera centre
    handed in as exactly the point the same call triangulated gives dist1 == 0 (then dist2 == 0): the n_zero_dist return."""
    X = (0.5, 0.0, 4.0)
    a, b = both(X)
    p1, p2 = L.pose12(np.eye(3), (0, 0, 0)), L.pose12(np.eye(3), C2)
    o, P = L.triangulate_one(p1, p2, (0, 0, 0), C2, K2, a[:2], b[:2])
    assert o == L.KEPT and np.abs(P - np.array(X)).max() <= REL_BOUND * np.linalg.norm(X)
    for k in (9, 11):
        for v in (np.inf, np.nan):
            broken = p2.copy()
            broken[k] = v
            assert L.triangulate_one(p1, broken, (0, 0, 0), C2, K2, a[:2], b[:2])[0] == L.W_ZERO
    assert L.triangulate_one(p1, p2, P, C2, K2, a[:2], b[:2])[0] == L.ZERO_DIST
    assert L.triangulate_one(p1, p2, (0, 0, 0), P, K2, a[:2], b[:2])[0] == L.ZERO_DIST
    # (the gates in front of them still come first)
    assert L.triangulate_one(p1, p2, P, C2, K2, a[:2], (b[0], b[1] + 8.0))[0] == L.REPROJ_1


def test_median_depth_gate_and_the_refused_pairs():
    a, b = both(along(1.0))
    w = L.hand_world([a], [b], median=50.0)  # baseline 1: 0.02
    assert L.search(w)["matches12"][0] == 0
    w = L.hand_world([a], [b], median=200.0)  # 0.005 < 0.01
    r = L.search(w, cap=4)
    assert int(r["res"]["status"]) == L.LOW_BASELINE and np.all(r["matches12"] == -1) and float(r["res"]["baseline"]) == 1.0
    assert int(r["res"]["n_queries"]) == 0
    # a median that is no positive finite number is garbage: flagged, and the pair is matched without the gate
    for bad in (0.0, -3.0, np.nan, np.inf):
        r = L.search(L.hand_world([a], [b], median=bad))
        assert int(r["res"]["status"]) == L.BAD_INPUT and r["matches12"][0] == 0, bad
    # a keyframe with itself
    w = L.hand_world([a], [a], centre2=(0, 0, 0))
    r = L.search(w)
    assert int(r["res"]["status"]) == L.ZERO_BASELINE and np.all(r["matches12"] == -1)
    assert not r["res"]["F12"].any() and float(r["res"]["ex"]) == 0 and float(r["res"]["baseline"]) == 0
    t = L.triangulate(w, np.array([0], np.int32))
    assert int(t["res"]["n_low_parallax"]) == 1 and int(t["res"]["n_points"]) == 0 and np.isfinite(t["points"]).all()


def test_garbage_is_flagged_and_not_followed():
    a, b = both(along(1.0))
    w = L.hand_world([a], [b])
    bad = L.World(L.KeyFrame(w.kf1.kps, w.kf1.desc, w.kf1.fv_node, w.kf1.fv_feat, np.r_[w.kf1.pose[:11], np.nan]), w.kf2, w.K, ori=False)
    r = L.search(bad)
    assert int(r["res"]["status"]) == L.NONFINITE and np.all(r["matches12"] == -1)
    t = L.triangulate(bad, np.array([0], np.int32))
    assert int(t["res"]["status"]) == L.NONFINITE and int(t["res"]["n_matches"]) == 0 and not t["mask"].any()
    # counts beyond the capacity are clamped and flagged
    r = L.search(w, cap=1, n1=5, fvn2=-2)
    assert int(r["res"]["status"]) == L.BAD_INPUT
    # an octave outside the pyramid, a FeatureVector entry that names no feature
    b9 = b[:2] + (9,) + b[3:]
    r = L.search(L.hand_world([a], [b9]))
    assert int(r["res"]["status"]) == L.BAD_INPUT and r["matches12"][0] == -1
    t = L.triangulate(L.hand_world([a], [b9]), np.array([0], np.int32))
    assert int(t["res"]["status"]) == L.BAD_INPUT and int(t["res"]["n_matches"]) == 0
    t = L.triangulate(w, np.array([3], np.int32))
    assert int(t["res"]["status"]) == L.BAD_INPUT and int(t["res"]["n_matches"]) == 0
    kf2 = L.KeyFrame(w.kf2.kps, w.kf2.desc, [5, 5], [0, 7], w.kf2.pose)
    r = L.search(L.World(w.kf1, kf2, w.K, ori=False), cap=8)
    assert int(r["res"]["status"]) == 0 and r["matches12"][0] == 0


# ---- 3. the C ABI ----

NEW_SYMBOLS = ("orbx_match_triangulation_batch_device", "orbx_match_triangulation", "orbx_triangulate_matches_batch_device",
               "orbx_triangulate_matches")


def test_tri_symbols_exported_and_bound(orbx):
    lib = ctypes.CDLL(orbx.lib_path())
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
    for m in ("match_triangulation_pairs_device", "triangulate_matches_pairs_device", "create_new_map_points_pairs_device",
              "match_triangulation", "triangulate_matches"):
        assert hasattr(orbx.ORBextractor, m), m
    assert hasattr(orbx.ORBmatcher, "SearchForTriangulation")
    assert orbx.TRI_MATCH_RESULT_DTYPE.itemsize == L.MATCH_RESULT_DTYPE.itemsize == 76 and orbx.TRI_MATCH_RESULT_DTYPE.names == L.MATCH_RESULT_DTYPE.names
    assert orbx.TRI_RESULT_DTYPE.itemsize == 44 and orbx.TRI_RESULT_DTYPE.names == L.TRI_FIELDS
    assert (orbx.TRI_BAD_INPUT, orbx.TRI_NONFINITE, orbx.TRI_LOW_BASELINE, orbx.TRI_ZERO_BASELINE) == (L.BAD_INPUT, L.NONFINITE, L.LOW_BASELINE,
                                                                                                     L.ZERO_BASELINE)


def test_tri_refusals_without_a_context(orbx):
    """Null required pointers, negative counts, capacity < 1, a pair index outside [0, n_frames) and a K that is no camera are
    ORBX_E_BADARG, a capacity above ORBX_BOW_MAX_FEATURES is ORBX_E_CAPACITY, and ctx == NULL with otherwise well-formed arguments
    is ORBX_E_HIP: all of it is decided before a device is touched (there is none here)."""
    lib = orbx.lib()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    k1, k2 = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    neg, beyond = np.array([0, -1], np.int32), np.array([2, 0], np.int32)  # (named: they must outlive the calls)
    K, Knan, Kflat = L.K_DEFAULT.copy(), L.K_DEFAULT.copy(), L.K_DEFAULT.copy()
    Knan[2], Kflat[4] = np.nan, 0.0
    buf = np.zeros(64, np.uint8)  # stands for every device array (never dereferenced)
    d = p(buf)

    def match(n_frames=2, n_pairs=2, h1=p(k1), h2=p(k2), kps=d, desc=d, n=d, cap=8, node=d, feat=d, fvn=d, mask=None, pose=d, Kp=p(K),
              med=None, out=d, res=d):
        return lib.orbx_match_triangulation_batch_device(None, n_frames, n_pairs, h1, h2, kps, desc, n, cap, node, feat, fvn, mask, pose,
                                                         Kp, med, 1, out, res)

    def tri(n_frames=2, n_pairs=2, h1=p(k1), h2=p(k2), kps=d, n=d, cap=8, pose=d, Kp=p(K), m12=d, pts=d, msk=d, nrm=d, dst=d, res=d):
        return lib.orbx_triangulate_matches_batch_device(None, n_frames, n_pairs, h1, h2, kps, n, cap, pose, Kp, m12, pts, msk, nrm, dst,
                                                         res)
    common = (dict(n_frames=-1), dict(n_pairs=-1), dict(cap=0), dict(cap=-3), dict(h1=None), dict(h2=None), dict(kps=None), dict(n=None),
              dict(pose=None), dict(Kp=None), dict(res=None), dict(n_frames=1), dict(h1=p(neg)), dict(h2=p(beyond)), dict(Kp=p(Knan)),
              dict(Kp=p(Kflat)))
    for call, own in ((match, (dict(desc=None), dict(node=None), dict(feat=None), dict(fvn=None), dict(out=None))),
                      (tri, (dict(m12=None), dict(pts=None), dict(msk=None), dict(nrm=None), dict(dst=None)))):
        assert call() == orbx.E_HIP
        assert call(n_pairs=0, h1=None, h2=None) == orbx.E_HIP  # (ORBX_OK with a context)
        for bad in common + own:
            assert call(**bad) == orbx.E_BADARG, (call.__name__, bad)
        assert call(cap=orbx.BOW_MAX_FEATURES + 1) == orbx.E_CAPACITY
        assert call(cap=orbx.BOW_MAX_FEATURES) == orbx.E_HIP
    assert match(mask=d, med=d) == orbx.E_HIP

    kp = np.zeros(4, orbx.KEYPOINT_DTYPE)
    desc, node, feat = np.zeros((4, 32), np.uint8), np.zeros(4, np.uint32), np.arange(4, dtype=np.uint32)
    pose = np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32)
    out, mres, tres = np.zeros(4, np.int32), orbx.TriMatchResult(), orbx.TriResult()

    def host(n1=4, fv1=4, n2=4, fv2=4, feat1=feat, feat2=feat, kp1=p(kp), o=p(out), res=ctypes.byref(mres), ps=p(pose), Kp=p(K)):
        return lib.orbx_match_triangulation(None, kp1, p(desc), n1, p(node), p(feat1), fv1, None, ps, p(kp), p(desc), n2, p(node), p(feat2),
                                            fv2, None, p(pose), Kp, 0.0, 1, o, res)
    assert host() == orbx.E_HIP
    for bad in (dict(n1=-1), dict(n2=-1), dict(fv1=-1), dict(fv2=-1), dict(kp1=None), dict(o=None), dict(res=None), dict(ps=None),
                dict(Kp=None), dict(Kp=p(Knan)), dict(feat1=np.array([0, 1, 2, 4], np.uint32)),
                dict(feat2=np.array([0, 1, 2, 3], np.uint32), n2=3)):
        assert host(**bad) == orbx.E_BADARG, bad
    assert host(n1=orbx.BOW_MAX_FEATURES + 1) == orbx.E_CAPACITY

    pts, msk, nrm, dst = np.zeros((4, 3), np.float32), np.zeros(4, np.uint8), np.zeros((4, 3), np.float32), np.zeros((4, 2), np.float32)

    def host_tri(n1=4, n2=4, kp1=p(kp), m=p(out), P=p(pts), res=ctypes.byref(tres), ps=p(pose), Kp=p(K)):
        return lib.orbx_triangulate_matches(None, kp1, n1, ps, p(kp), n2, p(pose), Kp, m, P, p(msk), p(nrm), p(dst), res)
    assert host_tri() == orbx.E_HIP
    for bad in (dict(n1=-1), dict(n2=-1), dict(kp1=None), dict(m=None), dict(P=None), dict(res=None), dict(ps=None), dict(Kp=p(Kflat))):
        assert host_tri(**bad) == orbx.E_BADARG, bad
    assert host_tri(n1=orbx.BOW_MAX_FEATURES + 1) == orbx.E_CAPACITY


def test_search_for_triangulation_needs_compute_bow(orbx):
    fr = orbx.Frame.from_arrays(np.zeros(3, orbx.KEYPOINT_DTYPE), np.zeros((3, 32), np.uint8), (0, 640, 0, 480))
    with pytest.raises(orbx.OrbxError, match="ComputeBoW"):
        orbx.ORBmatcher(0.6, True, extractor=object()).SearchForTriangulation(fr, fr, np.eye(4), np.eye(4), K=np.eye(3))
