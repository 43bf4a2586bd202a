"""Sim3Solver on the device (orbx_sim3_solve / orbx_sim3_solve_batch_device) equals the CPU restatement tests/cpp/sim3_ref.cpp BYTE
FOR BYTE: every field of orbx_sim3_result, d_sim3, the row of inlier matches and every flag byte.  Both sides share the
arithmetic and contract nothing (include/orbx.h).  What the restatement itself is worth is tests/test_sim3_host.py's business."""
import numpy as np
import pytest

import sim3_ref_lib as S
from test_sim3_host import GARBAGE, _worlds, bad

pytestmark = pytest.mark.gpu

# correspondences per problem: none, below Horn's three, bNoMore (3, 19), one iteration (20), the first N that iterates freely
# (21), a wave's edge in the constructor's compaction (63, 64, 65) and several waves (200)
COUNTS = (0, 2, 3, 19, 20, 21, 63, 64, 65, 200)
CAP = 256


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, S.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sized():
    """A world per count of COUNTS; from 21 correspondences on with half a sigma of noise and a fifth gross mismatches."""
    return {n: (S.make_world(n, 400 + k, cap=CAP, outliers=(n // 5 if n >= 21 else 0), noise=0.5 if n >= 21 else 0.0),
                S.make_draws(35, 400 + k)) for k, n in enumerate(COUNTS)}


def padded(w, cap):
    """The same problem in rows of a larger capacity."""
    def grow(a, fill=0):
        if a is None:
            return None
        out = np.zeros(cap, a.dtype) if a.dtype == S.KEYPOINT_DTYPE else np.full((cap,) + a.shape[1:], fill, a.dtype)
        out[:len(a)] = a
        return out
    m1, m2 = w.mask1, w.mask2
    if m1 is None and cap > w.cap:  # (entries beyond the old capacity are no points)
        m1, m2 = np.ones(w.cap, np.uint8), np.ones(w.cap, np.uint8)
    return S.World(grow(w.kps1), w.n1, grow(w.kps2), w.n2, grow(w.match, -1), grow(w.points1), grow(m1), grow(w.points2), grow(m2),
                   w.pose1.copy(), w.pose2.copy(), w.K, w.truth)


def run_batch(orbx, ext, worlds, draws, frames=None, lists=None, sigma2=None, want_flags=True, **params):
    """The worlds as one device batch -> (results [P], sims [P, 13], rows [P, cap], flags [P, cap] or None).  By default problem
    p has keyframes and point sets 2 p and 2 p + 1 of its own; frames: a list of (kps, n, points, mask, pose) rows -- keyframe k
    and point set k -- and lists = (kf1, kf2, set1, set2) name them.  draws [P, n_iter, 3]."""
    import torch
    Pn, cap = len(worlds), worlds[0].cap
    if frames is None:
        frames = [f for w in worlds for f in ((w.kps1, w.n1, w.points1, w.mask1, w.pose1), (w.kps2, w.n2, w.points2, w.mask2, w.pose2))]
        even = np.arange(0, 2 * Pn, 2, dtype=np.int32)
        lists = (even, even + 1, even, even + 1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_k, d_n = d(np.stack([f[0] for f in frames])), d(np.array([f[1] for f in frames], np.int32))
    d_p, d_pose = d(np.stack([f[2] for f in frames])), d(np.stack([f[4] for f in frames]))
    masked = any(f[3] is not None for f in frames)
    assert not masked or all(f[3] is not None for f in frames)
    d_mask = d(np.stack([f[3] for f in frames])) if masked else None
    d_m = d(np.stack([w.match for w in worlds]))
    draws = np.ascontiguousarray(draws, np.int32)
    assert draws.shape[0] == Pn and draws.shape[2] == 3
    d_draws = d(draws)
    fill = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_res, d_sim, d_row = fill(Pn * orbx.SIM3_RESULT_DTYPE.itemsize), fill(Pn * 52), fill(Pn * cap * 4)
    d_fl = fill(Pn * cap) if want_flags else None
    ext.sim3_solve_batch_device(len(frames), lists[0], lists[1], lists[2], lists[3], d_k, d_n, d_m, len(frames), d_p, d_mask, d_pose,
                                worlds[0].K, d_draws, d_res, d_sim, d_row, d_fl, sigma2=sigma2, n_iter=draws.shape[1], capacity=cap,
                                **params)
    torch.cuda.synchronize()
    return (d_res.cpu().numpy().view(orbx.SIM3_RESULT_DTYPE), d_sim.cpu().numpy().view(np.float32).reshape(Pn, 13),
            d_row.cpu().numpy().view(np.int32).reshape(Pn, cap), d_fl.cpu().numpy().reshape(Pn, cap) if want_flags else None)


def same(got, ref, what=""):
    """Byte for byte: the record field by field (so that a difference names its field), the similarity, the row, the flags."""
    res, sim, row, flags = got
    r, rsim, rrow, rflags = ref
    for f in S.SIM3_RESULT_DTYPE.names:
        assert np.asarray(res[f]).tobytes() == np.asarray(r[f]).tobytes(), (what, f, res[f], r[f])
    assert sim.tobytes() == rsim.tobytes(), what
    assert row.tobytes() == rrow.tobytes(), what
    if flags is not None:
        assert flags.tobytes() == rflags.tobytes(), what


def check(orbx, ext, pairs, sigma2=None, **kw):
    """pairs: (world, draws) per problem, draws of one length; the parameters are the batch's."""
    worlds, draws = [w for w, _ in pairs], np.stack([d for _, d in pairs])
    ref_kw = {k: v for k, v in kw.items() if k in S.PARAMS}
    res, sim, row, flags = run_batch(orbx, ext, worlds, draws, sigma2=sigma2, **kw)
    for p, (w, d) in enumerate(pairs):
        same((res[p], sim[p], row[p], None if flags is None else flags[p]), S.solve(w, d, 0, sigma2=sigma2, **ref_kw), "problem %d" % p)
    return res


@pytest.mark.parametrize("n", COUNTS)
def test_one_problem_of_each_size(orbx, ext, sized, n):
    res = check(orbx, ext, [sized[n]])
    assert res[0]["n_correspondences"] == n
    if n < 20:
        assert res[0]["status"] == S.FEW_POINTS | S.NO_RESULT and res[0]["its_run"] == 0
    else:
        assert res[0]["max_its"] == S.ransac_entry(n) == {20: 1, 21: 3, 63: 142, 64: 149, 65: 156, 200: 300}[n]
    if n >= 63:
        assert res[0]["status"] == 0 and res[0]["found_it"] >= 0 and res[0]["n_inliers"] > 20


def test_all_sizes_in_one_batch(orbx, ext, sized):
    res = check(orbx, ext, [sized[n] for n in COUNTS])
    assert list(res["n_correspondences"]) == list(COUNTS)


@pytest.mark.parametrize("n_iter", [1, 35, 64, 65, 300])
def test_partial_and_full_waves_of_hypotheses(orbx, ext, n_iter):
    """Four fifths gross mismatches, 24 clean correspondences: a clean triple is rare (one in 125), so late iterations decide --
    with all 300 draws the restatement ends these three at iteration 52, at 68 and never (its best is then the last of many
    hypotheses with three inliers, the triple itself)."""
    pairs = [(S.make_world(120, 500 + k, cap=CAP, outliers=96, noise=0.1), S.make_draws(n_iter, 500 + k)) for k in (1, 4, 7)]
    res = check(orbx, ext, pairs)
    assert (res["max_its"] == 300).all() and (res["its_run"] <= n_iter).all()
    if n_iter == 300:
        assert list(res["found_it"]) == [52, 68, -1] and list(res["its_run"]) == [53, 69, 300] and res["best_it"][2] > 65
        one = check(orbx, ext, pairs[:1])  # one problem: the grid's last wave is partial in another place
        assert one[0].tobytes() == res[0].tobytes()


def test_found_at_the_first_in_the_middle_at_the_last_iteration_and_never(orbx, ext):
    w = S.make_world(200, 1, cap=CAP, outliers=40, noise=0.5)
    pool = S.make_draws(300, 1)
    _, counts, flags, _ = S.hypotheses(w, pool)
    good, poor = pool[(counts > 20) & (flags == 0)], pool[(counts <= 20) & (flags == 0)]
    assert len(good) >= 1 and len(poor) >= 34
    at = lambda k: np.concatenate([poor[:k], good[:1], poor[k:34]])  # noqa: E731
    res = check(orbx, ext, [(w, at(0)), (w, at(17)), (w, at(34)), (w, poor[:35])])
    assert list(res["found_it"]) == [0, 17, 34, -1] and list(res["its_run"]) == [1, 18, 35, 35]
    assert list(res["status"]) == [0, 0, 0, S.NO_RESULT]


def test_each_branch_world(orbx, ext, ext2):
    """The host test's worlds (degenerate triples, the last of equals, fix_scale, no mask ...), grouped by what a batch shares;
    those of the second setting (solved under a sigma2 table of their own) on its context."""
    groups = {}
    for name, (w, d, prm) in _worlds().items():
        if w.mask1 is None:
            continue
        rest = tuple(sorted((k, v) for k, v in prm.items() if k != "sigma2"))
        groups.setdefault((len(d), rest, "sigma2" in prm), []).append((name, padded(w, CAP), d, prm.get("sigma2")))
    seen = {}
    for (_, prm, second), group in groups.items():
        res = check(orbx, ext2 if second else ext, [(w, d) for _, w, d, _ in group], sigma2=group[0][3], **dict(prm))
        seen.update({name: res[k] for k, (name, _, _, _) in enumerate(group)})
    assert seen["coincident"]["n_degenerate"] >= 1 and seen["coincident"]["found_it"] > 0
    assert seen["equals"]["found_it"] == -1 and seen["equals"]["n_best_inliers"] == 20 and seen["equals_19"]["found_it"] >= 0
    assert seen["fix_scale"]["s12"] == 1.0 and seen["truth"]["status"] == 0 and seen["exactly_min"]["its_run"] == 1
    w, d, _ = _worlds()["no_mask"]
    res = check(orbx, ext, [(w, d)])
    assert res[0]["status"] == 0 and res[0]["n_correspondences"] == 100


def test_each_garbage_kind_next_to_a_clean_problem(orbx, ext, sized):
    w, d = sized[65]
    clean = sized[200]
    pairs = [clean] + [(bad(w, what), d) for what, _ in GARBAGE]
    res = check(orbx, ext, pairs)
    assert list(res["status"]) == [0] + [bit | S.NO_RESULT for _, bit in GARBAGE]
    alone = check(orbx, ext, [clean])
    assert alone[0].tobytes() == res[0].tobytes()
    d2 = clean[1].copy()
    d2[0, 1] = -1
    res = check(orbx, ext, [clean, (clean[0], d2)])
    assert res[0]["status"] == 0 and res[1]["status"] & S.BAD_DRAWS


def test_shared_keyframes_on_either_side_and_a_keyframe_with_itself(orbx, ext):
    """Keyframes A, B, C: (A, B), (A, C) with C a disturbed copy of B, (B, A) through the inverted row, and (A, A)."""
    ab = S.make_world(150, 600, cap=CAP, outliers=30, noise=0.5)
    rng = np.random.default_rng(600)
    A = (ab.kps1, ab.n1, ab.points1, ab.mask1, ab.pose1)
    B = (ab.kps2, ab.n2, ab.points2, ab.mask2, ab.pose2)
    C = (ab.kps2, ab.n2, (ab.points2 + rng.normal(0, 0.002, ab.points2.shape)).astype(np.float32), ab.mask2, ab.pose2)
    inv = np.full(CAP, -1, np.int32)
    i1, i2 = ab.edges()
    inv[i2] = i1
    ident = np.where(np.arange(CAP) < ab.n1, np.arange(CAP), -1).astype(np.int32)

    def world(f1, f2, match):
        return S.World(f1[0], f1[1], f2[0], f2[1], match, f1[2], f1[3], f2[2], f2[3], f1[4], f2[4], ab.K)
    worlds = [world(A, B, ab.match), world(A, C, ab.match), world(B, A, inv), world(A, A, ident)]
    draws = [S.make_draws(35, 600 + k) for k in range(4)]
    lists = tuple(np.array(v, np.int32) for v in ([0, 0, 1, 0], [1, 2, 0, 0], [0, 0, 1, 0], [1, 2, 0, 0]))
    got = run_batch(orbx, ext, worlds, np.stack(draws), frames=[A, B, C], lists=lists)
    for p, w in enumerate(worlds):
        same(tuple(a[p] for a in got), S.solve(w, draws[p], 0), "problem %d" % p)
    res = got[0]
    assert (res["status"] == 0).all() and res["n_correspondences"][0] == res["n_correspondences"][2] == 150
    assert abs(res["s12"][0] * res["s12"][2] - 1) < 0.05  # (B, A) is the inverse similarity
    assert res["n_inliers"][3] == res["n_correspondences"][3] == int(ab.mask1[:ab.n1].sum()) and abs(res["s12"][3] - 1) < 1e-5
    # a point set that is not its keyframe's own index: the sets swapped against the keyframes
    frames = [A, (B[0], B[1], A[2], A[3], B[4]), (A[0], A[1], B[2], B[3], A[4])]  # keyframe 1 = B with A's points as set 1 ...
    lists = tuple(np.array(v, np.int32) for v in ([0], [1], [0], [2]))           # ... (A, B) with sets (0, 2): A's and B's points
    got = run_batch(orbx, ext, worlds[:1], np.stack(draws[:1]), frames=frames, lists=lists)
    same(tuple(a[0] for a in got), S.solve(worlds[0], draws[0], 0), "sets apart from keyframes")


def test_without_flags_and_with_the_contexts_table(orbx, ext, sized):
    pair = sized[200]
    a = check(orbx, ext, [pair])
    b = check(orbx, ext, [pair], want_flags=False)
    c = check(orbx, ext, [pair], sigma2=S.sigma2_table())
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes()
    assert np.array_equal(S.sigma2_table(), ext.GetScaleSigmaSquares())
    other = (S.sigma2_table() * np.float32(0.05)).astype(np.float32)  # a tighter table changes the answer
    e = check(orbx, ext, [pair], sigma2=other)
    assert e[0].tobytes() != a[0].tobytes()


def test_capacity_16(orbx, ext):
    w = S.make_world(11, 610, cap=16, extra=5)
    res = check(orbx, ext, [(w, S.make_draws(35, 610))], min_inliers=6)
    assert res[0]["n_correspondences"] == 11 and res[0]["found_it"] >= 0 and res[0]["n_inliers"] == 11


def test_capacity_1024_with_700_correspondences(orbx, ext):
    w = S.make_world(700, 620, cap=1024, outliers=140, noise=0.5)
    res = check(orbx, ext, [(w, S.make_draws(35, 620))])
    assert res[0]["n_correspondences"] == 700 and res[0]["found_it"] >= 0 and res[0]["n_inliers"] > 400


def test_the_largest_capacity(orbx, ext):
    """One problem at capacity ORBX_BOW_MAX_FEATURES, its features spread over the whole rows of both keyframes."""
    w = S.make_world(300, 630, cap=16384, outliers=60, noise=0.5)
    rng = np.random.default_rng(630)
    s1, s2 = np.sort(rng.permutation(16384)[:w.n1]), np.sort(rng.permutation(16384)[:w.n2])
    q = w.copy()
    for a in (q.kps1, q.kps2, q.mask1, q.mask2):
        a[:] = 0
    q.match[:] = -1
    q.kps1[s1], q.points1[s1], q.mask1[s1] = w.kps1[:w.n1], w.points1[:w.n1], w.mask1[:w.n1]
    q.kps2[s2], q.points2[s2], q.mask2[s2] = w.kps2[:w.n2], w.points2[:w.n2], w.mask2[:w.n2]
    has = w.match[:w.n1] >= 0
    q.match[s1[has]] = s2[w.match[:w.n1][has]]
    q.n1 = q.n2 = 16384
    res = check(orbx, ext, [(q, S.make_draws(35, 630))])
    assert res[0]["n_correspondences"] == 300 and res[0]["found_it"] >= 0


def test_lists_and_table_held_across_calls(orbx, sized):
    e = orbx.ORBextractor(1000, 1.2, S.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    a, b = sized[200], sized[65]
    first = check(orbx, e, [a, b])
    again = check(orbx, e, [a, b])  # the same call twice
    assert first.tobytes() == again.tobytes()
    swapped = check(orbx, e, [b, a])  # (same lists, other data)
    assert swapped[1].tobytes() == first[0].tobytes()
    # changed lists: both problems on a's keyframes
    fr = lambda w: [(w.kps1, w.n1, w.points1, w.mask1, w.pose1), (w.kps2, w.n2, w.points2, w.mask2, w.pose2)]  # noqa: E731
    zero, one = np.zeros(2, np.int32), np.ones(2, np.int32)
    got = run_batch(orbx, e, [a[0], a[0]], np.stack([a[1], b[1]]), frames=fr(a[0]) + fr(b[0]), lists=(zero, one, zero, one))
    same(tuple(x[0] for x in got), S.solve(a[0], a[1], 0))
    same(tuple(x[1] for x in got), S.solve(a[0], b[1], 0))
    # changed parameters (another table), then the first again
    loose = check(orbx, e, [a, b], min_inliers=40, max_iterations=50)
    assert loose[0]["max_its"] == 50 and loose[1]["max_its"] == S.ransac_entry(65, 0.99, 40, 50)
    back = check(orbx, e, [a, b])
    assert back.tobytes() == first.tobytes()
    e.close()


def test_host_form_equals_a_batch_of_one(orbx, ext, sized):
    for n in (19, 65, 200):
        w, d = sized[n]
        res, sim, row, inl = ext.sim3_solve(w.kps1[:w.n1], w.points1[:w.n1], w.mask1[:w.n1], w.pose1, w.kps2[:w.n2], w.points2[:w.n2],
                                            w.mask2[:w.n2], w.pose2, w.match[:w.n1], w.K, d)
        got = run_batch(orbx, ext, [w], d[None])
        assert bytes(res) == got[0][0].tobytes() and sim.tobytes() == got[1][0].tobytes()
        assert np.array_equal(row, got[2][0][:w.n1]) and np.array_equal(inl, got[3][0][:w.n1] != 0)
        assert bytes(res) == S.solve(w, d, 0)[0].tobytes()


# ---- the second setting (pose_ref_lib.SECOND): fx != fy, a context of 5 levels of 1.37, camera 1 rolled by 89 degrees ----

CAP_2 = 263  # just above the larger keyframe (257 correspondences + 5 other features)
BOUNDS_2 = (-12, 655, -9, 490)


@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, S.SCALE_FACTOR_2, S.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


def test_second_setting_solver_anisotropic_camera_and_five_levels(orbx, ext2):
    """Two problems (65 and 257 correspondences, a fifth gross mismatches, half a sigma of noise) under K_ANISO: once with the
    context's own table, once with the same table given explicitly; then the host form and Sim3Solver on the smaller one."""
    pairs = [(S.make_world(n, 440 + k, cap=CAP_2, outliers=n // 5, noise=0.5, rot=S.ROLL, **S.SECOND), S.make_draws(35, 440 + k))
             for k, n in enumerate((65, 257))]
    table = S.sigma2_table(S.NLEVELS_2, S.SCALE_FACTOR_2)
    assert ext2.GetScaleSigmaSquares().tobytes() == table.tobytes() and len(table) == S.NLEVELS_2
    worlds, draws = [w for w, _ in pairs], np.stack([d for _, d in pairs])
    res, sim, row, flags = run_batch(orbx, ext2, worlds, draws)  # (the context's table)
    for p, (w, d) in enumerate(pairs):
        same((res[p], sim[p], row[p], flags[p]), S.solve(w, d, 0, sigma2=table), "context's table, problem %d" % p)
    res2 = check(orbx, ext2, pairs, sigma2=table)
    assert res2.tobytes() == res.tobytes()
    for p, n in enumerate((65, 257)):  # not trivial: found, more inliers than the minimum, no planted mismatch among them
        assert res[p]["status"] == 0 and res[p]["found_it"] >= 0 and res[p]["n_correspondences"] == n and res[p]["n_inliers"] > 20
        i1, _ = worlds[p].edges()
        assert not flags[p][i1[worlds[p].truth["bad"]]].any()
    w, d = pairs[0]
    one, sim1, row1, inl = ext2.sim3_solve(w.kps1[:w.n1], w.points1[:w.n1], w.mask1[:w.n1], w.pose1, w.kps2[:w.n2], w.points2[:w.n2],
                                           w.mask2[:w.n2], w.pose2, w.match[:w.n1], w.K, d)
    assert bytes(one) == res[0].tobytes() and sim1.tobytes() == sim[0].tobytes()
    assert np.array_equal(row1, row[0][:w.n1]) and np.array_equal(inl, flags[0][:w.n1] != 0)
    it = iter(d.reshape(-1).tolist() + [0] * (3 * 300))
    kf1 = (w.kps1[:w.n1], w.points1[:w.n1], w.mask1[:w.n1], w.pose1)
    kf2 = (w.kps2[:w.n2], w.points2[:w.n2], w.mask2[:w.n2], w.pose2)
    s = orbx.Sim3Solver(kf1, kf2, w.match[:w.n1], w.K, False, extractor=ext2, rand=lambda: next(it))
    s.SetRansacParameters(0.99, 20, 300)
    d300 = np.zeros((300, 3), np.int32)
    d300[:35] = d
    ref = S.solve(w, d300, 0, sigma2=table)
    _, inl, n, r = s.find()
    assert bytes(r) == ref[0].tobytes() and n == ref[0]["n_inliers"] and np.array_equal(inl, ref[3][:w.n1] != 0)
    assert s.GetEstimatedRotation().tobytes() == ref[1][:9].tobytes() and s.GetEstimatedScale() == ref[1][12]


def test_second_setting_matcher_anisotropic_camera_and_five_levels(orbx, ext2):
    """SearchBySim3 on two truth worlds of 150 and 310 features per keyframe in one batch at the capacity of the larger, under
    the offset bounds; then the smaller one alone through the host form, at its own count and under the usual bounds.  The
    context's scale table (5 levels of 1.37) is the worlds'."""
    assert np.asarray(ext2.GetScaleFactors(), np.float32).tobytes() == S.scale_table(S.NLEVELS_2, S.SCALE_FACTOR_2).tobytes()
    small = S.make_match_world(130, 140, noise_bits=10, rot=S.ROLL, **S.SECOND)
    ws = [padded_m(small, 310), S.make_match_world(290, 141, noise_bits=20, s=0.7, rot=S.ROLL, t=(-3.0, 1.5, 0.6), **S.SECOND)]
    for w in ws:
        w.bounds, w.scale = BOUNDS_2, small.scale
    assert ws[1].cap == 310 == ws[1].n[0] and ws[0].n == [150, 150]
    rows, res = run_match_batch(orbx, ext2, ws)
    for p, w in enumerate(ws):
        same_match(rows[p], res[p], S.search_by_sim3(w), "pair %d" % p)
        assert res[p]["status"] == 0 and res[p]["n_found"] > 0.5 * (~w.truth["have"]).sum()  # not trivial: most partners found
    assert res[1]["n_out_image_21"] > 10  # (the larger world's baseline takes some of KF2's points out of image 1)
    w = small
    n1, n2 = w.n
    T = lambda p: np.c_[p[:9].reshape(3, 3), p[9:]]  # noqa: E731
    m, r = ext2.match_sim3(w.kps[0][:n1], w.desc[0][:n1], w.points[0][:n1], w.mask[0][:n1], w.dist[0][:n1], T(w.pose[0]),
                           w.kps[1][:n2], w.desc[1][:n2], w.points[1][:n2], w.mask[1][:n2], w.dist[1][:n2], T(w.pose[1]), w.sim, w.K,
                           w.bounds, w.match[:n1], 7.5, 100)
    ref = S.search_by_sim3(w)
    assert bytes(r) == ref["res"].tobytes() and np.array_equal(m, ref["matches"][:n1]) and ref["res"]["n_found"] > 30


def test_python_sim3solver(orbx, ext, sized):
    w, d = sized[200]
    it = iter(d.reshape(-1).tolist() + [0] * (3 * 300))
    kf1 = (w.kps1[:w.n1], w.points1[:w.n1], w.mask1[:w.n1], w.pose1)
    kf2 = (w.kps2[:w.n2], w.points2[:w.n2], w.mask2[:w.n2], w.pose2)
    s = orbx.Sim3Solver(kf1, kf2, w.match[:w.n1], w.K, False, extractor=ext, rand=lambda: next(it))
    s.SetRansacParameters(0.99, 20, 300)
    d300 = np.zeros((300, 3), np.int32)
    d300[:35] = d
    ref = S.solve(w, d300, 0)
    T, inl, n, res = s.find()
    assert bytes(res) == ref[0].tobytes() and n == ref[0]["n_inliers"] and np.array_equal(inl, ref[3][:w.n1] != 0)
    assert s.GetEstimatedRotation().tobytes() == ref[1][:9].tobytes() and s.GetEstimatedTranslation().tobytes() == ref[1][9:12].tobytes()
    assert s.GetEstimatedScale() == ref[1][12] and T[:3, 3].tobytes() == ref[1][9:12].tobytes()
    assert np.array_equal(T[:3, :3], np.float32(ref[1][12]) * ref[1][:9].reshape(3, 3))
    # iterate(5) in turns: the similarity comes in the turn found_it falls into
    it = iter(d.reshape(-1).tolist() + [0] * (3 * 300))
    s = orbx.Sim3Solver(kf1, kf2, w.match[:w.n1], w.K, False, extractor=ext, rand=lambda: next(it))
    s.SetRansacParameters(0.99, 20, 300)
    turns = 0
    while True:
        T2, no_more, inl2, n2, _ = s.iterate(5)
        turns += 1
        if T2 is not None or no_more:
            break
    assert turns == ref[0]["found_it"] // 5 + 1 and np.array_equal(T2, T) and n2 == n and not no_more


def test_chained_from_images(orbx, images, golden):
    """extract -> bow transform -> SearchByBoW -> Sim3Solver from two images with no copy between: a keyframe and a second one
    that is its copy shifted by (5, 3) pixels.  Each keyframe's map points lie under its own keypoints on a gently curved surface
    (computed on the device from the extractor's array), keyframe 1's at 1.25 times the depth: its map drifted in scale, and the
    similarity between the cameras has s12 = 1.25.  The row SearchByBoW wrote goes to the solver as it is.  Compared with the
    restatement fed the downloaded arrays."""
    import torch
    import bow_ref_lib as R
    a = images["dbow0"]
    b = np.roll(a, (3, 5), axis=(0, 1))
    h, wd = a.shape
    cap, B, n_iter = 1024, 2, 35
    K = np.array([[520.0, 0, wd / 2], [0, 520.0, h / 2], [0, 0, 1]], np.float32)
    base = R.full_vocabulary(golden["canonical/dbow0/desc"], k=10, L=3)
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=wd, max_height=h, max_batch=B, device=0)
    voc = orbx.Vocabulary.from_arrays(e, *base.arrays())
    z = lambda dt, m: torch.zeros(m, dtype=dt, device="cuda")  # noqa: E731
    d_img = torch.from_numpy(np.stack([a, b])).cuda()
    d_k, d_d, d_n = z(torch.uint8, B * cap * 28), z(torch.uint8, B * cap * 32), z(torch.int32, B)
    fv_node, fv_feat, fv_n = z(torch.int32, B * cap), z(torch.int32, B * cap), z(torch.int32, B)
    m, nm = torch.full((2 * cap,), -7, dtype=torch.int32, device="cuda"), z(torch.int32, 2)
    kf2, kf1 = np.array([0, 1], np.int32), np.array([1, 0], np.int32)  # (the row is indexed by the frame side: KF1)
    draws = np.stack([S.make_draws(n_iter, 700), S.make_draws(n_iter, 701)])
    d_draws = torch.from_numpy(draws).cuda()
    e.extract_batch_device(d_img, B, wd, h, wd, wd * h, d_k, d_d, d_n, cap)
    voc.transform_batch_device(B, d_d, d_n, z(torch.int32, B * cap), z(torch.float64, B * cap), z(torch.int32, B), fv_node, fv_feat, fv_n,
                               levelsup=2, capacity=cap)
    e.match_bow_pairs_device(B, kf2, kf1, d_k, d_d, d_n, fv_node, fv_feat, fv_n, m, nm, nnratio=0.7, checkOri=True, capacity=cap)
    xy = d_k.view(torch.float32).reshape(B, cap, 7)[:, :, :2]
    # one surface in the image's own coordinates: keyframe 1 (the shifted image) sees the point under pixel (x, y) of keyframe 0
    # at (x + 5, y + 3)
    shift = torch.tensor([[0.0, 0.0], [5.0, 3.0]], device="cuda").reshape(B, 1, 2)
    src = xy - shift
    depth = (8.0 + 0.8 * torch.sin(src[:, :, 0] / 40.0) * torch.cos(src[:, :, 1] / 30.0)) * torch.tensor([1.0, 1.25], device="cuda").reshape(B, 1)
    d_pts = torch.stack([(xy[:, :, 0] - K[0, 2]) / K[0, 0] * depth, (xy[:, :, 1] - K[1, 2]) / K[1, 1] * depth, depth], dim=2).contiguous()
    d_pose = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] * B, dtype=torch.float32, device="cuda")  # points in camera frames
    d_res, d_sim, d_row = z(torch.uint8, 2 * orbx.SIM3_RESULT_DTYPE.itemsize), z(torch.float32, 2 * 13), z(torch.int32, 2 * cap)
    e.sim3_solve_batch_device(B, kf1, kf2, kf1, kf2, d_k, d_n, m, B, d_pts, None, d_pose, K, d_draws, d_res, d_sim, d_row, None,
                              capacity=cap)
    torch.cuda.synchronize()
    kps, n = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap), d_n.cpu().numpy()
    match, pts, pose = m.cpu().numpy().reshape(2, cap), d_pts.cpu().numpy(), d_pose.cpu().numpy().reshape(B, 12)
    res, sim, row = d_res.cpu().numpy().view(orbx.SIM3_RESULT_DTYPE), d_sim.cpu().numpy().reshape(2, 13), d_row.cpu().numpy().reshape(2, cap)
    for p in range(2):
        w = S.World(kps[kf1[p]].copy(), n[kf1[p]], kps[kf2[p]].copy(), n[kf2[p]], match[p].copy(), pts[kf1[p]].copy(), None,
                    pts[kf2[p]].copy(), None, pose[kf1[p]].copy(), pose[kf2[p]].copy(), K.reshape(9))
        ref = S.solve(w, draws[p], 0, sigma2=e.GetScaleSigmaSquares())
        same((res[p], sim[p], row[p], None), ref, "sim3 %d" % p)
        print("chained: %d matches, sim3 status %d, N %d, found_it %d, %d inliers, s12 %.4f" %
              (nm[p].item(), res[p]["status"], res[p]["n_correspondences"], res[p]["found_it"], res[p]["n_inliers"], res[p]["s12"]))
        assert res[p]["status"] == 0 and res[p]["n_correspondences"] >= 50 and res[p]["n_inliers"] > 20
        assert abs(res[p]["s12"] / (1.25 if p == 0 else 0.8) - 1) < 0.05
    voc.close()
    e.close()


def test_shim_sim3_agrees_with_the_c_abi(orbx, tmp_path):
    """tests/cpp/shim_sim3.cpp: Sim3Solver of the C++ shim, iterate(5) in turns, gives the bytes of orbx_sim3_solve, and the
    similarity arrives in found_it's turn."""
    import subprocess
    from test_sim3_host import build_shim_sim3
    exe = build_shim_sim3(orbx, tmp_path)
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    status, inliers, n, wrong, turns, agrees = (int(v) for v in [l for l in p.stdout.splitlines() if l.startswith("RESULT")][0].split()[1:])
    assert agrees == 1 and status == 0 and n == 140 and wrong == 0 and 20 < inliers <= 110 and turns >= 1
    found = int([l for l in p.stdout.splitlines() if l.startswith("MATCHER")][0].split()[1])
    assert 8 <= found <= 10  # the ten true pairs the row lacks (the shim and the C ABI agreeing on them is part of `agrees`)


def test_chained_with_triangulated_point_sets(orbx, images, golden):
    """extract -> bow transform -> SearchByBoW -> triangulate_matches -> Sim3Solver with no copy to the host between: two
    keyframes, the second the first's image shifted by (15, 9) pixels -- a fronto-parallel plane at depth 8 seen from a camera
    moved sideways by (15, 9) * 8 / f.  Each keyframe's point set is what orbx_triangulate_matches_batch_device makes of the row
    SearchByBoW wrote for it, keyframe 1's in a map of true scale, keyframe 0's in a map whose poses are 1.25 times as far apart
    (a monocular map that drifted), written side by side into one array of two sets.  The similarity between the cameras then has
    s12 = 0.8 with keyframe 1 as the current one and 1.25 the other way round.  Compared with the restatement fed the
    downloaded arrays."""
    import torch
    import bow_ref_lib as R
    a = images["dbow0"]
    b = np.roll(a, (9, 15), axis=(0, 1))
    h, wd = a.shape
    cap, B, n_iter, f, Z = 1024, 2, 300, 520.0, 8.0
    K = np.array([[f, 0, wd / 2], [0, f, h / 2], [0, 0, 1]], np.float32)
    base = R.full_vocabulary(golden["canonical/dbow0/desc"], k=10, L=3)
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=wd, max_height=h, max_batch=B, device=0)
    voc = orbx.Vocabulary.from_arrays(e, *base.arrays())
    z = lambda dt, m: torch.zeros(m, dtype=dt, device="cuda")  # noqa: E731
    d_img = torch.from_numpy(np.stack([a, b])).cuda()
    d_k, d_d, d_n = z(torch.uint8, B * cap * 28), z(torch.uint8, B * cap * 32), z(torch.int32, B)
    fv_node, fv_feat, fv_n = z(torch.int32, B * cap), z(torch.int32, B * cap), z(torch.int32, B)
    m, nm = torch.full((2 * cap,), -7, dtype=torch.int32, device="cuda"), z(torch.int32, 2)
    kf2, kf1 = np.array([0, 1], np.int32), np.array([1, 0], np.int32)  # (SearchByBoW's row is indexed by its frame side: KF1)
    draws = np.stack([S.make_draws(n_iter, 710), S.make_draws(n_iter, 711)])
    d_draws = torch.from_numpy(draws).cuda()
    e.extract_batch_device(d_img, B, wd, h, wd, wd * h, d_k, d_d, d_n, cap)
    voc.transform_batch_device(B, d_d, d_n, z(torch.int32, B * cap), z(torch.float64, B * cap), z(torch.int32, B), fv_node, fv_feat, fv_n,
                               levelsup=2, capacity=cap)
    e.match_bow_pairs_device(B, kf2, kf1, d_k, d_d, d_n, fv_node, fv_feat, fv_n, m, nm, nnratio=0.7, checkOri=True, capacity=cap)
    t = np.array([15 * Z / f, 9 * Z / f, 0.0], np.float32)
    eye = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
    pose_true = np.stack([np.r_[eye, 0 * t], np.r_[eye, t]]).astype(np.float32)          # the map of keyframe 1's points
    pose_drift = np.stack([np.r_[eye, 0 * t], np.r_[eye, 1.25 * t]]).astype(np.float32)  # the map of keyframe 0's points
    d_pts, d_pmask = z(torch.float32, 2 * cap * 3), z(torch.uint8, 2 * cap)
    d_nrm, d_dist, d_tres = z(torch.float32, 2 * cap * 3), z(torch.float32, 2 * cap * 2), z(torch.uint8, 2 * orbx.TRI_RESULT_DTYPE.itemsize)
    d_maps = (torch.from_numpy(pose_true).cuda(), torch.from_numpy(pose_drift).cuda())  # (alive until the synchronisation below)
    for p, d_map in enumerate(d_maps):  # set p: the points of keyframe kf1[p], indexed by its features
        e.triangulate_matches_pairs_device(B, kf1[p:p + 1], kf2[p:p + 1], d_k, d_n, d_map, K,
                                           m[p * cap:(p + 1) * cap], d_pts[p * cap * 3:], d_pmask[p * cap:], d_nrm[p * cap * 3:],
                                           d_dist[p * cap * 2:], d_tres[p * orbx.TRI_RESULT_DTYPE.itemsize:], capacity=cap)
    # each keyframe's pose in the map its points live in: keyframe 0 in the drifted map, keyframe 1 in the true one
    d_pose = torch.from_numpy(np.stack([pose_drift[0], pose_true[1]])).cuda()
    set1, set2 = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    d_res, d_sim, d_row = z(torch.uint8, 2 * orbx.SIM3_RESULT_DTYPE.itemsize), z(torch.float32, 2 * 13), z(torch.int32, 2 * cap)
    e.sim3_solve_batch_device(B, kf1, kf2, set1, set2, d_k, d_n, m, 2, d_pts, d_pmask, d_pose, K, d_draws, d_res, d_sim, d_row, None,
                              capacity=cap)
    # ... -> match_sim3 on the similarity and the row the solver wrote, and the distances the triangulation wrote
    d_wide, d_mres = z(torch.int32, 2 * cap), z(torch.uint8, 2 * orbx.MSIM3_RESULT_DTYPE.itemsize)
    torch.cuda.synchronize()
    d_wide.copy_(d_row)
    torch.cuda.synchronize()
    e.match_sim3_pairs_device(B, kf1, kf2, set1, set2, d_k, d_d, d_n, 2, d_pts, d_pmask, d_dist, d_pose, d_sim, K, (0, wd, 0, h), d_wide,
                              d_mres, capacity=cap)
    torch.cuda.synchronize()
    kps, n = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap), d_n.cpu().numpy()
    match, pts, pmask = m.cpu().numpy().reshape(2, cap), d_pts.cpu().numpy().reshape(2, cap, 3), d_pmask.cpu().numpy().reshape(2, cap)
    pose, tres = d_pose.cpu().numpy().reshape(B, 12), d_tres.cpu().numpy().view(orbx.TRI_RESULT_DTYPE)
    desc, dist = d_d.cpu().numpy().reshape(B, cap, 32), d_dist.cpu().numpy().reshape(2, cap, 2)
    wide, mres = d_wide.cpu().numpy().reshape(2, cap), d_mres.cpu().numpy().view(orbx.MSIM3_RESULT_DTYPE)
    res, sim, row = d_res.cpu().numpy().view(orbx.SIM3_RESULT_DTYPE), d_sim.cpu().numpy().reshape(2, 13), d_row.cpu().numpy().reshape(2, cap)
    for p in range(2):
        w = S.World(kps[kf1[p]].copy(), n[kf1[p]], kps[kf2[p]].copy(), n[kf2[p]], match[p].copy(), pts[set1[p]].copy(),
                    pmask[set1[p]].copy(), pts[set2[p]].copy(), pmask[set2[p]].copy(), pose[kf1[p]].copy(), pose[kf2[p]].copy(), K.reshape(9))
        ref = S.solve(w, draws[p], 0, sigma2=e.GetScaleSigmaSquares())
        same((res[p], sim[p], row[p], None), ref, "sim3 %d" % p)
        print("triangulated: %d matches, %d points; sim3 status %d, N %d, found_it %d, %d inliers, s12 %.4f, t12 %s" %
              (nm[p].item(), tres[p]["n_points"], res[p]["status"], res[p]["n_correspondences"], res[p]["found_it"], res[p]["n_inliers"],
               res[p]["s12"], res[p]["t12"]))
        assert tres[p]["status"] == 0 and tres[p]["n_points"] >= 50
        assert res[p]["status"] == 0 and res[p]["n_correspondences"] >= 50 and res[p]["n_inliers"] > 20
        assert abs(res[p]["s12"] / (0.8 if p == 0 else 1.25) - 1) < 0.05
        # the matcher: equal to the restatement fed the same arrays; it keeps every entry of the solver's row and adds nFound, so
        # the row ends with at least the solver's inlier count
        q = S.MWorld(cap, K=K, bounds=(0, wd, 0, h))
        for side, (f, st) in enumerate(((kf1[p], set1[p]), (kf2[p], set2[p]))):
            q.kps[side], q.desc[side], q.n[side] = kps[f].copy(), desc[f].copy(), int(n[f])
            q.points[side], q.mask[side], q.dist[side], q.pose[side] = pts[st].copy(), pmask[st].copy(), dist[st].copy(), pose[f].copy()
        q.match, q.sim = row[p].copy(), sim[p].copy()
        mref = S.search_by_sim3(q, scale=e.GetScaleFactors())
        same_match(wide[p], mres[p], mref, "match_sim3 %d" % p)
        print("  match_sim3: nFound %d (%d + %d points searched), %d matches in the end" %
              (mres[p]["n_found"], mres[p]["n_points_12"], mres[p]["n_points_21"], (wide[p] >= 0).sum()))
        assert mres[p]["status"] == 0 and (wide[p] >= 0).sum() == res[p]["n_inliers"] + mres[p]["n_found"] >= res[p]["n_inliers"]
        assert (wide[p][row[p] >= 0] == row[p][row[p] >= 0]).all()
    voc.close()
    e.close()


# ======== ORBmatcher::SearchBySim3 on the device (orbx_match_sim3 / orbx_match_sim3_batch_device) ========

def run_match_batch(orbx, ext, worlds, th=7.5, orb_dist=100, frames=None, lists=None):
    """MWorlds of one capacity (and one K, one choice of masks / point descriptors) as one device batch -> (rows [P, cap], results
    [P]).  By default pair p has keyframes and sets 2 p, 2 p + 1; frames = [(world, side)] and lists = (kf1, kf2, set1, set2)."""
    import torch
    Pn, cap = len(worlds), worlds[0].cap
    if frames is None:
        frames = [(w, s) for w in worlds for s in (0, 1)]
        even = np.arange(0, 2 * Pn, 2, dtype=np.int32)
        lists = (even, even + 1, even, even + 1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    col = lambda f: np.stack([f(w, s) for w, s in frames])  # noqa: E731
    d_k, d_d, d_n = d(col(lambda w, s: w.kps[s])), d(col(lambda w, s: w.desc[s])), d(np.array([w.n[s] for w, s in frames], np.int32))
    d_p, d_q, d_pose = d(col(lambda w, s: w.points[s])), d(col(lambda w, s: w.dist[s])), d(col(lambda w, s: w.pose[s]))
    d_mask = d(col(lambda w, s: w.mask[s])) if worlds[0].mask is not None else None
    d_pd = d(col(lambda w, s: w.pdesc[s])) if worlds[0].pdesc is not None else None
    d_sim, d_m = d(np.stack([w.sim for w in worlds])), d(np.stack([w.match for w in worlds]))
    d_res = torch.full((Pn * orbx.MSIM3_RESULT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    ext.match_sim3_pairs_device(len(frames), lists[0], lists[1], lists[2], lists[3], d_k, d_d, d_n, len(frames), d_p, d_mask, d_q, d_pose,
                                d_sim, worlds[0].K, worlds[0].bounds, d_m, d_res, th, orb_dist, d_pd, capacity=cap)
    torch.cuda.synchronize()
    return d_m.cpu().numpy().view(np.int32).reshape(Pn, cap), d_res.cpu().numpy().view(orbx.MSIM3_RESULT_DTYPE)


def same_match(row, res, ref, what=""):
    for f in S.MSIM3_RESULT_DTYPE.names:
        assert res[f] == ref["res"][f], (what, f, res[f], ref["res"][f])
    assert row.tobytes() == ref["matches"].tobytes(), what


def padded_m(w, cap):
    """An MWorld in rows of a larger capacity."""
    q = S.MWorld(cap, K=w.K, bounds=w.bounds, masks=w.mask is not None, pdesc=w.pdesc is not None)
    for s in (0, 1):
        for name in ("kps", "desc", "points", "dist") + (("mask",) if w.mask is not None else ()) + (("pdesc",) if w.pdesc is not None else ()):
            getattr(q, name)[s][:w.cap] = getattr(w, name)[s]
    q.n, q.pose, q.sim, q.truth = list(w.n), [p.copy() for p in w.pose], w.sim.copy(), w.truth
    q.match[:w.cap] = w.match
    return q


def test_match_sim3_host_worlds(orbx, ext, ext2):
    """Every world of the host test, each alone at its own capacity (capacity = count for the truth worlds); those of the second
    setting on its context, whose scale table is theirs."""
    from test_sim3_host import _match_worlds
    for name, (w, th, od) in _match_worlds().items():
        row, res = run_match_batch(orbx, ext2 if name.endswith("@2") else ext, [w], th, od)
        same_match(row[0], res[0], S.search_by_sim3(w, th, od), name)
    assert _match_worlds()["w1500"][0].n == [1500, 1500] == [_match_worlds()["w1500"][0].cap] * 2


def test_match_sim3_batch_with_edge_pairs(orbx, ext):
    """One batch at capacity 512: truth worlds, a world with its counts out of range, one with a dead similarity, empty
    keyframes on either side and a garbage entry in the row -- next to one another."""
    from test_sim3_host import _disagree_world, _emptied, _two_on_one_world
    cap = 512
    ws = [padded_m(S.make_match_world(300, 40 + k, noise_bits=10 * k), cap) for k in range(3)]
    ws += [padded_m(_disagree_world(), cap), padded_m(_two_on_one_world(), cap)]
    ws += [_emptied(padded_m(S.make_match_world(100, 50), cap), 0), _emptied(padded_m(S.make_match_world(100, 51), cap), 1)]
    bad_n, dead, junk = ws[0].copy(), ws[1].copy(), ws[2].copy()
    bad_n.n = [cap + 7, -3]
    dead.sim[12] = 0.0
    junk.match[junk.truth["slots1"][0]] = 400  # beyond KF2's 320 features
    junk.points[1][junk.truth["slots2"][5], 0] = np.nan
    ws += [bad_n, dead, junk]
    rows, res = run_match_batch(orbx, ext, ws)
    for p, w in enumerate(ws):
        same_match(rows[p], res[p], S.search_by_sim3(w), "pair %d" % p)
    assert res["status"][-3] & S.MSIM3_BAD_INPUT and res["status"][-2] == S.MSIM3_NONFINITE
    assert res["status"][-1] == S.MSIM3_BAD_INPUT | S.MSIM3_NONFINITE and (res["n_found"][:3] > 100).all()
    alone = run_match_batch(orbx, ext, ws[:1])
    assert alone[0][0].tobytes() == rows[0].tobytes() and alone[1][0].tobytes() == res[0].tobytes()


def test_match_sim3_shared_keyframes_and_a_pair_of_one_frame(orbx, ext):
    """Keyframes A, B of a truth world: (A, B), (B, A) under the inverse similarity with the inverted row, and (A, A) under the
    identity, whose sides are one frame: every unmatched point finds itself."""
    w = S.make_match_world(300, 60, noise_bits=10)
    Rm, t, s = w.sim[:9].reshape(3, 3).astype(np.float64), w.sim[9:12].astype(np.float64), float(w.sim[12])
    ba = w.copy()
    for name in ("kps", "desc", "points", "dist", "mask", "pose", "n"):
        getattr(ba, name).reverse()
    ba.sim = np.r_[Rm.T.reshape(9), -(Rm.T @ t) / s, 1 / s].astype(np.float32)
    ba.match[:] = -1
    have = w.match >= 0
    ba.match[w.match[have]] = np.flatnonzero(have)
    aa = w.copy()
    for name in ("kps", "desc", "points", "dist", "mask", "pose"):
        getattr(aa, name)[1] = getattr(aa, name)[0].copy()
    aa.n[1], aa.sim = aa.n[0], S.IDENTITY_SIM.copy()
    aa.match[:] = -1
    # under the identity a point is 1 / 0.95 of its max away from its own camera only by chance: give every point room
    aa.dist[0][:, 0], aa.dist[0][:, 1] = 0.01, 1000.0
    aa.dist[1] = aa.dist[0].copy()
    aa.kps[0]["octave"][:] = 7  # (max / dist is large: level 7)
    aa.kps[1] = aa.kps[0].copy()
    worlds = [w, ba, aa]
    lists = tuple(np.array(v, np.int32) for v in ([0, 1, 2], [1, 0, 2], [0, 1, 2], [1, 0, 2]))
    rows, res = run_match_batch(orbx, ext, worlds, frames=[(w, 0), (w, 1), (aa, 0)], lists=lists)
    for p, q in enumerate(worlds):
        same_match(rows[p], res[p], S.search_by_sim3(q), "pair %d" % p)
    assert res["n_found"][0] > 100 and abs(int(res["n_found"][1]) - int(res["n_found"][0])) <= 3
    pts = np.flatnonzero(aa.mask[0][:aa.n[0]])
    assert res["n_points_12"][2] == len(pts) and res["n_found"][2] >= 0.9 * len(pts)
    assert (rows[2][rows[2] >= 0] == np.flatnonzero(rows[2] >= 0)).all()


def test_match_sim3_at_the_largest_capacity(orbx, ext):
    """Capacity ORBX_BOW_MAX_FEATURES launches the kernel with its largest LDS layout (110.0 KB); the features sit at the end of
    the rows, so the last words of every LDS array are used."""
    w = S.make_match_world(1000, 70, extra=15384, noise_bits=10)
    assert w.cap == 16384 == w.n[0] == w.n[1]
    row, res = run_match_batch(orbx, ext, [w])
    same_match(row[0], res[0], S.search_by_sim3(w), "16384")
    assert res[0]["n_found"] > 400 and max(w.truth["slots1"].max(), w.truth["slots2"].max()) > 16300


def test_match_sim3_host_form_and_python_matcher(orbx, ext):
    from test_sim3_host import _match_worlds
    for name in ("truth_noisy", "truth_pdesc", "disagree"):
        w, th, od = _match_worlds()[name]
        n1, n2 = w.n
        cut = lambda a, n: None if a is None else a[:n]  # noqa: E731
        pd = w.pdesc or [None, None]
        mk = w.mask or [None, None]
        T = lambda p: np.c_[p[:9].reshape(3, 3), p[9:]]  # noqa: E731
        m, res = ext.match_sim3(w.kps[0][:n1], w.desc[0][:n1], w.points[0][:n1], cut(mk[0], n1), w.dist[0][:n1], T(w.pose[0]),
                                w.kps[1][:n2], w.desc[1][:n2], w.points[1][:n2], cut(mk[1], n2), w.dist[1][:n2], T(w.pose[1]), w.sim, w.K,
                                w.bounds, w.match[:n1], th, od, cut(pd[0], n1), cut(pd[1], n2))
        ref = S.search_by_sim3(w, th, od)
        assert bytes(res) == ref["res"].tobytes() and np.array_equal(m, ref["matches"][:n1]), name
    w, th, od = _match_worlds()["truth_noisy"]

    class KF:
        def __init__(self, s):
            self.mvKeysUn, self.mDescriptors, self.mpORBextractor, self.bounds = w.kps[s][:w.n[s]], w.desc[s][:w.n[s]], ext, w.bounds
    T = lambda p: np.c_[p[:9].reshape(3, 3), p[9:]]  # noqa: E731
    maps = [(w.points[s][:w.n[s]], w.mask[s][:w.n[s]], w.dist[s][:w.n[s]], T(w.pose[s]), None) for s in (0, 1)]
    n, m, res = orbx.ORBmatcher(extractor=ext).SearchBySim3(KF(0), KF(1), maps[0], maps[1], w.match[:w.n[0]], w.sim[12], w.sim[:9], w.sim[9:12],
                                                            7.5, K=w.K)
    ref = S.search_by_sim3(w)
    assert n == ref["res"]["n_found"] and np.array_equal(m, ref["matches"][:w.n[0]])


def test_chained_solver_and_matcher_on_one_row(orbx, ext):
    """compute_sim3_pairs_device: the solver writes d_sim3 and the inlier row, the matcher reads and widens them, with no copy
    between.  A truth world whose row holds 40 % of the pairs, a fifth of those wrong.  Equal to the restatements chained; nFound
    + the inliers is at least the solver's inlier count."""
    import torch
    cap = 512
    mw = padded_m(S.make_match_world(400, 80, noise_bits=10), cap)
    rng = np.random.default_rng(80)
    t = mw.truth
    have = np.flatnonzero(t["have"])
    wrong = rng.choice(have, len(have) // 5, replace=False)
    mw.match[t["slots1"][wrong]] = rng.permutation(t["slots2"][wrong])  # mismatches among points
    sw = S.World(mw.kps[0], mw.n[0], mw.kps[1], mw.n[1], mw.match, mw.points[0], mw.mask[0], mw.points[1], mw.mask[1], mw.pose[0], mw.pose[1], mw.K)
    draws = S.make_draws(300, 80)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    col = lambda a: d(np.stack(a))  # noqa: E731
    z = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_sres, d_sim, d_row, d_mres = z(orbx.SIM3_RESULT_DTYPE.itemsize), z(52), z(cap * 4), z(orbx.MSIM3_RESULT_DTYPE.itemsize)
    one, two = np.array([0], np.int32), np.array([1], np.int32)
    ext.compute_sim3_pairs_device(2, one, two, one, two, col(mw.kps), col(mw.desc), d(np.array(mw.n, np.int32)), d(mw.match), 2, col(mw.points),
                                  col(mw.mask), col(mw.dist), col(mw.pose), mw.K, mw.bounds, d(draws), d_sres, d_sim, d_row, d_mres,
                                  capacity=cap)
    torch.cuda.synchronize()
    sres, sim = d_sres.cpu().numpy().view(orbx.SIM3_RESULT_DTYPE)[0], d_sim.cpu().numpy().view(np.float32)
    row, mres = d_row.cpu().numpy().view(np.int32), d_mres.cpu().numpy().view(orbx.MSIM3_RESULT_DTYPE)[0]
    ref = S.solve(sw, draws, 0)
    assert sres.tobytes() == ref[0].tobytes() and sim.tobytes() == ref[1].tobytes() and sres["status"] == 0
    q = mw.copy()
    q.match, q.sim = ref[2].copy(), ref[1].copy()
    mref = S.search_by_sim3(q)
    same_match(row, mres, mref, "chained")
    print("chained: solver %d inliers of %d, matcher nFound %d, %d matches in the end" %
          (sres["n_inliers"], sres["n_correspondences"], mres["n_found"], (row >= 0).sum()))
    assert mres["n_found"] >= 100 and (row >= 0).sum() == sres["n_inliers"] + mres["n_found"] >= sres["n_inliers"]
    assert (row[ref[2] >= 0] == ref[2][ref[2] >= 0]).all()  # the solver's entries are never changed
