"""Optimizer::PoseOptimization on the device (orbx_pose_optimize / orbx_pose_optimize_batch_device) equals the CPU restatement
tests/cpp/pose_ref.cpp BIT FOR BIT: every field of orbx_pose_result, the bytes of its f64 included, and every outlier flag.  Both
sides fix the same order of the sums, share the arithmetic and the round logic and contract nothing (include/orbx.h).  What the
restatement itself is worth is tests/test_pose_host.py's business, which also shows which branches the worlds used here run."""
import subprocess

import numpy as np
import pytest

import pose_ref_lib as P

pytestmark = pytest.mark.gpu

# correspondences per problem: none, below 3, 3, one round only (9), four rounds (10), around a wave, beyond two and four strides
COUNTS = (0, 2, 3, 9, 10, 63, 64, 65, 129, 300)
CAP = 307  # just above the largest frame (300 correspondences + 5 other features)


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, P.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sized():
    """A world per count of COUNTS, an eighth of them gross mismatches from 9 correspondences on."""
    return {n: P.make_world(n, 40 + k, cap=CAP, outliers=(max(n // 8, 1) if n >= 9 else 0)) for k, n in enumerate(COUNTS)}


def named(name):
    return P.world(name).padded(CAP)


def with_match(w):
    """The same problem through a match row: feature j names entry j."""
    q = w.copy()
    if q.match is None:
        q.match = np.full(q.cap, -1, np.int32)
        q.match[:max(min(q.n, q.cap), 0)] = np.arange(max(min(q.n, q.cap), 0))
    return q


def bad(w, what):
    q = w.copy()
    j, i = (int(v[0]) for v in w.edges())
    if what == "count":
        q.n = q.cap + 1
    elif what == "match":
        q = with_match(q)
        q.match[j] = q.cap
    elif what == "octave":
        q.kps["octave"][j] = P.NLEVELS
    elif what == "nan":
        q.points[i, 0] = np.nan
    return q


def run_batch(orbx, ext, worlds, n_iterations=10, inv_sigma2=None, frames=None, sets=None):
    """The worlds as one device batch -> (results [P], flags [P, cap]).  By default problem p has frame p and point set p of its
    own; frames / sets: lists of (kps, n) / (points, mask) rows and the worlds name them by their attributes frame / point_set.
    A match array goes down when any world has a match row (then every world needs one), a mask when any world has one."""
    import torch
    Pn, cap = len(worlds), worlds[0].cap
    if frames is None:
        frames, sets = [(w.kps, w.n) for w in worlds], [(w.points, w.mask) for w in worlds]
        fi, si = np.arange(Pn, dtype=np.int32), np.arange(Pn, dtype=np.int32)
    else:
        fi, si = np.array([w.frame for w in worlds], np.int32), np.array([w.point_set for w in worlds], np.int32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_k, d_n = d(np.stack([f[0] for f in frames])), d(np.array([f[1] for f in frames], np.int32))
    d_p = d(np.stack([s[0] for s in sets]))
    masked = any(s[1] is not None for s in sets)
    assert not masked or all(s[1] is not None for s in sets)
    d_mask = d(np.stack([s[1] for s in sets])) if masked else None
    matched = any(w.match is not None for w in worlds)
    assert not matched or all(w.match is not None for w in worlds)
    d_m = d(np.stack([w.match for w in worlds])) if matched else None
    d_pose = d(np.stack([w.pose0 for w in worlds]))
    d_res = torch.full((Pn * orbx.POSE_RESULT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    d_out = torch.full((Pn * cap,), 0xA5, dtype=torch.uint8, device="cuda")
    ext.pose_optimize_batch_device(len(frames), fi, si, d_k, d_n, d_m, len(sets), d_p, d_mask, d_pose, worlds[0].K, d_res, d_out,
                                   inv_sigma2=inv_sigma2, n_iterations=n_iterations, capacity=cap)
    torch.cuda.synchronize()
    return d_res.cpu().numpy().view(orbx.POSE_RESULT_DTYPE), d_out.cpu().numpy().reshape(Pn, cap)


def same(res, flags, ref, rflags, what=""):
    """Bit for bit: the record's bytes field by field (so that a difference names its field), then the flags."""
    for f in P.POSE_RESULT_DTYPE.names:
        assert np.asarray(res[f]).tobytes() == np.asarray(ref[f]).tobytes(), (what, f, res[f], ref[f])
    assert flags.tobytes() == rflags.tobytes(), what


def check(orbx, ext, worlds, **kw):
    ref_kw = {k: v for k, v in kw.items() if k in ("n_iterations", "inv_sigma2")}
    res, flags = run_batch(orbx, ext, worlds, **kw)
    for p, w in enumerate(worlds):
        r, rf, _, _ = P.pose_optimize(w, **ref_kw)
        same(res[p], flags[p], r, rf, "problem %d" % p)
    return res


@pytest.mark.parametrize("n", COUNTS)
def test_one_problem_of_each_size(orbx, ext, sized, n):
    res = check(orbx, ext, [sized[n]])
    assert res[0]["n_correspondences"] == n
    assert res[0]["status"] == (P.FEW_POINTS if n < 3 else 0)
    assert res[0]["rounds"] == (0 if n < 3 else 1 if n < 10 else 4)
    if n >= 9:
        assert res[0]["n_bad"] == max(n // 8, 1)


def _mixed(sized):
    """Nine problems side by side: refused, few-point, diverging (rejected trials, every stop reason) and clean ones."""
    return [bad(sized[64], "octave"), named("far"), sized[2], named("clean"), sized[300], bad(sized[65], "nan"), named("noisy"),
            sized[9], named("converged")]


@pytest.mark.parametrize("count", [3, 4, 5, 9])
def test_partial_and_full_workgroups(orbx, ext, sized, count):
    res = check(orbx, ext, _mixed(sized)[:count])
    assert list(res["status"][:3]) == [P.BAD_INPUT, 0, P.FEW_POINTS]
    assert res[1]["rejected_trials"] > 0


def test_each_garbage_kind_next_to_a_clean_problem(orbx, ext, sized):
    from test_pose_host import plane_world
    clean = with_match(sized[129])
    worlds = [bad(sized[65], "count"), clean, bad(sized[64], "match"), bad(sized[63], "octave"), bad(sized[300], "nan"),
              plane_world(CAP)]
    res = check(orbx, ext, [with_match(w) for w in worlds])
    assert list(res["status"]) == [P.BAD_INPUT, 0, P.BAD_INPUT, P.BAD_INPUT, P.NONFINITE, P.NONFINITE]
    for p, w in enumerate(worlds):
        if p != 1:
            assert res[p]["R"].tobytes() == w.pose0[:9].tobytes() and res[p]["tcw"].tobytes() == w.pose0[9:].tobytes()
    alone = check(orbx, ext, [clean])
    assert alone[0].tobytes() == res[1].tobytes()


def test_one_frame_in_several_problems(orbx, ext, sized):
    """Relocalisation candidates: the same frame against three point sets (its own, another world's, its own moved) from three
    start poses."""
    a, b = sized[129], sized[300]
    moved = a.points.copy()
    moved[:, 0] += np.float32(0.05)
    frames, sets = [(b.kps, b.n), (a.kps, a.n)], [(a.points, a.mask), (b.points, b.mask), (moved, a.mask)]
    worlds = []
    for point_set, pose0 in ((0, a.pose0), (1, b.pose0), (2, a.pose0), (0, b.pose0)):
        w = P.World(a.kps, a.n, None, sets[point_set][0], sets[point_set][1], pose0, a.K)
        w.frame, w.point_set = 1, point_set
        worlds.append(w)
    res = check(orbx, ext, worlds, frames=frames, sets=sets)
    assert res[0]["status"] == 0 and res[0]["n_bad"] == 129 // 8
    assert res[0].tobytes() != res[2].tobytes() and res[0].tobytes() != res[3].tobytes()


def test_match_form_against_the_direct_form(orbx, ext):
    """A problem through a match row (SearchByBoW's layout: the points in a set of their own) gives the bytes of the same problem
    with the points gathered per feature."""
    m = named("matched")
    j, i = m.edges()
    direct = m.copy()
    direct.match, direct.points, direct.mask = None, np.zeros_like(m.points), np.zeros_like(m.mask)
    direct.points[j], direct.mask[j] = m.points[i], 1
    res = check(orbx, ext, [m, with_match(named("clean"))])
    res2 = check(orbx, ext, [direct])
    assert res[0].tobytes() == res2[0].tobytes() and res[0]["status"] == 0 and res[0]["n_correspondences"] == 150


def test_without_a_point_mask(orbx, ext):
    w = P.make_world(100, 60, outliers=9, extra=0, use_mask=False)
    res = check(orbx, ext, [w, P.make_world(100, 61, outliers=4, extra=0, use_mask=False)])
    assert res[0]["n_correspondences"] == 100 and res[0]["n_bad"] == 9 and res[1]["n_bad"] == 4


def test_null_table_is_the_contexts(orbx, ext, sized):
    table = ext.GetInverseScaleSigmaSquares()
    res, flags = run_batch(orbx, ext, [sized[129]])
    r, rf, _, _ = P.pose_optimize(sized[129], inv_sigma2=table)
    same(res[0], flags[0], r, rf)
    other = (table * np.float32(0.5)).astype(np.float32)
    res2 = check(orbx, ext, [sized[129]], inv_sigma2=other)
    assert res2[0]["chi2_initial"] != res[0]["chi2_initial"]


def test_problem_list_and_table_held_across_calls(orbx, sized):
    """The problem list and the table live on the device between calls, each with the host copy its upload read: call after call
    on one context of its own -- a first list, the same again (no upload), as many problems over other frames and point sets
    (replaced in place), one problem, three (the device array grows), the first list again, and then the same two problems under
    another table (the table alone is replaced) and under the first one -- every call equals the restatement bit for bit."""
    e = orbx.ORBextractor(1000, 1.2, P.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    a, b, c = sized[63], sized[64], sized[65]
    off = P.inv_sigma2_table()
    off[P.NLEVELS - 1] = 0  # the usual table with the weight of the last level set to 0
    refs = {}

    def step(what, worlds, table=None, swapped=False):
        kw = {}
        if swapped:  # problem p reads frame and point set 1 - p
            worlds = [w.copy() for w in worlds]
            for p, w in enumerate(worlds):
                w.frame = w.point_set = 1 - p
            kw = dict(frames=[(w.kps, w.n) for w in worlds[::-1]], sets=[(w.points, w.mask) for w in worlds[::-1]])
        res, flags = run_batch(orbx, e, worlds, inv_sigma2=table, **kw)
        for p, w in enumerate(worlds):
            key = (w.n, table is not None)
            if key not in refs:
                refs[key] = P.pose_optimize(w, inv_sigma2=table)[:2]
            same(res[p], flags[p], *refs[key], what="%s, problem %d" % (what, p))

    try:
        step("two problems", [a, b])
        step("the same list", [a, b])
        step("as many problems, other frames and sets", [a, b], swapped=True)
        step("one problem", [c])
        step("three problems", [b, c, a])
        step("the first list again", [a, b])
        step("another table", [a, b], table=off)
        step("the first table again", [a, b])
    finally:
        e.close()


@pytest.mark.parametrize("n_iterations", [0, 3])
def test_few_and_no_iterations(orbx, ext, sized, n_iterations):
    res = check(orbx, ext, [named("far"), sized[9], sized[65]], n_iterations=n_iterations)
    assert list(res[0]["iterations"]) == [n_iterations] * 4 and list(res[1]["iterations"]) == [n_iterations, 0, 0, 0]


def test_host_form_equals_a_batch_of_one(orbx, ext, sized):
    for w in (sized[129], sized[2], bad(sized[65], "octave"), bad(sized[64], "nan")):
        res, flags = run_batch(orbx, ext, [w])
        T = np.c_[w.pose0[:9].reshape(3, 3), w.pose0[9:]]
        one, out = ext.pose_optimize(w.kps[:w.n], w.points[:w.n], w.mask[:w.n], T, w.K)
        assert bytes(one) == res[0].tobytes()
        assert np.array_equal(out, flags[0, :w.n] != 0) and not flags[0, w.n:].any()
    w = sized[129]
    frame = orbx.Frame.from_arrays(w.kps[:w.n], np.zeros((w.n, 32), np.uint8), (0, 640, 0, 480))
    n, T, out, r = orbx.Optimizer.PoseOptimization(frame, w.points[:w.n], w.mask[:w.n], np.c_[w.pose0[:9].reshape(3, 3), w.pose0[9:]],
                                                   K=w.K, extractor=ext)
    ref = P.pose_optimize(w)[0]
    assert n == ref["n_inliers"] and T[:3, :3].tobytes() == ref["R"].tobytes() and T[:3, 3].tobytes() == ref["tcw"].tobytes()


# ---- the second setting (pose_ref_lib.SECOND): fx != fy, a context of 5 levels of 1.37, a true pose rolled by 89 degrees ----

CAP_2 = 263  # just above the larger frame (257 correspondences + 5 other features)


@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, P.SCALE_FACTOR_2, P.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


def test_second_setting_anisotropic_camera_and_five_levels(orbx, ext2):
    """Two problems (65 and 257 correspondences) under K_ANISO: once with the context's own table, once with the same table
    given explicitly; then the host form and the Python class on the smaller one.  A v-projection that read fx, or a table of
    the usual 8 levels of 1.2, would change every chi2 here."""
    worlds = [P.make_world(n, 140 + k, cap=CAP_2, outliers=n // 8, motion=P.MOTION_2, **P.SECOND) for k, n in enumerate((65, 257))]
    table = P.inv_sigma2_of("second")
    assert ext2.GetInverseScaleSigmaSquares().tobytes() == table.tobytes() and len(table) == P.NLEVELS_2
    res, flags = run_batch(orbx, ext2, worlds)  # (the context's table)
    for p, w in enumerate(worlds):
        r, rf, _, _ = P.pose_optimize(w, inv_sigma2=table)
        same(res[p], flags[p], r, rf, "context's table, problem %d" % p)
    res2 = check(orbx, ext2, worlds, inv_sigma2=table)
    assert res2.tobytes() == res.tobytes()
    for p, n in enumerate((65, 257)):  # not trivial: four rounds, the planted mismatches flagged, the rest inliers
        assert res[p]["status"] == 0 and res[p]["rounds"] == 4 and res[p]["n_correspondences"] == n
        assert res[p]["n_bad"] == n // 8 and res[p]["n_inliers"] == n - n // 8 and res[p]["chi2_final"] < res[p]["chi2_initial"]
        assert np.array_equal(np.flatnonzero(flags[p]), worlds[p].truth["bad"])
    w = worlds[0]
    T = np.c_[w.pose0[:9].reshape(3, 3), w.pose0[9:]]
    one, out = ext2.pose_optimize(w.kps[:w.n], w.points[:w.n], w.mask[:w.n], T, w.K)
    assert bytes(one) == res[0].tobytes() and np.array_equal(out, flags[0, :w.n] != 0)
    frame = orbx.Frame.from_arrays(w.kps[:w.n], np.zeros((w.n, 32), np.uint8), (0, 640, 0, 480))
    n, T2, out2, _ = orbx.Optimizer.PoseOptimization(frame, w.points[:w.n], w.mask[:w.n], T, K=w.K, extractor=ext2)
    assert n == res[0]["n_inliers"] and T2[:3, :3].tobytes() == res[0]["R"].tobytes() and T2[:3, 3].tobytes() == res[0]["tcw"].tobytes()
    assert np.array_equal(np.asarray(out2, bool), out)


# ---- behind the LDS cache: a lane's edges from the seventh on are read from the problem's rows, their flags from its outlier row
# (tests/test_pose_host.py, test_the_cache_worlds_leave_the_cache, shows which worlds hold what there).  Capacity 1024, in a
# context of their own ----

BIG = P.BIG_CAP
CACHE_WORLDS = ("cache_edge", "cache_full", "cache_skewed", "cache_holes")


@pytest.fixture(scope="module")
def big(orbx):
    e = orbx.ORBextractor(1000, 1.2, P.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


def _as_given(res, flags, w, status):
    assert res["status"] == status and not flags.any()
    assert res["R"].tobytes() == w.pose0[:9].tobytes() and res["tcw"].tobytes() == w.pose0[9:].tobytes()


@pytest.mark.parametrize("name", CACHE_WORLDS)
def test_one_world_behind_the_cache(orbx, big, name):
    w = P.world(name)
    res = check(orbx, big, [w])
    assert w.cap == BIG and res[0]["status"] == 0 and res[0]["rounds"] == 4 and res[0]["n_correspondences"] == len(w.edges()[0])
    assert res[0]["n_bad"] >= len(w.truth["bad"]) > 0


def test_nine_problems_that_leave_the_cache_or_do_not(orbx, big, sized):
    """Two full workgroups and one wave, the waves of a workgroup ending at very different times: worlds with a few edges, with
    hundreds and with none behind the cache, a few-point problem and two refused ones -- a NaN point, and a match index >= cap
    on a feature behind its lane's cache."""
    full = P.world("cache_full")
    late = with_match(full)
    behind = P.lane_layout(full)[0]
    late.match[behind[len(behind) // 2]] = BIG
    worlds = [full, sized[2].padded(BIG), P.world("cache_skewed"), P.world("clean").padded(BIG), P.world("cache_holes"),
              bad(full, "nan"), P.world("cache_edge"), P.world("far").padded(BIG), late]
    res, flags = run_batch(orbx, big, [with_match(w) for w in worlds])
    for p, w in enumerate(worlds):
        r, rf, _, _ = P.pose_optimize(w)
        same(res[p], flags[p], r, rf, "problem %d" % p)
    assert list(res["status"]) == [0, P.FEW_POINTS, 0, 0, 0, P.NONFINITE, 0, 0, P.BAD_INPUT]
    for p in (1, 5, 8):
        _as_given(res[p], flags[p], worlds[p], res[p]["status"])
    assert res[0]["n_correspondences"] == 700 and res[2]["n_correspondences"] == 24 and res[7]["rejected_trials"] > 0


def test_a_point_in_the_plane_behind_the_cache(orbx, big):
    """NONFINITE with the in-plane point on an edge behind the cache: every flag that the rounds set (test_pose_host shows that
    they set some behind the cache) is cleared again."""
    from test_pose_host import plane_world
    w = plane_world(BIG, 450, True)
    res, flags = run_batch(orbx, big, [w])
    r, rf, per_round, _ = P.pose_optimize(w)
    same(res[0], flags[0], r, rf)
    assert per_round[:, P.lane_layout(w)[0]].any()
    _as_given(res[0], flags[0], w, P.NONFINITE)


@pytest.mark.parametrize("n_iterations", [0, 3])
def test_few_and_no_iterations_behind_the_cache(orbx, big, n_iterations):
    """With no iteration the classification alone walks the edges behind the cache."""
    res = check(orbx, big, [P.world("cache_full")], n_iterations=n_iterations)
    assert res[0]["status"] == 0 and list(res[0]["iterations"]) == [n_iterations] * 4 and res[0]["n_bad"] > 0


def test_host_forms_behind_the_cache(orbx, big):
    """orbx_pose_optimize, ORBextractor.pose_optimize and Optimizer.PoseOptimization at n = 705 (the capacity is then n, no
    multiple of 64) against a batch of one at capacity 1024."""
    w = P.world("cache_full")
    assert w.n == 705
    res, flags = run_batch(orbx, big, [w])
    T = np.c_[w.pose0[:9].reshape(3, 3), w.pose0[9:]]
    one, out = big.pose_optimize(w.kps[:w.n], w.points[:w.n], w.mask[:w.n], T, w.K)
    assert bytes(one) == res[0].tobytes() and one.status == 0
    assert np.array_equal(out, flags[0, :w.n] != 0) and not flags[0, w.n:].any()
    frame = orbx.Frame.from_arrays(w.kps[:w.n], np.zeros((w.n, 32), np.uint8), (0, 640, 0, 480))
    n, T2, out2, r2 = orbx.Optimizer.PoseOptimization(frame, w.points[:w.n], w.mask[:w.n], T, K=w.K, extractor=big)
    ref, rf, _, _ = P.pose_optimize(w)
    assert bytes(r2) == ref.tobytes() == res[0].tobytes() and np.array_equal(out2, rf[:w.n] != 0)
    assert n == ref["n_inliers"] and T2[:3, :3].tobytes() == ref["R"].tobytes() and T2[:3, 3].tobytes() == ref["tcw"].tobytes()


def test_one_frame_in_several_problems_behind_the_cache(orbx, big):
    """test_one_frame_in_several_problems with a frame of 450 correspondences."""
    a, b = P.make_world(450, 90, cap=BIG, outliers=50), P.world("cache_full")
    moved = a.points.copy()
    moved[:, 0] += np.float32(0.05)
    frames, sets = [(b.kps, b.n), (a.kps, a.n)], [(a.points, a.mask), (b.points, b.mask), (moved, a.mask)]
    worlds = []
    for point_set, pose0 in ((0, a.pose0), (1, b.pose0), (2, a.pose0), (0, b.pose0)):
        w = P.World(a.kps, a.n, None, sets[point_set][0], sets[point_set][1], pose0, a.K)
        w.frame, w.point_set = 1, point_set
        worlds.append(w)
    assert all(len(P.lane_layout(w)[0]) >= 60 for w in worlds)
    res = check(orbx, big, worlds, frames=frames, sets=sets)
    assert res[0]["status"] == 0 and res[0]["n_correspondences"] == 450 and res[0]["n_bad"] == 50
    assert res[0].tobytes() != res[2].tobytes() and res[0].tobytes() != res[3].tobytes()


# ---- failed 6x6 solves (tests/test_pose_host.py: test_a_table_of_zeros_fails_every_solve,
# test_solves_fail_once_every_weighted_edge_is_flagged).  A call has one table, so each table has a call of its own ----

def test_every_solve_fails_under_a_table_of_zeros(orbx, big, sized):
    """Hpp = 0, lambda = 0: forty failed solves per problem, next to a problem of one round.  Two of the problems walk edges
    behind the cache with ok == 0, but a weightless edge adds 0 to every sum: this test cannot tell whether that loop ran
    (test_solves_fail_behind_accepted_trials can)."""
    worlds = [P.world("far").padded(BIG), P.world("no_weight").padded(BIG), P.world("no_weight_big"), sized[9].padded(BIG),
              P.world("cache_full")]
    res = check(orbx, big, worlds, inv_sigma2=P.zero_table())
    assert list(res["status"]) == [0] * 5 and list(res["solver_failures"]) == [40, 40, 40, 10, 40]
    assert list(res["lm_trials"]) == list(res["rejected_trials"]) == [40, 40, 40, 10, 40]
    assert not res["n_bad"].any() and not res["chi2_initial"].any() and not res["lambda"].any()
    for p in range(5):
        assert list(res[p]["iterations"]) == ([1, 0, 0, 0] if p == 3 else [1, 1, 1, 1])
        assert res[p]["tcw"].tobytes() == worlds[p].pose0[9:].tobytes()


def test_solves_fail_behind_accepted_trials(orbx, big, sized):
    """weight_lost and weight_lost_big between clean and far, all under the table that weighs level 0 alone: in the two the
    solves fail from round 1 on, with flags set (behind the cache too); the other three keep weighted edges and solve."""
    names = ("clean", "weight_lost", "cache_edge", "weight_lost_big", "far")
    worlds = [P.world(name).padded(BIG) for name in names]
    res = check(orbx, big, worlds, inv_sigma2=P.level0_table())
    assert list(res["status"]) == [0] * 5 and list(res["solver_failures"]) == [0, 30, 0, 30, 0]
    for p, gross in ((1, 100), (3, 420)):
        assert res[p]["n_bad"] == gross and res[p]["lm_trials"] > res[p]["solver_failures"]
        assert res[p]["iterations"][0] > 1 and list(res[p]["iterations"][1:]) == [1, 1, 1]


# Whether test_chained_from_images' two problems hold an edge behind the cache: what the image pair happens to give, recorded here
# so that the test says what it covers (the worlds above are what covers the cache on purpose).
CHAINED_LEAVES_THE_CACHE = [True, True]


def test_chained_from_images(orbx, images, golden):
    """extract -> bow transform -> SearchByBoW -> PoseOptimization from two images, every stage reading what the stage before left
    on the device: a keyframe and a frame that is its copy shifted by (5, 3) pixels.  The keyframe's map points lie on the plane
    z = 8 under its keypoints (computed on the device from the extractor's array), so the frame's true pose is the identity
    rotation and a step parallel to the plane.  The match rows go from the matcher to the optimiser as they are.  Compared with
    the restatement fed the downloaded arrays."""
    import torch
    import bow_ref_lib as R
    a = images["dbow0"]
    b = np.roll(a, (3, 5), axis=(0, 1))
    h, wd = a.shape
    cap, B = 1024, 2
    K = np.array([[520.0, 0, wd / 2], [0, 520.0, h / 2], [0, 0, 1]], np.float32)
    base = R.full_vocabulary(golden["canonical/dbow0/desc"], k=10, L=3)
    e = orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=wd, max_height=h, max_batch=B, device=0)
    voc = orbx.Vocabulary.from_arrays(e, *base.arrays())
    z = lambda dt, m: torch.zeros(m, dtype=dt, device="cuda")  # noqa: E731
    d_img = torch.from_numpy(np.stack([a, b])).cuda()
    d_k, d_d, d_n = z(torch.uint8, B * cap * 28), z(torch.uint8, B * cap * 32), z(torch.int32, B)
    fv_node, fv_feat, fv_n = z(torch.int32, B * cap), z(torch.int32, B * cap), z(torch.int32, B)
    m, nm = torch.full((2 * cap,), -7, dtype=torch.int32, device="cuda"), z(torch.int32, 2)
    kf, fr = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    e.extract_batch_device(d_img, B, wd, h, wd, wd * h, d_k, d_d, d_n, cap)
    voc.transform_batch_device(B, d_d, d_n, z(torch.int32, B * cap), z(torch.float64, B * cap), z(torch.int32, B), fv_node, fv_feat, fv_n,
                               levelsup=2, capacity=cap)
    e.match_bow_pairs_device(B, kf, fr, d_k, d_d, d_n, fv_node, fv_feat, fv_n, m, nm, nnratio=0.7, checkOri=True, capacity=cap)
    # every frame's map points: its keypoints lifted to the plane z = 8 (set f = frame f as a keyframe)
    xy = d_k.view(torch.float32).reshape(B, cap, 7)[:, :, :2]
    d_pts = torch.stack([(xy[:, :, 0] - K[0, 2]) / K[0, 0] * 8, (xy[:, :, 1] - K[1, 2]) / K[1, 1] * 8, torch.full_like(xy[:, :, 0], 8.0)],
                        dim=2).contiguous()
    step = np.array([5 * 8 / 520.0, 3 * 8 / 520.0, 0.0])
    start = P.rotvec([0.01, -0.015, 0.02])
    pose0 = np.stack([np.r_[start.reshape(9), start @ step * 1.05 + 0.02], np.r_[start.reshape(9), start @ -step * 1.05 - 0.02]]).astype(np.float32)
    d_pose = torch.from_numpy(pose0).cuda()
    d_res, d_out = z(torch.uint8, 2 * orbx.POSE_RESULT_DTYPE.itemsize), z(torch.uint8, 2 * cap)
    e.pose_optimize_batch_device(B, fr, kf, d_k, d_n, m, B, d_pts, None, d_pose, K, d_res, d_out, capacity=cap)
    torch.cuda.synchronize()
    kps, n = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap), d_n.cpu().numpy()
    match, pts = m.cpu().numpy().reshape(2, cap), d_pts.cpu().numpy()
    res, flags = d_res.cpu().numpy().view(orbx.POSE_RESULT_DTYPE), d_out.cpu().numpy().reshape(2, cap)
    table = e.GetInverseScaleSigmaSquares()
    leaves_the_cache = []
    for p in range(2):
        w = P.World(kps[fr[p]].copy(), n[fr[p]], match[p].copy(), pts[kf[p]].copy(), None, pose0[p], K.reshape(9))
        r, rf, _, _ = P.pose_optimize(w, inv_sigma2=table)
        same(res[p], flags[p], r, rf, "problem %d" % p)
        true_t = step if p == 0 else -step
        print("chained: %d matches, status %d, %d correspondences, %d inliers, iterations %s, t %s (true %s)" %
              (nm[p].item(), res[p]["status"], res[p]["n_correspondences"], res[p]["n_inliers"], res[p]["iterations"], res[p]["tcw"], true_t))
        assert res[p]["status"] == 0 and res[p]["n_correspondences"] == (match[p, :n[fr[p]]] >= 0).sum() >= 50
        assert res[p]["n_inliers"] * 2 > res[p]["n_correspondences"]
        assert np.linalg.norm(res[p]["tcw"] - true_t) < np.linalg.norm(pose0[p, 9:] - true_t)
        behind, per_lane, _, _ = P.lane_layout(w)
        print("chained: problem %d has %d lanes with more than six correspondences, %d edges behind the cache" %
              (p, (per_lane > P.LANE_CACHE).sum(), len(behind)))
        leaves_the_cache.append(len(behind) > 0)
    assert leaves_the_cache == CHAINED_LEAVES_THE_CACHE
    voc.close()
    e.close()


def test_shim_pose_agrees_with_the_c_abi(orbx, tmp_path):
    """tests/cpp/shim_pose.cpp: Optimizer::PoseOptimization of the C++ shim gives the bytes of orbx_pose_optimize."""
    from test_pose_host import build_shim_pose
    exe = build_shim_pose(orbx, tmp_path)
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    status, inliers, n, flagged, agrees = (int(v) for v in [l for l in p.stdout.splitlines() if l.startswith("RESULT")][0].split()[1:])
    assert agrees == 1 and status == 0 and n == 150 and flagged == 12 and inliers == 138
