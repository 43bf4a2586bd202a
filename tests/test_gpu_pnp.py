"""PnPsolver on the device (orbx_pnp_solve / orbx_pnp_solve_batch_device) equals the CPU restatement tests/cpp/pnp_ref.cpp BIT FOR
BIT: every field of orbx_pnp_result, the bytes of its f64 included, the pose, the row of inlier matches and every flag byte.
Both sides share the arithmetic, fix the same order of Refine's sums and contract nothing (include/orbx.h).  What the
restatement itself is worth is tests/test_pnp_host.py's business, which also shows which branches the worlds used here run."""
import subprocess

import numpy as np
import pytest

import pnp_ref_lib as Q
import pose_ref_lib as P
from test_pnp_host import GARBAGE, _worlds, bad

pytestmark = pytest.mark.gpu

# correspondences per problem: bNoMore (3, 4, 9), every clamp of the table (10: one iteration, 11, 20), the wave edge of the
# strided sums (63, 64, 65) and beyond two strides (200)
COUNTS = (3, 4, 9, 10, 11, 20, 63, 64, 65, 200)
CAP = 256


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, Q.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sized():
    """A world per count of COUNTS with 0.5 sigma of noise, a fifth of them gross mismatches from 20 correspondences on."""
    return {n: (Q.make_world(n, 400 + k, cap=CAP, outliers=(n // 5 if n >= 20 else 0), noise=0.5 if n >= 20 else 0.0),
                Q.make_draws(35, 400 + k)) for k, n in enumerate(COUNTS)}


@pytest.fixture(scope="module")
def branch():
    return {name: (w.padded(CAP), d) for name, (w, d) in _worlds().items()}


def with_match(w):
    """The same problem through a match row: feature j names entry j."""
    q = w.copy()
    if q.match is None:
        n = max(min(q.n, q.cap), 0)
        q.match = np.full(q.cap, -1, np.int32)
        q.match[:n] = np.arange(n)
    return q


def run_batch(orbx, ext, worlds, draws, frames=None, sets=None, sigma2=None, want_flags=True, **params):
    """The worlds as one device batch -> (results [P], poses [P, 12], rows [P, cap], flags [P, cap] or None).  By default problem
    p has frame p and point set p of its own; frames / sets: lists of (kps, n) / (points, mask) rows and the worlds name them by
    their attributes frame / point_set.  draws [P, n_iter, 4]."""
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
    draws = np.ascontiguousarray(draws, np.int32)
    assert draws.shape[0] == Pn and draws.shape[2] == 4
    d_draws = d(draws)
    fill = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_res, d_pose, d_row = fill(Pn * orbx.PNP_RESULT_DTYPE.itemsize), fill(Pn * 48), fill(Pn * cap * 4)
    d_fl = fill(Pn * cap) if want_flags else None
    ext.pnp_solve_batch_device(len(frames), fi, si, d_k, d_n, d_m, len(sets), d_p, d_mask, worlds[0].K, d_draws, d_res, d_pose, d_row,
                               d_fl, sigma2=sigma2, n_iter=draws.shape[1], capacity=cap, **params)
    torch.cuda.synchronize()
    return (d_res.cpu().numpy().view(orbx.PNP_RESULT_DTYPE), d_pose.cpu().numpy().view(np.float32).reshape(Pn, 12),
            d_row.cpu().numpy().view(np.int32).reshape(Pn, cap), d_fl.cpu().numpy().reshape(Pn, cap) if want_flags else None)


def same(got, ref, what=""):
    """Bit for bit: the record's bytes field by field (so that a difference names its field), the pose, the row, the flags."""
    res, pose, row, flags = got
    r, rpose, rrow, rflags = ref
    for f in Q.PNP_RESULT_DTYPE.names:
        assert np.asarray(res[f]).tobytes() == np.asarray(r[f]).tobytes(), (what, f, res[f], r[f])
    assert pose.tobytes() == rpose.tobytes(), what
    assert row.tobytes() == rrow.tobytes(), what
    if flags is not None:
        assert flags.tobytes() == rflags.tobytes(), what


def check(orbx, ext, pairs, sigma2=None, **kw):
    """pairs: (world, draws) per problem, draws of one length."""
    worlds, draws = [w for w, _ in pairs], np.stack([d for _, d in pairs])
    ref_kw = {k: v for k, v in kw.items() if k in Q.PARAMS}
    res, pose, row, flags = run_batch(orbx, ext, worlds, draws, sigma2=sigma2, **kw)
    for p, (w, d) in enumerate(pairs):
        same((res[p], pose[p], row[p], None if flags is None else flags[p]), Q.solve(w, d, 0, sigma2=sigma2, **ref_kw), "problem %d" % p)
    return res


@pytest.mark.parametrize("n", COUNTS)
def test_one_problem_of_each_size(orbx, ext, sized, n):
    res = check(orbx, ext, [sized[n]])
    assert res[0]["n_correspondences"] == n
    if n < 10:
        assert res[0]["status"] == Q.FEW_POINTS | Q.NO_POSE and res[0]["its_run"] == 0
    else:
        assert res[0]["max_its"] == {10: 1, 11: 4}.get(n, 35)
    if n >= 20:
        assert res[0]["status"] == 0 and res[0]["refined"] == 1 and res[0]["n_inliers"] > res[0]["min_inliers"]


def test_all_sizes_in_one_batch(orbx, ext, sized):
    res = check(orbx, ext, [sized[n] for n in COUNTS])
    assert list(res["n_correspondences"]) == list(COUNTS)


# 70 % gross mismatches, minInliers 10 and epsilon 0.25 (293 iterations): a clean draw is rare, so late iterations decide
HARD = dict(min_inliers=10, epsilon=0.25)


@pytest.mark.parametrize("n_iter", [1, 35, 64, 65, 300])
def test_partial_and_full_waves_of_hypotheses(orbx, ext, n_iter):
    pairs = [(Q.make_world(60, 500 + k, cap=CAP, outliers=42, noise=0.3), Q.make_draws(n_iter, 500 + k)) for k in range(3)]
    res = check(orbx, ext, pairs, **HARD)
    assert (res["max_its"] == 293).all() and (res["its_run"] <= min(n_iter, 293)).all()
    if n_iter == 300:
        assert (res["its_run"] > 65).any() and (res["refined"] == 1).any()
        one = check(orbx, ext, pairs[:1], **HARD)  # one problem: the grid's last wave is partial in another place
        assert one[0].tobytes() == res[0].tobytes()


def test_each_branch_world(orbx, ext, ext2, branch):
    """The host test's worlds, grouped by what a batch shares; those of the second setting (named @2) on its context, under its
    table."""
    by_len = {}
    for name, (w, d) in branch.items():
        by_len.setdefault((len(d), name.endswith("@2")), []).append((name, with_match(w), d))
    seen = {}
    for (n_iter, second), group in by_len.items():
        if second:
            res = check(orbx, ext2, [(w, d) for _, w, d in group], sigma2=Q.sigma2_table(Q.NLEVELS_2, Q.SCALE_FACTOR_2))
        else:
            res = check(orbx, ext, [(w, d) for _, w, d in group])
        seen.update({name: res[k] for k, (name, _, _) in enumerate(group)})
    assert seen["unrefined"]["refined"] == 0 and seen["unrefined"]["found_it"] == -1 and seen["unrefined"]["n_inliers"] == 10
    assert seen["second_try"]["n_refines"] >= 2 and seen["second_try"]["refined"] == 1
    assert seen["same_point"]["n_degenerate"] > 0 and seen["collinear"]["n_degenerate"] > 0
    assert {1, 2, 3} <= {int(r["beta_choice"]) for r in seen.values()}
    assert np.isfinite(seen["planar"]["R"]).all()


def test_each_garbage_kind_next_to_a_clean_problem(orbx, ext, sized):
    w, d = sized[65]
    clean = (with_match(sized[200][0]), sized[200][1])
    pairs = [clean] + [(with_match(bad(w, what)), d) for what, _ in GARBAGE]
    res = check(orbx, ext, pairs)
    assert list(res["status"]) == [0] + [bit | Q.NO_POSE for _, bit in GARBAGE]
    alone = check(orbx, ext, [clean])
    assert alone[0].tobytes() == res[0].tobytes()
    d2 = sized[200][1].copy()
    d2[0, 1] = -1
    res = check(orbx, ext, [clean, (clean[0], d2)])
    assert list(res["status"]) == [0, Q.BAD_DRAWS]


def test_one_frame_against_five_point_sets(orbx, ext):
    """The relocaliser's shape: one frame, five candidate keyframes' map points; the candidates differ in how many of the
    frame's features they explain."""
    base = Q.make_world(150, 600, cap=CAP, outliers=20, noise=0.5, extra=0)
    frames, sets, worlds, draws = [(base.kps, base.n)], [], [], []
    rng = np.random.default_rng(600)
    for s in range(5):
        q = base.copy()
        drop = rng.permutation(base.n)[:s * 30]  # candidate s lacks s * 30 of the points
        q.mask[drop] = 0
        if s == 4:
            q.points[:] = rng.normal(0, 5, q.points.shape).astype(np.float32)  # a wrong candidate: no pose
        q.frame, q.point_set = 0, s
        sets.append((q.points, q.mask))
        worlds.append(q)
        draws.append(Q.make_draws(35, 600 + s))
    got = run_batch(orbx, ext, worlds, np.stack(draws), frames=frames, sets=sets)
    for p, w in enumerate(worlds):
        same(tuple(a[p] for a in got), Q.solve(w, draws[p], 0), "candidate %d" % p)
    assert list(got[0]["n_correspondences"]) == [150, 120, 90, 60, 30]
    assert (got[0]["refined"][:4] == 1).all() and got[0]["status"][4] & Q.NO_POSE


def test_match_form_against_the_direct_form(orbx, ext, sized):
    w, d = sized[200]
    direct = run_batch(orbx, ext, [w], d[None])
    through = run_batch(orbx, ext, [with_match(w)], d[None])
    for a, b in zip(direct, through):
        assert a.tobytes() == b.tobytes()
    m = Q.make_world(150, 2, cap=CAP, outliers=30, noise=0.5, matched=True)  # a permuted point set of its own
    res = check(orbx, ext, [(m, d)])
    assert res[0]["refined"] == 1


def test_without_a_mask_without_flags_and_with_the_contexts_table(orbx, ext, sized):
    w = Q.make_world(100, 610, cap=105, outliers=20, noise=0.5, extra=0, use_mask=False)
    w.n = 100
    d = Q.make_draws(35, 610)
    a = check(orbx, ext, [(w, d)])
    b = check(orbx, ext, [(w, d)], want_flags=False)
    c = check(orbx, ext, [(w, d)], sigma2=Q.sigma2_table())
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[0]["refined"] == 1
    assert np.array_equal(Q.sigma2_table(), ext.GetScaleSigmaSquares())
    other = (Q.sigma2_table() * np.float32(0.25)).astype(np.float32)  # a tighter table changes the answer
    e = check(orbx, ext, [(w, d)], sigma2=other)
    assert e[0]["n_inliers"] < a[0]["n_inliers"]


def test_capacity_1024_with_700_correspondences(orbx, ext):
    w = Q.make_world(700, 620, cap=1024, outliers=140, noise=0.5)
    res = check(orbx, ext, [(w, Q.make_draws(35, 620))])
    assert res[0]["n_correspondences"] == 700 and res[0]["min_inliers"] == 350 and res[0]["refined"] == 1


def test_the_largest_capacity(orbx, ext):
    """One problem at capacity ORBX_BOW_MAX_FEATURES: it sizes the inlier bit sets, whose LDS lies beside V."""
    w = Q.make_world(300, 630, cap=16384, outliers=60, noise=0.5, matched=True)
    rng = np.random.default_rng(630)
    # spread the frame's features over the whole capacity: feature j moves to a random slot, ascending
    slots = np.sort(rng.permutation(16384)[:w.n])
    q = w.copy()
    q.kps[:] = 0
    q.match[:] = -1
    q.kps[slots], q.match[slots], q.n = w.kps[:w.n], w.match[:w.n], 16384
    res = check(orbx, ext, [(q, Q.make_draws(35, 630))])
    assert res[0]["n_correspondences"] == 300 and res[0]["refined"] == 1


def test_lists_and_table_held_across_calls(orbx, sized):
    e = orbx.ORBextractor(1000, 1.2, Q.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    a, b = (with_match(sized[200][0]), sized[200][1]), (with_match(sized[65][0]), sized[65][1])
    first = check(orbx, e, [a, b])
    again = check(orbx, e, [a, b])  # the same call twice
    assert first.tobytes() == again.tobytes()
    swapped = check(orbx, e, [b, a])  # (same lists, other data)
    assert swapped[1].tobytes() == first[0].tobytes()
    # a changed list: both problems on frame 0 / set 0
    q0, q1 = a[0].copy(), a[0].copy()
    q0.frame = q0.point_set = q1.frame = q1.point_set = 0
    got = run_batch(orbx, e, [q0, q1], np.stack([a[1], b[1]]), frames=[(a[0].kps, a[0].n), (b[0].kps, b[0].n)],
                    sets=[(a[0].points, a[0].mask), (b[0].points, b[0].mask)])
    same(tuple(x[0] for x in got), Q.solve(a[0], a[1], 0))
    same(tuple(x[1] for x in got), Q.solve(a[0], b[1], 0))
    # a changed parameter, then the first again
    loose = check(orbx, e, [a, b], epsilon=0.3, min_inliers=12)
    assert loose[0]["min_inliers"] == 60 and loose[1]["min_inliers"] == 19
    back = check(orbx, e, [a, b])
    assert back.tobytes() == first.tobytes()
    e.close()


def test_host_form_equals_a_batch_of_one(orbx, ext, sized):
    for n in (9, 65, 200):
        w, d = sized[n]
        res, inl = ext.pnp_solve(w.kps[:w.n], w.points[:w.n], w.mask[:w.n], w.K, d)
        got = run_batch(orbx, ext, [w], d[None])
        assert bytes(res) == got[0][0].tobytes()
        assert np.array_equal(inl, got[3][0][:w.n] != 0)
        r = Q.solve(w, d, 0)
        assert bytes(res) == r[0].tobytes()


# ---- the second setting (pose_ref_lib.SECOND): fx != fy, a context of 5 levels of 1.37, a true pose rolled by 89 degrees ----

CAP_2 = 263  # just above the larger frame (257 correspondences + 5 other features)


@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, Q.SCALE_FACTOR_2, Q.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


def test_second_setting_anisotropic_camera_and_five_levels(orbx, ext2):
    """Two problems (65 and 257 correspondences, a fifth gross mismatches, 0.5 sigma of noise) under K_ANISO: once with the
    context's own table, once with the same table given explicitly; then the host form and PnPsolver on the smaller one."""
    pairs = [(Q.make_world(n, 440 + k, cap=CAP_2, outliers=n // 5, noise=0.5, motion=Q.MOTION_2, **Q.SECOND), Q.make_draws(35, 440 + k))
             for k, n in enumerate((65, 257))]
    table = Q.sigma2_table(Q.NLEVELS_2, Q.SCALE_FACTOR_2)
    assert ext2.GetScaleSigmaSquares().tobytes() == table.tobytes() and len(table) == Q.NLEVELS_2
    worlds, draws = [w for w, _ in pairs], np.stack([d for _, d in pairs])
    res, pose, row, flags = run_batch(orbx, ext2, worlds, draws)  # (the context's table)
    for p, (w, d) in enumerate(pairs):
        same((res[p], pose[p], row[p], flags[p]), Q.solve(w, d, 0, sigma2=table), "context's table, problem %d" % p)
    res2 = check(orbx, ext2, pairs, sigma2=table)
    assert res2.tobytes() == res.tobytes()
    for p, n in enumerate((65, 257)):  # not trivial: refined over more inliers than the minimum, no planted mismatch among them
        assert res[p]["status"] == 0 and res[p]["refined"] == 1 and res[p]["n_correspondences"] == n
        assert res[p]["n_inliers"] > res[p]["min_inliers"] and res[p]["n_inliers"] >= (n - n // 5) * 3 // 4
        assert not flags[p][worlds[p].truth["bad"]].any()
    w, d = pairs[0]
    one, inl = ext2.pnp_solve(w.kps[:w.n], w.points[:w.n], w.mask[:w.n], w.K, d)
    assert bytes(one) == res[0].tobytes() and np.array_equal(inl, flags[0][:w.n] != 0)
    it = iter(d.reshape(-1).tolist() + [0] * (4 * 300))
    s = orbx.PnPsolver(_Frame(w, ext2), w.points[:w.n], w.mask[:w.n], w.K.reshape(3, 3), rand=lambda: next(it))
    s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    d300 = np.zeros((300, 4), np.int32)
    d300[:35] = d
    ref = Q.solve(w, d300, 0, sigma2=table)
    T, inl, n, r = s.find()
    assert bytes(r) == ref[0].tobytes() and n == ref[0]["n_inliers"] and np.array_equal(inl, ref[3][:w.n] != 0)
    assert T[:3, :3].astype(np.float32).tobytes() == ref[1][:9].tobytes() and T[:3, 3].tobytes() == ref[1][9:].tobytes()


class _Frame:
    """What PnPsolver reads of a Frame."""

    def __init__(self, w, ext):
        self.mvKeysUn, self.mpORBextractor, self.camera = w.kps[:w.n], ext, None


def test_python_pnpsolver(orbx, ext, sized):
    w, d = sized[200]
    it = iter(d.reshape(-1).tolist() + [0] * (4 * 300))
    s = orbx.PnPsolver(_Frame(w, ext), w.points[:w.n], w.mask[:w.n], w.K.reshape(3, 3), rand=lambda: next(it))
    s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    d300 = np.zeros((300, 4), np.int32)
    d300[:35] = d
    ref = Q.solve(w, d300, 0)
    T, inl, n, res = s.find()
    assert bytes(res) == ref[0].tobytes() and n == ref[0]["n_inliers"] and np.array_equal(inl, ref[3][:w.n] != 0)
    assert T[:3, :3].astype(np.float32).tobytes() == ref[1][:9].tobytes() and T[:3, 3].tobytes() == ref[1][9:].tobytes()
    # iterate(5) in turns: the pose comes in the turn found_it falls into
    it = iter(d.reshape(-1).tolist() + [0] * (4 * 300))
    s = orbx.PnPsolver(_Frame(w, ext), w.points[:w.n], w.mask[:w.n], w.K.reshape(3, 3), rand=lambda: next(it))
    s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    turns = 0
    while True:
        T2, no_more, inl2, n2, _ = s.iterate(5)
        turns += 1
        if T2 is not None or no_more:
            break
    assert turns == ref[0]["found_it"] // 5 + 1 and np.array_equal(T2, T) and n2 == n and not no_more
    # a match row instead of a mask
    m = with_match(w)
    it = iter(d.reshape(-1).tolist() + [0] * (4 * 300))
    s = orbx.PnPsolver(_Frame(w, ext), w.points, np.where(w.mask[:w.n] != 0, m.match[:w.n], -1), w.K.reshape(3, 3), rand=lambda: next(it))
    s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    assert np.array_equal(s.find()[0], T)


def test_chained_from_images(orbx, images, golden):
    """extract -> bow transform -> SearchByBoW -> PnP -> PoseOptimization from two images with no copy between: a keyframe and
    a frame that is its copy shifted by (5, 3) pixels.  The keyframe's map points lie under its keypoints on a gently curved
    surface around z = 8 (EPnP needs points out of a plane), computed on the device from the extractor's array.  The PnP call's
    d_pose and d_match_inliers go to the pose call as its d_pose0 and d_match, as they are.  Compared with match rows ->
    pnp_ref -> pose_ref on the downloaded arrays."""
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
    kf, fr = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    draws = np.stack([Q.make_draws(n_iter, 700), Q.make_draws(n_iter, 701)])
    d_draws = torch.from_numpy(draws).cuda()
    e.extract_batch_device(d_img, B, wd, h, wd, wd * h, d_k, d_d, d_n, cap)
    voc.transform_batch_device(B, d_d, d_n, z(torch.int32, B * cap), z(torch.float64, B * cap), z(torch.int32, B), fv_node, fv_feat, fv_n,
                               levelsup=2, capacity=cap)
    e.match_bow_pairs_device(B, kf, fr, d_k, d_d, d_n, fv_node, fv_feat, fv_n, m, nm, nnratio=0.7, checkOri=True, capacity=cap)
    xy = d_k.view(torch.float32).reshape(B, cap, 7)[:, :, :2]
    depth = 8.0 + 0.8 * torch.sin(xy[:, :, 0] / 40.0) * torch.cos(xy[:, :, 1] / 30.0)
    d_pts = torch.stack([(xy[:, :, 0] - K[0, 2]) / K[0, 0] * depth, (xy[:, :, 1] - K[1, 2]) / K[1, 1] * depth, depth], dim=2).contiguous()
    d_pres, d_pose, d_row = z(torch.uint8, 2 * orbx.PNP_RESULT_DTYPE.itemsize), z(torch.float32, 2 * 12), z(torch.int32, 2 * cap)
    e.pnp_solve_batch_device(B, fr, kf, d_k, d_n, m, B, d_pts, None, K, d_draws, d_pres, d_pose, d_row, None, capacity=cap)
    d_res, d_out = z(torch.uint8, 2 * orbx.POSE_RESULT_DTYPE.itemsize), z(torch.uint8, 2 * cap)
    e.pose_optimize_batch_device(B, fr, kf, d_k, d_n, d_row, B, d_pts, None, d_pose, K, d_res, d_out, capacity=cap)
    torch.cuda.synchronize()
    kps, n = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(B, cap), d_n.cpu().numpy()
    match, pts = m.cpu().numpy().reshape(2, cap), d_pts.cpu().numpy()
    pres, pose, row = d_pres.cpu().numpy().view(orbx.PNP_RESULT_DTYPE), d_pose.cpu().numpy().reshape(2, 12), d_row.cpu().numpy().reshape(2, cap)
    res, flags = d_res.cpu().numpy().view(orbx.POSE_RESULT_DTYPE), d_out.cpu().numpy().reshape(2, cap)
    step = np.array([5 * 8 / 520.0, 3 * 8 / 520.0, 0.0])
    for p in range(2):
        w = P.World(kps[fr[p]].copy(), n[fr[p]], match[p].copy(), pts[kf[p]].copy(), None, np.zeros(12, np.float32), K.reshape(9))
        ref = Q.solve(w, draws[p], 0, sigma2=e.GetScaleSigmaSquares())
        same((pres[p], pose[p], row[p], None), ref, "pnp %d" % p)
        w2 = P.World(w.kps, w.n, ref[2].copy(), w.points, None, ref[1].copy(), w.K)
        r, rf, _, _ = P.pose_optimize(w2, inv_sigma2=e.GetInverseScaleSigmaSquares())
        for f in P.POSE_RESULT_DTYPE.names:
            assert np.asarray(res[p][f]).tobytes() == np.asarray(r[f]).tobytes(), (p, f)
        assert flags[p].tobytes() == rf.tobytes()
        print("chained: %d matches, pnp status %d, N %d, found_it %d, %d inliers; pose: %d inliers, t %s (about %s)" %
              (nm[p].item(), pres[p]["status"], pres[p]["n_correspondences"], pres[p]["found_it"], pres[p]["n_inliers"],
               res[p]["n_inliers"], res[p]["tcw"], step if p == 0 else -step))
        assert pres[p]["status"] == 0 and pres[p]["n_correspondences"] >= 50 and pres[p]["n_inliers"] >= pres[p]["min_inliers"]
        assert res[p]["status"] == 0 and res[p]["n_correspondences"] == pres[p]["n_inliers"]
    voc.close()
    e.close()


def test_shim_pnp_agrees_with_the_c_abi(orbx, tmp_path):
    """tests/cpp/shim_pnp.cpp: PnPsolver of the C++ shim, iterate(5) in turns, gives the bytes of orbx_pnp_solve, and the pose
    arrives in found_it's turn."""
    from test_pnp_host import build_shim_pnp
    exe = build_shim_pnp(orbx, tmp_path)
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    status, inliers, n, wrong, turns, agrees = (int(v) for v in [l for l in p.stdout.splitlines() if l.startswith("RESULT")][0].split()[1:])
    assert agrees == 1 and status == 0 and n == 150 and wrong == 0 and inliers == 120 and turns >= 1
