"""Optimizer::OptimizeSim3 on the device (orbx_optimize_sim3 / orbx_optimize_sim3_batch_device) equals the CPU restatement
tests/cpp/sim3opt_ref.cpp BYTE FOR BYTE: every field of orbx_sim3opt_result (the f64 bytes included), d_sim3_out and the whole
row.  Both sides share the arithmetic and contract nothing (include/orbx.h).  What the restatement itself is worth is
tests/test_sim3opt_host.py's business."""
import subprocess

import numpy as np
import pytest

import sim3opt_ref_lib as S
from test_sim3opt_host import _exact, _move, build_shim_sim3opt, garbage_kinds, spoiled

pytestmark = pytest.mark.gpu

# correspondences per problem: none, one, the `< 10` rule from both sides (9, 10, 11), a wave's edge (63, 64, 65: a lane with
# none, one and two), two full rounds of lanes and one more (129) and several per lane (300)
COUNTS = (0, 1, 9, 10, 11, 63, 64, 65, 129, 300)
CAP = 320


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, S.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sized():
    """A world per count of COUNTS; from 20 correspondences on with 0.3 sigma of noise and a tenth gross mismatches."""
    return {n: S.sized_world(n, 600 + k, cap=CAP) for k, n in enumerate(COUNTS)}


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
                   w.pose1.copy(), w.pose2.copy(), w.sim.copy(), w.K, w.truth)


def run_batch(orbx, ext, worlds, frames=None, lists=None, inv_sigma2=None, in_place=True, **params):
    """The worlds as one device batch -> (results [P], sims [P, 13], rows [P, cap]).  By default problem p has keyframes and point
    sets 2 p and 2 p + 1 of its own; frames: a list of (kps, n, points, mask, pose) rows -- keyframe k and point set k -- and
    lists = (kf1, kf2, set1, set2) name them.  in_place: d_sim3_out is d_sim3."""
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
    d_row, d_sim = d(np.stack([w.match for w in worlds])), d(np.stack([w.sim for w in worlds]))
    fill = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_res = fill(Pn * orbx.SIM3OPT_RESULT_DTYPE.itemsize)
    d_out = None if in_place else fill(Pn * 52)
    ext.optimize_sim3_pairs_device(len(frames), lists[0], lists[1], lists[2], lists[3], d_k, d_n, d_row, len(frames), d_p, d_mask, d_pose,
                                   d_sim, worlds[0].K, d_res, d_out, inv_sigma2=inv_sigma2, capacity=cap, **params)
    torch.cuda.synchronize()
    if not in_place:  # the input similarity is only read
        assert d_sim.cpu().numpy().tobytes() == np.stack([w.sim for w in worlds]).tobytes()
    out = d_sim if in_place else d_out
    return (d_res.cpu().numpy().view(orbx.SIM3OPT_RESULT_DTYPE), out.cpu().numpy().view(np.float32).reshape(Pn, 13),
            d_row.cpu().numpy().view(np.int32).reshape(Pn, cap))


def same(got, ref, what=""):
    """Byte for byte: the record field by field (so that a difference names its field), the similarity, the row."""
    res, sim, row = got
    r, rsim, rrow = ref[:3]
    for f in S.SIM3OPT_RESULT_DTYPE.names:
        assert np.asarray(res[f]).tobytes() == np.asarray(r[f]).tobytes(), (what, f, res[f], r[f])
    assert sim.tobytes() == rsim.tobytes(), what
    assert row.tobytes() == rrow.tobytes(), what


def check(orbx, ext, worlds, inv_sigma2=None, nlevels=S.NLEVELS, in_place=True, context_table=None, **kw):
    """context_table: the table the restatement is given where the device is given none and uses its context's own."""
    res, sim, row = run_batch(orbx, ext, worlds, inv_sigma2=inv_sigma2, in_place=in_place, **kw)
    ref_table = inv_sigma2 if inv_sigma2 is not None else context_table
    for p, w in enumerate(worlds):
        same((res[p], sim[p], row[p]), S.optimize(w, inv_sigma2=ref_table, nlevels=nlevels, **kw), "problem %d" % p)
    return res


@pytest.mark.parametrize("n", COUNTS)
def test_one_problem_of_each_size(orbx, ext, sized, n):
    res = check(orbx, ext, [sized[n]])
    assert res[0]["status"] == 0 and res[0]["n_correspondences"] == n
    assert res[0]["rounds"] == (0 if n == 0 else 1 if n < 10 else 2)
    if n >= 10:
        assert res[0]["n_inliers"] == n - (n // 10 if n >= 20 else 0)


def test_all_sizes_in_one_batch(orbx, ext, sized):
    res = check(orbx, ext, [sized[n] for n in COUNTS])
    assert list(res["n_correspondences"]) == list(COUNTS)


@pytest.mark.parametrize("n_left", [9, 10])
def test_the_ten_rule_after_removals(orbx, ext, n_left):
    w = _exact(14)
    for k in range(14 - n_left):
        _move(w, k, 30.0)
    w.sim = S.sim_row(w.truth["s"] * 1.001, w.truth["R"], w.truth["t"])
    res = check(orbx, ext, [w])
    assert res[0]["n_bad"] == 14 - n_left and res[0]["rounds"] == (2 if n_left == 10 else 1)


def mixture(sized):
    """Nine problems: refused, empty, return-0, nBad == 0 and nBad > 0, in an order that puts a different kind at every
    workgroup position."""
    refused = spoiled("s_zero", "mixed")[0]
    nobad = S.make_world(40, 640, cap=CAP, noise=0.05)
    few = sized[9]
    return [padded(refused, CAP), sized[0], few, nobad, sized[129], sized[300], padded(spoiled("row_beyond_n2", "mixed")[0], CAP),
            sized[65], sized[10]]


@pytest.mark.parametrize("n_problems", [1, 3, 4, 5, 9])
def test_problems_per_call_across_the_workgroup_edge(orbx, ext, sized, n_problems):
    worlds = mixture(sized)[:n_problems]
    res = check(orbx, ext, worlds)
    if n_problems == 9:
        assert res[0]["status"] == S.NONFINITE and res[6]["status"] == S.BAD_INPUT
        assert res[1]["rounds"] == 0 and res[2]["rounds"] == 1 and res[2]["n_inliers"] == 0
        assert res[3]["n_bad"] == 0 and res[3]["rounds"] == 2 and res[4]["n_bad"] > 0 and res[5]["n_bad"] > 0


def test_shared_keyframes_and_a_keyframe_against_itself(orbx, ext, sized):
    """Two keyframes in four problems: keyframe 0 with its point set is KF1 of three problems (two of them the same problem, one
    with a thinner row and another start) and both sides of the fourth, a keyframe against itself under the identity."""
    a = sized[129]
    b = a.copy()
    b.match[a.truth["slots1"][::7]] = -1
    b.sim = S.sim_row(a.truth["s"] * 0.98, a.truth["R"], a.truth["t"] * 1.01)
    self_w = S.World(a.kps1, a.n1, a.kps1, a.n1, np.where(a.mask1 != 0, np.arange(a.cap), -1).astype(np.int32), a.points1, a.mask1,
                     a.points1, a.mask1, a.pose1, a.pose1, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32), a.K, None)
    frames = [(a.kps1, a.n1, a.points1, a.mask1, a.pose1), (a.kps2, a.n2, a.points2, a.mask2, a.pose2)]
    lists = tuple(np.array(v, np.int32) for v in ([0, 0, 0, 0], [1, 1, 0, 1], [0, 0, 0, 0], [1, 1, 0, 1]))
    worlds = [a, b, self_w, a]
    res, sim, row = run_batch(orbx, ext, worlds, frames=frames, lists=lists)
    for p, w in enumerate(worlds):
        same((res[p], sim[p], row[p]), S.optimize(w), "problem %d" % p)
    assert res[0].tobytes() == res[3].tobytes() and res[2]["status"] == 0 and res[2]["rounds"] == 2
    # against itself every true correspondence survives; what goes are the masked entries that hold no real point
    assert res[2]["n_inliers"] == 129 and res[2]["n_bad"] == res[2]["n_correspondences"] - 129


def test_variants(orbx, ext, sized):
    nomask = padded(S.world("nomask"), 128)
    check(orbx, ext, [nomask])                                     # no mask
    table = (S.P.inv_sigma2_table() * np.float32(0.5)).astype(np.float32)
    check(orbx, ext, [sized[129], sized[65]], inv_sigma2=table)    # an explicit inv_sigma2
    check(orbx, ext, [sized[129]])                                 # the context's table again
    fixed = padded(S.world("fixed"), 256)
    res = check(orbx, ext, [fixed], fix_scale=1)
    assert res[0]["s"] == 1.0
    check(orbx, ext, [fixed], fix_scale=0)
    start_true = S.make_world(100, 641, cap=CAP, noise=0.3, outliers=10, start=None)
    res = check(orbx, ext, [start_true, sized[65]], n_iterations=0, n_more_iterations=0)  # 0 iterations
    assert res[0]["lm_trials"] == 0 and res[0]["rounds"] == 2
    check(orbx, ext, [sized[300], sized[9], sized[64]], in_place=False)                   # d_sim3_out != d_sim3
    check(orbx, ext, [sized[129]], n_iterations=2, n_more_iterations=3)


@pytest.mark.parametrize("kind", sorted(garbage_kinds()))
def test_garbage_next_to_a_clean_problem(orbx, ext, kind):
    clean = padded(S.world("mixed"), 512)
    w, status = spoiled(kind)
    res, sim, row = run_batch(orbx, ext, [clean, padded(w, 512), clean])
    ref = S.optimize(clean)
    same((res[0], sim[0], row[0]), ref, kind)
    same((res[2], sim[2], row[2]), ref, kind)
    same((res[1], sim[1], row[1]), S.optimize(padded(w, 512)), kind)
    assert res[1]["status"] & status and row[1].tobytes() == padded(w, 512).match.tobytes()


def test_capacity_1024_with_lanes_that_walk_ten_entries(orbx, ext):
    w = S.world("big")
    assert w.cap == 1024 and len(w.edges()[0]) >= 600
    res = check(orbx, ext, [w])
    assert res[0]["n_bad"] == 64 and res[0]["n_inliers"] == 576


def test_failed_solves(orbx, ext):
    w = padded(S.world("clean"), 256)
    res = check(orbx, ext, [w, padded(S.world("axis"), 256)], inv_sigma2=np.zeros(S.NLEVELS, np.float32))
    assert res[0]["solver_failures"] == 20 and res[0]["lm_trials"] == 20 and res[0]["n_bad"] == 0


@pytest.mark.parametrize("n", [65, 257])
def test_second_setting(orbx, n):
    e = orbx.ORBextractor(1000, S.SCALE_FACTOR_2, S.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2)
    try:
        w = S.sized_world(n, 700 + n, "second", cap=CAP)
        # (at 65 the device uses its context's own table, which must be the setting's: the restatement is given that explicitly)
        res = check(orbx, e, [w, S.sized_world(40, 701 + n, "second", cap=CAP)], nlevels=S.NLEVELS_2,
                    inv_sigma2=None if n == 65 else S.inv_sigma2_of("second"), context_table=S.inv_sigma2_of("second"))
        assert res[0]["status"] == 0 and res[0]["n_correspondences"] == n and res[0]["n_inliers"] == n - n // 10
    finally:
        e.close()


def test_host_form_and_python_optimizer(orbx, ext):
    w = S.world("mixed")
    cut = lambda a, n: None if a is None else a[:n]  # noqa: E731
    res, sim, row = ext.optimize_sim3(w.kps1[:w.n1], w.points1[:w.n1], cut(w.mask1, w.n1), w.pose1, w.kps2[:w.n2], w.points2[:w.n2],
                                      cut(w.mask2, w.n2), w.pose2, w.match[:w.n1], w.sim, w.K)
    ref = S.optimize(w)
    assert bytes(res) == ref[0].tobytes() and sim.tobytes() == ref[1].tobytes() and np.array_equal(row, ref[2][:w.n1])

    class KF:
        def __init__(self, kps, n):
            self.mvKeysUn, self.mpORBextractor = kps[:n], ext
    T = lambda p: np.c_[p[:9].reshape(3, 3), p[9:]]  # noqa: E731
    n_in, row2, (s12, R12, t12), res2 = orbx.Optimizer.OptimizeSim3(
        KF(w.kps1, w.n1), KF(w.kps2, w.n2), (w.points1[:w.n1], w.mask1[:w.n1], T(w.pose1)), (w.points2[:w.n2], w.mask2[:w.n2], T(w.pose2)),
        w.match[:w.n1], w.sim[12], w.sim[:9], w.sim[9:12], 10.0, False, K=w.K)
    assert n_in == ref[0]["n_inliers"] and np.array_equal(row2, row) and bytes(res2) == bytes(res)
    assert np.float32(s12) == sim[12] and R12.tobytes() == sim[:9].tobytes() and t12.tobytes() == sim[9:12].tobytes()


def test_chained_solver_matcher_and_optimiser(orbx, ext):
    """compute_sim3_optimized_pairs_device: the solver writes d_sim3 and the inlier row, the matcher widens the row, the optimiser
    refines d_sim3 in place and removes from the row, with no copy between.  Equal to the three restatements chained."""
    import torch
    import sim3_ref_lib as R
    from test_gpu_sim3 import padded_m
    cap = 512
    mw = padded_m(R.make_match_world(400, 80, noise_bits=10), cap)
    rng = np.random.default_rng(80)
    t = mw.truth
    have = np.flatnonzero(t["have"])
    wrong = rng.choice(have, len(have) // 5, replace=False)
    mw.match[t["slots1"][wrong]] = rng.permutation(t["slots2"][wrong])  # mismatches among points
    sw = R.World(mw.kps[0], mw.n[0], mw.kps[1], mw.n[1], mw.match, mw.points[0], mw.mask[0], mw.points[1], mw.mask[1], mw.pose[0], mw.pose[1], mw.K)
    draws = R.make_draws(300, 80)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    col = lambda a: d(np.stack(a))  # noqa: E731
    z = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_sres, d_sim, d_row, d_mres = z(orbx.SIM3_RESULT_DTYPE.itemsize), z(52), z(cap * 4), z(orbx.MSIM3_RESULT_DTYPE.itemsize)
    d_ores = z(orbx.SIM3OPT_RESULT_DTYPE.itemsize)
    one, two = np.array([0], np.int32), np.array([1], np.int32)
    ext.compute_sim3_optimized_pairs_device(2, one, two, one, two, col(mw.kps), col(mw.desc), d(np.array(mw.n, np.int32)), d(mw.match), 2,
                                            col(mw.points), col(mw.mask), col(mw.dist), col(mw.pose), mw.K, mw.bounds, d(draws), d_sres,
                                            d_sim, d_row, d_mres, d_ores, capacity=cap)
    torch.cuda.synchronize()
    sim, row = d_sim.cpu().numpy().view(np.float32), d_row.cpu().numpy().view(np.int32)
    ores = d_ores.cpu().numpy().view(orbx.SIM3OPT_RESULT_DTYPE)[0]
    ref = R.solve(sw, draws, 0)
    q = mw.copy()
    q.match, q.sim = ref[2].copy(), ref[1].copy()
    mref = R.search_by_sim3(q)
    ow = S.World(mw.kps[0], mw.n[0], mw.kps[1], mw.n[1], mref["matches"].copy(), mw.points[0], mw.mask[0], mw.points[1], mw.mask[1],
                 mw.pose[0], mw.pose[1], ref[1].copy(), mw.K)
    same((ores, sim, row), S.optimize(ow), "chained")
    print("chained: %d correspondences, %d removed first, nInliers %d" % (ores["n_correspondences"], ores["n_bad"], ores["n_inliers"]))
    assert ores["status"] == 0 and ores["n_inliers"] >= 20  # this candidate closes the loop


def test_shim_sim3opt_agrees_with_the_c_abi(orbx, tmp_path):
    """tests/cpp/shim_sim3opt.cpp: Optimizer::OptimizeSim3 of the C++ shim gives the bytes of orbx_optimize_sim3."""
    exe = build_shim_sim3opt(orbx, tmp_path)
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    f = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][0].split()[1:]
    status, n_in, n, removed, left, agrees = (int(v) for v in f[:6])
    assert agrees == 1 and status == 0 and n == 150 and left == 0 and removed >= 15 and n_in == n - removed
    assert abs(float(f[6]) / 1.25 - 1) < 0.01
