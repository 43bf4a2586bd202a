"""The two-view bundle adjustment on the device (orbx_bundle_adjust / orbx_bundle_adjust_batch_device) equals the CPU restatement
tests/cpp/ba_ref.cpp BIT FOR BIT: every field of orbx_ba_result, the bytes of its f64 and the counters included, and every refined
point.  Both sides fix the same order of the sums, share the sin / cos routine and contract nothing (include/orbx.h).  What the
restatement itself is worth is tests/test_ba_host.py's business, which also shows that the worlds used here run every branch."""
import subprocess

import numpy as np
import pytest

import ba_ref_lib as B

pytestmark = pytest.mark.gpu

# points per pair: none, one, around a wave, beyond the workgroup's 256 lanes, and beyond twice its stride
COUNTS = (0, 1, 63, 64, 65, 257, 520)
CAP = 531  # just above the largest frame (520 matches + 10 other keypoints)


@pytest.fixture(scope="module")
def ext(orbx):
    e = orbx.ORBextractor(1000, 1.2, B.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sized():
    """A pair per count of COUNTS, with gross mismatches from 63 points on (rejected trials, Huber's outlier branch)."""
    return {n: B.make_pair(n, 20 + k, cap=CAP, outliers=(n // 16 if n >= 63 else 0)) for k, n in enumerate(COUNTS)}


def _bad(pair, what):
    w = pair.padded(pair.cap)
    i = int(B.pair_graph(pair)[0][0])
    if what == "match":
        w.m12[i] = w.n2
    elif what == "octave":
        w.k2["octave"][w.m12[i]] = B.NLEVELS
    elif what == "count":
        w.n1 = w.cap + 1
    elif what == "nan":
        w.p3d[i, 0] = np.nan
    elif what == "plane":
        w.p3d[i, 2] = 0.0
    return w


def run_batch(orbx, ext, pairs, n_iterations=20, min_points=100, normalize=True, inv_sigma2=None, in_place=False, reverse=False):
    """The pairs as one device batch (pair p = frames 2p and 2p + 1, or the frames in reverse order) -> (results [P], points
    [P, cap, 3])."""
    import torch
    P, cap = len(pairs), pairs[0].cap
    frame = (lambda p, k: 2 * (P - 1 - p) + 1 - k) if reverse else (lambda p, k: 2 * p + k)
    kps, n = np.zeros((2 * P, cap), orbx.KEYPOINT_DTYPE), np.zeros(2 * P, np.int32)
    first, second = np.zeros(P, np.int32), np.zeros(P, np.int32)
    for p, w in enumerate(pairs):
        assert w.cap == cap
        first[p], second[p] = frame(p, 0), frame(p, 1)
        kps[first[p]], kps[second[p]], n[first[p]], n[second[p]] = w.k1, w.k2, w.n1, w.n2
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_k, d_n, d_m = d(kps), d(n), d(np.stack([w.m12 for w in pairs]))
    d_ir, d_p, d_t = d(np.concatenate([w.init for w in pairs])), d(np.stack([w.p3d for w in pairs])), d(np.stack([w.tri for w in pairs]))
    d_res = torch.full((P * orbx.BA_RESULT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    d_out = None if in_place else torch.full((P * cap * 12,), 0xA5, dtype=torch.uint8, device="cuda")
    ext.bundle_adjust_batch_device(2 * P, first, second, d_k, d_n, d_m, d_ir, d_p, d_t, pairs[0].K, d_res, d_out, inv_sigma2=inv_sigma2,
                                   n_iterations=n_iterations, min_points=min_points, normalize=normalize, capacity=cap)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(orbx.BA_RESULT_DTYPE)
    pts = (d_p if in_place else d_out).cpu().numpy().view(np.float32).reshape(P, cap, 3)
    return res, pts


def same(res, pts, ref, rpts, what=""):
    """Bit for bit: the record's bytes field by field (so that a difference names its field), then the points."""
    for f in B.BA_RESULT_DTYPE.names:
        assert np.asarray(res[f]).tobytes() == np.asarray(ref[f]).tobytes(), (what, f, res[f], ref[f])
    assert pts.tobytes() == rpts.tobytes(), what


def check(orbx, ext, pairs, **kw):
    ref_kw = {k: v for k, v in kw.items() if k in ("n_iterations", "min_points", "normalize", "inv_sigma2")}
    res, pts = run_batch(orbx, ext, pairs, **kw)
    for p, w in enumerate(pairs):
        r, rp, _ = B.bundle_adjust(w, **ref_kw)
        same(res[p], pts[p], r, rp, "pair %d" % p)
    return res


@pytest.mark.parametrize("n", COUNTS)
def test_one_pair_of_each_size(orbx, ext, sized, n):
    res = check(orbx, ext, [sized[n]], min_points=60)
    assert res[0]["n_points"] == n
    if n >= 63:
        assert res[0]["iterations"] > 0 and res[0]["status"] == 0


def test_three_pairs_mixed_in_place_and_reversed_frames(orbx, ext, sized):
    check(orbx, ext, [sized[257], B.skipped(sized[65]), sized[520]], in_place=True, reverse=True)


@pytest.mark.parametrize("in_place", [False, True])
def test_failed_solves_between_pairs_that_solve(orbx, ext, sized, in_place):
    """no_weight (every edge at a level that weighs nothing under this table: ten failed solves, decided by thread 0 and taken by
    the whole workgroup, the points passed through) as pair 1 of 3 between a pair that rejects trials and the largest one."""
    pairs = [B.world("rejecting").padded(CAP), B.world("no_weight").padded(CAP), sized[520]]
    res = check(orbx, ext, pairs, inv_sigma2=B.top_level_off_table(), in_place=in_place)
    assert list(res["status"]) == [0, 0, 0] and list(res["solver_failures"]) == [0, 10, 0]
    assert res[1]["lm_trials"] == 10 and res[1]["iterations"] == 1 and res[1]["stop_reason"] == 1 and res[1]["lambda"] == 0
    assert res[0]["rejected_trials"] > 0 and res[2]["iterations"] == 20


def test_every_pair_fails_every_solve_under_a_table_of_zeros(orbx, ext, sized):
    res = check(orbx, ext, [sized[65], B.world("general").padded(CAP), sized[520]], inv_sigma2=B.zero_table(), min_points=60)
    assert list(res["status"]) == [0, 0, 0] and list(res["solver_failures"]) == list(res["lm_trials"]) == [10, 10, 10]
    assert list(res["iterations"]) == [1, 1, 1] and list(res["stop_reason"]) == [1, 1, 1]


def test_five_pairs_diverging_workgroups(orbx, ext, sized):
    """Skipped and refused pairs leave early next to pairs that reject trials, run into Huber's outlier branch, stop by the
    _nBad rule or use every iteration."""
    pairs = [_bad(sized[64], "match"), B.world("rejecting").padded(CAP), B.skipped(sized[63]), B.world("huber").padded(CAP),
             B.world("converged").padded(CAP)]
    res = check(orbx, ext, pairs, normalize=False)
    assert list(res["status"]) == [B.BAD_INPUT, 0, B.SKIPPED, 0, 0]
    assert res[1]["rejected_trials"] > 0 and res[3]["iterations"] == 20 and res[4]["stop_reason"] == 2


def test_flags_next_to_each_other(orbx, ext, sized):
    pairs = [_bad(sized[65], "octave"), _bad(sized[65], "count"), _bad(sized[257], "nan"), _bad(sized[64], "plane"),
             B.world("mirrored").padded(CAP)]
    res = check(orbx, ext, pairs)
    assert list(res["status"]) == [B.BAD_INPUT, B.BAD_INPUT, B.NONFINITE, B.NONFINITE, B.NEGATIVE_DEPTH]


@pytest.mark.parametrize("normalize", [False, True])
def test_normalize_and_few_iterations(orbx, ext, sized, normalize):
    res = check(orbx, ext, [B.world("general").padded(CAP), sized[1], B.world("few").padded(CAP)], normalize=normalize, n_iterations=3,
                min_points=40)
    assert list(res["status"]) == [0, B.FEW_POINTS, 0] and res[0]["stop_reason"] == 0 and res[0]["iterations"] == 3


def test_no_iteration(orbx, ext, sized):
    check(orbx, ext, [sized[65]], n_iterations=0, normalize=False)


def test_null_table_is_the_contexts(orbx, ext, sized):
    table = ext.GetInverseScaleSigmaSquares()
    res, pts = run_batch(orbx, ext, [sized[257]])
    r, rp, _ = B.bundle_adjust(sized[257], inv_sigma2=table)
    same(res[0], pts[0], r, rp)
    other = (table * np.float32(0.5)).astype(np.float32)
    res2 = check(orbx, ext, [sized[257]], inv_sigma2=other)
    assert res2[0]["chi2_initial"] != res[0]["chi2_initial"]


def test_pair_list_and_table_held_across_calls(orbx, sized):
    """The pair list and the table live on the device between calls, each with the host copy its upload read: call after call on
    one context of its own -- a first list, the same again (no upload), as many pairs in other frames (replaced in place), one
    pair, three pairs (the device array grows), the first list again, and then the same two pairs under another table (the table
    alone is replaced) and under the first one -- every call equals the restatement bit for bit."""
    e = orbx.ORBextractor(1000, 1.2, B.NLEVELS, 20, 7, max_width=640, max_height=480, max_batch=2)
    a, b, c = sized[63], sized[65], sized[257]
    refs = {}

    def step(what, pairs, table=None, **kw):
        res, pts = run_batch(orbx, e, pairs, min_points=60, inv_sigma2=table, **kw)
        for p, w in enumerate(pairs):
            key = (id(w), table is not None)
            if key not in refs:
                refs[key] = B.bundle_adjust(w, min_points=60, inv_sigma2=table)[:2]
            same(res[p], pts[p], *refs[key], what="%s, pair %d" % (what, p))

    try:
        step("two pairs", [a, b])
        step("the same list", [a, b])
        step("as many pairs, other frames", [a, b], reverse=True)
        step("one pair", [c])
        step("three pairs", [b, c, a])
        step("the first list again", [a, b])
        step("another table", [a, b], table=B.top_level_off_table())
        step("the first table again", [a, b])
    finally:
        e.close()


def test_host_form_equals_the_batch(orbx, ext, sized):
    for w in (sized[257], B.skipped(sized[64]), _bad(sized[65], "match")):
        res, pts = run_batch(orbx, ext, [w])
        one, p1 = ext.bundle_adjust(w.k1[:w.n1], w.k2[:w.n2], w.m12[:w.n1], w.init, w.p3d[:w.n1], w.tri[:w.n1], w.K)
        assert bytes(one) == res[0].tobytes()
        assert p1.tobytes() == pts[0, :w.n1].tobytes()


# ---- the second setting (pose_ref_lib.SECOND): fx != fy, a context of 5 levels of 1.37, frame 2 rolled by 89 degrees ----

CAP_2 = 268  # just above the larger frame (257 matches + 10 other keypoints)


@pytest.fixture(scope="module")
def ext2(orbx):
    e = orbx.ORBextractor(1000, B.SCALE_FACTOR_2, B.NLEVELS_2, 20, 7, max_width=640, max_height=480, max_batch=2)
    yield e
    e.close()


def test_second_setting_anisotropic_camera_and_five_levels(orbx, ext2):
    """Two pairs (65 and 257 points) under K_ANISO: once with the context's own table, once with the same table given
    explicitly; then the host form on the smaller one."""
    pairs = [B.make_pair(n, 120 + k, cap=CAP_2, outliers=n // 16, motion=B.MOTION_ROLL, **B.SECOND) for k, n in enumerate((65, 257))]
    table = B.inv_sigma2_of("second")
    assert ext2.GetInverseScaleSigmaSquares().tobytes() == table.tobytes() and len(table) == B.NLEVELS_2
    res, pts = run_batch(orbx, ext2, pairs, min_points=60)  # (the context's table)
    for p, w in enumerate(pairs):
        r, rp, _ = B.bundle_adjust(w, min_points=60, inv_sigma2=table)
        same(res[p], pts[p], r, rp, "context's table, pair %d" % p)
    res2 = check(orbx, ext2, pairs, min_points=60, inv_sigma2=table)
    assert res2.tobytes() == res.tobytes()
    for p, n in enumerate((65, 257)):  # not trivial: every point in the graph, iterations that gain
        assert res[p]["status"] == 0 and res[p]["n_points"] == n and res[p]["iterations"] > 1
        assert res[p]["chi2_final"] < 0.5 * res[p]["chi2_initial"]
    w = pairs[0]
    one, p1 = ext2.bundle_adjust(w.k1[:w.n1], w.k2[:w.n2], w.m12[:w.n1], w.init, w.p3d[:w.n1], w.tri[:w.n1], w.K, min_points=60)
    assert bytes(one) == res[0].tobytes() and p1.tobytes() == pts[0, :w.n1].tobytes()


def test_chained_behind_the_initializer(orbx, ext):
    """Initializer -> bundle adjustment on the device, the second stage reading what the first left there (its results, vP3D,
    vbTriangulated), for three pairs: two two-view scenes with depth that the Initializer accepts and, between them, a scene it
    refuses.  The accepted pairs must really be optimised, and every result equals the restatement fed with the downloaded
    intermediates."""
    import torch
    scenes = [B.init_scene(seed) for seed in (3, 5, 11)]  # (5 is AMBIGUOUS)
    P, cap = len(scenes), len(scenes[0][1])
    K = scenes[0][0]
    kps = np.stack([k for s in scenes for k in (s[1], s[3])])
    n = np.array([c for s in scenes for c in (s[2], s[4])], np.int32)
    m12 = np.stack([s[5] for s in scenes])
    sets = np.stack([s[6] for s in scenes])
    first, second = np.arange(0, 2 * P, 2, dtype=np.int32), np.arange(1, 2 * P, 2, dtype=np.int32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_k, d_n, d_m, d_sets = d(kps), d(n), d(m12), d(sets)
    d_ir = torch.zeros(P * orbx.INIT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_p = torch.zeros(P * cap * 3, dtype=torch.float32, device="cuda")
    d_t = torch.zeros(P * cap, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(P * orbx.BA_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(P * cap * 3, dtype=torch.float32, device="cuda")
    ext.initialize_batch_device(2 * P, first, second, d_k, d_n, d_m, d_sets, K, d_ir, d_p, d_t, capacity=cap, n_iter=200)
    ext.bundle_adjust_batch_device(2 * P, first, second, d_k, d_n, d_m, d_ir, d_p, d_t, K, d_res, d_out, capacity=cap)
    torch.cuda.synchronize()
    ir = d_ir.cpu().numpy().view(B.INIT_RESULT_DTYPE)
    p3d, tri = d_p.cpu().numpy().reshape(P, cap, 3), d_t.cpu().numpy().reshape(P, cap)
    res, out = d_res.cpu().numpy().view(orbx.BA_RESULT_DTYPE), d_out.cpu().numpy().reshape(P, cap, 3)
    print("chained: init status", list(ir["status"]), "ba status", list(res["status"]), "points", list(res["n_points"]), "iterations",
          list(res["iterations"]))
    assert ir["status"][0] == 0 and ir["status"][2] == 0 and ir["status"][1] != 0
    assert res["status"][1] == B.SKIPPED
    table = ext.GetInverseScaleSigmaSquares()
    for p in range(P):
        if p != 1:
            assert res["status"][p] == 0 and res["iterations"][p] > 0 and res["n_points"][p] == tri[p].sum() > 100
            assert res["chi2_final"][p] < res["chi2_initial"][p]
        w = B.Pair(kps[2 * p].copy(), n[2 * p], kps[2 * p + 1].copy(), n[2 * p + 1], m12[p].copy(), ir[p:p + 1].copy(), p3d[p].copy(),
                   tri[p].copy(), K.reshape(9))
        r, rp, _ = B.bundle_adjust(w, 20, 100, True, inv_sigma2=table)
        same(res[p], out[p], r, rp, "pair %d" % p)


def test_chained_from_images(orbx, ext):
    """extract + match -> Initializer -> bundle adjustment from two images, every stage reading what the stage before left on the
    device; the result equals the restatement fed with the downloaded intermediates.  The pair is a shifted plane, which the
    Initializer may well refuse (the adjustment is then ORBX_BA_SKIPPED): this test is about the plumbing from the extractor's
    arrays on; test_chained_behind_the_initializer is the one in which the optimiser must run."""
    import ctypes
    import torch
    from orb_slam_tracking_amd import synth
    W, H = 640, 480
    cap = ext.capacity
    a, b = synth.synth_pair(W, H, 7)
    d_img = torch.from_numpy(np.stack([a, b])).cuda()
    d_k = torch.zeros(2 * cap * 28, dtype=torch.uint8, device="cuda")
    d_d = torch.zeros(2 * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_m = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(1, dtype=torch.int32, device="cuda")
    first, second = np.array([0], np.int32), np.array([1], np.int32)
    ext.extract_match_batch_device(d_img, 2, W, H, W, W * H, d_k, d_d, d_n, first, second, (0, W, 0, H), d_m, d_nm)
    torch.cuda.synchronize()
    n, m12 = d_n.cpu().numpy(), d_m.cpu().numpy()
    nm = int((m12[:n[0]] >= 0).sum())
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(1)
    sets = orbx.sample_sets(nm, 200, libc.rand) if nm >= 8 else np.zeros((200, 8), np.int32)
    d_sets = torch.from_numpy(sets.reshape(1, 200, 8)).cuda()
    K = np.array([[520.0, 0, 320], [0, 520, 240], [0, 0, 1]], np.float32)
    d_ir = torch.zeros(orbx.INIT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_p = torch.zeros(cap * 3, dtype=torch.float32, device="cuda")
    d_t = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(orbx.BA_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(cap * 3, dtype=torch.float32, device="cuda")
    ext.initialize_batch_device(2, first, second, d_k, d_n, d_m, d_sets, K, d_ir, d_p, d_t)
    ext.bundle_adjust_batch_device(2, first, second, d_k, d_n, d_m, d_ir, d_p, d_t, K, d_res, d_out, min_points=20)
    torch.cuda.synchronize()
    kps = d_k.cpu().numpy().view(orbx.KEYPOINT_DTYPE).reshape(2, cap)
    w = B.Pair(kps[0].copy(), n[0], kps[1].copy(), n[1], m12.copy(), d_ir.cpu().numpy().view(B.INIT_RESULT_DTYPE).copy(),
               d_p.cpu().numpy().reshape(cap, 3).copy(), d_t.cpu().numpy().copy(), K.reshape(9))
    r, rp, _ = B.bundle_adjust(w, 20, 20, True, inv_sigma2=ext.GetInverseScaleSigmaSquares())
    res = d_res.cpu().numpy().view(orbx.BA_RESULT_DTYPE)[0]
    print("chained: %d matches, init status %d, ba status %d, %d points, %d iterations" %
          (nm, w.init["status"][0], res["status"], res["n_points"], res["iterations"]))
    same(res, d_out.cpu().numpy().reshape(cap, 3), r, rp)


def test_shim_ba_agrees_with_the_c_abi(orbx, tmp_path):
    """tests/cpp/shim_ba.cpp: Optimizer::BundleAdjustmentTwoView of the C++ shim gives the bytes of orbx_bundle_adjust."""
    from test_ba_host import build_shim_ba
    exe = build_shim_ba(orbx, tmp_path)
    p = subprocess.run([exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    status, iterations, n_points, agrees = (int(v) for v in [l for l in p.stdout.splitlines() if l.startswith("RESULT")][0].split()[1:])
    assert agrees == 1 and status == 0 and iterations > 0 and n_points == 160
