"""The single-problem calls of one context stage in ONE device block (Staged and ctxIo in csrc/orbx_host.h), which keeps what the
last call left in it.  So every call here is made on a context that has just served other calls -- larger ones, ones whose
optional inputs were all set, ones of every other kind, one that its batch entry refused -- and must return, byte for byte, what
the same call returns on a fresh context: the block replaced by a larger one, the zero fill where a call has one, an absent
optional input that stays a null kernel argument, the wait on the refused path.  What the results are worth is the business of
each module's own tests; here only "the same as on a fresh context" is asked, of every output."""
import ctypes

import numpy as np
import pytest

import ba_ref_lib as B
import match_bow_ref_lib as MB
import match_kfproj_ref_lib as MK
import match_local_ref_lib as ML
import match_proj_ref_lib as MP
import match_scw_ref_lib as MS
import pnp_ref_lib as PN
import pose_ref_lib as P
import sim3_ref_lib as S
import sim3opt_ref_lib as SO
import tri_ref_lib as T

pytestmark = pytest.mark.gpu


def make_ext(orbx):
    return orbx.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2)


@pytest.fixture(scope="module")
def ext(orbx):
    e = make_ext(orbx)
    yield e
    e.close()


def blob(x):
    """Every output of a call as bytes: arrays with their type and shape, result records as they lie in memory."""
    if isinstance(x, (tuple, list)):
        return b"(" + b"|".join(blob(v) for v in x) + b")"
    if isinstance(x, np.ndarray):
        return ("%s%s:" % (x.dtype.str, x.shape)).encode() + np.ascontiguousarray(x).tobytes()
    if isinstance(x, ctypes.Structure):
        return bytes(x)
    if hasattr(x, "as_dict"):
        return repr(sorted(x.as_dict().items())).encode()
    return repr(x).encode()


def on_fresh(orbx, call):
    e = make_ext(orbx)
    try:
        return blob(call(e))
    finally:
        e.close()


def mat(pose):
    """[12] (R row-major, then t) -> Tcw 3x4"""
    return np.c_[pose[:9].reshape(3, 3), pose[9:]]


def cut(a, n):
    return None if a is None else a[:n]


# ---- the calls: each a function of the context; the worlds are made once -------------------------------------------------
def pose_call(n, seed):
    w = P.make_world(n, seed, outliers=max(n // 8, 1))
    return lambda e: e.pose_optimize(w.kps[:w.n], w.points[:w.n], w.mask[:w.n], mat(w.pose0), w.K)


def pnp_call(n, seed):
    w, d = PN.make_world(n, seed, outliers=max(n // 8, 1)), PN.make_draws(64, seed)
    return lambda e: e.pnp_solve(w.kps[:w.n], w.points[:w.n], w.mask[:w.n], w.K, d)


def sim3_solve_call(n, seed):
    w, d = S.make_world(n, seed, outliers=max(n // 8, 1)), S.make_draws(64, seed)
    return lambda e: e.sim3_solve(w.kps1[:w.n1], w.points1[:w.n1], w.mask1[:w.n1], w.pose1, w.kps2[:w.n2], w.points2[:w.n2],
                                  w.mask2[:w.n2], w.pose2, w.match[:w.n1], w.K, d)


def optimize_sim3_call(n, seed):
    w = SO.make_world(n, seed, noise=0.5, outliers=max(n // 8, 1))
    return lambda e: e.optimize_sim3(w.kps1[:w.n1], w.points1[:w.n1], cut(w.mask1, w.n1), w.pose1, w.kps2[:w.n2], w.points2[:w.n2],
                                     cut(w.mask2, w.n2), w.pose2, w.match[:w.n1], w.sim, w.K)


def projection_call(n, seed, optional="own", **kw):
    """optional: "own" the world's mask and outlier flags, "ones" both all ones, None neither"""
    w = MP.make_world(n, seed)
    ones = np.ones(w.n_l, np.uint8)
    mask, out = {"own": (w.mask, w.outlier), "ones": (ones, ones), None: (None, None)}[optional]
    th = kw.get("th", w.th)
    return lambda e: e.match_projection(w.kps_l, w.desc_l, w.kps_c, w.desc_c, w.points, mask, mat(w.pose), w.K, w.bounds, th, w.ori,
                                        point_desc=w.point_desc, last_outlier=out)


def local_map_call(n_m, seed, n_f=None):
    """n_f: the frame cut to its first n_f features"""
    w = ML.make_world(n_m, seed)
    assert n_f is None or w.n_f >= n_f
    f = slice(0, n_f)
    return lambda e: e.match_local_map(w.kps[f], w.desc[f], w.points, w.normals, w.dists, w.map_desc, w.mask, mat(w.pose), w.K, w.bounds,
                                       w.matches[f], w.th, w.nnratio, cut(w.outlier, n_f))


def kfproj_call(n, seed):
    w = MK.make_world(n, seed)
    return lambda e: e.match_keyframe_projection(w.kps_k, w.desc_k, w.kps_c, w.desc_c, w.points, w.mask, w.dists, mat(w.pose), w.K,
                                                 w.bounds, w.matches, w.th, w.orb_dist, w.ori, w.point_desc, w.outlier)


def match_sim3_call(n, seed):
    w = S.make_match_world(n, seed)
    n1, n2 = w.n
    mk = w.mask or [None, None]
    return lambda e: e.match_sim3(w.kps[0][:n1], w.desc[0][:n1], w.points[0][:n1], cut(mk[0], n1), w.dist[0][:n1], mat(w.pose[0]),
                                  w.kps[1][:n2], w.desc[1][:n2], w.points[1][:n2], cut(mk[1], n2), w.dist[1][:n2], mat(w.pose[1]),
                                  w.sim, w.K, w.bounds, w.match[:n1], 7.5, 100)


def scw_call(n_m, seed, table=True, **kw):
    w = MS.make_world(n_m, seed, table=table, **kw)
    assert (w.table is not None) == table
    return lambda e: e.match_scw(w.kps, w.desc, w.points, w.normals, w.dists, w.map_desc, w.mask, w.scw, w.K, w.bounds, w.matches,
                                 w.th, w.th_low, w.table)


def compose_call(seed):
    rng = np.random.default_rng(seed)
    pose, sim = rng.standard_normal(12).astype(np.float32), rng.standard_normal(13).astype(np.float32)
    return lambda e: e.sim3_compose_scw(pose, sim)


def bow_call(n, bad_feature=False):
    """A pair of the SearchByBoW world, cut to its first n features (the FeatureVector entries of the others dropped)."""
    w = MB.world(*MB.WORLDS[0])
    a, b = MB.PAIRS[0]
    na, nb = min(int(w.n[a]), n), min(int(w.n[b]), n)

    def fv(f, m):
        node, feat = (np.asarray(v) for v in w.fv[f])
        keep = feat < m
        return node[keep], feat[keep]
    (an, af), (bn, bf) = fv(a, na), fv(b, nb)
    if bad_feature:
        bf = bf.copy()
        bf[0] = nb  # a feature the frame does not have
    return lambda e: e.match_bow(w.kps[a, :na], w.desc[a, :na], an, af, w.kps[b, :nb], w.desc[b, :nb], bn, bf,
                                 kf_mask=w.mask[a, :na], nnratio=0.9, checkOri=True)


def tri_world(seed, n_points):
    return T.make_world(seed, n_points=n_points, n_distract=n_points // 5, n_random=n_points // 7)


def triangulation_call(seed, n_points, masks):
    w = tri_world(seed, n_points)
    m1, m2 = (np.ones(w.kf1.n, np.uint8), np.ones(w.kf2.n, np.uint8)) if masks else (None, None)
    return lambda e: e.match_triangulation(w.kf1.kps, w.kf1.desc, w.kf1.fv_node, w.kf1.fv_feat, mat(w.kf1.pose), w.kf2.kps, w.kf2.desc,
                                           w.kf2.fv_node, w.kf2.fv_feat, mat(w.kf2.pose), w.K, mask1=m1, mask2=m2)


def triangulate_call(seed, n_points):
    w = tri_world(seed, n_points)
    m12 = w.expected()["match"]["matches12"][:w.kf1.n]
    return lambda e: e.triangulate_matches(w.kf1.kps, mat(w.kf1.pose), w.kf2.kps, mat(w.kf2.pose), w.K, m12)


def ba_call(n, seed):
    w = B.make_pair(n, seed, outliers=n // 16)
    return lambda e: e.bundle_adjust(w.k1[:w.n1], w.k2[:w.n2], w.m12[:w.n1], w.init, w.p3d[:w.n1], w.tri[:w.n1], w.K, min_points=20)


def check_calls(n, seed):
    """check_homography, check_fundamental and check_rt over three models each, on a two-view pair's keypoints and matches"""
    w = B.make_pair(n, seed)
    rng = np.random.default_rng(seed)
    k1, k2, m12 = w.k1[:w.n1], w.k2[:w.n2], w.m12[:w.n1]
    near = lambda: (np.eye(3) + 0.01 * rng.standard_normal((3, 3, 3))).astype(np.float32)  # noqa: E731
    H21, H12, F21, R21 = near(), near(), (0.001 * rng.standard_normal((3, 3, 3))).astype(np.float32), near()
    t21 = rng.standard_normal((3, 3)).astype(np.float32)
    inl = (rng.random(int((m12 >= 0).sum())) < 0.8).astype(np.uint8)
    return (lambda e: e.check_homography(H21, H12, k1, k2, m12), lambda e: e.check_fundamental(F21, k1, k2, m12),
            lambda e: e.check_rt(R21, t21, w.K, k1, k2, m12, inl))


# ---- one block, growing ---------------------------------------------------------------------------------------------------
def test_the_block_grows_between_two_equal_calls(orbx, ext):
    """pose_optimize at 64 features, match_local_map with 300 features against 500 map points (the block is replaced by a larger
    one), the same pose_optimize again."""
    pose = pose_call(64, 3)
    local = local_map_call(500, 4, n_f=300)
    first, middle, again = blob(pose(ext)), blob(local(ext)), blob(pose(ext))
    assert first == again
    assert first == on_fresh(orbx, pose) and middle == on_fresh(orbx, local)


# ---- one block, stale contents ---------------------------------------------------------------------------------------------
STALE = {
    "match_projection": lambda: (projection_call(400, 21, "ones"), projection_call(50, 22, None)),
    "bundle_adjust": lambda: (ba_call(300, 23), ba_call(40, 24)),
    "match_triangulation": lambda: (triangulation_call(25, 220, True), triangulation_call(26, 45, False)),
    "match_scw": lambda: (scw_call(200, 27, True), scw_call(40, 28, False)),
}


@pytest.mark.parametrize("kind", sorted(STALE))
def test_a_small_call_after_a_large_one_with_every_optional_input(orbx, ext, kind):
    """The large call leaves its masks, flags and table in the block; the small one brings none and reads zeros / nothing."""
    large, small = STALE[kind]()
    large(ext)
    assert blob(small(ext)) == on_fresh(orbx, small)


# ---- every kind once, interleaved ---------------------------------------------------------------------------------------------
def test_every_single_problem_call_in_one_sequence(orbx, ext):
    hom, fun, rt = check_calls(64, 47)
    calls = [("pose_optimize", pose_call(64, 31)), ("pnp_solve", pnp_call(64, 32)), ("sim3_solve", sim3_solve_call(64, 33)),
             ("optimize_sim3", optimize_sim3_call(64, 34)), ("match_projection", projection_call(64, 35)),
             ("match_local_map", local_map_call(64, 36)), ("match_keyframe_projection", kfproj_call(64, 37)),
             ("match_sim3", match_sim3_call(64, 38)), ("match_scw", scw_call(64, 39)), ("sim3_compose_scw", compose_call(40)),
             ("match_bow", bow_call(64)), ("match_triangulation", triangulation_call(42, 45, False)),
             ("triangulate_matches", triangulate_call(42, 45)), ("bundle_adjust", ba_call(64, 44)), ("check_homography", hom),
             ("check_fundamental", fun), ("check_rt", rt)]
    got = [(name, blob(call(ext))) for name, call in calls]
    for (name, g), (_, call) in zip(got, calls):
        assert g == on_fresh(orbx, call), name


# ---- a refusal inside a staged call -------------------------------------------------------------------------------------------
def test_a_refused_batch_entry_leaves_the_context_usable(orbx, ext):
    """match_projection with th = NaN: the wrapper has queued its uploads when the batch entry refuses the radius factor.  The
    code and the message are the batch entry's, and the next call is served as on a fresh context.

    orbx_match_bow has no such refusal to offer: its batch entry checks null pointers, the pair indices and the capacity, and the
    wrapper passes its own block, the pair (0, 1) and a capacity it has already checked, so only a failed HIP call can make that
    entry return an error behind the uploads.  What the wrapper itself refuses (a FeatureVector that names a feature the frame
    does not have) comes before the staging; it is asked here all the same, with a valid call behind it."""
    good = projection_call(64, 51)
    with pytest.raises(orbx.OrbxError) as err:
        projection_call(64, 51, th=float("nan"))(ext)
    assert err.value.code == orbx.E_BADARG and "match projection: th is not a positive number" in str(err.value)
    assert blob(good(ext)) == on_fresh(orbx, good)
    bow = bow_call(64)
    with pytest.raises(orbx.OrbxError) as err:
        bow_call(64, bad_feature=True)(ext)
    assert err.value.code == orbx.E_BADARG and "match bow: a FeatureVector names a feature the frame does not have" in str(err.value)
    assert blob(bow(ext)) == on_fresh(orbx, bow)


# ---- held arrays ------------------------------------------------------------------------------------------------------------
def test_held_lists_and_table_of_pose_optimize_batch_device(orbx):
    """The same lists twice (no upload), one column changed, then only the sigma table changed: each call on the one context
    equals the call on a fresh one."""
    from test_gpu_pose import run_batch
    a, b = P.make_world(64, 61, cap=80, outliers=8), P.make_world(70, 62, cap=80, outliers=8)
    frames, sets = [(a.kps, a.n), (b.kps, b.n)], [(a.points, a.mask), (b.points, b.mask)]

    def problems(frame, point_set):
        out = []
        for w, f, s in zip((a, b), frame, point_set):
            q = w.copy()
            q.frame, q.point_set = f, s
            out.append(q)
        return out
    table = None
    steps = [(problems((0, 1), (0, 1)), None), (problems((0, 1), (0, 1)), None), (problems((0, 0), (0, 1)), None)]
    held = make_ext(orbx)
    try:
        table = (held.GetInverseScaleSigmaSquares() * np.float32(0.5)).astype(np.float32)
        steps.append((problems((0, 0), (0, 1)), table))
        for k, (ws, sig) in enumerate(steps):
            res, flags = run_batch(orbx, held, ws, inv_sigma2=sig, frames=frames, sets=sets)
            e = make_ext(orbx)
            try:
                res0, flags0 = run_batch(orbx, e, ws, inv_sigma2=sig, frames=frames, sets=sets)
            finally:
                e.close()
            assert res.tobytes() == res0.tobytes() and flags.tobytes() == flags0.tobytes(), "step %d" % k
        assert steps[0][0][0].n and res["status"][0] == 0  # (not trivial: the first problem is solved)
    finally:
        held.close()


def test_held_lists_of_match_sim3_pairs_device(orbx):
    """The same four lists twice, then one column changed: each call on the one context equals the call on a fresh one."""
    from test_gpu_sim3 import run_match_batch
    a, b = S.make_match_world(64, 63, cap=96), S.make_match_world(70, 64, cap=96)
    frames = [(a, 0), (a, 1), (b, 0), (b, 1)]
    i = lambda *v: np.array(v, np.int32)  # noqa: E731
    lists = (i(0, 2), i(1, 3), i(0, 2), i(1, 3))
    steps = [lists, lists, (i(0, 2), i(1, 3), i(0, 2), i(3, 1))]
    held = make_ext(orbx)
    try:
        for k, ls in enumerate(steps):
            rows, res = run_match_batch(orbx, held, [a, b], frames=frames, lists=ls)
            e = make_ext(orbx)
            try:
                rows0, res0 = run_match_batch(orbx, e, [a, b], frames=frames, lists=ls)
            finally:
                e.close()
            assert rows.tobytes() == rows0.tobytes() and res.tobytes() == res0.tobytes(), "step %d" % k
            if k == 0:
                assert res["status"][0] == 0 and res["n_found"][0] > 0  # (not trivial)
    finally:
        held.close()
