"""The guard behind the second setting of the back-end worlds (pose_ref_lib.K_ANISO: fx != fy; 5 levels of 1.37; a roll of 89
degrees), kept alive without a GPU.  Each case copies a CPU restatement and the headers it includes into a temporary tree of the
same layout, replaces fy by fx in the v-projection (and, where the file has them, in the v-rows of the Jacobian) of ONE file of
that copy, builds the copy with the ref lib's own compiler line (its build(src)) and runs that module's cheapest independent check
on one world of the second setting: the check must report a difference, and must pass on the unaltered copy.  Under the first
setting (fx == fy) none of the eight substitutions changes a single result.  Nothing under orb_slam_tracking_amd/ is written."""
import glob
import os
import shutil

import numpy as np
import pytest

import ba_ref_lib as B
import match_kfproj_ref_lib as MK
import match_local_ref_lib as ML
import match_proj_ref_lib as MP
import pnp_ref_lib as Q
import pose_ref_lib as P
import sim3_ref_lib as S
import tri_ref_lib as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("orb_slam_tracking_amd", "csrc")
CPP = os.path.join("tests", "cpp")


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ---- one check per module: True when the restatement (whichever library the module's lib() returns) agrees with its judge ----

def check_pose():
    """The first Levenberg-Marquardt step against the numerically differentiated numpy statement (test_pose_host's margin)."""
    w, sig = P.world("clean", "second"), P.inv_sigma2_of("second")
    a, b = P.first_step(w, sig), P.first_step_numpy(w, sig)
    return max(_rel(a["xp"], b["xp"]), _rel([a["chi2_initial"]], [b["chi2_initial"]]), _rel([a["lam"]], [b["lam"]])) <= 100 * 1.06e-5


def check_ba():
    """The first step of the two-view bundle adjustment against its numpy statement (test_ba_host's margin)."""
    w, sig = B.world("general", "second"), B.inv_sigma2_of("second")
    a, b = B.first_step(w, sig), B.first_step_numpy(w, sig)
    d = max(_rel(a["xp"], b["xp"]), _rel(a["xl"], b["xl"]), _rel([a["chi2_initial"]], [b["chi2_initial"]]), _rel([a["lam"]], [b["lam"]]))
    return d <= 100 * 1.02e-5


_pnp = {}


def check_pnp():
    """A noise-free world with gross mismatches: the returned inliers are exactly the clean set (ground truth)."""
    if not _pnp:
        _pnp["w"] = Q.make_world(90, 401, outliers=18, noise=0.0, motion=Q.MOTION_2, **Q.SECOND)
    w = _pnp["w"]
    r, _, _, inl = Q.solve(w, Q.make_draws(35, 1), 0, Q.sigma2_table(Q.NLEVELS_2, Q.SCALE_FACTOR_2))
    return bool(r["status"] == 0 and np.array_equal(np.flatnonzero(inl), w.truth["clean"]))


_sim3 = {}


def check_sim3():
    """Rule 5's squared pixel distances under a similarity that is a little off, against their numpy statement in f64 (f32
    against f64 on errors of tens of squared pixels: 1e-3 relative is far above the rounding and far below a third)."""
    if not _sim3:
        _sim3["w"] = S.make_world(80, 102, rot=S.ROLL, **S.SECOND)
    w = _sim3["w"]
    t = w.truth
    R = P.rotvec((0.01, -0.02, 0.015)) @ t["R"]
    sim = np.r_[R.reshape(9), t["t"] + 0.05, t["s"]].astype(np.float32)
    e = S.errors(w, sim, S.sigma2_table(S.NLEVELS_2, S.SCALE_FACTOR_2))
    _, _, Y1, Y2 = S.camera_points_numpy(w)
    e1, e2 = S.errors_numpy(Y1, Y2, float(sim[12]), sim[:9].reshape(3, 3).astype(np.float64), sim[9:12].astype(np.float64), w.K)
    assert e1.min() > 1.0 and e2.min() > 1.0  # (the similarity is off by pixels everywhere: relative differences mean something)
    return _rel(e["err"][:, 0] / e1, 1.0) <= 1e-3 and _rel(e["err"][:, 1] / e2, 1.0) <= 1e-3


def check_tri():
    """F12 and the epipole against numpy's, and every outcome of the triangulation that numpy is sure of."""
    w = T.world("small_nodes@2")
    m = T.search(w)
    F, ep, _ = T.geometry_numpy(w)
    ok = np.abs(m["res"]["F12"].reshape(3, 3) - F).max() <= 1e-5 * np.abs(F).max() and abs(m["res"]["ey"] - ep[1]) <= 1e-4 * abs(ep[1])
    rows = w.expected()["match"]["matches12"]  # (the committed restatement's rows: the triangulation is judged on its own)
    t, n = T.triangulate(w, rows), T.triangulate_numpy(w, rows[:w.kf1.n])
    sure = n["outcome"] >= 0
    return bool(ok and np.array_equal(t["outcome"][:w.kf1.n][sure], n["outcome"][sure]))


def check_match_proj():
    w = MP.world("w150@2")
    m, nm = MP.search_by_projection_numpy(w)
    e = MP.search_by_projection(w)
    return bool(np.array_equal(e["matches"], m) and e["res"]["nmatches"] == nm)


def check_match_local():
    w = ML.world("w150@2")
    m, view, nm = ML.search_local_points_numpy(w)
    e = ML.search_local_points(w)
    return bool(np.array_equal(e["matches"], m) and np.array_equal(e["view"], view) and e["res"]["nmatches"] == nm)


def check_match_kfproj():
    w = MK.world("w150@2")
    m, nm = MK.search_by_projection_numpy(w)
    e = MK.search_by_projection(w)
    return bool(np.array_equal(e["matches"], m) and e["res"]["nmatches"] == nm)


# (altered file, old text, new text, the ref lib whose restatement is rebuilt, its check)
MUTANTS = {
    "orbx_pnp_math.inc": (os.path.join(CSRC, "orbx_pnp_math.inc"), "K.fv", "K.fu", Q, check_pnp),
    "orbx_sim3_math.inc": (os.path.join(CSRC, "orbx_sim3_math.inc"), "K.fy", "K.fx", S, check_sim3),
    "orbx_ba_math.inc": (os.path.join(CSRC, "orbx_ba_math.inc"), "K.fy", "K.fx", B, check_ba),
    "orbx_tri_math.inc": (os.path.join(CSRC, "orbx_tri_math.inc"), "(fy * ", "(fx * ", T, check_tri),
    "pose_ref.cpp": (os.path.join(CPP, "pose_ref.cpp"), "(double)K[4]", "(double)K[0]", P, check_pose),
    "match_proj_ref.cpp": (os.path.join(CPP, "match_proj_ref.cpp"), "(fy * ", "(fx * ", MP, check_match_proj),
    "match_local_ref.cpp": (os.path.join(CPP, "match_local_ref.cpp"), "(fy * ", "(fx * ", ML, check_match_local),
    "match_kfproj_ref.cpp": (os.path.join(CPP, "match_kfproj_ref.cpp"), "(fy * ", "(fx * ", MK, check_match_kfproj),
}


def _copy_tree(dst):
    """The restatements and every header they can include, in the repository's layout."""
    for rel, patterns in (("include", ("*.h",)), (CSRC, ("*.inc", "*.h")), (CPP, ("*.cpp", "*.h"))):
        os.makedirs(os.path.join(dst, rel))
        for pat in patterns:
            for f in glob.glob(os.path.join(ROOT, rel, pat)):
                shutil.copy(f, os.path.join(dst, rel))


@pytest.mark.parametrize("name", list(MUTANTS))
def test_the_second_setting_notices_fx_in_place_of_fy(name, tmp_path, monkeypatch):
    path, old, new, lib, check = MUTANTS[name]
    assert check(), "the committed restatement misses its own check"  # (this also builds the world with the committed restatement)
    tree = str(tmp_path / "tree")
    _copy_tree(tree)
    src = os.path.join(tree, os.path.relpath(lib.SRC, ROOT))
    monkeypatch.setattr(lib, "_L", lib.build(src))
    assert check(), "the unaltered copy misses the check"
    before = open(os.path.join(tree, path)).read().split("\n")
    after = [line.replace(old, new) for line in before]
    changed = sum(a != b for a, b in zip(before, after))
    assert changed >= 1
    with open(os.path.join(tree, path), "w") as f:
        f.write("\n".join(after))
    monkeypatch.setattr(lib, "_L", lib.build(src))
    assert not check(), "%s with %r for %r in %d lines passes the check" % (name, new, old, changed)
