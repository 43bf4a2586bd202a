"""The records of ``include/orbx.h`` the package exchanges with liborbx.so, each described ONCE: a field list in the header's
order, from which ``_record`` makes the ``ctypes.Structure`` subclass, the numpy dtype and ``as_dict``.  RECORDS keeps every
pair under its C struct's name; tests/test_abi_host.py compiles a probe against the header and compares sizes and offsets.
RECORDS_FUSE is a second table of the same form for the records of "fusing map points into a keyframe"
(tests/test_fuse_abi_host.py probes it the same way), RECORDS_LBA a third for the record of "local mapping: local bundle
adjustment" (tests/test_lba_abi_host.py), RECORDS_MAP a fourth for the record of "local mapping: updating the map points"
(tests/test_map_update_abi_host.py), RECORDS_STEREO a fifth for the record of "stereo: matching left and right"
(tests/test_stereo_abi_host.py)."""
from __future__ import annotations

import ctypes
import keyword

import numpy as np

_CTYPES = {"i4": ctypes.c_int32, "f4": ctypes.c_float, "f8": ctypes.c_double}
RECORDS = {}  # C struct name -> (ctypes.Structure subclass or None, numpy dtype)
RECORDS_FUSE = {}  # the same for orbx_fuse_result
RECORDS_LBA = {}  # the same for orbx_lba_result
RECORDS_MAP = {}  # the same for orbx_map_result
RECORDS_STEREO = {}  # the same for orbx_stereo_result


def _as_dict(self) -> dict:
    """The record as a dict: scalars as Python numbers, arrays as numpy arrays of the field's type (or what the field list asks
    for: another shape, or a plain list); `reserved*` fields are left out."""
    d = {}
    for name, kind, shape, form in self._record_fields:
        if name.startswith("reserved"):
            continue
        v = getattr(self, name + "_" if keyword.iskeyword(name) else name)
        if shape is not None:
            v = list(v) if form is list else np.array(v[:], "<" + kind).reshape(form or shape)
        d[name] = v
    return d


def _record(c_name: str, py_name: str, fields, doc: str = None, table: dict = None):
    """(ctypes.Structure subclass, numpy dtype) of one C struct.  A field is (name, kind[, shape[, form]]): kind "i4" / "f4" /
    "f8"; shape None for a scalar, an int or a tuple for an array; form how as_dict returns an array when not as a numpy array of
    `shape` -- another shape, or `list`.  A name that is a Python keyword (lambda) gets a trailing underscore as the ctypes
    attribute and keeps its own name in the dtype and in as_dict.  The pair is kept in `table` (default RECORDS)."""
    norm = []
    for f in fields:
        name, kind, shape, form = (tuple(f) + (None, None))[:4]
        norm.append((name, kind, (shape,) if isinstance(shape, int) else shape, form))
    cfields = []
    for name, kind, shape, _ in norm:
        t = _CTYPES[kind]
        cfields.append((name + "_" if keyword.iskeyword(name) else name, t * int(np.prod(shape)) if shape is not None else t))
    cls = type(py_name, (ctypes.Structure,), {"_fields_": cfields, "_record_fields": tuple(norm), "as_dict": _as_dict,
                                              "__doc__": doc, "__module__": __package__})
    dtype = np.dtype([(n, "<" + k) if s is None else (n, "<" + k, s) for n, k, s, _ in norm])
    assert dtype.itemsize == ctypes.sizeof(cls), c_name
    (RECORDS if table is None else table)[c_name] = (cls, dtype)
    return cls, dtype


def _ints(*names):
    return [(n, "i4") for n in names]


def _floats(*names):
    return [(n, "f4") for n in names]


_M33 = (3, 3)

_Params, _ = _record("orbx_params", "_Params", [("nfeatures", "i4"), ("scale_factor", "f4"), ("nlevels", "i4"), ("ini_th_fast", "i4"),
                                                ("min_th_fast", "i4")])
_Bounds, _ = _record("orbx_bounds", "_Bounds", _ints("min_x", "max_x", "min_y", "max_y"))
_Camera, _ = _record("orbx_camera", "_Camera", _floats("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"))
_Stats, _ = _record("orbx_match_stats", "_Stats", _ints("invalid_by_distance", "invalid_by_ratio", "invalid_by_orientation"))
# mirrors cv::KeyPoint / orbx_keypoint (28 bytes)
_, KEYPOINT_DTYPE = _record("orbx_keypoint", "_Keypoint", _floats("x", "y", "size", "angle", "response") + _ints("octave", "class_id"))
assert KEYPOINT_DTYPE.itemsize == 28

HFResult, HF_RESULT_DTYPE = _record(
    "orbx_hf_result", "HFResult",
    _ints("status", "model", "n_matches", "best_it_h", "best_it_f", "n_inliers_h", "n_inliers_f", "reserved") +
    _floats("score_h", "score_f", "rh") + [("H21", "f4", _M33), ("H12", "f4", _M33), ("F21", "f4", _M33)],
    "orbx_hf_result: what Initializer::Initialize knows after its two RANSAC loops (Initializer.cpp:78-111).")
assert HF_RESULT_DTYPE.itemsize == 4 * (8 + 3 + 27)

InitResult, INIT_RESULT_DTYPE = _record(
    "orbx_init_result", "InitResult",
    _ints("status", "model", "n_matches", "best_it_h", "best_it_f", "n_inliers_h", "n_inliers_f", "n_solutions", "best_solution",
          "best_good", "second_good", "reserved") + _floats("score_h", "score_f", "rh", "parallax") +
    [("R21", "f4", _M33), ("t21", "f4", 3), ("H21", "f4", _M33), ("F21", "f4", _M33)],
    "orbx_init_result: Initializer::Initialize's outcome (status 0 = reconstructed) and the chosen (R21, t21).")
assert INIT_RESULT_DTYPE.itemsize == 184

BAResult, BA_RESULT_DTYPE = _record(
    "orbx_ba_result", "BAResult",
    _ints("status", "n_points", "iterations", "lm_trials", "rejected_trials", "solver_failures", "stop_reason", "reserved") +
    [("chi2_initial", "f8"), ("chi2_final", "f8"), ("lambda", "f8"), ("q", "f8", 4), ("t", "f8", 3), ("R21", "f4", _M33),
     ("t21", "f4", 3), ("median_depth", "f4"), ("reserved2", "f4")],
    "orbx_ba_result: the two-view bundle adjustment's outcome for one pair (status 0 = a usable initial map).")
assert BA_RESULT_DTYPE.itemsize == 168

PoseResult, POSE_RESULT_DTYPE = _record(
    "orbx_pose_result", "PoseResult",
    _ints("status", "n_correspondences", "n_bad", "n_inliers", "rounds") + [("iterations", "i4", 4)] +
    _ints("lm_trials", "rejected_trials", "solver_failures") + [("stop_reason", "i4", 4)] +
    [("chi2_initial", "f8"), ("chi2_final", "f8"), ("lambda", "f8"), ("q", "f8", 4), ("t", "f8", 3), ("R", "f4", _M33),
     ("tcw", "f4", 3)],
    "orbx_pose_result: Optimizer::PoseOptimization's outcome for one problem (n_inliers is the reference design's return value).")
assert POSE_RESULT_DTYPE.itemsize == 192

PnpResult, PNP_RESULT_DTYPE = _record(
    "orbx_pnp_result", "PnpResult",
    _ints("status", "n_correspondences", "min_inliers", "max_its", "its_run", "found_it", "best_it", "refined", "n_inliers",
          "n_best_inliers", "n_refines", "n_degenerate", "beta_choice", "reserved") +
    [("R", "f8", _M33), ("t", "f8", 3), ("Tcw", "f4", 12)],
    "orbx_pnp_result: PnPsolver's outcome for one problem (found_it tells which iterate() turn would have returned it).")
assert PNP_RESULT_DTYPE.itemsize == 200

Sim3Result, SIM3_RESULT_DTYPE = _record(
    "orbx_sim3_result", "Sim3Result",
    _ints("status", "n_correspondences", "max_its", "its_run", "found_it", "best_it", "n_inliers", "n_best_inliers", "n_degenerate") +
    [("reserved", "i4", 2), ("s12", "f4"), ("R12", "f4", _M33), ("t12", "f4", 3)],
    "orbx_sim3_result: Sim3Solver's outcome for one keyframe pair (found_it tells which iterate() turn would have returned it).")
assert SIM3_RESULT_DTYPE.itemsize == 96

# (iterations and stop_reason are plain lists in this record's as_dict, numpy arrays in PoseResult's)
Sim3OptResult, SIM3OPT_RESULT_DTYPE = _record(
    "orbx_sim3opt_result", "Sim3OptResult",
    _ints("status", "n_correspondences", "n_bad", "n_inliers", "rounds") + [("iterations", "i4", 2, list)] +
    _ints("lm_trials", "rejected_trials", "solver_failures") + [("stop_reason", "i4", 2, list)] +
    _ints("small_theta", "small_sigma", "small_both", "reserved") +
    [("chi2_initial", "f8"), ("chi2_final", "f8"), ("lambda", "f8"), ("q", "f8", 4), ("t", "f8", 3), ("s", "f8"), ("s12", "f4"),
     ("R12", "f4", _M33), ("t12", "f4", 3), ("reserved_f", "f4")],
    "orbx_sim3opt_result: Optimizer::OptimizeSim3's outcome for one keyframe pair (n_inliers is the design's return value).")
assert SIM3OPT_RESULT_DTYPE.itemsize == 208

PROJ_RESULT_FIELDS = ("status", "nmatches", "n_points", "n_in_image", "n_with_candidates", "n_displaced", "n_rot_removed", "rounds")
ProjResult, PROJ_RESULT_DTYPE = _record(
    "orbx_proj_result", "ProjResult", _ints(*PROJ_RESULT_FIELDS),
    "orbx_proj_result: ORBmatcher::SearchByProjection's counters for one pair (rounds is the device's own count).")
assert PROJ_RESULT_DTYPE.itemsize == 32

LOCAL_RESULT_FIELDS = ("status", "nmatches", "n_points", "n_seen", "n_behind", "n_out_image", "n_out_distance", "n_out_angle", "n_in_view",
                       "n_with_candidates", "n_over_th", "n_ratio_rejected", "n_displaced", "n_outliers_cleared", "rounds")
LocalResult, LOCAL_RESULT_DTYPE = _record(
    "orbx_local_result", "LocalResult", _ints(*LOCAL_RESULT_FIELDS),
    "orbx_local_result: SearchLocalPoints' counters for one (frame, map set) pair (rounds is the device's own count).")
assert LOCAL_RESULT_DTYPE.itemsize == 60

SCW_RESULT_FIELDS = ("status", "nmatches", "n_total", "n_points", "n_found", "n_unmapped", "n_behind", "n_out_image", "n_out_distance",
                     "n_out_angle", "n_with_candidates", "n_over_dist", "n_displaced", "rounds")
MatchScwResult, SCW_RESULT_DTYPE = _record(
    "orbx_scw_result", "MatchScwResult", _ints(*SCW_RESULT_FIELDS),
    """orbx_scw_result: the counters of the loop-closing SearchByProjection under Scw for one (keyframe, map set) pair (rounds is
    the device's own count; n_total is ComputeSim3's nTotalMatches).""")
assert SCW_RESULT_DTYPE.itemsize == 56

KFPROJ_RESULT_FIELDS = ("status", "nmatches", "n_points", "n_found", "n_behind_kept", "n_out_image", "n_out_distance", "n_with_candidates",
                        "n_over_dist", "n_displaced", "n_rot_removed", "n_outliers_cleared", "rounds")
KfProjResult, KFPROJ_RESULT_DTYPE = _record(
    "orbx_kfproj_result", "KfProjResult", _ints(*KFPROJ_RESULT_FIELDS),
    """orbx_kfproj_result: the counters of the relocalisation SearchByProjection for one (keyframe, frame) pair (rounds is the
    device's own count).""")
assert KFPROJ_RESULT_DTYPE.itemsize == 52

MSIM3_RESULT_FIELDS = ("status", "n_found", "n_points_12", "n_behind_12", "n_out_image_12", "n_out_distance_12", "n_with_candidates_12",
                       "n_over_dist_12", "n_points_21", "n_behind_21", "n_out_image_21", "n_out_distance_21", "n_with_candidates_21",
                       "n_over_dist_21", "n_one_sided", "reserved")
MatchSim3Result, MSIM3_RESULT_DTYPE = _record(
    "orbx_msim3_result", "MatchSim3Result", _ints(*MSIM3_RESULT_FIELDS),
    "orbx_msim3_result: the counters of ORBmatcher::SearchBySim3 for one (KF1, KF2) pair, per direction.")
assert MSIM3_RESULT_DTYPE.itemsize == 64

TRI_MATCH_COUNTERS = ("status", "nmatches", "n_queries", "n_with_candidates", "n_epipole_rejected", "n_epiline_rejected", "n_rot_removed")
# (F12 is nine floats in the dtype and 3x3 in as_dict)
TriMatchResult, TRI_MATCH_RESULT_DTYPE = _record(
    "orbx_tri_match_result", "TriMatchResult", _ints(*TRI_MATCH_COUNTERS) + _floats("baseline", "ex", "ey") + [("F12", "f4", 9, _M33)],
    "orbx_tri_match_result: SearchForTriangulation's counters and the pair's geometry (baseline, epipole, F12 row-major).")
assert TRI_MATCH_RESULT_DTYPE.itemsize == 76

TRI_RESULT_FIELDS = ("status", "n_matches", "n_points", "n_low_parallax", "n_w_zero", "n_behind_1", "n_behind_2", "n_reproj_1", "n_reproj_2",
                     "n_zero_dist", "n_scale")
TriResult, TRI_RESULT_DTYPE = _record(
    "orbx_tri_result", "TriResult", _ints(*TRI_RESULT_FIELDS),
    "orbx_tri_result: CreateNewMapPoints' counters for one (KF1, KF2) pair, one per gate.")
assert TRI_RESULT_DTYPE.itemsize == 44

FUSE_RESULT_FIELDS = ("status", "n_fused", "n_points", "n_in_kf", "n_behind", "n_out_image", "n_out_distance", "n_out_angle",
                      "n_with_candidates", "n_over_dist", "n_added", "n_kept_occupant", "n_replaced_occupant", "n_bad_occupant", "n_chained",
                      "rounds")
FuseResult, FUSE_RESULT_DTYPE = _record(
    "orbx_fuse_result", "FuseResult", _ints(*FUSE_RESULT_FIELDS),
    """orbx_fuse_result: ORBmatcher::Fuse's counters for one (keyframe, map set) pair, either overload (n_fused is the design's
    return value; rounds is the device's own count).""", table=RECORDS_FUSE)
assert FUSE_RESULT_DTYPE.itemsize == 64

# (the per-round fields are plain lists of two in as_dict)
LBA_ROUND_FIELDS = ("iterations", "lm_trials", "rejected_trials", "solver_failures", "stop_reason", "n_active_points", "n_active_free")
LbaResult, LBA_RESULT_DTYPE = _record(
    "orbx_lba_result", "LbaResult",
    _ints("status", "n_points", "n_edges", "n_free") + [(n, "i4", 2, list) for n in LBA_ROUND_FIELDS] + _ints("n_level1", "n_erased") +
    [("chi2_initial", "f8", 2, list), ("chi2_final", "f8", 2, list), ("lambda", "f8", 2, list)],
    """orbx_lba_result: Optimizer::LocalBundleAdjustment's outcome for one problem, per round where a field has two entries
    (n_erased is the size of vToErase).""", table=RECORDS_LBA)
assert LBA_RESULT_DTYPE.itemsize == 128

MAP_RESULT_FIELDS = ("status", "n_points", "n_observations", "n_erased", "n_bad_points", "n_cleared", "n_ref_moved", "max_observers",
                     "n_free")
MapResult, MAP_RESULT_DTYPE = _record(
    "orbx_map_result", "MapResult", _ints(*MAP_RESULT_FIELDS) + [("reserved", "i4", 7, list)],
    """orbx_map_result: what the update of the map points behind a local bundle adjustment did for one problem (n_erased:
    vToErase applied; n_bad_points: EraseObservation's SetBadFlag).""", table=RECORDS_MAP)
assert MAP_RESULT_DTYPE.itemsize == 64

STEREO_RESULT_FIELDS = ("status", "n_matches", "n_with_candidates", "n_orb_matched", "n_window_refused", "n_out_of_level", "n_edge",
                        "n_delta_refused", "n_disparity_refused", "n_clamped", "n_before_median", "median_sad", "th_dist",
                        "n_removed_by_median")
StereoResult, STEREO_RESULT_DTYPE = _record(
    "orbx_stereo_result", "StereoResult",
    [(n, "f4" if n == "th_dist" else "i4") for n in STEREO_RESULT_FIELDS] + [("reserved", "i4", 2, list)],
    """orbx_stereo_result: what Frame::ComputeStereoMatches did for one rig, a counter per place a left keypoint can end in
    (n_before_median: the matches rule 11 kept; n_matches: those the median filter left).""", table=RECORDS_STEREO)
assert STEREO_RESULT_DTYPE.itemsize == 64
