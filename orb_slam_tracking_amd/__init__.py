"""orb_slam_tracking_amd — MI355X-native ORB extraction + initialization matching.

Thin ctypes mirror of the C ABI in ``include/orbx.h`` (``liborbx.so``: hand-written HIP kernels for gfx950 plus the
C++ host pipeline).  The classes keep the names and argument meaning of the reference's C++ interface for this path:

* ``ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)`` / ``__call__``  -- Features/ORBextractor.hpp:68-85
* ``ORBmatcher(nnratio=0.6, checkOri=True).SearchForInitialization(F1, F2, windowSize=100)`` -- Features/ORBmatcher.hpp:15,36
* ``Frame`` -- the part of SlamTypes/Frame.{hpp,cpp} the matcher reads (mvKeys, mvKeysUn, mDescriptors, N, image bounds), and
  ``ComputeBoW`` (mBowVec / mFeatVec) with a ``Vocabulary`` (Features/ORBVocabulary.hpp: DBoW2's TemplatedVocabulary<FORB>)

There is NO CPU fallback: importing works anywhere, but every compute call raises ``OrbxError`` unless liborbx.so is
built and a HIP device is usable.  (The C++ drop-in classes live in include/orbx_shim.hpp.)
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import os
from typing import Optional, Sequence, Tuple

import numpy as np

__all__ = ["KEYPOINT_DTYPE", "OrbxError", "ORBextractor", "ORBmatcher", "Frame", "lib", "lib_path",
           "HFResult", "HF_RESULT_DTYPE", "Vocabulary", "BowResult", "BOW_MAX_FEATURES", "Database", "DB_MAX_RESULTS", "debug_database_shape", "InitResult", "INIT_RESULT_DTYPE", "BAResult", "BA_RESULT_DTYPE", "BA_SKIPPED", "BA_BAD_INPUT", "BA_NONFINITE", "BA_FEW_POINTS", "BA_NEGATIVE_DEPTH", "PoseResult", "POSE_RESULT_DTYPE", "POSE_BAD_INPUT", "POSE_NONFINITE", "POSE_FEW_POINTS", "PnpResult", "PNP_RESULT_DTYPE", "PNP_BAD_INPUT", "PNP_NONFINITE", "PNP_FEW_POINTS", "PNP_BAD_DRAWS", "PNP_NO_POSE", "PNP_RAND_MAX", "PnPsolver", "sample_pnp_draws", "Sim3Result", "SIM3_RESULT_DTYPE", "SIM3_BAD_INPUT", "SIM3_NONFINITE", "SIM3_FEW_POINTS", "SIM3_BAD_DRAWS", "SIM3_NO_RESULT", "Sim3Solver", "sample_sim3_draws", "MatchSim3Result", "MSIM3_RESULT_DTYPE", "MSIM3_BAD_INPUT", "MSIM3_NONFINITE", "ProjResult", "PROJ_RESULT_DTYPE", "PROJ_BAD_INPUT", "PROJ_NONFINITE", "LocalResult", "LOCAL_RESULT_DTYPE", "LOCAL_BAD_INPUT", "LOCAL_NONFINITE", "LOCAL_NOT_IN_VIEW", "LOCAL_SEEN", "KfProjResult", "KFPROJ_RESULT_DTYPE", "KFPROJ_BAD_INPUT", "KFPROJ_NONFINITE", "TriMatchResult", "TRI_MATCH_RESULT_DTYPE", "TriResult", "TRI_RESULT_DTYPE", "TRI_BAD_INPUT", "TRI_NONFINITE", "TRI_LOW_BASELINE", "TRI_ZERO_BASELINE", "Optimizer", "sample_sets", "INIT_TOO_FEW_MATCHES", "INIT_BAD_SETS", "INIT_NO_SCORE", "INIT_BAD_MATCHES",
           "STAGES", "E_EMPTY", "E_BADARG", "E_TOOSMALL", "E_HIP", "E_CAPACITY", "E_RCCL",
           "Sim3OptResult", "SIM3OPT_RESULT_DTYPE", "SIM3OPT_BAD_INPUT", "SIM3OPT_NONFINITE",
           "MatchScwResult", "SCW_RESULT_DTYPE", "SCW_BAD_INPUT", "SCW_NONFINITE", "SCW_TAKEN_UNMAPPED", "loop_accepted",
           "MapFuser", "FuseResult", "FUSE_RESULT_DTYPE", "FUSE_BAD_INPUT", "FUSE_NONFINITE", "FUSE_OCCUPIED_UNMAPPED", "FUSE_NONE",
           "FUSE_ADD", "FUSE_KEEP_OCCUPANT", "FUSE_REPLACE_OCCUPANT", "FUSE_BAD_OCCUPANT",
           "LbaResult", "LBA_RESULT_DTYPE", "LBA_BAD_INPUT", "LBA_NONFINITE", "LBA_MAX_FREE",
           "MapResult", "MAP_RESULT_DTYPE", "MAP_RESULT_FIELDS", "MAP_NORMALS", "MAP_DESCRIPTORS", "MAP_BAD_INPUT", "MAP_NONFINITE",
           "StereoResult", "STEREO_RESULT_DTYPE", "STEREO_RESULT_FIELDS", "STEREO_BAD_INPUT", "STEREO_NONFINITE"]

from ._records import (KEYPOINT_DTYPE, _Params, _Bounds, _Camera, _Stats, HFResult, HF_RESULT_DTYPE, InitResult,  # noqa: F401
                       INIT_RESULT_DTYPE, BAResult, BA_RESULT_DTYPE, PoseResult, POSE_RESULT_DTYPE, PnpResult, PNP_RESULT_DTYPE,
                       Sim3Result, SIM3_RESULT_DTYPE, Sim3OptResult, SIM3OPT_RESULT_DTYPE, ProjResult, PROJ_RESULT_DTYPE,
                       PROJ_RESULT_FIELDS, LocalResult, LOCAL_RESULT_DTYPE, LOCAL_RESULT_FIELDS, MatchScwResult, SCW_RESULT_DTYPE,
                       SCW_RESULT_FIELDS, KfProjResult, KFPROJ_RESULT_DTYPE, KFPROJ_RESULT_FIELDS, MatchSim3Result,
                       MSIM3_RESULT_DTYPE, MSIM3_RESULT_FIELDS, TriMatchResult, TRI_MATCH_RESULT_DTYPE, TRI_MATCH_COUNTERS,
                       TriResult, TRI_RESULT_DTYPE, TRI_RESULT_FIELDS, FuseResult, FUSE_RESULT_DTYPE, FUSE_RESULT_FIELDS,
                       LbaResult, LBA_RESULT_DTYPE, MapResult, MAP_RESULT_DTYPE, MAP_RESULT_FIELDS, StereoResult,
                       STEREO_RESULT_DTYPE, STEREO_RESULT_FIELDS)

E_EMPTY, E_BADARG, E_TOOSMALL, E_HIP, E_CAPACITY, E_RCCL = -1, -2, -3, -4, -5, -6
_ERRNAMES = {-1: "ORBX_E_EMPTY", -2: "ORBX_E_BADARG", -3: "ORBX_E_TOOSMALL", -4: "ORBX_E_HIP", -5: "ORBX_E_CAPACITY", -6: "ORBX_E_RCCL"}
STAGES = ("pyramid", "fast", "select", "describe", "match")


class OrbxError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        super().__init__("%s (%d)%s" % (_ERRNAMES.get(code, "ORBX_E_?"), code, (": " + what) if what else ""))


# the status bits of the records (_records.py), as include/orbx.h names them
INIT_TOO_FEW_MATCHES, INIT_BAD_SETS, INIT_NO_SCORE, INIT_BAD_MATCHES = 1, 2, 4, 128
INIT_AMBIGUOUS, INIT_LOW_PARALLAX, INIT_FEW_TRIANGULATED, INIT_FEW_INLIERS = 8, 16, 32, 64
BA_SKIPPED, BA_BAD_INPUT, BA_NONFINITE, BA_FEW_POINTS, BA_NEGATIVE_DEPTH = 1, 2, 4, 8, 16
POSE_BAD_INPUT, POSE_NONFINITE, POSE_FEW_POINTS = 2, 4, 8
PNP_BAD_INPUT, PNP_NONFINITE, PNP_FEW_POINTS, PNP_BAD_DRAWS, PNP_NO_POSE = 2, 4, 8, 16, 32
PNP_RAND_MAX = 2147483647
SIM3_BAD_INPUT, SIM3_NONFINITE, SIM3_FEW_POINTS, SIM3_BAD_DRAWS, SIM3_NO_RESULT = 2, 4, 8, 16, 32
SIM3OPT_BAD_INPUT, SIM3OPT_NONFINITE = 2, 4
LBA_BAD_INPUT, LBA_NONFINITE, LBA_MAX_FREE = 2, 4, 64
MAP_NORMALS, MAP_DESCRIPTORS, MAP_BAD_INPUT, MAP_NONFINITE = 1, 2, 2, 4
STEREO_BAD_INPUT, STEREO_NONFINITE = 2, 4
PROJ_BAD_INPUT, PROJ_NONFINITE = 2, 4
LOCAL_BAD_INPUT, LOCAL_NONFINITE, LOCAL_NOT_IN_VIEW, LOCAL_SEEN = 2, 4, 0xFF, 0xFE
SCW_BAD_INPUT, SCW_NONFINITE, SCW_TAKEN_UNMAPPED = 2, 4, -2
FUSE_BAD_INPUT, FUSE_NONFINITE, FUSE_OCCUPIED_UNMAPPED = 2, 4, -2
FUSE_NONE, FUSE_ADD, FUSE_KEEP_OCCUPANT, FUSE_REPLACE_OCCUPANT, FUSE_BAD_OCCUPANT = 0, 1, 2, 3, 4
KFPROJ_BAD_INPUT, KFPROJ_NONFINITE = 2, 4
MSIM3_BAD_INPUT, MSIM3_NONFINITE = 2, 4
TRI_BAD_INPUT, TRI_NONFINITE, TRI_LOW_BASELINE, TRI_ZERO_BASELINE = 2, 4, 8, 16


def _sample_draws(rand, n_iter: int, width: int) -> np.ndarray:
    out = np.zeros((int(n_iter), width), np.int32)
    for row in out:
        for j in range(width):
            row[j] = int(rand())
    return out


def sample_pnp_draws(rand, n_iter: int) -> np.ndarray:
    """The draws of n_iter PnP RANSAC hypotheses, int32 [n_iter, 4]: the next 4 * n_iter values of `rand`, a callable returning
    the host's next rand() value (as sample_sets takes it), in the order PnPsolver::iterate would draw them.  The device turns
    them into indices itself (DUtils::Random::RandomInt and the swap-and-pop), so the caller need not know N."""
    return _sample_draws(rand, n_iter, 4)


def sample_sim3_draws(rand, n_iter: int) -> np.ndarray:
    """The draws of n_iter Sim3 RANSAC hypotheses, int32 [n_iter, 3]: the next 3 * n_iter values of `rand`, as sample_pnp_draws
    takes them, in the order Sim3Solver::iterate would draw them."""
    return _sample_draws(rand, n_iter, 3)


def _libc_rand():
    """glibc's rand(), the default random stream of PnPsolver and Sim3Solver (the reference's)."""
    libc = ctypes.CDLL(None)
    libc.rand.restype = ctypes.c_int
    return libc.rand



def loop_accepted(opt_res, scw_res, min_inliers: int = 20, min_total: int = 40) -> np.ndarray:
    """LoopClosing::ComputeSim3's two gates over HOST record arrays (SIM3OPT_RESULT_DTYPE and SCW_RESULT_DTYPE, or their bytes):
    accepted[p] = opt_res[p].n_inliers >= 20 and scw_res[p].n_total >= 40.  It orders nothing: device arrays go through
    ORBextractor.loop_accepted, which reads them back behind the context's work; given one, this function refuses."""
    def host(a, dtype):
        if not isinstance(a, np.ndarray):
            raise OrbxError(E_BADARG, "loop_accepted takes host record arrays; device arrays go through ORBextractor.loop_accepted")
        return a.reshape(-1) if a.dtype == dtype else np.ascontiguousarray(a).reshape(-1).view(np.uint8).view(dtype)
    o, m = host(opt_res, SIM3OPT_RESULT_DTYPE), host(scw_res, SCW_RESULT_DTYPE)
    if len(o) != len(m):
        raise OrbxError(E_BADARG, "the two result arrays must have one record per pair")
    return (o["n_inliers"] >= int(min_inliers)) & (m["n_total"] >= int(min_total))


def sample_sets(n_matches: int, n_iter: int, rand) -> np.ndarray:
    """mvSets as Initializer::Initialize draws them (Initializer.cpp:50-63): per iteration 8 distinct indices into
    mvMatches12, each `rand() % available` with swap-with-last removal.  `rand` is a callable returning the host's next rand()
    value (tests pass glibc's through ctypes), so the caller's random stream advances exactly as the reference's would.
    n_matches < 8 raises ValueError (the reference computes rand() % 0 there)."""
    n_matches, n_iter = int(n_matches), int(n_iter)
    if n_matches < 8:
        raise ValueError("sample_sets needs at least 8 matches (rand() %% 0 upstream), got %d" % n_matches)
    out = np.zeros((n_iter, 8), np.int32)
    for it in range(n_iter):
        avail = list(range(n_matches))
        for j in range(8):
            randi = int(rand()) % len(avail)
            out[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


def lib_path() -> str:
    # ORBX_LIB (diagnostics): another build of the same sources, e.g. `make -C csrc VARIANT=name EXTRA=...` for an A/B comparison
    return os.environ.get("ORBX_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "liborbx.so")


_LIB = None


def _one_hip_runtime() -> None:
    """One HIP runtime per process.  liborbx.so needs `libamdhip64.so.7`; PyTorch-ROCm ships its own copy of that library and loads
    it by path.  If torch is imported first, liborbx resolves to torch's copy (same SONAME) and both share devices, streams and
    memory.  The other order used to give the process two runtimes -- the second one finds no device (`orbx_create` ->
    ORBX_E_HIP).  So when torch is installed but not yet imported, its copy is loaded here, before liborbx, without importing torch."""
    import sys
    if "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(p):
            ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)
    except Exception:  # no torch, or an unusual layout: liborbx takes the system's runtime
        pass


def hip_runtimes_mapped() -> list:
    """The distinct libamdhip64 files mapped into this process (Linux).  More than one means two HIP runtimes: the pre-load above
    only helps when torch's copy carries the SONAME liborbx.so was linked against (libamdhip64.so.7) -- a torch wheel built against
    another ROCm major leaves the process with both, and the second one finds no device."""
    try:
        return sorted(set(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    except OSError:
        return []


def lib() -> ctypes.CDLL:
    """Loads liborbx.so (built in-tree by ``__graft_entry__.build()`` / ``make -C orb_slam_tracking_amd/csrc``)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise OrbxError(E_HIP, "liborbx.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
    _one_hip_runtime()
    L = ctypes.CDLL(path)
    vp, i32, f32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    L.orbx_create.argtypes = [ctypes.POINTER(_Params), i32, i32, i32, i32, vp, ctypes.POINTER(vp)]
    L.orbx_destroy.argtypes = [vp]
    L.orbx_destroy.restype = None
    L.orbx_last_error.argtypes = [vp]
    L.orbx_last_error.restype = ctypes.c_char_p
    L.orbx_get_levels.argtypes = [vp]
    L.orbx_get_scale_factor.argtypes = [vp]
    L.orbx_get_scale_factor.restype = f32
    L.orbx_get_tables.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbx_get_umax.argtypes = [vp, vp]
    L.orbx_extract.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp]
    L.orbx_host_register.argtypes = [vp, vp, sz]
    L.orbx_host_unregister.argtypes = [vp, vp]
    L.orbx_extract_batch.argtypes = [vp, i32, vp, i32, i32, i32, sz, i32, i32, vp, vp, i32, vp, vp]
    L.orbx_extract_batch_device.argtypes = [vp, i32, vp, i32, i32, i32, sz, vp, vp, i32, vp]
    L.orbx_level_size.argtypes = [vp, i32, vp, vp]
    L.orbx_download_pyramid.argtypes = [vp, i32, i32, i32, vp, i32]
    L.orbx_match_init.argtypes = [vp, vp, vp, i32, vp, vp, i32, ctypes.POINTER(_Bounds), i32, f32, i32, vp,
                                  ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_Stats)]
    L.orbx_match_init_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, ctypes.POINTER(_Bounds), i32, f32, i32,
                                               vp, vp, vp]
    L.orbx_extract_match_batch_device.argtypes = [vp, i32, vp, i32, i32, i32, sz, vp, vp, i32, vp, i32, vp, vp,
                                                  ctypes.POINTER(_Bounds), i32, f32, i32, vp, vp, vp]
    L.orbx_extract_match_batch_device_async.argtypes = [vp, i32, vp, i32, i32, i32, sz, vp, vp, i32, vp, i32, vp, vp,
                                                  ctypes.POINTER(_Bounds), i32, f32, i32, vp, vp, vp]
    L.orbx_extract_match_batch_host_async.argtypes = L.orbx_extract_match_batch_device_async.argtypes
    L.orbx_set_opencv_variant.argtypes = [vp, i32, i32]
    L.orbx_set_libm_variant.argtypes = [vp, i32]
    L.orbx_set_pipeline_depth.argtypes = [vp, i32]
    L.orbx_wait_one.argtypes = [vp]
    L.orbx_wait.argtypes = [vp]
    L.orbx_order_after.argtypes = [vp, vp]
    L.orbx_order_before.argtypes = [vp, vp]
    L.orbx_profile_stages.argtypes = [vp, ctypes.c_uint]
    L.orbx_undistort_keypoints.argtypes = [vp, vp, i32, ctypes.POINTER(_Camera), vp]
    L.orbx_undistort_batch_device.argtypes = [vp, i32, vp, vp, i32, ctypes.POINTER(_Camera), vp]
    L.orbx_image_bounds.argtypes = [vp, ctypes.POINTER(_Camera), i32, i32, ctypes.POINTER(_Bounds)]
    L.orbx_to_gray.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32]
    L.orbx_to_gray_batch_device.argtypes = [vp, i32, vp, i32, i32, i32, sz, i32, i32, vp, i32, sz]
    L.orbx_check_homography.argtypes = [vp, i32, vp, vp, vp, i32, vp, i32, vp, f32, vp, vp, vp, vp]
    L.orbx_check_fundamental.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, f32, vp, vp, vp, vp]
    L.orbx_check_rt.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, f32, vp, vp, vp, vp]
    L.orbx_find_models_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, f32, vp, vp, vp, vp]
    L.orbx_find_models.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, f32, ctypes.POINTER(HFResult), vp, vp, vp]
    L.orbx_initialize_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, f32, f32, i32, vp, vp, vp]
    L.orbx_initialize.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, vp, f32, f32, i32, ctypes.POINTER(InitResult), vp, vp]
    L.orbx_bundle_adjust_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]
    L.orbx_bundle_adjust.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, ctypes.POINTER(BAResult), vp]
    L.orbx_pose_optimize_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp]
    L.orbx_pose_optimize.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32, ctypes.POINTER(PoseResult), vp]
    f64 = ctypes.c_double
    L.orbx_pnp_ransac_table.argtypes = [f64, i32, i32, f32, i32, vp]
    L.orbx_pnp_solve_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, f64, i32, i32, f32, f32, i32,
                                              vp, vp, vp, vp, vp]
    L.orbx_pnp_solve.argtypes = [vp, vp, i32, vp, vp, vp, vp, f64, i32, i32, f32, f32, i32, vp, ctypes.POINTER(PnpResult), vp]
    L.orbx_sim3_ransac_table.argtypes = [f64, i32, i32, i32, vp]
    L.orbx_sim3_solve_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, i32, f64, i32, i32,
                                               f32, i32, vp, vp, vp, vp, vp]
    L.orbx_match_sim3_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp,
                                               ctypes.POINTER(_Bounds), f32, i32, vp, vp]
    L.orbx_match_sim3.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(_Bounds),
                                  f32, i32, vp, ctypes.POINTER(MatchSim3Result)]
    L.orbx_sim3_solve.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, f64, i32, i32, f32, i32, vp,
                                  ctypes.POINTER(Sim3Result), vp, vp, vp]
    L.orbx_optimize_sim3_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, f32,
                                                  i32, i32, vp, vp]
    L.orbx_optimize_sim3.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32,
                                     ctypes.POINTER(Sim3OptResult), vp]
    L.orbx_match_scw_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp,
                                              ctypes.POINTER(_Bounds), f32, i32, vp, vp, vp]
    L.orbx_match_scw.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(_Bounds), f32, i32, vp, vp, i32,
                                 ctypes.POINTER(MatchScwResult)]
    L.orbx_sim3_compose_scw_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.orbx_sim3_compose_scw.argtypes = [vp, vp, vp, vp]
    L.orbx_fuse_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                         ctypes.POINTER(_Bounds), f32, i32, vp, vp, vp, vp, vp, vp]
    L.orbx_fuse_scw_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp,
                                             ctypes.POINTER(_Bounds), f32, i32, vp, vp, vp, vp, vp, vp]
    L.orbx_fuse.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(_Bounds), f32, i32, vp, vp, vp, vp, vp,
                            ctypes.POINTER(FuseResult)]
    L.orbx_fuse_scw.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(_Bounds), f32, i32, vp, vp, vp, vp, vp,
                                ctypes.POINTER(FuseResult)]
    L.orbx_local_ba_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32,
                                             vp, vp, vp, vp]
    L.orbx_local_ba.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, ctypes.POINTER(LbaResult)]
    L.orbx_debug_local_ba_lds_max_free.argtypes = [i32]
    L.orbx_map_update_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp,
                                               i32, vp, vp, vp, vp, vp]
    L.orbx_map_update.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, ctypes.POINTER(MapResult)]
    L.orbx_stereo_match_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, ctypes.c_float, ctypes.c_float, vp, vp, vp, vp, vp, vp, vp,
                                                 vp, vp, vp]
    L.orbx_extract_stereo.argtypes = [vp, vp, vp, i32, i32, i32, ctypes.c_float, ctypes.c_float, vp, vp, vp, vp, vp, vp, i32, vp, vp,
                                      ctypes.POINTER(StereoResult)]
    L.orbx_vocabulary_parse_text.argtypes = [ctypes.c_char_p, vp, vp, vp, vp, vp, vp, i32]
    L.orbx_vocabulary_create.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, ctypes.POINTER(vp)]
    L.orbx_vocabulary_load_text.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp)]
    L.orbx_vocabulary_destroy.argtypes = [vp]
    L.orbx_vocabulary_destroy.restype = None
    L.orbx_vocabulary_info.argtypes = [vp, vp]
    L.orbx_vocabulary_get_nodes.argtypes = [vp, vp, vp, vp, vp, i32]
    L.orbx_vocabulary_save_text.argtypes = [vp, ctypes.c_char_p, i32]
    L.orbx_vocabulary_train_device.argtypes = [vp, i32, i32, i32, i32, ctypes.c_uint64, i32, i32, vp, vp, i32, ctypes.POINTER(vp), vp, vp]
    L.orbx_vocabulary_train.argtypes = [vp, i32, i32, i32, i32, ctypes.c_uint64, i32, i32, vp, vp, ctypes.POINTER(vp), vp, vp]
    L.orbx_debug_voc_train_seed_grid_min.argtypes = [ctypes.c_longlong]
    L.orbx_bow_transform_batch_device.argtypes = [vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbx_bow_transform.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbx_bow_score_batch_device.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    L.orbx_bow_score.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, vp]
    L.orbx_match_bow_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, f32, i32, vp, vp]
    L.orbx_match_bow.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, f32, i32, vp, vp]
    L.orbx_match_projection_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp,
                                                     ctypes.POINTER(_Bounds), f32, i32, vp, vp]
    L.orbx_match_projection.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, ctypes.POINTER(_Bounds), f32, i32, vp,
                                        ctypes.POINTER(ProjResult)]
    L.orbx_match_local_map_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp,
                                                    ctypes.POINTER(_Bounds), f32, f32, vp, vp, vp, vp]
    L.orbx_match_local_map.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(_Bounds), f32, f32, vp, vp, vp,
                                       ctypes.POINTER(LocalResult)]
    L.orbx_match_keyframe_projection_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp,
                                                              ctypes.POINTER(_Bounds), f32, i32, i32, vp, vp, vp]
    L.orbx_match_keyframe_projection.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, ctypes.POINTER(_Bounds), f32,
                                                 i32, i32, vp, vp, ctypes.POINTER(KfProjResult)]
    L.orbx_match_triangulation_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]
    L.orbx_match_triangulation.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, f32, i32, vp,
                                           ctypes.POINTER(TriMatchResult)]
    L.orbx_triangulate_matches_batch_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbx_triangulate_matches.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(TriResult)]
    L.orbx_database_create.argtypes = [vp, vp, ctypes.POINTER(vp)]
    L.orbx_database_destroy.argtypes = [vp]
    L.orbx_database_destroy.restype = None
    L.orbx_database_clear.argtypes = [vp]
    L.orbx_database_size.argtypes = [vp]
    L.orbx_database_add_batch_device.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp]
    L.orbx_database_query_batch_device.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.orbx_database_add.argtypes = [vp, vp, vp, vp, i32, vp]
    L.orbx_database_query.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.orbx_database_get_inverted_file.argtypes = [vp, vp, vp, vp, ctypes.c_int64]
    L.orbx_database_get_inverted_file.restype = ctypes.c_int64
    L.orbx_debug_database_shape.argtypes = [i32, i32]
    L.orbx_multi_create.argtypes = [ctypes.POINTER(_Params), i32, vp, i32, i32, i32, ctypes.POINTER(vp)]
    L.orbx_multi_destroy.argtypes = [vp]
    L.orbx_multi_destroy.restype = None
    L.orbx_multi_size.argtypes = [vp]
    L.orbx_multi_ctx.argtypes = [vp, i32]
    L.orbx_multi_ctx.restype = vp
    L.orbx_multi_last_error.argtypes = [vp]
    L.orbx_multi_last_error.restype = ctypes.c_char_p
    L.orbx_multi_shard_range.argtypes = [i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.orbx_multi_extract_match_batch_device.argtypes = [vp, i32, vp, i32, i32, i32, sz, vp, vp, i32, vp, ctypes.POINTER(_Bounds), i32,
                                                        f32, i32, vp, vp, vp]
    L.orbx_multi_extract_match_batch_device_async.argtypes = L.orbx_multi_extract_match_batch_device.argtypes
    L.orbx_multi_set_pipeline_depth.argtypes = [vp, i32]
    L.orbx_multi_wait_one.argtypes = [vp]
    L.orbx_multi_wait.argtypes = [vp]
    L.orbx_profile_enable.argtypes = [vp, i32]
    L.orbx_profile_reset.argtypes = [vp]
    L.orbx_profile_get.argtypes = [vp, vp, vp]
    L.orbx_debug_candidates.argtypes = [vp, i32, i32, vp, i32]
    L.orbx_debug_distribute_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, i32]
    L.orbx_debug_std_sort.argtypes = [vp, vp, i32]
    L.orbx_debug_sincos.argtypes = [vp, vp, i32, vp, vp]
    L.orbx_debug_set.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
    L.orbx_debug_last_launch.argtypes = [vp, vp]
    L.orbx_debug_pyr_cols.argtypes = [ctypes.c_int, ctypes.c_int, vp]
    L.orbx_debug_fast_cells.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp]
    L.orbx_debug_match_counters.argtypes = [vp, vp]
    L.orbx_debug_selection_units.argtypes = [vp, i32, vp, vp]
    L.orbx_debug_path_codes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    _LIB = L
    # The library reads no environment variable; the profiling scripts' ORBX_<KNOB> settings are forwarded to orbx_debug_set here
    # (diagnostic knobs, csrc/orbx_knobs.h: they choose among kernels / launch shapes with identical results).
    for name in KNOBS:
        v = os.environ.get("ORBX_" + name.upper())
        if v is not None:
            debug_set(name, _knob_value(name, v))
    return L


KNOBS = ("no_bands", "pyr_bands", "pyr_strips", "bands_min_frames", "no_split", "lat_trace", "fast_wg_max_cells", "match_no_general",
         "match_no_mfma", "oct_big_depth", "oct_big_no_fallback", "multi_force_rccl")
KNOB_UNSET = -(1 << 63)


def _knob_value(name: str, text: str) -> int:
    try:
        return int(text)
    except ValueError:
        return 1  # (a flag set to anything: on)


def debug_set(name: str, value: Optional[int]) -> None:
    """Diagnostic knob of the library (orbx_debug_set, include/orbx.h): `None` unsets it."""
    r = lib().orbx_debug_set(name.encode(), KNOB_UNSET if value is None else int(value))
    if r != 0:
        raise OrbxError(r, "orbx_debug_set(%r)" % name)


@contextlib.contextmanager
def knobs(**values: Optional[int]):
    """Sets diagnostic knobs (`debug_set`) for the body of a `with` statement and unsets them afterwards, also when the body raises."""
    try:
        for name, value in values.items():
            debug_set(name, value)
        yield
    finally:
        for name in values:
            debug_set(name, None)


def _ptr(a) -> ctypes.c_void_p:
    if a is None:
        return ctypes.c_void_p(0)
    if isinstance(a, np.ndarray):
        return ctypes.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):  # torch tensor
        return ctypes.c_void_p(a.data_ptr())
    return ctypes.c_void_p(int(a))


def _nbytes(a):
    """Size in bytes of a numpy array / torch tensor, None for a raw pointer (an int: its size is the caller's business)."""
    if isinstance(a, np.ndarray):
        return int(a.nbytes)
    if hasattr(a, "data_ptr") and hasattr(a, "numel"):
        return int(a.numel()) * int(a.element_size())
    return None


def _need(what: str, a, nbytes: int) -> None:
    """A batch call reads / writes `nbytes` of `a`: an array that is shorter is a ValueError HERE -- behind the C ABI it would be a
    GPU memory fault (round 6: bench.py handed 64 frames' worth of arguments over 16-frame tensors)."""
    have = _nbytes(a)
    if have is not None and have < nbytes:
        raise ValueError("%s holds %d bytes, the call needs %d" % (what, have, nbytes))


def _pair_lists(names, lists, n_frames: Optional[int] = None, n_sets: Optional[int] = None, set_what: str = "") -> list:
    """The host index lists of a device-resident call, each as a flat int32 array.  Of one length, else OrbxError.  With n_frames
    the lists (but the last one when n_sets is given) must lie below it, and with n_sets the last list (the sets: `set_what` in
    the message) below that, else ValueError; None leaves the range to the C side, which answers ORBX_E_BADARG (each method
    keeps the check it always made)."""
    rows = [np.ascontiguousarray(a, np.int32).reshape(-1) for a in lists]
    n = len(rows[0])
    for r in rows:
        if len(r) != n:
            raise OrbxError(E_BADARG, "%s and %s must have the same length" % (", ".join(names[:-1]), names[-1]))
    if n and (n_frames is not None or n_sets is not None):
        top = [int(r.view(np.uint32).max()) for r in rows]  # (as unsigned, a negative index is a huge one)
        if n_frames is not None and max(top if n_sets is None else top[:-1]) >= n_frames:
            raise ValueError("a pair names a frame outside the batch of %d" % n_frames)
        if n_sets is not None and top[-1] >= n_sets:
            raise ValueError("a pair names a %s outside the %d given" % (set_what, n_sets))
    return rows


# -- the conversions of the single-problem calls: what the caller holds -> what the C ABI reads ----------------------------
def _k9(K) -> np.ndarray:
    return np.ascontiguousarray(K, np.float32).reshape(9)


def _bounds(bounds) -> _Bounds:
    return _Bounds(*[int(v) for v in bounds])


def _keys(keys) -> np.ndarray:
    return np.ascontiguousarray(keys, KEYPOINT_DTYPE).reshape(-1)


def _desc(desc, n: Optional[int] = None, message: str = "") -> Optional[np.ndarray]:
    """Descriptor rows uint8 [., 32].  With n: an optional array (None passes through) that must hold n rows."""
    if desc is None and n is not None:
        return None
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    if n is not None and len(d) != n:
        raise OrbxError(E_BADARG, message)
    return d


def _points(points, width: int = 3) -> np.ndarray:
    return np.ascontiguousarray(points, np.float32).reshape(-1, width)


def _flags(flags, n: int, message: str) -> Optional[np.ndarray]:
    """A row of n flags as uint8 (!= 0 -> 1); None passes through; another length is OrbxError(E_BADARG, message)."""
    if flags is None:
        return None
    f = np.ascontiguousarray(np.asarray(flags) != 0, np.uint8).reshape(-1)
    if len(f) != n:
        raise OrbxError(E_BADARG, message)
    return f


def _row(row, n: int, message: str) -> np.ndarray:
    """An int32 row of n entries (at least one is allocated), all -1 unless `row` gives them: then it must hold n."""
    out = np.full(max(n, 1), -1, np.int32)
    if row is not None:
        given = np.asarray(row, np.int32).reshape(-1)
        if len(given) != n:
            raise OrbxError(E_BADARG, message)
        out[:n] = given
    return out


def _per_level(table, nlevels: int, name: str) -> Optional[np.ndarray]:
    """A float32 table with one entry per pyramid level (inv_sigma2 / sigma2); None passes through."""
    t = None if table is None else np.ascontiguousarray(table, np.float32)
    if t is not None and len(t) != nlevels:
        raise OrbxError(E_BADARG, "%s must have one entry per pyramid level" % name)
    return t


def _pose12(Tcw) -> np.ndarray:
    """A pose (or Scw) as the C ABI takes it, row-major R [9] then t [3]: 12 floats as they are, a 3x4 or 4x4 matrix converted."""
    T = np.asarray(Tcw, np.float32)
    if T.ndim == 1:
        return np.ascontiguousarray(T.reshape(12))
    return np.ascontiguousarray(np.r_[T[:3, :3].reshape(9), T[:3, 3]], np.float32)


def _camera_K(K, holder, who: str, what: str = "frame") -> np.ndarray:
    """K as given, or the 3x3 of the camera `holder` (a Frame) carries; neither: OrbxError naming the caller."""
    if K is not None:
        return K
    cam = getattr(holder, "camera", None)
    if cam is None:
        raise OrbxError(E_BADARG, "%s needs K (the %s carries no camera)" % (who, what))
    return np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], np.float32)


def _need_batch(imgs, n_frames, width, height, stride, frame_stride, kps, desc, n, capacity, first=None, second=None, matches12=None,
                nmatches=None, stats=None, init_res=None, p3d=None, triangulated=None, ba_res=None, p3d_out=None) -> None:
    if n_frames > 0 and imgs is not None:
        _need("the frames", imgs, (n_frames - 1) * frame_stride + (height - 1) * stride + width)
    _need("the keypoint array", kps, n_frames * capacity * 28)
    _need("the descriptor array", desc, n_frames * capacity * 32)
    _need("the count array", n, n_frames * 4)
    if first is not None and len(first):
        if len(second) != len(first):
            raise ValueError("first / second: %d and %d pairs" % (len(first), len(second)))
        # (one pass over both: as unsigned, a negative index is a huge one)
        if n_frames > 0 and int(np.maximum(first.view(np.uint32), second.view(np.uint32)).max()) >= n_frames:
            raise ValueError("a pair names a frame outside the batch of %d" % n_frames)
        _need("matches12", matches12, len(first) * capacity * 4)
        _need("nmatches", nmatches, len(first) * 4)
        if stats is not None:
            _need("stats", stats, len(first) * 12)
        # the arrays of the bundle adjustment (each per pair)
        _need("the Initializer's results", init_res, len(first) * INIT_RESULT_DTYPE.itemsize)
        _need("the point array", p3d, len(first) * capacity * 12)
        _need("the triangulated array", triangulated, len(first) * capacity)
        _need("the result array", ba_res, len(first) * BA_RESULT_DTYPE.itemsize)
        _need("the refined point array", p3d_out, len(first) * capacity * 12)


def _torch_stream(*arrays):
    """The current torch stream (as an int handle) if any of the arguments is a torch CUDA tensor, else None: work
    issued on the context's own HIP streams must start after what torch has queued for those tensors."""
    for a in arrays:
        if a is not None and hasattr(a, "data_ptr") and getattr(a, "is_cuda", False):
            import torch
            st = torch.cuda.current_stream(a.device)
            if st.query():  # nothing queued on it: nothing to order behind (saves the event record + two stream waits)
                return None
            return int(st.cuda_stream)
    return None


class ORBextractor:
    """Features/ORBextractor.hpp:55-158.  One instance == one orbx_ctx bound to one device; calls are serialised by
    the caller (the reference's operator() is not re-entrant either, cpp:1669)."""

    HARRIS_SCORE, FAST_SCORE = 0, 1

    def __init__(self, nfeatures: int, scaleFactor: float, nlevels: int, iniThFAST: int, minThFAST: int, *,
                 max_width: int = 1920, max_height: int = 1080, max_batch: int = 1, device: int = 0,
                 stream: Optional[int] = None):
        self._L = lib()
        self._h = ctypes.c_void_p(0)
        p = _Params(int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST), int(minThFAST))
        r = self._L.orbx_create(ctypes.byref(p), int(device), int(max_width), int(max_height), int(max_batch),
                                ctypes.c_void_p(stream or 0), ctypes.byref(self._h))
        if r != 0:
            self._h = ctypes.c_void_p(0)
            what = "orbx_create"
            if r == E_HIP:
                what = "orbx_create failed (no usable HIP device / kernel image?)"
                rts = hip_runtimes_mapped()
                if len(rts) > 1:  # the diagnosis that used to take a debugger (gpurun_out/r05/create2.log)
                    what += ("; TWO HIP runtimes are mapped into this process (%s): liborbx.so and PyTorch each brought their own "
                             "libamdhip64 -- import torch before orb_slam_tracking_amd, or build liborbx.so against the ROCm that "
                             "torch ships" % ", ".join(rts))
            raise OrbxError(r, what)
        self.nfeatures, self.nlevels, self.device, self.max_batch = int(nfeatures), int(nlevels), int(device), int(max_batch)
        q = np.zeros(self.nlevels, np.int32)
        self._L.orbx_get_tables(self._h, None, None, None, None, _ptr(q))
        self.capacity = max(int(q.sum()), 1)
        self.order_with_torch = True  # device-resident calls given torch tensors are ordered behind torch's current stream

    # -- lifetime ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.orbx_destroy(self._h)
            self._h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    GAUSS_ERROR_DIFFUSION, GAUSS_ROUNDED, GRAY_14BIT, GRAY_15BIT = 0, 1, 0, 1

    def set_opencv_variant(self, gaussian_variant: int = 0, gray_variant: int = 0) -> None:
        """The two OpenCV-release dependent constants of the path (include/orbx.h): Gaussian Q8 taps, BGR2GRAY coefficients."""
        self._check(self._L.orbx_set_opencv_variant(self._h, int(gaussian_variant), int(gray_variant)), "orbx_set_opencv_variant")

    LIBM_DOUBLE, LIBM_FLOAT, LIBM_DEFAULT = 0, 1, 1

    def set_libm_variant(self, libm_variant: int = 1) -> None:
        """The libm reading of the reference's unqualified cos / sin / pow on floats (include/orbx.h): 0 = through double,
        1 = cosf / sinf / powf (glibc >= 2.28's algorithm; the default)."""
        self._check(self._L.orbx_set_libm_variant(self._h, int(libm_variant)), "orbx_set_libm_variant")

    def order_after(self, stream: Optional[int]) -> None:
        """Work issued on this context from now on starts after everything queued on `stream` (hipStream_t handle)."""
        self._check(self._L.orbx_order_after(self._h, ctypes.c_void_p(stream or 0)), "orbx_order_after")

    def order_before(self, stream: Optional[int]) -> None:
        """Work queued on `stream` from now on starts after everything issued on this context so far."""
        self._check(self._L.orbx_order_before(self._h, ctypes.c_void_p(stream or 0)), "orbx_order_before")

    def _order_torch(self, *arrays) -> None:
        # torch tensors in: the producer of the frames (and the last reader of the output arrays) runs on torch's current
        # stream, which the context's private streams know nothing about
        if self.order_with_torch:
            s = _torch_stream(*arrays)
            if s is not None:
                self.order_after(s)

    def _check(self, r: int, what: str = "") -> int:
        if r < 0:
            raise OrbxError(r, (self._L.orbx_last_error(self._h) or b"").decode() or what)
        return r

    def _device_call(self, fn: str, *args) -> int:
        """One device-resident C call, fn(ctx, *args), with every argument named once in the C order.  A device array (device
        pointer or torch tensor; None where the C side takes null) goes in as (what, array, bytes the call reads or writes): each
        one given is checked against its size (_need), the context is ordered behind torch for exactly these arrays, and the call
        gets their pointers.  Host arrays (numpy, or None) become pointers too; everything else is passed as it is."""
        given = [a for a in args if type(a) is tuple and a[1] is not None]
        for a in given:
            _need(*a)
        self._order_torch(*[a[1] for a in given])
        r = getattr(self._L, fn)(self._h, *[_ptr(a[1]) if type(a) is tuple else _ptr(a) if a is None or type(a) is np.ndarray else a
                                            for a in args])
        return self._check(r, fn)

    # -- getters (hpp:87-108) --------------------------------------------------------------------
    def GetLevels(self) -> int:
        return self._L.orbx_get_levels(self._h)

    def GetScaleFactor(self) -> float:
        return float(self._L.orbx_get_scale_factor(self._h))

    def _table(self, idx: int, dtype=np.float32) -> np.ndarray:
        out = np.zeros(self.nlevels, dtype)
        args = [None] * 5
        args[idx] = _ptr(out)
        self._L.orbx_get_tables(self._h, *args)
        return out

    def GetScaleFactors(self):
        return self._table(0)

    def GetInverseScaleFactors(self):
        return self._table(1)

    def GetScaleSigmaSquares(self):
        return self._table(2)

    def GetInverseScaleSigmaSquares(self):
        return self._table(3)

    def GetNumFeaturesPerLevel(self):
        return self._table(4, np.int32)

    def umax(self) -> np.ndarray:
        out = np.zeros(16, np.int32)
        self._L.orbx_get_umax(self._h, _ptr(out))
        return out

    # -- operator() (cpp:1531-1653) ----------------------------------------------------------------
    def __call__(self, image: np.ndarray, mask=None, vLappingArea: Sequence[int] = (0, 0)) -> Tuple[int, np.ndarray, np.ndarray]:
        """Returns (monoIndex, keypoints[KEYPOINT_DTYPE], descriptors[N,32] uint8); -1 for an empty image (cpp:1536)."""
        if image is None or image.size == 0:
            return -1, np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
        if image.dtype != np.uint8 or image.ndim != 2:
            raise OrbxError(E_BADARG, "image must be a 2-D uint8 array (CV_8UC1, cpp:1541)")
        if image.strides[1] != 1:
            image = np.ascontiguousarray(image)
        h, w = image.shape
        kps = np.empty(self.capacity, KEYPOINT_DTYPE)   # (the first n entries are written, only those are returned)
        desc = np.empty((self.capacity, 32), np.uint8)
        n = ctypes.c_int(0)
        r = self._L.orbx_extract(self._h, _ptr(image), w, h, image.strides[0], int(vLappingArea[0]), int(vLappingArea[1]),
                                 _ptr(kps), _ptr(desc), self.capacity, ctypes.byref(n))
        self._check(r, "orbx_extract")
        return r, kps[:n.value], desc[:n.value]  # (views of this call's own arrays)

    def extract_batch(self, images: np.ndarray, vLappingArea: Sequence[int] = (0, 0)):
        """images: [B, H, W] uint8 (host).  Returns a list of (monoIndex, keypoints, descriptors) per frame."""
        images = np.ascontiguousarray(images)
        if images.dtype != np.uint8 or images.ndim != 3:
            raise OrbxError(E_BADARG, "images must be [B,H,W] uint8")
        B, h, w = images.shape
        kps = np.zeros((B, self.capacity), KEYPOINT_DTYPE)
        desc = np.zeros((B, self.capacity, 32), np.uint8)
        n = np.zeros(B, np.int32)
        mono = np.zeros(B, np.int32)
        r = self._L.orbx_extract_batch(self._h, B, _ptr(images), w, h, w, w * h, int(vLappingArea[0]), int(vLappingArea[1]),
                                       _ptr(kps), _ptr(desc), self.capacity, _ptr(n), _ptr(mono))
        self._check(r, "orbx_extract_batch")
        return [(int(mono[f]), kps[f, :n[f]].copy(), desc[f, :n[f]].copy()) for f in range(B)]

    def extract_batch_device(self, d_imgs, n_frames: int, width: int, height: int, stride: int, frame_stride: int,
                             d_kps, d_desc, d_n, capacity: Optional[int] = None) -> None:
        """Frames resident in HBM in, keypoints/descriptors/counts resident in HBM out (device pointers or torch tensors)."""
        _need_batch(d_imgs, int(n_frames), int(width), int(height), int(stride), int(frame_stride), d_kps, d_desc, d_n,
                    int(capacity or self.capacity))
        self._order_torch(d_imgs, d_kps, d_desc, d_n)
        r = self._L.orbx_extract_batch_device(self._h, int(n_frames), _ptr(d_imgs), int(width), int(height), int(stride),
                                              int(frame_stride), _ptr(d_kps), _ptr(d_desc), int(capacity or self.capacity),
                                              _ptr(d_n))
        self._check(r, "orbx_extract_batch_device")

    def match_pairs_device(self, first: np.ndarray, second: np.ndarray, d_kps, d_desc, d_n, bounds: Tuple[int, int, int, int],
                           d_matches12, d_nmatches, d_stats=None, windowSize: int = 100, nnratio: float = 0.9,
                           checkOri: bool = True, capacity: Optional[int] = None) -> None:
        first = np.ascontiguousarray(first, np.int32)
        second = np.ascontiguousarray(second, np.int32)
        b = _bounds(bounds)
        if len(first):
            nfr = int(max(first.max(), second.max())) + 1
            _need_batch(None, nfr, 0, 0, 0, 0, d_kps, d_desc, d_n, int(capacity or self.capacity), first, second, d_matches12, d_nmatches, d_stats)
        self._order_torch(d_kps, d_desc, d_n, d_matches12, d_nmatches, d_stats)
        r = self._L.orbx_match_init_batch_device(self._h, len(first), _ptr(first), _ptr(second), _ptr(d_kps), _ptr(d_desc),
                                                 _ptr(d_n), int(capacity or self.capacity), ctypes.byref(b), int(windowSize),
                                                 float(nnratio), int(bool(checkOri)), _ptr(d_matches12), _ptr(d_nmatches),
                                                 _ptr(d_stats))
        self._check(r, "orbx_match_init_batch_device")

    def match_bow_pairs_device(self, n_frames: int, kf: np.ndarray, f: np.ndarray, d_kps, d_desc, d_n, d_fv_node, d_fv_feat, d_fv_n,
                               d_matches_f, d_nmatches, d_kf_mask=None, nnratio: float = 0.6, checkOri: bool = True,
                               capacity: Optional[int] = None) -> None:
        """ORBmatcher::SearchByBoW for pairs (keyframe kf[p], frame f[p]; host index arrays) of the arrays extract_batch_device
        and Vocabulary.transform_batch_device filled (same capacity): d_matches_f int32 [n_pairs, capacity] (row p: the keyframe
        feature matched to each of frame f[p]'s features, or -1), d_nmatches int32 [n_pairs]; d_kf_mask (optional) uint8
        [n_frames, capacity], 0 = the keyframe's feature has no map point.  Stream-ordered on the context's stream."""
        kf, f = _pair_lists(("kf", "f"), (kf, f))
        cap, nf, P = int(capacity or self.capacity), int(n_frames), len(kf)
        self._device_call("orbx_match_bow_batch_device", nf, P, kf, f, ("the keypoint array", d_kps, nf * cap * 28),
                          ("the descriptor array", d_desc, nf * cap * 32), ("the count array", d_n, nf * 4), cap,
                          ("the FeatureVector node array", d_fv_node, nf * cap * 4),
                          ("the FeatureVector feature array", d_fv_feat, nf * cap * 4), ("the FeatureVector count array", d_fv_n, nf * 4),
                          ("the keyframe mask", d_kf_mask, nf * cap), float(nnratio), int(bool(checkOri)),
                          ("matches_f", d_matches_f, P * cap * 4), ("nmatches", d_nmatches, P * 4))

    def match_bow(self, kf_keys, kf_desc, kf_fv_node, kf_fv_feat, f_keys, f_desc, f_fv_node, f_fv_feat, kf_mask=None,
                  nnratio: float = 0.6, checkOri: bool = True):
        """SearchByBoW for one pair in host memory (orbx_match_bow) -> (matches_f int32 [len(f_keys)], nmatches).  Synchronous."""
        kk, fk = _keys(kf_keys), _keys(f_keys)
        kd, fd = _desc(kf_desc), _desc(f_desc)
        kn, kft = np.ascontiguousarray(kf_fv_node, np.uint32).reshape(-1), np.ascontiguousarray(kf_fv_feat, np.uint32).reshape(-1)
        fn, fft = np.ascontiguousarray(f_fv_node, np.uint32).reshape(-1), np.ascontiguousarray(f_fv_feat, np.uint32).reshape(-1)
        if len(kk) != len(kd) or len(fk) != len(fd) or len(kn) != len(kft) or len(fn) != len(fft):
            raise OrbxError(E_BADARG, "keypoints / descriptors or FeatureVector nodes / features differ in length")
        mask = _flags(kf_mask, len(kk), "the mask needs one entry per keyframe feature")
        m = np.full(max(len(fk), 1), -1, np.int32)
        nm = ctypes.c_int32(0)
        r = self._L.orbx_match_bow(self._h, _ptr(kk), _ptr(kd), len(kk), _ptr(kn), _ptr(kft), len(kn), _ptr(fk), _ptr(fd), len(fk),
                                   _ptr(fn), _ptr(fft), len(fn), _ptr(mask), float(nnratio), int(bool(checkOri)), _ptr(m),
                                   ctypes.byref(nm))
        self._check(r, "orbx_match_bow")
        return m[:len(fk)].copy(), int(nm.value)

    def match_projection_pairs_device(self, n_frames: int, last: np.ndarray, cur: np.ndarray, point_set: np.ndarray, d_kps_un, d_desc,
                                      d_n, n_point_sets: int, d_points, d_point_mask, d_pose_cur, K, bounds: Tuple[int, int, int, int],
                                      d_matches_cur, d_res, th: float = 15.0, checkOri: bool = True, d_point_desc=None,
                                      d_last_outlier=None, capacity: Optional[int] = None) -> None:
        """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono=True) for pairs (last frame last[p], current frame
        cur[p], the last frame's map points = point set point_set[p]; host index arrays) of the arrays extract_batch_device and
        undistort_batch_device filled, with the point sets of pose_optimize_batch_device (d_points float32 [n_point_sets,
        capacity, 3], d_point_mask uint8 [n_point_sets, capacity] or None) and the predicted poses d_pose_cur float32 [n_pairs,
        12].  Optional: d_point_desc uint8 [n_point_sets, capacity, 32] (the map points' own descriptors; default the last
        frame's), d_last_outlier uint8 [n_pairs, capacity].  d_matches_cur int32 [n_pairs, capacity] (row p: the last frame's
        feature matched to each of frame cur[p]'s features, or -1: pose_optimize_batch_device's d_match), d_res [n_pairs]
        PROJ_RESULT_DTYPE records (32 bytes).  Stream-ordered on the context's stream."""
        cap, nf, ns = int(capacity or self.capacity), int(n_frames), int(n_point_sets)
        last, cur, point_set = _pair_lists(("last", "cur", "point_set"), (last, cur, point_set), nf, ns, "point set")
        P = len(last)
        self._device_call("orbx_match_projection_batch_device", nf, P, last, cur, point_set, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the descriptor array", d_desc, nf * cap * 32), ("the count array", d_n, nf * 4), cap, ns,
                          ("the point array", d_points, ns * cap * 12), ("the point mask", d_point_mask, ns * cap),
                          ("the point descriptor array", d_point_desc, ns * cap * 32), ("the outlier array", d_last_outlier, P * cap),
                          ("the pose array", d_pose_cur, P * 48), _k9(K), ctypes.byref(_bounds(bounds)), float(th), int(bool(checkOri)),
                          ("matches_cur", d_matches_cur, P * cap * 4), ("the result array", d_res, P * PROJ_RESULT_DTYPE.itemsize))

    def match_projection(self, last_keys_un, last_desc, cur_keys_un, cur_desc, points, mask, Tcw, K, bounds: Tuple[int, int, int, int],
                         th: float = 15.0, checkOri: bool = True, point_desc=None, last_outlier=None):
        """SearchByProjection for one pair in host memory (orbx_match_projection) -> (matches_cur int32 [len(cur_keys_un)],
        ProjResult).  points [n_last, 3] and mask [n_last] (or None) are the last frame's map points, Tcw (3x4 or 4x4) the
        current frame's predicted pose.  Synchronous."""
        lk, ck = _keys(last_keys_un), _keys(cur_keys_un)
        ld, cd = _desc(last_desc), _desc(cur_desc)
        pts = _points(points)
        if len(lk) != len(ld) or len(ck) != len(cd) or len(pts) != len(lk):
            raise OrbxError(E_BADARG, "keypoints / descriptors / points differ in length")
        m = _flags(mask, len(lk), "the mask needs one entry per feature of the last frame")
        out = _flags(last_outlier, len(lk), "last_outlier needs one entry per feature of the last frame")
        pd = _desc(point_desc, len(lk), "point_desc needs one entry per feature of the last frame")
        pose = _pose12(Tcw)
        Kf = _k9(K)
        b = _bounds(bounds)
        mc = np.full(max(len(ck), 1), -1, np.int32)
        res = ProjResult()
        r = self._L.orbx_match_projection(self._h, _ptr(lk), _ptr(ld), len(lk), _ptr(ck), _ptr(cd), len(ck), _ptr(pts), _ptr(m), _ptr(pd),
                                          _ptr(out), _ptr(pose), _ptr(Kf), ctypes.byref(b), float(th), int(bool(checkOri)), _ptr(mc),
                                          ctypes.byref(res))
        self._check(r, "orbx_match_projection")
        return mc[:len(ck)].copy(), res

    def match_local_map_pairs_device(self, n_frames: int, frame: np.ndarray, map_set: np.ndarray, d_kps_un, d_desc, d_n,
                                     n_map_sets: int, map_capacity: int, d_map_n, d_map_points, d_map_normals, d_map_dist, d_map_desc,
                                     d_map_mask, d_pose, K, bounds: Tuple[int, int, int, int], d_matches, d_res, th: float = 1.0,
                                     nnratio: float = 0.8, d_outlier=None, d_point_view=None, capacity: Optional[int] = None) -> None:
        """Tracking::SearchLocalPoints -- isInFrustum, PredictScale and ORBmatcher::SearchByProjection(Frame, local map points,
        th) -- for pairs (frame frame[p], map set map_set[p]; host index arrays) of the arrays extract_batch_device and
        undistort_batch_device filled and of map sets [n_map_sets, map_capacity]: d_map_n int32 counts, d_map_points and
        d_map_normals float32 [.., 3], d_map_dist float32 [.., 2] (mfMinDistance, mfMaxDistance), d_map_desc uint8 [.., 32],
        d_map_mask uint8 or None; d_pose float32 [n_pairs, 12].  d_matches int32 [n_pairs, capacity] is read and written: feature
        j's index into the pair's map set, or -1 (with map_capacity == capacity: pose_optimize_batch_device's d_match).
        Optional: d_outlier uint8 [n_pairs, capacity] (read only), d_point_view uint8 [n_pairs, map_capacity] (LOCAL_NOT_IN_VIEW,
        LOCAL_SEEN or the predicted level).  d_res [n_pairs] LOCAL_RESULT_DTYPE records (60 bytes).  Stream-ordered on the
        context's stream."""
        cap, mcap, nf, ns = int(capacity or self.capacity), int(map_capacity), int(n_frames), int(n_map_sets)
        frame, map_set = _pair_lists(("frame", "map_set"), (frame, map_set), nf, ns, "map set")
        P = len(frame)
        self._device_call("orbx_match_local_map_batch_device", nf, P, frame, map_set, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the descriptor array", d_desc, nf * cap * 32), ("the count array", d_n, nf * 4), cap, ns, mcap,
                          ("the map count array", d_map_n, ns * 4), ("the map point array", d_map_points, ns * mcap * 12),
                          ("the map normal array", d_map_normals, ns * mcap * 12), ("the map distance array", d_map_dist, ns * mcap * 8),
                          ("the map descriptor array", d_map_desc, ns * mcap * 32), ("the map mask", d_map_mask, ns * mcap),
                          ("the pose array", d_pose, P * 48), _k9(K), ctypes.byref(_bounds(bounds)), float(th), float(nnratio),
                          ("matches", d_matches, P * cap * 4), ("the outlier array", d_outlier, P * cap),
                          ("point_view", d_point_view, P * mcap), ("the result array", d_res, P * LOCAL_RESULT_DTYPE.itemsize))

    def match_local_map(self, keys_un, desc, map_points, map_normals, map_dist, map_desc, map_mask, Tcw, K,
                        bounds: Tuple[int, int, int, int], matches=None, th: float = 1.0, nnratio: float = 0.8, outlier=None):
        """SearchLocalPoints for one frame and one local map in host memory (orbx_match_local_map) -> (matches int32
        [len(keys_un)], point_view uint8 [n_map], LocalResult).  matches (default all -1) holds the map points the frame already
        has, as indices into the map arrays; Tcw is 3x4 or 4x4.  Synchronous."""
        k = _keys(keys_un)
        d = _desc(desc)
        mp = _points(map_points)
        mn = _points(map_normals)
        md = _points(map_dist, 2)
        mdesc = _desc(map_desc)
        if len(k) != len(d) or not (len(mp) == len(mn) == len(md) == len(mdesc)):
            raise OrbxError(E_BADARG, "keypoints / descriptors or the map arrays differ in length")
        mm = _flags(map_mask, len(mp), "the map mask needs one entry per map point")
        out = _flags(outlier, len(k), "outlier needs one entry per feature")
        m = _row(matches, len(k), "matches needs one entry per feature")
        pose = _pose12(Tcw)
        Kf = _k9(K)
        b = _bounds(bounds)
        view = np.zeros(max(len(mp), 1), np.uint8)
        res = LocalResult()
        r = self._L.orbx_match_local_map(self._h, _ptr(k), _ptr(d), len(k), len(mp), _ptr(mp), _ptr(mn), _ptr(md), _ptr(mdesc), _ptr(mm),
                                         _ptr(pose), _ptr(Kf), ctypes.byref(b), float(th), float(nnratio), _ptr(m), _ptr(out), _ptr(view),
                                         ctypes.byref(res))
        self._check(r, "orbx_match_local_map")
        return m[:len(k)].copy(), view[:len(mp)].copy(), res

    def match_keyframe_projection_pairs_device(self, n_frames: int, kf: np.ndarray, cur: np.ndarray, point_set: np.ndarray, d_kps_un,
                                               d_desc, d_n, n_point_sets: int, d_points, d_point_mask, d_point_dist, d_pose, K,
                                               bounds: Tuple[int, int, int, int], d_matches, d_res, th: float = 10.0, ORBdist: int = 100,
                                               checkOri: bool = True, d_point_desc=None, d_outlier=None,
                                               capacity: Optional[int] = None) -> None:
        """The relocalisation overload ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) for pairs
        (keyframe kf[p], current frame cur[p], the keyframe's map points = point set point_set[p]; host index arrays) of the
        arrays extract_batch_device and undistort_batch_device filled, with the point sets of pose_optimize_batch_device
        (d_points float32 [n_point_sets, capacity, 3], d_point_mask uint8 [n_point_sets, capacity] or None), d_point_dist float32
        [n_point_sets, capacity, 2] (mfMinDistance, mfMaxDistance) and the poses d_pose float32 [n_pairs, 12].  d_matches int32
        [n_pairs, capacity] is read and written: the current frame's feature j -> an index into the point set, or -1
        (match_bow_pairs_device's d_matches_f, pose_optimize_batch_device's d_match).  Optional: d_point_desc uint8 [n_point_sets,
        capacity, 32] (default the keyframe's descriptors), d_outlier uint8 [n_pairs, capacity] (read only).  d_res [n_pairs]
        KFPROJ_RESULT_DTYPE records (52 bytes).  Stream-ordered on the context's stream."""
        cap, nf, ns = int(capacity or self.capacity), int(n_frames), int(n_point_sets)
        kf, cur, point_set = _pair_lists(("kf", "cur", "point_set"), (kf, cur, point_set), nf, ns, "point set")
        P = len(kf)
        self._device_call("orbx_match_keyframe_projection_batch_device", nf, P, kf, cur, point_set,
                          ("the keypoint array", d_kps_un, nf * cap * 28), ("the descriptor array", d_desc, nf * cap * 32),
                          ("the count array", d_n, nf * 4), cap, ns, ("the point array", d_points, ns * cap * 12),
                          ("the point mask", d_point_mask, ns * cap), ("the point descriptor array", d_point_desc, ns * cap * 32),
                          ("the point distance array", d_point_dist, ns * cap * 8), ("the pose array", d_pose, P * 48), _k9(K),
                          ctypes.byref(_bounds(bounds)), float(th), int(ORBdist), int(bool(checkOri)), ("matches", d_matches, P * cap * 4),
                          ("the outlier array", d_outlier, P * cap), ("the result array", d_res, P * KFPROJ_RESULT_DTYPE.itemsize))

    def match_keyframe_projection(self, kf_keys_un, kf_desc, cur_keys_un, cur_desc, points, mask, point_dist, Tcw, K,
                                  bounds: Tuple[int, int, int, int], matches=None, th: float = 10.0, ORBdist: int = 100,
                                  checkOri: bool = True, point_desc=None, outlier=None):
        """The relocalisation SearchByProjection for one pair in host memory (orbx_match_keyframe_projection) -> (matches int32
        [len(cur_keys_un)], KfProjResult).  points [n_kf, 3], mask [n_kf] (or None) and point_dist [n_kf, 2] are the keyframe's
        map points; matches (default all -1) holds the points the current frame already has, as indices into them; Tcw (3x4 or
        4x4) is the current frame's pose.  Synchronous."""
        kk, ck = _keys(kf_keys_un), _keys(cur_keys_un)
        kd, cd = _desc(kf_desc), _desc(cur_desc)
        pts = _points(points)
        dst = _points(point_dist, 2)
        if len(kk) != len(kd) or len(ck) != len(cd) or len(pts) != len(kk) or len(dst) != len(kk):
            raise OrbxError(E_BADARG, "keypoints / descriptors / points / distances differ in length")
        m = _flags(mask, len(kk), "the mask needs one entry per feature of the keyframe")
        pd = _desc(point_desc, len(kk), "point_desc needs one entry per feature of the keyframe")
        out = _flags(outlier, len(ck), "outlier needs one entry per feature of the current frame")
        mc = _row(matches, len(ck), "matches needs one entry per feature of the current frame")
        pose = _pose12(Tcw)
        Kf = _k9(K)
        b = _bounds(bounds)
        res = KfProjResult()
        r = self._L.orbx_match_keyframe_projection(self._h, _ptr(kk), _ptr(kd), len(kk), _ptr(ck), _ptr(cd), len(ck), _ptr(pts), _ptr(m),
                                                   _ptr(pd), _ptr(dst), _ptr(pose), _ptr(Kf), ctypes.byref(b), float(th), int(ORBdist),
                                                   int(bool(checkOri)), _ptr(mc), _ptr(out), ctypes.byref(res))
        self._check(r, "orbx_match_keyframe_projection")
        return mc[:len(ck)].copy(), res

    # -- ORBmatcher::SearchBySim3 (include/orbx.h, "loop closing: matching under a similarity") ---------------------
    def match_sim3_pairs_device(self, n_frames: int, kf1: np.ndarray, kf2: np.ndarray, set1: np.ndarray, set2: np.ndarray, d_kps_un,
                                d_desc, d_n, n_point_sets: int, d_points, d_point_mask, d_point_dist, d_pose, d_sim3, K,
                                bounds: Tuple[int, int, int, int], d_matches, d_res, th: float = 7.5, ORBdist: int = 100,
                                d_point_desc=None, capacity: Optional[int] = None) -> None:
        """ORBmatcher::SearchBySim3 for pairs (KF1 kf1[p] with point set set1[p], KF2 kf2[p] with set2[p]; host index arrays):
        the point sets of sim3_solve_batch_device plus d_point_dist float32 [n_point_sets, capacity, 2] (mfMinDistance,
        mfMaxDistance) and optionally d_point_desc uint8 [n_point_sets, capacity, 32]; d_pose float32 [n_frames, 12] and d_sim3
        float32 [n_pairs, 13] as the solver takes and writes them.  d_matches int32 [n_pairs, capacity] is read and written (the
        solver's d_match_inliers): KF1's feature -> KF2's feature, or -1.  d_res [n_pairs] MSIM3_RESULT_DTYPE records (64 bytes).
        Stream-ordered on the context's stream."""
        cap, nf, ns = int(capacity or self.capacity), int(n_frames), int(n_point_sets)
        kf1, kf2 = _pair_lists(("kf1", "kf2"), (kf1, kf2), nf)  # (two lists at a time, as this method always checked them)
        set1, set2 = _pair_lists(("set1", "set2"), (set1, set2), ns)
        P = len(kf1)
        if len(set1) != P:
            raise OrbxError(E_BADARG, "kf1, kf2, set1 and set2 must have the same length")
        self._device_call("orbx_match_sim3_batch_device", nf, P, kf1, kf2, set1, set2, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the descriptor array", d_desc, nf * cap * 32), ("the count array", d_n, nf * 4), cap, ns,
                          ("the point array", d_points, ns * cap * 12), ("the point mask", d_point_mask, ns * cap),
                          ("the point descriptor array", d_point_desc, ns * cap * 32),
                          ("the point distance array", d_point_dist, ns * cap * 8), ("the pose array", d_pose, nf * 48),
                          ("the similarity array", d_sim3, P * 52), _k9(K), ctypes.byref(_bounds(bounds)), float(th), int(ORBdist),
                          ("matches", d_matches, P * cap * 4), ("the result array", d_res, P * MSIM3_RESULT_DTYPE.itemsize))

    def compute_sim3_pairs_device(self, n_frames: int, kf1, kf2, set1, set2, d_kps_un, d_desc, d_n, d_match, n_point_sets: int, d_points,
                                  d_point_mask, d_point_dist, d_pose, K, bounds: Tuple[int, int, int, int], d_draws, d_sim3_res, d_sim3,
                                  d_matches, d_msim3_res, d_point_desc=None, fix_scale: bool = False, th: float = 7.5, ORBdist: int = 100,
                                  capacity: Optional[int] = None, **ransac) -> None:
        """The geometry of LoopClosing::ComputeSim3 for pairs: sim3_solve_batch_device, then match_sim3_pairs_device on the
        similarity and the row of inlier matches it wrote (d_matches), queued one behind the other on the context's stream with
        no copy and no wait between them.  A pair without a similarity has zeros in d_sim3: the matcher flags it
        (MSIM3_NONFINITE: s12 <= 0) and leaves its all -1 row."""
        self.sim3_solve_batch_device(n_frames, kf1, kf2, set1, set2, d_kps_un, d_n, d_match, n_point_sets, d_points, d_point_mask, d_pose,
                                     K, d_draws, d_sim3_res, d_sim3, d_matches, None, fix_scale=fix_scale, capacity=capacity, **ransac)
        self.match_sim3_pairs_device(n_frames, kf1, kf2, set1, set2, d_kps_un, d_desc, d_n, n_point_sets, d_points, d_point_mask,
                                     d_point_dist, d_pose, d_sim3, K, bounds, d_matches, d_msim3_res, th, ORBdist, d_point_desc, capacity)

    def match_sim3(self, keys_un1, desc1, points1, mask1, point_dist1, Tcw1, keys_un2, desc2, points2, mask2, point_dist2, Tcw2, sim3,
                   K, bounds: Tuple[int, int, int, int], matches12=None, th: float = 7.5, ORBdist: int = 100, point_desc1=None,
                   point_desc2=None):
        """SearchBySim3 for one pair in host memory (orbx_match_sim3) -> (matches12 int32 [n1], MatchSim3Result).  sim3 [13]: R12
        row-major, t12, s12; matches12 (default all -1): the matches the pair already has.  Synchronous."""
        k1, k2 = _keys(keys_un1), _keys(keys_un2)
        d1, d2 = _desc(desc1), _desc(desc2)
        p1, p2 = _points(points1), _points(points2)
        q1, q2 = _points(point_dist1, 2), _points(point_dist2, 2)
        if not (len(k1) == len(d1) == len(p1) == len(q1)) or not (len(k2) == len(d2) == len(p2) == len(q2)):
            raise OrbxError(E_BADARG, "keypoints / descriptors / points / distances differ in length")
        if (mask1 is None) != (mask2 is None) or (point_desc1 is None) != (point_desc2 is None):
            raise OrbxError(E_BADARG, "the masks, and the point descriptors, are given together or not at all")
        opt = lambda a, n, w: None if a is None else np.ascontiguousarray(a, np.uint8).reshape(n, *w)  # noqa: E731
        m1, m2 = (_flags(m, len(k), "a mask needs one entry per feature of its keyframe") for m, k in ((mask1, k1), (mask2, k2)))
        pd1, pd2 = opt(point_desc1, len(k1), (32,)), opt(point_desc2, len(k2), (32,))
        row = _row(matches12, len(k1), "matches12 needs one entry per feature of KF1")
        T1, T2 = _pose12(Tcw1), _pose12(Tcw2)
        sim = np.ascontiguousarray(sim3, np.float32).reshape(13)
        Kf = _k9(K)
        b = _bounds(bounds)
        res = MatchSim3Result()
        r = self._L.orbx_match_sim3(self._h, _ptr(k1), _ptr(d1), len(k1), _ptr(p1), _ptr(m1), _ptr(pd1), _ptr(q1), _ptr(T1), _ptr(k2),
                                    _ptr(d2), len(k2), _ptr(p2), _ptr(m2), _ptr(pd2), _ptr(q2), _ptr(T2), _ptr(sim), _ptr(Kf),
                                    ctypes.byref(b), float(th), int(ORBdist), _ptr(row), ctypes.byref(res))
        self._check(r, "orbx_match_sim3")
        return row[:len(k1)].copy(), res

    def match_triangulation_pairs_device(self, n_frames: int, kf1: np.ndarray, kf2: np.ndarray, d_kps_un, d_desc, d_n, d_fv_node,
                                         d_fv_feat, d_fv_n, d_pose, K, d_matches12, d_res, d_mask=None, d_median_depth=None,
                                         checkOri: bool = True, capacity: Optional[int] = None) -> None:
        """ORBmatcher::SearchForTriangulation for pairs (new keyframe kf1[p], neighbour kf2[p]; host index arrays) of the arrays
        extract_batch_device, undistort_batch_device and Vocabulary.transform_batch_device filled (same capacity), with the
        keyframes' poses d_pose float32 [n_frames, 12] (Tcw: R row-major, then t) and K 3x3: d_matches12 int32 [n_pairs, capacity]
        (row p: the kf2 feature matched to each of kf1's features, or -1), d_res [n_pairs] TRI_MATCH_RESULT_DTYPE records (76
        bytes).  Optional: d_mask uint8 [n_frames, capacity] (!= 0 = the feature already has a map point), d_median_depth float32
        [n_frames] (the baseline gate).  Stream-ordered on the context's stream."""
        cap, nf = int(capacity or self.capacity), int(n_frames)
        kf1, kf2 = _pair_lists(("kf1", "kf2"), (kf1, kf2), nf)
        P = len(kf1)
        self._device_call("orbx_match_triangulation_batch_device", nf, P, kf1, kf2, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the descriptor array", d_desc, nf * cap * 32), ("the count array", d_n, nf * 4), cap,
                          ("the FeatureVector node array", d_fv_node, nf * cap * 4),
                          ("the FeatureVector feature array", d_fv_feat, nf * cap * 4), ("the FeatureVector count array", d_fv_n, nf * 4),
                          ("the mask", d_mask, nf * cap), ("the pose array", d_pose, nf * 48), _k9(K),
                          ("the median depth array", d_median_depth, nf * 4), int(bool(checkOri)), ("matches12", d_matches12, P * cap * 4),
                          ("the result array", d_res, P * TRI_MATCH_RESULT_DTYPE.itemsize))

    def triangulate_matches_pairs_device(self, n_frames: int, kf1: np.ndarray, kf2: np.ndarray, d_kps_un, d_n, d_pose, K, d_matches12,
                                         d_points, d_point_mask, d_point_normal, d_point_dist, d_res,
                                         capacity: Optional[int] = None) -> None:
        """The body of LocalMapping::CreateNewMapPoints behind the matcher, for the same pairs: every match of d_matches12 int32
        [n_pairs, capacity] is triangulated and gated; row p of d_points float32 [n_pairs, capacity, 3], d_point_mask uint8
        [n_pairs, capacity], d_point_normal float32 [n_pairs, capacity, 3] and d_point_dist float32 [n_pairs, capacity, 2]
        (mfMinDistance, mfMaxDistance) is a point set indexed by kf1's feature, as match_keyframe_projection_pairs_device and
        pose_optimize_batch_device read one.  d_res [n_pairs] TRI_RESULT_DTYPE records (44 bytes).  Stream-ordered."""
        cap, nf = int(capacity or self.capacity), int(n_frames)
        kf1, kf2 = _pair_lists(("kf1", "kf2"), (kf1, kf2), nf)
        P = len(kf1)
        self._device_call("orbx_triangulate_matches_batch_device", nf, P, kf1, kf2, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the count array", d_n, nf * 4), cap, ("the pose array", d_pose, nf * 48), _k9(K),
                          ("matches12", d_matches12, P * cap * 4), ("the point array", d_points, P * cap * 12),
                          ("the point mask", d_point_mask, P * cap), ("the point normal array", d_point_normal, P * cap * 12),
                          ("the point distance array", d_point_dist, P * cap * 8), ("the result array", d_res, P * TRI_RESULT_DTYPE.itemsize))

    def create_new_map_points_pairs_device(self, n_frames: int, kf1: np.ndarray, kf2: np.ndarray, d_kps_un, d_desc, d_n, d_fv_node,
                                           d_fv_feat, d_fv_n, d_pose, K, d_matches12, d_match_res, d_points, d_point_mask,
                                           d_point_normal, d_point_dist, d_res, d_mask=None, d_median_depth=None, checkOri: bool = True,
                                           capacity: Optional[int] = None) -> None:
        """LocalMapping::CreateNewMapPoints for pairs (kf1[p], kf2[p]): match_triangulation_pairs_device, then
        triangulate_matches_pairs_device on its rows, queued one behind the other on the context's stream with no copy and no
        wait between them (the pair list goes up once)."""
        self.match_triangulation_pairs_device(n_frames, kf1, kf2, d_kps_un, d_desc, d_n, d_fv_node, d_fv_feat, d_fv_n, d_pose, K,
                                              d_matches12, d_match_res, d_mask, d_median_depth, checkOri, capacity)
        self.triangulate_matches_pairs_device(n_frames, kf1, kf2, d_kps_un, d_n, d_pose, K, d_matches12, d_points, d_point_mask,
                                              d_point_normal, d_point_dist, d_res, capacity)

    def match_triangulation(self, keys_un1, desc1, fv_node1, fv_feat1, Tcw1, keys_un2, desc2, fv_node2, fv_feat2, Tcw2, K, mask1=None,
                            mask2=None, median_depth2: float = 0.0, checkOri: bool = True):
        """SearchForTriangulation for one pair in host memory (orbx_match_triangulation) -> (matches12 int32 [len(keys_un1)],
        TriMatchResult).  Synchronous."""
        k1, k2 = _keys(keys_un1), _keys(keys_un2)
        d1, d2 = _desc(desc1), _desc(desc2)
        n1, t1 = np.ascontiguousarray(fv_node1, np.uint32).reshape(-1), np.ascontiguousarray(fv_feat1, np.uint32).reshape(-1)
        n2, t2 = np.ascontiguousarray(fv_node2, np.uint32).reshape(-1), np.ascontiguousarray(fv_feat2, np.uint32).reshape(-1)
        if len(k1) != len(d1) or len(k2) != len(d2) or len(n1) != len(t1) or len(n2) != len(t2):
            raise OrbxError(E_BADARG, "keypoints / descriptors or FeatureVector nodes / features differ in length")
        masks = [_flags(m, len(k), "a mask needs one entry per feature of its keyframe") for m, k in ((mask1, k1), (mask2, k2))]
        p1, p2 = _pose12(Tcw1), _pose12(Tcw2)
        Kf = _k9(K)
        m12 = np.full(max(len(k1), 1), -1, np.int32)
        res = TriMatchResult()
        r = self._L.orbx_match_triangulation(self._h, _ptr(k1), _ptr(d1), len(k1), _ptr(n1), _ptr(t1), len(n1), _ptr(masks[0]), _ptr(p1),
                                             _ptr(k2), _ptr(d2), len(k2), _ptr(n2), _ptr(t2), len(n2), _ptr(masks[1]), _ptr(p2), _ptr(Kf),
                                             float(median_depth2), int(bool(checkOri)), _ptr(m12), ctypes.byref(res))
        self._check(r, "orbx_match_triangulation")
        return m12[:len(k1)].copy(), res

    def triangulate_matches(self, keys_un1, Tcw1, keys_un2, Tcw2, K, matches12):
        """CreateNewMapPoints' triangulation for one pair in host memory (orbx_triangulate_matches) -> (points [n1, 3], mask [n1],
        normals [n1, 3], dist [n1, 2], TriResult).  Synchronous."""
        k1, k2 = _keys(keys_un1), _keys(keys_un2)
        m12 = np.ascontiguousarray(matches12, np.int32).reshape(-1)
        if len(m12) != len(k1):
            raise OrbxError(E_BADARG, "matches12 needs one entry per feature of the first keyframe")
        n = max(len(k1), 1)
        pts, msk, nrm, dst = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32)
        p1, p2 = _pose12(Tcw1), _pose12(Tcw2)
        Kf = _k9(K)
        res = TriResult()
        r = self._L.orbx_triangulate_matches(self._h, _ptr(k1), len(k1), _ptr(p1), _ptr(k2), len(k2), _ptr(p2), _ptr(Kf), _ptr(m12),
                                             _ptr(pts), _ptr(msk), _ptr(nrm), _ptr(dst), ctypes.byref(res))
        self._check(r, "orbx_triangulate_matches")
        return pts[:len(k1)], msk[:len(k1)], nrm[:len(k1)], dst[:len(k1)], res

    def relocalize_refine_pairs_device(self, n_frames: int, kf: np.ndarray, cur: np.ndarray, point_set: np.ndarray, d_kps_un, d_desc,
                                       d_n, n_point_sets: int, d_points, d_point_mask, d_point_dist, d_pose0, d_matches, K,
                                       bounds: Tuple[int, int, int, int], d_point_desc=None, capacity: Optional[int] = None):
        """The tail of Tracking::Relocalization behind PnPsolver for a batch of (lost frame cur[p], candidate keyframe kf[p]) pairs,
        on torch tensors: d_pose0 float32 [n_pairs, 12] the start poses and d_matches int32 [n_pairs, capacity] the inlier rows as
        PnP leaves them (updated in place).  Each stage is ONE batched call over the pairs still alive; between stages the host
        reads the counts once (ORB-SLAM2's loop is host-driven there too):
          1. PoseOptimization; nGood < 10: dropped
          2. where nGood < 50: SearchByProjection(th 10, ORBdist 100) with that call's outlier flags
          3. where nadditional + nGood >= 50: PoseOptimization
          4. where 30 < nGood < 50: SearchByProjection(th 3, ORBdist 64), no outlier flags
          5. where nGood + nadditional >= 50: PoseOptimization, then the outliers' entries are cleared
        with ORBmatcher(0.9, true): the orientation check is on.  A pair that ends at stage 1 with nGood >= 10 has its outliers'
        entries cleared as Relocalization clears them.  -> (stage int32 [n_pairs] the last stage the pair ran, nGood int32
        [n_pairs], d_pose float32 [n_pairs, 12], d_matches)."""
        import torch
        kf, cur, point_set = _pair_lists(("kf", "cur", "point_set"), (kf, cur, point_set))
        cap, P = int(capacity or self.capacity), len(kf)
        _need("the pose array", d_pose0, P * 48)
        _need("matches", d_matches, P * cap * 4)
        dev = d_matches.device
        rows = d_matches.view(torch.int32).reshape(-1)[:P * cap].view(P, cap)
        pose = d_pose0.view(torch.float32).reshape(-1)[:P * 12].view(P, 12).clone()
        stage, n_good = np.zeros(P, np.int32), np.zeros(P, np.int32)
        mine = torch.cuda.current_stream(dev).cuda_stream

        def optimise(idx, which):
            """One PoseOptimization call over the pairs idx -> (nGood [len(idx)], their outlier flags [len(idx), cap], idx on the device)."""
            sel = torch.from_numpy(idx.astype(np.int64)).to(dev)
            r, p0 = rows[sel].contiguous(), pose[sel].contiguous()
            res = torch.empty(len(idx) * POSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            out = torch.zeros(len(idx) * cap, dtype=torch.uint8, device=dev)
            self.pose_optimize_batch_device(n_frames, cur[idx], point_set[idx], d_kps_un, d_n, r, n_point_sets, d_points, d_point_mask, p0, K,
                                            res, out, capacity=cap)
            self.order_before(mine)
            rec = res.view(len(idx), POSE_RESULT_DTYPE.itemsize)
            pose[sel] = rec[:, 144:192].contiguous().view(torch.float32)  # (the record ends with R [9] and tcw [3] as f32: a pose row)
            good = rec[:, 12:16].contiguous().view(torch.int32).reshape(-1).cpu().numpy()  # n_inliers: the design's return value
            stage[idx], n_good[idx] = which, good
            return good, out.view(len(idx), cap), sel

        def search(idx, th, orb_dist, outl):
            """One SearchByProjection call over the pairs idx -> nadditional [len(idx)]."""
            sel = torch.from_numpy(idx.astype(np.int64)).to(dev)
            r, p = rows[sel].contiguous(), pose[sel].contiguous()
            res = torch.empty(len(idx) * KFPROJ_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            self.match_keyframe_projection_pairs_device(n_frames, kf[idx], cur[idx], point_set[idx], d_kps_un, d_desc, d_n, n_point_sets,
                                                        d_points, d_point_mask, d_point_dist, p, K, bounds, r, res, th=th, ORBdist=orb_dist,
                                                        checkOri=True, d_point_desc=d_point_desc, d_outlier=outl, capacity=cap)
            self.order_before(mine)
            rows[sel] = r
            return res.view(len(idx), KFPROJ_RESULT_DTYPE.itemsize)[:, 4:8].contiguous().view(torch.int32).reshape(-1).cpu().numpy()

        def clear(sel, out):
            r = rows[sel]
            rows[sel] = torch.where(out != 0, torch.full_like(r, -1), r)

        if P == 0:
            return stage, n_good, pose, d_matches
        every = np.arange(P)
        good, out, sel = optimise(every, 1)                                             # 1
        done = np.flatnonzero((good >= 10) & (good >= 50))
        if len(done):
            k = torch.from_numpy(done.astype(np.int64)).to(dev)
            clear(sel[k], out[k])
        k = np.flatnonzero((good >= 10) & (good < 50))
        if len(k):
            idx = every[k]
            kk = torch.from_numpy(k.astype(np.int64)).to(dev)
            extra = search(idx, 10.0, 100, out[kk].contiguous())                        # 2
            stage[idx] = 2
            idx = idx[extra + n_good[idx] >= 50]
            if len(idx):
                good, out, sel = optimise(idx, 3)                                       # 3
                k = np.flatnonzero((good > 30) & (good < 50))
                if len(k):
                    idx = idx[k]
                    extra = search(idx, 3.0, 64, None)                                  # 4
                    stage[idx] = 4
                    idx = idx[n_good[idx] + extra >= 50]
                    if len(idx):
                        good, out, sel = optimise(idx, 5)                               # 5
                        clear(sel, out)
        return stage, n_good, pose, d_matches

    def extract_match_batch_device(self, d_imgs, n_frames: int, width: int, height: int, stride: int, frame_stride: int,
                                   d_kps, d_desc, d_n, first: np.ndarray, second: np.ndarray,
                                   bounds: Tuple[int, int, int, int], d_matches12, d_nmatches, d_stats=None,
                                   windowSize: int = 100, nnratio: float = 0.9, checkOri: bool = True,
                                   capacity: Optional[int] = None) -> None:
        """The whole hot path of one batch (extract + match of pairs inside the batch), two half-batches on two streams."""
        first = np.ascontiguousarray(first, np.int32)
        second = np.ascontiguousarray(second, np.int32)
        b = _Bounds(*[int(v) for v in bounds])
        _need_batch(d_imgs, int(n_frames), int(width), int(height), int(stride), int(frame_stride), d_kps, d_desc, d_n,
                    int(capacity or self.capacity), first, second, d_matches12, d_nmatches, d_stats)
        self._order_torch(d_imgs, d_kps, d_desc, d_n, d_matches12, d_nmatches, d_stats)
        r = self._L.orbx_extract_match_batch_device(self._h, int(n_frames), _ptr(d_imgs), int(width), int(height), int(stride),
                                                    int(frame_stride), _ptr(d_kps), _ptr(d_desc), int(capacity or self.capacity),
                                                    _ptr(d_n), len(first), _ptr(first), _ptr(second), ctypes.byref(b),
                                                    int(windowSize), float(nnratio), int(bool(checkOri)), _ptr(d_matches12),
                                                    _ptr(d_nmatches), _ptr(d_stats))
        self._check(r, "orbx_extract_match_batch_device")

    def extract_match_batch_device_async(self, d_imgs, n_frames: int, width: int, height: int, stride: int, frame_stride: int,
                                         d_kps, d_desc, d_n, first: np.ndarray, second: np.ndarray,
                                         bounds: Tuple[int, int, int, int], d_matches12, d_nmatches, d_stats=None,
                                         windowSize: int = 100, nnratio: float = 0.9, checkOri: bool = True,
                                         capacity: Optional[int] = None) -> None:
        """Stream-ordered form: issues the batch and returns; at most two batches in flight (``wait_one`` / ``wait``).
        Batches in flight together need different output arrays."""
        first = np.ascontiguousarray(first, np.int32)
        second = np.ascontiguousarray(second, np.int32)
        b = _Bounds(*[int(v) for v in bounds])
        _need_batch(d_imgs, int(n_frames), int(width), int(height), int(stride), int(frame_stride), d_kps, d_desc, d_n,
                    int(capacity or self.capacity), first, second, d_matches12, d_nmatches, d_stats)
        self._order_torch(d_imgs, d_kps, d_desc, d_n, d_matches12, d_nmatches, d_stats)
        r = self._L.orbx_extract_match_batch_device_async(self._h, int(n_frames), _ptr(d_imgs), int(width), int(height),
                                                          int(stride), int(frame_stride), _ptr(d_kps), _ptr(d_desc),
                                                          int(capacity or self.capacity), _ptr(d_n), len(first), _ptr(first),
                                                          _ptr(second), ctypes.byref(b), int(windowSize), float(nnratio),
                                                          int(bool(checkOri)), _ptr(d_matches12), _ptr(d_nmatches), _ptr(d_stats))
        self._check(r, "orbx_extract_match_batch_device_async")

    def extract_match_batch_host_async(self, h_imgs, n_frames: int, width: int, height: int, stride: int, frame_stride: int,
                                       h_kps, h_desc, h_n, first: np.ndarray, second: np.ndarray,
                                       bounds: Tuple[int, int, int, int], h_matches12, h_nmatches, h_stats=None,
                                       windowSize: int = 100, nnratio: float = 0.9, checkOri: bool = True,
                                       capacity: Optional[int] = None) -> None:
        """Stream-ordered call for HOST frames and HOST result arrays (numpy arrays or pinned torch CPU tensors; page-locked memory
        keeps the copies asynchronous): upload, kernels and the copies back are queued on the lane the batch goes to.  Valid after
        ``wait_one`` / ``wait``; everything must stay untouched until then."""
        first = np.ascontiguousarray(first, np.int32)
        second = np.ascontiguousarray(second, np.int32)
        b = _Bounds(*[int(v) for v in bounds])
        _need_batch(h_imgs, int(n_frames), int(width), int(height), int(stride), int(frame_stride), h_kps, h_desc, h_n,
                    int(capacity or self.capacity), first, second, h_matches12, h_nmatches, h_stats)
        r = self._L.orbx_extract_match_batch_host_async(self._h, int(n_frames), _ptr(h_imgs), int(width), int(height),
                                                        int(stride), int(frame_stride), _ptr(h_kps), _ptr(h_desc),
                                                        int(capacity or self.capacity), _ptr(h_n), len(first), _ptr(first),
                                                        _ptr(second), ctypes.byref(b), int(windowSize), float(nnratio),
                                                        int(bool(checkOri)), _ptr(h_matches12), _ptr(h_nmatches), _ptr(h_stats))
        self._check(r, "orbx_extract_match_batch_host_async")

    def set_pipeline_depth(self, depth: int) -> None:
        """depth >= 1: every stream-ordered batch goes, whole, to the next of `depth` lanes (own stream, own buffers); at most `depth`
        batches in flight, which need `depth` different output arrays.  0 (default): two half batches on the context's two streams."""
        self._check(self._L.orbx_set_pipeline_depth(self._h, int(depth)), "orbx_set_pipeline_depth")

    def wait_one(self) -> None:
        """Waits for the oldest batch in flight."""
        self._check(self._L.orbx_wait_one(self._h), "orbx_wait_one")

    def wait(self) -> None:
        """Waits for every batch in flight."""
        self._check(self._L.orbx_wait(self._h), "orbx_wait")

    # -- Converter::toGray (Utils/Converter.cpp:5-19) --------------------------------------------------
    def to_gray(self, image: np.ndarray, bRGB: bool = False) -> np.ndarray:
        """(h, w) or (h, w, 1) copies; (h, w, 3) is cvtColor(RGB2GRAY if bRGB else BGR2GRAY); else OrbxError (returns false upstream)."""
        im = np.asarray(image)
        if im.dtype != np.uint8 or im.ndim not in (2, 3):
            raise OrbxError(E_BADARG, "image must be uint8 (h, w) or (h, w, c)")
        ch = 1 if im.ndim == 2 else im.shape[2]
        h, w = im.shape[:2]
        if im.strides[-1] != 1 or (im.ndim == 3 and im.strides[1] != ch):
            im = np.ascontiguousarray(im)
        out = np.zeros((h, w), np.uint8)
        self._check(self._L.orbx_to_gray(self._h, _ptr(im), w, h, im.strides[0] if h else w * ch, ch, int(bool(bRGB)), _ptr(out),
                                         w), "orbx_to_gray")
        return out

    def to_gray_batch_device(self, d_src, n_frames: int, width: int, height: int, stride: int, frame_stride: int, channels: int,
                             bRGB: bool, d_gray, gray_stride: int, gray_frame_stride: int) -> None:
        nf, w, h, ch = int(n_frames), int(width), int(height), int(channels)
        some = nf > 0 and h > 0  # (the last frame's last row ends the bytes the call touches)
        self._device_call("orbx_to_gray_batch_device", nf,
                          ("the source frames", d_src, (nf - 1) * int(frame_stride) + (h - 1) * int(stride) + w * ch if some else 0), w, h,
                          int(stride), int(frame_stride), ch, int(bool(bRGB)),
                          ("the gray frames", d_gray, (nf - 1) * int(gray_frame_stride) + (h - 1) * int(gray_stride) + w if some else 0),
                          int(gray_stride), int(gray_frame_stride))

    # -- Frame::UndistortKeyPoints / ComputeImageBounds (SlamTypes/Frame.cpp:101-161) ----------------
    def undistort_keypoints(self, kps: np.ndarray, camera: Sequence[float]) -> np.ndarray:
        """mvKeysUn from mvKeys; camera = (fx, fy, cx, cy, k1, k2, p1, p2)."""
        kps = _keys(kps)
        out = np.zeros(len(kps), KEYPOINT_DTYPE)
        cam = _Camera(*[float(v) for v in camera])
        self._check(self._L.orbx_undistort_keypoints(self._h, _ptr(kps), len(kps), ctypes.byref(cam), _ptr(out)),
                    "orbx_undistort_keypoints")
        return out

    def undistort_batch_device(self, n_frames: int, d_kps, d_n, camera: Sequence[float], d_kps_un,
                               capacity: Optional[int] = None) -> None:
        cap, nf = int(capacity or self.capacity), int(n_frames)
        self._device_call("orbx_undistort_batch_device", nf, ("the keypoint array", d_kps, nf * cap * 28), ("the count array", d_n, nf * 4),
                          cap, ctypes.byref(_Camera(*[float(v) for v in camera])), ("the undistorted keypoint array", d_kps_un, nf * cap * 28))

    def image_bounds(self, camera: Sequence[float], width: int, height: int) -> Tuple[int, int, int, int]:
        cam = _Camera(*[float(v) for v in camera])
        b = _Bounds()
        self._check(self._L.orbx_image_bounds(self._h, ctypes.byref(cam), int(width), int(height), ctypes.byref(b)),
                    "orbx_image_bounds")
        return (b.min_x, b.max_x, b.min_y, b.max_y)

    # -- Initializer::CheckHomography / CheckFundamental (Initialization/Initializer.cpp:268-438) ------
    def _check_models(self, kind: int, M21, M12, keys1, keys2, matches12, sigma: float):
        M21 = np.ascontiguousarray(M21, np.float32).reshape(-1, 3, 3)
        k1 = _keys(keys1)
        k2 = _keys(keys2)
        m12 = np.ascontiguousarray(matches12, np.int32)
        if len(m12) != len(k1):
            raise OrbxError(E_BADARG, "matches12 must have one entry per keypoint of frame 1")
        nm = len(M21)
        scores = np.zeros(nm, np.float32)
        inl = np.zeros(max(nm * len(k1), 1), np.uint8)
        n, best = ctypes.c_int(0), ctypes.c_int(-1)
        if kind == 0:
            M12 = np.ascontiguousarray(M12, np.float32).reshape(-1, 3, 3)
            if len(M12) != nm:
                raise OrbxError(E_BADARG, "H21 and H12 must hold the same number of models")
            r = self._L.orbx_check_homography(self._h, nm, _ptr(M21), _ptr(M12), _ptr(k1), len(k1), _ptr(k2), len(k2), _ptr(m12),
                                              float(sigma), _ptr(scores), _ptr(inl), ctypes.byref(n), ctypes.byref(best))
        else:
            r = self._L.orbx_check_fundamental(self._h, nm, _ptr(M21), _ptr(k1), len(k1), _ptr(k2), len(k2), _ptr(m12),
                                               float(sigma), _ptr(scores), _ptr(inl), ctypes.byref(n), ctypes.byref(best))
        self._check(r, "orbx_check_homography" if kind == 0 else "orbx_check_fundamental")
        return scores, inl[:nm * n.value].reshape(nm, n.value).astype(bool), best.value

    def check_homography(self, H21, H12, keys1, keys2, matches12, sigma: float = 1.0):
        """CheckHomography for a stack of hypotheses -> (scores, vbMatchesInliers per model, index the RANSAC loop keeps)."""
        return self._check_models(0, H21, H12, keys1, keys2, matches12, sigma)

    def check_fundamental(self, F21, keys1, keys2, matches12, sigma: float = 1.0):
        """CheckFundamental for a stack of hypotheses -> (scores, vbMatchesInliers per model, index the RANSAC loop keeps)."""
        return self._check_models(1, F21, None, keys1, keys2, matches12, sigma)

    def check_rt(self, R21, t21, K, keys1, keys2, matches12, matches_inliers, th2: float = 4.0):
        """Initializer::CheckRT (Initializer.cpp:569-713) for a stack of (R21, t21) hypotheses ->
        (nGood[m], vbTriGood[m, n1], vP3D[m, n1, 3], parallax[m])."""
        R21 = np.ascontiguousarray(R21, np.float32).reshape(-1, 3, 3)
        t21 = _points(t21)
        K = np.ascontiguousarray(K, np.float32).reshape(3, 3)
        k1 = _keys(keys1)
        k2 = _keys(keys2)
        m12 = np.ascontiguousarray(matches12, np.int32)
        inl = np.ascontiguousarray(matches_inliers, np.uint8)
        nm = len(R21)
        if len(t21) != nm or len(m12) != len(k1) or len(inl) != int((m12 >= 0).sum()):
            raise OrbxError(E_BADARG, "check_rt: one t21 per R21, one matches12 entry per keypoint of frame 1, one inlier flag per match")
        ngood = np.zeros(max(nm, 1), np.int32)
        par = np.zeros(max(nm, 1), np.float32)
        good = np.zeros((max(nm, 1), max(len(k1), 1)), np.uint8)
        p3d = np.zeros((max(nm, 1), max(len(k1), 1), 3), np.float32)
        self._check(self._L.orbx_check_rt(self._h, nm, _ptr(R21), _ptr(t21), _ptr(K), _ptr(k1), len(k1), _ptr(k2), len(k2), _ptr(m12),
                                          _ptr(inl), float(th2), _ptr(ngood), _ptr(good), _ptr(p3d), _ptr(par)), "orbx_check_rt")
        return ngood[:nm], good[:nm, :len(k1)].astype(bool), p3d[:nm, :len(k1)], par[:nm]

    # -- the RANSAC stage of Initializer::Initialize (Initialization/Initializer.cpp:19-111) ---------
    def find_models(self, keys1, keys2, matches12, sets, sigma: float = 1.0, debug: bool = False):
        """One pair from host memory: mvKeys1 / mvKeys2 (mvKeysUn), vnMatches12 (one entry per keypoint of frame 1), mvSets
        [n_iter, 8] (sample_sets).  Returns (HFResult, inliers [2, N] bool: the kept H's, then F's, vbMatchesInliers); with
        debug=True also every hypothesis (models [3, n_iter, 3, 3] = H21, H12, F21) and its score (scores [2, n_iter])."""
        k1 = _keys(keys1)
        k2 = _keys(keys2)
        m12 = np.ascontiguousarray(matches12, np.int32)
        sets = np.ascontiguousarray(sets, np.int32)
        if len(m12) != len(k1):
            raise OrbxError(E_BADARG, "matches12 must have one entry per keypoint of frame 1")
        if sets.ndim != 2 or sets.shape[1] != 8:
            raise OrbxError(E_BADARG, "sets must be [n_iter, 8]")
        n_iter = len(sets)
        res = HFResult()
        inl = np.zeros((2, max(len(k1), 1)), np.uint8)
        models = np.zeros((3, max(n_iter, 1), 3, 3), np.float32) if debug else None
        scores = np.zeros((2, max(n_iter, 1)), np.float32) if debug else None
        self._check(self._L.orbx_find_models(self._h, _ptr(k1), len(k1), _ptr(k2), len(k2), _ptr(m12), n_iter, _ptr(sets),
                                             float(sigma), ctypes.byref(res), _ptr(inl), _ptr(models), _ptr(scores)),
                    "orbx_find_models")
        inliers = inl[:, :res.n_matches].astype(bool)
        if debug:
            return res, inliers, models, scores
        return res, inliers

    def find_models_batch_device(self, n_frames: int, first: np.ndarray, second: np.ndarray, d_kps_un, d_n, d_matches12, d_sets,
                                 d_res, d_inliers=None, d_models=None, d_scores=None, sigma: float = 1.0,
                                 capacity: Optional[int] = None, n_iter: Optional[int] = None) -> None:
        """Batched and device-resident (device pointers or torch tensors): pair p = frame first[p] vs second[p] of the
        extract / undistort layout; d_sets int32 [n_pairs, n_iter, 8]; d_res [n_pairs] HF_RESULT_DTYPE-sized records (152 bytes);
        d_inliers uint8 [n_pairs, 2, capacity], d_models float32 [3, n_pairs, n_iter, 9], d_scores float32 [2, n_pairs, n_iter]
        are optional.  n_iter: from d_sets' shape when it is a [n_pairs, n_iter, 8] tensor, else required.  Stream-ordered on the
        context's stream: the outputs are valid after a device synchronisation (torch.cuda.synchronize())."""
        first, second = _pair_lists(("first", "second"), (first, second))
        cap, nf, P = int(capacity or self.capacity), int(n_frames), len(first)
        n_iter = self._n_iter(d_sets, P, n_iter)
        self._device_call("orbx_find_models_batch_device", nf, P, first, second, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the count array", d_n, nf * 4), cap, ("matches12", d_matches12, P * cap * 4), n_iter,
                          ("the sets", d_sets, P * n_iter * 32), float(sigma), ("the result array", d_res, P * HF_RESULT_DTYPE.itemsize),
                          ("the inlier array", d_inliers, P * 2 * cap), ("the model array", d_models, 3 * P * n_iter * 36),
                          ("the score array", d_scores, 2 * P * n_iter * 4))

    @staticmethod
    def _n_iter(d_sets, n_pairs: int, n_iter: Optional[int]) -> int:
        shape = getattr(d_sets, "shape", None)
        if shape is not None and len(shape) == 3:
            if int(shape[0]) != n_pairs or int(shape[2]) != 8 or (n_iter is not None and int(n_iter) != int(shape[1])):
                raise OrbxError(E_BADARG, "d_sets must be [n_pairs, n_iter, 8]")
            return int(shape[1])
        if n_iter is None:
            raise OrbxError(E_BADARG, "n_iter is required when d_sets is not a [n_pairs, n_iter, 8] tensor")
        return int(n_iter)

    # -- Initializer::Initialize end to end (Initialization/Initializer.cpp:19-125) ------------------
    def initialize(self, keys1, keys2, matches12, sets, K, sigma: float = 1.0, min_parallax: float = 1.0, min_triangulated: int = 50):
        """One pair from host memory: mvKeys1 / mvKeys2 (mvKeysUn), vnMatches12, mvSets [n_iter, 8] (sample_sets), K 3x3.  Returns
        (InitResult, vP3D [n1, 3] float32, vbTriangulated [n1] bool); result.status == 0 is Initialize's `true`."""
        k1 = _keys(keys1)
        k2 = _keys(keys2)
        m12 = np.ascontiguousarray(matches12, np.int32)
        sets = np.ascontiguousarray(sets, np.int32)
        Kf = _k9(K)
        if len(m12) != len(k1):
            raise OrbxError(E_BADARG, "matches12 must have one entry per keypoint of frame 1")
        if sets.ndim != 2 or sets.shape[1] != 8:
            raise OrbxError(E_BADARG, "sets must be [n_iter, 8]")
        res = InitResult()
        p3d = np.zeros((max(len(k1), 1), 3), np.float32)
        tri = np.zeros(max(len(k1), 1), np.uint8)
        self._check(self._L.orbx_initialize(self._h, _ptr(k1), len(k1), _ptr(k2), len(k2), _ptr(m12), len(sets), _ptr(sets), _ptr(Kf),
                                            float(sigma), float(min_parallax), int(min_triangulated), ctypes.byref(res), _ptr(p3d),
                                            _ptr(tri)), "orbx_initialize")
        return res, p3d[:len(k1)], tri[:len(k1)].astype(bool)

    def initialize_batch_device(self, n_frames: int, first: np.ndarray, second: np.ndarray, d_kps_un, d_n, d_matches12, d_sets, K,
                                d_res, d_p3d=None, d_triangulated=None, sigma: float = 1.0, min_parallax: float = 1.0,
                                min_triangulated: int = 50, capacity: Optional[int] = None, n_iter: Optional[int] = None) -> None:
        """Batched and device-resident (device pointers or torch tensors), the layout of find_models_batch_device; d_res
        [n_pairs] INIT_RESULT_DTYPE records (184 bytes), d_p3d float32 [n_pairs, capacity, 3] and d_triangulated uint8
        [n_pairs, capacity] optional.  Stream-ordered: the outputs are valid after a device synchronisation."""
        first, second = _pair_lists(("first", "second"), (first, second))
        cap, nf, P = int(capacity or self.capacity), int(n_frames), len(first)
        n_iter = self._n_iter(d_sets, P, n_iter)
        self._device_call("orbx_initialize_batch_device", nf, P, first, second, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the count array", d_n, nf * 4), cap, ("matches12", d_matches12, P * cap * 4), n_iter,
                          ("the sets", d_sets, P * n_iter * 32), _k9(K), float(sigma), float(min_parallax), int(min_triangulated),
                          ("the result array", d_res, P * INIT_RESULT_DTYPE.itemsize), ("the point array", d_p3d, P * cap * 12),
                          ("the triangulated array", d_triangulated, P * cap))

    # -- two-view bundle adjustment behind the Initializer (include/orbx.h) ------------------------------
    def bundle_adjust(self, keys1, keys2, matches12, init_res, p3d, triangulated, K, inv_sigma2=None, n_iterations: int = 20,
                      min_points: int = 100, normalize: bool = True):
        """One pair from host memory: what initialize() took and returned (its InitResult, vP3D, vbTriangulated).  Returns
        (BAResult, refined vP3D [n1, 3] float32); result.status == 0 is an accepted initial map."""
        k1 = _keys(keys1)
        k2 = _keys(keys2)
        m12 = np.ascontiguousarray(matches12, np.int32)
        pts = _points(p3d)
        tri = np.ascontiguousarray(np.asarray(triangulated) != 0, np.uint8)
        Kf = _k9(K)
        if len(m12) != len(k1) or len(pts) != len(k1) or len(tri) != len(k1):
            raise OrbxError(E_BADARG, "matches12, p3d and triangulated must have one entry per keypoint of frame 1")
        if isinstance(init_res, InitResult):
            ir = init_res
        else:
            ir = InitResult.from_buffer_copy(np.ascontiguousarray(init_res, INIT_RESULT_DTYPE).tobytes())
        sig = _per_level(inv_sigma2, self.nlevels, "inv_sigma2")
        res = BAResult()
        out = np.zeros((max(len(k1), 1), 3), np.float32)
        self._check(self._L.orbx_bundle_adjust(self._h, _ptr(k1), len(k1), _ptr(k2), len(k2), _ptr(m12), ctypes.byref(ir), _ptr(pts),
                                               _ptr(tri), _ptr(Kf), _ptr(sig), int(n_iterations), int(min_points), int(bool(normalize)),
                                               ctypes.byref(res), _ptr(out)), "orbx_bundle_adjust")
        return res, out[:len(k1)]

    def bundle_adjust_batch_device(self, n_frames: int, first: np.ndarray, second: np.ndarray, d_kps_un, d_n, d_matches12, d_init_res,
                                   d_p3d, d_triangulated, K, d_res, d_p3d_out=None, inv_sigma2=None, n_iterations: int = 20,
                                   min_points: int = 100, normalize: bool = True, capacity: Optional[int] = None) -> None:
        """Batched and device-resident, chained behind initialize_batch_device on the same arrays (its d_res, d_p3d,
        d_triangulated); d_res [n_pairs] BA_RESULT_DTYPE records (168 bytes); d_p3d_out float32 [n_pairs, capacity, 3], None =
        in place (d_p3d).  Stream-ordered: the outputs are valid after a device synchronisation."""
        first = np.ascontiguousarray(first, np.int32)
        second = np.ascontiguousarray(second, np.int32)
        cap = int(capacity or self.capacity)
        if len(second) != len(first):
            raise OrbxError(E_BADARG, "first and second must have the same length")
        if d_p3d_out is None:
            d_p3d_out = d_p3d
        Kf = _k9(K)
        sig = _per_level(inv_sigma2, self.nlevels, "inv_sigma2")
        n_frames = int(n_frames)
        _need_batch(None, n_frames, 0, 0, 0, 0, d_kps_un, None, d_n, cap, first, second, d_matches12, None, None, init_res=d_init_res,
                    p3d=d_p3d, triangulated=d_triangulated, ba_res=d_res, p3d_out=d_p3d_out)
        self._order_torch(d_kps_un, d_n, d_matches12, d_init_res, d_p3d, d_triangulated, d_res, d_p3d_out)
        self._check(self._L.orbx_bundle_adjust_batch_device(self._h, n_frames, len(first), _ptr(first), _ptr(second), _ptr(d_kps_un),
                                                            _ptr(d_n), cap, _ptr(d_matches12), _ptr(d_init_res), _ptr(d_p3d),
                                                            _ptr(d_triangulated), _ptr(Kf), _ptr(sig), int(n_iterations),
                                                            int(min_points), int(bool(normalize)), _ptr(d_res), _ptr(d_p3d_out)),
                    "orbx_bundle_adjust_batch_device")

    # -- Optimizer::PoseOptimization behind SearchByBoW (include/orbx.h) -------------------------------------
    def pose_optimize(self, keys_un, points, mask, Tcw, K, inv_sigma2=None, n_iterations: int = 10):
        """One problem from host memory: the frame's mvKeysUn, one map point per feature (points [n, 3], mask [n] or None = every
        feature has one), the start pose Tcw (3x4 or 4x4) and K.  Returns (PoseResult, vbOutlier [n] bool); result.n_inliers is
        the reference design's return value."""
        k = _keys(keys_un)
        pts = _points(points)
        m = _flags(mask, len(k), "points and mask must have one entry per keypoint of the frame")
        if len(pts) != len(k):
            raise OrbxError(E_BADARG, "points and mask must have one entry per keypoint of the frame")
        pose0 = _pose12(Tcw)
        Kf = _k9(K)
        sig = _per_level(inv_sigma2, self.nlevels, "inv_sigma2")
        res = PoseResult()
        out = np.zeros(max(len(k), 1), np.uint8)
        self._check(self._L.orbx_pose_optimize(self._h, _ptr(k), len(k), _ptr(pts), _ptr(m), _ptr(pose0), _ptr(Kf), _ptr(sig),
                                               int(n_iterations), ctypes.byref(res), _ptr(out)), "orbx_pose_optimize")
        return res, out[:len(k)].astype(bool)

    def pose_optimize_batch_device(self, n_frames: int, frame: np.ndarray, point_set: np.ndarray, d_kps_un, d_n, d_match, n_point_sets: int,
                                   d_points, d_point_mask, d_pose0, K, d_res, d_outlier, inv_sigma2=None, n_iterations: int = 10,
                                   capacity: Optional[int] = None) -> None:
        """Batched and device-resident: problem p optimises frame frame[p] against point set point_set[p] (d_points float32
        [n_point_sets, capacity, 3], d_point_mask uint8 [n_point_sets, capacity] or None) from d_pose0 float32 [n_problems, 12].
        d_match int32 [n_problems, capacity] is match_bow_batch_device's d_matches_f (the point sets are then the keyframes' map
        points), or None = feature j's point is entry j.  d_res [n_problems] POSE_RESULT_DTYPE records (192 bytes), d_outlier
        uint8 [n_problems, capacity].  Stream-ordered: the outputs are valid after a device synchronisation."""
        frame, point_set = _pair_lists(("frame", "point_set"), (frame, point_set))
        cap, P, nf, ns = int(capacity or self.capacity), len(frame), int(n_frames), int(n_point_sets)
        sig = _per_level(inv_sigma2, self.nlevels, "inv_sigma2")
        self._device_call("orbx_pose_optimize_batch_device", nf, P, frame, point_set, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the count array", d_n, nf * 4), cap, ("the match array", d_match, P * cap * 4), ns,
                          ("the point array", d_points, ns * cap * 12), ("the point mask", d_point_mask, ns * cap),
                          ("the pose array", d_pose0, P * 48), _k9(K), sig, int(n_iterations),
                          ("the result array", d_res, P * POSE_RESULT_DTYPE.itemsize), ("the outlier array", d_outlier, P * cap))

    # -- Optimizer::LocalBundleAdjustment behind Fuse (include/orbx.h, "local mapping: local bundle adjustment") -----------
    def local_ba_problems_device(self, n_frames: int, first, count, n_free, map_set, entry_frame, d_kps_un, d_n, d_pose, d_rows,
                                 n_map_sets: int, map_capacity: int, d_map_n, d_map_points, d_map_mask, K, d_pose_out, d_obs_outlier,
                                 d_res, d_map_points_out=None, inv_sigma2=None, n_iterations: int = 5, n_more_iterations: int = 10,
                                 capacity: Optional[int] = None) -> None:
        """Batched and device-resident: problem p adjusts the entries first[p] .. first[p] + count[p] - 1 of the entry list (the
        first n_free[p] free, the rest fixed; entry e is frame entry_frame[e] of d_kps_un / d_n / d_pose float32 [n_frames, 12])
        against map set map_set[p].  d_rows int32 [n_entries, capacity]: the keyframes' mvpMapPoints as indices into the
        problem's set, what match_local_map_pairs_device, match_scw_pairs_device and MapFuser.fuse_pairs_device leave in their
        match arrays.  d_pose_out float32 [n_entries, 12], d_obs_outlier uint8 [n_entries, capacity], d_res [n_problems]
        LBA_RESULT_DTYPE records (128 bytes); d_map_points_out None = in place.  Stream-ordered."""
        first, count, n_free, map_set = _pair_lists(("first", "count", "n_free", "map_set"), (first, count, n_free, map_set))
        entry_frame = np.ascontiguousarray(entry_frame, np.int32).reshape(-1)
        cap, mcap, nf, ns, P, E = int(capacity or self.capacity), int(map_capacity), int(n_frames), int(n_map_sets), len(first), len(entry_frame)
        if d_map_points_out is None:
            d_map_points_out = d_map_points
        sig = _per_level(inv_sigma2, self.nlevels, "inv_sigma2")
        self._device_call("orbx_local_ba_batch_device", nf, P, first, count, n_free, map_set, E, entry_frame,
                          ("the keypoint array", d_kps_un, nf * cap * 28), ("the count array", d_n, nf * 4), cap,
                          ("the pose array", d_pose, nf * 48), ("the row array", d_rows, E * cap * 4), ns, mcap,
                          ("the map count array", d_map_n, ns * 4), ("the map point array", d_map_points, ns * mcap * 12),
                          ("the map mask", d_map_mask, ns * mcap), _k9(K), sig, int(n_iterations), int(n_more_iterations),
                          ("the pose output array", d_pose_out, E * 48), ("the map point output array", d_map_points_out, ns * mcap * 12),
                          ("the outlier array", d_obs_outlier, E * cap), ("the result array", d_res, P * LBA_RESULT_DTYPE.itemsize))

    def local_ba(self, keys_un, n, poses, rows, n_free: int, map_points, map_mask, K, inv_sigma2=None, n_iterations: int = 5,
                 n_more_iterations: int = 10):
        """One problem from host memory: keys_un [n_entries, capacity] keypoints (n [n_entries] of them valid per keyframe), poses
        [n_entries, 12], rows int32 [n_entries, capacity], the first n_free keyframes free; map_points [map_n, 3], map_mask [map_n]
        or None.  Returns (LbaResult, poses [n_entries, 12] float32, map points [map_n, 3] float32, vToErase as uint8 [n_entries,
        capacity])."""
        k = np.ascontiguousarray(keys_un, KEYPOINT_DTYPE)
        if k.ndim != 2:
            raise OrbxError(E_BADARG, "keys_un must be [n_entries, capacity]")
        E, cap = k.shape
        cnt = np.ascontiguousarray(n, np.int32).reshape(-1)
        pose = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
        r = np.ascontiguousarray(rows, np.int32).reshape(-1, cap) if E else np.zeros((0, cap), np.int32)
        pts = _points(map_points)
        if len(cnt) != E or len(pose) != E or len(r) != E:
            raise OrbxError(E_BADARG, "n, poses and rows must have one entry per keyframe")
        m = _flags(map_mask, len(pts), "the map mask needs one entry per map point")
        sig = _per_level(inv_sigma2, self.nlevels, "inv_sigma2")
        res = LbaResult()
        pose_out, pts_out = np.zeros((max(E, 1), 12), np.float32), np.zeros((max(len(pts), 1), 3), np.float32)
        outlier = np.zeros((max(E, 1), max(cap, 1)), np.uint8)
        self._check(self._L.orbx_local_ba(self._h, E, int(n_free), _ptr(k), _ptr(cnt), max(cap, 1), _ptr(pose), _ptr(r), len(pts), _ptr(pts),
                                          _ptr(m), _ptr(_k9(K)), _ptr(sig), int(n_iterations), int(n_more_iterations), _ptr(pose_out),
                                          _ptr(pts_out), _ptr(outlier), ctypes.byref(res)), "orbx_local_ba")
        return res, pose_out[:E], pts_out[:len(pts)], outlier[:E]

    # -- behind the local bundle adjustment (include/orbx.h, "local mapping: updating the map points") ---------------------
    def map_update_problems_device(self, n_frames: int, first, count, n_free, map_set, entry_frame, d_kps_un, d_desc, d_n, d_entry_pose,
                                   d_rows, d_obs_outlier, n_map_sets: int, map_capacity: int, d_map_n, d_map_points, d_map_mask,
                                   d_map_obs, d_res, d_map_normals=None, d_map_dist=None, d_map_desc=None, d_map_ref=None,
                                   d_map_mask_out=None, what: int = MAP_NORMALS | MAP_DESCRIPTORS, capacity: Optional[int] = None) -> None:
        """Batched and device-resident: the problems are those of local_ba_problems_device (d_entry_pose float32 [n_entries, 12] is
        its d_pose_out, d_obs_outlier its vToErase bytes or None, d_rows int32 [n_entries, capacity] is rewritten: erased and
        cleared observations become -1).  For every adjusted point: d_map_obs int32 [n_map_sets, map_capacity] (Observations()),
        with MAP_NORMALS d_map_normals float32 [.., 3] and d_map_dist float32 [.., 2] (UpdateNormalAndDepth), with
        MAP_DESCRIPTORS d_map_desc uint8 [.., 32] (ComputeDistinctiveDescriptors); d_map_mask_out None = in place (d_map_mask
        must then be given); d_map_ref int32 [.., map_capacity] or None: the reference keyframes as frame indices, in and out;
        d_res [n_problems] MAP_RESULT_DTYPE records (64 bytes).  Stream-ordered."""
        first, count, n_free, map_set = _pair_lists(("first", "count", "n_free", "map_set"), (first, count, n_free, map_set))
        entry_frame = np.ascontiguousarray(entry_frame, np.int32).reshape(-1)
        cap, mcap, nf, ns, P, E = int(capacity or self.capacity), int(map_capacity), int(n_frames), int(n_map_sets), len(first), len(entry_frame)
        if d_map_mask_out is None:
            d_map_mask_out = d_map_mask
        self._device_call("orbx_map_update_batch_device", nf, P, first, count, n_free, map_set, E, entry_frame,
                          ("the keypoint array", d_kps_un, nf * cap * 28), ("the descriptor array", d_desc, nf * cap * 32),
                          ("the count array", d_n, nf * 4), cap, ("the entry pose array", d_entry_pose, E * 48),
                          ("the row array", d_rows, E * cap * 4), ("the outlier array", d_obs_outlier, E * cap), ns, mcap,
                          ("the map count array", d_map_n, ns * 4), ("the map point array", d_map_points, ns * mcap * 12),
                          ("the map mask", d_map_mask, ns * mcap), ("the map mask output", d_map_mask_out, ns * mcap),
                          ("the reference keyframe array", d_map_ref, ns * mcap * 4), int(what),
                          ("the map normal array", d_map_normals, ns * mcap * 12), ("the map distance array", d_map_dist, ns * mcap * 8),
                          ("the map descriptor array", d_map_desc, ns * mcap * 32), ("the map observation array", d_map_obs, ns * mcap * 4),
                          ("the result array", d_res, P * MAP_RESULT_DTYPE.itemsize))

    def map_update(self, keys_un, desc, n, poses, rows, n_free: int, map_points, map_mask=None, obs_outlier=None, map_ref=None,
                   map_normals=None, map_dist=None, map_desc=None, map_obs=None, what: int = MAP_NORMALS | MAP_DESCRIPTORS):
        """One problem from host memory: keys_un [n_entries, capacity], desc [n_entries, capacity, 32], n [n_entries], poses
        [n_entries, 12] (the adjusted ones), rows int32 [n_entries, capacity], the first n_free keyframes free; obs_outlier
        [n_entries, capacity] or None; map_points [map_n, 3]; map_mask, map_ref (frame = keyframe index, -1 = none) [map_n] or
        None; map_normals / map_dist / map_desc / map_obs: the arrays as they stand (None = zeros), of which the call rewrites
        the adjusted points' rows.  Returns (MapResult, dict(rows, mask, ref, obs, normals, dist, desc))."""
        k = np.ascontiguousarray(keys_un, KEYPOINT_DTYPE)
        if k.ndim != 2:
            raise OrbxError(E_BADARG, "keys_un must be [n_entries, capacity]")
        E, cap = k.shape
        cnt = np.ascontiguousarray(n, np.int32).reshape(-1)
        pose = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
        r = np.array(rows, np.int32).reshape(-1, cap) if E else np.zeros((0, cap), np.int32)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, cap, 32) if E else np.zeros((0, cap, 32), np.uint8)
        pts = _points(map_points)
        N = len(pts)
        if len(cnt) != E or len(pose) != E or len(r) != E or len(d) != E:
            raise OrbxError(E_BADARG, "desc, n, poses and rows must have one entry per keyframe")
        m = _flags(map_mask, N, "the map mask needs one entry per map point")
        ol = None if obs_outlier is None else np.ascontiguousarray(np.asarray(obs_outlier) != 0, np.uint8).reshape(-1, cap)
        if ol is not None and len(ol) != E:
            raise OrbxError(E_BADARG, "obs_outlier needs one row per keyframe")

        def have(a, dtype, width, what_):
            out = np.zeros((max(N, 1),) + width, dtype)
            if a is not None:
                given = np.asarray(a, dtype).reshape((-1,) + width)
                if len(given) != N:
                    raise OrbxError(E_BADARG, "%s needs one row per map point" % what_)
                out[:N] = given
            return out
        mask_out = have(np.ones(N, np.uint8) if m is None else m, np.uint8, (), "the map mask")
        ref = None if map_ref is None else have(map_ref, np.int32, (), "map_ref")
        nrm, dst = have(map_normals, np.float32, (3,), "map_normals"), have(map_dist, np.float32, (2,), "map_dist")
        dsc, obs = have(map_desc, np.uint8, (32,), "map_desc"), have(map_obs, np.int32, (), "map_obs")
        res = MapResult()
        self._check(self._L.orbx_map_update(self._h, E, int(n_free), _ptr(k), _ptr(d), _ptr(cnt), max(cap, 1), _ptr(pose), _ptr(r), _ptr(ol), N,
                                            _ptr(pts), _ptr(m), _ptr(mask_out), _ptr(ref), int(what), _ptr(nrm), _ptr(dst), _ptr(dsc),
                                            _ptr(obs), ctypes.byref(res)), "orbx_map_update")
        return res, dict(rows=r, mask=mask_out[:N], ref=None if ref is None else ref[:N], obs=obs[:N], normals=nrm[:N], dist=dst[:N],
                         desc=dsc[:N])

    # -- the stereo Frame (include/orbx.h, "stereo: matching left and right") -------------------------------------------------
    def stereo_match_rigs_device(self, n_frames: int, left, right, d_kps, d_desc, d_n, bf: float, b: float, d_u_right, d_depth, d_res,
                                 d_match_right=None, d_sad=None, d_kps_un=None, K=None, d_pose_wc=None, d_points=None,
                                 d_point_mask=None, capacity: Optional[int] = None) -> None:
        """Frame::ComputeStereoMatches for rigs (left frame left[p], right frame right[p]; host index arrays) of the LAST
        extract_batch_device call, whose pyramid is still resident (its d_imgs must still be there: level 0 is read in place).
        d_kps / d_desc / d_n are that call's outputs (raw mvKeys).  Rows [n_rigs, capacity]: d_u_right, d_depth float32 (mvuRight,
        mvDepth; -1 = none), optional d_match_right, d_sad int32; with d_points float32 [n_rigs, capacity, 3] (and K) the
        matches are unprojected as Frame::UnprojectStereo does, (u, v) from d_kps_un when given, through d_pose_wc float32
        [n_rigs, 12] (Rwc row-major, then Ow) when given, d_point_mask uint8 [n_rigs, capacity] = depth > 0: a point set for
        match_projection_pairs_device / pose_optimize_batch_device.  d_res [n_rigs] STEREO_RESULT_DTYPE records (64 bytes).
        Stream-ordered."""
        left, right = _pair_lists(("left", "right"), (left, right))
        cap, nf, P = int(capacity or self.capacity), int(n_frames), len(left)
        self._device_call("orbx_stereo_match_batch_device", nf, P, left, right, ("the keypoint array", d_kps, nf * cap * 28),
                          ("the descriptor array", d_desc, nf * cap * 32), ("the count array", d_n, nf * 4), cap, float(bf), float(b),
                          ("the u_right array", d_u_right, P * cap * 4), ("the depth array", d_depth, P * cap * 4),
                          ("the right-match array", d_match_right, P * cap * 4), ("the SAD array", d_sad, P * cap * 4),
                          ("the undistorted keypoint array", d_kps_un, nf * cap * 28), None if K is None else _k9(K),
                          ("the pose array", d_pose_wc, P * 48), ("the point array", d_points, P * cap * 12),
                          ("the point mask", d_point_mask, P * cap), ("the result array", d_res, P * STEREO_RESULT_DTYPE.itemsize))

    def extract_stereo(self, left: np.ndarray, right: np.ndarray, bf: float, b: float):
        """The stereo Frame constructor for one rig in host memory (orbx_extract_stereo): both images through the extractor as a
        batch of two, then Frame::ComputeStereoMatches.  Returns ((keysL, descL), (keysR, descR), mvuRight, mvDepth,
        StereoResult), mvuRight / mvDepth float32 [len(keysL)] with -1 where there is no match.  Synchronous."""
        imgs = [np.ascontiguousarray(im) for im in (left, right)]
        if any(im.dtype != np.uint8 or im.ndim != 2 for im in imgs) or imgs[0].shape != imgs[1].shape:
            raise OrbxError(E_BADARG, "left and right must be 2-D uint8 arrays of one shape")
        h, w = imgs[0].shape
        cap = self.capacity
        kps, desc = np.zeros((2, cap), KEYPOINT_DTYPE), np.zeros((2, cap, 32), np.uint8)
        n = np.zeros(2, np.int32)
        ur, z = np.full(cap, -1, np.float32), np.full(cap, -1, np.float32)
        res = StereoResult()
        self._check(self._L.orbx_extract_stereo(self._h, _ptr(imgs[0]), _ptr(imgs[1]), w, h, w, float(bf), float(b), _ptr(kps[0]), _ptr(desc[0]),
                                                _ptr(n[0:1]), _ptr(kps[1]), _ptr(desc[1]), _ptr(n[1:2]), cap, _ptr(ur), _ptr(z),
                                                ctypes.byref(res)), "orbx_extract_stereo")
        nl, nr = int(n[0]), int(n[1])
        return (kps[0, :nl].copy(), desc[0, :nl].copy()), (kps[1, :nr].copy(), desc[1, :nr].copy()), ur[:nl].copy(), z[:nl].copy(), res

    # -- PnPsolver behind SearchByBoW (include/orbx.h, "behind SearchByBoW: PnP RANSAC") ------------------------
    def pnp_solve(self, keys_un, points, mask, K, draws, sigma2=None, probability: float = 0.99, min_inliers: int = 10,
                  max_iterations: int = 300, epsilon: float = 0.5, th2: float = 5.991):
        """One problem from host memory: the frame's mvKeysUn, one map point per feature (points [n, 3], mask [n] or None = every
        feature has one), K and the draws int32 [n_iter, 4] (sample_pnp_draws).  One call is the solver's whole life: up to
        min(n_iter, mRansacMaxIts) iterations.  Returns (PnpResult, vbInliers [n] bool)."""
        k = _keys(keys_un)
        pts = _points(points)
        m = _flags(mask, len(k), "points and mask must have one entry per keypoint of the frame")
        if len(pts) != len(k):
            raise OrbxError(E_BADARG, "points and mask must have one entry per keypoint of the frame")
        d = np.ascontiguousarray(draws, np.int32).reshape(-1, 4)
        Kf = _k9(K)
        sig = _per_level(sigma2, self.nlevels, "sigma2")
        res = PnpResult()
        out = np.zeros(max(len(k), 1), np.uint8)
        self._check(self._L.orbx_pnp_solve(self._h, _ptr(k), len(k), _ptr(pts), _ptr(m), _ptr(Kf), _ptr(sig), float(probability),
                                           int(min_inliers), int(max_iterations), float(epsilon), float(th2), len(d), _ptr(d),
                                           ctypes.byref(res), _ptr(out)), "orbx_pnp_solve")
        return res, out[:len(k)].astype(bool)

    def pnp_solve_batch_device(self, n_frames: int, frame: np.ndarray, point_set: np.ndarray, d_kps_un, d_n, d_match, n_point_sets: int,
                               d_points, d_point_mask, K, d_draws, d_res, d_pose, d_match_inliers, d_inliers=None, sigma2=None,
                               probability: float = 0.99, min_inliers: int = 10, max_iterations: int = 300, epsilon: float = 0.5,
                               th2: float = 5.991, n_iter: Optional[int] = None, capacity: Optional[int] = None) -> None:
        """Batched and device-resident: problem p solves frame frame[p] against point set point_set[p]; every array up to
        d_point_mask is pose_optimize_batch_device's.  d_draws int32 [n_problems, n_iter, 4] (n_iter: default from its size).
        Outputs: d_res [n_problems] PNP_RESULT_DTYPE records (200 bytes), d_pose float32 [n_problems, 12] and d_match_inliers int32
        [n_problems, capacity] -- pose_optimize_batch_device's d_pose0 and d_match for the same lists --, d_inliers uint8
        [n_problems, capacity] or None.  Stream-ordered: the outputs are valid after a device synchronisation."""
        frame, point_set = _pair_lists(("frame", "point_set"), (frame, point_set))
        cap, P, nf, ns = int(capacity or self.capacity), len(frame), int(n_frames), int(n_point_sets)
        n_iter = self._draws_n_iter(d_draws, P, 4, n_iter)
        sig = _per_level(sigma2, self.nlevels, "sigma2")
        self._device_call("orbx_pnp_solve_batch_device", nf, P, frame, point_set, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the count array", d_n, nf * 4), cap, ("the match array", d_match, P * cap * 4), ns,
                          ("the point array", d_points, ns * cap * 12), ("the point mask", d_point_mask, ns * cap), _k9(K), sig,
                          float(probability), int(min_inliers), int(max_iterations), float(epsilon), float(th2), n_iter,
                          ("the draws", d_draws, P * max(n_iter, 0) * 16), ("the result array", d_res, P * PNP_RESULT_DTYPE.itemsize),
                          ("the pose array", d_pose, P * 48), ("the inlier match array", d_match_inliers, P * cap * 4),
                          ("the inlier flags", d_inliers, P * cap))

    @staticmethod
    def _draws_n_iter(d_draws, n_problems: int, width: int, n_iter: Optional[int]) -> int:
        """n_iter as given, or from the size of d_draws int32 [n_problems, n_iter, width] (0 for a raw pointer)."""
        if n_iter is None:
            nbytes = _nbytes(d_draws)
            n_iter = nbytes // (4 * width * n_problems) if n_problems and nbytes is not None else 0
        return int(n_iter)

    # -- Sim3Solver of loop closing (include/orbx.h, "loop closing: Sim3 RANSAC") ----------------------------------
    def sim3_solve(self, keys_un1, points1, mask1, pose1, keys_un2, points2, mask2, pose2, match12, K, draws, sigma2=None,
                   fix_scale: bool = False, probability: float = 0.99, min_inliers: int = 20, max_iterations: int = 300,
                   th2: float = 9.210):
        """One keyframe pair from host memory: each keyframe's mvKeysUn, one map point per feature (points [n, 3], mask [n]; both
        masks None = every feature has one), its pose Tcw (12 floats: R row-major, then t), the row match12 [n1] (KF2's feature
        matched to KF1's, or -1), K and the draws int32 [n_iter, 3] (sample_sim3_draws).  One call is the solver's whole life.
        Returns (Sim3Result, sim3 [13] float32 = R12, t12, s12, the inlier row [n1] int32, vbInliers [n1] bool)."""
        k1 = _keys(keys_un1)
        k2 = _keys(keys_un2)
        p1 = _points(points1)
        p2 = _points(points2)
        if (mask1 is None) != (mask2 is None):
            raise OrbxError(E_BADARG, "the two masks are given together or not at all")
        message = "points, mask and match12 must have one entry per keypoint of their keyframe"
        m1, m2 = _flags(mask1, len(k1), message), _flags(mask2, len(k2), message)
        row = np.ascontiguousarray(match12, np.int32).reshape(-1)
        if len(p1) != len(k1) or len(p2) != len(k2) or len(row) != len(k1):
            raise OrbxError(E_BADARG, message)
        T1, T2 = (np.ascontiguousarray(np.asarray(T, np.float32).reshape(-1)[:12]) for T in (pose1, pose2))
        d = np.ascontiguousarray(draws, np.int32).reshape(-1, 3)
        Kf = _k9(K)
        sig = _per_level(sigma2, self.nlevels, "sigma2")
        res, sim = Sim3Result(), np.zeros(13, np.float32)
        out_row, out = np.full(max(len(k1), 1), -1, np.int32), np.zeros(max(len(k1), 1), np.uint8)
        self._check(self._L.orbx_sim3_solve(self._h, _ptr(k1), len(k1), _ptr(p1), _ptr(m1), _ptr(T1), _ptr(k2), len(k2), _ptr(p2),
                                            _ptr(m2), _ptr(T2), _ptr(row), _ptr(Kf), _ptr(sig), int(bool(fix_scale)),
                                            float(probability), int(min_inliers), int(max_iterations), float(th2), len(d), _ptr(d),
                                            ctypes.byref(res), _ptr(sim), _ptr(out_row), _ptr(out)), "orbx_sim3_solve")
        return res, sim, out_row[:len(k1)], out[:len(k1)].astype(bool)

    def sim3_solve_batch_device(self, n_frames: int, kf1: np.ndarray, kf2: np.ndarray, set1: np.ndarray, set2: np.ndarray, d_kps_un,
                                d_n, d_match, n_point_sets: int, d_points, d_point_mask, d_pose, K, d_draws, d_res, d_sim3,
                                d_match_inliers, d_inliers=None, sigma2=None, fix_scale: bool = False, probability: float = 0.99,
                                min_inliers: int = 20, max_iterations: int = 300, th2: float = 9.210, n_iter: Optional[int] = None,
                                capacity: Optional[int] = None) -> None:
        """Batched and device-resident: problem p finds the similarity between keyframe kf1[p] (the current one; its points are
        set set1[p]) and keyframe kf2[p] (the candidate; set set2[p]).  d_match int32 [n_problems, capacity]: KF2's feature
        matched to KF1's, or -1 (match_bow_pairs_device's row with KF1 on the frame side); d_pose float32 [n_frames, 12]; d_draws
        int32 [n_problems, n_iter, 3] (n_iter: default from its size).  Outputs: d_res [n_problems] SIM3_RESULT_DTYPE records (96
        bytes), d_sim3 float32 [n_problems, 13] (R12, t12, s12), d_match_inliers int32 [n_problems, capacity], d_inliers uint8
        [n_problems, capacity] or None.  Stream-ordered: the outputs are valid after a device synchronisation."""
        kf1, kf2, set1, set2 = _pair_lists(("kf1", "kf2", "set1", "set2"), (kf1, kf2, set1, set2))
        cap, P, nf, ns = int(capacity or self.capacity), len(kf1), int(n_frames), int(n_point_sets)
        n_iter = self._draws_n_iter(d_draws, P, 3, n_iter)
        sig = _per_level(sigma2, self.nlevels, "sigma2")
        self._device_call("orbx_sim3_solve_batch_device", nf, P, kf1, kf2, set1, set2, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the count array", d_n, nf * 4), cap, ("the match array", d_match, P * cap * 4), ns,
                          ("the point array", d_points, ns * cap * 12), ("the point mask", d_point_mask, ns * cap),
                          ("the pose array", d_pose, nf * 48), _k9(K), sig, int(bool(fix_scale)), float(probability), int(min_inliers),
                          int(max_iterations), float(th2), n_iter, ("the draws", d_draws, P * max(n_iter, 0) * 12),
                          ("the result array", d_res, P * SIM3_RESULT_DTYPE.itemsize), ("the similarity array", d_sim3, P * 52),
                          ("the inlier match array", d_match_inliers, P * cap * 4), ("the inlier flags", d_inliers, P * cap))

    # -- Optimizer::OptimizeSim3 of loop closing (include/orbx.h, "loop closing: Sim3 optimisation") ----------------
    def optimize_sim3(self, keys_un1, points1, mask1, pose1, keys_un2, points2, mask2, pose2, matches12, sim3, K, inv_sigma2=None,
                      fix_scale: bool = False, th2: float = 10.0, n_iterations: int = 5, n_more_iterations: int = 10):
        """One keyframe pair from host memory, in sim3_solve's layout: each keyframe's mvKeysUn, one map point per feature (points
        [n, 3], mask [n]; both masks None = every feature has one), its pose Tcw (12 floats), the row matches12 [n1] (KF2's
        feature matched to KF1's, or -1: vpMatches1), the start similarity sim3 [13] (R12, t12, s12) and K.  Returns
        (Sim3OptResult, sim3 [13] float32, the edited row [n1] int32: removed entries are -1)."""
        k1 = _keys(keys_un1)
        k2 = _keys(keys_un2)
        p1 = _points(points1)
        p2 = _points(points2)
        if (mask1 is None) != (mask2 is None):
            raise OrbxError(E_BADARG, "the two masks are given together or not at all")
        message = "points, mask and matches12 must have one entry per keypoint of their keyframe"
        m1, m2 = _flags(mask1, len(k1), message), _flags(mask2, len(k2), message)
        row = np.array(matches12, np.int32).reshape(-1)  # (a copy: edited in place)
        if len(p1) != len(k1) or len(p2) != len(k2) or len(row) != len(k1):
            raise OrbxError(E_BADARG, message)
        T1, T2 = (np.ascontiguousarray(np.asarray(T, np.float32).reshape(-1)[:12]) for T in (pose1, pose2))
        sim = np.ascontiguousarray(sim3, np.float32).reshape(13)
        Kf = _k9(K)
        sig = _per_level(inv_sigma2, self.nlevels, "inv_sigma2")
        res, out = Sim3OptResult(), np.zeros(13, np.float32)
        if len(row) == 0:
            row = np.full(1, -1, np.int32)
        self._check(self._L.orbx_optimize_sim3(self._h, _ptr(k1), len(k1), _ptr(p1), _ptr(m1), _ptr(T1), _ptr(k2), len(k2), _ptr(p2),
                                               _ptr(m2), _ptr(T2), _ptr(row), _ptr(sim), _ptr(Kf), _ptr(sig), int(bool(fix_scale)),
                                               float(th2), int(n_iterations), int(n_more_iterations), ctypes.byref(res), _ptr(out)),
                    "orbx_optimize_sim3")
        return res, out, row[:len(k1)]

    def optimize_sim3_pairs_device(self, n_frames: int, kf1, kf2, set1, set2, d_kps_un, d_n, d_matches, n_point_sets: int, d_points,
                                   d_point_mask, d_pose, d_sim3, K, d_res, d_sim3_out=None, inv_sigma2=None, fix_scale: bool = False,
                                   th2: float = 10.0, n_iterations: int = 5, n_more_iterations: int = 10,
                                   capacity: Optional[int] = None) -> None:
        """Batched and device-resident: problem p refines the similarity d_sim3[p] (float32 [n_problems, 13]: R12, t12, s12, as
        sim3_solve_batch_device writes it) between keyframe kf1[p] (point set set1[p]) and keyframe kf2[p] (set2[p]) over the
        row d_matches[p] (int32 [n_problems, capacity], as match_sim3_pairs_device leaves it), which is edited in place: a removed
        correspondence becomes -1.  Outputs: d_res [n_problems] SIM3OPT_RESULT_DTYPE records (208 bytes); d_sim3_out float32
        [n_problems, 13], default d_sim3 itself.  Stream-ordered: valid after a device synchronisation."""
        kf1, kf2, set1, set2 = _pair_lists(("kf1", "kf2", "set1", "set2"), (kf1, kf2, set1, set2))
        cap, P, nf, ns = int(capacity or self.capacity), len(kf1), int(n_frames), int(n_point_sets)
        sig = _per_level(inv_sigma2, self.nlevels, "inv_sigma2")
        self._device_call("orbx_optimize_sim3_batch_device", nf, P, kf1, kf2, set1, set2, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the count array", d_n, nf * 4), cap, ("the match array", d_matches, P * cap * 4), ns,
                          ("the point array", d_points, ns * cap * 12), ("the point mask", d_point_mask, ns * cap),
                          ("the pose array", d_pose, nf * 48), ("the similarity array", d_sim3, P * 52), _k9(K), sig,
                          int(bool(fix_scale)), float(th2), int(n_iterations), int(n_more_iterations),
                          ("the result array", d_res, P * SIM3OPT_RESULT_DTYPE.itemsize),
                          ("the output similarity array", d_sim3 if d_sim3_out is None else d_sim3_out, P * 52))

    def compute_sim3_optimized_pairs_device(self, n_frames: int, kf1, kf2, set1, set2, d_kps_un, d_desc, d_n, d_match, n_point_sets: int,
                                            d_points, d_point_mask, d_point_dist, d_pose, K, bounds: Tuple[int, int, int, int], d_draws,
                                            d_sim3_res, d_sim3, d_matches, d_msim3_res, d_opt_res, d_point_desc=None,
                                            fix_scale: bool = False, th: float = 7.5, ORBdist: int = 100, opt_th2: float = 10.0,
                                            n_iterations: int = 5, n_more_iterations: int = 10, inv_sigma2=None,
                                            capacity: Optional[int] = None, **ransac) -> None:
        """LoopClosing::ComputeSim3 for pairs up to the number that decides whether a candidate closes the loop: the two calls
        of compute_sim3_pairs_device, then optimize_sim3_pairs_device on the similarity and the widened row they leave, all
        three queued on the context's stream with no copy and no wait between them.  d_sim3 is refined in place, d_matches loses
        the correspondences the optimisation removes, d_opt_res[p].n_inliers is nInliers (a loop needs >= 20).  A pair without a
        similarity has zeros in d_sim3: the optimiser flags it (SIM3OPT_NONFINITE: s12 <= 0) and returns its inputs."""
        self.compute_sim3_pairs_device(n_frames, kf1, kf2, set1, set2, d_kps_un, d_desc, d_n, d_match, n_point_sets, d_points,
                                       d_point_mask, d_point_dist, d_pose, K, bounds, d_draws, d_sim3_res, d_sim3, d_matches, d_msim3_res,
                                       d_point_desc, fix_scale, th, ORBdist, capacity, **ransac)
        self.optimize_sim3_pairs_device(n_frames, kf1, kf2, set1, set2, d_kps_un, d_n, d_matches, n_point_sets, d_points, d_point_mask,
                                        d_pose, d_sim3, K, d_opt_res, None, inv_sigma2, fix_scale, opt_th2, n_iterations,
                                        n_more_iterations, capacity)

    # -- the Scw SearchByProjection of loop closing (include/orbx.h, "loop closing: matching the loop's points under Scw") ------
    def sim3_compose_scw_pairs_device(self, n_frames: int, kf2, d_pose, d_sim3, d_scw) -> None:
        """d_scw[p] (float32 [n_pairs, 12]: sR row-major, then t) = S12 * Tmw from d_sim3[p] (float32 [n_pairs, 13]: R12, t12,
        s12, keyframe 1 the current one) and the matched keyframe's pose d_pose[kf2[p]] (float32 [n_frames, 12]).  A pair without
        a similarity gets twelve zeros.  Stream-ordered on the context's stream."""
        kf2 = np.ascontiguousarray(kf2, np.int32).reshape(-1)
        P, nf = len(kf2), int(n_frames)
        self._device_call("orbx_sim3_compose_scw_batch_device", nf, P, kf2, ("the pose array", d_pose, nf * 48),
                          ("the similarity array", d_sim3, P * 52), ("the Scw array", d_scw, P * 48))

    def sim3_compose_scw(self, pose2, sim3) -> np.ndarray:
        """One pair from host memory: pose2 (Tmw, 12 floats or 3x4 / 4x4), sim3 [13] -> Scw [12] float32.  Synchronous."""
        T2 = _pose12(pose2)  # (12 floats as they are, a matrix as R [9] then t [3])
        sim = np.ascontiguousarray(sim3, np.float32).reshape(13)
        out = np.zeros(12, np.float32)
        self._check(self._L.orbx_sim3_compose_scw(self._h, _ptr(T2), _ptr(sim), _ptr(out)), "orbx_sim3_compose_scw")
        return out

    def match_scw_pairs_device(self, n_frames: int, kf: np.ndarray, map_set: np.ndarray, d_kps_un, d_desc, d_n, n_map_sets: int,
                               map_capacity: int, d_map_n, d_map_points, d_map_normals, d_map_dist, d_map_desc, d_map_mask, d_scw, K,
                               bounds: Tuple[int, int, int, int], d_matches, d_res, th: float = 10.0, th_low: int = 50,
                               d_kf2_to_map=None, capacity: Optional[int] = None) -> None:
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) of LoopClosing::ComputeSim3 for pairs (current
        keyframe kf[p], map set map_set[p]; host index arrays): the map sets are match_local_map_pairs_device's arrays, d_scw
        float32 [n_pairs, 12] is what sim3_compose_scw_pairs_device writes.  d_matches int32 [n_pairs, capacity] is read and
        written: feature j's index into the pair's map set, SCW_TAKEN_UNMAPPED, or another negative value (free).  With
        d_kf2_to_map int32 [n_pairs, capacity] the row holds the matched keyframe's feature indices on entry (the optimiser's
        row) and is translated through the table.  d_res [n_pairs] SCW_RESULT_DTYPE records (56 bytes); n_total is
        nTotalMatches.  Stream-ordered on the context's stream."""
        cap, mcap, nf, ns = int(capacity or self.capacity), int(map_capacity), int(n_frames), int(n_map_sets)
        kf, map_set = _pair_lists(("kf", "map_set"), (kf, map_set), nf, ns, "map set")
        P = len(kf)
        self._device_call("orbx_match_scw_batch_device", nf, P, kf, map_set, ("the keypoint array", d_kps_un, nf * cap * 28),
                          ("the descriptor array", d_desc, nf * cap * 32), ("the count array", d_n, nf * 4), cap, ns, mcap,
                          ("the map count array", d_map_n, ns * 4), ("the map point array", d_map_points, ns * mcap * 12),
                          ("the map normal array", d_map_normals, ns * mcap * 12), ("the map distance array", d_map_dist, ns * mcap * 8),
                          ("the map descriptor array", d_map_desc, ns * mcap * 32), ("the map mask", d_map_mask, ns * mcap),
                          ("the Scw array", d_scw, P * 48), _k9(K), ctypes.byref(_bounds(bounds)), float(th), int(th_low),
                          ("matches", d_matches, P * cap * 4),
                          ("the table from the matched keyframe's features to the map set", d_kf2_to_map, P * cap * 4),
                          ("the result array", d_res, P * SCW_RESULT_DTYPE.itemsize))

    def match_scw(self, keys_un, desc, map_points, map_normals, map_dist, map_desc, map_mask, Scw, K,
                  bounds: Tuple[int, int, int, int], matches=None, th: float = 10.0, th_low: int = 50, kf2_to_map=None):
        """The same for one keyframe and one map set in host memory (orbx_match_scw) -> (matches int32 [len(keys_un)],
        MatchScwResult).  Scw: 12 floats (sR row-major, then t) or a 3x4 / 4x4 matrix; matches (default all -1): vpMatched as
        indices into the map arrays, or with kf2_to_map as the matched keyframe's feature indices.  Synchronous."""
        k = _keys(keys_un)
        d = _desc(desc)
        mp = _points(map_points)
        mn = _points(map_normals)
        md = _points(map_dist, 2)
        mdesc = _desc(map_desc)
        if len(k) != len(d) or not (len(mp) == len(mn) == len(md) == len(mdesc)):
            raise OrbxError(E_BADARG, "keypoints / descriptors or the map arrays differ in length")
        mm = _flags(map_mask, len(mp), "the map mask needs one entry per map point")
        m = _row(matches, len(k), "matches needs one entry per feature")
        tab = None if kf2_to_map is None else np.ascontiguousarray(kf2_to_map, np.int32).reshape(-1)
        S = _pose12(Scw)
        Kf = _k9(K)
        b = _bounds(bounds)
        res = MatchScwResult()
        r = self._L.orbx_match_scw(self._h, _ptr(k), _ptr(d), len(k), len(mp), _ptr(mp), _ptr(mn), _ptr(md), _ptr(mdesc), _ptr(mm),
                                   _ptr(S), _ptr(Kf), ctypes.byref(b), float(th), int(th_low), _ptr(m), _ptr(tab),
                                   0 if tab is None else len(tab), ctypes.byref(res))
        self._check(r, "orbx_match_scw")
        return m[:len(k)].copy(), res

    def compute_sim3_loop_pairs_device(self, n_frames: int, kf1, kf2, set1, set2, d_kps_un, d_desc, d_n, d_match, n_point_sets: int,
                                       d_points, d_point_mask, d_point_dist, d_pose, K, bounds: Tuple[int, int, int, int], d_draws,
                                       d_sim3_res, d_sim3, d_matches, d_msim3_res, d_opt_res, map_set, n_map_sets: int,
                                       map_capacity: int, d_map_n, d_map_points, d_map_normals, d_map_dist, d_map_desc, d_map_mask,
                                       d_kf2_to_map, d_scw, d_scw_res, loop_th: float = 10.0, th_low: int = 50,
                                       capacity: Optional[int] = None, **sim3_args) -> None:
        """LoopClosing::ComputeSim3 for pairs up to its decision: compute_sim3_optimized_pairs_device (its arguments, and its
        keyword arguments through **sim3_args), then mScw = Scm * Smw (sim3_compose_scw_pairs_device into d_scw), then the Scw
        SearchByProjection of map set map_set[p] into keyframe kf1[p] on the row the optimiser leaves, translated through
        d_kf2_to_map -- all queued on the context's stream with no copy and no wait between them.  d_matches ends as
        mvpCurrentMatchedPoints (indices into the map set), d_scw_res[p].n_total is nTotalMatches; self.loop_accepted(d_opt_res,
        d_scw_res) reads the two arrays back behind these calls and applies the two gates."""
        self.compute_sim3_optimized_pairs_device(n_frames, kf1, kf2, set1, set2, d_kps_un, d_desc, d_n, d_match, n_point_sets,
                                                 d_points, d_point_mask, d_point_dist, d_pose, K, bounds, d_draws, d_sim3_res, d_sim3,
                                                 d_matches, d_msim3_res, d_opt_res, capacity=capacity, **sim3_args)
        self.sim3_compose_scw_pairs_device(n_frames, kf2, d_pose, d_sim3, d_scw)
        self.match_scw_pairs_device(n_frames, kf1, map_set, d_kps_un, d_desc, d_n, n_map_sets, map_capacity, d_map_n, d_map_points,
                                    d_map_normals, d_map_dist, d_map_desc, d_map_mask, d_scw, K, bounds, d_matches, d_scw_res, loop_th,
                                    th_low, d_kf2_to_map, capacity)

    def loop_accepted(self, d_opt_res, d_scw_res, min_inliers: int = 20, min_total: int = 40) -> np.ndarray:
        """ComputeSim3's decision from the two result arrays compute_sim3_loop_pairs_device filled (torch device tensors, or host
        record arrays) -> accepted [n_pairs] bool: n_inliers >= 20 and n_total >= 40.  Ordered: a device tensor is read back on
        torch's current stream of its device, which this call first places behind everything issued on the context so far
        (order_before), and the copy to the host waits for that stream -- no device-wide synchronisation is needed, or made,
        between the chain and this call.  Work issued on the context AFTER this call is not waited for."""
        def host(a):
            if isinstance(a, np.ndarray):
                return a
            import torch
            self.order_before(torch.cuda.current_stream(a.device).cuda_stream)
            return a.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()
        return loop_accepted(host(d_opt_res), host(d_scw_res), min_inliers, min_total)

    # -- mvImagePyramid (hpp:111) ----------------------------------------------------------------
    def level_size(self, level: int) -> Tuple[int, int]:
        w, h = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._L.orbx_level_size(self._h, level, ctypes.byref(w), ctypes.byref(h)), "orbx_level_size")
        return w.value, h.value

    def image_pyramid(self, level: int, frame: int = 0, border: int = 0) -> np.ndarray:
        w, h = self.level_size(level)
        out = np.zeros((h + 2 * border, w + 2 * border), np.uint8)
        self._check(self._L.orbx_download_pyramid(self._h, frame, level, border, _ptr(out), out.strides[0]), "orbx_download_pyramid")
        return out

    # -- measurement / test hooks ------------------------------------------------------------------
    def profile_enable(self, on: bool = True):
        self._L.orbx_profile_enable(self._h, int(on))

    def profile_stages(self, stages) -> None:
        """Bracket only the given stages (names of STAGES) with events."""
        mask = 0
        for name in stages:
            mask |= 1 << STAGES.index(name)
        self._L.orbx_profile_stages(self._h, mask)

    def profile_reset(self):
        self._L.orbx_profile_reset(self._h)

    def profile_get(self):
        ms = np.zeros(len(STAGES), np.float64)
        cnt = np.zeros(len(STAGES), np.int64)
        self._L.orbx_profile_get(self._h, _ptr(ms), _ptr(cnt))
        return {s: (float(ms[i]), int(cnt[i])) for i, s in enumerate(STAGES)}

    def debug_distribute_device(self, xyr: np.ndarray, min_x: int, max_x: int, min_y: int, max_y: int, n_features: int,
                                variant: int = 0) -> np.ndarray:
        """The device selection kernels on caller-supplied, row-major ordered candidates (test hook)."""
        xyr = _points(xyr)
        out = np.zeros((max(n_features, 1), 3), np.float32)
        r = self._check(self._L.orbx_debug_distribute_device(self._h, _ptr(xyr), len(xyr), min_x, max_x, min_y, max_y,
                                                             n_features, variant, _ptr(out), len(out)))
        return out[:r]

    def debug_std_sort(self, triples: np.ndarray) -> np.ndarray:
        t = np.ascontiguousarray(triples, np.int32).reshape(-1, 3).copy()
        self._check(self._L.orbx_debug_std_sort(self._h, _ptr(t), len(t)))
        return t

    def debug_sincos(self, angles_deg: np.ndarray):
        a = np.ascontiguousarray(angles_deg, np.float32)
        c, s = np.zeros(len(a), np.float32), np.zeros(len(a), np.float32)
        self._check(self._L.orbx_debug_sincos(self._h, _ptr(a), len(a), _ptr(c), _ptr(s)))
        return c, s

    def debug_last_launch(self) -> dict:
        """How the last extraction batch was issued (include/orbx.h: orbx_debug_last_launch)."""
        v = np.zeros(8, np.int32)
        self._check(self._L.orbx_debug_last_launch(self._h, _ptr(v)), "orbx_debug_last_launch")
        return dict(pyramid_banded=int(v[0]), pyramid_bands=int(v[1]), fast_wave=int(v[2]), octree_instance=int(v[3]),
                    split=int(v[4]) & 1, staged_lists=(int(v[4]) >> 1) & 1, describe_pairs=(int(v[4]) >> 2) & 1,
                    frames_per_launch=int(v[5]), wide_with_batch=int(v[6]),
                    lane=int(v[7]))

    def debug_match_counters(self) -> dict:
        """Which matcher kernels did the work, cumulative for this context (include/orbx.h: orbx_debug_match_counters)."""
        v = np.zeros(4, np.uint32)
        self._check(self._L.orbx_debug_match_counters(self._h, _ptr(v)), "orbx_debug_match_counters")
        return dict(bf_mfma_blocks=int(v[0]))

    def debug_selection_units(self, frame: int = 0):
        """(counts, redone) per pyramid level of one frame of the last batch (include/orbx.h: orbx_debug_selection_units)."""
        c, r = np.zeros(self.GetLevels(), np.int32), np.zeros(self.GetLevels(), np.int32)
        self._check(self._L.orbx_debug_selection_units(self._h, int(frame), _ptr(c), _ptr(r)), "orbx_debug_selection_units")
        return c, r

    def debug_candidates(self, frame: int, level: int) -> np.ndarray:
        n = self._check(self._L.orbx_debug_candidates(self._h, frame, level, None, 0))
        out = np.zeros((max(n, 1), 3), np.float32)
        self._check(self._L.orbx_debug_candidates(self._h, frame, level, _ptr(out), n))
        return out[:n]


def camera_from(K, distCoef) -> Tuple[float, ...]:
    """(fx, fy, cx, cy, k1, k2, p1, p2) from mK (3x3) and mDistCoef (4 entries), both float32 as in Settings.hpp:28-39."""
    K = np.asarray(K, np.float32).reshape(3, 3)
    d = np.asarray(distCoef, np.float32).reshape(-1)
    if d.size != 4:
        raise OrbxError(E_BADARG, "distCoef must hold k1 k2 p1 p2")
    return (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), float(d[0]), float(d[1]), float(d[2]), float(d[3]))


BOW_MAX_FEATURES = 16384  # ORBX_BOW_MAX_FEATURES: keypoints per frame of the bag-of-words calls
BowResult = collections.namedtuple("BowResult", "bow_word bow_value fv_node fv_feat feat_word")
BowResult.__doc__ = """One frame's transform: the BowVector as bow_word (uint32) / bow_value (float64) in ascending word order, the
FeatureVector as (fv_node, fv_feat) uint32 pairs in ascending order, and feat_word, each feature's word id (None if not asked)."""


class Vocabulary:
    """Features/ORBVocabulary.hpp -- DBoW2's TemplatedVocabulary<FORB> -- on the device of an ORBextractor's context: transform
    (BowVector, FeatureVector) and the L1 score (include/orbx.h, "bag of words", with its documented deviations).  The
    vocabulary keeps its extractor alive; close() it (or drop it) before the extractor."""

    TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
    L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5

    def __init__(self, extractor: ORBextractor, handle: ctypes.c_void_p):
        self._ext, self._L, self._h = extractor, extractor._L, handle
        info = np.zeros(6, np.int32)
        self._ext._check(self._L.orbx_vocabulary_info(self._h, _ptr(info)), "orbx_vocabulary_info")
        self.k, self.L, self.scoring, self.weighting, self.n_nodes, self.n_words = (int(v) for v in info)

    @staticmethod
    def parse_text(path: str):
        """The host parser of the text format (orbx_vocabulary_parse_text): (header [k, L, scoring, weighting], parent, is_leaf,
        desc [n, 32], weight) for nodes 1..n in file order."""
        L = lib()
        hdr, n = np.zeros(4, np.int32), ctypes.c_int32(0)
        r = L.orbx_vocabulary_parse_text(os.fsencode(path), _ptr(hdr), ctypes.byref(n), None, None, None, None, 0)
        if r < 0:
            raise OrbxError(r, "orbx_vocabulary_parse_text(%s)" % path)
        m = n.value
        parent, leaf = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32)
        desc, weight = np.zeros((max(m, 1), 32), np.uint8), np.zeros(max(m, 1), np.float64)
        r = L.orbx_vocabulary_parse_text(os.fsencode(path), _ptr(hdr), ctypes.byref(n), _ptr(parent), _ptr(leaf), _ptr(desc),
                                         _ptr(weight), len(parent))
        if r < 0:
            raise OrbxError(r, "orbx_vocabulary_parse_text(%s)" % path)
        return hdr, parent[:m], leaf[:m], desc[:m], weight[:m]

    @classmethod
    def from_text(cls, extractor: ORBextractor, path: str) -> "Vocabulary":
        """loadFromTextFile (saveToTextFile's format, ORB-SLAM's ORBvoc.txt)."""
        h = ctypes.c_void_p(0)
        extractor._check(extractor._L.orbx_vocabulary_load_text(extractor._h, os.fsencode(path), ctypes.byref(h)),
                         "orbx_vocabulary_load_text(%s)" % path)
        return cls(extractor, h)

    @classmethod
    def from_arrays(cls, extractor: ORBextractor, k: int, L: int, scoring: int, weighting: int, parent, is_leaf, desc,
                    weight) -> "Vocabulary":
        """Nodes 1..n in file order: parent [n] (node ids, root 0), is_leaf [n] (the file's flag), desc [n, 32], weight [n]."""
        parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
        n = len(parent)
        is_leaf = np.ascontiguousarray(is_leaf, np.int32).reshape(-1)
        desc = _desc(desc)
        weight = np.ascontiguousarray(weight, np.float64).reshape(-1)
        if len(is_leaf) != n or len(desc) != n or len(weight) != n:
            raise OrbxError(E_BADARG, "parent, is_leaf, desc and weight must describe the same nodes")
        h = ctypes.c_void_p(0)
        extractor._check(extractor._L.orbx_vocabulary_create(extractor._h, int(k), int(L), int(scoring), int(weighting), n, _ptr(parent),
                                                             _ptr(is_leaf), _ptr(desc), _ptr(weight), ctypes.byref(h)),
                         "orbx_vocabulary_create")
        return cls(extractor, h)

    TRAIN_STATS = ("nodes", "words", "kmeans_runs", "max_rounds_seen", "capped_runs", "emptied_clusters", "short_seedings",
                   "trivial_nodes")

    @classmethod
    def train(cls, extractor: ORBextractor, docs=None, k: int = 10, L: int = 6, weighting: int = 0, scoring: int = 0, seed: int = 0,
              max_rounds: int = 100, feat_word: bool = False, d_desc=None, d_n=None, n_docs: Optional[int] = None,
              capacity: Optional[int] = None, d_feat_word=None) -> "Vocabulary":
        """TemplatedVocabulary::create(training_features, k, L, weighting, scoring) on the device (orbx_vocabulary_train, with the
        deviations include/orbx.h lists: the draws are a function of `seed` and the node's path, an emptied cluster keeps its
        centre, a run stops after `max_rounds` rounds).  Either `docs`, a sequence of descriptor arrays [n_i, 32] in host memory
        (feat_word=True keeps each training feature's word in .train_feat_word, concatenated), or the device-resident layout of
        extract_batch_device: d_desc uint8 [n_docs, capacity, 32] and d_n int32 [n_docs] (device pointers or torch tensors), with
        d_feat_word uint32 [n_docs, capacity] optional.  The statistics are kept in .train_stats (a dict, TRAIN_STATS).
        Synchronous."""
        h, stats = ctypes.c_void_p(0), np.zeros(8, np.int32)
        fw = None
        if docs is not None:
            if d_desc is not None or d_n is not None:
                raise OrbxError(E_BADARG, "either docs or d_desc / d_n")
            arrs = [_desc(d) for d in docs]
            doc_n = np.array([len(a) for a in arrs], np.int32)
            cat = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros((0, 32), np.uint8))
            fw = np.zeros(max(len(cat), 1), np.uint32) if feat_word else None
            extractor._check(extractor._L.orbx_vocabulary_train(extractor._h, int(k), int(L), int(scoring), int(weighting), int(seed),
                                                                int(max_rounds), len(arrs), _ptr(cat) if len(cat) else None,
                                                                _ptr(doc_n) if len(arrs) else None, ctypes.byref(h), _ptr(stats),
                                                                _ptr(fw)), "orbx_vocabulary_train")
            fw = fw[:len(cat)] if feat_word else None
        else:
            if d_desc is None or d_n is None or n_docs is None:
                raise OrbxError(E_BADARG, "the device form needs d_desc, d_n and n_docs")
            cap, nd = int(capacity or extractor.capacity), int(n_docs)
            extractor._device_call("orbx_vocabulary_train_device", int(k), int(L), int(scoring), int(weighting), int(seed), int(max_rounds),
                                   nd, ("the descriptor array", d_desc, nd * cap * 32), ("the count array", d_n, nd * 4), cap,
                                   ctypes.byref(h), stats, ("the feature word array", d_feat_word, nd * cap * 4))
        v = cls(extractor, h)
        v.train_stats = dict(zip(cls.TRAIN_STATS, (int(x) for x in stats)))
        v.train_feat_word = fw
        return v

    def nodes(self):
        """(parent, is_leaf, desc [n, 32], weight) of nodes 1..n in file order (orbx_vocabulary_get_nodes), the layout from_arrays
        takes, for any vocabulary however it was made."""
        n = self.n_nodes
        m = max(n, 1)
        parent, leaf = np.zeros(m, np.int32), np.zeros(m, np.int32)
        desc, weight = np.zeros((m, 32), np.uint8), np.zeros(m, np.float64)
        r = self._L.orbx_vocabulary_get_nodes(self._h, _ptr(parent), _ptr(leaf), _ptr(desc), _ptr(weight), m)
        if r < 0:
            raise OrbxError(r, "orbx_vocabulary_get_nodes")
        return parent[:n], leaf[:n], desc[:n], weight[:n]

    def save_text(self, path: str, exact: bool = True) -> None:
        """saveToTextFile; exact=True writes the weights with 17 significant digits (a load returns the same bytes), exact=False
        as the reference's ostream does (6 significant digits)."""
        r = self._L.orbx_vocabulary_save_text(self._h, os.fsencode(path), 1 if exact else 0)
        if r < 0:
            raise OrbxError(r, "orbx_vocabulary_save_text(%s)" % path)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.orbx_vocabulary_destroy(self._h)
            self._h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transform(self, descriptors, levelsup: int = 4, feature_vector: bool = True, feat_word: bool = False) -> BowResult:
        """transform(features, BowVector&, FeatureVector&, levelsup) of one frame's descriptors [n, 32] from host memory
        (feature_vector=False: the two-argument transform, fv_* None).  Synchronous."""
        d = _desc(descriptors)
        n = len(d)
        m = max(n, 1)
        bw, bv, fn, ff, fw = np.zeros(m, np.uint32), np.zeros(m, np.float64), np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        bn, fvn = ctypes.c_int32(0), ctypes.c_int32(0)
        self._ext._check(self._L.orbx_bow_transform(self._ext._h, self._h, _ptr(d), n, int(levelsup), _ptr(bw), _ptr(bv), ctypes.byref(bn),
                                                    _ptr(fn) if feature_vector else None, _ptr(ff) if feature_vector else None,
                                                    ctypes.byref(fvn) if feature_vector else None, _ptr(fw) if feat_word else None),
                         "orbx_bow_transform")
        return BowResult(bw[:bn.value], bv[:bn.value], fn[:fvn.value] if feature_vector else None, ff[:fvn.value] if feature_vector else None,
                         fw[:n] if feat_word else None)

    def score(self, w1, v1, w2, v2) -> float:
        """L1Scoring::score of two BowVectors in host memory (ascending word arrays and their values).  Synchronous."""
        w1, w2 = np.ascontiguousarray(w1, np.uint32), np.ascontiguousarray(w2, np.uint32)
        v1, v2 = np.ascontiguousarray(v1, np.float64), np.ascontiguousarray(v2, np.float64)
        if len(w1) != len(v1) or len(w2) != len(v2):
            raise OrbxError(E_BADARG, "a BowVector's words and values differ in length")
        out = ctypes.c_double(0.0)
        self._ext._check(self._L.orbx_bow_score(self._ext._h, self._h, _ptr(w1), _ptr(v1), len(w1), _ptr(w2), _ptr(v2), len(w2),
                                                ctypes.byref(out)), "orbx_bow_score")
        return out.value

    def transform_batch_device(self, n_frames: int, d_desc, d_n, d_bow_word, d_bow_value, d_bow_n, d_fv_node=None, d_fv_feat=None,
                               d_fv_n=None, d_feat_word=None, levelsup: int = 4, capacity: Optional[int] = None) -> None:
        """Batched and device-resident (device pointers or torch tensors), the layout of extract_batch_device: d_desc uint8
        [n_frames, capacity, 32], d_n int32 [n_frames]; outputs d_bow_word uint32 / d_bow_value float64 / d_fv_node, d_fv_feat
        uint32 / d_feat_word uint32, all [n_frames, capacity], d_bow_n / d_fv_n int32 [n_frames]; d_fv_* (all three or none) and
        d_feat_word optional.  Stream-ordered on the context's stream: the outputs are valid after a device synchronisation."""
        cap, nf = int(capacity or self._ext.capacity), int(n_frames)
        if (d_fv_node is None) != (d_fv_feat is None) or (d_fv_node is None) != (d_fv_n is None):
            raise OrbxError(E_BADARG, "d_fv_node, d_fv_feat and d_fv_n go together")
        self._ext._device_call("orbx_bow_transform_batch_device", self._h, nf, ("the descriptor array", d_desc, nf * cap * 32),
                               ("the count array", d_n, nf * 4), cap, int(levelsup), ("the word array", d_bow_word, nf * cap * 4),
                               ("the value array", d_bow_value, nf * cap * 8), ("the BowVector count array", d_bow_n, nf * 4),
                               ("the FeatureVector node array", d_fv_node, nf * cap * 4),
                               ("the FeatureVector feature array", d_fv_feat, nf * cap * 4),
                               ("the FeatureVector count array", d_fv_n, nf * 4), ("the feature word array", d_feat_word, nf * cap * 4))

    def score_pairs_device(self, n_frames: int, first, second, d_bow_word, d_bow_value, d_bow_n, d_score,
                           capacity: Optional[int] = None) -> None:
        """L1Scoring::score of frame first[p] vs second[p] (host index arrays) of transform_batch_device's BowVectors (same
        capacity) into d_score float64 [n_pairs].  Stream-ordered like the transform."""
        first, second = _pair_lists(("first", "second"), (first, second))
        cap, nf, P = int(capacity or self._ext.capacity), int(n_frames), len(first)
        self._ext._device_call("orbx_bow_score_batch_device", self._h, nf, P, first, second, ("the word array", d_bow_word, nf * cap * 4),
                               ("the value array", d_bow_value, nf * cap * 8), ("the BowVector count array", d_bow_n, nf * 4), cap,
                               ("the score array", d_score, P * 8))


def debug_local_ba_lds_max_free(max_free: int = -1) -> None:
    """Measurement aid (orbx_debug_local_ba_lds_max_free): local bundle adjustments with at most max_free free keyframes keep the
    reduced system's factor in LDS; 0 = none does, -1 = the default (29).  Same results either way."""
    r = lib().orbx_debug_local_ba_lds_max_free(int(max_free))
    if r < 0:
        raise OrbxError(r, "orbx_debug_local_ba_lds_max_free")


DB_MAX_RESULTS = 256  # ORBX_DB_MAX_RESULTS: the longest result list of a database query
DB_ENTRIES_PER_SLICE, DB_LISTS_PER_MERGE = 2048, 8  # the defaults of orbx_debug_database_shape


def debug_database_shape(entries_per_slice: int = -1, lists_per_merge: int = -1) -> None:
    """Diagnostic (orbx_debug_database_shape): the entries one accumulate workgroup and the lists one merge workgroup of a
    database query take; negative values restore the defaults.  Every shape gives the same result."""
    r = lib().orbx_debug_database_shape(int(entries_per_slice), int(lists_per_merge))
    if r != 0:
        raise OrbxError(r, "orbx_debug_database_shape(%d, %d)" % (entries_per_slice, lists_per_merge))


class Database:
    """DBoW2's TemplatedDatabase on the device of a Vocabulary's context: the BowVectors of past frames in an inverted file, and
    the best-scoring entries for a new one (include/orbx.h, "database", with its documented deviations).  The scoring and
    weighting types are the vocabulary's; KL is not offered.  The database keeps its extractor alive; close() it (or drop it)
    before the extractor."""

    def __init__(self, vocabulary: Vocabulary):
        self._ext, self._L = vocabulary._ext, vocabulary._L
        self.n_words, self.scoring, self.weighting = vocabulary.n_words, vocabulary.scoring, vocabulary.weighting
        self._h = ctypes.c_void_p(0)
        self._ext._check(self._L.orbx_database_create(self._ext._h, vocabulary._h, ctypes.byref(self._h)), "orbx_database_create")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.orbx_database_destroy(self._h)
            self._h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self) -> int:
        """size(): the number of entries."""
        return self._ext._check(self._L.orbx_database_size(self._h), "orbx_database_size")

    def clear(self) -> None:
        """clear(): no entries; the next entry id is 0 again."""
        self._ext._check(self._L.orbx_database_clear(self._h), "orbx_database_clear")

    @staticmethod
    def _vector(word, value):
        w, v = np.ascontiguousarray(word, np.uint32).reshape(-1), np.ascontiguousarray(value, np.float64).reshape(-1)
        if len(w) != len(v):
            raise OrbxError(E_BADARG, "a BowVector's words and values differ in length")
        return w, v

    def add(self, word, value) -> int:
        """add(v) of one BowVector in host memory (ascending word ids and their values) -> its entry id.  Synchronous."""
        w, v = self._vector(word, value)
        eid = ctypes.c_int32(0)
        self._ext._check(self._L.orbx_database_add(self._ext._h, self._h, _ptr(w), _ptr(v), len(w), ctypes.byref(eid)),
                         "orbx_database_add")
        return eid.value

    def query(self, word, value, max_results: int = 1, max_id: int = -1):
        """query(vec, ret, max_results, max_id) of one BowVector in host memory -> (entry ids int32, scores float64), best first.
        max_results in [1, DB_MAX_RESULTS].  Synchronous."""
        w, v = self._vector(word, value)
        m = max(int(max_results), 1)
        e, s, n = np.zeros(m, np.int32), np.zeros(m, np.float64), ctypes.c_int32(0)
        self._ext._check(self._L.orbx_database_query(self._ext._h, self._h, _ptr(w), _ptr(v), len(w), int(max_results), int(max_id),
                                                     _ptr(e), _ptr(s), ctypes.byref(n)), "orbx_database_query")
        return e[:n.value], s[:n.value]

    def add_batch_device(self, n_frames: int, d_bow_word, d_bow_value, d_bow_n, capacity: Optional[int] = None) -> int:
        """add for a batch of BowVectors in the layout transform_batch_device writes (device pointers or torch tensors): d_bow_word
        uint32 / d_bow_value float64 [n_frames, capacity], d_bow_n int32 [n_frames] -> the first frame's entry id (frame f is
        entry first + f).  Stream-ordered on the context's stream."""
        cap, nf = int(capacity or self._ext.capacity), int(n_frames)
        first = ctypes.c_int32(0)
        self._ext._device_call("orbx_database_add_batch_device", self._h, nf, ("the word array", d_bow_word, nf * cap * 4),
                               ("the value array", d_bow_value, nf * cap * 8), ("the BowVector count array", d_bow_n, nf * 4), cap,
                               ctypes.byref(first))
        return first.value

    def query_batch_device(self, n_queries: int, d_bow_word, d_bow_value, d_bow_n, d_res_entry, d_res_score, d_res_n,
                           max_results: int = 1, max_id: int = -1, capacity: Optional[int] = None) -> None:
        """query for a batch of BowVectors (the layout of add_batch_device): d_res_entry int32 / d_res_score float64
        [n_queries, max_results] best first, d_res_n int32 [n_queries] the entries written for each query; nothing beyond them is
        written.  Stream-ordered on the context's stream: the results are valid after a device synchronisation."""
        cap, nq, m = int(capacity or self._ext.capacity), int(n_queries), max(int(max_results), 0)
        self._ext._device_call("orbx_database_query_batch_device", self._h, nq, ("the word array", d_bow_word, nq * cap * 4),
                               ("the value array", d_bow_value, nq * cap * 8), ("the BowVector count array", d_bow_n, nq * 4), cap,
                               int(max_results), int(max_id), ("the result entry array", d_res_entry, nq * m * 4),
                               ("the result score array", d_res_score, nq * m * 8), ("the result count array", d_res_n, nq * 4))

    def inverted_file(self):
        """Diagnostic readback (orbx_database_get_inverted_file): (row_start uint32 [words + 1], post_entry uint32, post_value
        float64), the postings word by word, each row in ascending entry id.  Synchronous."""
        n = self._ext._check(self._L.orbx_database_get_inverted_file(self._h, None, None, None, 0), "orbx_database_get_inverted_file")
        rs = np.zeros(self.n_words + 1, np.uint32)
        pe, pv = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64)
        self._ext._check(self._L.orbx_database_get_inverted_file(self._h, _ptr(rs), _ptr(pe), _ptr(pv), len(pe)),
                         "orbx_database_get_inverted_file")
        return rs, pe[:n], pv[:n]


class MapFuser:
    """ORBmatcher::Fuse, both overloads, on the device of an extractor's context (include/orbx.h, "fusing map points into a
    keyframe", with its documented deviations): MapFuser(extractor).  The keyframes and the map sets are the arrays of
    ORBextractor.match_scw_pairs_device; the fuser keeps its extractor alive."""

    def __init__(self, extractor: ORBextractor):
        self._ext, self._L = extractor, extractor._L

    def _pairs_device(self, fn, n_frames, kf, map_set, d_kps_un, d_desc, d_n, n_map_sets, map_capacity, d_map_n, d_map_points,
                      d_map_normals, d_map_dist, d_map_desc, d_map_mask, obs, d_pose, K, bounds, d_matches, d_occ_obs, d_fuse_idx,
                      d_fuse_act, d_fuse_other, d_res, th, th_low, capacity):
        cap, mcap, nf, ns = int(capacity or self._ext.capacity), int(map_capacity), int(n_frames), int(n_map_sets)
        kf, map_set = _pair_lists(("kf", "map_set"), (kf, map_set), nf, ns, "map set")
        P = len(kf)
        self._ext._device_call(fn, nf, P, kf, map_set, ("the keypoint array", d_kps_un, nf * cap * 28),
                               ("the descriptor array", d_desc, nf * cap * 32), ("the count array", d_n, nf * 4), cap, ns, mcap,
                               ("the map count array", d_map_n, ns * 4), ("the map point array", d_map_points, ns * mcap * 12),
                               ("the map normal array", d_map_normals, ns * mcap * 12), ("the map distance array", d_map_dist, ns * mcap * 8),
                               ("the map descriptor array", d_map_desc, ns * mcap * 32), ("the map mask", d_map_mask, ns * mcap), *obs,
                               d_pose + (P * 48,), _k9(K), ctypes.byref(_bounds(bounds)), float(th), int(th_low),
                               ("matches", d_matches, P * cap * 4), ("the occupants' observation counts", d_occ_obs, P * cap * 4),
                               ("the picked-feature array", d_fuse_idx, P * mcap * 4), ("the action array", d_fuse_act, P * mcap),
                               ("the occupant array", d_fuse_other, P * mcap * 4),
                               ("the result array", d_res, P * FUSE_RESULT_DTYPE.itemsize))

    def fuse_pairs_device(self, n_frames: int, kf, map_set, d_kps_un, d_desc, d_n, n_map_sets: int, map_capacity: int, d_map_n,
                          d_map_points, d_map_normals, d_map_dist, d_map_desc, d_map_mask, d_map_obs, d_pose, K,
                          bounds: Tuple[int, int, int, int], d_matches, d_occ_obs, d_fuse_idx, d_fuse_act, d_fuse_other, d_res,
                          th: float = 3.0, th_low: int = 50, capacity: Optional[int] = None) -> None:
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) of LocalMapping::SearchInNeighbors for pairs (keyframe kf[p], map set
        map_set[p]; host index arrays).  d_map_obs int32 [n_map_sets, map_capacity]: Observations(); d_pose float32 [n_pairs, 12]
        (Rcw row-major, then tcw).  d_matches int32 [n_pairs, capacity] is read and written: mvpMapPoints as indices into the
        pair's set, FUSE_OCCUPIED_UNMAPPED, or another negative value (free); d_occ_obs int32 [n_pairs, capacity] or None: the
        unmapped occupants' Observations(), negative = isBad().  Per map point: d_fuse_idx int32 / d_fuse_act uint8 /
        d_fuse_other int32 [n_pairs, map_capacity]; d_res [n_pairs] FUSE_RESULT_DTYPE records (64 bytes).  Stream-ordered on the
        context's stream."""
        self._pairs_device("orbx_fuse_batch_device", n_frames, kf, map_set, d_kps_un, d_desc, d_n, n_map_sets, map_capacity, d_map_n,
                           d_map_points, d_map_normals, d_map_dist, d_map_desc, d_map_mask,
                           [("the map observation array", d_map_obs, int(n_map_sets) * int(map_capacity) * 4)],
                           ("the pose array", d_pose), K, bounds, d_matches, d_occ_obs, d_fuse_idx,
                           d_fuse_act, d_fuse_other, d_res, th, th_low, capacity)

    def fuse_scw_pairs_device(self, n_frames: int, kf, map_set, d_kps_un, d_desc, d_n, n_map_sets: int, map_capacity: int, d_map_n,
                              d_map_points, d_map_normals, d_map_dist, d_map_desc, d_map_mask, d_scw, K,
                              bounds: Tuple[int, int, int, int], d_matches, d_occ_obs, d_fuse_idx, d_fuse_act, d_fuse_other, d_res,
                              th: float = 4.0, th_low: int = 50, capacity: Optional[int] = None) -> None:
        """ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) of LoopClosing::SearchAndFuse for pairs: as
        fuse_pairs_device with d_scw float32 [n_pairs, 12] (what sim3_compose_scw_pairs_device writes) in place of the pose and
        without observation counts; d_occ_obs is read for its sign only.  d_fuse_other is vpReplacePoint."""
        self._pairs_device("orbx_fuse_scw_batch_device", n_frames, kf, map_set, d_kps_un, d_desc, d_n, n_map_sets, map_capacity, d_map_n,
                           d_map_points, d_map_normals, d_map_dist, d_map_desc, d_map_mask, [],
                           ("the Scw array", d_scw), K, bounds, d_matches, d_occ_obs, d_fuse_idx,
                           d_fuse_act, d_fuse_other, d_res, th, th_low, capacity)

    def fuse_local_ba_device(self, create: dict, fuse: dict, local_ba: dict) -> None:
        """LocalMapping's chain behind a new keyframe, queued on the context's stream with no copy and no wait in between:
        ORBextractor.create_new_map_points_pairs_device(**create), fuse_pairs_device(**fuse), then
        ORBextractor.local_ba_problems_device(**local_ba).  The dictionaries hold the three calls' own arguments by name; the
        chain is in what they share: the point arrays `create` writes are map sets of `fuse` (map_capacity = capacity), and
        `fuse`'s d_matches is `local_ba`'s d_rows with the fuse pairs as the entry list (entry_frame = kf), each problem a run of
        pairs that name one map set."""
        self._ext.create_new_map_points_pairs_device(**create)
        self.fuse_pairs_device(**fuse)
        self._ext.local_ba_problems_device(**local_ba)

    def fuse_local_ba_update_device(self, create: dict, fuse: dict, local_ba: dict, update: dict) -> None:
        """fuse_local_ba_device(create, fuse, local_ba), then ORBextractor.map_update_problems_device(**update) on the same
        stream, again with no copy and no wait: `update` names `local_ba`'s problems, its d_pose_out as d_entry_pose, its
        d_obs_outlier and d_rows, and as outputs the arrays the next match_local_map_pairs_device reads (`fuse`'s d_map_normals,
        d_map_dist, d_map_desc, d_map_obs; d_map_mask in place or a d_map_mask_out)."""
        self.fuse_local_ba_device(create, fuse, local_ba)
        self._ext.map_update_problems_device(**update)

    def _one(self, scw_form, keys_un, desc, map_points, map_normals, map_dist, map_desc, map_mask, map_obs, T, K, bounds, matches,
             occ_obs, th, th_low):
        k = _keys(keys_un)
        d = _desc(desc)
        mp = _points(map_points)
        mn = _points(map_normals)
        md = _points(map_dist, 2)
        mdesc = _desc(map_desc)
        if len(k) != len(d) or not (len(mp) == len(mn) == len(md) == len(mdesc)):
            raise OrbxError(E_BADARG, "keypoints / descriptors or the map arrays differ in length")
        mm = _flags(map_mask, len(mp), "the map mask needs one entry per map point")
        m = _row(matches, len(k), "matches needs one entry per feature")
        occ = None if occ_obs is None else _row(occ_obs, len(k), "occ_obs needs one entry per feature")
        nm = max(len(mp), 1)
        idx, act, other = np.full(nm, -1, np.int32), np.zeros(nm, np.uint8), np.full(nm, -1, np.int32)
        S, Kf, b, res = _pose12(T), _k9(K), _bounds(bounds), FuseResult()
        head = (self._ext._h, _ptr(k), _ptr(d), len(k), len(mp), _ptr(mp), _ptr(mn), _ptr(md), _ptr(mdesc), _ptr(mm))
        tail = (_ptr(S), _ptr(Kf), ctypes.byref(b), float(th), int(th_low), _ptr(m), _ptr(occ), _ptr(idx), _ptr(act), _ptr(other),
                ctypes.byref(res))
        if scw_form:
            r, fn = self._L.orbx_fuse_scw(*head, *tail), "orbx_fuse_scw"
        else:
            if map_obs is None:
                raise OrbxError(E_BADARG, "MapFuser.fuse needs map_obs, the Observations() of every map point")
            obs = _row(map_obs, len(mp), "map_obs needs one entry per map point")
            r, fn = self._L.orbx_fuse(*head, _ptr(obs), *tail), "orbx_fuse"
        self._ext._check(r, fn)
        return m[:len(k)].copy(), idx[:len(mp)].copy(), act[:len(mp)].copy(), other[:len(mp)].copy(), res

    def fuse(self, keys_un, desc, map_points, map_normals, map_dist, map_desc, map_mask, map_obs, Tcw, K,
             bounds: Tuple[int, int, int, int], matches=None, occ_obs=None, th: float = 3.0, th_low: int = 50):
        """One keyframe and one map set in host memory (orbx_fuse) -> (row int32 [len(keys_un)], idx, act, other [n points],
        FuseResult).  Tcw: 12 floats (Rcw row-major, then tcw) or a 3x4 / 4x4 matrix; matches (default all -1): mvpMapPoints as
        indices into the map arrays.  Synchronous."""
        return self._one(False, keys_un, desc, map_points, map_normals, map_dist, map_desc, map_mask, map_obs, Tcw, K, bounds, matches,
                         occ_obs, th, th_low)

    def fuse_scw(self, keys_un, desc, map_points, map_normals, map_dist, map_desc, map_mask, Scw, K,
                 bounds: Tuple[int, int, int, int], matches=None, occ_obs=None, th: float = 4.0, th_low: int = 50):
        """The Scw form for one keyframe and one map set in host memory (orbx_fuse_scw) -> (row, idx, act, other, FuseResult);
        other is vpReplacePoint.  Synchronous."""
        return self._one(True, keys_un, desc, map_points, map_normals, map_dist, map_desc, map_mask, None, Scw, K, bounds, matches,
                         occ_obs, th, th_low)


class Frame:
    """The slice of SlamTypes/Frame.{hpp,cpp} on this path: runs the extractor (Frame.cpp:58-60), undistorts the
    keypoints (Frame.cpp:136-161) and keeps mvKeys / mvKeysUn / mDescriptors / N and the image bounds
    (Frame.cpp:101-134).  K / distCoef = None means no distortion (mvKeysUn = mvKeys, bounds = the image).  voc
    (mpORBvocabulary) is what ComputeBoW transforms with."""

    def __init__(self, im: np.ndarray, timestamp: float, extractor: ORBextractor, K=None, distCoef=None, voc: Optional[Vocabulary] = None):
        self.mTimestamp = timestamp
        self.mpORBextractor = extractor
        self.mpORBvocabulary = voc
        self.mBowVec, self.mFeatVec = {}, {}
        h, w = im.shape
        self.camera = camera_from(K, distCoef) if K is not None and distCoef is not None else None
        if self.camera is not None:
            self.bounds = extractor.image_bounds(self.camera, w, h)  # Frame.cpp:44
        else:
            self.bounds = (0, w, 0, h)  # mnMinX, mnMaxX, mnMinY, mnMaxY (Frame.cpp:127-131)
        self._image = im  # (ComputeStereoMatches correlates on the images)
        _, self.mvKeys, self.mDescriptors = extractor(im, None, (0, 0))
        if self.camera is not None and len(self.mvKeys):
            self.mvKeysUn = extractor.undistort_keypoints(self.mvKeys, self.camera)  # Frame.cpp:64
        else:
            self.mvKeysUn = self.mvKeys  # Frame.cpp:137-140
        self.N = len(self.mvKeysUn)

    @classmethod
    def from_arrays(cls, keys: np.ndarray, descriptors: np.ndarray, bounds: Tuple[int, int, int, int],
                    voc: Optional[Vocabulary] = None) -> "Frame":
        f = cls.__new__(cls)
        f.mTimestamp, f.mpORBextractor = 0.0, None
        f.mpORBvocabulary, f.mBowVec, f.mFeatVec = voc, {}, {}
        f.mvKeys = f.mvKeysUn = _keys(keys)
        f.mDescriptors = _desc(descriptors)
        f.N = len(f.mvKeysUn)
        f.bounds = tuple(int(v) for v in bounds)
        return f

    def ComputeStereoMatches(self, right_frame: "Frame", bf: float, b: float):
        """Frame::ComputeStereoMatches against the right image's frame (include/orbx.h, "stereo: matching left and right"): sets
        mvuRight / mvDepth (float32 [N], -1 = no match), mbf and mb, and returns the StereoResult.  Both frames must come from
        images of one size; they are extracted again as a batch of two, which is what leaves their pyramids side by side on the
        device (the keypoints are the same bytes)."""
        ext = self.mpORBextractor or right_frame.mpORBextractor
        if ext is None or getattr(self, "_image", None) is None or getattr(right_frame, "_image", None) is None:
            raise OrbxError(E_BADARG, "Frame.ComputeStereoMatches needs two frames made from images (Frame(im, ...))")
        (kl, _), _, self.mvuRight, self.mvDepth, res = ext.extract_stereo(self._image, right_frame._image, bf, b)
        if kl.tobytes() != _keys(self.mvKeys).tobytes():
            raise OrbxError(E_BADARG, "Frame.ComputeStereoMatches: the frame's keypoints are not its image's")
        self.mbf, self.mb = float(bf), float(b)
        return res

    def UnprojectStereo(self, i: int, Twc=None):
        """Frame::UnprojectStereo: the 3-D point of feature i from mvDepth (float32 [3]; in camera coordinates unless Twc, 12
        floats or a 3x4 / 4x4 matrix, is given), or None where the feature has no depth.  The arithmetic is rule 13's."""
        z = np.float32(self.mvDepth[i])
        if not z > 0:
            return None
        cam = self.camera if self.camera is not None else getattr(self, "stereo_camera", None)
        if cam is None:
            raise OrbxError(E_BADARG, "Frame.UnprojectStereo needs a camera (Frame(..., K=, distCoef=) or frame.stereo_camera = (fx, fy, cx, cy))")
        f32 = np.float32
        fx, fy, cx, cy = (f32(v) for v in cam[:4])
        u, v = f32(self.mvKeysUn["x"][i]), f32(self.mvKeysUn["y"][i])
        x, y = f32(f32(f32(u - cx) * z) * f32(f32(1) / fx)), f32(f32(f32(v - cy) * z) * f32(f32(1) / fy))
        if Twc is None:
            return np.array([x, y, z], f32)
        T = _pose12(Twc)
        return np.array([f32(f32(f32(f32(T[3 * k] * x) + f32(T[3 * k + 1] * y)) + f32(T[3 * k + 2] * z)) + T[9 + k]) for k in range(3)], f32)

    def ComputeBoW(self, levelsup: int = 4) -> None:
        """Frame::ComputeBoW: once, mBowVec {word id: value} and mFeatVec {node id: [feature indices]}, both in ascending key
        order, from mDescriptors with mpORBvocabulary (transform(..., mBowVec, mFeatVec, 4))."""
        if self.mBowVec:
            return
        if self.mpORBvocabulary is None:
            raise OrbxError(E_BADARG, "Frame.ComputeBoW needs a vocabulary (Frame(..., voc=))")
        r = self.mpORBvocabulary.transform(self.mDescriptors, levelsup)
        self.mBowVec = {int(w): float(v) for w, v in zip(r.bow_word, r.bow_value)}
        fv = {}
        for node, feat in zip(r.fv_node.tolist(), r.fv_feat.tolist()):
            fv.setdefault(node, []).append(feat)
        self.mFeatVec = fv
        self._bow_computed = True  # (both vectors may be empty: ORBmatcher.SearchByBoW asks whether this has run)


def _flat_feature_vector(fv):
    """mFeatVec {node id: [feature indices]} as the two parallel uint32 arrays of the C ABI, in ascending node order."""
    node = [n for n in sorted(fv) for _ in fv[n]]
    feat = [j for n in sorted(fv) for j in fv[n]]
    return np.asarray(node, np.uint32), np.asarray(feat, np.uint32)


class ORBmatcher:
    """Features/ORBmatcher.hpp:13-61."""

    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio: float = 0.6, checkOri: bool = True, extractor: Optional[ORBextractor] = None):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        self._ext = extractor
        self.last_stats = None

    def _extractor(self, *frames) -> ORBextractor:
        ext = self._ext or next((f.mpORBextractor for f in frames if f.mpORBextractor is not None), None)
        if ext is None:
            raise OrbxError(E_BADARG, "ORBmatcher needs an ORBextractor (device context); pass extractor=")
        return ext

    def SearchForInitialization(self, F1: Frame, F2: Frame, windowSize: int = 100):
        """Returns (nmatches, vnMatches12).  nmatches keeps the reference's double-decrement quirk (cpp:95-98,130-138)."""
        ext = self._extractor(F1, F2)
        k1 = _keys(F1.mvKeysUn)
        k2 = _keys(F2.mvKeysUn)
        d1 = np.ascontiguousarray(F1.mDescriptors, np.uint8)
        d2 = np.ascontiguousarray(F2.mDescriptors, np.uint8)
        m12 = np.full(max(len(k1), 1), -1, np.int32)
        st = _Stats()
        b = _bounds(F2.bounds)
        nm = ctypes.c_int32(0)
        r = ext._L.orbx_match_init(ext._h, _ptr(k1), _ptr(d1), len(k1), _ptr(k2), _ptr(d2), len(k2), ctypes.byref(b),
                                   int(windowSize), self.mfNNratio, int(self.mbCheckOrientation), _ptr(m12), ctypes.byref(nm),
                                   ctypes.byref(st))
        ext._check(r, "orbx_match_init")
        self.last_stats = (st.invalid_by_distance, st.invalid_by_ratio, st.invalid_by_orientation)
        return int(nm.value), m12[:len(k1)].copy()

    def SearchByBoW(self, KF: Frame, F: Frame, mask=None):
        """ORB-SLAM2's SearchByBoW(KeyFrame*, Frame&, ...) over the frames' mFeatVec (include/orbx.h, "matching through the
        FeatureVector") -> (matches_f, nmatches): matches_f[j] = the KF feature matched to F's feature j, or -1.  mask
        (optional): one entry per KF feature, false = it has no map point.  Both frames' ComputeBoW must have run."""
        ext = self._extractor(KF, F)
        for name, fr in (("KF", KF), ("F", F)):
            if not (getattr(fr, "_bow_computed", False) or fr.mBowVec or fr.mFeatVec):
                raise OrbxError(E_BADARG, "ORBmatcher.SearchByBoW: %s has no FeatureVector; call its ComputeBoW() first" % name)
        kn, kf = _flat_feature_vector(KF.mFeatVec)
        fn, ff = _flat_feature_vector(F.mFeatVec)
        return ext.match_bow(KF.mvKeysUn, KF.mDescriptors, kn, kf, F.mvKeysUn, F.mDescriptors, fn, ff, mask, self.mfNNratio,
                             self.mbCheckOrientation)

    def SearchForTriangulation(self, KF1: Frame, KF2: Frame, Tcw1, Tcw2, K=None, mask1=None, mask2=None, median_depth2: float = 0.0):
        """ORB-SLAM2's SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo=False) over the keyframes' mFeatVec
        (include/orbx.h, "growing the map") -> (nmatches, vMatchedPairs, TriMatchResult): vMatchedPairs int32 [nmatches, 2] =
        (KF1 feature, KF2 feature) in ascending KF1 index, as ORB-SLAM2 builds it.  F12 is computed from the two poses Tcw (3x4 or
        4x4) and K (3x3, default KF1's camera); mask1 / mask2 (optional): true = the feature already has a map point.  Both
        keyframes' ComputeBoW must have run."""
        ext = self._extractor(KF1, KF2)
        for name, fr in (("KF1", KF1), ("KF2", KF2)):
            if not (getattr(fr, "_bow_computed", False) or fr.mBowVec or fr.mFeatVec):
                raise OrbxError(E_BADARG, "ORBmatcher.SearchForTriangulation: %s has no FeatureVector; call its ComputeBoW() first" % name)
        K = _camera_K(K, KF1, "ORBmatcher.SearchForTriangulation", "keyframe")
        n1, f1 = _flat_feature_vector(KF1.mFeatVec)
        n2, f2 = _flat_feature_vector(KF2.mFeatVec)
        m12, res = ext.match_triangulation(KF1.mvKeysUn, KF1.mDescriptors, n1, f1, Tcw1, KF2.mvKeysUn, KF2.mDescriptors, n2, f2, Tcw2, K,
                                           mask1, mask2, median_depth2, self.mbCheckOrientation)
        i = np.flatnonzero(m12 >= 0)
        return int(res.nmatches), np.stack([i, m12[i]], axis=1).astype(np.int32), res

    def SearchByProjection(self, CurrentFrame: Frame, LastFrame: Frame, th: float, points, mask, Tcw, K=None, point_desc=None,
                           last_outlier=None):
        """ORB-SLAM2's SearchByProjection(CurrentFrame, LastFrame, th, bMono=True) (include/orbx.h, "matching by projection") ->
        (nmatches, matches_cur, ProjResult): matches_cur[j] = the LastFrame feature whose map point CurrentFrame's feature j
        got, or -1.  points [N_last, 3] / mask [N_last]: LastFrame's map points (mvpMapPoints); Tcw (3x4 or 4x4):
        CurrentFrame's predicted pose; K: 3x3, default CurrentFrame's camera; point_desc (optional): the map points' own
        descriptors; last_outlier (optional): LastFrame.mvbOutlier."""
        ext = self._extractor(CurrentFrame, LastFrame)
        K = _camera_K(K, CurrentFrame, "ORBmatcher.SearchByProjection", "frame")
        m, res = ext.match_projection(LastFrame.mvKeysUn, LastFrame.mDescriptors, CurrentFrame.mvKeysUn, CurrentFrame.mDescriptors,
                                      points, mask, Tcw, K, CurrentFrame.bounds, th, self.mbCheckOrientation, point_desc, last_outlier)
        return int(res.nmatches), m, res


    def SearchLocalPoints(self, F: Frame, map_points, map_normals, map_dist, map_desc, map_mask, Tcw, th: float = 1.0, K=None,
                          matches=None, outlier=None):
        """Tracking::SearchLocalPoints on a frame and the local map as arrays (include/orbx.h, "matching the local map by
        projection"): isInFrustum, PredictScale and ORB-SLAM2's SearchByProjection(F, vpMapPoints, th) with this matcher's
        nnratio -> (nmatches, matches, point_view, LocalResult).  matches (optional): the map points F already has, as indices
        into the map arrays (F.mvpMapPoints); outlier (optional): F.mvbOutlier; K: 3x3, default F's camera."""
        ext = self._extractor(F)
        K = _camera_K(K, F, "ORBmatcher.SearchLocalPoints", "frame")
        m, view, res = ext.match_local_map(F.mvKeysUn, F.mDescriptors, map_points, map_normals, map_dist, map_desc, map_mask, Tcw, K,
                                           F.bounds, matches, th, self.mfNNratio, outlier)
        return int(res.nmatches), m, view, res

    def SearchByProjectionScw(self, KF: Frame, Scw, map_points, map_normals, map_dist, map_desc, map_mask, matched=None,
                              th: float = 10.0, K=None, th_low: int = 50, kf2_to_map=None):
        """ORB-SLAM2's loop-closing overload SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (include/orbx.h, "loop closing:
        matching the loop's points under Scw") -> (nmatches, matched, MatchScwResult).  Scw: 12 floats (sR row-major, then t) or
        a 3x4 / 4x4 matrix; the map arrays are SearchLocalPoints'; matched (optional): vpMatched as indices into the map arrays
        (with kf2_to_map: as the matched keyframe's feature indices); K: 3x3, default KF's camera."""
        ext = self._extractor(KF)
        K = _camera_K(K, KF, "ORBmatcher.SearchByProjectionScw", "keyframe")
        m, res = ext.match_scw(KF.mvKeysUn, KF.mDescriptors, map_points, map_normals, map_dist, map_desc, map_mask, Scw, K, KF.bounds,
                               matched, th, th_low, kf2_to_map)
        return int(res.nmatches), m, res

    def Fuse(self, KF: Frame, map_points, map_normals, map_dist, map_desc, map_mask, map_obs, Tcw, th: float = 3.0, K=None,
             matches=None, occ_obs=None, th_low: int = 50):
        """ORB-SLAM2's Fuse(pKF, vpMapPoints, th) (include/orbx.h, "fusing map points into a keyframe") -> (nFused, row, idx, act,
        other, FuseResult).  The map arrays are SearchLocalPoints' plus map_obs, the points' Observations(); Tcw: KF's pose;
        matches (optional): KF's mvpMapPoints as indices into the map arrays (FUSE_OCCUPIED_UNMAPPED: a point that is not among
        them, with its Observations() in occ_obs); K: 3x3, default KF's camera.  The caller applies the decisions (Replace,
        AddObservation) from idx / act / other."""
        ext = self._extractor(KF)
        K = _camera_K(K, KF, "ORBmatcher.Fuse", "keyframe")
        row, idx, act, other, res = MapFuser(ext).fuse(KF.mvKeysUn, KF.mDescriptors, map_points, map_normals, map_dist, map_desc, map_mask,
                                                       map_obs, Tcw, K, KF.bounds, matches, occ_obs, th, th_low)
        return int(res.n_fused), row, idx, act, other, res

    def FuseScw(self, KF: Frame, Scw, map_points, map_normals, map_dist, map_desc, map_mask, th: float = 4.0, K=None, matches=None,
                occ_obs=None, th_low: int = 50):
        """ORB-SLAM2's Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) of LoopClosing::SearchAndFuse -> (nFused, row, idx, act,
        vpReplacePoint, FuseResult): vpReplacePoint[i] is the point of KF that map point i is to replace, or -1."""
        ext = self._extractor(KF)
        K = _camera_K(K, KF, "ORBmatcher.FuseScw", "keyframe")
        row, idx, act, other, res = MapFuser(ext).fuse_scw(KF.mvKeysUn, KF.mDescriptors, map_points, map_normals, map_dist, map_desc,
                                                           map_mask, Scw, K, KF.bounds, matches, occ_obs, th, th_low)
        return int(res.n_fused), row, idx, act, other, res

    def SearchByProjectionKeyFrame(self, CurrentFrame: Frame, KF: Frame, points, mask, point_dist, Tcw, th: float = 10.0, ORBdist: int = 100,
                                   K=None, matches=None, outlier=None, point_desc=None):
        """ORB-SLAM2's relocalisation overload SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (include/orbx.h,
        "matching a keyframe's points by projection") -> (nmatches, matches, KfProjResult).  points [N_kf, 3] / mask [N_kf] /
        point_dist [N_kf, 2]: the keyframe's map points (GetMapPointMatches, mfMinDistance and mfMaxDistance); Tcw (3x4 or 4x4):
        CurrentFrame's pose; matches (optional): the points CurrentFrame already has (mvpMapPoints = sAlreadyFound), as indices
        into the keyframe's features; outlier (optional): CurrentFrame.mvbOutlier; point_desc (optional): the map points' own
        descriptors; K: 3x3, default CurrentFrame's camera."""
        ext = self._extractor(CurrentFrame, KF)
        K = _camera_K(K, CurrentFrame, "ORBmatcher.SearchByProjectionKeyFrame", "frame")
        m, res = ext.match_keyframe_projection(KF.mvKeysUn, KF.mDescriptors, CurrentFrame.mvKeysUn, CurrentFrame.mDescriptors, points, mask,
                                               point_dist, Tcw, K, CurrentFrame.bounds, matches, th, ORBdist, self.mbCheckOrientation,
                                               point_desc, outlier)
        return int(res.nmatches), m, res


    def SearchBySim3(self, KF1: Frame, KF2: Frame, map1, map2, matches12, s12: float, R12, t12, th: float = 7.5, K=None,
                     bounds=None, ORBdist: int = 100):
        """ORB-SLAM2's SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (include/orbx.h, "loop closing: matching under a
        similarity") -> (nFound, matches12, MatchSim3Result).  map1 / map2: (points [N, 3], mask [N] or None, point_dist [N, 2],
        Tcw, point_desc [N, 32] or None) of each keyframe; matches12 int32 [N1]: KF2's feature per feature of KF1, or -1."""
        ext = self._extractor(KF1, KF2)
        K = _camera_K(K, KF1, "ORBmatcher.SearchBySim3", "keyframe")
        (p1, m1, q1, T1, pd1), (p2, m2, q2, T2, pd2) = map1, map2
        sim = np.r_[np.asarray(R12, np.float32).reshape(9), np.asarray(t12, np.float32).reshape(3), np.float32(s12)].astype(np.float32)
        m, res = ext.match_sim3(KF1.mvKeysUn, KF1.mDescriptors, p1, m1, q1, T1, KF2.mvKeysUn, KF2.mDescriptors, p2, m2, q2, T2, sim, K,
                                bounds if bounds is not None else KF1.bounds, matches12, th, ORBdist, pd1, pd2)
        return int(res.n_found), m, res


class PnPsolver:
    """ORB-SLAM2's PnPsolver for one frame and one candidate's map points (include/orbx.h, "behind SearchByBoW: PnP RANSAC"):
    PnPsolver(frame, points, mask_or_match, K), SetRansacParameters, then iterate(nIterations) or find().  mask_or_match: bool /
    uint8 [N] = feature j has the point points[j], or int32 [N] = feature j's point is points[match[j]] (-1: none), the row
    SearchByBoW returns.  The device runs a solver's whole life in one call (deviation 6): the first iterate() or find() runs
    every iteration on `rand`'s draws, and iterate(n) answers as the reference's n-at-a-time turns would."""

    def __init__(self, frame: Frame, points, mask_or_match, K=None, extractor: Optional[ORBextractor] = None, rand=None):
        self._ext = extractor or frame.mpORBextractor
        if self._ext is None:
            raise OrbxError(E_BADARG, "PnPsolver needs an ORBextractor (device context); pass extractor=")
        K = _camera_K(K, frame, "PnPsolver", "frame")
        self._K = np.ascontiguousarray(K, np.float32).reshape(3, 3)
        self._keys = _keys(frame.mvKeysUn)
        n = len(self._keys)
        pts = _points(points)
        mm = np.asarray(mask_or_match).reshape(-1)
        if len(mm) != n:
            raise OrbxError(E_BADARG, "mask_or_match must have one entry per keypoint of the frame")
        if mm.dtype.kind in "iu" and mm.dtype.itemsize >= 4:  # a match row: gather the points feature by feature
            ok = (mm >= 0) & (mm < len(pts))
            self._points = np.zeros((n, 3), np.float32)
            self._points[ok] = pts[mm[ok]]
            self._mask = ok.astype(np.uint8)
        else:
            if len(pts) != n:
                raise OrbxError(E_BADARG, "points must have one entry per keypoint of the frame")
            self._points, self._mask = pts, (mm != 0).astype(np.uint8)
        self._rand = rand or _libc_rand()
        self._params = dict(probability=0.99, min_inliers=8, max_iterations=300, epsilon=0.4, th2=5.991)  # the constructor's own
        self._turns = 0
        self._result = None

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 8, maxIterations: int = 300, minSet: int = 4,
                            epsilon: float = 0.4, th2: float = 5.991) -> None:
        if int(minSet) != 4:
            raise OrbxError(E_BADARG, "PnPsolver: minSet is 4 (EPnP's minimal set)")
        self._params = dict(probability=probability, min_inliers=minInliers, max_iterations=maxIterations, epsilon=epsilon, th2=th2)
        self._result, self._turns = None, 0

    def _run(self):
        if self._result is None:
            draws = sample_pnp_draws(self._rand, int(self._params["max_iterations"]))
            self._result = self._ext.pnp_solve(self._keys, self._points, self._mask, self._K, draws, **self._params)
        return self._result

    def _answer(self):
        res, inl = self._run()
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = np.array(res.Tcw[:9], np.float32).reshape(3, 3), np.array(res.Tcw[9:], np.float32)
        return T, inl, int(res.n_inliers)

    def iterate(self, nIterations: int):
        """-> (Tcw 4x4 float32 or None, bNoMore, vbInliers [N] bool, nInliers, the PnpResult): what the reference's iterate
        returns in this turn of nIterations iterations."""
        res, _ = self._run()
        self._turns += 1
        done = self._turns * int(nIterations)
        none = np.zeros(len(self._keys), bool)
        if res.status & PNP_FEW_POINTS or res.status & (PNP_BAD_INPUT | PNP_NONFINITE):
            return None, True, none, 0, res
        if res.refined and res.found_it < done:
            T, inl, n = self._answer()
            return T, False, inl, n, res
        if done >= res.its_run and not res.refined:
            if res.status & PNP_NO_POSE:
                return None, True, none, 0, res
            T, inl, n = self._answer()
            return T, True, inl, n, res
        return None, False, none, 0, res

    def find(self):
        """-> (Tcw 4x4 float32 or None, vbInliers [N] bool, nInliers, the PnpResult): iterate until a pose or bNoMore."""
        res, _ = self._run()
        if res.status & PNP_NO_POSE:
            return None, np.zeros(len(self._keys), bool), 0, res
        T, inl, n = self._answer()
        return T, inl, n, res


class Sim3Solver:
    """ORB-SLAM2's Sim3Solver for one keyframe pair (include/orbx.h, "loop closing: Sim3 RANSAC"), in the shape of PnPsolver:
    Sim3Solver(kf1, kf2, match12, K, bFixScale), SetRansacParameters, then iterate(nIterations) or find().  kf1 / kf2: (mvKeysUn,
    points [n, 3], mask [n] or None, Tcw 3x4 / 4x4 / 12 floats) of the current keyframe and of the candidate; match12 int32 [n1]:
    KF2's feature matched to KF1's, or -1 (vpMatched12 with GetIndexInKeyFrame taken as the identity).  The device runs a
    solver's whole life in one call: the first iterate() or find() runs every iteration on `rand`'s draws, and iterate(n) answers
    as the reference's n-at-a-time turns would."""

    def __init__(self, kf1, kf2, match12, K, bFixScale: bool = False, extractor: Optional[ORBextractor] = None, rand=None):
        if extractor is None:
            raise OrbxError(E_BADARG, "Sim3Solver needs an ORBextractor (device context); pass extractor=")
        self._ext, self._kf1, self._kf2 = extractor, tuple(kf1), tuple(kf2)
        self._match = np.ascontiguousarray(match12, np.int32).reshape(-1)
        self._K = np.ascontiguousarray(K, np.float32).reshape(3, 3)
        self._fix = bool(bFixScale)
        self._rand = rand or _libc_rand()
        self._params = dict(probability=0.99, min_inliers=6, max_iterations=300, th2=9.210)  # the constructor's own
        self._turns = 0
        self._result = None

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 6, maxIterations: int = 300) -> None:
        self._params = dict(self._params, probability=probability, min_inliers=minInliers, max_iterations=maxIterations)
        self._result, self._turns = None, 0

    def _run(self):
        if self._result is None:
            draws = sample_sim3_draws(self._rand, int(self._params["max_iterations"]))
            (k1, p1, m1, T1), (k2, p2, m2, T2) = self._kf1, self._kf2
            self._result = self._ext.sim3_solve(k1, p1, m1, _pose12(T1), k2, p2, m2, _pose12(T2), self._match, self._K,
                                                draws, fix_scale=self._fix, **self._params)
        return self._result

    def _answer(self):
        res, sim, _, inl = self._run()
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = np.float32(sim[12]) * sim[:9].reshape(3, 3), sim[9:12]
        return T, inl, int(res.n_inliers)

    def iterate(self, nIterations: int):
        """-> (T12 4x4 float32 = [s12 R12 | t12] or None, bNoMore, vbInliers [n1] bool, nInliers, the Sim3Result): what the
        reference's iterate returns in this turn of nIterations iterations."""
        res = self._run()[0]
        self._turns += max(int(nIterations), 0)  # (the iterations asked for so far, as the shim counts them)
        done = self._turns
        none = np.zeros(len(self._match), bool)
        if res.status & (SIM3_FEW_POINTS | SIM3_BAD_INPUT | SIM3_NONFINITE):
            return None, True, none, 0, res
        if res.found_it >= 0 and res.found_it < done:
            T, inl, n = self._answer()
            return T, False, inl, n, res
        return None, res.found_it < 0 and done >= res.its_run, none, 0, res

    def find(self):
        """-> (T12 4x4 float32 or None, vbInliers [n1] bool, nInliers, the Sim3Result): iterate until a result or bNoMore."""
        res = self._run()[0]
        if res.status & SIM3_NO_RESULT:
            return None, np.zeros(len(self._match), bool), 0, res
        T, inl, n = self._answer()
        return T, inl, n, res

    def GetEstimatedRotation(self) -> np.ndarray:
        return self._run()[1][:9].reshape(3, 3).copy()

    def GetEstimatedTranslation(self) -> np.ndarray:
        return self._run()[1][9:12].copy()

    def GetEstimatedScale(self) -> float:
        return float(self._run()[1][12])


class Optimizer:
    """The part of ORB-SLAM2's Optimizer a tracker calls on every frame (include/orbx.h, "behind SearchByBoW: pose optimisation")."""

    @staticmethod
    def PoseOptimization(frame: Frame, points, mask, Tcw, K=None, extractor: Optional[ORBextractor] = None, n_iterations: int = 10):
        """Optimizer::PoseOptimization(&frame): frame.mvKeysUn against one map point per feature (points [N, 3], mask [N] = the
        feature has one: mvpMapPoints), from the pose Tcw (3x4 or 4x4).  K: 3x3, default the frame's camera.  Returns (the inlier
        count, the refined Tcw 4x4 float32, vbOutlier [N] bool, the PoseResult)."""
        ext = extractor or frame.mpORBextractor
        if ext is None:
            raise OrbxError(E_BADARG, "Optimizer needs an ORBextractor (device context); pass extractor=")
        K = _camera_K(K, frame, "Optimizer.PoseOptimization", "frame")
        res, outlier = ext.pose_optimize(frame.mvKeysUn, points, mask, Tcw, K, None, n_iterations)
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = np.array(res.R[:], np.float32).reshape(3, 3), np.array(res.tcw[:], np.float32)
        return int(res.n_inliers), T, outlier, res

    @staticmethod
    def OptimizeSim3(kf1: Frame, kf2: Frame, map1, map2, matches12, s12: float, R12, t12, th2: float = 10.0, bFixScale: bool = False,
                     K=None, extractor: Optional[ORBextractor] = None, n_iterations: int = 5, n_more_iterations: int = 10):
        """Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (include/orbx.h, "loop closing: Sim3
        optimisation").  map1 / map2: (points [N, 3], mask [N] or None, Tcw 3x4 or 4x4) of each keyframe; matches12 int32 [N1]:
        KF2's feature per feature of KF1, or -1.  Returns (nIn, the edited matches12, (s12, R12 3x3, t12), the Sim3OptResult): the similarity is
        the one given when nIn is 0 because fewer than 10 correspondences survived the first classification."""
        ext = extractor or kf1.mpORBextractor or kf2.mpORBextractor
        if ext is None:
            raise OrbxError(E_BADARG, "Optimizer needs an ORBextractor (device context); pass extractor=")
        K = _camera_K(K, kf1, "Optimizer.OptimizeSim3", "keyframe")
        (p1, m1, T1), (p2, m2, T2) = map1, map2
        sim = np.r_[np.asarray(R12, np.float32).reshape(9), np.asarray(t12, np.float32).reshape(3), np.float32(s12)].astype(np.float32)
        res, out, row = ext.optimize_sim3(kf1.mvKeysUn, p1, m1, _pose12(T1), kf2.mvKeysUn, p2, m2, _pose12(T2), matches12, sim, K, None, bFixScale, th2,
                                          n_iterations, n_more_iterations)
        return int(res.n_inliers), row, (float(out[12]), out[:9].reshape(3, 3).copy(), out[9:12].copy()), res

    @staticmethod
    def LocalBundleAdjustment(keyframes, n_free: int, rows, map_points, map_mask=None, K=None, extractor: Optional[ORBextractor] = None,
                              n_iterations: int = 5, n_more_iterations: int = 10):
        """Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap) (include/orbx.h, "local mapping: local bundle adjustment").
        keyframes: a list of (Frame, Tcw 3x4 / 4x4 / 12 floats), lLocalKeyFrames (the first n_free) then lFixedCameras; rows: per
        keyframe its mvpMapPoints as indices into map_points [N, 3] (negative: none).  Returns (the poses [n, 4, 4] float32, the
        points [N, 3] float32, vToErase as a list of (keyframe, feature), the LbaResult); the erasures stay with the caller."""
        frames = [kf for kf, _ in keyframes]
        ext = extractor or next((f.mpORBextractor for f in frames if f.mpORBextractor is not None), None)
        if ext is None:
            raise OrbxError(E_BADARG, "Optimizer needs an ORBextractor (device context); pass extractor=")
        K = _camera_K(K, frames[0] if frames else None, "Optimizer.LocalBundleAdjustment", "keyframe")
        cap = max([len(f.mvKeysUn) for f in frames] + [1])
        keys, r = np.zeros((len(frames), cap), KEYPOINT_DTYPE), np.full((len(frames), cap), -1, np.int32)
        for e, f in enumerate(frames):
            keys[e, :len(f.mvKeysUn)] = _keys(f.mvKeysUn)
            r[e, :len(f.mvKeysUn)] = _row(rows[e], len(f.mvKeysUn), "rows needs one entry per feature of its keyframe")[:len(f.mvKeysUn)]
        poses = np.stack([_pose12(T) for _, T in keyframes]) if frames else np.zeros((0, 12), np.float32)
        res, pose_out, pts, outlier = ext.local_ba(keys, [len(f.mvKeysUn) for f in frames], poses, r, n_free, map_points, map_mask, K, None,
                                                   n_iterations, n_more_iterations)
        T = np.tile(np.eye(4, dtype=np.float32), (len(frames), 1, 1))
        T[:, :3, :3], T[:, :3, 3] = pose_out[:, :9].reshape(-1, 3, 3), pose_out[:, 9:]
        return T, pts, [(int(e), int(f)) for e, f in zip(*np.nonzero(outlier))], res
