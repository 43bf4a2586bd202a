"""The Python package against include/orbx.h, without a device: the argtypes table of lib(), the layouts of the record table
(_records.py), and the byte-size guard of every device-resident call."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_KINDS = {"int": "i4", "int32_t": "i4", "unsigned": "u4", "unsigned int": "u4", "uint32_t": "u4", "size_t": "u8", "uint64_t": "u8",
           "int64_t": "i8", "long long": "i8", "float": "f4", "double": "f8", "void": "void"}
CTYPES_KINDS = {"i": "i4", "I": "u4", "l": "i8", "q": "i8", "L": "u8", "Q": "u8", "f": "f4", "d": "f8", "P": "ptr", "z": "ptr"}


def prototypes():
    """{function: (return type, [(parameter type, parameter name)])} of include/orbx.h, comments stripped."""
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\s*\b(orbx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        plist = []
        for p in (q.strip() for q in params.split(",")):
            if p and p != "void":
                m = re.fullmatch(r"(.*?)(\w+)\s*(\[\s*\d*\s*\])?", p, flags=re.S)
                assert m, "%s: cannot read the parameter %r" % (name, p)
                plist.append((" ".join((m.group(1) + ("*" if m.group(3) else "")).split()), m.group(2)))
        out[name] = (" ".join(ret.replace("ORBX_API", "").split()), plist)
    return out


def c_kind(ctype: str, where: str) -> str:
    if "*" in ctype:
        return "ptr"
    base = " ".join(w for w in ctype.split() if w != "const")
    assert base in C_KINDS, "%s: a type this test does not know: %r" % (where, ctype)
    return C_KINDS[base]


def ctypes_kind(t, where: str) -> str:
    if t is None:
        return "void"
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return "ptr"
    code = getattr(t, "_type_", None)
    assert code in CTYPES_KINDS, "%s: a ctypes type this test does not know: %r" % (where, t)
    return CTYPES_KINDS[code]


def test_argtypes_match_the_header(orbx):
    """lib()'s hand-kept argtypes / restype of every function include/orbx.h declares: the same count and, position by position,
    the same kind (pointer, 32-bit int, unsigned, 64-bit, float, double) as the prototype."""
    protos = prototypes()
    assert len(protos) >= 100
    L = orbx.lib()
    for name, (ret, params) in sorted(protos.items()):
        fn = getattr(L, name)
        assert fn.argtypes is not None, "%s: lib() sets no argtypes" % name
        want = [c_kind(t, "%s(%s)" % (name, n)) for t, n in params]
        have = [ctypes_kind(t, "%s argument %d" % (name, i)) for i, t in enumerate(fn.argtypes)]
        assert have == want, "%s: argtypes %s, the header says %s" % (name, have, want)
        assert ctypes_kind(fn.restype, name + " restype") == c_kind(ret, name + " return type"), name


def test_record_layouts_match_the_header(orbx, tmp_path):
    """Every record of the record table against its C struct: a probe compiled with the host C compiler prints sizeof and each
    field's offset and size; the numpy dtype and the ctypes class must both agree with it, and the fields must tile the struct."""
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler on this machine")
    from orb_slam_tracking_amd._records import RECORDS
    assert len(RECORDS) == 19  # every struct of the header with a body
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "orbx.h"', "int main(void) {"]
    for c_name, (_, dtype) in RECORDS.items():
        lines.append('  printf("%s %%zu 0\\n", sizeof(%s));' % (c_name, c_name))
        for f in dtype.names:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (c_name, f, c_name, f, c_name, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe"), str(src)], check=True)
    seen = {}
    for ln in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split("\n"):
        if ln:
            key, a, b = ln.split()
            seen[key] = (int(a), int(b))
    for c_name, (cls, dtype) in RECORDS.items():
        assert dtype.itemsize == seen[c_name][0] == ctypes.sizeof(cls), c_name
        end = 0
        for f, (cname, _) in zip(dtype.names, cls._fields_):
            off, size = seen["%s.%s" % (c_name, f)]
            assert (dtype.fields[f][1], dtype.fields[f][0].itemsize) == (off, size), "%s.%s (dtype)" % (c_name, f)
            assert cname in (f, f + "_") and (getattr(cls, cname).offset, getattr(cls, cname).size) == (off, size), "%s.%s (ctypes)" % (c_name, f)
            assert off == end, "%s.%s: a gap, or a field of the struct the record table lacks" % (c_name, f)
            end = off + size
        assert end == dtype.itemsize, "%s: the record table ends before the struct does" % c_name
    assert orbx.KEYPOINT_DTYPE is RECORDS["orbx_keypoint"][1]


# ---- the guard of the device-resident calls -----------------------------------------------------------------------------------
class Recorder:
    """Stands in for liborbx.so: every orbx_* function records its arguments and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("orbx_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


CAP, NF, NS, P, MCAP, NIT, W, H = 8, 2, 2, 1, 4, 1, 16, 4  # capacity, frames, point / map sets, pairs, map capacity, n_iter, frame


@pytest.fixture
def fake(orbx):
    """(ORBextractor, Vocabulary, Database) without a context, over a Recorder.  The only place that knows the private names."""
    rec = Recorder()
    ext = object.__new__(orbx.ORBextractor)
    ext._L, ext._h, ext.capacity, ext.nlevels, ext.nfeatures, ext.order_with_torch = rec, ctypes.c_void_p(0), CAP, 8, 8, True
    voc = object.__new__(orbx.Vocabulary)
    voc._ext, voc._L, voc._h = ext, rec, ctypes.c_void_p(0)
    db = object.__new__(orbx.Database)
    db._ext, db._L, db._h = ext, rec, ctypes.c_void_p(0)
    return {"ext": ext, "voc": voc, "db": db, "rec": rec, "orbx": orbx}


K3, BOUNDS = np.eye(3, dtype=np.float32), (0, W, 0, H)
IMG = (NF - 1) * W * H + (H - 1) * W + W  # the last frame's last row ends here
FRAME = dict(width=W, height=H, stride=W, frame_stride=W * H)
KPS, DESC, CNT, ROW, POSE, SIM = NF * CAP * 28, NF * CAP * 32, NF * 4, P * CAP * 4, 48, 52
EXTRACT = [("d_kps", "d_kps", KPS), ("d_desc", "d_desc32", DESC), ("d_n", "d_n_out", CNT)]
MATCH_INIT = [("d_matches12", "d_matches12", ROW), ("d_nmatches", "d_nmatches", P * 4), ("d_stats", "d_stats", P * 12, True)]
POINT_SETS = [("d_points", "d_points", NS * CAP * 12), ("d_point_mask", "d_point_mask", NS * CAP, True)]
MAP_SETS = [("d_map_n", "d_map_n", NS * 4), ("d_map_points", "d_map_points", NS * MCAP * 12), ("d_map_normals", "d_map_normals", NS * MCAP * 12),
            ("d_map_dist", "d_map_dist", NS * MCAP * 8), ("d_map_desc", "d_map_desc32", NS * MCAP * 32),
            ("d_map_mask", "d_map_mask", NS * MCAP, True)]
FRAMES_UN = [("d_kps_un", "d_kps_un", KPS), ("d_desc", "d_desc32", DESC), ("d_n", "d_n", CNT)]
FRAMES_UN_NODESC = [("d_kps_un", "d_kps_un", KPS), ("d_n", "d_n", CNT)]
FV = [("d_fv_node", "d_fv_node", NF * CAP * 4), ("d_fv_feat", "d_fv_feat", NF * CAP * 4), ("d_fv_n", "d_fv_n", NF * 4)]
BOW = [("d_bow_word", "d_bow_word", NF * CAP * 4), ("d_bow_value", "d_bow_value", NF * CAP * 8), ("d_bow_n", "d_bow_n", NF * 4)]
PAIRS4 = dict(kf1=[0], kf2=[1], set1=[0], set2=[1])

# method -> (owner, C function, the other arguments, [(argument, the C parameter of include/orbx.h, bytes[, optional])]): the bytes
# are the layouts the header documents at the sizes above.  optional = True: None arrives as a null pointer; optional = the
# name of another argument: None stands for that array.
CASES = {
    "extract_batch_device": ("ext", "orbx_extract_batch_device", dict(n_frames=NF, **FRAME), [("d_imgs", "d_imgs", IMG)] + EXTRACT),
    "match_pairs_device": ("ext", "orbx_match_init_batch_device", dict(first=[0], second=[1], bounds=BOUNDS),
                           [("d_kps", "d_kps", KPS), ("d_desc", "d_desc32", DESC), ("d_n", "d_n", CNT)] + MATCH_INIT),
    "extract_match_batch_device": ("ext", "orbx_extract_match_batch_device", dict(n_frames=NF, first=[0], second=[1], bounds=BOUNDS, **FRAME),
                                   [("d_imgs", "d_imgs", IMG)] + EXTRACT + MATCH_INIT),
    "extract_match_batch_device_async": ("ext", "orbx_extract_match_batch_device_async",
                                         dict(n_frames=NF, first=[0], second=[1], bounds=BOUNDS, **FRAME),
                                         [("d_imgs", "d_imgs", IMG)] + EXTRACT + MATCH_INIT),
    "extract_match_batch_host_async": ("ext", "orbx_extract_match_batch_host_async",
                                       dict(n_frames=NF, first=[0], second=[1], bounds=BOUNDS, **FRAME),
                                       [("h_imgs", "h_imgs", IMG), ("h_kps", "h_kps", KPS), ("h_desc", "h_desc32", DESC), ("h_n", "h_n_out", CNT),
                                        ("h_matches12", "h_matches12", ROW), ("h_nmatches", "h_nmatches", P * 4),
                                        ("h_stats", "h_stats", P * 12, True)]),
    "to_gray_batch_device": ("ext", "orbx_to_gray_batch_device",
                             dict(n_frames=NF, width=W, height=H, stride=3 * W, frame_stride=3 * W * H, channels=3, bRGB=False, gray_stride=W,
                                  gray_frame_stride=W * H),
                             [("d_src", "d_src", (NF - 1) * 3 * W * H + (H - 1) * 3 * W + 3 * W), ("d_gray", "d_gray", IMG)]),
    "undistort_batch_device": ("ext", "orbx_undistort_batch_device", dict(n_frames=NF, camera=(1, 1, 0, 0, 0, 0, 0, 0)),
                               [("d_kps", "d_kps", KPS), ("d_n", "d_n", CNT), ("d_kps_un", "d_kps_un", KPS)]),
    "match_bow_pairs_device": ("ext", "orbx_match_bow_batch_device", dict(n_frames=NF, kf=[0], f=[1]),
                               [("d_kps", "d_kps", KPS), ("d_desc", "d_desc32", DESC), ("d_n", "d_n", CNT)] + FV +
                               [("d_kf_mask", "d_kf_mask", NF * CAP, True), ("d_matches_f", "d_matches_f", ROW), ("d_nmatches", "d_nmatches", P * 4)]),
    "match_projection_pairs_device": ("ext", "orbx_match_projection_batch_device",
                                      dict(n_frames=NF, last=[0], cur=[1], point_set=[1], n_point_sets=NS, K=K3, bounds=BOUNDS),
                                      FRAMES_UN + POINT_SETS + [("d_point_desc", "d_point_desc32", NS * CAP * 32, True),
                                                                ("d_last_outlier", "d_last_outlier", P * CAP, True),
                                                                ("d_pose_cur", "d_pose_cur", P * POSE), ("d_matches_cur", "d_matches_cur", ROW),
                                                                ("d_res", "d_res", P * 32)]),
    "match_local_map_pairs_device": ("ext", "orbx_match_local_map_batch_device",
                                     dict(n_frames=NF, frame=[1], map_set=[1], n_map_sets=NS, map_capacity=MCAP, K=K3, bounds=BOUNDS),
                                     FRAMES_UN + MAP_SETS + [("d_pose", "d_pose", P * POSE), ("d_matches", "d_matches", ROW),
                                                             ("d_outlier", "d_outlier", P * CAP, True),
                                                             ("d_point_view", "d_point_view", P * MCAP, True), ("d_res", "d_res", P * 60)]),
    "match_keyframe_projection_pairs_device": ("ext", "orbx_match_keyframe_projection_batch_device",
                                               dict(n_frames=NF, kf=[0], cur=[1], point_set=[1], n_point_sets=NS, K=K3, bounds=BOUNDS),
                                               FRAMES_UN + POINT_SETS + [("d_point_desc", "d_point_desc32", NS * CAP * 32, True),
                                                                         ("d_point_dist", "d_point_dist", NS * CAP * 8),
                                                                         ("d_pose", "d_pose", P * POSE), ("d_matches", "d_matches", ROW),
                                                                         ("d_outlier", "d_outlier", P * CAP, True), ("d_res", "d_res", P * 52)]),
    "match_sim3_pairs_device": ("ext", "orbx_match_sim3_batch_device", dict(n_frames=NF, n_point_sets=NS, K=K3, bounds=BOUNDS, **PAIRS4),
                                FRAMES_UN + POINT_SETS + [("d_point_desc", "d_point_desc32", NS * CAP * 32, True),
                                                          ("d_point_dist", "d_point_dist", NS * CAP * 8), ("d_pose", "d_pose", NF * POSE),
                                                          ("d_sim3", "d_sim3", P * SIM), ("d_matches", "d_matches", ROW), ("d_res", "d_res", P * 64)]),
    "match_triangulation_pairs_device": ("ext", "orbx_match_triangulation_batch_device", dict(n_frames=NF, kf1=[0], kf2=[1], K=K3),
                                         FRAMES_UN + FV + [("d_mask", "d_mask", NF * CAP, True), ("d_pose", "d_pose", NF * POSE),
                                                           ("d_median_depth", "d_median_depth", NF * 4, True),
                                                           ("d_matches12", "d_matches12", ROW), ("d_res", "d_res", P * 76)]),
    "triangulate_matches_pairs_device": ("ext", "orbx_triangulate_matches_batch_device", dict(n_frames=NF, kf1=[0], kf2=[1], K=K3),
                                         FRAMES_UN_NODESC + [("d_pose", "d_pose", NF * POSE), ("d_matches12", "d_matches12", ROW),
                                                             ("d_points", "d_points", P * CAP * 12), ("d_point_mask", "d_point_mask", P * CAP),
                                                             ("d_point_normal", "d_point_normal", P * CAP * 12),
                                                             ("d_point_dist", "d_point_dist", P * CAP * 8), ("d_res", "d_res", P * 44)]),
    "find_models_batch_device": ("ext", "orbx_find_models_batch_device", dict(n_frames=NF, first=[0], second=[1], n_iter=NIT),
                                 FRAMES_UN_NODESC + [("d_matches12", "d_matches12", ROW), ("d_sets", "d_sets", P * NIT * 32),
                                                     ("d_res", "d_res", P * 152), ("d_inliers", "d_inliers", P * 2 * CAP, True),
                                                     ("d_models", "d_models", 3 * P * NIT * 36, True),
                                                     ("d_scores", "d_scores", 2 * P * NIT * 4, True)]),
    "initialize_batch_device": ("ext", "orbx_initialize_batch_device", dict(n_frames=NF, first=[0], second=[1], n_iter=NIT, K=K3),
                                FRAMES_UN_NODESC + [("d_matches12", "d_matches12", ROW), ("d_sets", "d_sets", P * NIT * 32),
                                                    ("d_res", "d_res", P * 184), ("d_p3d", "d_p3d", P * CAP * 12, True),
                                                    ("d_triangulated", "d_triangulated", P * CAP, True)]),
    "bundle_adjust_batch_device": ("ext", "orbx_bundle_adjust_batch_device", dict(n_frames=NF, first=[0], second=[1], K=K3),
                                   FRAMES_UN_NODESC + [("d_matches12", "d_matches12", ROW), ("d_init_res", "d_init_res", P * 184),
                                                       ("d_p3d", "d_p3d", P * CAP * 12), ("d_triangulated", "d_triangulated", P * CAP),
                                                       ("d_res", "d_res", P * 168), ("d_p3d_out", "d_p3d_out", P * CAP * 12, "d_p3d")]),
    "pose_optimize_batch_device": ("ext", "orbx_pose_optimize_batch_device", dict(n_frames=NF, frame=[1], point_set=[1], n_point_sets=NS, K=K3),
                                   FRAMES_UN_NODESC + [("d_match", "d_match", ROW, True)] + POINT_SETS +
                                   [("d_pose0", "d_pose0", P * POSE), ("d_res", "d_res", P * 192), ("d_outlier", "d_outlier", P * CAP)]),
    "pnp_solve_batch_device": ("ext", "orbx_pnp_solve_batch_device",
                               dict(n_frames=NF, frame=[1], point_set=[1], n_point_sets=NS, K=K3, n_iter=NIT),
                               FRAMES_UN_NODESC + [("d_match", "d_match", ROW, True)] + POINT_SETS +
                               [("d_draws", "d_draws", P * NIT * 16), ("d_res", "d_res", P * 200), ("d_pose", "d_pose", P * POSE),
                                ("d_match_inliers", "d_match_inliers", ROW), ("d_inliers", "d_inliers", P * CAP, True)]),
    "sim3_solve_batch_device": ("ext", "orbx_sim3_solve_batch_device", dict(n_frames=NF, n_point_sets=NS, K=K3, n_iter=NIT, **PAIRS4),
                                FRAMES_UN_NODESC + [("d_match", "d_match", ROW)] + POINT_SETS +
                                [("d_pose", "d_pose", NF * POSE), ("d_draws", "d_draws", P * NIT * 12), ("d_res", "d_res", P * 96),
                                 ("d_sim3", "d_sim3", P * SIM), ("d_match_inliers", "d_match_inliers", ROW),
                                 ("d_inliers", "d_inliers", P * CAP, True)]),
    "optimize_sim3_pairs_device": ("ext", "orbx_optimize_sim3_batch_device", dict(n_frames=NF, n_point_sets=NS, K=K3, **PAIRS4),
                                   FRAMES_UN_NODESC + [("d_matches", "d_matches", ROW)] + POINT_SETS +
                                   [("d_pose", "d_pose", NF * POSE), ("d_sim3", "d_sim3", P * SIM), ("d_res", "d_res", P * 208),
                                    ("d_sim3_out", "d_sim3_out", P * SIM, "d_sim3")]),
    "sim3_compose_scw_pairs_device": ("ext", "orbx_sim3_compose_scw_batch_device", dict(n_frames=NF, kf2=[1]),
                                      [("d_pose", "d_pose", NF * POSE), ("d_sim3", "d_sim3", P * SIM), ("d_scw", "d_scw", P * POSE)]),
    "match_scw_pairs_device": ("ext", "orbx_match_scw_batch_device",
                               dict(n_frames=NF, kf=[0], map_set=[1], n_map_sets=NS, map_capacity=MCAP, K=K3, bounds=BOUNDS),
                               FRAMES_UN + MAP_SETS + [("d_scw", "d_scw", P * POSE), ("d_matches", "d_matches", ROW),
                                                       ("d_kf2_to_map", "d_kf2_to_map", ROW, True), ("d_res", "d_res", P * 56)]),
    "transform_batch_device": ("voc", "orbx_bow_transform_batch_device", dict(n_frames=NF),
                               [("d_desc", "d_desc32", DESC), ("d_n", "d_n", CNT)] + BOW + FV + [("d_feat_word", "d_feat_word", NF * CAP * 4, True)]),
    "score_pairs_device": ("voc", "orbx_bow_score_batch_device", dict(n_frames=NF, first=[0], second=[1]),
                           BOW + [("d_score", "d_score_f64", P * 8)]),
    "add_batch_device": ("db", "orbx_database_add_batch_device", dict(n_frames=NF), BOW),
    "query_batch_device": ("db", "orbx_database_query_batch_device", dict(n_queries=NF, max_results=3),
                           BOW + [("d_res_entry", "d_res_entry", NF * 3 * 4), ("d_res_score", "d_res_score", NF * 3 * 8),
                                  ("d_res_n", "d_res_n", NF * 4)]),
}
# Vocabulary.train's device form is a classmethod over an extractor: (C function, other arguments, arrays) as above
TRAIN_CASE = ("orbx_vocabulary_train_device", dict(n_docs=NF),
              [("d_desc", "d_desc32", DESC), ("d_n", "d_n", CNT), ("d_feat_word", "d_feat_word", NF * CAP * 4, True)])
# the chains: the C calls each makes, in order (their parts are the cases above).  relocalize_refine_pairs_device is not here: it
# indexes torch device tensors between its parts, which are pose_optimize_batch_device and match_keyframe_projection_pairs_device.
CHAINS = {
    "create_new_map_points_pairs_device": ("match_triangulation_pairs_device", "triangulate_matches_pairs_device"),
    "compute_sim3_pairs_device": ("sim3_solve_batch_device", "match_sim3_pairs_device"),
    "compute_sim3_optimized_pairs_device": ("sim3_solve_batch_device", "match_sim3_pairs_device", "optimize_sim3_pairs_device"),
    "compute_sim3_loop_pairs_device": ("sim3_solve_batch_device", "match_sim3_pairs_device", "optimize_sim3_pairs_device",
                                       "sim3_compose_scw_pairs_device", "match_scw_pairs_device"),
}
# (method, argument) pairs whose guard is known to be missing: none.  Filled in only for a run against a wrapper older than
# this test, to show which guards it lacked.
MISSING_GUARDS = ()


def address(arg):
    if arg is None:
        return 0
    if isinstance(arg, ctypes.c_void_p):
        return arg.value or 0
    return arg if isinstance(arg, int) else None


def run_case(fake, method, fn, scalars, arrays, protos, call):
    """The three assertions of the guard test for one method; call(**kwargs) invokes it."""
    rec = fake["rec"]
    pos = {n: i for i, (_, n) in enumerate(protos[fn][1])}

    def made(given):
        return {a[0]: (np.zeros(a[2], np.uint8) if a[0] in given else None) for a in arrays}

    def check(given):
        arrs = made(given)
        del rec.calls[:]
        call(**scalars, **arrs)
        assert [c[0] for c in rec.calls] == [fn], "%s: the C calls made were %s" % (method, [c[0] for c in rec.calls])
        args = rec.calls[0][1]
        assert len(args) == len(protos[fn][1]), method
        for a in arrays:
            src = arrs[a[0]]
            if src is None and isinstance(a[-1], str):  # None stands for another array
                src = arrs[a[-1]]
            want = 0 if src is None else src.ctypes.data
            assert address(args[pos[a[1]]]) == want, "%s: %s does not arrive as the C parameter %s" % (method, a[0], a[1])
    everything = [a[0] for a in arrays]
    check(everything)
    check([a[0] for a in arrays if len(a) == 3])  # every optional array left out
    for a in arrays:  # one byte short, one array at a time
        arrs = made(everything)
        arrs[a[0]] = np.zeros(a[2] - 1, np.uint8)
        del rec.calls[:]
        if (method, a[0]) in MISSING_GUARDS:
            call(**scalars, **arrs)
            continue
        with pytest.raises(ValueError):
            call(**scalars, **arrs)
        assert rec.calls == [], "%s: %s is one byte short and the C call was made" % (method, a[0])


@pytest.mark.parametrize("method", sorted(CASES))
def test_device_call_guards_every_array(fake, method):
    """No device: a context-less ORBextractor / Vocabulary / Database over a recording stand-in for the library.  With every
    array at exactly the size the header documents one C call is made and each array arrives at its parameter's position;
    optional arrays left out arrive as null; any one array one byte short is a ValueError before the call."""
    owner, fn, scalars, arrays = CASES[method]
    run_case(fake, method, fn, scalars, arrays, prototypes(), getattr(fake[owner], method))


def test_vocabulary_train_device_guards_every_array(fake, monkeypatch):
    fn, scalars, arrays = TRAIN_CASE
    Voc = fake["orbx"].Vocabulary
    monkeypatch.setattr(Voc, "__init__", lambda self, extractor, handle: None)  # (the real one asks the library for the tree's shape)
    run_case(fake, "Vocabulary.train", fn, scalars, arrays, prototypes(), lambda **kw: Voc.train(fake["ext"], **kw))


def test_every_device_method_is_in_the_table(orbx):
    listed = set(CASES) | set(CHAINS) | {"relocalize_refine_pairs_device"}
    for cls in (orbx.ORBextractor, orbx.Vocabulary, orbx.Database):
        for name in vars(cls):
            if name.endswith(("_batch_device", "_pairs_device", "_device_async", "_host_async")) and not name.startswith("_"):
                assert name in listed, "%s.%s has no case in this file" % (cls.__name__, name)


@pytest.mark.parametrize("method", sorted(CHAINS))
def test_device_chains_queue_their_parts(fake, method):
    """A chain makes its parts' C calls in order, each array at its parameter's position in every part that takes it, and nothing
    else (no copy, no wait)."""
    protos, rec = prototypes(), fake["rec"]
    scalars = {}
    for part in CHAINS[method]:
        sc = CASES[part][2]
        scalars.update(sc)
    # the chains name some arrays of their parts differently
    rename = {"compute_sim3_pairs_device": {"sim3_solve_batch_device": {"d_res": "d_sim3_res", "d_match_inliers": "d_matches", "d_inliers": None},
                                            "match_sim3_pairs_device": {"d_res": "d_msim3_res"},
                                            "optimize_sim3_pairs_device": {"d_res": "d_opt_res", "d_sim3_out": None},
                                            "match_scw_pairs_device": {"d_res": "d_scw_res"}},
              "create_new_map_points_pairs_device": {"match_triangulation_pairs_device": {"d_res": "d_match_res"}}}
    rename = rename["create_new_map_points_pairs_device" if method.startswith("create") else "compute_sim3_pairs_device"]
    given = {}
    for part in CHAINS[method]:
        for a in CASES[part][3]:
            n = rename.get(part, {}).get(a[0], a[0])
            if n is not None:
                given[n] = max(given.get(n, 0), a[2])
    if method == "compute_sim3_loop_pairs_device":
        scalars.update(map_set=[1])
        scalars.pop("kf", None)
    for k in ("n_iter",):
        scalars.pop(k, None)
    bufs = {n: np.zeros(b, np.uint8) for n, b in given.items()}
    if "d_draws" in bufs:
        scalars["n_iter"] = NIT
    del rec.calls[:]
    getattr(fake["ext"], method)(**scalars, **bufs)
    assert [c[0] for c in rec.calls] == [CASES[p][1] for p in CHAINS[method]]
    for (fn, args), part in zip(rec.calls, CHAINS[method]):
        pos = {n: i for i, (_, n) in enumerate(protos[fn][1])}
        for a in CASES[part][3]:
            n = rename.get(part, {}).get(a[0], a[0])
            if n is not None:
                assert address(args[pos[a[1]]]) == bufs[n].ctypes.data, "%s: %s in %s" % (method, n, fn)
