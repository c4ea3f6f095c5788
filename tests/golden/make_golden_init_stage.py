"""tests/golden/init_stage_vectors.npz: the tail of the reference's init stage, executed from the reference tree
(`ref_loader.REF`; build container only; needs scipy) on the seeded inputs of tests/init_stage_util.py (`synthetic_views`, the
project's own generator).  Only outputs are stored; prefix `covis_`.

What runs, all of it the reference's own source:
  * `compute_co_vis_masks` with `cal_co_vis_mask`, `project_points`, `normalize_depth` (utils/sfm_utils.py:342-432; function
    definitions executed from the file, `tqdm` bound to a pass-through);
  * `save_points3D`, `save_intrinsics`, `storePly` (utils/sfm_utils.py:227-316,495-510) through `ref_loader.sfm_writers`;
  * the ranking expression of init_geo.py:63-64 and the test-pose statement of init_geo.py:90-111 (the `if n_train < n_test`
    statement of `main`, cut out of the file and executed) with the reference's `generate_interpolated_path`.

Per case <tag> of init_stage_util.CASES (inputs float32, as the aligner hands them over):
  covis_<tag>_order               the ranking passed to compute_co_vis_masks
  covis_<tag>_masks               its result, bool [V,H,W], bit-packed (np.packbits of the flattened array)
  covis_<tag>_count               rows save_points3D kept with masks = ~result (its return value)
  covis_<tag>_head_* / _tail_*    the first / last 6 rows of what it stored: points (points3D.ply x y z), colors (the PLY's
                                  red green blue), confidence (confidence_dsp.npy)
  covis_<tag>_ranking             np.argsort(confs.mean(axis=(1, 2)))[::-1]
The stage case (init_stage_util.STAGE_CASE, run with ITS confidence ranking as the order):
  covis_<stage>_ranked_masks      bit-packed masks under that order
  covis_stage_confidence_dsp_npy / covis_stage_points3D_ply / covis_stage_cameras_txt / covis_stage_pts_num_txt
                                  the files save_points3D and save_intrinsics wrote (bytes as uint8 arrays, text as strings)
  covis_testposes_n<k>            init_geo.py:90-111 for the case's 3 training poses and n_test = k in TEST_POSE_COUNTS, [k,4,4]
Run:  python tests/golden/make_golden_init_stage.py"""
import ast
import importlib
import os
import sys
import tempfile
import textwrap
import types
from pathlib import Path

import numpy as np
import scipy
import scipy.interpolate  # noqa: F401  (the reference says `scipy.interpolate.splprep` after a bare `import scipy`)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402
from tests import init_stage_util as iu  # noqa: E402  (input data only)

REF = ref_loader.REF
sys.path.insert(0, REF)
for k in [k for k in list(sys.modules) if k == "scene" or k.startswith("scene.")]:
    del sys.modules[k]
scene_pkg = types.ModuleType("scene")            # bare package: scene/colmap_loader.py without scene/__init__.py's imports
scene_pkg.__path__ = [os.path.join(REF, "scene")]
sys.modules["scene"] = scene_pkg
spec = importlib.util.spec_from_file_location("plyfile", os.path.join(HERE, "plyfile_standin.py"))
ply = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ply)
W = ref_loader.sfm_writers(ply)

sfm = os.path.join(REF, "utils", "sfm_utils.py")
ns = {"np": np, "tqdm": lambda it, **k: it}
for name, src in ref_loader.function_sources(sfm, {"compute_co_vis_masks", "cal_co_vis_mask", "project_points", "normalize_depth"}).items():
    exec(compile(src, sfm, "exec"), ns)
compute_co_vis_masks = ns["compute_co_vis_masks"]

cu = os.path.join(REF, "utils", "camera_utils.py")
cns = {"np": np, "scipy": scipy}
for name, src in ref_loader.function_sources(cu, {"generate_interpolated_path", "viewmatrix", "normalize"}).items():
    exec(compile(src, cu, "exec"), cns)

# init_geo.py:90-111, the `if n_train < n_test: ... else: ...` statement of main()
geo = os.path.join(REF, "init_geo.py")
geo_src = open(geo).read()
main = next(n for n in ast.parse(geo_src).body if isinstance(n, ast.FunctionDef) and n.name == "main")
pose_stmt = next(n for n in ast.walk(main) if isinstance(n, ast.If) and isinstance(n.test, ast.Compare)
                 and isinstance(n.test.left, ast.Name) and n.test.left.id == "n_train")
pose_code = compile(textwrap.dedent(" " * pose_stmt.col_offset + ast.get_source_segment(geo_src, pose_stmt)), geo, "exec")


def reference_test_poses(extrinsics_w2c, n_test):
    env = {"np": np, "generate_interpolated_path": cns["generate_interpolated_path"], "extrinsics_w2c": extrinsics_w2c,
           "n_train": extrinsics_w2c.shape[0], "n_test": n_test}
    exec(pose_code, env)
    return np.asarray(env["pose_test_init"], dtype=np.float64)


def reference_masks(d, order, thr):
    V, H, Wd = d["depthmaps"].shape
    return compute_co_vis_masks(np.asarray(order), d["depthmaps"], d["pointmaps"].reshape(V, H * Wd, 3), d["intrinsics"], d["w2c"],
                                d["images"].shape, depth_threshold=thr)


def reference_points(d, masks, thr, keep_dir=None):
    """save_points3D as init_geo.py:125 calls it -> (count, points, colors, confidence, directory)"""
    V = d["depthmaps"].shape[0]
    td = keep_dir or tempfile.mkdtemp()
    n = W.save_points3D(Path(td), d["images"], d["pointmaps"], d["confidences"].reshape(V, -1), ~masks, use_masks=True,
                        save_all_pts=False, save_txt_path=td, depth_threshold=thr)
    v = ply.PlyData.read(os.path.join(td, "points3D.ply")).elements[0].data
    return (n, np.stack([v["x"], v["y"], v["z"]], axis=1), np.stack([v["red"], v["green"], v["blue"]], axis=1),
            np.load(os.path.join(td, "confidence_dsp.npy")), td)


out = {}
ROWS = 6
for tag in iu.CASES:
    d, thr, order = iu.case_inputs(tag)
    masks = reference_masks(d, order, thr)
    assert masks.dtype == bool and masks.shape == d["depthmaps"].shape and not masks[order[0]].any()
    n, pts, col, conf, _ = reference_points(d, masks, thr)
    assert n == int((~masks).sum()) == pts.shape[0] == conf.shape[0] and conf.shape[1] == 1
    out[f"covis_{tag}_order"] = np.asarray(order, dtype=np.int64)
    out[f"covis_{tag}_masks"] = np.packbits(masks.reshape(-1))
    out[f"covis_{tag}_count"] = np.int64(n)
    for part, rows in (("head", slice(0, ROWS)), ("tail", slice(n - ROWS, n))):
        out[f"covis_{tag}_{part}_points"], out[f"covis_{tag}_{part}_colors"] = pts[rows].copy(), col[rows].copy()
        out[f"covis_{tag}_{part}_confidence"] = conf[rows].copy()
    confs = d["confidences"]
    out[f"covis_{tag}_ranking"] = np.argsort(confs.mean(axis=(1, 2)))[::-1].astype(np.int64)   # init_geo.py:63-64
    mine = iu.covis_numpy(order, d["depthmaps"], d["pointmaps"], d["intrinsics"], d["w2c"], thr)
    print(f"{tag}: marked per view {[round(float(m.mean()), 4) for m in masks]}, kept {n} of {masks.size}, "
          f"restatement differs in {int((mine != masks).sum())} pixels, ranking {out[f'covis_{tag}_ranking'].tolist()}")

# the stage case under its own confidence ranking, with the files
tag = iu.STAGE_CASE
d, thr, _ = iu.case_inputs(tag)
ranking = out[f"covis_{tag}_ranking"]
masks = reference_masks(d, ranking, thr)
out[f"covis_{tag}_ranked_masks"] = np.packbits(masks.reshape(-1))
with tempfile.TemporaryDirectory() as td:
    n, pts, col, conf, _ = reference_points(d, masks, thr, keep_dir=td)
    V, H, Wd = d["depthmaps"].shape
    W.save_intrinsics(Path(td), np.repeat(d["focals"][0], V), iu.STAGE_ORG_SIZE, d["images"].shape, save_focals=False)
    out["covis_stage_confidence_dsp_npy"] = np.frombuffer(open(os.path.join(td, "confidence_dsp.npy"), "rb").read(), dtype=np.uint8)
    out["covis_stage_points3D_ply"] = np.frombuffer(open(os.path.join(td, "points3D.ply"), "rb").read(), dtype=np.uint8)
    out["covis_stage_cameras_txt"] = np.array(open(os.path.join(td, "cameras.txt")).read())
    out["covis_stage_pts_num_txt"] = np.array(open(os.path.join(td, "pts_num.txt")).read())
print(f"stage {tag}: ranking {ranking.tolist()}, kept {n}, marked per view {[round(float(m.mean()), 4) for m in masks]}")
for k in iu.TEST_POSE_COUNTS:
    out[f"covis_testposes_n{k}"] = reference_test_poses(d["w2c"], k)
    assert out[f"covis_testposes_n{k}"].shape == (k, 4, 4)

path = os.path.join(HERE, "init_stage_vectors.npz")
np.savez_compressed(path, **out)
print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes (interp_path_vectors.npz:",
      os.path.getsize(os.path.join(HERE, "interp_path_vectors.npz")), ")")
