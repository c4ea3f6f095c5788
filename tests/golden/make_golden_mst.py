"""tests/golden/mst_vectors.npz: the reference's `init_minimum_spanning_tree` (dust3r/cloud_opt/init_im_poses.py:66-221), executed
from the reference tree (`ref_loader.REF`; build container only) on its `PointCloudOptimizer`, in float32 on the CPU.

What is substituted, and why (README_mst.md): `roma` -> roma_standin_mst.py (not installed); `cv2`, `dust3r.viz`,
`dust3r.utils.image` -> stubs (imported, never used on this path); the `dust3r`, `dust3r.utils` and `dust3r.cloud_opt` packages
are bare; `fast_pnp` -> a function that returns None: the reference's own failed-PnP path (init_im_poses.py:213-216), which needs
no cv2 and is not random.  scipy and tqdm are the installed ones.

Inputs: tests/mst_init_util.py's `scaled_problem` per configuration of `CONFIGS`.  Per recording <tag> (1, 2, 2avg, 3, 4), prefix
`mst_<tag>_` (the inputs pred_i pred_j conf_i conf_j only under the plain tags):
  scores [E]            compute_edge_scores, in edge order
  mst_edges [V-1,2]     the tree, in the order the walk took its edges
  focal_edge [V]        the edge whose pred_i fed image v's focal (-1: none; found by matching the recorded estimate calls)
  focals [V]            the per-image Weiszfeld estimates before focal_avg (NaN: none)
  pts3d [V,n,3]         after the scale normalisation
  depth_log im_pose focal_log pp_raw pw_pose      the object's parameters afterwards
Run:  python tests/golden/make_golden_mst.py"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402
from tests import mst_init_util as mu  # noqa: E402

REF = ref_loader.REF


def _module(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


spec = importlib.util.spec_from_file_location("roma", os.path.join(HERE, "roma_standin_mst.py"))
roma = importlib.util.module_from_spec(spec)
spec.loader.exec_module(roma)
sys.modules["roma"] = roma
_module("cv2")
_module("dust3r", os.path.join(REF, "dust3r"))
_module("dust3r.utils", os.path.join(REF, "dust3r", "utils"))
_module("dust3r.cloud_opt", os.path.join(REF, "dust3r", "cloud_opt"))
_module("dust3r.utils.image", rgb=lambda x: x)
_module("dust3r.viz", SceneViz=None, segment_sky=None, auto_cam_size=None, to_numpy=lambda x: x)
from dust3r.cloud_opt.optimizer import PointCloudOptimizer  # noqa: E402  (the reference's)
from dust3r.cloud_opt import init_im_poses as init_fun  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(1)
init_fun.fast_pnp = lambda *a, **k: None

log = {}
_estimate_focal, _mst = init_fun.estimate_focal, init_fun.minimum_spanning_tree


def estimate_focal(pts3d_i, pp=None):
    f = _estimate_focal(pts3d_i, pp)
    log["estimates"].append((pts3d_i.data_ptr(), f))
    return f


def minimum_spanning_tree(*a, **k):
    pts3d, msp_edges, im_focals, im_poses = _mst(*a, **k)
    log["msp_edges"], log["im_focals"], log["im_poses"] = list(msp_edges), list(im_focals), im_poses.clone()
    return pts3d, msp_edges, im_focals, im_poses


init_fun.estimate_focal, init_fun.minimum_spanning_tree = estimate_focal, minimum_spanning_tree

out = {}
for tag in mu.ALL_TAGS:
    base, avg = (tag[:-3], True) if tag.endswith("avg") else (tag, False)
    V, H, W, edges, _, _ = mu.CONFIGS[base]
    a = mu.scaled_problem(base)
    E, n = len(edges), H * W
    t = {k: torch.from_numpy(v) for k, v in a.items()}
    view1, view2 = {"idx": [i for i, j in edges]}, {"idx": [j for i, j in edges]}
    pred1 = {"pts3d": t["pred_i"].view(E, H, W, 3), "conf": t["conf_i"].view(E, H, W)}
    pred2 = {"pts3d_in_other_view": t["pred_j"].view(E, H, W, 3), "conf": t["conf_j"].view(E, H, W)}
    scene = PointCloudOptimizer(view1, view2, pred1, pred2, verbose=False)
    assert scene.edges == [tuple(e) for e in edges] and scene.n_imgs == V and scene.norm_pw_scale
    log.clear()
    log["estimates"] = []
    init_fun.init_minimum_spanning_tree(scene, focal_avg=avg)
    assert scene.im_focals.requires_grad == (not avg)

    names = [f"{i}_{j}" for i, j in edges]
    scores = init_fun.compute_edge_scores(map(init_fun.i_j_ij, edges), scene.conf_i, scene.conf_j)
    vals = sorted(scores.values())
    assert all(b >= 1.05 * a_ for a_, b in zip(vals, vals[1:])), ("scores closer than 5 %", tag, vals)
    ptr_edge = {scene.pred_i[k].data_ptr(): e for e, k in enumerate(names)}
    focal_edge = -np.ones(V, dtype=np.int64)
    focals = np.full(V, np.nan, dtype=np.float32)
    for v in range(V):
        f = log["im_focals"][v]
        if f is None:
            continue
        fed = [ptr_edge[p] for p, val in log["estimates"] if val == f]
        assert len(set(fed)) == 1, (tag, v, fed)
        focal_edge[v], focals[v] = fed[0], f
    # the poses the walk itself set, against identities: the failed PnP leaves the others at the identity
    eye = torch.eye(4)
    walk_posed = [v for v in range(V) if not torch.equal(log["im_poses"][v], eye)]
    if not avg:
        for k in ("pred_i", "pred_j", "conf_i", "conf_j"):
            out[f"mst_{tag}_{k}"] = a[k]
    out[f"mst_{tag}_scores"] = np.asarray([scores[tuple(e)] for e in edges], dtype=np.float64)
    out[f"mst_{tag}_mst_edges"] = np.asarray(log["msp_edges"], dtype=np.int64)
    out[f"mst_{tag}_focal_edge"] = focal_edge
    out[f"mst_{tag}_focals"] = focals
    with torch.no_grad():
        out[f"mst_{tag}_depth_log"] = scene.im_depthmaps.detach().numpy().copy()
        out[f"mst_{tag}_im_pose"] = scene.im_poses.detach().numpy().copy()
        out[f"mst_{tag}_focal_log"] = scene.im_focals.detach().numpy().reshape(V).copy()
        out[f"mst_{tag}_pp_raw"] = scene.im_pp.detach().numpy().copy()
        out[f"mst_{tag}_pw_pose"] = scene.pw_poses.detach().numpy().copy()
    # pts3d after the scale normalisation: init_from_pts3d scaled the walk's tensors in place; minimum_spanning_tree returned them
    # — recover them from the object: depth, pose and focal are NOT enough (pixels need not lie on their rays), so re-run the walk
    # and scale it with the object's factor
    pts3d, _, _, _ = _mst(scene.imshapes, scene.edges, scene.pred_i, scene.pred_j, scene.conf_i, scene.conf_j, scene.im_conf, scene.min_conf_thr,
                          scene.device, has_im_poses=True, verbose=False)
    factor = scene.get_pw_norm_scale_factor().detach()
    out[f"mst_{tag}_pts3d"] = torch.stack([p.reshape(n, 3) * factor for p in pts3d]).numpy()

    if base == "4":   # the walk re-queued an edge, took both branches, and read the stale i_j for a focal
        done, i_side, j_side = set(log["msp_edges"][0]), [], []
        for i, j in log["msp_edges"][1:]:
            (i_side if i in done else j_side).append((i, j))
            done |= {i, j}
        assert i_side and j_side, ("both branches", log["msp_edges"])
        tree_by_score = sorted(log["msp_edges"], key=lambda e: -scores[tuple(e)])
        assert not set(tree_by_score[0]) & set(tree_by_score[1]), "the two best tree edges are not disjoint: nothing is re-queued"
        assert log["msp_edges"] != tree_by_score, "the walk took the tree edges in score order: nothing was re-queued"
        stale = [v for v in range(V) if focal_edge[v] >= 0 and edges[focal_edge[v]][0] != v]
        assert stale, "no focal came from another image's pred_i: the stale i_j was not hit"
        print("  4: branches i-done", i_side, "j-done", j_side, "stale focals of images", stale, "walk-posed", walk_posed)
    if base == "3":
        assert list(focal_edge[1:]) == [-1, -1] and walk_posed == [], (focal_edge, walk_posed)
    print(f"{tag}: tree {log['msp_edges']} focal_edge {focal_edge.tolist()} focals {focals.tolist()}")

path = os.path.join(HERE, "mst_vectors.npz")
np.savez_compressed(path, **out)
mu._G = None
print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 300 * 1024

# the yardstick of tests/mst_init_util.py: the reference's float32 recording against the float64 restatement
worst = {}
for tag in mu.ALL_TAGS:
    y, _ = mu.recording_yardstick(tag)
    print(tag, "recording yardstick:", {k: f"{v:.2e}" for k, v in y.items()})
    for k, v in y.items():
        worst[k] = max(worst.get(k, 0.0), v)
    mu.check_restatement_equals_recording(tag)
print("RECORDING_YARDSTICK =", {k: float(f"{v:.2e}") for k, v in worst.items()})
