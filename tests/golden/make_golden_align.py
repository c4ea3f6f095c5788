"""tests/golden/align_vectors.npz: the reference's global alignment, executed from the reference tree (`ref_loader.REF`; build
container only) in float32 on the CPU: `PointCloudOptimizer` (dust3r/cloud_opt/optimizer.py), `global_alignment_iter` /
`global_alignment_loop`'s body (dust3r/cloud_opt/base_opt.py:326-366) and the getters init_geo.py:51-59 reads.

What is substituted, and why (README_align.md): `roma` -> roma_standin.py (not installed); `cv2`, `dust3r.viz`,
`dust3r.utils.image` -> empty stubs (imported by the modules, never used on this path); the `dust3r`, `dust3r.utils` and
`dust3r.cloud_opt` packages are bare (their __init__ files import the network and the other optimizers).

Inputs: tests/global_align_util.py's seeded generator (`synthetic_problem`), per configuration of `CONFIGS`.  The state is written
into the reference object's parameters; configuration (b) then calls its `preset_focal`, (d) its `preset_pose` (which goes through
`_set_pose`: rotmat_to_unitquat and signed_log1p) — the recorded initial state is the object's own after that.

Per configuration <tag>, prefix `align_<tag>_`:
  pred_i pred_j conf_i conf_j                         the inputs [E,n,3] / [E,n]
  depth_log im_pose focal_log pp_raw pw_pose          the initial state
  losses                                              float(loss) of each of the 50 iterations (cosine schedule, lr 0.01)
  it<k>_<tensor>, k in 1, 10, 50                      the state after k iterations
  get_im_poses get_focals get_intrinsics get_pts3d get_depthmaps get_im_conf      the getters after the 50 iterations
Run:  python tests/golden/make_golden_align.py"""
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
from tests import global_align_util as gu  # noqa: E402

REF = ref_loader.REF


def _module(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


spec = importlib.util.spec_from_file_location("roma", os.path.join(HERE, "roma_standin.py"))
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
from dust3r.cloud_opt.base_opt import global_alignment_iter  # noqa: E402
from dust3r.utils.geometry import inv  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(1)
out = {}
for tag, (V, H, W, edges, sw) in gu.CONFIGS.items():
    a = gu.synthetic_problem(V, H, W, edges, gu.SEEDS[tag], norm_pw_scale=sw["norm_pw_scale"])
    E = len(edges)
    t = {k: torch.from_numpy(v) for k, v in a.items()}
    view1, view2 = {"idx": [i for i, j in edges]}, {"idx": [j for i, j in edges]}
    pred1 = {"pts3d": t["pred_i"].view(E, H, W, 3), "conf": t["conf_i"].view(E, H, W)}
    pred2 = {"pts3d_in_other_view": t["pred_j"].view(E, H, W, 3), "conf": t["conf_j"].view(E, H, W)}
    scene = PointCloudOptimizer(view1, view2, pred1, pred2, verbose=False)
    assert scene.edges == [tuple(e) for e in edges] and scene.n_imgs == V
    with torch.no_grad():
        scene.im_depthmaps.data[:] = t["depth_log"]
        scene.im_poses.data[:] = t["im_pose"]
        scene.im_focals.data[:] = t["focal_log"].view(V, 1)
        scene.im_pp.data[:] = t["pp_raw"]
        scene.pw_poses.data[:] = t["pw_pose"]
    if not sw["optimize_focals"]:
        scene.preset_focal([float(f) for f in scene.get_focals().detach().flatten()])
    if not sw["optimize_im_poses"]:
        scene.preset_pose([p.numpy() for p in scene.get_im_poses().detach()])
    assert scene.norm_pw_scale == sw["norm_pw_scale"]
    assert [scene.im_depthmaps.requires_grad, scene.im_poses.requires_grad, scene.im_focals.requires_grad, scene.pw_poses.requires_grad] == \
        [sw["optimize_depth"], sw["optimize_im_poses"], sw["optimize_focals"], sw["optimize_pw_poses"]]

    def state():
        return dict(depth_log=scene.im_depthmaps.detach().clone(), im_pose=scene.im_poses.detach().clone(),
                    focal_log=scene.im_focals.detach().clone().view(V), pp_raw=scene.im_pp.detach().clone(), pw_pose=scene.pw_poses.detach().clone())
    a.update({k: v.numpy() for k, v in state().items()})
    for k, v in a.items():
        out[f"align_{tag}_{k}"] = v.astype(np.float32)
    # global_alignment_loop's body (base_opt.py:326-349) with the iteration function called as it calls it
    params = [p for p in scene.parameters() if p.requires_grad]
    optimizer = torch.optim.Adam(params, lr=gu.LR, betas=(0.9, 0.9))
    losses = []
    for n in range(gu.NITER):
        loss, _ = global_alignment_iter(scene, n, gu.NITER, gu.LR, 1e-6, optimizer, "cosine")
        losses.append(loss)
        if n + 1 in gu.CHECKPOINTS:
            for k, v in state().items():
                out[f"align_{tag}_it{n + 1}_{k}"] = v.numpy().astype(np.float32)
    out[f"align_{tag}_losses"] = np.asarray(losses, dtype=np.float64)
    with torch.no_grad():
        out[f"align_{tag}_get_im_poses"] = scene.get_im_poses().numpy()
        out[f"align_{tag}_get_focals"] = scene.get_focals().numpy()
        out[f"align_{tag}_get_intrinsics"] = scene.get_intrinsics().numpy()
        out[f"align_{tag}_get_pts3d"] = torch.stack(scene.get_pts3d()).numpy()
        out[f"align_{tag}_get_depthmaps"] = torch.stack(scene.get_depthmaps()).numpy()
        out[f"align_{tag}_get_im_conf"] = torch.stack([c.detach() for c in scene.im_conf]).numpy()
        assert np.allclose(inv(scene.get_im_poses()).numpy() @ out[f"align_{tag}_get_im_poses"], np.eye(4), atol=1e-5)
    print(f"{tag}: loss {losses[0]:.6f} -> {losses[-1]:.6f}")

path = os.path.join(HERE, "align_vectors.npz")
np.savez_compressed(path, **out)
gu._G = None
print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")

# the yardsticks of tests/global_align_util.py: the reference's float32 run against the float64 restatement, and float32 CPU
# autograd of the restatement against float64
for tag in gu.CONFIGS:
    y, _, _ = gu.trajectory_yardstick(tag)
    print(tag, "trajectory yardstick:", {str(k): f"{v:.2e}" for k, v in y.items()})
    gu.check_restatement_equals_reference(tag)
    V, H, W, edges, sw, arrays = gu.golden_case(tag)
    g64, g32 = gu.restatement_grads(edges, H, W, arrays, sw, torch.float64), gu.restatement_grads(edges, H, W, arrays, sw, torch.float32)
    print(tag, "float32 autograd vs float64:", {k: f"{gu.rel(g32[k], g64[k]):.2e}" for k in g64})
