"""Test-view pose tracking rate on the C3 scene (3 views, 196,608 Gaussians, 512x512): the eager loop
(pose_tracking.optimize_view_pose, one autograd render + torch Adam per iteration) against the device tracker
(optimize_view_pose_fused, one library call per view), 500 iterations each, alternated twice, a synchronize around every timed
window.  Prints one JSON line.  --fused-only: one fused run (for a kernel trace of the loop).  Measurement helper, not product
code."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from instantsplat_amd import train  # noqa: E402
from instantsplat_amd.arguments import OptimizationParams  # noqa: E402
from instantsplat_amd.pose_tracking import freeze_gaussians, optimize_view_pose, optimize_view_pose_fused  # noqa: E402
from instantsplat_amd.pose_utils import get_tensor_from_camera  # noqa: E402
from instantsplat_amd.synthetic import syn_pointmap  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--train", type=int, default=200, help="one-call training iterations before tracking")
ap.add_argument("--fused-only", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")
st = train.setup_training(syn_pointmap(3, 256, 256, 512, 512, seed=0), dev,
                          opt=OptimizationParams(iterations=10 ** 9, pp_optimizer=True, optim_pose=True))
for _ in range(a.train):
    train.train_iteration(st, fused_step=True)
train.release_trainer(st)
torch.cuda.synchronize()
g = st.gaussians
freeze_gaussians(g)
view = st.cameras[1]
view.original_image = st.gt_images[1]
init = get_tensor_from_camera(view.world_view_transform.transpose(0, 1).cpu()).clone()
init[4:] += torch.tensor([0.03, -0.02, 0.04])
paths = {"eager": optimize_view_pose, "fused": optimize_view_pose_fused}
order = ["fused"] if a.fused_only else ["eager", "fused", "eager", "fused"]
rates, res = {"eager": [], "fused": []}, {}
for name in order:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = paths[name](view, g, st.pipe, st.background, init, a.iters)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rates[name].append(a.iters / dt)
    res[name] = r
out = {"scene": "C3", "gaussians": int(g._xyz.shape[0]), "W": 512, "H": 512, "iters": a.iters, "sh_degree": int(g.active_sh_degree),
       "iters_per_sec_fused": max(rates["fused"]), "iters_per_sec_fused_runs": rates["fused"],
       "ms_per_iter": 1e3 / max(rates["fused"]), "fused_best_loss": res["fused"]["best_loss"],
       "fused_initial_loss": res["fused"]["initial_loss"]}
if not a.fused_only:
    out.update(iters_per_sec_eager=max(rates["eager"]), iters_per_sec_eager_runs=rates["eager"], ms_per_iter_eager=1e3 / max(rates["eager"]),
               speedup=max(rates["fused"]) / max(rates["eager"]), eager_best_loss=res["eager"]["best_loss"],
               eager_initial_loss=res["eager"]["initial_loss"],
               pose_max_abs_diff=float((res["fused"]["pose"] - res["eager"]["pose"]).abs().max()))
print(json.dumps(out), flush=True)
