"""ORACLE — TEST INFRASTRUCTURE.  One iteration of test-view pose tracking (reference render.py:124-159, `render_set_optimize`)
in any float dtype: the frozen Gaussians' raw parameters and the 7-vector pose -> loss, dL/dpose and the per-Gaussian terms of it.

  pose        means_cam = R(q / |q|) xyz + t, rot_cam = q (x) rot           (pose_ref.forward)
  rasterizer  oracle/gs_ref at `sh_degree`, identity view, campos 0, the camera's projection matrix
  loss        mask = img > 0, loss = sum(|img - gt| m) / sum(m)             (reference utils/loss_utils.py:17-23)
  backward    dL/dmeans_cam and dL/drot_cam -> c[P,7] (pose_ref.pose_terms); dL/dpose = sum_i c[i]

In float64 this is the yardstick; in float32 it is the restatement whose distance from float64 sets the 2.5x term of a limit.
Generalises tests/ops_util.oracle_frame_grads (training loss, pose from a table) to the tracker's loss and a bare pose."""
import math

import torch

from oracle import gs_ref, pose_ref
from oracle.raster_torch import RasterSettings


def frame(params, pose, cam, gt, bg, sh_degree, dtype):
    """params: name -> tensor (xyz, f_dc, f_rest, opacity, scaling, rotation; the raw parameters of GaussianModel), pose [7],
    cam: a Camera (FoVx, FoVy, image size, projection_matrix), gt [3,H,W], bg [3].  -> dict(loss, d_pose [7], c [P,7], image)"""
    cpu = lambda t: t.detach().cpu().to(dtype)
    xyz, rot, pose = cpu(params["xyz"]), cpu(params["rotation"]), cpu(pose).reshape(7)
    with torch.no_grad():
        means, rots, scales, opac = pose_ref.forward(xyz, rot, cpu(params["scaling"]), cpu(params["opacity"]), pose)
    means, rots = means.clone().requires_grad_(True), rots.clone().requires_grad_(True)
    shs = torch.cat([cpu(params["f_dc"]), cpu(params["f_rest"])], dim=1)
    st = RasterSettings(int(cam.image_height), int(cam.image_width), math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), cpu(bg).reshape(3),
                        1.0, torch.eye(4, dtype=dtype), cpu(cam.projection_matrix), int(sh_degree), torch.zeros(3, dtype=dtype), False, False)
    with torch.enable_grad():
        img, _ = gs_ref.rasterize(means, torch.zeros_like(means, requires_grad=True), opac, st, shs=shs, scales=scales, rotations=rots)
        mask = (img > 0).to(dtype)
        loss = (torch.abs(img - cpu(gt)) * mask).sum() / mask.sum()
        loss.backward()
    c = pose_ref.pose_terms(xyz, rot, pose, means.grad, rots.grad)
    return dict(loss=loss.detach(), d_pose=c.sum(0), c=c, image=img.detach())
