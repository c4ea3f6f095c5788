"""Test-view pose tracking and the FPS benchmark — the second caller of `render()` in the reference
(reference render.py:99-186, `render_set_optimize`): Gaussians frozen, one 7-vector pose per test view
optimised by Adam (lr 3e-3 for t, 1e-3 for q, weight_decay 1e-4, cosine annealing to 1e-4), masked L1 loss
(reference utils/loss_utils.py:17-23, mask = render > 0), best-loss pose kept.

Only `dL/dmeans3D` and `dL/drotations` leave the rasterizer here; the fused pose kernel reduces them to the
seven pose gradients on the device, so one tracking iteration is ~15 kernel launches instead of ~150.
`optimize_view_pose_fused` (render_set_optimize(..., fused=True)) runs the whole loop of a view on the device instead.
"""
from __future__ import annotations

import os
import time
from typing import List

import torch

from . import _lib
from .diff_gaussian_rasterization import BinningPolicy
from .gaussian_renderer import render
from .handles import FrozenSceneHandle
from .pose_utils import get_tensor_from_camera


def l1_loss_mask(network_output, gt, mask):
    return (torch.abs(network_output - gt) * mask).sum() / mask.sum()


def freeze_gaussians(gaussians):
    for t in (gaussians._xyz, gaussians._features_dc, gaussians._features_rest, gaussians._opacity, gaussians._scaling,
              gaussians._rotation):
        t.requires_grad_(False)


def optimize_view_pose(view, gaussians, pipe, background, init_pose: torch.Tensor | None = None, num_iter: int = 500):
    """Returns dict(pose=[7], initial_loss, best_loss, render=[3,H,W]) for one view."""
    dev = gaussians.get_xyz.device
    if init_pose is None:
        init_pose = get_tensor_from_camera(view.world_view_transform.transpose(0, 1).cpu())
    camera_pose = init_pose.detach().to(dev).float()
    cam_T = camera_pose[-3:].clone().requires_grad_()
    cam_q = camera_pose[:4].clone().requires_grad_()
    optimizer = torch.optim.Adam([{"params": [cam_T], "lr": 0.003}, {"params": [cam_q], "lr": 0.001}], betas=(0.9, 0.999),
                                 weight_decay=1e-4)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=num_iter, eta_min=0.0001)
    cand_q, cand_T = cam_q.clone().detach(), cam_T.clone().detach()
    best = torch.full((), 1e20, device=dev)
    gt = view.original_image[0:3].to(dev)
    initial_loss = None
    for it in range(num_iter):
        rendering = render(view, gaussians, pipe, background, camera_pose=torch.cat([cam_q, cam_T]))["render"]
        mask = (rendering > 0.0).float()
        loss = l1_loss_mask(rendering, gt, mask)
        loss.backward()
        with torch.no_grad():
            optimizer.step()
            optimizer.zero_grad(set_to_none=True)
            if it == 0:
                initial_loss = float(loss)
            # keep the best pose without a host round trip (the reference compares on the host every iteration)
            better = loss < best
            best = torch.where(better, loss.detach(), best)
            cand_q = torch.where(better, cam_q.detach(), cand_q)
            cand_T = torch.where(better, cam_T.detach(), cand_T)
        scheduler.step()
    pose = torch.cat([cand_q, cand_T])
    with torch.no_grad():
        final = render(view, gaussians, pipe, background, camera_pose=pose)["render"]
    return dict(pose=pose, initial_loss=initial_loss, best_loss=float(best), render=final)


# ---- the same loop on the device (csrc/tracker.hip, include/mi355gs.h mi355gs_tracker_*): one library call enqueues a whole
# view's iterations, one read-back of the state block per view.

STATE_FLOATS, S_POSE, S_EXP_AVG, S_EXP_AVG_SQ, S_BEST, S_INITIAL, S_FLAG, S_COUNT, S_CAND = 40, 0, 8, 16, 24, 25, 26, 27, 32
_SCHEDULES = {}


def tracking_schedule(num_iter: int, dev) -> torch.Tensor:
    """[num_iter, 4] float32 per iteration: Adam's step size for t and for q (-lr / (1 - 0.9^step)) and sqrt(1 - 0.999^step), each
    formed in double as torch.optim.Adam forms them and rounded to fp32 once.  The learning rates come from a real
    CosineAnnealingLR (torch steps it in its recursive form), read at the moment optimize_view_pose's Adam step reads them."""
    key = (int(num_iter), str(dev))
    tab = _SCHEDULES.get(key)
    if tab is None:
        ps = [torch.zeros(1, requires_grad=True), torch.zeros(1, requires_grad=True)]
        opt = torch.optim.Adam([{"params": [ps[0]], "lr": 0.003}, {"params": [ps[1]], "lr": 0.001}], betas=(0.9, 0.999), weight_decay=1e-4)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=num_iter, eta_min=0.0001)
        rows = []
        for it in range(num_iter):
            step = float(it + 1)
            bc1, bc2 = 1 - 0.9 ** step, 1 - 0.999 ** step
            lr_t, lr_q = opt.param_groups[0]["lr"], opt.param_groups[1]["lr"]
            rows.append(((lr_t / bc1) * -1, (lr_q / bc1) * -1, bc2 ** 0.5, 0.0))
            opt.step()   # (no gradients: only keeps the scheduler's step-order check quiet)
            sched.step()
        tab = _SCHEDULES[key] = torch.tensor(rows, dtype=torch.float64).float().to(dev)
    return tab


class FusedPoseTracker(FrozenSceneHandle):
    """Handle of mi355gs_tracker_*: the frozen Gaussians' raw parameters, one image size and an instance capacity."""
    prefix, phrase = "tracker", "fused pose tracking"

    def count(self, view, sh_degree: int, pose: torch.Tensor) -> int:
        """Exact instance count of the view at `pose` (one blocking read)."""
        proj, tx, ty = self._camera(view, self.dev)
        pose = pose.detach().to(self.dev).float().contiguous()
        out = torch.zeros(1, dtype=torch.int32, device=self.dev)
        _lib.call(self.dev, "tracker_count", self._h, _lib.STREAM, int(sh_degree), proj, tx, ty, pose, out)
        return int(out[0])

    @staticmethod
    def initial_state(pose: torch.Tensor) -> torch.Tensor:
        st = torch.zeros(STATE_FLOATS, dtype=torch.float32, device=pose.device)
        st[S_POSE:S_POSE + 7] = pose
        st[S_CAND:S_CAND + 7] = pose
        st[S_BEST] = 1e20
        st[S_INITIAL] = float("nan")
        return st

    def run(self, view, background, sh_degree: int, state: torch.Tensor, num_iter: int, first_iter: int = 0, n_iters=None,
            traces=None):
        """Enqueues iterations first_iter .. first_iter + n_iters - 1 of a num_iter-iteration tracking run on `state`."""
        dev = self.dev
        n_iters = num_iter - first_iter if n_iters is None else n_iters
        proj, tx, ty = self._camera(view, dev)
        gt = view.original_image[0:3].to(dev).float().contiguous()
        if tuple(gt.shape) != (3, self.H, self.W):
            raise ValueError(f"ground-truth image of shape {tuple(gt.shape)}, the tracker renders {(3, self.H, self.W)}")
        bg = background.to(dev).float().contiguous()
        if bg.numel() != 3 or state.numel() != STATE_FLOATS or state.dtype != torch.float32 or state.device != dev:
            raise ValueError("background needs 3 floats and state the tracker's device block")
        sched = tracking_schedule(num_iter, dev)
        pt, lt, gt_ = (None, None, None) if traces is None else traces
        for t, n in ((pt, 7), (lt, 1), (gt_, 7)):
            if t is not None and (t.numel() != n * num_iter or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous()):
                raise ValueError("traces need float32 [num_iter, 7] / [num_iter] on the tracker's device")
        self._keep = (proj, gt, bg, sched)   # alive until the enqueued work has read them (the caller synchronises per view)
        _lib.call(dev, "tracker_run", self._h, _lib.STREAM, int(sh_degree), gt, proj, tx, ty, bg, sched, int(num_iter), int(first_iter),
                  int(n_iters), state, pt, lt, gt_)


def _state_word(st: torch.Tensor, i: int) -> int:
    return int(st[i:i + 1].view(torch.int32)[0])


def optimize_view_pose_fused(view, gaussians, pipe, background, init_pose: torch.Tensor | None = None, num_iter: int = 500,
                             record: bool = False, scaling_modifier: float = 1.0, capacity: int | None = None):
    """optimize_view_pose on the device: the whole loop in one library call, one read-back of the state per view.  Same keys
    (pose, initial_loss, best_loss, render — the last an ordinary no-grad render() at the best pose); record=True adds the
    traces `poses` [num_iter, 7] (the pose each render used), `losses` [num_iter] and `grads` [num_iter, 7] (d loss / d pose).
    capacity: instance capacity of the first attempt (default: the exact count at the initial pose, times
    BinningPolicy.slack, plus BinningPolicy.pad); a run that outgrows it is repeated from the initial pose with larger buffers."""
    if pipe.convert_SHs_python or pipe.compute_cov3D_python or scaling_modifier != 1.0:
        raise ValueError("fused pose tracking implements the default pipeline only (SH colours and covariance in the operator, "
                         "scaling_modifier 1)")
    if num_iter <= 0:
        raise ValueError("num_iter must be positive")
    dev = gaussians.get_xyz.device
    if init_pose is None:
        init_pose = get_tensor_from_camera(view.world_view_transform.transpose(0, 1).cpu())
    pose0 = init_pose.detach().to(dev).float().reshape(7).contiguous()
    W, H, D = int(view.image_width), int(view.image_height), int(gaussians.active_sh_degree)
    if capacity is None:
        probe = FusedPoseTracker(gaussians, W, H, 1)
        capacity = BinningPolicy.capacity_for(probe.count(view, D, pose0))
        probe.close()
    reruns = 0
    while True:
        tracker = FusedPoseTracker(gaussians, W, H, capacity)
        state = FusedPoseTracker.initial_state(pose0)
        traces = None
        if record:
            traces = (torch.empty(num_iter, 7, device=dev), torch.empty(num_iter, device=dev), torch.empty(num_iter, 7, device=dev))
        tracker.run(view, background, D, state, num_iter, traces=traces)
        st = state.cpu()   # the one read-back of the view
        tracker.close()
        if _state_word(st, S_FLAG) == 0:
            break
        reruns += 1
        capacity = BinningPolicy.regrown(_state_word(st, S_COUNT), capacity)
    pose = st[S_CAND:S_CAND + 7].to(dev)
    with torch.no_grad():
        final = render(view, gaussians, pipe, background, camera_pose=pose)["render"]
    out = dict(pose=pose, initial_loss=float(st[S_INITIAL]), best_loss=float(st[S_BEST]), render=final, reruns=reruns)
    if record:
        out.update(poses=traces[0], losses=traces[1], grads=traces[2])
    return out


def render_set_optimize(views: List, gaussians, pipe, background, num_iter: int = 500, init_poses=None, fused: bool = False):
    freeze_gaussians(gaussians)
    track = optimize_view_pose_fused if fused else optimize_view_pose
    out = []
    for i, view in enumerate(views):
        out.append(track(view, gaussians, pipe, background, None if init_poses is None else init_poses[i], num_iter))
    return out


def render_test_set(model_path, iteration, views: List, gaussians, pipe, background, num_iter: int = 500, fused: bool = True,
                    init_poses=None, png: str = "pil") -> dict:
    """The file-writing form of reference render.py:99-170: every view tracked by `render_set_optimize`, its final render and
    `view.original_image[0:3]` quantised as torchvision.utils.save_image does (render_path.quantize_rgb8) and written to
    <model_path>/test/ours_<iteration>/renders/<image_name>.png and .../gt/<image_name>.png.  png="device" encodes both sets of
    files on the GPU (instantsplat_amd/png.py) from the stacks that are already there; "pil" is the reference's writer.
    -> dict(results = the tracker's per-view dicts,
            frames = {"ours_<iteration>": [dict(names = file names, renders = uint8 [n,H,W,3], gts = uint8 [n,H,W,3]), ...]}:
            the two frame stacks as device tensors, one entry per image size — what `metrics.evaluate(model_path, frames=...)`
            scores without reading the files back)."""
    from .render_path import _check_png, _save_png, quantize_rgb8
    device_png = _check_png(png)
    views = list(views)
    method = f"ours_{iteration}"
    base = os.path.join(str(model_path), "test", method)
    render_dir, gts_dir = os.path.join(base, "renders"), os.path.join(base, "gt")
    os.makedirs(render_dir, exist_ok=True)
    os.makedirs(gts_dir, exist_ok=True)
    results = render_set_optimize(views, gaussians, pipe, background, num_iter=num_iter, init_poses=init_poses, fused=fused)
    dev = gaussians.get_xyz.device
    by_size = {}
    for view, res in zip(views, results):
        name = f"{view.image_name}.png"
        render8 = quantize_rgb8(res["render"].detach().float().contiguous())
        gt8 = quantize_rgb8(view.original_image[0:3].to(dev).float().contiguous())
        grp = by_size.setdefault(tuple(render8.shape), dict(names=[], renders=[], gts=[]))
        grp["names"].append(name); grp["renders"].append(render8); grp["gts"].append(gt8)
    groups = [dict(names=g["names"], renders=torch.stack(g["renders"]), gts=torch.stack(g["gts"])) for g in by_size.values()]
    for g in groups:   # one device-to-host copy per stack
        for stack, d in ((g["renders"], render_dir), (g["gts"], gts_dir)):
            if device_png:
                from .png import write_png_files
                write_png_files([os.path.join(d, name) for name in g["names"]], stack)
                continue
            for name, frame in zip(g["names"], stack.cpu().numpy()):
                _save_png(os.path.join(d, name), frame)
    return dict(results=results, frames={method: groups})


def measure_fps(view, gaussians, pipe, background, pose, frames: int = 1000) -> dict:
    """reference render.py:172-186: `frames` renders of one view, sorted, the middle 80 % averaged.  The reference
    relies on its operator's internal blocking read-back for the timing to mean anything; here every frame is
    followed by an explicit synchronize."""
    dev = gaussians.get_xyz.device
    times = []
    with torch.no_grad():
        for _ in range(frames):
            t0 = time.perf_counter()
            render(view, gaussians, pipe, background, camera_pose=pose)
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
    times.sort()
    lo, hi = frames // 10, frames - frames // 10
    mid = times[lo:hi] if hi > lo else times
    mean = sum(mid) / len(mid)
    return dict(fps=1.0 / mean, ms_per_frame=1e3 * mean)
