"""Checks of the device pose tracker (pose_tracking.optimize_view_pose_fused, csrc/tracker.hip), shared by the emulated
(CPU) and the GPU test files."""
import ctypes
import math
import os

import numpy as np
import torch

from tests.ops_util import bound


def _golden_setup(dev):
    from instantsplat_amd.camera import Camera
    from instantsplat_amd.scene import GaussianModel
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_vectors.npz"))
    T = lambda k: torch.from_numpy(G[k])
    _, _, W, H, _ = [int(x) for x in G["loop_config"]]
    g = GaussianModel(3)
    for n in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        setattr(g, n, torch.nn.Parameter(T("loop_final" + n).clone().to(dev)))
    view = Camera(0, T("track_w2c_guess"), float(G["loop_cam_fov"][1, 0]), float(G["loop_cam_fov"][1, 1]), W, H, image=T("track_gt")).to(dev)
    return G, T, g, view


def check_fused_tracking_matches_reference_function(dev):
    """The fused tracker vs the reference's own `render_set_optimize` (tests/golden `track_*`, the set-up and bounds of
    ops_util.check_pose_tracking_matches_reference_function): the pose of every render — the iterations' from the pose trace,
    the final render's from the result — the losses, the best pose and its rendering."""
    from instantsplat_amd.arguments import PipelineParams
    from instantsplat_amd.pose_tracking import freeze_gaussians, optimize_view_pose_fused
    G, T, g, view = _golden_setup(dev)
    freeze_gaussians(g)
    n = int(G["track_iters"])
    res = optimize_view_pose_fused(view, g, PipelineParams(), torch.zeros(3, device=dev), num_iter=n, record=True)
    poses = torch.cat([res["poses"].cpu(), res["pose"].cpu()[None]])
    ref_seq = T("track_pose_sequence")
    assert poses.shape == ref_seq.shape, (poses.shape, ref_seq.shape)
    bound("fused_tracking_ref/pose_sequence", (poses - ref_seq).abs().max(), 2e-5)
    losses = torch.from_numpy(G["track_losses"]).double()
    assert res["losses"].shape == (n,)
    bound("fused_tracking_ref/losses", ((res["losses"].cpu().double() - losses).abs() / losses).max(), 1e-4)
    bound("fused_tracking_ref/initial_loss", abs(res["initial_loss"] - G["track_losses"][0]) / G["track_losses"][0], 1e-4)
    bound("fused_tracking_ref/best_loss", abs(res["best_loss"] - G["track_losses"].min()) / G["track_losses"].min(), 2e-4)
    bound("fused_tracking_ref/optimal_pose", (res["pose"].cpu() - T("track_optimal_pose")).abs().max(), 2e-5)
    bound("fused_tracking_ref/final_render", (res["render"].cpu() - T("track_final_render")).abs().max(), 2e-4)
    assert res["reruns"] == 0


def synthetic_view(dev, Wm=12, W=32, degree=0, seed=11, shift=(0.03, -0.02, 0.04)):
    """A small synthetic scene (the set-up of ops_util.check_pose_tracking), view 1 with a perturbed initial pose; for
    degree > 0 the higher SH bands get small random coefficients so that the view-direction term matters."""
    from instantsplat_amd.pose_utils import get_tensor_from_camera
    from instantsplat_amd.synthetic import syn_pointmap
    from instantsplat_amd.train import setup_training
    from instantsplat_amd.pose_tracking import freeze_gaussians
    st = setup_training(syn_pointmap(3, Wm, Wm, W, W, seed=seed), dev)
    g = st.gaussians
    freeze_gaussians(g)
    if degree > 0:
        gen = torch.Generator().manual_seed(seed + 100)
        g._features_rest.data.copy_((0.2 * torch.randn(g._features_rest.shape, generator=gen)).to(dev))
    g.active_sh_degree = degree
    view = st.cameras[1]
    view.original_image = st.gt_images[1]
    init = get_tensor_from_camera(view.world_view_transform.transpose(0, 1).cpu()).clone()
    init[4:] += torch.tensor(shift)
    return st, g, view, init


def eager_with_poses(view, g, pipe, bg, init, num_iter):
    """optimize_view_pose with the pose of every render recorded (the golden test's way: monkeypatching pose_tracking.render)."""
    from instantsplat_amd import pose_tracking
    poses = []
    real_render = pose_tracking.render

    def recording_render(cam, pc, pipe_, bg_, camera_pose=None, **k):
        poses.append(camera_pose.detach().cpu().clone())
        return real_render(cam, pc, pipe_, bg_, camera_pose=camera_pose, **k)

    pose_tracking.render = recording_render
    try:
        res = pose_tracking.optimize_view_pose(view, g, pipe, bg, init, num_iter)
    finally:
        pose_tracking.render = real_render
    return res, torch.stack(poses)


def check_fused_equals_eager(dev, degree, num_iter=10, Wm=12, W=32, pose_bound=1e-5, loss_bound=1e-5, tag=""):
    from instantsplat_amd.pose_tracking import optimize_view_pose_fused
    st, g, view, init = synthetic_view(dev, Wm, W, degree)
    ref, ref_poses = eager_with_poses(view, g, st.pipe, st.background, init, num_iter)
    res = optimize_view_pose_fused(view, g, st.pipe, st.background, init, num_iter, record=True)
    poses = torch.cat([res["poses"].cpu(), res["pose"].cpu()[None]])
    assert poses.shape == ref_poses.shape
    label = f"fused_vs_eager{tag}/deg{degree}"
    bound(label + "/pose_sequence", (poses - ref_poses).abs().max(), pose_bound)
    bound(label + "/initial_loss", abs(res["initial_loss"] - ref["initial_loss"]) / ref["initial_loss"], loss_bound)
    bound(label + "/best_loss", abs(res["best_loss"] - ref["best_loss"]) / ref["best_loss"], loss_bound)
    bound(label + "/final_render", (res["render"] - ref["render"]).abs().max(), 1e-4)
    assert ref["best_loss"] < ref["initial_loss"]   # the run moved somewhere: the comparison is not of two idle loops
    return res, ref


def check_entry_points_reject_bad_arguments():
    """Argument checks of the mi355gs_tracker_* entry points, before any HIP call (bogus device pointers are never touched)."""
    from instantsplat_amd import _lib
    L = _lib.lib()
    EINVAL = -1
    assert L.mi355gs_tracker_workspace_bytes(0, 32, 32, 100) == 0
    assert L.mi355gs_tracker_workspace_bytes(10, 0, 32, 100) == 0
    assert L.mi355gs_tracker_workspace_bytes(10, 32, 32, 0) == 0
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below must fail its checks first
    ok_args = [fake] * 6
    assert not L.mi355gs_tracker_create(0, 16, 32, 32, 100, *ok_args, fake)
    assert not L.mi355gs_tracker_create(10, 17, 32, 32, 100, *ok_args, fake)
    assert not L.mi355gs_tracker_create(10, 16, 32, 32, 0, *ok_args, fake)
    assert not L.mi355gs_tracker_create(10, 16, 32, 32, 100, *ok_args, None)
    for k in range(6):
        args = list(ok_args)
        args[k] = None
        assert not L.mi355gs_tracker_create(10, 16, 32, 32, 100, *args, fake), k
    # f_rest may be null only without higher bands
    h1 = L.mi355gs_tracker_create(10, 1, 32, 32, 100, fake, fake, None, fake, fake, fake, fake)
    assert h1
    L.mi355gs_tracker_destroy(h1)
    h = L.mi355gs_tracker_create(10, 16, 32, 32, 100, *ok_args, fake)
    assert h
    try:
        run = lambda handle=h, deg=0, gt=fake, proj=fake, bg=fake, sched=fake, num_iter=10, first=0, n=10, state=fake: \
            L.mi355gs_tracker_run(handle, None, deg, gt, proj, 0.5, 0.5, bg, sched, num_iter, first, n, state, None, None, None)
        assert run(handle=None) == EINVAL
        for kw in ("gt", "proj", "bg", "sched", "state"):
            assert run(**{kw: None}) == EINVAL, kw
        assert run(deg=-1) == EINVAL and run(deg=4) == EINVAL
        assert run(n=-1) == EINVAL
        assert run(first=-1) == EINVAL
        assert run(first=5, n=6) == EINVAL          # first_iter + n_iters > num_iter
        assert run(num_iter=0, n=0) == EINVAL
        assert run(first=10, n=0) == 0              # nothing to enqueue: no launch either
        cnt = lambda handle=h, deg=0, proj=fake, pose=fake, out=fake: L.mi355gs_tracker_count(handle, None, deg, proj, 0.5, 0.5, pose, out)
        assert cnt(handle=None) == EINVAL
        for kw in ("proj", "pose", "out"):
            assert cnt(**{kw: None}) == EINVAL, kw
        assert cnt(deg=4) == EINVAL
    finally:
        L.mi355gs_tracker_destroy(h)
    h = L.mi355gs_tracker_create(10, 4, 32, 32, 100, *ok_args, fake)   # degree 1 at most
    try:
        assert L.mi355gs_tracker_run(h, None, 2, fake, fake, 0.5, 0.5, fake, fake, 10, 0, 1, fake, None, None, None) == EINVAL
    finally:
        L.mi355gs_tracker_destroy(h)


def check_pipe_flags_rejected(dev):
    import pytest
    from instantsplat_amd.arguments import PipelineParams
    from instantsplat_amd.pose_tracking import optimize_view_pose_fused
    st, g, view, init = synthetic_view(dev, 8, 16, 0)
    for pipe, kw in ((PipelineParams(convert_SHs_python=True), {}), (PipelineParams(compute_cov3D_python=True), {}),
                     (PipelineParams(), {"scaling_modifier": 0.5})):
        with pytest.raises(ValueError):
            optimize_view_pose_fused(view, g, pipe, st.background, init, 2, **kw)


class deterministic:
    """Deterministic-backward mode for a block (process-wide knob, restored on exit)."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        from instantsplat_amd.diff_gaussian_rasterization import set_deterministic
        self.old = set_deterministic(self.on)

    def __exit__(self, *a):
        from instantsplat_amd.diff_gaussian_rasterization import set_deterministic
        set_deterministic(self.old)


def check_tracking_gain_and_eager_agreement(dev, num_iter=120, Wm=64, W=128):
    """ops_util.check_pose_tracking's set-up (test_ops_gpu.py's sizes): the fused tracker pulls the pose in like the eager loop
    (best <= 0.7 x initial), and in deterministic mode both start from the same loss and render the same first 20 poses."""
    from instantsplat_amd.pose_tracking import optimize_view_pose_fused
    st, g, view, init = synthetic_view(dev, Wm, W, 0)
    res = optimize_view_pose_fused(view, g, st.pipe, st.background, init, num_iter)
    assert res["best_loss"] <= 0.7 * res["initial_loss"], (res["initial_loss"], res["best_loss"])
    assert res["render"].shape == (3, W, W)
    with deterministic():
        fused = optimize_view_pose_fused(view, g, st.pipe, st.background, init, 20, record=True)
        ref, ref_poses = eager_with_poses(view, g, st.pipe, st.background, init, 20)
    bound("fused_tracking_c/initial_loss", abs(fused["initial_loss"] - ref["initial_loss"]) / ref["initial_loss"], 1e-5)
    bound("fused_tracking_c/pose_sequence_20", (fused["poses"].cpu() - ref_poses[:20]).abs().max(), 1e-5)


def _ulps(a: torch.Tensor, b: torch.Tensor) -> int:
    ia = a.detach().cpu().float().contiguous().view(torch.int32).long()
    ib = b.detach().cpu().float().contiguous().view(torch.int32).long()
    # map the sign-magnitude float order onto the integers
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int((ia - ib).abs().max())


def check_adam_teacher_forced(dev, num_iter=40, Wm=24, W=64):
    """The device Adam against torch.optim.Adam + CosineAnnealingLR (the eager loop's optimizer, on tensors of the same device):
    the fused run's recorded d_pose replayed from the same initial pose must give the same pose trace to 2 ulp."""
    from instantsplat_amd.pose_tracking import optimize_view_pose_fused
    st, g, view, init = synthetic_view(dev, Wm, W, 0)
    res = optimize_view_pose_fused(view, g, st.pipe, st.background, init, num_iter, record=True)
    pose = init.to(dev).float()
    cam_T = pose[-3:].clone().requires_grad_()
    cam_q = pose[:4].clone().requires_grad_()
    opt = torch.optim.Adam([{"params": [cam_T], "lr": 0.003}, {"params": [cam_q], "lr": 0.001}], betas=(0.9, 0.999), weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=num_iter, eta_min=0.0001)
    grads = res["grads"]
    assert bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0
    replay = [torch.cat([cam_q, cam_T]).detach().clone()]
    for it in range(num_iter):
        cam_q.grad = grads[it, :4].clone()
        cam_T.grad = grads[it, 4:].clone()
        opt.step()
        sched.step()
        replay.append(torch.cat([cam_q, cam_T]).detach().clone())
    replay = torch.stack(replay)
    worst = _ulps(res["poses"], replay[:num_iter])
    assert worst <= 2, worst
    # the best pose is one of the post-step poses
    assert any(bool((res["pose"] == replay[k]).all()) for k in range(1, num_iter + 1)) or _ulps(res["pose"], replay[-1]) <= 2


def check_overflow_rerun(dev, num_iter=12, Wm=24, W=64):
    """A first attempt with a tiny instance capacity sets the sticky flag; the wrapper reruns with grown buffers and returns what
    a correctly sized run returns — bit for bit in deterministic mode."""
    from instantsplat_amd.pose_tracking import FusedPoseTracker, S_FLAG, S_COUNT, S_POSE, S_BEST, optimize_view_pose_fused, _state_word
    st, g, view, init = synthetic_view(dev, Wm, W, 0)
    with deterministic():
        tr = FusedPoseTracker(g, W, W, 64)
        state = FusedPoseTracker.initial_state(init.to(dev).float())
        tr.run(view, st.background, 0, state, num_iter)
        s = state.cpu()
        tr.close()
        assert _state_word(s, S_FLAG) == 1 and _state_word(s, S_COUNT) > 64
        assert bool((s[S_POSE:S_POSE + 7] == init.float()).all()) and float(s[S_BEST]) == float(torch.tensor(1e20))   # nothing committed
        a = optimize_view_pose_fused(view, g, st.pipe, st.background, init, num_iter, record=True)
        b = optimize_view_pose_fused(view, g, st.pipe, st.background, init, num_iter, record=True, capacity=64)
    assert a["reruns"] == 0 and b["reruns"] >= 1
    for k in ("pose", "poses", "losses", "grads", "render"):
        assert torch.equal(a[k], b[k]), k
    assert a["initial_loss"] == b["initial_loss"] and a["best_loss"] == b["best_loss"]


def check_deterministic_runs_identical(dev, num_iter=30, Wm=24, W=64):
    from instantsplat_amd.pose_tracking import optimize_view_pose_fused
    st, g, view, init = synthetic_view(dev, Wm, W, 1)
    with deterministic():
        a = optimize_view_pose_fused(view, g, st.pipe, st.background, init, num_iter, record=True)
        b = optimize_view_pose_fused(view, g, st.pipe, st.background, init, num_iter, record=True)
    for k in ("pose", "poses", "losses", "grads", "render"):
        assert torch.equal(a[k], b[k]), k
    assert a["initial_loss"] == b["initial_loss"] and a["best_loss"] == b["best_loss"]


def check_empty_view(dev, num_iter=6, Wm=12, W=32):
    """Camera moved behind every Gaussian: nothing is rendered, every mask is empty, the loss is NaN — the eager loop keeps
    the initial pose as the best (1e20 is never beaten by a NaN) while weight decay still moves the rendered poses."""
    from instantsplat_amd.pose_tracking import optimize_view_pose_fused
    st, g, view, init = synthetic_view(dev, Wm, W, 0)
    init = init.clone()
    init[6] -= 100.0
    ref, ref_poses = eager_with_poses(view, g, st.pipe, st.background, init, num_iter)
    res = optimize_view_pose_fused(view, g, st.pipe, st.background, init, num_iter, record=True)
    assert math.isnan(ref["initial_loss"]) and math.isnan(res["initial_loss"])
    assert res["best_loss"] == ref["best_loss"] == float(torch.tensor(1e20))
    assert torch.equal(res["pose"].cpu(), ref["pose"].cpu())
    assert bool(torch.isnan(res["losses"]).all())
    assert float(res["grads"].abs().max()) == 0.0
    bound("fused_tracking_empty/pose_sequence", (torch.cat([res["poses"].cpu(), res["pose"].cpu()[None]]) - ref_poses).abs().max(), 1e-7)
    assert torch.equal(res["render"], ref["render"])
