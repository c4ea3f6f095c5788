"""Checks of the device path renderer (render_path.render_pose_path / quantize_rgb8 / render_set, csrc/path.hip), shared by the
emulated (CPU) and the GPU test files."""
import contextlib
import copy
import ctypes
import faulthandler
import os

import numpy as np
import torch


@contextlib.contextmanager
def time_limit(seconds):
    """A step that has not finished after `seconds` ends the process with a traceback of where it stands — also when it waits
    inside a library call, where no Python exception could reach it."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


# ---------------------------------------------------------------------------------------------------- 8-bit conversion
def torch_rgb8(image: torch.Tensor) -> torch.Tensor:
    """torchvision.utils.save_image's quantisation, spelled out: [3,H,W] float -> [H,W,3] uint8"""
    return image.clone().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()


def rgb8_special_values() -> torch.Tensor:
    """Every value where the conversion could go wrong by one: k/255 and (k + 0.5)/255 (the rounding boundaries of the +0.5 and
    of the truncation) with their float32 neighbours on both sides, exact 0, 1, -0.0, large magnitudes, infinities."""
    k = torch.arange(256, dtype=torch.float64)
    out = []
    for base in ((k / 255).float(), ((k + 0.5) / 255).float()):
        out += [base, torch.nextafter(base, torch.full_like(base, 2.0)), torch.nextafter(base, torch.full_like(base, -2.0))]
    out.append(torch.tensor([0.0, 1.0, -0.0, 0.5, 1e30, -1e30, 3.4e38, -3.4e38, float("inf"), float("-inf"), 1e-45, -1e-45,
                             255.0, 256.0, 1.0000001, 0.99999994, 254.5 / 255, 255.5 / 255]))
    return torch.cat(out)


def rgb8_input(H, W, seed) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(3 * H * W, generator=g) * 1.4 - 0.2
    sp = rgb8_special_values()
    n = min(sp.numel(), x.numel())
    where = torch.randperm(x.numel(), generator=g)[:n]   # scattered over planes, rows and vector lanes
    x[where] = sp[torch.randperm(sp.numel(), generator=g)[:n]]
    return x.reshape(3, H, W)


def check_rgb8_equals_torch(dev, H, W, seeds=(0,)):
    from instantsplat_amd.render_path import quantize_rgb8
    for seed in seeds:
        x = rgb8_input(H, W, seed).to(dev)
        got, want = quantize_rgb8(x), torch_rgb8(x)
        assert got.shape == (H, W, 3) and got.dtype == torch.uint8
        bad = int((got != want).sum())
        print(f"rgb8 {H}x{W} seed {seed}: {bad} differing bytes of {got.numel()}")
        assert bad == 0


def check_rgb8_special_values_each(dev):
    """every special value once, in one 1 x n image (n a multiple of 4: the vector path; consecutive values fall on every lane
    position and in every plane), and a sample of them as 1 x 1 images (the plain path)"""
    from instantsplat_amd.render_path import quantize_rgb8
    sp = rgb8_special_values()
    n = (sp.numel() + 11) // 12 * 12
    x = torch.cat([sp, torch.zeros(n - sp.numel())]).reshape(3, 1, n // 3).to(dev)
    assert torch.equal(quantize_rgb8(x), torch_rgb8(x))
    for v in sp[::37].tolist() + [0.0, 1.0, float("inf")]:
        one = torch.tensor([v, 1.0 - v, 0.5 * v]).reshape(3, 1, 1).to(dev)
        assert torch.equal(quantize_rgb8(one), torch_rgb8(one)), v


def check_rgb8_nan_is_zero(dev, H=23, W=37):
    from instantsplat_amd.render_path import quantize_rgb8
    for h, w in ((H, W), (8, 16)):   # the plain and the vector path
        x = rgb8_input(h, w, 3)
        g = torch.Generator().manual_seed(9)
        nan = torch.rand(x.shape, generator=g) < 0.1
        nan[0, 0, 0] = nan[2, -1, -1] = True
        x[nan] = float("nan")
        got = quantize_rgb8(x.to(dev)).cpu()
        want = torch_rgb8(torch.where(nan, torch.zeros(()), x))   # (0 quantises to 0)
        assert torch.equal(got, want)
        assert int(got[nan.permute(1, 2, 0)].max()) == 0


def check_rgb8_misaligned_pointers_take_the_plain_path(dev):
    """A pixel count that is a multiple of 4 with an `img` that is not 16-byte aligned or an `out` that is not 4-byte aligned: the
    kernel must not use its vector loads / three-word stores.  Tensors from torch are always aligned, so the entry point is
    called with pointers into the middle of larger buffers; the bytes around the output must survive."""
    from instantsplat_amd import _lib
    H, W = 6, 8
    n = H * W
    x = rgb8_input(H, W, 7)
    want = torch_rgb8(x).reshape(-1)
    for img_off, out_off in ((1, 0), (0, 1), (3, 2), (2, 3), (0, 0)):   # floats / bytes
        src = torch.zeros(3 * n + 8, dtype=torch.float32)
        src[img_off:img_off + 3 * n] = x.reshape(-1)
        src = src.to(dev)
        dst = torch.full((3 * n + 16,), 0xCD, dtype=torch.uint8, device=dev)
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 4 == 0
        with _lib.on_device(dev):
            _lib.check(_lib.lib().mi355gs_rgb8_from_planar(_lib.stream_ptr(dev), H, W, src.data_ptr() + 4 * img_off, dst.data_ptr() + out_off),
                       "rgb8_from_planar")
        got = dst.cpu()
        assert torch.equal(got[out_off:out_off + 3 * n], want), (img_off, out_off)
        assert int((got[:out_off] != 0xCD).sum()) == 0 and int((got[out_off + 3 * n:] != 0xCD).sum()) == 0, (img_off, out_off)


def check_rgb8_rejects_bad_arguments():
    from instantsplat_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below must fail its checks first
    EINVAL = -1
    assert L.mi355gs_rgb8_from_planar(None, 4, 4, None, fake) == EINVAL
    assert L.mi355gs_rgb8_from_planar(None, 4, 4, fake, None) == EINVAL
    assert L.mi355gs_rgb8_from_planar(None, 0, 4, fake, fake) == EINVAL
    assert L.mi355gs_rgb8_from_planar(None, 4, 0, fake, fake) == EINVAL
    assert L.mi355gs_rgb8_from_planar(None, -1, 4, fake, fake) == EINVAL
    assert L.mi355gs_rgb8_from_planar(None, 65536, 65536, fake, fake) == EINVAL   # more pixels than an int indexes


# ---------------------------------------------------------------------------------------------------- scenes and paths
def small_scene(dev, Wm=12, Hm=10, W=48, H=32, degree=0, seed=11):
    """An untrained synthetic 3-view scene; for degree > 0 the higher SH bands get small random coefficients so that the
    view-direction term matters."""
    from instantsplat_amd.pose_tracking import freeze_gaussians
    from instantsplat_amd.synthetic import syn_pointmap
    from instantsplat_amd.train import setup_training
    st = setup_training(syn_pointmap(3, Wm, Hm, W, H, seed=seed), dev)
    g = st.gaussians
    freeze_gaussians(g)
    if degree > 0:
        gen = torch.Generator().manual_seed(seed + 100)
        g._features_rest.data.copy_((0.2 * torch.randn(g._features_rest.shape, generator=gen)).to(dev))
    g.active_sh_degree = degree
    for cam, gt in zip(st.cameras, st.gt_images):
        cam.original_image = gt
    return st


def keyframes(cameras) -> np.ndarray:
    """[V,4,4] float64 world-to-camera matrices of the cameras, as pose_optimized.npy holds them"""
    return np.stack([c.world_view_transform.t().double().cpu().numpy() for c in cameras])


def short_path(org_pose: np.ndarray, n_interp: int) -> np.ndarray:
    """interpolated_pose_path with a chosen number of poses per segment (the pieces called directly)"""
    from instantsplat_amd.camera_path import generate_interpolated_path
    segs = [generate_interpolated_path(org_pose[i:i + 2], n_interp) for i in range(len(org_pose) - 1)]
    path = np.concatenate(segs + [org_pose[-1][None, :3]], axis=0)
    out = np.tile(np.eye(4), (len(path), 1, 1))
    out[:, :3] = path
    return out


def path_views(st, poses44: np.ndarray, keep_images=True):
    """The cameras repeated along the path (load_cameras copies every camera it repeats: a long path of large views is given
    cameras without their ground-truth images)."""
    from instantsplat_amd.scene_io import load_cameras
    cams = [copy.copy(c) for c in st.cameras]
    if not keep_images:
        for c in cams:
            c.original_image = None
    return load_cameras(poses44, cams)


def view_pose(view, dev):
    from instantsplat_amd.pose_utils import get_tensor_from_camera
    return get_tensor_from_camera(view.world_view_transform.transpose(0, 1).cpu()).to(dev).float()


def eager_frames(views, st, poses=None) -> torch.Tensor:
    """The loop of reference render.py:85-93: a no-grad render() per view and the 8-bit conversion -> uint8 [N,H,W,3] (host)"""
    from instantsplat_amd.gaussian_renderer import render
    from instantsplat_amd.render_path import quantize_rgb8
    dev = st.gaussians.get_xyz.device
    out = []
    with torch.no_grad():
        for i, view in enumerate(views):
            pose = view_pose(view, dev) if poses is None else poses[i].to(dev).float()
            out.append(quantize_rgb8(render(view, st.gaussians, st.pipe, st.background, camera_pose=pose)["render"]).cpu())
    return torch.stack(out)


def assert_frames_equal(got: torch.Tensor, want: torch.Tensor, what: str):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.uint8, (got.shape, want.shape)
    per_frame = (got != want).flatten(1).sum(1)
    print(f"{what}: {int(per_frame.sum())} differing bytes in {int((per_frame > 0).sum())} of {got.shape[0]} frames")
    assert int(per_frame.sum()) == 0, [int(i) for i in torch.nonzero(per_frame).flatten()[:10]]


def exact_counts(views, st) -> list:
    """every frame's instance count from the tracker's count entry point"""
    from instantsplat_amd.pose_tracking import FusedPoseTracker
    dev = st.gaussians.get_xyz.device
    v0 = views[0]
    tr = FusedPoseTracker(st.gaussians, int(v0.image_width), int(v0.image_height), 1)
    out = [tr.count(v, int(st.gaussians.active_sh_degree), view_pose(v, dev)) for v in views]
    tr.close()
    return out


# ---------------------------------------------------------------------------------------------------- checks
def check_path_equals_eager(dev, st, views, pinned=False, what="path"):
    """frames[i] == quantize_rgb8(render(view_i, camera_pose=pose_i)) byte for byte; counts are the exact instance counts"""
    from instantsplat_amd.render_path import render_pose_path
    res = render_pose_path(views, st.gaussians, st.pipe, st.background, pinned=pinned)
    frames = res["frames"]
    v0 = views[0]
    assert tuple(frames.shape) == (len(views), int(v0.image_height), int(v0.image_width), 3) and frames.dtype == torch.uint8
    if pinned and dev.type == "cuda":
        assert frames.device.type == "cpu" and frames.is_pinned()
    else:
        assert frames.device == dev
    assert res["counts"].dtype == torch.int32 and res["counts"].shape == (len(views),)
    want = eager_frames(views, st)
    assert all(len(torch.unique(want[i])) > 16 for i in (0, len(views) // 2, len(views) - 1))   # not a comparison of blank frames
    assert_frames_equal(frames, want, what)
    return res, want


def check_counts_are_exact(st, views, res):
    assert res["counts"].tolist() == exact_counts(views, st)


def check_overflow_is_per_frame_and_rerun_repairs(dev, st, views, want):
    """A capacity between the smallest and the largest count: exactly the frames above it report so, the others are already
    right, and render_pose_path renders the flagged ones again."""
    from instantsplat_amd.render_path import FusedPathRenderer, render_pose_path
    import math
    counts = exact_counts(views, st)
    cap = sorted(counts)[len(counts) // 2 - 1]
    over = [c > cap for c in counts]
    assert any(over) and not all(over), counts
    v0 = views[0]
    W, H, N = int(v0.image_width), int(v0.image_height), len(views)
    poses = torch.stack([view_pose(v, dev) for v in views]).contiguous()
    frames = torch.zeros(N, H, W, 3, dtype=torch.uint8, device=dev)
    got = torch.zeros(N, dtype=torch.int32, device=dev)
    r = FusedPathRenderer(st.gaussians, W, H, cap)
    r.render(v0.projection_matrix, math.tan(v0.FoVx * 0.5), math.tan(v0.FoVy * 0.5), st.background, int(st.gaussians.active_sh_degree),
             poses, frames, got)
    got = got.cpu().tolist()
    r.close()
    assert got == counts                                  # the true count of every frame, overflowed or not
    assert [c > cap for c in got] == over                 # ... so the flag is per frame: a later frame that fits is not tainted
    fits = [i for i in range(N) if not over[i]]
    assert_frames_equal(frames.cpu()[fits], want[fits], "frames that fit a small capacity")
    res = render_pose_path(views, st.gaussians, st.pipe, st.background, capacity=cap)
    assert res["reruns"] == sum(over) and res["counts"].tolist() == counts
    assert_frames_equal(res["frames"], want, "after the rerun")


def check_subrange_writes_only_its_slots(dev, st, views, want):
    from instantsplat_amd.render_path import FusedPathRenderer
    import math
    v0 = views[0]
    W, H, N = int(v0.image_width), int(v0.image_height), len(views)
    assert N >= 5
    poses = torch.stack([view_pose(v, dev) for v in views]).contiguous()
    frames = torch.full((N, H, W, 3), 0xAB, dtype=torch.uint8, device=dev)
    counts = torch.full((N,), -7, dtype=torch.int32, device=dev)
    r = FusedPathRenderer(st.gaussians, W, H, 4 * max(exact_counts(views, st)) + 64)
    args = (v0.projection_matrix, math.tan(v0.FoVx * 0.5), math.tan(v0.FoVy * 0.5), st.background, int(st.gaussians.active_sh_degree), poses,
            frames, counts)
    r.render(*args, 1, 2)
    r.render(*args, 4, 0)   # nothing
    f, c = frames.cpu(), counts.cpu()
    for i in range(N):
        if i in (1, 2):
            assert torch.equal(f[i], want[i]) and int(c[i]) > 0, i
        else:
            assert int((f[i] != 0xAB).sum()) == 0 and int(c[i]) == -7, i
    r.render(*args, N - 1, 1)   # the last slot ends exactly at the end of the buffers
    assert torch.equal(frames.cpu()[N - 1], want[N - 1])
    import pytest
    for first, n in ((-1, 1), (0, N + 1), (N, 1), (2, -1)):
        with pytest.raises(ValueError):
            r.render(*args, first, n)
    r.close()


def check_projection_change_starts_a_group(dev, st, views):
    from instantsplat_amd.camera import Camera
    from instantsplat_amd.render_path import _groups, render_pose_path
    mixed = list(views[:2])
    for v in views[2:]:
        mixed.append(Camera(v.uid, v.world_view_transform.t().cpu(), v.FoVx * 0.8, v.FoVy * 0.8, int(v.image_width), int(v.image_height),
                            device=dev))
    assert _groups(mixed) == [(0, 2), (2, len(views))]
    assert _groups(list(views)) == [(0, len(views))]
    res = render_pose_path(mixed, st.gaussians, st.pipe, st.background)
    want = eager_frames(mixed, st)
    assert not torch.equal(want[2], eager_frames(views[2:3], st)[0])   # the other field of view is another image
    assert_frames_equal(res["frames"], want, "two groups")


def check_value_errors(dev, st, views):
    import pytest
    from instantsplat_amd.arguments import PipelineParams
    from instantsplat_amd.render_path import quantize_rgb8, render_pose_path
    g, bg = st.gaussians, st.background
    for pipe, kw in ((PipelineParams(convert_SHs_python=True), {}), (PipelineParams(compute_cov3D_python=True), {}),
                     (PipelineParams(), {"scaling_modifier": 0.5})):
        with pytest.raises(ValueError):
            render_pose_path(views, g, pipe, bg, **kw)
    with pytest.raises(ValueError):
        render_pose_path([], g, st.pipe, bg)
    with pytest.raises(ValueError):
        render_pose_path(views, g, st.pipe, bg, poses=torch.zeros(len(views) + 1, 7))
    with pytest.raises(ValueError):
        quantize_rgb8(torch.zeros(4, 8, 8, device=dev))
    with pytest.raises(RuntimeError):
        quantize_rgb8(torch.zeros(3, 8, 8, dtype=torch.float64, device=dev))


def check_entry_points_reject_bad_arguments():
    """Argument checks of the mi355gs_path_* entry points, before any HIP call (bogus device pointers are never touched)."""
    from instantsplat_amd import _lib
    L = _lib.lib()
    EINVAL = -1
    assert L.mi355gs_path_workspace_bytes(0, 32, 32, 100) == 0
    assert L.mi355gs_path_workspace_bytes(10, 0, 32, 100) == 0
    assert L.mi355gs_path_workspace_bytes(10, 32, -1, 100) == 0
    assert L.mi355gs_path_workspace_bytes(10, 32, 32, 0) == 0
    assert L.mi355gs_path_workspace_bytes(10, 32, 32, 100) > 3 * 32 * 32 * 4
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below must fail its checks first
    ok_args = [fake] * 6
    assert not L.mi355gs_path_create(0, 16, 32, 32, 100, *ok_args, fake)
    assert not L.mi355gs_path_create(10, 17, 32, 32, 100, *ok_args, fake)
    assert not L.mi355gs_path_create(10, 16, 32, 32, 0, *ok_args, fake)
    assert not L.mi355gs_path_create(10, 16, 32, 32, -5, *ok_args, fake)
    assert not L.mi355gs_path_create(10, 16, 0, 32, 100, *ok_args, fake)
    assert not L.mi355gs_path_create(10, 16, 32, 32, 100, *ok_args, None)
    for k in range(6):
        args = list(ok_args)
        args[k] = None
        assert not L.mi355gs_path_create(10, 16, 32, 32, 100, *args, fake), k
    h1 = L.mi355gs_path_create(10, 1, 32, 32, 100, fake, fake, None, fake, fake, fake, fake)   # no higher bands: f_rest may be null
    assert h1
    try:
        assert L.mi355gs_path_render(h1, None, 1, fake, 0.5, 0.5, fake, fake, 0, 1, fake, fake) == EINVAL   # degree 1 needs 4 coefficients
    finally:
        L.mi355gs_path_destroy(h1)
    h = L.mi355gs_path_create(10, 16, 32, 32, 100, *ok_args, fake)
    assert h
    try:
        run = lambda handle=h, deg=0, proj=fake, bg=fake, poses=fake, first=0, n=1, frames=fake, counts=fake: \
            L.mi355gs_path_render(handle, None, deg, proj, 0.5, 0.5, bg, poses, first, n, frames, counts)
        assert run(handle=None) == EINVAL
        for kw in ("proj", "bg", "poses", "frames", "counts"):
            assert run(**{kw: None}) == EINVAL, kw
        assert run(deg=-1) == EINVAL and run(deg=4) == EINVAL
        assert run(first=-1) == EINVAL and run(n=-1) == EINVAL
        assert run(first=2 ** 31 - 1, n=2) == EINVAL
        assert run(first=3, n=0) == 0              # nothing to enqueue: no launch either
    finally:
        L.mi355gs_path_destroy(h)
    h = L.mi355gs_path_create(10, 4, 32, 32, 100, *ok_args, fake)   # degree 1 at most
    try:
        assert L.mi355gs_path_render(h, None, 2, fake, 0.5, 0.5, fake, fake, 0, 1, fake, fake) == EINVAL
    finally:
        L.mi355gs_path_destroy(h)


def read_png(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def check_render_set_files(dev, st, views, want, tmp_path):
    """render_set writes renders/{idx:05d}.png holding exactly the frames' bytes, and gt/ only when the set is not "interp"."""
    from instantsplat_amd.render_path import quantize_rgb8, render_set
    N = len(views)
    names = [f"{i:05d}.png" for i in range(N)]
    for name, fused in (("interp", True), ("train", True), ("train_eager", False)):
        d = render_set(str(tmp_path), name, 30, views, st.gaussians, st.pipe, st.background, fused=fused)
        base = os.path.join(str(tmp_path), name, "ours_30")
        assert d == os.path.join(base, "renders") and sorted(os.listdir(d)) == names
        for i in range(N):
            assert np.array_equal(read_png(os.path.join(d, names[i])), want[i].numpy()), (name, i)
        gts = sorted(os.listdir(os.path.join(base, "gt")))
        if name == "interp":
            assert gts == []
        else:
            assert gts == names
            for i in range(N):
                gt = quantize_rgb8(views[i].original_image[0:3].to(dev).float().contiguous()).cpu().numpy()
                assert np.array_equal(read_png(os.path.join(base, "gt", names[i])), gt)
