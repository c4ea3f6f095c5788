"""Rendering a list of camera poses to 8-bit frames — the reference's `render_set` (render.py:78-97) and its `--infer_video`
stage (:233-248): the train-view renders of a trained scene, and the fly-through along the interpolated path of its poses.

`render_pose_path` runs the whole list on the device (csrc/path.hip, include/mi355gs.h mi355gs_path_*): one library call
enqueues every frame of a group of views — posed projection, binning, render-only compositing, 8-bit conversion straight into the
[N,H,W,3] frame array — with one read-back of the per-frame instance counts at the end.  `quantize_rgb8` is the conversion
alone (torchvision.utils.save_image's arithmetic), `render_set` writes the files, `render_interpolated` is the third stage of
the reference's run_infer.sh after `train.training()`.
"""
from __future__ import annotations

import copy
import math
import os
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from .camera_path import save_interpolate_pose
from .diff_gaussian_rasterization import BinningPolicy
from .gaussian_renderer import render
from .handles import FrozenSceneHandle
from .pose_utils import get_tensor_from_camera
from .scene_io import load_cameras


def quantize_rgb8(image: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """[3,H,W] float32 -> [H,W,3] uint8 as torchvision.utils.save_image quantises: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8),
    a NaN giving 0.  One launch (mi355gs_rgb8_from_planar)."""
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"quantize_rgb8 takes a [3,H,W] image, got {tuple(image.shape)}")
    image = _lib.f32c(image.detach())
    dev = _lib.require_device(image)
    H, W = int(image.shape[1]), int(image.shape[2])
    if out is None:
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or not out.is_contiguous():
        raise ValueError(f"quantize_rgb8 writes a contiguous uint8 [{H},{W},3] tensor")
    _lib.call(dev, "rgb8_from_planar", _lib.STREAM, H, W, image, out)
    return out


class FusedPathRenderer(FrozenSceneHandle):
    """Handle of mi355gs_path_*: the frozen Gaussians' raw parameters, one image size and an instance capacity."""
    prefix, phrase = "path", "path rendering"

    def render(self, proj: torch.Tensor, tanfovx: float, tanfovy: float, background: torch.Tensor, sh_degree: int, poses: torch.Tensor,
               frames: torch.Tensor, counts: torch.Tensor, first: int = 0, n: int | None = None):
        """Enqueues poses first .. first + n - 1 of `poses` [N,7] into frames[i] (uint8 [N,H,W,3] on the device, or pinned host
        memory) and counts[i] (int32 [N] on the device).  Nothing is waited for."""
        dev = self.dev
        N = int(poses.shape[0])
        n = N - first if n is None else n
        if poses.dim() != 2 or poses.shape[1] != 7 or poses.dtype != torch.float32 or poses.device != dev or not poses.is_contiguous():
            raise ValueError("poses must be contiguous float32 [N,7] on the renderer's device")
        if first < 0 or n < 0 or first + n > N:
            raise ValueError(f"frames {first} .. {first + n - 1} of a path of {N} poses")
        if frames.dtype != torch.uint8 or tuple(frames.shape) != (N, self.H, self.W, 3) or not frames.is_contiguous():
            raise ValueError(f"frames must be a contiguous uint8 [{N},{self.H},{self.W},3] tensor")
        if frames.device != dev and not (dev.type == "cuda" and frames.device.type == "cpu" and frames.is_pinned()):
            raise ValueError("frames must live on the renderer's device or in pinned host memory")
        if counts.dtype != torch.int32 or counts.numel() != N or counts.device != dev or not counts.is_contiguous():
            raise ValueError("counts must be contiguous int32 [N] on the renderer's device")
        proj = proj.to(dev).float().contiguous()
        bg = background.to(dev).float().contiguous()
        if proj.numel() != 16 or bg.numel() != 3:
            raise ValueError("the projection matrix needs 16 floats and the background 3")
        self._keep = (proj, bg, poses)   # alive until the enqueued work has read them (the caller synchronises per group)
        _lib.call(dev, "path_render", self._h, _lib.STREAM, int(sh_degree), proj, float(tanfovx), float(tanfovy), bg, poses, int(first), int(n),
                  frames, counts)


def _stacked_on_host(tensors) -> torch.Tensor:
    """The views' per-camera matrices as one host tensor: ONE device-to-host copy for the whole list, not one per view."""
    return torch.stack([t.detach() for t in tensors]).cpu()


def _groups(views):
    """[(start, stop)] of consecutive views that share the image size, the projection matrix and the field of view"""
    proj = _stacked_on_host([v.projection_matrix for v in views]).reshape(len(views), -1).tolist() if views else []
    out, start, key = [], 0, None
    for i, v in enumerate(views):
        k = (int(v.image_width), int(v.image_height), tuple(proj[i]), float(v.FoVx), float(v.FoVy))
        if i and k != key:
            out.append((start, i))
            start = i
        key = k
    if views:
        out.append((start, len(views)))
    return out


def _frame_buffer(N, H, W, dev, pinned):
    if pinned and dev.type == "cuda":   # the conversion kernel stores into it directly: no device-to-host copy of the frames
        return torch.empty(N, H, W, 3, dtype=torch.uint8, pin_memory=True)
    return torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)


def render_pose_path(views: List, gaussians, pipe, background, poses: torch.Tensor | None = None, capacity: int | None = None,
                     pinned: bool = False, scaling_modifier: float = 1.0) -> dict:
    """The frames of reference render.py:85-93 for a whole camera list, on the device.
    views: cameras as `load_cameras` returns them; poses [N,7]: the pose of every frame (default: each view's own,
    get_tensor_from_camera(view.world_view_transform.T) as render.py:86).  Consecutive views with one image size, projection matrix
    and field of view form a group, rendered through one handle by one library call.
    capacity: instance capacity of a group's first attempt (default: the exact count at the group's first pose, times
    BinningPolicy.slack, plus BinningPolicy.pad); after the one read-back of the counts, only the frames that outgrew it are
    rendered again, through a handle sized from the largest count.
    Host traffic of a call: the views' projection matrices in one copy and (with default poses) their view matrices in another,
    both before anything is enqueued; one blocking read of a single count per group when the capacity is probed; the read-back of
    the counts per group.
    pinned: the frames are written into pinned host memory by the kernels (returned as a CPU tensor) instead of device memory.
    -> dict(frames = uint8 [N,H,W,3] (a list of per-group tensors if the groups differ in size), counts = int32 [N] on the host,
            reruns = frames rendered twice)."""
    if pipe.convert_SHs_python or pipe.compute_cov3D_python or scaling_modifier != 1.0:
        raise ValueError("path rendering implements the default pipeline only (SH colours and covariance in the operator, "
                         "scaling_modifier 1)")
    views = list(views)
    if not views:
        raise ValueError("render_pose_path needs at least one view")
    dev = gaussians.get_xyz.device
    N = len(views)
    if poses is None:
        w2c = _stacked_on_host([v.world_view_transform for v in views]).transpose(1, 2)
        poses = torch.stack([get_tensor_from_camera(m) for m in w2c])
    poses = poses.detach().to(dev).float().reshape(-1, 7).contiguous()
    if poses.shape[0] != N:
        raise ValueError(f"{poses.shape[0]} poses for {N} views")
    D = int(gaussians.active_sh_degree)
    out_frames, out_counts, reruns = [], [], 0
    for start, stop in _groups(views):
        view = views[start]
        W, H = int(view.image_width), int(view.image_height)
        proj, tx, ty = view.projection_matrix, math.tan(view.FoVx * 0.5), math.tan(view.FoVy * 0.5)
        gposes = poses[start:stop].contiguous()
        n = stop - start
        frames = _frame_buffer(n, H, W, dev, pinned)
        counts = torch.zeros(n, dtype=torch.int32, device=dev)
        cap = capacity
        if cap is None:   # the exact count of the first pose: one frame through a handle of the smallest size
            probe = FusedPathRenderer(gaussians, W, H, 1)
            probe.render(proj, tx, ty, background, D, gposes, frames, counts, 0, 1)
            cap = BinningPolicy.capacity_for(int(counts[0]))
            probe.close()
        todo = None   # frames to render: all of them first, then those whose count exceeded the capacity
        while True:
            renderer = FusedPathRenderer(gaussians, W, H, cap)
            if todo is None:
                renderer.render(proj, tx, ty, background, D, gposes, frames, counts)
            else:
                for i in todo:
                    renderer.render(proj, tx, ty, background, D, gposes, frames, counts, i, 1)
            host_counts = counts.cpu()   # the one read-back of the group (it also orders the frames before the host reads them)
            renderer.close()
            todo = [i for i in (range(n) if todo is None else todo) if int(host_counts[i]) > cap]
            if not todo:
                break
            reruns += len(todo)
            cap = BinningPolicy.regrown(int(host_counts.max()), cap)
        out_frames.append(frames)
        out_counts.append(host_counts)
    same = all(f.shape[1:] == out_frames[0].shape[1:] for f in out_frames)
    frames = out_frames[0] if len(out_frames) == 1 else (torch.cat(out_frames) if same else out_frames)
    return dict(frames=frames, counts=torch.cat(out_counts), reruns=reruns)


def _save_png(path: str, hwc: np.ndarray):
    from PIL import Image
    Image.fromarray(hwc).save(path)   # (what torchvision.utils.save_image does with the bytes it has quantised)


def _check_png(png: str) -> bool:
    """the `png=` argument of the file-writing stages -> True for the device encoder (instantsplat_amd/png.py)"""
    if png not in ("pil", "device"):
        raise ValueError(f'png must be "pil" (PIL on the host) or "device" (instantsplat_amd.png on the GPU), got {png!r}')
    return png == "device"


def _write_png_device(paths: List[str], frames: List[torch.Tensor]):
    """uint8 [H,W,3] device frames to files through the device encoder: one encode per image size"""
    from .png import write_png_files
    by_size = {}
    for path, frame in zip(paths, frames):
        grp = by_size.setdefault(tuple(frame.shape), ([], []))
        grp[0].append(path); grp[1].append(frame)
    for group_paths, group in by_size.values():
        write_png_files(group_paths, torch.stack(group))


def render_set(model_path, name: str, iteration, views: List, gaussians, pipe, background, fused: bool = True, png: str = "pil", *,
               frames_out: Optional[list] = None) -> str:
    """reference render.py:78-97: <model_path>/<name>/ours_<iteration>/renders/{idx:05d}.png for every view and, unless name is
    "interp", gt/{idx:05d}.png.  fused=False renders frame by frame with render() and quantize_rgb8.  png="device" encodes the
    files on the GPU (instantsplat_amd/png.py: the same pixels in larger files, without PIL's host time per frame); "pil" is
    the reference's writer.  frames_out: a list that receives the rendered uint8 [H,W,3] frames as they stand in device memory,
    in view order (the video of `render_interpolated` is made of them).  Returns the renders' directory."""
    device_png = _check_png(png)
    views = list(views)
    base = os.path.join(str(model_path), name, f"ours_{iteration}")
    render_dir, gts_dir = os.path.join(base, "renders"), os.path.join(base, "gt")
    os.makedirs(render_dir, exist_ok=True)
    os.makedirs(gts_dir, exist_ok=True)
    to_host = (lambda f: f) if device_png else (lambda f: f.cpu().numpy())
    if fused:
        frames = render_pose_path(views, gaussians, pipe, background)["frames"]
        frames = frames if isinstance(frames, list) else [frames]
        if frames_out is not None:
            frames_out.extend(f for group in frames for f in group)
        frames = [f for group in frames for f in to_host(group)]
    else:
        frames = []
        with torch.no_grad():
            for view in views:
                pose = get_tensor_from_camera(view.world_view_transform.transpose(0, 1).cpu()).to(gaussians.get_xyz.device)
                frame = quantize_rgb8(render(view, gaussians, pipe, background, camera_pose=pose)["render"])
                if frames_out is not None:
                    frames_out.append(frame)
                frames.append(to_host(frame))
    if device_png:
        _write_png_device([os.path.join(render_dir, f"{idx:05d}.png") for idx in range(len(views))], frames)
        if name != "interp":
            gts = [quantize_rgb8(view.original_image[0:3].to(gaussians.get_xyz.device).float().contiguous()) for view in views]
            _write_png_device([os.path.join(gts_dir, f"{idx:05d}.png") for idx in range(len(views))], gts)
        return render_dir
    for idx, (view, frame) in enumerate(zip(views, frames)):
        _save_png(os.path.join(render_dir, f"{idx:05d}.png"), frame)
        if name != "interp":
            gt = view.original_image[0:3].to(gaussians.get_xyz.device).float().contiguous()
            _save_png(os.path.join(gts_dir, f"{idx:05d}.png"), quantize_rgb8(gt).cpu().numpy())
    return render_dir


def images_to_video(image_folder: str, output_video_path: str, fps: int = 30) -> bool:
    """reference render.py:59-76, if imageio is installed; False (and nothing written) if it is not."""
    try:
        import imageio
    except ImportError:
        return False
    images = [imageio.imread(os.path.join(image_folder, f)) for f in sorted(os.listdir(image_folder))
              if f.endswith((".png", ".jpg", ".jpeg", ".JPG", ".PNG"))]
    imageio.mimwrite(output_video_path, images, fps=fps)
    return True


def write_mjpeg_video(path: str, frames: List[torch.Tensor], quality=90, fps=30) -> None:
    """uint8 [H,W,3] device frames of one size -> an AVI file of 4:2:0 JPEG frames encoded on the device (instantsplat_amd/jpeg.py,
    instantsplat_amd/video.py)"""
    from .jpeg import encode_jpeg_rgb8
    from .video import write_mjpeg_avi
    if not frames or any(f.shape != frames[0].shape for f in frames):
        raise ValueError("a video needs at least one frame, and all frames of one size")
    enc = encode_jpeg_rgb8(torch.stack(list(frames)), quality=quality, subsampling="4:2:0")
    H, W = (int(s) for s in frames[0].shape[:2])
    write_mjpeg_avi(path, enc["stream"], enc["offsets"], W, H, fps=fps)


def render_interpolated(model_path, iteration, n_views: int, train_cameras: List, gaussians, pipe, background, fused: bool = True,
                        png: str = "pil", video: str = "imageio", video_quality=90) -> str:
    """The `--infer_video` stage (reference render.py:233-248): pose_interpolated.npy from the optimised poses, the training cameras
    repeated along it, every pose rendered to interp/ours_<iteration>/renders/, and interp_<n_views>_view.mp4 beside that
    directory if imageio is installed (otherwise a message says that the video was skipped).  png: as for `render_set`.
    video="mjpeg" writes interp_<n_views>_view.avi instead, 30 frames per second of Motion-JPEG at `video_quality` (4:2:0), encoded
    on the device from the frames the path renderer left there — the PNG files are written as `png` says, and not read back.
    Returns the frame directory."""
    _check_png(png)
    if video not in ("imageio", "mjpeg"):
        raise ValueError(f'video must be "imageio" (an mp4 through imageio, if installed) or "mjpeg" (an AVI encoded on the GPU), got {video!r}')
    pose_file = save_interpolate_pose(model_path, iteration, n_views)
    cams = [copy.copy(c) for c in train_cameras]
    for c in cams:   # load_cameras copies every camera it repeats along the path; the "interp" set writes no ground truth
        c.original_image = None
    views = load_cameras(np.load(pose_file), cams)
    if video == "mjpeg":
        device_frames: list = []
        render_dir = render_set(model_path, "interp", iteration, views, gaussians, pipe, background, fused=fused, png=png, frames_out=device_frames)
        avi = os.path.join(str(model_path), "interp", f"ours_{iteration}", f"interp_{n_views}_view.avi")
        write_mjpeg_video(avi, device_frames, quality=video_quality, fps=30)
        print(f"wrote {len(views)} frames and {avi}")
        return render_dir
    render_dir = render_set(model_path, "interp", iteration, views, gaussians, pipe, background, fused=fused, png=png)
    video = os.path.join(str(model_path), "interp", f"ours_{iteration}", f"interp_{n_views}_view.mp4")
    if images_to_video(render_dir, video):
        print(f"wrote {len(views)} frames and {video}")
    else:
        print(f"wrote {len(views)} frames to {render_dir}; the video was skipped (imageio is not installed)")
    return render_dir
