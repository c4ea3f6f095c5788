"""The tail of the init stage — reference init_geo.py:61-129, the part between `compute_global_alignment` and the directory
train.py opens: confidence-aware ranking, co-visibility pruning of the aligned pointmaps (utils/sfm_utils.py:342-432,
`compute_co_vis_masks`), the boolean compaction of points, colours and confidences (`save_points3D`, :250-316), the initial test
poses (:87-111) and the files of `sparse_<n>/0` and `sparse_<n>/1`.

The inputs are arrays — pointmaps, depth maps, confidences, intrinsics, poses, images — that any aligner can hand over; MASt3R,
DUSt3R and the global aligner themselves are out of scope.  The masks and the compaction run on the device (csrc/init.hip,
include/mi355gs.h mi355gs_pointmap_stats / mi355gs_covis_masks / mi355gs_compact_pointmaps): six kernel dispatches for a whole
scene, where the reference loops over the views in float64 numpy.  There is no CPU fallback.

  co_visibility_masks   `compute_co_vis_masks`: bool [V,H,W], True = co-visible with a better-ranked view, redundant
  confidence_ranking    init_geo.py:61-70: views by descending mean confidence (host)
  compact_pointmaps     `save_points3D`:264-277: the kept points, 8-bit colours and confidences, in view-major row-major order
  initial_test_poses    init_geo.py:87-111: poses for the held-out views, interpolated or sampled from the training poses (host)
  init_from_pointmaps   the stage: statistics -> ranking -> masks -> compaction -> files -> a trainable InitScene

Not reproduced: `max_pts_num` (the confidence-weighted random downsampling of `save_points3D`:280-292 draws from np.random and
never triggers at its default of 1.5e12), and the files train.py never reads (*.bin, confidence.npy, points3D_all.npy,
overlapping_masks_<n>/)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._frames import device_of, to_device

MAX_VIEWS = 256                    # include/mi355gs.h: V of one call
MAX_ELEMENTS = 2 ** 31 - 1         # ... and V H W
REFERENCE_MAX_PTS_NUM = 150 * 10 ** 10   # utils/sfm_utils.py:250, the default of `save_points3D`


def _as_tensor(x, dtype, what):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
    return t


def _check_maps(depthmaps, pointmaps=None, confidences=None, images=None, intrinsics=None, w2c=None):
    if depthmaps.dim() != 3 or min(depthmaps.shape) <= 0:
        raise ValueError(f"depthmaps must be a non-empty [V,H,W] array, got {tuple(depthmaps.shape)}")
    V, H, W = (int(s) for s in depthmaps.shape)
    if V > MAX_VIEWS or V * H * W > MAX_ELEMENTS:
        raise ValueError(f"{V} views of {H} x {W}: the library takes V <= {MAX_VIEWS} and V H W <= 2^31 - 1")
    for t, shape, what in ((pointmaps, (V, H, W, 3), "pointmaps"), (confidences, (V, H, W), "confidences"), (images, (V, H, W, 3), "images"),
                           (intrinsics, (V, 3, 3), "intrinsics"), (w2c, (V, 4, 4), "w2c")):
        if t is None:
            continue
        if what == "pointmaps" and tuple(t.shape) == (V, H * W, 3):
            continue   # the aligner's flat form; same memory
        if tuple(t.shape) != shape:
            raise ValueError(f"{what} must be {list(shape)}, got {list(t.shape)}")
    return V, H, W


def _check_order(order, V):
    order = [int(o) for o in np.asarray(order).reshape(-1)]
    if sorted(order) != list(range(V)):
        raise ValueError(f"order must be a permutation of 0 .. {V - 1}, got {order}")
    return order


def _pointmap_stats(depthmaps, confidences, dev):
    """-> (stats float64 [V,3] on the device: min depth, max depth, confidence sum; overlap uint8 [V,H,W], cleared)"""
    V, H, W = (int(s) for s in depthmaps.shape)
    scratch = _lib.scratch(dev, "pointmap_stats_scratch_bytes", V, H, W,
                           what=f"mi355gs_pointmap_stats does not take {V} views of {H} x {W} (include/mi355gs.h: the limits)")
    stats = torch.empty(V, 3, dtype=torch.float64, device=dev)
    overlap = torch.empty(V, H, W, dtype=torch.uint8, device=dev)   # cleared by the statistics pass
    _lib.call(dev, "pointmap_stats", _lib.STREAM, V, H, W, depthmaps, confidences, overlap, scratch, stats)
    return stats, overlap


def _covis_masks(order, pointmaps, depthmaps, intrinsics, w2c, stats, depth_threshold, overlap, dev):
    import ctypes
    V, H, W = (int(s) for s in depthmaps.shape)
    _lib.call(dev, "covis_masks", _lib.STREAM, V, H, W, (ctypes.c_int32 * V)(*order), pointmaps, depthmaps, intrinsics, w2c, stats,
              float(depth_threshold), overlap)


def co_visibility_masks(order, depthmaps, pointmaps, intrinsics, w2c, depth_threshold=0.1) -> torch.Tensor:
    """reference utils/sfm_utils.py:375-415 `compute_co_vis_masks(sorted_conf_indices, depthmaps, pointmaps, camera_intrinsics,
    extrinsics_w2c, image_sizes, depth_threshold)`: -> bool [V,H,W] on the device, True = the pixel of that view also sees a
    point of a view ranked before it at a consistent (normalised) depth — co-visible, redundant.  The first view of `order` is
    never marked.  All arrays float32: depthmaps [V,H,W], pointmaps [V,H,W,3] (or [V,H*W,3]), intrinsics [V,3,3], w2c [V,4,4];
    device tensors are used in place, CPU tensors and numpy arrays take one copy each.  Three kernel dispatches, no
    synchronisation.  The arithmetic is the reference's (projection in double from the float32 inputs, depths normalised and
    compared in float32): the masks are equal to its, pixel for pixel."""
    depthmaps, pointmaps = _as_tensor(depthmaps, torch.float32, "depthmaps"), _as_tensor(pointmaps, torch.float32, "pointmaps")
    intrinsics, w2c = _as_tensor(intrinsics, torch.float32, "intrinsics"), _as_tensor(w2c, torch.float32, "w2c")
    V, H, W = _check_maps(depthmaps, pointmaps=pointmaps, intrinsics=intrinsics, w2c=w2c)
    order = _check_order(order, V)
    dev = device_of((depthmaps, pointmaps, intrinsics, w2c))
    depthmaps, pointmaps, intrinsics, w2c = (to_device(t, dev) for t in (depthmaps, pointmaps, intrinsics, w2c))
    stats, overlap = _pointmap_stats(depthmaps, depthmaps, dev)   # (the confidence sums are not needed here)
    _covis_masks(order, pointmaps, depthmaps, intrinsics, w2c, stats, depth_threshold, overlap, dev)
    return overlap.view(torch.bool)


def confidence_ranking(conf_sums, H: int, W: int) -> np.ndarray:
    """reference init_geo.py:63-64: `np.argsort(confs.mean(axis=(1, 2)))[::-1]` — the views by descending mean confidence.
    conf_sums: the per-view sums of the statistics pass (accumulated in double; the reference's float32 mean carries its own
    rounding, so two views whose means agree to float32 precision may rank either way in either implementation)."""
    avg = np.asarray(conf_sums, dtype=np.float64).reshape(-1) / (float(H) * float(W))
    return np.argsort(avg)[::-1].copy()


def compact_pointmaps(pointmaps, images, confidences, overlap=None):
    """reference utils/sfm_utils.py:264-277: over the V H W elements in view-major, row-major order, those whose `overlap` is
    False (overlap None: all of them) -> (points float32 [M,3], rgb8 uint8 [M,3] = (uint8)(image * 255.f), confidence float32
    [M,1], M).  overlap: bool or uint8 [V,H,W] on the device.  Three kernel dispatches; M reaches the host through a word of
    pinned memory the scan kernel stores into, read after one stream synchronisation — the only one."""
    pointmaps, images = _as_tensor(pointmaps, torch.float32, "pointmaps"), _as_tensor(images, torch.float32, "images")
    confidences = _as_tensor(confidences, torch.float32, "confidences")
    n = int(confidences.numel())
    if n <= 0 or n > MAX_ELEMENTS or int(pointmaps.numel()) != 3 * n or int(images.numel()) != 3 * n:
        raise ValueError(f"compact_pointmaps takes n <= 2^31 - 1 elements: confidences [n], pointmaps and images [n,3]; got "
                         f"{list(confidences.shape)}, {list(pointmaps.shape)}, {list(images.shape)}")
    if overlap is not None:
        if not isinstance(overlap, torch.Tensor) or overlap.dtype not in (torch.bool, torch.uint8) or int(overlap.numel()) != n:
            raise ValueError("overlap must be a bool or uint8 tensor with one element per point")
    dev = device_of((pointmaps, images, confidences) + ((overlap,) if overlap is not None else ()))
    pointmaps, images, confidences = (to_device(t, dev) for t in (pointmaps, images, confidences))
    if overlap is not None:
        overlap = to_device(overlap, dev)
    scratch = _lib.scratch(dev, "compact_scratch_bytes", n, what=f"mi355gs_compact_pointmaps does not take {n} elements")
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    rgb8 = torch.empty(n, 3, dtype=torch.uint8, device=dev)
    conf = torch.empty(n, 1, dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    word = torch.full((1,), -1, dtype=torch.int32, pin_memory=(dev.type == "cuda"))
    _lib.call(dev, "compact_pointmaps", _lib.STREAM, n, overlap, pointmaps, images, confidences, scratch, points, rgb8, conf, count, word)
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()
    M = int(word[0])
    if not 0 <= M <= n:
        raise RuntimeError(f"compact_pointmaps: the count word holds {M} for {n} elements")
    return points[:M], rgb8[:M], conf[:M], M


def initial_test_poses(w2c_train, n_test: int) -> np.ndarray:
    """reference init_geo.py:87-111: [n_test,4,4] initial poses for the held-out views from the [n_train,4,4] training poses —
    with fewer training than test views, n_test // (n_train - 1) + 1 interpolated poses per pair of consecutive training poses
    (the two-keyframe case of `camera_path.generate_interpolated_path`) and the last training pose, sampled at
    linspace(0, len - 1, n_test) truncated to int; otherwise the training poses at those indices.  Host; float32 or float64 poses
    in (the aligner's are float32), float64 out."""
    from .camera_path import _poses_from_tracks, _sample_tracks, _tracks_from_keyframes
    w2c_train = np.asarray(w2c_train)
    if w2c_train.dtype not in (np.float32, np.float64):
        w2c_train = w2c_train.astype(np.float64)
    n_test = int(n_test)
    if w2c_train.ndim != 3 or w2c_train.shape[1:] != (4, 4) or w2c_train.shape[0] < 1 or n_test < 1:
        raise ValueError(f"initial_test_poses takes [n_train,4,4] poses and n_test >= 1, got {w2c_train.shape} and {n_test}")
    n_train = w2c_train.shape[0]
    if n_train >= n_test:
        return w2c_train[np.linspace(0, n_train - 1, n_test, dtype=int)].astype(np.float64)
    if n_train < 2:
        raise ValueError("one training pose cannot be interpolated to more test poses")
    n_interp = n_test // (n_train - 1) + 1
    # generate_interpolated_path(poses=w2c[i:i+2], n_interp): the three track points are formed in the poses' own precision (the
    # aligner's float32), the chord between them in double — as the reference's numpy expressions and scipy's fit do
    path = [_poses_from_tracks(_sample_tracks(_tracks_from_keyframes(w2c_train[i:i + 2], .1).astype(np.float64), n_interp, 5, .03))
            for i in range(n_train - 1)]
    path = np.concatenate(path + [w2c_train[-1][:3, :].reshape(1, 3, 4).astype(np.float64)], axis=0)
    out = np.tile(np.eye(4), (n_test, 1, 1))
    out[:, :3, :] = path[np.linspace(0, path.shape[0] - 1, n_test, dtype=int)]
    return out


def init_from_pointmaps(source_path, n_views, images, pointmaps, depthmaps, confidences, intrinsics, w2c, focals, org_size, *,
                        co_vis_dsp=True, depth_threshold=0.01, conf_aware_ranking=False, test_names=None, n_test=0,
                        max_pts_num=REFERENCE_MAX_PTS_NUM, image_names=None, image_files=None) -> dict:
    """The stage (reference init_geo.py:61-129 with the scripts' `--co_vis_dsp --conf_aware_ranking`), from the aligner's arrays —
    all float32: images [V,H,W,3] in [0,1], pointmaps [V,H,W,3] (or [V,H*W,3]), depthmaps / confidences [V,H,W], intrinsics
    [V,3,3], w2c [V,4,4] world-to-camera, focals [V] (or [V,1]); org_size = (width, height) of the photographs.

      1. statistics of the depth maps and confidences (2 dispatches, which also clear the masks);
      2. the ranking: `confidence_ranking` of the confidence sums with conf_aware_ranking — the one read-back (V x 3 doubles)
         before the count M — else 0 .. V-1 and no read-back;
      3. the co-visibility masks (1 dispatch); with depth_threshold <= 0 they are skipped and nothing is pruned (init_geo.py:74-79);
      4. the compaction (3 dispatches; everything is kept with co_vis_dsp=False) and the read of M;
      5. sparse_<n>/0 through `scene_io.write_init_scene`: images.txt, cameras.txt as `save_intrinsics` writes it (the FIRST
         view's focal for every view, scaled to org_size, principal point at the centre), points3D.ply and confidence_dsp.npy
         from the compacted tensors; images/<name> are `image_files` copied (the photographs), or without them the aligner's
         H x W images as PNG;
      6. with n_test > 0, sparse_<n>/1: `initial_test_poses` under `test_names`, the same camera for every view.
    source_path None: nothing is written (and no scene is loaded).

    -> dict(points [M,3], rgb8 [M,3], confidence [M,1] on the device; keep_masks bool [V,H,W] (None when the masks were skipped);
            order; pts_num = the numbers of pts_num.txt; test_poses; scene = the `scene_io.InitScene` of the written directory whose
            points, colours and confidence_lr are the device tensors — the PLY is not read back — or None).
    max_pts_num below the reference's default is refused: that downsampling is not implemented."""
    from . import scene_io
    from .scene import confidence_to_lr_modifiers
    if max_pts_num is None or max_pts_num < REFERENCE_MAX_PTS_NUM:
        raise ValueError(f"max_pts_num = {max_pts_num}: the confidence-weighted random downsampling of save_points3D is not "
                         f"implemented (out of scope); only the reference's default of {REFERENCE_MAX_PTS_NUM}, which never triggers, is taken")
    images, pointmaps = _as_tensor(images, torch.float32, "images"), _as_tensor(pointmaps, torch.float32, "pointmaps")
    depthmaps, confidences = _as_tensor(depthmaps, torch.float32, "depthmaps"), _as_tensor(confidences, torch.float32, "confidences")
    intrinsics, w2c = _as_tensor(intrinsics, torch.float32, "intrinsics"), _as_tensor(w2c, torch.float32, "w2c")
    V, H, W = _check_maps(depthmaps, pointmaps, confidences, images, intrinsics, w2c)
    if int(n_views) != V:
        raise ValueError(f"n_views = {n_views} but the arrays hold {V} views")
    focal0 = float(np.asarray(focals.detach().cpu() if isinstance(focals, torch.Tensor) else focals, dtype=np.float64).reshape(-1)[0])
    org_w, org_h = (int(s) for s in org_size)
    if org_w <= 0 or org_h <= 0 or not focal0 > 0:
        raise ValueError(f"org_size = {org_size}, focal = {focal0}: positive sizes and focal expected")
    n_test = int(n_test)
    if n_test > 0 and (test_names is None or len(test_names) != n_test):
        raise ValueError(f"n_test = {n_test} needs {n_test} test_names")
    dev = device_of((images, pointmaps, depthmaps, confidences, intrinsics, w2c))
    w2c_host = w2c.detach().cpu().numpy()
    images, pointmaps, depthmaps, confidences, intrinsics, w2c = (to_device(t, dev) for t in (images, pointmaps, depthmaps, confidences, intrinsics, w2c))

    stats, overlap = _pointmap_stats(depthmaps, confidences, dev)
    order = [int(o) for o in confidence_ranking(stats[:, 2].cpu().numpy(), H, W)] if conf_aware_ranking else list(range(V))
    pruned = depth_threshold > 0
    if pruned:
        _covis_masks(order, pointmaps, depthmaps, intrinsics, w2c, stats, depth_threshold, overlap, dev)
    points, rgb8, conf, M = compact_pointmaps(pointmaps, images, confidences, overlap if (pruned and co_vis_dsp) else None)
    total = V * H * W
    pts_num = {"depth_threshold": depth_threshold, "vanilla": total, "co_mask_dsp": M, "ratio": M / total}
    test_poses = initial_test_poses(w2c_host, n_test) if n_test > 0 else None
    out = dict(points=points, rgb8=rgb8, confidence=conf, keep_masks=(overlap == 0) if pruned else None, order=order, pts_num=pts_num,
               test_poses=test_poses, scene=None)
    if source_path is None:
        return out

    source_path = str(source_path)
    colors = (rgb8.double() / 255.0).float()   # what the loader makes of the PLY's bytes: u1 / 255.0 in double, then float32
    camera = (org_w, org_h, focal0 * (org_w / W), focal0 * (org_h / H))   # save_intrinsics: focal * scale_factor_x, focal * scale_factor_y
    names = list(image_names) if image_names is not None else [f"{v:04d}.png" for v in range(V)]
    if len(names) != V or (image_files is not None and len(image_files) != V):
        raise ValueError(f"{V} views need {V} image_names / image_files")
    stored = list(image_files) if image_files is not None else [images[v].permute(2, 0, 1) for v in range(V)]
    scene_io.write_init_scene(source_path, list(w2c_host.astype(np.float64)), None, stored, points, colors, conf, names=names, subdir="0", n_views=V,
                              cameras=[camera] * V)
    if n_test > 0:
        scene_io.write_init_scene(source_path, list(test_poses), None, None, None, None, None, names=list(test_names), subdir="1",
                                  n_views=V, cameras=[camera] * n_test)
    out["scene"] = scene_io.load_init_scene(source_path, V, device=dev, pointcloud=(points, colors, confidence_to_lr_modifiers(conf)))
    return out
