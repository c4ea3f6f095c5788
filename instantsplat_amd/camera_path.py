"""Interpolated camera paths — the host side of the reference's `render.py --infer_video` stage.

  generate_interpolated_path   the signature and result of reference utils/camera_utils.py:127-182: a path through keyframe
                               poses, interpolated as three moving points per camera and rebuilt into look-at poses
  interpolated_pose_path       what reference render.py:36-56 (`save_interpolate_pose`) stores: int(10 * 30 / n_views) poses per
                               pair of consecutive keyframes, then the last keyframe, each padded to 4x4
  save_interpolate_pose        the same with the files: pose/ours_<it>/pose_optimized.npy in, pose_interpolated.npy out
                               (the two matplotlib plots the reference also writes are not produced)

How a path is formed.  A keyframe [R | c] is replaced by a track of three points: its centre c, the point rot_weight behind it
along the third column of R, and the point rot_weight beside it along the second column.  The three points are interpolated
together (a 9-dimensional curve), and every sample is turned back into a pose whose third axis points from the second point to
the centre and whose second axis leans towards the third point.

The reference only ever passes two keyframes (render.py:43, init_geo.py:94).  Its smoothing B-spline then has degree
min(5, 1) = 1 and no interior knot, and the fit through two points is the chord between them, parametrised by chord length: plain
linear interpolation at n_interp equally spaced parameters starting at 0 and stopping short of 1.  That case is evaluated here in
numpy alone (scipy may be missing where this runs); more keyframes go through scipy.interpolate.splprep / splev, which is the
definition of the result there.  tests/test_camera_path.py pins both against the reference's own function to 1e-10.

Host-side only: nothing here launches a kernel.
"""
from __future__ import annotations

import os

import numpy as np


def _unit(v: np.ndarray) -> np.ndarray:
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _tracks_from_keyframes(keyframes: np.ndarray, reach: float) -> np.ndarray:
    """[n,>=3,4] poses -> [n,3,3]: per camera its centre, the point `reach` behind it and the point `reach` beside it"""
    axes, centre = keyframes[:, :3, :3], keyframes[:, :3, 3]
    return np.stack([centre, centre - reach * axes[:, :, 2], centre + reach * axes[:, :, 1]], axis=1)


def _poses_from_tracks(tracks: np.ndarray) -> np.ndarray:
    """[m,3,3] tracks -> [m,3,4] look-at poses, all at once: columns (first axis, second axis, third axis, centre)"""
    centre, behind, beside = tracks[:, 0], tracks[:, 1], tracks[:, 2]
    third = _unit(centre - behind)
    first = _unit(np.cross(beside - centre, third))
    second = _unit(np.cross(third, first))
    return np.stack([first, second, third, centre], axis=-1)


def _sample_tracks(tracks: np.ndarray, m: int, degree: int, smoothness: float) -> np.ndarray:
    """m samples of the curve through the n tracks at parameters 0, 1/m, .. (m-1)/m -> [m,3,3]"""
    n = tracks.shape[0]
    at = np.linspace(0.0, 1.0, m, endpoint=False)
    if n == 2:   # degree 1 through two points: the chord
        return tracks[0] + at[:, None, None] * (tracks[1] - tracks[0])
    try:
        from scipy.interpolate import splev, splprep
    except ImportError as e:
        raise ImportError("generate_interpolated_path with more than two keyframes fits a smoothing B-spline with "
                          "scipy.interpolate.splprep / splev, and scipy is not installed (two keyframes need no scipy)") from e
    spline, _ = splprep(list(tracks.reshape(n, 9).T), k=min(degree, n - 1), s=smoothness)
    return np.stack(splev(at, spline), axis=-1).reshape(m, 3, 3)


def generate_interpolated_path(poses, n_interp, spline_degree=5, smoothness=.03, rot_weight=.1):
    """poses (n, 3, 4) keyframes (rows beyond the third are ignored) -> (n_interp * (n - 1), 3, 4)"""
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim != 3 or poses.shape[0] < 2 or poses.shape[1] < 3 or poses.shape[2] != 4:
        raise ValueError(f"generate_interpolated_path needs at least two [3,4] keyframes, got an array of shape {poses.shape}")
    tracks = _tracks_from_keyframes(poses, rot_weight)
    return _poses_from_tracks(_sample_tracks(tracks, int(n_interp) * (poses.shape[0] - 1), spline_degree, smoothness))


def interpolated_pose_path(org_pose, n_views: int) -> np.ndarray:
    """org_pose [V,4,4] (V >= n_views) -> [int(10 * 30 / n_views) * (n_views - 1) + 1, 4, 4]: 10 seconds at 30 frames per
    second over the whole path, closed by the last keyframe as it is."""
    org_pose = np.asarray(org_pose, dtype=np.float64)
    n_views = int(n_views)
    if org_pose.ndim != 3 or org_pose.shape[1:] != (4, 4):
        raise ValueError(f"interpolated_pose_path needs [V,4,4] poses, got an array of shape {org_pose.shape}")
    if n_views < 2 or org_pose.shape[0] < n_views:
        raise ValueError(f"a path needs n_views >= 2 keyframes and one pose per view, got n_views = {n_views} and {org_pose.shape[0]} poses")
    per_segment = int(10 * 30 / n_views)
    total = per_segment * (n_views - 1) + 1
    out = np.zeros((total, 4, 4))
    out[:, 3, 3] = 1.0
    for s in range(n_views - 1):
        out[s * per_segment:(s + 1) * per_segment, :3] = generate_interpolated_path(org_pose[s:s + 2], per_segment)
    out[-1, :3] = org_pose[-1, :3]
    return out


def save_interpolate_pose(model_path, iteration, n_views: int) -> str:
    """reads pose/ours_<iteration>/pose_optimized.npy, writes pose_interpolated.npy beside it and returns its path"""
    pose_dir = os.path.join(str(model_path), "pose", f"ours_{iteration}")
    target = os.path.join(pose_dir, "pose_interpolated.npy")
    np.save(target, interpolated_pose_path(np.load(os.path.join(pose_dir, "pose_optimized.npy")), n_views))
    return target
