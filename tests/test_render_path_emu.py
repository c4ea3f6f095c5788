"""Device path renderer (csrc/path.hip, render_path.render_pose_path) under the SIMT emulator: CPU tensors, the same kernel
sources.  A 48 x 32 scene of 360 Gaussians and the 5-pose path of its three cameras (2 poses per segment + the last keyframe).

Every frame must equal quantize_rgb8(render(view_i, camera_pose=pose_i)["render"]) BYTE FOR BYTE: both go through the same
projection instantiation with the same arguments and the same render-only compositing, so a differing byte is a bug."""
import os

import numpy as np
import pytest
import torch

from tests import render_path_util as ru


def _scene(emu, degree):
    st = ru.small_scene(emu, degree=degree)
    views = ru.path_views(st, ru.short_path(ru.keyframes(st.cameras), 2))
    assert len(views) == 5
    return st, views


@pytest.mark.parametrize("degree", [0, 3])
def test_path_frames_equal_eager_renders(emu, degree):
    st, views = _scene(emu, degree)
    res, want = ru.check_path_equals_eager(emu, st, views)
    assert res["reruns"] == 0
    ru.check_counts_are_exact(st, views, res)


def test_explicit_poses_equal_default_poses(emu):
    from instantsplat_amd.render_path import render_pose_path
    st, views = _scene(emu, 0)
    poses = torch.stack([ru.view_pose(v, emu) for v in views])
    a = render_pose_path(views, st.gaussians, st.pipe, st.background)
    b = render_pose_path(views, st.gaussians, st.pipe, st.background, poses=poses)
    assert torch.equal(a["frames"], b["frames"]) and torch.equal(a["counts"], b["counts"])
    moved = poses.clone()
    moved[:, 4] += 0.05
    c = render_pose_path(views, st.gaussians, st.pipe, st.background, poses=moved)
    ru.assert_frames_equal(c["frames"], ru.eager_frames(views, st, poses=moved), "given poses")
    assert not torch.equal(c["frames"], a["frames"])


@pytest.mark.parametrize("degree", [0, 3])
def test_overflow_is_per_frame_and_rerun_repairs(emu, degree):
    st, views = _scene(emu, degree)
    ru.check_overflow_is_per_frame_and_rerun_repairs(emu, st, views, ru.eager_frames(views, st))


def test_subrange_writes_only_its_slots(emu):
    st, views = _scene(emu, 0)
    ru.check_subrange_writes_only_its_slots(emu, st, views, ru.eager_frames(views, st))


def test_changed_projection_starts_a_group(emu):
    st, views = _scene(emu, 0)
    ru.check_projection_change_starts_a_group(emu, st, views)


def test_value_errors(emu):
    st, views = _scene(emu, 0)
    ru.check_value_errors(emu, st, views)


def test_path_entry_points_reject_bad_arguments(emu):
    ru.check_entry_points_reject_bad_arguments()


def test_render_set_writes_the_frames(emu, tmp_path):
    st, views = _scene(emu, 0)
    ru.check_render_set_files(emu, st, views, ru.eager_frames(views, st), tmp_path)


def test_three_stage_flow_on_the_tiny_scene(emu, tmp_path):
    """init scene -> (the poses training would store) -> interpolated path -> cameras -> frames on disk, by calling the pieces of
    render_interpolated directly with 2 poses per segment"""
    from instantsplat_amd.io_formats import save_pose
    from instantsplat_amd.render_path import render_set
    from instantsplat_amd.scene_io import load_cameras
    st = ru.small_scene(emu, degree=0)
    pose_dir = tmp_path / "pose" / "ours_30"
    pose_dir.mkdir(parents=True)
    save_pose(str(pose_dir / "pose_optimized.npy"), st.gaussians.P, [int(c.colmap_id) for c in st.cameras])
    org = np.load(pose_dir / "pose_optimized.npy")
    assert org.shape == (3, 4, 4)
    path = ru.short_path(org, 2)
    np.save(pose_dir / "pose_interpolated.npy", path)
    views = load_cameras(np.load(pose_dir / "pose_interpolated.npy"), list(st.cameras))
    d = render_set(str(tmp_path), "interp", 30, views, st.gaussians, st.pipe, st.background)
    assert sorted(os.listdir(d)) == [f"{i:05d}.png" for i in range(5)]
    want = ru.eager_frames(views, st)
    for i in range(5):
        assert np.array_equal(ru.read_png(os.path.join(d, f"{i:05d}.png")), want[i].numpy())


def test_render_interpolated_runs_the_stage(emu, tmp_path, capsys):
    """render_interpolated itself: int(10 * 30 / 3) poses per segment of a 16 x 12 scene"""
    from instantsplat_amd.io_formats import save_pose
    from instantsplat_amd.render_path import render_interpolated
    st = ru.small_scene(emu, Wm=6, Hm=5, W=16, H=12, degree=0)
    pose_dir = tmp_path / "pose" / "ours_9"
    pose_dir.mkdir(parents=True)
    save_pose(str(pose_dir / "pose_optimized.npy"), st.gaussians.P, [int(c.colmap_id) for c in st.cameras])
    d = render_interpolated(str(tmp_path), 9, 3, st.cameras, st.gaussians, st.pipe, st.background)
    assert d == os.path.join(str(tmp_path), "interp", "ours_9", "renders")
    assert sorted(os.listdir(d)) == [f"{i:05d}.png" for i in range(201)]
    assert np.load(pose_dir / "pose_interpolated.npy").shape == (201, 4, 4)
    assert st.cameras[0].original_image is not None            # the caller's cameras are left as they were
    try:
        import imageio  # noqa: F401
    except ImportError:
        assert "video was skipped" in capsys.readouterr().out
        assert not os.path.exists(os.path.join(str(tmp_path), "interp", "ours_9", "interp_3_view.mp4"))
