"""Device path renderer (csrc/path.hip, render_path.render_pose_path) on the MI355X: every frame equals the eager
quantize_rgb8(render(...)) byte for byte — both go through the same projection instantiation with the same arguments and the
same render-only compositing, so a differing byte is a bug.  Every step runs under a time limit of its own."""
import os

import numpy as np
import pytest
import torch

from tests import render_path_util as ru

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _c3(gpu, degree=0):
    """C3 size: 196,608 Gaussians, 512 x 512, the untrained synthetic scene, and the 201-pose path of its three train poses"""
    from instantsplat_amd.camera_path import interpolated_pose_path
    st = ru.small_scene(gpu, Wm=256, Hm=256, W=512, H=512, degree=degree, seed=0)
    assert st.gaussians.get_xyz.shape[0] == 196608
    views = ru.path_views(st, interpolated_pose_path(ru.keyframes(st.cameras), 3), keep_images=False)
    assert len(views) == 201
    return st, views


def test_c3_full_path_into_device_frames(gpu):
    with ru.time_limit(240):
        st, views = _c3(gpu)
        res, want = ru.check_path_equals_eager(gpu, st, views, what="C3, 201 poses, device frames")
        assert res["reruns"] == 0 and int(res["counts"].min()) > 0
    with ru.time_limit(120):
        ru.check_counts_are_exact(st, views, res)


def test_c3_slice_into_pinned_frames(gpu):
    with ru.time_limit(240):
        st, views = _c3(gpu, degree=3)
        part = views[60:76]   # 16 poses across the first segment boundary
        ru.check_path_equals_eager(gpu, st, part, pinned=True, what="C3, 16 poses, pinned frames, degree 3")
        ru.check_path_equals_eager(gpu, st, part, pinned=False, what="C3, 16 poses, device frames, degree 3")


def test_sora_art_1280x720(gpu, tmp_path):
    from instantsplat_amd import scene_io
    from instantsplat_amd.train import setup_training
    from tests import sora_util
    with ru.time_limit(240):
        sora_util.write_sora_init_dir(str(tmp_path / "Art"), Wm=160, Hm=90)
        sc = scene_io.load_init_scene(str(tmp_path / "Art"), 3, resolution=1, device=gpu)
        st = setup_training(sc, gpu)
        from instantsplat_amd.pose_tracking import freeze_gaussians
        freeze_gaussians(st.gaussians)
        for cam, gt in zip(st.cameras, st.gt_images):
            cam.original_image = gt
        views = ru.path_views(st, ru.short_path(ru.keyframes(st.cameras), 4), keep_images=False)
        assert len(views) == 9 and (views[0].image_width, views[0].image_height) == (1280, 720)
        res, want = ru.check_path_equals_eager(gpu, st, views, what="sora/Art 1280x720, 9 poses")
    with ru.time_limit(120):
        ru.check_overflow_is_per_frame_and_rerun_repairs(gpu, st, views, want)


@pytest.mark.parametrize("H,W", [(1080, 1920), (23, 37), (1, 1)])
def test_rgb8_equals_torch_expression(gpu, H, W):
    with ru.time_limit(120):
        ru.check_rgb8_equals_torch(gpu, H, W, seeds=(0, 1))


def test_rgb8_special_values_and_nan(gpu):
    with ru.time_limit(120):
        ru.check_rgb8_special_values_each(gpu)
        ru.check_rgb8_nan_is_zero(gpu)
        ru.check_rgb8_nan_is_zero(gpu, 1080, 1920)
        ru.check_rgb8_misaligned_pointers_take_the_plain_path(gpu)


def test_rgb8_into_pinned_memory(gpu):
    from instantsplat_amd.render_path import quantize_rgb8
    with ru.time_limit(120):
        x = ru.rgb8_input(720, 1280, 4).to(gpu)
        out = torch.zeros(720, 1280, 3, dtype=torch.uint8, pin_memory=True)
        quantize_rgb8(x, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, ru.torch_rgb8(x).cpu())


def test_small_scene_overflow_subrange_groups_and_files(gpu, tmp_path):
    with ru.time_limit(240):
        for degree in (0, 3):
            st = ru.small_scene(gpu, Wm=24, Hm=20, W=96, H=64, degree=degree)
            views = ru.path_views(st, ru.short_path(ru.keyframes(st.cameras), 3))
            res, want = ru.check_path_equals_eager(gpu, st, views, what=f"96x64, degree {degree}")
            ru.check_counts_are_exact(st, views, res)
            ru.check_overflow_is_per_frame_and_rerun_repairs(gpu, st, views, want)
        ru.check_subrange_writes_only_its_slots(gpu, st, views, want)
        ru.check_projection_change_starts_a_group(gpu, st, views)
        ru.check_value_errors(gpu, st, views)
        ru.check_render_set_files(gpu, st, views, want, tmp_path)


def test_entry_points_reject_bad_arguments(gpu):
    ru.check_entry_points_reject_bad_arguments()
    ru.check_rgb8_rejects_bad_arguments()


def test_three_stage_flow_from_the_init_directory(gpu, tmp_path):
    """init directory -> training() -> render_interpolated(): the third stage of the reference's run_infer.sh"""
    from instantsplat_amd.pose_tracking import freeze_gaussians
    from instantsplat_amd.render_path import render_interpolated
    from instantsplat_amd.scene_io import load_cameras
    from instantsplat_amd.train import release_trainer, training
    out, IT = tmp_path / "model", 30
    with ru.time_limit(240):
        r = training(os.path.join(GOLDEN, "init_scene"), gpu, iterations=IT, n_views=3, model_path=str(out), saving_iterations=[IT])
        st = r["state"]
        release_trainer(st)
        freeze_gaussians(st.gaussians)
        assert (out / "pose" / f"ours_{IT}" / "pose_optimized.npy").exists()
    with ru.time_limit(240):
        d = render_interpolated(str(out), IT, 3, st.cameras, st.gaussians, st.pipe, st.background)
        assert d == str(out / "interp" / f"ours_{IT}" / "renders")
        assert sorted(os.listdir(d)) == [f"{i:05d}.png" for i in range(201)]
        assert os.listdir(out / "interp" / f"ours_{IT}" / "gt") == []
        path = np.load(out / "pose" / f"ours_{IT}" / "pose_interpolated.npy")
        assert path.shape == (201, 4, 4)
        views = load_cameras(path, list(st.cameras))
        want = ru.eager_frames(views, st)
        assert int(want.max()) > 0
        for i in range(201):
            assert np.array_equal(ru.read_png(os.path.join(d, f"{i:05d}.png")), want[i].numpy()), i
