"""The evaluation stage on the MI355X: image_metrics_rgb8 (csrc/ssim.hip k_metrics_rgb8) against integer numpy and a float64 SSIM,
against the reference's own numbers, and the stage end to end (training -> render_test_set -> evaluate).  The checks are
tests/metrics_util.py's; every step runs under a time limit of its own."""
import os

import numpy as np
import pytest
import torch

from tests import metrics_util as mu
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("H,W", mu.SHAPES)
def test_sq_sum_exact_and_ssim_against_float64(gpu, H, W):
    with ru.time_limit(120):
        mu.check_shape(gpu, H, W)


def test_identical_pairs_byte_values_and_misaligned_bases(gpu):
    with ru.time_limit(120):
        mu.check_all_black_pair_is_one(gpu)
        mu.check_all_byte_values(gpu)
        mu.check_misaligned_bases(gpu)


def test_empty_set_value_errors_and_bad_arguments(gpu):
    with ru.time_limit(120):
        mu.check_empty_set_and_value_errors(gpu)
        mu.check_entry_point_rejects_bad_arguments()


def test_host_frames_take_one_copy(gpu):
    """CPU and pinned tensors are scored on the device and give what device tensors give"""
    from instantsplat_amd.metrics import image_metrics_rgb8
    with ru.time_limit(120):
        renders, gts = mu.frame_pairs("noise3", 2, 23, 37, seed=6)
        r, g = torch.from_numpy(renders), torch.from_numpy(gts)
        want = image_metrics_rgb8(r.to(gpu), g.to(gpu))
        for a, b in ((r, g), (r.pin_memory(), g.pin_memory()), (r.to(gpu), g)):
            got = image_metrics_rgb8(a, b)
            for k in want:
                assert np.array_equal(got[k], want[k]), k


def test_1080p_black_against_white_needs_64_bits(gpu):
    """sq_sum = 65025 * 3 * 1080 * 1920 > 2^32: a 32-bit total would wrap; psnr = 0"""
    with ru.time_limit(120):
        H, W = 1080, 1920
        m = mu.score(gpu, np.zeros((1, H, W, 3), np.uint8), np.full((1, H, W, 3), 255, np.uint8))
        assert 65025 * 3 * H * W > 2 ** 32
        assert m["sq_sum"].tolist() == [65025 * 3 * H * W] and m["mse"].tolist() == [1.0] and m["psnr"].tolist() == [0.0]


def test_720p_stack_first_pair_against_float64(gpu):
    with ru.time_limit(120):
        renders, gts = mu.frame_pairs("noise3", 3, 720, 1280, seed=2)
        mu.check_against_yardsticks(gpu, renders, gts, "noise3 3x720x1280", ssim_frames=(0,))


def test_reference_image_values(gpu):
    with ru.time_limit(120):
        mu.check_golden_images(gpu)


def test_evaluate_files_and_frame_stacks(gpu, tmp_path):
    with ru.time_limit(120):
        mu.check_evaluate_files(gpu, str(tmp_path / "files"))
        mu.check_evaluate_from_frames_equals_files(gpu, str(tmp_path / "frames"))


def test_stage_end_to_end_from_the_init_directory(gpu, tmp_path):
    """init directory -> training() -> render_test_set() on the train cameras as stand-in test views -> evaluate(), from the
    files and from the frame stacks"""
    from instantsplat_amd.metrics import evaluate, image_metrics_rgb8
    from instantsplat_amd.pose_tracking import freeze_gaussians, render_test_set
    from instantsplat_amd.train import release_trainer, training
    out, IT = tmp_path / "model", 30
    with ru.time_limit(240):
        r = training(os.path.join(GOLDEN, "init_scene"), gpu, iterations=IT, n_views=3, model_path=str(out), saving_iterations=[IT])
        st = r["state"]
        release_trainer(st)
        freeze_gaussians(st.gaussians)
    with ru.time_limit(240):
        views = list(st.cameras)
        names = [f"{v.image_name}.png" for v in views]
        assert len(set(names)) == len(views) == 3 and all(v.original_image is not None for v in views)
        res = render_test_set(str(out), IT, views, st.gaussians, st.pipe, st.background, num_iter=20, fused=True)
        assert len(res["results"]) == 3 and list(res["frames"]) == [f"ours_{IT}"]
        base = out / "test" / f"ours_{IT}"
        assert sorted(os.listdir(base / "renders")) == sorted(names) == sorted(os.listdir(base / "gt"))
        for grp in res["frames"][f"ours_{IT}"]:
            assert grp["renders"].device == gpu and grp["renders"].dtype == torch.uint8 and grp["renders"].shape == grp["gts"].shape
            for k, name in enumerate(grp["names"]):
                assert np.array_equal(ru.read_png(str(base / "renders" / name)), grp["renders"][k].cpu().numpy())
                assert np.array_equal(ru.read_png(str(base / "gt" / name)), grp["gts"][k].cpu().numpy())
    with ru.time_limit(120):
        from_files = evaluate(str(out))
        for f in ("results.json", "per_view.json", os.path.join("test", f"ours_{IT}", "metrics.txt")):
            assert (out / f).exists(), f
        from_frames = evaluate(str(out), frames=res["frames"])
        assert from_files == from_frames
        assert sorted(from_files["results"][f"ours_{IT}"]) == ["PSNR", "SSIM"]
        psnr = from_files["per_view"][f"ours_{IT}"]["PSNR"]
        assert sorted(psnr) == sorted(names)
        for grp in res["frames"][f"ours_{IT}"]:
            black = image_metrics_rgb8(torch.zeros_like(grp["gts"]), grp["gts"])["psnr"]
            for k, name in enumerate(grp["names"]):
                print(f"{name}: PSNR {psnr[name]:.3f} dB, a black frame {black[k]:.3f} dB")
                assert np.isfinite(psnr[name]) and psnr[name] > black[k]
