"""The evaluation stage (instantsplat_amd/metrics.py, csrc/ssim.hip k_metrics_rgb8) under the SIMT emulator: CPU tensors, the same
kernel sources.  The checks are tests/metrics_util.py's; the host logic (files, pose errors) is tested here only."""
import pytest
import torch

from tests import metrics_util as mu


@pytest.mark.parametrize("H,W", mu.SHAPES)
def test_sq_sum_exact_and_ssim_against_float64(emu, H, W):
    mu.check_shape(emu, H, W)


def test_all_black_identical_pair_scores_one(emu):
    mu.check_all_black_pair_is_one(emu)


def test_all_256_byte_values_convert_as_torch_div(emu):
    mu.check_all_byte_values(emu)


def test_misaligned_bases_score_as_aligned_copies(emu):
    mu.check_misaligned_bases(emu)


def test_empty_set_and_value_errors(emu):
    mu.check_empty_set_and_value_errors(emu)


def test_entry_point_rejects_bad_arguments(emu):
    mu.check_entry_point_rejects_bad_arguments()


def test_product_path_refuses_cpu_frames_without_a_gpu():
    from instantsplat_amd import _lib
    from instantsplat_amd.metrics import image_metrics_rgb8
    _lib._use_library_for_testing(None)
    z = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    if torch.cuda.is_available():   # with a GPU the host frames take one copy each and are scored there
        assert image_metrics_rgb8(z, z)["ssim"].tolist() == [1.0]
    else:
        with pytest.raises(RuntimeError, match="GPU only"):
            image_metrics_rgb8(z, z)


def test_reference_image_values(emu):
    mu.check_golden_images(emu)


def test_reference_pose_values():
    mu.check_golden_poses()


def test_evaluate_writes_the_reference_files(emu, tmp_path):
    mu.check_evaluate_files(emu, str(tmp_path))


def test_evaluate_refuses_other_image_modes(emu, tmp_path):
    mu.check_unsupported_mode_raises(emu, str(tmp_path))


def test_evaluate_from_frame_stacks_reads_no_file(emu, tmp_path):
    mu.check_evaluate_from_frames_equals_files(emu, str(tmp_path))
