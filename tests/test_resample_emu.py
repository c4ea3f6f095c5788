"""The device resampler (instantsplat_amd/resample.py, csrc/resample.hip) on the CPU: the coefficient tables and a numpy restatement
of PIL's two passes against PIL with no device at all, then the same kernel sources under the SIMT emulator against PIL and torch.
The checks are tests/resample_util.py's; every comparison is exact."""
import pytest
import torch

from tests import resample_util as ru


def test_tables_have_pils_shape_and_refuse_other_filters():
    ru.check_tables_shape()


@pytest.mark.parametrize("n_in,n_out", ru.TABLE_SIZES)
def test_tables_resize_one_row_as_pil_does(n_in, n_out):
    ru.check_tables_one_row(n_in, n_out)


@pytest.mark.parametrize("case", list(ru.CASES))
def test_restatement_equals_pil(case):
    ru.check_restatement(case)


@pytest.mark.parametrize("case", list(ru.CASES))
def test_bytes_equal_pil(emu, case):
    ru.check_case(emu, case)


@pytest.mark.parametrize("case", ru.STACKED)
def test_stacks_of_three_equal_pil(emu, case):
    ru.check_case(emu, case, N=3)


def test_raw_call_stays_inside_its_buffers(emu):
    ru.check_raw_call_stays_inside_its_buffers(emu)


@pytest.mark.parametrize("case", ru.WINDOW_CASES)
def test_windows_equal_slices_of_the_full_result(emu, case):
    ru.check_windows(emu, case)


def test_float_outputs_have_torchs_bits(emu):
    ru.check_float_outputs(emu)


@pytest.mark.parametrize("size", (512, 224))
def test_load_images_art_frames(emu, size):
    ru.check_load_images_art(emu, size)


def test_load_images_synthetic_files(emu, tmp_path, capsys):
    ru.check_load_images_synthetic(emu, tmp_path, capsys)


def test_load_images_equals_the_references_own(emu, tmp_path):
    ru.check_golden_load_images(emu, tmp_path)


def test_load_cam_on_the_device_equals_pil(emu):
    ru.check_load_cam(emu)


def test_python_refusals(emu):
    ru.check_python_refusals(emu)


def test_entry_point_rejects_bad_arguments(emu):
    ru.check_entry_point_rejects_bad_arguments()


def test_product_path_refuses_cpu_images_without_a_gpu():
    from instantsplat_amd import _lib
    from instantsplat_amd.resample import resize_rgb8
    keep = (_lib._LIB, _lib._TEST_MODE, _lib._EXT_BOUND_TO)
    _lib._use_library_for_testing(None)
    try:
        with pytest.raises(ValueError, match=r"\.to\(device\)"):
            resize_rgb8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), (2, 2))
    finally:   # the module's state as the test found it
        _lib._LIB, _lib._TEST_MODE, _lib._EXT_BOUND_TO = keep
