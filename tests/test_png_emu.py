"""The device PNG encoder (instantsplat_amd/png.py, csrc/png.hip) under the SIMT emulator: CPU tensors, the same kernel sources.
The checks are tests/png_util.py's."""
import pytest
import torch

from tests import png_util as pu
from tests import render_path_util as ru


def test_host_restatement_checks_itself():
    pu.check_host_restatement()


@pytest.mark.parametrize("H,W", pu.SHAPES)
def test_stream_at_every_rows_per_block(emu, H, W):
    pu.check_shape(emu, H, W)


def test_odd_base_addresses(emu):
    pu.check_odd_base_address(emu)


def test_contents_from_zeros_to_noise(emu):
    pu.check_contents(emu)


def test_fibonacci_block_is_length_limited(emu):
    pu.check_fibonacci(emu)


def test_art_crop(emu):
    pu.check_art_crop(emu)


def test_entry_point_rejects_bad_arguments(emu):
    pu.check_entry_point_rejects_bad_arguments()


def test_python_refusals(emu):
    pu.check_python_refusals(emu)


def test_product_path_refuses_cpu_frames_without_a_gpu():
    from instantsplat_amd import _lib
    from instantsplat_amd.png import encode_png_rgb8
    keep = (_lib._LIB, _lib._TEST_MODE, _lib._EXT_BOUND_TO)
    _lib._use_library_for_testing(None)
    try:
        with pytest.raises(ValueError, match=r"\.to\(device\)"):
            encode_png_rgb8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    finally:   # the module's state as the test found it
        _lib._LIB, _lib._TEST_MODE, _lib._EXT_BOUND_TO = keep


def test_max_call_bytes_splits_into_equal_bytes(emu):
    pu.check_split_calls(emu)


def test_render_set_device_files_equal_pil_files(emu, tmp_path):
    st = ru.small_scene(emu, degree=0)
    views = ru.path_views(st, ru.short_path(ru.keyframes(st.cameras), 2))
    pu.check_render_set_device_equals_pil(emu, st, views, tmp_path)
