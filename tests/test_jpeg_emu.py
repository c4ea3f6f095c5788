"""The device JPEG encoder and the MJPEG container (instantsplat_amd/jpeg.py, instantsplat_amd/video.py, csrc/jpeg.hip) on the CPU:
the host restatement against PIL with no device at all, then the same kernel sources under the SIMT emulator against both.  The
checks are tests/jpeg_util.py's; every comparison is of whole files, byte for byte."""
import pytest
import torch

from tests import jpeg_util as ju
from tests import render_path_util as ru


@pytest.mark.parametrize("H,W", ju.SHAPES)
def test_restatement_equals_pil(H, W):
    ju.check_restatement_shape(H, W)


def test_quant_and_huffman_tables_equal_pils():
    ju.check_tables()


@pytest.mark.parametrize("H,W", ju.SHAPES)
def test_files_equal_restatement_and_pil(emu, H, W):
    ju.check_shape(emu, H, W)


def test_stacks_and_addresses(emu):
    ju.check_stacks_and_addresses(emu)


def test_capacity_protocol(emu):
    ju.check_capacity(emu)


def test_entry_point_rejects_bad_arguments(emu):
    ju.check_entry_point_rejects_bad_arguments()


def test_python_refusals(emu, tmp_path):
    ju.check_python_refusals(emu)
    ju.check_write_files(emu, tmp_path)


def test_product_path_refuses_cpu_frames_without_a_gpu():
    from instantsplat_amd import _lib
    from instantsplat_amd.jpeg import encode_jpeg_rgb8
    keep = (_lib._LIB, _lib._TEST_MODE, _lib._EXT_BOUND_TO)
    _lib._use_library_for_testing(None)
    try:
        with pytest.raises(ValueError, match=r"\.to\(device\)"):
            encode_jpeg_rgb8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    finally:   # the module's state as the test found it
        _lib._LIB, _lib._TEST_MODE, _lib._EXT_BOUND_TO = keep


def test_avi_container(tmp_path):
    ju.check_container(tmp_path)


def test_stage_writes_the_video_beside_the_png_files(emu, tmp_path):
    ju.check_stage(emu, ru.small_scene(emu, degree=0), tmp_path)
