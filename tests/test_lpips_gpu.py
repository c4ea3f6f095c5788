"""LPIPS-VGG on the MI355X (instantsplat_amd/lpips.py, csrc/lpips.hip: the f32-input matrix instruction): every shape at the real
widths (64, 128, 256, 512, 512) against the float64 restatement, the reference's recording on the thin net, and evaluate() with
the LPIPS keys.  The checks are tests/lpips_util.py's; every step runs under a time limit of its own."""
import pytest

from tests import lpips_util as lu
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H,W,N", lu.SHAPES_GPU)
def test_real_widths_against_float64(gpu, H, W, N):
    with ru.time_limit(120):
        lu.check_case(gpu, lu.REAL, "mixed", N, H, W)


@pytest.mark.parametrize("H,W,N", lu.SHAPES)
def test_thin_net_against_float64(gpu, H, W, N):
    with ru.time_limit(120):
        lu.check_case(gpu, lu.THIN, "mixed", N, H, W)


def test_one_changed_pixel_in_each_corner(gpu):
    with ru.time_limit(120):
        lu.check_case(gpu, lu.REAL, "corners", 4, 37, 50)


def test_signed_lin_weights(gpu):
    with ru.time_limit(120):
        lu.check_case(gpu, lu.REAL, "mixed", 2, 37, 50, signed_lin=True)


def test_biases_shifted_so_that_pixels_die(gpu):
    with ru.time_limit(120):
        lu.check_dead_pixels_present(lu.REAL, -0.5, 37, 50)
        lu.check_case(gpu, lu.REAL, "mixed", 2, 37, 50, bias_shift=-0.5)


def test_chunked_calls_offsets_host_frames_and_misaligned_bases(gpu):
    with ru.time_limit(120):
        lu.check_chunks_and_offsets(gpu, lu.REAL)


def test_reference_classes_on_a_thin_net(gpu):
    with ru.time_limit(120):
        lu.check_golden(gpu)


def test_key_namings_files_value_errors_and_bad_arguments(gpu, tmp_path):
    with ru.time_limit(120):
        lu.check_key_namings(gpu)
        lu.check_files_load(gpu, str(tmp_path))
        lu.check_value_errors(gpu)
        lu.check_entry_point_rejects_bad_arguments()


def test_evaluate_writes_the_lpips_fields(gpu, tmp_path):
    with ru.time_limit(120):
        lu.check_evaluate_files(gpu, str(tmp_path))
