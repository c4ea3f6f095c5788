"""LPIPS-VGG (instantsplat_amd/lpips.py, csrc/lpips.hip) under the SIMT emulator: CPU tensors, the same kernel sources — the matrix
instruction replaced by its k-ordered fmaf chain (csrc/lpips.hip lp_mfma_32x32x2).  The thin net (32, 32, 64, 64, 96) at every
shape, one real-width pair; the checks are tests/lpips_util.py's."""
import pytest
import torch

from tests import lpips_util as lu


@pytest.mark.parametrize("H,W,N", lu.SHAPES)
def test_thin_net_against_float64(emu, H, W, N):
    lu.check_case(emu, lu.THIN, "mixed", N, H, W, bits=(H, W) != (37, 50))   # exchange and repeat: at the three small shapes


def test_real_widths_16x16_pair_against_float64(emu):
    lu.check_case(emu, lu.REAL, "mixed", 1, 16, 16, bits=False)


def test_one_changed_pixel_in_each_corner(emu):
    lu.check_case(emu, lu.THIN, "corners", 4, 37, 50, bits=False)


def test_signed_lin_weights(emu):
    lu.check_case(emu, lu.THIN, "mixed", 2, 37, 50, signed_lin=True, bits=False)


def test_biases_shifted_so_that_pixels_die(emu):
    lu.check_dead_pixels_present(lu.THIN, -0.5, 37, 50)
    lu.check_case(emu, lu.THIN, "mixed", 2, 37, 50, bias_shift=-0.5, bits=False)


def test_chunked_calls_offsets_and_misaligned_bases(emu):
    lu.check_chunks_and_offsets(emu, lu.THIN)


def test_reference_classes_on_a_thin_net(emu):
    lu.check_golden(emu)


def test_both_key_namings_and_the_blob_layout(emu):
    lu.check_key_namings(emu)


def test_weight_files_load(emu, tmp_path):
    lu.check_files_load(emu, str(tmp_path))


def test_empty_set_and_value_errors(emu):
    lu.check_value_errors(emu)


def test_entry_point_rejects_bad_arguments(emu):
    lu.check_entry_point_rejects_bad_arguments()


def test_evaluate_writes_the_lpips_fields(emu, tmp_path):
    lu.check_evaluate_files(emu, str(tmp_path))


def test_product_path_refuses_cpu_weights_without_a_gpu():
    from instantsplat_amd import _lib
    from instantsplat_amd.lpips import LpipsVGG
    _lib._use_library_for_testing(None)
    vgg, lin = lu.make_weights(lu.THIN)
    if torch.cuda.is_available():
        assert LpipsVGG(vgg, lin).blob.is_cuda
    else:
        with pytest.raises(RuntimeError, match="GPU only"):
            LpipsVGG(vgg, lin)
