"""MASt3R's dense heads (instantsplat_amd/mast3r_heads.py, mast3r.py, csrc/dpt.hip) under the SIMT emulator: CPU tensors, the same
kernel sources — the matrix instruction replaced by its k-ordered fmaf chain (csrc/common.h lp_mfma_32x32x2).  The thin head at
every grid; the real widths run on the device only (test_heads_gpu.py).  The checks are tests/heads_util.py's."""
import pytest

from tests import heads_util as hu


@pytest.mark.parametrize("Ht,Wt", list(hu.GRIDS))
def test_thin_heads_against_float64(emu, Ht, Wt):
    hu.check_case(emu, hu.THIN, Ht, Wt, hu.GRIDS[(Ht, Wt)])


def test_every_kernel_instantiation_is_reached_by_a_device_case():
    hu.check_every_instantiation_is_reached()


def test_equal_bits_across_runs_batches_chunks_descriptors_and_copied_head(emu):
    hu.check_properties(emu, hu.THIN, (2, 3))   # 384 pixels of path_1 per edge: an edge's tiles move with its place in the batch


def test_zeroed_last_layer_gives_exact_zero_points_and_confidence_two(emu):
    hu.check_zeroed_last_layer(emu)


def test_one_confidence_for_points_and_descriptors(emu):
    hu.check_one_conf(emu)


def test_images_to_align_problem(emu):
    hu.check_pipeline(emu)


def test_loader_key_namings_missing_keys_and_checkpoint_file(emu, tmp_path):
    hu.check_loader(emu, str(tmp_path))


def test_value_errors(emu):
    hu.check_value_errors(emu)


def test_entry_points_reject_bad_arguments(emu):
    hu.check_entry_points_reject_bad_arguments()


def test_product_path_refuses_cpu_tensors():
    hu.check_cpu_tensors_refused()
