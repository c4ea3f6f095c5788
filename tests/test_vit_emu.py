"""MASt3R's transformer trunk (instantsplat_amd/mast3r_trunk.py, csrc/vit.hip) under the SIMT emulator: CPU tensors, the same kernel
sources — the matrix instruction replaced by its k-ordered fmaf chain (csrc/common.h lp_mfma_32x32x2).  The thin net at every
grid; the checks are tests/vit_util.py's."""
import pytest

from tests import vit_util as vu


def test_restatement_attention_against_sdpa_and_rope_properties():
    vu.check_attention_against_sdpa()


@pytest.mark.parametrize("Ht,Wt", vu.GRIDS)
def test_thin_net_encode_and_decode_against_float64(emu, Ht, Wt):
    vu.check_case(emu, vu.THIN, Ht, Wt)


def test_same_patches_on_transposed_grids_differ(emu):
    vu.check_transposed_grids_differ(emu)


def test_rows_of_zero_variance(emu):
    vu.check_degenerate_rows(emu)


def test_peaked_softmax_logits_past_80(emu):
    vu.check_peaked_softmax(emu)


def test_equal_bits_across_runs_batches_and_edge_sets(emu):
    vu.check_properties(emu)


def test_shared_decoder_side_1_of_ij_is_side_2_of_ji(emu):
    vu.check_shared_decoder_symmetry(emu)


def test_chunked_calls_equal_one_call(emu):
    vu.check_chunked_calls(emu)


def test_loader_key_namings_missing_keys_and_checkpoint_file(emu, tmp_path):
    vu.check_loader(emu, str(tmp_path))


def test_value_errors(emu):
    vu.check_value_errors(emu)


def test_entry_points_reject_bad_arguments(emu):
    vu.check_entry_points_reject_bad_arguments()


def test_product_path_refuses_cpu_tensors():
    vu.check_cpu_tensors_refused()
