"""MASt3R's transformer trunk on the MI355X (instantsplat_amd/mast3r_trunk.py, csrc/vit.hip: the f32-input matrix instruction): the
thin net at every grid and the real widths (1024 / 16 heads, 768 / 12 heads; K reaches 4096 in fc2) against the float64
restatement.  Only the real widths on the 18 x 32 grid reach the 128 x 128 GEMM tile (vit_util.check_both_gemm_tiles_are_reached);
every other case, and the whole emulated tier, runs the 128 x 64 instantiations.  The checks are tests/vit_util.py's; every step runs under a time limit of its own."""
import pytest

from tests import render_path_util as ru
from tests import vit_util as vu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Ht,Wt", vu.GRIDS + vu.GRIDS_GPU_ONLY)
def test_thin_net_encode_and_decode_against_float64(gpu, Ht, Wt):
    with ru.time_limit(120):
        vu.check_case(gpu, vu.THIN, Ht, Wt)


@pytest.mark.parametrize("Ht,Wt", vu.GRIDS_REAL)
def test_real_widths_encode_and_decode_against_float64(gpu, Ht, Wt):
    with ru.time_limit(180):
        vu.check_case(gpu, vu.REAL, Ht, Wt)


def test_real_width_18x32_case_reaches_both_gemm_tiles():
    vu.check_both_gemm_tiles_are_reached()


def test_equal_bits_across_the_gemm_tile_switch(gpu):
    """real widths, 18 x 32: one image alone (128 x 64 tiles) against the same image in the batch of 3 (128 x 128 for qkv and fc1);
    two edges (128 x 64) against the same edges among six (128 x 128)"""
    with ru.time_limit(180):
        vu.check_properties(gpu, vu.REAL, (18, 32))


def test_same_patches_on_transposed_grids_differ(gpu):
    with ru.time_limit(120):
        vu.check_transposed_grids_differ(gpu)


def test_rows_of_zero_variance(gpu):
    with ru.time_limit(120):
        vu.check_degenerate_rows(gpu)


def test_peaked_softmax_logits_past_80(gpu):
    with ru.time_limit(120):
        vu.check_peaked_softmax(gpu)


def test_equal_bits_across_runs_batches_and_edge_sets(gpu):
    with ru.time_limit(120):
        vu.check_properties(gpu)
        vu.check_properties(gpu, vu.THIN, (9, 15))


def test_shared_decoder_side_1_of_ij_is_side_2_of_ji(gpu):
    with ru.time_limit(120):
        vu.check_shared_decoder_symmetry(gpu)


def test_chunked_calls_equal_one_call(gpu):
    with ru.time_limit(120):
        vu.check_chunked_calls(gpu)


def test_loader_value_errors_cpu_tensors_and_bad_arguments(gpu, tmp_path):
    with ru.time_limit(120):
        vu.check_loader(gpu, str(tmp_path))
        vu.check_value_errors(gpu)
        vu.check_cpu_tensors_refused()
        vu.check_entry_points_reject_bad_arguments()
