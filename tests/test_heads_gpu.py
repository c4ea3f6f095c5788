"""MASt3R's dense heads on the MI355X (instantsplat_amd/mast3r_heads.py, mast3r.py, csrc/dpt.hip: the f32-input matrix instruction):
the thin head at every grid, the last stage at every width it is built for, and the real widths (1024 / 768 tokens, 96 .. 768,
F = 256, last_dim 128) against the float64 restatement.  heads_util.check_every_instantiation_is_reached says which case runs
which kernel instantiation.  The checks are tests/heads_util.py's; every step runs under a time limit of its own."""
import pytest

from tests import heads_util as hu
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Ht,Wt", list(hu.GRIDS))
def test_thin_heads_against_float64(gpu, Ht, Wt):
    with ru.time_limit(120):
        hu.check_case(gpu, hu.THIN, Ht, Wt, hu.GRIDS[(Ht, Wt)])


@pytest.mark.parametrize("last_dim", (64, 96))
def test_last_stage_at_every_width(gpu, last_dim):
    with ru.time_limit(120):
        hu.check_case(gpu, dict(hu.THIN, last_dim=last_dim), 3, 5, 1)


@pytest.mark.parametrize("Ht,Wt", list(hu.GRIDS_REAL))
def test_real_widths_against_float64(gpu, Ht, Wt):
    with ru.time_limit(180):
        hu.check_case(gpu, hu.REAL, Ht, Wt, hu.GRIDS_REAL[(Ht, Wt)])


def test_every_kernel_instantiation_is_reached_by_a_device_case():
    hu.check_every_instantiation_is_reached()


def test_equal_bits_across_runs_batches_chunks_descriptors_and_copied_head(gpu):
    with ru.time_limit(120):
        hu.check_properties(gpu)
        hu.check_properties(gpu, hu.THIN, (5, 13))


def test_zeroed_last_layer_gives_exact_zero_points_and_confidence_two(gpu):
    with ru.time_limit(120):
        hu.check_zeroed_last_layer(gpu)


def test_one_confidence_for_points_and_descriptors(gpu):
    with ru.time_limit(120):
        hu.check_one_conf(gpu)


def test_images_to_align_problem(gpu):
    with ru.time_limit(180):
        hu.check_pipeline(gpu)


def test_loader_value_errors_cpu_tensors_and_bad_arguments(gpu, tmp_path):
    with ru.time_limit(120):
        hu.check_loader(gpu, str(tmp_path))
        hu.check_value_errors(gpu)
        hu.check_cpu_tensors_refused()
        hu.check_entry_points_reject_bad_arguments()
