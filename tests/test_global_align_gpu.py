"""The global alignment loop on the MI355X (csrc/align.hip): gradients against float64 autograd, trajectories against the
reference's recording, switches, determinism, getters, the hand-over to the init stage, and one moderate shape where several
workgroups serve each image.  The checks are tests/global_align_util.py's; every step runs under a time limit of its own."""
import pytest

from tests import global_align_util as gu
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", list(gu.CONFIGS))
def test_gradients_of_golden_configurations(gpu, tag):
    with ru.time_limit(120):
        V, H, W, edges, sw, arrays = gu.golden_case(tag)
        gu.check_gradients(gpu, edges, H, W, arrays, sw, f"golden {tag}")


@pytest.mark.parametrize("label", [c[0] for c in gu.edge_shape_cases()])
def test_gradients_at_edge_shapes(gpu, label):
    with ru.time_limit(120):
        gu.check_edge_shape(gpu, label)


def test_zero_residual_contributes_zero(gpu):
    with ru.time_limit(120):
        gu.check_zero_residual(gpu)


@pytest.mark.parametrize("tag", list(gu.CONFIGS))
def test_trajectory_equals_reference_recording(gpu, tag):
    with ru.time_limit(120):
        gu.check_trajectory(gpu, tag)


def test_switches_schedules_and_zero_iterations(gpu):
    with ru.time_limit(120):
        gu.check_switches(gpu)


def test_two_runs_are_bit_identical(gpu):
    with ru.time_limit(120):
        gu.check_determinism(gpu)


def test_getters_equal_reference(gpu):
    with ru.time_limit(120):
        gu.check_getters(gpu)


def test_hand_over_to_the_init_stage(gpu):
    with ru.time_limit(120):
        gu.check_hand_over(gpu, None)


def test_bad_arguments_and_from_reference_scene(gpu):
    with ru.time_limit(120):
        gu.check_entry_points_reject_bad_arguments(gpu)
        gu.check_python_rejects_bad_arguments(gpu)
        gu.check_from_reference_scene(gpu)


def test_moderate_shape_gradients_and_ten_iterations(gpu):
    with ru.time_limit(120):
        gu.check_moderate_shape(gpu)
