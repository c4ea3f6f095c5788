"""The depth and accumulated-alpha maps (k_depth_fwd / k_depth_bwd / k_depth_dz of csrc/composite.hip, forward_depth, render_depth)
against float64 on the MI355X — the cases and checks of tests/depth_cases.py, whose header lists the limits and what the device
measured.  The time limits only end a run that hangs."""
import pytest

from tests import depth_cases as dc
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", dc.NAMES)
def test_forward_per_pixel(gpu, name):
    with ru.time_limit(120):
        dc.check_forward(gpu, name)


@pytest.mark.parametrize("name", dc.NAMES)
def test_same_bits_after_either_forward_and_at_unit_levels(gpu, name):
    with ru.time_limit(120):
        dc.check_layouts(gpu, name)


@pytest.mark.parametrize("name", dc.NAMES)
def test_sums_per_gaussian(gpu, name):
    with ru.time_limit(120):
        dc.check_backward(gpu, name)


def test_gradient_outputs_are_the_sums(gpu):
    with ru.time_limit(120):
        dc.check_gradient_outputs(gpu)


@pytest.mark.parametrize("name", sorted(dc.EXTRA))
def test_other_frame_sizes(gpu, name):
    with ru.time_limit(120):
        dc.small_frame(gpu, name)


def test_no_gaussians(gpu):
    with ru.time_limit(120):
        dc.check_no_gaussians(gpu)


def test_argument_checks(gpu):
    with ru.time_limit(120):
        dc.check_arguments(gpu)


def test_large_frame_far_corner(gpu):
    with ru.time_limit(120):
        dc.check_large_frame(gpu)


@pytest.mark.parametrize("name", sorted(dc.OPERATOR_CASES))
def test_operator_end_to_end(gpu, name):
    with ru.time_limit(120):
        dc.check_operator(gpu, name)


def test_operator_under_no_grad(gpu):
    with ru.time_limit(120):
        dc.check_operator_no_grad(gpu)


@pytest.mark.parametrize("python_flags", (False, True), ids=("default", "python-flags"))
def test_render_depth(gpu, python_flags):
    with ru.time_limit(120):
        dc.check_render_depth(gpu, python_flags)
