"""The composite kernels (csrc/composite.hip) per pixel and per Gaussian against a float64 replay on the MI355X — the cases and
checks of tests/composite_cases.py, whose header lists the limits and what the device measured.  Every frame is 50 x 37 pixels;
the time limits only end a run that hangs."""
import pytest

from tests import composite_cases as cc
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cc.NAMES)
def test_levels_share_records_lists_and_image(gpu, name):
    with ru.time_limit(120):
        print(name, cc.check_case_counts(gpu, name))
        cc.check_levels_agree(gpu, name)


@pytest.mark.parametrize("name", cc.NAMES)
def test_forward_per_pixel(gpu, name):
    with ru.time_limit(120):
        cc.check_forward(gpu, name)


@pytest.mark.parametrize("level", cc.LEVELS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_handoff_tables(gpu, name, level):
    with ru.time_limit(120):
        cc.check_handoff(gpu, name, level)


@pytest.mark.parametrize("level", cc.LEVELS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_moments_per_gaussian(gpu, name, level):
    with ru.time_limit(120):
        cc.check_moments(gpu, name, level)


def test_public_outputs_are_the_moments(gpu):
    with ru.time_limit(120):
        cc.check_public_outputs(gpu)


@pytest.mark.parametrize("level", cc.DET_LEVELS)
@pytest.mark.parametrize("name", cc.DET_NAMES)
def test_deterministic_instantiation(gpu, name, level):
    with ru.time_limit(120):
        cc.check_deterministic(gpu, name, level)
