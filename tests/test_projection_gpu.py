"""The per-Gaussian projection kernels (csrc/preprocess.hip) per row against float64 under general cameras on the MI355X — the
cases and checks of tests/projection_cases.py, whose header lists the limits and what the device measured.  Every case is at most
400 Gaussians on 64x48 pixels; the time limits only end a run that hangs."""
import pytest

from tests import projection_cases as pc
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", pc.NAMES)
def test_forward_records_per_gaussian(gpu, name):
    with ru.time_limit(60):
        pc.check_forward_records(gpu, name)


@pytest.mark.parametrize("name", pc.NAMES)
def test_gradient_rows_through_the_operator(gpu, name):
    with ru.time_limit(60):
        pc.check_gradient_rows(gpu, name)


@pytest.mark.parametrize("name", pc.SPLIT_ABI_NAMES)
def test_gradient_rows_through_the_c_abi_with_split_sh(gpu, name):
    with ru.time_limit(60):
        pc.check_gradient_rows(gpu, name, path="abi")


def test_posed_node_under_a_general_view(gpu):
    with ru.time_limit(60):
        pc.check_posed_under_view(gpu)


@pytest.mark.parametrize("camera", tuple(pc.CAMERAS))
def test_mark_visible_under_every_camera(gpu, camera):
    with ru.time_limit(60):
        pc.check_mark_visible(gpu, camera)
