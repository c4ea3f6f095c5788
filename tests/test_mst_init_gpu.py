"""The aligner's initialisation on the MI355X: tests/mst_init_util.py's checks on device tensors."""
import pytest

from tests import mst_init_util as mu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", mu.ALL_TAGS)
def test_init_equals_reference_recording(gpu, tag):
    mu.check_recording(gpu, tag)


@pytest.mark.parametrize("tag", mu.ALL_TAGS)
def test_default_pose_mode(gpu, tag):
    mu.check_default_mode(gpu, tag)


def test_hand_over_to_the_loop(gpu):
    mu.check_hand_over(gpu)


@pytest.mark.parametrize("B,n,kind,weights", mu.register_params())
def test_register_points_at_edge_shapes(gpu, B, n, kind, weights):
    mu.check_register(gpu, B, n, kind, weights)


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("H,W", mu.FOCAL_SHAPES)
def test_weiszfeld_focal(gpu, H, W, planted):
    mu.check_focals(gpu, H, W, planted)


def test_two_calls_are_bit_identical_and_refusals(gpu):
    mu.check_determinism_and_refusals(gpu)


def test_entry_points_refuse_bad_sizes(gpu):
    mu.check_entry_points_refuse_bad_sizes(gpu)


def test_full_size_smoke(gpu):
    mu.check_full_size_smoke(gpu)
