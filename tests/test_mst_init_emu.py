"""The aligner's initialisation (instantsplat_amd/global_align.py `init_minimum_spanning_tree`, `register_points`,
`compute_global_alignment`; csrc/align_init.hip) under the SIMT emulator: CPU tensors, the same kernel sources.  The checks are
tests/mst_init_util.py's; the restatement and the host-side tree are tested against the recording and scipy here only."""
import pytest

from tests import mst_init_util as mu


@pytest.mark.parametrize("tag", mu.ALL_TAGS)
def test_restatement_equals_reference_recording(tag):
    mu.check_restatement_equals_recording(tag)


def test_tree_equals_scipy_on_random_graphs():
    mu.check_tree_equals_scipy()


@pytest.mark.parametrize("tag", mu.ALL_TAGS)
def test_init_equals_reference_recording(emu, tag):
    mu.check_recording(emu, tag)


@pytest.mark.parametrize("tag", mu.ALL_TAGS)
def test_default_pose_mode(emu, tag):
    mu.check_default_mode(emu, tag)


def test_hand_over_to_the_loop(emu):
    mu.check_hand_over(emu)


@pytest.mark.parametrize("B,n,kind,weights", mu.register_params())
def test_register_points_at_edge_shapes(emu, B, n, kind, weights):
    mu.check_register(emu, B, n, kind, weights)


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("H,W", mu.FOCAL_SHAPES)
def test_weiszfeld_focal(emu, H, W, planted):
    mu.check_focals(emu, H, W, planted)


def test_two_calls_are_bit_identical_and_refusals(emu):
    mu.check_determinism_and_refusals(emu)


def test_entry_points_refuse_bad_sizes(emu):
    mu.check_entry_points_refuse_bad_sizes(emu)
