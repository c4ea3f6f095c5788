"""Device pose tracker (csrc/tracker.hip) under the SIMT emulator: CPU tensors, the same kernel sources."""
import pytest

from tests import pose_tracking_fused_util as fu


def test_fused_tracking_matches_reference_function(emu):
    fu.check_fused_tracking_matches_reference_function(emu)


@pytest.mark.parametrize("degree", [0, 1])
def test_fused_tracking_equals_eager(emu, degree):
    fu.check_fused_equals_eager(emu, degree, num_iter=10, pose_bound=1e-7, loss_bound=1e-6)


def test_tracker_entry_points_reject_bad_arguments(emu):
    fu.check_entry_points_reject_bad_arguments()


def test_fused_tracking_rejects_unimplemented_pipe_flags(emu):
    fu.check_pipe_flags_rejected(emu)


def test_fused_tracking_empty_view_equals_eager(emu):
    fu.check_empty_view(emu)


def test_fused_tracking_overflow_reruns_exactly(emu):
    fu.check_overflow_rerun(emu, num_iter=4, Wm=12, W=32)
