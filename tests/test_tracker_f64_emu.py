"""Device pose tracker (csrc/tracker.hip) under the SIMT emulator against the float64 tracking oracle (tests/tracker_f64_util.py):
small images, P > 49,152 only where the image is one pixel wide."""
import pytest

from tests import pose_tracking_fused_util as fu
from tests import tracker_f64_util as tu


@pytest.mark.parametrize("det", [False, True])
def test_tracker_teacher_forced_matches_float64(emu, det):
    tu.check_teacher_forced_f64(emu, 257, 50, 37, 1, 6, det)


@pytest.mark.parametrize("W,H,P,degree,bg", tu.SHAPES_EMU)
def test_tracker_frame_matches_float64(emu, W, H, P, degree, bg):
    tu.check_frame_f64(emu, W, H, P, degree, bg)


def test_tracker_zero_loss_is_exact(emu):
    tu.check_zero_loss(emu)


def test_tracker_tied_losses_keep_first_best(emu):
    tu.check_tied_losses_keep_first_best(emu)


@pytest.mark.parametrize("kind", ["unblended", "black"])
def test_tracker_all_masked_frame_equals_eager(emu, kind):
    tu.check_all_masked_frame(emu, kind)


@pytest.mark.parametrize("num_iter", [1, 2])
def test_tracker_adam_teacher_forced_short_runs(emu, num_iter):
    fu.check_adam_teacher_forced(emu, num_iter=num_iter, Wm=12, W=32)
