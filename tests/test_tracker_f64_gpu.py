"""Device pose tracker (csrc/tracker.hip) on the MI355X against the float64 tracking oracle (tests/tracker_f64_util.py): the emulated
tier's cases plus 640 x 560 and 1080p frames, P > 49,152 at every image size, reduction consistency at C3 and 1080p, and Adam
trajectories of 1, 2 and 500 iterations (40: test_pose_tracking_fused_gpu.py)."""
import pytest

from tests import pose_tracking_fused_util as fu
from tests import tracker_f64_util as tu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("det", [False, True])
def test_tracker_teacher_forced_matches_float64(gpu, det):
    tu.check_teacher_forced_f64(gpu, 65537, 96, 64, 2, 40, det)


@pytest.mark.parametrize("W,H,P,degree,bg", tu.SHAPES + tu.SHAPES_GPU_ONLY)
def test_tracker_frame_matches_float64(gpu, W, H, P, degree, bg):
    tu.check_frame_f64(gpu, W, H, P, degree, bg)


@pytest.mark.parametrize("kind", ["c3", "1080p"])
def test_tracker_reduction_at_production_size(gpu, kind):
    tu.check_reduction_at_size(gpu, kind)


def test_tracker_zero_loss_is_exact(gpu):
    tu.check_zero_loss(gpu)


def test_tracker_tied_losses_keep_first_best(gpu):
    tu.check_tied_losses_keep_first_best(gpu)


@pytest.mark.parametrize("kind", ["unblended", "black"])
def test_tracker_all_masked_frame_equals_eager(gpu, kind):
    tu.check_all_masked_frame(gpu, kind)


@pytest.mark.parametrize("num_iter", [1, 2, 500])
def test_tracker_adam_teacher_forced(gpu, num_iter):
    fu.check_adam_teacher_forced(gpu, num_iter=num_iter)
