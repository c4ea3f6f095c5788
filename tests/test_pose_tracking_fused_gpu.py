"""Device pose tracker (csrc/tracker.hip, pose_tracking.optimize_view_pose_fused) on the MI355X."""
import pytest

from tests import pose_tracking_fused_util as fu

pytestmark = pytest.mark.gpu


def test_fused_tracking_matches_reference_function(gpu):
    fu.check_fused_tracking_matches_reference_function(gpu)


def test_fused_tracking_reduces_masked_l1_and_agrees_with_eager(gpu):
    fu.check_tracking_gain_and_eager_agreement(gpu, num_iter=120, Wm=64, W=128)


def test_fused_adam_equals_torch_adam_teacher_forced(gpu):
    fu.check_adam_teacher_forced(gpu)


def test_fused_tracking_overflow_reruns_exactly(gpu):
    fu.check_overflow_rerun(gpu)


def test_fused_tracking_deterministic_runs_identical(gpu):
    fu.check_deterministic_runs_identical(gpu)


def test_fused_tracking_empty_view_equals_eager(gpu):
    fu.check_empty_view(gpu)


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_fused_tracking_equals_eager_sh_degrees(gpu, degree):
    with fu.deterministic():
        fu.check_fused_equals_eager(gpu, degree, num_iter=10, Wm=16, W=48, tag="_gpu")


def test_render_set_optimize_fused_flag(gpu):
    from instantsplat_amd.pose_tracking import render_set_optimize
    st, g, view, init = fu.synthetic_view(gpu, 12, 32, 0)
    out = render_set_optimize([view], g, st.pipe, st.background, num_iter=5, init_poses=[init], fused=True)
    assert len(out) == 1 and set(out[0]) >= {"pose", "initial_loss", "best_loss", "render"}
