"""GPU tier: the pose transform and pose gradient and per-point Adam on the MI355X against the float64 oracles of
tests/pose_adam_util.py: the emulated tier's cases plus the sizes where the kernels change path — both grid-stride loops of the pose
kernels (P > 1024 x 256 backward, P > 4096 x 256 forward), the 768 and 3,888 per-workgroup rows of C3 and C4's posed frames, and
C3's parameter tensors in Adam."""
import pytest

from tests import pose_adam_util as pau
from tests.test_pose_adam_emu import SMALL_P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", SMALL_P)
def test_pose_op_matches_float64(gpu, P):
    for pose in pau.POSES:
        for up in pau.UPSTREAM:
            pau.check_pose_op(gpu, P, pose, up, seed=P)


@pytest.mark.parametrize("P", [262144, 262145, 995328, 1048577])
def test_pose_op_large(gpu, P):
    for pose, up in (("far", "cancel"), ("near_180", "absent_rot")):
        pau.check_pose_op(gpu, P, pose, up, seed=P)


def test_pose_op_misaligned_quaternions(gpu):
    for pose in ("unit", "huge_q"):
        pau.check_pose_op(gpu, 257, pose, "random", misaligned=True)


# 1, 2, 193, 259, 768 (C3) and 3,888 (C4) rows of per-workgroup pose sums
@pytest.mark.parametrize("V,Wm", [(1, 16), (1, 20), (1, 222), (1, 257), (3, 256), (12, 288)])
def test_posed_node_pose_reduction(gpu, V, Wm):
    pau.check_posed_pose_reduction(gpu, V, Wm)


def test_posed_node_pose_gradient_matches_float64(gpu):
    pau.check_posed_pose_end_to_end(gpu)


@pytest.mark.parametrize("entry", ["ctypes", "compiled", "raw"])
def test_adam_gates_and_edges(gpu, entry):
    pau.check_adam_gates(gpu, entry, pau.edge_specs())


@pytest.mark.parametrize("entry", ["ctypes", "compiled"])
def test_adam_steady_state_and_misaligned_gradients(gpu, entry):
    pau.check_adam_gates(gpu, entry, pau.edge_specs()[:8], seed=3, misaligned=(2, 5, 6))


@pytest.mark.parametrize("entry", ["ctypes", "compiled"])
def test_adam_two_hyper_batches_and_weight_decay(gpu, entry):
    specs = pau.edge_specs()
    for i, s in enumerate(specs):
        if i % 2:
            s.update(betas=(0.8, 0.99), eps=1e-8)
    specs[3]["wd"] = 0.01
    pau.check_adam_gates(gpu, entry, specs, seed=5)


@pytest.mark.parametrize("entry", ["ctypes", "compiled"])
def test_adam_c3_shapes(gpu, entry):
    pau.check_adam_gates(gpu, entry, pau.c3_specs(), seed=7)


def test_adam_live_memory_sees_rewritten_moments(gpu):
    pau.check_adam_live_memory(gpu)


@pytest.mark.parametrize("entry", ["ctypes", "compiled"])
def test_adam_long_trajectory(gpu, entry):
    pau.check_adam_trajectory(gpu, entry)


def test_adam_resumed_at_step_30000(gpu):
    pau.check_adam_trajectory(gpu, "compiled", steps=100, checkpoints=(1, 2, 10, 100), start_step=30000)


def test_adam_after_posed_backward(gpu):
    pau.check_adam_after_posed_backward(gpu)
