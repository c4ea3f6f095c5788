"""CPU tier: the pose transform and pose gradient (csrc/pose.hip, the POSED projection kernels with k_pose_finish_partials) and
per-point Adam (csrc/adam.hip), real kernel sources under the emulator, against the float64 oracles of tests/pose_adam_util.py."""
import pytest

from tests import pose_adam_util as pau

SMALL_P = [0, 1, 63, 64, 255, 256, 257]


@pytest.mark.parametrize("P", SMALL_P)
def test_pose_op_matches_float64(emu, P):
    for pose in pau.POSES:
        for up in pau.UPSTREAM:
            pau.check_pose_op(emu, P, pose, up, seed=P)


def test_pose_op_backward_grid_stride(emu):
    # 262,145 Gaussians: more than the backward's 1024 workgroups x 256 threads cover in one pass
    pau.check_pose_op(emu, 262145, "unit", "random")


def test_pose_op_misaligned_quaternions(emu):
    for pose in ("unit", "huge_q"):
        pau.check_pose_op(emu, 257, pose, "random", misaligned=True)


# V = 1 frame of Wm x Wm Gaussians: 1, 2, 193 and 259 rows of per-workgroup pose sums (k_pose_finish_partials: the unrolled loop
# runs from 193 rows, where 63 of its 64 row groups still take three rows each in the tail loop; 259 > 256 leaves a tail)
@pytest.mark.parametrize("V,Wm", [(1, 16), (1, 20), (1, 222), (1, 257)])
def test_posed_node_pose_reduction(emu, V, Wm):
    pau.check_posed_pose_reduction(emu, V, Wm)


def test_posed_node_pose_gradient_matches_float64(emu):
    pau.check_posed_pose_end_to_end(emu)


@pytest.mark.parametrize("entry", ["ctypes", "compiled", "raw"])
def test_adam_gates_and_edges(emu, entry):
    pau.check_adam_gates(emu, entry, pau.edge_specs())


@pytest.mark.parametrize("entry", ["ctypes", "compiled"])
def test_adam_steady_state_and_misaligned_gradients(emu, entry):
    # eight tensors in one batch (the compiled plan's _step_fast from step 2); gradients 4 bytes past a 16-byte boundary
    pau.check_adam_gates(emu, entry, pau.edge_specs()[:8], seed=3, misaligned=(2, 5, 6))


@pytest.mark.parametrize("entry", ["ctypes", "compiled"])
def test_adam_two_hyper_batches_and_weight_decay(emu, entry):
    specs = pau.edge_specs()
    for i, s in enumerate(specs):
        if i % 2:
            s.update(betas=(0.8, 0.99), eps=1e-8)
    specs[3]["wd"] = 0.01   # weight decay: the Python fallback
    pau.check_adam_gates(emu, entry, specs, seed=5)


def test_adam_live_memory_sees_rewritten_moments(emu):
    pau.check_adam_live_memory(emu)


@pytest.mark.parametrize("entry", ["ctypes", "compiled"])
def test_adam_long_trajectory(emu, entry):
    pau.check_adam_trajectory(emu, entry)


def test_adam_resumed_at_step_30000(emu):
    pau.check_adam_trajectory(emu, "compiled", steps=100, checkpoints=(1, 2, 10, 100), start_step=30000)


def test_adam_after_posed_backward(emu):
    pau.check_adam_after_posed_backward(emu)
