"""The global alignment loop (instantsplat_amd/global_align.py, csrc/align.hip) under the SIMT emulator: CPU tensors, the same
kernel sources.  The checks are tests/global_align_util.py's; the restatement is tested against the reference's recording here only."""
import pytest
import torch

from tests import global_align_util as gu


@pytest.mark.parametrize("tag", list(gu.CONFIGS))
def test_restatement_equals_reference_recording(tag):
    gu.check_restatement_equals_reference(tag)


@pytest.mark.parametrize("tag", list(gu.CONFIGS))
def test_gradients_of_golden_configurations(emu, tag):
    V, H, W, edges, sw, arrays = gu.golden_case(tag)
    gu.check_gradients(emu, edges, H, W, arrays, sw, f"golden {tag}")


@pytest.mark.parametrize("label", [c[0] for c in gu.edge_shape_cases()])
def test_gradients_at_edge_shapes(emu, label):
    gu.check_edge_shape(emu, label)


def test_zero_residual_contributes_zero(emu):
    gu.check_zero_residual(emu)


@pytest.mark.parametrize("tag", list(gu.CONFIGS))
def test_trajectory_equals_reference_recording(emu, tag):
    gu.check_trajectory(emu, tag)


def test_switches_schedules_and_zero_iterations(emu):
    gu.check_switches(emu)


def test_two_runs_are_bit_identical(emu):
    gu.check_determinism(emu)


def test_getters_equal_reference(emu):
    gu.check_getters(emu)


def test_hand_over_to_the_init_stage(emu):
    gu.check_hand_over(emu, None)


def test_entry_points_reject_bad_arguments(emu):
    gu.check_entry_points_reject_bad_arguments(emu)


def test_from_reference_scene_and_its_refusals(emu):
    gu.check_from_reference_scene(emu)


def test_python_rejects_bad_arguments(emu):
    gu.check_python_rejects_bad_arguments(emu)


def test_product_path_refuses_cpu_tensors_without_a_gpu():
    from instantsplat_amd import _lib
    from instantsplat_amd.global_align import AlignProblem
    _lib._use_library_for_testing(None)
    V, H, W, edges, sw, arrays = gu.golden_case("a")
    t = [torch.from_numpy(arrays[k]) for k in ("pred_i", "pred_j", "conf_i", "conf_j")]
    if torch.cuda.is_available():   # with a GPU, tensors that live there are taken
        problem = AlignProblem(edges, *[x.cuda() for x in t], H, W)
        assert problem.im_conf().is_cuda
    else:
        with pytest.raises(RuntimeError, match="GPU only"):
            AlignProblem(edges, *t, H, W)
