"""The init stage (instantsplat_amd/init_stage.py, csrc/init.hip) under the SIMT emulator: CPU tensors, the same kernel sources.
The checks are tests/init_stage_util.py's; the host functions and the numpy restatement are tested here only."""
import pytest
import torch

from tests import init_stage_util as iu


@pytest.mark.parametrize("tag", list(iu.CASES))
def test_restatement_equals_reference_masks(tag):
    iu.check_restatement_equals_golden(tag)


@pytest.mark.parametrize("tag", list(iu.CASES))
def test_masks_and_compaction_equal_reference(emu, tag):
    iu.check_golden_case(emu, tag)


def test_one_and_two_views(emu):
    iu.check_one_and_two_views(emu)


def test_quirks_of_the_reference_arithmetic(emu):
    iu.check_quirks(emu)


@pytest.mark.parametrize("n", iu.COMPACT_SIZES)
def test_compaction_against_boolean_indexing(emu, n):
    iu.check_compaction(emu, n)


def test_compaction_scan_takes_a_second_turn(emu):
    iu.check_compaction(emu, iu.COMPACT_SIZE_TWO_TURNS)


@pytest.mark.parametrize("keep_fraction", (1.0, 0.0))
def test_compaction_all_kept_and_nearly_none_kept(emu, keep_fraction):
    iu.check_compaction(emu, 2 * iu.COUNT_BLOCK + 300, keep_fraction=keep_fraction)


def test_rgb8_of_every_byte_value(emu):
    iu.check_rgb8_values(emu)


def test_stage_writes_what_the_loader_reads(emu, tmp_path):
    iu.check_stage(emu, str(tmp_path))


def test_stage_switches(emu, tmp_path):
    iu.check_stage_switches(emu, str(tmp_path))


def test_test_poses_and_ranking_equal_reference():
    iu.check_test_poses_and_ranking()


def test_entry_points_reject_bad_arguments(emu):
    iu.check_entry_points_reject_bad_arguments()


def test_python_rejects_bad_arguments(emu):
    iu.check_python_rejects_bad_arguments(emu)


def test_product_path_refuses_cpu_tensors_without_a_gpu():
    from instantsplat_amd import _lib
    from instantsplat_amd.init_stage import co_visibility_masks, compact_pointmaps
    _lib._use_library_for_testing(None)
    d = iu.synthetic_views(2, 5, 7, 1)
    t = torch.from_numpy
    if torch.cuda.is_available():   # with a GPU the host arrays take one copy each and are processed there
        m = co_visibility_masks([0, 1], t(d["depthmaps"]), t(d["pointmaps"]), t(d["intrinsics"]), t(d["w2c"]), 0.05)
        assert m.is_cuda and m.dtype == torch.bool
    else:
        with pytest.raises(RuntimeError, match="GPU only"):
            co_visibility_masks([0, 1], t(d["depthmaps"]), t(d["pointmaps"]), t(d["intrinsics"]), t(d["w2c"]), 0.05)
        with pytest.raises(RuntimeError, match="GPU only"):
            compact_pointmaps(t(d["pointmaps"]), t(d["images"]), t(d["confidences"]))
