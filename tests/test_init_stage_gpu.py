"""The init stage on the MI355X: co-visibility masks and ordered compaction (csrc/init.hip) against the reference's own masks, a
numpy restatement and numpy's boolean indexing, and the stage end to end into three training iterations.  The checks are
tests/init_stage_util.py's; every step runs under a time limit of its own."""
import pytest

from tests import init_stage_util as iu
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", list(iu.CASES))
def test_masks_and_compaction_equal_reference(gpu, tag):
    with ru.time_limit(120):
        iu.check_golden_case(gpu, tag)


@pytest.mark.parametrize("tag", list(iu.GPU_CASES))
def test_full_size_masks_and_compaction_equal_restatement(gpu, tag):
    with ru.time_limit(180):
        iu.check_against_restatement(gpu, tag)


def test_one_and_two_views_and_quirks(gpu):
    with ru.time_limit(120):
        iu.check_one_and_two_views(gpu)
        iu.check_quirks(gpu)


@pytest.mark.parametrize("n", iu.COMPACT_SIZES + (iu.COMPACT_SIZE_TWO_TURNS,))
def test_compaction_against_boolean_indexing(gpu, n):
    with ru.time_limit(120):
        iu.check_compaction(gpu, n)


def test_compaction_all_kept_nearly_none_kept_and_rgb8(gpu):
    with ru.time_limit(120):
        for keep_fraction in (1.0, 0.0):
            iu.check_compaction(gpu, 2 * iu.COUNT_BLOCK + 300, keep_fraction=keep_fraction)
        iu.check_rgb8_values(gpu)


def test_stage_writes_what_the_loader_reads(gpu, tmp_path):
    with ru.time_limit(120):
        iu.check_stage(gpu, str(tmp_path / "a"))
        (tmp_path / "b").mkdir()
        iu.check_stage_switches(gpu, str(tmp_path / "b"))


def test_bad_arguments(gpu):
    with ru.time_limit(120):
        iu.check_entry_points_reject_bad_arguments()
        iu.check_python_rejects_bad_arguments(gpu)


def test_three_training_iterations_from_the_returned_scene(gpu, tmp_path):
    with ru.time_limit(240):
        iu.check_three_training_iterations(gpu, str(tmp_path))
