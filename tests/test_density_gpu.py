"""Adaptive density control on the MI355X (instantsplat_amd/density.py, csrc/density.hip): every event against the reference's
own result, a numpy restatement of its sequence and float64.  The checks are tests/density_cases.py's; every step runs under a
time limit of its own."""
import numpy as np
import pytest

from tests import density_cases as dc
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", dc.MODES)
@pytest.mark.parametrize("tag", list(dc.GOLDEN_CASES))
def test_event_equals_reference(gpu, tag, mode):
    with ru.time_limit(120):
        c, optimizer = dc.golden_case(tag)
        dc.check_event(gpu, c, mode, optimizer, golden=dc.load_golden(tag, mode)[0])


@pytest.mark.parametrize("tag", list(dc.GOLDEN_CASES))
def test_reset_opacity_equals_reference(gpu, tag):
    with ru.time_limit(120):
        dc.check_golden_reset(gpu, tag)


@pytest.mark.parametrize("P", dc.SIZES)
def test_sequence_at_every_size(gpu, P):
    with ru.time_limit(120):
        k = dc.SIZES.index(P)
        c = dc.make_case(P, "mixed", sh_degree=(3 if k % 2 else 0), N=(2 if k % 3 else 3), max_screen_size=(20 if k % 2 == 0 else None), seed=k)
        dc.check_event(gpu, c, "seq", "pp" if k % 2 else "adam")


def test_scan_takes_a_second_turn(gpu):
    with ru.time_limit(180):
        c = dc.make_case(dc.SIZE_TWO_SCAN_TURNS, "mixed", sh_degree=0, N=2, max_screen_size=20, seed=1)
        dc.check_event(gpu, c, "seq", "pp")


@pytest.mark.parametrize("mode", ("clone", "split", "prune_mask", "prune"))
def test_methods_alone(gpu, mode):
    with ru.time_limit(120):
        for P in (1, 65, 257):
            c = dc.make_case(P, "mixed", sh_degree=3 if P == 65 else 0, N=2, max_screen_size=20, seed=11)
            dc.check_event(gpu, c, mode, "plain")


@pytest.mark.parametrize("screen", (None, 20))
@pytest.mark.parametrize("family", dc.FAMILIES[1:])
def test_families(gpu, family, screen):
    with ru.time_limit(120):
        for mode in ("seq", "prune"):
            c = dc.make_case(257, family, sh_degree=0, N=2 if screen else 3, max_screen_size=screen, seed=21)
            dc.check_event(gpu, c, mode, "pp")


def test_children_pruned_by_the_world_size_term(gpu):
    with ru.time_limit(120):
        c = dc.make_case(257, "children_pruned", sh_degree=0, N=2, max_screen_size=20, seed=5)
        _, tot = dc.restate(c, "seq", np.float32)
        assert tot["split"] > 0 and tot["children"] < 2 * tot["split"]
        dc.check_event(gpu, c, "seq", "pp")


def test_statistics_and_reset_opacity(gpu):
    with ru.time_limit(120):
        for P in (1, 255, 256, 257, 1025):
            dc.check_stats(gpu, P)
        for optimizer in ("pp", "adam"):
            for P in (1, 257):
                dc.check_reset_opacity(gpu, P, optimizer)


def test_bad_arguments(gpu):
    with ru.time_limit(120):
        dc.check_rejects(gpu)
        dc.check_missing_radii(gpu)


def test_training_with_density_control(gpu, tmp_path):
    with ru.time_limit(240):
        dc.check_training(gpu, tmp_path, H=48, W=64)
