"""Adaptive density control (instantsplat_amd/density.py, csrc/density.hip) under the SIMT emulator: CPU tensors, the same
kernel sources.  The checks are tests/density_cases.py's."""
import pytest
import torch

from tests import density_cases as dc


@pytest.mark.parametrize("mode", dc.MODES)
@pytest.mark.parametrize("tag", list(dc.GOLDEN_CASES))
def test_restatement_equals_reference(tag, mode):
    dc.check_golden_restatement(tag, mode)


@pytest.mark.parametrize("mode", dc.MODES)
@pytest.mark.parametrize("tag", list(dc.GOLDEN_CASES))
def test_event_equals_reference(emu, tag, mode):
    c, optimizer = dc.golden_case(tag)
    dc.check_event(emu, c, mode, optimizer, golden=dc.load_golden(tag, mode)[0])


@pytest.mark.parametrize("tag", list(dc.GOLDEN_CASES))
def test_reset_opacity_equals_reference(emu, tag):
    dc.check_golden_reset(emu, tag)


@pytest.mark.parametrize("P", dc.SIZES)
def test_sequence_at_every_size(emu, P):
    """clone + split + prune at the wave, block and scan edges, both screen-size settings, N = 2 and 3, both SH widths"""
    k = dc.SIZES.index(P)
    c = dc.make_case(P, "mixed", sh_degree=(3 if k % 2 else 0), N=(2 if k % 3 else 3), max_screen_size=(20 if k % 2 == 0 else None), seed=k)
    dc.check_event(emu, c, "seq", "pp" if k % 2 else "adam")


def test_scan_takes_a_second_turn(emu):
    c = dc.make_case(dc.SIZE_TWO_SCAN_TURNS, "mixed", sh_degree=0, N=2, max_screen_size=20, seed=1)
    dc.check_event(emu, c, "seq", "pp")


@pytest.mark.parametrize("mode", ("clone", "split", "prune_mask", "prune"))
@pytest.mark.parametrize("P", (1, 65, 257))
def test_methods_alone(emu, P, mode):
    c = dc.make_case(P, "mixed", sh_degree=3 if P == 65 else 0, N=2, max_screen_size=20, seed=11)
    dc.check_event(emu, c, mode, "plain")


@pytest.mark.parametrize("screen", (None, 20))
@pytest.mark.parametrize("family", dc.FAMILIES[1:])
def test_families(emu, family, screen):
    for mode in ("seq", "prune"):
        c = dc.make_case(257, family, sh_degree=0, N=2 if screen else 3, max_screen_size=screen, seed=21)
        dc.check_event(emu, c, mode, "pp")


def test_children_pruned_by_the_world_size_term(emu):
    c = dc.make_case(257, "children_pruned", sh_degree=0, N=2, max_screen_size=20, seed=5)
    s, tot = dc.restate(c, "seq", __import__("numpy").float32)
    assert tot["split"] > 0 and tot["children"] < 2 * tot["split"]   # some parents leave no child behind
    dc.check_event(emu, c, "seq", "pp")


@pytest.mark.parametrize("P", (1, 255, 256, 257, 1025))
def test_statistics(emu, P):
    dc.check_stats(emu, P)


@pytest.mark.parametrize("optimizer", ("pp", "adam"))
def test_reset_opacity(emu, optimizer):
    for P in (1, 257):
        dc.check_reset_opacity(emu, P, optimizer)


def test_entry_points_reject_bad_arguments(emu):
    dc.check_rejects(emu)


def test_model_without_radii(emu):
    dc.check_missing_radii(emu)


def test_training_with_density_control(emu, tmp_path):
    dc.check_training(emu, tmp_path, H=24, W=32)


def test_product_path_refuses_cpu_tensors_without_a_gpu():
    from instantsplat_amd import _lib
    _lib._use_library_for_testing(None)
    c = dc.make_case(65, "mixed", sh_degree=0)
    m = dc.build_model(c, torch.device("cpu"), "adam")
    with pytest.raises(RuntimeError, match="GPU only"):
        m.densify_and_prune(dc.MAX_GRAD, dc.MIN_OPACITY, dc.EXTENT, None)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.prune_points(torch.zeros(65, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="GPU only"):
        m.reset_opacity()
    vs = torch.zeros(65, 3, requires_grad=True)
    vs.grad = torch.ones(65, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.add_densification_stats(vs, torch.ones(65, dtype=torch.bool))
