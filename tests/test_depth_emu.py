"""CPU tier: the depth and accumulated-alpha maps (k_depth_fwd / k_depth_bwd / k_depth_dz of csrc/composite.hip, forward_depth,
render_depth) against float64 on the emulated kernels — the cases and checks of tests/depth_cases.py, the same as the GPU tier's."""
import numpy as np
import pytest

from tests import composite_cases as cc
from tests import depth_cases as dc


def test_replay_on_a_hand_computed_pixel():
    """Two Gaussians (view depths 1 and 2) over one pixel, by hand: both blend at (3, 2) with alpha 0.5, the second is cut by 1/255
    one pixel away.  gD = 1 and gA = 2 at (3, 2), gD = 3 at (4, 2)."""
    rec = np.zeros((2, 12))
    rec[0] = [3.0, 2.0, 0, 0, -0.5, -0.5, 0.0, 0.5, 1.0, 0.0, 0.0, 1.0]
    rec[1] = [3.0, 2.0, 0, 0, -8.0, -8.0, 0.0, 0.5, 0.0, 1.0, 0.0, 2.0]
    start = np.zeros(13, dtype=np.int64)
    start[1:] = 2
    fwd = cc.replay_forward(rec, np.array([0, 1]), start, cc.BG, np.float64)
    depth = cc.to_image(dc.replay_depth(fwd, rec, np.float64))
    a = 0.5 * 2.0 ** -0.5                                       # the first Gaussian one pixel away, alone there
    assert np.isclose(depth[2, 3], 0.5 * 1.0 + 0.25 * 2.0, rtol=1e-15) and np.isclose(depth[2, 4], a, rtol=1e-15)
    assert np.isclose(1 - cc.to_image(fwd["T"])[2, 3], 0.75, rtol=1e-15)
    assert depth[2, 5] > 0 and depth[30, 30] == 0
    gD, gA = np.zeros((cc.H, cc.W)), np.zeros((cc.H, cc.W))
    gD[2, 3], gD[2, 4], gA[2, 3] = 1.0, 3.0, 2.0
    r = dc.replay_depth_backward(fwd, rec, gD, gA, np.float64)
    # the second Gaussian at (3, 2): T = 0.5, nothing behind: dL/dalpha = 1 (0.5 * 2) + 2 * 0.25 / 0.5 = 2, w = 0.5 * 2; dz = 1 * 0.5 * 0.5
    assert np.allclose(r["M"][1], [0, 0, 0, 0, 0, 1.0, 0.25], rtol=1e-14, atol=1e-16)
    # the first at (3, 2): T = 1, S = 0.25 * 2: dL/dalpha = (1 - 0.5 / 0.5) + 2 * 0.25 / 0.5 = 1, w = 0.5; at (4, 2), dx = -1: dL/dalpha = 3, w = 3 a
    w1 = 3.0 * a
    assert np.allclose(r["M"][0], [-w1, 0.0, w1, 0.0, 0.0, 0.5 + w1, 1.0 * 0.5 + 3.0 * a], rtol=1e-14, atol=1e-16)
    assert np.allclose(r["S"][0, [0, 5, 6]], [w1, 0.5 + w1, 0.5 + 3.0 * a], rtol=1e-14)
    assert r["touched"].tolist() == [True, True]


@pytest.mark.parametrize("name", dc.NAMES)
def test_forward_per_pixel(emu, name):
    dc.check_forward(emu, name)


@pytest.mark.parametrize("name", dc.NAMES)
def test_same_bits_after_either_forward_and_at_unit_levels(emu, name):
    dc.check_layouts(emu, name)


@pytest.mark.parametrize("name", dc.NAMES)
def test_sums_per_gaussian(emu, name):
    dc.check_backward(emu, name)


def test_gradient_outputs_are_the_sums(emu):
    dc.check_gradient_outputs(emu)


@pytest.mark.parametrize("name", sorted(dc.EXTRA))
def test_other_frame_sizes(emu, name):
    dc.small_frame(emu, name)


def test_no_gaussians(emu):
    dc.check_no_gaussians(emu)


def test_argument_checks(emu):
    dc.check_arguments(emu)


@pytest.mark.parametrize("name", sorted(dc.OPERATOR_CASES))
def test_operator_end_to_end(emu, name):
    dc.check_operator(emu, name)


def test_operator_under_no_grad(emu):
    dc.check_operator_no_grad(emu)


@pytest.mark.parametrize("python_flags", (False, True), ids=("default", "python-flags"))
def test_render_depth(emu, python_flags):
    dc.check_render_depth(emu, python_flags)
