"""CPU tier: the composite kernels (csrc/composite.hip) per pixel and per Gaussian against a float64 replay, on the emulated
kernels — the same cases and checks as the GPU tier (tests/composite_cases.py)."""
import numpy as np
import pytest

from tests import composite_cases as cc
from tests import frame_abi
from tests import tile_length_cases as tl


def test_constants_and_layouts_are_the_sources():
    """The thresholds of the replay and the unit lengths are the kernels'; the restated layouts give the library's own sizes
    (frame_abi.FrameViews asserts the totals of the layouts it reads through, for every frame a test looks at)."""
    src = cc.source_constants()
    assert src == dict(GS_TILE=cc.GS_TILE, GS_SEG=cc.GS_SEG, GS_UNIT_LEVELS=len(cc.LEVELS), ALPHA_MIN=cc.ALPHA_MIN, ALPHA_MAX=cc.ALPHA_MAX,
                       ALPHA_MAX_BWD=cc.ALPHA_MAX, T_MIN=cc.T_MIN, FWD_GROUP=2)
    assert tl.source_thresholds()["GS_SEG"] == cc.GS_SEG
    lay = frame_abi.tiles_layout(cc.W, cc.H)
    assert (lay["gx"], lay["gy"], lay["T"]) == (4, 3, 12) and cc.W % 16 == 2 and cc.H % 16 == 5


@pytest.mark.parametrize("det", (0, 1))
@pytest.mark.parametrize("min_units", (1, 3, None), ids=("1", "3", "default"))
def test_layout_totals_are_the_librarys(emu, min_units, det):
    """The layouts restated in tests/frame_abi.py give the library's own sizes at the edges of the arithmetic (the size queries are
    host code: the emulated library answers for the product).  P: P <= 0 counts as 1, 48 P and 8 P cross multiples of 256, the
    512-Gaussian binning chunk.  (W, H): one tile, a ragged grid, W H 4 not a multiple of 256, T + 1 crossing a 64-word boundary.
    R: around the chunk and the top unit length, and on both sides of by_chunks = by_rule (64 (2 min_units + 1)) and of the first
    capacity whose units may be longer than a chunk (128 min_units).  The deterministic mode adds rows to `binning` and the
    offsets table to the gradient scratch.  A render-only buffer ends where unit_tile begins."""
    from instantsplat_amd import _lib
    L = _lib.lib()
    before = frame_abi.current_knobs()
    with frame_abi.knobs(min_units=min_units, det=det):
        mu, det_on = frame_abi.current_knobs()
        assert det_on == det and mu == (before[0] if min_units is None else min_units)
        for P in (0, 1, 5, 6, 511, 512, 513, 1025):
            assert frame_abi.geom_layout(P)["total"] == L.mi355gs_raster_geom_bytes(P), P
            s = frame_abi.grad_scratch_layout(P, det)
            assert (s["total"], s["gate"]) == (L.mi355gs_raster_grad_scratch_bytes(P), L.mi355gs_raster_grad_gate_offset(P)), P
        for W, H in ((1, 1), (16, 16), (17, 33), (50, 37), (1040, 16)):
            t = frame_abi.tiles_layout(W, H)
            assert t["total"] == L.mi355gs_raster_tiles_bytes(W, H), (W, H)
            for R in sorted({0, 1, 63, 64, 65, 511, 512, 513, 64 * (2 * mu + 1) - 1, 64 * (2 * mu + 1) + 1, 128 * mu - 1, 128 * mu}):
                b = frame_abi.binning_layout(R, t["T"], mu, det)
                assert b["total"] == L.mi355gs_raster_binning_bytes(R, W, H), (W, H, R)
                assert b["unit_tile"] == L.mi355gs_raster_binning_bytes_render_only(R, W, H), (W, H, R)
    assert frame_abi.current_knobs() == before


def test_replay_on_a_hand_computed_pixel():
    """Two Gaussians over one pixel, by hand: the second is skipped by the 1/255 cut at a neighbouring pixel; moments and S of the
    first are its single term."""
    rec = np.zeros((2, 12))
    rec[0] = [3.0, 2.0, 0, 0, -0.5, -0.5, 0.0, 0.5, 1.0, 0.0, 0.0, 1.0]
    rec[1] = [3.0, 2.0, 0, 0, -8.0, -8.0, 0.0, 0.5, 0.0, 1.0, 0.0, 2.0]
    start = np.zeros(13, dtype=np.int64)
    start[1:] = 2
    dL = np.zeros((3, cc.H, cc.W))
    dL[:, 2, 3], dL[:, 2, 4] = (1.0, 2.0, 0.0), (1.0, 0.0, 0.0)
    r = cc.replay(rec, np.array([0, 1]), start, cc.BG, dL, np.float64)
    assert r["n_contrib"][2, 3] == 2 and r["n_contrib"][2, 4] == 1           # 0.5 * 2^-8 < 1/255 one pixel away
    assert np.allclose(r["image"][:, 2, 3], np.array([0.5, 0.25, 0.0]) + 0.25 * np.array(cc.BG), rtol=1e-15)
    a = 0.5 * 2.0 ** -0.5                                                     # the first Gaussian one pixel away, alone there
    assert np.isclose(r["final_T"][2, 4], 1 - a, rtol=1e-15)
    # the first Gaussian: at (3, 2) T = 1, behind = 0.25 * 2 (the second's green) + 0.25 * bg.g; at (4, 2) T = 1, behind = (1 - a) bg.g
    w0 = 0.5 * (1.0 - (0.25 * 2.0 + 0.25 * (0.2 + 1.0)) / 0.5)
    w1 = a * (1.0 - (1 - a) * 0.2 / (1 - a))
    assert np.allclose(r["M"][0], [-w1, 0.0, w1, 0.0, 0.0, w0 + w1, 0.5 + a, 1.0, 0.0], rtol=1e-14, atol=1e-16)
    assert np.allclose(r["S"][0, [0, 5, 6]], [abs(w1), abs(w0) + abs(w1), 0.5 + a], rtol=1e-14)
    assert r["touched"].tolist() == [True, True] and not r["B"].any()


@pytest.mark.parametrize("name", cc.NAMES)
def test_cases_hold_what_they_claim(emu, name):
    print(name, cc.check_case_counts(emu, name))


@pytest.mark.parametrize("name", cc.NAMES)
def test_levels_share_records_lists_and_image(emu, name):
    cc.check_levels_agree(emu, name)


@pytest.mark.parametrize("name", cc.NAMES)
def test_forward_per_pixel(emu, name):
    cc.check_forward(emu, name)


@pytest.mark.parametrize("level", cc.LEVELS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_handoff_tables(emu, name, level):
    cc.check_handoff(emu, name, level)


@pytest.mark.parametrize("level", cc.LEVELS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_moments_per_gaussian(emu, name, level):
    cc.check_moments(emu, name, level)


def test_public_outputs_are_the_moments(emu):
    cc.check_public_outputs(emu)


@pytest.mark.parametrize("level", cc.DET_LEVELS)
@pytest.mark.parametrize("name", cc.DET_NAMES)
def test_deterministic_instantiation(emu, name, level):
    cc.check_deterministic(emu, name, level)
