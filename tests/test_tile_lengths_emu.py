"""CPU tier: tile lists at every length boundary of the sort and of the backward's unit cut, on the emulated kernels — the same
frames and checks as the GPU tier (tests/tile_length_cases.py)."""
import pytest

from tests import tile_length_cases as tl

# the lengths this file is about, spelled out: what tile_length_cases.edge_lengths() derives from the thresholds must be these
# while the thresholds are today's
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281,
           1535, 1536, 1537, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 12289]


def test_thresholds_are_the_sources():
    """The lengths below are edges only while these constants, and the chain of tests in sort_one_tile, are the sources'."""
    mine = {k: getattr(tl, k) for k in ("SORT_THREADS", "SORT_SMALL_CAP", "SORT_LDS_CAP", "GS_SEG", "GS_UNIT_LEVELS")}
    assert tl.source_thresholds() == mine
    assert tl.source_sort_paths() == tl.SORT_PATHS


def test_every_edge_length_is_on_a_tile():
    assert tl.edge_lengths() == LENGTHS
    on_tiles = sorted(n for f in tl.FRAMES for n in f)
    assert on_tiles == LENGTHS                                   # each exactly once
    assert all(sum(f) <= tl.MAX_FRAME for f in tl.FRAMES) and len(tl.FRAMES) == 4
    tl.assert_unit_frame_holds_every_levels_edges()
    # both sides of every bound of sort_one_tile, named by the path they take
    for (bound, path), (_, above) in zip(tl.SORT_PATHS, tl.SORT_PATHS[1:] + [(None, "bitonic_sort_any")]):
        assert tl.sort_path(bound) == path and tl.sort_path(bound + 1) == above and {bound, bound + 1} <= set(LENGTHS)
    assert {tl.sort_path(n) for n in LENGTHS if n} == {p for _, p in tl.SORT_PATHS} | {"bitonic_sort_any"}
    assert tl.sort_path(tl.EQUAL_DEPTH_LENGTHS[0]) == "sort_tile_two_runs<2,1>" and tl.sort_path(tl.EQUAL_DEPTH_LENGTHS[1]) == "sort_long_tile"
    assert set(tl.EQUAL_DEPTH_LENGTHS) <= set(LENGTHS)


def test_frames_hold_the_depth_ties_they_claim():
    import numpy as np
    for lengths in tl.FRAMES:
        fr = tl.build_frame(lengths)
        for n, members in zip(lengths, fr["expected"]):
            assert len(members) == n
            distinct = len(np.unique(fr["zbits"][members]))
            if n in tl.EQUAL_DEPTH_LENGTHS:
                assert distinct == 1
            elif n >= 2:
                # the copies, and the few depths a long list of random fp32 values shares by chance
                assert 0.97 * n - 1 <= distinct <= n - min(max(1, n // 50), n // 2), (n, distinct)


@pytest.mark.parametrize("index", range(len(tl.FRAMES)), ids=tl.FRAME_IDS)
def test_lists_are_exact_and_units_are_their_definitions(emu, index):
    fr = tl.build_frame(tl.FRAMES[index])
    for level in range(tl.GS_UNIT_LEVELS):
        tl.check_lists_and_units(emu, fr, level)


@pytest.mark.parametrize("index", range(len(tl.FRAMES)), ids=tl.FRAME_IDS)
def test_composite_at_every_unit_level(emu, index):
    """Measured on the emulated kernels: see the table in test_tile_lengths_gpu.py."""
    tl.check_composite_at_every_level(emu, index)


def test_deterministic_backward_on_a_two_run_and_a_long_list(emu):
    tl.check_deterministic_backward(emu)
