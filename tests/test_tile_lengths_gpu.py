"""Tile lists at every length boundary of the sort and of the backward's unit cut on the MI355X (tests/tile_length_cases.py):
four frames of 12 ... 20 k Gaussians whose tiles hold exactly the lengths of tile_length_cases.edge_lengths().

Measured, errors against the float64 oracle (image: largest absolute difference; gradients: relative L2), fp32 oracle / device,
the device's the largest over unit levels 0 ... 3; the limit is max(1e-4, 2 x the fp32 oracle's) everywhere, and no frame needed
a wider one.  The emulated kernels give the same figures to within 3 % (largest difference: image 1.20e-6 for 1.26e-6).
    frame (shortest-longest list)   0-1281               1535-8191            1536-8193            1537-12289
    image                           4.91e-7 / 4.91e-7    1.15e-6 / 1.26e-6    1.21e-6 / 1.15e-6    9.28e-7 / 9.28e-7
    grad means3D                    3.69e-6 / 3.72e-6    2.61e-6 / 3.12e-6    2.14e-6 / 2.71e-6    2.16e-6 / 2.60e-6
    grad scales                     3.03e-6 / 3.06e-6    2.20e-6 / 2.71e-6    1.90e-6 / 2.42e-6    1.85e-6 / 2.33e-6
    grad rot                        2.40e-6 / 2.45e-6    1.68e-6 / 2.36e-6    1.53e-6 / 2.20e-6    1.48e-6 / 1.99e-6
    grad op                         2.46e-6 / 2.50e-6    2.06e-6 / 3.01e-6    1.76e-6 / 2.66e-6    1.74e-6 / 2.43e-6
    grad col                        2.49e-6 / 2.50e-6    1.96e-6 / 1.95e-6    1.68e-6 / 1.68e-6    1.64e-6 / 1.62e-6
    grad means2D                    3.60e-6 / 3.62e-6    3.00e-6 / 3.52e-6    2.56e-6 / 3.15e-6    2.55e-6 / 2.97e-6
Gradients of levels 1 ... 3 against level 0's, largest absolute difference: at most 0.09 of the limit 1e-5 x max(1, largest
gradient) (2.56e-6 for 2.85e-5, `grad scales` of frame 0-1281; emulated: 0.094).
Deterministic backward (frame 1536-8193, level 1): image 1.15e-6, gradients 1.66e-6 ... 3.14e-6, two runs bit-identical.
Every test takes under half a second on the MI355X; the time limits only end a run that hangs."""
import pytest

from tests import render_path_util as ru
from tests import tile_length_cases as tl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("index", range(len(tl.FRAMES)), ids=tl.FRAME_IDS)
def test_lists_are_exact_and_units_are_their_definitions(gpu, index):
    with ru.time_limit(60):
        fr = tl.build_frame(tl.FRAMES[index])
        for level in range(tl.GS_UNIT_LEVELS):
            tl.check_lists_and_units(gpu, fr, level)


@pytest.mark.parametrize("index", range(len(tl.FRAMES)), ids=tl.FRAME_IDS)
def test_composite_at_every_unit_level(gpu, index):
    with ru.time_limit(60):
        tl.check_composite_at_every_level(gpu, index)


def test_deterministic_backward_on_a_two_run_and_a_long_list(gpu):
    with ru.time_limit(60):
        tl.check_deterministic_backward(gpu)
