"""GPU tier: the loss kernels of instantsplat_amd/csrc/ssim.hip on the MI355X against the float64 oracle (tests/loss_util.py): the
emulated tier's edge shapes and contents, BASELINE's frame sizes (3 x 512^2; C1's 3 x 720 x 1280; C4's 3 x 1080 x 1920, where
1080 = 33 x 32 + 24 leaves a partial row of tiles) and the largest plane grid the entry points accept."""
import pytest

from tests import loss_util
from tests.test_loss_kernels_emu import DEGENERATE, PLANES, TILE_EDGES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H,W", DEGENERATE + TILE_EDGES)
def test_loss_kernels_match_float64(gpu, H, W):
    for content in loss_util.CONTENTS:
        loss_util.check_case(gpu, content, 1, 3, H, W)


@pytest.mark.parametrize("B,C", PLANES)
def test_loss_kernels_match_float64_over_planes(gpu, B, C):
    for content in loss_util.CONTENTS:
        loss_util.check_case(gpu, content, B, C, 17, 33, seed=B * 10 + C)


def test_loss_kernels_match_float64_at_512(gpu):
    for content in loss_util.CONTENTS:
        loss_util.check_case(gpu, content, 1, 3, 512, 512)


@pytest.mark.parametrize("H,W", [(720, 1280), (1080, 1920)])
def test_loss_kernels_match_float64_at_frame_size(gpu, H, W):
    # the two contents where kernels and float32 differ most (noise) and where float32 cancels (render = gt on a flat patch);
    # one float64 oracle run per content, "same" padding only (the training loss)
    for content in ("noise", "flat_quadrant"):
        loss_util.check_case(gpu, content, 1, 3, H, W, valid=False)


@pytest.mark.parametrize("B,C", [(65535, 1), (13107, 5)])
def test_loss_kernels_at_the_plane_limit(gpu, B, C):
    loss_util.check_case(gpu, "noise", B, C, 4, 4, valid=False)


@pytest.mark.parametrize("n", [1, 4097, 3 * 1080 * 1920 + 1])
def test_l1_loss_on_misaligned_views(gpu, n):
    loss_util.check_l1_misaligned(gpu, n)
