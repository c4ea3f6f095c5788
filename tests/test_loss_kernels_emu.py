"""CPU tier: the loss kernels of instantsplat_amd/csrc/ssim.hip (real sources under the emulator) against the float64 oracle at edge
shapes and on every content of tests/loss_util.py: fused_ssim in both paddings, fused_l1_ssim_loss at lambda 0 / 0.2 / 1, the loss
pair behind train.py's expression as written, l1_loss on misaligned views; and the plane limit of the four plane-grid entry points."""
import pytest

from tests import loss_util

# degenerate: smaller than the window, single rows / columns, the smallest "valid" region (12 x 11 -> 2 x 1)
DEGENERATE = [(1, 1), (1, 40), (40, 1), (5, 7), (11, 11), (12, 11)]
# tile edges: every H and W of {15, 16, 17, 31, 32, 33, 63, 65} once (32 x 16 tiles of k_ssim_*, 32 x 32 of k_l1_ssim_fused)
TILE_EDGES = [(15, 33), (16, 65), (17, 31), (31, 16), (32, 17), (33, 63), (63, 15), (65, 32)]
PLANES = [(1, 1), (2, 1), (3, 4), (2, 3)]   # (B, C): the blockIdx.z plane grid and its offsets


@pytest.mark.parametrize("H,W", DEGENERATE + TILE_EDGES)
def test_loss_kernels_match_float64(emu, H, W):
    for content in loss_util.CONTENTS:
        loss_util.check_case(emu, content, 1, 3, H, W)


@pytest.mark.parametrize("B,C", PLANES)
def test_loss_kernels_match_float64_over_planes(emu, B, C):
    for content in loss_util.CONTENTS:
        loss_util.check_case(emu, content, B, C, 17, 33, seed=B * 10 + C)


@pytest.mark.parametrize("n", [1, 7, 4097, 3 * 65 * 33])
def test_l1_loss_on_misaligned_views(emu, n):
    loss_util.check_l1_misaligned(emu, n)


def test_plane_grid_entry_points_refuse_65536_planes(emu_lib_path):
    codes = loss_util.plane_limit_einval(emu_lib_path)
    assert set(codes) == {"mi355gs_ssim_forward", "mi355gs_ssim_backward", "mi355gs_l1_ssim_loss_fused", "mi355gs_l1_ssim_pair_forward"}
    for name, got in codes.items():
        assert got == [-1, -1, -1], (name, got)   # MI355GS_EINVAL for (B, C) = (65536, 1), (1, 65536), (256, 256)
