"""CPU tier: frames with large tile grids on the emulated kernels — the same four edge frames of the tile-count classes of
csrc/binning.hip as the GPU tier (tests/large_grid_cases.py SHAPES) and the same checks, with sparse scenes.

The emulator's cost does not follow the pixel count but the tile count (a workgroup of 256 fibers per tile in the sort and in the
compositing kernels, ~2 ms per tile even when it is empty: 30 s for an empty 2048 x 2048 frame) plus ~13 ms per tile that holds
anything — a 98304 x 17 strip of 12288 tiles takes what 2048 x 1536 takes with the same Gaussians.  So these cases keep the full
frames, with the same tile indices, rows and columns as on the GPU, and populate one or two thousand of their tiles, spread over
the whole index range.  Each takes 45 ... 60 s.

Why the gradients are judged against float64 (large_grid_cases.check_blob_frame) and not by assert_raster_parity's 1e-4 between
the two fp32 implementations: run_blob_case(P=3000, 2048 x 2048, degree 1, scale_mean=0.02, seed=1) on the emulated kernels gives
`grad rot` 1.209e-4 from the fp32 oracle's (every other tensor <= 8.9e-5, image and radii inside their bounds).  Against the
float64 oracle, relative L2:
                         2048 x 2048 (16384 tiles, LDS histogram)      2049 x 2048 (16512 tiles, direct atomics)
               fp32 oracle   emulated device   between the two     fp32 oracle   emulated device   between the two
    means3D     8.986e-05       9.020e-05         1.914e-05         8.054e-05       8.192e-05         1.519e-05
    scaling     1.445e-04       1.216e-04         8.923e-05         1.621e-04       1.688e-04         4.917e-05
    rot         1.870e-04       1.483e-04         1.209e-04         1.292e-04       1.476e-04         7.225e-05
    op          3.684e-05       3.861e-05         1.528e-05         5.022e-05       5.096e-05         9.312e-06
    shs         2.825e-05       2.888e-05         1.092e-05         3.602e-05       3.621e-05         4.755e-06
    means2D     7.867e-05       7.866e-05         1.731e-05         9.309e-05       9.414e-05         1.407e-05
The device's `grad rot` is as far from float64 on the 64 KiB LDS path as on the direct path (1.48e-4 both) and closer than the
fp32 oracle's own (1.87e-4); what moved between the two frames is the oracle's error.  At a focal length of 1774 px with radii of
26 ... 271 px both fp32 evaluations sit 1 ... 2e-4 from the true gradient and need not be within 1e-4 of each other: conditioning,
not a defect of the large-grid binning — whose output, the per-tile lists, is checked exactly here.  (Those two runs take five
minutes each under the emulator and are not repeated as tests; the GPU tier runs the same case.)"""
import pytest

from tests import large_grid_cases as lg


def test_thresholds_are_the_sources():
    """The shapes below are edges only while these constants are binning.hip's."""
    mine = {k: getattr(lg, k) for k in ("SCAN_THREADS", "SCAN_STAGE_MAX_BYTES", "BIN_MAX_LDS_TILES", "BIN_WIDE", "BIN_CHUNK", "BIN_ENTRIES")}
    assert lg.source_thresholds() == mine
    assert lg.BIN_MAX_LDS_TILES <= 64 * 256 and lg.BIN_MAX_LDS_TILES <= 1 << 14     # the 64-bit bin mask; 14 bits of tile in a packed entry


def test_shapes_are_the_edges_of_their_classes():
    tiles = [lg.tile_grid(W, H)[2] for W, H, *_ in lg.SHAPES]
    assert tiles == [lg.LAST_STAGED, tiles[1], lg.BIN_MAX_LDS_TILES, tiles[3]]
    assert lg.LAST_STAGED < tiles[1] <= lg.LAST_STAGED + lg.SCAN_THREADS and lg.BIN_MAX_LDS_TILES < tiles[3] <= lg.BIN_MAX_LDS_TILES + 256
    for (W, H, scan, per, binning), T in zip(lg.SHAPES, tiles):
        assert lg.kernel_forms(T) == (scan, per, binning)
    assert lg.kernel_forms(lg.LAST_STAGED + 1)[0] == "unstaged" and lg.kernel_forms(lg.BIN_MAX_LDS_TILES + 1)[2] == "direct"
    assert lg.kernel_forms(8160) == ("staged", 8, "lds")                             # 1080p, the largest frame of the other files


@pytest.mark.parametrize("W,H,scan,per,binning", [pytest.param(*s, marks=[pytest.mark.slow] if s[1] == 2048 else []) for s in lg.SHAPES],
                         ids=lg.SHAPE_IDS)
def test_tile_lists_are_the_oracles(emu, W, H, scan, per, binning):
    """1024 Gaussians (two binning workgroups) of sigma 0.5 ... 6 px: ~2000 non-empty tiles over the whole index range, every list
    the oracle's minus instances that stay below 1/255.  On the LDS-histogram frames the first workgroup hands the scatter its
    tile list — with tile T - 1 in a packed entry — and the second one touches more than 1024 tiles and is counted again."""
    res = lg.check_tile_lists(emu, 1024, W, H, sigma_max_px=6.0)
    lg.assert_lists_reach_the_edges(res, W, H, scan, per, binning)


# (P, SH degree, scale_mean, seed) per shape, chosen by the fp32 oracle's own error (a sparse frame's gradient norms rest on few
# Gaussians, and one ill-conditioned one moves them)
BLOB_CASES = [(300, 1, 0.006, 1), (300, 3, 0.006, 1), (300, 1, 0.006, 1), (300, 3, 0.006, 2)]


@pytest.mark.parametrize("shape,case", list(zip(lg.SHAPES, BLOB_CASES)), ids=lg.SHAPE_IDS)
def test_forward_backward_against_fp32_and_float64_oracle(emu, shape, case):
    """Image, radii and every gradient of a sparse blob frame.  The fp32 oracle's own largest gradient error against float64 in
    these four cases: 2.3e-5, 3.7e-5, 2.6e-5, 4.2e-5 (the condition is < 2.5e-4), so the device is held to 1e-4."""
    W, H = shape[:2]
    P, deg, scale_mean, seed = case
    lg.check_blob_frame(emu, P, W, H, deg, scale_mean, seed=seed)


def test_workspace_sizes_at_a_large_grid(emu):
    lg.check_workspace_sizes(2049, 2048)
