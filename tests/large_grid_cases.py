"""Frames with large tile grids (csrc/binning.hip picks kernels and kernel forms by the tile count T = ceil(W/16) * ceil(H/16)),
shared by the emulated (CPU) and the GPU test files: the per-tile lists exactly against the oracle's, image / radii / gradients
against the fp32 and the float64 oracle, and which kernel form a frame takes."""
import math
import os
import re

import numpy as np
import torch

from tests import frame_abi
from tests.util import assert_raster_parity, run_blob_case

# The thresholds of csrc/binning.hip, restated (test_large_grid_emu.py::test_thresholds_are_the_sources holds them to the source:
# if a fix moves one, the edge shapes of both tiers move with it).
SCAN_THREADS = 1024                  # k_scan_tiles: one workgroup; more tiles than threads -> several consecutive tiles per thread
SCAN_STAGE_MAX_BYTES = 48 * 1024     # the staged form's LDS buffer (4 B per tile, whole rounds of the workgroup)
BIN_MAX_LDS_TILES = 16384            # k_count_tiles_lds / k_scatter_lds: 4 B of dynamic LDS per tile; above: the direct kernels
BIN_WIDE = 8                         # rectangles above this many tiles are walked by a 16-lane row instead of their own thread
BIN_CHUNK, BIN_ENTRIES = 512, 1024   # Gaussians per binning workgroup, touched tiles its entry list holds (common.h)
RECOUNT = 0xffffffff                 # entry_n of a workgroup that touched more
LAST_STAGED = SCAN_STAGE_MAX_BYTES // (SCAN_THREADS * 4) * SCAN_THREADS   # 12288 tiles = 12 per thread


# One frame per tile-count class, at its edges: (W, H, scan form, tiles per scan thread, binning form)
SHAPES = [
    (2048, 1536, "staged", 12, "lds"),       # 128 x 96 = 12288: the last staged scan (stage buffer = SCAN_STAGE_MAX_BYTES exactly)
    (2049, 1536, "unstaged", 13, "lds"),     # 129 x 96 = 12384: the first unstaged scan above it; one-pixel last tile column
    (2048, 2048, "unstaged", 16, "lds"),     # 128 x 128 = 16384 = BIN_MAX_LDS_TILES: 64 KiB histogram, tile 16383 in a packed entry
    (2049, 2048, "unstaged", 17, "direct"),  # 129 x 128 = 16512: the first direct-atomic binning; one-pixel last tile column
]
SHAPE_IDS = ["%dx%d" % s[:2] for s in SHAPES]


def source_thresholds():
    """The same constants, read from the kernel source."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "instantsplat_amd", "csrc", "binning.hip")).read()
    hdr = open(os.path.join(root, "instantsplat_amd", "csrc", "common.h")).read()

    def const(text, name):
        m = re.search(r"constexpr\s+(?:int|size_t)\s+%s\s*=\s*([0-9][0-9 *]*);" % name, text)
        assert m, name
        return math.prod(int(f) for f in m.group(1).split("*"))

    return dict(SCAN_THREADS=const(src, "SCAN_THREADS"), SCAN_STAGE_MAX_BYTES=const(src, "SCAN_STAGE_MAX_BYTES"),
                BIN_MAX_LDS_TILES=const(src, "BIN_MAX_LDS_TILES"), BIN_WIDE=const(src, "BIN_WIDE"),
                BIN_CHUNK=const(hdr, "GS_BIN_CHUNK"), BIN_ENTRIES=const(hdr, "GS_BIN_ENTRIES"))


def tile_grid(W, H):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    return gx, gy, gx * gy


def kernel_forms(T):
    """(scan form, tiles per scan thread, binning form) of a frame with T tiles, as gs_launch_scan_tiles / gs_launch_count_tiles /
    gs_launch_binning choose them."""
    per = (T + SCAN_THREADS - 1) // SCAN_THREADS
    staged = T > SCAN_THREADS and per * SCAN_THREADS * 4 <= SCAN_STAGE_MAX_BYTES
    return ("staged" if staged else "unstaged"), per, ("lds" if T <= BIN_MAX_LDS_TILES else "direct")


def check_tile_lists(dev, n, W, H, seed=5, sigma_max_px=20.0, first_chunk_tiny=True):
    """edge_cases.check_tile_lists_against_oracle for a frame of any aspect ratio: the device's per-tile lists are the oracle's
    (the reference's 3-sigma rectangles) in the same (depth, index) order, minus instances that stay below alpha = 1/255 at every
    pixel of the tile.  That function's scene leaves the lower 15 % of a square frame empty, so the Gaussians here are spread over
    1.04 x the frustum in both axes and sized in PIXELS (sigma 0.5 ... sigma_max_px, quadratically biased to the small end: at
    20 px rectangles from 1 tile to ~9 x 9), whatever the focal length.
    first_chunk_tiny: Gaussians 0 ... 511 — the first binning workgroup — are all sigma 0.5 px (1 ... 4 tiles each) and share the
    frame's last corner, a few hundred tiles up to the very last one (Gaussian 0, opaque, sits on its centre): a workgroup whose
    touched tiles fit the entry list, with the largest tile index among them.  The other workgroups' Gaussians touch more than
    1024 tiles each.  (One scene for what test_scatter_takes_the_count_kernels_tile_list_or_recounts does with a scale_boost pair.)
    Returns what the caller needs to show which paths ran: R, R_ref, worst (largest alpha of a dropped instance), count
    (instances per tile), area (tiles in each Gaussian's device rectangle), rect0 (Gaussian 0's), entry_n (per binning workgroup;
    LDS forms only)."""
    from oracle import gs_ref
    from oracle.raster_torch import RasterSettings
    g = torch.Generator().manual_seed(seed)
    tanx = math.tan(math.radians(60) / 2)
    tany = tanx * H / W
    focal = W / (2 * tanx)
    gx, gy, T = tile_grid(W, H)
    z = 2.0 + 4.0 * torch.rand(n, generator=g)
    means = torch.stack([1.04 * tanx * (2 * torch.rand(n, generator=g) - 1) * z, 1.04 * tany * (2 * torch.rand(n, generator=g) - 1) * z, z], dim=1)
    q = torch.randn(n, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    sigma_px = 0.5 + (sigma_max_px - 0.5) * torch.rand(n, 3, generator=g) ** 2
    opac = 0.005 + 0.9 * torch.rand(n, generator=g) ** 3        # faint large Gaussians: 3-sigma rectangle >> alpha >= 1/255 footprint
    if first_chunk_tiny:
        m = min(n, BIN_CHUNK)
        sigma_px[:m] = 0.5
        corner = 0.75 + 0.29 * torch.rand(m, 2, generator=g)    # NDC 0.75 ... 1.04: the last eighth of the frame in both axes
        # ... and Gaussian 0, opaque, on the centre of the very last tile (pixel p is NDC (2 p + 1) / size - 1)
        corner[0, 0] = (16 * (gx - 1) + W) / W - 1
        corner[0, 1] = (16 * (gy - 1) + H) / H - 1
        opac[0] = 0.9
        means[:m, 0], means[:m, 1] = corner[:, 0] * tanx * z[:m], corner[:, 1] * tany * z[:m]
    scales = sigma_px * z[:, None] / focal
    col = torch.rand(n, 3, generator=g)
    cam = frame_abi.identity_camera(W, H)
    res = frame_abi.run_frame(dev, dict(means=means, rots=q, scales=scales, opac=opac, colors=col), cam, bg=torch.zeros(3))
    v, R = res.views, res.R
    start, rect = v.np("tile_start"), v.np("rect")
    x0, y0, x1, y1 = rect[:, 0] & 0xffff, (rect[:, 0] >> 16) & 0xffff, rect[:, 1] & 0xffff, (rect[:, 1] >> 16) & 0xffff
    area = np.where((x1 > x0) & (y1 > y0), (x1 - x0) * (y1 - y0), 0)
    entry_n = [int(x) for x in v.np("bin_n")]

    settings = RasterSettings(image_height=H, image_width=W, tanfovx=tanx, tanfovy=tany, bg=torch.zeros(3), scale_modifier=1.0,
                              viewmatrix=torch.eye(4), projmatrix=cam["proj"].cpu(), sh_degree=0, campos=torch.zeros(3),
                              prefiltered=False, debug=False)
    _, _, ctx = gs_ref.forward(means, opac, settings, colors_precomp=col, scales=scales, rotations=q)
    R_ref = ctx.num_rendered
    assert start[0] == 0 and start[T] == R and 0 < R <= R_ref
    assert int(area.sum()) == R                                  # every instance of every device rectangle is in a list
    assert bool((np.diff(start) >= 0).all())
    kept, dropped, worst = frame_abi.lists_against_oracle(v, ctx.aux(W, H), W, H)
    assert kept == R and kept + dropped == R_ref
    return dict(R=R, R_ref=R_ref, worst=worst, count=np.diff(start), area=area, entry_n=entry_n,
                rect0=(int(x0[0]), int(y0[0]), int(x1[0]), int(y1[0])))


def assert_lists_reach_the_edges(res, W, H, scan, per, binning, min_top_tiles=64):
    """The frame is the edge of its tile-count class that the caller says it is, and the lists just checked are not vacuous there:
    instances in the last tile row, the last tile column, the very last tile (the largest index a packed entry or a scan thread's
    run holds), in at least min_top_tiles tiles of the top eighth of the index range and, on a direct-binning frame, in tiles past
    the LDS forms' range; rectangles on both sides of BIN_WIDE."""
    gx, gy, T = tile_grid(W, H)
    assert kernel_forms(T) == (scan, per, binning), (T, kernel_forms(T))
    count, area = res["count"].reshape(gy, gx), res["area"]
    assert res["R"] > 0 and res["R"] < res["R_ref"]              # something was binned, and something invisible was dropped
    assert int(count[-1].sum()) > 0 and int(count[:, -1].sum()) > 0 and int(count[-1, -1]) > 0, "no instance at the frame's far edges"
    x0, y0, x1, y1 = res["rect0"]
    assert x0 <= gx - 1 < x1 and y0 <= gy - 1 < y1, res["rect0"]  # Gaussian 0 (of the first workgroup) is binned to tile T - 1
    top = count.reshape(-1)[T - T // 8:]
    assert int((top > 0).sum()) >= min_top_tiles, int((top > 0).sum())   # the top eighth of the index range is populated
    if binning == "direct":
        assert int(res["count"][BIN_MAX_LDS_TILES:].sum()) > 0
    assert int((area > BIN_WIDE).sum()) > 0 and int(((area > 0) & (area <= BIN_WIDE)).sum()) > 0
    if binning == "lds":
        # the first workgroup (512 Gaussians of 1 ... 4 tiles in one corner) handed its tile list to the scatter; one of the others
        # touched more tiles than the list holds and was counted again
        assert 1 <= res["entry_n"][0] <= BIN_ENTRIES, res["entry_n"]
        assert RECOUNT in res["entry_n"][1:], res["entry_n"]


# ---------------------------------------------------------------------------------------------------- forward and backward
GRAD_FLOOR, GRAD_FACTOR, GRAD_CAP = 1e-4, 2.0, 5e-4
BLOB_BG = (0.2, 0.5, 0.9)   # run_blob_case's default background


def gradient_errors(out):
    """{tensor: (fp32 oracle's, device's)} relative L2 errors against the float64 oracle"""
    res = {}
    for k, g in out["f64"]["grads"].items():
        n = float(g.norm()) + 1e-30
        res[k] = (float((out["ref"]["grads"][k].double() - g).norm()) / n, float((out["dut"]["grads"][k].double() - g).norm()) / n)
    return res


def check_blob_frame(dev, P, W, H, deg, scale_mean, seed=1):
    """One blob frame forward and backward.  Image and radii: assert_raster_parity's forward bounds against the fp32 oracle.
    Gradients: at these focal lengths two fp32 implementations are not reliably within 1e-4 of EACH OTHER (see
    test_large_grid_emu.py), so each is measured against the float64 oracle and the device may be at most
    max(1e-4, 2 x the fp32 oracle's own error) away, and never more than 5e-4 (an allowance relative to another
    implementation's error needs an absolute cap).  The cap only means something while the oracle itself stays well below it:
    the case must keep the fp32 oracle under half the cap, or it is the case that has to change."""
    out = run_blob_case(dev, P, W, H, deg, scale_mean=scale_mean, seed=seed, bg=BLOB_BG, with_f64=True)
    fwd = lambda o: dict(color=o["color"], radii=o["radii"], grads={})
    assert_raster_parity(dict(ref=fwd(out["ref"]), dut=fwd(out["dut"])))
    assert int((out["dut"]["radii"] > 0).sum()) > P // 2
    gx, gy, _ = tile_grid(W, H)
    painted = (out["dut"]["color"] - torch.tensor(BLOB_BG)[:, None, None]).abs().amax(0) > 1e-3
    assert bool(painted[16 * (gy - 1):].any()) and bool(painted[:, 16 * (gx - 1):].any()), "nothing drawn in the last tile row / column"
    errs = gradient_errors(out)
    assert set(errs) == {"means3D", "scaling", "rot", "op", "shs", "means2D"}
    for k, (e_ref, e_dut) in errs.items():
        print("%dx%d grad %-8s fp32 oracle %.3e  device %.3e  (vs float64, relative L2)" % (W, H, k, e_ref, e_dut))
    for k, (e_ref, e_dut) in errs.items():
        assert e_ref < 0.5 * GRAD_CAP, f"grad {k}: the fp32 oracle itself is {e_ref:.3e} from float64: choose a better-conditioned case"
        assert e_dut <= min(max(GRAD_FLOOR, GRAD_FACTOR * e_ref), GRAD_CAP), f"grad {k}: device {e_dut:.3e}, fp32 oracle {e_ref:.3e}"
    return out, errs


# ---------------------------------------------------------------------------------------------------- the handles
def check_workspace_sizes(W, H, P=12288, V=3, capacity=1 << 20):
    """The path, trainer and tracker handles carve their workspaces from (P, W, H, capacity): a size at a large grid, and no
    smaller than for a 1080p frame of the same scene."""
    from instantsplat_amd import _lib
    L = _lib.lib()
    sizes = dict(path=lambda w, h: L.mi355gs_path_workspace_bytes(P, w, h, capacity),
                 trainer=lambda w, h: L.mi355gs_trainer_workspace_bytes(P, w, h, V, capacity),
                 tracker=lambda w, h: L.mi355gs_tracker_workspace_bytes(P, w, h, capacity))
    for name, f in sizes.items():
        big, hd = int(f(W, H)), int(f(1920, 1080))
        assert hd > 0 and big >= hd, (name, big, hd)
        assert big > 3 * W * H * 4, (name, big)                  # every one of them holds at least a float frame


def check_path_handle(dev, W, H, Wm, Hm, n_interp=2):
    """render_pose_path (the path handle: its own workspace, projection, binning and render-only compositing per pose) equals the
    eager render() frames byte for byte at a large grid, the frames are drawn down to the last tile row, and every frame's
    instance count is the one the tracker handle's count entry point gives for that pose."""
    from tests import render_path_util as ru
    st = ru.small_scene(dev, Wm=Wm, Hm=Hm, W=W, H=H, degree=1)
    views = ru.path_views(st, ru.short_path(ru.keyframes(st.cameras), n_interp), keep_images=False)
    assert (int(views[0].image_width), int(views[0].image_height)) == (W, H)
    res, want = ru.check_path_equals_eager(dev, st, views, what="%dx%d, %d poses" % (W, H, len(views)))
    gx, gy, _ = tile_grid(W, H)
    for frame in want:
        assert len(torch.unique(frame[16 * (gy - 1):])) > 16 and len(torch.unique(frame[:, 16 * (gx - 1):])) > 16
    assert int(res["counts"].min()) > 0
    ru.check_counts_are_exact(st, views, res)
