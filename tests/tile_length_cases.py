"""Frames with prescribed per-tile list lengths (csrc/binning.hip sort_one_tile picks one of nine sort paths by a tile's list
length n, and k_scan_tiles cuts the same n into the backward's units), shared by the emulated (CPU) and the GPU test files:
every tile holds exactly the number of instances the case asks for, on each side of every threshold; the device's lists exactly
against numpy's sort of (depth bits, index); the scan's unit tables against their definitions; image, radii and every gradient
at every unit length against the fp32 and the float64 oracle."""
import math
import os
import re

import numpy as np
import torch

from tests import frame_abi, ops_util
from tests.util import assert_no_worse_than_fp32_oracle, run_custom_case

# The thresholds of csrc/binning.hip and csrc/common.h, restated (test_tile_lengths_emu.py::test_thresholds_are_the_sources holds
# them to the sources: if a fix moves one, the edge lengths of both tiers move with it).
SORT_THREADS = 256       # sort_one_tile: one workgroup per tile; 1, 2, 4 or 8 keys per thread, or two runs of (2|4) + (1|2)
SORT_SMALL_CAP = 2048    # the register network's largest list; longer ones are sorted as runs of this length, placed by rank
SORT_LDS_CAP = 8192      # ... up to here; longer ones by the bitonic network in global memory
GS_SEG = frame_abi.GS_SEG             # instances per chunk; a backward unit is GS_SEG << level of them (read from common.h)
GS_UNIT_LEVELS = frame_abi.GS_UNIT_LEVELS
MAX_FRAME = 20000        # Gaussians per frame (edge_cases.check_long_tile_lists sends as many through the oracle)
GRID_X = 6               # tile columns of every frame


def source_thresholds():
    """The same constants, read from the kernel sources."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "instantsplat_amd", "csrc", "binning.hip")).read()
    hdr = open(os.path.join(root, "instantsplat_amd", "csrc", "common.h")).read()

    def const(text, name):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*([0-9A-Z_]+);" % name, text)
        assert m, name
        return int(m.group(1)) if m.group(1).isdigit() else const(hdr, m.group(1))

    return dict(SORT_THREADS=const(src, "SORT_THREADS"), SORT_SMALL_CAP=const(src, "SORT_SMALL_CAP"), SORT_LDS_CAP=const(src, "SORT_LDS_CAP"),
                GS_SEG=const(hdr, "GS_SEG"), GS_UNIT_LEVELS=const(hdr, "GS_UNIT_LEVELS"))


def source_sort_paths():
    """sort_one_tile's chain of `n <= bound` tests, read from the source: [(bound, path), ...] in the order it tries them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "instantsplat_amd", "csrc", "binning.hip")).read()
    body = src[src.index("void sort_one_tile("):]
    body = body[: body.index("\n}")]
    names = dict(SORT_THREADS=SORT_THREADS, SORT_SMALL_CAP=SORT_SMALL_CAP, SORT_LDS_CAP=SORT_LDS_CAP)
    res = []
    for bound, path in re.findall(r"if \(n <= ([A-Z_]+(?: \* \d+)?)\) (\w+(?:<[\d, ]+>)?)\(", body):
        f = bound.split(" * ")
        res.append((names[f[0]] * (int(f[1]) if len(f) > 1 else 1), path.replace(" ", "")))
    return res


# (largest n, path) as sort_one_tile tries them; above the last: bitonic_sort_any in global memory
SORT_PATHS = [(SORT_THREADS, "sort_tile_regs<1>"), (SORT_THREADS * 2, "sort_tile_regs<2>"), (SORT_THREADS * 3, "sort_tile_two_runs<2,1>"),
              (SORT_THREADS * 4, "sort_tile_regs<4>"), (SORT_THREADS * 5, "sort_tile_two_runs<4,1>"),
              (SORT_THREADS * 6, "sort_tile_two_runs<4,2>"), (SORT_SMALL_CAP, "sort_tile_regs<8>"), (SORT_LDS_CAP, "sort_long_tile")]


def sort_path(n):
    for bound, path in SORT_PATHS:
        if n <= bound:
            return path
    return "bitonic_sort_any"


def unit_lengths():
    return [GS_SEG << level for level in range(GS_UNIT_LEVELS)]


def edge_lengths():
    """0, 1, 2 and one list on, below and above: every bound of sort_one_tile (the last key of a path / the first of the next:
    nb == NBMAX and nb == 1 of the two-run paths, n == NMAX of sort_count_below, one ~0 pad or none); two full runs of
    sort_long_tile (its last run full, one short of full, or a single key; a single key again at SORT_SMALL_CAP + 1); every unit
    length U and 2 U (a tile without a short last unit beside one whose short unit holds one instance, or lacks one).  Then a list
    for the global-memory network that is not a power of two: SORT_LDS_CAP + 2 SORT_SMALL_CAP + 1."""
    on = [bound for bound, _ in SORT_PATHS] + [2 * SORT_SMALL_CAP] + [m * u for u in unit_lengths() for m in (1, 2)]
    return sorted({0, 1, 2} | {n + d for n in on for d in (-1, 0, 1)} | {SORT_LDS_CAP + 2 * SORT_SMALL_CAP + 1})


# The two lists whose depths are all equal (the index alone orders them): the longest two-run list of 2 + 1 keys per thread, and
# the long list whose last run is a single key.
EQUAL_DEPTH_LENGTHS = (SORT_THREADS * 3, SORT_SMALL_CAP + 1)


def frames():
    """The edge lengths dealt to as few frames of at most MAX_FRAME Gaussians as they fit: the lists above the unit lengths'
    range largest first, each to the first frame with room; then every list up to 2 U + 1 of the longest unit together, to the
    first frame that takes them all (so one frame holds U - 1, U, U + 1, 2 U - 1, 2 U, 2 U + 1 of all four levels).  A frame's
    tiles are in ascending length — a multiple of a unit length next to the list one longer — with the empty tile moved
    between the lists of 1 and 2.  Returns [per-tile lengths of frame 0, ...]."""
    top = 2 * unit_lengths()[-1] + 1
    small = [n for n in edge_lengths() if n <= top]
    bins = []
    for n in sorted((n for n in edge_lengths() if n > top), reverse=True):
        for b in bins:
            if sum(b) + n <= MAX_FRAME:
                b.append(n)
                break
        else:
            bins.append([n])
    for b in bins:
        if sum(b) + sum(small) <= MAX_FRAME:
            b.extend(small)
            break
    else:
        bins.append(list(small))
    res = []
    for b in bins:
        b = sorted(b)
        if b[:3] == [0, 1, 2]:
            b[:3] = [1, 0, 2]
        res.append(b)
    return res


FRAMES = frames()
assert sorted(n for f in FRAMES for n in f) == edge_lengths() and all(sum(f) <= MAX_FRAME for f in FRAMES)   # each length on one tile
FRAME_IDS = ["%d-%d" % (min(f), max(f)) for f in FRAMES]
UNIT_FRAME = next(i for i, f in enumerate(FRAMES) if 0 in f)     # the frame of the unit lengths' edges (and of the empty tile)
# the first frame with a two-run list and a long one: the deterministic backward's
DET_FRAME = next(i for i, f in enumerate(FRAMES) if any("two_runs" in sort_path(n) for n in f) and any(n > SORT_SMALL_CAP for n in f))


def frame_size(lengths):
    gy = (len(lengths) + GRID_X - 1) // GRID_X
    return 16 * GRID_X, 16 * gy


_BUILT = {}


def build_frame(lengths, seed=0):
    """Gaussians that put exactly lengths[t] instances into tile t of a frame of GRID_X tile columns (tiles the list does not
    reach stay empty): camera-frame means under an identity view matrix, about 0.5 px sigma (0.4 ... 0.6 per axis, sized in
    pixels: scales = sigma_px * z / focal), centres over pixels 4 ... 11 of their tile in both axes — the 3-sigma square of the
    reference, 3 px with the 0.3 px^2 low-pass, stays inside the tile —, opacity 0.02 ... 0.04 (at the pixel nearest its centre
    a Gaussian keeps > 0.6 of it: far above 1/255), precomputed colours.  The Gaussians of all tiles are interleaved at random,
    so a tile's indices are scattered over 0 ... n - 1.  In every tile 2 % of the depths (at least one) are exact copies of
    another Gaussian's of that tile; in the tiles of EQUAL_DEPTH_LENGTHS all depths are one value."""
    key = (tuple(lengths), seed)
    if key in _BUILT:
        return _BUILT[key]
    W, H = frame_size(lengths)
    n = int(sum(lengths))
    g = torch.Generator().manual_seed(1000 + seed)
    tile_of = torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths))[torch.randperm(n, generator=g)]
    z = 2.0 + 4.0 * torch.rand(n, generator=g)
    for t, length in enumerate(lengths):
        mine = torch.nonzero(tile_of == t).reshape(-1)
        if length in EQUAL_DEPTH_LENGTHS:
            z[mine] = float(z[mine[0]])
        elif length >= 2:
            k = min(max(1, length // 50), length // 2)
            pick = mine[torch.randperm(length, generator=g)]
            z[pick[:k]] = z[pick[k: 2 * k]].clone()
    tanx = math.tan(math.radians(60) / 2)
    tany = tanx * H / W
    focal = W / (2 * tanx)
    px = 16.0 * (tile_of % GRID_X) + 4.0 + 7.0 * torch.rand(n, generator=g)
    py = 16.0 * (tile_of // GRID_X) + 4.0 + 7.0 * torch.rand(n, generator=g)
    # pixel p is NDC (2 p + 1) / size - 1
    means = torch.stack([((2 * px + 1) / W - 1) * tanx * z, ((2 * py + 1) / H - 1) * tany * z, z], dim=1)
    q = torch.randn(n, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    scales = (0.4 + 0.2 * torch.rand(n, 3, generator=g)) * z[:, None] / focal
    opac = 0.02 + 0.02 * torch.rand(n, 1, generator=g)
    col = torch.rand(n, 3, generator=g)
    zbits = z.numpy().view(np.uint32).astype(np.int64)
    members = [np.nonzero(tile_of.numpy() == t)[0] for t in range(len(lengths))]
    # the reference order of every list: ascending (depth bits, index)
    expected = [m[np.lexsort((m, zbits[m]))] for m in members]
    fr = dict(lengths=list(lengths), W=W, H=H, n=n, means=means, q=q, scales=scales, opac=opac, col=col, z=z, zbits=zbits, expected=expected)
    _BUILT[key] = fr
    return fr


# ---------------------------------------------------------------------------------------------------- unit levels
def unit_level_for(instances, min_units):
    """gs_unit_level_for (csrc/common.h), restated"""
    level = 0
    while level + 1 < GS_UNIT_LEVELS and (instances >> (7 + level)) >= min_units:
        level += 1
    return level


def min_units_for(instances, level):
    """A value of the mi355gs_tune_min_units knob that puts a frame of `instances` at `level`: level L needs
    instances >> (6 + L) >= min_units and, below the top level, instances >> (7 + L) < min_units."""
    mu = (instances >> 7) + 1 if level == 0 else instances >> (6 + level)
    assert mu >= 1 and (level == 0 or instances >> (6 + level) >= mu) and (level == GS_UNIT_LEVELS - 1 or instances >> (7 + level) < mu)
    assert unit_level_for(instances, mu) == level
    return mu


def at_level(fr, level):
    """with at_level(frame, level): the knob is set so that the frame runs at that unit level, and restored afterwards"""
    return frame_abi.knobs(min_units=min_units_for(fr["n"], level))


# ---------------------------------------------------------------------------------------------------- exact lists
def device_lists(dev, fr, fill=0):
    """The frame through the C ABI (preprocess, then the training forward) with the knobs as they stand; every byte of `binning`
    pre-filled with `fill`.  The precondition of every check on these frames is asserted here: each tile's count is the case's,
    and the depth word of every geometry record has the bits of the z handed in.  Returns dict(start, lst, seg_first, part_first,
    meta, count)."""
    W, H, n = fr["W"], fr["H"], fr["n"]
    scene = dict(means=fr["means"], rots=fr["q"], scales=fr["scales"], opac=fr["opac"], colors=fr["col"])
    res = frame_abi.run_frame(dev, scene, frame_abi.identity_camera(W, H), bg=torch.zeros(3), binning_fill=fill)
    v, R, radii = res.views, res.R, res.radii
    assert R == n, (R, n)
    T = v.T
    start, lst, seg_first, part_first = v.np("tile_start"), v.np("list"), v.np("seg_first"), v.np("part_first")
    meta = [int(x) for x in v.np("meta")]
    depth = v.np("rec").view(np.uint32)[:, 11].astype(np.int64)     # the depth word of the record
    want = np.array(fr["lengths"] + [0] * (T - len(fr["lengths"])), dtype=np.int64)
    assert start[0] == 0 and start[T] == R
    assert bool((np.diff(start) == want).all()), (np.diff(start).tolist(), want.tolist())
    assert bool((depth == fr["zbits"]).all())
    assert int((radii > 0).sum()) == n
    return dict(start=start, lst=lst, seg_first=seg_first, part_first=part_first, meta=meta, count=want)


def assert_lists_exact(fr, res, what):
    start, lst = res["start"], res["lst"]
    for tile, want in enumerate(fr["expected"]):
        mine = lst[start[tile]: start[tile + 1]]
        if not np.array_equal(mine, want):
            bad = np.nonzero(mine != want)[0]
            raise AssertionError("tile %d, %d keys (%s), %s: %d entries differ, the first at %d: device %d, expected %d"
                                 % (tile, len(want), sort_path(len(want)), what, len(bad), bad[0], mine[bad[0]], want[bad[0]]))


def check_lists_and_units(dev, fr, level):
    """Every tile's list is numpy's lexsort over (depth bits, index) of the Gaussians placed in it, element for element; the scan's
    unit tables at this level are their definitions: meta[2] chunks per unit, ceil(n / U) units and (n % U != 0) short units per
    tile in the differences of seg_first and part_first, their totals in meta[1] and meta[3]."""
    if 0 in fr["lengths"]:
        assert_unit_frame_holds_every_levels_edges()
    # `binning` pre-filled with 0xFF bytes: an entry the sort never wrote reads 0xFFFFFFFF and cannot pass as Gaussian 0.  The
    # composite that follows the sort in the same call would fetch the record of that index, far outside `geom` — so the frame
    # runs with a zero fill first, where such an entry reads as Gaussian 0 and every wrong list but one (the missing entry is
    # Gaussian 0's own) fails right here, before anything is fetched through it.
    for fill in (0, 0xFF):
        with at_level(fr, level):
            res = device_lists(dev, fr, fill=fill)
        assert_lists_exact(fr, res, "level %d, fill %#x" % (level, fill))
    count = res["count"]
    U = GS_SEG << level
    meta = res["meta"]
    assert meta[2] == 1 << level, (meta, level)
    units, short = (count + U - 1) // U, (count % U != 0).astype(np.int64)
    assert res["seg_first"][0] == 0 and res["part_first"][0] == 0
    assert np.array_equal(np.diff(res["seg_first"]), units), (level, np.diff(res["seg_first"]).tolist(), units.tolist())
    assert np.array_equal(np.diff(res["part_first"]), short), (level, np.diff(res["part_first"]).tolist(), short.tolist())
    assert meta[1] == int(units.sum()) == int(res["seg_first"][-1]) and meta[3] == int(short.sum()) == int(res["part_first"][-1]), meta
    for tile in np.nonzero(count == 0)[0]:
        assert res["seg_first"][tile + 1] == res["seg_first"][tile] and res["part_first"][tile + 1] == res["part_first"][tile]
    return res


def assert_unit_frame_holds_every_levels_edges():
    """The unit frame holds U - 1, U, U + 1, 2 U - 1, 2 U, 2 U + 1 of every level, a multiple of U directly before the list one
    longer, and an empty tile between two non-empty ones."""
    f = FRAMES[UNIT_FRAME]
    for U in unit_lengths():
        for n in (U - 1, U, U + 1, 2 * U - 1, 2 * U, 2 * U + 1):
            assert n in f, (U, n)
        assert f[f.index(U) + 1] == U + 1 and f[f.index(2 * U) + 1] == 2 * U + 1
    e = f.index(0)
    assert 0 < e < len(f) - 1 and f[e - 1] > 0 and f[e + 1] > 0


# ---------------------------------------------------------------------------------------------------- composite
def oracle_errors(out):
    """{image | gradient tensor: (fp32 oracle's, device's)} errors against the float64 oracle, as assert_no_worse_than_fp32_oracle
    measures them: largest absolute difference of the image, relative L2 of each gradient"""
    t = out["f64"]
    res = {"image": tuple(float((out[w]["color"].double() - t["color"]).abs().max()) for w in ("ref", "dut"))}
    for k, g in t["grads"].items():
        n = float(g.norm()) + 1e-30
        res["grad " + k] = tuple(float((out[w]["grads"][k].double() - g).norm()) / n for w in ("ref", "dut"))
    return res


def assert_within_oracle_limits(out, label, factor=2.0, floor=1e-4):
    """assert_no_worse_than_fp32_oracle with its own factor and floor, each measured error also through ops_util.bound (a
    GS_CALIBRATE=1 run prints them instead of failing)"""
    errs = oracle_errors(out)
    assert set(errs) == {"image", "grad means3D", "grad scales", "grad rot", "grad op", "grad col", "grad means2D"}
    for k, (e_ref, e_dut) in errs.items():
        print("%s %-13s fp32 oracle %.3e  device %.3e  (vs float64)" % (label, k, e_ref, e_dut))
    for k, (e_ref, e_dut) in errs.items():
        ops_util.bound("tile lengths/%s/%s" % (label, k), e_dut, max(factor * e_ref, floor))
    if os.environ.get("GS_CALIBRATE") != "1":
        assert_no_worse_than_fp32_oracle(out, factor=factor, floor=floor)
    return errs


def run_frame(dev, fr, reuse=None):
    return run_custom_case(dev, fr["means"], fr["scales"], fr["q"], fr["opac"], fr["col"], fr["W"], fr["H"], reuse=reuse)


def check_composite_at_every_level(dev, index):
    """The frame through the operator at unit levels 0 ... 3 (the level is k_scan_tiles's function of the frame's instance count
    and the knob: read back as meta[2] from the same frame through the C ABI under the same knob) and once through both oracles:
    image and radii bit-identical across the levels, the gradients equal to level 0's up to the order of the float atomics; image
    and every gradient, per level, no further from the float64 oracle than max(1e-4, 2 x the fp32 oracle's own error)."""
    fr = build_frame(FRAMES[index])
    label = FRAME_IDS[index]
    if index == UNIT_FRAME:
        assert_unit_frame_holds_every_levels_edges()
    outs = []
    for level in range(GS_UNIT_LEVELS):
        with at_level(fr, level):
            res = device_lists(dev, fr)
            assert_lists_exact(fr, res, "level %d" % level)   # (the operator's composite fetches records through these lists)
            assert res["meta"][2] == 1 << level
            outs.append(run_frame(dev, fr, reuse=outs[0] if outs else None))
    mism = outs[0]["dut"]["radii"] != outs[0]["ref"]["radii"]     # assert_raster_parity's bound on the radii
    assert bool((outs[0]["dut"]["radii"] > 0).all()) and float(mism.float().mean()) <= 1e-4
    assert int((outs[0]["dut"]["radii"] - outs[0]["ref"]["radii"]).abs().max()) <= 1
    for level in range(1, GS_UNIT_LEVELS):
        assert torch.equal(outs[0]["dut"]["color"], outs[level]["dut"]["color"]), "image differs between unit levels 0 and %d" % level
        assert torch.equal(outs[0]["dut"]["radii"], outs[level]["dut"]["radii"])
    # ... and the gradients of the longer units are the one-chunk path's up to the order of the float atomics: the bound
    # edge_cases.check_multi_chunk_units holds its two unit lengths to
    for level in range(1, GS_UNIT_LEVELS):
        for k, g in outs[0]["dut"]["grads"].items():
            d = float((g - outs[level]["dut"]["grads"][k]).abs().max())
            ops_util.bound("tile lengths/%s/level %d against level 0/grad %s" % (label, level, k), d, 1e-5 * max(1.0, float(g.abs().max())))
    return [assert_within_oracle_limits(out, "%s/level %d" % (label, level)) for level, out in enumerate(outs)]


def check_deterministic_backward(dev, level=1):
    """The frame with a two-run list and a long one, deterministic backward on (set before the forward: the mode enters the
    layout of the frame's buffers, edge_cases.check_deterministic_toggle_between_forward_and_backward_is_refused): two runs give
    bit-identical gradients, inside the same limits; the image is the default mode's."""
    import instantsplat_amd.diff_gaussian_rasterization as dgr
    fr = build_frame(FRAMES[DET_FRAME])
    assert any("two_runs" in sort_path(n) for n in fr["lengths"]) and any(sort_path(n) == "sort_long_tile" for n in fr["lengths"])
    with at_level(fr, level):
        assert_lists_exact(fr, device_lists(dev, fr), "level %d" % level)
        base = run_frame(dev, fr)
        was = dgr.set_deterministic(True)
        try:
            a = run_frame(dev, fr, reuse=base)
            b = run_frame(dev, fr, reuse=base)
        finally:
            dgr.set_deterministic(was)
    assert torch.equal(a["dut"]["color"], base["dut"]["color"]) and torch.equal(a["dut"]["radii"], base["dut"]["radii"])
    for k in a["dut"]["grads"]:
        assert torch.equal(a["dut"]["grads"][k], b["dut"]["grads"][k]), k
    return assert_within_oracle_limits(a, "%s/deterministic" % FRAME_IDS[DET_FRAME])
