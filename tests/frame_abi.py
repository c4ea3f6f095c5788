"""The rasteriser's raw frame ABI for the tests: the one Python restatement of the scratch layouts of csrc/common.h, named views
of a frame's buffers, the one driver of the three calls, the knobs that enter the layouts, and the comparison of the device's
per-tile lists with the oracle's.

A pull request that moves a field of GeomLayout, TilesLayout, BinningLayout or the gradient scratch repeats the move in the four
*_layout functions below and nowhere else.  FrameViews holds every layout it reads through to the library's own size queries, so
a restatement that has fallen behind fails where a frame is first looked at (and, on the emulated library, in
test_composite_emu.py::test_layout_totals_are_the_librarys), not by reading whatever bytes sit at the old offset."""
import contextlib
import math
import os
import re
import types

import numpy as np
import torch


def source_constants():
    """The constants the layouts are made of, read from csrc/common.h."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "instantsplat_amd", "csrc", "common.h")).read()

    def const(name):
        m = re.search(r"(?:constexpr\s+int\s+%s\s*=|#define\s+%s)\s+(\d+)" % (name, name), hdr)
        assert m, name
        return int(m.group(1))

    def record_bytes(name):
        m = re.search(r"struct alignas\(16\) %s \{(.*?)\n\};" % name, hdr, re.S)
        assert m, name
        members = re.findall(r"^\s*(\w+) \w+;", m.group(1), re.M)
        assert members and set(members) == {"float4"}, (name, members)
        return 16 * len(members)

    res = {k: const(k) for k in ("GS_TILE", "GS_SEG", "GS_UNIT_LEVELS", "GS_BIN_CHUNK", "GS_BIN_ENTRIES")}
    res["REC_BYTES"] = record_bytes("GsRec")
    assert record_bytes("GsGrad") == res["REC_BYTES"]
    return res


_SRC = source_constants()
GS_TILE, GS_SEG, GS_UNIT_LEVELS = _SRC["GS_TILE"], _SRC["GS_SEG"], _SRC["GS_UNIT_LEVELS"]
GS_BIN_CHUNK, GS_BIN_ENTRIES = _SRC["GS_BIN_CHUNK"], _SRC["GS_BIN_ENTRIES"]
REC_BYTES = _SRC["REC_BYTES"]            # GsRec and GsGrad: three float4


# ---------------------------------------------------------------------------------------------------- layouts (csrc/common.h)
def _al(x):
    return (x + 255) & ~255


def _carve(fields):
    out, o = {}, 0
    for name, size in fields:
        out[name] = o
        o += _al(size)
    out["total"] = o
    return out


def geom_layout(P):
    """GeomLayout, restated: byte offsets of the per-Gaussian tables in `geom`"""
    n = max(int(P), 1)
    chunks = (n + GS_BIN_CHUNK - 1) // GS_BIN_CHUNK
    lay = _carve([("rec", n * REC_BYTES), ("cov3D", n * 24), ("rect", n * 8), ("clamped", n), ("depth", n * 4),
                  ("bin_entries", chunks * GS_BIN_ENTRIES * 4), ("bin_n", chunks * 4)])
    lay.update(chunks=chunks)
    return lay


def tiles_layout(W, H):
    """TilesLayout, restated: byte offsets of the per-tile and per-pixel tables in `tiles`"""
    gx, gy = (W + GS_TILE - 1) // GS_TILE, (H + GS_TILE - 1) // GS_TILE
    T, npix = gx * gy, W * H
    lay = _carve([("count", T * 4), ("cursor", T * 4), ("start", (T + 1) * 4), ("final_T", npix * 4), ("n_contrib", npix * 4), ("order", T * 4),
                  ("seg_first", (T + 1) * 4), ("part_first", (T + 1) * 4), ("meta", 16), ("qmax", T * 16)])
    lay.update(gx=gx, gy=gy, T=T)
    return lay


def binning_layout(R, T, min_units, det):
    """BinningLayout, restated: byte offsets in `binning`, max_units and max_chunks for a capacity of R instances.  A render-only
    buffer ends where unit_tile begins."""
    n = max(int(R), 1)
    top = GS_SEG << (GS_UNIT_LEVELS - 1)
    by_chunks, by_rule, by_top = (n + GS_SEG - 1) // GS_SEG, 2 * min_units + 1, (n + top - 1) // top
    max_units = max(min(by_chunks, by_rule), by_top) + max(T, 1)
    max_chunks = by_chunks + 8 * max(T, 1) + 8
    fields = [("keys", n * 8), ("list", n * 4), ("unit_tile", max_units * 16), ("bstate", max_units * 256 * 16), ("hitmask", max_chunks * 4 * 8)]
    if det:
        fields += [("det_rows", n * REC_BYTES), ("det_rowidx", n * 4)]
    lay = _carve(fields)
    lay.update(max_units=max_units, max_chunks=max_chunks)
    return lay


def grad_scratch_layout(P, det):
    """The gradient scratch, restated: the moment records, the 256 bytes of gate flags behind them (gs_grad_gate_offset) and, in the
    deterministic mode, DetScratchLayout behind those"""
    n = max(int(P), 1)
    fields = [("moments", n * REC_BYTES), ("gate", 256)]
    if det:
        fields += [("det_off", (n + 2) * 4), ("det_block_sums", ((n + 1 + 4095) // 4096 + 2) * 4)]
    return _carve(fields)


# ---------------------------------------------------------------------------------------------------- knobs
@contextlib.contextmanager
def knobs(min_units=None, det=None, scale_grad=None):
    """The process-wide knobs a test sets — mi355gs_tune_min_units and the deterministic backward, which both enter the layouts,
    and mi355gs_tune_scale_grad — each written, and restored on exit, only where a value is given."""
    from instantsplat_amd import _lib
    import instantsplat_amd.diff_gaussian_rasterization as dgr
    L = _lib.lib()
    undo = []
    try:
        if scale_grad is not None:
            undo.append((L.mi355gs_tune_scale_grad, L.mi355gs_tune_scale_grad(int(scale_grad))))
        if min_units is not None:
            undo.append((L.mi355gs_tune_min_units, L.mi355gs_tune_min_units(int(min_units))))
        if det is not None:
            undo.append((dgr.set_deterministic, dgr.set_deterministic(bool(det))))
        yield
    finally:
        for restore, old in reversed(undo):
            restore(old)


def current_knobs():
    """(min_units, det) as they stand"""
    from instantsplat_amd import _lib
    L = _lib.lib()
    return int(L.mi355gs_tune_min_units(0)), int(L.mi355gs_tune_deterministic(-1))


# ---------------------------------------------------------------------------------------------------- views
class FrameViews:
    """Named, typed torch views (no copy, on the buffers' device) of a frame's `geom`, `tiles` and `binning`: of a frame of P
    Gaussians and W x H pixels whose `binning` was sized for R instances under the knobs (min_units, det).  `binning` may be a
    render-only buffer (keys and list only) or None (a frame that was only projected).  Integer fields are int32 / int64 views of
    the device's unsigned words; np(name) gives a numpy copy with the unsigned reading.

      geom     rec [P,12] float  rect [P,2]  clamped [P] uint8  depth [P] float  bin_entries [chunks,GS_BIN_ENTRIES]  bin_n [chunks]
      tiles    tile_count [T]  tile_start [T+1]  final_T [H,W] float  n_contrib [H,W]  seg_first [T+1]  part_first [T+1]  meta [4]  qmax [T,4]
      binning  keys [R] int64  list [R]  unit_tile [max_units,4]  bstate [max_units,256,4] float  hitmask [max_chunks,4] int64"""

    def __init__(self, geom, tiles, binning, P, W, H, R, min_units, det):
        from instantsplat_amd import _lib
        L = _lib.lib()
        self.P, self.W, self.H, self.R = int(P), int(W), int(H), int(R)
        g, t = geom_layout(P), tiles_layout(W, H)
        b = binning_layout(R, t["T"], min_units, det)
        self.glay, self.tlay, self.blay = g, t, b
        self.gx, self.gy, self.T, self.max_units, self.max_chunks = t["gx"], t["gy"], t["T"], b["max_units"], b["max_chunks"]
        same = (int(min_units), int(bool(det))) == current_knobs()     # the size queries answer for the knobs as they stand
        with contextlib.nullcontext() if same else knobs(min_units=min_units, det=det):
            want = (L.mi355gs_raster_geom_bytes(P), L.mi355gs_raster_tiles_bytes(W, H), L.mi355gs_raster_binning_bytes(R, W, H),
                    L.mi355gs_raster_binning_bytes_render_only(R, W, H))
        assert (g["total"], t["total"], b["total"], b["unit_tile"]) == want, "a layout moved: restated %s, the library %s" % (
            (g["total"], t["total"], b["total"], b["unit_tile"]), want)
        assert geom.numel() == g["total"] and tiles.numel() == t["total"], (geom.numel(), g["total"], tiles.numel(), t["total"])
        self.render_only = binning is not None and binning.numel() == b["unit_tile"]
        assert binning is None or self.render_only or binning.numel() == b["total"], (binning.numel(), b["unit_tile"], b["total"])
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        T, chunks = t["T"], g["chunks"]
        self._fields = dict(
            rec=(geom, g["rec"], f32, (self.P, REC_BYTES // 4)), rect=(geom, g["rect"], i32, (self.P, 2)), clamped=(geom, g["clamped"], torch.uint8, (self.P,)),
            depth=(geom, g["depth"], f32, (self.P,)), bin_entries=(geom, g["bin_entries"], i32, (chunks, GS_BIN_ENTRIES)), bin_n=(geom, g["bin_n"], i32, (chunks,)),
            tile_count=(tiles, t["count"], i32, (T,)), tile_start=(tiles, t["start"], i32, (T + 1,)), final_T=(tiles, t["final_T"], f32, (self.H, self.W)),
            n_contrib=(tiles, t["n_contrib"], i32, (self.H, self.W)), seg_first=(tiles, t["seg_first"], i32, (T + 1,)),
            part_first=(tiles, t["part_first"], i32, (T + 1,)), meta=(tiles, t["meta"], i32, (4,)), qmax=(tiles, t["qmax"], i32, (T, 4)))
        if binning is not None:
            self._fields.update(keys=(binning, b["keys"], i64, (self.R,)), list=(binning, b["list"], i32, (self.R,)))
        if binning is not None and not self.render_only:
            self._fields.update(unit_tile=(binning, b["unit_tile"], i32, (b["max_units"], 4)), bstate=(binning, b["bstate"], f32, (b["max_units"], 256, 4)),
                                hitmask=(binning, b["hitmask"], i64, (b["max_chunks"], 4)))

    @classmethod
    def of_last_frame(cls, frame):
        """the frame dgr.keep_last_frame(True) kept (dgr._LAST_FRAME), under the knobs as they stand"""
        return cls(frame["geom"], frame["tiles"], frame["binning"], frame["P"], frame["W"], frame["H"], frame["capacity"], *current_knobs())

    def __getattr__(self, name):
        fields = self.__dict__.get("_fields", {})
        if name not in fields:
            raise AttributeError("%s: not a field of this frame's buffers (%s)" % (name, ", ".join(sorted(fields))))
        buf, off, dtype, shape = fields[name]
        return buf[off: off + math.prod(shape) * dtype.itemsize].view(dtype).view(shape)

    def np(self, name):
        """a numpy copy of the field: 1- and 4-byte integers as int64 and 8-byte ones as uint64, both read unsigned"""
        a = getattr(self, name).cpu().numpy()
        if a.dtype == np.int32:
            return a.view(np.uint32).astype(np.int64)
        if a.dtype == np.int64:
            return a.view(np.uint64).copy()
        return a.astype(np.int64) if a.dtype == np.uint8 else a.copy()


# ---------------------------------------------------------------------------------------------------- the three calls
def identity_camera(W, H):
    """The camera most raw-ABI frames use: identity view, 60 degrees across, square pixels."""
    from instantsplat_amd.camera import Camera
    tanx = math.tan(math.radians(60) / 2)
    tany = tanx * H / W
    cam = Camera(0, torch.eye(4), math.radians(60), 2 * math.atan(tany), W, H)
    return dict(W=W, H=H, view=torch.eye(4), proj=cam.projection_matrix, campos=torch.zeros(3), tanx=tanx, tany=tany)


def run_frame(dev, scene, camera, *, bg, sh=None, binning_fill=0, radii_fill=0, dL=None, preprocess_only=False):
    """One frame through the raw C ABI (include/mi355gs.h) with the knobs as they stand: stage 1 (projection, tile counts and
    their scan), the training stage 2 and — with a dL/dpixel — the backward of both.
      scene   means, opac, colors or shs (split storage: shs = the DC coefficient, shs_rest = the others), scales + rots or cov3D,
              and optionally mod (the scale modifier); camera: W, H, view, proj, campos, tanx, tany; sh: the active SH degree
      `binning` is pre-filled with the byte binning_fill, `radii` with radii_fill, every gradient output with NaN.
    -> image, radii (on the device), R, views (a FrameViews) and, after a backward, grads (name -> tensor) and moments (the [P,9]
    view of the gradient scratch).  preprocess_only stops after the first call: R, radii and the views of geom and tiles."""
    from instantsplat_amd import _lib
    dev = torch.device(dev)
    L = _lib.lib()
    t = lambda x: None if x is None else torch.as_tensor(x).float().contiguous().to(dev)
    means, shs, rest, col, opac, scales, rots, cov = (t(scene.get(k)) for k in ("means", "shs", "shs_rest", "colors", "opac", "scales", "rots", "cov3D"))
    opac = opac.reshape(-1)
    P, W, H = means.shape[0], camera["W"], camera["H"]
    D, M = int(sh or 0), 0 if shs is None else shs.shape[1] + (0 if rest is None else rest.shape[1])
    mod, tanx, tany = float(scene.get("mod", 1.0)), camera["tanx"], camera["tany"]
    view, proj, campos, bg = t(camera["view"].reshape(-1)), t(camera["proj"].reshape(-1)), t(camera["campos"]), t(bg)
    geom = torch.zeros(L.mi355gs_raster_geom_bytes(P), dtype=torch.uint8, device=dev)
    tiles = torch.zeros(L.mi355gs_raster_tiles_bytes(W, H), dtype=torch.uint8, device=dev)
    radii = torch.full((P,), radii_fill, dtype=torch.int32, device=dev)
    nr = torch.zeros(1, dtype=torch.int32, device=dev)
    p, stream = _lib.ptr, _lib.stream_ptr(dev)
    min_units, det = current_knobs()
    with _lib.on_device(dev):
        _lib.check(L.mi355gs_raster_forward_preprocess(stream, P, D, M, W, H, p(means), p(shs), p(rest), p(col), p(opac), p(scales), mod, p(rots), p(cov),
                                                       p(view), p(proj), p(campos), tanx, tany, 0, p(radii), p(geom), p(tiles), p(nr), None, None, 0), "preprocess")
        R = int(nr.item())
        if preprocess_only:
            return types.SimpleNamespace(R=R, radii=radii, views=FrameViews(geom, tiles, None, P, W, H, R, min_units, det))
        binning = torch.full((L.mi355gs_raster_binning_bytes(R, W, H),), binning_fill, dtype=torch.uint8, device=dev)
        img = torch.zeros(3, H, W, device=dev)
        _lib.check(L.mi355gs_raster_forward_render(stream, P, W, H, R, p(bg), p(geom), p(tiles), p(binning), p(img), 0), "render")
        res = types.SimpleNamespace(image=img, radii=radii, R=R, views=FrameViews(geom, tiles, binning, P, W, H, R, min_units, det))
        if dL is not None:
            slay = grad_scratch_layout(P, det)
            assert (slay["total"], slay["gate"]) == (L.mi355gs_raster_grad_scratch_bytes(P), L.mi355gs_raster_grad_gate_offset(P)), "a layout moved"
            scratch = torch.zeros(slay["total"], dtype=torch.uint8, device=dev)
            new = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)     # every output row must be written
            d = dict(means3D=new(P, 3), means2D=new(P, 3), colors=new(P, 3), opac=new(P))
            if shs is not None:
                d.update(shs=new(P, shs.shape[1], 3))
            if rest is not None:
                d.update(shs_rest=new(P, rest.shape[1], 3))
            d.update(dict(scales=new(P, 3), rots=new(P, 4)) if cov is None else dict(cov3D=new(P, 6)))
            g_pix, g = t(dL), lambda k: p(d.get(k))
            _lib.check(L.mi355gs_raster_backward(stream, P, D, M, W, H, p(bg), p(means), p(shs), p(rest), p(col), p(opac), p(scales), mod, p(rots), p(cov),
                                                 p(view), p(proj), p(campos), tanx, tany, p(geom), p(tiles), p(binning), R, p(radii), p(img), p(g_pix),
                                                 p(scratch), g("means3D"), g("means2D"), g("shs"), g("shs_rest"), g("colors"), g("opac"), g("scales"),
                                                 g("rots"), g("cov3D"), 0, 0), "backward")
            res.grads = d
            res.moments = scratch[: P * REC_BYTES].view(torch.float32).view(P, REC_BYTES // 4)[:, :9]
    return res


# ---------------------------------------------------------------------------------------------------- lists against the oracle
def lists_against_oracle(views, oracle_aux, W, H):
    """Every per-tile list of the device is a subset of the oracle's list of that tile (the reference's 3-sigma rectangle) in the
    same relative (depth, index) order, and every instance the device left out stays below alpha = 1/255 at every pixel of the
    tile.  -> (instances kept, instances dropped, the largest alpha of a dropped instance)"""
    start, lst, rec = views.np("tile_start"), views.np("list"), views.np("rec").astype(np.float64)
    o_start, o_list = oracle_aux["tile_start"].numpy(), oracle_aux["list"].numpy()
    dropped = kept = 0
    worst = 0.0
    for tile in range(views.T):
        mine = lst[start[tile]:start[tile + 1]]
        theirs = o_list[o_start[tile]:o_start[tile + 1]]
        if len(mine) == 0 and len(theirs) == 0:
            continue
        in_mine = np.isin(theirs, mine)
        assert len(np.unique(mine)) == len(mine) and bool(np.isin(mine, theirs).all()), tile       # subset of the reference's list
        assert bool((theirs[in_mine] == mine).all()), tile                                          # same relative order
        gone = theirs[~in_mine]
        kept += len(mine)
        dropped += len(gone)
        if len(gone) == 0:
            continue
        tx, ty = tile % views.gx, tile // views.gx
        xs = np.arange(tx * GS_TILE, min(tx * GS_TILE + GS_TILE, W), dtype=np.float64)
        ys = np.arange(ty * GS_TILE, min(ty * GS_TILE + GS_TILE, H), dtype=np.float64)
        r = rec[gone]   # x, y, hx, hy | A, C, B (log2-scaled conic), opacity | r, g, b, depth
        dx = r[:, 0, None, None] - xs[None, None, :]
        dy = r[:, 1, None, None] - ys[None, :, None]
        power2 = r[:, 4, None, None] * dx * dx + r[:, 5, None, None] * dy * dy + r[:, 6, None, None] * dx * dy
        alpha = r[:, 7, None, None] * np.exp2(np.minimum(power2, 0.0))
        alpha = np.where(power2 > 0, 0.0, alpha)
        worst = max(worst, float(alpha.max()))
        assert float(alpha.max()) < 1.0 / 255.0, (tile, float(alpha.max()))
    return kept, dropped, worst
