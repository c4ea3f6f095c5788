"""The depth and accumulated-alpha maps of the rasteriser — k_depth_fwd, k_depth_bwd and k_depth_dz of csrc/composite.hip behind
mi355gs_raster_depth_forward / _backward, GaussianRasterizer.forward_depth and gaussian_renderer.render_depth — against float64.
Cases, replays and checks shared by the emulated (CPU) and the GPU test files.

DEFINITIONS (include/mi355gs.h): over a pixel's depth-sorted tile list with the colour walk's rules (composite_cases.replay_forward:
alpha = min(0.99, opacity 2^power2), skip if power2 > 0 or alpha < 1/255, stop in front of the Gaussian that would take T below
1e-4), T_i the transmittance in front of entry i and z_i = GsRec.q2.w,
    depth = sum_i T_i alpha_i z_i,   alpha = 1 - final_T;
backward, back to front with S_i = sum_{j>i} T_j alpha_j z_j:
    dL/dalpha_i = gD (T_i z_i - S_i / (1 - alpha_i)) + gA final_T / (1 - alpha_i),   dL/dz_i += gD T_i alpha_i,
    w_i = (opacity 2^power2) dL/dalpha_i, unclamped; the SEVEN SUMS per Gaussian are those of w (dx, dy, dx^2, dx dy, dy^2, 1) and dL/dz.

THE REFERENCE is a float64 numpy replay of exactly that on the device's own records and lists (composite_cases.replay_forward
decides what blends; replay_depth / replay_depth_backward add the depth terms); the same replay in float32 is the yardstick.  The
code under test is never its own yardstick.  Fragile pixels are composite_cases' (decided from float64 alone, at most 2 % of a
case); gD and gA are seeded normal fields, zero on them.  Limits go through ops_util.bound.

CHECKS
  1 forward: alpha == 1 - final_T of the device bit for bit (every pixel); depth within max(2.5 E_32, FLOOR) of float64 on every
    non-fragile pixel, E_32 the float32 replay's largest error on the case, FLOOR the largest E_32 over the four families.
  2 layout independence: depth and alpha bit-identical after the training forward at unit levels 0 and 3 and after the
    render-only forward.
  3 backward, per Gaussian, for gD alone, gA alone and both: |dev - f64| <= max(2.5 F_m, FLOOR_m) S_im, S the sum of the absolute
    values of the row's terms, F_m the float32 replay's largest |f32 - f64| / S over the case's touched rows (condition, asserted:
    <= composite_cases.F_CAP), FLOOR_m the largest F_m over the families in that mode; a row float64 never blends is exactly
    zero; the colour slots of the scratch records stay zero.  No resume term: the walk is whole-list.
  4 operator, end to end (P = 300, 50 x 37; identity and generic camera; SH degree 3 / precomputed colours; scales + rotations /
    cov3D): both maps and every gradient tensor of sum gC color + sum gD depth + sum gA alpha within rel-L2 1e-4
    of rasterize_depth(), the float64 autograd restatement below on oracle.raster_torch.preprocess; colour and radii are
    forward()'s bits; with gD = gA = 0 the gradients are forward()'s bits (deterministic colour backward: its float atomics
    would otherwise differ between any two runs on the GPU).
  5 render_depth: render / radii / visibility_filter are render()'s bit for bit under the glue render_depth is built from (the
    posed node, render()'s default, applies the pose inside its projection kernel: equal radii and visibility, image within the
    1e-5 the glues are held to among themselves); d(sum gD depth) / d(camera_pose, _xyz) within the same
    criterion of the restatement composed with pose_utils in float64; the same maps under no_grad.
  6 argument checks; the ABI version is still 10.
Further frames: P = 0 (maps zero, every call OK), 1 x 1 and 17 x 33 (checks 1 and 3 with the families' floors), and on the GPU
2049 x 2048 with 2,000 Gaussians (the direct-atomic tile-count class), depth on the 4 x 4 tiles of the far corner.

MEASURED (GS_CALIBRATE=1 and the checks' own prints; emulated kernels / MI355X).  FLOOR (depth) = 4.73e-6, needles' E_32.
  forward, E_dev (E_32):  needles 3.30e-6 / 3.30e-6 (4.73e-6)   opaque 1.63e-6 / 1.63e-6 (1.87e-6)   faint 2.37e-6 / 2.37e-6 (2.77e-6)
                          edges 1.44e-6 / 1.30e-6 (1.54e-6)     17x33 1.32e-6 / 1.32e-6 (1.19e-6)    1x1 2.07e-7 / 2.07e-7 (2.07e-7)
                          2049 x 2048 corner: MI355X 1.89e-6 (E_32 1.89e-6)
  backward, the float32 replay's largest F over the seven sums, gD / gA / both (the condition F <= 2e-5 holds on every family;
  needles under gD alone comes closest, 1.9e-5 on w dy2 — why it stands three times above its colour moments' 6.4e-6 was not looked into):
      needles 1.9e-5 / 1.3e-5 / 1.8e-5   opaque 1.5e-6 / 7.4e-7 / 1.4e-6   faint 8.6e-6 / 5.0e-7 / 4.0e-6   edges 8.4e-6 / 6.0e-7 / 6.8e-6
  backward, worst ratio of check 3 over the seven sums (limit 1): emulated / MI355X
      needles gD 0.41 / 0.41  gA 0.48 / 0.48  both 0.40 / 0.40      opaque gD 0.33 / 0.24  gA 0.14 / 0.13  both 0.25 / 0.21
      faint   gD 0.42 / 0.37  gA 0.15 / 0.08  both 0.42 / 0.51      edges  gD 0.41 / 0.36  gA 0.10 / 0.09  both 0.59 / 0.41
      17x33   both 0.07 / 0.05                                     1x1    both 0.17 / 0.10
  operator and render_depth, worst rel-L2 over maps and gradient tensors (limit 1e-4): emulated 3.4e-6 (grad means2D); on the
  MI355X the tests pass under the limit, the values were not recorded.
"""
import contextlib
import functools
import math
import types

import numpy as np
import torch

from oracle import raster_torch as rt
from tests import composite_cases as cc
from tests import frame_abi, ops_util
from tests import projection_cases as pc
from tests import tile_length_cases as tl
from tests.projection_cases import REL

SUMS = ("w dx", "w dy", "w dx2", "w dxdy", "w dy2", "w", "dz")
MODES = ("gD", "gA", "both")
NAMES = cc.NAMES
SMALL = 1e-4                       # rel-L2 per tensor against float64 at small sizes
EXTRA = {"17x33": (17, 33, 60, 7), "1x1": (1, 1, 12, 9)}     # name -> W, H, Gaussians, seed
LARGE = (2049, 2048, 2000)         # 129 x 128 tiles: the direct-atomic tile-count class (large_grid_cases.SHAPES)
F64 = torch.float64


@contextlib.contextmanager
def frame_size(W, H):
    """composite_cases' replay, tile order and case builder are written for its module-level frame size: another one for a while"""
    old = cc.W, cc.H
    cc.W, cc.H = W, H
    try:
        yield
    finally:
        cc.W, cc.H = old


# ---------------------------------------------------------------------------------------------------- the device side
def _buffers(views):
    """the frame's geom, tiles and binning tensors behind a frame_abi.FrameViews"""
    f = views._fields
    return f["rec"][0], f["tile_start"][0], f["keys"][0] if "keys" in f else None


def depth_frame(dev, scene, camera, *, bg, render_only=False, grads=()):
    """One frame through the raw C ABI with the knobs as they stand: frame_abi.run_frame's stage 1 and training stage 2 (or, with
    render_only, its stage 1 and mi355gs_raster_forward_render_only), then mi355gs_raster_depth_forward and, for every (gD, gA)
    of `grads` ([H,W] arrays or None), mi355gs_raster_depth_backward.  Outputs are pre-filled with NaN and the scratch with the
    byte 0xA5: the calls must write every row and clear what they accumulate into.
    -> depth, alpha, final_T, image [numpy], views, R, and per entry of `grads` a dict: sums [P,7], colour_slots [P,6], the
    gradient tensors by name."""
    from instantsplat_amd import _lib
    dev = torch.device(dev)
    L, p, stream = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    W, H = camera["W"], camera["H"]
    t = lambda x: None if x is None else torch.as_tensor(x).float().contiguous().to(dev)
    if render_only:
        fr = frame_abi.run_frame(dev, scene, camera, bg=bg, preprocess_only=True)
    else:
        fr = frame_abi.run_frame(dev, scene, camera, bg=bg)
    geom, tiles, binning = _buffers(fr.views)
    P, R = fr.views.P, fr.R
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    depth, alpha = nan(H, W), nan(H, W)
    out = []
    with _lib.on_device(dev):
        if render_only:
            binning = torch.zeros(max(int(L.mi355gs_raster_binning_bytes_render_only(R, W, H)), 1), dtype=torch.uint8, device=dev)
            fr.image, bg_dev = torch.zeros(3, H, W, device=dev), t(bg)
            _lib.check(L.mi355gs_raster_forward_render_only(stream, P, W, H, R, p(bg_dev), p(geom), p(tiles), p(binning), p(fr.image), 0), "render_only")
        _lib.check(L.mi355gs_raster_depth_forward(stream, P, W, H, R, p(geom), p(tiles), p(binning), p(depth), p(alpha)), "depth_forward")
        means, scales, rots, cov = (t(scene.get(k)) for k in ("means", "scales", "rots", "cov3D"))
        view, proj, campos = t(camera["view"].reshape(-1)), t(camera["proj"].reshape(-1)), t(camera["campos"])
        nbytes = int(L.mi355gs_raster_depth_scratch_bytes(P))
        n = max(P, 1)
        assert nbytes == frame_abi._al(n * frame_abi.REC_BYTES) + frame_abi._al(n * 4)
        for gD, gA in grads:
            gD, gA = t(gD), t(gA)       # (held: an address outlives a temporary)
            scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
            d = dict(means3D=nan(P, 3), means2D=nan(P, 3), opac=nan(P))
            d.update(dict(scales=nan(P, 3), rots=nan(P, 4)) if cov is None else dict(cov3D=nan(P, 6)))
            g = lambda k: p(d.get(k))
            _lib.check(L.mi355gs_raster_depth_backward(stream, P, W, H, p(means), p(scales), float(scene.get("mod", 1.0)), p(rots), p(cov), p(view), p(proj),
                                                       p(campos), camera["tanx"], camera["tany"], p(geom), p(tiles), p(binning), R, p(fr.radii), p(gD),
                                                       p(gA), p(scratch), g("means3D"), g("means2D"), g("opac"), g("scales"), g("rots"), g("cov3D"), 0),
                       "depth_backward")
            recs = scratch[: P * frame_abi.REC_BYTES].view(torch.float32).view(P, frame_abi.REC_BYTES // 4).cpu().numpy()
            dz = scratch[frame_abi._al(n * frame_abi.REC_BYTES):][: P * 4].view(torch.float32).cpu().numpy()
            out.append(dict({k: v.cpu().numpy() for k, v in d.items()}, sums=np.concatenate([recs[:, :6], dz[:, None]], axis=1), colour_slots=recs[:, 6:]))
    v = fr.views
    return types.SimpleNamespace(depth=depth.cpu().numpy(), alpha=alpha.cpu().numpy(), final_T=v.np("final_T"), image=fr.image.cpu().numpy(), views=v, R=R, P=P,
                                 backward=out)


def run_family(dev, name, level=0, render_only=False, grads=()):
    """a composite_cases family through depth_frame at a unit level (composite_cases.run_device's frame, plus the depth calls)"""
    R = cc.reference(dev, name)["base"]["R"]
    with frame_abi.knobs(min_units=tl.min_units_for(R, level), det=False):
        o = depth_frame(dev, cc._scene(cc.get_case(name)), frame_abi.identity_camera(cc.W, cc.H), bg=cc.BG, render_only=render_only, grads=grads)
    assert o.R == R
    return o


# ---------------------------------------------------------------------------------------------------- the replays
def replay_depth(fwd, records, dtype):
    """depth [tiles, 256] in `dtype` over what composite_cases.replay_forward (same dtype) blended: sum T alpha z, front to back"""
    dt = np.dtype(dtype).type
    rec = np.asarray(records).astype(dtype)
    X, Y, _ = cc.tile_pixels()
    X, Y = X.astype(dtype), Y.astype(dtype)
    ids, blended = fwd["ids"], fwd["blended"]
    Tr, D = np.ones(X.shape, dtype=dtype), np.zeros(X.shape, dtype=dtype)
    for k in range(ids.shape[1]):
        bl = blended[:, k]
        if not bl.any():
            continue
        g = ids[:, k]
        alpha = cc._pair(rec, g, X, Y, dt)[4]
        D = D + np.where(bl, alpha * Tr, dt(0)) * rec[g, 11][:, None]
        Tr = np.where(bl, Tr * (dt(1.0) - alpha), Tr)
    assert np.array_equal(Tr, fwd["T"])
    return D


def replay_depth_backward(fwd, records, gD, gA, dtype):
    """Back to front in `dtype` (gD, gA: [H,W] or None) -> the seven sums per Gaussian M [P,7], the sums of their terms' absolute
    values S [P,7] (float64), and the rows some pixel blends."""
    dt = np.dtype(dtype).type
    rec = np.asarray(records).astype(dtype)
    P = rec.shape[0]
    X, Y, _ = cc.tile_pixels()
    X, Y = X.astype(dtype), Y.astype(dtype)
    ids, blended = fwd["ids"], fwd["blended"]
    field = lambda g: np.zeros(X.shape, dtype=dtype) if g is None else cc.from_image(np.asarray(g)).astype(dtype)
    gD, gA = field(gD), field(gA)
    Tf = fwd["T"]
    Tr, S = Tf.copy(), np.zeros(X.shape, dtype=dtype)
    M, A, touched = np.zeros((P, 7), dtype=dtype), np.zeros((P, 7), dtype=np.float64), np.zeros(P, dtype=bool)
    for k in range(ids.shape[1] - 1, -1, -1):
        bl = blended[:, k]
        rows = bl.any(axis=1)
        if not rows.any():
            continue
        g = ids[:, k]
        dx, dy, _, au, alpha = cc._pair(rec, g, X, Y, dt)
        one_m = dt(1.0) - alpha
        z = rec[g, 11][:, None]
        Tk = np.where(bl, Tr / one_m, Tr)
        w = np.where(bl, au * (gD * (Tk * z - S / one_m) + gA * Tf / one_m), dt(0))
        aT = np.where(bl, alpha * Tk, dt(0))
        S = S + z * aT
        Tr = Tk
        wdx, wdy = w * dx, w * dy
        terms = np.stack([wdx, wdy, wdx * dx, wdx * dy, wdy * dy, w, gD * aT], axis=2)
        np.add.at(M, g[rows], terms.sum(axis=1)[rows])
        np.add.at(A, g[rows], np.abs(terms).astype(np.float64).sum(axis=1)[rows])
        touched[g[rows]] = True
    return dict(M=M, S=A, touched=touched)


def _fields(shape, fragile_image, seed):
    g = torch.Generator().manual_seed(seed)
    gD, gA = (torch.randn(*shape, generator=g, dtype=F64).numpy() * ~fragile_image for _ in range(2))
    return gD.astype(np.float32), gA.astype(np.float32)


def _mode_fields(gD, gA, mode):
    return {"gD": (gD, None), "gA": (None, gA), "both": (gD, gA)}[mode]


def _reference_of(rec, lst, start, seed):
    """both replays, forward and the three backward modes, of one frame's records and lists (under cc.W, cc.H)"""
    f64 = cc.replay_forward(rec, lst, start, cc.BG, np.float64, states=False)
    f32 = cc.replay_forward(rec, lst, start, cc.BG, np.float32, states=False)
    keep = ~f64["fragile"] & f64["inside"]
    share = float(cc.to_image(f64["fragile"]).mean())
    assert share <= cc.FRAGILE_SHARE, share
    assert bool((f32["last"][keep] == f64["last"][keep]).all()), "the two replays decide differently on a non-fragile pixel"
    d64, d32 = replay_depth(f64, rec, np.float64), replay_depth(f32, rec, np.float32)
    gD, gA = _fields((cc.H, cc.W), cc.to_image(f64["fragile"]), seed)
    res = dict(f64=f64, keep=keep, share=share, depth=d64, gD=gD, gA=gA, E32=float(np.abs(d32.astype(np.float64) - d64)[keep].max(initial=0.0)), b64={}, F={})
    for mode in MODES:
        a, b = _mode_fields(gD, gA, mode)
        b64 = replay_depth_backward(f64, rec, a, b, np.float64)
        b32 = replay_depth_backward(f32, rec, a, b, np.float32)
        rows = b64["touched"]
        F = np.zeros(7)
        if rows.any():
            F = (np.abs(b32["M"].astype(np.float64) - b64["M"])[rows] / np.maximum(b64["S"][rows], 1e-300)).max(axis=0)
            F[(b64["S"][rows] == 0).all(axis=0)] = 0.0
        res["b64"][mode], res["F"][mode] = b64, F
    return res


@functools.lru_cache(maxsize=None)
def reference(dev, name):
    """The replays of a family on the records and lists the device made of it (composite_cases.reference's frame), once."""
    base = cc.reference(dev, name)["base"]
    res = _reference_of(base["rec"], base["lst"], base["start"], 1000 + NAMES.index(name))
    for mode in MODES:
        assert float(res["F"][mode].max()) <= cc.F_CAP, (name, mode, res["F"][mode].tolist())
    return res


@functools.lru_cache(maxsize=None)
def floors(dev):
    refs = [reference(dev, n) for n in NAMES]
    return dict(depth=max(r["E32"] for r in refs), F={m: np.max([r["F"][m] for r in refs], axis=0) for m in MODES})


# ---------------------------------------------------------------------------------------------------- checks on the raw ABI
def judge_forward(dev, label, o, ref):
    one_minus = np.float32(1.0) - o.final_T.astype(np.float32)
    assert np.array_equal(o.alpha.view(np.uint32), one_minus.view(np.uint32)), "%s: alpha is not 1 - final_T bit for bit" % label
    assert np.isfinite(o.depth).all()
    keep = ref["keep"]
    e = float(np.abs(cc.from_image(o.depth).astype(np.float64) - ref["depth"])[keep].max(initial=0.0))
    lim = max(REL * ref["E32"], floors(dev)["depth"])
    print("%s depth: E_dev %.2e (E_32 %.2e, limit %.2e), fragile %.2f %%" % (label, e, ref["E32"], lim, 100 * ref["share"]))
    ops_util.bound("depth/%s/depth" % label, e, lim)


def judge_sums(dev, label, mode, got, ref):
    b64, fl = ref["b64"][mode], floors(dev)["F"][mode]
    d = got["sums"].astype(np.float64)
    assert np.isfinite(d).all() and not got["colour_slots"].any()
    idle = ~b64["touched"]
    assert not d[idle].any(), "%s %s: %d rows the float64 replay never blends are not zero" % (label, mode, int(d[idle].any(axis=1).sum()))
    rows = b64["touched"]
    if not rows.any():
        return 0.0
    lim = np.maximum(REL * ref["F"][mode], fl)[None, :] * b64["S"]
    err = np.abs(d - b64["M"])
    ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))[rows]
    print("%s %s: worst ratio %.3f; E_dev/S %s; F %s" % (label, mode, ratio.max(), " ".join("%.1e" % v for v in (err[rows] / np.maximum(b64["S"][rows], 1e-300)).max(axis=0)),
                                                      " ".join("%.1e" % v for v in ref["F"][mode])))
    for m, name in enumerate(SUMS):
        ops_util.bound("depth/%s/%s/sum %s" % (label, mode, name), ratio[:, m].max(), 1.0)
    return float(ratio.max())


def check_forward(dev, name):
    """Check 1 on a family."""
    judge_forward(dev, name, run_family(dev, name), reference(dev, name))


def check_layouts(dev, name):
    """Check 2: the same bits after the training forward at unit levels 0 and 3 and after the render-only forward."""
    a = run_family(dev, name, 0)
    for what, o in (("level 3", run_family(dev, name, cc.LEVELS[-1])), ("render-only", run_family(dev, name, 0, render_only=True))):
        assert np.array_equal(a.final_T, o.final_T) and np.array_equal(a.image, o.image), (name, what)
        assert np.array_equal(a.depth.view(np.uint32), o.depth.view(np.uint32)), (name, what, "depth")
        assert np.array_equal(a.alpha.view(np.uint32), o.alpha.view(np.uint32)), (name, what, "alpha")


def check_backward(dev, name):
    """Check 3 on a family: the seven sums per Gaussian for gD alone, gA alone and both."""
    ref = reference(dev, name)
    o = run_family(dev, name, grads=[_mode_fields(ref["gD"], ref["gA"], m) for m in MODES])
    assert int(ref["b64"]["both"]["touched"].sum()) >= cc.get_case(name)["P"] // 6
    return {m: judge_sums(dev, name, m, got, ref) for m, got in zip(MODES, o.backward)}


def check_gradient_outputs(dev, name="needles"):
    """What leaves the call is what k_preprocess_bwd makes of the sums read above: dL_dopacities is the sum of w over the opacity;
    every output row is written; dL_dmeans3D differs between a run with gD and the same run's moments alone (gD's moments fed
    back as they are, dz left out, is not expressible through the ABI) — so the dz chain itself is judged end to end, under a
    rotated view, by check_operator."""
    ref = reference(dev, name)
    o = run_family(dev, name, grads=[(ref["gD"], ref["gA"])])
    got = o.backward[0]
    s = got["sums"].astype(np.float64)
    assert int((s[:, 5] != 0).sum()) >= 100 and int((s[:, 6] != 0).sum()) >= 100
    op = cc.get_case(name)["opac"].numpy().astype(np.float64)
    want = s[:, 5] / op
    ops_util.bound("depth/%s/dL_dopacities against the sums" % name, (np.abs(got["opac"].astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)).max(), 1e-6)
    for k in ("means3D", "means2D", "scales", "rots"):
        assert np.isfinite(got[k]).all(), k
    assert not got["means2D"][:, 2].any()


def small_frame(dev, name):
    """A seeded frame of another size (EXTRA): -> (device result with one backward in mode "both", its reference)"""
    W, H, n, seed = EXTRA[name]
    with frame_size(W, H):
        case = cc._random_family(name, seed, n, (1.0, 1.0, 1.0), (6.0, 6.0, 6.0), 0.05, 0.95)
        o = depth_frame(dev, cc._scene(case), frame_abi.identity_camera(W, H), bg=cc.BG)
        v = o.views
        ref = _reference_of(v.np("rec"), v.np("list"), v.np("tile_start"), seed)
        o = depth_frame(dev, cc._scene(case), frame_abi.identity_camera(W, H), bg=cc.BG, grads=[(ref["gD"], ref["gA"])])
        assert o.R > 0 and int(ref["b64"]["both"]["touched"].sum()) > 0
        judge_forward(dev, name, o, ref)
        judge_sums(dev, name, "both", o.backward[0], ref)


def check_no_gaussians(dev, W=50, H=37):
    """P = 0: every call returns OK and both maps are zero."""
    e = torch.zeros(0, 3)
    o = depth_frame(dev, dict(means=e, rots=torch.zeros(0, 4), scales=e, opac=torch.zeros(0), colors=e), frame_abi.identity_camera(W, H), bg=cc.BG,
                    grads=[(np.ones((H, W), np.float32), np.ones((H, W), np.float32))])
    assert o.R == 0 and not o.depth.any() and not o.alpha.any()


def check_arguments(dev):
    """Check 6: null geom, tiles or binning with capacity > 0 are refused by both calls; capacity 0 zeroes the maps without
    `binning`; the ABI version has not moved."""
    from instantsplat_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    dev = torch.device(dev)
    assert L.mi355gs_abi_version() == 10 == _lib.ABI_VERSION
    EINVAL, W, H, P = -1, 16, 16, 4
    buf = lambda n: torch.zeros(max(int(n), 1), dtype=torch.uint8, device=dev)
    geom, tiles, binning = buf(L.mi355gs_raster_geom_bytes(P)), buf(L.mi355gs_raster_tiles_bytes(W, H)), buf(L.mi355gs_raster_binning_bytes(64, W, H))
    depth, alpha = torch.ones(H, W, device=dev), torch.ones(H, W, device=dev)
    stream = _lib.stream_ptr(dev)
    with _lib.on_device(dev):
        for g, t, b in ((None, tiles, binning), (geom, None, binning), (geom, tiles, None)):
            assert L.mi355gs_raster_depth_forward(stream, P, W, H, 64, p(g), p(t), p(b), p(depth), p(alpha)) == EINVAL
        assert L.mi355gs_raster_depth_forward(stream, P, 0, H, 64, p(geom), p(tiles), p(binning), p(depth), p(alpha)) == EINVAL
        assert L.mi355gs_raster_depth_forward(stream, P, W, H, 0, p(geom), p(tiles), None, p(depth), None) == 0
        assert not depth.cpu().any() and bool((alpha.cpu() == 1).all())          # a null output is left alone
        f = lambda *s: torch.zeros(*s, device=dev)
        means, scales, rots, radii = f(P, 3), f(P, 3), f(P, 4), torch.zeros(P, dtype=torch.int32, device=dev)
        cam = frame_abi.identity_camera(W, H)
        view, proj, campos = (x.float().contiguous().to(dev) for x in (cam["view"].reshape(-1), cam["proj"].reshape(-1), cam["campos"]))
        scratch = buf(L.mi355gs_raster_depth_scratch_bytes(P))
        outs = [f(P, 3), f(P, 3), f(P), f(P, 3), f(P, 4)]

        def backward(g, t, b, cap, s=scratch, o0=outs[0]):
            return L.mi355gs_raster_depth_backward(stream, P, W, H, p(means), p(scales), 1.0, p(rots), None, p(view), p(proj), p(campos), cam["tanx"], cam["tany"],
                                                   p(g), p(t), p(b), cap, p(radii), p(depth), p(alpha), p(s), p(o0), p(outs[1]), p(outs[2]), p(outs[3]),
                                                   p(outs[4]), None, 0)
        for g, t, b in ((None, tiles, binning), (geom, None, binning), (geom, tiles, None)):
            assert backward(g, t, b, 64) == EINVAL
        assert backward(geom, tiles, binning, 64, s=None) == EINVAL and backward(geom, tiles, binning, 64, o0=None) == EINVAL
        for o_ in outs:
            o_.fill_(float("nan"))
        assert backward(geom, tiles, None, 0) == 0                                # capacity 0: OK, zeroed outputs
        assert all(not o_.cpu().any() for o_ in outs)
    assert L.mi355gs_raster_depth_scratch_bytes(0) == L.mi355gs_raster_depth_scratch_bytes(1) == 512


def check_large_frame(dev):
    """2049 x 2048, 2,000 Gaussians: depth on the 4 x 4 tiles of the far corner (a one-pixel last tile column) against the two
    replays, the tile and record indices of the whole frame behind them."""
    W, H, n = LARGE
    g = torch.Generator().manual_seed(17)
    tanx = math.tan(math.radians(60) / 2)
    tany, focal = tanx * H / W, W / (2 * tanx)
    z = 2.0 + 4.0 * torch.rand(n, generator=g)
    ndc = 1.04 * (2 * torch.rand(n, 2, generator=g) - 1)
    ndc[: n // 4] = 0.93 + 0.09 * torch.rand(n // 4, 2, generator=g)             # a quarter of them crowd the far corner
    means = torch.stack([ndc[:, 0] * tanx * z, ndc[:, 1] * tany * z, z], dim=1)
    q = torch.randn(n, 4, generator=g)
    sigma_px = 1.0 + 24.0 * torch.rand(n, 3, generator=g) ** 2
    scene = dict(means=means, rots=q / q.norm(dim=1, keepdim=True), scales=sigma_px * z[:, None] / focal, opac=0.05 + 0.9 * torch.rand(n, generator=g),
                 colors=torch.rand(n, 3, generator=g))
    o = depth_frame(dev, scene, frame_abi.identity_camera(W, H), bg=cc.BG)
    v = o.views
    assert (v.gx, v.gy) == (129, 128)
    start, lst, rec = v.np("tile_start"), v.np("list"), v.np("rec").astype(np.float64)
    tx0, ty0 = v.gx - 4, v.gy - 4
    tiles = [ty * v.gx + tx for ty in range(ty0, v.gy) for tx in range(tx0, v.gx)]
    sub_list = np.concatenate([lst[start[t]: start[t + 1]] for t in tiles])
    sub_start = np.concatenate([[0], np.cumsum([start[t + 1] - start[t] for t in tiles])])
    assert len(sub_list) >= 200
    rec[:, 0] -= 16 * tx0                                                         # exact in float32 as well: the centres move with the crop
    rec[:, 1] -= 16 * ty0
    Wc, Hc = W - 16 * tx0, H - 16 * ty0
    with frame_size(Wc, Hc):
        ref = _reference_of(rec, sub_list, sub_start, 5)
        crop = types.SimpleNamespace(depth=o.depth[16 * ty0:, 16 * tx0:].copy(), alpha=o.alpha[16 * ty0:, 16 * tx0:].copy(), final_T=o.final_T[16 * ty0:, 16 * tx0:].copy())
        assert float(ref["depth"].max()) > 1.0
        judge_forward(dev, "%dx%d corner" % (W, H), crop, ref)
    assert np.isfinite(o.depth).all() and float(o.depth.min()) >= 0.0 and float(o.alpha.min()) >= 0.0 and float(o.alpha.max()) <= 1.0


# ---------------------------------------------------------------------------------------------------- the operator, end to end
def rasterize_depth(means3D, opacities, settings, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None, means2D=None):
    """oracle.raster_torch.rasterize's blend on oracle.raster_torch.preprocess, with the two maps added:
    -> (color [3,H,W], radii [P], depth [1,H,W] = wgt @ view depth, alpha [1,H,W] = 1 - final_T).  Dense, autograd-differentiable."""
    dt = means3D.dtype
    W, H = settings.image_width, settings.image_height
    g = rt.preprocess(means3D, opacities, settings, shs, colors_precomp, scales, rotations, cov3D_precomp, means2D)
    idx = torch.nonzero(g["visible"]).reshape(-1)
    order = torch.argsort(g["depth"].detach().to(torch.float32)[idx].contiguous().view(torch.int32), stable=True)
    idx = idx[order]
    assert idx.numel() > 0
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    pixx, pixy = xs.reshape(-1).to(dt), ys.reshape(-1).to(dt)
    tix, tiy = xs.reshape(-1) // rt.TILE, ys.reshape(-1) // rt.TILE
    rect = g["rect"][idx]
    in_rect = (tix[:, None] >= rect[None, :, 0]) & (tix[:, None] < rect[None, :, 2]) & (tiy[:, None] >= rect[None, :, 1]) & (tiy[:, None] < rect[None, :, 3])
    dx, dy = g["px"][idx][None, :] - pixx[:, None], g["py"][idx][None, :] - pixy[:, None]
    con = g["conic"][idx]
    power = -0.5 * (con[None, :, 0] * dx * dx + con[None, :, 2] * dy * dy) - con[None, :, 1] * dx * dy
    raw_alpha = g["opacity"][idx][None, :] * torch.exp(power)
    alpha = raw_alpha + (torch.clamp(raw_alpha, max=0.99) - raw_alpha).detach()       # straight-through min(0.99, .)
    keep = in_rect & (power.detach() <= 0) & (alpha.detach() >= 1.0 / 255.0)
    alpha = torch.where(keep, alpha, torch.zeros_like(alpha))
    one_m = 1.0 - alpha
    Tincl = torch.cumprod(one_m, dim=1)
    Texcl = torch.cat([torch.ones_like(Tincl[:, :1]), Tincl[:, :-1]], dim=1)
    alive = Tincl.detach() >= 1e-4
    wgt = torch.where(alive & keep, alpha * Texcl, torch.zeros_like(alpha))
    final_T = torch.where(alive, one_m, torch.ones_like(one_m)).prod(dim=1)
    color = (wgt @ g["rgb"][idx] + final_T[:, None] * settings.bg.to(dt).reshape(3)[None, :]).t().reshape(3, H, W)
    return color, g["radius"], (wgt @ g["depth"][idx]).reshape(1, H, W), (1.0 - final_T).reshape(1, H, W)


OPERATOR_CASES = {   # name -> projection_cases.build_case arguments: both cameras, both colour forms, both covariance forms
    "identity/sh3": dict(camera="identity", deg=3), "generic/sh3": dict(camera="generic", deg=3),
    "generic/colors": dict(camera="generic", colors=True), "identity/cov3D": dict(camera="identity", deg=3, cov=True),
    "generic/colors+cov3D": dict(camera="generic", colors=True, cov=True),
}


@functools.lru_cache(maxsize=None)
def operator_case(name):
    case = pc.build_case("blob", P=300, W=cc.W, H=cc.H, seed=23, name="depth/" + name, **OPERATOR_CASES[name])
    g = torch.Generator().manual_seed(77)
    case.gD, case.gA = torch.randn(1, cc.H, cc.W, generator=g), torch.randn(1, cc.H, cc.W, generator=g)
    return case


@functools.lru_cache(maxsize=None)
def operator_reference(name):
    case = operator_case(name)
    lv, m2d = pc._leaves(case, F64, "cpu")
    color, radii, depth, alpha = rasterize_depth(lv["means3D"], lv["opac"], pc.settings(case, rt.RasterSettings, F64), means2D=m2d, **pc._raster_kwargs(lv))
    ((color * case.wgt.to(F64)).sum() + (depth * case.gD.to(F64)).sum() + (alpha * case.gA.to(F64)).sum()).backward()
    return dict(pc._collect(lv, m2d, color, radii), depth=depth.detach(), alpha=alpha.detach())


def _run_operator(dev, case, depth_maps, gD=None, gA=None):
    from instantsplat_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    lv, m2d = pc._leaves(case, torch.float32, dev)
    r = GaussianRasterizer(pc.settings(case, GaussianRasterizationSettings, torch.float32, dev))
    kw = dict(means3D=lv["means3D"], means2D=m2d, opacities=lv["opac"], **pc._raster_kwargs(lv))
    if depth_maps:
        color, radii, depth, alpha = r.forward_depth(**kw)
        loss = (color * case.wgt.to(dev)).sum()
        if gD is not None:
            loss = loss + (depth * gD.to(dev)).sum() + (alpha * gA.to(dev)).sum()
    else:
        color, radii = r(**kw)
        depth = alpha = None
        loss = (color * case.wgt.to(dev)).sum()
    loss.backward()
    return dict(pc._collect(lv, m2d, color, radii), depth=None if depth is None else depth.detach().cpu(), alpha=None if alpha is None else alpha.detach().cpu())


def check_operator(dev, name):
    """Check 4."""
    dev = torch.device(dev)
    case, ref = operator_case(name), operator_reference(name)
    out = _run_operator(dev, case, True, case.gD, case.gA)
    assert out["depth"].shape == (1, case.H, case.W) == out["alpha"].shape
    for k in ("depth", "alpha"):
        ops_util.bound("depth/operator/%s/%s" % (name, k), ops_util.rel_l2(out[k], ref[k]), SMALL)
    assert set(out["grads"]) == set(ref["grads"])
    for k, g in out["grads"].items():
        assert float(ref["grads"][k].norm()) > 0, k
        ops_util.bound("depth/operator/%s/grad %s" % (name, k), ops_util.rel_l2(g, ref["grads"][k]), SMALL)
    with frame_abi.knobs(det=True):     # the colour backward's float atomics differ between two runs on the GPU
        plain = _run_operator(dev, case, False)
        zero = _run_operator(dev, case, True, torch.zeros_like(case.gD), torch.zeros_like(case.gA))
        unused = _run_operator(dev, case, True)
    assert torch.equal(out["color"], plain["color"]) and torch.equal(out["radii"], plain["radii"])
    for other in (zero, unused):
        assert torch.equal(other["color"], plain["color"])
        for k, g in plain["grads"].items():
            assert torch.equal(other["grads"][k], g), (name, k)


def check_operator_no_grad(dev, name="generic/sh3"):
    """under no_grad the operator takes the render-only stage 2 and gives the same maps"""
    from instantsplat_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    import instantsplat_amd.diff_gaussian_rasterization as dgr
    dev = torch.device(dev)
    case = operator_case(name)
    out = _run_operator(dev, case, True, case.gD, case.gA)
    lv, m2d = pc._leaves(case, torch.float32, dev)
    dgr.keep_last_frame(True)
    try:
        with torch.no_grad():
            color, radii, depth, alpha = GaussianRasterizer(pc.settings(case, GaussianRasterizationSettings, torch.float32, dev)).forward_depth(
                means3D=lv["means3D"], means2D=m2d, opacities=lv["opac"], **pc._raster_kwargs(lv))
        assert frame_abi.FrameViews.of_last_frame(dgr._LAST_FRAME).render_only
    finally:
        dgr.keep_last_frame(False)
    assert not depth.requires_grad
    assert torch.equal(color.cpu(), out["color"]) and torch.equal(depth.cpu(), out["depth"]) and torch.equal(alpha.cpu(), out["alpha"])


# ---------------------------------------------------------------------------------------------------- render_depth
def check_render_depth(dev, python_flags=False):
    """Check 5."""
    import instantsplat_amd.gaussian_renderer as gr
    from instantsplat_amd.pose_utils import get_camera_from_tensor, quadmultiply
    from instantsplat_amd.synthetic import syn_pointmap
    from instantsplat_amd.train import setup_training
    st = ops_util.generic_start(setup_training(syn_pointmap(3, 24, 24, 64, 64, seed=5), dev))
    g, cam = st.gaussians, st.cameras[1]
    g.active_sh_degree = 2
    with torch.no_grad():
        g._features_rest.copy_(0.05 * torch.randn(g._features_rest.shape, generator=torch.Generator().manual_seed(3)).to(dev))
    old = st.pipe.compute_cov3D_python, st.pipe.convert_SHs_python
    st.pipe.compute_cov3D_python = st.pipe.convert_SHs_python = bool(python_flags)
    try:
        H, W = int(cam.image_height), int(cam.image_width)
        gD = torch.randn(1, H, W, generator=torch.Generator().manual_seed(9))
        pose = g.get_RT(cam.uid)
        # render() under the glue render_depth is built from (pose / activation node + SH view + operator; the python-flag
        # variants have one glue only): the same kernels, so the same bits.  The default glue of render() is the posed node,
        # whose projection kernel applies the pose itself: its image is held to the bound the glues are held to among
        # themselves (ops_util.check_fused_render_equals_unfused), its radii and visibility are equal.
        default = gr.FUSED_GLUE
        gr.FUSED_GLUE = True
        try:
            base = gr.render(cam, g, st.pipe, st.background, camera_pose=pose)
        finally:
            gr.FUSED_GLUE = default
        with torch.no_grad():
            posed = gr.render(cam, g, st.pipe, st.background, camera_pose=pose)
        assert torch.equal(posed["radii"], base["radii"]) and torch.equal(posed["visibility_filter"], base["visibility_filter"])
        ops_util.bound("depth/render_depth/image against the posed node", (posed["render"] - base["render"].detach()).abs().max(), 1e-5)
        for t in (g._xyz, g.P):
            t.grad = None
        pkg = gr.render_depth(cam, g, st.pipe, st.background, camera_pose=pose)
        assert set(pkg) == set(base) | {"depth", "alpha"} and pkg["depth"].shape == (1, H, W) == pkg["alpha"].shape
        assert torch.equal(pkg["render"], base["render"]) and torch.equal(pkg["radii"], base["radii"])
        assert torch.equal(pkg["visibility_filter"], base["visibility_filter"])
        (pkg["depth"] * gD.to(dev)).sum().backward()
        got = dict(xyz=g._xyz.grad.detach().cpu().clone(), pose=g.P.grad.detach().cpu().clone())
        with torch.no_grad():
            again = gr.render_depth(cam, g, st.pipe, st.background, camera_pose=g.get_RT(cam.uid))
        assert torch.equal(again["depth"], pkg["depth"]) and torch.equal(again["alpha"], pkg["alpha"]) and torch.equal(again["render"], pkg["render"])
        assert float(got["xyz"].abs().max()) > 0 and float(got["pose"][cam.uid].abs().max()) > 0
        if python_flags:    # (the python-flag variants hand over world-frame covariances, as the reference does: not what is restated below)
            return
        # the restatement in float64, composed with pose_utils as render_depth's glue composes the operator
        xyz, Pm = g._xyz.detach().cpu().to(F64).requires_grad_(True), g.P.detach().cpu().to(F64).requires_grad_(True)
        p64 = Pm[cam.uid]
        w2c = get_camera_from_tensor(p64)
        d = lambda t: t.detach().cpu().to(F64)
        settings = rt.RasterSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), d(st.background), 1.0, torch.eye(4, dtype=F64),
                                     d(cam.projection_matrix), g.active_sh_degree, torch.zeros(3, dtype=F64), False, False)
        shs = torch.cat([d(g._features_dc), d(g._features_rest)], dim=1)
        _, _, depth, alpha = rasterize_depth(xyz @ w2c[:3, :3].t() + w2c[:3, 3], torch.sigmoid(d(g._opacity)), settings, shs=shs,
                                             scales=torch.exp(d(g._scaling)), rotations=quadmultiply(p64[:4], d(g._rotation)))
        (depth * gD.to(F64)).sum().backward()
        what = "python flags" if python_flags else "default"
        ops_util.bound("depth/render_depth/%s/depth" % what, ops_util.rel_l2(pkg["depth"], depth), SMALL)
        ops_util.bound("depth/render_depth/%s/alpha" % what, ops_util.rel_l2(pkg["alpha"], alpha), SMALL)
        ops_util.bound("depth/render_depth/%s/grad _xyz" % what, ops_util.rel_l2(got["xyz"], xyz.grad), SMALL)
        ops_util.bound("depth/render_depth/%s/grad camera_pose" % what, ops_util.rel_l2(got["pose"][cam.uid], Pm.grad[cam.uid]), SMALL)
    finally:
        st.pipe.compute_cov3D_python, st.pipe.convert_SHs_python = old
