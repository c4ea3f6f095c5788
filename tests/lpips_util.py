"""Checks of LPIPS-VGG (instantsplat_amd/lpips.py, csrc/lpips.hip), shared by the emulated tier (test_lpips_emu.py, CPU tensors) and
the MI355X (test_lpips_gpu.py).

YARDSTICKS.  `forward_ref(..., torch.float64)` restates the reference's forward (lpipsPyTorch/modules/{lpips,networks,utils}.py:
z_score, the VGG16 feature stack, normalize_activation, the squared difference through the 1x1 lin layers, the spatial mean, the
sum of the five terms) with torch's CPU ops in float64 on the float32 quotient byte / 255; `torch.float32` is its twin, the
arithmetic the reference itself runs.  The twin's distance from float64, E32, is the unit of every bound: per case (one call's
pairs) the largest relative error of a pair's total, and the largest relative error of any tap of any pair.  Relative means
divided by the float64 value computed with |lin| — the value itself for the usual non-negative lin weights, and a scale that
cannot cancel to zero for the signed case.

For the total, E32 is the twin's error or the root-sum-square of its five tap errors, whichever is larger: with signed lin weights
the tap errors can cancel in the twin's sum by luck (seen: 5.5e-8 against 1.3e-7), which says nothing about another summation.

BOUNDS.  A pair's total and taps must be within FACTOR x E32 of float64, and every total within TOTAL_REL = 1e-4 (the fourth decimal
the files print) whatever E32 is.  Why the device sits several E32 out: it sums a convolution's K <= 4608 products in ONE k-ordered
fmaf chain (the matrix instruction's rounding), torch's float32 convolution in blocked partial sums; a chain's error grows like
sqrt(K) to K times half an ulp where a blocked sum's stays near sqrt(K / block), i.e. a few times smaller (the instruction's
documented error is 3.5e-7 sum|a b| at K = 4096 against 0.75 - 1.5e-7 at K <= 1024), and E32 itself moves by 2x from case to case
and by 20 % between machines (torch's CPU convolution splits its sums by thread count).  The factor was set from the MI355X run:
MEASURED (the case with the largest ratio, and the one with the largest error, per tier):
  tier                          E32 total   device total   ratio   E32 tap    device tap   ratio
  MI355X, real widths, mixed    4.8e-7      3.0e-6         6.3     1.1e-6     8.4e-6       7.4     (16x16 N=3 | 37x50 N=2)
  MI355X, real widths, largest  1.1e-6      3.8e-6         3.4     3.7e-5     1.4e-4       3.8     (33x16 | the four corners)
  MI355X, real widths, signed   1.4e-7      1.2e-6         8.3     1.2e-6     7.2e-6       6.3
  MI355X, real widths, bias-.5  4.5e-7      1.8e-7         0.4     5.2e-7     4.1e-7       0.8
  thin net, MI355X = emulator   1.3e-6      2.4e-7         0.2     5.4e-6     1.8e-5       3.3     (16x16 N=3; equal digits on both)
  thin net, corners, emulator   2.7e-6      5.9e-6         2.2     9.6e-5     2.2e-4       2.3
  recording (golden), both      8.2e-7      3.1e-6         3.8     6.7e-6     2.5e-5       3.7     (device against the reference's float32)
The largest total error seen anywhere is 3.8e-6 relative: 26x inside TOTAL_REL.  FACTOR = 16 is twice the largest ratio (8.3).
Identical frames must give exactly 0.0 (total and taps); (a, b) and (b, a), and two runs of one call, equal bits.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import metrics_util as mu
from tests import ops_util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THIN = (32, 32, 64, 64, 96)
REAL = (64, 128, 256, 512, 512)
CONV_LAYERS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
BLOCK_CONVS = (2, 2, 3, 3, 3)
FACTOR = 16.0
TOTAL_REL = 1e-4
# (H, W, N): the smallest shapes that reach each path — odd sizes (every pool floors: 18x25, 9x12, 4x6, 2x3); block 5 of one pixel
# and a batch; one pixel past a tile in each direction; (GPU only) several workgroups per image
SHAPES = ((37, 50, 2), (16, 16, 3), (33, 16, 2), (16, 33, 2))
SHAPES_GPU = SHAPES + ((96, 160, 1),)


# ---------------------------------------------------------------------------------------------------- weights and frames
@functools.lru_cache(maxsize=None)
def make_weights(channels, seed=0, signed_lin=False, bias_shift=0.0):
    """(vgg_state, lin_state) in the official files' naming: He-scaled convolutions (std sqrt(2 / (9 Cin))), biases N(0, 0.1^2)
    + bias_shift, lin weights |N(0,1)| (signed_lin: N(0,1))"""
    g = torch.Generator().manual_seed(1234 + seed)
    vgg, lin, cin, i = {}, {}, 3, 0
    for blk, count in enumerate(BLOCK_CONVS):
        for _ in range(count):
            c = channels[blk]
            vgg[f"features.{CONV_LAYERS[i]}.weight"] = torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
            vgg[f"features.{CONV_LAYERS[i]}.bias"] = torch.randn(c, generator=g) * 0.1 + bias_shift
            cin, i = c, i + 1
        w = torch.randn(1, channels[blk], 1, 1, generator=g)
        lin[f"lin{blk}.model.1.weight"] = w if signed_lin else w.abs()
    return vgg, lin


def frames(kind, N, H, W, seed=0):
    """(a, b) uint8 [N,H,W,3].  kind 'mixed': pair 0 noise against noise +- 20, pair 1 two independent noise frames, pair 2
    identical frames, then again; 'corners': a flat frame against itself with one changed pixel, once per corner (N = 4)"""
    rng = np.random.default_rng(77 * seed + 13 * H + W + 5 * N)
    if kind == "corners":
        assert N == 4
        b = np.full((4, H, W, 3), 128, np.uint8)
        a = b.copy()
        for i, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
            a[i, y, x] = (250, 20, 90)
        return a, b
    b = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    a = b.copy()
    for i in range(N):
        if i % 3 == 0:
            a[i] = np.clip(b[i].astype(np.int32) + rng.integers(-20, 21, b[i].shape), 0, 255).astype(np.uint8)
        elif i % 3 == 1:
            a[i] = rng.integers(0, 256, b[i].shape, dtype=np.uint8)
    return a, b


# ---------------------------------------------------------------------------------------------------- the restatement
def forward_ref(vgg_state, lin_state, a, b, dtype, abs_lin=False):
    """-> (lpips [N], taps [N,5]) float64 numpy, computed in `dtype` on the CPU from uint8 [N,H,W,3] stacks"""
    pick = lambda n, what: (vgg_state[f"features.{n}.{what}"] if f"features.{n}.{what}" in vgg_state else vgg_state[f"{n}.{what}"]).to(dtype)
    wts = {n: (pick(n, "weight"), pick(n, "bias")) for n in CONV_LAYERS}
    lins = [v for _, v in sorted((k, v) for k, v in lin_state.items())]
    mean = torch.tensor([-.030, -.088, -.188], dtype=torch.float32).to(dtype)[None, :, None, None]
    std = torch.tensor([.458, .448, .450], dtype=torch.float32).to(dtype)[None, :, None, None]

    def feats(u8):
        x = torch.from_numpy(u8).permute(0, 3, 1, 2).contiguous().float().div(255).to(dtype)   # to_tensor's float32 quotient
        x = (x - mean) / std
        out, i = [], 0
        for blk, count in enumerate(BLOCK_CONVS):
            if blk:
                x = F.max_pool2d(x, 2, 2)
            for _ in range(count):
                x = F.relu(F.conv2d(x, *wts[CONV_LAYERS[i]], padding=1))
                i += 1
            out.append(x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10))
        return out

    with torch.no_grad():
        taps = []
        for fa, fb, lw in zip(feats(a), feats(b), lins):
            lw = lw.to(dtype).abs() if abs_lin else lw.to(dtype)
            taps.append(F.conv2d((fa - fb) ** 2, lw.reshape(1, -1, 1, 1)).mean((2, 3)).reshape(-1))
        taps = torch.stack(taps, 1)
        return taps.sum(1).double().numpy(), taps.double().numpy()


@functools.lru_cache(maxsize=None)
def case(channels, kind, N, H, W, seed=0, signed_lin=False, bias_shift=0.0):
    """one call's inputs and yardsticks, computed once per session and shared (nothing writes to them)"""
    vgg, lin = make_weights(channels, seed, signed_lin, bias_shift)
    a, b = frames(kind, N, H, W, seed)
    t64, p64 = forward_ref(vgg, lin, a, b, torch.float64)
    t32, p32 = forward_ref(vgg, lin, a, b, torch.float32)
    st, sp = forward_ref(vgg, lin, a, b, torch.float64, abs_lin=True) if signed_lin else (t64, p64)
    live, live_taps = st > 0, sp > 0   # identical pairs, and taps behind which every pixel of both frames is dead, are exactly 0
    assert (p32[~live_taps] == 0).all()
    # the twin's total error, or the root-sum-square of its five tap errors where those happen to cancel in the sum
    e_total = np.maximum(np.abs(t32 - t64), np.sqrt(((p32 - p64) ** 2).sum(1)))
    e32_total = float(np.max(e_total[live] / st[live])) if live.any() else 0.0
    e32_tap = float(np.max(np.abs(p32 - p64)[live_taps] / sp[live_taps])) if live_taps.any() else 0.0
    return dict(vgg=vgg, lin=lin, a=a, b=b, total=t64, taps=p64, scale_total=st, scale_taps=sp, e32_total=e32_total, e32_tap=e32_tap, live=live,
                live_taps=live_taps)


@functools.lru_cache(maxsize=None)
def _model(channels, seed, signed_lin, bias_shift, dev_str):
    from instantsplat_amd.lpips import LpipsVGG
    vgg, lin = make_weights(channels, seed, signed_lin, bias_shift)
    return LpipsVGG(vgg, lin, device=None if dev_str == "cpu" else torch.device(dev_str))


def model(dev, channels, seed=0, signed_lin=False, bias_shift=0.0):
    return _model(channels, seed, signed_lin, bias_shift, str(dev))


def run(dev, net, a, b, **kw):
    return net.lpips_rgb8(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), **kw)


# ---------------------------------------------------------------------------------------------------- kernel checks
def check_case(dev, channels, kind, N, H, W, seed=0, signed_lin=False, bias_shift=0.0, bits=True):
    """device against float64 in units of the float32 twin's own error; identical pairs exactly zero; bits: (b, a) and a second
    run of (a, b) give equal bits"""
    c = case(channels, kind, N, H, W, seed, signed_lin, bias_shift)
    net = model(dev, channels, seed, signed_lin, bias_shift)
    got = run(dev, net, c["a"], c["b"])
    assert got["lpips"].dtype == np.float32 and got["lpips"].shape == (N,) and got["taps"].dtype == np.float32 and got["taps"].shape == (N, 5)
    label = f"{'x'.join(map(str, channels))} {kind} {N}x{H}x{W}" + (" signed" if signed_lin else "") + (f" bias{bias_shift:+g}" if bias_shift else "")
    live, live_taps = c["live"], c["live_taps"]
    assert (got["taps"][~live_taps] == 0.0).all(), (label, got["taps"])
    for i in range(N):
        same = np.array_equal(c["a"][i], c["b"][i])
        if same:
            assert got["lpips"][i] == 0.0 and (got["taps"][i] == 0.0).all(), (label, i, got["lpips"][i], got["taps"][i])
        elif not signed_lin:
            assert got["lpips"][i] > 0.0, (label, i)
    if live.any():
        dev_total = float(np.max(np.abs(got["lpips"].astype(np.float64) - c["total"])[live] / c["scale_total"][live]))
        dev_tap = float(np.max(np.abs(got["taps"].astype(np.float64) - c["taps"])[live_taps] / c["scale_taps"][live_taps]))
        print(f"LPIPS {label}: total float64 {c['total'].tolist()} device {got['lpips'].tolist()}")
        print(f"LPIPS {label}: E32 total {c['e32_total']:.3e} device {dev_total:.3e} | E32 tap {c['e32_tap']:.3e} device {dev_tap:.3e}")
        ops_util.bound(f"lpips total vs float64, relative [{label}]", dev_total, FACTOR * c["e32_total"])
        ops_util.bound(f"lpips taps vs float64, relative [{label}]", dev_tap, FACTOR * c["e32_tap"])
        ops_util.bound(f"lpips total vs float64, fourth decimal [{label}]", dev_total, TOTAL_REL)
    if not bits:
        return got
    swapped = run(dev, net, c["b"], c["a"])
    again = run(dev, net, c["a"], c["b"])
    for k in ("lpips", "taps"):
        assert np.array_equal(got[k].view(np.uint32), swapped[k].view(np.uint32)), (label, k, "exchange")
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), (label, k, "repeat")
    return got


def check_dead_pixels_present(channels, bias_shift, H, W):
    """the shifted-bias case is there for pixels that are all-zero behind a ReLU (the eps sits outside the root: 0 / (0 + eps) = 0,
    not NaN): make sure it has them, next to live ones"""
    c = case(channels, "mixed", 2, H, W, 0, False, bias_shift)
    x = torch.from_numpy(c["a"]).permute(0, 3, 1, 2).float().div(255).double()
    x = (x - torch.tensor([-.030, -.088, -.188], dtype=torch.float32).double()[None, :, None, None]) / \
        torch.tensor([.458, .448, .450], dtype=torch.float32).double()[None, :, None, None]
    dead, pixels, i = [], [], 0
    for blk, count in enumerate(BLOCK_CONVS):
        if blk:
            x = F.max_pool2d(x, 2, 2)
        for _ in range(count):
            n = CONV_LAYERS[i]
            x = F.relu(F.conv2d(x, c["vgg"][f"features.{n}.weight"].double(), c["vgg"][f"features.{n}.bias"].double(), padding=1))
            i += 1
        dead.append(int((x.abs().sum(1) == 0).sum()))
        pixels.append(x.shape[0] * x.shape[2] * x.shape[3])
    print(f"bias {bias_shift:+g}: all-zero pixels per tap {dead} of {pixels}")
    assert any(0 < d < p for d, p in zip(dead, pixels)), (dead, pixels)
    assert np.isfinite(c["total"]).all() and (c["total"] > 0).all()


def check_chunks_and_offsets(dev, channels):
    """a scratch budget that forces one pair per call gives the bits of one call; frames[1:] of an odd-sized stack (odd base
    address, storage offset) and host tensors score as fresh aligned device copies"""
    c = case(channels, "mixed", 3, 16, 16)
    net = model(dev, channels)
    whole = run(dev, net, c["a"], c["b"])
    split = run(dev, net, c["a"], c["b"], scratch_budget=1)
    for k in whole:
        assert np.array_equal(whole[k].view(np.uint32), split[k].view(np.uint32)), k
    a, b = frames("mixed", 3, 33, 17, seed=5)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    assert ta[1:].data_ptr() % 2 == 1 and ta[1:].is_contiguous() and ta[1:].storage_offset() == 33 * 17 * 3
    x, y = net.lpips_rgb8(ta[1:], tb[1:]), net.lpips_rgb8(ta[1:].clone(), tb[1:].clone())
    first = net.lpips_rgb8(ta[:2], tb[:2])
    for k in x:
        assert np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)), k
        assert np.array_equal(x[k][0].view(np.uint32), first[k][1].view(np.uint32)), k   # a pair's value does not depend on its place
    if dev.type == "cuda":
        z = net.lpips_rgb8(torch.from_numpy(a[1:]), torch.from_numpy(b[1:]).pin_memory())
        for k in x:
            assert np.array_equal(x[k].view(np.uint32), z[k].view(np.uint32)), k


# ---------------------------------------------------------------------------------------------------- the reference's numbers
def golden():
    return np.load(os.path.join(GOLDEN, "lpips_vectors.npz"))


def golden_states(g):
    """the recorded thin net: weights are stored as small integers, value = integer / lpips_weight_scale"""
    s = float(g["lpips_weight_scale"])
    vgg = {}
    for n in CONV_LAYERS:
        vgg[f"{n}.weight"] = torch.from_numpy(g[f"lpips_conv{n}_weight_q"].astype(np.float32) / np.float32(s))   # bare `N.weight` keys
        vgg[f"{n}.bias"] = torch.from_numpy(g[f"lpips_conv{n}_bias_q"].astype(np.float32) / np.float32(s))
    lin = {f"{i}.1.weight": torch.from_numpy(g[f"lpips_lin{i}_q"].astype(np.float32) / np.float32(s)).reshape(1, -1, 1, 1) for i in range(5)}
    return vgg, lin   # the reference's renamed lin keys


def check_golden(dev):
    """the reference's own LPIPS / VGG16 / LinLayers classes on a thin VGG-shaped net (tests/golden/README_lpips.md)"""
    from instantsplat_amd.lpips import LpipsVGG
    g = golden()
    vgg, lin = golden_states(g)
    net = LpipsVGG(vgg, lin, device=None if dev.type == "cpu" else dev)
    assert net.channels == tuple(int(c) for c in g["lpips_channels"])
    a, b = g["lpips_renders"], g["lpips_gts"]
    got = run(dev, net, a, b)
    t64, p64 = forward_ref(vgg, lin, a, b, torch.float64)
    t32, p32 = forward_ref(vgg, lin, a, b, torch.float32)
    ref_t, ref_p = g["lpips_total"].astype(np.float64), g["lpips_taps"].astype(np.float64)
    # the recording is the reference's float32 run: it sits E32 from float64 itself, and the device FACTOR x E32
    e32_total = max(float(np.max(np.abs(t32 - t64) / t64)), float(np.max(np.abs(ref_t - t64) / t64)))
    e32_tap = max(float(np.max(np.abs(p32 - p64) / p64)), float(np.max(np.abs(ref_p - p64) / p64)))
    d_total = float(np.max(np.abs(got["lpips"] - ref_t) / t64))
    d_tap = float(np.max(np.abs(got["taps"] - ref_p) / p64))
    print(f"LPIPS golden: reference {ref_t.tolist()} device {got['lpips'].tolist()} float64 {t64.tolist()}")
    print(f"LPIPS golden: E32 total {e32_total:.3e} device-reference {d_total:.3e} | E32 tap {e32_tap:.3e} device-reference {d_tap:.3e}")
    ops_util.bound("lpips total vs the reference's recording, relative", d_total, (FACTOR + 1) * e32_total)
    ops_util.bound("lpips taps vs the reference's recording, relative", d_tap, (FACTOR + 1) * e32_tap)
    ops_util.bound("lpips total vs the reference's recording, fourth decimal", d_total, TOTAL_REL)


# ---------------------------------------------------------------------------------------------------- host side
def check_key_namings(dev):
    """features.N / bare N for the trunk, lin{i}.model.1 / {i}.1 for the lin layers: one blob; torch.load(weights_only) files too"""
    from instantsplat_amd.lpips import LpipsVGG
    vgg, lin = make_weights(THIN)
    d = None if dev.type == "cpu" else dev
    base = LpipsVGG(vgg, lin, device=d)
    assert base.channels == THIN
    bare = {k.replace("features.", ""): v for k, v in vgg.items()}
    renamed = {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}
    assert sorted(renamed)[0] == "0.1.weight"
    for v, l in ((bare, lin), (vgg, renamed), (bare, renamed)):
        assert torch.equal(LpipsVGG(v, l, device=d).blob, base.blob)
    full = dict(vgg)
    full["classifier.0.weight"] = torch.zeros(4, 4)   # torchvision's file carries the classifier too
    assert torch.equal(LpipsVGG(full, lin, device=d).blob, base.blob)
    # blob layout (include/mi355gs.h): the first convolution's matrix is [27][C], row (3 ky + kx) 3 + ci
    w0 = vgg["features.0.weight"]
    assert torch.equal(base.blob[:27 * THIN[0]].cpu().reshape(3, 3, 3, THIN[0]), w0.permute(2, 3, 1, 0))
    assert torch.equal(base.blob[-THIN[4]:].cpu(), lin["lin4.model.1.weight"].reshape(-1))


def check_files_load(dev, root):
    from instantsplat_amd.lpips import LpipsVGG
    vgg, lin = make_weights(THIN)
    os.makedirs(root, exist_ok=True)
    torch.save(vgg, os.path.join(root, "vgg16.pth")), torch.save(lin, os.path.join(root, "vgg_lin.pth"))
    d = None if dev.type == "cpu" else dev
    assert torch.equal(LpipsVGG.from_files(os.path.join(root, "vgg16.pth"), os.path.join(root, "vgg_lin.pth"), device=d).blob,
                       LpipsVGG(vgg, lin, device=d).blob)


def check_value_errors(dev):
    from instantsplat_amd.lpips import LpipsVGG
    vgg, lin = make_weights(THIN)
    d = None if dev.type == "cpu" else dev
    net = model(dev, THIN)
    e = torch.zeros(0, 16, 16, 3, dtype=torch.uint8, device=dev)
    m = net.lpips_rgb8(e, e)
    assert m["lpips"].shape == (0,) and m["taps"].shape == (0, 5) and m["lpips"].dtype == np.float32
    ok = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=dev)
    for a, b in ((ok.float(), ok.float()), (ok, ok.float()), (ok[0], ok[0]), (ok, ok[:1]), (ok[:, :15], ok[:, :15]), (ok[:, :, :15], ok[:, :, :15]),
                 (torch.zeros(2, 16, 16, 4, dtype=torch.uint8, device=dev),) * 2, (ok.cpu().numpy(), ok.cpu().numpy())):
        with pytest.raises(ValueError):
            net.lpips_rgb8(a, b)
    def without(dct, key):
        return {k: v for k, v in dct.items() if k != key}
    odd = dict(vgg)
    odd["features.0.weight"], odd["features.0.bias"] = torch.zeros(48, 3, 3, 3), torch.zeros(48)   # not a multiple of 32
    wide = dict(vgg)
    wide["features.28.weight"] = torch.zeros(96, 64, 3, 3)                                          # Cin does not follow the block before
    for v, l in ((without(vgg, "features.17.bias"), lin), (vgg, without(lin, "lin3.model.1.weight")), (odd, lin), (wide, lin),
                 (vgg, dict(lin, **{"lin2.model.1.weight": torch.zeros(1, 32, 1, 1)}))):
        with pytest.raises(ValueError):
            LpipsVGG(v, l, device=d)


def check_entry_point_rejects_bad_arguments():
    """Argument checks of mi355gs_lpips_vgg_rgb8, before any HIP call (bogus device pointers are never touched)."""
    from instantsplat_amd import _lib
    L = _lib.lib()
    EINVAL = -1
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below must fail its checks first
    ch = lambda *c: (ctypes.c_int * 5)(*c)

    def call(N=2, H=16, W=16, a=fake, b=fake, channels=ch(*THIN), weights=fake, scratch=fake, lpips=fake, taps=fake):
        return L.mi355gs_lpips_vgg_rgb8(None, N, H, W, a, b, channels, weights, scratch, lpips, taps)
    for kw in ("a", "b", "channels", "weights", "scratch", "lpips"):
        assert call(**{kw: None}) == EINVAL, kw
    assert call(weights=ctypes.c_void_p(0x1004)) == EINVAL and call(scratch=ctypes.c_void_p(0x1008)) == EINVAL   # 16-byte alignment
    bad = (dict(N=0), dict(N=-1), dict(N=65536), dict(H=15), dict(W=15), dict(H=0), dict(W=-3), dict(H=30000, W=30000),
           dict(N=64, H=1024, W=1024),                      # 2 N H W x 32 channels > 2^31 - 1 elements
           dict(channels=ch(48, 32, 64, 64, 96)), dict(channels=ch(32, 32, 64, 64, 0)), dict(channels=ch(32, 32, 64, 64, 544)),
           dict(channels=ch(32, 32, 64, 64, -32)), dict(channels=ch(16, 32, 64, 64, 96)))
    for kw in bad:
        assert call(**kw) == EINVAL, {k: (list(v) if k == "channels" else v) for k, v in kw.items()}
        assert L.mi355gs_lpips_vgg_scratch_bytes(kw.get("N", 2), kw.get("H", 16), kw.get("W", 16), kw.get("channels", ch(*THIN))) == 0
    assert L.mi355gs_lpips_vgg_scratch_bytes(2, 16, 16, None) == 0
    assert L.mi355gs_lpips_vgg_scratch_bytes(1, 720, 1280, ch(*REAL)) >= 2 * (2 * 720 * 1280 * 64 * 4)
    assert L.mi355gs_lpips_vgg_scratch_bytes(2, 16, 16, ch(*THIN)) > 0
    assert L.mi355gs_abi_version() == 10


# ---------------------------------------------------------------------------------------------------- files
def check_evaluate_files(dev, root):
    """evaluate(lpips=net) writes the three files with the LPIPS fields an `lpips_fn` built on the float32 restatement writes: the
    values within TOTAL_REL (plus EVAL_ABS = 1e-8 — four orders below the files' fourth decimal — for the one-byte pair, whose
    LPIPS of 7e-8 is all cancellation), the text fields equal wherever the fourth decimal is not within that of a rounding
    boundary; evaluate() without it writes the lines it wrote before (no LPIPS field, the golden PSNR / SSIM); both: ValueError"""
    from instantsplat_amd.metrics import evaluate
    vgg, lin = make_weights(THIN)
    net = model(dev, THIN)
    listing = mu.build_model_dir(root)
    read = lambda: {f: open(os.path.join(root, f), "rb").read() for f in
                    ["results.json", "per_view.json"] + [os.path.join("test", m, "metrics.txt") for m in listing]}

    def lpips_fn(r, t):   # what a caller had to bring before: the reference's forward on [1,3,H,W] float32 in [0,1]
        to_u8 = lambda x: x.mul(255).round().to(torch.uint8)[0].permute(1, 2, 0).contiguous().numpy()[None]
        return forward_ref(vgg, lin, to_u8(r.cpu()), to_u8(t.cpu()), torch.float32)[0][0]
    EVAL_ABS = 1e-8
    g = mu.golden()
    plain = evaluate(root)
    plain_bytes = read()
    assert all(sorted(plain["results"][m]) == ["PSNR", "SSIM"] and sorted(plain["per_view"][m]) == ["PSNR", "SSIM"] for m in listing)
    for method, files in listing.items():
        lines = plain_bytes[os.path.join("test", method, "metrics.txt")].decode().splitlines()
        assert lines == [f"image name{name}, image idx: {idx}, PSNR: {float(g[f'metrics_{tag}_psnr'][i]):.2f}, "
                         f"SSIM: {float(g[f'metrics_{tag}_ssim'][i]):.4f}" for idx, (name, tag, i) in enumerate(files)]
    want = evaluate(root, lpips_fn=lpips_fn)
    want_bytes = read()
    got = evaluate(root, lpips=net)
    got_bytes = read()
    assert json.load(open(os.path.join(root, "results.json"))) == json.loads(json.dumps(got["results"]))
    for method, files in listing.items():
        assert sorted(got["results"][method]) == ["LPIPS", "PSNR", "SSIM"] and sorted(got["per_view"][method]) == ["LPIPS", "PSNR", "SSIM"]
        assert list(got["per_view"][method]["LPIPS"]) == [f[0] for f in files]
        for k in ("PSNR", "SSIM"):
            assert got["per_view"][method][k] == want["per_view"][method][k] and (got["results"][method][k] == want["results"][method][k]
                                                                                 or np.isinf(got["results"][method][k]))
        lines_g = got_bytes[os.path.join("test", method, "metrics.txt")].decode().splitlines()
        lines_w = want_bytes[os.path.join("test", method, "metrics.txt")].decode().splitlines()
        lines_p = plain_bytes[os.path.join("test", method, "metrics.txt")].decode().splitlines()
        assert len(lines_g) == len(lines_w) == len(files)
        for idx, (name, _, _) in enumerate(files):
            g_, w_ = got["per_view"][method]["LPIPS"][name], want["per_view"][method]["LPIPS"][name]
            assert abs(g_ - w_) <= TOTAL_REL * abs(w_) + EVAL_ABS, (name, g_, w_)
            assert lines_g[idx] == lines_p[idx] + f", LPIPS: {g_:.4f}", lines_g[idx]
            if abs(w_ * 1e4 - np.floor(w_ * 1e4) - 0.5) > 2 * (TOTAL_REL * w_ + EVAL_ABS) * 1e4:   # not on a rounding boundary of the 4th decimal
                assert lines_g[idx] == lines_w[idx], (lines_g[idx], lines_w[idx])
        assert abs(got["results"][method]["LPIPS"] - want["results"][method]["LPIPS"]) <= TOTAL_REL * abs(want["results"][method]["LPIPS"]) + EVAL_ABS
    with pytest.raises(ValueError):
        evaluate(root, lpips=net, lpips_fn=lpips_fn)
