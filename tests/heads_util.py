"""Checks of MASt3R's dense heads (instantsplat_amd/mast3r_heads.py, instantsplat_amd/mast3r.py, csrc/dpt.hip), shared by the
emulated tier (test_heads_emu.py, CPU tensors) and the MI355X (test_heads_gpu.py).

YARDSTICK.  `HeadRef(state, cfg, side, torch.float64)` restates one head with torch's CPU ops — F.conv2d, F.conv_transpose2d,
F.interpolate(bilinear, align_corners=True), F.gelu (erf), F.pixel_shuffle — in the order of dust3r/heads/dpt_head.py
(DPTOutputAdapter_fix.forward), mast3r/catmlp_dpt_head.py (forward, postprocess) and dust3r/heads/postprocess.py.  The block
definitions (act_postprocess, ResidualConvUnit, FeatureFusionBlock, the head, croco's Mlp) are the published croco ones, recalled
(croco is not vendored): this pins the device against the restatement, not against a checkpoint.  `HeadRef(..., torch.float32)`
is its twin; the twin's distance from float64 on the SAME case and tensor is E32, the unit of every bound.

BOUND.  Per output tensor (pts3d, conf, desc, desc_conf; under GS_CALIBRATE=1 also L0..L3, path_4..path_1 and the four channels
in front of postprocess, so that a failure names a layer): max |device - float64| <= FACTOR x max |twin - float64| and relative L2
likewise.  The kernels are deterministic, so the margin covers seeds and shapes not tried, not noise.
MEASURED on the MI355X (largest ratio device error / E32 over every tensor and side of the cases; tests/ops_util.bound under
GS_CALIBRATE=1; the case that holds the maximum):
  cases, tensors                                              max-abs ratio                       rel-L2 ratio
  thin (six grids, last_dim 64 / 96, pipeline): outputs       1.58  (pipeline side 2 pts3d)       1.26  (1x1 side 2 raw4)
  thin: L0..L3, path_4..path_1                                3.70  (last_dim 96 3x5 side 2 L2)   1.69  (last_dim 64 3x5 side 2 L2)
  thin: desc, desc_conf                                       4.79  (last_dim 96 3x5 desc_conf)   1.85  (1x1 side 2 desc_conf)
  real 3x5 / 5x13: pts3d, conf, raw4                          1.45  (3x5 side 2 pts3d)            1.50  (3x5 side 2 conf)
  real: L0..L3, path_4..path_1                                4.58  (3x5 side 2 L2)               3.02  (3x5 side 2 L2)
  real: desc, desc_conf                                       9.14  (3x5 side 1 desc_conf)        4.37  (5x13 side 2 desc_conf)
FACTOR = 16.  The DPT tensors alone give 16 by the rule (twice 4.58, rounded up to a power of two).  The local-feature MLP's
9.14 would give 32 by the rule; 16 — LPIPS's factor, the ceiling — is kept, which leaves it a margin of 1.75 x instead of 2 x.
What was traced: the MLP is two products of K = 1792 and K = 7168 (the trunk's longest is 4096, ratio 2.82), each ONE k-ordered
fmaf chain per output here and blocked partial sums in torch's float32 GEMM; the relative-L2 ratio follows the chain length
(1.85 at K = 192 / 768, 4.37 at 1792 / 7168), and max-abs over 3840 .. 66560 pixels follows the tail of that.  The DPT outputs,
whose chains are at most 9 x 768 = 6912 long but averaged by the layers behind them, stay below 1.6.
The weights are seeded so that the four channels in front of postprocess, and the descriptor confidence's logit, stay below 4
in magnitude (asserted on the float64 result): exp multiplies an error by the value, and a maximum over pixels then follows the
few pixels in the tail (with N(0, 1) logits the emulated thin 3 x 5 case read 8.0 x E32 in max-abs and 2.0 x in relative L2).
"""
import ctypes
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import ops_util
from tests import vit_util as vu

FACTOR = 16.0
THIN = dict(dim_tokens=(128, 64, 64, 64), layer_dims=(32, 32, 64, 64), feature_dim=64, last_dim=32, local_feat_dim=8)
REAL = dict(dim_tokens=(1024, 768, 768, 768), layer_dims=(96, 192, 384, 768), feature_dim=256, last_dim=128, local_feat_dim=24)
# (Ht, Wt) -> edges of the case.  1 x 1: a size-1 bilinear input (scale 0), the stride-2 convolution on one pixel, the crop 2 -> 1;
# 3 x 5 and 5 x 3: the crop in each dimension, transposed grids; 8 x 8: no crop; 5 x 13 (130 token rows with E = 2: two GEMM row
# tiles), 7 x 9.
GRIDS = {(1, 1): 3, (3, 5): 2, (5, 3): 1, (8, 8): 1, (5, 13): 2, (7, 9): 1}
# real widths, device only: 3 x 5 with one edge; 5 x 13 with FOUR edges — 4 x 64 x 65 = 16640 pixel rows reach the 128 x 128 GEMM tile
GRIDS_REAL = {(3, 5): 1, (5, 13): 4}
RAW_LIMIT = 4.0


def config(net):
    from instantsplat_amd.mast3r_heads import HeadsConfig
    return HeadsConfig(**net)


def _key(net):
    return tuple(sorted(net.items()))


# ---------------------------------------------------------------------------------------------------- weights and inputs
@functools.lru_cache(maxsize=None)
def _make_state(net_key, seed, naming):
    """seeded weights in the checkpoint's naming: weights N(0, 1 / fan_in) (activations stay O(1)), biases N(0, 0.1^2); the second
    convolution of every ResidualConvUnit and head.4 scaled down so that the four output channels stay moderate.
    naming 'layer_rn' | 'layerK_rn' | 'both': which of the checkpoint's two names for the layer_rn tensors the dict holds."""
    cfg = config(dict(net_key))
    g = torch.Generator().manual_seed(8765 + seed)
    sd = {}

    def conv(key, cin, cout, k, bias=True, scale=1.0):
        sd[key + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * (scale / (cin * k * k) ** 0.5)
        if bias:
            sd[key + ".bias"] = torch.randn(cout, generator=g) * (0.1 * scale)

    def lin(key, K, N):
        sd[key + ".weight"] = torch.randn(N, K, generator=g) / K ** 0.5
        sd[key + ".bias"] = torch.randn(N, generator=g) * 0.1

    ct, ld, Fd, LD = cfg.dim_tokens, cfg.layer_dims, cfg.feature_dim, cfg.last_dim
    for s in (1, 2):
        d = f"downstream_head{s}.dpt."
        for k in range(4):
            conv(f"{d}act_postprocess.{k}.0", ct[k], ld[k], 1)
        for k, st in ((0, 4), (1, 2)):
            sd[f"{d}act_postprocess.{k}.1.weight"] = torch.randn(ld[k], ld[k], st, st, generator=g) / ld[k] ** 0.5
            sd[f"{d}act_postprocess.{k}.1.bias"] = torch.randn(ld[k], generator=g) * 0.1
        conv(f"{d}act_postprocess.3.1", ld[3], ld[3], 3)
        for k in range(4):
            w = torch.randn(Fd, ld[k], 3, 3, generator=g) / (9 * ld[k]) ** 0.5
            if naming in ("layer_rn", "both"):
                sd[f"{d}scratch.layer_rn.{k}.weight"] = w
            if naming in ("layerK_rn", "both"):
                sd[f"{d}scratch.layer{k + 1}_rn.weight"] = w
        for n in (4, 3, 2, 1):
            for unit in ("resConfUnit1", "resConfUnit2"):
                conv(f"{d}scratch.refinenet{n}.{unit}.conv1", Fd, Fd, 3)
                conv(f"{d}scratch.refinenet{n}.{unit}.conv2", Fd, Fd, 3, scale=0.5)
            conv(f"{d}scratch.refinenet{n}.out_conv", Fd, Fd, 1, scale=0.7)
        conv(d + "head.0", Fd, Fd // 2, 3)
        conv(d + "head.2", Fd // 2, LD, 3)
        conv(d + "head.4", LD, 4, 1, scale=0.5)
        m = f"downstream_head{s}.head_local_features."
        K = ct[0] + ct[3]
        lin(m + "fc1", K, cfg.mlp_hidden())
        lin(m + "fc2", cfg.mlp_hidden(), (cfg.local_feat_dim + int(cfg.two_confs)) * 256)
        if cfg.two_confs:   # the descriptor confidence's logit goes through exp as c does: kept moderate in the same way
            sd[m + "fc2.weight"][cfg.local_feat_dim * 256:] *= 0.3
            sd[m + "fc2.bias"][cfg.local_feat_dim * 256:] *= 0.3
    return sd


def make_state(net, seed=0, naming="layer_rn"):
    return _make_state(_key(net), seed, naming)


def hooks(net, E, Ht, Wt, seed=0):
    """per side the four hooked tensors [E, Ht Wt, C_k], N(0, 1) — what a LayerNorm'd token row looks like"""
    g = torch.Generator().manual_seed(51 + 7 * seed + 31 * Ht + Wt)
    return tuple(tuple(torch.randn(E, Ht * Wt, C, generator=g) for C in net["dim_tokens"]) for _ in range(2))


# ---------------------------------------------------------------------------------------------------- the restatement
class HeadRef:
    def __init__(self, state, cfg, side, dtype):
        self.cfg, self.dtype = cfg, dtype
        p = f"downstream_head{side}."
        self.sd = {k[len(p):]: v.to(dtype) for k, v in state.items() if k.startswith(p)}
        for k in range(4):   # either name of the layer_rn tensors
            if f"dpt.scratch.layer_rn.{k}.weight" not in self.sd:
                self.sd[f"dpt.scratch.layer_rn.{k}.weight"] = self.sd[f"dpt.scratch.layer{k + 1}_rn.weight"]

    def conv(self, key, x, **kw):
        return F.conv2d(x, self.sd[key + ".weight"], self.sd.get(key + ".bias"), **kw)

    def rcu(self, key, x):
        return x + self.conv(key + ".conv2", F.relu(self.conv(key + ".conv1", F.relu(x), padding=1)), padding=1)

    def fusion(self, n, a, b=None):
        key = f"dpt.scratch.refinenet{n}"
        o = a
        if b is not None:
            o = a + self.rcu(key + ".resConfUnit1", b)
        o = self.rcu(key + ".resConfUnit2", o)
        o = F.interpolate(o, scale_factor=2, mode="bilinear", align_corners=True)
        return self.conv(key + ".out_conv", o)

    def dpt(self, hooked, Ht, Wt):
        """-> dict: L0..L3, path_4..path_1, raw4 (all channels-last), pts3d, conf"""
        sd = self.sd
        layers = [t.to(self.dtype).transpose(1, 2).reshape(t.shape[0], t.shape[2], Ht, Wt) for t in hooked]
        for k in range(4):
            layers[k] = self.conv(f"dpt.act_postprocess.{k}.0", layers[k])
        layers[0] = F.conv_transpose2d(layers[0], sd["dpt.act_postprocess.0.1.weight"], sd["dpt.act_postprocess.0.1.bias"], stride=4)
        layers[1] = F.conv_transpose2d(layers[1], sd["dpt.act_postprocess.1.1.weight"], sd["dpt.act_postprocess.1.1.bias"], stride=2)
        layers[3] = self.conv("dpt.act_postprocess.3.1", layers[3], stride=2, padding=1)
        L = [self.conv(f"dpt.scratch.layer_rn.{k}", layers[k], padding=1) for k in range(4)]
        path_4 = self.fusion(4, L[3])[:, :, :L[2].shape[2], :L[2].shape[3]]
        path_3 = self.fusion(3, path_4, L[2])
        path_2 = self.fusion(2, path_3, L[1])
        path_1 = self.fusion(1, path_2, L[0])
        o = self.conv("dpt.head.0", path_1, padding=1)
        o = F.interpolate(o, scale_factor=2, mode="bilinear", align_corners=True)
        o = self.conv("dpt.head.4", F.relu(self.conv("dpt.head.2", o, padding=1)))
        fmap = o.permute(0, 2, 3, 1)
        out = {f"L{k}": L[k] for k in range(4)}
        out.update(path_4=path_4, path_3=path_3, path_2=path_2, path_1=path_1)
        out = {k: v.permute(0, 2, 3, 1) for k, v in out.items()}
        out["raw4"] = fmap
        xyz = fmap[..., 0:3]
        d = xyz.norm(dim=-1, keepdim=True)
        out["pts3d"] = xyz / d.clip(min=1e-8) * torch.expm1(d)                                   # reg_dense_depth, ('exp', -inf, inf)
        _, vmin, vmax = self.cfg.conf_mode
        out["conf"] = vmin + fmap[..., 3].exp().clip(max=vmax - vmin)                            # reg_dense_conf
        return out

    def local(self, hooked, Ht, Wt, conf):
        cat = torch.cat([hooked[0], hooked[3]], dim=-1).to(self.dtype)
        f = F.linear(F.gelu(F.linear(cat, self.sd["head_local_features.fc1.weight"], self.sd["head_local_features.fc1.bias"])),
                     self.sd["head_local_features.fc2.weight"], self.sd["head_local_features.fc2.bias"])
        f = F.pixel_shuffle(f.transpose(-1, -2).reshape(f.shape[0], -1, Ht, Wt), 16).permute(0, 2, 3, 1)
        D = self.cfg.local_feat_dim
        desc = f[..., :D] / f[..., :D].norm(dim=-1, keepdim=True)
        if self.cfg.two_confs:
            _, vmin, vmax = self.cfg.desc_conf_mode or self.cfg.conf_mode
            return dict(desc=desc, desc_conf=vmin + f[..., D].exp().clip(max=vmax - vmin))
        return dict(desc=desc, desc_conf=conf.clone())

    def forward(self, hooked, Ht, Wt):
        out = self.dpt(hooked, Ht, Wt)
        out.update(self.local(hooked, Ht, Wt, out["conf"]))
        return out


def reference(state, cfg, hooked, Ht, Wt):
    """{'f64' | 'f32': (side 1's dict, side 2's dict)} of float64 tensors"""
    res = {}
    with torch.no_grad():
        for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            res[name] = tuple({k: v.double() for k, v in HeadRef(state, cfg, s + 1, dtype).forward(hooked[s], Ht, Wt).items()} for s in range(2))
    for side in res["f64"]:
        assert float(side["raw4"].abs().max()) < RAW_LIMIT, float(side["raw4"].abs().max())   # exp(4) x the error is the worst the bound sees
        assert float(side["desc_conf"].max()) < math.exp(RAW_LIMIT), float(side["desc_conf"].max())
    return res


@functools.lru_cache(maxsize=None)
def _case(net_key, Ht, Wt, E, seed):
    net = dict(net_key)
    state, cfg, hk = make_state(net, seed), config(net), hooks(net, E, Ht, Wt, seed)
    return dict(state=state, cfg=cfg, hooks=hk, **reference(state, cfg, hk, Ht, Wt))


def case(net, Ht, Wt, E, seed=0):
    """one case's inputs and yardsticks, computed once per session and shared (nothing writes to them)"""
    return _case(_key(net), Ht, Wt, E, seed)


@functools.lru_cache(maxsize=None)
def _heads(net_key, seed, dev_str, naming):
    from instantsplat_amd.mast3r_heads import Mast3rHeads
    net = dict(net_key)
    return Mast3rHeads(make_state(net, seed, naming), config(net), device=None if dev_str == "cpu" else torch.device(dev_str))


def heads(dev, net, seed=0, naming="layer_rn"):
    return _heads(_key(net), seed, str(dev), naming)


# ---------------------------------------------------------------------------------------------------- kernel checks
def _errors(got, want):
    d = got.detach().double().cpu() - want
    return float(d.abs().max()), float(d.norm() / (want.norm() + 1e-300))


def bound_tensor(label, got, want, twin):
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.float32, (label, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), label
    e_abs, e_rel = _errors(twin, want)
    d_abs, d_rel = _errors(got, want)
    print(f"HEADS {label}: E32 max-abs {e_abs:.3e} device {d_abs:.3e} ({d_abs / max(e_abs, 1e-300):.2f}x) | "
          f"E32 rel-L2 {e_rel:.3e} device {d_rel:.3e} ({d_rel / max(e_rel, 1e-300):.2f}x)")
    ops_util.bound(f"heads max-abs vs float64 in E32 [{label}]", d_abs / max(e_abs, 1e-300), FACTOR)
    ops_util.bound(f"heads rel-L2 vs float64 in E32 [{label}]", d_rel / max(e_rel, 1e-300), FACTOR)


def name_of(net):
    return "thin" if net == THIN else "real" if net == REAL else f"thin-last{net['last_dim']}"


def check_case(dev, net, Ht, Wt, E):
    """both heads of one case, descriptors included, against float64 in units of the float32 twin's own error"""
    from instantsplat_amd import mast3r_heads
    c = case(net, Ht, Wt, E)
    h = heads(dev, net)
    label = f"{name_of(net)} {Ht}x{Wt} E={E}"
    dec = [tuple(t.to(dev) for t in side) for side in c["hooks"]]
    taps = [] if os.environ.get("GS_CALIBRATE") == "1" else None
    outs = h.heads(dec[0], dec[1], (Ht, Wt), descriptors=True, taps=taps)
    for s in range(2):
        assert set(outs[s]) == {"pts3d", "conf", "desc", "desc_conf"}
        if taps is not None:
            for name in mast3r_heads.TAPS + ("raw4",):
                bound_tensor(f"{label} side {s + 1} {name}", taps[s][name], c["f64"][s][name], c["f32"][s][name])
        for name in ("pts3d", "conf", "desc", "desc_conf"):
            bound_tensor(f"{label} side {s + 1} {name}", outs[s][name], c["f64"][s][name], c["f32"][s][name])
    return c, outs


# The host's kernel-selection rules (csrc/dpt.hip dp_conv_nt, k_dpt_final's NT, mm_tile.h vt_gemm<true>), restated.
def conv_nt(cout):
    return 4 if cout % 128 == 0 else 2 if cout % 64 == 0 else 1


def gemm_tile(M, N):
    return 128 if vu.wide_tile(M, N) else 32 if N % 64 else 64


def selections(net, Ht, Wt, E):
    """every (kernel, instantiation) one case runs, descriptors included"""
    ct, ld, Fd, LD, D = net["dim_tokens"], net["layer_dims"], net["feature_dim"], net["last_dim"], net["local_feat_dim"]
    N, M = Ht * Wt, E * Ht * Wt
    got = set()
    for k in range(4):
        got.add(("gemm", gemm_tile(M, ld[k])))
    got.add(("gemm", gemm_tile(M, 16 * ld[0])))
    got.add(("gemm", gemm_tile(M, 4 * ld[1])))
    got.add(("conv", conv_nt(ld[3]), "stride 2"))
    got.add(("conv", conv_nt(Fd), "stride 1"))
    got.add(("conv", conv_nt(Fd // 2), "stride 1"))
    if Ht % 2 or Wt % 2:
        got.add(("up2", "cropped"))
    got.add(("up2", "whole"))
    for pixels in (N, 4 * N, 16 * N, 64 * N):
        got.add(("gemm", gemm_tile(E * pixels, Fd)))
    got.add(("final", LD // 32))
    hid = 4 * (ct[0] + ct[3])
    got.add(("gemm", gemm_tile(M, hid)))
    got.add(("gemm", gemm_tile(M, (D + 1) * 256)))
    return got


def check_every_instantiation_is_reached():
    """Every instantiation the host can pick must be run by a float64 case of the DEVICE tier; which case covers which:
    thin grids: conv NT 2 (F = 64, 64 -> 64 stride 2) and NT 1 (F / 2 = 32), final NT 1, GEMM tiles 32 (layer_dims 32) and 64;
    thin with last_dim 64 / 96 on 3 x 5: final NT 2 / 3;
    real 3 x 5 and 5 x 13: conv NT 4 at both strides, final NT 4, GEMM tile 32 (96 columns);
    real 5 x 13 with E = 4: refinenet1's out_conv on 16640 pixel rows, the 128 x 128 GEMM tile (with E = 3 it would not be)."""
    want = {("gemm", 32), ("gemm", 64), ("gemm", 128), ("up2", "cropped"), ("up2", "whole"), ("final", 1), ("final", 2), ("final", 3), ("final", 4)}
    want |= {("conv", nt, "stride 1") for nt in (1, 2, 4)} | {("conv", nt, "stride 2") for nt in (2, 4)}
    got = set()
    for (Ht, Wt), E in GRIDS.items():
        got |= selections(THIN, Ht, Wt, E)
    for LD in (64, 96):
        got |= selections(dict(THIN, last_dim=LD), 3, 5, 1)
    for (Ht, Wt), E in GRIDS_REAL.items():
        got |= selections(REAL, Ht, Wt, E)
    # a stride-2 convolution's width is layer_dims[3]; NT 1 there needs a width that is no multiple of 64, which the real net
    # (768) and the thin one (64) do not have: the kernel is the one template, its stride a runtime argument
    assert want <= got, want - got
    assert ("gemm", 128) not in selections(REAL, 5, 13, 3) and ("gemm", 128) in selections(REAL, 5, 13, 4)
    assert ("up2", "cropped") not in selections(THIN, 8, 8, 1)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _same_out(a, b):
    return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)


def check_properties(dev, net=THIN, grid=(3, 5)):
    """exact bits: two runs; an edge alone against the same edge in a batch of three; three calls under a small scratch budget
    against one; descriptors on or off; head 2 a copy of head 1 on swapped inputs"""
    from instantsplat_amd import _lib
    from instantsplat_amd.mast3r_heads import Mast3rHeads
    Ht, Wt = grid
    h = heads(dev, net)
    dec = [tuple(t.to(dev) for t in side) for side in hooks(net, 3, Ht, Wt)]
    a = h.heads(dec[0], dec[1], grid, descriptors=True)
    b = h.heads(dec[0], dec[1], grid, descriptors=True)
    assert _same_out(a[0], b[0]) and _same_out(a[1], b[1])
    plain = h.heads(dec[0], dec[1], grid)
    for s in range(2):
        assert set(plain[s]) == {"pts3d", "conf"} and _same(plain[s]["pts3d"], a[s]["pts3d"]) and _same(plain[s]["conf"], a[s]["conf"])
    for e in range(3):
        one = h.heads(tuple(t[e:e + 1] for t in dec[0]), tuple(t[e:e + 1] for t in dec[1]), grid, descriptors=True)
        for s in range(2):
            assert all(_same(one[s][k][0], a[s][k][e]) for k in a[s]), (e, s)
    calls = []
    real = _lib.call
    try:
        _lib.call = lambda d, name, *args: (calls.append(name), real(d, name, *args))[1]
        c = h.heads(dec[0], dec[1], grid, descriptors=True, scratch_budget=1)
    finally:
        _lib.call = real
    assert calls == ["dpt_head", "local_features"] * 6 and _same_out(c[0], a[0]) and _same_out(c[1], a[1])
    # head 2 = head 1: side 2 on side 1's inputs gives side 1's output
    state = dict(make_state(net))
    state.update({k.replace("downstream_head1", "downstream_head2"): v for k, v in make_state(net).items() if k.startswith("downstream_head1")})
    twin = Mast3rHeads(state, config(net), device=None if dev.type == "cpu" else dev)
    t = twin.heads(dec[0], dec[1], grid, descriptors=True)
    u = twin.heads(dec[1], dec[0], grid, descriptors=True)
    assert _same_out(t[0], a[0]) and _same_out(u[1], t[0]) and _same_out(u[0], t[1]) and not _same(t[1]["conf"], a[1]["conf"])


def check_zeroed_last_layer(dev, net=THIN, grid=(3, 5)):
    """head.4 zeroed: pts3d is exactly 0 everywhere (no NaN from 0 / 0) and conf exactly 1 + exp(0) = 2"""
    from instantsplat_amd.mast3r_heads import Mast3rHeads
    state = dict(make_state(net))
    for s in (1, 2):
        for part in ("weight", "bias"):
            state[f"downstream_head{s}.dpt.head.4.{part}"] = torch.zeros_like(state[f"downstream_head{s}.dpt.head.4.{part}"])
    h = Mast3rHeads(state, config(net), device=None if dev.type == "cpu" else dev)
    dec = [tuple(t.to(dev) for t in side) for side in hooks(net, 2, *grid)]
    for out in h.heads(dec[0], dec[1], grid):
        assert float(out["pts3d"].abs().max()) == 0.0 and not bool(torch.isnan(out["pts3d"]).any())
        assert float(out["conf"].min()) == 2.0 == float(out["conf"].max())


def check_one_conf(dev, grid=(3, 5)):
    """two_confs false: fc2 has local_feat_dim x 256 outputs and desc_conf has conf's bits; desc against float64"""
    net = dict(THIN, two_confs=False)
    c = case(net, *grid, 1)
    outs = heads(dev, net).heads(*[tuple(t.to(dev) for t in side) for side in c["hooks"]], grid, descriptors=True)
    for s in range(2):
        assert _same(outs[s]["desc_conf"], outs[s]["conf"]) and outs[s]["desc_conf"].data_ptr() != outs[s]["conf"].data_ptr()
        bound_tensor(f"thin one conf side {s + 1} desc", outs[s]["desc"], c["f64"][s]["desc"], c["f32"][s]["desc"])


# ---------------------------------------------------------------------------------------------------- closing the pipeline
PIPELINE_SEED = 8


def pipeline_head_state():
    """The head weights of the pipeline case.  An untrained head emits no scene, and the aligner's start (as the reference's)
    clips a negative Weiszfeld focal to 0, whose logarithm is -inf.  So: head.4's z bias is 1.5 (depths in front of the camera),
    and the seed is one at which the untrained pointmaps give every image a clearly positive focal (seeds 0..31 were tried on the
    float32 restatement: 8 gives 42.8, 39.2, 21.2 pixels; most give a 0 somewhere).  The four channels stay below RAW_LIMIT."""
    state = dict(make_state(THIN, seed=PIPELINE_SEED))
    for s in (1, 2):
        b = state[f"downstream_head{s}.dpt.head.4.bias"].clone()
        b[2] = 1.5
        state[f"downstream_head{s}.dpt.head.4.bias"] = b
    return state


@functools.lru_cache(maxsize=None)
def _pipeline_case():
    """vit_util.Ref chained into HeadRef on the thin net, 3 images on 3 x 5, the six edges of the complete graph"""
    from instantsplat_amd.mast3r_trunk import complete_edges
    state = dict(vu.make_state(vu.THIN))
    state.update(pipeline_head_state())
    img = vu.images(3, 3, 5)
    edges = complete_edges(3)
    res = {}
    with torch.no_grad():
        for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            ref = vu.Ref(state, vu.config(vu.THIN), dtype)
            feat, pos = ref.encode(img)
            d1, d2 = ref.decode(feat, pos, edges)
            res[name] = tuple({k: v.double() for k, v in HeadRef(state, config(THIN), s + 1, dtype).forward(d, 3, 5).items()}
                              for s, d in enumerate((d1, d2)))
    for side in res["f64"]:
        assert float(side["raw4"].abs().max()) < RAW_LIMIT
    return dict(state=state, images=img, edges=edges, **res)


def check_pipeline(dev):
    from instantsplat_amd.global_align import AlignProblem, compute_global_alignment
    from instantsplat_amd.mast3r import Mast3r
    c = _pipeline_case()
    d = None if dev.type == "cpu" else dev
    model = Mast3r(c["state"], vu.config(vu.THIN), config(THIN), device=d)
    img = c["images"].to(dev)
    out = model.inference(img, descriptors=True)
    assert set(out) == {"view1", "view2", "pred1", "pred2", "edges", "loss"} and out["loss"] is None
    assert out["edges"].tolist() == c["edges"].tolist() == [[1, 0], [2, 0], [2, 1], [0, 1], [0, 2], [1, 2]]
    assert out["view1"]["idx"].tolist() == [1, 2, 2, 0, 0, 1] and out["view2"]["idx"].tolist() == [0, 0, 1, 1, 2, 2]
    assert out["view1"]["true_shape"].tolist() == [[48, 80]] * 6 == out["view2"]["true_shape"].tolist()
    assert set(out["pred1"]) == {"pts3d", "conf", "desc", "desc_conf"} and set(out["pred2"]) == {"pts3d_in_other_view", "conf", "desc", "desc_conf"}
    assert tuple(out["pred1"]["pts3d"].shape) == (6, 48, 80, 3) and tuple(out["pred2"]["conf"].shape) == (6, 48, 80)
    assert tuple(out["pred1"]["desc"].shape) == (6, 48, 80, 8) and tuple(out["pred2"]["desc_conf"].shape) == (6, 48, 80)
    for s, pred in ((0, out["pred1"]), (1, out["pred2"])):
        for name in ("pts3d", "conf", "desc", "desc_conf"):
            got = pred["pts3d_in_other_view" if (s, name) == (1, "pts3d") else name]
            bound_tensor(f"pipeline side {s + 1} {name}", got, c["f64"][s][name], c["f32"][s][name])
    plain = model.inference(img)
    assert set(plain["pred1"]) == {"pts3d", "conf"} and _same(plain["pred1"]["pts3d"], out["pred1"]["pts3d"])
    problem = model.align_problem(img)
    assert isinstance(problem, AlignProblem) and problem.edges == [tuple(e) for e in c["edges"].tolist()] and (problem.H, problem.W) == (48, 80)
    assert _same(problem.conf_i, out["pred1"]["conf"].reshape(6, -1)) and _same(problem.conf_j, out["pred2"]["conf"].reshape(6, -1))
    state, _, losses = compute_global_alignment(problem, niter=2)
    assert bool(torch.isfinite(state.im_poses()).all()) and tuple(state.im_poses().shape) == (3, 4, 4)
    assert float(state.focals().min()) > 1.0 and bool(torch.isfinite(torch.as_tensor(losses)).all())
    problem.close()


# ---------------------------------------------------------------------------------------------------- host side
def check_loader(dev, root):
    import argparse
    from instantsplat_amd.mast3r import Mast3r
    from instantsplat_amd.mast3r_heads import Mast3rHeads
    d = None if dev.type == "cpu" else dev
    cfg = config(THIN)
    base = heads(dev, THIN)
    assert torch.equal(heads(dev, THIN, naming="layerK_rn").blob, base.blob) and torch.equal(heads(dev, THIN, naming="both").blob, base.blob)
    both = dict(make_state(THIN, naming="both"))
    for k in range(4):   # layer_rn is the one that is read when both are there
        both[f"downstream_head1.dpt.scratch.layer{k + 1}_rn.weight"] = torch.zeros(1)
    assert torch.equal(Mast3rHeads(both, cfg, device=d).blob, base.blob)
    state = make_state(THIN)
    unused = {k: v for k, v in state.items() if "refinenet4.resConfUnit1" not in k}
    assert len(unused) == len(state) - 8 and torch.equal(Mast3rHeads(unused, cfg, device=d).blob, base.blob)
    extra = dict(state, **vu.make_state(vu.THIN))                       # the trunk's keys are ignored
    assert torch.equal(Mast3rHeads(extra, cfg, device=d).blob, base.blob)
    for key in ("downstream_head1.dpt.act_postprocess.0.1.weight", "downstream_head2.dpt.scratch.layer_rn.2.weight",
                "downstream_head1.dpt.scratch.refinenet4.resConfUnit2.conv1.bias", "downstream_head2.dpt.scratch.refinenet1.resConfUnit1.conv2.weight",
                "downstream_head1.dpt.scratch.refinenet2.out_conv.bias", "downstream_head2.dpt.head.4.bias", "downstream_head1.dpt.head.0.weight",
                "downstream_head2.head_local_features.fc2.bias"):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            Mast3rHeads({k: v for k, v in state.items() if k != key}, cfg, device=d)
    for key, bad in (("downstream_head1.dpt.head.4.weight", torch.zeros(3, 32, 1, 1)), ("downstream_head2.dpt.act_postprocess.1.1.weight", torch.zeros(32, 32, 4, 4)),
                     ("downstream_head1.dpt.scratch.layer_rn.0.weight", torch.zeros(64, 32, 1, 1)), ("downstream_head1.head_local_features.fc1.bias", torch.zeros(7))):
        with pytest.raises(ValueError, match=key.rsplit(".", 1)[0].replace(".", r"\.")):
            Mast3rHeads(dict(state, **{key: bad}), cfg, device=d)
    # the blob's layout (include/mi355gs.h): act_postprocess.0.0 first, [K][N] = the 1x1 weight transposed; head 2's MLP bias last
    K, N = THIN["dim_tokens"][0], THIN["layer_dims"][0]
    assert torch.equal(base.blob[:K * N].cpu().reshape(K, N), state["downstream_head1.dpt.act_postprocess.0.0.weight"].reshape(N, K).t())
    assert torch.equal(base.blob[-9 * 256:].cpu(), state["downstream_head2.head_local_features.fc2.bias"])
    assert base.blob.data_ptr() % 16 == 0 and all(t.data_ptr() % 16 == 0 and t.untyped_storage().data_ptr() == base.blob.untyped_storage().data_ptr()
                                                   for t in base._dpt + base._mlp)
    # a file in the checkpoint's shape, read with weights_only=True; its args string is never evaluated
    os.makedirs(root, exist_ok=True)
    path = os.path.join(root, "ckpt.pth")
    torch.save({"args": argparse.Namespace(model="__import__('os').abort()"), "model": extra, "epoch": 3}, path)
    assert torch.equal(Mast3rHeads.from_checkpoint(path, cfg, device=d).blob, base.blob)
    whole = Mast3r.from_checkpoint(path, vu.config(vu.THIN), cfg, device=d)
    assert torch.equal(whole.heads.blob, base.blob) and torch.equal(whole.trunk.blob, vu.trunk(dev, vu.THIN).blob)
    torch.save(state, path)
    with pytest.raises(ValueError, match="model"):
        Mast3rHeads.from_checkpoint(path, cfg, device=d)


def check_value_errors(dev):
    from instantsplat_amd.mast3r_heads import HeadsConfig, Mast3rHeads
    d = None if dev.type == "cpu" else dev
    h = heads(dev, THIN)
    dec = [tuple(t.to(dev) for t in side) for side in hooks(THIN, 2, 2, 3)]
    h.heads(dec[0], dec[1], (2, 3))
    for grid in ((3, 3), None, 6, (6,), (0, 6)):
        with pytest.raises(ValueError):
            h.heads(dec[0], dec[1], grid)
    bad1 = (dec[0][0], dec[0][1], dec[0][2])
    bad2 = (dec[0][0], dec[0][1].double(), dec[0][2], dec[0][3])
    bad3 = (dec[0][0], dec[0][1][:, :, :32], dec[0][2], dec[0][3])
    bad4 = (dec[0][0], dec[0][1][:1], dec[0][2], dec[0][3])
    bad5 = tuple(t[:1] for t in dec[0])
    for bad in (bad1, bad2, bad3, bad4, None, dec[0][0]):
        with pytest.raises(ValueError):
            h.heads(bad, dec[1], (2, 3))
    with pytest.raises(ValueError):
        h.heads(dec[0], bad5, (2, 3))
    state = make_state(THIN)
    for over in (dict(depth_mode=("linear", -math.inf, math.inf)), dict(depth_mode=("exp", 0.0, math.inf)), dict(conf_mode=("sigmoid", 0.0, 1.0)),
                 dict(desc_conf_mode=("sigmoid", 0.0, 1.0)), dict(conf_mode=("exp", 1.0, 1.0)), dict(desc_mode="raw"), dict(feature_dim=96),
                 dict(feature_dim=320), dict(last_dim=160), dict(last_dim=48), dict(layer_dims=(32, 32, 64, 48)), dict(local_feat_dim=0)):
        with pytest.raises(ValueError):
            Mast3rHeads(state, HeadsConfig(**dict(THIN, **over)), device=d)
    with pytest.raises(ValueError, match="expected"):
        Mast3rHeads(state, HeadsConfig(**dict(THIN, last_dim=64)), device=d)      # sizes that do not follow the tensors


def check_cpu_tensors_refused():
    """the product path (no emulated library bound) refuses CPU tensors in _lib.gpu_only()'s words"""
    from instantsplat_amd import _lib
    from instantsplat_amd.mast3r_heads import Mast3rHeads
    _lib._use_library_for_testing(None)
    state, cfg = make_state(THIN), config(THIN)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU only"):
            Mast3rHeads(state, cfg)
        return
    h = Mast3rHeads(state, cfg)
    assert h.blob.is_cuda
    dec = hooks(THIN, 1, 1, 1)
    with pytest.raises(ValueError, match="on the GPU only"):
        h.heads(dec[0], dec[1], (1, 1))


def check_entry_points_reject_bad_arguments():
    """Argument checks of the entry points, before any HIP call (bogus device pointers are never touched)."""
    from instantsplat_amd import _lib
    from instantsplat_amd.mast3r_heads import _Config
    L = _lib.lib()
    EINVAL = -1
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below must fail its checks first
    odd = ctypes.c_void_p(0x1008)    # off a 16-byte boundary

    def cfg(**over):
        n = dict(dict(THIN, mlp_hidden=768, two_confs=1, conf=(1.0, math.inf), desc_conf=(0.0, math.inf)), **over)
        return _Config((ctypes.c_int * 4)(*n["dim_tokens"]), (ctypes.c_int * 4)(*n["layer_dims"]), n["feature_dim"], n["last_dim"], n["mlp_hidden"],
                       n["local_feat_dim"], n["two_confs"], n["conf"][0], n["conf"][1], n["desc_conf"][0], n["desc_conf"][1])
    four = (ctypes.c_void_p * 4)(*[0x1000] * 4)

    def head(c=cfg(), Ht=2, Wt=3, E=1, weights=fake, hooks=four, scratch=fake, pts3d=fake, conf=fake, raw4=None):
        return L.mi355gs_dpt_head(None, ctypes.byref(c) if c is not None else None, weights, Ht, Wt, E, hooks, scratch, pts3d, conf, raw4)

    def local(c=cfg(), Ht=2, Wt=3, E=1, weights=fake, hook0=fake, hook3=fake, scratch=fake, desc=fake, desc_conf=fake):
        return L.mi355gs_local_features(None, ctypes.byref(c) if c is not None else None, weights, Ht, Wt, E, hook0, hook3, scratch, desc, desc_conf)
    for kw in ("c", "weights", "hooks", "scratch", "pts3d", "conf"):
        assert head(**{kw: None}) == EINVAL, kw
    for kw in ("c", "weights", "hook0", "hook3", "scratch", "desc", "desc_conf"):
        assert local(**{kw: None}) == EINVAL, kw
    for kw in ("weights", "scratch", "raw4"):
        assert head(**{kw: odd}) == EINVAL, kw
    for kw in ("weights", "hook0", "hook3", "scratch"):
        assert local(**{kw: odd}) == EINVAL, kw
    assert head(hooks=(ctypes.c_void_p * 4)(0x1000, 0x1000, 0x1008, 0x1000)) == EINVAL
    assert head(hooks=(ctypes.c_void_p * 4)(0x1000, 0, 0x1000, 0x1000)) == EINVAL
    q = lambda fn, c, Ht=2, Wt=3, E=1: getattr(L, fn)(ctypes.byref(c) if c is not None else None, Ht, Wt, E)
    for over in (dict(feature_dim=96), dict(feature_dim=320), dict(feature_dim=0), dict(last_dim=160), dict(last_dim=48), dict(last_dim=0),
                 dict(layer_dims=(32, 32, 64, 48)), dict(layer_dims=(32, 32, 64, 1056)), dict(dim_tokens=(128, 64, 72, 64)), dict(conf=(1.0, 1.0))):
        c = cfg(**over)
        assert head(c=c) == EINVAL, over
        assert q("mi355gs_dpt_head_scratch_bytes", c) == 0 and L.mi355gs_dpt_head_tap_offset(ctypes.byref(c), 2, 3, 1, 0) == 0, over
    for over in (dict(mlp_hidden=100), dict(mlp_hidden=0), dict(local_feat_dim=0), dict(local_feat_dim=256), dict(dim_tokens=(100, 64, 64, 64)),
                 dict(desc_conf=(1.0, 0.0))):
        c = cfg(**over)
        assert local(c=c) == EINVAL, over
        assert q("mi355gs_local_features_scratch_bytes", c) == 0, over
    for kw in (dict(Ht=0), dict(Wt=-1), dict(Ht=65, Wt=64), dict(E=0), dict(E=65536), dict(Ht=64, Wt=64, E=600)):
        assert head(**kw) == EINVAL and q("mi355gs_dpt_head_scratch_bytes", cfg(), **kw) == 0, kw
    for kw in (dict(Ht=0), dict(Wt=-1), dict(Ht=65, Wt=64), dict(E=0), dict(E=65536)):
        assert local(**kw) == EINVAL and q("mi355gs_local_features_scratch_bytes", cfg(), **kw) == 0, kw
    assert q("mi355gs_dpt_head_scratch_bytes", None) == 0 and q("mi355gs_local_features_scratch_bytes", None) == 0
    c = cfg()
    total = q("mi355gs_dpt_head_scratch_bytes", c, E=2)
    offs = [L.mi355gs_dpt_head_tap_offset(ctypes.byref(c), 2, 3, 2, k) for k in range(8)]
    assert all(0 < o < total and o % 256 == 0 for o in offs) and len(set(offs)) == 8
    assert L.mi355gs_dpt_head_tap_offset(ctypes.byref(c), 2, 3, 2, 8) == 0 and L.mi355gs_dpt_head_tap_offset(ctypes.byref(c), 2, 3, 2, -1) == 0
    assert total >= 2 * 6 * 4 * (64 * 64 + 256 * 32)      # path_1 (64 N pixels x F) and the head's upsampled input (256 N x F / 2) alone
    assert q("mi355gs_local_features_scratch_bytes", c, E=2) >= 2 * 6 * 4 * (192 + 768 + 9 * 256)
    assert L.mi355gs_abi_version() == 10
