"""Checks of MASt3R's transformer trunk (instantsplat_amd/mast3r_trunk.py, csrc/vit.hip), shared by the emulated tier
(test_vit_emu.py, CPU tensors) and the MI355X (test_vit_gpu.py).

YARDSTICK.  `Ref(state, cfg, torch.float64)` restates the trunk with torch's CPU ops — F.layer_norm, F.linear, F.gelu (erf), softmax,
RoPE2D from its formula — wired as the reference wires it: the encoder of dust3r/model.py:127-139, the two-sided decoder of
model.py:171-190 (both sides read the PREVIOUS layer's pair, dec_norm on the last pair only), the hooks of
mast3r/catmlp_dpt_head.py:115-116.  The block definitions are the published croco ones, recalled (croco is not vendored): this
pins the device against the restatement, not against a checkpoint.  `Ref(..., torch.float32)` is its twin, the arithmetic the
reference runs; the twin's distance from float64 on the SAME case and tensor is E32, the unit of every bound.

BOUND.  Per output tensor (feat; the four hooked tensors of each side): max |device - float64| <= FACTOR x max |twin - float64|
and relative L2 likewise.  The kernels are deterministic, so the margin covers seeds and shapes not tried, not noise.
MEASURED on the MI355X (largest ratio device error / E32 over every tensor of every case; tests/ops_util.bound under
GS_CALIBRATE=1; the case that holds the maximum):
  cases                                          max-abs ratio                     rel-L2 ratio
  thin net, the eight grids                      1.70  (18x32 side 2 hook 2)       1.39  (18x32 side 2 hook 3)
  real widths, 3x5 / 5x13 / 9x15                 2.63  (5x13 side 2 hook 2)        2.14  (9x15 side 2 hook 1)
  real widths, 18x32 (the 128 x 128 GEMM tile)   2.82  (side 2 hook 1)       2.34  (side 2 hook 1)
  thin, rows of zero variance, 3x5               1.36                              1.30
  thin, peaked softmax (|logit| to 134), 7x9     0.77                              0.95
  thin, same patches on 3x5 and 5x3              0.96                              1.06
  emulator, thin net, the seven grids            1.40  (1x1 side 2 hook 0)         1.29  (1x1 side 1 hook 1)
Typical sizes: E32 max-abs 2e-6 .. 6e-6 and rel-L2 4e-7 .. 7e-7 on the plain cases (device 5.2e-6 / 9.7e-7 at the real widths);
the peaked case is ill-conditioned in itself (E32 rel-L2 4e-3 after four decoder layers) and the device sits inside it.
FACTOR = 8: twice the largest ratio (2.82), rounded up to a power of two — half of LPIPS's 16.  Why the real widths sit 2x out
and the thin net does not: a K = 1024 .. 4096 product is ONE k-ordered fmaf chain here and blocked partial sums in torch's
float32 GEMM (tests/lpips_util.py has the same observation for the convolutions).
The emulator and the device do NOT print the same digits here (they do for LPIPS): DESIGN.md 5.12 says which kernels differ.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ops_util

FACTOR = 8.0
THIN = dict(enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=64, dec_depth=4, dec_heads=1, hooks=(0, 2, 3, 4))
REAL = dict(enc_dim=1024, enc_depth=2, enc_heads=16, dec_dim=768, dec_depth=4, dec_heads=12, hooks=(0, 2, 3, 4))
# (Ht, Wt): one token; non-square both ways (a y / x swap in RoPE shows); one below, at and one above a 64-key chunk and a
# 64-row tile; just past two 64-row tiles with a third key chunk of 7; (GPU only) the 512 x 288 grid
GRIDS = ((1, 1), (3, 5), (5, 3), (7, 9), (8, 8), (5, 13), (9, 15))
GRIDS_GPU_ONLY = ((18, 32),)
GRIDS_REAL = ((3, 5), (5, 13), (9, 15), (18, 32))   # the last: M = 1728 and 3456 rows, where the 128 x 128 GEMM tile takes over


def wide_tile(M, N):
    """the host's tile rule (csrc/vit.hip vt_gemm): 128 x 128 where that still yields 256 workgroups, else 128 x 64"""
    return N % 128 == 0 and -(-M // 128) * (N // 128) >= 256
EDGE_SETS = {1: ((0, 0),), 2: ((0, 1),), 3: ((1, 0), (2, 0), (2, 1), (0, 1), (0, 2), (1, 2))}
# which view set a grid is run with: every set appears below, at and above the tile sizes
VIEWS = {(1, 1): 3, (3, 5): 2, (5, 3): 2, (7, 9): 3, (8, 8): 1, (5, 13): 3, (9, 15): 3, (18, 32): 3}
STATS = {"max_logit": 0.0}


def config(net):
    from instantsplat_amd.mast3r_trunk import TrunkConfig
    return TrunkConfig(**net)


def _key(net):
    return tuple(sorted(net.items()))


# ---------------------------------------------------------------------------------------------------- weights and images
@functools.lru_cache(maxsize=None)
def _make_state(net_key, seed, both_sides, variant):
    """seeded weights in the checkpoint's naming: linear weights N(0, 1 / K) (activations stay O(1)), biases N(0, 0.1^2), norm
    weights 1 + N(0, 0.1^2).  variant 'flat': a zero patch embedding with the constant bias 0.5 (every token row constant: its
    variance is exactly 0 in any summation order, 0.5 k being exact); 'peaked': q and k projections x 5 (logits x 25)."""
    net = dict(net_key)
    g = torch.Generator().manual_seed(4321 + seed)
    sd = {}

    def lin(key, K, N, scale=1.0):
        sd[key + ".weight"] = torch.randn(N, K, generator=g) * (scale / K ** 0.5)
        sd[key + ".bias"] = torch.randn(N, generator=g) * (0.1 * scale)

    def norm(key, D):
        sd[key + ".weight"] = 1.0 + 0.1 * torch.randn(D, generator=g)
        sd[key + ".bias"] = 0.1 * torch.randn(D, generator=g)

    De, Dd = net["enc_dim"], net["dec_dim"]
    qk = 5.0 if variant == "peaked" else 1.0
    sd["patch_embed.proj.weight"] = torch.randn(De, 3, 16, 16, generator=g) / 768 ** 0.5
    sd["patch_embed.proj.bias"] = torch.randn(De, generator=g) * 0.1
    if variant == "flat":
        sd["patch_embed.proj.weight"].zero_()
        sd["patch_embed.proj.bias"].fill_(0.5)

    def qkv(key, D):
        lin(key, D, 3 * D)
        sd[key + ".weight"][:2 * D] *= qk
        sd[key + ".bias"][:2 * D] *= qk

    for n in range(net["enc_depth"]):
        b = f"enc_blocks.{n}."
        norm(b + "norm1", De), qkv(b + "attn.qkv", De), lin(b + "attn.proj", De, De)
        norm(b + "norm2", De), lin(b + "mlp.fc1", De, 4 * De), lin(b + "mlp.fc2", 4 * De, De)
    norm("enc_norm", De), lin("decoder_embed", De, Dd)
    for side in ("dec_blocks", "dec_blocks2")[:2 if both_sides else 1]:
        for n in range(net["dec_depth"]):
            b = f"{side}.{n}."
            norm(b + "norm1", Dd), qkv(b + "attn.qkv", Dd), lin(b + "attn.proj", Dd, Dd)
            norm(b + "norm_y", Dd), norm(b + "norm2", Dd)
            lin(b + "cross_attn.projq", Dd, Dd, qk), lin(b + "cross_attn.projk", Dd, Dd, qk)
            lin(b + "cross_attn.projv", Dd, Dd), lin(b + "cross_attn.proj", Dd, Dd)
            norm(b + "norm3", Dd), lin(b + "mlp.fc1", Dd, 4 * Dd), lin(b + "mlp.fc2", 4 * Dd, Dd)
    norm("dec_norm", Dd)
    return sd


def make_state(net, seed=0, both_sides=True, variant="plain"):
    return _make_state(_key(net), seed, both_sides, variant)


def images(V, Ht, Wt, seed=0):
    """float32 [V,3,16 Ht,16 Wt] in [-1, 1], as the reference's loader normalises them"""
    g = torch.Generator().manual_seed(99 + 7 * seed + 31 * Ht + Wt)
    return torch.rand(V, 3, 16 * Ht, 16 * Wt, generator=g) * 2 - 1


# ---------------------------------------------------------------------------------------------------- the restatement
def rope2d(t, pos, dtype, base=100.0):
    """t [B,heads,N,64], pos [B,N,2] = (y, x): the first 32 channels turn by y, the last 32 by x; inside a half, angle[j] =
    p base^(-2 (j mod 16) / 32) and out = t cos + rotate_half(t) sin with rotate_half = (-t[16:], t[:16])"""
    inv_freq = 1.0 / (base ** (torch.arange(0, 32, 2, device=t.device).to(dtype) / 32))
    out = []
    for half in range(2):
        ang = pos[:, :, half].to(dtype)[:, :, None] * inv_freq[None, None, :]
        ang = torch.cat((ang, ang), -1)[:, None]                          # [B,1,N,32]
        th = t[..., 32 * half:32 * half + 32]
        rot = torch.cat((-th[..., 16:], th[..., :16]), -1)
        out.append(th * ang.cos() + rot * ang.sin())
    return torch.cat(out, -1)


def attend(q, k, v, qpos, kpos, dtype):
    """q [B,Nq,D], k, v [B,Nk,D] -> [B,Nq,D]: heads of 64, RoPE on q and k, softmax(q k^T / 8) v"""
    B, Nq, D = q.shape
    split = lambda t: t.reshape(B, t.shape[1], D // 64, 64).transpose(1, 2)
    qh, kh, vh = rope2d(split(q), qpos, dtype), rope2d(split(k), kpos, dtype), split(v)
    logits = qh @ kh.transpose(-1, -2) * 0.125
    STATS["max_logit"] = max(STATS["max_logit"], float(logits.abs().max()))
    return (logits.softmax(-1) @ vh).transpose(1, 2).reshape(B, Nq, D)


class Ref:
    def __init__(self, state, cfg, dtype):
        self.cfg, self.dtype = cfg, dtype
        sd = dict(state)
        if not any(k.startswith("dec_blocks2") for k in sd):                         # dust3r/model.py:90-97
            sd.update({k.replace("dec_blocks", "dec_blocks2"): v for k, v in state.items() if k.startswith("dec_blocks")})
        self.sd = {k: v.to(dtype) for k, v in sd.items()}

    def lin(self, key, x):
        return F.linear(x, self.sd[key + ".weight"], self.sd[key + ".bias"])

    def norm(self, key, x):
        return F.layer_norm(x, x.shape[-1:], self.sd[key + ".weight"], self.sd[key + ".bias"], eps=1e-6)

    def self_attn(self, b, x, pos):
        D = x.shape[-1]
        qkv = self.lin(b + "attn.qkv", x)                                              # channel = which D + head 64 + d
        return self.lin(b + "attn.proj", attend(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], pos, pos, self.dtype))

    def mlp(self, b, x):
        return self.lin(b + "mlp.fc2", F.gelu(self.lin(b + "mlp.fc1", x)))

    def encode(self, imgs):
        """[V,3,H,W] -> (feat [V,N,De], pos [V,N,2]): dust3r/patch_embed.py:19-29 then model.py:127-139"""
        x = F.conv2d(imgs.to(self.dtype), self.sd["patch_embed.proj.weight"], self.sd["patch_embed.proj.bias"], stride=16)
        V, _, Ht, Wt = x.shape
        x = x.flatten(2).transpose(1, 2)
        y, xx = torch.meshgrid(torch.arange(Ht, device=x.device), torch.arange(Wt, device=x.device), indexing="ij")
        pos = torch.stack((y, xx), -1).reshape(1, Ht * Wt, 2).expand(V, -1, -1)
        for n in range(self.cfg.enc_depth):
            b = f"enc_blocks.{n}."
            x = x + self.self_attn(b, self.norm(b + "norm1", x), pos)
            x = x + self.mlp(b, self.norm(b + "norm2", x))
        return self.norm("enc_norm", x), pos

    def dec_block(self, b, x, y, xpos, ypos):
        x = x + self.self_attn(b, self.norm(b + "norm1", x), xpos)
        y_ = self.norm(b + "norm_y", y)
        q, k, v = self.lin(b + "cross_attn.projq", self.norm(b + "norm2", x)), self.lin(b + "cross_attn.projk", y_), self.lin(b + "cross_attn.projv", y_)
        x = x + self.lin(b + "cross_attn.proj", attend(q, k, v, xpos, ypos, self.dtype))
        return x + self.mlp(b, self.norm(b + "norm3", x))

    def decode(self, feat, pos, edges):
        """model.py:171-190 on the batch of edges -> (dec1, dec2), the hooked entries of each side's list"""
        e = torch.as_tensor(edges, device=feat.device)
        f1, f2, pos1, pos2 = feat[e[:, 0]], feat[e[:, 1]], pos[e[:, 0]], pos[e[:, 1]]
        final = [(f1, f2)]
        f1, f2 = self.lin("decoder_embed", f1), self.lin("decoder_embed", f2)
        final.append((f1, f2))
        for n in range(self.cfg.dec_depth):
            a, b = final[-1]
            f1 = self.dec_block(f"dec_blocks.{n}.", a, b, pos1, pos2)      # img1 side: final_output[-1][::+1]
            f2 = self.dec_block(f"dec_blocks2.{n}.", b, a, pos2, pos1)     # img2 side: final_output[-1][::-1]
            final.append((f1, f2))
        del final[1]
        final[-1] = (self.norm("dec_norm", final[-1][0]), self.norm("dec_norm", final[-1][1]))
        hooks = self.cfg.hook_layers()
        return tuple(final[h][0] for h in hooks), tuple(final[h][1] for h in hooks)


@functools.lru_cache(maxsize=None)
def _case(net_key, Ht, Wt, V, seed, both_sides, variant):
    net = dict(net_key)
    state, cfg, img = make_state(net, seed, both_sides, variant), config(net), images(V, Ht, Wt, seed)
    edges = EDGE_SETS[V]
    out = {}
    with torch.no_grad():
        for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            ref = Ref(state, cfg, dtype)
            STATS["max_logit"] = 0.0
            feat, pos = ref.encode(img)
            d1, d2 = ref.decode(feat, pos, edges)
            out[name] = dict(feat=feat.double(), dec1=tuple(t.double() for t in d1), dec2=tuple(t.double() for t in d2))
            out["max_logit_" + name] = STATS["max_logit"]
    return dict(state=state, cfg=cfg, images=img, edges=edges, **out)


def case(net, Ht, Wt, V=None, seed=0, both_sides=True, variant="plain"):
    """one case's inputs and yardsticks, computed once per session and shared (nothing writes to them)"""
    return _case(_key(net), Ht, Wt, V or VIEWS[(Ht, Wt)], seed, both_sides, variant)


@functools.lru_cache(maxsize=None)
def _trunk(net_key, seed, both_sides, variant, dev_str):
    from instantsplat_amd.mast3r_trunk import Mast3rTrunk
    net = dict(net_key)
    return Mast3rTrunk(make_state(net, seed, both_sides, variant), config(net), device=None if dev_str == "cpu" else torch.device(dev_str))


def trunk(dev, net, seed=0, both_sides=True, variant="plain"):
    return _trunk(_key(net), seed, both_sides, variant, str(dev))


# ---------------------------------------------------------------------------------------------------- kernel checks
def _errors(got, want):
    d = got.detach().double().cpu() - want
    return float(d.abs().max()), float(d.norm() / (want.norm() + 1e-300))


def _bound_tensor(label, got, c, pick):
    want, twin = pick(c["f64"]), pick(c["f32"])
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.float32, (label, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), label
    e_abs, e_rel = _errors(twin, want)
    d_abs, d_rel = _errors(got, want)
    print(f"VIT {label}: E32 max-abs {e_abs:.3e} device {d_abs:.3e} ({d_abs / max(e_abs, 1e-300):.2f}x) | "
          f"E32 rel-L2 {e_rel:.3e} device {d_rel:.3e} ({d_rel / max(e_rel, 1e-300):.2f}x)")
    ops_util.bound(f"vit max-abs vs float64 in E32 [{label}]", d_abs / max(e_abs, 1e-300), FACTOR)
    ops_util.bound(f"vit rel-L2 vs float64 in E32 [{label}]", d_rel / max(e_rel, 1e-300), FACTOR)


def check_case(dev, net, Ht, Wt, V=None, variant="plain", name=None):
    """encode and decode (four hooks, both sides) of one case against float64 in units of the float32 twin's own error"""
    c = case(net, Ht, Wt, V, variant=variant)
    t = trunk(dev, net, variant=variant)
    label = f"{name or ('thin' if net == THIN else 'real')} {variant} {Ht}x{Wt} V={c['images'].shape[0]}"
    feat, pos = t.encode(c["images"].to(dev))
    assert pos.dtype == torch.int64 and tuple(pos.shape) == (c["images"].shape[0], Ht * Wt, 2)
    assert torch.equal(pos[0, :, 0].cpu(), torch.arange(Ht * Wt) // Wt) and torch.equal(pos[-1, :, 1].cpu(), torch.arange(Ht * Wt) % Wt)
    _bound_tensor(f"{label} feat", feat, c, lambda r: r["feat"])
    dec1, dec2 = t.decode(feat, c["edges"], (Ht, Wt))
    for s, dec in ((1, dec1), (2, dec2)):
        assert len(dec) == 4
        for h in range(4):
            _bound_tensor(f"{label} side {s} hook {h}", dec[h], c, lambda r, s=s, h=h: r[f"dec{s}"][h])
    return c, feat, dec1, dec2


def check_transposed_grids_differ(dev, net=THIN):
    """3 x 5 and 5 x 3: the SAME 15 patches in the same order, laid out on the transposed grid.  Without RoPE the two encodings
    would be equal; they must differ, and each must match float64 (a y / x swap in RoPE gives the other grid's angles)"""
    cfg, state, t = config(net), make_state(net), trunk(dev, net)
    a = images(1, 3, 5)
    seq = a.reshape(1, 3, 3, 16, 5, 16).permute(0, 2, 4, 1, 3, 5).reshape(1, 5, 3, 3, 16, 16)
    b = seq.permute(0, 3, 1, 4, 2, 5).reshape(1, 3, 80, 48).contiguous()
    got = {}
    with torch.no_grad():
        for name, img in (("3x5", a), ("5x3", b)):
            c = {k: dict(feat=Ref(state, cfg, dt).encode(img)[0].double()) for k, dt in (("f64", torch.float64), ("f32", torch.float32))}
            got[name] = t.encode(img.to(dev))[0]
            _bound_tensor(f"thin same patches on {name} feat", got[name], c, lambda r: r["feat"])
    assert got["3x5"].shape == got["5x3"].shape and float((got["3x5"] - got["5x3"]).abs().max()) > 1e-3


def check_attention_against_sdpa():
    """the restatement's attention against F.scaled_dot_product_attention in float64 (same RoPE'd heads)"""
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(2, 15, 128, generator=g, dtype=torch.float64) for _ in range(3))
    y, x = torch.meshgrid(torch.arange(3), torch.arange(5), indexing="ij")
    pos = torch.stack((y, x), -1).reshape(1, 15, 2).expand(2, -1, -1)
    got = attend(q, k, v, pos, pos, torch.float64)
    split = lambda t: t.reshape(2, 15, 2, 64).transpose(1, 2)
    want = F.scaled_dot_product_attention(rope2d(split(q), pos, torch.float64), rope2d(split(k), pos, torch.float64), split(v))
    assert float((got - want.transpose(1, 2).reshape(2, 15, 128)).abs().max()) < 1e-13
    # RoPE is a rotation (norms kept) and relative: logits depend on position differences only
    t = split(q)
    assert torch.allclose(rope2d(t, pos, torch.float64).norm(dim=-1), t.norm(dim=-1), rtol=1e-12)
    shifted = pos + torch.tensor([2, 3])
    la = rope2d(t, pos, torch.float64) @ rope2d(split(k), pos, torch.float64).transpose(-1, -2)
    lb = rope2d(t, shifted, torch.float64) @ rope2d(split(k), shifted, torch.float64).transpose(-1, -2)
    assert float((la - lb).abs().max()) < 1e-11


def check_degenerate_rows(dev, net=THIN, grid=(3, 5)):
    """a zero patch embedding with the constant bias 0.5: the first LayerNorm sees rows of variance exactly 0"""
    c = case(net, *grid, variant="flat")
    x = F.conv2d(c["images"], c["state"]["patch_embed.proj.weight"], c["state"]["patch_embed.proj.bias"], stride=16)
    assert float(x.var(dim=1, unbiased=False).abs().max()) == 0.0 and float(x.min()) == 0.5
    assert all(bool(torch.isfinite(t).all()) for t in (c["f64"]["feat"],) + c["f64"]["dec1"] + c["f64"]["dec2"])
    check_case(dev, net, *grid, variant="flat")


def check_peaked_softmax(dev, net=THIN, grid=(7, 9)):
    """q and k scaled until |logit| passes 80 (asserted on the float64 restatement): exp overflows float32 there unless the
    maximum is subtracted first"""
    c = case(net, *grid, variant="peaked")
    print(f"VIT peaked: largest |logit| of the float64 restatement {c['max_logit_f64']:.1f}")
    assert c["max_logit_f64"] > 80.0
    check_case(dev, net, *grid, variant="peaked")


def check_both_gemm_tiles_are_reached():
    """which GEMMs of the real-width 18 x 32 case (3 images, 6 edges) run on which tile — the rule restated, so that a change of
    the rule or of the case that leaves a tile without a float64 case fails here.  Every smaller case runs 128 x 64 only."""
    enc, dec = 3 * 576, 6 * 576                                    # rows: neither a multiple of 128 (1728 = 13.5, 3456 = 27 tiles)
    assert enc % 128 and wide_tile(enc, 3 * 1024) and wide_tile(enc, 4 * 1024) and not wide_tile(enc, 1024)     # qkv, fc1 | proj, fc2, patches
    assert wide_tile(dec, 3 * 768) and wide_tile(dec, 4 * 768) and not wide_tile(dec, 768)                      # qkv, fc1 | every D -> D
    assert not wide_tile(576, 4 * 1024) and not wide_tile(2 * 576, 4 * 768)     # one image alone, two edges: narrow everywhere
    for Ht, Wt in GRIDS + GRIDS_GPU_ONLY:
        assert not any(wide_tile(6 * Ht * Wt, N) for N in (128, 384, 512, 64, 192, 256)), (Ht, Wt)              # the thin net never
    assert not any(wide_tile(6 * 9 * 15, N) for N in (1024, 3072, 4096, 768, 2304))                             # nor the smaller real-width grids


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_properties(dev, net=THIN, grid=(5, 13)):
    """exact bits: two runs; an image alone against the same image in a batch of 3; an edge set against the matching rows of a
    larger set; hook 0 against the gathered encoder rows"""
    Ht, Wt = grid
    c = case(net, Ht, Wt, 3)
    t = trunk(dev, net)
    img = c["images"].to(dev)
    feat, _ = t.encode(img)
    again, _ = t.encode(img)
    assert _same(feat, again)
    for v in range(3):
        alone, _ = t.encode(img[v:v + 1])
        assert _same(alone[0], feat[v]), v
    edges = c["edges"]
    d1, d2 = t.decode(feat, edges, grid)
    e1, e2 = t.decode(feat, edges, grid)
    assert all(_same(a, b) for a, b in zip(d1 + d2, e1 + e2))
    rows = [4, 1]                                                      # A = two edges of A u B, in another order and place
    a1, a2 = t.decode(feat, [edges[r] for r in rows], grid)
    for h in range(4):
        assert _same(a1[h], d1[h][rows]) and _same(a2[h], d2[h][rows]), h
    idx = torch.tensor(edges)
    assert _same(d1[0], feat[idx[:, 0]]) and _same(d2[0], feat[idx[:, 1]])


def check_shared_decoder_symmetry(dev, net=THIN, grid=(3, 5)):
    """dec_blocks2 absent from the state dict: side 1 of (i, j) equals side 2 of (j, i), bit for bit"""
    Ht, Wt = grid
    t = trunk(dev, net, both_sides=False)
    feat, _ = t.encode(images(3, Ht, Wt).to(dev))
    edges = EDGE_SETS[3]
    d1, d2 = t.decode(feat, edges, grid)
    for a, (i, j) in enumerate(edges):
        b = edges.index((j, i))
        for h in range(4):
            assert _same(d1[h][a], d2[h][b]), (i, j, h)
    # and it is a different network from the one with two decoders
    o1, o2 = trunk(dev, net).decode(trunk(dev, net).encode(images(3, Ht, Wt).to(dev))[0], edges, grid)
    assert not _same(o2[3], d2[3])


def check_chunked_calls(dev, net=THIN, grid=(3, 5)):
    """a scratch budget that forces one edge / one image per call (3+ calls) gives the bits of one call; forward_pairs' default
    edges are make_pairs' complete symmetrized graph"""
    from instantsplat_amd import _lib
    from instantsplat_amd.mast3r_trunk import complete_edges
    Ht, Wt = grid
    t = trunk(dev, net)
    img = images(3, Ht, Wt).to(dev)
    calls = []
    real = _lib.call
    try:
        _lib.call = lambda d, name, *a: (calls.append(name), real(d, name, *a))[1]
        feat, pos, d1, d2, edges = t.forward_pairs(img)
        whole = list(calls)
        del calls[:]
        feat_s, _, s1, s2, _ = t.forward_pairs(img, scratch_budget=1)
    finally:
        _lib.call = real
    assert whole == ["vit_encode", "vit_decode"] and calls == ["vit_encode"] * 3 + ["vit_decode"] * 6
    assert edges.tolist() == [[1, 0], [2, 0], [2, 1], [0, 1], [0, 2], [1, 2]] == complete_edges(3).tolist()
    assert complete_edges(1).tolist() == [[0, 0]] and complete_edges(2).tolist() == [[1, 0], [0, 1]]
    assert _same(feat, feat_s) and all(_same(a, b) for a, b in zip(d1 + d2, s1 + s2))
    budget = int(_lib.lib().mi355gs_vit_decode_scratch_bytes(ctypes.byref(t._cfg_c), Ht, Wt, 2))
    del calls[:]
    try:
        _lib.call = lambda d, name, *a: (calls.append(name), real(d, name, *a))[1]
        m1, m2 = t.decode(feat, edges, grid, scratch_budget=budget)
    finally:
        _lib.call = real
    assert calls == ["vit_decode"] * 3 and all(_same(a, b) for a, b in zip(d1 + d2, m1 + m2))
    # a storage offset that keeps 16-byte alignment is taken as it is
    shifted = torch.cat((torch.zeros(1, *img.shape[1:], device=dev), img))[1:]
    assert shifted.storage_offset() > 0 and _same(t.encode(shifted)[0], feat)
    # one that does not (4 bytes past a boundary: the library would refuse the address) takes a copy in the wrapper
    flat = torch.zeros(img.numel() + 1, device=dev)
    flat[1:] = img.reshape(-1)
    odd = flat[1:].view(img.shape)
    assert odd.data_ptr() % 16 == 4 and odd.is_contiguous() and _same(t.encode(odd)[0], feat)
    fflat = torch.zeros(feat.numel() + 1, device=dev)
    fflat[1:] = feat.reshape(-1)
    o1, o2 = t.decode(fflat[1:].view(feat.shape), edges, grid)
    assert all(_same(a, b) for a, b in zip(d1 + d2, o1 + o2))


# ---------------------------------------------------------------------------------------------------- host side
def check_loader(dev, root):
    from instantsplat_amd.mast3r_trunk import Mast3rTrunk
    import argparse
    d = None if dev.type == "cpu" else dev
    cfg = config(THIN)
    both, one = make_state(THIN), make_state(THIN, both_sides=False)
    base = Mast3rTrunk(both, cfg, device=d)
    explicit = dict(one)
    explicit.update({k.replace("dec_blocks", "dec_blocks2"): v for k, v in one.items() if k.startswith("dec_blocks")})
    assert torch.equal(Mast3rTrunk(one, cfg, device=d).blob, Mast3rTrunk(explicit, cfg, device=d).blob)     # duplicated = explicit copy
    assert not torch.equal(Mast3rTrunk(one, cfg, device=d).blob, base.blob)
    extra = dict(both)
    extra.update({"mask_token": torch.zeros(1, 1, 64), "downstream_head1.dpt.act_postprocess.0.0.weight": torch.zeros(3, 3),
                  "downstream_head2.head_local_features.fc1.bias": torch.zeros(7), "enc_pos_embed": torch.zeros(2)})
    assert torch.equal(Mast3rTrunk(extra, cfg, device=d).blob, base.blob)
    for key, bad in (("patch_embed.proj.bias", torch.zeros(7)), ("patch_embed.proj.weight", torch.zeros(128, 3, 8, 8))):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            Mast3rTrunk(dict(both, **{key: bad}), cfg, device=d)
    for key in ("enc_blocks.1.attn.qkv.bias", "dec_blocks.3.norm_y.weight", "dec_blocks2.0.cross_attn.projk.weight", "dec_norm.bias",
                "patch_embed.proj.weight", "decoder_embed.bias"):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            Mast3rTrunk({k: v for k, v in both.items() if k != key}, cfg, device=d)
    # the blob's layout (include/mi355gs.h): the patch embedding first, [768][De] = torch's weight flattened and transposed
    De = THIN["enc_dim"]
    assert torch.equal(base.blob[:768 * De].cpu().reshape(768, De), both["patch_embed.proj.weight"].reshape(De, 768).t())
    assert torch.equal(base.blob[-THIN["dec_dim"]:].cpu(), both["dec_norm.bias"])
    # a file in the checkpoint's shape: {'args': Namespace, 'model': state dict, ...}
    os.makedirs(root, exist_ok=True)
    path = os.path.join(root, "ckpt.pth")
    torch.save({"args": argparse.Namespace(model="AsymmetricMASt3R(...)", lr=1e-4), "model": extra, "epoch": 3}, path)
    assert torch.equal(Mast3rTrunk.from_checkpoint(path, cfg, device=d).blob, base.blob)
    torch.save(both, path)
    with pytest.raises(ValueError, match="model"):
        Mast3rTrunk.from_checkpoint(path, cfg, device=d)


def check_value_errors(dev):
    from instantsplat_amd.mast3r_trunk import Mast3rTrunk, TrunkConfig
    d = None if dev.type == "cpu" else dev
    t = trunk(dev, THIN)
    ok = torch.zeros(2, 3, 32, 48, device=dev)
    for bad in (ok[:, :, :31], ok[:, :, :, :40], ok.double(), ok[0], ok[:, :2], ok.to(torch.uint8), ok.cpu().numpy(), ok[:0],
                torch.zeros(1, 3, 16 * 65, 16 * 64, device=dev)):
        with pytest.raises(ValueError):
            t.encode(bad)
    feat, _ = t.encode(ok)
    for edges in ([(0, 2)], [(-1, 0)], [(0, 1, 1)], [], [(0.0, 1.0)], torch.zeros(2, 2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            t.decode(feat, edges, (2, 3))
    with pytest.raises(TypeError):
        t.decode(feat, [(0, 1)])                       # the grid is an argument, not something a past encode left behind
    for f, grid in ((feat, (3, 3)), (feat, None), (feat, 6), (feat, (6,)), (feat.double(), (2, 3)), (feat[0], (2, 3)), (feat[:, :, :64], (2, 3))):
        with pytest.raises(ValueError):
            t.decode(f, [(0, 1)], grid)
    state = make_state(THIN)
    for over in (dict(enc_dim=96, enc_heads=1), dict(enc_dim=128, enc_heads=4), dict(dec_dim=1088, dec_heads=17), dict(patch=8),
                 dict(hooks=(0, 2, 2, 4)), dict(hooks=(0, 1, 2, 3)), dict(hooks=(1, 2, 3, 4))):
        with pytest.raises(ValueError):
            Mast3rTrunk(state, TrunkConfig(**dict(THIN, **over)), device=d)
    with pytest.raises(ValueError, match="expected"):
        Mast3rTrunk(state, TrunkConfig(**dict(THIN, dec_dim=128, dec_heads=2)), device=d)      # widths that do not follow the tensors


def check_cpu_tensors_refused():
    """the product path (no emulated library bound) refuses CPU tensors in _lib.gpu_only()'s words"""
    from instantsplat_amd import _lib
    from instantsplat_amd.mast3r_trunk import Mast3rTrunk
    _lib._use_library_for_testing(None)
    state, cfg = make_state(THIN), config(THIN)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU only"):
            Mast3rTrunk(state, cfg)
        return
    t = Mast3rTrunk(state, cfg)
    assert t.blob.is_cuda
    with pytest.raises(ValueError, match="on the GPU only"):
        t.encode(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="on the GPU only"):
        t.decode(torch.zeros(1, 1, THIN["enc_dim"]), [(0, 0)], (1, 1))


def check_entry_points_reject_bad_arguments():
    """Argument checks of the four entry points, before any HIP call (bogus device pointers are never touched)."""
    from instantsplat_amd import _lib
    from instantsplat_amd.mast3r_trunk import _Config
    L = _lib.lib()
    EINVAL = -1
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below must fail its checks first
    odd = ctypes.c_void_p(0x1008)    # off a 16-byte boundary

    def cfg(**over):
        net = dict(dict(THIN, patch=16), **over)
        return _Config(net["enc_dim"], net["enc_depth"], net["enc_heads"], net["dec_dim"], net["dec_depth"], net["dec_heads"], net["patch"],
                       (ctypes.c_int * 4)(*net["hooks"]))
    outs = (ctypes.c_void_p * 4)(*[0x1000] * 4)
    edges_of = lambda *e: (ctypes.c_int32 * len(e))(*e)   # host memory, as the header says

    def enc(c=cfg(), Ht=2, Wt=3, V=2, weights=fake, rope=fake, images=fake, scratch=fake, feat=fake):
        return L.mi355gs_vit_encode(None, ctypes.byref(c) if c is not None else None, weights, rope, Ht, Wt, V, images, scratch, feat)

    def dec(c=cfg(), Ht=2, Wt=3, V=2, E=1, weights=fake, rope=fake, edges=edges_of(0, 1), feat=fake, scratch=fake, out1=outs, out2=outs):
        return L.mi355gs_vit_decode(None, ctypes.byref(c) if c is not None else None, weights, rope, Ht, Wt, V, E, edges, feat, scratch, out1, out2)
    for kw in ("c", "weights", "rope", "images", "scratch", "feat"):
        assert enc(**{kw: None}) == EINVAL, kw
    for kw in ("c", "weights", "rope", "edges", "feat", "scratch", "out1", "out2"):
        assert dec(**{kw: None}) == EINVAL, kw
    for kw in ("weights", "images", "scratch", "feat"):
        assert enc(**{kw: odd}) == EINVAL, kw
    for kw in ("weights", "feat", "scratch"):
        assert dec(**{kw: odd}) == EINVAL, kw
    assert dec(out1=(ctypes.c_void_p * 4)(0x1000, 0x1000, 0x1008, 0x1000)) == EINVAL
    assert dec(out2=(ctypes.c_void_p * 4)(0x1000, 0, 0x1000, 0x1000)) == EINVAL
    bad_cfg = (dict(enc_dim=96, enc_heads=1), dict(enc_dim=160, enc_heads=2), dict(enc_heads=3), dict(dec_heads=2), dict(dec_dim=1088, dec_heads=17),
               dict(enc_dim=0, enc_heads=0), dict(enc_depth=0), dict(dec_depth=0, hooks=(0, 0, 0, 0)), dict(patch=8), dict(hooks=(0, 2, 2, 4)),
               dict(hooks=(0, 1, 2, 3)), dict(hooks=(1, 2, 3, 4)))
    for over in bad_cfg:
        c = cfg(**over)
        assert enc(c=c) == EINVAL and dec(c=c) == EINVAL, over
        assert L.mi355gs_vit_encode_scratch_bytes(ctypes.byref(c), 2, 3, 2) == 0 and L.mi355gs_vit_decode_scratch_bytes(ctypes.byref(c), 2, 3, 1) == 0
    for kw in (dict(Ht=0), dict(Wt=-1), dict(Ht=65, Wt=64), dict(V=0), dict(V=257)):
        assert enc(**kw) == EINVAL, kw
        assert L.mi355gs_vit_encode_scratch_bytes(ctypes.byref(cfg()), kw.get("Ht", 2), kw.get("Wt", 3), kw.get("V", 2)) == 0
    for kw in (dict(Ht=0), dict(Ht=65, Wt=64), dict(V=0), dict(V=257), dict(E=0), dict(E=65536)):
        assert dec(**kw) == EINVAL, kw
    assert L.mi355gs_vit_decode_scratch_bytes(ctypes.byref(cfg()), 2, 3, 0) == 0 and L.mi355gs_vit_decode_scratch_bytes(ctypes.byref(cfg()), 2, 3, 65536) == 0
    for e in ((0, 2), (2, 0), (-1, 0), (0, -1)):
        assert dec(edges=edges_of(*e)) == EINVAL, e
    assert dec(E=2, edges=edges_of(0, 1, 1, 2)) == EINVAL
    assert L.mi355gs_vit_encode_scratch_bytes(None, 2, 3, 2) == 0 and L.mi355gs_vit_decode_scratch_bytes(None, 2, 3, 1) == 0
    c = cfg()
    M = 2 * 6
    assert L.mi355gs_vit_encode_scratch_bytes(ctypes.byref(c), 2, 3, 2) >= M * 4 * (128 + 3 * 128 + 768)
    assert L.mi355gs_vit_decode_scratch_bytes(ctypes.byref(c), 2, 3, 2) >= M * 4 * 64 * (4 + 1 + 1 + 3 + 4)
    assert L.mi355gs_abi_version() == 10
