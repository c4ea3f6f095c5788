"""MASt3R's dense heads on the device — `downstream_head1` / `downstream_head2` of dust3r/model.py:192-210: the DPT head that turns
the four hooked token tensors of one side (Mast3rTrunk.decode's, as they are) into a pointmap and a confidence per pixel, and the
local-feature MLP of mast3r/catmlp_dpt_head.py (csrc/dpt.hip, include/mi355gs.h mi355gs_dpt_head / mi355gs_local_features).

The order of operations is the reference's (dust3r/heads/dpt_head.py, mast3r/catmlp_dpt_head.py, dust3r/heads/postprocess.py); the
block definitions — croco's DPT adapter, ResidualConvUnit, FeatureFusionBlock, Mlp — are the published ones, recalled, and checked
here against a float64 restatement on seeded weights (tests/heads_util.py).  The trained checkpoint is not part of this package
and no test pins a real output.
"""
from __future__ import annotations

import argparse
import ctypes
import math
from dataclasses import dataclass

import torch

from . import _frames, _lib
from .mast3r_trunk import DEFAULT_SCRATCH_BUDGET, _tensor

TAPS = ("L0", "L1", "L2", "L3", "path_4", "path_3", "path_2", "path_1")


class _Config(ctypes.Structure):   # include/mi355gs.h mi355gs_dpt_config
    _fields_ = [("dim_tokens", ctypes.c_int * 4), ("layer_dims", ctypes.c_int * 4), ("feature_dim", ctypes.c_int), ("last_dim", ctypes.c_int),
                ("mlp_hidden", ctypes.c_int), ("local_feat_dim", ctypes.c_int), ("two_confs", ctypes.c_int), ("conf_vmin", ctypes.c_float),
                ("conf_vmax", ctypes.c_float), ("desc_conf_vmin", ctypes.c_float), ("desc_conf_vmax", ctypes.c_float)]


@dataclass(frozen=True)
class HeadsConfig:
    """The sizes and modes; the defaults are MASt3R_ViTLarge_BaseDecoder_512_catmlpdpt_metric's (mast3r_head_factory with
    'pts3d+desc24', depth_mode ('exp', -inf, inf), conf_mode ('exp', 1, inf), desc_conf_mode ('exp', 0, inf), two_confs).  They are
    stated here, never evaluated from the checkpoint's `args` string."""
    dim_tokens: tuple = (1024, 768, 768, 768)
    layer_dims: tuple = (96, 192, 384, 768)
    feature_dim: int = 256
    last_dim: int = 128
    local_feat_dim: int = 24
    hidden_dim_factor: float = 4.0
    two_confs: bool = True
    depth_mode: tuple = ("exp", -math.inf, math.inf)
    conf_mode: tuple = ("exp", 1.0, math.inf)
    desc_conf_mode: tuple | None = ("exp", 0.0, math.inf)
    desc_mode: str = "norm"

    def mlp_hidden(self):
        return int(self.hidden_dim_factor * (self.dim_tokens[0] + self.dim_tokens[3]))


def _conv1(sd, key, K, N):
    """a 1x1 convolution [N,K,1,1] -> [K][N] + bias"""
    w, b = _tensor(sd, key + ".weight"), _tensor(sd, key + ".bias")
    if tuple(w.shape) != (N, K, 1, 1) or tuple(b.shape) != (N,):
        raise ValueError(f"{key}: weight {tuple(w.shape)}, bias {tuple(b.shape)}; expected ({N}, {K}, 1, 1) and ({N},)")
    return [w.reshape(N, K).t().contiguous().reshape(-1), b]


def _conv3(sd, key, K, N, bias=True):
    """a 3x3 convolution [N,K,3,3] -> [(3 ky + kx) K + ci][N] (+ bias)"""
    w = _tensor(sd, key + ".weight")
    if tuple(w.shape) != (N, K, 3, 3):
        raise ValueError(f"{key}.weight {tuple(w.shape)}; expected ({N}, {K}, 3, 3)")
    out = [w.permute(2, 3, 1, 0).contiguous().reshape(-1)]
    if bias:
        b = _tensor(sd, key + ".bias")
        if tuple(b.shape) != (N,):
            raise ValueError(f"{key}.bias {tuple(b.shape)}; expected ({N},)")
        out.append(b)
    return out


def _convT(sd, key, C, s):
    """a ConvTranspose [C,C,s,s] with stride s -> [ci][(dy s + dx) C + co] + the bias repeated s s times"""
    w, b = _tensor(sd, key + ".weight"), _tensor(sd, key + ".bias")
    if tuple(w.shape) != (C, C, s, s) or tuple(b.shape) != (C,):
        raise ValueError(f"{key}: weight {tuple(w.shape)}, bias {tuple(b.shape)}; expected ({C}, {C}, {s}, {s}) and ({C},)")
    return [w.permute(0, 2, 3, 1).contiguous().reshape(-1), b.repeat(s * s)]


def _linear(sd, key, K, N):
    w, b = _tensor(sd, key + ".weight"), _tensor(sd, key + ".bias")
    if tuple(w.shape) != (N, K) or tuple(b.shape) != (N,):
        raise ValueError(f"{key}: weight {tuple(w.shape)}, bias {tuple(b.shape)}; expected ({N}, {K}) and ({N},)")
    return [w.t().contiguous().reshape(-1), b]


def _pack_head(sd, prefix, cfg: HeadsConfig):
    """-> (dpt floats, mlp floats) of one head, in the header's order"""
    ct, ld, F, LD = cfg.dim_tokens, cfg.layer_dims, cfg.feature_dim, cfg.last_dim
    d = prefix + "dpt."
    parts = []
    for k in range(4):
        parts += _conv1(sd, f"{d}act_postprocess.{k}.0", ct[k], ld[k])
        if k < 2:
            parts += _convT(sd, f"{d}act_postprocess.{k}.1", ld[k], 4 if k == 0 else 2)
        elif k == 3:
            parts += _conv3(sd, f"{d}act_postprocess.3.1", ld[3], ld[3])
    for k in range(4):   # the checkpoint holds the same tensor as layer_rn.K and layerK+1_rn: either is taken, layer_rn first
        key = f"{d}scratch.layer_rn.{k}"
        if key + ".weight" not in sd and f"{d}scratch.layer{k + 1}_rn.weight" in sd:
            key = f"{d}scratch.layer{k + 1}_rn"
        parts += _conv3(sd, key, ld[k], F, bias=False)
    for n in (4, 3, 2, 1):
        r = f"{d}scratch.refinenet{n}."
        for unit in (("resConfUnit2",) if n == 4 else ("resConfUnit1", "resConfUnit2")):   # refinenet4.resConfUnit1: unused
            parts += _conv3(sd, f"{r}{unit}.conv1", F, F) + _conv3(sd, f"{r}{unit}.conv2", F, F)
        parts += _conv1(sd, r + "out_conv", F, F)
    parts += _conv3(sd, d + "head.0", F, F // 2) + _conv3(sd, d + "head.2", F // 2, LD)
    w4, b4 = _tensor(sd, d + "head.4.weight"), _tensor(sd, d + "head.4.bias")
    if tuple(w4.shape) != (4, LD, 1, 1) or tuple(b4.shape) != (4,):
        raise ValueError(f"{d}head.4: weight {tuple(w4.shape)}, bias {tuple(b4.shape)}; expected (4, {LD}, 1, 1) and (4,)")
    pad_w, pad_b = torch.zeros(LD, 32), torch.zeros(32)
    pad_w[:, :4] = w4.reshape(4, LD).t()
    pad_b[:4] = b4
    parts += [pad_w.reshape(-1), pad_b]
    K, hid = ct[0] + ct[3], cfg.mlp_hidden()
    m = prefix + "head_local_features."
    mlp = _linear(sd, m + "fc1", K, hid) + _linear(sd, m + "fc2", hid, (cfg.local_feat_dim + int(cfg.two_confs)) * 256)
    return torch.cat([p.reshape(-1) for p in parts]), torch.cat([p.reshape(-1) for p in mlp])


class Mast3rHeads:
    """Both packed heads.  state_dict: the checkpoint's `model` dict (keys `downstream_head{1,2}.dpt.*`,
    `downstream_head{1,2}.head_local_features.*`; the trunk's keys are ignored).  Raises ValueError naming a missing key, for shapes
    that do not follow `config`, for modes other than the checkpoint's and for sizes the kernels do not take."""

    def __init__(self, state_dict, config: HeadsConfig | None = None, device=None):
        cfg = config or HeadsConfig()
        if tuple(cfg.depth_mode) != ("exp", -math.inf, math.inf):
            raise ValueError(f"depth_mode {cfg.depth_mode}: only ('exp', -inf, inf) is built")
        dcm = cfg.desc_conf_mode if cfg.desc_conf_mode is not None else cfg.conf_mode
        for name, mode in (("conf_mode", cfg.conf_mode), ("desc_conf_mode", dcm)):
            if len(mode) != 3 or mode[0] != "exp" or not mode[2] > mode[1]:
                raise ValueError(f"{name} {mode}: only ('exp', vmin, vmax > vmin) is built")
        if cfg.desc_mode != "norm":
            raise ValueError(f"Unknown desc mode {cfg.desc_mode}")
        F, LD = cfg.feature_dim, cfg.last_dim
        if len(cfg.dim_tokens) != 4 or len(cfg.layer_dims) != 4 or any(c < 32 or c % 32 or c > 4096 for c in cfg.dim_tokens) \
                or any(c < 32 or c % 32 or c > 1024 for c in cfg.layer_dims) or F < 64 or F > 256 or F % 64 or LD < 32 or LD > 128 or LD % 32 \
                or not 1 <= cfg.local_feat_dim <= 255 or cfg.mlp_hidden() % 32 or not 32 <= cfg.mlp_hidden() <= 32768:
            raise ValueError(f"{cfg}: the kernels take channel counts that are multiples of 32, feature_dim a multiple of 64 up to 256, "
                             "last_dim up to 128 and local_feat_dim up to 255")
        dev = _frames.device_of((), default=device)
        packed = [_pack_head(state_dict, f"downstream_head{s}.", cfg) for s in (1, 2)]
        self._n_dpt = int(packed[0][0].numel())
        self.config = cfg
        # ONE blob: head 1's DPT part, its MLP, head 2's DPT part, its MLP (every part a multiple of 32 floats: 16-byte aligned views)
        self.blob = torch.cat([t for pair in packed for t in pair]).contiguous().to(dev)
        n_head = int(packed[0][0].numel() + packed[0][1].numel())
        self._dpt = [self.blob[s * n_head:s * n_head + self._n_dpt] for s in range(2)]
        self._mlp = [self.blob[s * n_head + self._n_dpt:(s + 1) * n_head] for s in range(2)]
        self._cfg_c = _Config((ctypes.c_int * 4)(*cfg.dim_tokens), (ctypes.c_int * 4)(*cfg.layer_dims), F, LD, cfg.mlp_hidden(), cfg.local_feat_dim,
                              int(cfg.two_confs), cfg.conf_mode[1], cfg.conf_mode[2], dcm[1], dcm[2])

    @classmethod
    def from_checkpoint(cls, path, config: HeadsConfig | None = None, device=None):
        """The heads of a MASt3R checkpoint file: `ckpt['model']`, read with weights_only=True (the file's `args` Namespace is let
        through and never evaluated)."""
        return cls(load_checkpoint_model(path), config, device=device)

    # ------------------------------------------------------------------------------------------------ the stage
    def _check(self, dec, side, grid):
        cfg = self.config
        if not isinstance(dec, (tuple, list)) or len(dec) != 4:
            raise ValueError(f"dec{side}: the four hooked tensors of Mast3rTrunk.decode, got {type(dec)}")
        out = []
        for k, t in enumerate(dec):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != cfg.dim_tokens[k]:
                raise ValueError(f"dec{side}[{k}] must be float32 [E, N, {cfg.dim_tokens[k]}], got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)} {getattr(t, 'dtype', '')}")
            if not t.is_cuda and not _lib._TEST_MODE:
                raise ValueError(_lib.gpu_only("Mast3rHeads.heads runs") + ": pass the tensors on the device")
            if tuple(t.shape[:2]) != tuple(dec[0].shape[:2]):
                raise ValueError(f"dec{side}[{k}] has {tuple(t.shape[:2])} edges x tokens, dec{side}[0] {tuple(dec[0].shape[:2])}")
            t = t.contiguous()
            out.append(t if t.data_ptr() % 16 == 0 else t.clone())
        return out

    def heads(self, dec1, dec2, grid, descriptors=False, scratch_budget: int = DEFAULT_SCRATCH_BUDGET, taps=None):
        """dec1, dec2: Mast3rTrunk.decode's tuples, grid = (Ht, Wt) -> (out1, out2): per side a dict of `pts3d` float32 [E,H,W,3] and
        `conf` [E,H,W] (H = 16 Ht, W = 16 Wt) and, with descriptors=True, `desc` [E,H,W,local_feat_dim] and `desc_conf` [E,H,W].
        E is split into calls whose scratch stays under `scratch_budget` (at least one edge per call).
        taps: a list that receives, per side, a dict of the intermediates the library leaves in its scratch (TAPS, channels-last,
        plus `raw4`, the four channels in front of postprocess) — calibration only: it forces one edge set per call to be copied out."""
        try:
            Ht, Wt = (int(g) for g in grid)
        except (TypeError, ValueError):
            raise ValueError(f"grid: the token grid (Ht, Wt), got {grid!r}") from None
        sides = [self._check(dec1, 1, grid), self._check(dec2, 2, grid)]
        E, N = int(sides[0][0].shape[0]), int(sides[0][0].shape[1])
        if tuple(sides[1][0].shape[:2]) != (E, N) or Ht < 1 or Ht * Wt != N or N > 4096 or E < 1:
            raise ValueError(f"{E} edges of {N} tokens (side 2: {tuple(sides[1][0].shape[:2])}) do not fit a grid of {Ht} x {Wt} (at most 4096 tokens)")
        dev = _lib.require_device(self.blob, *sides[0], *sides[1])
        cfgp, cfg = self.config, ctypes.byref(self._cfg_c)
        H, W, D = 16 * Ht, 16 * Wt, cfgp.local_feat_dim
        L = _lib.lib()

        def need(k):
            a = int(L.mi355gs_dpt_head_scratch_bytes(cfg, Ht, Wt, k))
            b = int(L.mi355gs_local_features_scratch_bytes(cfg, Ht, Wt, k)) if descriptors else 1
            return max(a, b) if a and b else 0
        n = _frames.frames_per_call(lambda k: 0 < need(k) <= scratch_budget, min(E, 65535), int(scratch_budget) // max(need(1), 1))
        what = f"mi355gs_dpt_head does not take {n} edges of {Ht} x {Wt} tokens"
        if not need(n):
            raise ValueError(what)
        scratch = torch.empty(need(n), dtype=torch.uint8, device=dev)
        outs = []
        for s in range(2):
            o = dict(pts3d=torch.empty(E, H, W, 3, dtype=torch.float32, device=dev), conf=torch.empty(E, H, W, dtype=torch.float32, device=dev))
            if descriptors:
                o["desc"] = torch.empty(E, H, W, D, dtype=torch.float32, device=dev)
                if cfgp.two_confs:
                    o["desc_conf"] = torch.empty(E, H, W, dtype=torch.float32, device=dev)
            outs.append(o)
        tapped = [dict() for _ in range(2)] if taps is not None else None
        for first in range(0, E, n):
            m = min(n, E - first)
            for s in range(2):
                o = outs[s]
                hooks = (ctypes.c_void_p * 4)(*[t[first:first + m].data_ptr() for t in sides[s]])
                raw4 = torch.empty(m, H, W, 4, dtype=torch.float32, device=dev) if tapped is not None else None
                _lib.call(dev, "dpt_head", _lib.STREAM, cfg, self._dpt[s], Ht, Wt, m, hooks, scratch, o["pts3d"][first:first + m],
                          o["conf"][first:first + m], raw4)
                if tapped is not None:
                    self._read_taps(tapped[s], scratch, Ht, Wt, m, raw4)
                if descriptors:
                    _lib.call(dev, "local_features", _lib.STREAM, cfg, self._mlp[s], Ht, Wt, m, sides[s][0][first:first + m],
                              sides[s][3][first:first + m], scratch, o["desc"][first:first + m],
                              o["desc_conf"][first:first + m] if cfgp.two_confs else None)
        if descriptors and not cfgp.two_confs:
            for o in outs:
                o["desc_conf"] = o["conf"].clone()
        if taps is not None:
            taps.extend({k: torch.cat(v) for k, v in t.items()} for t in tapped)
        return outs[0], outs[1]

    def _read_taps(self, into, scratch, Ht, Wt, m, raw4):
        cfg, F = ctypes.byref(self._cfg_c), self.config.feature_dim
        h3, w3 = (Ht + 1) // 2, (Wt + 1) // 2
        shapes = [(4 * Ht, 4 * Wt), (2 * Ht, 2 * Wt), (Ht, Wt), (h3, w3), (Ht, Wt), (2 * Ht, 2 * Wt), (4 * Ht, 4 * Wt), (8 * Ht, 8 * Wt)]
        for which, (name, (h, w)) in enumerate(zip(TAPS, shapes)):
            off = int(_lib.lib().mi355gs_dpt_head_tap_offset(cfg, Ht, Wt, m, which))
            assert off > 0, name
            nbytes = m * h * w * F * 4
            into.setdefault(name, []).append(scratch[off:off + nbytes].view(torch.float32).view(m, h, w, F).clone())
        into.setdefault("raw4", []).append(raw4)


def load_checkpoint_model(path):
    """`ckpt['model']` of a MASt3R / DUSt3R checkpoint file, read with weights_only=True"""
    with torch.serialization.safe_globals([argparse.Namespace]):
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ckpt, dict) or "model" not in ckpt:
        raise ValueError(f"{path}: not a checkpoint with a 'model' state dict")
    return ckpt["model"]
