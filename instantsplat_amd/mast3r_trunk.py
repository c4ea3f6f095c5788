"""MASt3R's transformer trunk on the device — the ViT encoder, `decoder_embed` and the two cross-attending decoders behind the
reference's `inference(pairs, model, device, batch_size=1)` (init_geo.py:45; dust3r/model.py:127-190), as two library calls
(csrc/vit.hip, include/mi355gs.h mi355gs_vit_encode / mi355gs_vit_decode).  Every image is encoded ONCE and every directed pair
decoded, where the reference's loop encodes both images of every pair (2 V (V - 1) encoder passes for V images).

The arithmetic is built and checked here against a float64 restatement on seeded weights (tests/vit_util.py); the block
definitions are the published croco ones, recalled — the trained checkpoint is not part of this package and no test pins a real
output.  The DPT heads, the local-feature MLP and the assembly of `inference()`'s output are mast3r_heads.py and mast3r.py: `decode`
returns what the heads read.
"""
from __future__ import annotations

import argparse
import ctypes
from dataclasses import dataclass

import torch

from . import _frames, _lib

DEFAULT_SCRATCH_BUDGET = 4 << 30


class _Config(ctypes.Structure):   # include/mi355gs.h mi355gs_vit_config
    _fields_ = [("enc_dim", ctypes.c_int), ("enc_depth", ctypes.c_int), ("enc_heads", ctypes.c_int), ("dec_dim", ctypes.c_int),
                ("dec_depth", ctypes.c_int), ("dec_heads", ctypes.c_int), ("patch", ctypes.c_int), ("hooks", ctypes.c_int * 4)]


@dataclass(frozen=True)
class TrunkConfig:
    """The sizes; the defaults are MASt3R_ViTLarge_BaseDecoder_512's.  hooks: None = [0, L 2 // 4, L 3 // 4, L] of the decoder
    depth L (mast3r/catmlp_dpt_head.py:115-116)."""
    enc_dim: int = 1024
    enc_depth: int = 24
    enc_heads: int = 16
    dec_dim: int = 768
    dec_depth: int = 12
    dec_heads: int = 12
    patch: int = 16
    rope_base: float = 100.0
    hooks: tuple | None = None

    def hook_layers(self):
        L = self.dec_depth
        return tuple(self.hooks) if self.hooks is not None else (0, L * 2 // 4, L * 3 // 4, L)


def _linear(sd, key, K, N):
    w, b = _tensor(sd, key + ".weight"), _tensor(sd, key + ".bias")
    if tuple(w.shape) != (N, K) or tuple(b.shape) != (N,):
        raise ValueError(f"{key}: weight {tuple(w.shape)}, bias {tuple(b.shape)}; expected ({N}, {K}) and ({N},)")
    return [w.t().contiguous().reshape(-1), b]


def _norm(sd, key, D):
    w, b = _tensor(sd, key + ".weight"), _tensor(sd, key + ".bias")
    if tuple(w.shape) != (D,) or tuple(b.shape) != (D,):
        raise ValueError(f"{key}: weight {tuple(w.shape)}, bias {tuple(b.shape)}; expected ({D},) twice")
    return [w, b]


def _tensor(sd, key):
    if key not in sd:
        raise ValueError(f"the state dict lacks {key}")
    return sd[key].detach().to("cpu", torch.float32)


class Mast3rTrunk:
    """The packed trunk.  state_dict: the checkpoint's `model` dict (keys `patch_embed.proj`, `enc_blocks.N.*`, `enc_norm`,
    `decoder_embed`, `dec_blocks.N.*`, `dec_blocks2.N.*`, `dec_norm`); absent `dec_blocks2.*` keys are taken from `dec_blocks.*`
    (dust3r/model.py:90-97); `mask_token` and the heads' keys are ignored.  The blob the library reads is packed once, here,
    with torch ops.  Raises ValueError naming a missing key, for shapes that do not follow `config`, and for sizes the kernels do
    not take (widths: multiples of 64 up to 1024 with heads of 64 channels; patch 16)."""

    def __init__(self, state_dict, config: TrunkConfig | None = None, device=None):
        cfg = config or TrunkConfig()
        hooks = cfg.hook_layers()
        for name, D, heads in (("encoder", cfg.enc_dim, cfg.enc_heads), ("decoder", cfg.dec_dim, cfg.dec_heads)):
            if D < 64 or D > 1024 or D % 64 or heads * 64 != D:
                raise ValueError(f"{name} width {D} with {heads} heads: the kernels take multiples of 64 up to 1024 and heads of 64 channels")
        if cfg.patch != 16 or cfg.enc_depth < 1 or cfg.dec_depth < 1 or cfg.enc_depth > 256 or cfg.dec_depth > 256:
            raise ValueError(f"patch {cfg.patch}, depths {cfg.enc_depth} / {cfg.dec_depth}: the kernels take patch 16 and depths 1..256")
        if len(hooks) != 4 or not (0 == hooks[0] < hooks[1] < hooks[2] < hooks[3] == cfg.dec_depth):
            raise ValueError(f"hooks {hooks}: need 0 = h0 < h1 < h2 < h3 = decoder depth {cfg.dec_depth}")
        sd = dict(state_dict)
        if not any(k.startswith("dec_blocks2") for k in sd):
            for key, value in state_dict.items():
                if key.startswith("dec_blocks"):
                    sd[key.replace("dec_blocks", "dec_blocks2")] = value
        De, Dd, K0 = cfg.enc_dim, cfg.dec_dim, 3 * cfg.patch * cfg.patch
        w0 = _tensor(sd, "patch_embed.proj.weight")
        if tuple(w0.shape) != (De, 3, cfg.patch, cfg.patch):
            raise ValueError(f"patch_embed.proj.weight {tuple(w0.shape)}; expected ({De}, 3, {cfg.patch}, {cfg.patch})")
        b0 = _tensor(sd, "patch_embed.proj.bias")
        if tuple(b0.shape) != (De,):
            raise ValueError(f"patch_embed.proj.bias {tuple(b0.shape)}; expected ({De},)")
        parts = [w0.reshape(De, K0).t().contiguous().reshape(-1), b0]
        for n in range(cfg.enc_depth):
            b = f"enc_blocks.{n}."
            parts += _norm(sd, b + "norm1", De) + _linear(sd, b + "attn.qkv", De, 3 * De) + _linear(sd, b + "attn.proj", De, De)
            parts += _norm(sd, b + "norm2", De) + _linear(sd, b + "mlp.fc1", De, 4 * De) + _linear(sd, b + "mlp.fc2", 4 * De, De)
        parts += _norm(sd, "enc_norm", De) + _linear(sd, "decoder_embed", De, Dd)
        for side in ("dec_blocks", "dec_blocks2"):
            for n in range(cfg.dec_depth):
                b = f"{side}.{n}."
                parts += _norm(sd, b + "norm1", Dd) + _linear(sd, b + "attn.qkv", Dd, 3 * Dd) + _linear(sd, b + "attn.proj", Dd, Dd)
                parts += _norm(sd, b + "norm_y", Dd) + _norm(sd, b + "norm2", Dd)
                for p in ("projq", "projk", "projv", "proj"):
                    parts += _linear(sd, b + "cross_attn." + p, Dd, Dd)
                parts += _norm(sd, b + "norm3", Dd) + _linear(sd, b + "mlp.fc1", Dd, 4 * Dd) + _linear(sd, b + "mlp.fc2", 4 * Dd, Dd)
        parts += _norm(sd, "dec_norm", Dd)
        self.config = cfg
        self.hooks = hooks
        self._cfg_c = _Config(De, cfg.enc_depth, cfg.enc_heads, Dd, cfg.dec_depth, cfg.dec_heads, cfg.patch, (ctypes.c_int * 4)(*hooks))
        self.blob = torch.cat([p.reshape(-1) for p in parts]).contiguous().to(_frames.device_of((), default=device))
        self._rope = {}

    @classmethod
    def from_checkpoint(cls, path, config: TrunkConfig | None = None, device=None):
        """The trunk of a MASt3R / DUSt3R checkpoint file: `ckpt['model']`, read with weights_only=True (the file's `args`
        Namespace is let through, nothing else)."""
        with torch.serialization.safe_globals([argparse.Namespace]):
            ckpt = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(ckpt, dict) or "model" not in ckpt:
            raise ValueError(f"{path}: not a checkpoint with a 'model' state dict")
        return cls(ckpt["model"], config, device=device)

    # ------------------------------------------------------------------------------------------------ helpers
    def _rope_table(self, Ht, Wt, dev):
        """cos [P][16] then sin [P][16], P = max(Ht, Wt): float32 cos / sin of float32 angles, built once per grid with torch"""
        key = (max(Ht, Wt), str(dev))
        if key not in self._rope:
            inv_freq = 1.0 / (self.config.rope_base ** (torch.arange(0, 32, 2, dtype=torch.float32, device=dev) / 32))
            angle = torch.arange(key[0], dtype=torch.float32, device=dev)[:, None] * inv_freq[None, :]
            self._rope[key] = torch.stack((angle.cos(), angle.sin())).contiguous()
        return self._rope[key]

    def _check_device(self, who, t):
        if not t.is_cuda and not _lib._TEST_MODE:
            raise ValueError(_lib.gpu_only(f"{who} runs") + ": pass the tensor on the device")

    @staticmethod
    def _aligned(t):
        """t, contiguous and on a 16-byte boundary as the library asks (a slice with an odd storage offset takes one copy)"""
        t = t.contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()

    def positions(self, Ht, Wt, V, dev):
        """pos[v][n] = (y, x) of token n, int64 [V, Ht Wt, 2] (dust3r/patch_embed.py:19-29: row-major)"""
        y, x = torch.meshgrid(torch.arange(Ht, device=dev), torch.arange(Wt, device=dev), indexing="ij")
        return torch.stack((y, x), -1).reshape(1, Ht * Wt, 2).expand(V, -1, -1)

    # ------------------------------------------------------------------------------------------------ the stages
    def encode(self, images: torch.Tensor, scratch_budget: int = DEFAULT_SCRATCH_BUDGET):
        """images float32 [V,3,H,W] (H, W multiples of 16, H W / 256 <= 4096 tokens) -> (feat float32 [V, N, enc_dim], pos int64
        [V, N, 2]).  The images go through the library in calls whose scratch stays under `scratch_budget` (at least one image
        per call).  Raises ValueError for anything else."""
        if not isinstance(images, torch.Tensor) or images.dtype != torch.float32 or images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"encode takes a float32 [V,3,H,W] tensor, got "
                             f"{tuple(images.shape) if isinstance(images, torch.Tensor) else type(images)} {getattr(images, 'dtype', '')}")
        self._check_device("Mast3rTrunk.encode", images)
        V, _, H, W = (int(s) for s in images.shape)
        p = self.config.patch
        if V < 1 or H < p or W < p or H % p or W % p or (H // p) * (W // p) > 4096:
            raise ValueError(f"{V} images of {H} x {W}: H and W must be multiples of {p} with at most 4096 patches")
        Ht, Wt = H // p, W // p
        images = self._aligned(images)
        dev = _lib.require_device(images, self.blob)
        cfg = ctypes.byref(self._cfg_c)
        query = lambda v: int(_lib.lib().mi355gs_vit_encode_scratch_bytes(cfg, Ht, Wt, v))
        n = _frames.frames_per_call(lambda v: 0 < query(v) <= scratch_budget, min(V, 256), int(scratch_budget) // max(query(1), 1))
        feat = torch.empty(V, Ht * Wt, self.config.enc_dim, dtype=torch.float32, device=dev)
        scratch = _lib.scratch(dev, "vit_encode_scratch_bytes", cfg, Ht, Wt, n, what=f"mi355gs_vit_encode does not take {n} images of {H} x {W}")
        rope = self._rope_table(Ht, Wt, dev)
        for first in range(0, V, n):
            m = min(n, V - first)
            _lib.call(dev, "vit_encode", _lib.STREAM, cfg, self.blob, rope, Ht, Wt, m, images[first:first + m], scratch, feat[first:first + m])
        return feat, self.positions(Ht, Wt, V, dev)

    def decode(self, feat: torch.Tensor, edges, grid, scratch_budget: int = DEFAULT_SCRATCH_BUDGET):
        """feat float32 [V, N, enc_dim] (encode's), edges: E directed pairs (i, j) (a sequence or an integer tensor [E,2]), grid =
        (Ht, Wt) of the token grid, i.e. (H // 16, W // 16) of the encoded images -> (dec1, dec2): per side the four tensors the heads read —
        [E, N, enc_dim] (the image's encoder rows), then [E, N, dec_dim] after decoder layers hooks[1], hooks[2] and, through
        dec_norm, the last.  E is split into calls whose scratch stays under `scratch_budget` (at least one edge per call)."""
        cfgp = self.config
        if not isinstance(feat, torch.Tensor) or feat.dtype != torch.float32 or feat.dim() != 3 or feat.shape[2] != cfgp.enc_dim:
            raise ValueError(f"decode takes feat float32 [V, N, {cfgp.enc_dim}], got "
                             f"{tuple(feat.shape) if isinstance(feat, torch.Tensor) else type(feat)} {getattr(feat, 'dtype', '')}")
        self._check_device("Mast3rTrunk.decode", feat)
        V, N = int(feat.shape[0]), int(feat.shape[1])
        try:
            Ht, Wt = (int(g) for g in grid)
        except (TypeError, ValueError):
            raise ValueError(f"grid: the token grid (Ht, Wt), got {grid!r}") from None
        if Ht * Wt != N or Ht < 1 or N > 4096 or V < 1 or V > 256:
            raise ValueError(f"feat of {V} x {N} tokens does not fit a grid of {Ht} x {Wt} (at most 4096 tokens, 256 images)")
        e = torch.as_tensor(edges).cpu()
        if e.dim() != 2 or e.shape[1] != 2 or e.shape[0] < 1 or e.is_floating_point() or e.dtype == torch.bool:
            raise ValueError(f"edges: E >= 1 integer pairs [E,2], got {tuple(e.shape)} {e.dtype}")
        if int(e.min()) < 0 or int(e.max()) >= V:
            raise ValueError(f"edges name images outside 0..{V - 1}")
        e = e.to(torch.int32).contiguous()
        E = int(e.shape[0])
        feat = self._aligned(feat)
        dev = _lib.require_device(feat, self.blob)
        cfg = ctypes.byref(self._cfg_c)
        query = lambda k: int(_lib.lib().mi355gs_vit_decode_scratch_bytes(cfg, Ht, Wt, k))
        n = _frames.frames_per_call(lambda k: 0 < query(k) <= scratch_budget, min(E, 65535), int(scratch_budget) // max(query(1), 1))
        scratch = _lib.scratch(dev, "vit_decode_scratch_bytes", cfg, Ht, Wt, n, what=f"mi355gs_vit_decode does not take {n} edges of {N} tokens")
        rope = self._rope_table(Ht, Wt, dev)
        widths = (cfgp.enc_dim, cfgp.dec_dim, cfgp.dec_dim, cfgp.dec_dim)
        outs = [[torch.empty(E, N, D, dtype=torch.float32, device=dev) for D in widths] for _ in range(2)]
        for first in range(0, E, n):
            m = min(n, E - first)
            ptrs = [(ctypes.c_void_p * 4)(*[t[first:first + m].data_ptr() for t in side]) for side in outs]
            # e is pageable host memory and stays alive until this method returns: the library's copy of a call's edges has left
            # it when the call returns (include/mi355gs.h)
            _lib.call(dev, "vit_decode", _lib.STREAM, cfg, self.blob, rope, Ht, Wt, V, m, e[first:first + m], feat, scratch, ptrs[0], ptrs[1])
        return tuple(outs[0]), tuple(outs[1])

    def forward_pairs(self, images: torch.Tensor, edges=None, scratch_budget: int = DEFAULT_SCRATCH_BUDGET):
        """encode + decode.  edges=None: the complete symmetrized graph in `make_pairs`' order (dust3r/image_pairs.py:13-16, 58-59):
        (i, j) for i in range(V) for j in range(i), then every pair reversed.  -> (feat, pos, dec1, dec2, edges int64 [E,2])"""
        feat, pos = self.encode(images, scratch_budget)
        if edges is None:
            edges = complete_edges(int(images.shape[0]))
        Ht, Wt = int(images.shape[2]) // self.config.patch, int(images.shape[3]) // self.config.patch
        dec1, dec2 = self.decode(feat, edges, (Ht, Wt), scratch_budget)
        return feat, pos, dec1, dec2, torch.as_tensor(edges).to(torch.int64).cpu()


def complete_edges(V: int) -> torch.Tensor:
    """make_pairs(scene_graph='complete', symmetrize=True) as index pairs, int64 [V (V - 1), 2]; one image: the pair (0, 0)"""
    half = [(i, j) for i in range(V) for j in range(i)]
    if not half:
        return torch.zeros(1, 2, dtype=torch.int64)
    return torch.tensor(half + [(j, i) for i, j in half], dtype=torch.int64)
