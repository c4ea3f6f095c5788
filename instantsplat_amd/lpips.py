"""LPIPS with the VGG16 trunk on the device — reference lpipsPyTorch/modules/{lpips,networks,utils}.py as metrics.py:69 calls it
(`lpips(render, gt, net_type='vgg')`), behind one library call per chunk of pairs (csrc/lpips.hip, include/mi355gs.h
mi355gs_lpips_vgg_rgb8) on the interleaved bytes the evaluation stage already holds.

The arithmetic is built and pinned here (tests/lpips_util.py: a float64 restatement, the reference's own classes on a thin net);
the TRAINED weights are not part of this package and cannot be fetched offline, so no test pins a real LPIPS value.  A user
supplies the two files the reference downloads: torchvision's `vgg16` ImageNet state dict and the `vgg.pth` lin layers of
richzhang/PerceptualSimilarity v0.1 — `LpipsVGG.from_files(vgg_path, lin_path)`.
"""
from __future__ import annotations

import ctypes
import re

import numpy as np
import torch

from . import _frames, _lib

CONV_LAYERS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # torchvision vgg16().features indices of the convolutions
BLOCK_CONVS = (2, 2, 3, 3, 3)
DEFAULT_SCRATCH_BUDGET = 4 << 30


def _conv_tensors(vgg_state):
    """[(weight [Cout,Cin,3,3], bias [Cout])] x 13 from `features.N.weight` / `N.weight` keys"""
    found = {}
    for key, val in vgg_state.items():
        m = re.fullmatch(r"(?:features\.)?(\d+)\.(weight|bias)", key)
        if m and int(m.group(1)) in CONV_LAYERS:
            found[(int(m.group(1)), m.group(2))] = val
    out = []
    for n in CONV_LAYERS:
        if (n, "weight") not in found or (n, "bias") not in found:
            raise ValueError(f"VGG16 state dict lacks features.{n}.weight / .bias")
        out.append((found[(n, "weight")], found[(n, "bias")]))
    return out


def _lin_tensors(lin_state):
    """[lin weight [C]] x 5 from `lin{i}.model.1.weight` (the official file) or `{i}.1.weight` (the reference's renaming)"""
    found = {}
    for key, val in lin_state.items():
        m = re.fullmatch(r"(?:lin)?(\d)\.(?:model\.)?1\.weight", key)
        if m:
            found[int(m.group(1))] = val
    if sorted(found) != [0, 1, 2, 3, 4]:
        raise ValueError(f"lin state dict needs lin0..lin4 (.model.1.weight), found {sorted(lin_state)}")
    return [found[i] for i in range(5)]


class LpipsVGG:
    """The packed network.  vgg_state: torchvision's VGG16 state dict (`features.N.weight` or bare `N.weight`); lin_state: the
    five 1x1 lin layers.  The block widths are read off the tensors (the trained net: 64, 128, 256, 512, 512; every multiple of
    32 up to 512 is taken).  The blob mi355gs_lpips_vgg_rgb8 reads is packed once, here, with torch ops.
    Raises ValueError for missing keys, shapes that are not a VGG16 trunk, or unsupported widths."""

    def __init__(self, vgg_state, lin_state, device=None):
        convs, lins = _conv_tensors(vgg_state), _lin_tensors(lin_state)
        parts, channels, cin, i = [], [], 3, 0
        for blk, count in enumerate(BLOCK_CONVS):
            width = int(convs[i][0].shape[0]) if convs[i][0].dim() == 4 else -1
            if width < 32 or width > 512 or width % 32:
                raise ValueError(f"block {blk + 1}: width {width}; the kernels take multiples of 32 from 32 to 512")
            for _ in range(count):
                w, b = convs[i]
                if tuple(w.shape) != (width, cin, 3, 3) or tuple(b.shape) != (width,):
                    raise ValueError(f"convolution features.{CONV_LAYERS[i]}: weight {tuple(w.shape)}, bias {tuple(b.shape)}; "
                                     f"expected ({width}, {cin}, 3, 3) and ({width},)")
                parts += [w.detach().to("cpu", torch.float32).permute(2, 3, 1, 0).reshape(-1), b.detach().to("cpu", torch.float32).reshape(-1)]
                cin, i = width, i + 1
            channels.append(width)
        for blk, lw in enumerate(lins):
            if lw.numel() != channels[blk]:
                raise ValueError(f"lin{blk}: {lw.numel()} weights for {channels[blk]} channels")
            parts.append(lw.detach().to("cpu", torch.float32).reshape(-1))
        self.channels = tuple(channels)
        self._channels_c = (ctypes.c_int * 5)(*channels)
        blob = torch.cat(parts).contiguous()
        self.blob = blob.to(_frames.device_of((), default=device))

    @classmethod
    def from_files(cls, vgg_path, lin_path, device=None):
        return cls(torch.load(vgg_path, map_location="cpu", weights_only=True), torch.load(lin_path, map_location="cpu", weights_only=True),
                   device=device)

    def _scratch_bytes(self, n, H, W):
        return int(_lib.lib().mi355gs_lpips_vgg_scratch_bytes(n, H, W, self._channels_c))

    def lpips_rgb8(self, renders: torch.Tensor, gts: torch.Tensor, scratch_budget: int = DEFAULT_SCRATCH_BUDGET) -> dict:
        """LPIPS of N pairs of 8-bit frames, uint8 [N,H,W,3] each (device, pinned or host memory; the rules of
        `metrics.image_metrics_rgb8`).  The pairs go through the library in chunks whose scratch (two float32 activation buffers
        of 2 n H W x the widest block) stays under `scratch_budget` bytes — at least one pair per call — and both results come
        back in ONE read-back.  -> dict of host arrays: lpips float32 [N], taps float32 [N,5] (the five layers' terms).
        Raises ValueError for anything but two uint8 [N,H,W,3] tensors of one shape with H, W >= 16."""
        N, H, W = _frames.check_pair("lpips_rgb8", renders, gts)
        if N == 0:
            return dict(lpips=np.zeros(0, np.float32), taps=np.zeros((0, 5), np.float32))
        if H < 16 or W < 16:
            raise ValueError(f"frames of {H} x {W}: the fifth block needs at least 16 x 16")
        a, b, dev = _frames.pair_on_device(renders, gts, self.blob, default=self.blob.device if self.blob.is_cuda else None)
        if not self._scratch_bytes(1, H, W):
            raise ValueError(f"mi355gs_lpips_vgg_rgb8 does not take frames of {H} x {W} (include/mi355gs.h: the limits)")
        n = _frames.frames_per_call(lambda n: 0 < self._scratch_bytes(n, H, W) <= scratch_budget, N,
                                    int(scratch_budget) // self._scratch_bytes(1, H, W))
        out = torch.empty(6 * N, dtype=torch.float32, device=dev)   # lpips [N] then taps [N][5]: one block, one read-back
        scratch = _lib.scratch(dev, "lpips_vgg_scratch_bytes", n, H, W, self._channels_c, what=None)
        for first in range(0, N, n):
            m = min(n, N - first)
            _lib.call(dev, "lpips_vgg_rgb8", _lib.STREAM, m, H, W, a[first:first + m], b[first:first + m], self._channels_c, self.blob, scratch,
                      out.data_ptr() + 4 * first, out.data_ptr() + 4 * (N + 5 * first))
        host = out.cpu().numpy()   # the one read-back (it also orders the launches before the scratch block is released)
        return dict(lpips=host[:N].copy(), taps=host[N:].reshape(N, 5).copy())
