"""PNG files of 8-bit frames, encoded on the device (csrc/png.hip, include/mi355gs.h mi355gs_png_rgb8).

The frames `render_pose_path` / `quantize_rgb8` leave in device memory are interleaved [H,W,3] bytes — a PNG scanline's layout.
`encode_png_rgb8` turns a stack of them into complete PNG files with three kernel launches per call (Paeth filter, an optimal
length-limited Huffman code per block of rows, Adler-32, CRC-32, chunk framing) and copies only the files' bytes to the host;
`write_png_files` writes each with one `open(...).write`.

What it leaves out is LZ77 matching, the part of deflate that does not parallelise: the files are those of zlib's Z_HUFFMAN_ONLY
strategy, 10-18 % larger than PIL's on photographic content, and never smaller than one bit per byte — a constant-colour frame
comes to 1/8 of its raw size where PIL's file is tiny.  Every PNG reader decodes them to the identical pixels."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _lib

MAX_FRAMES_PER_CALL = 65535   # include/mi355gs.h: N of one mi355gs_png_rgb8 call (a grid dimension)


def _call_sizes(L, n, H, W, R):
    return int(L.mi355gs_png_rgb8_scratch_bytes(n, H, W, R)), int(L.mi355gs_png_rgb8_stream_bytes(n, H, W, R))


def encode_png_rgb8(frames: torch.Tensor, rows_per_block: int | None = None, max_call_bytes: int = 1 << 30) -> dict:
    """frames: contiguous uint8 [N,H,W,3] (or [H,W,3]) on the device -> dict(stream: uint8 host tensor holding the N files back to
    back, offsets: int64 [N+1] numpy array; file i is stream[offsets[i]:offsets[i+1]]).

    rows_per_block: filtered rows per deflate block (None: the largest with rows x (3 W + 1) <= 65536).  N is split into library
    calls whose scratch and output buffers together stay under max_call_bytes (one frame per call at least); per call `offsets`
    is read back once and only the used prefix of the output is copied to the host.
    Raises ValueError for anything but a contiguous uint8 device tensor of that shape, or sizes beyond the library's limits."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError("encode_png_rgb8 takes a uint8 [N,H,W,3] or [H,W,3] tensor, got "
                         f"{tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames)} {getattr(frames, 'dtype', '')}")
    if not frames.is_cuda and not _lib._TEST_MODE:
        raise ValueError("encode_png_rgb8 encodes on the GPU only (got a CPU tensor; there is no CPU fallback): pass frames.to(device)")
    if not frames.is_contiguous():
        raise ValueError("encode_png_rgb8 takes a contiguous tensor")
    if frames.dim() == 3:
        frames = frames[None]
    N, H, W = (int(s) for s in frames.shape[:3])
    if H <= 0 or W <= 0:
        raise ValueError(f"empty frames: {H} x {W}")
    R = 0 if rows_per_block is None else int(rows_per_block)
    if rows_per_block is not None and R < 1:
        raise ValueError(f"rows_per_block must be at least 1, got {rows_per_block}")
    if N == 0:
        return dict(stream=torch.empty(0, dtype=torch.uint8), offsets=np.zeros(1, np.int64))
    L = _lib.lib()
    scratch1, stream1 = _call_sizes(L, 1, H, W, R)
    if not scratch1:
        raise ValueError(f"mi355gs_png_rgb8 does not take frames of {H} x {W} with rows_per_block = {rows_per_block} "
                         "(include/mi355gs.h: the limits)")
    fits = lambda n: sum(_call_sizes(L, n, H, W, R)) + 8 * (n + 1) <= max_call_bytes
    cap = min(MAX_FRAMES_PER_CALL, N)
    per_call = max(1, min(cap, int(max_call_bytes) // (scratch1 + stream1 + 8)))   # an estimate: the buffers are padded
    while per_call > 1 and not fits(per_call):
        per_call -= 1
    while per_call < cap and fits(per_call + 1):
        per_call += 1
    dev = frames.device
    frame_bytes = 3 * H * W
    parts, offsets, base = [], [np.zeros(1, np.int64)], 0
    with _lib.on_device(dev):
        scratch = out = offs = None
        for first in range(0, N, per_call):
            n = min(per_call, N - first)
            if scratch is None or n != per_call:
                nscratch, nstream = _call_sizes(L, n, H, W, R)
                if not nscratch:
                    raise ValueError(f"mi355gs_png_rgb8 does not take {n} frames of {H} x {W} (include/mi355gs.h: the limits)")
                scratch = torch.empty(nscratch, dtype=torch.uint8, device=dev)
                out = torch.empty(nstream, dtype=torch.uint8, device=dev)
                offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
            _lib.check(L.mi355gs_png_rgb8(_lib.stream_ptr(dev), n, H, W, R, frames.data_ptr() + first * frame_bytes, _lib.ptr(scratch),
                                          _lib.ptr(out), _lib.ptr(offs)), "png_rgb8")
            o = offs.cpu().numpy()   # the call's one read-back; the copy below takes only the bytes the files have
            files = out[:int(o[-1])].cpu()
            parts.append(files if out.is_cuda else files.clone())   # (the buffers are reused by the next call)
            offsets.append(o[1:] + base)
            base += int(o[-1])
    return dict(stream=parts[0] if len(parts) == 1 else torch.cat(parts), offsets=np.concatenate(offsets))


def write_png_files(paths: Sequence[str], frames: torch.Tensor, **kw) -> None:
    """Encode frames (as `encode_png_rgb8` takes them) and write file i to paths[i] with one write each."""
    paths = list(paths)
    n = 1 if isinstance(frames, torch.Tensor) and frames.dim() == 3 else len(frames)
    if len(paths) != n:
        raise ValueError(f"{len(paths)} paths for {n} frames")
    enc = encode_png_rgb8(frames, **kw)
    data, offsets = memoryview(enc["stream"].numpy()), enc["offsets"]
    for i, path in enumerate(paths):
        with open(path, "wb") as fh:
            fh.write(data[int(offsets[i]):int(offsets[i + 1])])
