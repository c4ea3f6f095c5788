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

from . import _frames, _lib

MAX_FRAMES_PER_CALL = 65535   # include/mi355gs.h: N of one mi355gs_png_rgb8 call (a grid dimension)


def encode_png_rgb8(frames: torch.Tensor, rows_per_block: int | None = None, max_call_bytes: int = 1 << 30) -> dict:
    """frames: contiguous uint8 [N,H,W,3] (or [H,W,3]) on the device -> dict(stream: uint8 host tensor holding the N files back to
    back, offsets: int64 [N+1] numpy array; file i is stream[offsets[i]:offsets[i+1]]).

    rows_per_block: filtered rows per deflate block (None: the largest with rows x (3 W + 1) <= 65536).  N is split into library
    calls whose scratch and output buffers together stay under max_call_bytes (one frame per call at least); per call `offsets`
    is read back once and only the used prefix of the output is copied to the host.
    Raises ValueError for anything but a contiguous uint8 device tensor of that shape, or sizes beyond the library's limits."""
    frames, N, H, W = _frames.check_frames("encode_png_rgb8", frames)
    R = 0 if rows_per_block is None else int(rows_per_block)
    if rows_per_block is not None and R < 1:
        raise ValueError(f"rows_per_block must be at least 1, got {rows_per_block}")
    if N == 0:
        return dict(stream=torch.empty(0, dtype=torch.uint8), offsets=np.zeros(1, np.int64))
    L = _lib.lib()
    sizes = lambda n: (int(L.mi355gs_png_rgb8_scratch_bytes(n, H, W, R)), int(L.mi355gs_png_rgb8_stream_bytes(n, H, W, R)))
    scratch1, stream1 = sizes(1)
    if not scratch1:
        raise ValueError(f"mi355gs_png_rgb8 does not take frames of {H} x {W} with rows_per_block = {rows_per_block} "
                         "(include/mi355gs.h: the limits)")
    per_call = _frames.frames_per_call(lambda n: sum(sizes(n)) + 8 * (n + 1) <= max_call_bytes, min(MAX_FRAMES_PER_CALL, N),
                                       int(max_call_bytes) // (scratch1 + stream1 + 8))
    dev = frames.device
    frame_bytes = 3 * H * W

    def buffers(n):
        scratch = _lib.scratch(dev, "png_rgb8_scratch_bytes", n, H, W, R,
                               what=f"mi355gs_png_rgb8 does not take {n} frames of {H} x {W} (include/mi355gs.h: the limits)")
        return (scratch, torch.empty(sizes(n)[1], dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev))

    def encode_call(first, n, scratch, out, offs):
        _lib.call(dev, "png_rgb8", _lib.STREAM, n, H, W, R, frames.data_ptr() + first * frame_bytes, scratch, out, offs)
        o = offs.cpu().numpy()   # the call's one read-back; the copy below takes only the bytes the files have
        return o, [_frames.host_bytes(out, int(o[-1]))]

    return _frames.encode_in_calls(N, per_call, buffers, encode_call)


def write_png_files(paths: Sequence[str], frames: torch.Tensor, **kw) -> None:
    """Encode frames (as `encode_png_rgb8` takes them) and write file i to paths[i] with one write each."""
    _frames.write_stream_files(paths, frames, encode_png_rgb8, **kw)
