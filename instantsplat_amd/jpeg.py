"""Baseline JPEG files of 8-bit frames, encoded on the device (csrc/jpeg.hip, include/mi355gs.h mi355gs_jpeg_rgb8).

`encode_jpeg_rgb8` turns the interleaved [H,W,3] frames `render_pose_path` / `quantize_rgb8` leave in device memory into complete
JPEG files with three kernel launches per call: libjpeg's integer colour conversion, 4:2:0 or 4:4:4, the `islow` DCT, the
standard's typical Huffman tables and one restart interval per MCU row.  The files equal, byte for byte, what PIL (libjpeg-turbo)
writes with `quality=q, subsampling=0|2, optimize=False, restart_marker_rows=1`.  They are the frames of the Motion-JPEG video
`instantsplat_amd.video.write_mjpeg_avi` frames on the host."""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from . import _frames, _lib

MAX_FRAMES_PER_CALL = 65535   # include/mi355gs.h: N of one mi355gs_jpeg_rgb8 call (a grid dimension)
HEADER_BYTES = 1024           # room per file for its 629 bytes of header, the restart markers and EOI in the default capacity
SUBSAMPLINGS = {"4:4:4": 0, "4:2:0": 2}

# JPEG standard, Annex K.1 and K.2: the example quantisation tables, natural order
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def quant_tables(quality) -> np.ndarray:
    """libjpeg's `jpeg_set_quality`: quality (clamped to 1..100) -> uint8 [2,64], luma and chroma, natural order."""
    if isinstance(quality, bool) or not isinstance(quality, (int, float, np.integer, np.floating)) or not math.isfinite(quality):
        raise ValueError(f"quality must be a number, got {quality!r}")
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([_BASE_LUMA, _BASE_CHROMA], np.int64)
    return np.clip((base * s + 50) // 100, 1, 255).astype(np.uint8)


def encode_jpeg_rgb8(frames: torch.Tensor, quality=90, subsampling: str = "4:2:0", qtables=None, capacity: int | None = None,
                     max_call_bytes: int = 1 << 30) -> dict:
    """frames: contiguous uint8 [N,H,W,3] (or [H,W,3]) on the device -> dict(stream: uint8 host tensor holding the N files back to
    back, offsets: int64 [N+1] numpy array; file i is stream[offsets[i]:offsets[i+1]]).

    quality: libjpeg's 1..100 (`quant_tables`); qtables: uint8 [2,64] in natural order, entries 1..255, instead of a quality.
    subsampling: "4:2:0" or "4:4:4".
    capacity: bytes of the output buffer of one library call.  None: half the call's raw bytes plus HEADER_BYTES per frame — rendered
    frames at quality 90 come to a tenth of raw or less, so the buffer and its copy stay small, while the library's worst case is
    above four times raw.  The library reports every file's exact size whatever the capacity; the frames of a call whose files
    did not fit are encoded once more into a buffer of exactly their size, so the result never misses a file.
    N is split into library calls whose scratch and output buffers together stay under max_call_bytes (one frame per call at
    least); per call `offsets` is read back once and only the files' bytes are copied to the host.
    Raises ValueError for anything but a contiguous uint8 device tensor of that shape, or sizes beyond the library's limits."""
    frames, N, H, W = _frames.check_frames("encode_jpeg_rgb8", frames)
    if not isinstance(subsampling, str) or subsampling not in SUBSAMPLINGS:
        raise ValueError(f'subsampling must be "4:2:0" or "4:4:4", got {subsampling!r}')
    sub = SUBSAMPLINGS[subsampling]
    if qtables is None:
        qt = quant_tables(quality)
    else:
        qt = np.asarray(qtables)
        if qt.shape != (2, 64) or qt.dtype.kind not in "iu" or qt.min() < 1 or qt.max() > 255:
            raise ValueError("qtables must be integers 1..255 of shape [2,64] (luma, chroma; natural order)")
    qt = np.ascontiguousarray(qt, dtype=np.uint8)
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0):
        raise ValueError(f"capacity must be a non-negative integer or None, got {capacity!r}")
    if N == 0:
        return dict(stream=torch.empty(0, dtype=torch.uint8), offsets=np.zeros(1, np.int64))
    L = _lib.lib()
    scratch_bytes = lambda n: int(L.mi355gs_jpeg_rgb8_scratch_bytes(n, H, W, sub))
    stream_bytes = lambda n: int(L.mi355gs_jpeg_rgb8_stream_bytes(n, H, W, sub))
    if not scratch_bytes(1):
        raise ValueError(f"mi355gs_jpeg_rgb8 does not take frames of {H} x {W} (include/mi355gs.h: the limits)")
    frame_bytes = 3 * H * W
    room = lambda n: min(n * (frame_bytes // 2 + HEADER_BYTES), stream_bytes(n)) if capacity is None else int(capacity)
    per_call = _frames.frames_per_call(lambda n: scratch_bytes(n) + room(n) + 8 * (n + 1) <= max_call_bytes, min(MAX_FRAMES_PER_CALL, N),
                                       int(max_call_bytes) // (scratch_bytes(1) + room(1) + 8))
    dev = frames.device

    def call(first, n, scratch, out, out_bytes, offs):
        _lib.call(dev, "jpeg_rgb8", _lib.STREAM, n, H, W, sub, qt.ctypes.data, frames.data_ptr() + first * frame_bytes, scratch, out, out_bytes,
                  offs)
        return offs.cpu().numpy().copy()   # the call's one read-back; the copies below take only the bytes the files have

    def buffers(n):
        scratch = _lib.scratch(dev, "jpeg_rgb8_scratch_bytes", n, H, W, sub,
                               what=f"mi355gs_jpeg_rgb8 does not take {n} frames of {H} x {W} (include/mi355gs.h: the limits)")
        out_bytes = room(n)
        return (scratch, torch.empty(max(out_bytes, 1), dtype=torch.uint8, device=dev),   # (an empty tensor has no address)
                out_bytes, torch.empty(n + 1, dtype=torch.int64, device=dev))

    def encode_call(first, n, scratch, out, out_bytes, offs):
        o = call(first, n, scratch, out, out_bytes, offs)
        done = int(np.searchsorted(o, out_bytes, side="right")) - 1   # files 0 .. done-1 fitted: offsets[i+1] <= capacity
        files = [_frames.host_bytes(out, int(o[done]))]
        if done < n:   # the rest once more, into exactly their bytes
            rest = torch.empty(int(o[n] - o[done]), dtype=torch.uint8, device=dev)
            o2 = call(first + done, n - done, scratch, rest, rest.numel(), offs[:n - done + 1])
            if int(o2[-1]) != rest.numel():
                raise RuntimeError("mi355gs_jpeg_rgb8 reported different sizes for the same frames")
            files.append(rest.cpu())
        return o, files

    return _frames.encode_in_calls(N, per_call, buffers, encode_call)


def write_jpeg_files(paths: Sequence[str], frames: torch.Tensor, **kw) -> None:
    """Encode frames (as `encode_jpeg_rgb8` takes them) and write file i to paths[i] with one write each."""
    _frames.write_stream_files(paths, frames, encode_jpeg_rgb8, **kw)
