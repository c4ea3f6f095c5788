"""Motion-JPEG video in an AVI container: host framing around complete JPEG files (instantsplat_amd/jpeg.py encodes them on the
device).  Every frame is a key frame; the container is a few hundred bytes of headers and a 16-byte index entry per frame."""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
MAX_FILE_BYTES = (1 << 31) - 1   # plain AVI (no OpenDML): sizes and index offsets of 2 GiB and more are refused


def _chunk(fourcc: bytes, body: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _list(kind: bytes, body: bytes) -> bytes:
    return b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body


def write_mjpeg_avi(path, stream, offsets, W: int, H: int, fps=30) -> None:
    """stream: the N JPEG files back to back (a uint8 tensor or array, or bytes), offsets: [N+1] with file i at
    stream[offsets[i]:offsets[i+1]] — what `encode_jpeg_rgb8` returns; W, H: the frames' size.  Writes RIFF 'AVI ' with
    LIST hdrl (avih; LIST strl: strh vids/MJPG, strf BITMAPINFOHEADER), LIST movi (one '00dc' chunk per frame, padded to an even
    length) and idx1 (offsets counted from the 'movi' fourcc).  fps: the rate as scale / rate of `Fraction(fps)` (1 / fps for an
    integer).  ValueError for inconsistent offsets, non-positive sizes or rate, and for a file of 2 GiB or more."""
    offsets = [int(o) for o in np.asarray(offsets).reshape(-1)]
    N = len(offsets) - 1
    total = len(stream) if isinstance(stream, (bytes, bytearray, memoryview)) else int(np.prod(tuple(stream.shape)))
    if N < 1 or offsets[0] != 0 or any(b <= a for a, b in zip(offsets, offsets[1:])) or offsets[-1] > total:
        raise ValueError(f"offsets must start at 0 and increase within the stream's {total} bytes, with one file at least")
    if int(W) <= 0 or int(H) <= 0 or int(W) > 65535 or int(H) > 65535:
        raise ValueError(f"bad frame size {W} x {H}")
    if not fps > 0:
        raise ValueError(f"fps must be positive, got {fps!r}")
    sizes = [b - a for a, b in zip(offsets, offsets[1:])]
    movi_bytes = 4 + sum(8 + s + (s & 1) for s in sizes)
    header_bytes = 12 + (12 + (8 + 56) + 12 + (8 + 56) + (8 + 40))
    if header_bytes + 8 + movi_bytes + 8 + 16 * N > MAX_FILE_BYTES:
        raise ValueError("the AVI file would reach 2 GiB (OpenDML is not written): encode fewer frames or a lower quality")
    data = stream if isinstance(stream, (bytes, bytearray, memoryview)) else memoryview(np.ascontiguousarray(np.asarray(stream)).reshape(-1))
    rate = Fraction(fps).limit_denominator(1 << 20)
    largest = max(sizes)
    avih = struct.pack("<14I", round(1e6 / fps), 0, 0, AVIF_HASINDEX, N, 0, 1, largest, W, H, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IIIIIIIIiI", 0, 0, 0, rate.denominator, rate.numerator, 0, N, largest, -1, 0) + struct.pack("<4h", 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", 3 * W * H, 0, 0, 0, 0)
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf)))
    assert len(hdrl) == header_bytes - 12
    index, at = [], 4
    for s in sizes:
        index.append(b"00dc" + struct.pack("<3I", AVIIF_KEYFRAME, at, s))
        at += 8 + s + (s & 1)
    idx1 = _chunk(b"idx1", b"".join(index))
    riff_bytes = 4 + len(hdrl) + 8 + movi_bytes + len(idx1)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_bytes) + b"movi")
        for a, s in zip(offsets, sizes):
            fh.write(b"00dc" + struct.pack("<I", s))
            fh.write(data[a:a + s])
            if s & 1:
                fh.write(b"\0")
        fh.write(idx1)
