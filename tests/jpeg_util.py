"""Checks of the device JPEG encoder and the MJPEG container (instantsplat_amd/jpeg.py, instantsplat_amd/video.py, csrc/jpeg.hip,
include/mi355gs.h mi355gs_jpeg_rgb8), shared by the emulated (CPU) and the GPU test files.

Yardsticks: PIL (libjpeg-turbo) writing the same stream structure — `quality=q, subsampling=0|2, optimize=False,
restart_marker_rows=1` — and a numpy restatement of libjpeg's integer arithmetic (`encode`), which `check_restatement` holds to
PIL's whole files.  The device is held to both, byte for byte; nothing here has a tolerance."""
import ctypes
import io
import os
import struct

import numpy as np
import pytest
import torch
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1
GUARD = 256
SHAPES = [(1, 1), (1, 9), (7, 9), (8, 8), (9, 8), (8, 40), (16, 16), (17, 16), (16, 17), (24, 40), (40, 48), (33, 17), (31, 31),
          (10, 70), (150, 24), (9, 4096)]   # H, W
QUALITIES = (1, 30, 49, 50, 75, 90, 95, 100)
SUBSAMPLINGS = ("4:4:4", "4:2:0")

# ---------------------------------------------------------------------------------------------------- tables of the standard
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32)
# Annex K.3: (class << 4 | id, the 16 counts per code length, the values)
DHT = [
    (0x00, [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0x10, [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
     [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98,
      114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86,
      87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138,
      146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
      194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233,
      234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250]),
    (0x01, [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (0x11, [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
     [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114,
      209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84,
      85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135,
      136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183,
      184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231,
      232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250]),
]


def huffman_codes(bits, vals):
    """-> (code[256], length[256]) of the canonical code (JPEG Annex C)"""
    code, length, c, k = np.zeros(256, np.int64), np.zeros(256, np.int64), 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            code[vals[k]], length[vals[k]] = c, l
            c, k = c + 1, k + 1
        c <<= 1
    return code, length


_CODES = {tid: huffman_codes(bits, vals) for tid, bits, vals in DHT}


def quant_tables(quality) -> np.ndarray:
    """the restatement's own: libjpeg's jpeg_set_quality -> uint8 [2,64], natural order"""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * s + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA)]).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- host restatement
def _pad_edge(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def _up(n, m):
    return (n + m - 1) // m * m


def planes(frame: np.ndarray, sub: int):
    """uint8 [H,W,3] -> the three component planes, padded to whole blocks as libjpeg pads them"""
    H, W = frame.shape[:2]
    r, g, b = (frame[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    if sub == 0:
        return [_pad_edge(p, _up(H, 8), _up(W, 8)) for p in (y, cb, cr)]
    out = [_pad_edge(y, _up(H, 8), _up(W, 8))]
    for p in (cb, cr):
        p = _pad_edge(p, _up(H, 2), _up(W, 16))
        bias = np.tile(np.array([1, 2]), p.shape[1] // 4)[None]
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(_pad_edge(d, _up(d.shape[0], 8), d.shape[1]))   # the DOWNSAMPLED plane is padded at the bottom
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first):
    """libjpeg jfdctint.c (islow) along the last axis; first: pass 1 (results scaled up by 4), else pass 2"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z = (t12 + t13) * 4433
    o[2] = _descale(z + t13 * 6270, n)
    o[6] = _descale(z - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def quantised_blocks(plane: np.ndarray, q: np.ndarray) -> np.ndarray:
    """padded plane -> int64 [rows of blocks, blocks per row, 64] quantised coefficients in zigzag order"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
    c = _dct_pass(blk, True)                                      # rows
    c = _dct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)     # columns
    assert np.abs(c).max(initial=0) < 1 << 31
    q8 = q.astype(np.int64).reshape(8, 8) << 3
    v = np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8)
    return v.reshape(bh, bw, 64)[..., ZIGZAG]


def mcu_rows(frame: np.ndarray, qt: np.ndarray, sub: int):
    """-> per MCU row: (int64 [blocks, 64] in coding order with the true DC, component of every block)"""
    H, W = frame.shape[:2]
    p = planes(frame, sub)
    Y, Cb, Cr = quantised_blocks(p[0], qt[0]), quantised_blocks(p[1], qt[1]), quantised_blocks(p[2], qt[1])
    if sub == 0:
        return [(np.stack([Y[r], Cb[r], Cr[r]], axis=1).reshape(-1, 64), np.tile([0, 1, 2], Y.shape[1])) for r in range(Y.shape[0])]
    rows = []
    nmr, nmc = (H + 15) // 16, (W + 15) // 16
    for r in range(nmr):
        blocks = []
        for m in range(nmc):
            for j in range(4):
                by, bx = 2 * r + (j >> 1), 2 * m + (j & 1)
                if by < Y.shape[0] and bx < Y.shape[1]:
                    blocks.append(Y[by, bx])
                else:   # a dummy block: no AC, the DC of the block coded just before it
                    d = np.zeros(64, np.int64)
                    d[0] = blocks[-1][0]
                    blocks.append(d)
            blocks += [Cb[r, m], Cr[r, m]]
        rows.append((np.stack(blocks), np.tile([0, 0, 0, 0, 1, 2], nmc)))
    return rows


def _bit_length(a):
    a = np.abs(a)
    n = np.zeros(a.shape, np.int64)
    for k in range(12):
        n += a >= (1 << k)
    return n


def interval_bytes(blocks: np.ndarray, comp: np.ndarray) -> bytes:
    """one restart interval: predictors from 0, Huffman codes, 1-bits to the byte, a zero behind every FF"""
    nb = blocks.shape[0]
    z = blocks.copy()
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        z[idx[1:], 0] = blocks[idx[1:], 0] - blocks[idx[:-1], 0]
    chroma = comp > 0
    # tokens as (block, order inside the block, value, bits); DC first
    cat = _bit_length(z[:, 0])
    dc_code = np.where(chroma, _CODES[0x01][0][cat], _CODES[0x00][0][cat])
    dc_len = np.where(chroma, _CODES[0x01][1][cat], _CODES[0x00][1][cat])
    low = lambda v, n: np.where(v >= 0, v, v - 1) & ((1 << n) - 1)
    tok = [(np.arange(nb), np.zeros(nb, np.int64), (dc_code << cat) | low(z[:, 0], cat), dc_len + cat)]
    b, k = np.nonzero(z[:, 1:])
    k = k + 1
    prev = np.zeros_like(k)
    same = np.zeros(len(k), bool)
    same[1:] = b[1:] == b[:-1]
    prev[1:] = np.where(same[1:], k[:-1], 0)
    run = k - prev - 1
    size = _bit_length(z[b, k])
    sym = ((run & 15) << 4) | size
    ch = chroma[b]
    code = np.where(ch, _CODES[0x11][0][sym], _CODES[0x10][0][sym])
    ln = np.where(ch, _CODES[0x11][1][sym], _CODES[0x10][1][sym])
    assert np.all(ln > 0)
    tok.append((b, 4 * k + 3, (code << size) | low(z[b, k], size), ln + size))
    for i in range(1, 4):   # up to three ZRL codes in front of a coefficient
        m = (run >> 4) >= i
        tok.append((b[m], 4 * k[m] + i - 1, np.where(ch[m], _CODES[0x11][0][0xF0], _CODES[0x10][0][0xF0]), np.where(ch[m], _CODES[0x11][1][0xF0], _CODES[0x10][1][0xF0])))
    last = np.zeros(nb, np.int64)
    np.maximum.at(last, b, k)
    e = np.nonzero(last < 63)[0]
    tok.append((e, np.full(len(e), 4 * 64), np.where(chroma[e], _CODES[0x11][0][0], _CODES[0x10][0][0]), np.where(chroma[e], _CODES[0x11][1][0], _CODES[0x10][1][0])))
    tb, to, tv, tn = (np.concatenate([t[i] for t in tok]) for i in range(4))
    order = np.lexsort((to, tb))
    tv, tn = tv[order], tn[order]
    total = int(tn.sum())
    start = np.cumsum(tn) - tn
    j = np.arange(total) - np.repeat(start, tn)
    bits = ((np.repeat(tv, tn) >> (np.repeat(tn, tn) - 1 - j)) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones(-total % 8, np.uint8)])
    by = np.packbits(bits)
    out = np.repeat(by, 1 + (by == 255))
    out[np.cumsum(1 + (by == 255))[by == 255] - 1] = 0
    return out.tobytes()


def header(H, W, qt: np.ndarray, sub: int) -> bytes:
    seg = lambda m, body: bytes([0xFF, m]) + struct.pack(">H", len(body) + 2) + body
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i in range(2):
        out += seg(0xDB, bytes([i]) + bytes(int(v) for v in qt[i][ZIGZAG]))
    out += seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22 if sub else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tid, bits, vals in DHT:
        out += seg(0xC4, bytes([tid] + bits + vals))
    out += seg(0xDD, struct.pack(">H", (W + 15) // 16 if sub else (W + 7) // 8))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def sub_code(subsampling) -> int:
    return {"4:4:4": 0, "4:2:0": 2}[subsampling]


def encode(frame: np.ndarray, quality=90, subsampling="4:2:0", qtables=None) -> bytes:
    """the whole file, from numpy integer arithmetic"""
    sub = sub_code(subsampling)
    qt = quant_tables(quality) if qtables is None else np.asarray(qtables)
    H, W = frame.shape[:2]
    out = [header(H, W, qt, sub)]
    for r, (blocks, comp) in enumerate(mcu_rows(frame, qt, sub)):
        if r:
            out.append(bytes([0xFF, 0xD0 + ((r - 1) & 7)]))
        out.append(interval_bytes(blocks, comp))
    return b"".join(out) + b"\xff\xd9"


def pil_encode(frame: np.ndarray, quality=90, subsampling="4:2:0", qtables=None) -> bytes:
    b = io.BytesIO()
    kw = dict(quality=quality) if qtables is None else dict(qtables=[[int(v) for v in t[ZIGZAG]] for t in np.asarray(qtables)])
    Image.fromarray(frame).save(b, "JPEG", subsampling=sub_code(subsampling), optimize=False, restart_marker_rows=1, **kw)
    return b.getvalue()


def segments(data: bytes):
    """the marker segments in front of the scan -> [(marker, body)]"""
    assert data[:2] == b"\xff\xd8"
    pos, out = 2, []
    while True:
        assert data[pos] == 0xFF
        n, = struct.unpack(">H", data[pos + 2:pos + 4])
        out.append((data[pos + 1], data[pos + 4:pos + 2 + n]))
        pos += 2 + n
        if out[-1][0] == 0xDA:
            return out, pos


def decode(data: bytes) -> np.ndarray:
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.format == "JPEG" and im.mode == "RGB"
    return np.asarray(im)


# ---------------------------------------------------------------------------------------------------- contents
def art_frames():
    names = sorted(n for n in os.listdir(os.path.join(GOLDEN, "sora_art")) if n.startswith("art_frame_") and n.endswith(".jpg"))
    return np.stack([np.asarray(Image.open(os.path.join(GOLDEN, "sora_art", n)).convert("RGB")) for n in names])


_ART = []


def contents(H, W):
    """-> {name: uint8 [H,W,3]}; the same arrays at every call"""
    rng = np.random.default_rng(1000 * H + W)
    if not _ART:
        _ART.append(art_frames()[0])
    art = _ART[0]
    y0, x0 = (37 * H) % (art.shape[0] - min(H, art.shape[0]) + 1), (53 * W) % (art.shape[1] - min(W, art.shape[1]) + 1)
    crop = art[y0:y0 + H, x0:x0 + W]
    crop = np.pad(crop, ((0, H - crop.shape[0]), (0, W - crop.shape[1]), (0, 0)), mode="reflect") if crop.shape[:2] != (H, W) else crop
    out = {"noise": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "binary noise": (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)}
    for v in (0, 200, 255):
        out[f"constant {v}"] = np.full((H, W, 3), v, np.uint8)
    out["ramp"] = np.broadcast_to(((np.arange(W) * 3) % 256).astype(np.uint8)[None, :, None] + np.array([0, 40, 90], np.uint8), (H, W, 3)).copy()
    out["art crop"] = np.ascontiguousarray(crop)
    return out


def scan_of(data: bytes) -> bytes:
    return data[segments(data)[1]:-2]


def assert_hard_cases(H, W, sub, q, files: dict):
    """Conditions on the restatement's files, by content name, that keep the cases from going soft.
    Stuffing: the quality-100 noise of every shape holds an FF 00 in one of its two noise files at least (a 1 x 1 frame is one
    short interval, which may hold none).
    The 16-zeros code 0xF0: at quality 100 every quantiser is 1 and noise leaves no run of 16 zero coefficients (none in 30 of
    the 32 shape x subsampling cases), so the code is asserted where noise does produce it: at quality 30, from 16 x 16 on.
    150 x 24: 19 / 10 MCU rows, so RST7 is followed by a second RST0."""
    if q == 100:
        assert any(b"\xff\x00" in scan_of(files[n]) for n in ("noise", "binary noise")), (H, W, sub)
        if H * W >= 512:
            assert all(b"\xff\x00" in scan_of(files[n]) for n in ("noise", "binary noise")), (H, W, sub)
    if q == 30 and H >= 16 and W >= 16:
        frames = contents(H, W)
        assert count_zrl(frames["noise"], 30, sub) + count_zrl(frames["binary noise"], 30, sub) > 0, (H, W, sub)
    if (H, W) == (150, 24):
        for d in files.values():
            scan = scan_of(d)
            assert b"\xff\xd7" in scan and b"\xff\xd0" in scan[scan.index(b"\xff\xd7"):]


def count_zrl(frame, quality, subsampling) -> int:
    """0xF0 codes in the frame's file: zero runs of 16 and more in front of a coefficient"""
    n = 0
    for blocks, _ in mcu_rows(frame, quant_tables(quality), sub_code(subsampling)):
        b, k = np.nonzero(blocks[:, 1:])
        prev = np.zeros_like(k)
        prev[1:] = np.where(b[1:] == b[:-1], k[:-1] + 1, 0)
        n += int(np.count_nonzero(k + 1 - prev - 1 >= 16))
    return n


# ---------------------------------------------------------------------------------------------------- 1. restatement vs PIL
def check_restatement_shape(H, W):
    for sub in SUBSAMPLINGS:
        for q in QUALITIES:
            got = {}
            for name, frame in contents(H, W).items():
                got[name] = encode(frame, q, sub)
                want = pil_encode(frame, q, sub)
                assert got[name] == want, (H, W, sub, q, name, len(got[name]), len(want), first_difference(got[name], want))
            assert_hard_cases(H, W, sub, q, got)


def check_tables():
    for q in range(1, 101):
        for sub in SUBSAMPLINGS:
            segs, _ = segments(pil_encode(np.zeros((8, 8, 3), np.uint8), q, sub))
            dqt = [body for m, body in segs if m == 0xDB]
            assert [d[0] for d in dqt] == [0, 1]
            nat = np.zeros((2, 64), np.uint8)
            for i, d in enumerate(dqt):
                nat[i][ZIGZAG] = np.frombuffer(d[1:], np.uint8)
            from instantsplat_amd.jpeg import quant_tables as product_tables
            t = product_tables(q)
            assert isinstance(t, np.ndarray) and t.dtype == np.uint8 and t.shape == (2, 64)
            assert np.array_equal(t, nat) and np.array_equal(quant_tables(q), nat), q
    from instantsplat_amd.jpeg import quant_tables as product_tables
    assert np.array_equal(product_tables(0), product_tables(1)) and np.array_equal(product_tables(1000), product_tables(100))
    segs, _ = segments(pil_encode(np.zeros((8, 8, 3), np.uint8)))
    assert [bytes([tid] + bits + vals) for tid, bits, vals in DHT] == [body for m, body in segs if m == 0xC4]
    assert [len(body) + 2 for m, body in segs if m == 0xC4] == [31, 181, 31, 181]


# ---------------------------------------------------------------------------------------------------- device calls
def raw_encode(dev, frames: torch.Tensor, quality=90, subsampling="4:2:0", out_bytes=None, qtables=None, fills=(0xA5, 0x5A)):
    """mi355gs_jpeg_rgb8 itself, between guard bytes, once per fill of the buffers -> (out bytes [out_bytes], offsets)"""
    from instantsplat_amd import _lib
    L = _lib.lib()
    sub = sub_code(subsampling)
    N, H, W = frames.shape[:3]
    nscratch, nstream = int(L.mi355gs_jpeg_rgb8_scratch_bytes(N, H, W, sub)), int(L.mi355gs_jpeg_rgb8_stream_bytes(N, H, W, sub))
    assert nscratch > 0 and nstream > 0
    cap = nstream if out_bytes is None else int(out_bytes)
    qt = np.ascontiguousarray(quant_tables(quality) if qtables is None else qtables, dtype=np.uint8)
    results = []
    for fill in fills:
        scratch = torch.full((nscratch + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
        out = torch.full((cap + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
        offs = torch.full((N + 3,), -7, dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.mi355gs_jpeg_rgb8(_lib.stream_ptr(dev), N, H, W, sub, qt.ctypes.data, frames.data_ptr(), scratch.data_ptr() + GUARD,
                                           out.data_ptr() + GUARD, cap, offs.data_ptr() + 8), "jpeg_rgb8")
        o, s, host = offs.cpu().numpy(), scratch.cpu().numpy(), out.cpu().numpy()
        assert o[0] == -7 and o[-1] == -7 and o[1] == 0
        o = o[1:-1]
        assert np.all(s[:GUARD] == fill) and np.all(s[GUARD + nscratch:] == fill)
        assert np.all(host[:GUARD] == fill) and np.all(host[GUARD + cap:] == fill)   # nothing at or beyond out_bytes
        if out_bytes is None:   # nothing behind the last file either
            assert np.all(host[GUARD + int(o[-1]):GUARD + cap] == fill)
        assert int(o[-1]) <= nstream
        results.append((host[GUARD:GUARD + cap].tobytes(), o, fill))
    a, b = results[0], results[-1]
    assert np.array_equal(a[1], b[1])
    for i in range(N):   # every file that fits is identical whatever the buffers held
        if a[1][i + 1] <= cap:
            assert a[0][int(a[1][i]):int(a[1][i + 1])] == b[0][int(a[1][i]):int(a[1][i + 1])]
    return a[0], a[1]


def split_files(stream: bytes, offsets):
    return [stream[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def check_device_files(dev, frames_np: np.ndarray, quality, subsampling, label="", restate=True, fills=(0xA5, 0x5A)):
    """bare call and wrapper against the restatement (unless restate=False) and PIL, file by file"""
    from instantsplat_amd.jpeg import encode_jpeg_rgb8
    frames = torch.from_numpy(np.ascontiguousarray(frames_np)).to(dev)
    N, H, W = frames_np.shape[:3]
    stream, offsets = raw_encode(dev, frames, quality, subsampling, fills=fills)
    files = split_files(stream, offsets)
    enc = encode_jpeg_rgb8(frames, quality=quality, subsampling=subsampling)
    assert enc["stream"].dtype == torch.uint8 and enc["stream"].device.type == "cpu" and enc["offsets"].dtype == np.int64
    assert np.array_equal(enc["offsets"], offsets), (label, enc["offsets"], offsets)
    assert split_files(enc["stream"].numpy().tobytes(), enc["offsets"]) == files, label
    for i, data in enumerate(files):
        want = pil_encode(frames_np[i], quality, subsampling)
        if restate:
            mine = encode(frames_np[i], quality, subsampling)
            assert data == mine, (label, i, len(data), len(mine), first_difference(data, mine))
        assert data == want, (label, i, len(data), len(want), first_difference(data, want))
        assert decode(data).shape == (H, W, 3)
    return files


def first_difference(a: bytes, b: bytes):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return int(d[0]) if len(d) else n


def check_shape(dev, H, W):
    """every content (one call per quality and subsampling, the contents as its frames) at every quality"""
    cs = contents(H, W)
    stack = np.stack(list(cs.values()))
    for sub in SUBSAMPLINGS:
        for q in QUALITIES:
            # (the buffers' second fill — identical files whatever they held — at one quality per subsampling)
            files = check_device_files(dev, stack, q, sub, f"{H}x{W} {sub} q{q}", fills=(0xA5, 0x5A) if q == 90 else (0xA5,))
            assert_hard_cases(H, W, sub, q, dict(zip(cs, files)))


# ---------------------------------------------------------------------------------------------------- 3. stacks, addresses
def check_stacks_and_addresses(dev):
    from instantsplat_amd import _lib
    from instantsplat_amd.jpeg import encode_jpeg_rgb8
    rng = np.random.default_rng(5)
    cs = contents(24, 40)
    check_device_files(dev, np.stack([cs["noise"], cs["ramp"], cs["art crop"]]), 90, "4:2:0", "three contents")
    stack = rng.integers(0, 256, (3, 7, 9, 3), dtype=np.uint8)
    t = torch.from_numpy(stack).to(dev)
    assert t[1:].data_ptr() % 2 == 1 and t[1:].is_contiguous()
    for sub in SUBSAMPLINGS:
        stream, offsets = raw_encode(dev, t[1:], 90, sub)
        assert split_files(stream, offsets) == [pil_encode(f, 90, sub) for f in stack[1:]]
        assert split_files(stream, offsets) == [encode(f, 90, sub) for f in stack[1:]]
    frames = rng.integers(0, 256, (5, 9, 30, 3), dtype=np.uint8)
    t = torch.from_numpy(frames).to(dev)
    one = encode_jpeg_rgb8(t, quality=100)
    L = _lib.lib()
    calls = []
    real = L.mi355gs_jpeg_rgb8

    class Spy:   # counts the library calls of the split encode
        def __getattr__(self, name):
            if name == "mi355gs_jpeg_rgb8":
                return lambda *a: (calls.append(a[1]), real(*a))[1]
            return getattr(L, name)
    keep = _lib._LIB
    _lib._LIB = Spy()
    try:
        split = encode_jpeg_rgb8(t, quality=100, max_call_bytes=1)
    finally:
        _lib._LIB = keep
    assert len(calls) >= 5 and set(calls) == {1}   # (a file that outgrows the default capacity costs a second call)
    assert split["stream"].numpy().tobytes() == one["stream"].numpy().tobytes() and np.array_equal(split["offsets"], one["offsets"])
    assert split_files(one["stream"].numpy().tobytes(), one["offsets"]) == [pil_encode(f, 100) for f in frames]


# ---------------------------------------------------------------------------------------------------- 4. capacity
def check_capacity(dev):
    from instantsplat_amd.jpeg import encode_jpeg_rgb8
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, (3, 17, 33, 3), dtype=np.uint8)
    frames[2] = (rng.integers(0, 2, (17, 33, 3)) * 255).astype(np.uint8)
    t = torch.from_numpy(frames).to(dev)
    for sub in SUBSAMPLINGS:
        want = [pil_encode(f, 100, sub) for f in frames]
        exact = np.concatenate([[0], np.cumsum([len(w) for w in want])])
        cap = int(exact[1]) + len(want[1]) // 2                 # file 0 fits, file 1 does not
        out, offsets = raw_encode(dev, t, 100, sub, out_bytes=cap)
        assert np.array_equal(offsets, exact), (offsets, exact)
        assert out[:int(exact[1])] == want[0]
        scan2 = want[2][segments(want[2])[1]:-2]                # no byte of file 2: its scan data is nowhere in `out`
        assert len(scan2) > 64 and scan2[:64] not in out and scan2[-64:] not in out
        out, offsets = raw_encode(dev, t, 100, sub, out_bytes=int(exact[2]))   # exactly room for two
        assert np.array_equal(offsets, exact) and out == want[0] + want[1]
        out, offsets = raw_encode(dev, t, 100, sub, out_bytes=0)
        assert np.array_equal(offsets, exact) and out == b""
        enc = encode_jpeg_rgb8(t, quality=100, subsampling=sub)   # noise at quality 100 outgrows half of raw: the redo
        assert int(enc["offsets"][-1]) > 3 * (frames[0].size // 2 + 700)
        assert split_files(enc["stream"].numpy().tobytes(), enc["offsets"]) == want
        enc = encode_jpeg_rgb8(t, quality=100, subsampling=sub, capacity=int(exact[1]) + 5)
        assert split_files(enc["stream"].numpy().tobytes(), enc["offsets"]) == want
        enc = encode_jpeg_rgb8(t, quality=100, subsampling=sub, capacity=0)
        assert split_files(enc["stream"].numpy().tobytes(), enc["offsets"]) == want


# ---------------------------------------------------------------------------------------------------- 5. refusals
def check_entry_point_rejects_bad_arguments():
    """before any HIP call: the bogus device pointers are never touched"""
    from instantsplat_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    good = np.ascontiguousarray(quant_tables(90))
    keep = [good]

    def run(N=2, H=8, W=8, sub=2, qt=good, frames=fake, scratch=fake, out=fake, out_bytes=1 << 20, offs=fake):
        q = None if qt is None else qt.ctypes.data
        return L.mi355gs_jpeg_rgb8(None, N, H, W, sub, q, frames, scratch, out, out_bytes, offs)
    for kw in ("qt", "frames", "scratch", "out", "offs"):
        assert run(**{kw: None}) == EINVAL, kw
    for k in (0, 63, 64, 127):
        zero = good.copy()
        zero.reshape(-1)[k] = 0
        keep.append(zero)
        assert run(qt=zero) == EINVAL, k
    assert run(scratch=ctypes.c_void_p(0x1008)) == EINVAL and run(offs=ctypes.c_void_p(0x1004)) == EINVAL
    bad = (dict(N=0), dict(N=-1), dict(H=0), dict(H=-2), dict(W=0), dict(W=-2), dict(sub=1), dict(sub=3), dict(sub=-1), dict(N=65536),
           dict(H=65536, W=8), dict(H=8, W=65536), dict(H=65535, W=65535), dict(H=32768, W=21846))
    for kw in bad:
        assert run(**kw) == EINVAL, kw
        args = (kw.get("N", 2), kw.get("H", 8), kw.get("W", 8), kw.get("sub", 2))
        assert L.mi355gs_jpeg_rgb8_scratch_bytes(*args) == 0 and L.mi355gs_jpeg_rgb8_stream_bytes(*args) == 0, kw
    for args in ((1, 1, 1, 0), (1, 1, 1, 2), (65535, 8, 8, 2), (1, 65535, 8, 0), (1, 8, 65535, 2), (1, 32768, 21845, 2)):
        assert L.mi355gs_jpeg_rgb8_scratch_bytes(*args) > 0 and L.mi355gs_jpeg_rgb8_stream_bytes(*args) > 0, args


def check_python_refusals(dev):
    from instantsplat_amd.jpeg import encode_jpeg_rgb8, write_jpeg_files
    ok = torch.zeros(2, 4, 5, 3, dtype=torch.uint8, device=dev)
    for bad in (ok.float(), ok[..., :2], ok[None], ok[0, 0], ok.cpu().numpy(), ok[:, :, ::2]):
        with pytest.raises(ValueError):
            encode_jpeg_rgb8(bad)
    for kw in (dict(subsampling="4:2:2"), dict(subsampling=2), dict(quality="high"), dict(quality=None), dict(quality=float("nan")),
               dict(qtables=np.zeros((2, 64), np.uint8)), dict(qtables=np.ones((2, 63), np.uint8)), dict(qtables=np.full((2, 64), 300)),
               dict(capacity=-1)):
        with pytest.raises(ValueError):
            encode_jpeg_rgb8(ok, **kw)
    with pytest.raises(ValueError):
        write_jpeg_files(["a.jpg"], ok)
    empty = encode_jpeg_rgb8(ok[:0])
    assert empty["stream"].numel() == 0 and empty["offsets"].tolist() == [0]
    single = encode_jpeg_rgb8(ok[0], quality=75, subsampling="4:4:4")
    assert single["offsets"].shape == (2,) and single["stream"].numpy().tobytes() == pil_encode(np.zeros((4, 5, 3), np.uint8), 75, "4:4:4")
    qt = np.full((2, 64), 7, np.uint8)
    custom = encode_jpeg_rgb8(ok[0], qtables=qt)
    assert custom["stream"].numpy().tobytes() == pil_encode(np.zeros((4, 5, 3), np.uint8), qtables=qt)


def check_write_files(dev, tmp_path):
    from instantsplat_amd.jpeg import write_jpeg_files
    frames = np.stack([contents(16, 17)[n] for n in ("noise", "ramp")])
    paths = [os.path.join(str(tmp_path), f"{i}.jpg") for i in range(2)]
    write_jpeg_files(paths, torch.from_numpy(frames).to(dev), quality=75)
    for p, f in zip(paths, frames):
        assert open(p, "rb").read() == pil_encode(f, 75)


# ---------------------------------------------------------------------------------------------------- 6. the container
AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10


def walk_avi(data: bytes, files, W, H, fps=30):
    """every size, header field and index entry of an AVI/MJPG file as instantsplat_amd/video.py writes it; `files`: the
    stand-alone JPEG files expected as payloads, in order"""
    from fractions import Fraction
    N = len(files)
    u32 = lambda p: struct.unpack("<I", data[p:p + 4])[0]
    assert data[:4] == b"RIFF" and u32(4) == len(data) - 8 and data[8:12] == b"AVI " and len(data) % 2 == 0

    def children(start, end):
        out, p = [], start
        while p < end:
            four, size = data[p:p + 4], u32(p + 4)
            assert p + 8 + size <= end, (four, p, size, end)
            out.append((four, p, size))
            p += 8 + size + (size & 1)
        assert p == end, (p, end)
        return out
    top = children(12, len(data))
    assert [c[0] for c in top] == [b"LIST", b"LIST", b"idx1"]
    hdrl, movi, idx1 = top
    assert data[hdrl[1] + 8:hdrl[1] + 12] == b"hdrl" and data[movi[1] + 8:movi[1] + 12] == b"movi"
    h = children(hdrl[1] + 12, hdrl[1] + 8 + hdrl[2])
    assert [c[0] for c in h] == [b"avih", b"LIST"] and h[0][2] == 56
    largest = max(len(f) for f in files)
    rate = Fraction(fps).limit_denominator(1 << 20)
    avih = struct.unpack("<14I", data[h[0][1] + 8:h[0][1] + 64])
    assert avih[0] == round(1e6 / fps) and avih[3] == AVIF_HASINDEX and avih[4] == N and avih[6] == 1 and avih[7] == largest
    assert avih[8:10] == (W, H) and avih[1] == 0 and avih[2] == 0 and avih[5] == 0 and avih[10:] == (0, 0, 0, 0)
    assert data[h[1][1] + 8:h[1][1] + 12] == b"strl"
    s = children(h[1][1] + 12, h[1][1] + 8 + h[1][2])
    assert [c[0] for c in s] == [b"strh", b"strf"] and s[0][2] == 56 and s[1][2] == 40
    p = s[0][1] + 8
    assert data[p:p + 8] == b"vidsMJPG"
    flags, prio, init, scale, srate, start, length, buf, quality, sample = struct.unpack("<IIIIIIIIiI", data[p + 8:p + 48])
    assert (flags, prio, init, start, sample) == (0, 0, 0, 0, 0)
    assert (scale, srate) == (rate.denominator, rate.numerator) and length == N and buf == largest and quality == -1
    assert struct.unpack("<4h", data[p + 48:p + 56]) == (0, 0, W, H)
    bi = struct.unpack("<IiiHH4sIiiII", data[s[1][1] + 8:s[1][1] + 48])
    assert bi == (40, W, H, 1, 24, b"MJPG", 3 * W * H, 0, 0, 0, 0)
    chunks = children(movi[1] + 12, movi[1] + 8 + movi[2])
    assert len(chunks) == N and idx1[2] == 16 * N
    for i, (four, pos, size) in enumerate(chunks):
        assert four == b"00dc" and size == len(files[i])
        payload = data[pos + 8:pos + 8 + size]
        assert payload == files[i], i
        if size & 1:
            assert data[pos + 8 + size] == 0
        assert decode(payload).shape == (H, W, 3)
        e = idx1[1] + 8 + 16 * i
        assert data[e:e + 4] == b"00dc" and struct.unpack("<3I", data[e + 4:e + 16]) == (AVIIF_KEYFRAME, pos - (movi[1] + 8), size)
    return chunks


def check_container(tmp_path):
    """host framing only: the files come from PIL"""
    from instantsplat_amd.video import write_mjpeg_avi
    rng = np.random.default_rng(12)
    H, W = 16, 24
    files = []
    k = 0
    while len(files) < 5 or len({len(f) & 1 for f in files}) < 2:   # until both parities occur
        files.append(pil_encode(rng.integers(0, 256, (H, W, 3), dtype=np.uint8) >> (k % 4), 80))
        k += 1
        assert k < 64
    files = files[-5:] if len({len(f) & 1 for f in files[-5:]}) == 2 else files[:4] + files[-1:]
    assert {len(f) & 1 for f in files} == {0, 1} and len(files) == 5
    for fps in (30, 24):
        for n in (1, 5):
            sel = files[:n]
            stream = torch.from_numpy(np.frombuffer(b"".join(sel), np.uint8).copy())
            offsets = np.concatenate([[0], np.cumsum([len(f) for f in sel])]).astype(np.int64)
            path = os.path.join(str(tmp_path), f"v_{fps}_{n}.avi")
            write_mjpeg_avi(path, stream, offsets, W, H, fps=fps)
            walk_avi(open(path, "rb").read(), sel, W, H, fps)
    path = os.path.join(str(tmp_path), "bytes.avi")
    write_mjpeg_avi(path, b"".join(files), [0] + list(np.cumsum([len(f) for f in files])), W, H)   # bytes and a list do as well
    walk_avi(open(path, "rb").read(), files, W, H, 30)
    for bad in (dict(offsets=[0]), dict(offsets=[1, 5]), dict(offsets=[0, 5, 3]), dict(offsets=[0, len(files[0]) + 1]), dict(W=0), dict(fps=0)):
        kw = dict(stream=files[0], offsets=[0, len(files[0])], W=W, H=H, fps=30)
        kw.update(bad)
        with pytest.raises(ValueError):
            write_mjpeg_avi(path, **kw)

    class Huge(bytes):   # a stream that claims 2 GiB without holding it
        def __len__(self):
            return 1 << 31
    with pytest.raises(ValueError, match="2 GiB"):
        write_mjpeg_avi(path, Huge(), [0, 1 << 31], W, H)


# ---------------------------------------------------------------------------------------------------- 7. the stage
def check_stage(dev, st, tmp_path):
    """render_interpolated over a short path between two keyframes (the stage's own pose step would make 151 poses of them)"""
    from instantsplat_amd import render_path as rp
    from instantsplat_amd.io_formats import save_pose
    from instantsplat_amd.render_path import render_interpolated
    from tests.render_path_util import read_png, short_path
    seen = {}
    real_set, real_pose = rp.render_set, rp.save_interpolate_pose

    def spy(*a, **kw):   # the list the stage's own render_set call fills with its device frames
        seen["frames"] = kw.get("frames_out")
        return real_set(*a, **kw)

    def short(model_path, iteration, n_views):
        pose_dir = os.path.join(str(model_path), "pose", f"ours_{iteration}")
        target = os.path.join(pose_dir, "pose_interpolated.npy")
        np.save(target, short_path(np.load(os.path.join(pose_dir, "pose_optimized.npy"))[:n_views], 3))
        return target
    roots, args = {}, (30, 2, st.cameras[:2], st.gaussians, st.pipe, st.background)
    rp.render_set, rp.save_interpolate_pose = spy, short
    try:
        for video in ("mjpeg", "imageio"):
            root = os.path.join(str(tmp_path), video)
            os.makedirs(os.path.join(root, "pose", "ours_30"))
            save_pose(os.path.join(root, "pose", "ours_30", "pose_optimized.npy"), st.gaussians.P, [int(c.colmap_id) for c in st.cameras])
            roots[video] = os.path.dirname(render_interpolated(root, *args, video=video, png="device"))
            if video == "mjpeg":
                assert all(f.device.type == dev.type and f.dtype == torch.uint8 for f in seen["frames"])
                frames = torch.stack(list(seen["frames"])).cpu().numpy()
            else:
                assert seen["frames"] is None
        with pytest.raises(ValueError, match="video"):
            render_interpolated(roots["mjpeg"], *args, video="h264")
    finally:
        rp.render_set, rp.save_interpolate_pose = real_set, real_pose
    base = roots["mjpeg"]
    avi = os.path.join(base, "interp_2_view.avi")
    assert os.path.exists(avi)
    assert not [n for n in os.listdir(roots["imageio"]) if n.endswith(".avi")]
    names = sorted(os.listdir(os.path.join(base, "renders")))
    assert names == [f"{i:05d}.png" for i in range(4)] == sorted(os.listdir(os.path.join(roots["imageio"], "renders"))) and len(frames) == 4
    H, W = frames.shape[1:3]
    for i, n in enumerate(names):   # the PNG files as before, and of the very frames the video holds
        png = read_png(os.path.join(base, "renders", n))
        assert np.array_equal(png, frames[i]) and np.array_equal(png, read_png(os.path.join(roots["imageio"], "renders", n)))
    walk_avi(open(avi, "rb").read(), [pil_encode(f, 90, "4:2:0") for f in frames], W, H, 30)
