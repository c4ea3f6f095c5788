"""Checks of the device PNG encoder (instantsplat_amd/png.py, csrc/png.hip, include/mi355gs.h mi355gs_png_rgb8), shared by the
emulated (CPU) and the GPU test files.

Yardsticks: zlib (`crc32`, `decompress`, which verifies the Adler-32), PIL's decoder, and a host restatement of the stream — the
numpy Paeth filter, the per-block histogram, package-merge and the size prediction — that holds the device to the optimum's
cost per block, exactly, and to every file's byte count.  The restatement checks itself first (`check_host_restatement`)."""
import ctypes
import heapq
import io
import itertools
import os
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HDR_BITS = 74 + 258 * 4
SHAPES = [(1, 1), (1, 5), (7, 1), (3, 21), (5, 85), (5, 86), (17, 1365), (4, 2049), (33, 64)]   # H, W
COUNTS = (1, 3)
GUARD = 256
EINVAL = -1


# ---------------------------------------------------------------------------------------------------- host restatement
def paeth_filter(frame: np.ndarray) -> np.ndarray:
    """uint8 [H,W,3] -> uint8 [H, 3W+1]: filter byte 4, then the Paeth residuals (PNG specification 9.4, bpp = 3)"""
    H, W = frame.shape[:2]
    x = frame.reshape(H, 3 * W).astype(np.int32)
    a = np.zeros_like(x); a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, 3:] = x[:-1, :-3]
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    out = np.empty((H, 3 * W + 1), np.uint8)
    out[:, 0] = 4
    out[:, 1:] = ((x - pred) & 255).astype(np.uint8)
    return out


def default_rows(W):
    return max(1, 65536 // (3 * W + 1))


def block_counts(filtered: np.ndarray, R: int):
    """per block of R rows: the 257 counts (end of block counts 1)"""
    out = []
    for r0 in range(0, filtered.shape[0], R):
        f = np.bincount(filtered[r0:r0 + R].reshape(-1), minlength=257)
        f[256] = 1
        out.append(f)
    return out


def package_merge(counts, limit=15):
    """optimal code lengths under `limit` bits, in the prefix-count form: per level only a leaf / package flag is kept"""
    used = sorted((int(c), s) for s, c in enumerate(counts) if c > 0)
    n, lens = len(used), [0] * len(counts)
    if n == 1:
        lens[used[0][1]] = 1
        return lens
    assert n <= 1 << limit
    w = [c for c, _ in used]
    levels, prev = [], []
    for _ in range(limit):
        packages = [prev[2 * j] + prev[2 * j + 1] for j in range(len(prev) // 2)]
        merged = sorted([(x, 0) for x in w] + [(x, 1) for x in packages])
        prev = [m[0] for m in merged]
        levels.append([m[1] for m in merged])
    take, l = 2 * n - 2, [0] * n
    for flags in reversed(levels):
        assert take <= len(flags)
        p = sum(flags[:take])
        for i in range(take - p):
            l[i] += 1
        take = 2 * p
    for (_, s), li in zip(used, l):
        lens[s] = li
    return lens


def cost(counts, lens):
    return int(sum(int(c) * int(l) for c, l in zip(counts, lens)))


def huffman(counts):
    """unrestricted Huffman -> (cost, depth)"""
    heap = [(int(c), 0) for c in counts if c > 0]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    total = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        total += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return total, heap[0][1]


def brute_force_cost(counts, limit):
    best = None
    for lens in itertools.product(range(1, limit + 1), repeat=len(counts)):
        if sum(2.0 ** -l for l in lens) <= 1.0:
            c = cost(counts, lens)
            best = c if best is None else min(best, c)
    return best


def canonical_codes(lens):
    """deflate's canonical code (RFC 1951 3.2.2) -> codes, most significant bit first"""
    bl = [0] * 16
    for l in lens:
        bl[l] += 1
    bl[0], code, nxt = 0, 0, [0] * 16
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):   # least significant bit first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):   # a Huffman code: most significant bit first
        self.bits(int(format(c, "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


def model_block(data: bytes, final: bool, first: bool) -> bytes:
    """the block the issue fixes, from the host's own bit writer"""
    f = np.bincount(np.frombuffer(data, np.uint8), minlength=257)
    f[256] = 1
    lens = package_merge(f)
    codes = canonical_codes(lens)
    w = BitWriter()
    if first:
        w.bits(0x78, 8), w.bits(0x01, 8)
    w.bits(0, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(15, 4)
    for k in range(19):
        w.bits(0 if k < 3 else 4, 3)
    for l in list(lens) + [1]:
        w.code(l, 4)
    for s in list(data) + [256]:
        w.code(codes[s], lens[s])
    w.bits(1 if final else 0, 1), w.bits(0, 2)
    w.align()
    return bytes(w.out) + b"\x00\x00\xff\xff"


def chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_from_idat(H, W, idats) -> bytes:
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + b"".join(chunk(b"IDAT", d) for d in idats)
            + chunk(b"IEND", b""))


def model_file(frame: np.ndarray, R: int) -> bytes:
    filt = paeth_filter(frame)
    H = filt.shape[0]
    starts = list(range(0, H, R))
    idats = [model_block(filt[r0:r0 + R].tobytes(), r0 == starts[-1], r0 == 0) for r0 in starts]
    return png_from_idat(H, frame.shape[1], idats + [struct.pack(">I", zlib.adler32(filt.tobytes()))])


def predicted_file_bytes(frame: np.ndarray, R: int):
    """-> (file bytes, [sum f l of every block])"""
    costs = [cost(f, package_merge(f)) for f in block_counts(paeth_filter(frame), R)]
    size = 33 + sum(12 + (2 if i == 0 else 0) + (HDR_BITS + c + 3 + 7) // 8 + 4 for i, c in enumerate(costs)) + 16 + 12
    return size, costs


def decode(data: bytes) -> np.ndarray:
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB"
    return np.asarray(im)


def check_host_restatement():
    rng = np.random.default_rng(11)
    for k in range(300):   # package-merge against brute force, at limits that bind
        n = int(rng.integers(2, 7))
        limit = int(rng.integers(max(1, int(np.ceil(np.log2(n)))), 5))
        counts = [int(c) for c in (rng.integers(1, 40, n) if k % 2 else np.sort(rng.integers(1, 5, n)).cumsum())]
        lens = package_merge(counts, limit)
        assert max(lens) <= limit and sum(2.0 ** -l for l in lens) <= 1.0
        assert cost(counts, lens) == brute_force_cost(counts, limit), (counts, limit, lens)
    limited = 0
    for k in range(200):   # ... and against unrestricted Huffman wherever that fits 15 bits
        n = int(rng.integers(1, 258))
        counts = (rng.integers(1, 1000, n) if k % 3 else np.floor(1.5 ** rng.uniform(0, 30, n)).astype(np.int64) + 1)
        lens = package_merge(counts)
        hc, depth = huffman(counts)
        assert max(lens) <= 15 and (n == 1 or abs(sum(2.0 ** -l for l in lens) - 1.0) < 1e-12)
        if depth <= 15:
            assert cost(counts, lens) == hc
        else:
            limited += 1
            assert cost(counts, lens) > hc
    assert limited > 10
    for H, W, R in ((5, 7, 2), (1, 1, 1), (9, 40, 9)):   # the model file decodes in PIL and is as long as predicted
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        data = model_file(frame, R)
        assert np.array_equal(decode(data), frame)
        assert len(data) == predicted_file_bytes(frame, R)[0]


# ---------------------------------------------------------------------------------------------------- parsing
def parse_png(data: bytes):
    """-> (W, H, [IDAT data]); every chunk's CRC is checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body), (kind, len(chunks))
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data)
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and chunks[-1][1] == b"" and set(kinds[1:-1]) == {b"IDAT"}
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    return W, H, [body for _, body in chunks[1:-1]]


def header_lengths(data: bytes, first: bool):
    """the 258 code lengths of a block's header, read at their fixed position; the 74 bits in front of them are checked"""
    bits = int.from_bytes(data[:2 + (HDR_BITS + 7) // 8 + 1], "little")
    if first:
        assert bits & 0xffff == 0x0178
        bits >>= 16
    assert bits & 1 == 0 and (bits >> 1) & 3 == 2 and (bits >> 3) & 31 == 0 and (bits >> 8) & 31 == 0 and (bits >> 13) & 15 == 15
    for k in range(19):
        assert (bits >> (17 + 3 * k)) & 7 == (0 if k < 3 else 4)
    return [int(format((bits >> (74 + 4 * s)) & 15, "04b")[::-1], 2) for s in range(258)]


# ---------------------------------------------------------------------------------------------------- device calls
def raw_encode(dev, frames: torch.Tensor, R: int):
    """mi355gs_png_rgb8 itself, between guard bytes -> (stream bytes, offsets, stream bound)"""
    from instantsplat_amd import _lib
    L = _lib.lib()
    N, H, W = frames.shape[:3]
    nscratch, nstream = int(L.mi355gs_png_rgb8_scratch_bytes(N, H, W, R)), int(L.mi355gs_png_rgb8_stream_bytes(N, H, W, R))
    assert nscratch > 0 and nstream > 0
    results = []
    for fill in (0xA5, 0x5A):   # two calls: identical files whatever the buffers held
        scratch = torch.full((nscratch + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
        out = torch.full((nstream + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
        offs = torch.full((N + 3,), -7, dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.mi355gs_png_rgb8(_lib.stream_ptr(dev), N, H, W, R, frames.data_ptr(), scratch.data_ptr() + GUARD,
                                          out.data_ptr() + GUARD, offs.data_ptr() + 8), "png_rgb8")
        o, s, host = offs.cpu().numpy(), scratch.cpu().numpy(), out.cpu().numpy()
        assert o[0] == -7 and o[-1] == -7 and o[1] == 0
        o = o[1:-1]
        assert np.all(s[:GUARD] == fill) and np.all(s[GUARD + nscratch:] == fill)
        assert np.all(host[:GUARD] == fill) and np.all(host[GUARD + int(o[-1]):] == fill)   # nothing behind the last file is written
        assert int(o[-1]) <= nstream
        results.append((host[GUARD:GUARD + int(o[-1])].tobytes(), o))
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1])
    return results[0][0], results[0][1], nstream


def check_files(stream: bytes, offsets, frames_np: np.ndarray, R: int, label=""):
    """every property of the files of one call that the stream's definition fixes"""
    N, H, W = frames_np.shape[:3]
    R = R or default_rows(W)
    assert offsets[0] == 0 and len(offsets) == N + 1
    for i in range(N):
        data = stream[int(offsets[i]):int(offsets[i + 1])]
        w, h, idats = parse_png(data)
        assert (w, h) == (W, H)
        filt = paeth_filter(frames_np[i])
        counts = block_counts(filt, R)
        assert len(idats) == len(counts) + 1 and len(idats[-1]) == 4
        raw = zlib.decompress(b"".join(idats))   # checks the Adler-32
        assert len(raw) == H * (3 * W + 1) and raw == filt.tobytes(), (label, i)
        assert np.array_equal(decode(data), frames_np[i]), (label, i)
        size, costs = predicted_file_bytes(frames_np[i], R)
        for b, (f, body) in enumerate(zip(counts, idats)):
            lens = header_lengths(body, b == 0)
            assert lens[257] == 1 and max(lens) <= 15
            assert all((l == 0) == (c == 0) for l, c in zip(lens[:257], f)), (label, i, b)
            if np.count_nonzero(f) > 1:
                assert sum(2.0 ** -l for l in lens[:257] if l) == 1.0, (label, i, b)
            assert cost(f, lens[:257]) == costs[b], (label, i, b, cost(f, lens[:257]), costs[b])
            assert len(body) == (2 if b == 0 else 0) + (HDR_BITS + costs[b] + 3 + 7) // 8 + 4
        assert len(data) == size, (label, i, len(data), size)


def check_stream(dev, frames_np: np.ndarray, R: int, label=""):
    """frames_np uint8 [N,H,W,3]; R = 0: the default rows per block"""
    from instantsplat_amd.png import encode_png_rgb8
    frames = torch.from_numpy(np.array(frames_np)).to(dev)
    stream, offsets, _ = raw_encode(dev, frames, R)
    check_files(stream, offsets, frames_np, R, label)
    enc = encode_png_rgb8(frames, rows_per_block=R or None)   # the Python entry gives the same bytes
    assert enc["stream"].dtype == torch.uint8 and enc["stream"].device.type == "cpu" and enc["offsets"].dtype == np.int64
    assert enc["stream"].numpy().tobytes() == stream and np.array_equal(enc["offsets"], offsets)
    return stream, offsets


def rows_choices(H):
    return (1, 2, 3, H, H + 1, 0)


def check_shape(dev, H, W):
    rng = np.random.default_rng(100 * H + W)
    for N in COUNTS:
        base = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        smooth = (np.add.outer(np.arange(H), np.arange(W))[None, :, :, None] * np.array([1, 2, 3]) // 2 + rng.integers(0, 3, (N, H, W, 3))).astype(np.uint8)
        # Each R sees one of the two contents (odd R: noise, even R and the default: the smooth ramp); both contents meet every
        # shape.  An R whose block would exceed 65536 bytes is refused by the library (check_entry_point_rejects_bad_arguments)
        # and left out here: R = H = 17 and R = H + 1 = 18 at W = 1365, whose default is 16.
        for R in rows_choices(H):
            if R * (3 * W + 1) > 65536:
                continue
            check_stream(dev, base if R % 2 else smooth, R, f"{N}x{H}x{W} R={R}")


def check_odd_base_address(dev):
    """a stack of odd-sized frames sliced behind its first frame, and a view one byte into a buffer"""
    rng = np.random.default_rng(3)
    stack = rng.integers(0, 256, (3, 5, 7, 3), dtype=np.uint8)
    t = torch.from_numpy(stack).to(dev)
    assert t[1:].data_ptr() % 2 == 1 and t[1:].is_contiguous()
    stream, offsets, _ = raw_encode(dev, t[1:], 2)
    check_files(stream, offsets, stack[1:], 2, "odd slice")
    frames = rng.integers(0, 256, (2, 6, 40, 3), dtype=np.uint8)
    buf = torch.zeros(frames.size + 8, dtype=torch.uint8)
    buf[1:1 + frames.size] = torch.from_numpy(frames).reshape(-1)
    buf = buf.to(dev)
    view = buf[1:1 + frames.size].view(2, 6, 40, 3)
    assert view.data_ptr() % 4 == 1
    stream, offsets, _ = raw_encode(dev, view, 0)
    check_files(stream, offsets, frames, 0, "offset view")


# ---------------------------------------------------------------------------------------------------- contents
def equal_frequency_frame():
    """one block whose 256 literals are equally frequent: two rows of 3 x 85 + 1 = 256 bytes, every literal twice (the two filter
    bytes are literal 4's two) -> with the end of block's 1, lengths 8 and 9"""
    seq = np.repeat(np.arange(256, dtype=np.uint8), 2)
    return frame_from_residuals(np.random.default_rng(6).permutation(seq[seq != 4]).reshape(2, 255))


def frame_from_residuals(residuals: np.ndarray) -> np.ndarray:
    """uint8 [H, 3W] Paeth residuals -> the frame [1,H,W,3] that has them, by decoding a host-made PNG in PIL"""
    H, W = residuals.shape[0], residuals.shape[1] // 3
    filt = np.concatenate([np.full((H, 1), 4, np.uint8), residuals], axis=1)
    frame = decode(png_from_idat(H, W, [zlib.compress(filt.tobytes())]))
    assert np.array_equal(paeth_filter(frame), filt)
    return frame[None]


def fibonacci_frame():
    """One row whose literal counts are 1, 2, 3, 5, 8, ... over 20 literals — with the end-of-block symbol's 1 the Fibonacci
    sequence, the deepest Huffman tree a block of its size can have (20 levels).  The filter byte 4 is the literal counted once.
    The 19 residual literals sum to 28654 bytes, which is no multiple of 3: the most frequent literal gives up one (10945 instead
    of 10946), which changes no merge of the tree but the last."""
    fib = [1, 2]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    fib[-1] -= 1
    literals = [4] + [s for s in range(7, 200, 10)][:19]
    residuals = np.concatenate([np.full(c, s, np.uint8) for s, c in zip(literals[1:], fib[1:])])
    assert residuals.size % 3 == 0 and residuals.size == 28653
    residuals = np.random.default_rng(9).permutation(residuals)
    frames = frame_from_residuals(residuals[None])
    f = block_counts(paeth_filter(frames[0]), 1)[0]
    assert sorted(int(c) for c in f if c) == sorted([1] + fib)
    assert huffman(f)[1] > 15   # the limit binds: the case cannot pass vacuously
    return frames


def check_fibonacci(dev):
    frames = fibonacci_frame()
    stream, offsets = check_stream(dev, frames, 1, "fibonacci")
    _, _, idats = parse_png(stream)
    lens = header_lengths(idats[0], True)
    assert max(lens) == 15   # the limit is reached and kept
    f = block_counts(paeth_filter(frames[0]), 1)[0]
    assert cost(f, lens[:257]) > huffman(f)[0]


def check_contents(dev):
    rng = np.random.default_rng(21)
    H, W = 6, 50
    check_stream(dev, np.zeros((2, H, W, 3), np.uint8), 4, "zeros")   # literals 0 and 4 and the end of block
    check_stream(dev, np.broadcast_to(np.array([200, 17, 3], np.uint8), (1, H, W, 3)).copy(), 0, "constant")
    noise = rng.integers(0, 256, (1, 40, 300, 3), dtype=np.uint8)    # all 256 literals: the size bound
    stream, offsets, bound = raw_encode(dev, torch.from_numpy(noise).to(dev), 0)
    check_files(stream, offsets, noise, 0, "noise")
    assert 36000 < len(stream) <= bound
    eq = equal_frequency_frame()
    stream, _ = check_stream(dev, eq, 2, "equal frequencies")
    lens = header_lengths(parse_png(stream)[2][0], True)
    assert sorted(set(lens[:257])) == [8, 9]
    ramp = np.broadcast_to((np.arange(300) % 256).astype(np.uint8)[None, None, :, None], (1, 9, 300, 3)).copy()
    check_stream(dev, ramp, 4, "ramp")


def art_frames():
    names = sorted(n for n in os.listdir(os.path.join(GOLDEN, "sora_art")) if n.startswith("art_frame_") and n.endswith(".jpg"))
    return np.stack([np.asarray(Image.open(os.path.join(GOLDEN, "sora_art", n)).convert("RGB")) for n in names])


def check_art_crop(dev):
    crop = art_frames()[:1, 300:364, 500:596].copy()   # 64 x 96
    check_stream(dev, crop, 0, "art crop")
    check_stream(dev, crop, 16, "art crop R=16")


# ---------------------------------------------------------------------------------------------------- refusals, splitting
def check_entry_point_rejects_bad_arguments():
    """before any HIP call: the bogus device pointers are never touched"""
    from instantsplat_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    run = lambda N=2, H=8, W=8, R=0, frames=fake, scratch=fake, out=fake, offs=fake: L.mi355gs_png_rgb8(None, N, H, W, R, frames, scratch, out, offs)
    for kw in ("frames", "scratch", "out", "offs"):
        assert run(**{kw: None}) == EINVAL, kw
    bad = (dict(N=0), dict(N=-1), dict(H=0), dict(H=-2), dict(W=0), dict(W=-2), dict(R=-1), dict(N=65536), dict(W=21846), dict(W=21845, R=2),
           dict(W=85, R=257), dict(W=8, R=2622), dict(N=65535, H=1 << 20, W=8, R=1), dict(H=(1 << 31) - 1, W=1, R=1))
    for kw in bad:
        assert run(**kw) == EINVAL, kw
        args = (kw.get("N", 2), kw.get("H", 8), kw.get("W", 8), kw.get("R", 0))
        assert L.mi355gs_png_rgb8_scratch_bytes(*args) == 0 and L.mi355gs_png_rgb8_stream_bytes(*args) == 0, kw
    assert L.mi355gs_png_rgb8_scratch_bytes(1, 1, 1, 0) > 0 and L.mi355gs_png_rgb8_stream_bytes(1, 1, 1, 0) > 0
    assert L.mi355gs_png_rgb8_scratch_bytes(2, 8, 21845, 1) > 0 and L.mi355gs_png_rgb8_scratch_bytes(2, 8, 85, 256) > 0
    assert L.mi355gs_png_rgb8_stream_bytes(201, 720, 1280, 0) >= 201 * 720 * 3841 * 9 // 8


def check_python_refusals(dev):
    from instantsplat_amd.png import encode_png_rgb8, write_png_files
    ok = torch.zeros(2, 4, 5, 3, dtype=torch.uint8, device=dev)
    for bad in (ok.float(), ok[..., :2], ok[None], ok[0, 0], ok.cpu().numpy(), ok[:, :, ::2]):
        with pytest.raises(ValueError):
            encode_png_rgb8(bad)
    for kw in (dict(rows_per_block=0), dict(rows_per_block=-1), dict(rows_per_block=4097)):
        with pytest.raises(ValueError):
            encode_png_rgb8(ok, **kw)
    with pytest.raises(ValueError):
        write_png_files(["a.png"], ok)
    empty = encode_png_rgb8(ok[:0])
    assert empty["stream"].numel() == 0 and empty["offsets"].tolist() == [0]
    single = encode_png_rgb8(ok[0])
    assert single["offsets"].shape == (2,) and np.array_equal(decode(single["stream"].numpy().tobytes()), ok[0].cpu().numpy())


def check_split_calls(dev):
    """5 frames under a limit that forces three library calls give the one-call result byte for byte"""
    from instantsplat_amd import _lib
    from instantsplat_amd.png import encode_png_rgb8
    frames = np.random.default_rng(4).integers(0, 256, (5, 9, 30, 3), dtype=np.uint8)
    t = torch.from_numpy(frames).to(dev)
    one = encode_png_rgb8(t)
    L = _lib.lib()
    size = lambda n: int(L.mi355gs_png_rgb8_scratch_bytes(n, 9, 30, 0)) + int(L.mi355gs_png_rgb8_stream_bytes(n, 9, 30, 0)) + 8 * (n + 1)
    limit = size(2)
    assert size(3) > limit
    calls = []
    real = L.mi355gs_png_rgb8
    class Spy:   # counts the library calls of the split encode
        def __getattr__(self, name):
            if name == "mi355gs_png_rgb8":
                return lambda *a: (calls.append(a[1]), real(*a))[1]
            return getattr(L, name)
    keep = _lib._LIB
    _lib._LIB = Spy()
    try:
        split = encode_png_rgb8(t, max_call_bytes=limit)
    finally:
        _lib._LIB = keep
    assert calls == [2, 2, 1]
    assert split["stream"].numpy().tobytes() == one["stream"].numpy().tobytes() and np.array_equal(split["offsets"], one["offsets"])
    check_files(one["stream"].numpy().tobytes(), one["offsets"], frames, 0, "split")


# ---------------------------------------------------------------------------------------------------- the stages' files
def check_render_set_device_equals_pil(dev, st, views, tmp_path):
    """render_set(png="device") and png="pil" write the same file names, and every pair of files holds the same pixels"""
    from instantsplat_amd.render_path import render_interpolated, render_set
    from tests.render_path_util import read_png
    for name in ("interp", "train"):
        dirs = {}
        for png in ("pil", "device"):
            root = os.path.join(str(tmp_path), png)
            d = render_set(root, name, 30, views, st.gaussians, st.pipe, st.background, png=png)
            dirs[png] = os.path.dirname(d)
        for sub in ("renders", "gt"):
            a, b = (sorted(os.listdir(os.path.join(dirs[png], sub))) for png in ("pil", "device"))
            assert a == b and len(a) == (0 if (name, sub) == ("interp", "gt") else len(views)), (name, sub, a, b)
            for f in a:
                assert np.array_equal(read_png(os.path.join(dirs["pil"], sub, f)), read_png(os.path.join(dirs["device"], sub, f))), (name, sub, f)
                parse_png(open(os.path.join(dirs["device"], sub, f), "rb").read())   # the device's stream: IDAT per block, CRCs
    for fn, args in ((render_set, (str(tmp_path), "train", 30, views, st.gaussians, st.pipe, st.background)),
                     (render_interpolated, (str(tmp_path), 30, 3, st.cameras, st.gaussians, st.pipe, st.background))):
        with pytest.raises(ValueError, match="png"):
            fn(*args, png="zlib")


def check_test_set_device_files(dev, st, tmp_path, num_iter=5):
    """render_test_set(png="device"): renders and ground truth decode to the frame stacks, and evaluate() scores the files as it
    scores the stacks"""
    import copy
    from instantsplat_amd.metrics import evaluate
    from instantsplat_amd.pose_tracking import render_test_set
    from tests.render_path_util import read_png
    views = [copy.copy(c) for c in st.cameras]
    for i, v in enumerate(views):
        v.image_name = f"view_{i}"
    root = os.path.join(str(tmp_path), "model")
    with pytest.raises(ValueError, match="png"):
        render_test_set(root, 30, views, st.gaussians, st.pipe, st.background, num_iter=num_iter, png="host")
    res = render_test_set(root, 30, views, st.gaussians, st.pipe, st.background, num_iter=num_iter, fused=True, png="device")
    base = os.path.join(root, "test", "ours_30")
    names = sorted(f"view_{i}.png" for i in range(len(views)))
    assert sorted(os.listdir(os.path.join(base, "renders"))) == names == sorted(os.listdir(os.path.join(base, "gt")))
    for grp in res["frames"]["ours_30"]:
        for k, name in enumerate(grp["names"]):
            for sub, stack in (("renders", grp["renders"]), ("gt", grp["gts"])):
                path = os.path.join(base, sub, name)
                assert np.array_equal(read_png(path), stack[k].cpu().numpy()), (sub, name)
                parse_png(open(path, "rb").read())
    assert evaluate(root) == evaluate(root, frames=res["frames"])
