"""Resizing the input images on the device (csrc/resample.hip, include/mi355gs.h mi355gs_resample_rgb8): PIL's `Image.resize` for
8-bit RGB images, byte for byte, with the crop and the conversion to float that follow it in the reference's two loaders.

  resample_coeffs   PIL's coefficient tables (libImaging Resample.c, precompute_coeffs + normalize_coeffs_8bpc) for one axis, built
                    on the host in doubles: the device multiplies and adds integers, it evaluates no filter
  resize_rgb8       uint8 [N,H,W,3] on the device -> the resized images, or a window of them, as bytes (`np.array(img.resize(size,
                    filter).crop(box))`), as `unit` floats (reference utils/general_utils.py:21-27 PILtoTorch) or as `normalized`
                    floats (ToTensor + Normalize((.5,.5,.5), (.5,.5,.5)): `ImgNorm` of dust3r/utils/image.py); two kernel launches
  load_images       reference utils/sfm_utils.py:123-176 (= dust3r/utils/image.py:73-126), the input stage of init_geo.py:39 and
                    init_test_pose.py:39: files are decoded by PIL on the host; resize, centre crop and normalisation are one
                    `resize_rgb8` call per group of equally sized sources

Only PIL's LANCZOS, BICUBIC and BILINEAR filters and 8-bit RGB; there is no CPU fallback."""
from __future__ import annotations

import functools
import math
import os

import numpy as np
import torch

from . import _frames, _lib

PRECISION_BITS = 22          # libImaging Resample.c: 32 - 8 - 2
MAX_SIZE = 65535             # include/mi355gs.h: N and every size of one mi355gs_resample_rgb8 call
OUTPUTS = ("rgb8", "unit", "normalized")


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0)}
_PIL_CODES = {1: "lanczos", 2: "bilinear", 3: "bicubic"}   # PIL.Image.Resampling


def filter_name(resample) -> str:
    """"lanczos" | "bicubic" | "bilinear" (any case), or PIL's code for one of them -> the name"""
    if isinstance(resample, str) and resample.lower() in FILTERS:
        return resample.lower()
    if not isinstance(resample, (str, bool)) and isinstance(resample, (int, np.integer)) and int(resample) in _PIL_CODES:
        return _PIL_CODES[int(resample)]
    raise ValueError(f'resample must be "lanczos", "bicubic" or "bilinear" (or PIL\'s code for one of them), got {resample!r}')


@functools.lru_cache(maxsize=64)
def _coeffs(n_in: int, n_out: int, name: str):
    filt, filter_support = FILTERS[name]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = filter_support * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs   # (PIL multiplies by the reciprocal)
    k = np.zeros((n_out, ksize), np.int32)
    bounds = np.zeros((n_out, 2), np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k[xx, :xmax] = [int(v * one + 0.5) if v >= 0 else int(v * one - 0.5) for v in w]   # int(): truncation, as C's cast
        bounds[xx] = (xmin, xmax)
    assert int(np.abs(k).max()) < 1 << 23   # include/mi355gs.h: the kernels multiply by the low 24 bits
    k.setflags(write=False)
    bounds.setflags(write=False)
    return k, bounds


def resample_coeffs(n_in: int, n_out: int, filter="bicubic"):
    """-> (int32 [n_out, ksize] coefficients with 22 fractional bits, int32 [n_out, 2] = (first source index, taps) per output index):
    what PIL computes for resizing an axis of n_in samples to n_out with LANCZOS (support 3), BICUBIC (support 2, a = -0.5) or
    BILINEAR (support 1).  ksize = 2 ceil(support max(n_in / n_out, 1)) + 1; a row's coefficients beyond its taps are 0.
    The arrays are cached and read-only."""
    if isinstance(n_in, bool) or isinstance(n_out, bool) or not all(isinstance(n, (int, np.integer)) for n in (n_in, n_out)) or n_in <= 0 or n_out <= 0:
        raise ValueError(f"resample_coeffs takes two positive sizes, got {n_in!r}, {n_out!r}")
    return _coeffs(int(n_in), int(n_out), filter_name(filter))


_DEVICE_TABLES: dict = {}


def _device_tables(n_in, n_out, name, dev):
    key = (n_in, n_out, name, str(dev))
    t = _DEVICE_TABLES.get(key)
    if t is None:
        if len(_DEVICE_TABLES) >= 32:
            _DEVICE_TABLES.clear()
        k, b = _coeffs(n_in, n_out, name)
        t = _DEVICE_TABLES[key] = (torch.from_numpy(k.copy()).to(dev), torch.from_numpy(b.copy()).to(dev), b)
    return t


def resize_rgb8(images: torch.Tensor, size, resample="bicubic", window=None, out="rgb8"):
    """images: contiguous uint8 [N,H,W,3] (or [H,W,3]) on the device; size: (W', H') as PIL takes it.
    window: (x0, y0, w, h) inside the resized image: only that crop is computed (default: all of it).
    out: "rgb8" -> uint8 [N,h,w,3], the bytes of `Image.resize(size, resample)` (cropped to the window); "unit" -> float32 [N,3,h,w] =
    bytes / 255; "normalized" -> float32 [N,3,h,w] = (bytes / 255 - 0.5) / 0.5; or a tuple of these names -> a tuple of tensors, all
    from the same launches.  A [H,W,3] input gives outputs without the leading N.
    An axis whose size does not change is not resampled, as in PIL.
    Raises ValueError for anything but a contiguous uint8 device tensor of that shape, an empty target, a window outside it, or
    sizes beyond the library's limits."""
    single = isinstance(images, torch.Tensor) and images.dim() == 3
    images, N, H, W = _frames.check_frames("resize_rgb8", images, verb="resizes", arg="images")
    name = filter_name(resample)
    names = (out,) if isinstance(out, str) else tuple(out)
    if not names or any(not isinstance(o, str) or o not in OUTPUTS for o in names) or len(set(names)) != len(names):
        raise ValueError(f"out must be one of {OUTPUTS} or a tuple of them, got {out!r}")
    try:
        Wo, Ho = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (width, height), got {size!r}") from None
    if Wo <= 0 or Ho <= 0:
        raise ValueError(f"empty target: {Wo} x {Ho}")
    if window is None:
        x0, y0, w, h = 0, 0, Wo, Ho
    else:
        try:
            x0, y0, w, h = (int(v) for v in window)
        except (TypeError, ValueError):
            raise ValueError(f"window must be (x0, y0, w, h), got {window!r}") from None
        if x0 < 0 or y0 < 0 or w <= 0 or h <= 0 or x0 + w > Wo or y0 + h > Ho:
            raise ValueError(f"window {window!r} is empty or outside the {Wo} x {Ho} target")
    if max(N, H, W, Ho, Wo) > MAX_SIZE or 3 * H * W > 0x7fffffff or 3 * Ho * Wo > 0x7fffffff:
        raise ValueError(f"mi355gs_resample_rgb8 does not take {N} images of {H} x {W} -> {Ho} x {Wo} (include/mi355gs.h: the limits)")
    dev = images.device
    results = {o: torch.empty((N, h, w, 3) if o == "rgb8" else (N, 3, h, w), dtype=torch.uint8 if o == "rgb8" else torch.float32, device=dev)
               for o in names}
    if N:
        kx = bx = ky = by = scratch = None
        ksx = ksy = row0 = rows = 0
        if Wo != W:
            kx, bx, _ = _device_tables(W, Wo, name, dev)
            ksx = int(kx.shape[1])
        if Ho != H:
            ky, by, host = _device_tables(H, Ho, name, dev)
            ksy = int(ky.shape[1])
            if kx is not None:   # the source rows the window's vertical taps reach
                row0 = int(host[y0:y0 + h, 0].min())
                rows = int((host[y0:y0 + h, 0] + host[y0:y0 + h, 1]).max()) - row0
                scratch = _lib.scratch(dev, "resample_rgb8_scratch_bytes", N, rows, w, what=f"mi355gs_resample_rgb8 does not take an "
                                       f"intermediate of {N} x {rows} x {w} (include/mi355gs.h: the limits)")
        _lib.call(dev, "resample_rgb8", _lib.STREAM, N, H, W, Ho, Wo, images, kx, bx, ksx, ky, by, ksy, x0, y0, w, h, row0, rows, scratch,
                  results.get("rgb8"), results.get("unit"), results.get("normalized"))
    got = tuple(results[o][0] if single else results[o] for o in names)
    return got[0] if isinstance(out, str) else got


# ---------------------------------------------------------------------------------------------------- the network's input stage
IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".JPG", "PNG")   # the reference's list, as it stands (matched against the lowered name)


def _round_half_even_box(box):
    return tuple(int(round(v)) for v in box)   # PIL's Image.crop: map(int, map(round, box))


def load_geometry(W1: int, H1: int, size: int, square_ok: bool = False):
    """What the reference's load_images does to a W1 x H1 image -> (filter name, (W, H) of the resize, crop window (x0, y0, w, h))"""
    S = max(W1, H1)
    long_edge = round(size * max(W1 / H1, H1 / W1)) if size == 224 else size   # 224: the SHORT side becomes 224
    name = "lanczos" if S > long_edge else "bicubic"
    W, H = (int(round(x * long_edge / S)) for x in (W1, H1))
    cx, cy = W // 2, H // 2
    if size == 224:
        half = min(cx, cy)
        box = (cx - half, cy - half, cx + half, cy + half)
    else:
        halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
        if not square_ok and W == H:
            halfh = 3 * halfw / 4
        box = (cx - halfw, cy - halfh, cx + halfw, cy + halfh)
    l, t, r, b = _round_half_even_box(box)
    return name, (W, H), (l, t, r - l, b - t)


def load_images(folder_or_list, size, square_ok=False, verbose=True, device="cuda"):
    """The reference's `load_images`: every image of a folder (sorted names) or of a list of paths whose name has a supported
    extension, EXIF-transposed and converted to RGB on the host, then on the device resized (long side to `size`, LANCZOS when that
    shrinks it and BICUBIC otherwise; size 224: short side to 224), centre-cropped (to multiples of 16, 4:3 for a square image
    unless square_ok; size 224: to the square) and normalised to [-1, 1].
    -> ([dict(img=float32 [1,3,H2,W2] on `device`, true_shape=np.int32([[H2, W2]]), idx=i, instance=str(i))], (W1, H1) of the last
    image).  Sources of equal size share one `resize_rgb8` call."""
    from PIL import Image
    from PIL.ImageOps import exif_transpose
    if isinstance(folder_or_list, str):
        if verbose:
            print(f">> Loading images from {folder_or_list}")
        root, folder_content = folder_or_list, sorted(os.listdir(folder_or_list))
    elif isinstance(folder_or_list, list):
        if verbose:
            print(f">> Loading a list of {len(folder_or_list)} images")
        root, folder_content = "", folder_or_list
    else:
        raise ValueError(f"bad {folder_or_list=} ({type(folder_or_list)})")
    device = torch.device(device)
    sources, groups = [], {}
    for path in folder_content:
        if not path.lower().endswith(IMAGE_EXTENSIONS):
            continue
        img = exif_transpose(Image.open(os.path.join(root, path))).convert("RGB")
        groups.setdefault(img.size, []).append(len(sources))
        sources.append((path, np.asarray(img)))
    assert sources, "no images foud at " + root
    tensors = [None] * len(sources)
    for (W1, H1), members in groups.items():
        name, target, window = load_geometry(W1, H1, size, square_ok)
        if window[2] <= 0 or window[3] <= 0:
            raise ValueError(f"a {W1}x{H1} image leaves an empty crop at size {size}")
        stack = torch.from_numpy(np.stack([sources[i][1] for i in members]))
        batch = resize_rgb8(stack.to(device), target, resample=name, window=window, out="normalized")
        for j, i in enumerate(members):
            tensors[i] = batch[j:j + 1]
    imgs = []
    for i, (path, arr) in enumerate(sources):
        H2, W2 = (int(s) for s in tensors[i].shape[2:])
        if verbose:
            print(f" - adding {path} with resolution {arr.shape[1]}x{arr.shape[0]} --> {W2}x{H2}")
        imgs.append(dict(img=tensors[i], true_shape=np.int32([[H2, W2]]), idx=i, instance=str(i)))
    if verbose:
        print(f" (Found {len(imgs)} images)")
    W1, H1 = sources[-1][1].shape[1], sources[-1][1].shape[0]
    return imgs, (W1, H1)
