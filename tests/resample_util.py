"""Checks of the device resampler (instantsplat_amd/resample.py, csrc/resample.hip, include/mi355gs.h mi355gs_resample_rgb8) and of
what is built on it (`load_images`, `scene_io.load_cam(resize="device")`), shared by the emulated (CPU) and the GPU test files.

Yardsticks, all run in the test itself: PIL's `Image.resize` / `Image.crop` for the bytes, torch on the host for the float outputs,
and a numpy restatement of PIL's two integer passes driven by `resample_coeffs` (`restate`), which localises a failure to the tables
or to the kernels.  torchvision is not installed, so its two transforms are restated: `ToTensor` as
`torch.from_numpy(bytes).permute(2, 0, 1).float().div(255)` and `Normalize((.5,.5,.5), (.5,.5,.5))` as `.sub(0.5).div(0.5)`.
Every comparison is exact — bytes equal, float32 bit patterns equal; nothing here has a tolerance."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1
GUARD = 256
PIL_FILTER = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}

# (H, W) -> (W', H'), filter
CASES = {
    "both passes, odd sizes": (37, 53, 19, 11, "lanczos"),
    "horizontal pass skipped": (37, 53, 53, 11, "lanczos"),
    "vertical pass skipped": (37, 53, 19, 37, "lanczos"),
    "upscaling": (37, 53, 80, 61, "bicubic"),
    "upscaling from 3x2": (3, 2, 9, 7, "bicubic"),
    "upscaling from 1x1": (1, 1, 4, 4, "bicubic"),
    "one output pixel": (7, 5, 1, 1, "lanczos"),
    "long tap loops": (120, 160, 16, 12, "lanczos"),
    "longer tap loops": (301, 403, 51, 38, "lanczos"),
    "bilinear, one axis up and one down": (64, 48, 33, 65, "bilinear"),
    "copy": (37, 53, 53, 37, "bicubic"),
}
STACKED = ("both passes, odd sizes", "horizontal pass skipped", "vertical pass skipped", "upscaling", "upscaling from 3x2", "upscaling from 1x1")
WINDOW_CASES = ("both passes, odd sizes", "longer tap loops")
# beyond the issue's table: sizes at which libm's sin and the reciprocal of the scale are exercised at other arguments
TABLE_SIZES = [(53, 19), (37, 11), (403, 51), (301, 38), (160, 16), (1280, 512), (720, 288), (4032, 384), (3024, 512), (2, 9), (1, 4),
               (5, 1), (48, 33), (64, 65), (100, 99), (99, 100), (1000, 7)]


def inputs(N, H, W, seed=0):
    """-> {name: uint8 [N,H,W,3]}: uniform bytes, and 0 / 255 bytes (the negative lobes then overshoot both ends: the clip to 0, the
    clip to 255 and the 8-bit intermediate all decide bytes); a different image per slot"""
    rng = np.random.default_rng(100003 * H + 101 * W + seed)
    return {"noise": rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8), "binary": (rng.integers(0, 2, (N, H, W, 3)) * 255).astype(np.uint8)}


def pil_resize(a: np.ndarray, size, name) -> np.ndarray:
    return np.array(Image.fromarray(a).resize(tuple(size), PIL_FILTER[name]))


# ---------------------------------------------------------------------------------------------------- host restatement
def _pass(a: np.ndarray, k: np.ndarray, bounds: np.ndarray) -> np.ndarray:
    """one pass along axis 0 of an int64 array holding bytes"""
    out = np.empty((k.shape[0],) + a.shape[1:], np.int64)
    for i in range(k.shape[0]):
        lo, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << 21) + np.tensordot(k[i, :n].astype(np.int64), a[lo:lo + n], axes=1)
        assert np.all(np.abs(acc) < 1 << 31)
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


def restate(a: np.ndarray, size, name) -> np.ndarray:
    """uint8 [H,W,3] -> uint8 [H',W',3]: PIL's horizontal pass, 8 bits, then its vertical pass, from the product's tables"""
    from instantsplat_amd.resample import resample_coeffs
    Wo, Ho = size
    v = a.astype(np.int64)
    if Wo != a.shape[1]:
        v = _pass(v.transpose(1, 0, 2), *resample_coeffs(a.shape[1], Wo, name)).transpose(1, 0, 2)
    if Ho != a.shape[0]:
        v = _pass(v, *resample_coeffs(a.shape[0], Ho, name))
    return v.astype(np.uint8)


def check_tables_shape():
    from instantsplat_amd.resample import resample_coeffs
    for name, support in (("lanczos", 3), ("bicubic", 2), ("bilinear", 1)):
        for n_in, n_out in ((8 * 64, 64), (40 * 16, 16), (16, 64), (7, 7)):
            k, b = resample_coeffs(n_in, n_out, name)
            taps = 2 * int(np.ceil(support * max(n_in / n_out, 1))) + 1
            assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape == (n_out, taps) and b.shape == (n_out, 2)
            assert np.all(b[:, 0] >= 0) and np.all(b[:, 1] >= 1) and np.all(b[:, 0] + b[:, 1] <= n_in) and np.all(b[:, 1] <= taps)
            assert all(not k[i, b[i, 1]:].any() for i in range(n_out))
            assert np.all(np.abs(k.sum(axis=1) - (1 << 22)) <= taps)   # a row sums to one, up to its roundings
    assert resample_coeffs(8 * 64, 64, "lanczos")[0].shape[1] == 49 and resample_coeffs(40 * 16, 16, "lanczos")[0].shape[1] == 241
    assert resample_coeffs(10, 5, Image.LANCZOS)[0] is resample_coeffs(10, 5, "LANCZOS")[0]
    for bad in ((0, 4, "lanczos"), (4, 0, "lanczos"), (4, 4, "box"), (4, 4, 0), (4.5, 4, "lanczos")):
        with pytest.raises(ValueError):
            resample_coeffs(*bad)


def check_tables_one_row(n_in, n_out):
    """a one-row image resized along x by the table alone must be PIL's"""
    rng = np.random.default_rng(n_in * 7 + n_out)
    row = np.concatenate([rng.integers(0, 256, (1, n_in, 3), dtype=np.uint8), (rng.integers(0, 2, (1, n_in, 3)) * 255).astype(np.uint8)])
    for name in PIL_FILTER:
        for r in row:
            assert np.array_equal(restate(r[None], (n_out, 1), name), pil_resize(r[None], (n_out, 1), name)), (n_in, n_out, name)


def check_restatement(case):
    H, W, Wo, Ho, name = CASES[case]
    for label, stack in inputs(1, H, W).items():
        assert np.array_equal(restate(stack[0], (Wo, Ho), name), pil_resize(stack[0], (Wo, Ho), name)), (case, label)


# ---------------------------------------------------------------------------------------------------- device calls
def device_resize(dev, stack: np.ndarray, size, name, **kw):
    from instantsplat_amd.resample import resize_rgb8
    return resize_rgb8(torch.from_numpy(np.ascontiguousarray(stack)).to(dev), size, resample=name, **kw)


def first_difference(got: np.ndarray, want: np.ndarray):
    d = np.argwhere(got != want)
    return (len(d), tuple(int(v) for v in d[0]), int(got[tuple(d[0])]), int(want[tuple(d[0])])) if len(d) else None


def check_case(dev, case, N=1, restated=True):
    H, W, Wo, Ho, name = CASES[case]
    for label, stack in inputs(N, H, W).items():
        got = device_resize(dev, stack, (Wo, Ho), name)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (N, Ho, Wo, 3) and got.device.type == dev.type
        got = got.cpu().numpy()
        for i in range(N):
            want = pil_resize(stack[i], (Wo, Ho), name)
            if restated:
                mine = restate(stack[i], (Wo, Ho), name)
                assert np.array_equal(got[i], mine), (case, label, i, first_difference(got[i], mine))
            assert np.array_equal(got[i], want), (case, label, i, first_difference(got[i], want))


def raw_call(dev, stack: np.ndarray, size, name, window=None, fill=0xA5):
    """mi355gs_resample_rgb8 itself, every buffer between guard bytes, all three outputs at once -> (rgb8, unit, normalized) numpy"""
    from instantsplat_amd import _lib
    from instantsplat_amd.resample import resample_coeffs
    L = _lib.lib()
    N, H, W = stack.shape[:3]
    Wo, Ho = size
    x0, y0, w, h = window or (0, 0, Wo, Ho)
    images = torch.from_numpy(np.ascontiguousarray(stack)).to(dev)
    keep, args = [], {}
    for axis, n_in, n_out in (("x", W, Wo), ("y", H, Ho)):
        if n_in == n_out:
            args[axis] = (None, None, 0)
            continue
        k, b = resample_coeffs(n_in, n_out, name)
        tk, tb = torch.from_numpy(k.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
        keep += [tk, tb]
        args[axis] = (tk.data_ptr(), tb.data_ptr(), k.shape[1])
    row0 = rows = nscratch = 0
    if W != Wo and H != Ho:
        by = resample_coeffs(H, Ho, name)[1]
        row0 = int(by[y0, 0])
        rows = int(by[y0 + h - 1, 0] + by[y0 + h - 1, 1]) - row0
        nscratch = int(L.mi355gs_resample_rgb8_scratch_bytes(N, rows, w))
        assert nscratch >= N * rows * w * 3
    scratch = torch.full((nscratch + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    n8 = N * h * w * 3
    bufs = [torch.full((n8 + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)]
    fbufs = [torch.full((n8 + 2 * GUARD,), float.fromhex("0x1.8p+100"), dtype=torch.float32, device=dev) for _ in range(2)]
    with _lib.on_device(dev):
        _lib.check(L.mi355gs_resample_rgb8(_lib.stream_ptr(dev), N, H, W, Ho, Wo, images.data_ptr(), *args["x"], *args["y"], x0, y0, w, h, row0,
                                           rows, scratch.data_ptr() + GUARD, bufs[0].data_ptr() + GUARD, fbufs[0].data_ptr() + 4 * GUARD,
                                           fbufs[1].data_ptr() + 4 * GUARD), "resample_rgb8")
    s = scratch.cpu().numpy()
    assert np.all(s[:GUARD] == fill) and np.all(s[GUARD + nscratch:] == fill)
    b8 = bufs[0].cpu().numpy()
    assert np.all(b8[:GUARD] == fill) and np.all(b8[GUARD + n8:] == fill)
    floats = []
    for f in fbufs:
        f = f.cpu().numpy()
        assert np.all(f[:GUARD] == f[0]) and np.all(f[GUARD + n8:] == f[0]) and f[0] > 1e30
        floats.append(f[GUARD:GUARD + n8].reshape(N, 3, h, w))
    return b8[GUARD:GUARD + n8].reshape(N, h, w, 3), floats[0], floats[1]


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def torch_unit(rgb8: np.ndarray) -> np.ndarray:
    """PILtoTorch's conversion (reference utils/general_utils.py:21-27) of one [h,w,3] image"""
    return (torch.from_numpy(rgb8).permute(2, 0, 1) / 255.0).numpy()


def torch_normalized(rgb8: np.ndarray) -> np.ndarray:
    """ToTensor, then Normalize((.5,.5,.5), (.5,.5,.5))"""
    return torch.from_numpy(rgb8).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5).numpy()


def check_raw_call_stays_inside_its_buffers(dev):
    for case in ("both passes, odd sizes", "horizontal pass skipped", "vertical pass skipped", "upscaling from 1x1", "copy"):
        H, W, Wo, Ho, name = CASES[case]
        stack = inputs(2, H, W)["binary"]
        windows = [None] if case != "both passes, odd sizes" else [None, (3, 2, 5, 7)]
        for window in windows:
            rgb8, unit, normalized = raw_call(dev, stack, (Wo, Ho), name, window)
            x0, y0, w, h = window or (0, 0, Wo, Ho)
            for i in range(2):
                want = pil_resize(stack[i], (Wo, Ho), name)[y0:y0 + h, x0:x0 + w]
                assert np.array_equal(rgb8[i], want), (case, window, i)
                assert same_bits(unit[i], torch_unit(want)) and same_bits(normalized[i], torch_normalized(want)), (case, window, i)


# ---------------------------------------------------------------------------------------------------- 3. windows
def windows_of(Wo, Ho):
    return [(0, 0, Wo, Ho), (0, 0, 1, 1), (Wo - 1, 0, 1, 1), (0, Ho - 1, 1, 1), (Wo - 1, Ho - 1, 1, 1), (3, 1, min(Wo - 4, 11), min(Ho - 2, 7))]


def check_windows(dev, case):
    H, W, Wo, Ho, name = CASES[case]
    for label, stack in inputs(2, H, W, seed=1).items():
        full = np.stack([pil_resize(f, (Wo, Ho), name) for f in stack])
        for x0, y0, w, h in windows_of(Wo, Ho):
            assert x0 % 2 == 1 or (w, h) in ((1, 1), (Wo, Ho))
            got = device_resize(dev, stack, (Wo, Ho), name, window=(x0, y0, w, h)).cpu().numpy()
            assert got.shape == (2, h, w, 3) and np.array_equal(got, full[:, y0:y0 + h, x0:x0 + w]), (case, label, (x0, y0, w, h))


# ---------------------------------------------------------------------------------------------------- 4. float outputs
def check_float_outputs(dev):
    every = (np.arange(256, dtype=np.uint8).reshape(16, 16)[..., None] + np.array([0, 85, 170], np.uint8)).astype(np.uint8)   # all 256 values per channel
    assert all(len(np.unique(every[..., c])) == 256 for c in range(3))
    sources = [("all byte values, copied", every[None], (16, 16), "bicubic", None)]
    for case in ("both passes, odd sizes", "upscaling", "vertical pass skipped"):
        H, W, Wo, Ho, name = CASES[case]
        for label, stack in inputs(2, H, W, seed=2).items():
            sources.append((f"{case} {label}", stack, (Wo, Ho), name, None))
    H, W, Wo, Ho, name = CASES["both passes, odd sizes"]
    sources.append(("window", inputs(2, H, W, seed=3)["noise"], (Wo, Ho), name, (3, 1, 11, 7)))
    for label, stack, size, name, window in sources:
        rgb8, unit, normalized = device_resize(dev, stack, size, name, window=window, out=("rgb8", "unit", "normalized"))
        assert unit.dtype == torch.float32 and normalized.dtype == torch.float32
        alone = device_resize(dev, stack, size, name, window=window, out="normalized")
        assert torch.equal(alone, normalized), label
        x0, y0, w, h = window or (0, 0) + tuple(size)
        for i in range(len(stack)):
            want = pil_resize(stack[i], size, name)[y0:y0 + h, x0:x0 + w]
            assert np.array_equal(rgb8[i].cpu().numpy(), want), (label, i)
            assert same_bits(unit[i].cpu().numpy(), torch_unit(want)), (label, i)
            assert same_bits(normalized[i].cpu().numpy(), torch_normalized(want)), (label, i)
    single = device_resize(dev, every, (7, 5), "lanczos", out="unit")   # [H,W,3] in -> no leading N out
    assert tuple(single.shape) == (3, 5, 7) and same_bits(single.cpu().numpy(), torch_unit(pil_resize(every, (7, 5), "lanczos")))


# ---------------------------------------------------------------------------------------------------- 5. load_images
def pil_load_images(folder_or_list, size, square_ok=False):
    """The reference's load_images (utils/sfm_utils.py:123-176) with PIL doing resize and crop and torch the normalisation"""
    from PIL.ImageOps import exif_transpose
    root, names = (folder_or_list, sorted(os.listdir(folder_or_list))) if isinstance(folder_or_list, str) else ("", folder_or_list)
    out = []
    for name in names:
        if not name.lower().endswith((".jpg", ".jpeg", ".png")):
            continue
        img = exif_transpose(Image.open(os.path.join(root, name))).convert("RGB")
        W1, H1 = img.size
        long_edge = round(size * max(W1 / H1, H1 / W1)) if size == 224 else size
        S = max(img.size)
        img = img.resize(tuple(int(round(x * long_edge / S)) for x in img.size), Image.LANCZOS if S > long_edge else Image.BICUBIC)
        W, H = img.size
        cx, cy = W // 2, H // 2
        if size == 224:
            half = min(cx, cy)
            img = img.crop((cx - half, cy - half, cx + half, cy + half))
        else:
            halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
            if not square_ok and W == H:
                halfh = 3 * halfw / 4
            img = img.crop((cx - halfw, cy - halfh, cx + halfw, cy + halfh))
        out.append(dict(img=torch.from_numpy(torch_normalized(np.array(img)))[None], true_shape=np.int32([img.size[::-1]]), idx=len(out),
                        instance=str(len(out))))
    return out, (W1, H1)


def assert_same_views(got, want, dev):
    (g_imgs, g_size), (w_imgs, w_size) = got, want
    assert tuple(g_size) == tuple(w_size) and len(g_imgs) == len(w_imgs)
    for g, w in zip(g_imgs, w_imgs):
        assert set(g) == {"img", "true_shape", "idx", "instance"}
        assert g["img"].device.type == dev.type and g["img"].dtype == torch.float32 and tuple(g["img"].shape) == tuple(w["img"].shape)
        assert same_bits(g["img"].cpu().numpy(), w["img"].numpy()), g["idx"]
        assert g["true_shape"].dtype == np.int32 and np.array_equal(g["true_shape"], w["true_shape"])
        assert g["idx"] == w["idx"] and g["instance"] == w["instance"] and isinstance(g["instance"], str)


def check_load_images_art(dev, size):
    from instantsplat_amd.resample import load_images
    folder = os.path.join(GOLDEN, "sora_art")   # three frames and SHA256SUMS, which is skipped
    assert any(not n.endswith(".jpg") for n in os.listdir(folder))
    want = pil_load_images(folder, size)
    assert len(want[0]) == 3 and tuple(want[0][0]["img"].shape) == ((1, 3, 288, 512) if size == 512 else (1, 3, 224, 224))
    assert_same_views(load_images(folder, size, verbose=False, device=dev), want, dev)


SYNTHETIC = {"b_square.png": (96, 96), "a_portrait.png": (120, 70), "c_small.png": (20, 31), "d_square.png": (96, 96)}   # H, W


def write_synthetic_files(folder):
    """seeded noise as PNG files (lossless: the same pixels wherever they are written), and a file that is no image"""
    rng = np.random.default_rng(77)
    for name, (H, W) in SYNTHETIC.items():
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(str(folder), name))
    with open(os.path.join(str(folder), "notes.txt"), "w") as fh:
        fh.write("not an image\n")


def golden_cases(folder):
    """-> [(key, folder_or_list, size, square_ok)]: the calls tests/golden/load_images_vectors.npz records"""
    art = os.path.join(GOLDEN, "sora_art")
    listed = [os.path.join(str(folder), n) for n in ("c_small.png", "notes.txt", "a_portrait.png")]
    return [("art512", art, 512, False), ("art224", art, 224, False), ("syn64", str(folder), 64, False), ("syn64sq", str(folder), 64, True),
            ("syn224", str(folder), 224, False), ("list64", listed, 64, False)]


def check_golden_load_images(dev, tmp_path):
    """against what the reference's own load_images returned (tests/golden/make_golden_load_images.py)"""
    import hashlib
    from instantsplat_amd.resample import load_images
    gold = np.load(os.path.join(GOLDEN, "load_images_vectors.npz"))
    write_synthetic_files(tmp_path)
    for key, arg, size, square_ok in golden_cases(tmp_path):
        imgs, last = load_images(arg, size, square_ok=square_ok, verbose=False, device=dev)
        assert tuple(last) == tuple(gold[f"li_{key}_last_size"]), key
        assert np.array_equal(np.concatenate([v["true_shape"] for v in imgs]), gold[f"li_{key}_shapes"]), key
        assert [v["idx"] for v in imgs] == gold[f"li_{key}_idx"].tolist() and [v["instance"] for v in imgs] == gold[f"li_{key}_instance"].tolist()
        for v, want in zip(imgs, gold[f"li_{key}_sha256"]):
            assert v["img"].dtype == torch.float32 and tuple(v["img"].shape[:2]) == (1, 3)
            assert hashlib.sha256(v["img"].cpu().contiguous().numpy().tobytes()).hexdigest() == str(want), (key, v["idx"])


def check_load_images_synthetic(dev, tmp_path, capsys):
    from instantsplat_amd.resample import load_images
    write_synthetic_files(tmp_path)
    folder = str(tmp_path)
    for size, square_ok in ((64, False), (64, True), (224, False)):
        want = pil_load_images(folder, size, square_ok)
        assert len(want[0]) == 4
        assert_same_views(load_images(folder, size, square_ok=square_ok, verbose=False, device=dev), want, dev)
    square = pil_load_images(folder, 64)[0][1]
    assert tuple(square["true_shape"][0]) == (48, 64)   # the 3:4 crop of a square image
    assert tuple(pil_load_images(folder, 64)[0][2]["true_shape"][0]) == (32, 64)   # 20x31 upscaled (BICUBIC) to 41x64, cropped
    listed = [os.path.join(folder, n) for n in ("c_small.png", "notes.txt", "a_portrait.png")]   # list form: the given order
    assert_same_views(load_images(listed, 64, verbose=False, device=dev), pil_load_images(listed, 64), dev)
    capsys.readouterr()
    load_images(listed, 64, device=dev)
    said = capsys.readouterr().out
    assert ">> Loading a list of 3 images" in said and "with resolution 31x20 --> 64x32" in said and "(Found 2 images)" in said
    with pytest.raises(AssertionError):
        load_images([os.path.join(folder, "notes.txt")], 64, verbose=False, device=dev)
    with pytest.raises(ValueError):
        load_images(("a.png",), 64, device=dev)


# ---------------------------------------------------------------------------------------------------- 6. load_cam
def check_load_cam(dev):
    from instantsplat_amd.scene_io import CameraInfo, load_cam
    rng = np.random.default_rng(9)

    def info(img):
        return CameraInfo(uid=4, R=np.eye(3), T=np.array([0.1, -0.2, 2.0]), FovY=0.8, FovX=1.1, image=img, image_path="x.png", image_name="x",
                          width=img.size[0], height=img.size[1])
    rgb = Image.fromarray(rng.integers(0, 256, (75, 106, 3), dtype=np.uint8))
    for resolution in (2, 4, 40, 1):
        a = load_cam(info(rgb), 0, resolution, device=dev)
        b = load_cam(info(rgb), 0, resolution, device=dev, resize="device")
        assert (a.image_width, a.image_height) == (b.image_width, b.image_height)
        assert a.original_image.dtype == b.original_image.dtype == torch.float32 and b.original_image.device.type == dev.type
        assert tuple(a.original_image.shape) == tuple(b.original_image.shape) == (3, a.image_height, a.image_width)
        assert same_bits(a.original_image.cpu().numpy(), b.original_image.cpu().numpy()), resolution
    assert (a.image_width, a.image_height) == (106, 75)   # -r 1: no resampling
    grey = Image.fromarray(rng.integers(0, 256, (20, 30), dtype=np.uint8))
    assert tuple(load_cam(info(grey), 0, 2, device=dev).original_image.shape) == (1, 10, 15)   # the default takes it, as before
    with pytest.raises(ValueError, match="RGB"):
        load_cam(info(grey), 0, 2, device=dev, resize="device")
    with pytest.raises(ValueError, match="resize"):
        load_cam(info(rgb), 0, 2, device=dev, resize="gpu")


# ---------------------------------------------------------------------------------------------------- 7. refusals
def check_python_refusals(dev):
    from instantsplat_amd.resample import resize_rgb8
    ok = torch.zeros(2, 6, 5, 3, dtype=torch.uint8, device=dev)
    for bad in (ok.float(), torch.zeros(2, 6, 5, 4, dtype=torch.uint8, device=dev), ok[None], ok[0, 0], ok.cpu().numpy(), ok[:, :, ::2]):
        with pytest.raises(ValueError):
            resize_rgb8(bad, (3, 3))
    for kw in (dict(size=(0, 3)), dict(size=(3, 0)), dict(size=(3, -1)), dict(size=3), dict(size=(3, 3), resample="box"),
               dict(size=(3, 3), resample=0), dict(size=(3, 3), out="float"), dict(size=(3, 3), out=()), dict(size=(3, 3), out=("unit", "unit")),
               dict(size=(3, 4), window=(0, 0, 4, 4)), dict(size=(3, 4), window=(0, 0, 3, 5)), dict(size=(3, 4), window=(2, 0, 2, 1)),
               dict(size=(3, 4), window=(-1, 0, 2, 2)), dict(size=(3, 4), window=(0, 0, 0, 2)), dict(size=(3, 4), window=(0, 0, 2)),
               dict(size=(70000, 4))):
        with pytest.raises(ValueError):
            resize_rgb8(ok, **kw)
    empty = resize_rgb8(ok[:0], (3, 4), out="unit")
    assert tuple(empty.shape) == (0, 3, 4, 3)


def check_entry_point_rejects_bad_arguments():
    """before any HIP call: the bogus device pointers are never touched"""
    from instantsplat_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)

    def run(N=2, H=8, W=9, Ho=4, Wo=5, images=fake, kx=fake, bx=fake, ksx=7, ky=fake, by=fake, ksy=7, x0=0, y0=0, w=5, h=4, row0=0, rows=8,
            scratch=fake, rgb8=fake, unit=None, normalized=None):
        return L.mi355gs_resample_rgb8(None, N, H, W, Ho, Wo, images, kx, bx, ksx, ky, by, ksy, x0, y0, w, h, row0, rows, scratch, rgb8, unit,
                                       normalized)
    bad = (dict(N=0), dict(N=65536), dict(H=0), dict(W=-1), dict(Ho=0), dict(Wo=0), dict(H=65536), dict(H=40000, W=40000), dict(images=None),
           dict(rgb8=None), dict(bx=None), dict(by=None), dict(ksx=0), dict(ksy=-1), dict(kx=None), dict(ky=None), dict(x0=-1), dict(y0=-1),
           dict(w=0), dict(h=0), dict(w=6), dict(h=5), dict(x0=1), dict(y0=1), dict(scratch=None), dict(row0=-1), dict(rows=0), dict(rows=9),
           dict(row0=1))
    for kw in bad:
        assert run(**kw) == EINVAL, kw
    for args in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (65536, 4, 4), (1, 65536, 4), (1, 40000, 40000)):
        assert L.mi355gs_resample_rgb8_scratch_bytes(*args) == 0, args
    assert L.mi355gs_resample_rgb8_scratch_bytes(3, 7, 5) >= 3 * 7 * 5 * 3 and L.mi355gs_resample_rgb8_scratch_bytes(1, 65535, 8) > 0
