"""Resizing rate of the network's input stage (instantsplat_amd/resample.py), LANCZOS, `normalized` output, two sets:
  * art3_1280x720:     the three 1280x720 example frames (tests/golden/sora_art) -> 512x288, what load_images(size=512) does to them;
  * photos12_3024x4032: 12 synthetic 12-megapixel portrait photographs (W 3024, H 4032; seeded noise with a saturated region each)
                        -> 384x512;
four forms, siblings of one run:
  (a) pil:      per image `Image.fromarray(a).resize(size, LANCZOS)` and the normalisation to [-1, 1] in torch, on one host thread,
                the image already decoded (the path without this stage); the resize alone is reported too;
  (b) upload:   ONE resize_rgb8 call for the set, the copy of the bytes from pinned host memory included;
  (c) resident: ONE resize_rgb8 call for the set, the bytes already in device memory;
  (d) library:  the bare mi355gs_resample_rgb8 call between two device events (tables and buffers made beforehand).
Each is warmed up, then timed --reps times in one process with a synchronize before every reading of the clock; the medians and every
repetition are reported, with the algorithmic bytes of the call (source read once, intermediate written and read once, floats
written once) and whether the device's bytes equal PIL's on every image.  Prints one JSON line and, with --out, writes it to a file.
  --fused-only   warm-up and ONE resident call per set (for `rocprofv3 --kernel-trace --stats`, in a run of its own)
Measurement helper, not product code."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fused-only", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from instantsplat_amd import _lib  # noqa: E402
from instantsplat_amd.resample import _device_tables, resize_rgb8  # noqa: E402

dev = torch.device("cuda:0")
FILTER = "lanczos"


def art_frames():
    folder = os.path.join(ROOT, "tests", "golden", "sora_art")
    names = sorted(n for n in os.listdir(folder) if n.endswith(".jpg"))
    return np.stack([np.asarray(Image.open(os.path.join(folder, n)).convert("RGB")) for n in names])


def photos(n=12, H=4032, W=3024):
    rng = np.random.default_rng(18)
    out = np.empty((n, H, W, 3), np.uint8)
    for i in range(n):
        out[i] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        out[i, 1000:2000, 500:2500] = (rng.integers(0, 2, (1000, 2000, 3)) * 255).astype(np.uint8)
    return out


SETS = {"art3_1280x720": (art_frames(), (512, 288)), "photos12_3024x4032": (photos(), (384, 512))}


def pil_leg(images, size, normalize=True):
    out = []
    for im in images:
        r = np.array(Image.fromarray(im).resize(size, Image.LANCZOS))
        out.append(torch.from_numpy(r).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5) if normalize else r)
    return out


def device_leg(source, size):
    """source: pinned host tensor (upload included) or device tensor -> seconds, result"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = resize_rgb8(source.to(dev, non_blocking=True), size, resample=FILTER, out="normalized")
    torch.cuda.synchronize()
    return time.perf_counter() - t0, got


def library_leg(resident, size):
    """the bare entry point under device events -> ms"""
    L = _lib.lib()
    N, H, W = (int(s) for s in resident.shape[:3])
    Wo, Ho = size
    kx, bx, _ = _device_tables(W, Wo, FILTER, dev)
    ky, by, host = _device_tables(H, Ho, FILTER, dev)
    row0, rows = int(host[0, 0]), int(host[-1, 0] + host[-1, 1]) - int(host[0, 0])
    scratch = torch.empty(int(L.mi355gs_resample_rgb8_scratch_bytes(N, rows, Wo)), dtype=torch.uint8, device=dev)
    out = torch.empty((N, 3, Ho, Wo), dtype=torch.float32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(L.mi355gs_resample_rgb8(_lib.stream_ptr(dev), N, H, W, Ho, Wo, resident.data_ptr(), kx.data_ptr(), bx.data_ptr(), int(kx.shape[1]),
                                       ky.data_ptr(), by.data_ptr(), int(ky.shape[1]), 0, 0, Wo, Ho, row0, rows, scratch.data_ptr(), None, None,
                                       out.data_ptr()), "resample_rgb8")
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


if a.fused_only:
    rec = {}
    for name, (images, size) in SETS.items():
        resident = torch.from_numpy(images).to(dev)
        device_leg(resident, size)
        rec[name] = {"images": int(images.shape[0]), "ms_resident_single_run": 1e3 * device_leg(resident, size)[0]}
    print(json.dumps(rec), flush=True)
    sys.exit(0)

rec = {"filter": FILTER, "output": "normalized", "reps": a.reps, "pil_version": Image.__version__, "sets": {}}
for name, (images, size) in SETS.items():
    N, H, W = (int(s) for s in images.shape[:3])
    Wo, Ho = size
    pinned = torch.from_numpy(images).pin_memory()
    resident = pinned.to(dev)
    want = pil_leg(images, size, normalize=False)   # warm-up
    pil_leg(images[:1], size)
    device_leg(pinned, size)
    _, got = device_leg(resident, size)
    library_leg(resident, size)
    bytes8 = resize_rgb8(resident, size, resample=FILTER).cpu().numpy()
    equal = [bool(np.array_equal(bytes8[i], want[i])) for i in range(N)]
    want_f = pil_leg(images, size)
    equal_f = [bool(torch.equal(got[i].cpu(), want_f[i])) for i in range(N)]
    runs = {"pil_ms_per_image": [], "pil_resize_only_ms_per_image": [], "upload_ms": [], "resident_ms": [], "library_ms": []}
    for _ in range(a.reps):
        t0 = time.perf_counter()
        pil_leg(images, size)
        runs["pil_ms_per_image"].append(1e3 * (time.perf_counter() - t0) / N)
        t0 = time.perf_counter()
        pil_leg(images, size, normalize=False)
        runs["pil_resize_only_ms_per_image"].append(1e3 * (time.perf_counter() - t0) / N)
        runs["upload_ms"].append(1e3 * device_leg(pinned, size)[0])
        runs["resident_ms"].append(1e3 * device_leg(resident, size)[0])
        runs["library_ms"].append(library_leg(resident, size))
    med = {k: statistics.median(v) for k, v in runs.items()}
    # the call's algorithmic bytes: every source byte once, the 8-bit intermediate (all H rows x Wo columns) written and read, floats out
    alg = N * (3 * H * W + 2 * 3 * H * Wo + 4 * 3 * Ho * Wo)
    rec["sets"][name] = {
        "images": N, "H": H, "W": W, "Hout": Ho, "Wout": Wo, "source_bytes": N * 3 * H * W, "algorithmic_bytes": alg,
        "device_bytes_equal_pil": all(equal), "device_floats_equal_torch": all(equal_f),
        "pil_ms_per_image": med["pil_ms_per_image"], "pil_ms_per_image_runs": runs["pil_ms_per_image"],
        "pil_resize_only_ms_per_image": med["pil_resize_only_ms_per_image"], "pil_resize_only_ms_per_image_runs": runs["pil_resize_only_ms_per_image"],
        "upload_ms_per_set": med["upload_ms"], "upload_ms_per_set_runs": runs["upload_ms"],
        "resident_ms_per_set": med["resident_ms"], "resident_ms_per_set_runs": runs["resident_ms"],
        "library_ms_per_set": med["library_ms"], "library_ms_per_set_runs": runs["library_ms"],
        "upload_ms_per_image": med["upload_ms"] / N, "resident_ms_per_image": med["resident_ms"] / N, "library_ms_per_image": med["library_ms"] / N,
        "library_algorithmic_GB_per_s": alg / (1e6 * med["library_ms"]), "upload_source_GB_per_s": N * 3 * H * W / (1e6 * med["upload_ms"]),
        "pil_over_upload_time_per_image": med["pil_ms_per_image"] / (med["upload_ms"] / N),
        "pil_over_resident_time_per_image": med["pil_ms_per_image"] / (med["resident_ms"] / N)}
line = json.dumps(rec)
print(line, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
