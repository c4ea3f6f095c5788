"""JPEG encoding rate of 8-bit frame stacks at quality 90, both subsamplings, two sets:
  * path_1280x720:   the 201 frames of the interpolated path of the C3 scene (196,608 Gaussians) rendered at 1280x720 by
                     render_pose_path;
  * stack12_512x512: the first 12 frames of the same path rendered at 512x512;
three forms, siblings of one run:
  (a) pil:     per frame `Image.fromarray(frame).save(buffer, "JPEG", quality=90, subsampling=..., optimize=False,
               restart_marker_rows=1)` on one host thread, the frame already on the host; timed on --pil-frames frames spread
               evenly over the set, reported per frame;
  (b) device:  ONE jpeg.encode_jpeg_rgb8 call for the set, its read-back of the offsets and its copy of the files included;
  (c) library: the bare mi355gs_jpeg_rgb8 call between two device events (buffers allocated beforehand, the library's worst-case
               output size, nothing read back).
Each is warmed up, then timed --reps times in one process with a synchronize before every reading of the clock; the medians and
every repetition are reported, with the files' total bytes against raw and against the device PNG files of the same frames, and
whether the device's files equal PIL's on the frames PIL was given.  Prints one JSON line and, with --out, writes it to a file.
  --fused-only   warm-up and ONE device call per set and subsampling (for `rocprofv3 --kernel-trace --stats`, in a run of its own)
Measurement helper, not product code."""
import argparse
import copy
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--pil-frames", type=int, default=6, help="frames of a set PIL is timed on (spread evenly)")
ap.add_argument("--quality", type=int, default=90)
ap.add_argument("--fused-only", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from instantsplat_amd import _lib, train  # noqa: E402
from instantsplat_amd.camera_path import interpolated_pose_path  # noqa: E402
from instantsplat_amd.jpeg import SUBSAMPLINGS, encode_jpeg_rgb8, quant_tables  # noqa: E402
from instantsplat_amd.png import encode_png_rgb8  # noqa: E402
from instantsplat_amd.pose_tracking import freeze_gaussians  # noqa: E402
from instantsplat_amd.render_path import render_pose_path  # noqa: E402
from instantsplat_amd.scene_io import load_cameras  # noqa: E402
from instantsplat_amd.synthetic import syn_pointmap  # noqa: E402

dev = torch.device("cuda:0")


def path_frames(W, H, count=None):
    st = train.setup_training(syn_pointmap(3, 256, 256, W, H, seed=0), dev)
    freeze_gaussians(st.gaussians)
    org = np.stack([c.world_view_transform.t().double().cpu().numpy() for c in st.cameras])
    cams = [copy.copy(c) for c in st.cameras]
    for c in cams:
        c.original_image = None
    views = load_cameras(interpolated_pose_path(org, 3), cams)[:count]
    frames = render_pose_path(views, st.gaussians, st.pipe, st.background)["frames"]
    assert tuple(frames.shape) == (len(views), H, W, 3) and frames.device == dev
    return frames, int(st.gaussians._xyz.shape[0])


big, gaussians = path_frames(1280, 720)
small, _ = path_frames(512, 512, 12)
assert big.shape[0] == 201
SETS = {"path_1280x720": big, "stack12_512x512": small}


def pil_encode(host_frames, sub):
    files = []
    for f in host_frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=a.quality, subsampling=SUBSAMPLINGS[sub], optimize=False, restart_marker_rows=1)
        files.append(buf.getvalue())
    return files


def device_call(frames, sub):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enc = encode_jpeg_rgb8(frames, quality=a.quality, subsampling=sub)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, enc


def library_call(frames, sub):
    """the bare entry point under device events -> ms"""
    L = _lib.lib()
    N, H, W = (int(s) for s in frames.shape[:3])
    code = SUBSAMPLINGS[sub]
    qt = np.ascontiguousarray(quant_tables(a.quality))
    scratch = torch.empty(int(L.mi355gs_jpeg_rgb8_scratch_bytes(N, H, W, code)), dtype=torch.uint8, device=dev)
    out = torch.empty(int(L.mi355gs_jpeg_rgb8_stream_bytes(N, H, W, code)), dtype=torch.uint8, device=dev)
    offs = torch.empty(N + 1, dtype=torch.int64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(L.mi355gs_jpeg_rgb8(_lib.stream_ptr(dev), N, H, W, code, qt.ctypes.data, _lib.ptr(frames), _lib.ptr(scratch), _lib.ptr(out),
                                   out.numel(), _lib.ptr(offs)), "jpeg_rgb8")
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


if a.fused_only:
    rec = {}
    for name, frames in SETS.items():
        for sub in SUBSAMPLINGS:
            device_call(frames, sub)
            rec[f"{name} {sub}"] = {"frames": int(frames.shape[0]), "ms_device_single_run": 1e3 * device_call(frames, sub)[0]}
    print(json.dumps(rec), flush=True)
    sys.exit(0)

rec = {"scene": "C3 (untrained synthetic)", "gaussians": gaussians, "reps": a.reps, "quality": a.quality, "sets": {}}
for name, frames in SETS.items():
    N, H, W = (int(s) for s in frames.shape[:3])
    picks = sorted(set(np.linspace(0, N - 1, min(N, a.pil_frames)).astype(int).tolist()))
    host = [frames[i].cpu().numpy() for i in picks]
    png_bytes = int(encode_png_rgb8(frames)["offsets"][-1])
    for sub in SUBSAMPLINGS:
        pil_files = pil_encode(host, sub)   # warm-up
        _, enc = device_call(frames, sub)
        library_call(frames, sub)
        o = enc["offsets"]
        data = enc["stream"].numpy()
        equal = [data[int(o[i]):int(o[i + 1])].tobytes() == pil_files[k] for k, i in enumerate(picks)]
        runs = {"pil_ms_per_frame": [], "device_ms": [], "library_ms": []}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            pil_encode(host, sub)
            runs["pil_ms_per_frame"].append(1e3 * (time.perf_counter() - t0) / len(host))
            runs["device_ms"].append(1e3 * device_call(frames, sub)[0])
            runs["library_ms"].append(library_call(frames, sub))
        med = {k: statistics.median(v) for k, v in runs.items()}
        rec["sets"][f"{name} {sub}"] = {
            "frames": N, "H": H, "W": W, "subsampling": sub, "raw_bytes": N * H * W * 3, "device_bytes": int(o[-1]),
            "device_png_bytes": png_bytes, "device_over_raw_bytes": int(o[-1]) / (N * H * W * 3), "device_over_device_png_bytes": int(o[-1]) / png_bytes,
            "pil_frames": [int(i) for i in picks], "device_files_equal_pil_on_those": bool(all(equal)),
            "pil_ms_per_frame": med["pil_ms_per_frame"], "pil_ms_per_frame_runs": runs["pil_ms_per_frame"],
            "device_ms_per_set": med["device_ms"], "device_ms_per_set_runs": runs["device_ms"],
            "library_ms_per_set": med["library_ms"], "library_ms_per_set_runs": runs["library_ms"],
            "device_ms_per_frame": med["device_ms"] / N, "library_ms_per_frame": med["library_ms"] / N,
            "device_frames_per_s": 1e3 * N / med["device_ms"], "library_frames_per_s": 1e3 * N / med["library_ms"],
            "pil_over_device_time_per_frame": med["pil_ms_per_frame"] / (med["device_ms"] / N)}
line = json.dumps(rec)
print(line, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
