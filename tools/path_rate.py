"""Camera-path rendering rate on the C3 scene (3 views, 196,608 Gaussians, 512x512) along the 201-pose interpolated path of its
three train poses — the reference's `render.py --infer_video` loop without the file writes:
  (a) eager: per frame a no-grad render(), the 8-bit conversion as a torch expression (x.mul(255).add_(0.5).clamp_(0, 255)
      .to(uint8), five elementwise launches with the permute's copy) and a blocking .cpu();
  (b) fused: one render_pose_path call (one library call for the whole path) including its one copy of the frames to the host;
  (c) fused_pinned (extra): the same call with pinned=True — the kernels store the frames into pinned host memory, no copy.
Each is warmed up, then timed --reps times in one process with a synchronize before every reading of the clock; the median is
reported.  Prints one JSON line.
  --fused-only        warm-up and ONE fused call (for `rocprofv3 --kernel-trace` of the loop)
  --trace-csv FILE    no GPU work: reads the kernel trace of such a run and adds the dispatch count per frame and the idle gaps
                      between consecutive dispatches of the call to the JSON line; --trimmed-out FILE keeps the call's rows
Measurement helper, not product code."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--train", type=int, default=200, help="one-call training iterations before rendering")
ap.add_argument("--fused-only", action="store_true")
ap.add_argument("--trace-csv")
ap.add_argument("--trimmed-out", help="with --trace-csv: write the timed call's dispatches (frame, kernel, start and end in ns from its first) here")
a = ap.parse_args()
N_FRAMES = 201


def trace_summary(path):
    """The last N_FRAMES conversion launches of the trace end the frames of the timed call (it reported no rerun): dispatches per
    frame = launches from one of them to the next; gap = start of a dispatch - end of the one before it, inside the call."""
    with open(path, newline="") as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    ends = [i for i, r in enumerate(rows) if "k_rgb8_from_planar" in r[0]]
    if len(ends) < N_FRAMES:
        raise SystemExit(f"{path}: {len(ends)} conversion launches, expected at least {N_FRAMES}")
    ends = ends[-N_FRAMES:]
    per_frame = [ends[k + 1] - ends[k] for k in range(N_FRAMES - 1)]
    call = rows[ends[0] - int(statistics.median(per_frame)) + 1: ends[-1] + 1]   # from the first frame's projection launch on
    gaps = [(call[k + 1][1] - call[k][2]) / 1e3 for k in range(len(call) - 1)]   # us
    short = lambda name: (re.search(r"\bk_\w+", name) or re.search(r"\w+", name)).group(0)
    m = int(statistics.median(per_frame))
    long_gaps = [{"frame": (k + 1) // m, "before": short(call[k + 1][0]), "us": round(gaps[k], 1)} for k in range(len(gaps)) if gaps[k] > 20.0]
    busy = sum(r[2] - r[1] for r in call) / 1e3
    if a.trimmed_out:
        with open(a.trimmed_out, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["frame", "kernel", "start_ns", "end_ns"])
            for k, r in enumerate(call):
                w.writerow([k // m, short(r[0]), r[1] - call[0][1], r[2] - call[0][1]])
    return {"dispatches_per_frame": statistics.median(per_frame), "dispatches_per_frame_min_max": [min(per_frame), max(per_frame)],
            "dispatches_of_last_frame": [short(r[0]) for r in rows[ends[-2] + 1: ends[-1] + 1]],
            "gap_us_median": statistics.median(gaps), "gap_us_p99": sorted(gaps)[int(0.99 * len(gaps))],
            "gap_us_max": max(gaps), "gaps_over_20us": long_gaps, "call_span_ms": (call[-1][2] - call[0][1]) / 1e6,
            "call_kernel_busy_ms": busy / 1e3}


if a.trace_csv:
    print(json.dumps({"trace": os.path.basename(a.trace_csv), **trace_summary(a.trace_csv)}), flush=True)
    sys.exit(0)

import copy  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from instantsplat_amd import train  # noqa: E402
from instantsplat_amd.arguments import OptimizationParams  # noqa: E402
from instantsplat_amd.camera_path import interpolated_pose_path  # noqa: E402
from instantsplat_amd.gaussian_renderer import render  # noqa: E402
from instantsplat_amd.pose_tracking import freeze_gaussians  # noqa: E402
from instantsplat_amd.pose_utils import get_tensor_from_camera  # noqa: E402
from instantsplat_amd.render_path import render_pose_path  # noqa: E402
from instantsplat_amd.scene_io import load_cameras  # noqa: E402
from instantsplat_amd.synthetic import syn_pointmap  # noqa: E402

dev = torch.device("cuda:0")
st = train.setup_training(syn_pointmap(3, 256, 256, 512, 512, seed=0), dev,
                          opt=OptimizationParams(iterations=10 ** 9, pp_optimizer=True, optim_pose=True))
for _ in range(a.train):
    train.train_iteration(st, fused_step=True)
train.release_trainer(st)
torch.cuda.synchronize()
g = st.gaussians
freeze_gaussians(g)
org = np.stack([c.world_view_transform.t().double().cpu().numpy() for c in st.cameras])
cams = [copy.copy(c) for c in st.cameras]
for c in cams:
    c.original_image = None
views = load_cameras(interpolated_pose_path(org, 3), cams)
assert len(views) == N_FRAMES
poses = torch.stack([get_tensor_from_camera(v.world_view_transform.transpose(0, 1).cpu()) for v in views]).to(dev)


def eager():
    out = []
    with torch.no_grad():
        for i, view in enumerate(views):
            img = render(view, g, st.pipe, st.background, camera_pose=poses[i])["render"]
            out.append(img.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).cpu())
    return torch.stack(out)


RERUNS = []


def fused():
    res = render_pose_path(views, g, st.pipe, st.background, poses=poses)
    RERUNS.append(res["reruns"])
    return res["frames"].cpu()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return N_FRAMES / (time.perf_counter() - t0), out


if a.fused_only:
    fused()
    reruns = []
    rate, frames = timed(lambda: reruns.append(render_pose_path(views, g, st.pipe, st.background, poses=poses)["reruns"]))
    print(json.dumps({"scene": "C3", "frames": N_FRAMES, "fps_fused_single_run_no_copy": rate, "reruns": reruns[0]}), flush=True)
    sys.exit(0)

def fused_pinned():
    return render_pose_path(views, g, st.pipe, st.background, poses=poses, pinned=True)["frames"]


ref, got, got_pinned = eager(), fused(), fused_pinned()   # warm-up, and the loops must agree
same = bool(torch.equal(ref, got)) and bool(torch.equal(ref, got_pinned))
del got_pinned   # (its pinned block goes back to torch's host allocator, which hands it to the next call)
rates = {"eager": [], "fused": [], "fused_pinned": []}
for _ in range(a.reps):
    for name, fn in (("eager", eager), ("fused", fused), ("fused_pinned", fused_pinned)):
        rates[name].append(timed(fn)[0])
out = {"scene": "C3", "gaussians": int(g._xyz.shape[0]), "W": 512, "H": 512, "frames": N_FRAMES, "sh_degree": int(g.active_sh_degree),
       "trained_iterations": a.train, "reps": a.reps, "frames_identical": same, "frames_rendered_twice_per_call": max(RERUNS),
       "fps_eager": statistics.median(rates["eager"]), "fps_eager_runs": rates["eager"],
       "fps_fused": statistics.median(rates["fused"]), "fps_fused_runs": rates["fused"],
       "fps_fused_pinned": statistics.median(rates["fused_pinned"]), "fps_fused_pinned_runs": rates["fused_pinned"],
       "ms_per_frame_eager": 1e3 / statistics.median(rates["eager"]), "ms_per_frame_fused": 1e3 / statistics.median(rates["fused"]),
       "speedup": statistics.median(rates["fused"]) / statistics.median(rates["eager"])}
print(json.dumps(out), flush=True)
