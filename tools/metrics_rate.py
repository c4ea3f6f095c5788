"""Scoring rate of 8-bit frame sets (PSNR + SSIM per pair), two sets:
  * path:  the 201 frames of the interpolated path of the C3 scene (196,608 Gaussians, 512x512) from render_pose_path, each frame
           scored against its neighbour (frames[1:] vs frames[:-1], 200 pairs);
  * 1080p: 12 pairs of 1080x1920 frames (seeded bytes, the second of a pair the first plus noise in +-3);
two forms:
  (a) eager: per pair the uint8 -> float planar conversion (permute, float, div by 255: a copy at 4x the bytes), loss_utils.ssim
      under no_grad, train.psnr, and both .item() reads — what the package offered before metrics.image_metrics_rgb8;
  (b) fused: ONE image_metrics_rgb8 call for the set, its read-back included.
Each is warmed up, then timed --reps times in one process with a synchronize before every reading of the clock; the medians and
every repetition are reported.  Prints one JSON line.
  --fused-only   warm-up and ONE fused call per set (for `rocprofv3 --kernel-trace --stats`)
Measurement helper, not product code."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--train", type=int, default=200, help="one-call training iterations before the path is rendered")
ap.add_argument("--fused-only", action="store_true")
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from instantsplat_amd import train  # noqa: E402
from instantsplat_amd.arguments import OptimizationParams  # noqa: E402
from instantsplat_amd.camera_path import interpolated_pose_path  # noqa: E402
from instantsplat_amd.loss_utils import ssim  # noqa: E402
from instantsplat_amd.metrics import image_metrics_rgb8  # noqa: E402
from instantsplat_amd.pose_tracking import freeze_gaussians  # noqa: E402
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
freeze_gaussians(st.gaussians)
org = np.stack([c.world_view_transform.t().double().cpu().numpy() for c in st.cameras])
cams = [copy.copy(c) for c in st.cameras]
for c in cams:
    c.original_image = None
views = load_cameras(interpolated_pose_path(org, 3), cams)
frames = render_pose_path(views, st.gaussians, st.pipe, st.background)["frames"]
assert tuple(frames.shape) == (201, 512, 512, 3) and frames.device == dev

gen = torch.Generator().manual_seed(0)
big_gt = torch.randint(0, 256, (12, 1080, 1920, 3), generator=gen, dtype=torch.uint8)
big = (big_gt.to(torch.int16) + torch.randint(-3, 4, big_gt.shape, generator=gen, dtype=torch.int16)).clamp_(0, 255).to(torch.uint8)
SETS = {"path_512x512": (frames[1:], frames[:-1]), "pairs_1080x1920": (big.to(dev), big_gt.to(dev))}


def eager(renders, gts):
    ps, ss = [], []
    with torch.no_grad():
        for r, g in zip(renders, gts):
            x = r.permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0)
            y = g.permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0)
            ss.append(ssim(x, y).item())
            ps.append(train.psnr(x, y).item())
    return np.array(ps), np.array(ss, dtype=np.float32)


def fused(renders, gts):
    m = image_metrics_rgb8(renders, gts)
    return m["psnr"], m["ssim"]


def timed(fn, renders, gts):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(renders, gts)
    torch.cuda.synchronize()
    return int(renders.shape[0]) / (time.perf_counter() - t0), out


if a.fused_only:
    out = {}
    for name, (r, g) in SETS.items():
        fused(r, g)
        out[name] = {"pairs": int(r.shape[0]), "pairs_per_s_fused_single_run": timed(fused, r, g)[0]}
    print(json.dumps(out), flush=True)
    sys.exit(0)

out = {"scene": "C3", "gaussians": int(st.gaussians._xyz.shape[0]), "trained_iterations": a.train, "reps": a.reps, "sets": {}}
for name, (r, g) in SETS.items():
    (pe, se), (pf, sf) = eager(r, g), fused(r, g)   # warm-up, and the two forms must agree
    finite = np.isfinite(pe) & np.isfinite(pf)
    rates = {"eager": [], "fused": []}
    for _ in range(a.reps):
        for form, fn in (("eager", eager), ("fused", fused)):
            rates[form].append(timed(fn, r, g)[0])
    me, mf = statistics.median(rates["eager"]), statistics.median(rates["fused"])
    out["sets"][name] = {"pairs": int(r.shape[0]), "H": int(r.shape[1]), "W": int(r.shape[2]),
                         "max_abs_psnr_difference_db": float(np.abs(pe[finite] - pf[finite]).max()) if finite.any() else 0.0,
                         "max_abs_ssim_difference": float(np.abs(se.astype(np.float64) - sf.astype(np.float64)).max()),
                         "pairs_per_s_eager": me, "pairs_per_s_eager_runs": rates["eager"],
                         "pairs_per_s_fused": mf, "pairs_per_s_fused_runs": rates["fused"],
                         "ms_per_pair_eager": 1e3 / me, "ms_per_pair_fused": 1e3 / mf, "speedup": mf / me}
print(json.dumps(out), flush=True)
