"""Time of the global alignment loop at the two sizes the reference runs it at, 3 x 512 x 288 (6 edges, 300 iterations:
init_geo.py:48) and 15 x 512 x 288 (210 edges, 500 iterations: init_test_pose.py:59), on synthetic problems generated on the
device (the scene of tests/global_align_util.py's generator, in torch), two forms on the same device:
  (a) eager: the torch restatement of the reference's loop (global_align_util.restatement_run in float32: forward, autograd,
      torch.optim.Adam — a few dozen elementwise launches per iteration);
  (b) fused: ONE global_align.global_alignment call (1 + 3 niter kernel dispatches, its read of the last loss included).
Each is warmed up (a short run), then timed --reps times from the same start, with a synchronize before every reading of the
clock; the medians and every repetition are reported, and the two forms must land together (both losses fall; the final ones within 2 %,
their relative difference in the record — the tests, not this tool, hold the arithmetic to its tolerance).  Prints one JSON
line and, with --out, writes it.
  --fused-only   warm-up and ONE fused call per size (for `rocprofv3 --kernel-trace --stats`)
  --sizes        comma-separated subset of v3,v15
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--fused-only", action="store_true")
ap.add_argument("--sizes", default="v3,v15")
ap.add_argument("--out", default=None)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from instantsplat_amd.global_align import AlignProblem, AlignState, global_alignment  # noqa: E402
from tests import global_align_util as gu  # noqa: E402

dev = torch.device("cuda:0")
H, W = 288, 512
SETS = {"v3": (3, 300), "v15": (15, 500)}


def scene(V, seed):
    """global_align_util.synthetic_problem's scene at full size, formed on the device in float32"""
    g = torch.Generator(device=dev).manual_seed(seed)
    edges = [(i, j) for i in range(V) for j in range(V) if i != j]
    E, n = len(edges), H * W
    focal = 1.2 * max(H, W)
    rows = torch.arange(H, device=dev, dtype=torch.float32).repeat_interleave(W)
    cols = torch.arange(W, device=dev, dtype=torch.float32).repeat(H)
    R, T, X, depth, quat = [], [], [], [], []
    for v in range(V):
        ang, tilt = 0.12 * (v - (V - 1) / 2) + 0.05, 0.02 * (v + 1)
        ca, sa, ct, st = np.cos(ang), np.sin(ang), np.cos(tilt), np.sin(tilt)
        Rv = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]])
        Tv = np.array([-2.5 * sa, 0.05 * v, 2.5 * (1 - ca)]) + 0.3
        d = 2.0 + 0.3 * torch.sin(3.0 * cols / W + v) * torch.cos(2.0 * rows / H) + 0.1 * cols / W
        c = torch.stack([d * (cols - W / 2) / focal, d * (rows - H / 2) / focal, d], dim=1)
        Rt, Tt = torch.tensor(Rv, dtype=torch.float32, device=dev), torch.tensor(Tv, dtype=torch.float32, device=dev)
        R.append(Rt); T.append(Tt); depth.append(d); X.append(c @ Rt.T + Tt); quat.append(gu._rotmat_to_quat(Rv))
    delta = np.random.default_rng(seed).normal(0, 0.2, E)
    sigma = 0.5 * np.exp(delta - delta.mean())
    pred_i = torch.empty(E, n, 3, device=dev)
    pred_j = torch.empty(E, n, 3, device=dev)
    pw = np.zeros((E, 8))
    for e, (i, j) in enumerate(edges):
        pred_i[e] = ((X[i] - T[i]) @ R[i]) / float(sigma[e])
        pred_j[e] = ((X[j] - T[i]) @ R[i]) / float(sigma[e])
        pw[e, :4], pw[e, 4:7], pw[e, 7] = quat[i], gu._signed_log1p(T[i].cpu().numpy().astype(np.float64) / sigma[e]), np.log(sigma[e] / 0.5)
    pred_i += 0.01 * torch.randn(pred_i.shape, device=dev, generator=g)
    pred_j += 0.01 * torch.randn(pred_j.shape, device=dev, generator=g)
    conf_i = 1 + 3 * torch.rand(E, n, device=dev, generator=g)
    conf_j = 1 + 3 * torch.rand(E, n, device=dev, generator=g)
    p = 0.02
    f32 = dict(dtype=torch.float32, device=dev)
    im_pose = np.stack([np.concatenate([quat[v], gu._signed_log1p(T[v].cpu().numpy().astype(np.float64))]) for v in range(V)])
    arrays = dict(pred_i=pred_i, pred_j=pred_j, conf_i=conf_i, conf_j=conf_j,
                  depth_log=torch.stack(depth).log() + p * torch.randn(V, n, device=dev, generator=g),
                  im_pose=torch.tensor(im_pose, **f32) + p * torch.randn(V, 7, device=dev, generator=g),
                  focal_log=torch.full((V,), 20 * np.log(focal), **f32) + 10 * p * torch.randn(V, device=dev, generator=g),
                  pp_raw=0.05 * torch.randn(V, 2, device=dev, generator=g),
                  pw_pose=torch.tensor(pw, **f32) + p * torch.randn(E, 8, device=dev, generator=g))
    return edges, arrays


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


out = {"H": H, "W": W, "reps": a.reps, "lr": gu.LR, "schedule": "cosine", "sets": {}}
for name in a.sizes.split(","):
    V, niter = SETS[name]
    edges, arrays = scene(V, 40 + V)
    E = len(edges)
    problem = AlignProblem(edges, arrays["pred_i"], arrays["pred_j"], arrays["conf_i"], arrays["conf_j"], H, W)

    def fused(iters=niter):
        state = AlignState(problem, *[arrays[k] for k in gu.STATE])
        return global_alignment(problem, state, niter=iters, lr=gu.LR)[1]

    def eager(iters=niter):
        return gu.restatement_run(edges, H, W, arrays, gu.ALL_ON, iters, torch.float32, checkpoints=(), dev=dev)[0]

    rec = {"views": V, "edges": E, "niter": niter, "residuals": 2 * E * H * W,
           "algorithmic_bytes_per_iteration": 32 * E * H * W + 24 * V * H * W}
    fused(5)   # warm-up
    if a.fused_only:
        ms, losses = timed(fused)
        rec.update(ms_fused_single_run=ms, loss_first=float(losses[0]), loss_last=float(losses[-1]))
        out["sets"][name] = rec
        continue
    eager(3)   # warm-up
    ms = {"eager": [], "fused": []}
    for _ in range(a.reps):
        t, le = timed(eager)
        ms["eager"].append(t)
        t, lf = timed(fused)
        ms["fused"].append(t)
    le, lf = le.cpu(), lf.cpu()
    diff = abs(float(le[-1]) - float(lf[-1])) / abs(float(le[-1]))
    assert diff <= 2e-2 and float(lf[-1]) < float(lf[0]) and float(le[-1]) < float(le[0]), (name, float(le[-1]), float(lf[-1]))
    me, mf = statistics.median(ms["eager"]), statistics.median(ms["fused"])
    rec.update(final_loss_rel_diff=diff, loss_first=float(lf[0]), loss_last_fused=float(lf[-1]), loss_last_eager=float(le[-1]), ms_eager=me, ms_eager_runs=ms["eager"],
               ms_fused=mf, ms_fused_runs=ms["fused"], us_per_iteration_eager=1e3 * me / niter, us_per_iteration_fused=1e3 * mf / niter,
               speedup=me / mf)
    out["sets"][name] = rec
    del problem, arrays
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
