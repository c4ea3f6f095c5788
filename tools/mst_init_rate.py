"""Time of the aligner's initialisation at the two sizes the reference runs it at, 3 x 512 x 288 (6 edges) and 15 x 512 x 288
(210 edges), on synthetic problems generated on the device, two forms on the same device:
  (a) eager: the float32 torch restatement of the reference (tests/mst_init_util.restate_init with the library's default pose
      rule: E + V - 1 registrations, one after the other, each with a 3 x 3 SVD and the host round trips torch.linalg makes);
  (b) fused: ONE global_align.init_minimum_spanning_tree call, default pose mode, its one read-back included.
Each is warmed up, then timed --reps times with a synchronize before every reading of the clock; medians and every repetition
are reported.  Per stage (device events around the library's own entry points, same buffers): the confidence means, the batched
pair registration (with its achieved bytes/s: two passes over E n points of 16 + 12 + 4 bytes), the focals, the state kernels.
The gate: the fused call is faster than the restatement at both sizes.  Prints one JSON line and, with --out, writes it.
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
ap.add_argument("--sizes", default="v3,v15")
ap.add_argument("--out", default=None)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from instantsplat_amd import _lib  # noqa: E402
from instantsplat_amd import global_align as ga  # noqa: E402
from tests import mst_init_util as mu  # noqa: E402

dev = torch.device("cuda:0")
H, W = 288, 512
SETS = {"v3": 3, "v15": 15}


def scene(V, seed):
    """tests/global_align_util.synthetic_problem's scene at full size, formed on the device in float32; the confidences of edge e
    are scaled by 1.01^k, k a permutation of the edges, so that no two scores come close"""
    g = torch.Generator(device=dev).manual_seed(seed)
    edges = [(i, j) for i in range(V) for j in range(V) if i != j]
    E, n = len(edges), H * W
    focal = 1.2 * max(H, W)
    rows = torch.arange(H, device=dev, dtype=torch.float32).repeat_interleave(W)
    cols = torch.arange(W, device=dev, dtype=torch.float32).repeat(H)
    R, T, X = [], [], []
    for v in range(V):
        ang, tilt = 0.12 * (v - (V - 1) / 2) + 0.05, 0.02 * (v + 1)
        ca, sa, ct, st = np.cos(ang), np.sin(ang), np.cos(tilt), np.sin(tilt)
        Rv = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]])
        Tv = np.array([-2.5 * sa, 0.05 * v, 2.5 * (1 - ca)]) + 0.3
        d = 2.0 + 0.3 * torch.sin(3.0 * cols / W + v) * torch.cos(2.0 * rows / H) + 0.1 * cols / W
        c = torch.stack([d * (cols - W / 2) / focal, d * (rows - H / 2) / focal, d], dim=1)
        Rt, Tt = torch.tensor(Rv, dtype=torch.float32, device=dev), torch.tensor(Tv, dtype=torch.float32, device=dev)
        R.append(Rt); T.append(Tt); X.append(c @ Rt.T + Tt)
    delta = np.random.default_rng(seed).normal(0, 0.2, E)
    sigma = 0.5 * np.exp(delta - delta.mean())
    pred_i, pred_j = torch.empty(E, n, 3, device=dev), torch.empty(E, n, 3, device=dev)
    for e, (i, j) in enumerate(edges):
        pred_i[e] = ((X[i] - T[i]) @ R[i]) / float(sigma[e])
        pred_j[e] = ((X[j] - T[i]) @ R[i]) / float(sigma[e])
    pred_i += 0.01 * torch.randn(pred_i.shape, device=dev, generator=g)
    pred_j += 0.01 * torch.randn(pred_j.shape, device=dev, generator=g)
    scale = torch.tensor([1.01 ** int(k) for k in np.random.default_rng(seed + 1).permutation(E)], dtype=torch.float32, device=dev)[:, None]
    conf_i = (1 + 3 * torch.rand(E, n, device=dev, generator=g)) * scale
    conf_j = (1 + 3 * torch.rand(E, n, device=dev, generator=g)) * scale
    return edges, dict(pred_i=pred_i, pred_j=pred_j, conf_i=conf_i, conf_j=conf_j)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def device_ms(fn, reps):
    """median over `reps` of the device time of fn() (events on the current stream), after one warm-up call"""
    fn()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return statistics.median(times)


out = {"H": H, "W": W, "reps": a.reps, "sets": {}}
for name in a.sizes.split(","):
    V = SETS[name]
    edges, arrays = scene(V, 40 + V)
    E, n = len(edges), H * W
    problem = ga.AlignProblem(edges, arrays["pred_i"], arrays["pred_j"], arrays["conf_i"], arrays["conf_j"], H, W)

    def fused():
        return ga.init_minimum_spanning_tree(problem)

    def eager():
        return mu.restate_init(edges, H, W, arrays, torch.float32, pose_mode="default")

    fused(); eager()   # warm-up
    ms = {"eager": [], "fused": []}
    for _ in range(a.reps):
        t, re_ = timed(eager)
        ms["eager"].append(t)
        t, st = timed(fused)
        ms["fused"].append(t)
    assert st.mst_edges == re_["mst_edges"], "the two forms walked different trees"
    d = mu.distances(mu.device_result(st), {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in re_.items()})
    me, mf = statistics.median(ms["eager"]), statistics.median(ms["fused"])
    # stages, through the library's own entry points on the problem's buffers
    L, stp = _lib.lib(), _lib.stream_ptr(dev)
    ws = ga._init_workspace(dev, max(E, V), n)
    means = torch.empty(2 * E, device=dev)
    recs = int(L.mi355gs_align_records(problem._handle))
    idx_src = torch.arange(0, 2 * E, 2, dtype=torch.int32, device=dev)
    idx_tgt = torch.tensor([i for i, j in edges], dtype=torch.int32, device=dev)
    pts3d = st.init_pts3d.reshape(V, n, 3).clone()
    srt, pw, foc = torch.empty(E, 16, device=dev), torch.empty(E, 8, device=dev), torch.empty(V, device=dev)
    img_src = torch.tensor([2 * min(e for e, (i, j) in enumerate(edges) if i == v) for v in range(V)], dtype=torch.int32, device=dev)
    stages = {
        "means": device_ms(lambda: (L.mi355gs_align_init_means(_lib.ptr(ws), stp, E, n, _lib.ptr(problem.conf_i), _lib.ptr(means)),
                                    L.mi355gs_align_init_means(_lib.ptr(ws), stp, E, n, _lib.ptr(problem.conf_j), _lib.ptr(means) + 4 * E)), a.reps),
        "pair_registration": device_ms(lambda: L.mi355gs_align_init_register(_lib.ptr(ws), stp, E, n, recs, _lib.ptr(idx_src), 4 * n, 4, _lib.ptr(pts3d),
                                                                             _lib.ptr(idx_tgt), 3 * n, _lib.ptr(problem.conf_i), None, n, _lib.ptr(srt),
                                                                             _lib.ptr(pw)), a.reps),
        "one_walk_step": device_ms(lambda: (L.mi355gs_align_init_register(_lib.ptr(ws), stp, 1, n, recs, None, 0, 4, _lib.ptr(pts3d), None, 0,
                                                                           _lib.ptr(problem.conf_i), None, 0, _lib.ptr(srt), None),
                                            L.mi355gs_align_init_apply(stp, n, recs + 16 * n, 4, _lib.ptr(srt), _lib.ptr(pts3d) + 12 * n)), a.reps),
        "focals": device_ms(lambda: L.mi355gs_align_init_focals(_lib.ptr(ws), stp, V, H, W, recs, _lib.ptr(img_src), 4 * n, 4, _lib.ptr(foc)), a.reps),
    }
    reg_bytes = 2 * E * n * (16 + 12 + 4)
    rec = {"views": V, "edges": E, "points_per_image": n, "ms_eager": me, "ms_eager_runs": ms["eager"], "ms_fused": mf, "ms_fused_runs": ms["fused"],
           "speedup": me / mf, "fused_vs_eager_rel_l2": d, "stage_ms": stages, "pair_registration_bytes": reg_bytes,
           "pair_registration_GBps": reg_bytes / (stages["pair_registration"] * 1e-3) / 1e9}
    assert mf < me, (name, "the fused call is not faster than the restatement", mf, me)
    out["sets"][name] = rec
    del problem, arrays, st, re_, pts3d
    torch.cuda.empty_cache()
line = json.dumps(out)
print(line, flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
