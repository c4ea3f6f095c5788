"""Time of ONE clone + split + prune event of the adaptive density control at C3's 196,608 Gaussians (max_sh_degree 3, a stepped
per-point optimizer's state, roughly 10 % of the rows selected and a few per cent pruned; tests/density_cases.py's seeded
generator), two forms on the same device:
  (a) eager: the torch restatement of the reference's sequence (scene/gaussian_model.py:344-472 with :464-465 restored) on device
      tensors — boolean indexing, `cat` and `zeros_like` over the 6 per-Gaussian parameters, their 12 moments, the per-point
      rates and the statistics, with the host synchronisations boolean indexing implies;
  (b) fused: ONE GaussianModel.densify_and_prune(clone_and_split=True) call — plan, the read-back of the totals, torch.randn for
      the children, apply and the optimizer surgery.
Each is warmed up, then timed --reps times in one process with a synchronize before every reading of the clock, every repetition
on a freshly built model; the medians and every repetition are reported, and the two forms must agree (new P, and every copied
row to the bit).  Also prints k_density_scatter's algorithmic bytes (rows read + rows written, from the shapes), to be divided
by its duration in a kernel trace.  Prints one JSON line.
  --fused-only   warm-up and ONE fused call (for `rocprofv3 --kernel-trace --stats`)
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
ap.add_argument("--P", type=int, default=196608)
ap.add_argument("--fused-only", action="store_true")
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import density_cases as dc  # noqa: E402

dev = torch.device("cuda:0")
N, SCREEN = 2, 20
c = dc.make_case(a.P, "nothing", sh_degree=3, N=N, max_screen_size=SCREEN, seed=1)
r = np.random.RandomState(5)
hot = r.rand(a.P) < 0.10                                    # ~10 % over the gradient threshold: cloned or split by their size
c["accum"][hot, 0] = np.float32(5 * dc.MAX_GRAD) * np.maximum(c["denom"][hot, 0], 1)
c["denom"][hot, 0] = np.maximum(c["denom"][hot, 0], 1)
faint = r.rand(a.P) < 0.03                                  # ~3 % under the opacity threshold
c["opacity"][faint, 0] = np.float32(np.log(0.002 / 0.998))
dc.assert_margins(c)
NAMES = dc.PARAM_NAMES


def eager(m, noise):
    """the reference's sequence on the model's tensors, eagerly; returns the new rows (the model is left alone)"""
    t = {n: getattr(m, dc.ATTR[n]).detach() for n in NAMES}
    mom = {n: (m.optimizer.state[getattr(m, dc.ATTR[n])]["exp_avg"], m.optimizer.state[getattr(m, dc.ATTR[n])]["exp_avg_sq"]) for n in NAMES}
    pp = m.per_point_lr
    P = t["xyz"].shape[0]
    grads = m.xyz_gradient_accum / m.denom
    grads[grads.isnan()] = 0.0

    def cat(new, rows):
        nonlocal pp
        for n in NAMES:
            t[n] = torch.cat((t[n], new[n]), dim=0)
            mom[n] = (torch.cat((mom[n][0], torch.zeros_like(new[n])), dim=0), torch.cat((mom[n][1], torch.zeros_like(new[n])), dim=0))
        pp = torch.cat((pp, rows), dim=0)

    def prune(mask):
        nonlocal pp
        keep = ~mask
        for n in NAMES:
            t[n] = t[n][keep]
            mom[n] = (mom[n][0][keep], mom[n][1][keep])
        pp = pp[keep]
    limit = dc.PERCENT_DENSE * dc.EXTENT
    sel = torch.logical_and(torch.norm(grads, dim=-1) >= dc.MAX_GRAD, torch.max(torch.exp(t["scaling"]), dim=1).values <= limit)
    cat({n: t[n][sel] for n in NAMES}, pp[sel])
    padded = torch.zeros(t["xyz"].shape[0], device=dev)
    padded[:P] = grads.squeeze()
    sel = torch.logical_and(padded >= dc.MAX_GRAD, torch.max(torch.exp(t["scaling"]), dim=1).values > limit)
    stds = torch.exp(t["scaling"][sel]).repeat(N, 1)
    samples = stds * noise[:stds.shape[0]]
    q = t["rotation"][sel]
    q = q / torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3).repeat(N, 1, 1)
    new = {n: t[n][sel].repeat(N, *([1] * (t[n].dim() - 1))) for n in NAMES}
    new["xyz"] = torch.bmm(R, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][sel].repeat(N, 1)
    new["scaling"] = torch.log(stds / (0.8 * N))
    cat(new, pp[sel].repeat(N, 1))
    prune(torch.cat((sel, torch.zeros(N * int(sel.sum()), device=dev, dtype=torch.bool))))
    k = t["xyz"].shape[0]
    max_radii = torch.zeros(k, device=dev)   # densification_postfix: the statistics start again
    mask = (torch.sigmoid(t["opacity"]) < dc.MIN_OPACITY).squeeze()
    mask = torch.logical_or(torch.logical_or(mask, max_radii > SCREEN), torch.max(torch.exp(t["scaling"]), dim=1).values > 0.1 * dc.EXTENT)
    prune(mask)
    k = t["xyz"].shape[0]
    return t, mom, pp, (torch.zeros(k, 1, device=dev), torch.zeros(k, 1, device=dev), torch.zeros(k, device=dev))


def fused(m, noise):
    return m.densify_and_prune(dc.MAX_GRAD, dc.MIN_OPACITY, dc.EXTENT, SCREEN, clone_and_split=True, N=N, noise=noise)


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


noise = torch.from_numpy(c["noise"]).to(dev)
m = dc.build_model(c, dev, "pp")
want = eager(m, noise)              # warm-up, and the two forms must agree
tot = fused(m, noise)               # warm-up
assert tot["new_P"] == want[0]["xyz"].shape[0], (tot, want[0]["xyz"].shape)
n_copied = tot["originals"] + tot["clones"]
for n in NAMES:
    got = getattr(m, dc.ATTR[n]).detach()
    rows = n_copied if n in ("xyz", "scaling") else tot["new_P"]
    assert torch.equal(got[:rows], want[0][n][:rows]), n
    assert torch.equal(m.optimizer.state[getattr(m, dc.ATTR[n])]["exp_avg"], want[1][n][0]), n
assert torch.equal(m.per_point_lr, want[2])
row_in = 4 * (3 * (3 + 3 + 45 + 1 + 3 + 4) + 1)            # parameters + both moments + the per-point rate, bytes per input row
row_out = row_in + 4 * 3                                   # ... + the three zeroed statistics
scatter_bytes = a.P * (row_in + 4) + tot["new_P"] * row_out + tot["split"] * N * 12   # + a code word per row, a normal per child
out = {"P": a.P, "sh_degree": 3, "N": N, "totals": tot, "selected_fraction": (tot["split"] + tot["clone_selected"]) / a.P,
       "k_density_scatter_algorithmic_bytes": scatter_bytes}
if a.fused_only:
    m = dc.build_model(c, dev, "pp")
    out["ms_fused_single_run"] = timed(fused, m, None)[0]
else:
    ms = {"eager": [], "fused": [], "fused_given_noise": []}
    for _ in range(a.reps):
        m = dc.build_model(c, dev, "pp")
        ms["eager"].append(timed(eager, m, noise)[0])
        ms["fused"].append(timed(fused, m, None)[0])        # as training calls it: torch.randn after the read-back included
        m = dc.build_model(c, dev, "pp")
        ms["fused_given_noise"].append(timed(fused, m, noise)[0])
    me, mf = statistics.median(ms["eager"]), statistics.median(ms["fused"])
    out.update({"reps": a.reps, "ms_eager": me, "ms_eager_runs": ms["eager"], "ms_fused": mf, "ms_fused_runs": ms["fused"],
                "ms_fused_given_noise": statistics.median(ms["fused_given_noise"]), "ms_fused_given_noise_runs": ms["fused_given_noise"],
                "speedup": me / mf})
print(json.dumps(out), flush=True)
