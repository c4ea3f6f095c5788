"""Rate of MASt3R's dense heads at the checkpoint's sizes (tokens 1024 / 768, layer_dims 96 .. 768, F = 256, last_dim 128, 24
descriptor channels + 1) with seeded weights on the 18 x 32 token grid (512 x 288 images): 6 edges (3 images) and 210 edges (15
images), both sides; the hooked tensors are seeded N(0, 1) rows, so no trunk runs.  Three forms on one device:
  (a) torch:    a float32 restatement (tests/heads_util.HeadRef: F.conv2d, F.conv_transpose2d, F.interpolate) one edge at a time,
                the reference's inference(batch_size=1) loop shape;
  (b) wrapper:  ONE Mast3rHeads.heads call, its allocations included (descriptors off, as init_geo.py runs it; --descriptors: on);
  (c) library:  the bare mi355gs_dpt_head calls on buffers allocated beforehand (the same chunks).
Each is warmed up, then timed --reps times with a synchronize before every reading of the clock; medians and every repetition are
reported, and TFLOP/s against the 157.3 TFLOP/s FP32 matrix peak.  FLOP of one head on one edge (multiply and add counted
separately; ReLU, bilinear, GELU, postprocess not counted), N tokens, c_k = dim_tokens, l_k = layer_dims, n3 = ceil(Ht/2) ceil(Wt/2):
  act_postprocess = 2 N sum_k c_k l_k + 2 N (16 l_0^2 + 4 l_1^2) + 18 n3 l_3^2
  layer_rn        = 18 F (16 N l_0 + 4 N l_1 + N l_2 + n3 l_3)
  fusion blocks   = 18 F^2 (2 n3 + 4 N + 16 N + 64 N) + 2 F^2 (N + 4 N + 16 N + 64 N)
  head            = 18 F (F/2) 64 N + 18 (F/2) last 256 N + 8 last 256 N
  local features  = 2 N (K hid + hid (D + 1) 256)            (counted only with --descriptors)
--end-to-end: also Mast3r.inference (full-depth seeded trunk + heads) on the 3-image set against the restatement looped as the
reference loops (both images of every pair encoded, the pair decoded, both heads), and on the 15-image set alone.
  --fused-only   warm-up and ONE wrapper call per set (for `rocprofv3 --kernel-trace --stats`)
  --sets a,b     which sets (default: both)
Prints one JSON line.  Measurement helper, not product code."""
import argparse
import ctypes
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
ap.add_argument("--descriptors", action="store_true")
ap.add_argument("--end-to-end", action="store_true")
ap.add_argument("--sets", default="views3_edges6,views15_edges210")
a = ap.parse_args()

import torch  # noqa: E402

from instantsplat_amd import _frames, _lib  # noqa: E402
from instantsplat_amd.mast3r_heads import DEFAULT_SCRATCH_BUDGET, Mast3rHeads  # noqa: E402
from tests import heads_util as hu  # noqa: E402

PEAK_TFLOPS = 157.3
Ht, Wt = 18, 32
N, H, W = Ht * Wt, 16 * Ht, 16 * Wt
dev = torch.device("cuda:0")
net = hu.REAL
cfg = hu.config(net)
state = hu.make_state(net)
heads = Mast3rHeads(state, cfg, device=dev)
state_dev = {k: v.to(dev) for k, v in state.items()}
refs = [hu.HeadRef(state_dev, cfg, s + 1, torch.float32) for s in range(2)]


def head_flop():
    c, l, F, LD = cfg.dim_tokens, cfg.layer_dims, cfg.feature_dim, cfg.last_dim
    n3 = ((Ht + 1) // 2) * ((Wt + 1) // 2)
    act = 2 * N * sum(ck * lk for ck, lk in zip(c, l)) + 2 * N * (16 * l[0] ** 2 + 4 * l[1] ** 2) + 18 * n3 * l[3] ** 2
    rn = 18 * F * (16 * N * l[0] + 4 * N * l[1] + N * l[2] + n3 * l[3])
    fusion = 18 * F * F * (2 * n3 + 84 * N) + 2 * F * F * 85 * N
    head = 18 * F * (F // 2) * 64 * N + 18 * (F // 2) * LD * 256 * N + 8 * LD * 256 * N
    return act + rn + fusion + head


def mlp_flop():
    K, hid = cfg.dim_tokens[0] + cfg.dim_tokens[3], cfg.mlp_hidden()
    return 2 * N * (K * hid + hid * (cfg.local_feat_dim + 1) * 256)


def torch_loop(dec, keep=False):
    kept = []
    with torch.no_grad():
        for e in range(dec[0][0].shape[0]):
            for s in range(2):
                hooked = tuple(t[e:e + 1] for t in dec[s])
                o = refs[s].dpt(hooked, Ht, Wt)
                if a.descriptors:
                    o.update(refs[s].local(hooked, Ht, Wt, o["conf"]))
                if keep:
                    kept.append({k: o[k] for k in ("pts3d", "conf") + (("desc", "desc_conf") if a.descriptors else ())})
    return kept


def wrapper(dec):
    return heads.heads(dec[0], dec[1], (Ht, Wt), descriptors=a.descriptors)


class Bare:
    """the wrapper's library calls on buffers allocated once"""

    def __init__(self, E):
        self.c = ctypes.byref(heads._cfg_c)
        L = _lib.lib()

        def need(k):
            x = int(L.mi355gs_dpt_head_scratch_bytes(self.c, Ht, Wt, k))
            y = int(L.mi355gs_local_features_scratch_bytes(self.c, Ht, Wt, k)) if a.descriptors else 1
            return max(x, y) if x and y else 0
        self.n = _frames.frames_per_call(lambda k: 0 < need(k) <= DEFAULT_SCRATCH_BUDGET, E, DEFAULT_SCRATCH_BUDGET // need(1))
        self.scratch = torch.empty(need(self.n), dtype=torch.uint8, device=dev)
        self.out = [dict(pts3d=torch.empty(E, H, W, 3, device=dev), conf=torch.empty(E, H, W, device=dev)) for _ in range(2)]
        if a.descriptors:
            for o in self.out:
                o.update(desc=torch.empty(E, H, W, cfg.local_feat_dim, device=dev), desc_conf=torch.empty(E, H, W, device=dev))

    def __call__(self, dec):
        E = dec[0][0].shape[0]
        for first in range(0, E, self.n):
            m = min(self.n, E - first)
            for s in range(2):
                o = self.out[s]
                ptrs = (ctypes.c_void_p * 4)(*[t[first:first + m].data_ptr() for t in dec[s]])
                _lib.call(dev, "dpt_head", _lib.STREAM, self.c, heads._dpt[s], Ht, Wt, m, ptrs, self.scratch, o["pts3d"][first:first + m],
                          o["conf"][first:first + m], None)
                if a.descriptors:
                    _lib.call(dev, "local_features", _lib.STREAM, self.c, heads._mlp[s], Ht, Wt, m, dec[s][0][first:first + m],
                              dec[s][3][first:first + m], self.scratch, o["desc"][first:first + m], o["desc_conf"][first:first + m])
        return self.out


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def errors(got, want):
    d = got.double() - want.double()
    return {"max_abs": float(d.abs().max()), "rel_l2": float(d.norm() / want.double().norm())}


SETS = {"views3_edges6": 6, "views15_edges210": 210}
per_edge = 2 * (head_flop() + (mlp_flop() if a.descriptors else 0))
out = {"config": {k: list(v) if isinstance(v, tuple) else v for k, v in net.items()}, "grid": [Ht, Wt], "reps": a.reps, "descriptors": a.descriptors,
       "peak_tflops_fp32_matrix": PEAK_TFLOPS, "gflop_one_head_one_edge": head_flop() / 1e9, "gflop_local_features_one_edge_side": mlp_flop() / 1e9,
       "gflop_per_edge_both_sides": per_edge / 1e9, "sets": {}}
for name in a.sets.split(","):
    E = SETS[name]
    dec = [tuple(t.to(dev) for t in side) for side in hu.hooks(net, E, Ht, Wt)]
    if a.fused_only:
        wrapper(dec)
        out["sets"][name] = {"edges": E, "ms_wrapper_single_run": timed(wrapper, dec)[0]}
        continue
    bare = Bare(E)
    got = wrapper(dec)
    bare(dec)
    rec = {"edges": E, "edges_per_library_call": bare.n, "library_equals_wrapper_bits": all(torch.equal(bare.out[s][k], got[s][k]) for s in range(2) for k in got[s])}
    small = [tuple(t[:2] for t in side) for side in dec]
    kept = torch_loop(small, keep=True)      # warm-up, and the yardstick of the error figure (the first two edges)
    rec["error_vs_float32_restatement_first_two_edges"] = {
        f"side{s + 1}_{k}": errors(got[s][k][:2], torch.cat([kept[2 * e + s][k] for e in range(2)])) for s in range(2) for k in got[s]}
    del got, kept
    ms = {"torch": [], "wrapper": [], "library": []}
    for _ in range(a.reps):
        for form, fn in (("torch", torch_loop), ("wrapper", wrapper), ("library", bare)):
            ms[form].append(timed(fn, dec)[0])
    for form in ms:
        med = statistics.median(ms[form])
        rec[f"ms_{form}"], rec[f"ms_{form}_runs"] = med, ms[form]
        rec[f"tflops_{form}"] = E * per_edge / (med * 1e-3) / 1e12
        rec[f"fraction_of_peak_{form}"] = rec[f"tflops_{form}"] / PEAK_TFLOPS
    out["sets"][name] = rec
    del dec, bare

if a.end_to_end:
    from instantsplat_amd.mast3r import Mast3r
    from instantsplat_amd.mast3r_trunk import TrunkConfig, complete_edges
    from tests import vit_util as vu
    FULL = dict(enc_dim=1024, enc_depth=24, enc_heads=16, dec_dim=768, dec_depth=12, dec_heads=12)
    tstate = dict(vu.make_state(FULL))
    tstate.update(state)
    model = Mast3r(tstate, TrunkConfig(**FULL), cfg, device=dev)
    tref = vu.Ref({k: v.to(dev) for k, v in vu.make_state(FULL).items()}, TrunkConfig(**FULL), torch.float32)

    def torch_pairs(img, edges):
        with torch.no_grad():
            for i, j in edges.tolist():
                feat, pos = tref.encode(img[[i, j]])
                d1, d2 = tref.decode(feat, pos, [(0, 1)])
                refs[0].dpt(d1, Ht, Wt), refs[1].dpt(d2, Ht, Wt)

    e2e = {}
    for V in (3, 15):
        img = vu.images(V, Ht, Wt).to(dev)
        edges = complete_edges(V)
        model.inference(img)
        runs = [timed(model.inference, img)[0] for _ in range(a.reps)]
        rec = {"views": V, "edges": int(edges.shape[0]), "ms_inference": statistics.median(runs), "ms_inference_runs": runs}
        if V == 3:
            torch_pairs(img, edges[:1])
            truns = [timed(torch_pairs, img, edges)[0] for _ in range(a.reps)]
            rec.update(ms_torch_pairs=statistics.median(truns), ms_torch_pairs_runs=truns)
        e2e[f"views{V}"] = rec
    out["end_to_end"] = e2e
print(json.dumps(out), flush=True)
