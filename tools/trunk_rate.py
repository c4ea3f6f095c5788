"""Rate of MASt3R's transformer trunk at the checkpoint's sizes (ViT-L encoder 1024 / 24 / 16, decoders 768 / 12 / 12) with seeded
weights, two sets of 512 x 288 images: 3 images with the 6 directed edges and 15 images with the 210; four forms on one device:
  (a) torch_pairs:  a float32 restatement (tests/vit_util.Ref) looped as the reference's inference(batch_size=1) loops: for every
      directed pair both images encoded (one batch of 2), then the pair decoded;
  (b) torch_once:   the same restatement with each image encoded once (one batch of V), then one pair decoded at a time;
  (c) wrapper:      ONE Mast3rTrunk.forward_pairs call, its allocations included;
  (d) library:      the bare mi355gs_vit_encode / mi355gs_vit_decode calls on buffers allocated beforehand (the same chunks).
Each is warmed up, then timed --reps times with a synchronize before every reading of the clock; medians and every repetition
are reported, and TFLOP/s against the 157.3 TFLOP/s FP32 matrix peak.  FLOP (multiply and add counted separately; LayerNorm,
softmax, GELU, RoPE not counted), N tokens per image, D_e / D_d the widths, L_e / L_d the depths:
  encode one image  = N (2 x 768 D_e + L_e x 24 D_e^2) + L_e x 4 N^2 D_e
  decode one edge   = 2 sides x [N (2 D_e D_d + L_d x 32 D_d^2) + L_d x 8 N^2 D_d]
  (a) counts 2 encodes per edge, (b)-(d) one per image.
The error figure is the wrapper's output against the float32 restatement (b) at full depth: max-abs and relative L2 per tensor.
Prints one JSON line.
  --fused-only   warm-up and ONE wrapper call per set (for `rocprofv3 --kernel-trace --stats`)
  --sets a,b     which sets (default: both)
Measurement helper, not product code."""
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
ap.add_argument("--sets", default="views3_edges6,views15_edges210")
a = ap.parse_args()

import torch  # noqa: E402

from instantsplat_amd import _lib  # noqa: E402
from instantsplat_amd.mast3r_trunk import DEFAULT_SCRATCH_BUDGET, Mast3rTrunk, TrunkConfig, complete_edges  # noqa: E402
from tests import vit_util as vu  # noqa: E402

PEAK_TFLOPS = 157.3
FULL = dict(enc_dim=1024, enc_depth=24, enc_heads=16, dec_dim=768, dec_depth=12, dec_heads=12)
Ht, Wt = 18, 32
N = Ht * Wt
dev = torch.device("cuda:0")
cfg = TrunkConfig(**FULL)
state = vu.make_state(FULL)
net = Mast3rTrunk(state, cfg, device=dev)
ref = vu.Ref({k: v.to(dev) for k, v in state.items()}, cfg, torch.float32)


def encode_flop():
    D, L = cfg.enc_dim, cfg.enc_depth
    return N * (2 * 768 * D + L * 24 * D * D) + L * 4 * N * N * D


def decode_flop():
    De, D, L = cfg.enc_dim, cfg.dec_dim, cfg.dec_depth
    return 2 * (N * (2 * De * D + L * 32 * D * D) + L * 8 * N * N * D)


def torch_pairs(img, edges):
    out = None
    with torch.no_grad():
        for i, j in edges.tolist():
            feat, pos = ref.encode(torch.stack((img[i], img[j])))
            out = ref.decode(feat, pos, [(0, 1)])
    return out


def torch_once(img, edges, keep=False):
    kept = []
    with torch.no_grad():
        feat, pos = ref.encode(img)
        for e in edges.tolist():
            out = ref.decode(feat, pos, [tuple(e)])
            if keep:
                kept.append(out)
    return feat, kept


def wrapper(img, edges):
    return net.forward_pairs(img, edges)


class Bare:
    """the library calls of one forward_pairs call, on buffers allocated beforehand"""
    def __init__(self, img, edges):
        V, E = int(img.shape[0]), int(edges.shape[0])
        L, c = _lib.lib(), ctypes.byref(net._cfg_c)
        self.n = E
        while self.n > 1 and L.mi355gs_vit_decode_scratch_bytes(c, Ht, Wt, self.n) > DEFAULT_SCRATCH_BUDGET:
            self.n -= 1
        self.enc_scratch = torch.empty(L.mi355gs_vit_encode_scratch_bytes(c, Ht, Wt, V), dtype=torch.uint8, device=dev)
        self.dec_scratch = torch.empty(L.mi355gs_vit_decode_scratch_bytes(c, Ht, Wt, self.n), dtype=torch.uint8, device=dev)
        self.feat = torch.empty(V, N, cfg.enc_dim, device=dev)
        self.outs = [[torch.empty(E, N, D, device=dev) for D in (cfg.enc_dim, cfg.dec_dim, cfg.dec_dim, cfg.dec_dim)] for _ in range(2)]
        self.rope = net._rope_table(Ht, Wt, dev)
        self.edges = edges.to(torch.int32).contiguous()

    def __call__(self, img, edges):
        V, E = int(img.shape[0]), int(edges.shape[0])
        c = ctypes.byref(net._cfg_c)
        _lib.call(dev, "vit_encode", _lib.STREAM, c, net.blob, self.rope, Ht, Wt, V, img, self.enc_scratch, self.feat)
        for first in range(0, E, self.n):
            m = min(self.n, E - first)
            ptrs = [(ctypes.c_void_p * 4)(*[t[first:first + m].data_ptr() for t in side]) for side in self.outs]
            _lib.call(dev, "vit_decode", _lib.STREAM, c, net.blob, self.rope, Ht, Wt, V, m, self.edges[first:first + m].contiguous(), self.feat,
                      self.dec_scratch, ptrs[0], ptrs[1])
        return self.outs


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def errors(got, want):
    d = got.double() - want.double()
    return {"max_abs": float(d.abs().max()), "rel_l2": float(d.norm() / want.double().norm())}


SETS = {"views3_edges6": 3, "views15_edges210": 15}
out = {"config": FULL, "grid": [Ht, Wt], "reps": a.reps, "peak_tflops_fp32_matrix": PEAK_TFLOPS,
       "gflop_encode_one_image": encode_flop() / 1e9, "gflop_decode_one_edge": decode_flop() / 1e9,
       "flop_formula": "encode image = N (2 768 De + Le 24 De^2) + Le 4 N^2 De; decode edge = 2 [N (2 De Dd + Ld 32 Dd^2) + Ld 8 N^2 Dd]",
       "sets": {}}
for name in a.sets.split(","):
    V = SETS[name]
    img = vu.images(V, Ht, Wt).to(dev)
    edges = complete_edges(V)
    E = int(edges.shape[0])
    if a.fused_only:
        wrapper(img, edges)
        out["sets"][name] = {"views": V, "edges": E, "ms_wrapper_single_run": timed(wrapper, img, edges)[0]}
        continue
    bare = Bare(img, edges)
    feat_t, kept = torch_once(img, edges, keep=V == 3)   # warm-up, and the yardstick of the error figure
    got = wrapper(img, edges)
    bare(img, edges)
    torch_pairs(img, edges[:2])
    rec = {"views": V, "edges": E, "edges_per_library_call": bare.n, "error_vs_float32_restatement": {"feat": errors(got[0], feat_t)}}
    if kept:
        for s in (0, 1):
            for h in range(4):
                want = torch.cat([k[s][h] for k in kept])
                rec["error_vs_float32_restatement"][f"side{s + 1}_hook{h}"] = errors(got[2 + s][h], want)
    rec["library_equals_wrapper_bits"] = all(torch.equal(x, y) for s in (0, 1) for x, y in zip(bare.outs[s], got[2 + s]))
    del got, kept
    ms = {"torch_pairs": [], "torch_once": [], "wrapper": [], "library": []}
    for _ in range(a.reps):
        for form, fn in (("torch_pairs", torch_pairs), ("torch_once", torch_once), ("wrapper", wrapper), ("library", bare)):
            ms[form].append(timed(fn, img, edges)[0])
    for form in ms:
        med = statistics.median(ms[form])
        flop = (2 * E if form == "torch_pairs" else V) * encode_flop() + E * decode_flop()
        rec[f"ms_{form}"], rec[f"ms_{form}_runs"] = med, ms[form]
        rec[f"tflops_{form}"] = flop / (med * 1e-3) / 1e12
        rec[f"fraction_of_peak_{form}"] = rec[f"tflops_{form}"] / PEAK_TFLOPS
    out["sets"][name] = rec
print(json.dumps(out), flush=True)
