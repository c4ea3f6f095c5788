"""Rate of LPIPS-VGG on 8-bit frame pairs at the real widths (64, 128, 256, 512, 512) with seeded weights, two sets:
12 x 512x512 and 12 x 1280x720 (seeded bytes, the second of a pair the first plus noise in +-20); three forms:
  (a) torch: a float32 restatement of the reference's forward with F.conv2d on the same device, per pair, as an `lpips_fn`
      handed to `evaluate` would run (conversion, two trunk passes, five taps, one .item());
  (b) wrapper: ONE `LpipsVGG.lpips_rgb8` call for the set, its scratch allocation and read-back included;
  (c) library: the bare mi355gs_lpips_vgg_rgb8 calls on device buffers (the same chunks), no allocation, no read-back.
Each is warmed up, then timed --reps times with a synchronize before every reading of the clock; medians and every repetition
are reported, and TFLOP/s of the convolutions against the 157.3 TFLOP/s FP32 matrix peak:
  FLOP per pair = 2 images x sum over the 13 convolutions of 2 x 9 x Cin x Cout x H_b x W_b   (H_b = H >> b, W_b = W >> b)
(multiply and add counted separately; pools, taps and the first layer's conversion not counted).  Prints one JSON line.
  --fused-only   warm-up and ONE wrapper call per set (for `rocprofv3 --kernel-trace --stats`)
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
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from instantsplat_amd import _lib  # noqa: E402
from instantsplat_amd.lpips import BLOCK_CONVS, CONV_LAYERS, LpipsVGG  # noqa: E402

PEAK_TFLOPS = 157.3
CHANNELS = (64, 128, 256, 512, 512)
dev = torch.device("cuda:0")
gen = torch.Generator().manual_seed(0)
vgg, lin, cin, i = {}, {}, 3, 0
for blk, count in enumerate(BLOCK_CONVS):
    for _ in range(count):
        c = CHANNELS[blk]
        vgg[f"features.{CONV_LAYERS[i]}.weight"] = torch.randn(c, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5
        vgg[f"features.{CONV_LAYERS[i]}.bias"] = torch.randn(c, generator=gen) * 0.1
        cin, i = c, i + 1
    lin[f"lin{blk}.model.1.weight"] = torch.randn(1, CHANNELS[blk], 1, 1, generator=gen).abs()
net = LpipsVGG(vgg, lin, device=dev)
dvgg = {k: v.to(dev) for k, v in vgg.items()}
dlin = [lin[f"lin{b}.model.1.weight"].to(dev) for b in range(5)]
MEAN = torch.tensor([-.030, -.088, -.188], device=dev)[None, :, None, None]
STD = torch.tensor([.458, .448, .450], device=dev)[None, :, None, None]


def conv_flop_per_pair(H, W):
    total, cin, h, w = 0, 3, H, W
    for blk, count in enumerate(BLOCK_CONVS):
        if blk:
            h, w = h // 2, w // 2
        for _ in range(count):
            total += 2 * 9 * cin * CHANNELS[blk] * h * w
            cin = CHANNELS[blk]
    return 2 * total


def make_set(N, H, W):
    gt = torch.randint(0, 256, (N, H, W, 3), generator=gen, dtype=torch.uint8)
    r = (gt.to(torch.int16) + torch.randint(-20, 21, gt.shape, generator=gen, dtype=torch.int16)).clamp_(0, 255).to(torch.uint8)
    return r.to(dev), gt.to(dev)


def trunk(x):
    x = (x - MEAN) / STD
    out, i = [], 0
    for blk, count in enumerate(BLOCK_CONVS):
        if blk:
            x = F.max_pool2d(x, 2, 2)
        for _ in range(count):
            n = CONV_LAYERS[i]
            x = F.relu(F.conv2d(x, dvgg[f"features.{n}.weight"], dvgg[f"features.{n}.bias"], padding=1))
            i += 1
        out.append(x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10))
    return out


def torch_form(renders, gts):
    vals = []
    with torch.no_grad():
        for r, g in zip(renders, gts):
            x = r.permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0)
            y = g.permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0)
            res = [F.conv2d((fx - fy) ** 2, lw).mean((2, 3), True) for fx, fy, lw in zip(trunk(x), trunk(y), dlin)]
            vals.append(torch.sum(torch.cat(res, 0), 0, True).item())
    return np.array(vals, dtype=np.float32)


def wrapper_form(renders, gts):
    return net.lpips_rgb8(renders, gts)["lpips"]


class Bare:
    """the library calls of one wrapper call, on buffers allocated beforehand"""
    def __init__(self, renders, gts):
        self.r, self.g = renders, gts
        N, H, W = (int(s) for s in renders.shape[:3])
        self.n = max(1, min(N, (4 << 30) // net._scratch_bytes(1, H, W)))
        while self.n > 1 and not 0 < net._scratch_bytes(self.n, H, W) <= (4 << 30):
            self.n -= 1
        self.scratch = torch.empty(net._scratch_bytes(self.n, H, W), dtype=torch.uint8, device=dev)
        self.out = torch.empty(6 * N, dtype=torch.float32, device=dev)

    def __call__(self, renders, gts):
        L, (N, H, W) = _lib.lib(), (int(s) for s in self.r.shape[:3])
        for first in range(0, N, self.n):
            m = min(self.n, N - first)
            _lib.check(L.mi355gs_lpips_vgg_rgb8(_lib.stream_ptr(dev), m, H, W, _lib.ptr(self.r[first:first + m]), _lib.ptr(self.g[first:first + m]),
                                                net._channels_c, _lib.ptr(net.blob), _lib.ptr(self.scratch), self.out.data_ptr() + 4 * first,
                                                self.out.data_ptr() + 4 * (N + 5 * first)), "lpips_vgg_rgb8")
        return self.out


def timed(fn, renders, gts):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(renders, gts)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


SETS = {"pairs_512x512": make_set(12, 512, 512), "pairs_720x1280": make_set(12, 720, 1280)}
if a.fused_only:
    out = {}
    for name, (r, g) in SETS.items():
        wrapper_form(r, g)
        out[name] = {"pairs": int(r.shape[0]), "ms_wrapper_single_run": timed(wrapper_form, r, g)[0]}
    print(json.dumps(out), flush=True)
    sys.exit(0)

out = {"channels": list(CHANNELS), "reps": a.reps, "peak_tflops_fp32_matrix": PEAK_TFLOPS,
       "flop_formula": "per pair: 2 images x sum over 13 convolutions of 2 x 9 x Cin x Cout x H_b x W_b", "sets": {}}
for name, (r, g) in SETS.items():
    N, H, W = (int(s) for s in r.shape[:3])
    bare = Bare(r, g)
    vt, vw = torch_form(r, g), wrapper_form(r, g)   # warm-up, and the forms must agree
    vb = bare(r, g)[:N].cpu().numpy()
    ms = {"torch": [], "wrapper": [], "library": []}
    for _ in range(a.reps):
        for form, fn in (("torch", torch_form), ("wrapper", wrapper_form), ("library", bare)):
            ms[form].append(timed(fn, r, g)[0])
    flop = conv_flop_per_pair(H, W) * N
    rec = {"pairs": N, "H": H, "W": W, "pairs_per_library_call": bare.n, "conv_gflop_per_pair": conv_flop_per_pair(H, W) / 1e9,
           "max_rel_difference_wrapper_vs_torch": float(np.max(np.abs(vw.astype(np.float64) - vt) / np.abs(vt))),
           "library_equals_wrapper_bits": bool(np.array_equal(vb.view(np.uint32), vw.view(np.uint32)))}
    for form in ms:
        med = statistics.median(ms[form])
        rec[f"ms_{form}"], rec[f"ms_{form}_runs"] = med, ms[form]
        rec[f"conv_tflops_{form}"] = flop / (med * 1e-3) / 1e12
        rec[f"fraction_of_peak_{form}"] = rec[f"conv_tflops_{form}"] / PEAK_TFLOPS
    out["sets"][name] = rec
print(json.dumps(out), flush=True)
