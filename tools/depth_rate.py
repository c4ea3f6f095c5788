"""Time of the depth / accumulated-alpha pass beside the colour composite kernels, at BASELINE config C3 (3 views, 196,608
Gaussians, 512x512, SH degree 0 as training starts), one view, through the raw C ABI in one process:
  depth forward   mi355gs_raster_depth_forward (one launch: k_depth_fwd) after a RENDER-ONLY frame
  depth backward  mi355gs_raster_depth_backward after a training frame: the whole call (memset, k_depth_bwd, k_preprocess_bwd,
                  k_depth_dz) and, from a second timing with dL_ddepth = dL_dalpha = null (which skips k_depth_bwd only), the
                  difference of the two — k_depth_bwd's own share
  colour forward / backward / render-only forward: k_composite_fwd and k_composite_bwd of the same frames, from the library's own
                  event pairs around those launches (mi355gs_profile_*)
Every timing is an event pair on the launch stream around one call, --reps times after --warmup; medians and every repetition
are reported.  Writes one JSON line (and --out).  Measurement helper, not product code."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--train", type=int, default=0, help="one-call training iterations before the measurement")
ap.add_argument("--out")
a = ap.parse_args()

import torch  # noqa: E402

from instantsplat_amd import _lib, train  # noqa: E402
from instantsplat_amd.arguments import OptimizationParams  # noqa: E402
from instantsplat_amd.pose_utils import get_camera_from_tensor, quadmultiply  # noqa: E402
from instantsplat_amd.synthetic import syn_pointmap  # noqa: E402

dev = torch.device("cuda:0")
st = train.setup_training(syn_pointmap(3, 256, 256, 512, 512, seed=0), dev, opt=OptimizationParams(iterations=10 ** 9, pp_optimizer=True, optim_pose=True))
for _ in range(a.train):
    train.train_iteration(st, fused_step=True)
if a.train:
    train.release_trainer(st)
g, cam = st.gaussians, st.cameras[0]
with torch.no_grad():
    pose = g.P[cam.uid]
    w2c = get_camera_from_tensor(pose)
    means = (g._xyz @ w2c[:3, :3].t() + w2c[:3, 3]).contiguous()
    rots, scales, opac = quadmultiply(pose[:4], g._rotation).contiguous(), torch.exp(g._scaling).contiguous(), torch.sigmoid(g._opacity).reshape(-1).contiguous()
    shs = g._features_dc.detach().contiguous()
P, W, H, D = means.shape[0], int(cam.image_width), int(cam.image_height), 0
import math  # noqa: E402
tanx, tany = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
view, proj, campos = torch.eye(4, device=dev).reshape(-1), cam.projection_matrix.to(dev).float().contiguous().reshape(-1), torch.zeros(3, device=dev)
bg = st.background.float().contiguous()

L, p, stream = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
u8 = lambda n: torch.zeros(max(int(n), 1), dtype=torch.uint8, device=dev)
f = lambda *s: torch.zeros(*s, device=dev)
geom, tiles, radii, nr = u8(L.mi355gs_raster_geom_bytes(P)), u8(L.mi355gs_raster_tiles_bytes(W, H)), torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
img, depth, alpha = f(3, H, W), f(H, W), f(H, W)
gen = torch.Generator().manual_seed(0)
gC, gD, gA = (torch.randn(*s, generator=gen).to(dev) for s in ((3, H, W), (H, W), (H, W)))
out_c = [f(P, 3), f(P, 3), f(P, 1, 3), f(P), f(P, 3), f(P, 4)]
out_d = [f(P, 3), f(P, 3), f(P), f(P, 3), f(P, 4)]
scratch_c, scratch_d = u8(L.mi355gs_raster_grad_scratch_bytes(P)), u8(L.mi355gs_raster_depth_scratch_bytes(P))


def preprocess():
    _lib.check(L.mi355gs_raster_forward_preprocess(stream, P, D, 1, W, H, p(means), p(shs), None, None, p(opac), p(scales), 1.0, p(rots), None, p(view), p(proj),
                                                   p(campos), tanx, tany, 0, p(radii), p(geom), p(tiles), p(nr), None, None, 0), "preprocess")


preprocess()
R = int(nr.item())
bin_train, bin_ro = u8(L.mi355gs_raster_binning_bytes(R, W, H)), u8(L.mi355gs_raster_binning_bytes_render_only(R, W, H))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(torch.cuda.current_stream(dev))
    fn()
    e1.record(torch.cuda.current_stream(dev))
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)      # us


def depth_fwd(binning):
    _lib.check(L.mi355gs_raster_depth_forward(stream, P, W, H, R, p(geom), p(tiles), p(binning), p(depth), p(alpha)), "depth_forward")


def depth_bwd(gd, ga):
    _lib.check(L.mi355gs_raster_depth_backward(stream, P, W, H, p(means), p(scales), 1.0, p(rots), None, p(view), p(proj), p(campos), tanx, tany, p(geom), p(tiles),
                                               p(bin_train), R, p(radii), p(gd), p(ga), p(scratch_d), p(out_d[0]), p(out_d[1]), p(out_d[2]), p(out_d[3]), p(out_d[4]),
                                               None, 0), "depth_backward")


def colour_bwd():
    _lib.check(L.mi355gs_raster_backward(stream, P, D, 1, W, H, p(bg), p(means), p(shs), None, None, p(opac), p(scales), 1.0, p(rots), None, p(view), p(proj), p(campos),
                                         tanx, tany, p(geom), p(tiles), p(bin_train), R, p(radii), p(img), p(gC), p(scratch_c), p(out_c[0]), p(out_c[1]), p(out_c[2]),
                                         None, None, p(out_c[3]), p(out_c[4]), p(out_c[5]), None, 0, 0), "backward")


us = {"depth_forward_after_render_only": [], "depth_forward_after_training_forward": [], "depth_backward_call": [], "depth_backward_call_without_k_depth_bwd": []}
same = True
for it in range(a.warmup + a.reps):
    if it == a.warmup:
        L.mi355gs_profile_begin()
    preprocess()
    _lib.check(L.mi355gs_raster_forward_render_only(stream, P, W, H, R, p(bg), p(geom), p(tiles), p(bin_ro), p(img), 0), "render_only")
    t_ro = timed(lambda: depth_fwd(bin_ro))
    d_ro = depth.clone()
    preprocess()
    _lib.check(L.mi355gs_raster_forward_render(stream, P, W, H, R, p(bg), p(geom), p(tiles), p(bin_train), p(img), 0), "render")
    t_tr = timed(lambda: depth_fwd(bin_train))
    same = same and torch.equal(d_ro, depth)
    colour_bwd()
    t_b = timed(lambda: depth_bwd(gD, gA))
    t_b0 = timed(lambda: depth_bwd(None, None))
    if it >= a.warmup:
        for k, v in zip(us, (t_ro, t_tr, t_b, t_b0)):
            us[k].append(v)
prof = {}
for kind, name in ((0, "colour_composite_forward_training"), (1, "colour_composite_backward"), (2, "colour_composite_forward_render_only")):
    ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
    _lib.check(L.mi355gs_profile_read(kind, ctypes.byref(ms), ctypes.byref(n)), "profile_read")
    prof[name + "_us"] = 1e3 * ms.value / max(n.value, 1)
    prof[name + "_launches"] = n.value
L.mi355gs_profile_end()
med = {k + "_us": statistics.median(v) for k, v in us.items()}
out = {"scene": "C3", "gaussians": P, "W": W, "H": H, "sh_degree": D, "instances": R, "trained_iterations": a.train, "reps": a.reps,
       "depth_identical_after_both_forwards": bool(same), **med,
       "k_depth_bwd_share_us": med["depth_backward_call_us"] - med["depth_backward_call_without_k_depth_bwd_us"], **prof,
       "runs_us": us, "timing": "event pair around one call (depth) / around one launch (colour, mi355gs_profile_*), same process and frames"}
print(json.dumps(out), flush=True)
if a.out:
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
