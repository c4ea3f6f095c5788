"""Output bits of every entry point that runs a kernel of csrc/ssim.hip (and of k_pose_finish_partials, which finishes the one-call
step's loss), on seeded inputs: prints ONE JSON object, label -> sha256 of the output's bytes.  Two trees compute the same thing
when their objects are equal key for key:

    python tools/loss_bits.py [--tree DIR] [--emu] [--skip-trainer] > bits.json

--tree DIR   import the package (and tests/) from DIR instead of this file's repository
--emu        route to DIR/tests/emu/libmi355gs_emu.so on CPU tensors (built if missing); without it cuda:0, which also adds the
             3x512x512 / 3x1080x1920 cases, a 1080x1920 metrics set and the C3 scene for the trainer steps
Set MI355GS_DETERMINISTIC=1 for the trainer steps (the pose gradient otherwise meets in float atomics).
Measurement helper, not product code."""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--emu", action="store_true")
ap.add_argument("--skip-trainer", action="store_true")
a = ap.parse_args()
ROOT = os.path.abspath(a.tree)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from instantsplat_amd import _lib, lazy_loss  # noqa: E402
from instantsplat_amd import fused_ssim as fs  # noqa: E402
from instantsplat_amd.loss_utils import l1_loss  # noqa: E402
from instantsplat_amd.metrics import image_metrics_rgb8  # noqa: E402
from tests import loss_util, metrics_util  # noqa: E402
from tests.test_loss_kernels_emu import DEGENERATE, PLANES, TILE_EDGES  # noqa: E402

assert os.path.abspath(_lib.__file__).startswith(ROOT + os.sep), _lib.__file__
if a.emu:
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    _lib._use_library_for_testing(os.path.join(ROOT, "tests", "emu", "libmi355gs_emu.so"))
    dev = torch.device("cpu")
else:
    dev = torch.device("cuda:0")
OUT = {}


def put(label, t):
    if isinstance(t, float):
        data = struct.pack("<f", t)
    elif isinstance(t, np.ndarray):
        data = np.ascontiguousarray(t).tobytes()
    else:
        data = t.detach().cpu().contiguous().numpy().tobytes()
    assert label not in OUT, label
    OUT[label] = hashlib.sha256(data).hexdigest()


def loss_case(tag, content, B, C, H, W, seed=0):
    x0, y0 = loss_util.make_case(content, B, C, H, W, seed)
    y = y0.to(dev)
    for padding in ("same", "valid"):
        valid = padding == "valid"
        if valid and (H <= 10 or W <= 10):
            continue
        t = "%s/fused_ssim_%s" % (tag, padding)
        lazy_loss.forget()
        x = x0.to(dev, copy=True).requires_grad_(True)
        v = fs.fused_ssim(x, y, padding=padding)
        v.backward()
        put(t + "/value", v); put(t + "/grad", x.grad)
        xa, ya, d1, d2, d3, means = fs._run_forward(x0.to(dev), y, True, valid)   # the ctypes entry point: the maps themselves
        put(t + "/means", means[:1] if valid else means)
        put(t + "/dm_dmu1", d1); put(t + "/dm_dsigma1_sq", d2); put(t + "/dm_dsigma12", d3)
        ks, kl = torch.tensor([0.8], device=dev), torch.tensor([-0.2], device=dev)
        put(t + "/grad_scaled", fs._run_backward(xa, ya, d1, d2, d3, ks, None if valid else kl, valid))
    for lam in (0.0, 0.2, 1.0):
        t = "%s/fused_l1_ssim_lam%g" % (tag, lam)
        x = x0.to(dev, copy=True).requires_grad_(True)
        loss, means = fs.fused_l1_ssim_loss(x, y, lam)
        loss.backward()
        put(t + "/loss", loss); put(t + "/means", means); put(t + "/grad", x.grad)
    # train.py:171-176 as written (tests/loss_util.check_lazy_pair), in both orders: backward() first (program eval + grad in one
    # launch), item() first (program eval, then the pair backward)
    was, lazy_loss.ENABLED = lazy_loss.ENABLED, True
    try:
        for order in ("backward_first", "item_first"):
            t = "%s/lazy_pair_%s" % (tag, order)
            leaf = x0.reshape(B * C, H, W).to(dev, copy=True).requires_grad_(True)
            image, gt = leaf * 1.0, y0.reshape(B * C, H, W).to(dev)
            Ll1 = l1_loss(image, gt)
            ss = fs.fused_ssim(image.unsqueeze(0), gt.unsqueeze(0))
            assert type(Ll1) is lazy_loss.LazyScalar and type(ss) is lazy_loss.LazyScalar, "the pair was not taken"
            loss = (1.0 - 0.2) * Ll1 + 0.2 * (1.0 - ss)
            if order == "item_first":
                put(t + "/value", float(loss.item()))
            loss.backward()
            if order == "backward_first":
                put(t + "/value", float(loss.item()))
            put(t + "/l1_mean", float(Ll1._rec.l1)); put(t + "/ssim_mean", float(ss._rec.ssim)); put(t + "/grad", leaf.grad)
            lazy_loss.forget()
    finally:
        lazy_loss.ENABLED = was
        lazy_loss.forget()


def l1_case(tag, n, misaligned):
    g = torch.Generator().manual_seed(0)
    abuf, bbuf = torch.rand(n + 1, generator=g), torch.rand(n + 1, generator=g)
    bbuf[1::3] = abuf[1::3]
    abuf, bbuf = abuf.to(dev).requires_grad_(True), bbuf.to(dev)
    lo = 1 if misaligned else 0
    x, y = abuf[lo:lo + n], bbuf[lo:lo + n]
    assert x.data_ptr() % 16 == 4 * lo
    lazy_loss.forget()
    v = l1_loss(x, y)
    (0.8 * v).backward()
    put(tag + "/value", v); put(tag + "/grad", abuf.grad)


def metrics_case(tag, renders, gts):
    m = image_metrics_rgb8(renders, gts)
    put(tag + "/sq_sum", m["sq_sum"]); put(tag + "/ssim", m["ssim"])


for content in loss_util.CONTENTS:
    for H, W in DEGENERATE + TILE_EDGES:
        loss_case("%s/1x3x%dx%d" % (content, H, W), content, 1, 3, H, W)
    for B, C in PLANES:
        loss_case("%s/%dx%dx17x33" % (content, B, C), content, B, C, 17, 33, seed=B * 10 + C)
if not a.emu:
    for content in ("noise", "flat_quadrant"):
        for H, W in ((512, 512), (1080, 1920)):
            loss_case("%s/1x3x%dx%d" % (content, H, W), content, 1, 3, H, W)
l1_case("l1_loss/aligned_4097", 4097, False)
l1_case("l1_loss/misaligned_4097", 4097, True)

for H, W in metrics_util.SHAPES:
    for kind in metrics_util.KINDS:
        r, g = metrics_util.frame_pairs(kind, 2, H, W)
        metrics_case("metrics/%s/2x%dx%d" % (kind, H, W), torch.from_numpy(r).to(dev), torch.from_numpy(g).to(dev))
r, g = metrics_util.frame_pairs("random", 2, 16, 32, seed=4)   # W a multiple of 4, bases one byte into their buffers: the byte loads
br, bg = torch.zeros(r.size + 8, dtype=torch.uint8), torch.zeros(r.size + 8, dtype=torch.uint8)
br[1:1 + r.size] = torch.from_numpy(r).reshape(-1); bg[1:1 + r.size] = torch.from_numpy(g).reshape(-1)
br, bg = br.to(dev), bg.to(dev)
vr, vg = br[1:1 + r.size].view(2, 16, 32, 3), bg[1:1 + r.size].view(2, 16, 32, 3)
assert vr.data_ptr() % 4 != 0
metrics_case("metrics/random_misaligned/2x16x32", vr, vg)
if not a.emu:
    r, g = metrics_util.frame_pairs("noise3", 2, 1080, 1920)
    metrics_case("metrics/noise3/2x1080x1920", torch.from_numpy(r).to(dev), torch.from_numpy(g).to(dev))

if not a.skip_trainer:
    # 20 one-call trainer steps: the loss k_pose_finish_partials finishes from the loss kernel's partials, and the pose gradient
    from instantsplat_amd.arguments import OptimizationParams
    from instantsplat_amd.synthetic import syn_pointmap
    from instantsplat_amd.train import release_trainer, setup_training, train_iteration
    scene = syn_pointmap(3, 8, 8, 24, 24, seed=2) if a.emu else syn_pointmap(3, 256, 256, 512, 512, seed=0)
    st = setup_training(scene, dev, opt=OptimizationParams(iterations=10 ** 9, pp_optimizer=True, optim_pose=True))
    for i in range(20):
        put("trainer/step%02d/loss_out" % i, float(train_iteration(st, fused_step=True)))
        if dev.type == "cuda":
            torch.cuda.synchronize()
        # (the forward + backward of the NEXT iteration is already enqueued behind this one: its pose gradient, in stream order)
        assert st._trainer is not None
        put("trainer/step%02d/pose_grad" % i, st._trainer.gradients()["P"])
    release_trainer(st)

print(json.dumps(OUT, sort_keys=True))
