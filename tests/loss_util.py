"""Loss kernels (instantsplat_amd/csrc/ssim.hip) against the float64 oracle — checks shared by the CPU (emulated kernels) and GPU tiers.

Every entry point that produces a training loss runs on one (shape, content) case on the device under test, and so does
oracle/ssim_ref.py, in float32 and in float64, on the same inputs.  With e_dev and e_32 the device's and the float32 oracle's
distances from float64, every criterion is

    e_dev <= min(CAP, max(FLOOR, 2.5 * e_32))

for the value(s), the gradient's rel-L2 and its max-norm (max |delta| / max |g64| over pixels: one wrong pixel of a 1080p frame
moves rel-L2 by ~4e-4 of its own error, max-norm by all of it).  FLOOR is what the kernels hold on inputs whose float32 rounding is
benign; 2.5 * e_32 lets inputs where float32 itself cancels (flat regions where render = gt: sigma^2 = E[x^2] - mu^2) be judged by
what float32 can do there; CAP is never exceeded.  One float32 restatement can land near float64 by chance where float32 cancels
(a mean over a 2 x 1 "valid" map of a smooth image), so e_32 is the larger error of two: the reference's 11 x 11 convolution as
written and the same window applied as two 1-D passes, the kernels' own order.  All limits go through ops_util.bound
(GS_CALIBRATE=1 lists them).

Entry points:  fused_ssim "same" / "valid" (k_ssim_fwd / k_ssim_bwd);  fused_l1_ssim_loss (k_l1_ssim_fused, one pass) at
lambda 0, 0.2, 1;  the loss pair behind train.py's expression as written (lazy_loss.py: l1_loss + fused_ssim on the same two
tensors -> mi355gs_l1_ssim_pair_forward, the same kernel);  l1_loss on a 4-byte-misaligned view (the scalar paths of
k_l1_partial / k_l1_bwd)."""
import ctypes

import torch
import torch.nn.functional as F

from oracle import ssim_ref
from tests.ops_util import bound

CONTENTS = ("noise", "smooth", "flat_quadrant", "l1_ties", "over_one", "zeros", "const_vs_noise")

# (FLOOR, CAP) per criterion.  MI355X, GS_CALIBRATE=1, tests/test_loss_kernels_gpu.py: the largest device error on a case judged by
# the FLOOR alone was 7.9e-7 (value), 3.6e-6 (gradient rel-L2), 2.3e-6 (gradient max-norm); the largest on any case, where the
# 2.5 x e_32 term applies (smooth images, flat regions, small "valid" maps), 7.8e-6, 4.1e-5 and 6.8e-5.  Inputs and reductions are
# deterministic, so the value FLOOR stays at 1e-6 although that is only 1.3x its measurement.
LIMITS = {"value": (1e-6, 1e-5), "grad_rel": (1e-5, 5e-4), "grad_max": (1e-5, 5e-4)}
REL = 2.5   # x the float32 oracle's own error


def make_case(content, B, C, H, W, seed=0):
    """-> (img1, img2), float32 [B,C,H,W] on the CPU"""
    g = torch.Generator().manual_seed(seed)
    rand = lambda: torch.rand(B, C, H, W, generator=g)
    randn = lambda: torch.randn(B, C, H, W, generator=g)
    if content == "noise":         # what check_ssim_random draws
        x = rand()
        y = (x + 0.2 * randn()).clamp(0, 1)
    elif content == "smooth":      # noise blurred (box 9, twice): slowly varying images, small local variances
        def blur(t):
            k = torch.full((B * C, 1, 9, 9), 1.0 / 81)
            for _ in range(2):
                t = F.conv2d(F.pad(t.reshape(1, B * C, H, W), (4, 4, 4, 4), mode="replicate"), k, groups=B * C).reshape(B, C, H, W)
            return t
        x = blur(rand())
        y = blur((x + 0.3 * randn()).clamp(0, 1))
    elif content == "flat_quadrant":   # a converged patch of uniform background: render = gt = const on the top-left quadrant
        x = rand()
        y = (x + 0.2 * randn()).clamp(0, 1)
        h, w = (H + 1) // 2, (W + 1) // 2
        x[..., :h, :w] = 0.37
        y[..., :h, :w] = 0.37
    elif content == "l1_ties":     # |x - y| = 0 exactly at every 7th element (and everywhere on 1-pixel images)
        x = rand()
        y = (x + 0.2 * randn()).clamp(0, 1)
        y.view(-1)[::7] = x.view(-1)[::7]
    elif content == "over_one":    # renders are not clamped above 1
        x = 1.5 * rand()
        y = rand()
    elif content == "zeros":
        x = torch.zeros(B, C, H, W)
        y = torch.zeros(B, C, H, W)
    elif content == "const_vs_noise":
        x = torch.full((B, C, H, W), 0.3)
        y = rand()
    else:
        raise ValueError(content)
    return x.contiguous(), y.contiguous()


class Case:
    """One (shape, content) pair of inputs and its oracle results, computed once per padding and dtype."""

    def __init__(self, content, B, C, H, W, seed=0):
        self.content, self.shape = content, (B, C, H, W)
        self.x, self.y = make_case(content, B, C, H, W, seed)
        self._parts = {}

    def parts(self, padding, dtype, separable):
        key = (padding, dtype, separable)
        if key not in self._parts:
            self._parts[key] = ssim_ref.l1_ssim_parts(self.x, self.y, padding, dtype, separable)
        return self._parts[key]

    def oracle(self, lam, padding="same"):
        """-> ([the two float32 results], float64 result) of ssim_ref.l1_ssim_loss"""
        run = lambda dt, sep: ssim_ref.l1_ssim_loss(self.x, self.y, lam, padding, dt, parts=self.parts(padding, dt, sep))
        return [run(torch.float32, False), run(torch.float32, True)], run(torch.float64, True)


def _err(a, b64, kind):
    """value: |a - b64|.  Gradients: relative to max(g64, 1/n per pixel) — 1/n is the L1 term's |gradient| and the scale of every
    loss gradient here; the floor only matters where the true gradient vanishes (img1 = img2 everywhere: SSIM's maximum)."""
    d = (a.detach().cpu().double() - b64).abs()
    if kind == "value":
        return float(d.max())
    n = b64.numel()
    if kind == "grad_rel":
        return float(d.norm()) / max(float(b64.norm()), n ** -0.5)
    return float(d.max()) / max(float(b64.abs().max()), 1.0 / n)


def judge(label, kind, dev, r32s, r64):
    """e_dev <= min(CAP, max(FLOOR, 2.5 e_32)); every device output finite"""
    dev = dev.detach().cpu()
    assert bool(torch.isfinite(dev).all()), (label, kind, "non-finite device output")
    e_dev, e_32 = _err(dev, r64, kind), max(_err(r, r64, kind) for r in r32s)
    floor, cap = LIMITS[kind]
    bound("%s/%s" % (label, kind), e_dev, min(cap, max(floor, REL * e_32)))


def _label(entry, case):
    return "loss_kernels/%s[%s]" % (entry, case.content)


def check_fused_ssim(dev, case, padding):
    """fused_ssim(img1, img2, padding): the SSIM mean and d/d img1 (k_ssim_fwd, k_ssim_finish, k_ssim_bwd)"""
    from instantsplat_amd import lazy_loss
    from instantsplat_amd.fused_ssim import fused_ssim
    lazy_loss.forget()   # not the second half of a pair
    x = case.x.to(dev, copy=True).requires_grad_(True)
    v = fused_ssim(x, case.y.to(dev), padding=padding)
    v.backward()
    o32, o64 = case.oracle(1.0, padding)
    label = _label("fused_ssim_" + padding, case)
    judge(label, "value", v, [o["ssim_mean"] for o in o32], o64["ssim_mean"])
    judge(label, "grad_rel", -x.grad, [o["grad"] for o in o32], o64["grad"])   # lambda = 1: grad = -d ssim
    judge(label, "grad_max", -x.grad, [o["grad"] for o in o32], o64["grad"])


def check_fused_l1_ssim(dev, case, lam):
    """fused_l1_ssim_loss(img1, img2, lam): loss, [ssim_mean, l1_mean] and d loss / d img1 from one pass (k_l1_ssim_fused)"""
    from instantsplat_amd.fused_ssim import fused_l1_ssim_loss
    x = case.x.to(dev, copy=True).requires_grad_(True)
    loss, out = fused_l1_ssim_loss(x, case.y.to(dev), lam)
    loss.backward()
    o32, o64 = case.oracle(lam)
    label = _label("fused_l1_ssim_lam%g" % lam, case)
    judge(label, "value", loss, [o["loss"] for o in o32], o64["loss"])
    judge(label + "/ssim_mean", "value", out[0], [o["ssim_mean"] for o in o32], o64["ssim_mean"])
    judge(label + "/l1_mean", "value", out[1], [o["l1_mean"] for o in o32], o64["l1_mean"])
    judge(label, "grad_rel", x.grad, [o["grad"] for o in o32], o64["grad"])
    judge(label, "grad_max", x.grad, [o["grad"] for o in o32], o64["grad"])
    if lam == 0:   # the L1 term alone: sgn(x - y) * float32(1 / n) bit for bit, 0 at ties (the SSIM term is multiplied by -0)
        inv_n = torch.tensor(1.0 / x.numel(), dtype=torch.float32)
        want = torch.sign(case.x - case.y) * inv_n
        got = x.grad.detach().cpu()
        assert torch.equal(got, want), (label, int((got != want).sum()), "of", got.numel(), "differ")


def check_lazy_pair(dev, case, lam=0.2):
    """train.py:171-176 as written on a non-leaf image: l1_loss(image, gt), fused_ssim(image[None], gt[None]), the scalar
    expression, backward(), item() — the loss pair (mi355gs_l1_ssim_pair_forward, k_loss_program, k_loss_pair_bwd) against float64.
    The B x C planes of the case are one [B*C, H, W] image here (the shape train.py hands over)."""
    from instantsplat_amd import lazy_loss
    from instantsplat_amd.fused_ssim import fused_ssim
    from instantsplat_amd.loss_utils import l1_loss
    B, C, H, W = case.shape
    was, lazy_loss.ENABLED = lazy_loss.ENABLED, True
    try:
        leaf = case.x.reshape(B * C, H, W).to(dev, copy=True).requires_grad_(True)
        image = leaf * 1.0
        gt = case.y.reshape(B * C, H, W).to(dev)
        Ll1 = l1_loss(image, gt)
        ssim_value = fused_ssim(image.unsqueeze(0), gt.unsqueeze(0))
        assert type(Ll1) is lazy_loss.LazyScalar and type(ssim_value) is lazy_loss.LazyScalar, "the pair was not taken"
        loss = (1.0 - lam) * Ll1 + lam * (1.0 - ssim_value)
        loss.backward()
        value = torch.tensor(loss.item())
        l1v, ssv = torch.tensor(float(Ll1._rec.l1)), torch.tensor(float(ssim_value._rec.ssim))
    finally:
        lazy_loss.ENABLED = was
        lazy_loss.forget()
    o32, o64 = case.oracle(lam)
    label = _label("lazy_pair", case)
    judge(label, "value", value, [o["loss"] for o in o32], o64["loss"])
    judge(label + "/ssim_mean", "value", ssv, [o["ssim_mean"] for o in o32], o64["ssim_mean"])
    judge(label + "/l1_mean", "value", l1v, [o["l1_mean"] for o in o32], o64["l1_mean"])
    g = leaf.grad.reshape(B, C, H, W)
    judge(label, "grad_rel", g, [o["grad"] for o in o32], o64["grad"])
    judge(label, "grad_max", g, [o["grad"] for o in o32], o64["grad"])


def check_case(dev, content, B, C, H, W, seed=0, valid=True):
    """every loss entry point on one (shape, content) case (valid=False: not fused_ssim's "valid" padding, which is no training path
    and costs a second float64 oracle run)"""
    case = Case(content, B, C, H, W, seed)
    check_fused_ssim(dev, case, "same")
    if valid and H > 10 and W > 10:
        check_fused_ssim(dev, case, "valid")
    for lam in (0.0, 0.2, 1.0):
        check_fused_l1_ssim(dev, case, lam)
    check_lazy_pair(dev, case)


def check_l1_misaligned(dev, n, seed=0):
    """l1_loss on contiguous views 4 bytes past a 16-byte boundary (buf[1:n+1], n odd): the scalar paths of k_l1_partial and
    k_l1_bwd.  A 1-D shape is no loss pair, so this is the plain L1 node.  Value against float64, gradient bit for bit against
    eager PyTorch's abs(a - b).mean() (reference utils/loss_utils.py:39-40), ties included."""
    from instantsplat_amd.loss_utils import l1_loss
    assert n % 2 == 1
    g = torch.Generator().manual_seed(seed)
    abuf, bbuf = torch.rand(n + 1, generator=g), torch.rand(n + 1, generator=g)
    bbuf[1::3] = abuf[1::3]   # exact ties
    abuf, bbuf = abuf.to(dev).requires_grad_(True), bbuf.to(dev)
    a, b = abuf[1:n + 1], bbuf[1:n + 1]
    assert a.is_contiguous() and a.data_ptr() % 16 == 4 and b.data_ptr() % 16 == 4
    v = l1_loss(a, b)
    assert "L1Loss" in v.grad_fn.name(), v.grad_fn.name()
    (0.8 * v).backward()
    mine, abuf.grad = abuf.grad[1:].detach().clone(), None
    r = torch.abs(a - b).mean()
    (0.8 * r).backward()
    assert torch.equal(mine, abuf.grad[1:]), int((mine != abuf.grad[1:]).sum())
    r32 = torch.abs(a.detach().cpu() - b.cpu()).mean()
    r64 = torch.abs(a.detach().cpu().double() - b.cpu().double()).mean()
    judge("loss_kernels/l1_loss_misaligned", "value", v, [r32], r64)   # -> label .../l1_loss_misaligned/value


def plane_limit_einval(lib_path):
    """The four entry points that launch one workgroup column per (batch, channel) plane refuse 65536 planes (the grid's z
    dimension) before launching anything: -> {entry point: [return codes]} for (B, C) = (65536, 1), (1, 65536), (256, 256).
    Buffers are sized for the call (1 x 1 planes), so even an entry point that did launch would stay inside them."""
    from instantsplat_amd import _lib
    L = _lib._bind(lib_path)
    n = 65536
    bufs = [(ctypes.c_float * n)() for _ in range(6)]
    scratch = (ctypes.c_char * int(L.mi355gs_ssim_scratch_bytes(n, 1, 1, 1)))()
    f = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    s = ctypes.cast(scratch, ctypes.c_void_p)
    m = [ctypes.cast((ctypes.c_float * 2)(), ctypes.c_void_p) for _ in range(3)]
    out = {}
    for B, C in ((n, 1), (1, n), (256, 256)):
        out.setdefault("mi355gs_ssim_forward", []).append(L.mi355gs_ssim_forward(None, B, C, 1, 1, f[0], f[1], f[2], f[3], f[4], s, m[0], m[1], 0))
        out.setdefault("mi355gs_ssim_backward", []).append(L.mi355gs_ssim_backward(None, B, C, 1, 1, f[0], f[1], f[2], f[3], f[4], m[0], m[1], f[5], 0))
        out.setdefault("mi355gs_l1_ssim_loss_fused", []).append(L.mi355gs_l1_ssim_loss_fused(None, B, C, 1, 1, f[0], f[1], s, 0.2, m[0], m[1], m[2], f[5]))
        out.setdefault("mi355gs_l1_ssim_pair_forward", []).append(L.mi355gs_l1_ssim_pair_forward(None, B, C, 1, 1, f[0], f[1], s, f[5]))
    return out
