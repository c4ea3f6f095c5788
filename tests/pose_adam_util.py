"""Pose transform / pose gradient (instantsplat_amd/csrc/pose.hip, pose_math.h, the POSED projection kernels of preprocess.hip with
k_pose_finish_partials) and per-point Adam (csrc/adam.hip) against float64 oracles — checks shared by the CPU (emulated kernels)
and GPU tiers.

As in tests/loss_util.py, every criterion is   e_dev <= min(CAP, max(FLOOR, 2.5 * e_32)),   with e_dev and e_32 the distances of
the device and of a float32 restatement from float64:
  * per tensor (pose outputs, per-Gaussian gradients, Adam's parameter displacement and moments): rel-L2 and max-norm
    (max |delta| / max |ref|);
  * per pose component k, each of the 7 on its own: |d_dev - d_64| / S_k, with S_k = sum_i |c_ik| the sum of the absolute
    per-Gaussian terms of that component (oracle/pose_ref.py).  A component's rounding error scales with S_k, not with the
    component itself (translation sums cancel when the upstream gradients do), and one wrong quaternion component cannot hide
    under a translation-dominated norm.
Adam's moment gate is compared exactly: a tensor's moments change iff the reference's `grad.norm() > 0` (float32, on the device
under test) holds.  All limits go through ops_util.bound (GS_CALIBRATE=1 lists them)."""
import math

import torch

from oracle import adam_ref, pose_ref
from tests.ops_util import bound, generic_start

# (FLOOR, CAP) per criterion.  MI355X, GS_CALIBRATE=1, tests/test_pose_adam_gpu.py — largest device error on a case judged by the
# FLOOR alone / on any case:
#   pose_out   2.5e-7 / 2.5e-7   (the four outputs)
#   pose_grad  3.0e-7 / 3.0e-7   (the four per-Gaussian gradients)
#   pose_sum   3.7e-6 / 6.0e-6   (x S_k; the largest where ONE Gaussian contributes: its quaternion terms pass through the
#                                 projection onto the tangent of q / |q|, which cancels; 1.6e-9 at P = 1,048,577)
#   posed_sum  1.6e-7 / 1.6e-7   (x S_k; posed render node, reduction consistency at up to 3,888 rows and end to end)
#   adam       1.3e-5 / 1.8e-5   (exp_avg_sq: betas cross the C ABI as float32, and 1 - 0.999f is 1.3e-5 below the reference's
#                                 1 - 0.999; the displacement carries half of it through sqrt(v))
LIMITS = {
    "pose_out": (1e-6, 1e-4),
    "pose_grad": (1e-6, 1e-4),
    "pose_sum": (1e-5, 1e-4),
    "posed_sum": (1e-6, 1e-4),
    "adam": (3e-5, 1e-4),
}
REL = 2.5


def _errs(a, b64, scale=None):
    """-> (rel-L2, max-norm) of a against b64, each relative to the larger of b64 and `scale` (a tensor of b64's shape: where the
    reference itself is far below the size of its inputs); an all-zero reference must be matched exactly"""
    d = a.detach().cpu().double() - b64
    if d.numel() == 0:
        return 0.0, 0.0
    tiny = 1e-300
    sn, sm = (0.0, 0.0) if scale is None else (float(scale.norm()), float(scale.abs().max()))
    return float(d.norm()) / max(float(b64.norm()), sn, tiny), float(d.abs().max()) / max(float(b64.abs().max()), sm, tiny)


def judge(group, label, dev, r32, r64, scale=None):
    dev = dev.detach().cpu()
    assert bool(torch.isfinite(dev).all()), (label, "non-finite device output")
    floor, cap = LIMITS[group]
    for kind, e_dev, e_32 in zip(("rel", "max"), _errs(dev, r64, scale), _errs(r32, r64, scale)):
        bound("%s/%s" % (label, kind), e_dev, min(cap, max(floor, REL * e_32)))


def judge_components(group, label, d_dev, d_32, d_64, S):
    """per pose component: |d_dev - d_64| <= min(CAP S_k, max(FLOOR S_k, 2.5 |d_32 - d_64|)); group: a key of LIMITS or (FLOOR, CAP)"""
    floor, cap = LIMITS[group] if isinstance(group, str) else group
    d_dev, d_32 = d_dev.detach().cpu().double().reshape(7), d_32.detach().cpu().double().reshape(7)
    assert bool(torch.isfinite(d_dev).all()), (label, d_dev)
    for k in range(7):
        s = float(S[k])
        e_dev, e_32 = abs(float(d_dev[k] - d_64[k])), abs(float(d_32[k] - d_64[k]))
        if s == 0.0:   # no Gaussian contributes: exactly zero
            assert e_dev == 0.0, (label, k, float(d_dev[k]))
            continue
        bound("%s/q%d" % (label, k) if k < 4 else "%s/t%d" % (label, k - 4), e_dev / s, min(cap, max(floor, REL * e_32 / s)))


# ================================================================ pose: the stand-alone op (fused.pose_activations)

POSES = ("identity", "unit", "tiny_q", "huge_q", "neg_w", "near_180", "far")
UPSTREAM = ("random", "absent_means", "absent_rot", "absent_scales", "absent_opac", "single", "cancel")


def make_pose(kind, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    q, t = rn(4), rn(3)
    q = q / q.norm()
    if kind == "identity":
        return torch.tensor([1.0, 0, 0, 0, 0, 0, 0])
    if kind == "tiny_q":
        q = q * 1e-3
    elif kind == "huge_q":
        q = q * 1e3
    elif kind == "neg_w":
        q[0] = -abs(float(q[0])) - 0.3
    elif kind == "near_180":   # w ~ 0: a rotation by ~180 degrees about (x, y, z)
        q[0] = 1e-4
    elif kind == "far":
        t = t / t.norm() * 1e3
    return torch.cat([q, t]).float()


def make_gaussians(P, seed=0):
    """xyz of order 1; raw quaternions of norm 0.3 .. 3 with every 7th row zero; log-scales over [-20, 10]; opacity logits of
    order 3 with every 5th at +-30"""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(P, 3, generator=g)
    rot = torch.randn(P, 4, generator=g)
    rot = rot / rot.norm(dim=1, keepdim=True).clamp_min(1e-12) * (0.3 + 2.7 * torch.rand(P, 1, generator=g))
    rot[::7] = 0.0
    scaling = -20.0 + 30.0 * torch.rand(P, 3, generator=g)
    opl = 3.0 * torch.randn(P, 1, generator=g)
    opl[::5] = 30.0
    opl[2::10] = -30.0
    return xyz, rot, scaling, opl


def make_upstream(kind, P, seed=0):
    """-> [g_means, g_rot, g_scales, g_opac] (None: that output takes no part in the loss)"""
    g = torch.Generator().manual_seed(2000 + seed)
    gs = [torch.randn(P, n, generator=g) for n in (3, 4, 3, 1)]
    if kind.startswith("absent_"):
        gs[("means", "rot", "scales", "opac").index(kind[7:])] = None
    elif kind == "single":
        j = P // 2
        for x in gs:
            keep = x[j].clone()
            x.zero_()
            x[j] = keep
    elif kind == "cancel":   # sum_i g_means ~ 0: dL/dt is small against its terms
        gs[0] = gs[0] - gs[0].mean(dim=0, keepdim=True)
    return gs


def check_pose_op(dev, P, pose_kind, up_kind, seed=0, misaligned=False):
    """fused.pose_activations forward and backward on one case against pose_ref in float64 (float32: the reference's graph)."""
    from instantsplat_amd.fused import pose_activations
    xyz, rot, scaling, opl = make_gaussians(P, seed)
    pose = make_pose(pose_kind, seed)
    ups = make_upstream(up_kind, P, seed) if P else [torch.zeros(0, n) for n in (3, 4, 3, 1)]
    r64 = pose_ref.reference(xyz, rot, scaling, opl, pose, ups, torch.float64)
    r32 = pose_ref.reference(xyz, rot, scaling, opl, pose, ups, torch.float32)

    t = [v.to(dev).requires_grad_(True) for v in (xyz, rot, scaling, opl, pose)]
    rot_in = t[1]
    if misaligned:   # rot as a contiguous view 4 bytes past a 16-byte boundary: the wrapper must copy it before a float4 kernel reads it
        buf = torch.zeros(4 * P + 1, device=dev)
        buf[1:].copy_(rot.detach().reshape(-1))
        buf.requires_grad_(True)
        rot_in = buf[1:].view(P, 4)
        assert rot_in.is_contiguous() and rot_in.data_ptr() % 16 == 4
    outs = pose_activations(t[0], rot_in, t[2], t[3], t[4])
    loss = sum((o * u.to(dev)).sum() for o, u in zip(outs, ups) if u is not None)
    if torch.is_tensor(loss) and loss.requires_grad:
        loss.backward()
    grads = [v.grad if v.grad is not None else torch.zeros_like(v) for v in t]
    if misaligned:
        grads[1] = buf.grad[1:].view(P, 4)
    label = "pose_op/P%d/%s/%s" % (P, pose_kind, up_kind) + ("/misaligned" if misaligned else "")
    for name, o, o32, o64 in zip(("means", "rot", "scales", "opac"), outs, r32["out"], r64["out"]):
        assert o.shape == o64.shape, (label, name)
        judge("pose_out", "%s/out_%s" % (label, name), o, o32, o64)
    # d_opacity = g o (1 - o): at logits of +-30, float32's o (1 - o) is 0 or its ulp, float64's 1e-13 — judged against the largest
    # value it can take, g / 4
    scales = (None, None, None, None if ups[3] is None else 0.25 * ups[3].double())
    for name, d, d32, d64, sc in zip(("xyz", "rot", "scaling", "opacity"), grads[:4], r32["d"], r64["d"], scales):
        judge("pose_grad", "%s/d_%s" % (label, name), d, d32, d64, sc)
    c = r64["c"]
    S = c.abs().sum(0)
    assert torch.allclose(c.sum(0), r64["d_pose"], rtol=1e-12, atol=1e-12 * float(S.max() + 1))   # the terms sum to autograd's gradient
    judge_components("pose_sum", label + "/d_pose", grads[4], r32["d_pose"], r64["d_pose"], S)


# ================================================================ pose: the posed render node (default glue)

def _posed_state(dev, V, Wm, W, H, seed):
    from instantsplat_amd.synthetic import syn_pointmap
    from instantsplat_amd.train import setup_training
    return generic_start(setup_training(syn_pointmap(V, Wm, Wm, W, H, seed=seed), dev))


def check_posed_pose_reduction(dev, V, Wm, W=32, H=24, seed=0):
    """render(..., camera_pose=g.get_RT(uid)) and a random linear loss of the image: the pose gradient the node's last kernel
    (k_pose_finish_partials) reduces from the per-workgroup rows must be the float64 sum of the per-Gaussian terms, rebuilt from
    the node's own raw-parameter gradients (g_m = R d_xyz, g_r = H(q) d_rot / |q|^2).  Needs no rasterizer oracle."""
    from instantsplat_amd.gaussian_renderer import render
    st = _posed_state(dev, V, Wm, W, H, seed)
    g = st.gaussians
    P = g._xyz.shape[0]
    cam = st.cameras[V // 2]
    img = render(cam, g, st.pipe, st.background, camera_pose=g.get_RT(cam.uid))["render"]
    w = torch.randn(img.shape, generator=torch.Generator().manual_seed(seed)).to(dev)
    (img * w).sum().backward()
    table = g.P.grad.detach().cpu()
    others = torch.cat([table[:cam.uid], table[cam.uid + 1:]])
    assert bool((others == 0).all()), "rows of other cameras must be zero"
    pose = g.P.detach()[cam.uid].cpu()
    d_xyz, d_rot = g._xyz.grad.detach().cpu(), g._rotation.grad.detach().cpu()
    xyz, rot = g._xyz.detach().cpu(), g._rotation.detach().cpu()
    terms = {}
    for dt in (torch.float64, torch.float32):
        gm, gr = pose_ref.camera_frame_grads(pose.to(dt), d_xyz.to(dt), d_rot.to(dt))
        terms[dt] = pose_ref.pose_terms(xyz.to(dt), rot.to(dt), pose.to(dt), gm, gr)
    c = terms[torch.float64]
    assert float(c.abs().sum()) > 0, "no Gaussian reached the image"
    judge_components("posed_sum", "posed_node/V%d_Wm%d_P%d/d_pose" % (V, Wm, P), table[cam.uid], terms[torch.float32].sum(0), c.sum(0),
                     c.abs().sum(0))


def check_posed_pose_end_to_end(dev, V=3, Wm=12, W=32, H=24, seed=0):
    """one frame of the training loss (0.8 L1 + 0.2 (1 - SSIM)) through the posed node: its pose gradient against
    ops_util.oracle_frame_grads in float64 (the float32 oracle sets the 2.5x term), per component, S_k from the float64 oracle's
    own per-Gaussian terms."""
    from instantsplat_amd.fused_ssim import fused_l1_ssim_loss
    from instantsplat_amd.gaussian_renderer import render
    from tests.ops_util import oracle_frame_grads
    st = _posed_state(dev, V, Wm, W, H, seed)
    g = st.gaussians
    cam = st.cameras[1 % V]
    params = dict(xyz=g._xyz, f_dc=g._features_dc, f_rest=g._features_rest, opacity=g._opacity, scaling=g._scaling,
                  rotation=g._rotation, pose=g.P)
    img = render(cam, g, st.pipe, st.background, camera_pose=g.get_RT(cam.uid))["render"]
    loss, _ = fused_l1_ssim_loss(img.unsqueeze(0), st.gt_images[cam.uid].unsqueeze(0), 0.2)
    loss.backward()
    o64 = oracle_frame_grads(params, cam, st.gt_images[cam.uid], torch.float64)
    o32 = oracle_frame_grads(params, cam, st.gt_images[cam.uid], torch.float32)
    pose = g.P.detach()[cam.uid].cpu().double()
    gm, gr = pose_ref.camera_frame_grads(pose, o64["xyz"], o64["rotation"])
    c = pose_ref.pose_terms(g._xyz.detach().cpu().double(), g._rotation.detach().cpu().double(), pose, gm, gr)
    assert torch.allclose(c.sum(0), o64["pose"][cam.uid], rtol=1e-9, atol=1e-12 * float(c.abs().sum()))
    judge_components("posed_sum", "posed_e2e/V%d_Wm%d/d_pose" % (V, Wm), g.P.grad[cam.uid], o32["pose"][cam.uid], o64["pose"][cam.uid],
                     c.abs().sum(0))


# ================================================================ Adam

def _run_step(entry, opt, params, grads, lrs, L=None, dev=None):
    """one optimizer step of every tensor through `entry`"""
    if entry == "raw":   # mi355gs_adam_step (k_adam), one call per tensor, with the caller's float32 sum of squares
        from instantsplat_amd import _lib
        for p, gr, lr, grp in zip(params, grads, lrs, opt.param_groups):
            st = opt.state[p]
            if not st:
                st["step"], st["exp_avg"], st["exp_avg_sq"] = 0, torch.zeros_like(p), torch.zeros_like(p)
            st["step"] += 1
            pp = grp.get("per_point_lr")
            sumsq = (gr * gr).sum().reshape(1)
            b1, b2 = grp["betas"]
            with _lib.on_device(dev):
                _lib.check(L.mi355gs_adam_step(_lib.stream_ptr(dev), p.numel(), p.numel() // p.shape[0] if pp is not None else 1,
                                               _lib.ptr(p.data), _lib.ptr(gr), _lib.ptr(st["exp_avg"]), _lib.ptr(st["exp_avg_sq"]),
                                               _lib.ptr(pp), _lib.ptr(sumsq), float(lr), b1, b2, float(grp["eps"]), st["step"]), "adam_step")
        return
    for p, gr in zip(params, grads):
        p.grad = gr
    opt.step()


class AdamRun:
    """Device PerPointAdam (one param group per tensor) next to its float64 and float32 oracle twins (oracle/adam_ref.update_).

    specs: list of dict(shape, pplr=None | float32 [rows] CPU tensor, betas=(0.9, 0.999), eps=1e-15, wd=0.0, lr=1e-3)."""

    def __init__(self, dev, entry, specs, seed=0, label="adam"):
        from instantsplat_amd.optim import PerPointAdam
        self.dev, self.entry, self.specs, self.label = dev, entry, specs, label
        g = torch.Generator().manual_seed(seed)
        # parameters of the size of a few steps: the float32 rounding of an O(1) parameter (6e-8) is 1e-3 of a 1e-4 step, and the
        # displacement would measure that instead of the update
        self.p0 = [1e-3 * torch.randn(s["shape"], generator=g) for s in specs]
        self.params = [p.clone().to(dev).requires_grad_(True) for p in self.p0]
        groups = []
        for s, p in zip(specs, self.params):
            grp = {"params": [p], "lr": s.get("lr", 1e-3), "betas": s.get("betas", (0.9, 0.999)), "eps": s.get("eps", 1e-15),
                   "weight_decay": s.get("wd", 0.0)}
            if s.get("pplr") is not None:
                grp["per_point_lr"] = s["pplr"].reshape((s["shape"][0],) + (1,) * (len(s["shape"]) - 1)).to(dev)
            groups.append(grp)
        self.opt = PerPointAdam(groups, lr=0.0, betas=(0.9, 0.999), eps=1e-15)
        self.ref = {dt: [dict(p=p.to(dt).clone(), m=torch.zeros_like(p, dtype=dt), v=torch.zeros_like(p, dtype=dt), step=0) for p in self.p0]
                    for dt in (torch.float64, torch.float32)}
        self.L = None
        if entry == "raw":
            from instantsplat_amd import _lib
            self.L = _lib.lib()
        self.k = 0

    def _moments(self, i):
        st = self.opt.state.get(self.params[i])
        if not st:
            return None
        return st["exp_avg"].detach().cpu().clone(), st["exp_avg_sq"].detach().cpu().clone()

    def step(self, grads, lrs=None, misaligned=()):
        """grads: float32 CPU tensors (one per spec); misaligned: indices handed over as views 4 bytes past a 16-byte boundary"""
        self.k += 1
        lrs = lrs or [s.get("lr", 1e-3) for s in self.specs]
        for grp, lr in zip(self.opt.param_groups, lrs):
            grp["lr"] = lr
        gdev, gates, before = [], [], []
        for i, (gr, s, p) in enumerate(zip(grads, self.specs, self.params)):
            gd = gr.to(self.dev)
            if i in misaligned:
                buf = torch.zeros(gr.numel() + 1, device=self.dev)
                buf[1:].copy_(gd.reshape(-1))
                gd = buf[1:].view(gr.shape)
                assert gd.is_contiguous() and gd.data_ptr() % 16 == 4
            eff = gd.add(p.detach(), alpha=s["wd"]) if s.get("wd", 0.0) else gd
            gates.append(bool(eff.norm() > 0))   # the reference's gate, float32 on the device under test
            gdev.append(gd)
            before.append((self._moments(i), p.detach().cpu().clone()))
        _run_step(self.entry, self.opt, self.params, gdev, lrs, self.L, self.dev)
        for dt, refs in self.ref.items():
            for r, gr, s, lr, gate, grp in zip(refs, grads, self.specs, lrs, gates, self.opt.param_groups):
                r["step"] += 1
                pp = s.get("pplr")
                pp = None if pp is None else pp.reshape((s["shape"][0],) + (1,) * (len(s["shape"]) - 1))
                adam_ref.update_(r["p"], gr, r["m"], r["v"], r["step"], lr, grp["betas"], grp["eps"], pp, s.get("wd", 0.0), gate)
        for i, (gate, (mv, p_before)) in enumerate(zip(gates, before)):
            m1, v1 = self._moments(i)
            m0, v0 = mv if mv is not None else (torch.zeros_like(m1), torch.zeros_like(v1))
            moved = not (torch.equal(m0, m1) and torch.equal(v0, v1))
            assert moved == gate, (self.label, "step", self.k, "tensor", i, "moment gate", moved, "reference", gate)
            if not gate and not bool(m0.any()):   # gated off with a zero first moment: p - s * (0 / denom) == p, bit for bit
                assert torch.equal(self.params[i].detach().cpu(), p_before), (self.label, self.k, i, "parameter moved")
        return gates

    def rewrite_moments(self, i, fn):
        """fn(m, v) edits one tensor's moments in place; applied to the device state (under no_grad) and to both oracles"""
        with torch.no_grad():
            st = self.opt.state[self.params[i]]
            fn(st["exp_avg"], st["exp_avg_sq"])
        for refs in self.ref.values():
            m, v = refs[i]["m"], refs[i]["v"]
            m32, v32 = m.float(), v.float()   # the device holds float32 moments: edit the float32 values, as the device does
            fn(m32, v32)
            m.copy_(m32)
            v.copy_(v32)

    def check(self, tag=""):
        for i, p in enumerate(self.params):
            st = self.opt.state[p]
            p0 = self.p0[i].double()
            lab = "%s/%s/t%d%s" % (self.label, self.entry, i, tag)
            r64, r32 = self.ref[torch.float64][i], self.ref[torch.float32][i]
            assert st["step"] == r64["step"], (lab, st["step"], r64["step"])
            judge("adam", lab + "/displacement", p.detach().cpu().double() - p0, r32["p"].double() - p0, r64["p"] - p0, _ulps(r64["p"]))
            judge("adam", lab + "/exp_avg", st["exp_avg"], r32["m"], r64["m"])
            judge("adam", lab + "/exp_avg_sq", st["exp_avg_sq"], r32["v"], r64["v"])


def _ulps(p):
    """The displacement's scale where the parameter's own float32 rounding dominates it (an O(1) pose moved by 1e-4: one ulp is
    1e-3 of the step): two ulps of the parameter count as an error of FLOOR.  A wrong step still shows at ~1e-2."""
    return 2.0 * 2.0 ** -23 * p.abs() / LIMITS["adam"][0]


def _binding(entry):
    import contextlib
    from tests.ops_util import _with_binding
    if entry == "ctypes":
        return _with_binding("ctypes")
    if entry == "compiled":
        return _with_binding("compiled")
    return contextlib.nullcontext()


def pplr_rows(n, seed):
    """per-point multipliers in [0, 2) with every 4th zero"""
    x = 2.0 * torch.rand(n, generator=torch.Generator().manual_seed(seed))
    x[::4] = 0.0
    return x


def edge_specs():
    """numel 1, 3, 4, 5, 2047, 2048, 2049, 8195 and a float4 tensor with 45-float rows; per-point rows of 1, 3, 4 and 45"""
    return [dict(shape=(1, 1), pplr=pplr_rows(1, 1) + 0.5), dict(shape=(1, 3), pplr=pplr_rows(1, 2) + 0.5), dict(shape=(1, 4), pplr=pplr_rows(1, 3) + 0.5),
            dict(shape=(5,)), dict(shape=(2047, 1), pplr=pplr_rows(2047, 4)), dict(shape=(512, 4), pplr=pplr_rows(512, 5)),
            dict(shape=(2049,)), dict(shape=(8195,)), dict(shape=(48, 45), pplr=pplr_rows(48, 6))]


def c3_specs():
    """C3's seven parameter tensors (3 x 256^2 Gaussians at SH degree 3) and its 3 x 7 pose table"""
    n = 3 * 256 * 256
    return [dict(shape=(n, 3), pplr=pplr_rows(n, 7)), dict(shape=(n, 1, 3)), dict(shape=(n, 15, 3)), dict(shape=(n, 1)),
            dict(shape=(n, 3)), dict(shape=(n, 4)), dict(shape=(3, 7))]


def _grad(shape, kind, gen):
    x = torch.randn(shape, generator=gen)
    if kind == "rand":
        return x
    if kind == "zero":
        return torch.zeros(shape)
    if kind == "tiny":   # squares underflow to 0 in float32: the reference's float32 norm is 0
        return 1e-23 * torch.sign(x)
    if kind == "nan":   # one NaN next to non-zero elements (in another 2048-element chunk when there is one)
        x.view(-1)[min(5, x.numel() - 1)] = float("nan")
        return x
    raise ValueError(kind)


GATE_SCHEDULE = (  # per step: the gradient kind of tensor i is SCHEDULE[k][i % len]
    ("rand",), ("zero", "rand", "tiny"), ("rand", "zero"), ("tiny", "rand", "zero"), ("nan", "rand"), ("rand",), ("zero",),
)


def check_adam_gates(dev, entry, specs, seed=0, misaligned=(), label="adam_gates"):
    """seven steps over the gate schedule (zero gradients with and without a first moment, underflowing squares, a NaN):
    gate outcomes exact, displacement and moments against float64 after every step"""
    with _binding(entry):
        run = AdamRun(dev, entry, specs, seed=seed, label=label)
        gen = torch.Generator().manual_seed(seed + 1)
        for k, row in enumerate(GATE_SCHEDULE):
            kinds = [row[i % len(row)] for i in range(len(specs))]
            # torch's float32 norm of ONE element is |x| itself, not sqrt(x^2): the reference's gate is x != 0 there, the kernels'
            # sum of squares underflows.  No parameter tensor has one element; underflow is tested on all the others.
            kinds = ["zero" if kd == "tiny" and math.prod(s["shape"]) == 1 else kd for kd, s in zip(kinds, specs)]
            grads = [_grad(s["shape"], kd, gen) for kd, s in zip(kinds, specs)]
            run.step(grads, misaligned=misaligned)
            run.check("/step%d" % (k + 1))
        if entry == "compiled" and len(specs) <= 8 and len({(s.get("betas"), s.get("eps")) for s in specs}) == 1:
            assert run.opt.__dict__.get("_fast") is not None, "the steady-state path was not taken"
    return run


def check_adam_live_memory(dev, entry="compiled", seed=0):
    """gated-off tensors whose moments the caller rewrites between steps — in place under no_grad (as train.py:_restore does)
    and through load_state_dict: the next step must use the new moments, not the library's memory of a zero first moment"""
    specs = [dict(shape=(1024, 4)), dict(shape=(2049,)), dict(shape=(7,))]
    gen = torch.Generator().manual_seed(seed)
    zero = lambda: [torch.zeros(s["shape"]) for s in specs]
    with _binding(entry):
        run = AdamRun(dev, entry, specs, seed=seed, label="adam_live")
        for _ in range(3):   # gated off from the start: the memory records "scanned, first moment zero"
            run.step(zero())
        run.check("/zero")
        for i, s in enumerate(specs):
            M, A = 1e-3 * torch.randn(s["shape"], generator=gen), 1e-6 * torch.rand(s["shape"], generator=gen)
            run.rewrite_moments(i, lambda m, v, M=M, A=A: (m.copy_(M.to(m.device)), v.add_(A.to(v.device))))
        run.step(zero())
        run.check("/after_copy")
        run.step(zero())
        run.step([_grad(s["shape"], "rand", gen) for s in specs])   # gate on once, then off again
        run.step(zero())
        run.rewrite_moments(0, lambda m, v: m.add_(5e-4))
        run.step(zero())
        run.check("/after_add")
        # load_state_dict with new moments for a gated-off tensor
        sd = run.opt.state_dict()
        for i, st in sd["state"].items():
            m = 2e-3 * torch.randn(st["exp_avg"].shape, generator=gen)
            v = 1e-6 + 1e-6 * torch.rand(st["exp_avg_sq"].shape, generator=gen)
            st["exp_avg"], st["exp_avg_sq"] = m.to(dev, copy=True), v.to(dev, copy=True)
            for refs in run.ref.values():
                refs[i]["m"].copy_(m)
                refs[i]["v"].copy_(v)
        run.opt.load_state_dict(sd)
        run.step(zero())
        run.check("/after_load_state_dict")
        run.step([_grad(s["shape"], "rand", gen) for s in specs])
        run.check("/end")


def check_adam_trajectory(dev, entry, steps=3000, checkpoints=(1, 2, 10, 100, 1000, 3000), start_step=0, seed=0):
    """a training run's schedule: exponential LR decay (1.6e-4 -> 1.6e-6), eps 1e-15, each tensor gated off at random on ~20 % of
    the steps; start_step > 0 resumes from a state_dict at that step with non-zero moments"""
    from instantsplat_amd.optim import get_expon_lr_func
    specs = [dict(shape=(4,)), dict(shape=(5,)), dict(shape=(2049,)), dict(shape=(16, 45), pplr=pplr_rows(16, 9)), dict(shape=(3, 7))]
    sched = get_expon_lr_func(1.6e-4, 1.6e-6, max_steps=start_step + steps)
    gen = torch.Generator().manual_seed(seed)
    with _binding(entry):
        run = AdamRun(dev, entry, specs, seed=seed, label="adam_traj%s" % ("_from%d" % start_step if start_step else ""))
        if start_step:
            for i, p in enumerate(run.params):
                m = 1e-3 * torch.randn(p.shape, generator=gen)
                v = 1e-6 * torch.rand(p.shape, generator=gen) + 1e-8
                run.opt.state[p] = dict(step=start_step, exp_avg=m.to(dev, copy=True), exp_avg_sq=v.to(dev, copy=True))
                for refs in run.ref.values():
                    refs[i].update(step=start_step, m=m.to(refs[i]["p"].dtype, copy=True), v=v.to(refs[i]["p"].dtype, copy=True))
            run.opt.load_state_dict(run.opt.state_dict())
        for k in range(1, steps + 1):
            off = torch.rand(len(specs), generator=gen) < 0.2
            grads = [torch.zeros(s["shape"]) if bool(o) else 1e-3 * torch.randn(s["shape"], generator=gen) for s, o in zip(specs, off)]
            run.step(grads, lrs=[sched(start_step + k)] * len(specs))
            if k in checkpoints:
                run.check("/step%d" % (start_step + k))


def check_adam_after_posed_backward(dev, V=3, Wm=12, W=32, H=24, seed=0):
    """the compiled plan after a real posed backward: the gate flags the backward left take the place of the pass over the
    gradients, the pose table (no flag, 21 floats) is gated by the workgroup that owns it (the -2 path).  Second iteration: a NaN in
    a row of the pose table the frame did not touch — the reference's gate is off there, so the table's moments stay frozen."""
    from instantsplat_amd.fused_ssim import fused_l1_ssim_loss
    from instantsplat_amd.gaussian_renderer import render
    from instantsplat_amd.arguments import OptimizationParams
    from instantsplat_amd.synthetic import syn_pointmap
    from instantsplat_amd.train import setup_training
    with _binding("compiled"):
        st = generic_start(setup_training(syn_pointmap(V, Wm, Wm, W, H, seed=seed), dev,
                                          opt=OptimizationParams(iterations=1000, pp_optimizer=True, optim_pose=True)))
        g = st.gaussians
        g.update_learning_rate(1)
        opt = g.optimizer
        params = [p for grp in opt.param_groups for p in grp["params"]]
        groups = [grp for grp in opt.param_groups for _ in grp["params"]]
        p0 = [p.detach().cpu().double().clone() for p in params]
        refs = {dt: [dict(p=p.detach().cpu().to(dt).clone(), m=torch.zeros(p.shape, dtype=dt), v=torch.zeros(p.shape, dtype=dt)) for p in params]
                for dt in (torch.float64, torch.float32)}
        for it in range(2):
            cam = st.cameras[it % V]
            img = render(cam, g, st.pipe, st.background, camera_pose=g.get_RT(cam.uid))["render"]
            loss, _ = fused_l1_ssim_loss(img.unsqueeze(0), st.gt_images[cam.uid].unsqueeze(0), 0.2)
            loss.backward()
            if it == 1:
                with torch.no_grad():
                    g.P.grad[(cam.uid + 1) % V, 2] = float("nan")
            grads = [p.grad.detach().cpu().clone() for p in params]
            gates = [bool(p.grad.norm() > 0) for p in params]
            before = [None if not opt.state.get(p) else (opt.state[p]["exp_avg"].cpu().clone(), opt.state[p]["exp_avg_sq"].cpu().clone())
                      for p in params]
            opt.step()
            plan = [b.get("compiled") for pl in opt._plans.values() for b in pl["batches"]][0]
            assert plan is not None and plan.last_used_gates > 0, "the backward's gate flags were not used"
            for i, (p, grp) in enumerate(zip(params, groups)):
                stp = opt.state[p]
                for dt, rr in refs.items():
                    r = rr[i]
                    pp = grp.get("per_point_lr")
                    adam_ref.update_(r["p"], grads[i], r["m"], r["v"], stp["step"], grp["lr"], grp["betas"], grp["eps"],
                                     None if pp is None else pp.detach().cpu(), grp["weight_decay"], gates[i])
                m0, v0 = before[i] if before[i] is not None else (torch.zeros(p.shape), torch.zeros(p.shape))
                moved = not (torch.equal(m0, stp["exp_avg"].cpu()) and torch.equal(v0, stp["exp_avg_sq"].cpu()))
                assert moved == gates[i], ("iteration", it, grp.get("name"), "moment gate", moved, "reference", gates[i])
                lab = "adam_posed/it%d/%s" % (it, grp.get("name"))
                r64, r32 = refs[torch.float64][i], refs[torch.float32][i]
                judge("adam", lab + "/displacement", p.detach().cpu().double() - p0[i], r32["p"].double() - p0[i], r64["p"] - p0[i],
                      _ulps(r64["p"]))
                judge("adam", lab + "/exp_avg", stp["exp_avg"], r32["m"], r64["m"])
                judge("adam", lab + "/exp_avg_sq", stp["exp_avg_sq"], r32["v"], r64["v"])
            opt.zero_grad(set_to_none=True)
        assert not gates[-1] and groups[-1].get("name") == "pose", "the NaN pose-table gradient must gate its moments off"
