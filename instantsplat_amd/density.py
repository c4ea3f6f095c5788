"""Adaptive density control on the device — reference scene/gaussian_model.py:328-477 (`add_densification_stats`,
`densify_and_clone`, `densify_and_split`, `prune_points`, `densify_and_prune`, `reset_opacity` and the optimizer surgery below
them) over csrc/density.hip (include/mi355gs.h mi355gs_density_* / mi355gs_reset_opacity).  `scene.GaussianModel` carries the
reference's method names; they call into this module.

One event — any of clone, split and prune — is one plan call (the per-Gaussian decisions, per-block counts and their scan), one
read-back of 16 words through pinned host memory (the new P and the number of split rows size the new buffers and the normal
samples) and one apply call that reads every row of the 6 per-Gaussian parameter tensors, their 12 Adam moments, the per-point
learning rates and the three statistics once and writes every row of the new tensors once.  The torch-eager form of the same event is some
forty boolean-index, `cat` and `zeros_like` launches, each a full copy.  There is no CPU fallback.

Not the reference's: the per-point learning-rate row of `PerPointAdam` is resized with the model — a survivor keeps its rate, a
clone or child inherits its parent's.  The reference never resizes that tensor (a pruned model fails in its next optimizer
step); the rule is this package's choice.  `torch.cuda.empty_cache()` at the end of `densify_and_prune` is not reproduced.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _lib

CLONE, SPLIT, PRUNE, SCREEN = 1, 2, 4, 8   # include/mi355gs.h MI355GS_DENSITY_*
MAX_N = 8
N_TENSORS = 22
EXP_AVG, EXP_AVG_SQ, PER_POINT_LR, GRAD_ACCUM, DENOM, MAX_RADII = 6, 12, 18, 19, 20, 21
# (optimizer group, model attribute) in the order of MI355GS_DENSITY_XYZ .. MI355GS_DENSITY_ROTATION
PARAMS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
          ("scaling", "_scaling"), ("rotation", "_rotation"))
TOTAL_NAMES = ("originals", "clones", "children", "pruned", "split", "new_P", "clone_selected")


def _groups(model):
    """name -> (param group, its state dict or None) for the six per-Gaussian groups of the model's optimizer"""
    out = {}
    opt = model.optimizer
    if opt is None:
        return out
    names = {n for n, _ in PARAMS}
    for group in opt.param_groups:
        if group.get("name") in names:
            if len(group["params"]) != 1:
                raise RuntimeError(f"density control needs one tensor per param group, '{group['name']}' has {len(group['params'])}")
            st = opt.state.get(group["params"][0], None)
            out[group["name"]] = (group, st if st else None)
    return out


def _forget_optimizer_caches(opt):
    """PerPointAdam keys its launch plans and its fast path on the identity of the parameters and moments (optim.py), and the
    compiled binding remembers which gradient tensors the last backward wrote: all of them describe tensors that are gone."""
    if hasattr(opt, "_plans"):
        opt._plans = {}
    if hasattr(opt, "_fast"):
        opt._fast = None
    if _lib._EXT is not None:
        _lib._EXT.forget_gates()


def _stat(t, P, shape):
    """a statistics tensor as the kernels take it, or None when the model does not carry it at this P (a model that was never
    set up for training holds empty placeholders)"""
    if not isinstance(t, torch.Tensor) or t.numel() != P or t.dtype is not torch.float32:
        return None
    return t.reshape(shape).contiguous()


def add_stats(model, viewspace_point_tensor, update_filter, radii=None):
    """`add_densification_stats` (:476-478) and, with `radii`, the max_radii2D update of train.py:198, in one launch."""
    grad = viewspace_point_tensor.grad if isinstance(viewspace_point_tensor, torch.Tensor) and viewspace_point_tensor.grad is not None \
        else None
    if grad is None:
        raise RuntimeError("add_densification_stats: viewspace_point_tensor has no .grad (call it after loss.backward())")
    P = int(model._xyz.shape[0])
    if grad.dim() != 2 or grad.shape[0] != P or grad.shape[1] < 2:
        raise ValueError(f"add_densification_stats: the screen-space gradient must be [{P}, >= 2], got {list(grad.shape)}")
    grad = _lib.f32c(grad)
    filt = update_filter
    if filt.dtype is torch.bool:
        filt = filt.view(torch.uint8)
    if filt.dtype is not torch.uint8 or filt.numel() != P:
        raise ValueError("add_densification_stats: update_filter must be a bool mask with one entry per Gaussian")
    filt = filt.contiguous()
    accum, denom = _stat(model.xyz_gradient_accum, P, (P, 1)), _stat(model.denom, P, (P, 1))
    if accum is None or denom is None:
        raise RuntimeError("add_densification_stats: the model carries no statistics (training_setup creates them)")
    maxr = None
    if radii is not None:
        if radii.numel() != P:
            raise ValueError("add_densification_stats: radii must have one entry per Gaussian")
        radii = radii.to(torch.int32).contiguous()
        maxr = _stat(model.max_radii2D, P, (P,))
        if maxr is None:
            raise RuntimeError("add_densification_stats: the model carries no max_radii2D")
    dev = _lib.require_device(grad, filt, accum, denom, radii, maxr)
    if P == 0:
        return
    _lib.call(dev, "density_stats", _lib.STREAM, P, grad, int(grad.shape[1]), filt, radii, accum, denom, maxr)
    # (reshape / contiguous hand back the same storage for the layouts training_setup creates; anything else is written back)
    for name, t in (("xyz_gradient_accum", accum), ("denom", denom), ("max_radii2D", maxr)):
        if t is not None and t.data_ptr() != getattr(model, name).data_ptr():
            setattr(model, name, t)


def event(model, flags, N=2, max_grad=0.0, dense_limit=0.0, min_opacity=0.0, max_screen_size=None, world_limit=0.0, grads=None,
          mask=None, noise=None):
    """One clone / split / prune event on `model` and its optimizer -> the totals as a dict (TOTAL_NAMES).  flags: CLONE | SPLIT
    | PRUNE; grads: explicit per-Gaussian gradients (else xyz_gradient_accum / denom); mask: explicit prune mask (else the
    reference's opacity / size mask); noise: [>= N n_split, 3] unit normals for the children (default: torch.randn on the
    device, drawn after the read-back)."""
    P = int(model._xyz.shape[0])
    N = int(N)
    if not 1 <= N <= MAX_N:
        raise ValueError(f"densify_and_split takes 1 <= N <= {MAX_N}, got {N}")
    if P == 0:   # an earlier event pruned everything: nothing to decide, nothing to move
        _lib.require_device(model._xyz)
        return dict(zip(TOTAL_NAMES, [0] * len(TOTAL_NAMES)))
    if max_screen_size and (flags & PRUNE) and mask is None:
        flags |= SCREEN
    groups = _groups(model)
    ins = [None] * N_TENSORS
    for k, (gname, attr) in enumerate(PARAMS):
        p = getattr(model, attr)
        if gname in groups and groups[gname][0]["params"][0] is not p:
            raise RuntimeError(f"the optimizer's '{gname}' group does not hold the model's {attr}")
        ins[k] = _lib.f32c(p.detach())
        st = groups[gname][1] if gname in groups else None
        if st is not None:
            ins[EXP_AVG + k], ins[EXP_AVG_SQ + k] = _lib.f32c(st["exp_avg"]), _lib.f32c(st["exp_avg_sq"])
    rest_width = int(ins[2].numel() // P)
    pplr = groups["xyz"][0].get("per_point_lr") if "xyz" in groups else None
    if pplr is not None:
        if pplr.numel() != P:
            raise RuntimeError(f"per_point_lr holds {pplr.numel()} rows for {P} Gaussians")
        ins[PER_POINT_LR] = _lib.f32c(pplr)
    densify = bool(flags & (CLONE | SPLIT))
    ins[GRAD_ACCUM], ins[DENOM] = _stat(model.xyz_gradient_accum, P, (P, 1)), _stat(model.denom, P, (P, 1))
    ins[MAX_RADII] = _stat(model.max_radii2D, P, (P,))
    n_grads = 0
    if grads is not None:
        grads = _lib.f32c(grads.detach().reshape(-1))
        n_grads = int(grads.numel())
        if n_grads > P:
            raise ValueError(f"{n_grads} gradients for {P} Gaussians")
    elif densify and (ins[GRAD_ACCUM] is None or ins[DENOM] is None):
        raise RuntimeError("densification needs the model's statistics (training_setup creates them)")
    if mask is not None:
        if mask.dtype is torch.bool:
            mask = mask.view(torch.uint8)
        if mask.dtype is not torch.uint8 or mask.numel() != P:
            raise ValueError("prune_points takes a bool mask with one entry per Gaussian")
        mask = mask.reshape(-1).contiguous()
    if (flags & SCREEN) and not densify and ins[MAX_RADII] is None:
        raise RuntimeError("pruning by screen size needs the model's max_radii2D")
    dev = _lib.require_device(*ins, grads, mask, noise)
    is_cuda = dev.type == "cuda"
    scratch = _lib.scratch(dev, "density_scratch_bytes", P, N, what=f"density control: P = {P} with N = {N} is beyond the kernels' limits")
    code = torch.empty(P, dtype=torch.int32, device=dev)
    word = torch.full((16,), -1, dtype=torch.int32, pin_memory=is_cuda)
    child_div = 0.8 * N
    _lib.call(dev, "density_plan", _lib.STREAM, P, N, flags, ins[GRAD_ACCUM], ins[DENOM], grads, n_grads, mask, ins[MAX_RADII], ins[4], ins[3],
              float(max_grad), float(dense_limit), float(min_opacity), float(max_screen_size or 0.0), float(world_limit), child_div, code,
              scratch, word)
    if is_cuda:
        torch.cuda.current_stream(dev).synchronize()   # the one read-back of the event: 16 words the scan kernel stored
    totals = [int(v) for v in word.tolist()]
    new_P, n_sel = totals[5], totals[4]
    if not (0 <= new_P <= P * (N + 1) and 0 <= n_sel <= P):
        raise RuntimeError(f"density_plan: the totals hold new P = {new_P}, split = {n_sel} for P = {P}")
    if n_sel > 0:
        if noise is None:
            noise = torch.randn(N * n_sel, 3, dtype=torch.float32, device=dev)
        else:
            noise = _lib.f32c(noise)
            if noise.dim() != 2 or noise.shape[1] != 3 or noise.shape[0] < N * n_sel:
                raise ValueError(f"noise must be [>= {N * n_sel}, 3] for {n_sel} split Gaussians, got {list(noise.shape)}")
    else:
        noise = None
    outs = [None if t is None else torch.empty((new_P,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev) for t in ins]
    if new_P > 0:
        PTR = ctypes.c_void_p * N_TENSORS
        _lib.call(dev, "density_apply", _lib.STREAM, P, N, flags, rest_width, code, scratch, noise, 0 if noise is None else int(noise.shape[0]),
                  n_sel, child_div, PTR(*[_lib.ptr(t) for t in ins]), PTR(*[_lib.ptr(t) for t in outs]), new_P)
    # ---- the optimizer surgery (reference :328-398): each group's parameter is replaced and its state moves under the new one
    opt = model.optimizer
    with torch.no_grad():
        for k, (gname, attr) in enumerate(PARAMS):
            new_p = nn.Parameter(outs[k].requires_grad_(True))
            if gname in groups:
                group, st = groups[gname]
                old = group["params"][0]
                if st is not None:
                    st["exp_avg"], st["exp_avg_sq"] = outs[EXP_AVG + k], outs[EXP_AVG_SQ + k]
                    del opt.state[old]
                    opt.state[new_p] = st
                elif old in opt.state:
                    del opt.state[old]
                group["params"][0] = new_p
            setattr(model, attr, new_p)
        if pplr is not None:
            groups["xyz"][0]["per_point_lr"] = outs[PER_POINT_LR]
            if getattr(model, "per_point_lr", None) is not None:   # (after a restore() it can be another tensor than the group's)
                model.per_point_lr = outs[PER_POINT_LR]
        for t, attr, shape in ((GRAD_ACCUM, "xyz_gradient_accum", (new_P, 1)), (DENOM, "denom", (new_P, 1)), (MAX_RADII, "max_radii2D", (new_P,))):
            if outs[t] is not None:
                setattr(model, attr, outs[t])
            elif densify:   # densification_postfix creates them whatever was there
                setattr(model, attr, torch.zeros(shape, dtype=torch.float32, device=dev))
    if opt is not None:
        _forget_optimizer_caches(opt)
    return dict(zip(TOTAL_NAMES, totals))


def reset_opacity(model):
    """`reset_opacity` (:280-283 + replace_tensor_to_optimizer): the opacities capped at 0.01 under a NEW Parameter, both of its
    Adam moments zeroed, in one launch on a copy."""
    P = int(model._opacity.shape[0])
    groups = _groups(model)
    new = _lib.f32c(model._opacity.detach()).clone()
    st = groups["opacity"][1] if "opacity" in groups else None
    m = v = None
    if st is not None:
        m, v = torch.empty_like(new), torch.empty_like(new)
    dev = _lib.require_device(new, m, v)
    if P > 0:
        _lib.call(dev, "reset_opacity", _lib.STREAM, P, new, m, v)
    new_p = nn.Parameter(new.requires_grad_(True))
    if "opacity" in groups:
        group = groups["opacity"][0]
        old = group["params"][0]
        opt = model.optimizer
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = m, v
            del opt.state[old]
            opt.state[new_p] = st
        elif old in opt.state:
            del opt.state[old]
        group["params"][0] = new_p
        _forget_optimizer_caches(opt)
    model._opacity = new_p
