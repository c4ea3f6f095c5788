"""ORACLE — TEST INFRASTRUCTURE.  Pure-PyTorch restatement of the update rule of the reference's
PerPointAdam (reference scene/per_point_adam.py:34-100), pinned by the trajectory in
tests/golden/reference_vectors.npz that was produced by the reference class itself.

  mask  = ||grad|| > 0                      (ONE boolean for the whole tensor)
  if mask: m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
  denom = sqrt(v) + eps
  step  = lr * sqrt(1-b2^t) / (1-b1^t)
  p    -= step * per_point_lr * m / denom   (per_point_lr broadcast over the row; constant)
"""
import torch


@torch.no_grad()
def update_(p, g, m, v, step, lr, betas, eps, per_point_lr=None, weight_decay=0.0, gate=None):
    """One PerPointAdam update of one tensor, in place, in the dtype of p / m / v (g and per_point_lr are converted).
    step: the 1-based step count.  gate: the whole-tensor moment gate; None computes the reference's own,
    bool(||g|| > 0), in the dtype at hand.  A float64 run that stands for a float32 device passes the gate that
    device computes (a float64 norm is > 0 where float32 squares underflow).  betas, eps and lr stay Python floats
    (doubles), as in the reference.  -> the gate used."""
    b1, b2 = betas
    g = g.to(p.dtype)
    if weight_decay != 0:
        g = g + weight_decay * p
    if gate is None:
        gate = bool(g.norm() > 0)
    if gate:
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
    denom = v.sqrt().add_(eps)
    s = lr * ((1 - b2 ** step) ** 0.5 / (1 - b1 ** step))
    upd = m / denom
    p.add_(-(s * per_point_lr.to(p.dtype)) * upd if per_point_lr is not None else -s * upd)
    return gate


class PerPointAdamRef(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, per_point_lr=None))

    @torch.no_grad()
    def step(self, gates=None):
        """gates: optional {parameter: bool} overriding the reference's gate for those tensors (see update_)"""
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"], st["m"], st["v"] = 0, torch.zeros_like(p), torch.zeros_like(p)
                st["step"] += 1
                update_(p, p.grad, st["m"], st["v"], st["step"], group["lr"], group["betas"], group["eps"], group.get("per_point_lr"),
                        group["weight_decay"], None if gates is None else gates.get(p))
