"""roma_standin.py plus the one further thing of `roma` (not installed here) that the reference's
`init_minimum_spanning_tree` touches (dust3r/cloud_opt/init_im_poses.py:232-235), written from roma's documented conventions:

  rigid_points_registration(x, y, weights=None, compute_scaling=False) -> (R, t) or (R, t, scale)
      y ~ scale * R x + t in the weighted least-squares sense: weighted centroids, M = sum w yh xh^T on the centred points,
      R = the special-orthogonal Procrustes solution of M (SVD; the last singular direction is flipped when det(U) det(V) < 0),
      scale = (sum of the singular values, the last one signed by that determinant) / sum w |xh|^2, t = ymean - scale R xmean.

Only the generator of tests/golden/mst_vectors.npz loads this; roma's own rounding (the order of its products and sums, its SVD) is
therefore NOT pinned by the goldens.  Test infrastructure; never imported by the product."""
import torch
from roma_standin import RigidUnitQuat, rotmat_to_unitquat, unitquat_to_rotmat  # noqa: F401


def special_procrustes(M, return_singular_values=False):
    U, D, Vt = torch.linalg.svd(M)
    sign = torch.sign(torch.det(U) * torch.det(Vt))
    U, D = U.clone(), D.clone()
    U[..., :, -1] = U[..., :, -1] * sign[..., None]
    D[..., -1] = D[..., -1] * sign
    R = U @ Vt
    return (R, D) if return_singular_values else R


def rigid_points_registration(x, y, weights=None, compute_scaling=False):
    if weights is None:
        xmean, ymean = x.mean(dim=-2, keepdim=True), y.mean(dim=-2, keepdim=True)
    else:
        total = weights.sum(dim=-1, keepdim=True)[..., None]
        xmean = (weights[..., None] * x).sum(dim=-2, keepdim=True) / total
        ymean = (weights[..., None] * y).sum(dim=-2, keepdim=True) / total
    xhat, yhat = x - xmean, y - ymean
    M = yhat.transpose(-1, -2) @ xhat if weights is None else (weights[..., None] * yhat).transpose(-1, -2) @ xhat
    if compute_scaling:
        R, DS = special_procrustes(M, return_singular_values=True)
        trace = DS.sum(dim=-1)
        denom = xhat.square().sum(dim=(-1, -2)) if weights is None else (weights[..., None] * xhat.square()).sum(dim=(-1, -2))
        scale = trace / denom
        t = ymean.squeeze(-2) - scale[..., None] * (R @ xmean.transpose(-1, -2)).squeeze(-1)
        return R, t, scale
    R = special_procrustes(M)
    return R, ymean.squeeze(-2) - (R @ xmean.transpose(-1, -2)).squeeze(-1)
