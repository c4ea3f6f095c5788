"""Stand-in for the three things of `roma` (not installed here) that the reference's global alignment loop touches
(dust3r/cloud_opt/base_opt.py `_get_poses`, `_set_pose`), written from roma's documented conventions — quaternions are
scalar-last (x, y, z, w):

  RigidUnitQuat(q, t).normalize()   q / |q|, t unchanged
  .to_homogeneous()                 [..., 4, 4] with the rotation matrix of the unit quaternion, t, and the row (0, 0, 0, 1)
  rotmat_to_unitquat(R)             the unit quaternion of a rotation matrix (largest-component branch of Shepperd's method)

Only the generator of tests/golden/align_vectors.npz loads this; roma's own rounding (the order of its products, its choice of
branch in rotmat_to_unitquat) is therefore NOT pinned by the goldens.  Test infrastructure; never imported by the product."""
import torch


def unitquat_to_rotmat(q):
    x, y, z, w = torch.unbind(q, dim=-1)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = torch.ones_like(x)
    rows = [one - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, one - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, one - (txx + tyy)]
    return torch.stack(rows, dim=-1).reshape(q.shape[:-1] + (3, 3))


def rotmat_to_unitquat(R):
    R = torch.as_tensor(R)
    flat = R.reshape(-1, 3, 3)
    out = []
    for m in flat:
        d = [m[0, 0], m[1, 1], m[2, 2]]
        trace = d[0] + d[1] + d[2]
        choice = max(range(4), key=lambda k: float(d[k]) if k < 3 else float(trace))
        if choice == 3:
            q = [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1 + trace]
        else:
            i, j, k = choice, (choice + 1) % 3, (choice + 2) % 3
            q = [None] * 4
            q[i] = 1 - trace + 2 * m[i, i]
            q[j] = m[j, i] + m[i, j]
            q[k] = m[k, i] + m[i, k]
            q[3] = m[k, j] - m[j, k]
        q = torch.stack(q)
        out.append(q / q.norm())
    return torch.stack(out).reshape(R.shape[:-2] + (4,))


class RigidUnitQuat:
    def __init__(self, linear, translation):
        self.linear, self.translation = linear, translation

    def normalize(self):
        return RigidUnitQuat(self.linear / torch.norm(self.linear, dim=-1, keepdim=True), self.translation)

    def to_homogeneous(self):
        R = unitquat_to_rotmat(self.linear)
        batch = R.shape[:-2]
        out = torch.zeros(batch + (4, 4), dtype=R.dtype, device=R.device)
        out[..., :3, :3] = R
        out[..., :3, 3] = self.translation
        out[..., 3, 3] = 1
        return out
