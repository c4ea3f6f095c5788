"""tests/golden/metrics_vectors.npz: the reference's own evaluation arithmetic (metrics.py:60-111), executed from the reference tree
(`ref_loader.REF`; build container only; needs scipy).  Only arrays and name lists are stored.

Image half, prefix `metrics_` — `ssim` (utils/loss_utils.py:55-85) and `psnr` (utils/image_utils.py:17-19) on 8-bit pairs generated
here from a seed and converted as torchvision's `to_tensor` converts a PIL image (torchvision is not installed: the conversion is
spelled out from memory, permute(2,0,1).contiguous().float().div(255)), then `[:, :3]` of an added batch dimension as readImages
(utils/sfm_utils.py:452-462) does, and the means of metrics.py:79-81 (`torch.tensor(values).mean().item()`):
  metrics_<set>_names                  the pairs' names, in the order of every other array of the set
  metrics_<set>_renders / _gts         uint8 [n,H,W,3]
  metrics_<set>_ssim / _psnr           float32 [n], the reference's per-image values (psnr = inf for the identical pair)
  metrics_<set>_ssim_mean / _psnr_mean float32 scalars
sets: s23x37 (random, noise3, one_byte, identical) and s64x48 (random, noise3, noise3_dark).

Pose half, prefix `posemetric_` — metrics.py:95-111: `align_pose` (utils/sfm_utils.py:464-493, taken as a function definition
because that file imports cv2), `align_ate_c2b_use_a2b` (utils/utils_poses/align_traj.py), `compute_ATE` and `compute_rpe`
(utils/utils_poses/comp_ate.py), imported with a stub `matplotlib`, on seeded trajectories: a ground truth of random rigid
poses and an estimate that is a similarity transform of it plus noise:
  posemetric_<tag>_gt / _est           float64 [n,4,4]
  posemetric_<tag>_rpe_t / _rpe_r / _ate   float64 scalars, scaled as metrics.py:109-111 scales them (x100, degrees, as is)
tags: n3, n12.
Run:  python tests/golden/make_golden_metrics.py"""
import os
import sys
import types
import warnings

import numpy as np
import scipy
import scipy.linalg  # noqa: F401  (align_pose says `scipy.linalg.orthogonal_procrustes`)
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

REF = ref_loader.REF

for k in [k for k in list(sys.modules) if k == "utils" or k.startswith("utils.")]:
    del sys.modules[k]
mpl = types.ModuleType("matplotlib")
mpl.pyplot = types.ModuleType("matplotlib.pyplot")
sys.modules.setdefault("matplotlib", mpl)
sys.modules.setdefault("matplotlib.pyplot", mpl.pyplot)
sys.path.insert(0, REF)
from utils.image_utils import psnr  # noqa: E402  (reference)
from utils.loss_utils import ssim  # noqa: E402  (reference)
from utils.utils_poses.align_traj import align_ate_c2b_use_a2b  # noqa: E402  (reference)
from utils.utils_poses.comp_ate import compute_ATE, compute_rpe  # noqa: E402  (reference)

ns = {"np": np, "scipy": scipy}
sfm = os.path.join(REF, "utils", "sfm_utils.py")
for name, src in ref_loader.function_sources(sfm, {"align_pose"}).items():
    exec(compile(src, sfm, "exec"), ns)
align_pose = ns["align_pose"]

rng = np.random.default_rng(2024)
out = {}


def to_tensor(hwc: np.ndarray) -> torch.Tensor:
    """torchvision.transforms.functional.to_tensor for a uint8 image (recalled, not executed: torchvision is not installed)"""
    return torch.from_numpy(hwc).permute(2, 0, 1).contiguous().float().div(255)


def noisy(gt, amp=3):
    return np.clip(gt.astype(np.int32) + rng.integers(-amp, amp + 1, gt.shape), 0, 255).astype(np.uint8)


def image_set(tag, H, W, kinds):
    names, renders, gts = [], [], []
    for kind in kinds:
        gt = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if kind == "random":
            render = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        elif kind == "noise3":
            render = noisy(gt)
        elif kind == "noise3_dark":
            gt = (gt // 6).astype(np.uint8)
            render = noisy(gt)
        elif kind == "one_byte":
            render = gt.copy()
            render[H // 2, W // 3, 1] ^= 1
        elif kind == "identical":
            render = gt.copy()
        names.append(kind); renders.append(render); gts.append(gt)
    ssims, psnrs = [], []
    for r, g in zip(renders, gts):   # readImages' tensors, then metrics.py:67-68
        rt, gt_ = to_tensor(r).unsqueeze(0)[:, :3, :, :], to_tensor(g).unsqueeze(0)[:, :3, :, :]
        ssims.append(ssim(rt, gt_))
        psnrs.append(psnr(rt, gt_))
    out[f"metrics_{tag}_names"] = np.array(names)
    out[f"metrics_{tag}_renders"], out[f"metrics_{tag}_gts"] = np.stack(renders), np.stack(gts)
    out[f"metrics_{tag}_ssim"] = torch.tensor(ssims).numpy()
    out[f"metrics_{tag}_psnr"] = torch.tensor(psnrs).numpy()
    out[f"metrics_{tag}_ssim_mean"] = np.float32(torch.tensor(ssims).mean().item())
    out[f"metrics_{tag}_psnr_mean"] = np.float32(torch.tensor(psnrs).mean().item())
    assert out[f"metrics_{tag}_ssim"].dtype == np.float32 and out[f"metrics_{tag}_psnr"].shape == (len(kinds),)


image_set("s23x37", 23, 37, ("random", "noise3", "one_byte", "identical"))
image_set("s64x48", 64, 48, ("random", "noise3", "noise3_dark"))


def rand_rot(scale=None):
    if scale is None:
        q = rng.standard_normal(4)
    else:
        q = np.concatenate([[1.0], scale * rng.standard_normal(3)])
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def trajectories(n):
    gt = np.tile(np.eye(4), (n, 1, 1))
    est = gt.copy()
    R0, s0, t0 = rand_rot(), 0.37, rng.standard_normal(3)
    for i in range(n):
        gt[i, :3, :3], gt[i, :3, 3] = rand_rot(), 2.0 * rng.standard_normal(3)
        est[i, :3, :3] = R0 @ gt[i, :3, :3] @ rand_rot(0.01)
        est[i, :3, 3] = s0 * (R0 @ gt[i, :3, 3]) + t0 + 0.02 * rng.standard_normal(3)
    return gt, est


with warnings.catch_warnings():
    warnings.simplefilter("ignore", DeprecationWarning)   # (the reference says np.linalg.linalg.svd)
    for n in (3, 12):
        gt, est = trajectories(n)
        out[f"posemetric_n{n}_gt"], out[f"posemetric_n{n}_est"] = gt.copy(), est.copy()
        # metrics.py:95-111
        pose_optimized = torch.from_numpy(est.copy())
        poses_gt = torch.from_numpy(np.array(gt.copy()))
        trans_gt_align, trans_est_align, _ = align_pose(poses_gt[:, :3, -1].numpy(), pose_optimized[:, :3, -1].numpy())
        poses_gt[:, :3, -1] = torch.from_numpy(trans_gt_align)
        pose_optimized[:, :3, -1] = torch.from_numpy(trans_est_align)
        c2ws_est_aligned = align_ate_c2b_use_a2b(pose_optimized, poses_gt)
        ate = compute_ATE(poses_gt.cpu().numpy(), c2ws_est_aligned.cpu().numpy())
        rpe_trans, rpe_rot = compute_rpe(poses_gt.cpu().numpy(), c2ws_est_aligned.cpu().numpy())
        out[f"posemetric_n{n}_rpe_t"] = np.float64(rpe_trans * 100)
        out[f"posemetric_n{n}_rpe_r"] = np.float64(rpe_rot * 180 / np.pi)
        out[f"posemetric_n{n}_ate"] = np.float64(ate)

path = os.path.join(HERE, "metrics_vectors.npz")
np.savez_compressed(path, **out)
print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")
for k, v in out.items():
    if v.size <= 8 and v.dtype.kind == "f":
        print(k, v)
