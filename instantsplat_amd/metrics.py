"""The evaluation stage — reference metrics.py:35-122 without the parts that cannot run offline: per-view and mean PSNR and SSIM
of a rendered test set, ATE / RPE of the optimised poses, and the files results.json, per_view.json, metrics.txt, pose_eval.txt.

`image_metrics_rgb8` scores a whole set of 8-bit frame pairs with one library call (csrc/ssim.hip k_metrics_rgb8, include/mi355gs.h
mi355gs_metrics_rgb8) on the interleaved bytes the device already holds after `render_pose_path` / `render_test_set`.
`pose_metrics` is the pose half on the host (numpy).  `evaluate` reads a model directory (or takes the frame stacks
`pose_tracking.render_test_set` returned) and writes the reference's files.

In: PSNR, SSIM, LPIPS (the VGG16 forward on the device, instantsplat_amd/lpips.py: `evaluate(..., lpips=LpipsVGG(...))`), ATE,
RPE_t, RPE_r and the four files.  Out: LPIPS's trained weights — they cannot be had offline, the caller loads the two files
(`LpipsVGG.from_files`) or passes an `lpips_fn` of their own; without either the files lack the LPIPS keys —, reading COLMAP
ground-truth poses and the train/test split (dataset conventions: the caller passes `gt_poses`), the plot.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import _frames, _lib

MAX_FRAMES_PER_CALL = 65535   # include/mi355gs.h: N of one mi355gs_metrics_rgb8 call (a grid dimension)


def _empty():
    return dict(sq_sum=np.zeros(0, np.int64), mse=np.zeros(0, np.float64), psnr=np.zeros(0, np.float64), ssim=np.zeros(0, np.float32))


def image_metrics_rgb8(renders: torch.Tensor, gts: torch.Tensor) -> dict:
    """PSNR and SSIM of N pairs of 8-bit frames, uint8 [N,H,W,3] each, as reference metrics.py:67-68 computes them from the PNG
    files: `ssim` of utils/loss_utils.py:55-85 and `psnr` of utils/image_utils.py:17-19 on `to_tensor` inputs (byte / 255).

    The tensors may live on the device, in pinned memory or on the CPU (the last two take one host-to-device copy each);
    contiguous slices with a storage offset are used in place, whatever their alignment.  One library call (more only for
    N > 65535), two kernel launches per call, and ONE read-back of both result arrays.
    -> dict of host arrays: sq_sum int64 [N] (sum of squared byte differences, exact), mse float64 [N] = sq_sum / (65025 * 3 H W),
       psnr float64 [N] = 20 log10(1 / sqrt(mse)) (inf for identical frames), ssim float32 [N].

    PSNR: the reference forms (x - y)^2 per element, their mean, sqrt, reciprocal, log10 and the product by 20 in float32 — each a
    rounding of up to half an ulp, the result near 4.7 for log10 and between 64 and 128 dB for close pairs, where one ulp is
    7.6e-6 dB; its value therefore carries an error of the order of 1e-5 dB (the largest difference from the value below that
    was seen on the golden pairs: 4.7e-6 dB).  Here the sum is an exact integer and everything after it is float64 on the host, so
    the value is at least as close to the true PSNR as the reference's.
    Raises ValueError for anything but two uint8 [N,H,W,3] tensors of one shape, or sizes beyond the library's limits."""
    N, H, W = _frames.check_pair("image_metrics_rgb8", renders, gts)
    if N == 0:
        return _empty()
    if H <= 0 or W <= 0:
        raise ValueError(f"empty frames: {H} x {W}")
    a, b, dev = _frames.pair_on_device(renders, gts)
    out = torch.empty(12 * N, dtype=torch.uint8, device=dev)   # int64 [N] then float32 [N]: one block, one read-back
    for first in range(0, N, MAX_FRAMES_PER_CALL):
        n = min(MAX_FRAMES_PER_CALL, N - first)
        scratch = _lib.scratch(dev, "metrics_rgb8_scratch_bytes", n, H, W,
                               what=f"mi355gs_metrics_rgb8 does not take {n} frames of {H} x {W} (include/mi355gs.h: the limits)")
        _lib.call(dev, "metrics_rgb8", _lib.STREAM, n, H, W, a[first:first + n], b[first:first + n], scratch, out.data_ptr() + 8 * first,
                  out.data_ptr() + 8 * N + 4 * first)
    host = out.cpu().numpy()   # the one read-back (it also orders the launches before the scratch blocks are released)
    sq = host[:8 * N].view(np.int64).copy()
    ssim = host[8 * N:].view(np.float32).copy()
    mse = sq.astype(np.float64) / (65025.0 * 3.0 * H * W)
    with np.errstate(divide="ignore"):
        psnr = 20.0 * np.log10(1.0 / np.sqrt(mse))
    return dict(sq_sum=sq, mse=mse, psnr=psnr, ssim=ssim)


# ------------------------------------------------------------------------------------------------------------ pose half
def _unit_centred(points: np.ndarray) -> np.ndarray:
    p = np.array(points, dtype=np.float64, copy=True)
    if p.ndim != 2 or p.size == 0:
        raise ValueError("pose alignment needs a non-empty [n,3] array of translations")
    p -= p.mean(0)
    norm = np.linalg.norm(p)
    if norm == 0:
        raise ValueError("pose alignment needs more than one distinct translation")
    return p / norm


def align_translations(t_gt: np.ndarray, t_est: np.ndarray):
    """reference utils/sfm_utils.py:464-493 (`align_pose`): both point sets centred and scaled to unit Frobenius norm, the second
    then multiplied by the orthogonal-Procrustes scale — the sum of the singular values of t_gt^T t_est.  (The rotation of that
    fit is not applied, as in the reference: the similarity alignment that follows finds it.)"""
    a, b = _unit_centred(t_gt), _unit_centred(t_est)
    if a.shape != b.shape:
        raise ValueError(f"{a.shape[0]} ground-truth and {b.shape[0]} estimated translations")
    return a, b * np.linalg.svd(a.T @ b, compute_uv=False).sum()


def _umeyama(target: np.ndarray, source: np.ndarray):
    """s, R, t minimising sum |target - (s R source + t)|^2 (Umeyama 1991), in the arrays' own precision up to the SVD."""
    n = target.shape[0]
    f = target.dtype.type
    mu_t, mu_s = target.mean(0), source.mean(0)
    tc, sc = target - mu_t, source - mu_s
    cov = f(1.0 / n) * (tc.T @ sc)
    var_s = f(1.0 / n) * (sc * sc).sum()
    U, D, Vh = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh.T) < 0:
        S[2, 2] = -1.0
    R = U @ (S @ Vh)                                   # float64 from here on: S is
    s = (f(1.0) / var_s) * np.trace(np.diag(D) @ S)
    return float(s), R, mu_t - s * (R @ mu_s)


def pose_metrics(poses_est, poses_gt) -> dict:
    """reference metrics.py:95-111 for two [n,4,4] pose lists (the optimised train poses and their ground truth):
      1. `align_translations` on the two translation sets, both written back into their poses;
      2. the similarity transform that carries the estimated positions onto the ground truth's (align_ate_c2b_use_a2b,
         utils/utils_poses/align_traj.py:34-77 with ATE/align_utils.py's sim3), fitted and applied in float32 — the reference
         passes both trajectories through `.float()` there, and so does this;
      3. ATE: root mean square of the position differences; RPE: over consecutive pairs, the mean norm of the translation and
         the mean angle of the rotation of inv(gt_rel) @ est_rel (utils/utils_poses/comp_ate.py).
    -> dict(RPE_t = 100 x mean translation error, RPE_r = mean angle in degrees, ATE), as the reference scales them."""
    est = np.array(poses_est, dtype=np.float64, copy=True)
    gt = np.array(poses_gt, dtype=np.float64, copy=True)
    if est.ndim != 3 or est.shape[1:] != (4, 4) or est.shape != gt.shape or est.shape[0] < 2:
        raise ValueError(f"pose_metrics takes two [n,4,4] arrays with n >= 2, got {est.shape} and {gt.shape}")
    gt[:, :3, 3], est[:, :3, 3] = align_translations(gt[:, :3, 3], est[:, :3, 3])
    est32, gt32 = est.astype(np.float32), gt.astype(np.float32)
    s, R, t = _umeyama(gt32[:, :3, 3], est32[:, :3, 3])
    R32, t32 = R.astype(np.float32), t.astype(np.float32)
    aligned = np.tile(np.eye(4, dtype=np.float32), (est.shape[0], 1, 1))
    aligned[:, :3, :3] = R32[None] @ est32[:, :3, :3]
    aligned[:, :3, 3:4] = np.float32(s) * (R32[None] @ est32[:, :3, 3:4]) + t32[None, :, None]
    d = gt[:, :3, 3] - aligned[:, :3, 3]
    ate = float(np.sqrt(np.mean(np.sqrt((d ** 2).sum(1)) ** 2)))
    te, re = [], []
    for i in range(est.shape[0] - 1):
        gt_rel = np.linalg.inv(gt[i]) @ gt[i + 1]
        est_rel = np.linalg.inv(aligned[i]) @ aligned[i + 1]   # float32, as the aligned trajectory is
        err = np.linalg.inv(gt_rel) @ est_rel
        te.append(np.sqrt(err[0, 3] ** 2 + err[1, 3] ** 2 + err[2, 3] ** 2))
        re.append(np.arccos(max(min(0.5 * (err[0, 0] + err[1, 1] + err[2, 2] - 1.0), 1.0), -1.0)))
    return dict(RPE_t=float(np.mean(te)) * 100, RPE_r=float(np.mean(re)) * 180 / np.pi, ATE=ate)


# ------------------------------------------------------------------------------------------------------------ files
def _read_rgb8(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        if im.mode == "RGB":
            return np.asarray(im).copy()
        if im.mode == "RGBA":   # the reference's [:, :3]: the alpha channel is dropped, not composited
            return np.asarray(im)[:, :, :3].copy()
        raise ValueError(f"{path}: image mode {im.mode!r}; the evaluation reads RGB and RGBA files")


def _read_groups(method_dir: str):
    """[dict(names, renders, gts)] of test/<method>/{renders,gt}: the files in sorted name order, grouped by image size"""
    renders_dir, gt_dir = os.path.join(method_dir, "renders"), os.path.join(method_dir, "gt")
    by_size = {}
    for name in sorted(os.listdir(renders_dir)):
        r, g = _read_rgb8(os.path.join(renders_dir, name)), _read_rgb8(os.path.join(gt_dir, name))
        if r.shape != g.shape:
            raise ValueError(f"{name}: render {r.shape} and ground truth {g.shape} differ in size")
        grp = by_size.setdefault(r.shape, dict(names=[], renders=[], gts=[]))
        grp["names"].append(name); grp["renders"].append(r); grp["gts"].append(g)
    return [dict(names=g["names"], renders=torch.from_numpy(np.stack(g["renders"])), gts=torch.from_numpy(np.stack(g["gts"])))
            for g in by_size.values()]


def _f32_mean(values) -> float:
    return torch.tensor(values, dtype=torch.float32).mean().item()   # the reference's torch.tensor(values).mean()


def _f32_list(values) -> list:
    return torch.tensor(values, dtype=torch.float32).tolist()


def evaluate(model_path, gt_poses=None, lpips_fn=None, frames=None, lpips=None) -> dict:
    """reference metrics.py:35-122 for one model directory.  For every test/<method> directory (in sorted order):
      * renders/ and gt/ are read with PIL in SORTED name order (the reference takes os.listdir's order; only the order of the
        lines, of the per-view entries and of the float32 accumulation of the means depends on it), RGB as is, RGBA without its
        alpha channel, any other mode a ValueError; the images are grouped by size and scored by `image_metrics_rgb8`.
        frames = {method: [dict(names, renders, gts)]} (what `pose_tracking.render_test_set` returns under "frames"): those
        stacks are scored instead, and no image file is read;
      * test/<method>/metrics.txt: one line per image, `image name{n}, image idx: {i}, PSNR: {p:.2f}, SSIM: {s:.4f}`, with
        `, LPIPS: {l:.4f}` only if lpips or lpips_fn is given;
      * results.json {method: {SSIM, PSNR[, LPIPS][, RPE_t, RPE_r, ATE]}} and per_view.json {method: {SSIM: {name: value},
        PSNR: {...}[, LPIPS: {...}]}}: the means are float32 means of the float32 per-view values, as the reference takes them.
        lpips (an `instantsplat_amd.lpips.LpipsVGG`) supplies LPIPS with one `lpips_rgb8` call per group of frames;
        lpips_fn(render [1,3,H,W] float32, gt [1,3,H,W] float32) -> float supplies it view by view instead (both: ValueError);
        with neither (the VGG weights cannot be had offline) the files simply lack the "LPIPS" keys;
      * with gt_poses ([n,4,4], the train views' ground truth) the pose half: pose/<method>/pose_optimized.npy against them
        through `pose_metrics`, RPE_t / RPE_r / ATE added to results.json and pose/<method>/pose_eval.txt written.
    Errors propagate (the reference's bare `except` is not reproduced).  -> dict(results=..., per_view=...), the two files' content."""
    if lpips is not None and lpips_fn is not None:
        raise ValueError("evaluate takes lpips (an LpipsVGG) or lpips_fn, not both")
    model_path = str(model_path)
    test_dir = os.path.join(model_path, "test")
    methods = sorted(frames) if frames is not None else sorted(os.listdir(test_dir))
    full, per_view = {}, {}
    for method in methods:
        method_dir = os.path.join(test_dir, method)
        groups = frames[method] if frames is not None else _read_groups(method_dir)
        scored = {}
        for grp in groups:
            if len(grp["names"]) != int(grp["renders"].shape[0]):
                raise ValueError(f"{len(grp['names'])} names for {int(grp['renders'].shape[0])} frames")
            m = image_metrics_rgb8(grp["renders"], grp["gts"])
            lp = lpips.lpips_rgb8(grp["renders"], grp["gts"])["lpips"] if lpips is not None else None
            for k, name in enumerate(grp["names"]):
                if name in scored:
                    raise ValueError(f"image name {name!r} appears twice")
                scored[name] = (float(m["psnr"][k]), float(m["ssim"][k]), grp, k, None if lp is None else float(lp[k]))
        names = sorted(scored)
        psnrs, ssims = _f32_list([scored[n][0] for n in names]), _f32_list([scored[n][1] for n in names])
        lpipss = _f32_list([scored[n][4] for n in names]) if lpips is not None else None
        if lpips_fn is not None:
            to_f32 = lambda t: t.permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0)
            lpipss = _f32_list([float(lpips_fn(to_f32(scored[n][2]["renders"][scored[n][3]]), to_f32(scored[n][2]["gts"][scored[n][3]])))
                                for n in names])
        os.makedirs(method_dir, exist_ok=True)
        with open(os.path.join(method_dir, "metrics.txt"), "w") as f:
            for idx, name in enumerate(names):
                line = f"image name{name}, image idx: {idx}, PSNR: {psnrs[idx]:.2f}, SSIM: {ssims[idx]:.4f}"
                if lpipss is not None:
                    line += f", LPIPS: {lpipss[idx]:.4f}"
                f.write(line + "\n")
        full[method] = {"SSIM": _f32_mean(ssims), "PSNR": _f32_mean(psnrs)}
        per_view[method] = {"SSIM": dict(zip(names, ssims)), "PSNR": dict(zip(names, psnrs))}
        if lpipss is not None:
            full[method]["LPIPS"] = _f32_mean(lpipss)
            per_view[method]["LPIPS"] = dict(zip(names, lpipss))
        if gt_poses is not None:
            pose_dir = os.path.join(model_path, "pose", method)
            pm = pose_metrics(np.load(os.path.join(pose_dir, "pose_optimized.npy")), gt_poses)
            full[method].update(pm)
            with open(os.path.join(pose_dir, "pose_eval.txt"), "w") as f:
                f.write("RPE_t: {:.04f}, RPE_r: {:.04f}, ATE: {:.04f}".format(pm["RPE_t"], pm["RPE_r"], pm["ATE"]))
    with open(os.path.join(model_path, "results.json"), "w") as fp:
        json.dump(full, fp, indent=True)
    with open(os.path.join(model_path, "per_view.json"), "w") as fp:
        json.dump(per_view, fp, indent=True)
    return dict(results=full, per_view=per_view)
