"""Checks of the evaluation stage (instantsplat_amd/metrics.py, csrc/ssim.hip k_metrics_rgb8, pose_tracking.render_test_set), shared
by the emulated (CPU) and the GPU test files.

Yardsticks: for the sum of squared differences plain integer numpy; for SSIM a float64 evaluation of the formula of
include/mi355gs.h (11x11 Gaussian window of sigma 1.5 with the float32 coefficients the reference's create_window produces, zero
"same" padding, C1 = 0.01^2, C2 = 0.03^2, mean over 3 H W) on the float32 inputs byte / 255 as torch's div rounds them; for the
reference's own numbers tests/golden/metrics_vectors.npz (make_golden_metrics.py, README_metrics.md)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import ops_util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SSIM_BOUND = 1e-6        # the project's SSIM bound against float64; the reference's own fp32 ssim is within 5.5e-7 on these shapes
PSNR_BOUND_DB = 2e-5     # against the reference's float32 chain, below 128 dB: one ulp between 64 and 128 is 7.6e-6; the log10 result
                         # (~4.7) carries one ulp x 20 = 9.5e-6, the final multiply half an ulp = 3.8e-6, the argument's few-ulp relative
                         # error ~2e-6 through 8.7 dB per unit relative error
SHAPES = [(1, 1), (5, 7), (11, 11), (16, 32), (17, 33), (23, 37), (64, 48)]   # H, W
COUNTS = (1, 2, 5)
KINDS = ("random", "noise3", "identical", "one_byte", "black_white")


def golden():
    return np.load(os.path.join(GOLDEN, "metrics_vectors.npz"))


# ---------------------------------------------------------------------------------------------------- yardsticks
def _window():
    g = torch.tensor([math.exp(-((x - 5) ** 2) / (2.0 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return (g / g.sum()).double().numpy()


def _band(n):
    """[n,n] matrix of the zero-padded 11-tap window: (band @ v)[i] = sum_k w[k] v[i + k - 5]"""
    w, m = _window(), np.zeros((n, n))
    for i in range(n):
        for k in range(11):
            j = i + k - 5
            if 0 <= j < n:
                m[i, j] = w[k]
    return m


def ssim_f64(render: np.ndarray, gt: np.ndarray) -> float:
    """one pair of uint8 [H,W,3] frames"""
    x = torch.from_numpy(render).float().div(255).double().numpy()   # the float32 quotient, then exact
    y = torch.from_numpy(gt).float().div(255).double().numpy()
    H, W = x.shape[:2]
    gh, gwt = _band(H), _band(W).T
    conv = lambda t: np.stack([gh @ t[:, :, c] @ gwt for c in range(3)], axis=2)
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return float(m.mean())


def sq_sum_int(renders: np.ndarray, gts: np.ndarray) -> np.ndarray:
    d = renders.astype(np.int64) - gts.astype(np.int64)
    return (d * d).reshape(d.shape[0], -1).sum(1)


# ---------------------------------------------------------------------------------------------------- inputs
def frame_pairs(kind, N, H, W, seed=0):
    """(renders, gts) uint8 [N,H,W,3]; every frame's content differs from every other's wherever the kind allows it"""
    rng = np.random.default_rng(1000 * seed + 17 * H + W + 7 * N)
    gts = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    if kind == "random":
        renders = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    elif kind == "noise3":
        renders = np.clip(gts.astype(np.int32) + rng.integers(-3, 4, gts.shape), 0, 255).astype(np.uint8)
    elif kind == "identical":
        renders = gts.copy()
    elif kind == "one_byte":
        renders = gts.copy()
        flat = renders.reshape(N, -1)
        for i in range(N):
            flat[i, int(rng.integers(0, flat.shape[1]))] ^= 0x80
    elif kind == "black_white":
        renders, gts = np.zeros_like(gts), np.full_like(gts, 255)
    else:
        raise KeyError(kind)
    return renders, gts


def score(dev, renders: np.ndarray, gts: np.ndarray):
    from instantsplat_amd.metrics import image_metrics_rgb8
    return image_metrics_rgb8(torch.from_numpy(renders).to(dev), torch.from_numpy(gts).to(dev))


# ---------------------------------------------------------------------------------------------------- kernel checks
def check_against_yardsticks(dev, renders, gts, label, ssim_frames=None):
    """every output of image_metrics_rgb8 for one set; the float64 SSIM of the frames in ssim_frames (default: all)"""
    N, H, W = renders.shape[:3]
    m = score(dev, renders, gts)
    assert m["sq_sum"].dtype == np.int64 and m["mse"].dtype == np.float64 and m["psnr"].dtype == np.float64 and m["ssim"].dtype == np.float32
    assert all(m[k].shape == (N,) for k in ("sq_sum", "mse", "psnr", "ssim"))
    want = sq_sum_int(renders, gts)
    assert np.array_equal(m["sq_sum"], want), (label, m["sq_sum"], want)
    assert np.array_equal(m["mse"], want.astype(np.float64) / (65025.0 * 3.0 * H * W))
    for i in range(N):
        if want[i] == 0:
            assert m["psnr"][i] == np.inf and m["ssim"][i] == np.float32(1.0), (label, i, m["ssim"][i])
        else:
            assert m["psnr"][i] == 20.0 * np.log10(1.0 / np.sqrt(m["mse"][i]))
    for i in (range(N) if ssim_frames is None else ssim_frames):
        ops_util.bound(f"metrics ssim vs float64 [{label}]", abs(float(m["ssim"][i]) - ssim_f64(renders[i], gts[i])), SSIM_BOUND)
    return m


def check_shape(dev, H, W):
    for N in COUNTS:
        for kind in KINDS:
            renders, gts = frame_pairs(kind, N, H, W)
            check_against_yardsticks(dev, renders, gts, f"{kind} {N}x{H}x{W}")


def check_all_black_pair_is_one(dev):
    for H, W in ((5, 7), (16, 32), (23, 37)):
        z = np.zeros((2, H, W, 3), np.uint8)
        m = score(dev, z, z)
        assert np.array_equal(m["ssim"], np.ones(2, np.float32)) and np.array_equal(m["sq_sum"], np.zeros(2, np.int64))
        assert np.all(m["psnr"] == np.inf)


def check_all_byte_values(dev):
    """A 16 x 16 pair whose red channels enumerate the 256 byte values (ascending in one frame, a permutation in the other): the
    kernel's byte -> float conversion must be torch.arange(256).float().div(255) bit for bit, which the yardstick's inputs are."""
    table = torch.arange(256).float().div(255)
    assert torch.equal(table, torch.from_numpy(np.arange(256, dtype=np.uint8)).float().div(255))
    assert int((table != torch.arange(256).float() * (1.0 / 255.0)).sum()) == 126   # the multiply is NOT that conversion
    rng = np.random.default_rng(5)
    renders, gts = rng.integers(0, 256, (2, 16, 16, 3), dtype=np.uint8), rng.integers(0, 256, (2, 16, 16, 3), dtype=np.uint8)
    renders[0, :, :, 0] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    gts[0, :, :, 0] = rng.permutation(256).astype(np.uint8).reshape(16, 16)
    renders[1, :, :, 0] = gts[0, :, :, 0]
    gts[1, :, :, 0] = np.arange(256, dtype=np.uint8).reshape(16, 16)[::-1]
    check_against_yardsticks(dev, renders, gts, "all byte values 16x16")


def check_misaligned_bases(dev):
    """frames[1:] of a 23 x 37 stack of 3 starts at an odd byte; a 16 x 32 set (W a multiple of 4: the word loads when aligned) one
    byte into a buffer must take the byte loads.  Both must score exactly as a fresh, aligned copy of the same data."""
    from instantsplat_amd.metrics import image_metrics_rgb8
    renders, gts = frame_pairs("noise3", 3, 23, 37, seed=3)
    r, g = torch.from_numpy(renders).to(dev), torch.from_numpy(gts).to(dev)
    assert r[1:].data_ptr() % 2 == 1 and r[1:].is_contiguous() and r[1:].storage_offset() == 23 * 37 * 3
    a, b = image_metrics_rgb8(r[1:], g[1:]), image_metrics_rgb8(r[1:].clone(), g[1:].clone())
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["sq_sum"], sq_sum_int(renders[1:], gts[1:]))
    renders, gts = frame_pairs("random", 2, 16, 32, seed=4)
    n = renders.size
    for off_r, off_g in ((1, 0), (0, 3), (2, 2)):
        br, bg = torch.zeros(n + 8, dtype=torch.uint8), torch.zeros(n + 8, dtype=torch.uint8)
        br[off_r:off_r + n] = torch.from_numpy(renders).reshape(-1)
        bg[off_g:off_g + n] = torch.from_numpy(gts).reshape(-1)
        br, bg = br.to(dev), bg.to(dev)
        vr, vg = br[off_r:off_r + n].view(2, 16, 32, 3), bg[off_g:off_g + n].view(2, 16, 32, 3)
        assert (vr.data_ptr() | vg.data_ptr()) % 4 != 0
        a, b = image_metrics_rgb8(vr, vg), image_metrics_rgb8(vr.clone(), vg.clone())
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, off_r, off_g)
        assert np.array_equal(a["sq_sum"], sq_sum_int(renders, gts))


def check_empty_set_and_value_errors(dev):
    from instantsplat_amd.metrics import image_metrics_rgb8
    e = torch.zeros(0, 4, 5, 3, dtype=torch.uint8, device=dev)
    m = image_metrics_rgb8(e, e)
    assert [m[k].shape for k in ("sq_sum", "mse", "psnr", "ssim")] == [(0,)] * 4
    assert m["sq_sum"].dtype == np.int64 and m["ssim"].dtype == np.float32
    ok = torch.zeros(2, 4, 5, 3, dtype=torch.uint8, device=dev)
    for a, b in ((ok.float(), ok.float()), (ok, ok.float()), (ok[0], ok[0]), (ok, ok[:1]), (ok, torch.zeros(2, 5, 4, 3, dtype=torch.uint8, device=dev)),
                 (torch.zeros(2, 4, 5, 4, dtype=torch.uint8, device=dev),) * 2, (ok.cpu().numpy(), ok.cpu().numpy())):
        with pytest.raises(ValueError):
            image_metrics_rgb8(a, b)


def check_entry_point_rejects_bad_arguments():
    """Argument checks of mi355gs_metrics_rgb8, before any HIP call (bogus device pointers are never touched)."""
    from instantsplat_amd import _lib
    L = _lib.lib()
    EINVAL = -1
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below must fail its checks first
    run = lambda N=2, H=8, W=8, a=fake, b=fake, scratch=fake, sq=fake, ss=fake: L.mi355gs_metrics_rgb8(None, N, H, W, a, b, scratch, sq, ss)
    for kw in ("a", "b", "scratch", "sq", "ss"):
        assert run(**{kw: None}) == EINVAL, kw
    bad = (dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(H=-3), dict(W=-3), dict(N=65536), dict(H=30000, W=30000),
           dict(H=65535 * 16 + 1, W=1), dict(N=65535, H=4096, W=4128))
    for kw in bad:
        assert run(**kw) == EINVAL, kw
        assert L.mi355gs_metrics_rgb8_scratch_bytes(kw.get("N", 2), kw.get("H", 8), kw.get("W", 8)) == 0, kw
    assert L.mi355gs_metrics_rgb8_scratch_bytes(5, 1080, 1920) >= 5 * 68 * 60 * 8
    assert L.mi355gs_metrics_rgb8_scratch_bytes(1, 1, 1) > 0


# ---------------------------------------------------------------------------------------------------- the reference's numbers
def check_golden_images(dev):
    from instantsplat_amd.metrics import _f32_list, _f32_mean
    g = golden()
    for tag in ("s23x37", "s64x48"):
        m = score(dev, g[f"metrics_{tag}_renders"], g[f"metrics_{tag}_gts"])
        ref_s, ref_p = g[f"metrics_{tag}_ssim"], g[f"metrics_{tag}_psnr"]
        for i, name in enumerate(g[f"metrics_{tag}_names"]):
            ops_util.bound(f"metrics ssim vs reference [{tag} {name}]", abs(float(m["ssim"][i]) - float(ref_s[i])), SSIM_BOUND)
            if np.isinf(ref_p[i]):
                assert m["psnr"][i] == np.inf
            else:
                assert ref_p[i] < 128
                print(f"psnr {tag} {name}: {m['psnr'][i]:.9f} reference {float(ref_p[i]):.9f}")
                ops_util.bound(f"metrics psnr vs reference, dB [{tag} {name}]", abs(m["psnr"][i] - float(ref_p[i])), PSNR_BOUND_DB)
        ssims, psnrs = _f32_list(m["ssim"].tolist()), _f32_list(m["psnr"].tolist())
        ops_util.bound(f"metrics mean ssim vs reference [{tag}]", abs(_f32_mean(ssims) - float(g[f"metrics_{tag}_ssim_mean"])), SSIM_BOUND)
        ref_mean = float(g[f"metrics_{tag}_psnr_mean"])
        if np.isinf(ref_mean):
            assert _f32_mean(psnrs) == np.inf
        else:
            ops_util.bound(f"metrics mean psnr vs reference, dB [{tag}]", abs(_f32_mean(psnrs) - ref_mean), PSNR_BOUND_DB)


POSE_REL_BOUND = 1e-6


def check_golden_poses():
    from instantsplat_amd.metrics import pose_metrics
    g = golden()
    for tag in ("n3", "n12"):
        est, gt = g[f"posemetric_{tag}_est"], g[f"posemetric_{tag}_gt"]
        keep_est, keep_gt = est.copy(), gt.copy()
        pm = pose_metrics(est, gt)
        assert np.array_equal(est, keep_est) and np.array_equal(gt, keep_gt)   # the caller's arrays are not written
        assert sorted(pm) == ["ATE", "RPE_r", "RPE_t"]
        for key, ref in (("RPE_t", "rpe_t"), ("RPE_r", "rpe_r"), ("ATE", "ate")):
            want = float(g[f"posemetric_{tag}_{ref}"])
            print(f"pose {tag} {key}: {pm[key]!r} reference {want!r}")
            ops_util.bound(f"pose_metrics {key} vs reference, relative [{tag}]", abs(pm[key] - want) / abs(want), POSE_REL_BOUND)
    with pytest.raises(ValueError):
        pose_metrics(g["posemetric_n3_est"], g["posemetric_n12_gt"])
    with pytest.raises(ValueError):
        pose_metrics(g["posemetric_n3_est"][:1], g["posemetric_n3_gt"][:1])


# ---------------------------------------------------------------------------------------------------- files
def _save(path, arr, mode="RGB"):
    from PIL import Image
    im = Image.fromarray(arr)   # [H,W,3] -> RGB, [H,W,4] -> RGBA, [H,W] -> L
    assert im.mode == mode
    im.save(path)


def build_model_dir(root):
    """<root>/test/ours_7: the s64x48 pairs (one render stored as RGBA); <root>/test/ours_9: the pairs of both sets, two image
    sizes in one directory; <root>/pose/<method>/pose_optimized.npy: the n3 estimate.  -> {method: [(file name, set, index)]}"""
    g = golden()
    rng = np.random.default_rng(8)
    layout = {"ours_7": [("s64x48", "b_")], "ours_9": [("s23x37", "a_"), ("s64x48", "b_")]}
    listing = {}
    for method, sets in layout.items():
        rd, gd = os.path.join(root, "test", method, "renders"), os.path.join(root, "test", method, "gt")
        os.makedirs(rd), os.makedirs(gd)
        os.makedirs(os.path.join(root, "pose", method))
        np.save(os.path.join(root, "pose", method, "pose_optimized.npy"), g["posemetric_n3_est"])
        listing[method] = []
        for tag, prefix in sets:
            for i, kind in enumerate(g[f"metrics_{tag}_names"]):
                name = f"{prefix}{kind}.png"
                render, gt = g[f"metrics_{tag}_renders"][i], g[f"metrics_{tag}_gts"][i]
                if kind == "noise3":   # RGBA: the alpha channel is dropped, whatever it holds
                    alpha = rng.integers(0, 256, render.shape[:2] + (1,), dtype=np.uint8)
                    _save(os.path.join(rd, name), np.concatenate([render, alpha], axis=2), "RGBA")
                else:
                    _save(os.path.join(rd, name), render)
                _save(os.path.join(gd, name), gt)
                listing[method].append((name, tag, i))
        listing[method].sort()
    return listing


def check_evaluate_files(dev, root):
    from instantsplat_amd.metrics import evaluate
    g = golden()
    listing = build_model_dir(root)
    lpips_stub = lambda r, t: float((r - t).abs().mean()) if tuple(r.shape) == tuple(t.shape) and r.shape[:2] == (1, 3) and r.dtype == torch.float32 else None
    for with_lpips, with_poses in ((False, False), (True, True)):
        out = evaluate(root, gt_poses=g["posemetric_n3_gt"] if with_poses else None, lpips_fn=lpips_stub if with_lpips else None)
        results, per_view = json.load(open(os.path.join(root, "results.json"))), json.load(open(os.path.join(root, "per_view.json")))
        strip = lambda d: json.loads(json.dumps(d))   # (inf survives as Infinity)
        assert results == strip(out["results"]) and per_view == strip(out["per_view"])
        assert sorted(results) == sorted(per_view) == ["ours_7", "ours_9"]
        image_keys = ["LPIPS", "PSNR", "SSIM"] if with_lpips else ["PSNR", "SSIM"]
        pose_keys = ["ATE", "RPE_r", "RPE_t"] if with_poses else []
        for method, files in listing.items():
            assert sorted(results[method]) == sorted(image_keys + pose_keys)
            assert sorted(per_view[method]) == image_keys
            names = [f[0] for f in files]
            for k in image_keys:
                assert list(per_view[method][k]) == names   # sorted name order
            lines = open(os.path.join(root, "test", method, "metrics.txt")).read().splitlines()
            assert len(lines) == len(files)
            for idx, (name, tag, i) in enumerate(files):
                p, s = float(g[f"metrics_{tag}_psnr"][i]), float(g[f"metrics_{tag}_ssim"][i])
                want = f"image name{name}, image idx: {idx}, PSNR: {p:.2f}, SSIM: {s:.4f}"   # reference metrics.py:70 on the golden values
                if with_lpips:
                    assert lines[idx] == want + f", LPIPS: {per_view[method]['LPIPS'][name]:.4f}", lines[idx]
                else:
                    assert lines[idx] == want, (lines[idx], want)
                assert abs(per_view[method]["SSIM"][name] - s) <= SSIM_BOUND
                assert per_view[method]["PSNR"][name] == p == np.inf or abs(per_view[method]["PSNR"][name] - p) <= PSNR_BOUND_DB
            pose_file = os.path.join(root, "pose", method, "pose_eval.txt")
            if with_poses:
                for key, ref in (("RPE_t", "rpe_t"), ("RPE_r", "rpe_r"), ("ATE", "ate")):
                    want = float(g[f"posemetric_n3_{ref}"])
                    assert abs(results[method][key] - want) <= POSE_REL_BOUND * abs(want)
                assert open(pose_file).read() == "RPE_t: {:.04f}, RPE_r: {:.04f}, ATE: {:.04f}".format(
                    float(g["posemetric_n3_rpe_t"]), float(g["posemetric_n3_rpe_r"]), float(g["posemetric_n3_ate"]))
            else:
                assert not os.path.exists(pose_file)
        # ours_7 is the s64x48 set: the reference's means (accumulated in another order: float32, within the per-image bounds)
        assert abs(results["ours_7"]["SSIM"] - float(g["metrics_s64x48_ssim_mean"])) <= SSIM_BOUND
        assert abs(results["ours_7"]["PSNR"] - float(g["metrics_s64x48_psnr_mean"])) <= PSNR_BOUND_DB
        assert results["ours_9"]["PSNR"] == np.inf   # it holds the identical pair


def check_unsupported_mode_raises(dev, root):
    from instantsplat_amd.metrics import evaluate
    g = golden()
    rd, gd = os.path.join(root, "test", "ours_1", "renders"), os.path.join(root, "test", "ours_1", "gt")
    os.makedirs(rd), os.makedirs(gd)
    _save(os.path.join(rd, "x.png"), g["metrics_s23x37_renders"][0][:, :, 0].copy(), "L")
    _save(os.path.join(gd, "x.png"), g["metrics_s23x37_gts"][0])
    with pytest.raises(ValueError, match="mode"):
        evaluate(root)


def check_evaluate_from_frames_equals_files(dev, root):
    """frames = {method: [dict(names, renders, gts)]} gives the dicts the files give (PNG is lossless), without reading them"""
    from instantsplat_amd.metrics import evaluate
    g = golden()
    build_model_dir(root)
    from_files = evaluate(root)
    groups = lambda sets: [dict(names=[f"{p}{k}.png" for k in g[f"metrics_{t}_names"]], renders=torch.from_numpy(g[f"metrics_{t}_renders"]).to(dev),
                                gts=torch.from_numpy(g[f"metrics_{t}_gts"]).to(dev)) for t, p in sets]
    frames = {"ours_7": groups([("s64x48", "b_")]), "ours_9": groups([("s23x37", "a_"), ("s64x48", "b_")])}
    for method in frames:   # nothing left to read
        for sub in ("renders", "gt"):
            for f in os.listdir(os.path.join(root, "test", method, sub)):
                os.remove(os.path.join(root, "test", method, sub, f))
    assert evaluate(root, frames=frames) == from_files
