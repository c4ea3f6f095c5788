"""Checks of the init stage (instantsplat_amd/init_stage.py, csrc/init.hip), shared by the emulated tier (test_init_stage_emu.py)
and the MI355X tier (test_init_stage_gpu.py) — test infrastructure.

  synthetic_views      the seeded input generator (the project's own code: tests/golden/make_golden_init_stage.py runs the
                       reference on its output and stores only what the reference computed)
  covis_numpy          a numpy restatement of reference utils/sfm_utils.py:342-432 with the kernel's arithmetic: projection in
                       float64 from the float32 inputs, depths normalised and compared in float32.  It is itself held to the
                       golden masks (check_restatement_equals_golden) before anything is compared with it.
  compact_numpy        numpy's boolean indexing, the definition of the compaction

The masks are compared for EQUALITY: no pixel may differ."""
import ctypes
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "init_stage_vectors.npz")

# tag -> (V, H, W, seed, depth_threshold, order); order None = 0 .. V-1
CASES = {
    "v3_t01": (3, 36, 64, 11, 0.01, None),
    "v3_t05": (3, 36, 64, 11, 0.05, None),
    "v4_perm": (4, 55, 97, 12, 0.01, [2, 0, 3, 1]),      # odd sizes, H W not a multiple of 64, a permuted ranking
    "v12": (12, 72, 128, 13, 0.01, None),                 # 66 pairs, the prefix min / max chain
}
GPU_CASES = {"v3_full": (3, 288, 512, 14, 0.01, None), "v12_full": (12, 288, 512, 15, 0.01, None)}
STAGE_CASE = "v3_t01"            # the smallest: its files are golden too
STAGE_ORG_SIZE = (256, 144)      # the "photographs" are 4 x the pointmaps
TEST_POSE_COUNTS = (2, 3, 12)    # n_test for n_train = 3: sampled, sampled, interpolated

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as f:
            _golden = {k: f[k] for k in f.files}
    return _golden


# ---------------------------------------------------------------------------------------------------- the input generator
def _surface(x, y):
    return 0.4 * np.sin(1.3 * x) * np.cos(0.9 * y)


def synthetic_views(V, H, W, seed):
    """V cameras on an arc (yaw -12 .. +12 degrees, radius 5, a small vertical wobble) looking at the origin, focal
    W / (2 tan 30 deg), each seeing the surface z = 0.4 sin(1.3 x) cos(0.9 y) (intersected per pixel by fixed-point iteration);
    depths multiplied by 1 + 0.01 N(0,1), the points placed at the noisy depths; random confidences with a per-view level, smooth
    colours.  Everything float32.  -> dict(images [V,H,W,3], pointmaps [V,H,W,3], depthmaps, confidences [V,H,W], intrinsics
    [V,3,3], w2c [V,4,4], focals [V])"""
    rng = np.random.default_rng(seed)
    f = W / (2.0 * np.tan(np.radians(30.0)))
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
    u, v = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    rays_cam = np.stack([(u - W / 2.0) / f, (v - H / 2.0) / f, np.ones_like(u)], axis=-1)
    yaws = np.radians(np.linspace(-12.0, 12.0, V)) if V > 1 else np.zeros(1)
    out = {k: [] for k in ("images", "pointmaps", "depthmaps", "confidences", "intrinsics", "w2c")}
    for i, yaw in enumerate(yaws):
        centre = np.array([5.0 * np.sin(yaw), 0.15 * np.sin(2.1 * i + 0.3), -5.0 * np.cos(yaw)])
        fwd = -centre / np.linalg.norm(centre)
        right = np.cross(np.array([0.0, -1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = np.stack([right, down, fwd], axis=1), centre
        rays = rays_cam @ c2w[:3, :3].T
        t = -centre[2] / rays[..., 2]
        for _ in range(30):
            p = centre + t[..., None] * rays
            t = (_surface(p[..., 0], p[..., 1]) - centre[2]) / rays[..., 2]
        depth = (t * (1.0 + 0.01 * rng.standard_normal(t.shape))).astype(np.float32)
        pts = (centre + depth.astype(np.float64)[..., None] * rays).astype(np.float32)
        conf = (1.0 + (1.0 + 0.3 * np.sin(1.7 * i + 4.0)) * np.exp(0.5 * rng.standard_normal(t.shape))).astype(np.float32)
        col = 0.5 + 0.5 * np.stack([np.sin(2.0 * pts[..., 0]), np.cos(1.5 * pts[..., 1]), np.sin(pts[..., 0] + pts[..., 1])], axis=-1)
        col = np.clip(col + 0.05 * rng.standard_normal(col.shape), 0.0, 1.0).astype(np.float32)
        for k, a in (("images", col), ("pointmaps", pts), ("depthmaps", depth), ("confidences", conf),
                     ("intrinsics", K.astype(np.float32)), ("w2c", np.linalg.inv(c2w).astype(np.float32))):
            out[k].append(a)
    out = {k: np.stack(a) for k, a in out.items()}
    out["focals"] = np.full(V, f, dtype=np.float64)
    return out


def case_inputs(tag):
    V, H, W, seed, thr, order = {**CASES, **GPU_CASES}[tag]
    return synthetic_views(V, H, W, seed), thr, (list(range(V)) if order is None else list(order))


# ---------------------------------------------------------------------------------------------------- numpy restatements
def covis_numpy(order, depthmaps, pointmaps, intrinsics, w2c, depth_threshold):
    """bool [V,H,W]; see the module docstring.  Sums in the order the kernel writes them."""
    V, H, W = depthmaps.shape
    pts = pointmaps.reshape(V, H * W, 3).astype(np.float64)
    out = np.zeros((V, H, W), dtype=bool)
    thr = np.float32(depth_threshold)
    with np.errstate(all="ignore"):
        for i in range(1, V):
            c = order[i]
            before = list(order[:i])
            bmin, bmax = np.min(depthmaps[before]), np.max(depthmaps[before])
            cmin, cmax = np.min(depthmaps[c]), np.max(depthmaps[c])
            cur = ((depthmaps[c] - cmin) / (cmax - cmin)).astype(np.float32)
            E, K = w2c[c].astype(np.float64), intrinsics[c].astype(np.float64)
            for s in before:
                x, y, z = pts[s, :, 0], pts[s, :, 1], pts[s, :, 2]
                cam = [((E[r, 0] * x + E[r, 1] * y) + E[r, 2] * z) + E[r, 3] for r in range(3)]
                h = [(K[r, 0] * cam[0] + K[r, 1] * cam[1]) + K[r, 2] * cam[2] for r in range(3)]
                px, py = h[0] / h[2], h[1] / h[2]
                valid = (px >= 0) & (px < W) & (py >= 0) & (py < H)
                xi, yi = px[valid].astype(int), py[valid].astype(int)
                a = ((depthmaps[s].reshape(-1)[valid] - bmin) / (bmax - bmin)).astype(np.float32)
                hit = np.abs(a - cur[yi, xi]) < thr
                out[c, yi[hit], xi[hit]] = True
    return out


def compact_numpy(pointmaps, images, confidences, overlap):
    keep = np.ones(confidences.size, dtype=bool) if overlap is None else ~overlap.reshape(-1).astype(bool)
    rgb8 = (np.clip(images.reshape(-1, 3), np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.uint8)
    return pointmaps.reshape(-1, 3)[keep], rgb8[keep], confidences.reshape(-1, 1)[keep]


# ---------------------------------------------------------------------------------------------------- running the device
def device_masks(dev, order, d, thr):
    from instantsplat_amd.init_stage import co_visibility_masks
    t = lambda a: torch.from_numpy(a).to(dev)
    m = co_visibility_masks(order, t(d["depthmaps"]), t(d["pointmaps"]), t(d["intrinsics"]), t(d["w2c"]), thr)
    assert m.dtype == torch.bool and tuple(m.shape) == d["depthmaps"].shape and m.device.type == dev.type
    return m.cpu().numpy()


def device_compact(dev, pointmaps, images, confidences, overlap):
    from instantsplat_amd.init_stage import compact_pointmaps
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p, c, f, M = compact_pointmaps(t(pointmaps), t(images), t(confidences), t(overlap))
    assert p.dtype == torch.float32 and c.dtype == torch.uint8 and f.dtype == torch.float32
    assert tuple(p.shape) == (M, 3) and tuple(c.shape) == (M, 3) and tuple(f.shape) == (M, 1)
    return p.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy(), M


def assert_masks_equal(got, want, what):
    diff = int((got != want).sum())
    print(f"{what}: {int(want.sum())} of {want.size} marked ({[round(float(m.mean()), 4) for m in want]}), {diff} differ")
    assert diff == 0, f"{what}: {diff} pixels differ"


def unpack_mask(g, tag, shape):
    return np.unpackbits(g[f"covis_{tag}_masks"])[:int(np.prod(shape))].reshape(shape).astype(bool)


# ---------------------------------------------------------------------------------------------------- golden cases
def check_restatement_equals_golden(tag):
    d, thr, order = case_inputs(tag)
    want = unpack_mask(golden(), tag, d["depthmaps"].shape)
    assert 0 < want.sum() < want.size and not want[order[0]].any()
    assert_masks_equal(covis_numpy(order, d["depthmaps"], d["pointmaps"], d["intrinsics"], d["w2c"], thr), want, f"restatement {tag}")


def check_golden_case(dev, tag):
    """masks, M and the first / last compacted rows against what the reference's compute_co_vis_masks and save_points3D gave"""
    g = golden()
    d, thr, order = case_inputs(tag)
    assert order == g[f"covis_{tag}_order"].tolist()
    want = unpack_mask(g, tag, d["depthmaps"].shape)
    got = device_masks(dev, order, d, thr)
    assert_masks_equal(got, want, f"device {tag}")
    p, c, f, M = device_compact(dev, d["pointmaps"], d["images"], d["confidences"], got)
    assert M == int(g[f"covis_{tag}_count"]) == int((~want).sum())
    k = g[f"covis_{tag}_head_points"].shape[0]
    for part, rows in (("head", slice(0, k)), ("tail", slice(M - k, M))):
        assert np.array_equal(p[rows], g[f"covis_{tag}_{part}_points"]), part
        assert np.array_equal(c[rows], g[f"covis_{tag}_{part}_colors"].astype(np.uint8)), part   # storePly's cast of col * 255.
        assert np.array_equal(f[rows], g[f"covis_{tag}_{part}_confidence"]), part


def check_against_restatement(dev, tag):
    """the large cases (GPU tier): masks and compaction equal to the restatement's"""
    d, thr, order = case_inputs(tag)
    want = covis_numpy(order, d["depthmaps"], d["pointmaps"], d["intrinsics"], d["w2c"], thr)
    assert 0 < want.sum() < want.size
    got = device_masks(dev, order, d, thr)
    assert_masks_equal(got, want, f"device {tag}")
    p, c, f, M = device_compact(dev, d["pointmaps"], d["images"], d["confidences"], got)
    wp, wc, wf = compact_numpy(d["pointmaps"], d["images"], d["confidences"], want)
    assert M == wp.shape[0] and np.array_equal(p, wp) and np.array_equal(c, wc) and np.array_equal(f, wf)


# ---------------------------------------------------------------------------------------------------- degenerate view counts, quirks
def check_one_and_two_views(dev):
    d = synthetic_views(1, 9, 13, 3)
    m = device_masks(dev, [0], d, 0.5)
    assert not m.any()
    p, c, f, M = device_compact(dev, d["pointmaps"], d["images"], d["confidences"], m)
    assert M == 9 * 13 and np.array_equal(p, d["pointmaps"].reshape(-1, 3)) and np.array_equal(f, d["confidences"].reshape(-1, 1))
    d = synthetic_views(2, 21, 30, 4)
    for order in ([0, 1], [1, 0]):
        want = covis_numpy(order, d["depthmaps"], d["pointmaps"], d["intrinsics"], d["w2c"], 0.05)
        assert want[order[1]].any() and not want[order[0]].any()
        assert_masks_equal(device_masks(dev, order, d, 0.05), want, f"two views {order}")


def _plain_pair(H=8, W=12, seed=5):
    """two views with identity poses and a pinhole camera of focal 8: a point (x, y, z) of view 0 projects to
    (8 x / z + W / 2, 8 y / z + H / 2) in view 1, in exact arithmetic for the dyadic values used below"""
    rng = np.random.default_rng(seed)
    d = dict(intrinsics=np.tile(np.array([[8, 0, W / 2], [0, 8, H / 2], [0, 0, 1]], dtype=np.float32), (2, 1, 1)),
             w2c=np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)),
             depthmaps=rng.uniform(1.0, 2.0, (2, H, W)).astype(np.float32),
             pointmaps=rng.uniform(-5.0, 5.0, (2, H, W, 3)).astype(np.float32))
    d["pointmaps"][..., 2] = rng.uniform(1.0, 3.0, (2, H, W))
    return d


def check_quirks(dev):
    """every quirk of the reference's arithmetic, each against the restatement (which the golden masks vouch for).  With a
    threshold of 2 every valid point is a hit: the normalised depths lie in [0, 1]."""
    def run(d, what, thr=2.0, order=(0, 1)):
        want = covis_numpy(list(order), d["depthmaps"], d["pointmaps"], d["intrinsics"], d["w2c"], thr)
        assert_masks_equal(device_masks(dev, list(order), d, thr), want, what)
        return want

    H, W = 8, 12
    # points BEHIND the target camera that land inside the frame are valid
    d = _plain_pair(H, W)
    d["pointmaps"][0, :, :, 2] = -np.abs(d["pointmaps"][0, :, :, 2])
    assert run(d, "behind the camera")[1].any(), "no point behind the camera landed in the frame"
    # h2 = 0: x / 0 = +-inf and 0 / 0 = NaN fail the bounds test; the other rows still mark
    d = _plain_pair(H, W)
    d["pointmaps"][0, 0, :, 2] = 0.0
    d["pointmaps"][0, 0, 0, :2] = 0.0
    full = run(_plain_pair(H, W), "plain pair")
    assert 0 < run(d, "h2 = 0")[1].sum() < full[1].sum()
    # x = 0 and y = 0 exactly are inside (pixel 0), x = W and y = H exactly are outside
    d = _plain_pair(H, W)
    d["pointmaps"][0] = 100.0                          # everything else projects far outside the frame
    d["pointmaps"][0, 0, 0] = (-1.5, 0.0, 2.0)         # x = (8 * -1.5 + 6 * 2) / 2 = 0, y = 4
    d["pointmaps"][0, 0, 1] = (1.5, 0.0, 2.0)          # x = 12 = W
    d["pointmaps"][0, 0, 2] = (0.0, -1.0, 2.0)         # x = 6, y = (8 * -1 + 4 * 2) / 2 = 0
    d["pointmaps"][0, 0, 3] = (0.0, 1.0, 2.0)          # y = 8 = H
    want = run(d, "x = 0, x = W, y = 0, y = H")
    assert want[1].sum() == 2 and want[1, 4, 0] and want[1, 0, 6]
    # x = -0.0: every term of both sums is -0.0, and -0.0 >= 0 holds: pixel 0
    d = _plain_pair(H, W)
    d["pointmaps"][0] = 100.0
    d["pointmaps"][0, 0, 0] = (-0.0, 0.25, 2.0)
    d["w2c"][1, 0] = (1.0, -0.0, -0.0, -0.0)
    d["intrinsics"][1, 0] = (8.0, -0.0, -0.0)
    want = run(d, "x = -0.0")
    assert want[1].sum() == 1 and want[1, 5, 0]        # y = (8 * 0.25 + 4 * 2) / 2 = 5
    # a constant depth map: (d - min) / 0 = NaN on either side, never a hit
    for view in (0, 1):
        d = _plain_pair(H, W)
        d["pointmaps"][0, :, :, :2] *= 0.1
        d["depthmaps"][view] = 1.5
        assert not run(d, f"constant depth map of view {view}", thr=1e9).any()
    # the first-ranked view is never marked, whichever it is
    d = synthetic_views(3, 17, 23, 6)
    for order in ([1, 2, 0], [2, 0, 1]):
        want = run(d, f"order {order}", thr=0.05, order=order)
        assert not want[order[0]].any() and want[order[1]].any()


# ---------------------------------------------------------------------------------------------------- compaction
COUNT_BLOCK = 1024   # csrc/init.hip COMPACT_BLOCK: elements per workgroup of the count and scatter kernels
SCAN_TURN = 1024     # ... SCAN_THREADS: block counts per turn of the scan's loop
COMPACT_SIZES = (1, 63, COUNT_BLOCK - 1, COUNT_BLOCK, COUNT_BLOCK + 1, 3 * COUNT_BLOCK + 77)
COMPACT_SIZE_TWO_TURNS = SCAN_TURN * COUNT_BLOCK + 5   # 1025 blocks: the scan's loop takes a second turn


def check_compaction(dev, n, seed=0, keep_fraction=0.6):
    """order, values and M against numpy's boolean indexing; keep_fraction 1: all kept (also with no mask at all), ~0: nearly none"""
    rng = np.random.default_rng(seed + n)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    img = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    conf = rng.uniform(1, 9, (n,)).astype(np.float32)
    if keep_fraction >= 1:
        masks = [None, np.zeros(n, dtype=bool)]
    elif keep_fraction <= 0:
        m = np.ones(n, dtype=bool)
        m[[0, n // 2, n - 1]] = False     # the first, one in the middle, the last
        masks = [m, np.ones(n, dtype=bool)]
    else:
        masks = [rng.uniform(0, 1, n) >= keep_fraction]
    for overlap in masks:
        p, c, f, M = device_compact(dev, pts, img, conf, overlap)
        wp, wc, wf = compact_numpy(pts, img, conf, overlap)
        assert M == wp.shape[0], (n, M, wp.shape[0])
        assert np.array_equal(p, wp) and np.array_equal(c, wc) and np.array_equal(f, wf), n


def check_rgb8_values(dev):
    """(uint8)(x * 255.f) for all 256 values k / 255 and 1.0 (and the clamp: below 0, above 1, NaN -> 0)"""
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    vals = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-2)),
                           np.array([1.0, -0.0, -1.0, 1.5, 1e30, np.nan, np.inf, -np.inf], dtype=np.float32)])
    vals = np.concatenate([vals, np.zeros(-len(vals) % 3, np.float32)]).reshape(-1, 3)
    n = vals.shape[0]
    _, c, _, M = device_compact(dev, np.zeros((n, 3), np.float32), vals, np.ones(n, np.float32), None)
    with np.errstate(invalid="ignore"):
        clamped = np.where(np.isnan(vals), np.float32(0), np.clip(vals, np.float32(0), np.float32(1)))
        want = (clamped * np.float32(255.0)).astype(np.uint8)
    assert M == n and np.array_equal(c, want)
    assert c.reshape(-1)[255] == 255 and c.reshape(-1)[0] == 0   # 1.0 -> 255, 0.0 -> 0


# ---------------------------------------------------------------------------------------------------- the stage
def _stage_call(dev, d, thr, src, **kw):
    from instantsplat_amd.init_stage import init_from_pointmaps
    t = lambda a: torch.from_numpy(a).to(dev)
    V = d["depthmaps"].shape[0]
    return init_from_pointmaps(src, V, t(d["images"]), t(d["pointmaps"]), t(d["depthmaps"]), t(d["confidences"]), t(d["intrinsics"]),
                               t(d["w2c"]), d["focals"], STAGE_ORG_SIZE, depth_threshold=thr, **kw)


def check_stage(dev, tmp):
    """init_from_pointmaps on the smallest golden case: the returned InitScene against load_init_scene of the directory it wrote,
    cameras.txt against save_intrinsics', sparse_<n>/1 against the golden test poses, the files against save_points3D's"""
    from instantsplat_amd import io_formats as iof
    from instantsplat_amd import scene_io
    g = golden()
    d, thr, _ = case_inputs(STAGE_CASE)
    V, H, W = d["depthmaps"].shape
    names = [f"test_{i}.png" for i in range(12)]
    src = os.path.join(tmp, "scene")
    r = _stage_call(dev, d, thr, src, conf_aware_ranking=True, n_test=12, test_names=names)
    assert r["order"] == g[f"covis_{STAGE_CASE}_ranking"].tolist()
    want = unpack_mask(g, f"{STAGE_CASE}_ranked", (V, H, W))
    assert_masks_equal(~r["keep_masks"].cpu().numpy(), want, "stage, ranked")
    M = int((~want).sum())
    assert r["pts_num"] == {"depth_threshold": thr, "vanilla": V * H * W, "co_mask_dsp": M, "ratio": M / (V * H * W)}
    ref = dict(line.split(": ") for line in str(g["covis_stage_pts_num_txt"]).strip().split("\n"))   # what save_points3D appended
    assert (float(ref["Depth threshold"]), int(ref["Vanilla points num"]), int(ref["Co_Mask DSP points num"]),
            float(ref["Co_Mask DSP ratio"])) == tuple(r["pts_num"].values())
    sparse0 = os.path.join(src, f"sparse_{V}", "0")
    # the files: confidence_dsp.npy byte for byte, the PLY's vertices, cameras.txt read back
    assert open(os.path.join(sparse0, "confidence_dsp.npy"), "rb").read() == g["covis_stage_confidence_dsp_npy"].tobytes()
    ref_ply = os.path.join(tmp, "reference.ply")
    with open(ref_ply, "wb") as f:
        f.write(g["covis_stage_points3D_ply"].tobytes())
    ours, theirs = iof.read_ply_vertices(os.path.join(sparse0, "points3D.ply")), iof.read_ply_vertices(ref_ply)
    assert ours.shape == theirs.shape == (M,)
    for k in ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"):
        assert np.array_equal(ours[k], theirs[k]), k
    ref_cam = os.path.join(tmp, "reference_cameras.txt")
    with open(ref_cam, "w") as f:
        f.write(str(g["covis_stage_cameras_txt"]))
    for sub, n in (("0", V), ("1", 12)):
        ours, theirs = iof.read_cameras_text(os.path.join(src, f"sparse_{V}", sub, "cameras.txt")), iof.read_cameras_text(ref_cam)
        assert sorted(ours) == list(range(1, n + 1))
        for cam in ours.values():
            t = theirs[1]
            assert (cam.model, cam.width, cam.height) == (t.model, t.width, t.height) and np.array_equal(cam.params, t.params)
    # sparse_<n>/1: the golden test poses under the given names
    imgs = iof.read_images_text(os.path.join(src, f"sparse_{V}", "1", "images.txt"))
    assert [imgs[i + 1].name for i in range(12)] == names
    assert np.abs(r["test_poses"] - g["covis_testposes_n12"]).max() <= 1e-10   # (the bound of check_test_poses_and_ranking)
    for i in range(12):   # images.txt stores a quaternion: the nearest rotation.  The last pose is a float32 training pose, orthonormal
        # to a few float32 ulp (1.2e-7) only, so the round trip moves its entries by that much; 1e-6 is 8 ulp
        assert np.abs(iof.qvec2rotmat(imgs[i + 1].qvec) - r["test_poses"][i, :3, :3]).max() <= 1e-6
        assert np.array_equal(imgs[i + 1].tvec, r["test_poses"][i, :3, 3])
    # the returned scene against the loader's, bit for bit
    sc = r["scene"]
    assert sc.points.device.type == dev.type and sc.points.data_ptr() == r["points"].data_ptr()
    loaded = scene_io.load_init_scene(src, V, device=dev)
    assert torch.equal(sc.points.cpu(), loaded.points) and torch.equal(sc.colors.cpu(), loaded.colors)
    assert torch.equal(sc.confidence_lr.cpu(), loaded.confidence_lr.cpu())
    assert [c.image_name for c in sc.cameras] == [c.image_name for c in loaded.cameras] and sc.cameras_extent == loaded.cameras_extent
    assert loaded.points.shape[0] == M
    return r


def check_stage_switches(dev, tmp):
    """depth_threshold <= 0: no masks, nothing pruned; co_vis_dsp=False: masks computed, nothing pruned; nothing written without a
    source path; max_pts_num refused"""
    import pytest
    d, thr, _ = case_inputs(STAGE_CASE)
    n = d["depthmaps"].size
    r = _stage_call(dev, d, 0.0, None)
    assert r["keep_masks"] is None and r["pts_num"]["co_mask_dsp"] == n and r["scene"] is None and r["points"].shape[0] == n
    r = _stage_call(dev, d, thr, None, co_vis_dsp=False)
    assert r["points"].shape[0] == n and 0 < int(r["keep_masks"].sum()) < n
    assert np.array_equal(r["points"].cpu().numpy(), d["pointmaps"].reshape(-1, 3))
    assert os.listdir(tmp) == []
    with pytest.raises(ValueError, match="not implemented"):
        _stage_call(dev, d, thr, None, max_pts_num=100000)


def check_test_poses_and_ranking():
    """host functions against the reference's own lines (init_geo.py:61-70, 87-111)"""
    from instantsplat_amd.init_stage import confidence_ranking, initial_test_poses
    g = golden()
    d, _, _ = case_inputs(STAGE_CASE)
    for n_test in TEST_POSE_COUNTS:
        got = initial_test_poses(d["w2c"], n_test)
        want = g[f"covis_testposes_n{n_test}"]
        assert got.shape == (n_test, 4, 4) == want.shape
        if n_test <= d["w2c"].shape[0]:
            assert np.array_equal(got, want), n_test          # sampled training poses
        else:   # interpolated: the bound tests/test_camera_path.py holds generate_interpolated_path to against the reference's
            assert np.abs(got - want).max() <= 1e-10, (n_test, np.abs(got - want).max())
    for tag in CASES:
        c = case_inputs(tag)[0]["confidences"]
        got = confidence_ranking(c.astype(np.float64).sum(axis=(1, 2)), c.shape[1], c.shape[2])
        assert got.tolist() == g[f"covis_{tag}_ranking"].tolist(), tag


# ---------------------------------------------------------------------------------------------------- arguments
def check_entry_points_reject_bad_arguments():
    """argument checks of the five entry points, before any HIP call (the bogus device pointers are never touched)"""
    from instantsplat_amd import _lib
    L = _lib.lib()
    EINVAL = -1
    fake = ctypes.c_void_p(0x1000)
    order3 = (ctypes.c_int32 * 3)(0, 1, 2)
    stats = lambda V=3, H=8, W=8, d=fake, c=fake, o=fake, s=fake, out=fake: L.mi355gs_pointmap_stats(None, V, H, W, d, c, o, s, out)
    masks = lambda V=3, H=8, W=8, order=order3, p=fake, d=fake, k=fake, e=fake, s=fake, o=fake: \
        L.mi355gs_covis_masks(None, V, H, W, order, p, d, k, e, s, 0.01, o)
    compact = lambda n=100, ov=fake, p=fake, i=fake, c=fake, s=fake, op=fake, oc=fake, of=fake, cd=fake, ch=fake: \
        L.mi355gs_compact_pointmaps(None, n, ov, p, i, c, s, op, oc, of, cd, ch)
    for fn, kws in ((stats, ("d", "c", "o", "s", "out")), (masks, ("order", "p", "d", "k", "e", "s", "o")), (compact, ("p", "i", "c", "s", "op", "oc", "of", "cd"))):
        for kw in kws:
            assert fn(**{kw: None}) == EINVAL, (fn, kw)
    sizes = (dict(V=0), dict(V=-1), dict(H=0), dict(W=0), dict(H=-2), dict(W=-2), dict(V=257), dict(V=2, H=32768, W=32768),
             dict(V=1, H=65536, W=32768))
    for kw in sizes:
        assert stats(**kw) == EINVAL and masks(**{**kw, "order": (ctypes.c_int32 * 257)(*range(257))}) == EINVAL, kw
        assert L.mi355gs_pointmap_stats_scratch_bytes(kw.get("V", 3), kw.get("H", 8), kw.get("W", 8)) == 0, kw
    for bad in ((0, 1, 1), (0, 1, 3), (-1, 0, 1), (2, 1, 1)):   # not a permutation
        assert masks(order=(ctypes.c_int32 * 3)(*bad)) == EINVAL, bad
    for n in (0, -5, 2 ** 31, 2 ** 40):
        assert compact(n=n) == EINVAL and L.mi355gs_compact_scratch_bytes(n) == 0, n
    assert L.mi355gs_pointmap_stats_scratch_bytes(256, 288, 512) > 0 and L.mi355gs_pointmap_stats_scratch_bytes(1, 1, 1) > 0
    assert L.mi355gs_compact_scratch_bytes(2 ** 31 - 1) >= 4 * (2 ** 31 // COUNT_BLOCK) and L.mi355gs_compact_scratch_bytes(1) > 0


def check_python_rejects_bad_arguments(dev):
    import pytest
    from instantsplat_amd.init_stage import co_visibility_masks, compact_pointmaps, initial_test_poses
    d = synthetic_views(2, 5, 7, 1)
    t = lambda a: torch.from_numpy(a).to(dev)
    good = dict(order=[0, 1], depthmaps=t(d["depthmaps"]), pointmaps=t(d["pointmaps"]), intrinsics=t(d["intrinsics"]), w2c=t(d["w2c"]))
    for kw in (dict(order=[0, 0]), dict(order=[0]), dict(order=[0, 2]), dict(depthmaps=t(d["depthmaps"]).double()),
               dict(pointmaps=t(d["pointmaps"])[:1]), dict(intrinsics=t(d["intrinsics"])[:, :2]), dict(w2c=t(d["w2c"])[:, :3]),
               dict(depthmaps=t(d["depthmaps"])[0])):
        with pytest.raises(ValueError):
            co_visibility_masks(**{**good, **kw})
    with pytest.raises(ValueError):
        compact_pointmaps(t(d["pointmaps"]), t(d["images"])[:1], t(d["confidences"]))
    with pytest.raises(ValueError):
        compact_pointmaps(t(d["pointmaps"]), t(d["images"]), t(d["confidences"]), torch.zeros(3, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError):
        initial_test_poses(d["w2c"][:1], 3)
    with pytest.raises(ValueError):
        initial_test_poses(d["w2c"], 0)


# ---------------------------------------------------------------------------------------------------- training from the scene
def check_three_training_iterations(dev, tmp):
    """setup_training_from_init takes the returned InitScene as it is; the loss is finite and falls"""
    from instantsplat_amd.train import setup_training_from_init, train_iteration
    d, thr, _ = case_inputs(STAGE_CASE)
    r = _stage_call(dev, d, thr, os.path.join(tmp, "scene"), conf_aware_ranking=True)
    st = setup_training_from_init(r["scene"], dev)
    assert st.gaussians._xyz.shape[0] == r["pts_num"]["co_mask_dsp"]
    view = st.rng.getstate()
    losses = []
    for _ in range(3):
        st.rng.setstate(view)   # the same view every time: the loss of one view must fall
        losses.append(float(train_iteration(st)))
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[2] < losses[0]
