"""The device pose tracker (csrc/tracker.hip, pose_tracking.FusedPoseTracker) against float64 — checks shared by the CPU (emulated
kernels) and GPU tiers.

The yardstick is oracle/track_ref.frame: one tracking iteration (pose -> C rasterizer -> masked L1 -> backward -> per-Gaussian pose
terms c[P,7]) evaluated in float64; the same function in float32 sets the 2.5x term.  As in tests/pose_adam_util.py every limit is
min(CAP, max(FLOOR, 2.5 * e_32)):
  * loss:    |l_dev - l_64| / l_64;
  * d_pose:  per component k, |d_dev - d_64| / S_k with S_k = sum_i |c_ik| (pose_adam_util.judge_components).
Each check starts from a pose the device itself rendered (the trace), so float-atomic drift of a run cannot compound.

(FLOOR, CAP) per criterion.  MI355X, GS_CALIBRATE=1, tests/test_tracker_f64_gpu.py — largest device error on a case judged by the FLOOR
alone / on any case:
  track_loss  1.7e-6 / 7.3e-6   (1 x 1 to 1920 x 1080; the largest at 1 x 37 with 49,153 Gaussians, where the float32 oracle errs
                                 as much; 2.4e-8 for the production-size reductions)
  track_pose  3.5e-5 / 1.0e-4   (x S_k; 1 to 65,537 Gaussians, SH degrees 0-3; the largest in the 96 x 64 teacher-forced run, where
                                 the float32 oracle's 2.5x is 2.6e-4: thin views and single Gaussians condition the sums badly)
  posed_sum   5.1e-8 / 5.1e-8   (pose_adam_util's limits, x S_k; C3's 768 rows and a 1080p frame's 257 rows against the eager
                                 node's own terms)
"""
import math

import torch

from oracle import track_ref
from tests import pose_adam_util as pau
from tests.ops_util import bound
from tests.pose_tracking_fused_util import deterministic

LIMITS = {
    "track_loss": (1e-5, 1e-3),
    "track_pose": (1e-4, 1e-3),
}
REL = 2.5


# ================================================================ scenes

def make_scene(dev, P, W, H, degree=0, seed=0, bg="black", spread=1.25):
    """The first P rows of a square syn_pointmap grid (ceil(sqrt(P)) points a side) as frozen Gaussians, seen by its own camera
    through a W x H image whose field of view is `spread` times the grid's (black borders), from a perturbed pose, against a
    random gt.  Every SH band carries small random coefficients (the view-direction term matters from degree 1).
    -> (g, view, pose0, bg)"""
    from instantsplat_amd.camera import Camera
    from instantsplat_amd.pose_utils import get_tensor_from_camera
    from instantsplat_amd.scene import GaussianModel
    from instantsplat_amd.synthetic import SH_C0, syn_pointmap
    Wm = max(1, math.isqrt(P - 1) + 1)
    pm = syn_pointmap(1, Wm, Wm, 64, 64, seed=seed)
    gen = torch.Generator().manual_seed(seed + 7)
    spacing = 8.0 * math.tan(math.radians(30.0)) / Wm
    rot = torch.randn(P, 4, generator=gen)
    rot = rot / rot.norm(dim=1, keepdim=True) * (0.9 + 0.2 * torch.rand(P, 1, generator=gen))
    raw = dict(_xyz=pm.points[:P], _features_dc=((pm.colors[:P] - 0.5) / SH_C0).reshape(P, 1, 3),
               _features_rest=0.2 * torch.randn(P, 15, 3, generator=gen), _opacity=1.0 + torch.randn(P, 1, generator=gen),
               _scaling=math.log(0.8 * spacing) + 0.3 * torch.randn(P, 3, generator=gen), _rotation=rot)
    g = GaussianModel(3)
    for k, v in raw.items():
        setattr(g, k, torch.nn.Parameter(v.float().contiguous().to(dev), requires_grad=False))
    g.active_sh_degree = degree
    w2c = pm.cameras[0].world_view_transform.t().cpu()
    fov = 2.0 * math.atan(spread * math.tan(math.radians(30.0)))
    view = Camera(0, w2c, fov, fov, W, H).to(dev)
    view.original_image = (0.05 + 0.9 * torch.rand(3, H, W, generator=gen)).to(dev)
    pose0 = get_tensor_from_camera(w2c)
    pose0[:4] = pose0[:4] + 0.01 * torch.randn(4, generator=gen)
    pose0[4:] += torch.tensor([0.03, -0.02, 0.04])
    bgt = torch.zeros(3) if bg == "black" else torch.tensor([0.3, 0.6, 0.2])
    return g, view, pose0.float(), bgt.to(dev)


def params_of(g):
    return dict(xyz=g._xyz, f_dc=g._features_dc, f_rest=g._features_rest, opacity=g._opacity, scaling=g._scaling, rotation=g._rotation)


def run_tracker(g, view, bg, degree, pose0, num_iter, det=False):
    """FusedPoseTracker at an exactly counted capacity, all iterations, traces on -> dict(poses, losses, grads, state (CPU), count)"""
    from instantsplat_amd.diff_gaussian_rasterization import BinningPolicy
    from instantsplat_amd.pose_tracking import S_FLAG, FusedPoseTracker, _state_word
    dev = g._xyz.device
    W, H = int(view.image_width), int(view.image_height)
    pose0 = pose0.to(dev).float().contiguous()
    with deterministic(det):
        probe = FusedPoseTracker(g, W, H, 1)
        cnt = probe.count(view, degree, pose0)
        probe.close()
        tr = FusedPoseTracker(g, W, H, BinningPolicy.capacity_for(cnt))
        state = FusedPoseTracker.initial_state(pose0)
        traces = (torch.empty(num_iter, 7, device=dev), torch.empty(num_iter, device=dev), torch.empty(num_iter, 7, device=dev))
        tr.run(view, bg, degree, state, num_iter, traces=traces)
        st = state.cpu()
        tr.close()
    assert _state_word(st, S_FLAG) == 0
    return dict(poses=traces[0].cpu(), losses=traces[1].cpu(), grads=traces[2].cpu(), state=st, count=cnt)


# ================================================================ a, b: one iteration against the float64 oracle

def judge_frame(label, g, view, bg, degree, pose, loss_dev, d_dev):
    """the device's loss and d_pose of one frame rendered at `pose` against track_ref.frame in float64 (float32 sets the 2.5x term)"""
    p = params_of(g)
    o64 = track_ref.frame(p, pose, view, view.original_image, bg, degree, torch.float64)
    o32 = track_ref.frame(p, pose, view, view.original_image, bg, degree, torch.float32)
    l64, l32 = float(o64["loss"]), float(o32["loss"])
    assert math.isfinite(l64) and l64 > 0, (label, l64)
    floor, cap = LIMITS["track_loss"]
    bound(label + "/loss", abs(float(loss_dev) - l64) / l64, min(cap, max(floor, REL * abs(l32 - l64) / l64)))
    c = o64["c"]
    S = c.abs().sum(0)
    assert float(S.sum()) > 0, (label, "no Gaussian reaches the loss")
    pau.judge_components(LIMITS["track_pose"], label + "/d_pose", d_dev, o32["d_pose"], o64["d_pose"], S)


def check_teacher_forced_f64(dev, P, W, H, degree, num_iter, det, bg="black", seed=0):
    """(a) a whole tracking run with traces; iterations 0, 1 and the last are re-evaluated in float64 at the pose the device
    rendered.  The run must also have moved the pose (a run of idle iterations would test one frame three times)."""
    g, view, pose0, bgt = make_scene(dev, P, W, H, degree, seed, bg)
    r = run_tracker(g, view, bgt, degree, pose0, num_iter, det)
    assert not torch.equal(r["poses"][0], r["poses"][-1])
    for i in sorted({0, min(1, num_iter - 1), num_iter - 1}):
        judge_frame("track_tf/%s/P%d_%dx%d_deg%d_%s/it%d" % ("det" if det else "fast", P, W, H, degree, bg, i), g, view, bgt, degree,
                    r["poses"][i], r["losses"][i], r["grads"][i])


def check_frame_f64(dev, W, H, P, degree, bg, seed=0):
    """(b) one iteration of one shape case"""
    g, view, pose0, bgt = make_scene(dev, P, W, H, degree, seed, bg)
    r = run_tracker(g, view, bgt, degree, pose0, 1)
    assert torch.equal(r["poses"][0], pose0)
    judge_frame("track_frame/%dx%d_P%d_deg%d_%s" % (W, H, P, degree, bg), g, view, bgt, degree, pose0, r["losses"][0], r["grads"][0])


# (W, H, P, degree, bg): every size, count, degree and background at least twice, paired so that each image size meets a
# different count; 1,050 masked-L1 workgroups at 640 x 560 (the loss loop's 1024 stride), 193 and 257 pose-partial rows at
# 49,153 and 65,537 Gaussians (the four-way unrolled loop), partial tiles, quadrants and last L1 workgroups everywhere but 96 x 64
SHAPES = [
    (1, 1, 1, 0, "black"), (1, 1, 257, 2, "color"),
    (1, 37, 255, 1, "black"), (1, 37, 49153, 3, "color"),
    (37, 1, 256, 2, "black"), (37, 1, 65537, 0, "black"),
    (17, 9, 257, 3, "black"), (17, 9, 1, 1, "color"),
    (50, 37, 49153, 1, "black"), (50, 37, 256, 0, "color"),
    (96, 64, 65537, 2, "black"), (96, 64, 255, 3, "color"),
    (160, 140, 257, 1, "black"),
    (640, 560, 49152, 0, "black"), (640, 560, 65537, 3, "black"), (640, 560, 257, 1, "color"),
]
# the emulated tier's share: P > 49,152 only at a one-pixel-wide image, 66 masked-L1 workgroups at 160 x 140 (> 64)
SHAPES_EMU = [s for s in SHAPES if s[0] * s[1] <= 160 * 140 and (s[2] <= 49152 or min(s[0], s[1]) == 1)]
SHAPES_GPU_ONLY = [(1920, 1080, 65537, 1, "black"), (1920, 1080, 49153, 3, "color")]


# ================================================================ c: reduction consistency at production size

def c3_scene(dev):
    """SYN-POINTMAP(3,256,256,512,512) (196,608 Gaussians, 768 pose-partial rows): view 1 from the student's pose, SH degree 3 with
    small random higher bands, the teacher's image as gt, black background"""
    from instantsplat_amd.synthetic import syn_pointmap
    from instantsplat_amd.train import setup_training
    st = setup_training(syn_pointmap(3, 256, 256, 512, 512, seed=0), dev)
    g = st.gaussians
    with torch.no_grad():
        g._features_rest.copy_((0.05 * torch.randn(g._features_rest.shape, generator=torch.Generator().manual_seed(5))).to(dev))
    for t in params_of(g).values():
        t.requires_grad_(False)
    g.active_sh_degree = 3
    view = st.cameras[1]
    view.original_image = st.gt_images[1]
    return g, view, g.P.detach()[1].cpu().clone(), st.background


def check_reduction_at_size(dev, kind):
    """(c) deterministic mode, no rasterizer oracle: the tracker's grads[0] against the float64 sum of the per-Gaussian terms rebuilt
    from the eager render node's own raw-parameter gradients under the same masked L1 (check_posed_pose_reduction's way); its
    losses[0] against the float64 masked L1 of the eager image."""
    from instantsplat_amd.arguments import PipelineParams
    from instantsplat_amd.gaussian_renderer import render
    from oracle import pose_ref
    if kind == "c3":
        g, view, pose0, bg = c3_scene(dev)
        degree = 3
    else:   # one 1080p view of 65,537 Gaussians
        degree = 2
        g, view, pose0, bg = make_scene(dev, 65537, 1920, 1080, degree, seed=3)
    P = g._xyz.shape[0]
    with deterministic():
        r = run_tracker(g, view, bg, degree, pose0, 1, det=True)
        params = list(params_of(g).values())
        for t in params:
            t.requires_grad_(True)
        try:
            img = render(view, g, PipelineParams(), bg, camera_pose=pose0.to(dev).clone().requires_grad_(True))["render"]
            gt = view.original_image
            m = (img > 0).float()
            ((img - gt).abs() * m).sum().div(m.sum()).backward()
            d_xyz, d_rot = g._xyz.grad.detach().cpu(), g._rotation.grad.detach().cpu()
        finally:
            for t in params:
                t.grad = None
                t.requires_grad_(False)
    label = "track_reduction/%s_P%d" % (kind, P)
    im, gtc = img.detach().cpu(), gt.cpu()
    losses = {}
    for dt in (torch.float64, torch.float32):
        mm = (im > 0).to(dt)
        losses[dt] = float(((im.to(dt) - gtc.to(dt)).abs() * mm).sum() / mm.sum())
    l64 = losses[torch.float64]
    floor, cap = LIMITS["track_loss"]
    bound(label + "/loss", abs(float(r["losses"][0]) - l64) / l64, min(cap, max(floor, REL * abs(losses[torch.float32] - l64) / l64)))
    xyz, rot = g._xyz.detach().cpu(), g._rotation.detach().cpu()
    terms = {}
    for dt in (torch.float64, torch.float32):
        gm, gr = pose_ref.camera_frame_grads(pose0.to(dt), d_xyz.to(dt), d_rot.to(dt))
        terms[dt] = pose_ref.pose_terms(xyz.to(dt), rot.to(dt), pose0.to(dt), gm, gr)
    c = terms[torch.float64]
    assert float(c.abs().sum()) > 0
    pau.judge_components("posed_sum", label + "/d_pose", r["grads"][0], terms[torch.float32].sum(0), c.sum(0), c.abs().sum(0))


# ================================================================ d: zero loss and ties

def check_zero_loss(dev, W=40, H=28, P=257, degree=1):
    """(d) gt = render() at pose0: the tracker runs the same projection and composite kernels, so every masked pixel differs by
    exactly 0 — sgn(0) = 0 makes loss and d_pose exactly 0; best becomes 0 and the candidate is the post-step pose (weight decay
    alone moved it), which the next iteration renders with a loss above 0."""
    from instantsplat_amd.arguments import PipelineParams
    from instantsplat_amd.gaussian_renderer import render
    from instantsplat_amd.pose_tracking import S_BEST, S_CAND, S_INITIAL
    g, view, pose0, bg = make_scene(dev, P, W, H, degree, seed=4)
    with torch.no_grad():
        view.original_image = render(view, g, PipelineParams(), bg, camera_pose=pose0.to(dev))["render"].contiguous()
    assert bool((view.original_image == 0).any()) and bool((view.original_image > 0).any())   # the mask matters
    for det in (False, True):
        r = run_tracker(g, view, bg, degree, pose0, 2, det)
        st = r["state"]
        assert float(r["losses"][0]) == 0.0 and float(st[S_INITIAL]) == 0.0, (det, r["losses"])
        assert float(r["grads"][0].abs().max()) == 0.0, (det, r["grads"][0])
        assert float(st[S_BEST]) == 0.0
        assert not torch.equal(r["poses"][1], r["poses"][0])
        assert float(r["losses"][1]) > 0.0
        assert torch.equal(st[S_CAND:S_CAND + 7], r["poses"][1]), (det, st[S_CAND:S_CAND + 7], r["poses"][1])


def flat_scene(dev, W=24, H=20):
    """One opaque Gaussian far larger than the view, straight ahead: every pixel clamps alpha at 0.99, so the image is the same
    at every pose near pose0 — a view whose loss stays exactly 0 while the pose moves"""
    from instantsplat_amd.camera import Camera
    from instantsplat_amd.scene import GaussianModel
    from instantsplat_amd.synthetic import SH_C0
    g = GaussianModel(3)
    raw = dict(_xyz=torch.tensor([[0.0, 0.0, 3.0]]), _features_dc=((torch.tensor([0.3, 0.5, 0.7]) - 0.5) / SH_C0).reshape(1, 1, 3),
               _features_rest=torch.zeros(1, 15, 3), _opacity=torch.tensor([[10.0]]), _scaling=torch.full((1, 3), math.log(50.0)),
               _rotation=torch.tensor([[1.0, 0.0, 0.0, 0.0]]))
    for k, v in raw.items():
        setattr(g, k, torch.nn.Parameter(v.to(dev), requires_grad=False))
    g.active_sh_degree = 0
    view = Camera(0, torch.eye(4), 2 * math.atan(0.5), 2 * math.atan(0.5 * H / W), W, H).to(dev)
    return g, view, torch.tensor([1.0, 0, 0, 0, 0, 0, 0]), torch.zeros(3, device=dev)


def check_tied_losses_keep_first_best(dev, num_iter=4):
    """(d) every iteration ties at loss 0: keep-best compares with `<`, so the candidate stays the post-step pose of iteration 0"""
    from instantsplat_amd.arguments import PipelineParams
    from instantsplat_amd.gaussian_renderer import render
    from instantsplat_amd.pose_tracking import S_BEST, S_CAND, S_POSE
    g, view, pose0, bg = flat_scene(dev)
    with torch.no_grad():
        view.original_image = render(view, g, PipelineParams(), bg, camera_pose=pose0.to(dev))["render"].contiguous()
    assert bool((view.original_image > 0).all())
    r = run_tracker(g, view, bg, 0, pose0, num_iter)
    st = r["state"]
    assert bool((r["losses"] == 0).all()) and float(r["grads"].abs().max()) == 0.0, (r["losses"], r["grads"])
    assert len({tuple(p.tolist()) for p in r["poses"]}) == num_iter   # the pose moved every iteration
    assert float(st[S_BEST]) == 0.0
    assert torch.equal(st[S_CAND:S_CAND + 7], r["poses"][1]) and not torch.equal(st[S_CAND:S_CAND + 7], st[S_POSE:S_POSE + 7])


# ================================================================ e: all-masked frames

def masked_scene(dev, kind, W=32, H=32):
    """Gaussians on a 7 x 7 grid of pixel corners (between four pixel centres), black background, camera at the origin.
    kind "unblended": sub-pixel, opacity just above 1/255 — binned, but the alpha at the nearest pixel centre is below 1/255, so
    nothing is blended and the image is exactly black.  kind "black": opaque, blended, SH colour clamped to 0 — black as well."""
    from instantsplat_amd.camera import Camera
    from instantsplat_amd.scene import GaussianModel
    k = torch.arange(4, W, 4, dtype=torch.float32)[:7]
    focal, z = W / (2 * 0.5), 2.0
    ys, xs = torch.meshgrid(k, k, indexing="ij")
    xyz = torch.stack([(xs + 1 - W / 2) / focal * z, (ys + 1 - H / 2) / focal * z, torch.full_like(xs, z)], -1).reshape(-1, 3)
    P = xyz.shape[0]
    g = GaussianModel(3)
    p = 1.02 / 255 if kind == "unblended" else 0.9
    raw = dict(_xyz=xyz, _features_dc=torch.full((P, 1, 3), 0.5 if kind == "unblended" else -10.0), _features_rest=torch.zeros(P, 15, 3),
               _opacity=torch.full((P, 1), math.log(p / (1 - p))), _scaling=torch.full((P, 3), math.log(1e-4 if kind == "unblended" else 0.05)),
               _rotation=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1))
    for n, v in raw.items():
        setattr(g, n, torch.nn.Parameter(v.float().contiguous().to(dev), requires_grad=False))
    g.active_sh_degree = 0
    view = Camera(0, torch.eye(4), 2 * math.atan(0.5), 2 * math.atan(0.5), W, H).to(dev)
    view.original_image = (0.05 + 0.9 * torch.rand(3, H, W, generator=torch.Generator().manual_seed(9))).to(dev)
    return g, view, torch.tensor([1.0, 0, 0, 0, 0, 0, 0]), torch.zeros(3, device=dev)


def _same_nan_pattern(a, b):
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def check_all_masked_frame(dev, kind):
    """(e) one iteration on a frame whose mask is empty although instances were binned: loss (NaN), d_pose, best and candidate as
    the eager loop has them, NaN pattern included.  d_pose is NaN exactly when a (pixel, Gaussian) pair was blended — the eager
    backward reaches a Gaussian's means only through a blended pair — and exactly 0 otherwise."""
    from instantsplat_amd.arguments import PipelineParams
    from instantsplat_amd.gaussian_renderer import render
    from instantsplat_amd.pose_tracking import S_BEST, S_CAND, l1_loss_mask, optimize_view_pose
    g, view, pose0, bg = masked_scene(dev, kind)
    pipe = PipelineParams()
    cam = pose0.to(dev).clone().requires_grad_(True)
    img = render(view, g, pipe, bg, camera_pose=cam)["render"]
    assert bool((img == 0).all())
    loss = l1_loss_mask(img, view.original_image, (img > 0.0).float())
    loss.backward()
    eager = optimize_view_pose(view, g, pipe, bg, pose0, 1)
    r = run_tracker(g, view, bg, 0, pose0, 1)
    assert r["count"] > 0, "no instance was binned: this is the empty view, not an all-masked frame"
    st = r["state"]
    assert math.isnan(float(loss.detach())) and math.isnan(float(r["losses"][0])) and math.isnan(eager["initial_loss"])
    assert _same_nan_pattern(r["grads"][0], cam.grad), (kind, r["grads"][0], cam.grad)
    assert bool(torch.isnan(cam.grad).all()) == (kind == "black") and bool(torch.isnan(cam.grad).any()) == (kind == "black")
    assert float(st[S_BEST]) == eager["best_loss"] == float(torch.tensor(1e20))
    assert torch.equal(st[S_CAND:S_CAND + 7], eager["pose"].cpu()) and torch.equal(eager["pose"].cpu(), pose0)
