"""The per-Gaussian kernels of csrc/preprocess.hip — projection forward, its closed-form backward, k_mark_visible — against
float64, per Gaussian, under general cameras.  Cases and checks shared by the emulated (CPU) and the GPU test files.

Everything else in tests/ hands the rasterizer an identity view matrix and a camera at the origin (four of the six entries of
M = J W are then zero) and compares one relative L2 per gradient tensor.  Here every case has a rigid world-to-camera (R, t)
(CAMERAS), the families place Gaussians where the kernels branch (FAMILIES), and every quantity is compared row by row:

  row error of a tensor g:   e_i = |d_i - g64_i| / max(|g64_i|, 1e-3 max_j |g64_j|)      (|.|: L2 norm of the row; every row)
  criterion per case/tensor: E_dev = max_i e_i <= min(CAP, max(FLOOR, 2.5 E_32))

E_32 is the same quantity for the float32 restatement against float64 (gradients: the float32 build of oracle/gs_ref.c against
its float64 build; forward records: oracle/raster_torch.preprocess in float32 against float64).  CAP = 1e-2 is a condition, not
a measurement: a wrong branch changes a row at order 1.  FLOOR is the largest E_32 of that tensor over all cases of the family
(family_floors(): from the two oracles alone, on the CPU, when a test first asks for it; the values it gives are listed below;
for the forward records the maximum runs over the cases of all families, see there).
Rows whose float64 gradient is all zero (culled, invisible, masked) must be exactly zero on the device; visibility and SH clamp
bits are compared exactly, which is a property of the inputs, not of rounding: settle() keeps every depth 1e-3 away from 0.2,
every t.x/t.z 1e-4 away from the EWA limit, every SH colour channel 1e-3 away from 0 and every 3-sigma radius away from an
integer, and bounds the condition of every 2-D covariance.  The device runs the judged frames with the composite backward's
units at their longest and its deterministic sums (device_mode() says what each keeps out of the comparison, with figures).  All
limits go through ops_util.bound (GS_CALIBRATE=1 lists them with the measured values).

FLOORS (CPU, the two oracles alone; largest E_32 over the family's cases):
  (gradients: columns means3D, means2D, opac, shs, colors, scales, rots, cov3D; forward records: centre, conic, colour, depth)
  blob                   1.1e-4  1.2e-4  1.4e-4  4.0e-5  -       5.1e-5  9.6e-5  -      |
  frustum                2.0e-5  2.6e-5  9.4e-5  3.4e-6  -       3.0e-5  3.6e-5  -      |  1.0e-5  5.4e-6  3.0e-6  1.2e-7
  frustum, clamped rows  2.0e-5  2.6e-5  9.4e-5  3.4e-6  -       1.2e-5  2.4e-5  -      |  6.6e-7  4.7e-7  1.2e-7  1.0e-7
  sh_clamp               1.8e-4  1.4e-4  1.4e-3  1.8e-4  -       2.5e-4  1.2e-4  -      |  (forward records: one floor for all
  precomp                3.0e-5  3.3e-5  1.5e-4  2.8e-5  1.6e-5  -       -       4.7e-5 |   families, see family_floors)
  modifier               4.3e-5  5.6e-5  9.7e-5  2.5e-5  -       3.4e-5  3.6e-5  -      |
  block_edges            1.1e-4  9.6e-5  1.9e-4  6.8e-5  -       7.3e-5  1.2e-4  -      |

DEVICE (largest E_dev over the family's cases; emulated kernels / MI355X):
  (same columns; the MI355X's figure only where it differs from the emulated kernels' in the digits shown)
  blob                   1.1e-4  1.2e-4  1.3e-4/1.4e-4  3.8e-5  -  5.0e-5/8.2e-5  9.7e-5  -              |  5.2e-6  3.9e-6  2.9e-6  1.2e-7
  frustum                2.0e-5/2.2e-5  1.7e-5/2.3e-5  9.2e-5/9.8e-5  3.4e-6/3.5e-6  -  3.4e-5/1.6e-5  3.4e-5/3.0e-5  -  |  1.1e-6  5.6e-7  1.3e-7  1.0e-7
  frustum, clamped rows  2.0e-5/2.2e-5  1.7e-5/2.3e-5  4.8e-5/9.8e-5  3.4e-6/3.5e-6  -  1.7e-5/1.6e-5  3.4e-5/3.0e-5  -  |  6.6e-7  5.6e-7  1.2e-7  1.0e-7
  sh_clamp               1.9e-4  1.4e-4  1.4e-3  2.1e-4  -       2.5e-4  1.3e-4  -                        |  7.0e-7  4.8e-7  1.3e-6  9.0e-8
  precomp                2.9e-5  3.2e-5  1.2e-4  2.8e-5  1.6e-5  -       -       5.0e-5                   |  1.8e-6  3.0e-6  4.4e-7  8.6e-8
  modifier               4.1e-5/4.0e-5  5.4e-5/5.2e-5  9.7e-5/9.8e-5  2.4e-5  -  2.5e-5/4.6e-5  3.6e-5/4.6e-5  -  |  4.9e-7  5.2e-6  2.8e-6  7.7e-8
  block_edges            1.1e-4  9.7e-5/9.4e-5  2.0e-4/1.9e-4  6.8e-5  -  7.1e-5  1.2e-4  -               |  1.0e-5  2.4e-6  4.8e-7  9.5e-8
  posed node (check 3):  posed against unposed rows 8e-6 (f_dc, opl) ... 5.8e-5 (scaling) on the MI355X, bit-identical on the emulated
  kernels; pose components <= 3.0e-7 S_k on both.  Every test of the GPU file takes under 0.05 s.

ROWS per case, from the float64 oracle (check_case_counts; moved: rows with a non-zero means3D gradient; clamped: by the EWA limit in
x only / y only / both; SH-clamped: visible rows with a clamp bit set):
  blob                   P 400: visible 381 ... 395, moved 374 ... 388, SH-clamped 139 ... 170
  frustum                P 300: visible 296 ... 299, moved 267 ... 276; clamped, visible and moved: identity 67 / 90 / 30, generic 79 / 88 / 30,
                         rot180y 68 / 94 / 29, translation 74 / 85 / 29, rotation 76 / 79 / 23
  sh_clamp               P 240: all visible and moved; each of the 8 clamp-bit patterns on 30 rows (210 rows with a bit set)
  precomp                P 300: visible 290 / 294, moved 286 / 290, SH-clamped 136 (cov+sh2)
  modifier               P 300: visible 290, moved 287, SH-clamped 122
  block_edges            P 1 / 255 / 256 / 257: visible 1 / 246 / 247 / 246, moved 1 / 240 / 242 / 244, first and last row among them

MUTATIONS (each applied to a copy of the tree outside the repository, emulated library built from it with tests/emu/build_emu.sh,
tests/test_projection_emu.py run on it; the first failing test of each is named, the number is how many of the file's tests fail):
  (a) xmul / ymul forced to 1 in the backward        6: test_gradient_rows_through_the_operator[frustum/identity] (all five frustum cases,
                                                        and frustum/rot180y through the C ABI); nothing outside the frustum family
  (b) view[4] and view[1] swapped in ewa_setup        33: test_forward_records_per_gaussian[blob/generic/sh3] (every case under the generic and the
                                                        rotation camera: records, gradients, posed node; none under a diagonal W)
  (c) campos taken as zero in the backward's SH dir.  22: test_gradient_rows_through_the_operator[blob/generic/sh3] (every SH case with campos != 0)
  (d) clamp bit 2 ignored in the backward             19: test_gradient_rows_through_the_operator[blob/identity/sh3] (every SH case: "a clamped
                                                        channel received a gradient", and the means3D rows)
  (e) mean gradient rotated by W instead of W^T       18: test_gradient_rows_through_the_operator[blob/generic/sh3] (generic and rotation cameras,
                                                        posed node; rot180y's W is symmetric)
"""
import contextlib
import functools
import math
from types import SimpleNamespace

import torch

from instantsplat_amd.camera import Camera
from instantsplat_amd.synthetic import syn_blob
from oracle import gs_ref, pose_ref
from oracle import raster_torch as rt
from tests import frame_abi, ops_util
from tests.pose_adam_util import LIMITS, judge_components

F64, F32 = torch.float64, torch.float32
CAP = 1e-2
REL = 2.5
LOG2E = 1.4426950408889634
BG = (0.2, 0.5, 0.9)
MAX_CONDITION = 50.0   # largest eigenvalue ratio of a case's 2-D covariances (settle)


# ---------------------------------------------------------------------------------------------------- cameras
def _axis_angle(axis, angle):
    a = torch.tensor(axis, dtype=F64)
    a = a / a.norm()
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=F64)
    return torch.eye(3, dtype=F64) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


# name -> (R, t) of x_cam = R x_world + t
CAMERAS = {
    "identity": (torch.eye(3, dtype=F64), torch.zeros(3, dtype=F64)),                                     # the control
    "generic": (_axis_angle((0.3, -0.8, 0.5), 1.1), torch.tensor([0.7, -1.3, 2.1], dtype=F64)),
    "rot180y": (torch.diag(torch.tensor([-1.0, 1.0, -1.0], dtype=F64)), torch.tensor([0.4, -0.2, 0.6], dtype=F64)),   # negative diagonal in W
    "translation": (torch.eye(3, dtype=F64), torch.tensor([-0.9, 0.6, 1.4], dtype=F64)),                  # identity W, campos != 0
    "rotation": (_axis_angle((-0.5, 0.4, 0.75), 0.8), torch.zeros(3, dtype=F64)),                        # campos = 0
}


def camera_setup(R, t, cam):
    """A rigid world-to-camera (R, t) and a Camera (for its projection) in the row-vector convention of include/mi355gs.h:
    -> (viewmatrix = W2C^T, projmatrix = viewmatrix @ projection_matrix, campos = -R^T t), float64."""
    R, t = R.to(F64), t.to(F64)
    w2c = torch.eye(4, dtype=F64)
    w2c[:3, :3], w2c[:3, 3] = R, t
    view = w2c.t().contiguous()
    return view, view @ cam.projection_matrix.to(F64).cpu(), -(R.t() @ t)


def to_world(x_cam, R, t):
    """camera-frame points [n,3] -> world frame: the rows (x_cam - t) R"""
    return (x_cam.to(F64) - t.to(F64)) @ R.to(F64)


def pinhole(W, H, fovx_deg=60.0):
    fovx = math.radians(fovx_deg)
    tanx = math.tan(fovx / 2)
    tany = tanx * H / W
    return Camera(0, torch.eye(4), fovx, 2 * math.atan(tany), W, H), tanx, tany


# ---------------------------------------------------------------------------------------------------- families (camera frame, float64)
def _quats(g, n, lo, hi):
    q = torch.randn(n, 4, generator=g, dtype=F64)
    return q / q.norm(dim=1, keepdim=True) * (lo + (hi - lo) * torch.rand(n, 1, generator=g, dtype=F64))


def _blob(P, W, H, seed, scale_mean, q_lo=0.3, q_hi=3.0, log_spread=0.6):
    """syn_blob with raw quaternions of norm 0.3 ... 3 (the operator uses them un-normalised: sizes x 0.09 ... 9), higher SH
    bands three times syn_blob's, and the 2 % it puts behind the near plane kept away from the plane itself"""
    sc = syn_blob(P, W, H, seed=seed, scale_mean=scale_mean)
    g = torch.Generator().manual_seed(7000 + seed)
    means = sc.means3D.double().clone()
    near = (means[:, 2] - 0.2).abs() < 0.01
    means[near, 2] = 0.1
    log_scales = math.log(scale_mean) + (log_spread / 0.6) * (sc.scaling_logit.double() - math.log(scale_mean))   # syn_blob's spread is 0.6
    return dict(means=means, scales=torch.exp(log_scales), rots=_quats(g, P, q_lo, q_hi),
                opac=torch.sigmoid(sc.opacity_logit.double()), shs=torch.cat([sc.shs[:, :1].double(), 3.0 * sc.shs[:, 1:].double()], 1))


def _block_edges(P, W, H, seed, tanx, tany):
    """P = 1, 255, 256, 257 (one thread per Gaussian, 256-thread workgroups): the first and the last Gaussian in the image"""
    d = _blob(P, W, H, seed, 0.03)
    d["means"][0] = torch.tensor([0.1 * tanx * 3.0, -0.1 * tany * 3.0, 3.0], dtype=F64)
    d["means"][P - 1] = torch.tensor([-0.2 * tanx * 4.0, 0.15 * tany * 4.0, 4.0], dtype=F64) if P > 1 else d["means"][0]
    d["rots"][0] = d["rots"][0] / d["rots"][0].norm()
    d["rots"][P - 1] = d["rots"][P - 1] / d["rots"][P - 1].norm()
    d["scales"][0] = d["scales"][P - 1] = 0.08
    d["opac"][0] = d["opac"][P - 1] = 0.6
    return d


FRUSTUM_KINDS = ("x", "y", "xy")


def _frustum(P, seed, tanx, tany):
    """Gaussians outside the frustum that still reach pixels: centres at 1.0 ... 1.8 x the frustum edge (the EWA clamp is at
    1.3 x; none within 0.02 of it) in x only, in y only, or in both — a third each, both signs —, depth 2 ... 5, scales about
    0.25 z tan(fov/2), so most of them cover pixels of the border.  Opacity 0.04 ... 0.14: every tile of these frames holds
    100 - 150 instances, and with opaque Gaussians (0.3 ... 0.9) the transmittance falls to 1e-4 across them — the back-to-front
    replay then rebuilds T over four decades, and the worst rows of both float32 sides are decided by that, not by the branch
    this family is about; at these opacities T stays above 0.2."""
    g = torch.Generator().manual_seed(8000 + seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    z = 2.0 + 3.0 * u(P)
    kind = torch.arange(P) % 3
    out = 1.0 + 0.8 * u(P, 2)
    close = (out - 1.3).abs() < 0.02
    out = torch.where(close, torch.full_like(out, 1.33), out)
    inside = 0.8 * (2.0 * u(P, 2) - 1.0)
    sign = torch.where(u(P, 2) < 0.5, -1.0, 1.0).to(F64)
    fx = torch.where(kind != 1, sign[:, 0] * out[:, 0], inside[:, 0])
    fy = torch.where(kind != 0, sign[:, 1] * out[:, 1], inside[:, 1])
    means = torch.stack([fx * tanx * z, fy * tany * z, z], dim=1)
    scales = 0.25 * z[:, None] * tanx * (0.7 + 0.6 * u(P, 3))
    shs = torch.zeros(P, 16, 3, dtype=F64)
    shs[:, 0] = (u(P, 3) - 0.3) / rt.SH_C0 * 0.8
    shs[:, 1:] = 0.1 * torch.randn(P, 15, 3, generator=g, dtype=F64)
    return dict(means=means, scales=scales, rots=_quats(g, P, 0.9, 1.1), opac=0.04 + 0.1 * u(P, 1), shs=shs), kind


def _sh_clamp(P, seed, tanx, tany):
    """Gaussians inside the frustum; higher SH bands of size 0.15 (the view-direction term carries weight); the DC coefficient
    is set afterwards, under the case's camera, so that row i has clamp-bit pattern i % 8 (_set_clamp_patterns)"""
    g = torch.Generator().manual_seed(9000 + seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    z = 2.0 + 4.0 * u(P)
    means = torch.stack([0.9 * (2 * u(P) - 1) * tanx * z, 0.9 * (2 * u(P) - 1) * tany * z, z], dim=1)
    scales = 0.05 * torch.exp(0.4 * torch.randn(P, 3, generator=g, dtype=F64))
    shs = torch.zeros(P, 16, 3, dtype=F64)
    shs[:, 1:] = 0.15 * torch.randn(P, 15, 3, generator=g, dtype=F64)
    target = 0.05 + 0.55 * u(P, 3)
    return dict(means=means, scales=scales, rots=_quats(g, P, 0.9, 1.1), opac=0.2 + 0.7 * u(P, 1), shs=shs), target


def _set_clamp_patterns(case, target):
    """DC coefficients such that, under the case's camera and degree, channel c of row i has the colour -target (clamped) if bit
    c of i % 8 is set and +target otherwise: |colour| is 0.05 ... 0.6, far from the edge of the clamp"""
    i = case.inp
    P = i["means3D"].shape[0]
    d = i["means3D"].double() - case.campos.double()[None]
    d = d / d.norm(dim=1, keepdim=True)
    shs = i["shs"].double().clone()
    shs[:, 0] = 0.0
    rest = rt.sh_to_rgb(case.deg, shs, d)
    bits = (torch.arange(P)[:, None] >> torch.arange(3)[None]) & 1
    want = torch.where(bits == 1, -target, target)
    shs[:, 0] = (want - 0.5 - rest) / rt.SH_C0
    i["shs"] = shs.float()


# ---------------------------------------------------------------------------------------------------- cases
# name -> (family, camera, dict of what differs from the defaults P=400, W=64, H=48, deg=3, seed=1)
SPECS = {
    "blob/identity/sh3": ("blob", "identity", dict(seed=1)),
    "blob/generic/sh3": ("blob", "generic", dict(seed=2)),
    "blob/rot180y/sh2": ("blob", "rot180y", dict(seed=3, deg=2)),
    "blob/translation/sh1": ("blob", "translation", dict(seed=4, deg=1)),
    "blob/rotation/sh0": ("blob", "rotation", dict(seed=5, deg=0)),
    "blob/generic/sh2/50x37": ("blob", "generic", dict(seed=6, deg=2, W=50, H=37)),   # last tile row and column partial
    "frustum/identity": ("frustum", "identity", dict(P=300, seed=1, deg=1)),
    "frustum/generic": ("frustum", "generic", dict(P=300, seed=2, deg=1)),
    "frustum/rot180y": ("frustum", "rot180y", dict(P=300, seed=3, deg=1)),
    "frustum/translation": ("frustum", "translation", dict(P=300, seed=4, deg=1)),
    "frustum/rotation": ("frustum", "rotation", dict(P=300, seed=5, deg=1)),
    "sh_clamp/generic/sh1": ("sh_clamp", "generic", dict(P=240, seed=1, deg=1)),
    "sh_clamp/translation/sh2": ("sh_clamp", "translation", dict(P=240, seed=2, deg=2)),
    "sh_clamp/generic/sh3": ("sh_clamp", "generic", dict(P=240, seed=3, deg=3)),
    "precomp/generic/cov+sh2": ("precomp", "generic", dict(P=300, seed=1, deg=2, cov=True)),
    "precomp/generic/cov+colors": ("precomp", "generic", dict(P=300, seed=2, cov=True, colors=True)),
    "modifier/generic/published": ("modifier", "generic", dict(P=300, seed=1, deg=1, mod=1.7, exact=0)),
    "modifier/generic/exact": ("modifier", "generic", dict(P=300, seed=1, deg=1, mod=1.7, exact=1)),
    "block_edges/generic/P1": ("block_edges", "generic", dict(P=1, seed=1, deg=1)),
    "block_edges/generic/P255": ("block_edges", "generic", dict(P=255, seed=2, deg=1)),
    "block_edges/generic/P256": ("block_edges", "generic", dict(P=256, seed=3, deg=1)),
    "block_edges/generic/P257": ("block_edges", "generic", dict(P=257, seed=4, deg=1)),
}
FAMILIES = ("blob", "frustum", "sh_clamp", "precomp", "modifier", "block_edges")
NAMES = tuple(SPECS)
SPLIT_ABI_NAMES = ("blob/generic/sh3", "sh_clamp/translation/sh2", "frustum/rot180y", "block_edges/generic/P257")   # raw C ABI, shs + shs_rest


def family_cases(family):
    return [n for n in NAMES if SPECS[n][0] == family]


def build_case(family, camera, P=400, W=64, H=48, deg=3, seed=1, mod=1.0, exact=0, cov=False, colors=False, name=None):
    """One case: float32 inputs in the WORLD frame of `camera` (generated in the camera frame in float64, transported, rounded
    once — the float32 values are the case; both oracles and the device read them) and the seeded dL/dpixel."""
    cam, tanx, tany = pinhole(W, H)
    R, t = CAMERAS[camera]
    kind = target = None
    if family in ("blob", "precomp", "modifier"):
        d = _blob(P, W, H, seed, 0.03 if family != "modifier" else 0.02)
    elif family == "block_edges":
        d = _block_edges(P, W, H, seed, tanx, tany)
    elif family == "frustum":
        d, kind = _frustum(P, seed, tanx, tany)
    elif family == "sh_clamp":
        d, target = _sh_clamp(P, seed, tanx, tany)
    else:
        raise KeyError(family)
    view, proj, campos = camera_setup(R, t, cam)
    inp = dict(means3D=to_world(d["means"], R, t).float(), opac=d["opac"].float())
    if colors:
        inp["colors"] = torch.sigmoid(d["shs"][:, 0] * 1.5).float()
    else:
        inp["shs"] = d["shs"].float()
    if cov:
        inp["cov3D"] = rt.cov3d_from_scale_rot(d["scales"], 1.0, d["rots"]).float()
    else:
        inp["scales"], inp["rots"] = d["scales"].float(), d["rots"].float()
    wgt = torch.randn(3, H, W, generator=torch.Generator().manual_seed(100 + seed))
    case = SimpleNamespace(name=name or "%s/%s" % (family, camera), family=family, camera=camera, P=P, W=W, H=H, deg=0 if colors else deg,
                           mod=mod, exact=exact, tanx=tanx, tany=tany, view=view.float(), proj=proj.float(), campos=campos.float(),
                           bg=torch.tensor(BG), inp=inp, wgt=wgt, kind=kind)
    if target is not None:
        _set_clamp_patterns(case, target)
    settle(case)
    return case


@functools.lru_cache(maxsize=None)
def get_case(name):
    family, camera, kw = SPECS[name]
    return build_case(family, camera, name=name, **kw)


ORACLE_DEFAULTS = {   # what tests/test_oracle.py runs through both oracles under every camera
    "blob": dict(P=200, deg=3), "frustum": dict(P=300, deg=1), "sh_clamp": dict(P=240, deg=2), "precomp": dict(P=150, deg=2, cov=True),
    "modifier": dict(P=150, deg=1, mod=1.7, exact=1), "block_edges": dict(P=257, deg=1),
}


@functools.lru_cache(maxsize=None)
def oracle_case(family, camera):
    return build_case(family, camera, seed=11, **ORACLE_DEFAULTS[family])


def settings(case, cls, dtype=F32, dev="cpu"):
    """the 12-field settings tuple (oracle.raster_torch.RasterSettings or the operator's GaussianRasterizationSettings)"""
    c = lambda x: x.to(dev, dtype)
    return cls(case.H, case.W, case.tanx, case.tany, c(case.bg), case.mod, c(case.view), c(case.proj), case.deg, c(case.campos), False, False)


def _raster_kwargs(lv):
    kw = {}
    if "colors" in lv:
        kw["colors_precomp"] = lv["colors"]
    else:
        kw["shs"] = lv["shs"]
    if "cov3D" in lv:
        kw["cov3D_precomp"] = lv["cov3D"]
    else:
        kw["scales"], kw["rotations"] = lv["scales"], lv["rots"]
    return kw


def geometry(case, dtype=F64):
    """oracle/raster_torch.preprocess on the case's inputs in `dtype`, plus the branch flags of ewa_setup and the unrounded
    3-sigma radius"""
    with torch.no_grad():
        lv = {k: v.to(dtype) for k, v in case.inp.items()}
        st = settings(case, rt.RasterSettings, dtype)
        g = rt.preprocess(lv["means3D"], lv["opac"], st, **_raster_kwargs(lv))
        pv = rt._tp43(lv["means3D"], st.viewmatrix.reshape(-1))
        front = pv[:, 2] > 0.2
        zs = torch.where(front, pv[:, 2], torch.ones_like(pv[:, 2]))
        g["txtz"], g["tytz"] = pv[:, 0] / zs, pv[:, 1] / zs
        g["front"] = front
        g["clamp_x"] = front & (g["txtz"].abs() > 1.3 * case.tanx)
        g["clamp_y"] = front & (g["tytz"].abs() > 1.3 * case.tany)
        cA, cB, cC = g["conic"].unbind(-1)
        dc = cA * cC - cB * cB
        a, b, c = cC / dc, -cB / dc, cA / dc
        mid = 0.5 * (a + c)
        g["cov2"] = torch.stack([a, b, c], -1)
        g["radius_raw"] = 3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - (a * c - b * b), min=0.1)))
        if "shs" in lv:
            d = lv["means3D"] - st.campos[None]
            g["raw_rgb"] = rt.sh_to_rgb(case.deg, lv["shs"], d / d.norm(dim=1, keepdim=True)) + 0.5
        g["clamp_bits"] = (g["clamped"].to(torch.int64) * torch.tensor([1, 2, 4])).sum(1)
    return g


def settle(case):
    """Makes every discrete outcome of the projection a property of the inputs: no depth within 1e-3 of the 0.2 cull plane, no
    t.x/t.z (t.y/t.z) within 1e-4 of the EWA limit (asserted: the families are built that way), no SH colour channel within
    1e-3 of the clamp at 0 and no 3-sigma radius within float32's reach of an integer (nudged: the DC coefficient by 0.02, the
    size by 1.3 %).
    And bounds the conditioning: no 2-D covariance (low-pass included) with an eigenvalue ratio above MAX_CONDITION; such a
    Gaussian shrinks by 0.8 until it has.  The conic backward divides by det^2, so whatever rounding its inputs carry reaches
    dL/dscales and dL/drots multiplied by about that ratio: a needle of ratio 220 (|q| 2.9, one axis 12 px, one below a pixel)
    stood 1.6e-4 from float64 in the float32 oracle and 4e-4 ... 6e-4 on the MI355X depending on the order of its sums — which
    float32 evaluation is luckier in such a row says nothing about a branch.  Needles are edge_cases.check_giant_and_needle_gaussians's."""
    for _ in range(40):
        g = geometry(case)
        assert float((g["depth"] - 0.2).abs().min()) >= 1e-3, case.name
        f = g["front"]
        if bool(f.any()):
            assert float((g["txtz"][f].abs() - 1.3 * case.tanx).abs().min()) >= 1e-4, case.name
            assert float((g["tytz"][f].abs() - 1.3 * case.tany).abs().min()) >= 1e-4, case.name
        r = g["radius_raw"]
        bad_r = f & ((r - torch.round(r)).abs() < 1e-4 + 2e-5 * r)
        bad_c = None
        if "raw_rgb" in g:
            bad_c = f[:, None] & (g["raw_rgb"].abs() < 1e-3)
        a, b, c = g["cov2"].unbind(-1)
        root = torch.sqrt((0.5 * (a - c)) ** 2 + b * b)
        bad_k = f & ((0.5 * (a + c) + root) > MAX_CONDITION * (0.5 * (a + c) - root))
        if not bool(bad_r.any()) and not bool(bad_k.any()) and (bad_c is None or not bool(bad_c.any())):
            return
        if bool(bad_k.any()):
            if "cov3D" in case.inp:
                case.inp["cov3D"][bad_k] *= 0.64
            else:
                case.inp["scales"][bad_k] *= 0.8
            continue
        if bool(bad_r.any()):
            if "cov3D" in case.inp:
                case.inp["cov3D"][bad_r] *= 1.026
            else:
                case.inp["scales"][bad_r] *= 1.013
        if bad_c is not None and bool(bad_c.any()):
            step = torch.where(g["raw_rgb"] < 0, -0.02, 0.02).float() / rt.SH_C0
            case.inp["shs"][:, 0] += torch.where(bad_c, step, torch.zeros_like(step))
    raise AssertionError("settle: %s did not settle" % case.name)


# ---------------------------------------------------------------------------------------------------- the oracles
@contextlib.contextmanager
def oracle_scale_grad(exact):
    old = gs_ref.lib().gsref_set_scale_grad_exact(int(exact))
    old_t, rt.SCALE_GRAD_EXACT = rt.SCALE_GRAD_EXACT, bool(exact)
    try:
        yield
    finally:
        gs_ref.lib().gsref_set_scale_grad_exact(old)
        rt.SCALE_GRAD_EXACT = old_t


def _leaves(case, dtype, dev):
    lv = {k: v.clone().to(dev, dtype).requires_grad_(True) for k, v in case.inp.items()}
    m2d = torch.zeros(case.P, 3, dtype=dtype, device=dev, requires_grad=True)
    return lv, m2d


def _collect(lv, m2d, color, radii):
    grads = {k: v.grad.detach().cpu().clone() for k, v in lv.items()}
    grads["means2D"] = m2d.grad.detach().cpu().clone()
    return dict(color=color.detach().cpu(), radii=radii.cpu(), grads=grads)


def run_reference(case, dtype, which="c"):
    """forward + backward of sum(image * case.wgt) through the C oracle ("c") or the dense autograd restatement ("torch")"""
    lv, m2d = _leaves(case, dtype, "cpu")
    st = settings(case, rt.RasterSettings, dtype)
    with oracle_scale_grad(case.exact):
        if which == "c":
            color, radii = gs_ref.rasterize(lv["means3D"], m2d, lv["opac"], st, **_raster_kwargs(lv))
        else:
            color, radii = rt.rasterize(lv["means3D"], lv["opac"], st, means2D=m2d, **_raster_kwargs(lv))
        (color * case.wgt.to(dtype)).sum().backward()
    return _collect(lv, m2d, color, radii)


@functools.lru_cache(maxsize=None)
def oracle(name, double):
    """the C oracle's result for a named case, computed once and shared (never modified)"""
    return run_reference(get_case(name), F64 if double else F32)


# ---------------------------------------------------------------------------------------------------- row errors and limits
def row_errors(d, g64):
    """e_i = |d_i - g64_i| / max(|g64_i|, 1e-3 max_j |g64_j|) for every row i"""
    n = g64.shape[0]
    d, g = d.detach().cpu().double().reshape(n, -1), g64.detach().cpu().double().reshape(n, -1)
    if n == 0:
        return torch.zeros(0, dtype=F64)
    norm = g.norm(dim=1)
    top = float(norm.max())
    if top == 0.0:   # an all-zero reference: only an exact match has no error
        return torch.where((d != 0).any(dim=1), torch.full_like(norm, float("inf")), torch.zeros_like(norm))
    return (d - g).norm(dim=1) / torch.clamp(norm, min=1e-3 * top)


def _emax(e, rows=None):
    if rows is not None:
        e = e[rows]
    return float(e.max()) if e.numel() else 0.0


def forward_rows(g, rows=None):
    """the per-Gaussian forward quantities of a preprocess() result as row tensors"""
    return {"fwd centre": torch.stack([g["px"], g["py"]], -1), "fwd conic": g["conic"], "fwd colour": g["rgb"], "fwd depth": g["depth"][:, None]}


def subsets(case):
    """name -> row mask (None: all rows) of the row sets a case is judged on"""
    if case.family != "frustum":
        return {"": None}
    g = geometry(case)
    return {"": None, " [clamped rows]": g["visible"] & (g["clamp_x"] | g["clamp_y"])}


@functools.lru_cache(maxsize=None)
def family_floors(family):
    """{(tensor, subset): largest E_32 over the family's cases} from the two oracles alone (CPU).  Gradients: the float32 build of
    gs_ref.c against its float64 build, over the cases of `family`.  Forward records: raster_torch.preprocess in float32 against
    float64 over ALL cases of this file (the clamped rows: over the frustum family, which alone has them) — the projection is
    the same arithmetic in every family, and PyTorch's float32 operators round in another order than the kernel, so the worst row
    of two or three cases is too small a sample of it to be a floor."""
    floors = {}
    for name in family_cases(family):
        case = get_case(name)
        o32, o64 = oracle(name, False), oracle(name, True)
        for sub, rows in subsets(case).items():
            for k, g in o64["grads"].items():
                key = ("grad " + k, sub)
                floors[key] = max(floors.get(key, 0.0), _emax(row_errors(o32["grads"][k], g), rows))
    for name in NAMES:
        case = get_case(name)
        g32, g64 = geometry(case, F32), geometry(case, F64)
        vis = g64["visible"] & g32["visible"]
        for sub, rows in subsets(case).items():
            for k, g in forward_rows(g64).items():
                sel = vis if rows is None else vis & rows
                key = (k, sub)
                floors[key] = max(floors.get(key, 0.0), _emax(row_errors(forward_rows(g32)[k][sel], g[sel])))
    return floors


def describe_rows(case, idx):
    """family, camera and branch flags of the given rows, from the float64 oracle"""
    g = geometry(case)
    lines = []
    for i in idx:
        i = int(i)
        lines.append("    row %3d: %s, camera %s, depth %+.4f, visible %d, radius %d, t.x/t.z %+.3f (lim %.3f, clamped %d), t.y/t.z %+.3f (lim %.3f, "
                     "clamped %d), SH clamp bits %d" % (i, case.family, case.camera, float(g["depth"][i]), int(g["visible"][i]), int(g["radius"][i]),
                                                        float(g["txtz"][i]), 1.3 * case.tanx, int(g["clamp_x"][i]), float(g["tytz"][i]),
                                                        1.3 * case.tany, int(g["clamp_y"][i]), int(g["clamp_bits"][i])))
    return "\n".join(lines)


def judge_rows(case, what, tensor, dev, r32, r64, index=None, path="operator"):
    """The criterion of this file for one tensor of one case, on every row set of the case; `index`: the rows of the case the
    given row tensors hold (forward records: the visible ones).  The worst rows are printed when a limit is missed."""
    floors = family_floors(case.family)
    e_dev, e_32 = row_errors(dev, r64), row_errors(r32, r64)
    for sub, rows in subsets(case).items():
        if rows is not None and index is not None:
            rows = rows[index]
        E_dev, E_32 = _emax(e_dev, rows), _emax(e_32, rows)
        limit = min(CAP, max(floors[(tensor, sub)], REL * E_32))
        if not E_dev <= limit:
            e = e_dev if rows is None else torch.where(rows, e_dev, torch.zeros_like(e_dev))
            worst = torch.argsort(e, descending=True)[:5]
            ids = worst if index is None else torch.nonzero(index).reshape(-1)[worst]
            print("%s %s %s%s: E_dev %.3e > limit %.3e (E_32 %.3e, floor %.3e); worst rows, errors %s\n%s"
                  % (case.name, what, tensor, sub, E_dev, limit, E_32, floors[(tensor, sub)], ["%.2e" % float(e[w]) for w in worst],
                     describe_rows(case, ids)))
        ops_util.bound("projection/%s/%s/%s/%s%s" % (what, path, case.name, tensor, sub), E_dev, limit)


# ---------------------------------------------------------------------------------------------------- check 1: forward records
def _scene(case, split_sh=False):
    i = case.inp
    sc = dict(means=i["means3D"], opac=i["opac"], colors=i.get("colors"), scales=i.get("scales"), rots=i.get("rots"), cov3D=i.get("cov3D"), mod=case.mod)
    shs = i.get("shs")
    sc.update(dict(shs=shs[:, :1], shs_rest=shs[:, 1:]) if split_sh else dict(shs=shs))
    return sc


def _camera(case):
    return dict(W=case.W, H=case.H, view=case.view, proj=case.proj, campos=case.campos, tanx=case.tanx, tany=case.tany)


def device_preprocess(dev, case):
    """mi355gs_raster_forward_preprocess alone -> (GsRec rows [P,12] float64, radii, clamp bytes): csrc/common.h GsRec is
    x, y, hx, hy | -a/2 log2e, -c/2 log2e, -b log2e, opacity | r, g, b, depth.  The radii are pre-filled with -7: every radius is
    written, 0 for a culled Gaussian."""
    res = frame_abi.run_frame(dev, _scene(case), _camera(case), bg=case.bg, sh=case.deg, radii_fill=-7, preprocess_only=True)
    return res.views.rec.cpu().double(), res.radii.cpu(), res.views.clamped.cpu().to(torch.int64)


def check_forward_records(dev, name):
    """Check 1: the records the projection kernel leaves for the rest of the frame, per Gaussian, against
    oracle/raster_torch.preprocess in float64."""
    case = get_case(name)
    g64, g32 = geometry(case, F64), geometry(case, F32)
    rec, radii, clamp = device_preprocess(dev, case)
    vis = g64["visible"]
    assert torch.equal(radii > 0, vis), "visibility differs in rows %s\n%s" % (
        torch.nonzero((radii > 0) != vis).reshape(-1).tolist(), describe_rows(case, torch.nonzero((radii > 0) != vis).reshape(-1)[:5]))
    if case.family != "block_edges":
        assert int(vis.sum()) >= case.P // 3, (name, int(vis.sum()))
    else:
        assert bool(vis[0]) and bool(vis[-1])
    assert torch.equal(clamp[vis], g64["clamp_bits"][vis]), "SH clamp bits differ in rows %s" % torch.nonzero(vis & (clamp != g64["clamp_bits"])).reshape(-1).tolist()
    off = radii.to(torch.int64) - g64["radius"].to(torch.int64)
    assert int(off.abs().max()) <= 1 and float((off != 0).double().mean()) <= 1e-4, "radii differ in rows %s" % torch.nonzero(off).reshape(-1).tolist()
    A, C, B = rec[:, 4], rec[:, 5], rec[:, 6]
    dev_rows = {"fwd centre": rec[:, 0:2], "fwd conic": torch.stack([A * (-2.0 / LOG2E), B * (-1.0 / LOG2E), C * (-2.0 / LOG2E)], -1),
                "fwd colour": rec[:, 8:11], "fwd depth": rec[:, 11:12]}
    assert torch.equal(rec[vis, 7].float(), case.inp["opac"].reshape(-1)[vis])            # the opacity is passed through
    both = vis & g32["visible"]
    r32, r64 = forward_rows(g32), forward_rows(g64)
    for k in dev_rows:
        judge_rows(case, "records", k, dev_rows[k][both], r32[k][both], r64[k][both], index=both, path="abi")
    return case


# ---------------------------------------------------------------------------------------------------- check 2: gradients per row
def device_mode(case):
    """How the device runs a case whose gradients are judged row by row: the case's dL/dscale convention, and two settings that
    keep csrc/composite.hip's own rounding out of a comparison that is about the per-Gaussian kernels.
      * The backward's units at their longest (mi355gs_tune_min_units(1): 512 instances, every tile list of these cases in one
        piece, as the oracle walks it).  A unit that is not the deepest of its tile resumes from (final colour - colour in front
        of it), a difference of order-1 numbers that stands for a quantity of order T, the transmittance at the unit's boundary:
        its rounding enters dL/dalpha as eps / T.  On the frustum family (100 - 150 instances per tile, T ~ 1e-2 at the first
        64-instance boundary) that alone put the worst rows of every alpha-borne gradient at 1e-4 ... 2e-4, 10 - 40 x the float32
        oracle's 1e-5, while dL/dcolour stood at the oracle's 3e-6; with whole-list units the device stands at 1e-5 as well
        (emulated kernels; the MI355X agrees).  The unit cut itself is tile_length_cases's subject, per tensor.
      * The deterministic backward: the order of the float atomics differs between any two runs on the GPU, which moved the
        worst row of a tensor by tens of per cent from run to run (blob/translation/sh1, grad scales: under and over its limit in
        two runs of the same build) — a maximum over rows judged against a limit has to be the same number every time."""
    return frame_abi.knobs(min_units=1, det=True, scale_grad=int(case.exact))


def run_operator(dev, case):
    """the case through the drop-in GaussianRasterizer"""
    from instantsplat_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    dev = torch.device(dev)
    lv, m2d = _leaves(case, F32, dev)
    st = settings(case, GaussianRasterizationSettings, F32, dev)
    with device_mode(case):
        color, radii = GaussianRasterizer(st)(means3D=lv["means3D"], means2D=m2d, opacities=lv["opac"], **_raster_kwargs(lv))
        (color * case.wgt.to(dev)).sum().backward()
    return _collect(lv, m2d, color, radii)


def run_split_abi(dev, case):
    """the case through the raw C ABI with split SH storage: shs = the DC coefficient [P,1,3], shs_rest = the other 15"""
    with device_mode(case):
        res = frame_abi.run_frame(dev, _scene(case, split_sh=True), _camera(case), bg=case.bg, sh=case.deg, dL=case.wgt)
    d, P = res.grads, case.P
    grads = dict(means3D=d["means3D"], means2D=d["means2D"], opac=d["opac"].reshape(P, 1), shs=torch.cat([d["shs"], d["shs_rest"]], 1), scales=d["scales"], rots=d["rots"])
    return dict(color=res.image.cpu(), radii=res.radii.cpu(), grads={k: v.cpu() for k, v in grads.items()})


def check_gradient_rows(dev, name, path="operator"):
    """Check 2: every gradient tensor of the case, row by row, against the float64 C oracle."""
    case = get_case(name)
    o32, o64 = oracle(name, False), oracle(name, True)
    out = run_operator(dev, case) if path == "operator" else run_split_abi(dev, case)
    g = geometry(case)
    assert torch.equal(out["radii"] > 0, g["visible"])
    assert set(out["grads"]) == set(o64["grads"]), (sorted(out["grads"]), sorted(o64["grads"]))
    check_case_counts(name)
    for k, g64 in o64["grads"].items():
        gd = out["grads"][k]
        assert gd.shape == g64.shape and bool(torch.isfinite(gd).all()), (name, k)
        zero = (g64.reshape(case.P, -1) == 0).all(dim=1)
        wrong = zero & (gd.reshape(case.P, -1) != 0).any(dim=1)
        assert not bool(wrong.any()), "%s grad %s: rows the float64 oracle gives no gradient are not zero\n%s" % (
            name, k, describe_rows(case, torch.nonzero(wrong).reshape(-1)[:5]))
        judge_rows(case, "gradients", "grad " + k, gd, o32["grads"][k], g64, path=path)
    if "shs" in out["grads"]:
        # a clamped channel gets no gradient in any of its coefficients; its share of the view-direction term is then missing
        # from dL/dmeans3D, which the row comparison above sees
        masked = g["visible"][:, None] & g["clamped"]
        gsh = out["grads"]["shs"]
        assert float((gsh.abs().amax(dim=1) * masked).max()) == 0.0, "a clamped channel received a gradient"
        live = g["visible"][:, None] & ~g["clamped"] & (o64["grads"]["shs"][:, 0] != 0)
        assert bool((gsh[:, 0][live] != 0).all())
    return out


def check_case_counts(name):
    """What a case claims to contain, asserted from the float64 oracle; -> the counts listed in this file's header."""
    case = get_case(name)
    g, o64 = geometry(case), oracle(name, True)
    vis = g["visible"]
    moved = (o64["grads"]["means3D"] != 0).any(dim=1)
    res = dict(P=case.P, visible=int(vis.sum()), moved=int(moved.sum()))
    cx, cy = g["clamp_x"] & vis & moved, g["clamp_y"] & vis & moved
    res["clamped"] = [int((cx & ~cy).sum()), int((cy & ~cx).sum()), int((cx & cy).sum())]
    res["sh_clamped"] = int((vis & (g["clamp_bits"] > 0)).sum())
    if case.family == "frustum":
        assert sum(res["clamped"]) >= 100 and min(res["clamped"]) >= 20, res
        for j, kind in enumerate(FRUSTUM_KINDS):   # each kind was placed on purpose: a third of the rows each
            placed = case.kind == j
            assert int(((cx | cy) & placed).sum()) >= 20, (kind, res)
        assert int((vis & ~g["clamp_x"] & ~g["clamp_y"] & moved).sum()) >= 20, res    # ... and both sides of the 1.3 x limit
    if case.family == "sh_clamp":
        per = [int((vis & (g["clamp_bits"] == b)).sum()) for b in range(8)]
        res["patterns"] = per
        assert min(per) >= 10, per
        assert float(g["raw_rgb"][g["front"]].abs().min()) >= 1e-3
    if case.family == "block_edges":
        assert bool(vis[0]) and bool(vis[-1]) and bool(moved[0]) and bool(moved[-1])
    return res


# ---------------------------------------------------------------------------------------------------- check 3: the posed node
def posed_state(seed=3, P=300, W=64, H=48, deg=2):
    """Raw parameters, a pose and the generic view: x_cam = R_v (R_p xyz + t_p) + t_v lands in the frustum of a blob scene.
    The Gaussians are nearly isotropic (log-scales spread by 0.15, quaternion norms 0.9 ... 1.1) on purpose: the posed kernel
    rounds the camera-frame mean differently from pose_activations, and through the inverse of an ill-conditioned 2-D covariance
    that last bit reaches dL/dscaling and dL/drot multiplied by the condition number — with syn_blob's spread of 0.6 (axis
    ratios up to 10) the two float32 paths, and the float32 oracle, each stand 1e-4 ... 6e-4 from float64 in their worst row,
    above the 1e-4 the two paths are held to here.  The un-normalised, anisotropic Gaussians are the `blob` family's."""
    cam, tanx, tany = pinhole(W, H)
    d = _blob(P, W, H, seed, 0.03, 0.9, 1.1, log_spread=0.15)
    Rv, tv = CAMERAS["generic"]
    g = torch.Generator().manual_seed(500 + seed)
    pose = torch.cat([torch.randn(4, generator=g, dtype=F64) * 1.3, 0.5 * torch.randn(3, generator=g, dtype=F64)]).float()
    M = pose_ref.get_camera_from_tensor(pose.double())
    Rp, tp = M[:3, :3], M[:3, 3]
    xyz = to_world(to_world(d["means"], Rv, tv), Rp, tp).float()
    view, proj, campos = camera_setup(Rv, tv, cam)
    opac = d["opac"].clamp(1e-4, 1 - 1e-4)
    raw = dict(xyz=xyz, rot=d["rots"].float(), scaling=torch.log(d["scales"]).float(), opl=torch.log(opac / (1 - opac)).float(),
               f_dc=d["shs"][:, :1].float().contiguous(), f_rest=d["shs"][:, 1:].float().contiguous(), pose=pose)
    # dL/dpixel smooth and of one sign (as ops_util.check_split_sh_equals_concatenated): the two device paths are compared with
    # each other at 1e-4 per row and the pose sums at 1e-6 S_k, which a seeded random dL/dpixel does not allow — a row's terms then
    # cancel, and every float32 evaluation (the float32 oracle included) stands 2e-4 ... 5e-4 from float64 in its worst row
    wgt = torch.linspace(0.2, 1.0, 3 * H * W).reshape(3, H, W)
    case = SimpleNamespace(name="posed/generic", family="posed", camera="generic", P=P, W=W, H=H, deg=deg, mod=1.0, exact=0, tanx=tanx, tany=tany,
                           view=view.float(), proj=proj.float(), campos=campos.float(), bg=torch.tensor(BG), wgt=wgt)
    return case, raw


def posed_oracle(case, raw, dtype):
    """raw-parameter gradients through the reference's glue (oracle/pose_ref.forward) and the C oracle in `dtype`"""
    t = {k: v.clone().to(dtype).requires_grad_(True) for k, v in raw.items()}
    means, rots, scales, opac = pose_ref.forward(t["xyz"], t["rot"], t["scaling"], t["opl"], t["pose"])
    m2d = torch.zeros(case.P, 3, dtype=dtype, requires_grad=True)
    color, radii = gs_ref.rasterize(means, m2d, opac, settings(case, rt.RasterSettings, dtype), shs=torch.cat([t["f_dc"], t["f_rest"]], 1),
                                    scales=scales, rotations=rots)
    (color * case.wgt.to(dtype)).sum().backward()
    return {k: v.grad.detach() for k, v in t.items()}, radii


def check_posed_under_view(dev):
    """Check 3: render_posed (the projection kernels' POSED instantiation) with a pose and the generic settings.viewmatrix gives,
    per row, the raw-parameter gradients of pose_activations followed by the unposed operator with the same settings.  Both sides
    are device float32: each may stand 2.5 E_32 from float64 by this file's criterion (E_32: the float32 oracle's row error on
    this scene), so their difference is held to min(CAP, max(FLOOR, 2 x 2.5 E_32)) with pose_adam_util's (FLOOR, CAP) for
    "pose_grad"; the seven pose components of the node go through judge_components ("posed_sum") against the float64 sum of the
    per-Gaussian terms.  MI355X: rows 8e-6 (f_dc, opl) ... 5.8e-5 (scaling), pose components <= 3.0e-7 S_k; emulated: the two
    paths are bit-identical, pose components <= 3.0e-7 S_k."""
    from instantsplat_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from instantsplat_amd.fused import pose_activations, render_posed
    dev = torch.device(dev)
    case, raw = posed_state()
    st = settings(case, GaussianRasterizationSettings, F32, dev)
    res = {}
    for which in ("posed", "unposed"):
        t = {k: v.clone().to(dev).requires_grad_(True) for k, v in raw.items()}
        m2d = torch.zeros(case.P, 3, device=dev, requires_grad=True)
        with device_mode(case):
            if which == "posed":
                pc = SimpleNamespace(_xyz=t["xyz"], _rotation=t["rot"], _scaling=t["scaling"], _opacity=t["opl"], _features_dc=t["f_dc"], _features_rest=t["f_rest"])
                color, radii = render_posed(pc, t["pose"], m2d, st)
            else:
                means, rots, scales, opac = pose_activations(t["xyz"], t["rot"], t["scaling"], t["opl"], t["pose"])
                color, radii = GaussianRasterizer(st)(means3D=means, means2D=m2d, opacities=opac, shs=t["f_dc"], shs_rest=t["f_rest"], scales=scales, rotations=rots)
            (color * case.wgt.to(dev)).sum().backward()
        res[which] = ({k: v.grad.detach().cpu() for k, v in t.items()}, radii.cpu(), color.detach().cpu())
    o64, radii64 = posed_oracle(case, raw, F64)
    o32, _ = posed_oracle(case, raw, F32)
    assert torch.equal(res["posed"][1], res["unposed"][1]) and torch.equal(res["posed"][1] > 0, radii64 > 0)
    assert int((radii64 > 0).sum()) >= case.P // 3
    ops_util.bound("projection/posed/image", (res["posed"][2] - res["unposed"][2]).abs().max(), 1e-5)   # the limit ops_util holds render()'s glues to
    floor, cap = LIMITS["pose_grad"]
    for k in ("xyz", "rot", "scaling", "opl", "f_dc", "f_rest"):
        a, b = res["posed"][0][k], res["unposed"][0][k]
        zero = (o64[k].reshape(case.P, -1) == 0).all(dim=1)
        for side in (a, b):
            assert not bool((zero & (side.reshape(case.P, -1) != 0).any(dim=1)).any()), k
        e_pp, e_32 = _emax(row_errors(a, b.double())), _emax(row_errors(o32[k], o64[k]))
        ops_util.bound("projection/posed/posed vs unposed/grad " + k, e_pp, min(cap, max(floor, 2.0 * REL * e_32)))
        for side, g in (("posed", a), ("unposed", b)):      # ... and each of them by the criterion itself
            ops_util.bound("projection/posed/%s/grad %s" % (side, k), _emax(row_errors(g, o64[k])), min(CAP, max(floor, REL * e_32)))
    pose64 = raw["pose"].double()
    gm, gr = pose_ref.camera_frame_grads(pose64, o64["xyz"], o64["rot"])
    c = pose_ref.pose_terms(raw["xyz"].double(), raw["rot"].double(), pose64, gm, gr)
    S = c.abs().sum(0)
    assert torch.allclose(c.sum(0), o64["pose"], rtol=1e-9, atol=1e-12 * float(S.max()))
    judge_components("posed_sum", "projection/posed/d_pose", res["posed"][0]["pose"], o32["pose"], o64["pose"], S)


# ---------------------------------------------------------------------------------------------------- check 4: mark_visible
def check_mark_visible(dev, camera, n=300):
    """Check 4: k_mark_visible under `camera` against float64 on points at least 1e-3 away from the z = 0.2 plane of the camera
    frame (a fifth of them 2e-3 from it, on either side; a fifth behind the camera), and on no point at all."""
    from instantsplat_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    dev = torch.device(dev)
    cam, tanx, tany = pinhole(64, 48)
    R, t = CAMERAS[camera]
    view, proj, campos = camera_setup(R, t, cam)
    g = torch.Generator().manual_seed(77)
    z = 0.3 + 6.0 * torch.rand(n, generator=g, dtype=F64)
    z[::5] = 0.2 + torch.where(torch.rand(n, generator=g)[::5] < 0.5, -2e-3, 2e-3).double()
    z[1::5] = -4.0 * torch.rand(n, generator=g, dtype=F64)[1::5] - 0.01
    pts_cam = torch.stack([3.0 * torch.randn(n, generator=g, dtype=F64), 3.0 * torch.randn(n, generator=g, dtype=F64), z], 1)
    pts = to_world(pts_cam, R, t).float()
    st = GaussianRasterizationSettings(48, 64, tanx, tany, torch.zeros(3, device=dev), 1.0, view.float().to(dev), proj.float().to(dev), 0,
                                       campos.float().to(dev), False, False)
    depth = rt._tp43(pts.double(), view.float().double().reshape(-1))[:, 2]
    assert float((depth - 0.2).abs().min()) >= 1e-3
    want = depth > 0.2
    assert 0.2 * n <= int(want.sum()) <= 0.8 * n
    got = GaussianRasterizer(st).markVisible(pts.to(dev))
    assert got.dtype == torch.bool and torch.equal(got.cpu(), want), torch.nonzero(got.cpu() != want).reshape(-1).tolist()
    none = GaussianRasterizer(st).markVisible(torch.zeros(0, 3, device=dev))
    assert none.shape == (0,) and none.dtype == torch.bool
