"""Checks of the global alignment loop (instantsplat_amd/global_align.py, csrc/align.hip), shared by the emulator and the GPU tier.

References, in the order of trust:
  * tests/golden/align_vectors.npz: the reference's own `PointCloudOptimizer`, `global_alignment_loop` and getters, executed in
    float32 on the CPU (tests/golden/make_golden_align.py) — losses of every iteration, the state after 1, 10 and 50;
  * `restatement` below: the same arithmetic in torch at any precision, differentiated by autograd.  It must itself reproduce the
    reference's recording (check_restatement_equals_reference) before anything is measured against its float64 form.

Every limit is 10 x a measured yardstick (ops_util.bound's convention): for gradients the larger of the device's own error
(GS_CALIBRATE=1 on the MI355X) and float32 CPU autograd's error against float64 on the same case; for trajectories the distance of
the reference's float32 run from the float64 restatement at the same iteration.  A dropped edge side or a wrong chain term moves a
gradient by O(1 / E) or more — orders above rounding."""
import os

import numpy as np
import pytest
import torch

from tests import ops_util

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "align_vectors.npz")
STATE = ("depth_log", "im_pose", "focal_log", "pp_raw", "pw_pose")
TRAINED = ("depth_log", "im_pose", "focal_log", "pw_pose")
CHECKPOINTS = (1, 10, 50)
LR, NITER = 0.01, 50

# tag -> (V, H, W, edges, switches)
_SYM2 = [(0, 1), (1, 0)]
_SYM3 = [(0, 1), (0, 2), (1, 2), (1, 0), (2, 0), (2, 1)]
ALL_ON = dict(optimize_depth=True, optimize_im_poses=True, optimize_focals=True, optimize_pw_poses=True, norm_pw_scale=True)
CONFIGS = {
    "a": (2, 12, 10, _SYM2, dict(ALL_ON)),
    "b": (3, 24, 20, _SYM3, dict(ALL_ON, optimize_focals=False)),
    "c": (3, 24, 20, [(0, 1), (0, 2)], dict(ALL_ON)),
    "d": (3, 12, 10, _SYM3, dict(ALL_ON, optimize_im_poses=False, norm_pw_scale=False)),
}
SEEDS = {"a": 11, "b": 12, "c": 13, "d": 14}

# ------------------------------------------------------------------------------------------------------------ synthetic scenes
def _rotmat_to_quat(R):
    """scalar-last unit quaternion of a rotation matrix (numpy, float64)"""
    t = np.trace(R)
    d = [R[0, 0], R[1, 1], R[2, 2], t]
    c = int(np.argmax(d))
    if c == 3:
        q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1 + t])
    else:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = 1 - t + 2 * R[i, i], R[j, i] + R[i, j], R[k, i] + R[i, k], R[k, j] - R[j, k]
    return q / np.linalg.norm(q)


def _signed_log1p(x):
    return np.sign(x) * np.log1p(np.abs(x))


def synthetic_problem(V, H, W, edges, seed, *, norm_pw_scale=True, noise=0.01, perturb=0.02):
    """A smooth surface seen from V cameras on an arc (non-trivial rotations), pairwise predictions equal to the truth in the
    pair's frame plus seeded noise, confidences in [1, 4) (some exactly 1: weight 0), and a seeded perturbation of the true state
    as the start.  -> dict of float32 arrays: pred_i, pred_j [E,n,3], conf_i, conf_j [E,n], and the STATE tensors."""
    g = np.random.default_rng(seed)
    n, E = H * W, len(edges)
    focal = 1.2 * max(H, W)
    rows, cols = np.divmod(np.arange(n), W)
    R, T, X, depth = [], [], [], []
    for v in range(V):
        ang = 0.5 * (v - (V - 1) / 2) + 0.1
        ca, sa = np.cos(ang), np.sin(ang)
        tilt = 0.15 * (v + 1)
        ct, st = np.cos(tilt), np.sin(tilt)
        Rv = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]])
        Tv = np.array([-2.5 * sa, 0.2 * v, 2.5 * (1 - ca)]) + 0.3
        d = 2.0 + 0.3 * np.sin(3.0 * cols / W + v) * np.cos(2.0 * rows / H) + 0.1 * cols / W
        c = np.stack([d * (cols - W / 2) / focal, d * (rows - H / 2) / focal, d], axis=1)
        R.append(Rv); T.append(Tv); depth.append(d); X.append(c @ Rv.T + Tv)
    delta = g.normal(0, 0.2, E)
    if norm_pw_scale:
        delta -= delta.mean()    # the geometric mean of the pair scales is pinned to base_scale
    sigma = 0.5 * np.exp(delta)
    pred_i, pred_j, pw = np.zeros((E, n, 3)), np.zeros((E, n, 3)), np.zeros((E, 8))
    for e, (i, j) in enumerate(edges):
        pred_i[e] = ((X[i] - T[i]) @ R[i]) / sigma[e]     # camera i's frame, at the pair's scale
        pred_j[e] = ((X[j] - T[i]) @ R[i]) / sigma[e]
        pw[e, :4], pw[e, 4:7], pw[e, 7] = _rotmat_to_quat(R[i]), _signed_log1p(T[i] / sigma[e]), np.log(sigma[e] / 0.5) if norm_pw_scale else np.log(sigma[e])
    pred_i += g.normal(0, noise, pred_i.shape)
    pred_j += g.normal(0, noise, pred_j.shape)
    pred_i, pred_j = np.round(pred_i * 4096) / 4096, np.round(pred_j * 4096) / 4096   # (fewer mantissa bits: a smaller fixture)
    conf_i, conf_j = 1 + g.integers(0, 192, (E, n)) / 64, 1 + g.integers(0, 192, (E, n)) / 64
    conf_i[g.random((E, n)) < 0.05] = 1.0
    conf_j[g.random((E, n)) < 0.05] = 1.0
    im_pose = np.stack([np.concatenate([_rotmat_to_quat(R[v]) * (1.0 + 0.2 * v), _signed_log1p(T[v])]) for v in range(V)])
    out = dict(pred_i=pred_i, pred_j=pred_j, conf_i=conf_i, conf_j=conf_j,
               depth_log=np.log(np.stack(depth)) + perturb * g.normal(0, 1, (V, n)),
               im_pose=im_pose + perturb * g.normal(0, 1, (V, 7)),
               focal_log=20 * np.log(focal) + 10 * perturb * g.normal(0, 1, V),
               pp_raw=0.05 * g.normal(0, 1, (V, 2)),
               pw_pose=pw + perturb * g.normal(0, 1, (E, 8)))
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------ the restatement
def _poses(raw):
    q = raw[:, :4] / raw[:, :4].norm(dim=1, keepdim=True)
    x, y, z, w = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
    t = raw[:, 4:7]
    return R, torch.sign(t) * torch.expm1(t.abs())


def world_points(H, W, s):
    """X_v[p] = R_v (d u / f, d v / f, d) + T_v, [V,n,3]"""
    dt, dev = s["depth_log"].dtype, s["depth_log"].device
    rows = torch.arange(H, dtype=dt, device=dev).repeat_interleave(W)
    cols = torch.arange(W, dtype=dt, device=dev).repeat(H)
    grid = torch.stack([cols, rows], dim=1)[None]                                   # [1,n,2]
    pp = torch.tensor([W / 2, H / 2], dtype=dt, device=dev) + 10 * s["pp_raw"]      # [V,2]
    focal = (s["focal_log"] / 20).exp()
    d = s["depth_log"].exp()[..., None]
    rel = torch.cat([d * (grid - pp[:, None]) / focal[:, None, None], d], dim=-1)
    R, T = _poses(s["im_pose"])
    return torch.einsum("vij,vnj->vni", R, rel) + T[:, None]


def restatement(edges, H, W, data, s, norm_pw_scale, base_scale=0.5):
    """The loss of optimizer.py:188-201 for equal image shapes; data: pred_i, pred_j, wi, wj (the log confidences)."""
    E, n = len(edges), H * W
    X = world_points(H, W, s)
    R, T = _poses(s["pw_pose"])
    scale = s["pw_pose"][:, 7].exp()
    if norm_pw_scale:
        scale = scale * (np.log(base_scale) - s["pw_pose"][:, 7].mean()).exp()
    M, t = scale[:, None, None] * R, scale[:, None] * T
    ei = torch.tensor([i for i, j in edges], device=X.device)
    ej = torch.tensor([j for i, j in edges], device=X.device)
    ai = torch.einsum("eij,enj->eni", M, data["pred_i"]) + t[:, None]
    aj = torch.einsum("eij,enj->eni", M, data["pred_j"]) + t[:, None]
    li = ((X[ei] - ai).norm(dim=-1) * data["wi"]).sum() / (E * n)
    lj = ((X[ej] - aj).norm(dim=-1) * data["wj"]).sum() / (E * n)
    return li + lj


def as_torch(arrays, dtype, dev="cpu"):
    data = {k: torch.as_tensor(arrays[k]).to(dev, dtype) for k in ("pred_i", "pred_j")}
    data["wi"] = torch.as_tensor(arrays["conf_i"]).to(dev).log().to(dtype)   # the float32 logarithm the aligner forms, widened
    data["wj"] = torch.as_tensor(arrays["conf_j"]).to(dev).log().to(dtype)
    state = {k: torch.as_tensor(arrays[k]).to(dev, dtype).clone() for k in STATE}
    return data, state


def _trainable(sw):
    return [k for k, on in (("depth_log", sw["optimize_depth"]), ("im_pose", sw["optimize_im_poses"]), ("focal_log", sw["optimize_focals"]),
                            ("pw_pose", sw["optimize_pw_poses"])) if on]


def lr_at(k, niter, lr, schedule, lr_min):
    t = k / niter
    return lr_min + (lr - lr_min) * (1 + np.cos(t * np.pi)) / 2 if schedule == "cosine" else lr + (lr_min - lr) * t


def restatement_grads(edges, H, W, arrays, sw, dtype):
    data, s = as_torch(arrays, dtype)
    for k in TRAINED:
        s[k].requires_grad_(True)
    loss = restatement(edges, H, W, data, s, sw["norm_pw_scale"])
    loss.backward()
    return {"loss": loss.detach(), **{k: s[k].grad for k in TRAINED}}


def restatement_run(edges, H, W, arrays, sw, niter, dtype, lr=LR, schedule="cosine", lr_min=1e-6, checkpoints=CHECKPOINTS, dev="cpu"):
    """global_alignment_loop with torch.optim.Adam on the restatement -> (losses [niter], {iterations done: state})"""
    data, s = as_torch(arrays, dtype, dev)
    params = [s[k].requires_grad_(True) for k in _trainable(sw)]
    opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.9))
    losses, snaps = [], {}
    for k in range(niter):
        for grp in opt.param_groups:
            grp["lr"] = lr_at(k, niter, lr, schedule, lr_min)
        opt.zero_grad()
        loss = restatement(edges, H, W, data, s, sw["norm_pw_scale"])
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        if k + 1 in checkpoints:
            snaps[k + 1] = {name: s[name].detach().clone() for name in STATE}
    return torch.stack(losses), snaps


# ------------------------------------------------------------------------------------------------------------ goldens
_G = None


def golden():
    global _G
    if _G is None:
        _G = dict(np.load(GOLDEN))
    return _G


def golden_case(tag):
    V, H, W, edges, sw = CONFIGS[tag]
    g = golden()
    arrays = {k: g[f"align_{tag}_{k}"] for k in ("pred_i", "pred_j", "conf_i", "conf_j") + STATE}
    return V, H, W, edges, sw, arrays


def golden_state(tag, it):
    return {k: torch.from_numpy(golden()[f"align_{tag}_it{it}_{k}"]) for k in STATE}


# ------------------------------------------------------------------------------------------------------------ device side
def device_problem(dev, edges, H, W, arrays, sw):
    from instantsplat_amd.global_align import AlignProblem, AlignState
    t = {k: torch.from_numpy(np.ascontiguousarray(arrays[k])).to(dev) for k in arrays}
    problem = AlignProblem(edges, t["pred_i"], t["pred_j"], t["conf_i"], t["conf_j"], H, W, **sw)
    return problem, AlignState(problem, *[t[k] for k in STATE])


def rel(a, b):
    return ops_util.rel_l2(a.reshape(-1), b.reshape(-1))


# The device's own error (rel. L2 against float64 autograd), measured with GS_CALIBRATE=1, worst over every case that goes through
# check_gradients: under the emulator depth_log 2.5e-6, im_pose 8.6e-7, focal_log 4.0e-6,
# pw_pose 7.3e-7, loss 3.6e-7; on the MI355X 2.6e-6, 7.9e-7, 4.5e-6, 6.3e-7, 3.6e-7 (the larger of the two is used)
# float32 CPU autograd of the restatement on the golden cases, for comparison (make_golden_align.py prints it): depth_log 3.1e-6,
# im_pose 1.3e-6, focal_log 3.3e-6, pw_pose 1.2e-6, loss 2.6e-7.  The limit of a case is 10 x the larger of the device's number
# here and float32 autograd's own error ON THAT CASE, which check_gradients measures.
GRAD_DEVICE = {"depth_log": 2.6e-6, "im_pose": 8.6e-7, "focal_log": 4.5e-6, "pw_pose": 7.3e-7, "loss": 3.6e-7}


def check_gradients(dev, edges, H, W, arrays, sw, label):
    from instantsplat_amd.global_align import gradients
    ref = restatement_grads(edges, H, W, arrays, sw, torch.float64)
    f32 = restatement_grads(edges, H, W, arrays, sw, torch.float32)
    problem, state = device_problem(dev, edges, H, W, arrays, sw)
    before = {k: getattr(state, k).clone() for k in STATE}
    got = gradients(problem, state)
    for k in STATE:
        assert torch.equal(before[k], getattr(state, k)), f"{label}: the gradient call changed {k}"
    for k in TRAINED + ("loss",):
        assert bool(torch.isfinite(got[k]).all()), f"{label}: {k} gradient is not finite"
        ops_util.bound(f"align grad {k} [{label}]", rel(got[k], ref[k]), 10 * max(GRAD_DEVICE[k], rel(f32[k], ref[k])))
    return got, ref


def edge_shape_cases():
    """(label, V, H, W, edges): where the kernel can go wrong.  csrc/align.hip: a workgroup of the step kernel takes 1024 pixels of
    one image (ALIGN_BLOCK), 4 per thread; the reduce stage adds partial rows in 16 groups; the finish stage has 256 threads."""
    sym = lambda V: [(i, j) for i in range(V) for j in range(V) if i != j]   # noqa: E731
    return [
        ("n=wg-1", 2, 31, 33, _SYM2),              # 1023 pixels: one below a workgroup's 1024
        ("n=wg", 2, 32, 32, _SYM2),                # exactly one workgroup
        ("n=wg+1", 2, 25, 41, _SYM2),              # 1025: a second workgroup with one pixel
        ("n%4!=0", 3, 7, 37, _SYM3),               # 259 pixels: not a multiple of the 4 per thread, a wave with idle lanes
        ("single side", 3, 9, 11, [(0, 1), (0, 2)]),   # images 1 and 2 have one edge side each, and only as j
        ("V=2 one edge", 2, 9, 11, [(0, 1)]),
        ("finish loops", 17, 3, 4, sym(17)),       # 272 edges: the finish stage's 256 threads take a second turn over the edges
        ("reduce loops", 2, 136, 128, _SYM2),      # 17 workgroups per image: the reduce stage's 16 row groups take a second turn
    ]


def check_edge_shape(dev, label):
    _, V, H, W, edges = next(c for c in edge_shape_cases() if c[0] == label)
    arrays = synthetic_problem(V, H, W, edges, 100 + len(label))
    check_gradients(dev, edges, H, W, arrays, ALL_ON, label)


def check_zero_residual(dev):
    """A pixel whose residual is exactly zero contributes 0, not NaN.  The residual must be zero in float32 AND in the float64
    reference (a residual of 1e-8 has a unit-length gradient direction): identity poses, sigma = 1, focal = 1 and depth = 1 at
    the planted pixels make every factor exact in both."""
    V, H, W, edges = 2, 6, 5, _SYM2
    arrays = synthetic_problem(V, H, W, edges, 77, norm_pw_scale=False)
    arrays["im_pose"][:] = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float32)
    arrays["pw_pose"][:] = np.array([0, 0, 0, 1, 0, 0, 0, 0], dtype=np.float32)
    arrays["pp_raw"][:] = 0
    arrays["focal_log"][:] = 0
    sw = dict(ALL_ON, norm_pw_scale=False)
    planted = ((0, "pred_i", "conf_i", 7), (1, "pred_j", "conf_j", 3))   # edge 0 = (0, 1): its i side, edge 1 = (1, 0): its j side — image 0
    for e, pred, conf, p in planted:
        arrays["depth_log"][0, p] = 0
        arrays[pred][e, p] = np.array([p % W - W / 2, p // W - H / 2, 1.0], dtype=np.float32)
        arrays[conf][e, p] = 3.0
    data, s64 = as_torch(arrays, torch.float64)
    X = world_points(H, W, s64)
    for e, pred, conf, p in planted:
        assert torch.equal(X[0, p], data[pred][e, p]), "the planted residual is not zero in the reference"
    got, ref = check_gradients(dev, edges, H, W, arrays, sw, "zero residual")
    assert bool(torch.isfinite(ref["depth_log"]).all())


def trajectory_yardstick(tag):
    """the distance of the reference's float32 recording from the float64 restatement, per checkpoint and tensor, and for the losses"""
    V, H, W, edges, sw, arrays = golden_case(tag)
    losses64, snaps64 = restatement_run(edges, H, W, arrays, sw, NITER, torch.float64)
    g = golden()
    y = {"losses": rel(torch.from_numpy(g[f"align_{tag}_losses"]), losses64)}
    for it in CHECKPOINTS:
        ref = golden_state(tag, it)
        for k in _trainable(sw):
            y[(it, k)] = rel(ref[k], snaps64[it][k])
    return y, losses64, snaps64


# measured: the reference's float32 run against the float64 restatement (trajectory_yardstick; make_golden_align.py prints it),
# rel. L2 per checkpoint and tensor, the worst of the four configurations; and of the 50 losses.
TRAJ_YARDSTICK = {"losses": 2.33e-6,
                  1: {"depth_log": 3.37e-6, "im_pose": 2.10e-8, "focal_log": 3.52e-8, "pw_pose": 1.32e-8},
                  10: {"depth_log": 1.70e-6, "im_pose": 1.39e-7, "focal_log": 8.64e-8, "pw_pose": 7.72e-8},
                  50: {"depth_log": 3.63e-7, "im_pose": 3.06e-7, "focal_log": 1.56e-7, "pw_pose": 2.01e-7}}


def check_trajectory(dev, tag):
    """One 50-iteration run, enqueued in three calls that stop at the checkpoints (the moments and the step count live in the
    state, the schedule rows are the full run's: continuing is the same run)."""
    V, H, W, edges, sw, arrays = golden_case(tag)
    ref_losses = torch.from_numpy(golden()[f"align_{tag}_losses"])
    problem, state = device_problem(dev, edges, H, W, arrays, sw)
    losses = []
    for it in CHECKPOINTS:
        losses.append(_run_segment(problem, state, it - state.step, NITER))
        assert state.step == it
        ref = golden_state(tag, it)
        for k in _trainable(sw):
            ops_util.bound(f"align state {k} after {it} [{tag}]", rel(getattr(state, k).cpu(), ref[k]), 10 * TRAJ_YARDSTICK[it][k])
    losses = torch.cat(losses).cpu()
    ops_util.bound(f"align losses [{tag}]", rel(losses, ref_losses), 10 * TRAJ_YARDSTICK["losses"])
    assert float(ref_losses[-1]) < float(ref_losses[0]) and float(losses[-1]) < float(losses[0]), "the loss does not decrease"


def _run_segment(problem, state, count, niter):
    """the next `count` iterations of an `niter`-iteration run -> their losses"""
    from instantsplat_amd import _lib
    from instantsplat_amd import global_align as ga
    dev = problem.device
    table = torch.from_numpy(ga.step_table(0, niter, LR, "cosine", 1e-6)[state.step:state.step + count].copy()).to(dev)
    losses = torch.empty(count, dtype=torch.float32, device=dev)
    moments = [_lib.ptr(t) for k in TRAINED for t in state.moments[k]]
    with _lib.on_device(dev):
        _lib.check(_lib.lib().mi355gs_align_run(problem._handle, _lib.stream_ptr(dev), count, _lib.ptr(table), *state._state_ptrs(), *moments,
                                                _lib.ptr(losses)), "align_run")
    out = losses.cpu()   # (waits for the run: `table` may go)
    state.step += count
    return out


def check_restatement_equals_reference(tag):
    """CPU only: the float32 restatement reproduces the reference's iteration-0 loss and its state after one iteration"""
    V, H, W, edges, sw, arrays = golden_case(tag)
    g = golden()
    losses32, snaps32 = restatement_run(edges, H, W, arrays, sw, 1, torch.float32, checkpoints=(1,))
    # float32 sums of a few thousand terms in another order: a few ulp
    assert abs(float(losses32[0]) - float(g[f"align_{tag}_losses"][0])) <= 4e-6 * abs(float(g[f"align_{tag}_losses"][0]))
    ref = golden_state(tag, 1)
    for k in STATE:
        # one Adam step moves every trained element by lr (the first step's m / sqrt(v) is +-1 wherever the gradient is not
        # tiny): a wrong sign or a missing term is an error of 2 lr = 2e-2 absolute
        assert float((snaps32[1][k] - ref[k]).abs().max()) <= 2e-5, (tag, k)
    for k in STATE:
        if k not in _trainable(sw):
            assert torch.equal(ref[k], torch.from_numpy(arrays[k])), (tag, k)


def check_switches(dev):
    from instantsplat_amd.global_align import global_alignment
    V, H, W, edges, sw, arrays = golden_case("a")
    results = {}
    for name, switches in (("all", sw), ("no focal", dict(sw, optimize_focals=False)), ("no poses", dict(sw, optimize_im_poses=False, norm_pw_scale=False)),
                           ("no depth", dict(sw, optimize_depth=False)), ("no pw", dict(sw, optimize_pw_poses=False)),
                           ("no norm", dict(sw, norm_pw_scale=False))):
        problem, state = device_problem(dev, edges, H, W, arrays, switches)
        start = {k: getattr(state, k).clone() for k in STATE}
        last, losses = global_alignment(problem, state, niter=5, lr=LR)
        assert bool(torch.isfinite(losses).all()) and last == float(losses[-1])
        for k in STATE:
            frozen = k not in _trainable(switches)
            assert torch.equal(start[k], getattr(state, k)) == frozen, (name, k, "frozen" if frozen else "trained")
        l64, s64 = restatement_run(edges, H, W, arrays, switches, 5, torch.float64, checkpoints=(5,))
        ops_util.bound(f"align losses [switch {name}]", rel(losses.cpu(), l64), 10 * TRAJ_YARDSTICK["losses"])
        for k in _trainable(switches):
            ops_util.bound(f"align state {k} after 5 [switch {name}]", rel(getattr(state, k).cpu(), s64[5][k]), 10 * TRAJ_YARDSTICK[10][k])
        results[name] = losses.cpu()
    assert not torch.equal(results["all"], results["no norm"]), "norm_pw_scale changes nothing"
    # the linear schedule
    problem, state = device_problem(dev, edges, H, W, arrays, sw)
    last, losses = global_alignment(problem, state, niter=5, lr=LR, schedule="linear")
    l64, s64 = restatement_run(edges, H, W, arrays, sw, 5, torch.float64, schedule="linear", checkpoints=(5,))
    ops_util.bound("align losses [linear]", rel(losses.cpu(), l64), 10 * TRAJ_YARDSTICK["losses"])
    for k in _trainable(sw):
        ops_util.bound(f"align state {k} after 5 [linear]", rel(getattr(state, k).cpu(), s64[5][k]), 10 * TRAJ_YARDSTICK[10][k])
    assert not torch.equal(losses.cpu(), results["all"])
    with pytest.raises(ValueError, match="schedule"):
        global_alignment(problem, state, niter=2, schedule="step")
    # niter = 0
    problem, state = device_problem(dev, edges, H, W, arrays, sw)
    start = {k: getattr(state, k).clone() for k in STATE}
    last, losses = global_alignment(problem, state, niter=0)
    assert last == float("inf") and losses.numel() == 0 and state.step == 0
    assert all(torch.equal(start[k], getattr(state, k)) for k in STATE)


def check_determinism(dev):
    from instantsplat_amd.global_align import global_alignment
    V, H, W, edges, sw, arrays = golden_case("b")
    sw = dict(ALL_ON)
    runs = []
    for _ in range(2):
        problem, state = device_problem(dev, edges, H, W, arrays, sw)
        _, losses = global_alignment(problem, state, niter=8, lr=LR)
        runs.append([losses.clone()] + [getattr(state, k).clone() for k in STATE] + [m for k in TRAINED for m in state.moments[k]])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def check_getters(dev):
    g = golden()
    for tag in CONFIGS:
        V, H, W, edges, sw, arrays = golden_case(tag)
        final = {k: g[f"align_{tag}_it{NITER}_{k}"] for k in STATE}
        problem, state = device_problem(dev, edges, H, W, {**arrays, **final}, sw)
        for name, got in (("im_poses", state.im_poses()), ("focals", state.focals()), ("intrinsics", state.intrinsics()), ("pts3d", state.pts3d()),
                          ("depthmaps", state.depthmaps())):
            want = torch.from_numpy(g[f"align_{tag}_get_{name}"])
            assert tuple(got.shape) == tuple(want.shape), (tag, name, got.shape, want.shape)
            assert rel(got.cpu(), want) <= 1e-6, (tag, name, rel(got.cpu(), want))
        assert torch.equal(state.im_conf().cpu(), torch.from_numpy(g[f"align_{tag}_get_im_conf"])), tag


def check_hand_over(dev, tmp):
    """to_init_stage_inputs() into init_from_pointmaps on configuration (b)"""
    from instantsplat_amd.init_stage import init_from_pointmaps
    V, H, W, edges, sw, arrays = golden_case("b")
    final = {k: golden()[f"align_b_it{NITER}_{k}"] for k in STATE}
    problem, state = device_problem(dev, edges, H, W, {**arrays, **final}, sw)
    kw = state.to_init_stage_inputs()
    assert set(kw) == {"pointmaps", "depthmaps", "confidences", "intrinsics", "w2c", "focals"}
    eye = torch.eye(4, device=dev).expand(V, 4, 4)
    assert float((kw["w2c"] @ state.im_poses() - eye).abs().max()) < 1e-5
    images = torch.rand(V, H, W, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    out = init_from_pointmaps(tmp, V, images, org_size=(4 * W, 4 * H), depth_threshold=0.01, conf_aware_ranking=True, **kw)
    M = out["pts_num"]["co_mask_dsp"]
    assert 1 <= M <= V * H * W and out["points"].shape == (M, 3)
    assert state.to_init_stage_inputs(log_depth=True)["depthmaps"].shape == (V, H, W)


def check_entry_points_reject_bad_arguments(dev):
    import ctypes
    from instantsplat_amd import _lib
    L = _lib.lib()
    ok_flags = 31

    def edges_c(e):
        return (ctypes.c_int32 * (2 * len(e)))(*[x for p in e for x in p])
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    good = dict(V=2, H=4, W=5, edges=[(0, 1)], flags=ok_flags, base=0.5)

    def create(**kw):
        a = dict(good, **kw)
        return L.mi355gs_align_create(_lib.ptr(ws) if a.get("ws", True) else None, a["V"], a["H"], a["W"],
                                      edges_c(a["edges"]) if a["edges"] is not None else None, len(a["edges"] or [(0, 1)]), a["flags"], a["base"])
    h = create()
    assert h
    L.mi355gs_align_destroy(h)
    assert L.mi355gs_align_workspace_bytes(2, 4, 5, 1, ok_flags) > 0
    for bad in (dict(ws=False), dict(edges=None), dict(V=0), dict(H=0), dict(W=-1), dict(edges=[(0, 0)]), dict(edges=[(0, 2)]), dict(edges=[(-1, 1)]),
                dict(V=3), dict(V=257), dict(flags=32), dict(flags=-1), dict(base=0.0)):
        assert not create(**bad), bad
    # sizes: workspace_bytes answers 0 where create refuses
    for V, H, W, E in ((0, 4, 5, 1), (2, 0, 5, 1), (2, 4, 0, 1), (2, 4, 5, 0), (257, 4, 5, 1), (2, 4, 5, 65536), (2, 1 << 15, 1 << 15, 2),
                       (2, 1 << 16, 1 << 15, 1)):
        assert L.mi355gs_align_workspace_bytes(V, H, W, E, ok_flags) == 0, (V, H, W, E)
    assert L.mi355gs_align_workspace_bytes(2, 4, 5, 65535, ok_flags) > 0
    many = [(0, 1)] * 65536
    assert not L.mi355gs_align_create(_lib.ptr(ws), 2, 1, 1, edges_c(many), len(many), ok_flags, 0.5)
    # null pointers and sizes of the calls
    h = create()
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    p, st = _lib.ptr(f), _lib.stream_ptr(dev)
    assert L.mi355gs_align_pack(None, st, p, p, p, p) == -1
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert L.mi355gs_align_pack(h, st, *args) == -1
    for k in range(10):
        args = [p] * 10
        args[k] = None
        assert L.mi355gs_align_grad(h, st, *args) == -1
    assert L.mi355gs_align_grad(None, st, *([p] * 10)) == -1
    for k in range(15):
        args = [p] * 15
        args[k] = None
        assert L.mi355gs_align_run(h, st, 1, *args) == -1, k
    assert L.mi355gs_align_run(h, st, -1, *([p] * 15)) == -1
    assert L.mi355gs_align_run(None, st, 1, *([p] * 15)) == -1
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert L.mi355gs_align_points(h, st, *args) == -1
    assert L.mi355gs_align_points(None, st, *([p] * 7)) == -1
    L.mi355gs_align_destroy(h)
    L.mi355gs_align_destroy(None)


class _Param:
    def __init__(self, t, requires_grad=True):
        self._t, self.requires_grad = t, requires_grad

    def detach(self):
        return self._t

    def __getattr__(self, name):
        return getattr(self._t, name)


def fake_scene(dev, tag="a", **over):
    """a duck-typed stand-in for the reference's PointCloudOptimizer with exactly the attributes from_reference_scene reads"""
    import types
    V, H, W, edges, sw, arrays = golden_case(tag)
    t = {k: torch.from_numpy(arrays[k]).to(dev) for k in arrays}
    names = [f"{i}_{j}" for i, j in edges]
    sc = types.SimpleNamespace(
        edges=edges, imshapes=[(H, W)] * V, _stacked_pred_i=t["pred_i"], _stacked_pred_j=t["pred_j"],
        conf_i={k: t["conf_i"][e].view(H, W) for e, k in enumerate(names)}, conf_j={k: t["conf_j"][e].view(H, W) for e, k in enumerate(names)},
        im_depthmaps=_Param(t["depth_log"], sw["optimize_depth"]), im_poses=_Param(t["im_pose"], sw["optimize_im_poses"]),
        im_focals=_Param(t["focal_log"].view(V, 1), sw["optimize_focals"]), im_pp=_Param(t["pp_raw"], False),
        pw_poses=_Param(t["pw_pose"], sw["optimize_pw_poses"]), pw_adaptors=_Param(torch.zeros(len(edges), 2, device=dev), False),
        norm_pw_scale=sw["norm_pw_scale"], base_scale=0.5, focal_break=20, pw_break=20,
        dist=lambda a, b, weight: (a - b).norm(dim=-1) * weight, conf_trf=lambda x: x.log())
    for k, v in over.items():
        setattr(sc, k, v)
    return sc


def check_from_reference_scene(dev):
    from instantsplat_amd.global_align import from_reference_scene, global_alignment
    V, H, W, edges, sw, arrays = golden_case("b")
    problem, state = from_reference_scene(fake_scene(dev, "b"))
    assert (problem.V, problem.H, problem.W, problem.E) == (V, H, W, len(edges)) and not problem.flags & 4 and problem.flags & 16
    last, losses = global_alignment(problem, state, niter=5, lr=LR)
    l64, _ = restatement_run(edges, H, W, arrays, sw, 5, torch.float64, checkpoints=())
    ops_util.bound("align losses [from_reference_scene b]", rel(losses.cpu(), l64), 10 * TRAJ_YARDSTICK["losses"])
    E = len(CONFIGS["a"][3])
    for over, word in ((dict(pw_adaptors=_Param(torch.zeros(E, 2, device=dev), True)), "allow_pw_adaptors"),
                       (dict(pw_adaptors=_Param(torch.full((E, 2), 0.1, device=dev), False)), "pw_adaptors"),
                       (dict(im_pp=_Param(torch.zeros(2, 2, device=dev), True)), "optimize_pp"),
                       (dict(dist=lambda a, b, weight: (a - b).square().sum(dim=-1) * weight), "dist"),
                       (dict(conf_trf=lambda x: x.sqrt()), "conf"),
                       (dict(focal_break=10), "focal_break"),
                       (dict(imshapes=[(12, 10), (10, 12)]), "different shapes")):
        with pytest.raises(ValueError, match=word):
            from_reference_scene(fake_scene(dev, "a", **over))


def check_python_rejects_bad_arguments(dev):
    from instantsplat_amd.global_align import AlignProblem, AlignState, global_alignment
    V, H, W, edges, sw, arrays = golden_case("a")
    t = {k: torch.from_numpy(arrays[k]).to(dev) for k in arrays}
    inputs = [t[k] for k in ("pred_i", "pred_j", "conf_i", "conf_j")]
    for bad_edges in ([(0, 0), (1, 0)], [(0, 2), (2, 0)]):     # an edge from an image to itself; image 1 uncovered
        with pytest.raises(ValueError, match="refused"):
            AlignProblem(bad_edges, *inputs, H, W)
    with pytest.raises(ValueError, match="different shapes"):
        AlignProblem(edges, *inputs, H, W + 1)
    with pytest.raises(ValueError, match="float32"):
        AlignProblem(edges, inputs[0].double(), *inputs[1:], H, W)
    problem = AlignProblem(edges, *inputs, H, W)
    with pytest.raises(ValueError, match="im_pose"):
        AlignState(problem, t["depth_log"], t["im_pose"][:, :6].contiguous(), t["focal_log"], t["pp_raw"], t["pw_pose"])
    state = AlignState(problem, *[t[k] for k in STATE])
    other = AlignProblem(edges, *inputs, H, W)
    with pytest.raises(ValueError, match="another problem"):
        global_alignment(other, state, niter=1)


MODERATE = (3, 72, 128, _SYM3)   # 3 x 128 x 72: nine workgroups per image


def check_moderate_shape(dev):
    """GPU only: gradients as in check_gradients, and 10 iterations against the float64 restatement"""
    from instantsplat_amd.global_align import global_alignment
    V, H, W, edges = MODERATE
    arrays = synthetic_problem(V, H, W, edges, 31)
    check_gradients(dev, edges, H, W, arrays, ALL_ON, "3x128x72")
    problem, state = device_problem(dev, edges, H, W, arrays, ALL_ON)
    last, losses = global_alignment(problem, state, niter=10, lr=LR)
    l64, s64 = restatement_run(edges, H, W, arrays, ALL_ON, 10, torch.float64, checkpoints=(10,))
    ops_util.bound("align losses [3x128x72]", rel(losses.cpu(), l64), 10 * TRAJ_YARDSTICK["losses"])
    for k in TRAINED:
        ops_util.bound(f"align state {k} after 10 [3x128x72]", rel(getattr(state, k).cpu(), s64[10][k]), 10 * TRAJ_YARDSTICK[10][k])
