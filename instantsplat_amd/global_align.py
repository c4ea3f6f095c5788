"""The global alignment loop — reference dust3r/cloud_opt/base_opt.py:326-366 (`global_alignment_loop`) over
dust3r/cloud_opt/optimizer.py:188-201 (`PointCloudOptimizer.forward`): the stage that turns the network's pairwise pointmaps
into one scene.  The reference runs it with 300 iterations for the training views (init_geo.py:48) and with 500 over training
and test views together (init_test_pose.py:59).  Here the whole loop is ONE library call (csrc/align.hip, include/mi355gs.h
mi355gs_align_*): three kernel dispatches per iteration, no host synchronisation, the Adam step of the depth maps applied in the
kernel that forms their gradient.  There is no CPU fallback.

  AlignProblem            the fixed side: edges, the packed pairwise pointmaps and confidences, the switches
  AlignState              the five parameter tensors, the Adam moments, the step count; the reference's getters
  from_reference_scene    reads a duck-typed reference `PointCloudOptimizer` (after `init_minimum_spanning_tree`) -> (problem, state)
  global_alignment        the loop -> (last loss, losses[niter])
  init_minimum_spanning_tree   the step in front of the loop (dust3r/cloud_opt/init_im_poses.py:66-221): edge scores, the tree and
                          the walk over it (host decisions), V - 1 chained and E batched similarity registrations, Weiszfeld
                          focals, scale normalisation and the state write-out (csrc/align_init.hip) -> AlignState
  compute_global_alignment     the reference's entry point (base_opt.py:275-287): init="mst" or a caller's state, then the loop
  register_points         the batched weighted similarity registration both stages call (roma's conventions)
  spanning_tree, walk_plan     the host side of the initialisation, without scipy

Out of scope: the network, cv2's RANSAC PnP (`pnp_fn` takes a caller's; the default is a deterministic registration, see
`init_minimum_spanning_tree`), `init_from_known_poses` and the known-poses branch of `init_from_pts3d`,
`ModularPointCloudOptimizer`, `PairViewer`, `clean_pointcloud`, optimised pw_adaptors and principal points (both off in every
InstantSplat script), images of different shapes within one problem."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from .handles import LibraryHandle

MAX_VIEWS = 256
MAX_EDGES = 65535
MAX_ELEMENTS = 2 ** 31 - 1
FOCAL_BREAK = 20.0     # reference optimizer.py:22
PP_BREAK = 10.0        # reference optimizer.py:141-142
OPT_DEPTH, OPT_IM_POSES, OPT_FOCALS, OPT_PW_POSES, NORM_PW_SCALE = 1, 2, 4, 8, 16   # include/mi355gs.h MI355GS_ALIGN_*


def _f32(x, shape, what, dev):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be {list(shape)}, got {list(t.shape)}")
    _lib.require_device(t.contiguous())
    if dev is not None and t.device != dev:
        raise ValueError(f"{what} is on {t.device}, the problem on {dev}")
    return t.detach().contiguous()


class AlignProblem(LibraryHandle):
    """The fixed side of one alignment: V images of H x W, E directed edges (i, j) covering every image (any list: it need not
    be symmetrised, an image may appear only as a j), the pairwise pointmaps pred_i / pred_j [E,H*W,3] (or [E,H,W,3]) and raw
    confidences conf_i / conf_j [E,H*W] >= 1 (the reference's _stacked_pred_i / _j, conf_i / conf_j), and the switches: which
    parameter groups take Adam steps (the reference's requires_grad: optimize_im_poses is off after `preset_pose`, which also
    turns norm_pw_scale off; optimize_focals is off under --focal_avg / known_focal) and norm_pw_scale."""
    prefix = "align"
    _handle = property(lambda self: self.handle)   # (the name the tests and tools know it by)

    def __init__(self, edges, pred_i, pred_j, conf_i, conf_j, H, W, *, optimize_depth=True, optimize_im_poses=True, optimize_focals=True,
                 optimize_pw_poses=True, norm_pw_scale=True, base_scale=0.5):
        edges = [(int(i), int(j)) for i, j in edges]
        E, H, W = len(edges), int(H), int(W)
        if E < 1 or H < 1 or W < 1:
            raise ValueError(f"{E} edges over images of {H} x {W}: positive sizes expected")
        V = max(max(e) for e in edges) + 1
        n = H * W
        for t in (pred_i, pred_j, conf_i, conf_j):
            if not isinstance(t, torch.Tensor):
                raise ValueError("pred_i, pred_j, conf_i, conf_j must be torch tensors on the device")
        dev = _lib.require_device(pred_i.contiguous(), pred_j.contiguous(), conf_i.contiguous(), conf_j.contiguous())
        for name, t in (("pred_i", pred_i), ("pred_j", pred_j)):
            if t.dim() < 2 or t.shape[0] != E or t.numel() != E * n * 3:
                raise ValueError(f"{name} must be [{E},{n},3]: images of different shapes within one problem are not taken; got {list(t.shape)}")
        for name, t in (("conf_i", conf_i), ("conf_j", conf_j)):
            if t.dim() < 1 or t.shape[0] != E or t.numel() != E * n:
                raise ValueError(f"{name} must be [{E},{n}]: images of different shapes within one problem are not taken; got {list(t.shape)}")
        self.flags = (OPT_DEPTH * bool(optimize_depth) | OPT_IM_POSES * bool(optimize_im_poses) | OPT_FOCALS * bool(optimize_focals)
                      | OPT_PW_POSES * bool(optimize_pw_poses) | NORM_PW_SCALE * bool(norm_pw_scale))
        self.V, self.H, self.W, self.E, self.edges, self.device, self.base_scale = V, H, W, E, edges, dev, float(base_scale)
        self.conf_i = _f32(conf_i.reshape(E, n), (E, n), "conf_i", dev)
        self.conf_j = _f32(conf_j.reshape(E, n), (E, n), "conf_j", dev)
        pred_i = _f32(pred_i.reshape(E, n, 3), (E, n, 3), "pred_i", dev)
        pred_j = _f32(pred_j.reshape(E, n, 3), (E, n, 3), "pred_j", dev)
        host_edges = (ctypes.c_int32 * (2 * E))(*[x for e in edges for x in e])
        refused = ValueError(f"mi355gs_align_create refused {V} images of {H} x {W} with {E} edges (include/mi355gs.h: V <= {MAX_VIEWS}, "
                             f"E <= {MAX_EDGES}, E H W <= 2^31 - 1, every image covered by an edge, no edge from an image to itself)")
        self._open(dev, (V, H, W, E, self.flags), lambda ws: (ws, V, H, W, host_edges, E, self.flags, self.base_scale), refused, refused)
        _lib.call(dev, "align_pack", self._h, _lib.STREAM, pred_i, pred_j, self.conf_i, self.conf_j)
        if dev.type == "cuda":
            torch.cuda.current_stream(dev).synchronize()   # pred_i / pred_j may go once the records are written

    @classmethod
    def from_arrays(cls, *args, **kwargs):
        return cls(*args, **kwargs)

    def im_conf(self) -> torch.Tensor:
        """`_compute_img_conf` (base_opt.py:137-143): per image the element-wise maximum of the raw confidences over every edge
        side at which it occurs, [V,H,W]."""
        out = torch.zeros(self.V, self.H * self.W, dtype=torch.float32, device=self.device)
        for e, (i, j) in enumerate(self.edges):
            out[i] = torch.maximum(out[i], self.conf_i[e])
            out[j] = torch.maximum(out[j], self.conf_j[e])
        return out.view(self.V, self.H, self.W)


class AlignState:
    """depth_log [V,H*W] (depth = exp), im_pose [V,7] (quaternion x y z w, then t; T = sign(t) expm1|t|), focal_log [V]
    (focal = exp(focal_log / 20)), pp_raw [V,2] (constant; principal point = (W/2, H/2) + 10 pp_raw), pw_pose [E,8] (quaternion,
    t, log-scale) — the reference's im_depthmaps, im_poses, im_focals, im_pp, pw_poses — with the Adam moments and step count."""
    NAMES = ("depth_log", "im_pose", "focal_log", "pp_raw", "pw_pose")

    def __init__(self, problem: AlignProblem, depth_log, im_pose, focal_log, pp_raw, pw_pose):
        P, dev = problem, problem.device
        self.problem = P
        self.depth_log = _f32(depth_log.reshape(P.V, -1) if isinstance(depth_log, torch.Tensor) else depth_log, (P.V, P.H * P.W), "depth_log", dev).clone()
        self.im_pose = _f32(im_pose, (P.V, 7), "im_pose", dev).clone()
        self.focal_log = _f32(focal_log.reshape(-1) if isinstance(focal_log, torch.Tensor) else focal_log, (P.V,), "focal_log", dev).clone()
        self.pp_raw = _f32(pp_raw, (P.V, 2), "pp_raw", dev).clone()
        self.pw_pose = _f32(pw_pose, (P.E, 8), "pw_pose", dev).clone()
        self.moments = {k: (torch.zeros_like(getattr(self, k)), torch.zeros_like(getattr(self, k))) for k in self.NAMES if k != "pp_raw"}
        self.step = 0

    @classmethod
    def from_arrays(cls, problem, depth_log, im_pose, focal_log, pp_raw, pw_pose):
        return cls(problem, depth_log, im_pose, focal_log, pp_raw, pw_pose)

    def _state_ptrs(self):
        return [_lib.ptr(getattr(self, k)) for k in self.NAMES]

    # ---- the getters init_geo.py:51-59 reads, with the reference's meanings
    def _poses(self, raw):
        q = raw[:, :4] / raw[:, :4].norm(dim=1, keepdim=True)
        x, y, z, w = q.unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
        t = raw[:, 4:7]
        out = torch.zeros(raw.shape[0], 4, 4, dtype=raw.dtype, device=raw.device)
        out[:, :3, :3], out[:, :3, 3], out[:, 3, 3] = R, torch.sign(t) * torch.expm1(t.abs()), 1
        return out

    def im_poses(self) -> torch.Tensor:
        """`get_im_poses`: camera-to-world [V,4,4]"""
        return self._poses(self.im_pose)

    def focals(self) -> torch.Tensor:
        """`get_focals`: [V,1]"""
        return (self.focal_log.view(-1, 1) / FOCAL_BREAK).exp()

    def principal_points(self) -> torch.Tensor:
        P = self.problem
        return torch.tensor([P.W / 2, P.H / 2], dtype=torch.float32, device=P.device) + PP_BREAK * self.pp_raw

    def intrinsics(self) -> torch.Tensor:
        """`get_intrinsics`: [V,3,3]"""
        K = torch.zeros(self.problem.V, 3, 3, dtype=torch.float32, device=self.problem.device)
        K[:, 0, 0] = K[:, 1, 1] = self.focals().flatten()
        K[:, :2, 2] = self.principal_points()
        K[:, 2, 2] = 1
        return K

    def _points(self):
        P = self.problem
        pts = torch.empty(P.V, P.H, P.W, 3, dtype=torch.float32, device=P.device)
        depth = torch.empty(P.V, P.H, P.W, dtype=torch.float32, device=P.device)
        _lib.call(P.device, "align_points", P._h, _lib.STREAM, *self._state_ptrs(), pts, depth)
        return pts, depth

    def pts3d(self) -> torch.Tensor:
        """`get_pts3d`: [V,H,W,3] (one kernel dispatch)"""
        return self._points()[0]

    def depthmaps(self) -> torch.Tensor:
        """`get_depthmaps`: [V,H,W]"""
        return self._points()[1]

    def im_conf(self) -> torch.Tensor:
        return self.problem.im_conf()

    def to_init_stage_inputs(self, log_depth=False) -> dict:
        """The keyword arrays `init_stage.init_from_pointmaps` takes from the aligner (init_geo.py:51-59): w2c = the inverse of
        im_poses(), intrinsics, focals, pointmaps, depthmaps and confidences (im_conf()).  log_depth=True hands over
        `im_depthmaps` as init_geo.py:56 does — the raw parameter, the LOG of the depth — instead of get_depthmaps()."""
        P = self.problem
        pts, depth = self._points()
        return dict(pointmaps=pts, depthmaps=self.depth_log.view(P.V, P.H, P.W).clone() if log_depth else depth, confidences=self.im_conf(),
                    intrinsics=self.intrinsics(), w2c=torch.linalg.inv(self.im_poses()).contiguous(), focals=self.focals().flatten())


def from_reference_scene(scene):
    """(problem, state) from a reference `PointCloudOptimizer` — duck-typed, nothing is imported from the reference — as it stands
    after `global_aligner(...)` and `init_fun.init_minimum_spanning_tree(scene, ...)`, in place of `global_alignment_loop(scene)`.
    Read: edges, _stacked_pred_i / _j, conf_i / conf_j, im_depthmaps, im_poses, im_focals, im_pp, pw_poses, pw_adaptors,
    norm_pw_scale, base_scale, focal_break, pw_break and every parameter's requires_grad.  Refused with a ValueError naming the
    switch: non-zero or trainable pw_adaptors (allow_pw_adaptors), trainable im_pp (optimize_pp), dist other than l1, a conf
    transform other than log, a focal_break other than 20, images of different shapes."""
    if getattr(scene.pw_adaptors, "requires_grad", False):
        raise ValueError("allow_pw_adaptors=True (trainable pw_adaptors) is out of scope")
    if bool((scene.pw_adaptors.detach() != 0).any()):
        raise ValueError("non-zero pw_adaptors (allow_pw_adaptors) are out of scope")
    if getattr(scene.im_pp, "requires_grad", False):
        raise ValueError("optimize_pp=True (trainable im_pp) is out of scope")
    probe_a, probe_b = torch.tensor([[3.0, 4.0, 0.0]]), torch.zeros(1, 3)
    if not torch.allclose(torch.as_tensor(scene.dist(probe_a, probe_b, weight=torch.ones(1))).float(), torch.tensor([5.0])):
        raise ValueError("dist: only dist='l1' (the weighted Euclidean norm) is implemented")
    probe = torch.tensor([1.0, math.e, 7.5])
    if not torch.allclose(torch.as_tensor(scene.conf_trf(probe)).float(), probe.log()):
        raise ValueError("conf: only the conf='log' transform is implemented")
    if float(scene.focal_break) != FOCAL_BREAK:
        raise ValueError(f"focal_break = {scene.focal_break}: only {FOCAL_BREAK} is implemented")
    float(scene.pw_break)   # only scales the adaptors, which are zero
    shapes = {tuple(int(s) for s in hw) for hw in scene.imshapes}
    if len(shapes) != 1:
        raise ValueError(f"images of different shapes within one problem are not taken: {sorted(shapes)}")
    H, W = shapes.pop()
    edges = [(int(i), int(j)) for i, j in scene.edges]
    names = [f"{i}_{j}" for i, j in edges]
    conf_i = torch.stack([scene.conf_i[k].detach().reshape(-1) for k in names]).float()
    conf_j = torch.stack([scene.conf_j[k].detach().reshape(-1) for k in names]).float()
    problem = AlignProblem(edges, scene._stacked_pred_i.detach(), scene._stacked_pred_j.detach(), conf_i, conf_j, H, W,
                           optimize_depth=scene.im_depthmaps.requires_grad, optimize_im_poses=scene.im_poses.requires_grad,
                           optimize_focals=scene.im_focals.requires_grad, optimize_pw_poses=scene.pw_poses.requires_grad,
                           norm_pw_scale=bool(scene.norm_pw_scale), base_scale=float(scene.base_scale))
    state = AlignState(problem, scene.im_depthmaps.detach(), scene.im_poses.detach(), scene.im_focals.detach().reshape(-1),
                       scene.im_pp.detach(), scene.pw_poses.detach())
    return problem, state


def step_table(first_step: int, niter: int, lr: float, schedule: str, lr_min: float) -> np.ndarray:
    """float32 [niter,4]: row k = (-lr_k / (1 - 0.9^t), sqrt(1 - 0.9^t), 0, 0) with t = first_step + k + 1 and lr_k the schedule's
    rate at k / niter (base_opt.py:352-357, commons.py:83-90), all formed in float64 as the reference and torch.optim.Adam do."""
    if schedule not in ("cosine", "linear"):
        raise ValueError(f"bad lr schedule={schedule!r}")
    rows = np.zeros((niter, 4), dtype=np.float64)
    for k in range(niter):
        t = k / niter
        lr_k = lr_min + (lr - lr_min) * (1 + np.cos(t * np.pi)) / 2 if schedule == "cosine" else lr + (lr_min - lr) * t
        step = first_step + k + 1
        bc1, bc2 = 1 - 0.9 ** step, 1 - 0.9 ** step
        rows[k, 0], rows[k, 1] = -(lr_k / bc1), bc2 ** 0.5
    return rows.astype(np.float32)


def global_alignment(problem: AlignProblem, state: AlignState, niter=300, lr=0.01, schedule="cosine", lr_min=1e-6):
    """`global_alignment_loop(net, lr, niter, schedule, lr_min)`: niter Adam iterations on `state`, in place, enqueued by one
    library call (1 + 3 niter kernel dispatches).  -> (the loss of the last iteration, taken before that iteration's step, as a
    float — the one synchronisation, after the run; losses float32 [niter] on the device).  niter = 0 leaves the state unchanged
    and returns inf (base_opt.py:339)."""
    if state.problem is not problem:
        raise ValueError("the state belongs to another problem")
    niter = int(niter)
    if niter < 0:
        raise ValueError(f"niter = {niter}")
    dev = problem.device
    losses = torch.empty(niter, dtype=torch.float32, device=dev)
    if niter == 0 or not (problem.flags & (OPT_DEPTH | OPT_IM_POSES | OPT_FOCALS | OPT_PW_POSES)):
        return float("inf"), losses[:0]   # (with nothing to optimise the reference returns before its loop, base_opt.py:327-329)
    table = torch.from_numpy(step_table(state.step, niter, float(lr), schedule, float(lr_min))).to(dev)
    moments = [t for k in ("depth_log", "im_pose", "focal_log", "pw_pose") for t in state.moments[k]]
    _lib.call(dev, "align_run", problem._h, _lib.STREAM, niter, table, *state._state_ptrs(), *moments, losses)
    state.step += niter
    return float(losses[-1]), losses   # (the read of the last loss also keeps `table` alive until the run has finished)


# ------------------------------------------------------------------------------------------------ the initialisation (csrc/align_init.hip)
def _init_workspace(dev, B, n):
    return _lib.scratch(dev, "align_init_workspace_bytes", int(B), int(n), what=f"mi355gs_align_init_workspace_bytes refused {B} jobs of {n} "
                        f"points (include/mi355gs.h: 1 <= B <= {MAX_EDGES}, n >= 1, B n <= 2^31 - 1)")


def register_points(x, y, weights=None):
    """The similarity registration y ~ scale * R x + T of B point sets, roma's `rigid_points_registration(x, y, weights,
    compute_scaling=True)` conventions (weighted centroids; M = sum w yh xh^T; R the special-orthogonal Procrustes solution, the
    last singular direction flipped when det < 0; scale = sum of the signed singular values / sum w |xh|^2).  x, y: float32
    [B,n,3] on the device, weights [B,n] or None -> (scale [B], R [B,3,3], T [B,3]).  Four kernel dispatches, no synchronisation."""
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[-1] != 3:
            raise ValueError(f"{name} must be a [B,n,3] tensor on the device")
    B, n = int(x.shape[0]), int(x.shape[1])
    if B < 1 or n < 1:
        raise ValueError(f"{B} point sets of {n} points: positive sizes expected")
    dev = _lib.require_device(x.contiguous())
    x, y = _f32(x, (B, n, 3), "x", dev), _f32(y, (B, n, 3), "y", dev)
    w = None if weights is None else _f32(weights, (B, n), "weights", dev)
    ws = _init_workspace(dev, B, n)
    srt = torch.empty(B, 16, dtype=torch.float32, device=dev)
    _lib.call(dev, "align_init_register", ws, _lib.STREAM, B, n, x, None, 3 * n, 3, y, None, 3 * n, w, None, n, srt, None)
    return srt[:, 0].clone(), srt[:, 1:10].reshape(B, 3, 3).clone(), srt[:, 10:13].clone()


def spanning_tree(scores: dict, V: int) -> list:
    """The tree `scipy.sparse.csgraph.minimum_spanning_tree` returns for the negated scores (init_im_poses.py:138-139), without
    scipy: an image pair takes the better of its two directions, the tree keeps the spanning edges of the largest scores, and an
    edge comes back in the direction that won.  -> [(score, i, j)].  The order among EQUAL scores is not pinned (neither is
    scipy's): the first direction met and the first edge sorted win here."""
    if V > MAX_VIEWS:
        raise ValueError(f"{V} images: the host-side tree takes V <= {MAX_VIEWS}")
    best = {}
    for (i, j), s in scores.items():
        key = (min(i, j), max(i, j))
        if key not in best or s > best[key][0]:
            best[key] = (s, i, j)
    parent = list(range(V))

    def root(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    tree = []
    for s, i, j in sorted(best.values(), key=lambda t: -t[0]):
        ri, rj = root(i), root(j)
        if ri != rj:
            parent[ri] = rj
            tree.append((s, i, j))
    return tree


def walk_plan(tree, edges, scores):
    """The walk of init_im_poses.py:144-207 with the data left out: which records are copied, registered and applied in which
    order, and which edge's pred_i feeds which image's focal.  -> dict(first=(e, i, j), steps=[(e, side, i, j)], mst_edges,
    focal_edge={image: e}, pose_step={image: step index, or -1 for the identity of the first edge's i}).
    side 0: i was done — pred_i[e] is registered onto pts3d[i] and pts3d[j] = s R pred_j[e] + T; side 1: the mirror image."""
    eidx = {tuple(e): k for k, e in enumerate(edges)}
    todo = sorted(tree)
    _, i, j = todo.pop()                       # the strongest edge
    cur = eidx[(i, j)]
    first, done, mst = (cur, i, j), {i, j}, [(i, j)]
    focal_edge, pose_step, steps = {i: cur}, {i: -1}, []
    while todo:
        score, i, j = todo.pop()
        # The reference's quirk, reproduced: the focal of a not-yet-seen i is estimated from pred_i of the edge processed BEFORE
        # this one (init_im_poses.py:166-167 reads `i_j` before the branches below reassign it), not from an edge of i.
        if i not in focal_edge:
            focal_edge[i] = cur
        if i in done:
            cur = eidx[(i, j)]
            steps.append((cur, 0, i, j))
            done.add(j)
        elif j in done:
            cur = eidx[(i, j)]
            steps.append((cur, 1, i, j))
            done.add(i)
        else:
            todo.insert(0, (score, i, j))      # touches neither end yet: back to the front of the queue
            continue
        mst.append((i, j))
        if i not in pose_step:
            pose_step[i] = len(steps) - 1
    best_first = sorted(scores, key=lambda e: -scores[e])
    best_edge_of = {}
    for (i, j) in best_first:                  # the best-scoring edge whose first image is i
        best_edge_of.setdefault(i, eidx[(i, j)])
    for i, e in best_edge_of.items():
        focal_edge.setdefault(i, e)
    return dict(first=first, steps=steps, mst_edges=mst, focal_edge=focal_edge, pose_step=pose_step, best_edge_of=best_edge_of)


def init_minimum_spanning_tree(problem: AlignProblem, *, focal_avg=False, known_focal=None, pnp_fn=None, min_conf_thr=3.0) -> AlignState:
    """`init_fun.init_minimum_spanning_tree(scene, focal_avg=..., known_focal=...)` (init_im_poses.py:66-221) -> the state the
    reference object holds afterwards (depth_log, im_pose, focal_log, zero pp_raw, pw_pose, fresh moments, step 0), ready for
    `global_alignment`.  Also attached: `state.mst_edges` (the tree as directed edges, in the order the walk took them),
    `state.init_pts3d` [V,H,W,3] (the initial world pointmaps, after scale normalisation), `state.focal_edge` ({image: the edge
    whose pred_i fed its focal}), `state.init_focals` (those Weiszfeld estimates, in the order of sorted(focal_edge)) and
    `state.edge_scores` ({edge: score}).

    Everything is enqueued on the current stream.  There is ONE host synchronisation: the read of the 2 E confidence means the
    tree is built from (the tree and the walk are host decisions; the V - 1 dependent registrations of the walk are chained on the
    stream).  A second one happens only with `pnp_fn`.

    Poses.  The walk gives at most V - 1 images a pose.  The reference fills the rest with `fast_pnp` (cv2.solvePnPRansac: random,
    and not available here).  `pnp_fn(pts3d_i [H,W,3], focal, mask [H,W]) -> (focal, cam2world [4,4]) | None` takes a caller's
    implementation under fast_pnp's contract (mask = im_conf[i] > min_conf_thr; None -> the identity, the reference's fallback).
    THE DEFAULT (pnp_fn=None) DEPARTS FROM THE REFERENCE: a deterministic stand-in registers the image's own-frame pointmap
    (pred_i of the best-scoring edge whose first image is i, weights conf_i) onto pts3d[i] and takes [R | T] — the step the walk's
    own branches use, no synchronisation, no random sampling; an image that is never a first image gets the identity.  On
    noise-free pointmaps both give the camera-to-world pose; they differ by what RANSAC's sampling and the registration's
    least-squares fit make of the noise.

    focal_avg / known_focal freeze the focals in the reference (`preset_focal`); a problem's switches are fixed when it is made,
    so either is refused on a problem built without optimize_focals=False."""
    P = problem
    if not P.flags & OPT_IM_POSES:
        raise ValueError("optimize_im_poses=False: the known-poses branch of init_from_pts3d (init_im_poses.py:95-106) is out of scope")
    if (focal_avg or known_focal is not None) and P.flags & OPT_FOCALS:
        raise ValueError("focal_avg / known_focal freeze the focals (preset_focal): build the AlignProblem with optimize_focals=False")
    if known_focal is not None and not float(known_focal) > 0:
        raise ValueError(f"known_focal = {known_focal}: a positive focal expected")
    dev, V, E, n, H, W = P.device, P.V, P.E, P.H * P.W, P.H, P.W
    ws = _init_workspace(dev, max(E, V), n)
    run = lambda name, *args: _lib.call(dev, "align_init_" + name, *args)       # noqa: E731
    i32 = lambda values: torch.tensor(list(values), dtype=torch.int32).to(dev)   # noqa: E731
    means = torch.empty(2 * E, dtype=torch.float32, device=dev)
    run("means", ws, _lib.STREAM, E, n, P.conf_i, means)
    run("means", ws, _lib.STREAM, E, n, P.conf_j, means[E:])
    m = means.cpu().numpy()                                                  # the one synchronisation
    scores = {e: float(m[k] * m[E + k]) for k, e in enumerate(P.edges)}      # commons.py:20-25
    tree = spanning_tree(scores, V)
    if len(tree) != V - 1:
        raise ValueError("the edges do not connect every image: no spanning tree (the reference's walk would not end)")
    plan = walk_plan(tree, P.edges, scores)
    if focal_avg and len(plan["focal_edge"]) != V:
        missing = sorted(set(range(V)) - set(plan["focal_edge"]))
        raise ValueError(f"focal_avg: images {missing} are never the first image of an edge and have no focal estimate "
                         "(the reference fails there too)")

    # every index table is uploaded here, while the stream is idle: a host-to-device copy behind enqueued kernels would wait for them
    n_steps = len(plan["steps"])
    focal_images = sorted(plan["focal_edge"])
    focal_row = {v: k for k, v in enumerate(focal_images)}
    src_idx = i32(2 * plan["focal_edge"][v] for v in focal_images)
    pair_src, pair_tgt = i32(2 * e for e in range(E)), i32(i for i, j in P.edges)
    pose_row = [-1] * V
    for v in range(V):
        if v in plan["pose_step"]:
            pose_row[v] = plan["pose_step"][v]
        elif pnp_fn is None and v in plan["best_edge_of"]:
            # the stand-in for PnP: the pair registration of the best edge of v IS the registration of v's own-frame pointmap
            # onto pts3d[v] — its row of the pair batch is the pose
            pose_row[v] = n_steps + plan["best_edge_of"][v]
    if pnp_fn is None:
        pose_row_d, focal_row_d = i32(pose_row), i32(focal_row.get(v, -1) for v in range(V))
    recs = int(_lib.lib().mi355gs_align_records(P._h))
    rec = lambda e, side: recs + 16 * n * (2 * e + side)                     # noqa: E731
    pts3d = torch.empty(V, n, 3, dtype=torch.float32, device=dev)
    img = lambda v: _lib.ptr(pts3d) + 12 * n * v                             # noqa: E731
    srt = torch.zeros(n_steps + E + V, 16, dtype=torch.float32, device=dev)  # walk rows, pair rows, rows of pnp_fn
    row = lambda k: _lib.ptr(srt) + 64 * k                                   # noqa: E731
    e0, i0, j0 = plan["first"]
    run("apply", _lib.STREAM, n, rec(e0, 0), 4, None, img(i0))
    run("apply", _lib.STREAM, n, rec(e0, 1), 4, None, img(j0))
    for k, (e, side, i, j) in enumerate(plan["steps"]):
        known, new = (i, j) if side == 0 else (j, i)
        conf = (P.conf_i if side == 0 else P.conf_j)[e]
        run("register", ws, _lib.STREAM, 1, n, rec(e, side), None, 0, 4, img(known), None, 0, conf, None, 0, row(k), None)
        run("apply", _lib.STREAM, n, rec(e, 1 - side), 4, row(k), img(new))

    # focals: one batch over the images that have a source record (they do not depend on the walk's results)
    focals = torch.zeros(len(focal_images) + V, dtype=torch.float32, device=dev)   # the estimates, then pnp_fn's
    run("focals", ws, _lib.STREAM, len(focal_images), H, W, recs, src_idx, 4 * n, 4, focals)

    # pair poses: every edge's pred_i onto pts3d[i], weights conf_i (init_im_poses.py:109-113)
    pw_pose = torch.empty(E, 8, dtype=torch.float32, device=dev)
    run("register", ws, _lib.STREAM, E, n, recs, pair_src, 4 * n, 4, pts3d, pair_tgt, 3 * n, P.conf_i, None, n, row(n_steps), pw_pose)

    if pnp_fn is not None:
        im_conf, host_focals = P.im_conf(), None
        for v in range(V):
            if v in plan["pose_step"]:
                continue
            if host_focals is None:
                host_focals = focals.cpu()                                   # the second synchronisation
            focal = float(host_focals[focal_row[v]]) if v in focal_row else None
            res = pnp_fn(pts3d[v].view(H, W, 3), focal, im_conf[v] > min_conf_thr)
            if not res:
                continue                                                     # the identity (init_im_poses.py:215-216)
            focal, cam2world = res
            c2w = torch.as_tensor(cam2world, dtype=torch.float32).reshape(4, 4).cpu()
            pose_row[v] = n_steps + E + v
            srt[pose_row[v]] = torch.cat([torch.ones(1), c2w[:3, :3].reshape(9), c2w[:3, 3], torch.zeros(3)]).to(dev)
            focal_row[v] = len(focal_images) + v
            focals[focal_row[v]] = float(focal)

    depth_log = torch.empty(V, n, dtype=torch.float32, device=dev)
    im_pose = torch.empty(V, 7, dtype=torch.float32, device=dev)
    focal_log = torch.empty(V, dtype=torch.float32, device=dev)
    if pnp_fn is not None:
        pose_row_d, focal_row_d = i32(pose_row), i32(focal_row.get(v, -1) for v in range(V))
    mode = 2 if known_focal is not None else (1 if focal_avg else 0)
    run("state", ws, _lib.STREAM, V, E, H, W, 1 if P.flags & NORM_PW_SCALE else 0, P.base_scale, mode,
        float(known_focal) if known_focal is not None else 0.0, srt, pose_row_d, focals, focal_row_d, pw_pose, pts3d, depth_log, im_pose, focal_log)
    state = AlignState(P, depth_log, im_pose, focal_log, torch.zeros(V, 2, dtype=torch.float32, device=dev), pw_pose)
    state.mst_edges, state.init_pts3d, state.focal_edge, state.edge_scores = plan["mst_edges"], pts3d.view(V, H, W, 3), dict(plan["focal_edge"]), scores
    state.init_focals = focals[:len(focal_images)]   # the per-image Weiszfeld estimates, in the order of sorted(focal_edge)
    return state


def compute_global_alignment(problem: AlignProblem, init="mst", niter=300, schedule="cosine", lr=0.01, lr_min=1e-6, focal_avg=False,
                             known_focal=None, pnp_fn=None, state=None):
    """`compute_global_alignment` (base_opt.py:275-287): the initialisation, then the loop -> (state, last loss, losses).
    init="mst": `init_minimum_spanning_tree`; init=None: the caller's `state` as it stands; init="known_poses" is out of scope."""
    if init == "mst":
        state = init_minimum_spanning_tree(problem, focal_avg=focal_avg, known_focal=known_focal, pnp_fn=pnp_fn)
    elif init == "known_poses":
        raise ValueError("init='known_poses' (init_from_known_poses) is out of scope")
    elif init is None:
        if state is None:
            raise ValueError("init=None takes the caller's state: pass state=")
    else:
        raise ValueError(f"bad value for init={init!r}")
    last, losses = global_alignment(problem, state, niter=niter, lr=lr, schedule=schedule, lr_min=lr_min)
    return state, last, losses


def gradients(problem: AlignProblem, state: AlignState) -> dict:
    """The loss and every gradient at `state`, nothing updated (mi355gs_align_grad; tests)."""
    dev = problem.device
    g = {k: torch.empty_like(getattr(state, k)) for k in ("depth_log", "im_pose", "focal_log", "pw_pose")}
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.call(dev, "align_grad", problem._h, _lib.STREAM, *state._state_ptrs(), *g.values(), loss)
    g["loss"] = loss
    return g
