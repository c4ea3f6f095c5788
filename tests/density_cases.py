"""Cases and checks of the adaptive density control (instantsplat_amd/density.py, csrc/density.hip), shared by the emulated
(CPU) and the GPU test files.

What is held:
  * DECISIONS are a condition, not a tolerance.  The inputs are built so that every decision quantity (|grads|, max(exp(s)),
    sigmoid(o), the children's scales, the radii) is at least 1e-3 relative away from its threshold (`assert_margins`), the
    float32 and the float64 restatement of the reference's sequence must agree on every mask for them (`assert_decisions_agree`,
    on the CPU, at import of a case), and then the device must agree exactly: new P, the class totals and the output order.
  * COPIED values (parameters, moments, per-point rates, statistics) are bit-equal to the reference's own result
    (tests/golden/density_vectors.npz, written by tests/golden/make_golden_density.py from the reference's GaussianModel
    methods) and to the numpy restatement of the reference's sequence below.
  * COMPUTED values (child positions, child scalings, reset opacities, the statistics after several k_density_stats calls) are
    compared with the float64 restatement: the maximum absolute error per tensor may be FACTOR x the float32 golden's (for
    cases without a golden: the float32 restatement's) own distance to float64 on the same case, with a floor of one ulp of the
    tensor's largest magnitude.  FACTOR = 2.5 is the multiple the suite uses for fixed inputs (tests/loss_util.py REL,
    tests/test_baseline_sizes_gpu.py FACTOR_FIXED_INPUTS); the limits go through tests/ops_util.bound (GS_CALIBRATE=1 prints
    them).

Measured device maxima (GS_CALIBRATE=1), in units of the limit's yardstick max(own distance, 1 ulp): DEVICE_MAXIMA below.
"""
import os

import numpy as np
import torch

from tests import ops_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "density_vectors.npz")
FACTOR = 2.5
# MI355X, worst case of the GPU tier (tests/test_density_gpu.py) in units of max(own distance, 1 ulp), the limit being FACTOR;
# the emulated kernels on x86-64 measure 1.79 / 0.72 / 0.22 / 0.88
DEVICE_MAXIMA = {"child_xyz": 1.79, "child_scaling": 0.99, "reset_opacity": 1.00, "stats": 0.88}

EXTENT, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY = 2.0, 0.01, 0.0002, 0.005
MARGIN = 1e-3
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025, 3000)
SIZE_TWO_SCAN_TURNS = 1024 * 256 + 77   # more than 1024 blocks of 256: the scan kernel's loop takes a second turn
FAMILIES = ("mixed", "nothing", "all_pruned", "all_split", "all_clone", "denom0", "children_pruned")
MODES = ("clone", "split", "prune_mask", "prune", "seq")
PARAM_NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation"}


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_case(P, family="mixed", sh_degree=3, N=2, max_screen_size=None, seed=0):
    """Inputs of one event, float32 numpy: the model's rows, the optimizer's moments, per-point rates, the statistics, the
    unit normals of the children and a prune mask for prune_points.  Every decision quantity is drawn from ranges that keep
    clear of the thresholds."""
    r = np.random.RandomState(1000 * seed + 7 * P + 13 * FAMILIES.index(family) + N)
    f32 = np.float32
    rest = 3 * ((sh_degree + 1) ** 2 - 1)
    dense, world = PERCENT_DENSE * EXTENT, 0.1 * EXTENT
    div = 0.8 * N
    pick = lambda *opts: np.array(opts)[r.randint(0, len(opts), P)]

    def choose(kind, table):
        lo = np.array([table[k][0] for k in kind])
        hi = np.array([table[k][1] for k in kind])
        return lo + (hi - lo) * r.rand(P)

    small, large, huge = (0.2 * dense, 0.9 * dense), (1.25 * dense, 0.75 * world), (1.15 * world * div, 1.6 * world * div)
    low_o, high_o = (0.1 * MIN_OPACITY, 0.8 * MIN_OPACITY), (2.0 * MIN_OPACITY, 0.95)
    low_g, high_g = (0.0, 0.5 * MAX_GRAD), (1.5 * MAX_GRAD, 20.0 * MAX_GRAD)
    scale_kind, opac_kind, grad_kind = pick(0, 1, 2), pick(0, 1, 1, 1), pick(0, 1)
    denom = r.randint(1, 6, P).astype(np.float64)
    if family == "nothing":
        scale_kind, opac_kind, grad_kind = pick(0, 1), np.ones(P, int), np.zeros(P, int)
    elif family == "all_pruned":
        opac_kind, grad_kind = np.zeros(P, int), np.zeros(P, int)
    elif family == "all_split":
        scale_kind, opac_kind, grad_kind = np.ones(P, int), np.ones(P, int), np.ones(P, int)
    elif family == "all_clone":
        scale_kind, opac_kind, grad_kind = np.zeros(P, int), np.ones(P, int), np.ones(P, int)
    elif family == "denom0":
        denom[r.rand(P) < 0.5] = 0.0
    elif family == "children_pruned":   # with max_screen_size: parents of the world-size class, whose children are too large as well
        scale_kind = np.where(r.rand(P) < 0.7, 2, scale_kind)
        grad_kind = np.where(scale_kind == 2, 1, grad_kind)
        opac_kind = np.where(scale_kind == 2, 1, opac_kind)
    smax = choose(scale_kind, (small, large, huge))
    factors = 0.3 + 0.7 * r.rand(P, 3)
    factors[np.arange(P), r.randint(0, 3, P)] = 1.0
    scaling = np.log(smax[:, None] * factors)
    sig = choose(opac_kind, (low_o, high_o))
    opacity = np.log(sig / (1.0 - sig))[:, None]
    g = choose(grad_kind, (low_g, high_g))
    accum = g * denom
    zero = denom == 0.0   # 0 / 0 = NaN -> 0 for some, x / 0 = inf >= max_grad for the others
    accum[zero] = np.where(r.rand(int(zero.sum())) < 0.5, 0.0, 0.3)
    radii = np.where(r.rand(P) < 0.7, r.randint(0, 16, P), r.randint(25, 60, P)).astype(np.float64)
    c = {"P": P, "family": family, "sh_degree": sh_degree, "N": N, "max_screen_size": max_screen_size, "rest_width": rest,
         "xyz": r.randn(P, 3), "f_dc": 0.3 * r.randn(P, 1, 3), "f_rest": 0.1 * r.randn(P, rest // 3, 3), "opacity": opacity,
         "scaling": scaling, "rotation": r.randn(P, 4) + 0.1, "per_point_lr": 1.0 + 99.0 * r.rand(P, 1),
         "accum": accum[:, None], "denom": denom[:, None], "max_radii": radii, "noise": r.randn(N * P, 3),
         "mask": r.rand(P) < 0.4}
    for n in PARAM_NAMES:
        c["m_" + n] = 0.01 * r.randn(*c[n].shape)
        c["v_" + n] = 1e-4 * r.rand(*c[n].shape)
    for k, v in c.items():
        if isinstance(v, np.ndarray) and v.dtype == np.float64:
            c[k] = np.ascontiguousarray(v.astype(f32))
    assert_margins(c)
    assert_decisions_agree(c)
    return c


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def assert_margins(c):
    """every decision quantity at least MARGIN (relative) away from its threshold, in float64"""
    def clear(x, t, what):
        x = np.asarray(x, np.float64)
        fin = np.isfinite(x)
        d = np.abs(x[fin] - t) / t
        assert d.size == 0 or d.min() >= MARGIN, (what, float(d.min()))
    with np.errstate(divide="ignore", invalid="ignore"):
        g = c["accum"].astype(np.float64) / c["denom"].astype(np.float64)
    g[np.isnan(g)] = 0.0
    smax = np.exp(c["scaling"].astype(np.float64)).max(axis=1)
    clear(g, MAX_GRAD, "grads")
    clear(smax, PERCENT_DENSE * EXTENT, "scale vs percent_dense")
    clear(smax, 0.1 * EXTENT, "scale vs world size")
    clear(smax / (0.8 * c["N"]), 0.1 * EXTENT, "child scale vs world size")
    clear(_sigmoid(c["opacity"].astype(np.float64)), MIN_OPACITY, "opacity")
    if c["max_screen_size"]:
        clear(c["max_radii"], c["max_screen_size"], "radii")


# ------------------------------------------------------------------------------------------- the reference's sequence, in numpy
def _build_rotation(q):
    """reference utils/general_utils.py build_rotation, in q's dtype"""
    norm = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    q = q / norm[:, None]
    R = np.zeros((q.shape[0], 3, 3), q.dtype)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


class _Rows:
    """The per-Gaussian state the reference's methods edit: parameters, moments, the per-point rates (this package's rule),
    the statistics.  Values computed in `dt` (float32: the reference's arithmetic; float64: the yardstick)."""

    def __init__(self, c, dt):
        self.dt = dt
        self.t = {n: c[n].astype(dt) for n in PARAM_NAMES}
        for n in PARAM_NAMES:
            self.t["m_" + n], self.t["v_" + n] = c["m_" + n].astype(dt), c["v_" + n].astype(dt)
        self.t["per_point_lr"] = c["per_point_lr"].astype(dt)
        self.accum, self.denom, self.max_radii = c["accum"].astype(dt), c["denom"].astype(dt), c["max_radii"].astype(dt)
        self.origin = np.arange(c["P"])   # input row each row was copied / made from
        self.kind = np.zeros(c["P"], int)   # 0: an input row, 1: a clone, 2 + k: a child of copy k
        self.decisions = []

    def n(self):
        return self.t["xyz"].shape[0]

    def scaling_max(self):
        return np.exp(self.t["scaling"]).max(axis=1)

    def append(self, sel_rows, new, kind):   # cat_tensors_to_optimizer + densification_postfix
        self.kind = np.concatenate([self.kind, kind])
        for n in PARAM_NAMES:
            self.t[n] = np.concatenate([self.t[n], new[n]])
            self.t["m_" + n] = np.concatenate([self.t["m_" + n], np.zeros_like(new[n])])
            self.t["v_" + n] = np.concatenate([self.t["v_" + n], np.zeros_like(new[n])])
        self.t["per_point_lr"] = np.concatenate([self.t["per_point_lr"], self.t["per_point_lr"][sel_rows]])
        self.origin = np.concatenate([self.origin, self.origin[sel_rows]])
        k = self.n()
        self.accum, self.denom, self.max_radii = np.zeros((k, 1), self.dt), np.zeros((k, 1), self.dt), np.zeros(k, self.dt)

    def prune(self, mask):   # prune_points
        keep = ~mask
        for k in self.t:
            self.t[k] = self.t[k][keep]
        self.origin, self.kind = self.origin[keep], self.kind[keep]
        self.accum, self.denom, self.max_radii = self.accum[keep], self.denom[keep], self.max_radii[keep]


def restate(c, mode, dt):
    """The reference's sequence for one event -> (_Rows after it, totals).  mode: 'clone' / 'split' (the method alone, on the
    statistics' gradient), 'prune_mask' (prune_points(c['mask'])), 'prune' (densify_and_prune as written), 'seq' (with :464-465
    restored)."""
    s = _Rows(c, dt)
    N, P = c["N"], c["P"]
    thr = (lambda x: dt(x))   # a Python scalar meets a float32 tensor as float32
    with np.errstate(divide="ignore", invalid="ignore"):
        grads = s.accum / s.denom
    grads[np.isnan(grads)] = 0.0
    tot = dict(clone_selected=0, split=0)
    if mode in ("clone", "seq"):
        sel = (np.abs(grads[:, 0]) >= thr(MAX_GRAD)) & (s.scaling_max() <= thr(PERCENT_DENSE * EXTENT))
        s.decisions.append(sel)
        tot["clone_selected"] = int(sel.sum())
        s.append(np.nonzero(sel)[0], {n: s.t[n][sel] for n in PARAM_NAMES}, np.ones(int(sel.sum()), int))
    if mode in ("split", "seq"):
        padded = np.zeros(s.n(), dt)
        padded[:P] = grads[:, 0]
        sel = (padded >= thr(MAX_GRAD)) & (s.scaling_max() > thr(PERCENT_DENSE * EXTENT))
        s.decisions.append(sel)
        n_sel = int(sel.sum())
        tot["split"] = n_sel
        stds = np.tile(np.exp(s.t["scaling"][sel]), (N, 1))
        samples = stds * c["noise"][:N * n_sel].astype(dt)
        rots = np.tile(_build_rotation(s.t["rotation"][sel]), (N, 1, 1))
        new = {n: np.tile(s.t[n][sel], (N,) + (1,) * (s.t[n].ndim - 1)) for n in PARAM_NAMES}
        new["xyz"] = ((rots[:, :, 0] * samples[:, None, 0] + rots[:, :, 1] * samples[:, None, 1]) + rots[:, :, 2] * samples[:, None, 2]) \
            + np.tile(s.t["xyz"][sel], (N, 1))
        new["scaling"] = np.log(stds / dt(0.8 * N))
        rows = np.tile(np.nonzero(sel)[0], N)
        s.append(rows, new, 2 + np.repeat(np.arange(N), n_sel))
        s.prune(np.concatenate([sel, np.zeros(N * n_sel, bool)]))
    if mode == "prune_mask":
        s.decisions.append(c["mask"])
        s.prune(c["mask"])
    if mode in ("prune", "seq"):
        mask = _sigmoid(s.t["opacity"])[:, 0] < thr(MIN_OPACITY)
        if c["max_screen_size"]:
            mask = (mask | (s.max_radii > thr(c["max_screen_size"]))) | (s.scaling_max() > thr(0.1 * EXTENT))
        s.decisions.append(mask)
        s.prune(mask)
    tot["new_P"] = s.n()
    tot["originals"], tot["clones"], tot["children"] = int((s.kind == 0).sum()), int((s.kind == 1).sum()), int((s.kind >= 2).sum())
    assert np.all(np.diff(s.kind) >= 0)   # originals, clones, copy 0, copy 1, ...: each in index order
    return s, tot


def assert_decisions_agree(c):
    for mode in MODES:
        a, _ = restate(c, mode, np.float32)
        b, _ = restate(c, mode, np.float64)
        assert len(a.decisions) == len(b.decisions)
        for x, y in zip(a.decisions, b.decisions):
            assert np.array_equal(x, y), (c["family"], c["P"], mode, int((x != y).sum()))
        assert np.array_equal(a.origin, b.origin) and np.array_equal(a.kind, b.kind)


# ------------------------------------------------------------------------------------------------------------ the device side
def opt_params():
    from instantsplat_amd.arguments import OptimizationParams
    return OptimizationParams(iterations=1000, pp_optimizer=True, optim_pose=True)


def build_model(c, dev, optimizer="pp"):
    """A GaussianModel holding the case's rows with a stepped optimizer's state: optimizer 'pp' (PerPointAdam with per-point
    rates), 'plain' (the package's training_setup) or 'adam' (torch.optim.Adam over the same groups)."""
    import torch.nn as nn
    from instantsplat_amd.scene import GaussianModel
    m = GaussianModel(c["sh_degree"])
    m.active_sh_degree = c["sh_degree"]
    m.spatial_lr_scale = 1.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for n in PARAM_NAMES:
        setattr(m, ATTR[n], nn.Parameter(t(c[n]).requires_grad_(True)))
    m.P = torch.zeros(2, 7, device=dev)
    m.P[:, 0] = 1
    m.P.requires_grad_(True)
    o = opt_params()
    if optimizer == "pp":
        m.training_setup_pp(o, t(c["per_point_lr"]))
    elif optimizer == "plain":
        m.training_setup(o)
    else:
        m.optimizer = torch.optim.Adam(m._groups(o, None), lr=0.0, eps=1e-15)
        m._schedulers(o)
    m.percent_dense = PERCENT_DENSE
    for n in PARAM_NAMES:
        step = torch.tensor(3.0) if optimizer == "adam" else 3
        m.optimizer.state[getattr(m, ATTR[n])] = {"step": step, "exp_avg": t(c["m_" + n]), "exp_avg_sq": t(c["v_" + n])}
    m.xyz_gradient_accum, m.denom, m.max_radii2D = t(c["accum"]), t(c["denom"]), t(c["max_radii"])
    return m


def run_event(m, c, mode, n_sel):
    dev = m._xyz.device
    noise = torch.from_numpy(c["noise"][:c["N"] * n_sel]).to(dev) if n_sel else None
    with np.errstate(divide="ignore", invalid="ignore"):
        grads = c["accum"] / c["denom"]
    grads[np.isnan(grads)] = 0.0
    grads = torch.from_numpy(grads).to(dev)
    if mode == "clone":
        return m.densify_and_clone(grads, MAX_GRAD, EXTENT)
    if mode == "split":
        return m.densify_and_split(grads, MAX_GRAD, EXTENT, N=c["N"], noise=noise)
    if mode == "prune_mask":
        return m.prune_points(torch.from_numpy(c["mask"]).to(dev))
    return m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, c["max_screen_size"], clone_and_split=(mode == "seq"), N=c["N"], noise=noise)


def _ulp(x):
    return float(np.spacing(np.float32(max(float(np.abs(x).max()), 1e-30)))) if x.size else 0.0


def hold_computed(label, got, ref32, ref64):
    """max |got - float64| <= FACTOR x max(the float32 reference's own distance, one ulp of the largest magnitude)"""
    if ref64.size == 0:
        assert got.size == 0
        return 0.0
    own = float(np.abs(ref32.astype(np.float64) - ref64).max())
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    yard = max(own, _ulp(ref64))
    print(f"{label}: device {err:.3e}  float32 reference {own:.3e}  ulp {_ulp(ref64):.3e}  -> {err / yard:.2f} of the yardstick")
    ops_util.bound(label, err / yard, FACTOR)
    return err / yard


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_event(dev, c, mode, optimizer="pp", golden=None, step_after=True):
    """One event on the device against the float32 restatement (or the reference's own result `golden`: a dict of arrays) and
    the float64 restatement."""
    s32, tot = restate(c, mode, np.float32)
    s64, _ = restate(c, mode, np.float64)
    P, N = c["P"], c["N"]
    m = build_model(c, dev, optimizer)
    old_params = [getattr(m, ATTR[n]) for n in PARAM_NAMES]
    got_tot = run_event(m, c, mode, tot["split"])
    new_P = tot["new_P"]
    n_orig = tot["originals"]
    # ---- decisions: new P, the class totals, the order
    assert got_tot["new_P"] == new_P == m._xyz.shape[0], (got_tot, tot)
    assert got_tot["split"] == tot["split"] and got_tot["clone_selected"] == tot["clone_selected"], (got_tot, tot)
    assert got_tot["originals"] == n_orig, (got_tot, n_orig)
    assert got_tot["clones"] == tot["clones"] and got_tot["children"] == tot["children"], (got_tot, tot)
    assert got_tot["originals"] + got_tot["clones"] + got_tot["children"] == new_P
    assert got_tot["pruned"] == P + tot["clone_selected"] + (N - 1) * tot["split"] - new_P
    n_copied = got_tot["originals"] + got_tot["clones"]
    ref = {k: v for k, v in s32.t.items()}
    ref["accum"], ref["denom"], ref["max_radii"] = s32.accum, s32.denom, s32.max_radii
    if golden is not None:   # the reference's own result: bit-equal to the restatement wherever values are copied
        for k, v in golden.items():
            if k in ref and k not in ("xyz", "scaling"):
                assert np.array_equal(bits(v.reshape(ref[k].shape)), bits(ref[k])), k
        for k in ("xyz", "scaling"):
            assert np.array_equal(bits(golden[k][:n_copied]), bits(ref[k][:n_copied])), k
            ref[k] = golden[k].astype(np.float32)
    opt = m.optimizer
    state = lambda n: opt.state[getattr(m, ATTR[n])]
    got = {n: getattr(m, ATTR[n]).detach().cpu().numpy() for n in PARAM_NAMES}
    for n in PARAM_NAMES:
        got["m_" + n], got["v_" + n] = state(n)["exp_avg"].cpu().numpy(), state(n)["exp_avg_sq"].cpu().numpy()
    if optimizer == "pp":
        pp = opt.param_groups[0]["per_point_lr"]
        assert pp is m.per_point_lr
        got["per_point_lr"] = pp.cpu().numpy()
    got["accum"], got["denom"], got["max_radii"] = m.xyz_gradient_accum.cpu().numpy(), m.denom.cpu().numpy(), m.max_radii2D.cpu().numpy()
    # ---- copied values: bit-equal
    for k, v in got.items():
        assert v.shape == ref[k].shape, (k, v.shape, ref[k].shape)
        if k in ("xyz", "scaling"):
            assert np.array_equal(bits(v[:n_copied]), bits(ref[k][:n_copied])), k
        else:
            assert np.array_equal(bits(v), bits(ref[k])), (k, int((bits(v) != bits(ref[k])).sum()))
    # ---- computed values: the children's positions and scalings against float64
    for k in ("xyz", "scaling"):
        hold_computed(f"density child {k}", got[k][n_copied:], ref[k][n_copied:], s64.t[k][n_copied:])
    # ---- the optimizer: state keyed under the new parameters, the old ones gone, the groups hold the model's tensors
    for g in opt.param_groups:
        if g["name"] in ATTR:
            p = g["params"][0]
            assert p is getattr(m, ATTR[g["name"]]) and p.requires_grad and p.is_leaf
            assert p in opt.state and opt.state[p]["exp_avg"].shape == p.shape
            assert int(opt.state[p]["step"]) == 3
    for p in old_params:
        assert p not in opt.state
    assert len(opt.state) == len(PARAM_NAMES)
    # ---- a following step runs and updates all rows
    if step_after and new_P > 0:
        gen = torch.Generator().manual_seed(5)
        before = {n: getattr(m, ATTR[n]).detach().clone() for n in PARAM_NAMES}
        for n in PARAM_NAMES:
            p = getattr(m, ATTR[n])
            p.grad = (0.5 + torch.rand(p.shape, generator=gen)).to(dev)
        for g in opt.param_groups:
            if g["name"] == "xyz":
                g["lr"] = 1.6e-4
        opt.step()
        for n in PARAM_NAMES:
            p = getattr(m, ATTR[n])
            if p.numel():
                assert bool((p.detach() != before[n]).all()), n
                assert bool(torch.isfinite(p).all()), n
                assert bool((opt.state[p]["exp_avg"] != 0).all()), n
    return m


def check_stats(dev, P, calls=3, seed=0):
    """several add_densification_stats calls (k_density_stats) against numpy: denom and max_radii2D exactly, the accumulated
    norms against float64"""
    from instantsplat_amd.scene import GaussianModel
    r = np.random.RandomState(100 + P + seed)
    m = GaussianModel(0)
    m._xyz = torch.zeros(P, 3, device=dev)
    acc0, den0, rad0 = r.rand(P, 1).astype(np.float32), r.randint(0, 4, (P, 1)).astype(np.float32), r.randint(0, 30, P).astype(np.float32)
    m.xyz_gradient_accum, m.denom, m.max_radii2D = (torch.from_numpy(a.copy()).to(dev) for a in (acc0, den0, rad0))
    a32, a64, den, rad = acc0.copy(), acc0.astype(np.float64), den0.copy(), rad0.copy()
    for k in range(calls):
        g = (r.randn(P, 3) * 10.0 ** r.randint(-6, 1, (P, 1))).astype(np.float32)
        radii = np.where(r.rand(P) < 0.6, r.randint(1, 50, P), 0).astype(np.int32)
        f = radii > 0
        vs = torch.zeros(P, 3, device=dev, requires_grad=True)
        vs.grad = torch.from_numpy(g).to(dev)
        if k % 2 == 0:
            m.add_densification_stats(vs, torch.from_numpy(f).to(dev), radii=torch.from_numpy(radii).to(dev))
            rad[f] = np.maximum(rad[f], radii[f].astype(np.float32))
        else:   # the reference's signature: no radii, max_radii2D untouched
            m.add_densification_stats(vs, torch.from_numpy(f).to(dev))
        n32 = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
        a32[f, 0] += n32[f]
        a64[f, 0] += np.sqrt(g[f, 0].astype(np.float64) ** 2 + g[f, 1].astype(np.float64) ** 2)
        den[f] += 1
    assert np.array_equal(m.denom.cpu().numpy(), den)
    assert np.array_equal(m.max_radii2D.cpu().numpy(), rad)
    return hold_computed("density stats accum", m.xyz_gradient_accum.cpu().numpy(), a32, a64)


def check_reset_opacity(dev, P, optimizer="pp", seed=0):
    c = make_case(P, "mixed", sh_degree=0, seed=seed)
    m = build_model(c, dev, optimizer)
    old = m._opacity
    others = {n: getattr(m, ATTR[n]) for n in PARAM_NAMES if n != "opacity"}
    m.reset_opacity()
    o64 = c["opacity"].astype(np.float64)
    x64 = np.minimum(_sigmoid(o64), 0.01)
    ref64 = np.log(x64 / (1 - x64))
    x32 = np.minimum(_sigmoid(c["opacity"]), np.float32(0.01)).astype(np.float32)
    ref32 = np.log(x32 / (np.float32(1) - x32))
    assert m._opacity is not old and m._opacity.requires_grad and m._opacity.shape == (P, 1)
    st = m.optimizer.state[m._opacity]
    assert old not in m.optimizer.state and int(st["step"]) == 3
    assert not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any()) and st["exp_avg"].shape == (P, 1)
    assert [g for g in m.optimizer.param_groups if g["name"] == "opacity"][0]["params"][0] is m._opacity
    for n, p in others.items():   # nothing else moved
        assert getattr(m, ATTR[n]) is p and np.array_equal(bits(p.detach().cpu().numpy()), bits(c[n]))
    got = m._opacity.detach().cpu().numpy()
    assert bool((_sigmoid(got.astype(np.float64)) <= 0.0100001).all())
    return hold_computed("density reset opacity", got, ref32, ref64)


def check_rejects(dev):
    """bad sizes, N < 1, a null noise pointer while something is split: negative codes from the entry points, exceptions from
    the Python layer"""
    import ctypes
    from instantsplat_amd import _lib, density
    L = _lib.lib()
    assert L.mi355gs_density_scratch_bytes(0, 2) == 0 and L.mi355gs_density_scratch_bytes(10, 0) == 0
    assert L.mi355gs_density_scratch_bytes(10, 9) == 0 and L.mi355gs_density_scratch_bytes(2 ** 30, 2) == 0
    assert L.mi355gs_density_scratch_bytes(10, 2) > 0
    c = make_case(65, "all_split", sh_degree=0)
    m = build_model(c, dev, "pp")
    P = 65
    scratch = torch.empty(int(L.mi355gs_density_scratch_bytes(P, 2)), dtype=torch.uint8, device=dev)
    code = torch.empty(P, dtype=torch.int32, device=dev)
    p = _lib.ptr
    plan = lambda P_, N_, flags: L.mi355gs_density_plan(
        _lib.stream_ptr(dev), P_, N_, flags, p(m.xyz_gradient_accum), p(m.denom), None, 0, None, p(m.max_radii2D), p(m._scaling), p(m._opacity),
        MAX_GRAD, 0.02, MIN_OPACITY, 0.0, 0.2, 1.6, p(code), p(scratch), None)
    assert plan(0, 2, 7) < 0 and plan(-3, 2, 7) < 0 and plan(P, 0, 7) < 0 and plan(P, 9, 7) < 0 and plan(P, 2, 0) < 0 and plan(P, 2, 16) < 0
    assert plan(P, 2, 7) == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    PTR = ctypes.c_void_p * density.N_TENSORS
    ins = [None] * density.N_TENSORS
    for k, n in enumerate(PARAM_NAMES):
        ins[k] = getattr(m, ATTR[n]).detach()
    outs = [None if t is None else torch.empty((3 * P,) + tuple(t.shape[1:]), device=dev) for t in ins]
    apply = lambda N_, noise, rows, n_sel, out_rows: L.mi355gs_density_apply(
        _lib.stream_ptr(dev), P, N_, 7, 0, p(code), p(scratch), p(noise), rows, n_sel, 1.6, PTR(*[p(t) for t in ins]),
        PTR(*[p(t) for t in outs]), out_rows)
    noise = torch.zeros(2 * P, 3, device=dev)
    assert apply(2, None, 0, P, 2 * P) < 0            # something is split and there is no noise
    assert apply(2, noise, 2 * P - 1, P, 2 * P) < 0   # ... or too little of it
    assert apply(0, noise, 2 * P, P, 2 * P) < 0 and apply(2, noise, 2 * P, P, -1) < 0 and apply(2, noise, 2 * P, P + 1, 2 * P) < 0
    assert apply(2, noise, 2 * P, P, 2 * P) == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert L.mi355gs_reset_opacity(_lib.stream_ptr(dev), 0, p(m._opacity), None, None) < 0
    assert L.mi355gs_density_stats(_lib.stream_ptr(dev), P, p(m._xyz), 1, None, None, p(m.xyz_gradient_accum), p(m.denom), None) < 0
    import pytest
    with pytest.raises(ValueError):
        m.densify_and_split(torch.zeros(P, 1, device=dev), MAX_GRAD, EXTENT, N=0)
    with pytest.raises(ValueError):
        m.densify_and_split(torch.zeros(P, 1, device=dev), MAX_GRAD, EXTENT, N=9)
    with pytest.raises(ValueError):   # too few normal samples for what is split
        m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None, clone_and_split=True, noise=torch.zeros(3, 3, device=dev))
    with pytest.raises(ValueError):
        m.prune_points(torch.zeros(P + 1, dtype=torch.bool, device=dev))
    assert m._xyz.shape[0] == P   # a refused call leaves the model as it was


def check_missing_radii(dev):
    """A model that carries no max_radii2D (a loaded PLY with training_setup: the empty placeholder).  Without max_screen_size the
    as-written densify_and_prune does not need the radii and must not read them; with it the call is refused, by the Python layer
    and by the entry point (a null max_radii with SCREEN in the prune-only form)."""
    import pytest
    from instantsplat_amd import _lib
    c = make_case(257, "mixed", sh_degree=0, max_screen_size=None, seed=9)
    s32, tot = restate(c, "prune", np.float32)
    m = build_model(c, dev, "pp")
    m.max_radii2D = torch.empty(0)
    got = m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None)
    assert got["new_P"] == tot["new_P"] == m._xyz.shape[0] and 0 < tot["new_P"] < 257
    assert np.array_equal(bits(m._xyz.detach().cpu().numpy()), bits(s32.t["xyz"]))
    assert np.array_equal(bits(m.xyz_gradient_accum.cpu().numpy()), bits(s32.accum))
    assert m.max_radii2D.numel() == 0   # nothing to compact: left as it was
    m = build_model(c, dev, "pp")
    m.max_radii2D = torch.empty(0)
    with pytest.raises(RuntimeError, match="max_radii2D"):
        m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, 20)
    assert m._xyz.shape[0] == 257
    got = m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, 20, clone_and_split=True, noise=torch.from_numpy(c["noise"]).to(dev))
    assert got["new_P"] == restate(dict(c, max_screen_size=20), "seq", np.float32)[1]["new_P"]   # the sequence sees radii of zero whatever the model holds
    L, p, P = _lib.lib(), _lib.ptr, 257
    m = build_model(c, dev, "pp")
    scratch = torch.empty(int(L.mi355gs_density_scratch_bytes(P, 2)), dtype=torch.uint8, device=dev)
    code = torch.empty(P, dtype=torch.int32, device=dev)
    plan = lambda flags, radii: L.mi355gs_density_plan(
        _lib.stream_ptr(dev), P, 2, flags, None, None, None, 0, None, p(radii), p(m._scaling), p(m._opacity),
        MAX_GRAD, 0.02, MIN_OPACITY, 20.0, 0.2, 1.6, p(code), p(scratch), None)
    assert plan(4 | 8, None) < 0 and plan(4 | 8, m.max_radii2D) == 0 and plan(4, None) == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ golden
# (tag: P, family, sh_degree, N, max_screen_size, optimizer) of the cases tests/golden/make_golden_density.py records
GOLDEN_CASES = {"p65_sh3_pp": (65, "mixed", 3, 2, 20, "pp"), "p257_sh0_adam": (257, "mixed", 0, 3, None, "adam")}
GOLDEN_KEYS = PARAM_NAMES + tuple("m_" + n for n in PARAM_NAMES) + tuple("v_" + n for n in PARAM_NAMES) + ("accum", "denom", "max_radii")


def golden_case(tag):
    P, family, sh, N, screen, optimizer = GOLDEN_CASES[tag]
    return make_case(P, family, sh_degree=sh, N=N, max_screen_size=screen, seed=3), optimizer


def load_golden(tag, mode):
    z = np.load(GOLDEN)
    c, _ = golden_case(tag)
    assert np.array_equal(z[f"{tag}/input_checksum"], input_checksum(c)), "the golden file was recorded for other inputs"
    return {k: z[f"{tag}/{mode}/{k}"] for k in GOLDEN_KEYS}, z


def input_checksum(c):
    return np.array([np.float64(np.sum(c[k].astype(np.float64))) for k in sorted(c) if isinstance(c[k], np.ndarray)])


def check_golden_restatement(tag, mode):
    """no device: the float32 numpy restatement against the reference's own (torch) result — order and copied values to the bit.
    The children's positions and scalings go through exp / log / sqrt of two libraries: each side is allowed 2 ulps of the
    tensor's largest magnitude from the exact value (one for the library function feeding the result, one for the result's own
    roundings), so the two may be 4 ulps apart; measured: 1.0 ulp at worst over all golden cases.  This is a cross-check of the
    two references, not the device's bound (hold_computed)."""
    c, _ = golden_case(tag)
    g, z = load_golden(tag, mode)
    s32, tot = restate(c, mode, np.float32)
    assert int(z[f"{tag}/{mode}/new_P"]) == tot["new_P"]
    ref = dict(s32.t)
    ref["accum"], ref["denom"], ref["max_radii"] = s32.accum, s32.denom, s32.max_radii
    for k in GOLDEN_KEYS:
        a, b = g[k].reshape(ref[k].shape), ref[k]
        if k in ("xyz", "scaling"):
            assert float(np.abs(a.astype(np.float64) - b).max(initial=0.0)) <= 4 * _ulp(b), k
        else:
            assert np.array_equal(bits(a), bits(b)), k


def check_golden_reset(dev, tag):
    c, optimizer = golden_case(tag)
    z = np.load(GOLDEN)
    m = build_model(c, dev, optimizer)
    m.reset_opacity()
    o64 = c["opacity"].astype(np.float64)
    x64 = np.minimum(_sigmoid(o64), 0.01)
    st = m.optimizer.state[m._opacity]
    assert not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any())
    assert np.array_equal(z[f"{tag}/reset/m_opacity"], st["exp_avg"].cpu().numpy())
    return hold_computed("density reset opacity (golden)", m._opacity.detach().cpu().numpy(), z[f"{tag}/reset/opacity"], np.log(x64 / (1 - x64)))


# ---------------------------------------------------------------------------------------------------------------- end to end
# training(syn_pointmap(3, 10, 8, W, H, seed=2), iterations=6, run_ahead=False, opt=<check_training's>) in the deterministic mode,
# run on the commit BEFORE density control existed: first / last loss and the float64 sum of every parameter tensor, as hex
# floats.  "cuda": MI355X at 48 x 64; "cpu": the emulated kernels at 24 x 32.
PARENT_RECORD = {
    "cuda": {"first_loss": "0x1.4ee8be0000000p-7", "last_loss": "0x1.2901c20000000p-7", "_xyz": "-0x1.f6d465d790000p+7",
             "_features_dc": "-0x1.9dd07a5600000p+4", "_features_rest": "0x0.0p+0", "_opacity": "-0x1.06d8e17400000p+9",
             "_scaling": "-0x1.9e70986b00000p+9", "_rotation": "0x1.da839e038ae80p+7", "P": "0x1.2254eb77be000p+4"},
    "cpu": {"first_loss": "0x1.3d43320000000p-7", "last_loss": "0x1.29b53e0000000p-7", "_xyz": "-0x1.f6abe55df0000p+7",
            "_features_dc": "-0x1.ba3d586d00000p+4", "_features_rest": "0x0.0p+0", "_opacity": "-0x1.06c22c3e00000p+9",
            "_scaling": "-0x1.9ee1dcb780000p+9", "_rotation": "0x1.db2fc0b559000p+7", "P": "0x1.2254ec33be000p+4"},
}


def check_training(dev, tmp_path, H=48, W=64, iterations=14):
    """training(densify=True) through two events and one opacity reset: another P, finite losses, a model that survives
    capture / restore and save_ply / load_ply; training(densify=False) reproduces the loop without the keyword bit for bit."""
    import dataclasses
    from instantsplat_amd import _lib
    from instantsplat_amd.scene import GaussianModel
    from instantsplat_amd.synthetic import syn_pointmap
    from instantsplat_amd.train import training
    make_scene = lambda: syn_pointmap(3, 10, 8, W, H, seed=2)   # 240 Gaussians
    scene = make_scene()
    o = dataclasses.replace(opt_params(), densification_interval=4, densify_from_iter=2, opacity_reset_interval=6, densify_until_iter=13,
                            densify_grad_threshold=1e-7)
    seen = []
    run_dir = os.path.join(str(tmp_path), "run")
    out = training(scene, dev, iterations=iterations, run_ahead=False, opt=o, densify=True, densify_clone_and_split=True,
                   after_setup=lambda st: seen.append(int(st.gaussians._xyz.shape[0])), model_path=run_dir, checkpoint_iterations=(9,))
    g = out["state"].gaussians
    P1 = int(g._xyz.shape[0])
    print(f"densify=True: P {seen[0]} -> {P1}, events {out['density_events']}, first loss {out['first_loss']:.5f}, last {out['last_loss']:.5f}")
    assert len(out["density_events"]) >= 2 and out["opacity_resets"] >= 1
    assert P1 != seen[0] and P1 > 0
    assert np.isfinite(out["first_loss"]) and np.isfinite(out["last_loss"]) and np.isfinite(out["psnr_after"])
    for n_ in PARAM_NAMES:
        assert getattr(g, ATTR[n_]).shape[0] == P1 and bool(torch.isfinite(getattr(g, ATTR[n_])).all())
    assert g.xyz_gradient_accum.shape == (P1, 1) and g.denom.shape == (P1, 1) and g.max_radii2D.shape == (P1,)
    assert g.optimizer.param_groups[0]["per_point_lr"].shape == (P1, 1)
    # capture / restore
    cap = g.capture()
    g2 = GaussianModel(g.max_sh_degree)
    g2.restore(cap, o, confidence_lr=g.per_point_lr)
    for n_ in PARAM_NAMES:
        assert torch.equal(getattr(g2, ATTR[n_]), getattr(g, ATTR[n_]))
        assert torch.equal(g2.optimizer.state[getattr(g2, ATTR[n_])]["exp_avg"], g.optimizer.state[getattr(g, ATTR[n_])]["exp_avg"])
    assert torch.equal(g2.denom, g.denom) and torch.equal(g2.max_radii2D, g.max_radii2D)
    # save_ply / load_ply
    path = os.path.join(str(tmp_path), "point_cloud.ply")
    g.save_ply(path)
    g3 = GaussianModel(g.max_sh_degree)
    g3.load_ply(path, device=dev)
    for n_ in PARAM_NAMES:
        assert torch.equal(getattr(g3, ATTR[n_]).detach(), getattr(g, ATTR[n_]).detach()), n_
    # resume from the checkpoint written between the second and the third event: the run continues at the checkpoint's P, with
    # the per-point rates its optimizer state holds, through the third event
    res = training(make_scene(), dev, iterations=iterations, run_ahead=False, opt=o, densify=True, densify_clone_and_split=True,
                   start_checkpoint=os.path.join(run_dir, "chkpnt9.pth"))
    gr = res["state"].gaussians
    P_chk = out["density_events"][1][1]["new_P"]
    assert [it for it, _ in res["density_events"]] == [12] and res["density_events"][0][1]["originals"] <= P_chk
    Pr = int(gr._xyz.shape[0])
    assert Pr == res["density_events"][0][1]["new_P"] and np.isfinite(res["last_loss"])
    assert gr.per_point_lr is gr.optimizer.param_groups[0]["per_point_lr"] and gr.per_point_lr.shape == (Pr, 1)
    # densify=False: today's loop, bit for bit (deterministic backward)
    L = _lib.lib()
    was = L.mi355gs_tune_deterministic(-1)
    L.mi355gs_tune_deterministic(1)
    try:
        a = training(make_scene(), dev, iterations=6, run_ahead=False, opt=o)
        b = training(make_scene(), dev, iterations=6, run_ahead=False, opt=o, densify=False)
    finally:
        L.mi355gs_tune_deterministic(was)
    assert a["last_loss"] == b["last_loss"] and a["first_loss"] == b["first_loss"]
    # ... and what the commit before the feature left on the same seed (PARENT_RECORD): to the bit on the device; on the emulated
    # tier within 1e-5, because there torch's CPU kernels take part (create_from_pcd, the sums below) and their vector width, and
    # with it last bits, follows the host's CPU — the suite's recorded trajectories hold 6e-7 to 8e-6 across hosts
    want = PARENT_RECORD["cuda" if dev.type == "cuda" else "cpu"]
    got = {"first_loss": float(b["first_loss"]), "last_loss": float(b["last_loss"])}
    for n_ in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "P"):
        got[n_] = float(getattr(b["state"].gaussians, n_).detach().double().sum().cpu())
    for k, v in want.items():
        w = float.fromhex(v)
        print(f"default path {k}: {got[k]!r} recorded {w!r}")
        assert got[k] == w if dev.type == "cuda" else abs(got[k] - w) <= 1e-5 * abs(w), (k, got[k], w)
    for n_ in PARAM_NAMES:
        assert torch.equal(getattr(a["state"].gaussians, ATTR[n_]), getattr(b["state"].gaussians, ATTR[n_])), n_
