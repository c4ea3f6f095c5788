"""Generates tests/golden/density_vectors.npz by EXECUTING the reference's own GaussianModel methods (scene/gaussian_model.py:
280-283 and 328-477) on the CPU, the way make_golden.py does it: the module is executed from its file with `.cuda()` /
device="cuda" rewritten in memory, stand-ins for the imports that do not exist here, and no reference text is written anywhere.
Possible only where the reference tree is present; the vectors are committed.

For every case of tests/density_cases.GOLDEN_CASES (the inputs come from density_cases.make_case, so the file holds results and
a checksum of the inputs only) it records, each from a fresh model holding the same rows and a stepped optimizer's state:

  clone        densify_and_clone(grads, max_grad, extent)            on its own
  split        densify_and_split(grads, max_grad, extent, N)         on its own
  prune_mask   prune_points(mask)                                    on its own
  prune        densify_and_prune(...) as written (:464-465 are comments: it only prunes)
  seq          densify_and_prune(...) with :464-465 restored (the comment marks removed in memory; split with the case's N)
  reset        reset_opacity()

with torch.optim.Adam (training_setup) or the reference's PerPointAdam (training_setup_pp).  Nothing is stepped afterwards:
with the per-point optimizer the reference cannot (its per-point rates are never resized), so the record ends at the surgery.

Two things about the reference as it stands, handled here and said in README_density.md:
  * its optimizer holds a seventh group, the poses [V,7]; `_prune_optimizer` and `cat_tensors_to_optimizer` loop over ALL groups
    and index that table with the Gaussians' mask (or look its name up among the Gaussians' tensors), so the methods fail
    while it is there.  The group is taken out of the optimizer before a method is called.
  * `torch.normal(mean, std)` is replaced by `mean + std * z` for the case's recorded z.

Run:  python tests/golden/make_golden_density.py
"""
import os
import sys
import types
from argparse import ArgumentParser

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
OUT = os.path.join(HERE, "density_vectors.npz")

from tests import density_cases as dc  # noqa: E402

knn_mod = types.ModuleType("simple_knn._C")
knn_mod.distCUDA2 = lambda pts: None
sys.modules["simple_knn"] = types.ModuleType("simple_knn")
sys.modules["simple_knn._C"] = knn_mod
ply_mod = types.ModuleType("plyfile")
ply_mod.PlyData = ply_mod.PlyElement = object
sys.modules["plyfile"] = ply_mod
scene_pkg = types.ModuleType("scene")
scene_pkg.__path__ = [os.path.join(REF, "scene")]
sys.modules["scene"] = scene_pkg
gm_path = os.path.join(REF, "scene", "gaussian_model.py")
gm_src = open(gm_path).read().replace(".cuda()", "").replace('device="cuda"', 'device="cpu"')
gm = types.ModuleType("ref_gaussian_model")
exec(compile(gm_src, gm_path, "exec"), gm.__dict__)
# the sequence with :464-465 restored: the same module text with the comment marks of those two lines removed, in memory
import re  # noqa: E402
seq_lines = gm_src.split("\n")
for ln in (464, 465):
    assert re.match(r"^\s*# self\.densify_and_", seq_lines[ln - 1]), (ln, seq_lines[ln - 1])
    seq_lines[ln - 1] = re.sub(r"^(\s*)# ", r"\1", seq_lines[ln - 1])
seq_src = "\n".join(seq_lines)
gm_seq = types.ModuleType("ref_gaussian_model_seq")
exec(compile(seq_src, gm_path, "exec"), gm_seq.__dict__)
from arguments import OptimizationParams as RefOptimizationParams  # noqa: E402

_zeros, _normal, _empty_cache = torch.zeros, torch.normal, torch.cuda.empty_cache
torch.zeros = lambda *a, **k: _zeros(*a, **{kk: vv for kk, vv in k.items() if kk != "device"})   # general_utils: device='cuda'
torch.cuda.empty_cache = lambda: None


def ref_model(module, c, optimizer):
    m = module.GaussianModel(c["sh_degree"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for n in dc.PARAM_NAMES:
        setattr(m, dc.ATTR[n], torch.nn.Parameter(t(c[n]).clone().requires_grad_(True)))
    m.spatial_lr_scale = 1.0
    m.P = torch.zeros(2, 7).requires_grad_(True)
    o = RefOptimizationParams(ArgumentParser())
    o.iterations = 1000
    if optimizer == "pp":
        m.training_setup_pp(o, t(c["per_point_lr"]).clone())
    else:
        m.training_setup(o)
    assert m.percent_dense == dc.PERCENT_DENSE
    m.optimizer.param_groups[:] = [g for g in m.optimizer.param_groups if g["name"] != "pose"]   # see the module docstring
    for n in dc.PARAM_NAMES:
        m.optimizer.state[getattr(m, dc.ATTR[n])] = {"step": torch.tensor(3.0) if optimizer == "adam" else 3,
                                                     "exp_avg": t(c["m_" + n]).clone(), "exp_avg_sq": t(c["v_" + n]).clone()}
    m.xyz_gradient_accum, m.denom, m.max_radii2D = t(c["accum"]).clone(), t(c["denom"]).clone(), t(c["max_radii"]).clone()
    split = m.densify_and_split   # the restored call of :465 takes the method's default N: give it the case's
    m.densify_and_split = lambda grads, threshold, extent, N=c["N"]: split(grads, threshold, extent, N=N)
    return m


def record(out, prefix, m):
    for n in dc.PARAM_NAMES:
        p = getattr(m, dc.ATTR[n])
        st = m.optimizer.state[p]
        assert len(m.optimizer.state) == len(dc.PARAM_NAMES)
        out[f"{prefix}/{n}"] = p.detach().numpy().copy()
        out[f"{prefix}/m_{n}"], out[f"{prefix}/v_{n}"] = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
    out[f"{prefix}/accum"], out[f"{prefix}/denom"] = m.xyz_gradient_accum.numpy().copy(), m.denom.numpy().copy()
    out[f"{prefix}/max_radii"] = m.max_radii2D.numpy().copy()
    out[f"{prefix}/new_P"] = np.array(m._xyz.shape[0])


out = {}
for tag in dc.GOLDEN_CASES:
    c, optimizer = dc.golden_case(tag)
    out[f"{tag}/input_checksum"] = dc.input_checksum(c)
    z = torch.from_numpy(c["noise"])
    torch.normal = lambda mean, std: mean + std * z[:std.shape[0]]
    grads = torch.from_numpy(c["accum"]) / torch.from_numpy(c["denom"])
    grads[grads.isnan()] = 0.0
    for mode in dc.MODES:
        m = ref_model(gm_seq if mode == "seq" else gm, c, optimizer)
        if mode == "clone":
            m.densify_and_clone(grads, dc.MAX_GRAD, dc.EXTENT)
        elif mode == "split":
            m.densify_and_split(grads, dc.MAX_GRAD, dc.EXTENT, N=c["N"])
        elif mode == "prune_mask":
            m.prune_points(torch.from_numpy(c["mask"]))
        else:
            m.densify_and_prune(dc.MAX_GRAD, dc.MIN_OPACITY, dc.EXTENT, c["max_screen_size"])
        record(out, f"{tag}/{mode}", m)
        print(tag, mode, "P", c["P"], "->", m._xyz.shape[0])
    m = ref_model(gm, c, optimizer)
    m.reset_opacity()
    record(out, f"{tag}/reset", m)
torch.zeros, torch.normal, torch.cuda.empty_cache = _zeros, _normal, _empty_cache
np.savez_compressed(OUT, **out)
print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")
