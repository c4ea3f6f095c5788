"""tests/golden/interp_path_vectors.npz: the reference's own `generate_interpolated_path` (utils/camera_utils.py:127-182, with
`viewmatrix` / `normalize`) and `save_interpolate_pose` (render.py:36-56), executed from /root/reference (build container only;
needs scipy).  The two matplotlib plots of save_interpolate_pose are bound to a no-op.  Only arrays are stored (float64):
  interp_<tag>_org        [V,4,4]  seeded random rigid world-to-camera poses (the pose_optimized.npy the reference reads)
  interp_<tag>_segments   [V-1, n_interp, 3, 4]  generate_interpolated_path(org[i:i+2], n_interp), n_interp = int(10 * 30 / V)
  interp_<tag>_path       [n_interp * (V-1) + 1, 4, 4]  the pose_interpolated.npy the reference writes
tags: v2, v3, v5, v12 (V views) and zero_t (two views whose translations are both zero).
Run:  python tests/golden/make_golden_interp.py"""
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import scipy
import scipy.interpolate  # noqa: F401  (the reference says `scipy.interpolate.splprep` after a bare `import scipy`)

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

ns = {"np": np, "scipy": scipy, "visualizer": lambda *a, **k: None}
cu = os.path.join(REF, "utils", "camera_utils.py")
for name, src in ref_loader.function_sources(cu, {"generate_interpolated_path", "viewmatrix", "normalize"}).items():
    exec(compile(src, cu, "exec"), ns)
rp = os.path.join(REF, "render.py")
for name, src in ref_loader.function_sources(rp, {"save_interpolate_pose"}).items():
    exec(compile(src, rp, "exec"), ns)

rng = np.random.default_rng(20)


def rand_w2c(zero_t=False):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    m = np.eye(4)
    m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                 [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                 [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    if not zero_t:
        m[:3, 3] = rng.standard_normal(3) * 2.0
    return m


out = {}
for tag, V, zero_t in (("v2", 2, False), ("v3", 3, False), ("v5", 5, False), ("v12", 12, False), ("zero_t", 2, True)):
    org = np.stack([rand_w2c(zero_t) for _ in range(V)])
    n_interp = int(10 * 30 / V)
    out[f"interp_{tag}_org"] = org
    out[f"interp_{tag}_segments"] = np.stack([ns["generate_interpolated_path"](poses=org[i:i + 2], n_interp=n_interp) for i in range(V - 1)])
    with tempfile.TemporaryDirectory() as td:
        os.makedirs(os.path.join(td, "pose", "ours_7"))
        np.save(os.path.join(td, "pose", "ours_7", "pose_optimized.npy"), org)
        ns["save_interpolate_pose"](Path(td), 7, V)
        out[f"interp_{tag}_path"] = np.load(os.path.join(td, "pose", "ours_7", "pose_interpolated.npy"))
    assert out[f"interp_{tag}_path"].shape == (n_interp * (V - 1) + 1, 4, 4)
assert all(v.dtype == np.float64 for v in out.values())
np.savez_compressed(os.path.join(HERE, "interp_path_vectors.npz"), **out)
print("wrote", len(out), "arrays:", {k: v.shape for k, v in out.items() if k.endswith("_path")})
