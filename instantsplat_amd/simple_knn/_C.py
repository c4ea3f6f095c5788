"""`simple_knn._C.distCUDA2` — mean squared distance to the 3 nearest other points.
Call site being served: reference scene/gaussian_model.py:156."""
import torch

from .. import _lib


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    pts = _lib.f32c(points.float() if points.dtype == torch.float64 else points)   # point clouds read from files are float64
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError("points must have dimensions (num_points, 3)")
    dev = _lib.require_device(pts)
    n = pts.shape[0]
    out = torch.zeros(n, dtype=torch.float32, device=dev)
    _lib.call(dev, "knn_dist2", _lib.STREAM, n, pts, out, _lib.scratch(dev, "knn_scratch_bytes", n, what=None))
    return out
