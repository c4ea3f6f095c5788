"""Owners of the library's handles (include/mi355gs.h mi355gs_<prefix>_workspace_bytes / _create / _destroy).

  LibraryHandle       `handle`, `workspace`, the query-then-create sequence and a `close()` that is safe to call twice, from
                      `__del__` and during interpreter shutdown — FusedTrainer and AlignProblem use it for ownership
  FrozenSceneHandle   a handle over the frozen Gaussians' six raw parameter tensors, one image size and an instance capacity:
                      FusedPoseTracker ("tracker") and FusedPathRenderer ("path") are this plus their own calls
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib


class LibraryHandle:
    prefix = None      # "tracker": mi355gs_tracker_workspace_bytes / _create / _destroy
    handle = None      # the library's pointer as an int (None once closed)
    workspace = None   # the device block the handle's buffers live in

    def _open(self, dev, sizes, create_args, refused=None, failed=None):
        """workspace = mi355gs_<prefix>_workspace_bytes(*sizes) bytes on `dev`, handle = mi355gs_<prefix>_create(*create_args(workspace)).
        `refused` is raised when the library takes the sizes for too large (a workspace of 0 bytes) — before create is called —
        and `failed` when create returns NULL."""
        L = _lib.lib()
        nbytes = int(getattr(L, f"mi355gs_{self.prefix}_workspace_bytes")(*sizes))
        if not nbytes:
            raise refused or ValueError(f"mi355gs_{self.prefix}_workspace_bytes rejected the sizes")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in create_args(self.workspace)]
        self.handle = getattr(L, f"mi355gs_{self.prefix}_create")(*args) or None
        if not self.handle:
            raise failed or RuntimeError(f"mi355gs_{self.prefix}_create failed")

    @property
    def _h(self):
        """the handle as a library call takes it"""
        return ctypes.c_void_p(self.handle)

    def close(self):
        handle, self.handle = getattr(self, "handle", None), None
        if handle:
            try:
                getattr(_lib.lib(), f"mi355gs_{self.prefix}_destroy")(ctypes.c_void_p(handle))
            except Exception:  # interpreter shutdown: module globals may already be gone (the handle is host memory only)
                pass

    __del__ = close


class FrozenSceneHandle(LibraryHandle):
    phrase = None   # what the subclass does, for the messages: "fused pose tracking"

    def __init__(self, gaussians, W: int, H: int, capacity: int):
        g = gaussians
        self.params = [t.detach() for t in (g._xyz, g._features_dc, g._features_rest, g._opacity, g._scaling, g._rotation)]
        dev = _lib.require_device(*self.params)
        P = int(self.params[0].shape[0])
        M = 1 + int(self.params[2].shape[1]) if self.params[2].dim() == 3 else 1
        shapes = ((P, 3), (P, 1, 3), (P, M - 1, 3), (P, 1), (P, 3), (P, 4))
        for t, shape in zip(self.params, shapes):   # the library indexes raw pointers with these shapes
            if t.dtype != torch.float32 or tuple(t.shape) != shape:
                raise ValueError(f"{self.phrase} needs float32 parameters of shape {shape}, got {tuple(t.shape)} {t.dtype}")
        self.dev, self.P, self.M, self.W, self.H, self.capacity = dev, P, M, int(W), int(H), int(capacity)
        self._open(dev, (P, self.W, self.H, self.capacity), lambda ws: (P, M, self.W, self.H, self.capacity, *self.params, ws))

    @staticmethod
    def _camera(view, dev):
        proj = view.projection_matrix.to(dev).float().contiguous()
        return proj, math.tan(view.FoVx * 0.5), math.tan(view.FoVy * 0.5)
