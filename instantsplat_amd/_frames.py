"""What the stages over batches of 8-bit frames share (png.py, jpeg.py, metrics.py, lpips.py, resample.py, init_stage.py): the
argument checks, "which device does this stage run on", the split of N frames into library calls under a byte budget, and
the encoders' loop over those calls."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


def device_of(tensors, default=None):
    """The device a stage runs on: the one device of the CUDA tensors among its arguments, else `default`, else the current one
    (host tensors then take one copy each, `to_device`).  Under the emulator's test mode CPU tensors are used where they are;
    otherwise a missing GPU is an error (there is no CPU fallback)."""
    cuda = {t.device for t in tensors if t.is_cuda}
    if len(cuda) > 1:
        raise ValueError(f"tensors on different devices: {sorted(str(d) for d in cuda)}")
    if cuda:
        return cuda.pop()
    if default is not None:
        return default
    if _lib._TEST_MODE:
        return torch.device("cpu")
    if not torch.cuda.is_available():
        raise RuntimeError(_lib.gpu_only())
    return torch.device("cuda", torch.cuda.current_device())


def to_device(t: torch.Tensor, dev) -> torch.Tensor:
    """`t`, contiguous, on `dev`: device tensors stay; host tensors (pinned or not) take ONE host-to-device copy."""
    if t.device != dev:
        t = t.to(dev, non_blocking=t.is_pinned())
    return t if t.is_contiguous() else t.contiguous()


def check_frames(who: str, frames, verb: str = "encodes", arg: str = "frames"):
    """uint8 [N,H,W,3] or [H,W,3], contiguous, on the device -> (frames as [N,H,W,3], N, H, W); ValueError otherwise, in the name
    of the public function `who`."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError(f"{who} takes a uint8 [N,H,W,3] or [H,W,3] tensor, got "
                         f"{tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames)} {getattr(frames, 'dtype', '')}")
    if not frames.is_cuda and not _lib._TEST_MODE:
        raise ValueError(_lib.gpu_only(f"{who} {verb}") + f": pass {arg}.to(device)")
    if not frames.is_contiguous():
        raise ValueError(f"{who} takes a contiguous tensor")
    if frames.dim() == 3:
        frames = frames[None]
    N, H, W = (int(s) for s in frames.shape[:3])
    if H <= 0 or W <= 0:
        raise ValueError(f"empty {arg}: {H} x {W}")
    return frames, N, H, W


def check_pair(who: str, renders, gts):
    """two uint8 [N,H,W,3] tensors of one shape -> (N, H, W); ValueError otherwise, in the name of the public function `who`."""
    for t in (renders, gts):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
            raise ValueError(f"{who} takes two uint8 [N,H,W,3] tensors, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)} {getattr(t, 'dtype', '')}")
    if renders.shape != gts.shape:
        raise ValueError(f"renders {tuple(renders.shape)} and ground truth {tuple(gts.shape)} differ in shape")
    return tuple(int(s) for s in renders.shape[:3])


def pair_on_device(renders, gts, *also, default=None):
    """-> (renders, gts, dev): both contiguous on the one device the scoring runs on (`device_of`), which every tensor of `also`
    must share."""
    dev = device_of((renders, gts), default)
    a, b = to_device(renders, dev), to_device(gts, dev)
    return a, b, _lib.require_device(a, b, *also)


def frames_per_call(fits, cap: int, estimate: int) -> int:
    """The largest n <= cap with fits(n), searched from `estimate` (the padding of the library's buffers makes a division
    of the budget by one frame's bytes an estimate only): down while it does not fit, then up while one more does.  At least 1,
    whatever fits(1) says: one frame per call is always tried."""
    n = max(1, min(cap, int(estimate)))
    while n > 1 and not fits(n):
        n -= 1
    while n < cap and fits(n + 1):
        n += 1
    return n


def host_bytes(buf: torch.Tensor, nbytes: int) -> torch.Tensor:
    """the first nbytes of a device buffer that the next call reuses, on the host (a copy of its own under the emulator's test
    mode, where .cpu() aliases the buffer)"""
    files = buf[:nbytes].cpu()
    return files if buf.is_cuda else files.clone()


def encode_in_calls(N: int, per_call: int, buffers, encode_call) -> dict:
    """The encoders' loop: N frames in calls of per_call.  buffers(n) -> the device buffers of a call of n frames, allocated
    again only when n changes (the last, shorter call); encode_call(first, n, *buffers) -> (offsets int64 numpy [n+1] within
    the call, from its one read-back; [host tensors holding the call's files back to back]).
    -> dict(stream = the N files back to back, offsets int64 [N+1])."""
    parts, offsets, base, bufs = [], [np.zeros(1, np.int64)], 0, None
    for first in range(0, N, per_call):
        n = min(per_call, N - first)
        if bufs is None or n != per_call:
            bufs = buffers(n)
        o, files = encode_call(first, n, *bufs)
        parts += files
        offsets.append(o[1:] + base)
        base += int(o[-1])
    return dict(stream=parts[0] if len(parts) == 1 else torch.cat(parts), offsets=np.concatenate(offsets))


def write_stream_files(paths, frames, encode, **kw) -> None:
    """Encode frames (as `encode` takes them) and write file i to paths[i] with one write each."""
    paths = list(paths)
    n = 1 if isinstance(frames, torch.Tensor) and frames.dim() == 3 else len(frames)
    if len(paths) != n:
        raise ValueError(f"{len(paths)} paths for {n} frames")
    enc = encode(frames, **kw)
    data, offsets = memoryview(enc["stream"].numpy()), enc["offsets"]
    for i, path in enumerate(paths):
        with open(path, "wb") as fh:
            fh.write(data[int(offsets[i]):int(offsets[i + 1])])
