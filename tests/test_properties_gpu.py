"""GPU tier, BASELINE sizes (200k Gaussians, 512x512): properties that hold at any size, where the dense
oracle would be too slow to be the checker.
  * forward is run-to-run bit-identical (sorted per-tile lists, no atomics in the forward path);
  * backward is linear in dL/dpixel;
  * with a black background the image is linear in precomputed colours (transmittance does not depend on colour);
  * every per-tile list the binning produces is sorted by (depth, index) and its length matches the tile counts."""

import pytest
import torch

from instantsplat_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
from instantsplat_amd.synthetic import syn_blob
from tests import frame_abi
from tests.util import settings_for

pytestmark = pytest.mark.gpu
P, W, H = 200000, 512, 512


def _scene(gpu, deg=0, seed=0):
    sc = syn_blob(P, W, H, seed=seed)
    st = settings_for(sc.camera, deg, GaussianRasterizationSettings, sc.bg, device=gpu)
    t = dict(means3D=sc.means3D.to(gpu), opacities=torch.sigmoid(sc.opacity_logit).to(gpu), scales=torch.exp(sc.scaling_logit).to(gpu),
             rotations=sc.rotation.to(gpu))
    return sc, st, t


def test_forward_is_bitwise_deterministic(gpu):
    sc, st, t = _scene(gpu, deg=3)
    r = GaussianRasterizer(st)
    with torch.no_grad():
        a, ra = r(means2D=torch.zeros(P, 3, device=gpu), shs=sc.shs.to(gpu), **t)
        b, rb = r(means2D=torch.zeros(P, 3, device=gpu), shs=sc.shs.to(gpu), **t)
    assert torch.equal(a, b) and torch.equal(ra, rb)


def test_backward_is_linear_in_pixel_gradient(gpu):
    sc, st, t = _scene(gpu)
    leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    shs = sc.shs.to(gpu).requires_grad_(True)
    img, _ = GaussianRasterizer(st)(means2D=torch.zeros(P, 3, device=gpu), shs=shs, **leaves)
    g = torch.Generator().manual_seed(5)
    g1, g2 = torch.randn(3, H, W, generator=g).to(gpu), torch.randn(3, H, W, generator=g).to(gpu)
    names = list(leaves) + ["shs"]
    tens = list(leaves.values()) + [shs]
    ga = torch.autograd.grad(img, tens, g1, retain_graph=True)
    gb = torch.autograd.grad(img, tens, g2, retain_graph=True)
    gc = torch.autograd.grad(img, tens, 2.0 * g1 + g2)
    for n, a, b, c in zip(names, ga, gb, gc):
        ref = 2.0 * a + b
        assert float((c - ref).norm() / (ref.norm() + 1e-30)) <= 1e-4, n


def test_image_is_linear_in_precomputed_colours(gpu):
    sc, st, t = _scene(gpu)
    g = torch.Generator().manual_seed(6)
    c1, c2 = torch.rand(P, 3, generator=g).to(gpu), torch.rand(P, 3, generator=g).to(gpu)
    r = GaussianRasterizer(st)
    z = torch.zeros(P, 3, device=gpu)
    with torch.no_grad():
        a = r(means2D=z, colors_precomp=c1, **t)[0]
        b = r(means2D=z, colors_precomp=c2, **t)[0]
        c = r(means2D=z, colors_precomp=c1 + c2, **t)[0]
    assert float((c - (a + b)).abs().max()) <= 2e-5


def test_largest_config_1M_gaussians_1080p(gpu):
    """BASELINE config C4 (1 M Gaussians, 1920x1080, ~7 M instances): forward run-to-run identical, backward linear in
    dL/dpixel and finite — the same size-independent properties, at the largest size the reference quotes."""
    Pn, Wn, Hn = 1000000, 1920, 1080
    sc = syn_blob(Pn, Wn, Hn, seed=3)
    st = settings_for(sc.camera, 0, GaussianRasterizationSettings, sc.bg, device=gpu)
    t = dict(means3D=sc.means3D.to(gpu), opacities=torch.sigmoid(sc.opacity_logit).to(gpu), scales=torch.exp(sc.scaling_logit).to(gpu),
             rotations=sc.rotation.to(gpu))
    r = GaussianRasterizer(st)
    z = torch.zeros(Pn, 3, device=gpu)
    with torch.no_grad():
        a, ra = r(means2D=z, shs=sc.shs.to(gpu), **t)
        b, rb = r(means2D=z, shs=sc.shs.to(gpu), **t)
    assert torch.equal(a, b) and torch.equal(ra, rb)
    assert int((ra > 0).sum()) > Pn // 2
    leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    img, _ = r(means2D=z, shs=sc.shs.to(gpu), **leaves)
    g = torch.Generator().manual_seed(9)
    g1 = torch.randn(3, Hn, Wn, generator=g).to(gpu)
    tens = list(leaves.values())
    ga = torch.autograd.grad(img, tens, g1, retain_graph=True)
    gb = torch.autograd.grad(img, tens, -0.5 * g1)
    for n, x, y in zip(leaves, ga, gb):
        assert bool(torch.isfinite(x).all()), n
        ref = -0.5 * x
        assert float((y - ref).norm() / (ref.norm() + 1e-30)) <= 1e-4, n


def _all_tile_lists_sorted_on_device(frame):
    """Every per-tile list of the kept frame: ascending (depth bits, Gaussian index) keys, no duplicates, and together exactly the
    (Gaussian, tile) pairs of the tile rectangles — checked on the device over the whole instance array at once (scratch
    layouts: csrc/common.h).  -> (instances, per-tile counts)"""
    v = frame_abi.FrameViews.of_last_frame(frame)
    R, P, T, gx = v.R, v.P, v.T, v.gx
    start = v.tile_start.long()
    n = int(start[T])
    assert 0 < n <= R and int(start[0]) == 0
    lst = v.list[:n].long()
    assert int(lst.min()) >= 0 and int(lst.max()) < P
    depth_bits = v.rec.view(torch.int32)[:, 11].long()                            # the record's depth word (non-negative floats: ordered as ints)
    key = (depth_bits[lst] << 32) | lst
    ascending = key[1:] > key[:-1]
    first_of_tile = torch.zeros(n + 1, dtype=torch.bool, device=key.device)
    first_of_tile[start[: T + 1]] = True                                          # list boundaries: no order across them
    bad = ~ascending & ~first_of_tile[1:n]
    assert not bool(bad.any()), int(bad.sum())
    # ... and the lists are exactly the (Gaussian, tile) pairs of the projection kernel's tile rectangles: as many instances as
    # the rectangles have tiles, every entry's rectangle contains its tile (with the lists duplicate-free: a bijection)
    rect = v.rect.long()
    x0, y0, x1, y1 = rect[:, 0] & 0xffff, (rect[:, 0] >> 16) & 0xffff, rect[:, 1] & 0xffff, (rect[:, 1] >> 16) & 0xffff
    area = (x1 - x0).clamp(min=0) * (y1 - y0).clamp(min=0)
    assert int(area.sum()) == n, (int(area.sum()), n)
    tile = torch.searchsorted(start[1:].contiguous(), torch.arange(n, device=key.device), right=True)
    tx, ty = tile % gx, tile // gx
    inside = (x0[lst] <= tx) & (tx < x1[lst]) & (y0[lst] <= ty) & (ty < y1[lst])
    assert bool(inside.all()), int((~inside).sum())
    return n, (start[1:] - start[:-1])


def test_c4_tile_lists_are_sorted(gpu):
    """Sortedness at BASELINE's largest size (C4: 995,328 Gaussians, 1920x1080, 8160 tiles of ~900 keys — the lengths where the
    tile sort takes its two-run form for a fifth of the tiles): all 7.3 M instances in ascending (depth, index) order per tile."""
    from instantsplat_amd import diff_gaussian_rasterization as dgr
    from instantsplat_amd.gaussian_renderer import render
    from instantsplat_amd.synthetic import syn_pointmap
    from instantsplat_amd.train import setup_training
    st = setup_training(syn_pointmap(12, 288, 288, 1920, 1080, seed=0), gpu)
    g = st.gaussians
    dgr.keep_last_frame(True)
    try:
        for v in (0, 7):
            cam = st.cameras[v]
            with torch.no_grad():
                render(cam, g, st.pipe, st.background, camera_pose=g.get_RT(cam.uid))
            n, counts = _all_tile_lists_sorted_on_device(dgr._LAST_FRAME)
            assert n > 5_000_000 and int(counts.max()) > 1024                     # (some tiles beyond one 1024-key network)
            two_run = int(((counts > 1024) & (counts <= 1536)).sum()) + int(((counts > 512) & (counts <= 768)).sum())
            assert two_run > 500, two_run
    finally:
        dgr.keep_last_frame(False)
