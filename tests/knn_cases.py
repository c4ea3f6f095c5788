"""The 3-NN kernel (csrc/knn.hip, `mi355gs_knn_dist2`, served as simple_knn._C.distCUDA2) on every search path and grid edge
against the float64 k-d tree (oracle/knn_ref.py): case builders and checks shared by the emulated (CPU) and the GPU test files.

The builders restate the kernel's grid in numpy float32, operation by operation (no multiply-add pair occurs in it, so
contraction cannot change it, and both divisions are correctly rounded), and from it and a float64 k-d tree they certify, on
the CPU and before the device is called, which path every point of a cloud takes:
    the search of a point whose true third neighbour is d3 away ends at ring ceil(d3 / h): every point within r h of it lies
    inside the cube of ring r, and the exit needs b2 <= (r h)^2; it goes to the exhaustive fallback iff d3 > KNN_MAX_RING h.
A point is certified for a ring when d3 / h is at least 1e-3 away from an integer (or d3 == 0: ring 0), for the fallback when
d3 > 6.001 h.  The margin is far above the 1e-4 by which the kernel shrinks its reach to cover the rounding of the cell indices.

The limit is derived, not measured.  The kernel returns the mean of the three smallest of its own computed squared distances.
With u = 2^-24 a squared distance carries at most 5 u relative error (one rounded difference per axis: 2 u on its square, the
square's rounding, two additions; contraction only lowers this), the mean at most 3 u more: 8 u on every point's value.  Every
point is held, on its own, to LIMIT = 2^-20 = 16 u (the factor 2 covers the second-order terms and the oracle's rounding of
its float64 result to float32); where the oracle says 0 the kernel must say exactly 0."""
import functools
import os
import re

import numpy as np
import torch
from scipy.spatial import cKDTree

from oracle import knn_ref
from tests import ops_util

LIMIT = 2.0 ** -20
F = np.float32

# the constants of csrc/knn.hip that the restated grid and the certificates are built on (source_constants() reads the file)
KNN_MAX_RING = 6
CELL_GROWTH = "1.0001"
EXTENT_FLOOR = "1e-20"
RESOLUTION = ("12", "256", "4", "4")          # while (G * G * 12 < N && G < 256) ++G; return G < 4 ? 4 : G
BBOX_SPLIT = ("1024", "4095", "4096")         # bbox_blocks = min(1024, (N + 4095) / 4096); more than one: two stages
FALLBACK = 7                                   # path number of the exhaustive fallback (rings are 0 ... KNN_MAX_RING)

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instantsplat_amd", "csrc", "knn.hip")


def source_constants():
    src = open(SOURCE).read()
    return {
        "KNN_MAX_RING": int(re.search(r"constexpr int KNN_MAX_RING = (\d+);", src).group(1)),
        "CELL_GROWTH": re.search(r"g\.h = emax / \(float\)G \* ([0-9.]+)f;", src).group(1),
        "EXTENT_FLOOR": re.search(r"fmaxf\(ez, ([0-9.e+-]+)f\)", src).group(1),
        "RESOLUTION": re.search(r"while \(\(long long\)G \* G \* (\d+) < N && G < (\d+)\) \+\+G;\s*return G < (\d+) \? (\d+) : G;", src).groups(),
        "BBOX_SPLIT": re.search(r"bbox_blocks = min\((\d+), \(N \+ (\d+)\) / (\d+)\);", src).groups(),
        # the box is the first thing in the scratch (check_bbox reads it back there), and the fallback is still in the query
        "bbox_heads_the_scratch": bool(re.search(r"size_t o = 0;\s*bbox = o;", src)),
        "has_fallback": bool(re.search(r"if \(!done\) \{[^}]*for \(int j = 0; j < N; \+\+j\)", src)),
    }


# ------------------------------------------------------------------------------------------------------ the restated grid
def resolution(n):
    g = 1
    while 12 * g * g < n and g < 256:
        g += 1
    return max(g, 4)


class Grid:
    """knn_grid() and knn_cell_of() of csrc/knn.hip in numpy float32."""

    def __init__(self, lo, hi, n):
        self.lo, self.hi = np.asarray(lo, F), np.asarray(hi, F)
        self.G = resolution(n)
        ext = self.hi - self.lo
        emax = max(ext.max(), F(float(EXTENT_FLOOR)))
        self.h = F(F(emax / F(self.G)) * F(float(CELL_GROWTH)))
        self.inv_h = F(F(1.0) / self.h)
        self.dims = np.minimum(self.G, (ext * self.inv_h).astype(np.int32) + 1)

    @classmethod
    def of(cls, pts):
        return cls(pts.min(0), pts.max(0), len(pts))

    def raw_cell(self, x, axis):
        """int((x - min) * inv_h) before the clamp, x a float32 scalar or array"""
        x = np.asarray(x, F)
        assert x.dtype == F
        return ((x - self.lo[axis]) * self.inv_h).astype(np.int32)

    def cells(self, pts):
        c = np.stack([self.raw_cell(pts[:, a], a) for a in range(3)], 1)
        return np.clip(c, 0, self.dims - 1)


def three_nearest(pts):
    """[n, 3] float64: distances to the three nearest other points (self dropped by index; missing ones are 0), ascending"""
    p = np.asarray(pts, np.float64)
    n = len(p)
    k = min(4, n)
    d, idx = cKDTree(p).query(p, k=k)
    d, idx = d.reshape(n, k), idx.reshape(n, k)
    me = idx == np.arange(n)[:, None]
    me[~me.any(1), 0] = True        # more than three coincident points: self may be missing; drop one of the zeros
    keep = d[~me].reshape(n, k - 1)
    return np.concatenate([keep, np.zeros((n, 4 - k))], 1) if k < 4 else keep


def certified_paths(pts, grid=None):
    """per point: the ring 0 ... 6 its search must end at, FALLBACK, or -1 where the float64 certificate has no margin"""
    if len(pts) < 4:                 # no third neighbour: b2 stays at its start value, no ring ends the search
        return np.full(len(pts), FALLBACK)
    g = grid or Grid.of(pts)
    d3 = three_nearest(pts)[:, 2]
    x = d3 / float(g.h)
    path = np.full(len(pts), -1)
    ring = np.ceil(x).astype(int)
    ok = (np.abs(x - np.rint(x)) >= 1e-3) & (ring <= KNN_MAX_RING)
    path[ok] = ring[ok]
    path[d3 == 0] = 0
    path[x > KNN_MAX_RING + 1e-3] = FALLBACK
    return path


def path_counts(path):
    return {r: int((path == r).sum()) for r in range(FALLBACK + 1)}


# ------------------------------------------------------------------------------------------------------ calling the kernel
GUARD = 256
GUARD_BYTE = 0x3C


def _guarded(dev, nbytes, fill):
    buf = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    buf[GUARD:GUARD + nbytes] = fill
    return buf


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == GUARD_BYTE).all()) and bool((buf[GUARD + nbytes:] == GUARD_BYTE).all())


def scratch_bytes(n):
    from instantsplat_amd import _lib
    return int(_lib.lib().mi355gs_knn_scratch_bytes(n))


def run(dev, pts, fill=0xA5, scratch=None, want_box=False):
    """mi355gs_knn_dist2 through the C ABI on `pts` (numpy [n, 3] float32): the output, float32 on the CPU.  The scratch, of
    exactly mi355gs_knn_scratch_bytes(n) pre-filled with `fill`, and the output lie between guard regions that the call must
    leave as they were.  `scratch` = (buffer, nbytes): use that guarded buffer as it is.  want_box: also the six floats the
    call left at the head of its scratch (its bounding box: lo xyz, hi xyz)."""
    from instantsplat_amd import _lib
    L = _lib.lib()
    pts = np.ascontiguousarray(pts, F)
    n = len(pts)
    assert pts.shape == (n, 3)
    p = torch.from_numpy(pts).to(dev)
    sbuf, nbytes = scratch if scratch is not None else (None, scratch_bytes(n))
    if sbuf is None:
        sbuf = _guarded(dev, nbytes, fill)
    assert nbytes >= scratch_bytes(n)
    obuf = _guarded(dev, 4 * n, 0xEE)
    with _lib.on_device(dev):
        _lib.check(L.mi355gs_knn_dist2(_lib.stream_ptr(dev), n, _lib.ptr(p), obuf.data_ptr() + GUARD, sbuf.data_ptr() + GUARD), "knn_dist2")
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    assert _guards_intact(obuf, 4 * n), "the call wrote outside its output"
    assert _guards_intact(sbuf, nbytes), "the call wrote outside its scratch"
    out = obuf[GUARD:GUARD + 4 * n].cpu().view(torch.float32).clone()
    if want_box:
        return out, sbuf[GUARD:GUARD + 24].cpu().view(torch.float32).numpy().copy()
    return out


_REFERENCES = {}


def reference(label, pts):
    """oracle.knn_ref.dist2 of the cloud, computed once per label and shared"""
    if label not in _REFERENCES:
        ref = knn_ref.dist2(torch.from_numpy(np.ascontiguousarray(pts, F)))
        _REFERENCES[label] = (pts.copy(), ref)
    kept, ref = _REFERENCES[label]
    assert kept.shape == pts.shape and np.array_equal(kept, pts), label
    return ref


def worst_error(out, ref):
    """the largest |out - ref| / ref over the points with ref > 0; where ref == 0, out must be exactly 0"""
    o, r = out.double().numpy(), ref.double().numpy()
    assert o.shape == r.shape
    zero = r == 0
    assert (o[zero] == 0).all(), "a point whose three nearest coincide with it must give exactly 0"
    if zero.all():
        return 0.0
    rel = np.abs(o[~zero] - r[~zero]) / r[~zero]
    return float("nan") if np.isnan(rel).any() else float(rel.max())


def check(dev, label, pts, **kw):
    out = run(dev, pts, **kw)
    ops_util.bound("knn %s: worst relative error of a point" % label, worst_error(out, reference(label, pts)), LIMIT)
    return out


def bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------------ 1. ring ladder
LADDER_GPU = (36, 14.0)      # filler lattice side, isolation of every probe group in cells: 46728 points, G = 63
LADDER_EMU = (22, 6.0)       # 10720 points, G = 30 (a box of 30 cells has no room for 14)


@functools.lru_cache(maxsize=None)
def ring_ladder(filler_side, isolation):
    """A box fixed by its 8 corner points, a dense lattice cube at its centre that raises N, and probe groups at the centres of
    the faces and of the edges, each further than `isolation` cells from everything else:
      ring r = 1 ... 6: the 8 corners of a small cube of edge (r - 0.5) h: the three nearest of each are its edge neighbours;
      ring 0: three quadruples of coincident points;  fallback: the box's corners and four single points.
    -> (points, per-point certified path, name -> indices of each group)"""
    rng = np.random.default_rng(11)
    n = 8 + filler_side ** 3 + 6 * 8 + 3 * 4 + 4
    G = resolution(n)
    L = float(G)                                  # the box is [0, G]^3: h = 1.0001f
    h = float(F(F(F(L) / F(G)) * F(1.0001)))
    corners = np.array([[x, y, z] for x in (0, L) for y in (0, L) for z in (0, L)], np.float64)
    k = np.arange(filler_side) - (filler_side - 1) / 2
    filler = L / 2 + 0.25 * np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)

    def place(site, local):
        """`local` (>= 0, extent e per axis) at site in {0, 1, 2}^3: against the low face, centred (with a jitter), against the high face"""
        e = local.max(0)
        org = np.array([0.0 if s == 0 else L - e[a] if s == 2 else L / 2 - e[a] / 2 + rng.uniform(-0.4, 0.4) for a, s in enumerate(site)])
        return org + local

    faces = [(1, 1, 0), (1, 1, 2), (1, 0, 1), (1, 2, 1), (0, 1, 1), (2, 1, 1)]
    edges = [(1, 0, 0), (1, 0, 2), (1, 2, 0), (1, 2, 2), (0, 1, 0), (0, 1, 2), (2, 1, 0)]
    unit = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    parts, names = [corners, filler], ["corners", "filler"]
    for r in range(1, KNN_MAX_RING + 1):
        parts.append(place(faces[r - 1], unit * (r - 0.5) * h))
        names.append("ring%d" % r)
    for i in range(3):
        parts.append(place(edges[i], np.zeros((4, 3))))
        names.append("ring0_%d" % i)
    for i in range(4):
        parts.append(place(edges[3 + i], np.zeros((1, 3))))
        names.append("single%d" % i)
    pts = np.concatenate(parts).astype(F)
    assert len(pts) == n
    bounds = np.cumsum([0] + [len(p) for p in parts])
    groups = {nm: np.arange(bounds[i], bounds[i + 1]) for i, nm in enumerate(names)}
    order = rng.permutation(n)                    # no group is contiguous in memory
    pts = pts[order]
    inv = np.argsort(order)
    groups = {nm: inv[ix] for nm, ix in groups.items()}

    g = Grid.of(pts)
    assert g.G == G >= 30 and float(g.h) == h and (g.lo == 0).all() and (g.hi == F(L)).all()
    p64 = pts.astype(np.float64)
    for nm, ix in groups.items():
        if nm in ("filler", "corners"):
            continue
        rest = np.ones(n, bool)
        rest[ix] = False
        assert cKDTree(p64[rest]).query(p64[ix])[0].min() > isolation * h, nm
    rest = np.ones(n, bool)
    rest[groups["corners"]] = False
    assert cKDTree(p64[rest]).query(p64[groups["corners"]])[0].min() > min(isolation, 10.0) * h
    path = certified_paths(pts, g)
    for r in range(1, KNN_MAX_RING + 1):
        assert (path[groups["ring%d" % r]] == r).all(), r
    for i in range(3):
        assert (path[groups["ring0_%d" % i]] == 0).all()
    assert (path[groups["corners"]] == FALLBACK).all() and all((path[groups["single%d" % i]] == FALLBACK).all() for i in range(4))
    counts = path_counts(path)
    assert all(counts[r] >= 8 for r in range(FALLBACK + 1)), counts
    return pts, path, groups


# ------------------------------------------------------------------------------------------------------ 2. resolution / scan edges
RESOLUTION_SIZES = {192: 4, 193: 5, 2700: 15, 2701: 16, 3072: 16, 3073: 17}   # N -> G; G = 16: G^3 + 1 = 4097 counters


@functools.lru_cache(maxsize=None)
def uniform_cloud(n, seed=5):
    """uniform in a box, so that the occupied cells are spread over the whole table: with N <= 12 G^2 points in G^3 cells
    a cell holds 12 / G points on average, and a share 1 - exp(-12 / G) of them is occupied"""
    rng = np.random.default_rng(seed + n)
    pts = rng.uniform(-3.7, 5.9, (n, 3)).astype(F)
    g = Grid.of(pts)
    occupied = len(np.unique(g.cells(pts) @ np.array([1, 1000, 1000000])))
    assert (g.dims == g.G).all() and occupied >= 0.9 * (1 - np.exp(-n / g.G ** 3)) * g.G ** 3, (n, occupied)
    return pts


# ------------------------------------------------------------------------------------------------------ 3. bounding-box stages
BBOX_SIZES = (4095, 4096, 4097, 8193)


def bbox_stage_count(n):
    return min(1024, (n + 4095) // 4096)


@functools.lru_cache(maxsize=None)
def bbox_cloud(n):
    """A compact cloud in [-1, 1]^3 and six far points, each the sole holder of one extreme of the box and several cells
    outside the cloud, at the indices where the two-stage reduction's partition has its edges: 0, 1023 | 1024 (first and second
    workgroup), 4095 (the end of a workgroup's pass), the last two (a pass of its own) -- and 2048 where two of those coincide.
    -> (points, holders: the index of the point that alone holds lo x, y, z, hi x, y, z)"""
    rng = np.random.default_rng(300 + n)
    pts = rng.uniform(-1, 1, (n, 3)).astype(F)
    where = []
    for i in (0, 1023, 1024, 4095, n - 2, n - 1, 2048):
        if 0 <= i < n and i not in where:
            where.append(i)
    where = where[:6]
    assert len(where) == 6
    far = [-3.0, -3.25, -3.5, 3.125, 3.375, 3.625]
    for k, i in enumerate(where):
        pts[i, k % 3] = far[k]
    g = Grid.of(pts)
    lo, hi = pts.min(0), pts.max(0)
    for k, i in enumerate(where):
        col = pts[:, k % 3]
        assert (col == (lo, hi)[k // 3][k % 3]).sum() == 1 and col[i] == far[k]
        assert abs(far[k]) - 1 > 4 * float(g.h)                          # a box without it clamps it >= 4 cells off
    return pts, tuple(where)


def check_bbox(dev, n, fill=0xA5):
    """The values, and the box itself as the call leaves it at the head of its scratch.  (The values alone cannot see a box
    that misses a point: clamping a point into the nearest cell of too small a box moves no two points further apart, so the
    bound that ends the search stays true and the search exact.  The box is therefore read back.)"""
    pts, holders = bbox_cloud(n)
    assert bbox_stage_count(n) == (1 if n <= 4096 else 2 if n <= 8192 else 3)
    out, box = run(dev, pts, fill=fill, want_box=True)
    assert np.array_equal(box, np.concatenate([pts.min(0), pts.max(0)])), (box, holders)
    ops_util.bound("knn bbox N=%d: worst relative error of a point" % n, worst_error(out, reference("bbox%d" % n, pts)), LIMIT)
    return out


# ------------------------------------------------------------------------------------------------------ 4. few points
@functools.lru_cache(maxsize=None)
def few_points(n, coincident=False):
    pts = np.random.default_rng(40 + n).normal(size=(n, 3)).astype(F)
    if coincident:
        pts[n - 1] = pts[1]
    return pts


# ------------------------------------------------------------------------------------------------------ 5. degenerate geometry
@functools.lru_cache(maxsize=None)
def identical(n):
    return np.tile(np.array([[1.25, -0.3, 7.0]], F), (n, 1))


@functools.lru_cache(maxsize=None)
def collinear(axis, n=300 + 137):
    pts = np.tile(np.array([[1.5, -2.25, 0.75]], F), (n, 1))
    pts[:, axis] = np.random.default_rng(50 + axis).uniform(-4, 9, n).astype(F)
    return pts


@functools.lru_cache(maxsize=None)
def coplanar(normal_axis, n=1000):
    pts = np.random.default_rng(60 + normal_axis).uniform(-2, 5, (n, 3)).astype(F)
    pts[:, normal_axis] = F(-0.625)
    return pts


# ------------------------------------------------------------------------------------------------------ 6. unit lattice
LATTICE_SHIFT = (1000.0, -2000.0, 4096.0)


@functools.lru_cache(maxsize=None)
def lattice(side=12):
    k = np.arange(side)
    return np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3).astype(F)


def check_lattice(dev):
    """Every point of a cubic lattice of spacing 1 has at least three neighbours at distance exactly 1 (a corner has three, an
    edge four): every value is exactly 1, and stays so, bit for bit, when the lattice is moved, since differences of nearby
    floats are exact.  (A |p|^2 + |q|^2 - 2 p.q formulation would lose that.)"""
    pts = lattice()
    ref = reference("lattice", pts)
    assert (ref == 1.0).all()
    out = run(dev, pts)
    assert torch.equal(bits(out), bits(ref))
    moved = pts + np.array(LATTICE_SHIFT, F)
    assert np.array_equal((moved.astype(np.float64) - np.array(LATTICE_SHIFT)), pts.astype(np.float64))
    assert torch.equal(bits(run(dev, moved)), bits(ref))


# ------------------------------------------------------------------------------------------------------ 7. cluster + outliers
@functools.lru_cache(maxsize=None)
def cluster_and_outliers(cluster=2000, outliers=50):
    """The regime of real pointmaps: nearly all points (within 1 unit) share one cell of a box that a few far points span
    (1000 units).  Eight triples at the box's corners, whose third neighbour is most of the box away, and the rest around the
    middle.  -> (points, is_outlier, path)"""
    rng = np.random.default_rng(7)
    centre = np.array([452.0, 538.0, 471.0])
    cl = centre + rng.uniform(-0.5, 0.5, (cluster, 3))
    corners = np.array([[x, y, z] for x in (0.0, 1000.0) for y in (0.0, 1000.0) for z in (0.0, 1000.0)])
    inward = np.where(corners == 0, 1.0, -1.0)
    triples = np.concatenate([corners, corners + inward * rng.uniform(1, 6, (8, 3)), corners + inward * rng.uniform(1, 6, (8, 3))])
    middle = 500.0 + rng.uniform(-250, 250, (outliers - 24, 3))
    pts = np.concatenate([cl, triples, middle]).astype(F)
    is_out = np.arange(len(pts)) >= cluster
    order = rng.permutation(len(pts))
    pts, is_out = pts[order], is_out[order]
    g = Grid.of(pts)
    cells = g.cells(pts[~is_out]) @ np.array([1, 1000, 1000000])
    assert np.bincount(np.unique(cells, return_inverse=True)[1]).max() >= 0.9 * cluster
    path = certified_paths(pts, g)
    assert (path[is_out] == FALLBACK).sum() >= 10 and is_out.sum() == outliers
    return pts, is_out, path


# ------------------------------------------------------------------------------------------------------ 8. duplicates
@functools.lru_cache(maxsize=None)
def duplicates(n=3000):
    """10 pairs, 5 triples, 5 quadruples and one 20-fold point in a uniform cloud.  A member of a set of m coincident points has
    m - 1 neighbours at distance 0: from m = 4 on its value is exactly 0; in a pair or a triple the third neighbour is a
    distinct point and the value is held to the limit.  -> (points, multiplicity of every point)"""
    rng = np.random.default_rng(8)
    pts = rng.uniform(-3.7, 5.9, (n, 3)).astype(F)
    mult = np.ones(n, int)
    slots = rng.permutation(n)
    at = 0
    for m, times in ((2, 10), (3, 5), (4, 5), (20, 1)):
        for _ in range(times):
            ix = slots[at:at + m]
            at += m
            pts[ix] = pts[ix[0]]
            mult[ix] = m
    ref = reference("duplicates", pts)
    assert (ref[torch.from_numpy(mult >= 4)] == 0).all() and (ref[torch.from_numpy(mult <= 3)] > 0).all()
    return pts, mult


# ------------------------------------------------------------------------------------------------------ 9. ring-termination rounding
ADVERSARIAL = {"G71_x": (39, 0), "G8_z": (9, 2)}       # filler lattice side (N = side^3 + 13), the axis q and p lie along


def _edge(g, axis, c, a, b):
    """(largest float32 whose raw cell on `axis` is < c, smallest whose cell is >= c) between a and b: the cell is a monotone
    function of the coordinate (every operation in it is)"""
    a, b = F(a), F(b)
    assert g.raw_cell(a, axis) < c <= g.raw_cell(b, axis)
    up = F(np.inf)
    while np.nextafter(a, up) < b:
        m = F((float(a) + float(b)) / 2)
        if not a < m < b:
            m = np.nextafter(a, up)
        if g.raw_cell(m, axis) < c:
            a = m
        else:
            b = m
    return a, b


@functools.lru_cache(maxsize=None)
def adversarial(filler_side, axis):
    """The doubt about `done = b2 <= (r h)^2`: cell indices come from the rounded product (x - min) * inv_h, so the largest
    float q of a cell c and the smallest float p of cell c + 2 on one axis line can be closer than the rounded 1 h.  q gets two
    neighbours at 0.1 h and a candidate t inside its ring-1 cube, off the axis, with p - q < t and fl(t^2) <= fl(h^2): the true
    third neighbour is p, outside the cube; a search that ends at ring 1 because b2 = t^2 <= h^2 returns t.
    -> dict(points, q: index of q, predicted: the relative error of q's value in that event, G, gap: 1 - (p - q)^2 / h^2)"""
    lo, hi = F(-3.7), F(5.9)
    n = filler_side ** 3 + 8 + 5
    g = Grid([lo] * 3, [hi] * 3, n)
    h = g.h
    h2 = F(h * h)                                 # reach * reach for r = 1: (float)1 * h is h
    best = None
    for c in range(1, g.G - 3):
        x1, x2 = float(lo) + (c + 1) * float(h), float(lo) + (c + 2) * float(h)
        q, _ = _edge(g, axis, c + 1, x1 - 1e-3 * float(h), x1 + 1e-3 * float(h))
        _, p = _edge(g, axis, c + 2, x2 - 1e-3 * float(h), x2 + 1e-3 * float(h))
        assert g.raw_cell(q, axis) == c and g.raw_cell(p, axis) == c + 2
        e = F(p - q)
        if F(e * e) < h2 and (best is None or float(p) - float(q) < best[0]):
            best = (float(p) - float(q), q, p, c)
    assert best is not None, "no pair of floats two cells apart and closer than the rounded h"
    d, q, p, c = best
    t = h                                          # the largest float with fl(t * t) <= fl(h * h)
    while True:
        nxt = np.nextafter(t, F(np.inf))
        if F(nxt * nxt) > h2:
            break
        t = nxt
    assert F(t * t) <= h2 and d < float(t) <= float(np.nextafter(h, F(np.inf)))
    a1, a2 = (axis + 1) % 3, (axis + 2) % 3

    def at(x, y=0.0, z=0.0):
        v = np.zeros(3, F)
        v[axis], v[a1], v[a2] = x, y, z
        return v
    tenth = F(0.1) * h
    probe = np.stack([at(q), at(p), at(q, y=-t), at(q, z=tenth), at(q, z=-tenth)])
    # everything of q's is inside its ring-1 cube except p
    cq = [int(g.raw_cell(probe[0][a], a)) for a in range(3)]
    for row in probe[2:]:
        assert all(abs(int(g.raw_cell(row[a], a)) - cq[a]) <= 1 for a in range(3))
    assert int(g.raw_cell(probe[1][axis], axis)) - cq[axis] == 2
    # the distances as the kernel computes them: each along one axis, so one rounded difference and one rounded square
    ey = F(probe[0][a1] - probe[2][a1])
    assert ey == t and F(ey * ey) <= h2 and F(F(p - q) * F(p - q)) < h2
    corners = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], F)
    k = np.arange(filler_side, dtype=np.float64)
    filler = (-3.6 + 0.05 * np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)).astype(F)
    pts = np.concatenate([probe, corners, filler])
    order = np.random.default_rng(9).permutation(len(pts))
    pts = pts[order]
    qi = int(np.argsort(order)[0])
    g2 = Grid.of(pts)
    assert len(pts) == n and g2.G == g.G and g2.h == h and g2.inv_h == g.inv_h and (g2.lo == lo).all()
    near = three_nearest(pts)[qi]
    assert abs(near[0] - float(tenth)) < 1e-6 * float(h) and abs(near[1] - float(tenth)) < 1e-6 * float(h) and near[2] == d
    others = np.delete(np.arange(n), [qi] + [int(np.argsort(order)[j]) for j in range(1, 5)])
    assert np.linalg.norm(pts[others].astype(np.float64) - pts[qi].astype(np.float64), axis=1).min() > 1.5 * float(h)
    right = near[0] ** 2 + near[1] ** 2 + d ** 2
    predicted = (float(t) ** 2 - d ** 2) / right
    return {"points": pts, "q": qi, "predicted": predicted, "G": g.G, "gap": 1 - d ** 2 / float(h) ** 2}


def check_adversarial(dev, name):
    case = adversarial(*ADVERSARIAL[name])
    pts, qi = case["points"], case["q"]
    ref = reference("adversarial " + name, pts)
    out = run(dev, pts)
    ops_util.bound("knn adversarial %s: relative error of q" % name, abs(float(out[qi]) - float(ref[qi])) / float(ref[qi]), LIMIT)
    ops_util.bound("knn adversarial %s: worst relative error of a point" % name, worst_error(out, ref), LIMIT)


# ------------------------------------------------------------------------------------------------------ properties
def check_properties(dev, label, pts):
    """two runs give equal bits; a permutation of the rows gives the permuted bits (the box, the cells and the three smallest
    distances do not depend on the order; the scatter's atomics may reorder a cell, which the result must not see)"""
    first = check(dev, label, pts)
    assert torch.equal(bits(run(dev, pts)), bits(first))
    perm = np.random.default_rng(123).permutation(len(pts))
    assert torch.equal(bits(run(dev, pts[perm])), bits(first)[torch.from_numpy(perm)])
    return first


def check_scratch_contents_do_not_matter(dev, label, pts):
    outs = [check(dev, label, pts, fill=fill) for fill in (0x00, 0xA5, 0xFF)]
    assert torch.equal(bits(outs[0]), bits(outs[1])) and torch.equal(bits(outs[0]), bits(outs[2]))


def check_large_scratch_reused(dev):
    """one scratch sized for N = 8193, used at 8193 and then, as the first call left it, at N = 300"""
    big, _ = bbox_cloud(8193)
    nbytes = scratch_bytes(8193)
    assert nbytes >= scratch_bytes(300)
    sbuf = _guarded(dev, nbytes, 0xA5)
    check(dev, "bbox8193", big, scratch=(sbuf, nbytes))
    check(dev, "uniform N=300", uniform_cloud(300), scratch=(sbuf, nbytes))


def check_refusals(dev):
    """Decided from the arguments alone, before any device work: the pointers are bogus and must never be touched."""
    from instantsplat_amd import _lib
    L = _lib.lib()
    bogus = [0x1000, 0x2000, 0x3000]
    stream = _lib.stream_ptr(dev)
    with _lib.on_device(dev):
        assert L.mi355gs_knn_dist2(stream, -1, *bogus) == -1 and L.mi355gs_knn_dist2(stream, -2 ** 31, *bogus) == -1
        assert L.mi355gs_knn_dist2(stream, 0, *bogus) == 0 and L.mi355gs_knn_dist2(stream, 0, None, None, None) == 0
        for missing in range(3):
            args = [None if k == missing else bogus[k] for k in range(3)]
            assert L.mi355gs_knn_dist2(stream, 5, *args) == -1, missing
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def check_scratch_sizes():
    for n in (0, 1, 192, 193, 1_000_000):
        assert scratch_bytes(n) > 0
    sizes = [scratch_bytes(n) for n in sorted(RESOLUTION_SIZES)]
    assert sizes == sorted(sizes)
    assert [resolution(n) for n in sorted(RESOLUTION_SIZES)] == [RESOLUTION_SIZES[n] for n in sorted(RESOLUTION_SIZES)]
    assert resolution(12 * 255 * 255 + 1) == 256 == resolution(2 ** 31 - 1) and resolution(0) == resolution(1) == 4


# ------------------------------------------------------------------------------------------------------ the Python wrapper
def check_wrapper(dev):
    from instantsplat_amd.simple_knn._C import distCUDA2
    wide = torch.from_numpy(np.random.default_rng(70).normal(size=(333, 4)).astype(F)).to(dev)
    sliced = wide[:, :3]
    assert not sliced.is_contiguous()
    straight = distCUDA2(sliced.contiguous())
    assert straight.dtype == torch.float32 and straight.shape == (333,) and straight.device.type == dev.type
    ops_util.bound("knn wrapper: worst relative error of a point", worst_error(straight.cpu(), reference("wrapper", sliced.cpu().numpy())), LIMIT)
    assert torch.equal(bits(distCUDA2(sliced)), bits(straight))
    assert torch.equal(bits(distCUDA2(sliced.double())), bits(straight))           # float64 holding float32 values
    empty = distCUDA2(torch.zeros(0, 3, device=dev))
    assert empty.shape == (0,) and empty.dtype == torch.float32 and empty.device.type == dev.type
    for bad in (torch.zeros(7, 2, device=dev), torch.zeros(9, device=dev)):
        try:
            distCUDA2(bad)
        except RuntimeError as e:
            assert "points must have dimensions (num_points, 3)" in str(e)
        else:
            raise AssertionError("accepted a tensor of shape %s" % (tuple(bad.shape),))
