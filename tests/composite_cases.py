"""The two kernels of csrc/composite.hip — k_composite_fwd and k_composite_bwd — on their own, per pixel and per Gaussian, against a
float64 replay of the same walk.  Cases, the replay and the checks shared by the emulated (CPU) and the GPU test files.

Everything else in tests/ reaches these kernels through the whole operator and compares one relative L2 per gradient tensor
(projection, binning and composite mixed), or switches the composite's own rounding off to judge the projection
(projection_cases.device_mode).  Here the device runs the raw C ABI (preprocess, the training forward, the backward; precomputed
colours, identity view, background BG, every byte of `binning` 0 beforehand) at unit levels 0 ... 3, and what the two kernels read
and leave is read back through the layouts of csrc/common.h, restated in tests/frame_abi.py (FrameViews holds their totals to the
library's size queries for every frame): the records and lists they read; image, final_T, n_contrib; the quadrant maxima, boundary records and
hit masks the forward hands to the backward; the nine moments per Gaussian the backward leaves in the gradient scratch.

THE REFERENCE is replay(): numpy, per tile and pixel, on the device's own records and lists cast to the dtype (projection and sort
are out of the comparison; they have their own tests): front to back with alpha = min(0.99, opacity 2^power2), skip if power2 > 0
or alpha < 1/255, stop in front of the Gaussian that would take T below 1e-4; back to front with the reference recursion,
dL/dalpha = T_k (c.g) - behind / (1 - alpha), w = (opacity 2^power2) dL/dalpha unclamped.  float64 is the reference; float32, on
whole lists with no unit cut, is the yardstick (the E_32 of projection_cases).  The code under test is never its own yardstick.
FRAGILE pixels are decided from the float64 forward alone: a pixel that, while live, meets a pair with |255 alpha - 1| <= 1e-4,
|T (1 - alpha) / 1e-4 - 1| <= 1e-4 or |power2| <= 1e-5.  dL/dpixel is zero on them for both sides and they are left out of the
forward comparisons; at most 2 % of a case's pixels may be fragile (asserted).  A differing decision on any other pixel fails.

CHECKS (limits through ops_util.bound: GS_CALIBRATE=1 lists the measured values)
  1 forward, per non-fragile pixel: n_contrib exact; image and final_T within max(2.5 E_32, FLOOR) of float64, E_32 the float32
    replay's largest error on the case, FLOOR the largest E_32 over the cases.
  2 hand-off, per level: qmax[tile][quadrant] is the maximum of the device's n_contrib over the quadrant, and float64's where the
    quadrant has no fragile pixel; every boundary record (slot seg_first[tile] + boundary - 1) against the float64 state in front
    of that list position under the image's limit (a finished pixel holds its final state, a pixel outside the image (1, 0, 0, 0));
    for every chunk and quadrant with chunk start < qmax the hit mask holds every instance float64 blends at a non-fragile
    pixel of the quadrant (extra hits are printed and recorded, not limited).
  3 moments, per Gaussian and level: a row float64 never blends is exactly zero; every other row i, moment m:
        |dev - f64| <= max(2.5 F_m, FLOOR_m) S_im + 4 B_im
    S: the sum of the absolute values of the row's terms; F_m: the float32 replay's largest |f32 - f64| / S over the case's
    touched rows (condition, asserted: <= 2e-5); FLOOR_m: the largest F_m over the cases; 2.5: projection_cases.REL.  B is the
    resume model, derived, float64: a Gaussian at list position k is resumed at unit length U if (k // U + 1) U < tile_max; per
    blended pixel delta = 2^-24 sum_c |g_c| (|final colour_c| + |colour in front of the boundary_c|), B_im = sum over pixels of
    (opacity 2^power2) delta / (1 - alpha) |phi_m|, phi = (dx, dy, dx^2, dx dy, dy^2, 1); zero for the colour moments.  It
    bounds the one loss the design accepts — a unit that is not the deepest of its tile resumes from dL/dC . (final colour -
    colour in front of the boundary), order-1 numbers standing for a quantity of order T — and 4 covers what first order
    leaves out (the stored colours carry accumulated rounding).  At level 3 every tile of needles and opaque fits one unit: B is
    identically zero there (asserted) and the strict limit judges every row.
  4 dL_dcolors is moments 6 - 8 and dL_dopacities moment 5 / opacity to 1e-6 relative: what is read here is what k_preprocess_bwd
    consumes.
  5 the deterministic instantiation (needles, edges; levels 0 and 2): bit-identical moments in two runs, check 3, the default image.

CASES (50 x 37 px: 4 x 3 tiles, a 2-px partial column, a 5-px partial row; centres -4 px ... size + 4 px, depth 2 ... 6, sigma in
pixels).  From the float64 replay (check_case_counts asserts what is claimed; the same on both tiers):
  needles  P  600: sigma (6 ... 16, 0.3 ... 0.8, 0.3 ... 0.8), opacity 0.05 ... 0.95.  3334 instances, lists <= 405, tile_max 404;
           591 rows touched, resumed at levels 0 ... 3: 546 / 528 / 491 / 0; 66 pixels terminate; fragile 0.11 %
  opaque   P 1200: sigma 2 ... 8, opacity 0.5 ... 0.999.  7242 instances, lists <= 989, tile_max 213; 264 rows touched, resumed
           227 / 217 / 0 / 0; all 1850 pixels terminate; 4 pairs clamped at 0.99; fragile 0.27 %
  faint    P 1500: sigma 1 ... 5, opacity 0.01 ... 0.31.  5010 instances, lists <= 656, tile_max 656; 1497 rows touched, resumed
           1451 / 1412 / 1366 / 1268; no pixel terminates; fragile 0.65 %
  edges    P 1260, hand-built (_edges says why its walls are not walls).  1392 instances; 869 rows touched, resumed 664 / 472 /
           216 / 0; 94 pixels terminate; fragile 0.22 %.  Tiles (0,0) (1,0) (2,0) (0,1) (0,2): largest contributor exactly 64, 65, 128,
           129, 256 with 70 list entries behind it that blend nowhere (tile_max <= boff, boff + seg_len < tile_max and `reach`
           on both sides of equality for U = 64 and 128); tile (3,0) empty between two non-empty ones; tile (2,1): quadrant 3
           terminates inside chunk 0, quadrant 0 never does and blends past instance 128 (different qmax per quadrant, a forward
           wave that breaks early, trailing boundary records from the "never reached" loop); tile (1,1): chunk 0 has exactly one
           hit in quadrant 0 and three in quadrant 1 (the padding of the forward's two-hit walk step).

MEASURED, forward and hand-off (emulated kernels / MI355X; FLOOR: image 1.79e-6, final_T 5.34e-7, both needles' E_32)
  needles  image 1.49e-6 / 1.49e-6 (E_32 1.79e-6), final_T 4.4e-7 / 4.1e-7 (E_32 5.3e-7); boundary records 45 / 20 / 7 / 0 at levels
           0 ... 3, worst 2.74e-6 / 2.77e-6 (limit 4.47e-6); hit masks 3891 needed, 161 extra
  opaque   image 4.5e-7 / 4.3e-7 (E_32 4.5e-7), final_T 1.3e-9 / 1.3e-9 (E_32 1.2e-9); records 107 / 51 / 21 / 7, worst 4.6e-7 / 4.3e-7
           (limit 1.79e-6); hit masks 2493 needed, 806 extra
  faint    image 5.7e-7 / 6.3e-7 (E_32 5.7e-7), final_T 9.6e-9 / 7.7e-9 (E_32 7.6e-9); records 73 / 35 / 16 / 5, worst 5.2e-7 / 5.8e-7;
           hit masks 8548 needed, 108 extra
  edges    image 3.2e-7 / 3.3e-7 (E_32 3.1e-7), final_T 1.8e-7 / 1.6e-7 (E_32 2.8e-7); records 19 / 8 / 2 / 0, worst 2.3e-7 / 2.5e-7;
           hit masks 1613 needed, 80 extra

MEASURED, moments (per family: F_m, then per level and tier the worst E_dev / S of the nine moments | the worst ratio of check 3 |
the share of rows where 4 B > max(2.5 F, FLOOR) S | the largest (error - strict part) / B, which the factor 4 bounds).
FLOOR_m = 5.5e-6  5.9e-6  6.1e-6  7.3e-6  6.4e-6  4.5e-6  1.9e-6  4.9e-6  2.1e-6.  The deterministic runs give the same digits.
   needles  F         4.4e-6  4.2e-6  6.1e-6  6.3e-6  6.4e-6  2.1e-6  1.9e-6  4.9e-6  2.1e-6
            L0 emulated 1.9e-5  1.0e-5  1.1e-5  8.8e-6  2.3e-5  7.6e-6  2.1e-6  4.3e-6  2.2e-6 | 0.45 | 67.3 % | 0.07
            L0 MI355X   1.9e-5  1.0e-5  1.2e-5  8.6e-6  2.3e-5  8.2e-6  2.1e-6  4.3e-6  2.2e-6 | 0.45 | 67.3 % | 0.08
            L1 emulated 1.9e-5  1.0e-5  1.1e-5  6.9e-6  2.3e-5  7.6e-6  2.1e-6  4.3e-6  2.2e-6 | 0.45 | 62.1 % | 0.07
            L1 MI355X   1.9e-5  1.0e-5  1.2e-5  6.8e-6  2.3e-5  7.8e-6  2.1e-6  4.3e-6  2.2e-6 | 0.45 | 62.1 % | 0.06
            L2 emulated 1.9e-5  1.0e-5  1.1e-5  6.4e-6  2.3e-5  8.2e-6  2.1e-6  4.3e-6  2.3e-6 | 0.45 | 53.1 % | 0.07
            L2 MI355X   1.9e-5  1.0e-5  1.2e-5  6.7e-6  2.3e-5  8.3e-6  2.1e-6  4.3e-6  2.2e-6 | 0.45 | 53.1 % | 0.06
            L3 emulated 3.6e-6  3.6e-6  5.9e-6  5.9e-6  5.7e-6  1.4e-6  2.1e-6  4.3e-6  2.3e-6 | 0.45 |  0.0 % | 0.00
            L3 MI355X   3.7e-6  3.6e-6  5.9e-6  5.9e-6  5.7e-6  1.7e-6  2.1e-6  4.3e-6  2.2e-6 | 0.45 |  0.0 % | 0.00
   opaque   F         2.2e-6  2.2e-6  2.3e-6  2.2e-6  2.2e-6  2.2e-6  9.7e-7  7.2e-7  7.8e-7
            L0 emulated 3.8e-4  3.6e-4  3.7e-4  3.6e-4  3.6e-4  3.9e-4  5.9e-7  5.4e-7  5.4e-7 | 0.40 | 81.4 % | 0.24
            L0 MI355X   3.8e-4  3.6e-4  3.7e-4  3.6e-4  3.6e-4  3.9e-4  5.3e-7  5.7e-7  5.7e-7 | 0.36 | 81.4 % | 0.24
            L1 emulated 3.8e-4  3.6e-4  3.7e-4  3.6e-4  3.6e-4  3.9e-4  5.9e-7  5.4e-7  5.4e-7 | 0.40 | 73.9 % | 0.29
            L1 MI355X   3.8e-4  3.6e-4  3.7e-4  3.6e-4  3.6e-4  3.9e-4  5.3e-7  5.7e-7  5.7e-7 | 0.36 | 73.9 % | 0.29
            L2 emulated 2.2e-6  2.2e-6  2.3e-6  2.2e-6  2.2e-6  2.2e-6  5.9e-7  5.4e-7  5.4e-7 | 0.40 |  0.0 % | 0.00
            L2 MI355X   2.0e-6  2.0e-6  2.0e-6  2.0e-6  2.0e-6  2.0e-6  5.3e-7  5.7e-7  5.7e-7 | 0.36 |  0.0 % | 0.00
            L3 emulated 2.2e-6  2.2e-6  2.3e-6  2.2e-6  2.2e-6  2.2e-6  5.9e-7  5.4e-7  5.4e-7 | 0.40 |  0.0 % | 0.00
            L3 MI355X   2.0e-6  2.0e-6  2.0e-6  2.0e-6  2.0e-6  2.0e-6  5.3e-7  5.7e-7  5.7e-7 | 0.36 |  0.0 % | 0.00
   faint    F         1.1e-6  1.4e-6  8.5e-7  1.1e-6  1.3e-6  1.4e-6  5.5e-7  5.6e-7  4.4e-7
            L0 emulated 5.5e-5  6.4e-5  5.3e-5  7.0e-5  7.5e-5  6.0e-5  5.5e-7  3.1e-7  3.6e-7 | 0.30 | 78.6 % | 0.36
            L0 MI355X   5.5e-5  6.4e-5  5.4e-5  7.0e-5  7.5e-5  6.0e-5  4.4e-7  3.3e-7  3.5e-7 | 0.24 | 78.6 % | 0.36
            L1 emulated 5.5e-5  6.4e-5  5.3e-5  7.0e-5  7.5e-5  6.0e-5  6.0e-7  6.0e-7  6.0e-7 | 0.33 | 76.6 % | 0.44
            L1 MI355X   5.5e-5  6.4e-5  5.4e-5  7.0e-5  7.5e-5  6.0e-5  4.6e-7  6.4e-7  4.0e-7 | 0.25 | 76.6 % | 0.44
            L2 emulated 5.5e-5  6.4e-5  5.3e-5  7.0e-5  7.5e-5  6.0e-5  1.1e-6  1.2e-6  1.2e-6 | 0.61 | 73.7 % | 0.44
            L2 MI355X   5.5e-5  6.4e-5  5.4e-5  7.0e-5  7.5e-5  6.0e-5  6.3e-7  7.0e-7  4.2e-7 | 0.34 | 73.7 % | 0.44
            L3 emulated 5.5e-5  6.4e-5  5.3e-5  7.0e-5  7.5e-5  6.0e-5  1.2e-6  1.2e-6  1.2e-6 | 0.66 | 60.8 % | 0.17
            L3 MI355X   5.5e-5  6.4e-5  5.4e-5  7.0e-5  7.5e-5  6.0e-5  7.4e-7  7.0e-7  6.5e-7 | 0.40 | 60.8 % | 0.16
   edges    F         5.5e-6  5.9e-6  5.4e-6  7.3e-6  6.0e-6  4.5e-6  4.3e-7  4.9e-7  4.2e-7
            L0 emulated 2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  7.1e-7  5.5e-7  5.3e-7 | 0.38 | 12.5 % | 1.14
            L0 MI355X   2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  5.0e-7  5.5e-7  5.3e-7 | 0.29 | 12.5 % | 1.14
            L1 emulated 2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  7.1e-7  6.4e-7  6.1e-7 | 0.38 | 12.3 % | 1.14
            L1 MI355X   2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  6.4e-7  5.6e-7  5.5e-7 | 0.35 | 12.3 % | 1.14
            L2 emulated 2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  8.1e-7  6.4e-7  6.6e-7 | 0.44 | 12.4 % | 0.25
            L2 MI355X   2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  2.3e-3  6.4e-7  5.6e-7  5.5e-7 | 0.35 | 12.4 % | 0.25
            L3 emulated 8.0e-6  8.0e-6  8.0e-6  8.1e-6  8.0e-6  8.0e-6  8.1e-7  6.4e-7  6.6e-7 | 0.71 |  0.0 % | 0.00
            L3 MI355X   5.7e-6  9.8e-6  5.7e-6  6.9e-6  1.0e-5  7.5e-6  7.4e-7  6.2e-7  6.1e-7 | 0.66 |  0.0 % | 0.00

THE PRICE OF THE UNIT CUT (worst E_dev / F_m over the six alpha-borne moments, level 0 against level 3; both tiers alike):
  needles 4.3 against 1.0;  opaque 177 against 1.0 (0.9 on the MI355X);  faint 64 against 64 (its lists are longer than 512: 1268
  rows are still resumed at level 3);  edges 511 against 1.8 (1.7).  The colour moments stay at F at every level.  All of it is
  inside 4 B (largest share of B used: 1.14, edges levels 0 and 1): the known loss of resuming from a colour difference, recorded
  here, not a wrong record.  With whole-list units the MI355X stands where the emulated kernels and the float32 replay stand, so
  its 1-ulp v_exp_f32 / v_rcp_f32 cost nothing that shows at this scale.

MUTATIONS (each applied to a copy of the tree outside the repository, emulated library built from it with tests/emu/build_emu.sh,
tests/test_composite_emu.py run on it; the first failing test is named, the number is how many of the file's 51 tests fail):
  (a) sign of the cross term in two of quad_hit's edge maximisers   29: test_forward_per_pixel[needles] (forward, hand-off and moments
                                                                     of needles, opaque and faint at every level; edges, whose
                                                                     Gaussians are round, passes everything)
  (b) Tr[qd] = brec[qd].x * 1.0001f at resume                       16: test_moments_per_gaussian[needles-0] (moments and deterministic
                                                                     runs at exactly the levels that have resumed rows)
  (c) `reach` one short                                             20: test_moments_per_gaussian[needles-0] (every moments test)
  (d) the blue channel dropped from the resumed `behind`            16: test_moments_per_gaussian[needles-0] (as (b))
  (e) forward boundary stored one group late                        28: test_handoff_tables[needles-0] (boundary records and moments
                                                                     at the levels that have boundaries)
  (f) `last` not updated for the second hit of a walk step          40: test_forward_per_pixel[needles] (n_contrib; then everything
                                                                     but the case counts)
"""
import functools
import math
import os
import re

import numpy as np
import torch

from tests import frame_abi, ops_util
from tests import tile_length_cases as tl
from tests.projection_cases import REL

# csrc/composite.hip and csrc/common.h, restated (source_constants() reads the same from the sources)
GS_TILE = frame_abi.GS_TILE
GS_SEG = tl.GS_SEG
LEVELS = tuple(range(tl.GS_UNIT_LEVELS))
ALPHA_MIN = 1.0 / 255.0
ALPHA_MAX = 0.99
T_MIN = 1e-4

W, H = 50, 37             # 4 x 3 tiles, a 2-px partial column and a 5-px partial row
BG = (0.2, 0.5, 0.9)
FRAGILE = 1e-4            # relative distance of a decision's operand from its threshold below which a pixel is left out
FRAGILE_POWER = 1e-5
FRAGILE_SHARE = 0.02      # condition: at most this share of a case's pixels is fragile
F_CAP = 2e-5              # condition: the float32 replay's row error over S, every case and moment
RESUME_FACTOR = 4.0
ULP = 2.0 ** -24
MOMENTS = ("w dx", "w dy", "w dx2", "w dxdy", "w dy2", "w", "dr", "dg", "db")
NAMES = ("needles", "opaque", "faint", "edges")
DET_NAMES = ("needles", "edges")
DET_LEVELS = (0, 2)


def source_constants():
    """The constants above, read from the kernel sources."""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instantsplat_amd", "csrc")
    src = open(os.path.join(root, "composite.hip")).read()
    hdr = open(os.path.join(root, "common.h")).read()

    def one(pattern, text):
        m = re.search(pattern, text)
        assert m, pattern
        return m.group(1)

    assert "alignas(16) GsRec {\n  float4 q0;" in hdr and "float4 g0;" in hdr and "float4 g2;" in hdr      # three float4 each
    assert one(r"constexpr float ALPHA_MIN = ([^;]+);", src) == "1.0f / 255.0f"
    return dict(GS_TILE=int(one(r"#define GS_TILE (\d+)", hdr)), GS_SEG=int(one(r"constexpr int GS_SEG = (\d+);", hdr)),
                GS_UNIT_LEVELS=int(one(r"constexpr int GS_UNIT_LEVELS = (\d+);", hdr)), ALPHA_MIN=1.0 / 255.0,
                ALPHA_MAX=float(one(r"alpha = fminf\(([0-9.]+)f, a1\.w \* gs_exp2\(power2\)\)", src)),
                ALPHA_MAX_BWD=float(one(r"fmed3f\(av, 0\.0f, ([0-9.]+)f\)", src)),
                T_MIN=float(one(r"constexpr float T_MIN = ([0-9.]+)f;", src)), FWD_GROUP=int(one(r"constexpr int FWD_GROUP = (\d+);", src)))


# ---------------------------------------------------------------------------------------------------- cases
def _camera():
    tanx = math.tan(math.radians(60) / 2)
    tany = tanx * H / W
    return tanx, tany, W / (2 * tanx)


class _Builder:
    """Gaussians given in pixels: centre (pixel p is NDC (2 p + 1) / size - 1), depth, sigma per axis in pixels (scales = sigma
    z / focal under an identity view), rotation, opacity; precomputed colours."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.rows = []

    def u(self, n, lo, hi):
        return lo + (hi - lo) * torch.rand(n, generator=self.g, dtype=torch.float64)

    def add(self, px, py, z, sigma, opac, q=None):
        n = px.shape[0]
        if q is None:
            q = torch.randn(n, 4, generator=self.g, dtype=torch.float64)
            q = q / q.norm(dim=1, keepdim=True)
        self.rows.append((px, py, z, sigma, opac, q))

    def case(self, name):
        tanx, tany, focal = _camera()
        px, py, z, sigma, opac, q = (torch.cat([r[i] for r in self.rows]) for i in range(6))
        n = px.shape[0]
        perm = torch.randperm(n, generator=self.g)      # a tile's Gaussians are scattered over the index range
        px, py, z, sigma, opac, q = (x[perm] for x in (px, py, z, sigma, opac, q))
        means = torch.stack([((2 * px + 1) / W - 1) * tanx * z, ((2 * py + 1) / H - 1) * tany * z, z], dim=1)
        col = torch.rand(n, 3, generator=self.g, dtype=torch.float64)
        wgt = torch.randn(3, H, W, generator=self.g, dtype=torch.float64)
        return dict(name=name, P=n, means=means.float(), scales=(sigma * z[:, None] / focal).float(), q=q.float(), opac=opac.float(), col=col.float(),
                    wgt=wgt.float())


def _random_family(name, seed, n, sigma_lo, sigma_hi, op_lo, op_hi):
    b = _Builder(seed)
    lo, hi = torch.tensor(sigma_lo, dtype=torch.float64), torch.tensor(sigma_hi, dtype=torch.float64)
    sigma = lo + (hi - lo) * torch.rand(n, 3, generator=b.g, dtype=torch.float64)
    b.add(b.u(n, -4.0, W + 4.0), b.u(n, -4.0, H + 4.0), b.u(n, 2.0, 6.0), sigma, b.u(n, op_lo, op_hi))
    return b.case(name)


# the edges family: (tile x, tile y, largest contributor index asked for, the side of the image the dead tail sits on)
EXACT_TILES = ((0, 0, 64, "top"), (1, 0, 65, "top"), (2, 0, 128, "top"), (0, 1, 129, "left"), (0, 2, 256, "bottom"))
TAIL = 70                 # list entries behind the largest contributor: more than a chunk, so whole units lie behind tile_max
EMPTY_TILE = 3            # (3, 0), between (2, 0) and (0, 1)
SPLIT_TILE = 6            # (2, 1): quadrant 3 ends inside chunk 0, another never ends over more than two units
PAD_TILE = 5              # (1, 1): chunk 0 has one blended instance in quadrant 0 and three in quadrant 1


def _edges():
    """The hand-built family.  A Gaussian that ends a whole 16-px tile (alpha near 0.99 on all of it) reaches every tile of a
    50 x 37 frame, so a tile's largest contributor index M is not set by a wall in front of more list: the tile holds M - 1 faint
    Gaussians and an opaque one behind them, all confined to it (centres 4 ... 11 px inside, under 0.6 px sigma), and behind
    those TAIL entries that are in its list and blend nowhere: opacity 0.008 and 0.3 px sigma, centred 1 px outside the image,
    so the half-pixel slack of the binning box reaches the tile's border pixels while their alpha there is 0.6 / 255."""
    b = _Builder(41)
    one = lambda v: torch.tensor([v], dtype=torch.float64)
    for tx, ty, M, side in EXACT_TILES:
        x0, y0 = 16.0 * tx, 16.0 * ty
        ylo, yhi = (y0 + 4.0, y0 + 11.0) if side != "bottom" else (34.7, 36.0)
        n = M - 1
        b.add(b.u(n, x0 + 4, x0 + 11), b.u(n, ylo, yhi), b.u(n, 2.0, 5.0), torch.stack([b.u(n, 0.4, 0.6) for _ in range(3)], 1), b.u(n, 0.02, 0.04))
        b.add(b.u(1, x0 + 4, x0 + 11), b.u(1, ylo if side != "bottom" else 35.5, yhi), one(5.5), torch.full((1, 3), 0.5, dtype=torch.float64), one(0.95))
        along_x, along_y = b.u(TAIL, x0 + 4, x0 + 11), b.u(TAIL, y0 + 4, y0 + 11)
        px, py = {"top": (along_x, torch.full_like(along_x, -1.0)), "left": (torch.full_like(along_y, -1.0), along_y),
                  "bottom": (along_x, torch.full_like(along_x, float(H)))}[side]
        b.add(px, py, b.u(TAIL, 5.8, 6.0), torch.full((TAIL, 3), 0.3, dtype=torch.float64), torch.full((TAIL,), 0.008, dtype=torch.float64))
    # SPLIT_TILE: four layers of a 4 x 4 grid of opaque 2-px Gaussians over quadrant 3 in front (64 instances: chunk 0), 200
    # faint ones confined to the tile behind them
    x0, y0 = 16.0 * (SPLIT_TILE % 4), 16.0 * (SPLIT_TILE // 4)
    grid = torch.tensor([0.5, 2.5, 4.5, 6.5], dtype=torch.float64)
    gx_, gy_ = torch.meshgrid(grid, grid, indexing="ij")
    wx, wy = (x0 + 8 + gx_.reshape(-1)).repeat(4), (y0 + 8 + gy_.reshape(-1)).repeat(4)
    b.add(wx, wy, 2.0 + 0.001 * torch.arange(64, dtype=torch.float64), torch.full((64, 3), 2.0, dtype=torch.float64), torch.full((64,), 0.95, dtype=torch.float64))
    b.add(b.u(200, x0 + 4, x0 + 11), b.u(200, y0 + 4, y0 + 11), b.u(200, 3.0, 5.0), torch.stack([b.u(200, 0.8, 1.0) for _ in range(3)], 1), b.u(200, 0.02, 0.04))
    # PAD_TILE: one Gaussian in quadrant 0, three in quadrant 1
    x0, y0 = 16.0 * (PAD_TILE % 4), 16.0 * (PAD_TILE // 4)
    px = torch.tensor([x0 + 4.0, x0 + 11.5, x0 + 12.0, x0 + 11.0], dtype=torch.float64)
    py = torch.tensor([y0 + 4.0, y0 + 3.0, y0 + 4.0, y0 + 5.0], dtype=torch.float64)
    b.add(px, py, torch.tensor([3.0, 3.1, 3.2, 3.3], dtype=torch.float64), torch.full((4, 3), 0.3, dtype=torch.float64), torch.full((4,), 0.5, dtype=torch.float64))
    return b.case("edges")


@functools.lru_cache(maxsize=None)
def get_case(name):
    if name == "needles":    # graze quadrant corners: quad_hit's edge maximisers
        return _random_family(name, 11, 600, (6.0, 0.3, 0.3), (16.0, 0.8, 0.8), 0.05, 0.95)
    if name == "opaque":     # every pixel terminates; 0.99-clamped pairs
        return _random_family(name, 21, 1200, (2.0, 2.0, 2.0), (8.0, 8.0, 8.0), 0.5, 0.999)
    if name == "faint":      # alphas around the 1/255 cut; most pixels never terminate
        return _random_family(name, 13, 1500, (1.0, 1.0, 1.0), (5.0, 5.0, 5.0), 0.01, 0.31)
    assert name == "edges", name
    return _edges()


# ---------------------------------------------------------------------------------------------------- the device side
def _mode(level, R, det):
    """the unit level (mi355gs_tune_min_units, for a frame of R instances) and the deterministic instantiation, both set before
    the frame's buffers are sized and restored afterwards"""
    return frame_abi.knobs(min_units=tl.min_units_for(R, level), det=bool(det))


def _scene(case):
    return dict(means=case["means"], rots=case["q"], scales=case["scales"], opac=case["opac"], colors=case["col"])


@functools.lru_cache(maxsize=None)
def _instances(dev, name):
    """the frame's instance count: the unit level is the scan's function of it and of the knob, so it is needed before the frame runs"""
    return frame_abi.run_frame(dev, _scene(get_case(name)), frame_abi.identity_camera(W, H), bg=BG, preprocess_only=True).R


def run_device(dev, name, level, det=False, dL=None):
    """The case through the raw C ABI at a unit level: preprocess, the training forward and — with a dL/dpixel — the backward.
    Every byte of `binning` is 0 beforehand.  Returns what the composite kernels read and left, as numpy arrays."""
    case = get_case(name)
    P = case["P"]
    R = _instances(str(dev), name)
    with _mode(level, R, det):
        assert frame_abi.current_knobs()[1] == int(bool(det))
        fr = frame_abi.run_frame(dev, _scene(case), frame_abi.identity_camera(W, H), bg=BG, dL=dL)
    assert fr.R == R
    v = fr.views
    out = dict(name=name, level=level, det=det, R=R, P=P, max_units=v.max_units, max_chunks=v.max_chunks)
    if dL is not None:
        out["moments"] = fr.moments.cpu().numpy().copy()
        out["dL_dcolors"], out["dL_dopac"] = fr.grads["colors"].cpu().numpy(), fr.grads["opac"].cpu().numpy()
    T = v.T
    out["rec"] = v.np("rec")
    out["start"], out["seg_first"], out["meta"], out["qmax"] = v.np("tile_start"), v.np("seg_first"), v.np("meta"), v.np("qmax")
    out["final_T"], out["n_contrib"] = v.np("final_T"), v.np("n_contrib")
    out["lst"], out["bstate"], out["hitmask"] = v.np("list"), v.np("bstate"), v.np("hitmask")
    out["image"] = fr.image.cpu().numpy()
    assert out["meta"][2] == 1 << level, (out["meta"], level)
    assert out["start"][0] == 0 and out["start"][T] == R and bool((np.diff(out["start"]) >= 0).all()) and int(out["lst"].max(initial=0)) < P
    return out


# ---------------------------------------------------------------------------------------------------- the reference
def tile_pixels():
    """-> (x, y, inside), each [tiles, 256]: the pixels of every tile in the order of the kernels' per-tile state (quadrant-major:
    slot = quadrant * 64 + lane, quadrant = (x >= 8) + 2 (y >= 8) inside the tile, lane = x % 8 + 8 (y % 8))"""
    gx, gy = (W + GS_TILE - 1) // GS_TILE, (H + GS_TILE - 1) // GS_TILE
    slot = np.arange(256)
    qd, lane = slot // 64, slot % 64
    ox, oy = (qd & 1) * 8 + (lane & 7), (qd >> 1) * 8 + (lane >> 3)
    tile = np.arange(gx * gy)
    x, y = (tile % gx)[:, None] * GS_TILE + ox[None], (tile // gx)[:, None] * GS_TILE + oy[None]
    return x, y, (x < W) & (y < H)


def _padded_lists(lists, tile_start):
    T = len(tile_start) - 1
    n = np.diff(tile_start)
    ids = np.zeros((T, max(int(n.max()), 1)), dtype=np.int64)
    for t in range(T):
        ids[t, : n[t]] = lists[tile_start[t]: tile_start[t + 1]]
    return ids, n


def _pair(rec, g, X, Y, dt):
    """dx, dy, power2, opacity 2^power2 (unclamped) and alpha of the Gaussians g [tiles] at the pixels [tiles, 256]"""
    dx, dy = rec[g, 0][:, None] - X, rec[g, 1][:, None] - Y
    power2 = (dx * rec[g, 4][:, None]) * dx + (dy * rec[g, 5][:, None]) * dy + (rec[g, 6][:, None] * dx) * dy
    au = rec[g, 7][:, None] * np.exp2(np.minimum(power2, dt(0)))
    return dx, dy, power2, au, np.minimum(dt(ALPHA_MAX), au)


def replay_forward(records, lists, tile_start, bg, dtype, states=True):
    """Front to back over every tile's list, every pixel on its own, in `dtype`: skip a Gaussian if power2 > 0 or alpha < 1/255,
    stop in front of one that would take T below 1e-4.  Everything per tile and pixel is [tiles, 256] in tile_pixels()'s order."""
    dt = np.dtype(dtype).type
    rec = np.asarray(records).astype(dtype)
    ids, n = _padded_lists(lists, tile_start)
    X, Y, inside = tile_pixels()
    X, Y = X.astype(dtype), Y.astype(dtype)
    T_, Lmax = ids.shape
    Tr, C = np.ones((T_, 256), dtype=dtype), np.zeros((T_, 256, 3), dtype=dtype)
    done, last, fragile = ~inside, np.zeros((T_, 256), dtype=np.int64), np.zeros((T_, 256), dtype=bool)
    blended = np.zeros((T_, Lmax, 256), dtype=bool)
    clamped = 0
    st_T = np.ones((T_, Lmax + 1, 256), dtype=dtype) if states else None
    st_C = np.zeros((T_, Lmax + 1, 256, 3), dtype=dtype) if states else None
    amin, tmin = dt(1.0) / dt(255.0), dt(T_MIN)
    for k in range(Lmax):
        if states:
            st_T[:, k], st_C[:, k] = Tr, C
        g = ids[:, k]
        live = (k < n)[:, None] & ~done
        dx, dy, power2, au, alpha = _pair(rec, g, X, Y, dt)
        ok = live & (power2 <= 0) & (alpha >= amin)
        test = Tr * (dt(1.0) - alpha)
        stop = ok & (test < tmin)
        bl = ok & ~stop
        fragile |= live & ((np.abs(dt(255.0) * alpha - dt(1.0)) <= FRAGILE) | (np.abs(power2) <= FRAGILE_POWER))
        fragile |= ok & (np.abs(test / tmin - dt(1.0)) <= FRAGILE)
        w = np.where(bl, alpha * Tr, dt(0))
        C = C + rec[g, 8:11][:, None, :] * w[:, :, None]
        Tr = np.where(bl, test, Tr)
        last = np.where(bl, k + 1, last)
        done = done | stop
        blended[:, k] = bl
        clamped += int((bl & (au > dt(ALPHA_MAX))).sum())
    if states:
        st_T[:, Lmax], st_C[:, Lmax] = Tr, C
    bgv = np.asarray(bg, dtype=dtype)
    return dict(T=Tr, C=C, colour=C + Tr[:, :, None] * bgv[None, None, :], last=last, done=done & inside, inside=inside, fragile=fragile & inside,
                blended=blended, st_T=st_T, st_C=st_C, ids=ids, n=n, clamped=clamped)


def to_image(per_tile):
    """[tiles, 256, ...] in tile_pixels()'s order -> [H, W, ...]"""
    X, Y, inside = tile_pixels()
    out = np.zeros((H, W) + per_tile.shape[2:], dtype=per_tile.dtype)
    out[Y[inside], X[inside]] = per_tile[inside]
    return out


def from_image(img):
    """[H, W, ...] -> [tiles, 256, ...], zero outside the image"""
    X, Y, inside = tile_pixels()
    out = np.zeros(X.shape + img.shape[2:], dtype=img.dtype)
    out[inside] = img[Y[inside], X[inside]]
    return out


def replay_backward(fwd, records, dL_dpix, bg, dtype, resume_model=False):
    """Back to front with the reference recursion: T_k = T_(k+1) / (1 - alpha_k), dL/dalpha = T_k (c.g) - behind / (1 - alpha),
    w = (opacity 2^power2) dL/dalpha unclamped.  -> the nine moments per Gaussian, the sums of their terms' absolute values S,
    the rows touched; with resume_model (float64 only) the bound B of the resume rounding per unit level, [levels, P, 6], and
    the rows resumed per level."""
    dt = np.dtype(dtype).type
    rec = np.asarray(records).astype(dtype)
    P = rec.shape[0]
    ids, n, blended = fwd["ids"], fwd["n"], fwd["blended"]
    X, Y, _ = tile_pixels()
    X, Y = X.astype(dtype), Y.astype(dtype)
    g_pix = from_image(np.moveaxis(np.asarray(dL_dpix), 0, -1)).astype(dtype)          # [tiles, 256, 3]
    bgv = np.asarray(bg, dtype=dtype)
    Tr = fwd["T"].copy()
    behind = Tr * (g_pix @ bgv)
    M, S, touched = np.zeros((P, 9), dtype=dtype), np.zeros((P, 9), dtype=np.float64), np.zeros(P, dtype=bool)
    tile_max = fwd["last"].max(axis=1)
    if resume_model:
        assert dtype == np.float64
        B, resumed = np.zeros((len(LEVELS), P, 6)), np.zeros((len(LEVELS), P), dtype=bool)
        g_abs, final_abs = np.abs(g_pix), np.abs(fwd["colour"])
        tiles = np.arange(ids.shape[0])
    for k in range(ids.shape[1] - 1, -1, -1):
        bl = blended[:, k]
        rows = bl.any(axis=1)
        if not rows.any():
            continue
        g = ids[:, k]
        dx, dy, power2, au, alpha = _pair(rec, g, X, Y, dt)
        one_m = dt(1.0) - alpha
        Tk = np.where(bl, Tr / one_m, Tr)
        cg = (rec[g, 8:11][:, None, :] * g_pix).sum(axis=2)
        w = np.where(bl, au * (Tk * cg - behind / one_m), dt(0))
        aT = np.where(bl, alpha * Tk, dt(0))
        behind = behind + cg * aT
        Tr = Tk
        wdx, wdy = w * dx, w * dy
        terms = np.stack([wdx, wdy, wdx * dx, wdx * dy, wdy * dy, w, aT * g_pix[:, :, 0], aT * g_pix[:, :, 1], aT * g_pix[:, :, 2]], axis=2)
        np.add.at(M, g[rows], terms.sum(axis=1)[rows])
        np.add.at(S, g[rows], np.abs(terms).astype(np.float64).sum(axis=1)[rows])
        touched[g[rows]] = True
        if resume_model:
            phi = np.abs(np.stack([dx, dy, dx * dx, dx * dy, dy * dy, np.ones_like(dx)], axis=2))
            for level in LEVELS:
                U = GS_SEG << level
                b = (k // U + 1) * U
                res = rows & (b < tile_max)
                if not res.any():
                    continue
                front = np.abs(fwd["st_C"][tiles, min(b, fwd["st_C"].shape[1] - 1)])
                delta = ULP * (g_abs * (final_abs + front)).sum(axis=2)
                e = np.where(bl & res[:, None], au * delta / one_m, 0.0)
                np.add.at(B[level], g[res], (e[:, :, None] * phi).sum(axis=1)[res])
                resumed[level][g[res]] = True
    out = dict(M=M, S=S, touched=touched, tile_max=tile_max)
    if resume_model:
        out.update(B=B, resumed=resumed)
    return out


def replay(records, lists, tile_start, bg, dL_dpix, dtype):
    """The whole walk in `dtype` on the device's own records and lists: image, final_T, n_contrib, the state in front of every
    instance, the blended mask, the nine moments per Gaussian and the sums S of their terms' absolute values."""
    fwd = replay_forward(records, lists, tile_start, bg, dtype)
    bwd = replay_backward(fwd, records, dL_dpix, bg, dtype, resume_model=np.dtype(dtype) == np.float64)
    return dict(fwd, **bwd, image=np.moveaxis(to_image(fwd["colour"]), -1, 0), final_T=to_image(fwd["T"]), n_contrib=to_image(fwd["last"]))


@functools.lru_cache(maxsize=None)
def reference(dev, name):
    """Both replays of a case on the records and lists the device made of it (level 0; check_levels_agree holds the other levels
    to the same bits), computed once and never modified.  The fragile pixels come from the float64 forward alone; dL/dpixel is
    the case's seeded one with those pixels zeroed, for both replays and the device.  Of the per-instance states the boundaries
    of the 64-instance chunks are kept."""
    base = run_device(dev, name, 0)
    args = (base["rec"], base["lst"], base["start"], BG)
    f64 = replay_forward(*args, np.float64)
    fragile = to_image(f64["fragile"])
    share = float(fragile.mean())
    assert share <= FRAGILE_SHARE, (name, share)
    dL = get_case(name)["wgt"].numpy().astype(np.float64) * ~fragile[None]
    r64 = dict(f64, **replay_backward(f64, base["rec"], dL, BG, np.float64, resume_model=True))
    f32 = replay_forward(*args, np.float32, states=False)
    r32 = dict(f32, **replay_backward(f32, base["rec"], dL, BG, np.float32))
    keep = ~f64["fragile"] & f64["inside"]
    assert bool((f32["last"][keep] == f64["last"][keep]).all()), "%s: the two replays decide differently on a non-fragile pixel" % name
    r64["st_T"], r64["st_C"] = f64["st_T"][:, ::GS_SEG].copy(), f64["st_C"][:, ::GS_SEG].copy()
    rows = r64["touched"]
    F = (np.abs(r32["M"].astype(np.float64) - r64["M"])[rows] / np.maximum(r64["S"][rows], 1e-300)).max(axis=0)
    F[(r64["S"][rows] == 0).all(axis=0)] = 0.0
    res = dict(base=base, r64=r64, r32=r32, dL=dL.astype(np.float32), fragile=f64["fragile"], keep=keep, share=share, F=F,
               E32_image=float(np.abs(f32["colour"].astype(np.float64) - f64["colour"])[keep].max()),
               E32_T=float(np.abs(f32["T"].astype(np.float64) - f64["T"])[keep].max()))
    assert float(F.max()) <= F_CAP, (name, F.tolist())
    return res


@functools.lru_cache(maxsize=None)
def floors(dev):
    """FLOOR of the image, of final_T and of every moment: the largest E_32 (F_m) over all cases, from the two replays alone"""
    refs = [reference(dev, n) for n in NAMES]
    return dict(image=max(r["E32_image"] for r in refs), T=max(r["E32_T"] for r in refs), F=np.max([r["F"] for r in refs], axis=0))


def limit(dev, name, what):
    ref, fl = reference(dev, name), floors(dev)
    return max(REL * ref["E32_" + what], fl[what])


# ---------------------------------------------------------------------------------------------------- what a case holds
def case_counts(dev, name):
    """touched rows, resumed rows per level, clamped pairs, terminated pixels, fragile share — from the float64 replay"""
    ref = reference(dev, name)
    r = ref["r64"]
    return dict(P=get_case(name)["P"], R=ref["base"]["R"], longest=int(r["n"].max()), tile_max=int(r["tile_max"].max()), touched=int(r["touched"].sum()),
                resumed=[int(x.sum()) for x in r["resumed"]], clamped=r["clamped"], terminated=int(r["done"].sum()), fragile=round(ref["share"], 4))


def _quadrant(a):
    return a.reshape(a.shape[0], 4, 64)


def check_case_counts(dev, name):
    """What a case claims to contain, asserted from the float64 replay; -> the counts listed in this file's header."""
    c = case_counts(dev, name)
    r = reference(dev, name)["r64"]
    npix = W * H
    assert c["touched"] >= c["P"] // 6, c
    if name in ("needles", "opaque"):       # B is identically zero at the top level: the strict limit applies to every row
        assert c["tile_max"] <= GS_SEG << LEVELS[-1] and c["resumed"][-1] == 0 and not r["B"][-1].any(), c
        assert c["resumed"][0] >= 0.25 * c["touched"], c
    if name == "opaque":
        assert c["terminated"] == npix and c["clamped"] >= 1 and c["longest"] >= 900, c
    if name == "faint":
        assert c["terminated"] <= 0.5 * npix and c["longest"] >= 400 and c["resumed"][0] >= 0.5 * c["touched"], c
    if name == "edges":
        last, done, inside, n = r["last"], r["done"], r["inside"], r["n"]
        for tx, ty, M, _ in EXACT_TILES:
            t = ty * 4 + tx
            assert r["tile_max"][t] == M and n[t] == M + TAIL, (t, M, int(r["tile_max"][t]), int(n[t]))
            assert not r["blended"][t, M:].any()
        assert {M for _, _, M, _ in EXACT_TILES} == {u * m + d for u, m, d in ((64, 1, 0), (64, 1, 1), (64, 2, 0), (128, 1, 1), (128, 2, 0))}
        assert n[EMPTY_TILE] == 0 and n[EMPTY_TILE - 1] > 0 and n[EMPTY_TILE + 1] > 0
        ql, qd, qi = (a[SPLIT_TILE].reshape(4, 64) for a in (last, done, inside))
        assert bool(qi.all()) and bool(qd[3].all()) and int(ql[3].max()) <= GS_SEG          # quadrant 3 ends inside chunk 0 ...
        assert int(np.where(~qd[0], ql[0], 0).max()) > 2 * GS_SEG                          # ... quadrant 0 never does, over more than two units
        hits = [int(_quadrant(r["blended"][PAD_TILE, :GS_SEG])[:, qd_].any(axis=1).sum()) for qd_ in range(4)]
        assert hits[0] == 1 and hits[1] == 3, hits
        c["pad_hits"] = hits
    return c


# ---------------------------------------------------------------------------------------------------- checks
def check_levels_agree(dev, name):
    """records, lists, per-pixel state and image are bit-identical at every unit level (so one replay serves them all)"""
    base = reference(dev, name)["base"]
    for level in LEVELS[1:]:
        o = run_device(dev, name, level)
        for k in ("rec", "start", "lst", "image", "final_T", "n_contrib", "qmax"):
            assert np.array_equal(base[k], o[k]), (name, level, k)


def check_forward(dev, name):
    """Check 1: n_contrib exact, image and final_T within max(2.5 E_32, FLOOR) of float64, on every non-fragile pixel."""
    ref = reference(dev, name)
    base, r64, keep = ref["base"], ref["r64"], ref["keep"]
    nc = from_image(base["n_contrib"])
    bad = keep & (nc != r64["last"])
    assert not bad.any(), "%s: n_contrib differs on %d non-fragile pixels, e.g. tile %d slot %d: device %d, float64 %d" % (
        (name, int(bad.sum())) + tuple(int(v[0]) for v in np.nonzero(bad)) + (int(nc[bad][0]), int(r64["last"][bad][0])))
    e_img = np.abs(from_image(np.moveaxis(base["image"], 0, -1)).astype(np.float64) - r64["colour"])[keep].max()
    e_T = np.abs(from_image(base["final_T"]).astype(np.float64) - r64["T"])[keep].max()
    print("%s forward: image E_dev %.2e (E_32 %.2e, limit %.2e), final_T E_dev %.2e (E_32 %.2e, limit %.2e), fragile %.2f %%" % (
        name, e_img, ref["E32_image"], limit(dev, name, "image"), e_T, ref["E32_T"], limit(dev, name, "T"), 100 * ref["share"]))
    ops_util.bound("composite/%s/image" % name, e_img, limit(dev, name, "image"))
    ops_util.bound("composite/%s/final_T" % name, e_T, limit(dev, name, "T"))


def check_handoff(dev, name, level):
    """Check 2: what the forward leaves for the backward at this unit level — quadrant maxima, boundary records, hit masks."""
    ref = reference(dev, name)
    r64, keep, inside = ref["r64"], ref["keep"], ref["r64"]["inside"]
    o = run_device(dev, name, level)
    T = o["qmax"].shape[0]
    U, cpu = GS_SEG << level, 1 << level
    nc = np.where(inside, from_image(o["n_contrib"]), 0)
    assert np.array_equal(o["qmax"], _quadrant(nc).max(axis=2)), "%s: qmax is not the maximum of the device's n_contrib" % name
    clean = ~_quadrant(ref["fragile"]).any(axis=2)
    want = _quadrant(np.where(inside, r64["last"], 0)).max(axis=2)
    assert np.array_equal(o["qmax"][clean], want[clean]), "%s: qmax differs from float64 in a quadrant without a fragile pixel" % name
    lim = limit(dev, name, "image")
    worst, nrec = 0.0, 0
    for t in range(T):
        nseg = int(o["seg_first"][t + 1] - o["seg_first"][t])
        assert nseg == -(-int(r64["n"][t]) // U)
        for b in range(1, nseg):
            slot = int(o["seg_first"][t]) + b - 1
            assert slot < o["max_units"]
            recd = o["bstate"][slot].astype(np.float64)
            want = np.concatenate([r64["st_T"][t, b * cpu][:, None], r64["st_C"][t, b * cpu]], axis=1)     # the state in front of instance b U
            outside = ~inside[t]
            assert np.array_equal(recd[outside], np.tile([1.0, 0.0, 0.0, 0.0], (int(outside.sum()), 1)))
            if keep[t].any():
                worst = max(worst, float(np.abs(recd - want)[keep[t]].max()))
            nrec += 1
    print("%s level %d: %d boundary records, worst %.2e (limit %.2e)" % (name, level, nrec, worst, lim))
    ops_util.bound("composite/%s/level %d/boundary records" % (name, level), worst, lim)
    needed = extra = 0
    bit = np.uint64(1) << np.arange(GS_SEG, dtype=np.uint64)
    for t in range(T):
        first = int(o["seg_first"][t]) * cpu
        for c in range(-(-int(r64["n"][t]) // GS_SEG)):
            assert first + c < o["max_chunks"]
            bl = _quadrant_rows(r64["blended"][t, c * GS_SEG: (c + 1) * GS_SEG] & keep[t][None])           # [instances of the chunk, 4]
            for qd in range(4):
                if c * GS_SEG >= o["qmax"][t, qd]:
                    continue
                need = int((bit[: bl.shape[0]][bl[:, qd]]).sum())
                got = int(o["hitmask"][first + c, qd])
                assert need & ~got == 0, "%s level %d: tile %d chunk %d quadrant %d: hit mask %#x misses %#x" % (name, level, t, c, qd, got, need & ~got)
                needed += bin(need).count("1")
                extra += bin(got & ~need).count("1")
    print("%s level %d: hit masks hold %d needed instances and %d extra" % (name, level, needed, extra))
    ops_util.MEASURED.append(("composite/%s/level %d/extra hits (recorded, no limit)" % (name, level), float(extra), float("inf")))
    return dict(records=nrec, worst=worst, needed=needed, extra=extra)


def _quadrant_rows(bl):
    """[instances, 256] -> [instances, 4]: blended at some pixel of the quadrant"""
    return bl.reshape(bl.shape[0], 4, 64).any(axis=2)


def judge_moments(dev, name, level, moments, what):
    """Check 3 on one [P, 9] table of moments."""
    ref, fl = reference(dev, name), floors(dev)
    r64 = ref["r64"]
    d = moments.astype(np.float64)
    assert np.isfinite(d).all()
    idle = ~r64["touched"]
    assert not d[idle].any(), "%s %s: %d rows the float64 replay never blends are not zero" % (name, what, int(d[idle].any(axis=1).sum()))
    rel = np.maximum(REL * ref["F"], fl["F"])[None, :]
    B = np.concatenate([r64["B"][level], np.zeros((d.shape[0], 3))], axis=1)
    strict = rel * r64["S"]
    lim = strict + RESUME_FACTOR * B
    err = np.abs(d - r64["M"])
    rows = r64["touched"]
    ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))[rows]
    e_over_s = (err[rows] / np.maximum(r64["S"][rows], 1e-300)).max(axis=0)
    model = (RESUME_FACTOR * B > strict).any(axis=1)[rows].mean()
    over_model = np.where(B[rows] > 0, np.maximum(err[rows] - strict[rows], 0) / np.where(B[rows] > 0, B[rows], 1.0), 0.0).max()
    print("%s level %d %s: worst ratio %.3f; E_dev/S %s; F %s; rows judged by the resume model %.1f %%; largest (err - strict) / B %.2f; rows over: %d" % (
        name, level, what, ratio.max(), " ".join("%.1e" % v for v in e_over_s), " ".join("%.1e" % v for v in ref["F"]), 100 * model, over_model,
        int((ratio > 1).any(axis=1).sum())))
    ops_util.MEASURED.append(("composite/%s/level %d/%s/share of rows under the resume model (recorded, no limit)" % (name, level, what), float(model), float("inf")))
    for m, label in enumerate(MOMENTS):
        ops_util.bound("composite/%s/level %d/%s/moment %s" % (name, level, what, label), ratio[:, m].max(), 1.0)
    return dict(ratio=float(ratio.max()), e_over_s=e_over_s, model=float(model))


def check_moments(dev, name, level):
    """Check 3: the nine moments of every Gaussian at this unit level against float64."""
    ref = reference(dev, name)
    check_case_counts(dev, name)
    o = run_device(dev, name, level, dL=ref["dL"])
    assert np.array_equal(o["image"], ref["base"]["image"])
    return judge_moments(dev, name, level, o["moments"], "moments")


def check_public_outputs(dev, name="needles", level=0):
    """Check 4: what the test reads from the scratch is what k_preprocess_bwd consumes: dL_dcolors is moments 6 - 8, dL_dopacities
    moment 5 over the opacity."""
    ref = reference(dev, name)
    o = run_device(dev, name, level, dL=ref["dL"])
    m = o["moments"].astype(np.float64)
    assert int((m[:, 5] != 0).sum()) >= 100
    op = get_case(name)["opac"].numpy().astype(np.float64)
    for label, got, want in (("dL_dcolors", o["dL_dcolors"], m[:, 6:9]), ("dL_dopacities", o["dL_dopac"], m[:, 5] / op)):
        got = got.astype(np.float64)
        assert np.isfinite(got).all() and not got[want == 0].any()
        ops_util.bound("composite/%s/%s against the moments" % (name, label), (np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max(), 1e-6)


def check_deterministic(dev, name, level):
    """Check 5: the deterministic instantiation, set before the frame's buffers are sized: bit-identical moments in two runs, inside
    check 3's limits; the image is the default mode's."""
    ref = reference(dev, name)
    a = run_device(dev, name, level, det=True, dL=ref["dL"])
    b = run_device(dev, name, level, det=True, dL=ref["dL"])
    assert np.array_equal(a["moments"].view(np.uint32), b["moments"].view(np.uint32))
    assert np.array_equal(a["image"], ref["base"]["image"]) and np.array_equal(a["n_contrib"], ref["base"]["n_contrib"])
    return judge_moments(dev, name, level, a["moments"], "deterministic")
