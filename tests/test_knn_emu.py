"""CPU tier: the 3-NN kernel on every search path and grid edge, on the emulated kernels -- the same builders and checks as the
GPU tier (tests/knn_cases.py; measured values: the table in test_knn_gpu.py).  The ring ladder uses a smaller filler here
(10720 points, G = 30, every probe group more than 6 cells from everything else) and keeps all eight certified counts."""
import numpy as np
import pytest

from tests import knn_cases as kc


def test_constants_are_the_sources():
    """The restated grid and the path certificates hold only while these are the constants of csrc/knn.hip."""
    assert kc.source_constants() == {"KNN_MAX_RING": kc.KNN_MAX_RING, "CELL_GROWTH": kc.CELL_GROWTH, "EXTENT_FLOOR": kc.EXTENT_FLOOR,
                                     "RESOLUTION": kc.RESOLUTION, "BBOX_SPLIT": kc.BBOX_SPLIT, "bbox_heads_the_scratch": True,
                                     "has_fallback": True}
    assert kc.KNN_MAX_RING == 6 and kc.FALLBACK == 7 and kc.LIMIT == 16 * 2.0 ** -24


def test_builders_certify_what_they_claim():
    for ladder in (kc.LADDER_GPU, kc.LADDER_EMU):
        pts, path, groups = kc.ring_ladder(*ladder)
        counts = kc.path_counts(path)
        assert min(counts.values()) >= 8 and counts[kc.FALLBACK] == 12 and counts[0] == 12
    assert kc.Grid.of(kc.ring_ladder(*kc.LADDER_GPU)[0]).G == 63 and kc.Grid.of(kc.ring_ladder(*kc.LADDER_EMU)[0]).G == 30
    assert [kc.Grid.of(kc.uniform_cloud(n)).G for n in kc.RESOLUTION_SIZES] == list(kc.RESOLUTION_SIZES.values())
    assert kc.RESOLUTION_SIZES[3072] ** 3 + 1 == 4097
    assert [kc.bbox_stage_count(n) for n in kc.BBOX_SIZES] == [1, 1, 2, 3]
    assert kc.bbox_cloud(8193)[1] == (0, 1023, 1024, 4095, 8191, 8192) and kc.bbox_cloud(4097)[1] == (0, 1023, 1024, 4095, 4096, 2048)
    pts, is_out, path = kc.cluster_and_outliers()
    assert (path[is_out] == kc.FALLBACK).sum() >= 24
    pts, mult = kc.duplicates()
    assert sorted(set(mult)) == [1, 2, 3, 4, 20] and (mult == 20).sum() == 20
    big, small = kc.adversarial(*kc.ADVERSARIAL["G71_x"]), kc.adversarial(*kc.ADVERSARIAL["G8_z"])
    assert big["G"] == 71 and small["G"] == 8
    # the G = 71 case can tell: a search that ends at ring 1 there misses the limit by more than a factor 2
    assert big["predicted"] > 2 * kc.LIMIT and 0 < small["predicted"]


def test_ring_ladder_and_its_properties(emu):
    pts, path, groups = kc.ring_ladder(*kc.LADDER_EMU)
    kc.check_properties(emu, "ring ladder (emulated size)", pts)


@pytest.mark.parametrize("n", list(kc.RESOLUTION_SIZES))
def test_resolution_and_scan_edges(emu, n):
    kc.check(emu, "uniform N=%d" % n, kc.uniform_cloud(n))


@pytest.mark.parametrize("n", kc.BBOX_SIZES)
def test_bounding_box_stages(emu, n):
    kc.check_bbox(emu, n)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_few_points(emu, n):
    kc.check(emu, "few N=%d" % n, kc.few_points(n))


def test_four_points_two_coincident(emu):
    kc.check(emu, "few N=4, two coincident", kc.few_points(4, True))


@pytest.mark.parametrize("n", [5, 300])
def test_identical_points_give_zero(emu, n):
    out = kc.check(emu, "identical N=%d" % n, kc.identical(n))
    assert (out == 0).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_collinear_and_coplanar(emu, axis):
    kc.check(emu, "collinear%d" % axis, kc.collinear(axis))
    kc.check(emu, "coplanar%d" % axis, kc.coplanar(axis))


def test_unit_lattice_is_exact_and_translation_invariant(emu):
    kc.check_lattice(emu)


def test_cluster_plus_far_outliers_and_its_properties(emu):
    kc.check_properties(emu, "cluster + outliers", kc.cluster_and_outliers()[0])


def test_duplicates_and_their_properties(emu):
    pts, mult = kc.duplicates()
    out = kc.check_properties(emu, "duplicates", pts)
    assert (out.numpy()[mult >= 4] == 0).all() and (out.numpy()[mult <= 3] > 0).all()


@pytest.mark.parametrize("name", list(kc.ADVERSARIAL))
def test_ring_termination_rounding(emu, name):
    kc.check_adversarial(emu, name)


def test_scratch_contents_do_not_matter(emu):
    kc.check_scratch_contents_do_not_matter(emu, "bbox4097", kc.bbox_cloud(4097)[0])
    kc.check_scratch_contents_do_not_matter(emu, "duplicates", kc.duplicates()[0])
    for fill in (0x00, 0xFF):
        kc.check_bbox(emu, 8193, fill=fill)


def test_large_scratch_reused(emu):
    kc.check_large_scratch_reused(emu)


def test_refusals_and_scratch_sizes(emu):
    kc.check_refusals(emu)
    kc.check_scratch_sizes()


def test_wrapper(emu):
    kc.check_wrapper(emu)


def test_certificates_know_a_ring_from_its_neighbour():
    """the certificate itself, on a cloud small enough to see: four points on a line in a box of 4 cells"""
    pts = np.array([[0, 0, 0], [1, 0, 0], [2.2, 0, 0], [4, 0, 0], [4, 4, 4]], np.float32)
    g = kc.Grid.of(pts)
    assert g.G == 4 and abs(float(g.h) - 1.0001) < 1e-6 and list(g.dims) == [4, 4, 4]
    assert [list(c) for c in g.cells(pts)] == [[0, 0, 0], [0, 0, 0], [2, 0, 0], [3, 0, 0], [3, 3, 3]]
    d3 = kc.three_nearest(pts)[:, 2]
    assert np.allclose(d3, [4, 3, 2.2, 4, np.sqrt(9 + 16 + 16)])
    # 4 / h and 3 / h are within 1e-3 of an integer: no certificate; 2.2 / h ends at ring 3; 6.4 / h > 6.001: the fallback
    assert list(kc.certified_paths(pts)) == [-1, -1, 3, -1, kc.FALLBACK]
