"""CPU tier: the per-Gaussian projection kernels (csrc/preprocess.hip) per row against float64 under general cameras, on the
emulated kernels — the same cases and checks as the GPU tier (tests/projection_cases.py)."""
import pytest
import torch

from tests import projection_cases as pc


def test_camera_helper_is_the_row_vector_convention():
    """viewmatrix = W2C^T, projmatrix = viewmatrix @ projection, campos = -R^T t, world means = (x_cam - t) R: a world point goes
    to its camera-frame coordinates through the flat matrix as the kernels read it, and the camera centre to the origin."""
    cam, tanx, tany = pc.pinhole(64, 48)
    for name, (R, t) in pc.CAMERAS.items():
        view, proj, campos = pc.camera_setup(R, t, cam)
        assert torch.allclose(R @ R.t(), torch.eye(3, dtype=pc.F64), atol=1e-14) and abs(float(torch.linalg.det(R)) - 1.0) < 1e-14, name
        x_cam = torch.tensor([[0.3, -0.2, 2.5], [-1.0, 0.7, 4.0]], dtype=pc.F64)
        x_w = pc.to_world(x_cam, R, t)
        assert torch.allclose(x_w @ R.t() + t, x_cam, atol=1e-14)
        assert torch.allclose(pc.rt._tp43(x_w, view.reshape(-1)), x_cam, atol=1e-14), name
        assert torch.allclose(pc.rt._tp43(campos[None], view.reshape(-1)), torch.zeros(1, 3, dtype=pc.F64), atol=1e-14), name
        hom = pc.rt._tp44(x_w, proj.reshape(-1))
        assert torch.allclose(hom[:, 0] / hom[:, 3], x_cam[:, 0] / x_cam[:, 2] / tanx, atol=1e-12), name
        assert torch.allclose(hom[:, 1] / hom[:, 3], x_cam[:, 1] / x_cam[:, 2] / tany, atol=1e-12), name
    assert float(pc.CAMERAS["rot180y"][0].diagonal().sum()) == -1.0 and float(pc.CAMERAS["rotation"][1].abs().max()) == 0.0
    assert torch.equal(pc.CAMERAS["translation"][0], torch.eye(3, dtype=pc.F64))


@pytest.mark.parametrize("name", pc.NAMES)
def test_cases_hold_the_rows_they_claim(name):
    """From the float64 oracle alone: clamped, masked and visible rows of every case (the counts in projection_cases's header)."""
    counts = pc.check_case_counts(name)
    print(name, counts)


@pytest.mark.parametrize("name", pc.NAMES)
def test_forward_records_per_gaussian(emu, name):
    pc.check_forward_records(emu, name)


@pytest.mark.parametrize("name", pc.NAMES)
def test_gradient_rows_through_the_operator(emu, name):
    pc.check_gradient_rows(emu, name)


@pytest.mark.parametrize("name", pc.SPLIT_ABI_NAMES)
def test_gradient_rows_through_the_c_abi_with_split_sh(emu, name):
    pc.check_gradient_rows(emu, name, path="abi")


def test_posed_node_under_a_general_view(emu):
    pc.check_posed_under_view(emu)


@pytest.mark.parametrize("camera", tuple(pc.CAMERAS))
def test_mark_visible_under_every_camera(emu, camera):
    pc.check_mark_visible(emu, camera)
