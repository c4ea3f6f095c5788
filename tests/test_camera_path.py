"""Interpolated camera paths (instantsplat_amd/camera_path.py) against the reference's own functions, executed from its files
by tests/golden/make_golden_interp.py (interp_path_vectors.npz).

Bound: both sides evaluate the same float64 formula on values of magnitude 1-10, about 20 operations deep; 1e-10 is a cap far above
the rounding of that (1e-13) and far below what a wrong formula gives (1e-3 or more)."""
import os

import numpy as np
import pytest

from instantsplat_amd.camera_path import generate_interpolated_path, interpolated_pose_path, save_interpolate_pose

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "interp_path_vectors.npz"))
CASES = (("v2", 2), ("v3", 3), ("v5", 5), ("v12", 12), ("zero_t", 2))
ATOL = 1e-10


@pytest.mark.parametrize("tag,V", CASES)
def test_generate_interpolated_path_matches_reference(tag, V):
    org, ref = G[f"interp_{tag}_org"], G[f"interp_{tag}_segments"]
    n_interp = int(10 * 30 / V)
    assert ref.shape == (V - 1, n_interp, 3, 4)
    for i in range(V - 1):
        got = generate_interpolated_path(org[i:i + 2], n_interp)
        assert got.shape == (n_interp, 3, 4) and got.dtype == np.float64
        err = np.abs(got - ref[i]).max()
        print(f"{tag} segment {i}: max |d| = {err:.3e}")
        assert err <= ATOL
        assert np.abs(generate_interpolated_path(org[i:i + 2, :3], n_interp) - ref[i]).max() <= ATOL   # (n,3,4) keyframes


@pytest.mark.parametrize("tag,V", CASES)
def test_interpolated_pose_path_matches_reference(tag, V):
    org, ref = G[f"interp_{tag}_org"], G[f"interp_{tag}_path"]
    got = interpolated_pose_path(org, V)
    assert got.shape == ref.shape == (int(10 * 30 / V) * (V - 1) + 1, 4, 4)
    err = np.abs(got - ref).max()
    print(f"{tag}: max |d| = {err:.3e}")
    assert err <= ATOL
    assert np.array_equal(got[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (got.shape[0], 1)))
    assert np.array_equal(got[-1, :3], org[-1, :3])          # the last keyframe closes the path
    assert np.abs(got[0, :3, 3] - org[0, :3, 3]).max() <= ATOL   # u = 0 is the first keyframe's position


def test_path_starts_at_every_keyframe_and_is_orthonormal():
    org = G["interp_v5_org"]
    got = interpolated_pose_path(org, 5)
    n_interp = int(10 * 30 / 5)
    for i in range(4):
        assert np.abs(got[i * n_interp, :3] - org[i, :3]).max() <= 1e-12
    R = got[:, :3, :3]
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 1e-12


def test_save_interpolate_pose_round_trip(tmp_path):
    org = G["interp_v3_org"]
    pose_dir = tmp_path / "pose" / "ours_30"
    pose_dir.mkdir(parents=True)
    np.save(pose_dir / "pose_optimized.npy", org)
    out = save_interpolate_pose(tmp_path, 30, 3)
    assert out == str(pose_dir / "pose_interpolated.npy")
    stored = np.load(out)
    assert stored.shape == (201, 4, 4) and stored.dtype == np.float64
    assert np.array_equal(stored, interpolated_pose_path(org, 3))
    assert np.abs(stored - G["interp_v3_path"]).max() <= ATOL
    assert sorted(p.name for p in pose_dir.iterdir()) == ["pose_interpolated.npy", "pose_optimized.npy"]   # no plots


def test_bad_arguments_are_refused():
    org = G["interp_v3_org"]
    with pytest.raises(ValueError):
        interpolated_pose_path(org, 1)
    with pytest.raises(ValueError):
        interpolated_pose_path(org, 4)          # fewer poses than views
    with pytest.raises(ValueError):
        interpolated_pose_path(org[:, :3], 3)   # not padded
    with pytest.raises(ValueError):
        generate_interpolated_path(org[:1], 10)


def test_more_than_two_keyframes_equal_scipy():
    """The n > 2 branch is the reference's own sequence of scipy calls."""
    interpolate = pytest.importorskip("scipy.interpolate")
    org = G["interp_v5_org"]
    got = generate_interpolated_path(org[:, :3], 7)
    assert got.shape == (7 * 4, 3, 4)
    pos = org[:, :3, 3]
    pts = np.stack([pos, pos - 0.1 * org[:, :3, 2], pos + 0.1 * org[:, :3, 1]], 1).reshape(5, -1)
    tck, _ = interpolate.splprep(pts.T, k=4, s=.03)
    new = np.array(interpolate.splev(np.linspace(0, 1, 28, endpoint=False), tck)).T.reshape(28, 3, 3)
    assert np.abs(got[:, :, 3] - new[:, 0]).max() <= ATOL
    look = new[:, 0] - new[:, 1]
    assert np.abs(got[:, :, 2] - look / np.linalg.norm(look, axis=1, keepdims=True)).max() <= ATOL


def test_two_keyframes_equal_scipy():
    """The closed form of the two-keyframe case is what splprep / splev give for it."""
    interpolate = pytest.importorskip("scipy.interpolate")
    for tag in ("v2", "zero_t"):
        org = G[f"interp_{tag}_org"]
        pos = org[:, :3, 3]
        pts = np.stack([pos, pos - 0.1 * org[:, :3, 2], pos + 0.1 * org[:, :3, 1]], 1).reshape(2, -1)
        tck, _ = interpolate.splprep(pts.T, k=1, s=.03)
        new = np.array(interpolate.splev(np.linspace(0, 1, 150, endpoint=False), tck)).T.reshape(150, 3, 3)
        assert np.abs(generate_interpolated_path(org, 150)[:, :, 3] - new[:, 0]).max() <= ATOL
