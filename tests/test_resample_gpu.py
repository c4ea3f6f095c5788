"""The device resampler (instantsplat_amd/resample.py, csrc/resample.hip) on the MI355X.  The checks are tests/resample_util.py's:
bytes against PIL and the host restatement, float outputs against torch's bit patterns, `load_images` and
`load_cam(resize="device")` against PIL-and-torch restatements of the reference's loaders; then two cases at the sizes the stage
runs at.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from tests import resample_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(ru.CASES))
def test_bytes_equal_pil(gpu, case):
    ru.check_case(gpu, case)


@pytest.mark.parametrize("case", ru.STACKED)
def test_stacks_of_three_equal_pil(gpu, case):
    ru.check_case(gpu, case, N=3)


def test_raw_call_stays_inside_its_buffers(gpu):
    ru.check_raw_call_stays_inside_its_buffers(gpu)


@pytest.mark.parametrize("case", ru.WINDOW_CASES)
def test_windows_equal_slices_of_the_full_result(gpu, case):
    ru.check_windows(gpu, case)


def test_float_outputs_have_torchs_bits(gpu):
    ru.check_float_outputs(gpu)


@pytest.mark.parametrize("size", (512, 224))
def test_load_images_art_frames(gpu, size):
    ru.check_load_images_art(gpu, size)


def test_load_images_synthetic_files(gpu, tmp_path, capsys):
    ru.check_load_images_synthetic(gpu, tmp_path, capsys)


def test_load_images_equals_the_references_own(gpu, tmp_path):
    ru.check_golden_load_images(gpu, tmp_path)


def test_load_cam_on_the_device_equals_pil(gpu):
    ru.check_load_cam(gpu)


def test_refusals(gpu):
    from instantsplat_amd.resample import resize_rgb8
    ru.check_entry_point_rejects_bad_arguments()
    ru.check_python_refusals(gpu)
    with pytest.raises(ValueError, match=r"\.to\(device\)"):
        resize_rgb8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), (2, 2))


def test_art_frames_720p_to_512x288(gpu):
    """the three 1280 x 720 frames, LANCZOS, as load_images(size=512) resizes them: bytes and the normalised floats"""
    from tests.jpeg_util import art_frames
    frames = art_frames()
    assert frames.shape == (3, 720, 1280, 3)
    rgb8, normalized = ru.device_resize(gpu, frames, (512, 288), "lanczos", out=("rgb8", "normalized"))
    for i in range(3):
        want = ru.pil_resize(frames[i], (512, 288), "lanczos")
        got = rgb8[i].cpu().numpy()
        assert np.array_equal(got, want), (i, ru.first_difference(got, want))
        assert ru.same_bits(normalized[i].cpu().numpy(), ru.torch_normalized(want)), i


@pytest.mark.parametrize("H,W", ((4032, 3024), (3024, 4032)))
def test_photograph_3024x4032_to_384x512(gpu, H, W):
    """one synthetic 12-megapixel photograph to 384 x 512 (W' x H'), LANCZOS: the portrait one keeps its shape (7.9x, 49 taps per
    pass), the landscape one is squeezed (10.5x across: 65 taps, 5.9x down: 37)"""
    rng = np.random.default_rng(12)
    photo = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    photo[1000:2500, 500:2500] = (rng.integers(0, 2, (1500, 2000, 3)) * 255).astype(np.uint8)   # a saturated region
    got = ru.device_resize(gpu, photo[None], (384, 512), "lanczos")[0].cpu().numpy()
    want = ru.pil_resize(photo, (384, 512), "lanczos")
    assert np.array_equal(got, want), ru.first_difference(got, want)
