"""The device PNG encoder (instantsplat_amd/png.py, csrc/png.hip) on the MI355X.  The checks are tests/png_util.py's: zlib, PIL and
a host restatement that holds every block to the optimal code's cost and every file to its predicted length.  Every step runs
under a time limit of its own."""
import numpy as np
import pytest
import torch

from tests import png_util as pu
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H,W", pu.SHAPES)
def test_stream_at_every_rows_per_block(gpu, H, W):
    with ru.time_limit(120):
        pu.check_shape(gpu, H, W)


def test_odd_base_addresses(gpu):
    with ru.time_limit(120):
        pu.check_odd_base_address(gpu)


def test_contents_from_zeros_to_noise(gpu):
    with ru.time_limit(120):
        pu.check_contents(gpu)


def test_fibonacci_block_is_length_limited(gpu):
    with ru.time_limit(120):
        pu.check_fibonacci(gpu)


def test_art_frames_720p_at_the_default_rows(gpu):
    """the three 1280 x 720 frames at the default 17 rows per block (43 blocks each), nearly all of them length-limited"""
    with ru.time_limit(120):
        frames = pu.art_frames()
        assert frames.shape == (3, 720, 1280, 3)
        pu.check_stream(gpu, frames, 0, "art 720p")
        limited = sum(pu.huffman(f)[1] > 15 for f in pu.block_counts(pu.paeth_filter(frames[0]), pu.default_rows(1280)))
        assert limited >= 30


def test_refusals(gpu):
    with ru.time_limit(120):
        pu.check_entry_point_rejects_bad_arguments()
        pu.check_python_refusals(gpu)
        from instantsplat_amd.png import encode_png_rgb8
        with pytest.raises(ValueError, match=r"\.to\(device\)"):
            encode_png_rgb8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))


def test_max_call_bytes_splits_into_equal_bytes(gpu):
    with ru.time_limit(120):
        pu.check_split_calls(gpu)


def test_noise_stack_720p_stays_within_the_bound(gpu):
    from instantsplat_amd import _lib
    from instantsplat_amd.png import encode_png_rgb8
    with ru.time_limit(120):
        noise = torch.randint(0, 256, (3, 720, 1280, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        enc = encode_png_rgb8(noise.to(gpu))
        data, o = enc["stream"].numpy().tobytes(), enc["offsets"]
        assert noise.numel() < int(o[-1]) <= int(_lib.lib().mi355gs_png_rgb8_stream_bytes(3, 720, 1280, 0))
        for i in range(3):
            assert np.array_equal(pu.decode(data[int(o[i]):int(o[i + 1])]), noise[i].numpy())


def test_path_frames_512(gpu):
    """12 frames of 512 x 512 as render_pose_path leaves them on the device"""
    from instantsplat_amd.png import encode_png_rgb8
    from instantsplat_amd.render_path import render_pose_path
    with ru.time_limit(240):
        st = ru.small_scene(gpu, Wm=64, Hm=64, W=512, H=512, degree=0, seed=0)
        views = ru.path_views(st, ru.short_path(ru.keyframes(st.cameras), 6), keep_images=False)[:12]
        frames = render_pose_path(views, st.gaussians, st.pipe, st.background)["frames"]
        assert frames.shape == (12, 512, 512, 3) and frames.device == gpu
    with ru.time_limit(120):
        enc = encode_png_rgb8(frames)
        pu.check_files(enc["stream"].numpy().tobytes(), enc["offsets"], frames.cpu().numpy(), 0, "path frames")


def test_stage_files_equal_pil_files_and_evaluate(gpu, tmp_path):
    with ru.time_limit(240):
        st = ru.small_scene(gpu, Wm=24, Hm=20, W=96, H=64, degree=0)
        views = ru.path_views(st, ru.short_path(ru.keyframes(st.cameras), 2))
        pu.check_render_set_device_equals_pil(gpu, st, views, tmp_path)
    with ru.time_limit(240):
        pu.check_test_set_device_files(gpu, st, tmp_path)
