"""The device JPEG encoder and the MJPEG stage (instantsplat_amd/jpeg.py, instantsplat_amd/video.py, csrc/jpeg.hip) on the MI355X.
The checks are tests/jpeg_util.py's: whole files against the host restatement and against PIL, byte for byte.  Every step runs
under a time limit of its own."""
import numpy as np
import pytest
import torch

from tests import jpeg_util as ju
from tests import render_path_util as ru

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H,W", ju.SHAPES)
def test_files_equal_restatement_and_pil(gpu, H, W):
    with ru.time_limit(120):
        ju.check_shape(gpu, H, W)


def test_stacks_and_addresses(gpu):
    with ru.time_limit(120):
        ju.check_stacks_and_addresses(gpu)


def test_capacity_protocol(gpu):
    with ru.time_limit(120):
        ju.check_capacity(gpu)


def test_refusals(gpu, tmp_path):
    with ru.time_limit(120):
        ju.check_entry_point_rejects_bad_arguments()
        ju.check_python_refusals(gpu)
        ju.check_write_files(gpu, tmp_path)
        from instantsplat_amd.jpeg import encode_jpeg_rgb8
        with pytest.raises(ValueError, match=r"\.to\(device\)"):
            encode_jpeg_rgb8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))


@pytest.mark.parametrize("subsampling", ju.SUBSAMPLINGS)
def test_art_frames_720p(gpu, subsampling):
    """the three 1280 x 720 frames at quality 90: 90 / 45 restart intervals of 480 blocks each, whole files against PIL's"""
    with ru.time_limit(120):
        frames = ju.art_frames()
        assert frames.shape == (3, 720, 1280, 3)
        ju.check_device_files(gpu, frames, 90, subsampling, "art 720p", restate=False)


def test_path_frames_512(gpu):
    """12 frames of 512 x 512 as render_pose_path leaves them on the device"""
    from instantsplat_amd.jpeg import encode_jpeg_rgb8
    from instantsplat_amd.render_path import render_pose_path
    with ru.time_limit(240):
        st = ru.small_scene(gpu, Wm=64, Hm=64, W=512, H=512, degree=0, seed=0)
        views = ru.path_views(st, ru.short_path(ru.keyframes(st.cameras), 6), keep_images=False)[:12]
        frames = render_pose_path(views, st.gaussians, st.pipe, st.background)["frames"]
        assert frames.shape == (12, 512, 512, 3) and frames.device == gpu
    with ru.time_limit(120):
        host = frames.cpu().numpy()
        for sub in ju.SUBSAMPLINGS:
            enc = encode_jpeg_rgb8(frames, quality=90, subsampling=sub)
            assert ju.split_files(enc["stream"].numpy().tobytes(), enc["offsets"]) == [ju.pil_encode(f, 90, sub) for f in host]


def test_noise_stack_720p_stays_within_the_bound(gpu):
    """quality 100 on noise: every interval far beyond one round of staging, the files beyond the default capacity"""
    from instantsplat_amd import _lib
    from instantsplat_amd.jpeg import encode_jpeg_rgb8
    with ru.time_limit(240):
        noise = torch.randint(0, 256, (3, 720, 1280, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        for sub in ju.SUBSAMPLINGS:
            enc = encode_jpeg_rgb8(noise.to(gpu), quality=100, subsampling=sub)
            o = enc["offsets"]
            assert int(o[-1]) <= int(_lib.lib().mi355gs_jpeg_rgb8_stream_bytes(3, 720, 1280, ju.sub_code(sub)))
            files = ju.split_files(enc["stream"].numpy().tobytes(), o)
            for i in range(3):
                want = ju.pil_encode(noise[i].numpy(), 100, sub)
                assert files[i] == want, (sub, i, len(files[i]), len(want), ju.first_difference(files[i], want))


def test_stage_writes_the_video_beside_the_png_files(gpu, tmp_path):
    with ru.time_limit(240):
        st = ru.small_scene(gpu, Wm=24, Hm=20, W=96, H=64, degree=0)
        ju.check_stage(gpu, st, tmp_path)
