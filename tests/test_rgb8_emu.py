"""mi355gs_rgb8_from_planar (csrc/path.hip) under the SIMT emulator against torchvision.utils.save_image's quantisation spelled
out in torch, x.mul(255).add_(0.5).clamp_(0, 255).to(uint8): every byte equal."""
import pytest
import torch

from tests import render_path_util as ru


@pytest.mark.parametrize("H,W", [(1, 1), (23, 37), (64, 48), (16, 4096)])
def test_rgb8_equals_torch_expression(emu, H, W):
    ru.check_rgb8_equals_torch(emu, H, W, seeds=(0, 1))


def test_rgb8_every_special_value(emu):
    ru.check_rgb8_special_values_each(emu)


def test_rgb8_nan_gives_zero(emu):
    ru.check_rgb8_nan_is_zero(emu)


def test_rgb8_misaligned_pointers_take_the_plain_path(emu):
    ru.check_rgb8_misaligned_pointers_take_the_plain_path(emu)


def test_rgb8_rejects_bad_arguments(emu):
    ru.check_rgb8_rejects_bad_arguments()


def test_rgb8_output_buffer_and_shapes(emu):
    from instantsplat_amd.render_path import quantize_rgb8
    x = ru.rgb8_input(6, 10, 5)
    out = torch.full((6, 10, 3), 7, dtype=torch.uint8)
    assert quantize_rgb8(x, out=out) is out and torch.equal(out, ru.torch_rgb8(x))
    assert torch.equal(quantize_rgb8(x.permute(0, 2, 1)), ru.torch_rgb8(x.permute(0, 2, 1)))   # made contiguous first
    with pytest.raises(ValueError):
        quantize_rgb8(x, out=torch.zeros(10, 6, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        quantize_rgb8(x[0])


def test_quantize_rgb8_refuses_cpu_tensors():
    """no emulator: the product path has no CPU fallback"""
    from instantsplat_amd import _lib
    from instantsplat_amd.render_path import quantize_rgb8
    _lib._use_library_for_testing(None)
    with pytest.raises(RuntimeError, match="GPU only"):
        quantize_rgb8(torch.zeros(3, 4, 4))
