"""What the reference's `ImgNorm` (utils/sfm_utils.py:37-40, dust3r/utils/image.py:23) touches of `torchvision.transforms` (not
installed here), written from torchvision's documented behaviour for an 8-bit RGB PIL image:
  * `ToTensor`: the image's bytes as a [C,H,W] tensor, `.to(float32).div(255)`;
  * `Normalize(mean, std)`: a float32 copy, `sub_(mean[:, None, None]).div_(std[:, None, None])` with mean / std as float32 tensors;
  * `Compose`: the transforms in order.
Test infrastructure; never imported by the product."""
import numpy as np
import torch


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class ToTensor:
    def __call__(self, pic):
        assert pic.mode == "RGB"
        img = torch.from_numpy(np.array(pic, np.uint8, copy=True)).view(pic.size[1], pic.size[0], 3)
        return img.permute((2, 0, 1)).contiguous().to(dtype=torch.float32).div(255)


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, tensor):
        tensor = tensor.clone()
        mean = torch.as_tensor(self.mean, dtype=tensor.dtype).view(-1, 1, 1)
        std = torch.as_tensor(self.std, dtype=tensor.dtype).view(-1, 1, 1)
        return tensor.sub_(mean).div_(std)
