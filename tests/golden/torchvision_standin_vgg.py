"""What the reference's lpipsPyTorch/modules/networks.py touches of `torchvision.models` (not installed here) on its 'vgg' path:
`models.vgg16(weights=models.VGG16_Weights.IMAGENET1K_V1).features`, written from torchvision's documented VGG16 (configuration
"D"): convolutions 3x3 / padding 1 each followed by ReLU(inplace), 2, 2, 3, 3, 3 of them, a MaxPool2d(2, 2) behind every block —
31 feature layers, the convolutions at indices 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28.

The block WIDTHS are a module variable (torchvision's are 64, 128, 256, 512, 512) and the "pretrained" weights are whatever
STATE holds (`features.N.weight` / `.bias`): the generator of tests/golden/lpips_vectors.npz sets both before anything is
constructed.  Nothing is downloaded.  Test infrastructure; never imported by the product."""
import torch.nn as nn

WIDTHS = (64, 128, 256, 512, 512)
STATE = None


class VGG16_Weights:
    IMAGENET1K_V1 = "IMAGENET1K_V1"


class _VGG(nn.Module):
    def __init__(self):
        super().__init__()
        layers, cin = [], 3
        for width, count in zip(WIDTHS, (2, 2, 3, 3, 3)):
            for _ in range(count):
                layers += [nn.Conv2d(cin, width, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = width
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        self.features = nn.Sequential(*layers)


def vgg16(weights=None, **kwargs):
    net = _VGG()
    if weights is not None:
        if STATE is None:
            raise RuntimeError("torchvision_standin_vgg.STATE is not set: there are no pretrained weights to load offline")
        net.load_state_dict(STATE)
    return net
