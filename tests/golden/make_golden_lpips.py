"""tests/golden/lpips_vectors.npz: the reference's own `LPIPS` / `VGG16` / `LinLayers` / `normalize_activation`
(lpipsPyTorch/modules/{lpips,networks,utils}.py), executed from the reference tree (`ref_loader.REF`; build container only) in
float32 on the CPU, on a THIN VGG-shaped net with seeded weights and two 37 x 50 pairs.

What is substituted, and why (README_lpips.md):
  * `torchvision.models` -> torchvision_standin_vgg.py (not installed): the VGG16 feature stack at the widths WIDTHS;
  * `get_state_dict` (utils.py: a download) -> a function returning the seeded lin weights in the official file's naming, run
    through the reference's own renaming lines; patched in both modules BEFORE anything is constructed: nothing is fetched;
  * `get_network` (as lpips.py imported it) -> a function that builds the reference's `VGG16` and sets its `n_channels_list` —
    hard-coded 64, 128, 256, 512, 512 in networks.py — to WIDTHS, so that `LinLayers` is built for the thin net;
  * torchvision's `to_tensor` is recalled, not executed: permute(2, 0, 1).contiguous().float().div(255), then `.unsqueeze(0)`.
The weights are stored as small integers (value = integer / 64, exact in float32), the frames as bytes.
Run:  python tests/golden/make_golden_lpips.py"""
import importlib.util
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402
from tests import lpips_util as lu  # noqa: E402

WIDTHS = (32, 32, 32, 32, 32)
SCALE = 64


def quantised_states(seed=7):
    vgg, lin = lu.make_weights(WIDTHS, seed)
    q = lambda t, lo, hi: torch.clamp(torch.round(t * SCALE), lo, hi)
    vgg_q = {k: q(v, -127, 127) for k, v in vgg.items()}
    lin_q = {k: torch.clamp(q(v, 0, 32767), min=1) for k, v in lin.items()}
    return vgg_q, lin_q


def main():
    vgg_q, lin_q = quantised_states()
    spec = importlib.util.spec_from_file_location("torchvision_standin_vgg", os.path.join(HERE, "torchvision_standin_vgg.py"))
    models = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(models)
    models.WIDTHS = WIDTHS
    models.STATE = OrderedDict((k, v / SCALE) for k, v in vgg_q.items())
    tv = types.ModuleType("torchvision")
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models

    sys.path.insert(0, ref_loader.REF)
    import lpipsPyTorch.modules.utils as ref_utils
    official = OrderedDict((k, v / SCALE) for k, v in lin_q.items())   # lin{i}.model.1.weight

    def get_state_dict(net_type="alex", version="0.1"):
        assert net_type == "vgg"
        renamed = OrderedDict()
        for key, val in official.items():   # the reference's renaming (utils.py), without its download
            renamed[key.replace("lin", "").replace("model.", "")] = val
        return renamed
    ref_utils.get_state_dict = get_state_dict
    import lpipsPyTorch.modules.networks as ref_networks
    import lpipsPyTorch.modules.lpips as ref_lpips
    ref_lpips.get_state_dict = get_state_dict

    def get_network(net_type):
        assert net_type == "vgg"
        net = ref_networks.VGG16()
        net.n_channels_list = list(WIDTHS)
        return net
    ref_lpips.get_network = get_network

    torch.set_num_threads(1)
    a, b = lu.frames("mixed", 2, 37, 50, seed=9)
    criterion = ref_lpips.LPIPS("vgg", "0.1")
    to_tensor = lambda u8: torch.from_numpy(u8).permute(2, 0, 1).contiguous().float().div(255).unsqueeze(0)
    totals, taps = [], []
    with torch.no_grad():
        for i in range(2):
            x, y = to_tensor(a[i]), to_tensor(b[i])
            totals.append(float(criterion(x, y).reshape(())))
            fx, fy = criterion.net(x), criterion.net(y)
            taps.append([float(l((p - q) ** 2).mean((2, 3), True).reshape(())) for p, q, l in zip(fx, fy, criterion.lin)])
    out = dict(lpips_channels=np.array(WIDTHS, np.int32), lpips_weight_scale=np.float32(SCALE), lpips_renders=a, lpips_gts=b,
               lpips_total=np.array(totals, np.float32), lpips_taps=np.array(taps, np.float32))
    for n in lu.CONV_LAYERS:
        out[f"lpips_conv{n}_weight_q"] = vgg_q[f"features.{n}.weight"].numpy().astype(np.int8)
        out[f"lpips_conv{n}_bias_q"] = vgg_q[f"features.{n}.bias"].numpy().astype(np.int8)
    for i in range(5):
        out[f"lpips_lin{i}_q"] = lin_q[f"lin{i}.model.1.weight"].reshape(-1).numpy().astype(np.int16)
    path = os.path.join(HERE, "lpips_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; totals", totals, "taps", taps)


if __name__ == "__main__":
    main()
