"""tests/golden/load_images_vectors.npz: the reference's own `load_images` (utils/sfm_utils.py:123-176) with its
`_resize_pil_image` (dust3r/utils/image.py:63-70) and its `ImgNorm`, executed from the reference tree (`ref_loader.REF`; build
container only) on the three example frames (tests/golden/sora_art) and on the synthetic PNG files of
tests/resample_util.py::write_synthetic_files, at size 512 / 64 (with and without square_ok) and 224, folder and list forms.

utils/sfm_utils.py cannot be imported whole here (cv2, open3d, roma, torchvision ...): the two function definitions and the
`ImgNorm` assignment are taken from the files as source segments and executed in a namespace that holds what they name.
What is substituted, and why (README_load_images.md):
  * `torchvision.transforms` -> torchvision_standin_transforms.py (not installed);
  * `heif_support_enabled` -> False (pillow_heif is not installed; the reference's own value without it).
Stored: per case the shapes, the returned size, idx / instance and a SHA-256 of every image tensor's float32 bytes — no tensors.
Run:  python tests/golden/make_golden_load_images.py"""
import hashlib
import importlib.util
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402
from tests import resample_util as ru  # noqa: E402


def reference_load_images():
    import PIL.Image
    import torch
    from PIL.ImageOps import exif_transpose
    spec = importlib.util.spec_from_file_location("torchvision_standin_transforms", os.path.join(HERE, "torchvision_standin_transforms.py"))
    tvf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tvf)
    ns = dict(os=os, np=np, torch=torch, PIL=PIL, exif_transpose=exif_transpose, tvf=tvf, heif_support_enabled=False)
    image_py = os.path.join(ref_loader.REF, "dust3r", "utils", "image.py")
    sfm_py = os.path.join(ref_loader.REF, "utils", "sfm_utils.py")
    exec(ref_loader.function_sources(image_py, {"_resize_pil_image"})["_resize_pil_image"], ns)
    exec(ref_loader.assignment_sources(sfm_py, {"ImgNorm"}), ns)
    exec(ref_loader.function_sources(sfm_py, {"load_images"})["load_images"], ns)
    return ns["load_images"]


def main():
    load_images = reference_load_images()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ru.write_synthetic_files(tmp)
        for key, arg, size, square_ok in ru.golden_cases(tmp):
            imgs, last = load_images(arg, size, square_ok=square_ok, verbose=False)
            out[f"li_{key}_shapes"] = np.concatenate([v["true_shape"] for v in imgs]).astype(np.int32)
            out[f"li_{key}_last_size"] = np.int32(last)
            out[f"li_{key}_idx"] = np.int32([v["idx"] for v in imgs])
            out[f"li_{key}_instance"] = np.array([v["instance"] for v in imgs])
            out[f"li_{key}_sha256"] = np.array([hashlib.sha256(v["img"].contiguous().numpy().tobytes()).hexdigest() for v in imgs])
            assert all(v["img"].dtype.is_floating_point and v["img"].element_size() == 4 and tuple(v["img"].shape[:2]) == (1, 3) for v in imgs)
    path = os.path.join(HERE, "load_images_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
