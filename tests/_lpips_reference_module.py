"""The reference's own LPIPS module on synthetic weights, with every download path closed -- TEST INFRASTRUCTURE ONLY.

`reference_lpips(features, lin)` is a context manager: inside it `torchvision.models` is a stub whose `vgg16(...)` returns the real
architecture loaded from `features`, `lpipsPyTorch.modules.lpips.get_state_dict` returns `lin` in the reference's renamed key form, and
`torch.hub.load_state_dict_from_url` raises.  It yields `make(dtype)` -> the reference's `LPIPS('vgg')` in eval mode (for float64 the
module is converted and its mean / std buffers are set to the exact constants).  Usable only where a checkout of the reference exists."""
import contextlib
import os
import sys
import types

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)


def available() -> bool:
    return os.path.isdir(os.path.join(ref_import.REFERENCE_ROOT, "lpipsPyTorch"))


def vgg16_architecture(features):
    """torchvision's vgg16() as far as the reference reads it: an object whose `.features` is the nn.Sequential of 31 modules."""
    layers, cin = [], 3
    for v in CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    seq = nn.Sequential(*layers)
    seq.load_state_dict({k[len("features."):] if k.startswith("features.") else k: v for k, v in features.items()})
    return types.SimpleNamespace(features=seq)


@contextlib.contextmanager
def reference_lpips(features, lin):
    if not available():
        raise RuntimeError("reference tree not present")
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.models")}
    models = types.ModuleType("torchvision.models")
    models.vgg16 = lambda *a, **k: vgg16_architecture(features)
    models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1="IMAGENET1K_V1")
    tv = types.ModuleType("torchvision")
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models
    added_path = ref_import.REFERENCE_ROOT not in sys.path
    if added_path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    real_hub = torch.hub.load_state_dict_from_url

    def no_download(*a, **k):
        raise AssertionError("the test reached a download path")

    torch.hub.load_state_dict_from_url = no_download
    try:
        import lpipsPyTorch.modules.lpips as ref_lpips
        real_get = ref_lpips.get_state_dict
        renamed = {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}        # utils.py:23-28
        ref_lpips.get_state_dict = lambda *a, **k: renamed

        def make(dtype=torch.float32):
            crit = ref_lpips.LPIPS("vgg").eval()
            if dtype == torch.float64:
                crit = crit.double()
                with torch.no_grad():
                    crit.net.mean.copy_(torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1))
                    crit.net.std.copy_(torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1))
            return lambda x, y: crit(x, y).detach()

        try:
            yield make
        finally:
            ref_lpips.get_state_dict = real_get
    finally:
        torch.hub.load_state_dict_from_url = real_hub
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        for k in [k for k in sys.modules if k == "lpipsPyTorch" or k.startswith("lpipsPyTorch.")]:
            del sys.modules[k]
        if added_path:
            sys.path.remove(ref_import.REFERENCE_ROOT)
