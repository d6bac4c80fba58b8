"""LPIPS (VGG16, version 0.1) restated in plain torch for the tests: lpipsPyTorch/modules/networks.py:41-64 and :89-96 (z-score,
vgg16().features, the outputs of layers 4, 9, 16, 23, 30 counted from 1), modules/utils.py:6-8 (normalize_activation) and
modules/lpips.py:30-36 (squared difference, the 1x1 `lin` convolution, the spatial mean, torch.sum(torch.cat(res, 0), 0, True)).
The reference package itself needs torchvision for the network definition; this needs F.conv2d and F.max_pool2d only, and runs on
the CPU in whatever dtype it is asked for (float64: the yardstick; float32: what the reference computes)."""
import torch
import torch.nn.functional as F

CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)
# vgg16().features: 'M' = MaxPool2d(2, 2); every convolution is followed by a ReLU
CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
TARGET_LAYERS = (4, 9, 16, 23, 30)
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)


def features(x, feats, dtype):
    """x [N,3,H,W] -> the five tap maps (before normalize_activation), the layers walked as BaseNet.forward walks them"""
    x = x.to(dtype)
    mean = torch.tensor(MEAN, dtype=torch.float32).to(dtype)[None, :, None, None]
    std = torch.tensor(STD, dtype=torch.float32).to(dtype)[None, :, None, None]
    x = (x - mean) / std
    layers = []  # the modules of vgg16().features, by index
    for v in CFG:
        layers += ["pool"] if v == "M" else [("conv", len(layers)), "relu"]
    assert tuple(m[1] for m in layers if m[0] == "conv") == CONV_INDICES
    out = []
    for i, m in enumerate(layers, 1):
        if m == "pool":
            x = F.max_pool2d(x, 2, 2)
        elif m == "relu":
            x = F.relu(x)
        else:
            x = F.conv2d(x, feats[f"{m[1]}.weight"].to(dtype), feats[f"{m[1]}.bias"].to(dtype), padding=1)
        if i in TARGET_LAYERS:
            out.append(x)
        if len(out) == len(TARGET_LAYERS):
            break
    return out


def normalize_activation(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def lpips(x, y, weights, dtype):
    """-> (value [1,1,1,1], per-tap values [5] each summed over the batch, x's tap maps)"""
    fx, fy = features(x, weights["features"], dtype), features(y, weights["features"], dtype)
    res = []
    for k, (a, b) in enumerate(zip(fx, fy)):
        d = (normalize_activation(a) - normalize_activation(b)) ** 2
        res.append(F.conv2d(d, weights["lin"][f"lin{k}.model.1.weight"].to(dtype)).mean((2, 3), True))
    value = torch.sum(torch.cat(res, 0), 0, True)
    taps = torch.stack([r.sum() for r in res])
    return value, taps, fx
