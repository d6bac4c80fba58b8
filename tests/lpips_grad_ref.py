"""tests/lpips_ref.py's lpips() restated so that its ReLU and max-pool DECISIONS can be frozen, for the gradient tests.

A gradient through ReLU and max pool is discontinuous in the decisions: an activation within rounding of zero, or a tie in a pool
window, can fall the other way in float32 than in float64, and the gradient then differs by a whole path's contribution, not by
rounding. So the decisions come from outside, per picture, as that picture's 13 post-ReLU maps from some run (`maps`):
  ReLU   becomes a multiplication by (maps[l] > 0),
  pool   becomes a gather at the first-max indices of the frozen map in front of it, F.max_pool2d(maps[l], 2, 2,
         return_indices=True) -- torch's rule, `val > maxval`, the first maximum in row-major order.
With the decisions frozen the function is smooth in x, and what is left between two evaluations is rounding. `maps=None` makes the
picture's own decisions (F.relu, F.max_pool2d): lpips_ref.lpips itself, which test_lpips_backward_cpu.py checks."""
import torch
import torch.nn.functional as F

from tests import lpips_ref

POOL_BEHIND = (1, 3, 6, 9)  # the convolutions (counted from 0) whose ReLU output a pool follows: the first four taps
TAP_LAYERS = (1, 3, 6, 9, 12)


def activations(x, feats, dtype, maps=None, reroute=None):
    """x [N,3,H,W] -> the 13 post-ReLU maps, under the decisions of `maps` (None: its own). `reroute(l, where) -> indices` (with
    frozen decisions only) sends the pool's gradient behind map l elsewhere than its value comes from: for the test that shows a
    wrong pool winner to the comparison."""
    x = x.to(dtype)
    mean = torch.tensor(lpips_ref.MEAN, dtype=torch.float32).to(dtype)[None, :, None, None]
    std = torch.tensor(lpips_ref.STD, dtype=torch.float32).to(dtype)[None, :, None, None]
    x = (x - mean) / std
    out = []
    for l, idx in enumerate(lpips_ref.CONV_INDICES):
        x = F.conv2d(x, feats[f"{idx}.weight"].to(dtype), feats[f"{idx}.bias"].to(dtype), padding=1)
        x = F.relu(x) if maps is None else x * (maps[l] > 0).to(dtype)
        out.append(x)
        if l in POOL_BEHIND:
            if maps is None:
                x = F.max_pool2d(x, 2, 2)
            else:
                _, where = F.max_pool2d(maps[l].detach(), 2, 2, return_indices=True)
                picked = x.flatten(2).gather(2, where.flatten(2)).view(where.shape)
                if reroute is not None:
                    other = x.flatten(2).gather(2, reroute(l, where).flatten(2)).view(where.shape)
                    picked = picked.detach() + other - other.detach()
                x = picked
    return out


def value(ax, ay, lin, dtype):
    """the 13 maps of both pictures -> the [1,1,1,1] value, as lpips_ref.lpips forms it"""
    res = []
    for k, l in enumerate(TAP_LAYERS):
        d = (lpips_ref.normalize_activation(ax[l]) - lpips_ref.normalize_activation(ay[l])) ** 2
        res.append(F.conv2d(d, lin[f"lin{k}.model.1.weight"].to(dtype)).mean((2, 3), True))
    return torch.sum(torch.cat(res, 0), 0, True)


def lpips_grad(x, y, weights, dtype, x_maps=None, y_maps=None):
    """-> (value [1,1,1,1], d value / d x [N,3,H,W], x's 13 maps), all detached, in `dtype`, by torch.autograd"""
    x = x.detach().to(dtype).requires_grad_(True)
    ax = activations(x, weights["features"], dtype, x_maps)
    with torch.no_grad():
        ay = activations(y.detach(), weights["features"], dtype, y_maps)
    v = value(ax, ay, weights["lin"], dtype)
    g, = torch.autograd.grad(v.sum(), x)
    return v.detach(), g, [a.detach() for a in ax]
