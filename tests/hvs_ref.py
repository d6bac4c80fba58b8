"""Torch restatement of the reference's uniform metameric (HVS) loss, written from
  metamer/odak_perception/metameric_loss_uniform.py:8-12 (uniform_blur), :46-88 (calc_statsmaps), :90-100 (the loss),
  metamer/odak_perception/spatial_steerable_pyramid.py:132-180 (construct_pyramid, bilinear_downsampling=True),
  metamer/odak_perception/color_conversion.py:382-404 (rgb_2_ycrcb).
The filter coefficients are an ARGUMENT (a dict in the layout of get_steerable_pyramid_filters: "l0", "h0" [1,1,5,5], "b" a list
of [1,1,5,5]); this file holds none. It runs in whatever dtype / device its inputs have: float64 on the CPU is the yardstick
of the tests, float32 on the GPU the timing baseline of tools/hvs_bench.py. Each channel is filtered on its own (a grouped
convolution): the reference's dense 3->3 filters are zero off the diagonal, so the sums are the same numbers.
"""
import math

import torch
import torch.nn.functional as F

VAR_FLOOR = 1e-7


def rgb_2_ycrcb(image):
    """color_conversion.py:400-403"""
    r, g, b = image[:, 0], image[:, 1], image[:, 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    return torch.stack([y, 0.5 + 0.713 * (r - y), 0.5 + 0.564 * (b - y)], dim=1)


def n_stats(n_levels, n_orientations):
    return 2 * (1 + (n_levels - 1) * n_orientations) + 1


def pooled_size(n, pooling):
    """interpolate(scale_factor=1/p, mode="area") without recompute_scale_factor: floor(n * (1/p)) in double"""
    return int(math.floor(float(n) * (1.0 / pooling)))


def window(j, n, n_out):
    """adaptive average pooling's window of output j: [floor(j n / n'), ceil((j+1) n / n'))"""
    return (j * n) // n_out, -((-(j + 1) * n) // n_out)


def _conv(x, filt):
    c = x.size(1)
    w = filt.to(dtype=x.dtype, device=x.device).reshape(1, 1, 5, 5).expand(c, 1, 5, 5)
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), w, groups=c)


def uniform_blur(x, pooling):
    """metameric_loss_uniform.py:8-12"""
    down = F.interpolate(x, scale_factor=1.0 / pooling, mode="area")
    return F.interpolate(down, size=x.shape[-2:], mode="bilinear")


def find_stats(x, pooling):
    """metameric_loss_uniform.py:57-69 -> (mean, std, var before the clamp)"""
    mean = uniform_blur(x, pooling)
    var = uniform_blur(x * x, pooling) - mean * mean
    std = torch.sqrt(torch.where(var < VAR_FLOOR, torch.full_like(var, VAR_FLOOR), var))
    return mean, std, var


def pyramid(x, filters, n_levels):
    """spatial_steerable_pyramid.py:132-180 -> (h, [bands of level 0, bands of level 1, ...], last lowpass)"""
    h = _conv(x, filters["h0"])
    low = _conv(x, filters["l0"])
    bands = []
    for _ in range(n_levels - 1):
        bands.append([_conv(low, fb) for fb in filters["b"]])
        low = F.interpolate(low, scale_factor=0.5, mode="area", recompute_scale_factor=False)
    return h, bands, low


def stats_maps(x, filters, pooling, n_levels, want_vars=False):
    """metameric_loss_uniform.py:71-88: [mean h, std h, (mean, std) per band per level ..., last lowpass]"""
    h, bands, low = pyramid(x, filters, n_levels)
    out, variances = [], []
    p = float(pooling)
    m, s, v = find_stats(h, p)
    out += [m, s]
    variances.append(v)
    for level in bands:
        for b in level:
            m, s, v = find_stats(b, p)
            out += [m, s]
            variances.append(v)
        p /= 2
    out.append(low)
    return (out, variances) if want_vars else out


def check_size(h, w, n_levels):
    d = 2 ** n_levels
    if h % d or w % d:
        raise ValueError("Please make the image size valid (Multiplies of 2 ** n_pyramid_levels) before input to HVS function.")


def hvs_loss(image, target, filters, pooling_size, n_pyramid_levels=5, loss_type="L1", image_colorspace="RGB", return_maps=False):
    """MetamericLossUniform.__call__ (:135-156): image, target [1,3,H,W]; autograd to image only."""
    check_size(image.size(2), image.size(3), n_pyramid_levels)
    target = target.detach()
    if image_colorspace == "RGB":
        image, target = rgb_2_ycrcb(image), rgb_2_ycrcb(target)
    a = stats_maps(image, filters, pooling_size, n_pyramid_levels)
    with torch.no_grad():
        b = stats_maps(target, filters, pooling_size, n_pyramid_levels)
    loss = 0.0
    for x, y in zip(a, b):
        loss = loss + (F.mse_loss(x, y) if loss_type == "MSE" else F.l1_loss(x, y))
    loss = loss / len(a)
    return (loss, a) if return_maps else loss


def variances_outside_band(image, target, filters, pooling_size, n_pyramid_levels, lo=2e-8, hi=5e-7, image_colorspace="RGB"):
    """number of pooled variances of either picture in [lo, hi]: the tests' inputs keep the clamp away from its kink"""
    n = 0
    with torch.no_grad():
        for x in (image, target):
            if image_colorspace == "RGB":
                x = rgb_2_ycrcb(x)
            for v in stats_maps(x, filters, pooling_size, n_pyramid_levels, want_vars=True)[1]:
                n += int(((v >= lo) & (v <= hi)).sum())
    return n


UNDECIDED = 1e-9


def undecided_sign_gradient(image, target, filters, pooling_size, n_pyramid_levels, threshold=UNDECIDED, image_colorspace="RGB"):
    """|a - b| has a kink at a = b. The reference's float32 statistics are 1e-9 .. 5e-9 rms (up to 7e-8) off their float64 values
    (measured on these cases), so where a statistic of the image and of the target differ by a few 1e-9 a float32 evaluation
    takes either sign, and ONE flipped sign moves the L1 gradient by 1e-4 .. 1e-3 of its maximum. A picture of 10^5 .. 10^6
    statistics has 5 .. 25 differences below 3e-9, whatever the seed, so float32 evaluations differ there by chance. The library
    therefore evaluates its statistics with double sums (csrc/hvs.hip), an order of magnitude closer to float64, and the
    fixtures keep clear of what remains: -> (number of statistics with |a - b| < threshold, max |gradient of their share of the
    loss| / max |gradient of the loss|), in the precision of the inputs. (Bands of odd filters vanish at a reflected border in
    both pictures: elements there can be below the threshold and carry no gradient, so the second figure is what matters.)"""
    img = image.detach().clone().requires_grad_(True)
    x, t = (rgb_2_ycrcb(img), rgb_2_ycrcb(target)) if image_colorspace == "RGB" else (img, target)
    a = stats_maps(x, filters, pooling_size, n_pyramid_levels)
    with torch.no_grad():
        b = stats_maps(t, filters, pooling_size, n_pyramid_levels)
    full, part, n = 0.0, 0.0, 0
    for u, v in zip(a, b):
        d = (u - v).abs()
        sel = (d < threshold).detach()
        n += int(sel.sum())
        full = full + d.mean() / len(a)
        part = part + (d * sel).sum() / d.numel() / len(a)
    g_full, = torch.autograd.grad(full, img, retain_graph=True)
    g_part, = torch.autograd.grad(part, img)
    return n, float(g_part.abs().max() / g_full.abs().max())


def decode_u16(q):
    """the float32 picture of a 16-bit fixture picture (tests/golden/make_hvs_golden.py ran the reference on exactly these values)"""
    import numpy as np
    return np.asarray(q).astype(np.float32) / np.float32(65535)


def filters_from_npz(z, n_orientations, prefix="filters"):
    """prefix "filters": the reference's own sets (ref_hvs.npz); "afilters": the asymmetric sets of ref_hvs_edges.npz"""
    return {"l0": torch.tensor(z[f"{prefix}{n_orientations}_l0"]), "h0": torch.tensor(z[f"{prefix}{n_orientations}_h0"]),
            "b": [torch.tensor(b) for b in z[f"{prefix}{n_orientations}_b"]]}


def filters_to(filters, dtype=None, device=None):
    return {"l0": filters["l0"].to(dtype=dtype, device=device), "h0": filters["h0"].to(dtype=dtype, device=device),
            "b": [b.to(dtype=dtype, device=device) for b in filters["b"]]}
