"""Torch restatement of the reference's metamer, written from
  metamer/odak_perception/metamer_mse_loss.py:63-123 (gen_metamer, with avg_pooling_downup=True) and :125-152 (the loss),
  metamer/odak_perception/spatial_steerable_pyramid.py:182-223 (reconstruct_from_pyramid, use_bilinear_downup=True),
  metamer/odak_perception/color_conversion.py:405-428 (ycrcb_2_rgb).
The pyramid, the LOD maps and the blended statistics are tests/hvs_ref.py's and tests/hvs_fov_ref.py's; the filters AND THE NOISE
are arguments (the reference draws the noise from torch's global generator, whose numbers depend on the device and the build).
It runs in whatever dtype its inputs have: float64 on the CPU is the yardstick of the tests.
`drop` names one piece of the pyramid to leave out of the synthesis ("h", or (level, band)): a synthesis that forgets that piece.
"""
import torch
import torch.nn.functional as F

from tests import hvs_fov_ref, hvs_ref

RMS_FLOOR = 1e-6


def ycrcb_2_rgb(x):
    """color_conversion.py:424-427"""
    y, cr, cb = x[:, 0], x[:, 1] - 0.5, x[:, 2] - 0.5
    return torch.stack([y + 1.403 * cr, y - 0.714 * cr - 0.344 * cb, y + 1.773 * cb], dim=1)


def match_level(level, target_mean, target_std):
    """metamer_mse_loss.py:97-107: ONE mean and ONE root mean square over the whole band (all channels)"""
    level = level - level.mean()
    rms = torch.sqrt((level * level).mean())
    rms = torch.where(rms < RMS_FLOOR, torch.full_like(rms, RMS_FLOOR), rms)
    return level / rms * target_std + target_mean


def reconstruct(h, bands, low, filters, drop=None):
    """spatial_steerable_pyramid.py:207-223: from the coarsest level up, image = bilinear-up(image) + sum_b conv(pad(band_b), -b_b);
    then conv(pad(image), l0) + conv(pad(h), h0)"""
    image = low
    for l in reversed(range(len(bands))):
        image = F.interpolate(image, size=bands[l][0].shape[-2:], mode="bilinear", align_corners=False)
        for b, band in enumerate(bands[l]):
            if drop == (l, b):
                continue
            image = image + hvs_ref._conv(band, -filters["b"][b])
    image = hvs_ref._conv(image, filters["l0"])
    if drop != "h":
        image = image + hvs_ref._conv(h, filters["h0"])
    return image


def roundtrip(x, filters, n_levels, image_colorspace="RGB", drop=None):
    """reconstruct_from_pyramid(construct_pyramid(x)); RGB: converted on the way in and back on the way out"""
    hvs_ref.check_size(x.size(2), x.size(3), n_levels)
    rgb = image_colorspace == "RGB"
    h, bands, low = hvs_ref.pyramid(hvs_ref.rgb_2_ycrcb(x) if rgb else x, filters, n_levels)
    out = reconstruct(h, bands, low, filters, drop)
    return ycrcb_2_rgb(out) if rgb else out


def gen_metamer(target, noise, filters, gaze=(0.5, 0.5), alpha=0.2, real_image_width=0.2, real_viewing_distance=0.7, n_pyramid_levels=5,
                mode="quadratic", image_colorspace="RGB", drop=None):
    """metamer_mse_loss.py:63-123 with the noise as an input -> [1,3,H,W], RGB"""
    hvs_ref.check_size(target.size(2), target.size(3), n_pyramid_levels)
    x = hvs_ref.rgb_2_ycrcb(target) if image_colorspace == "RGB" else target
    lods = hvs_fov_ref.lod_maps(gaze, x.size(2), x.size(3), n_pyramid_levels, alpha, real_image_width, real_viewing_distance, mode,
                                x.dtype, x.device)
    stats = hvs_fov_ref.stats_maps(x, filters, lods, n_pyramid_levels)
    means, stds = stats[:-1:2], stats[1:-1:2]
    h, bands, _ = hvs_ref.pyramid(noise, filters, n_pyramid_levels)
    h = match_level(h, means[0], stds[0])
    nb = len(filters["b"])
    bands = [[match_level(band, means[1 + l * nb + b], stds[1 + l * nb + b]) for b, band in enumerate(level)] for l, level in enumerate(bands)]
    return ycrcb_2_rgb(reconstruct(h, bands, stats[-1], filters, drop))


def loss(image, metamer, loss_type):
    """metamer_mse_loss.py:152"""
    return F.mse_loss(image, metamer) if loss_type == "MSE" else F.l1_loss(image, metamer)
