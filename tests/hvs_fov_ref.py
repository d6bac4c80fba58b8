"""Torch restatement of the reference's foveated (gaze-dependent) metameric loss, written from
  metamer/odak_perception/foveation.py:6-39 (make_3d_location_map), :42-91 (make_eccentricity_distance_maps),
                                       :94-146 (make_pooling_size_map_pixels), :149-179 (make_pooling_size_map_lod),
  metamer/odak_perception/radially_varying_blur.py:61-98 (the LOD map of one size), :100-109 (the mip chain),
                                       :111-118 (every level straight to full size), :120-140 (the blend),
  metamer/odak_perception/metameric_loss.py:86-167 (calc_statsmaps with use_l2_foveal_loss=False, use_fullres_l0=False),
                                       :169-191 (the loss without the radial weight), :204-271 (__call__).
The pyramid, the colour conversion and the variance floor are tests/hvs_ref.py's; the filters are an ARGUMENT. It runs in
whatever dtype / device its inputs have: float64 on the CPU is the yardstick of the tests, float32 on the GPU the timing
baseline of tools/hvs_bench.py --foveated.
Not reproduced: the reference keeps the target's statistics of the PREVIOUS gaze when only the gaze changes (:239-249); here
both pictures are always evaluated with the gaze of the call.
"""
import math

import torch
import torch.nn.functional as F

from tests import hvs_ref

VAR_FLOOR = hvs_ref.VAR_FLOOR


def _eccentricity_distance(gaze, size, width, distance, dtype, device):
    """foveation.py:6-39, :70-91 -> (eccentricity [h,w] in radians, distance to the pixel [h,w])"""
    h, w = size
    height = (width / w) * h
    x = torch.linspace(-0.5, 0.5, w, dtype=dtype, device=device) * width
    y = torch.linspace(-0.5, 0.5, h, dtype=dtype, device=device) * height
    loc = torch.stack([x[None, :].expand(h, w), y[:, None].expand(h, w), torch.full((h, w), distance, dtype=dtype, device=device)])
    dist = torch.sqrt((loc * loc).sum(0))
    g = torch.tensor([(gaze[0] * 2 - 1) * width * 0.5, (gaze[1] * 2 - 1) * height * 0.5, distance], dtype=dtype, device=device)
    g = g / torch.sqrt((g * g).sum())
    dot = torch.clamp((g[:, None, None] * (loc / dist)).sum(0), min=-1.0, max=1.0)
    return torch.acos(dot), dist


def pooling_size_map_pixels(gaze, size, alpha, width, distance, mode, dtype=torch.float64, device="cpu"):
    """foveation.py:123-146: gaze[0] is x, gaze[1] is y; the ellipse's major axis is laid around the eccentricity from the
    picture's CENTRE (:125-126), whatever the gaze"""
    ecc, dist = _eccentricity_distance(gaze, size, width, distance, dtype, device)
    ecc_centre, _ = _eccentricity_distance([0.5, 0.5], size, width, distance, dtype, device)
    rad = alpha * ecc
    if mode == "quadratic":
        rad = rad * ecc
    major = (torch.tan(ecc_centre + rad * 0.5) - torch.tan(ecc_centre - rad * 0.5)) * distance
    minor = 2 * dist * torch.tan(rad * 0.5)
    area = torch.abs(math.pi * major * minor * 0.25)
    return (torch.sqrt(area) / width) * size[1]


def lod_map(gaze, size, alpha, width, distance, mode, dtype=torch.float64, device="cpu"):
    """foveation.py:174-179"""
    lod = torch.log2(1e-6 + pooling_size_map_pixels(gaze, size, alpha, width, distance, mode, dtype, device))
    return torch.where(lod < 0, torch.zeros_like(lod), lod)


def chain_sizes(h, w):
    """radially_varying_blur.py:100-109 -> [(h_0, w_0) .. (h_K, w_K)]: halved (floor) while both sides exceed 1; a chain that
    stops at 1x2 gets the mean of its two values as one more level. Raises ValueError where the reference's own broadcast
    fails: a chain that ends at 1 x w' (w' >= 3) or h' x 1 (h' >= 2, which includes its size(-2) == 2 branch)."""
    sizes = [(h, w)]
    while sizes[-1][0] > 1 and sizes[-1][1] > 1:
        sizes.append((sizes[-1][0] // 2, sizes[-1][1] // 2))
    if sizes[-1] == (1, 2):
        sizes.append((1, 1))
    if sizes[-1] != (1, 1):
        raise ValueError(f"the mip chain of a {h}x{w} map ends at {sizes[-1][0]}x{sizes[-1][1]}, not at 1x1 or 1x2")
    return sizes


def mip_chain(x):
    """radially_varying_blur.py:100-109"""
    sizes = chain_sizes(x.size(-2), x.size(-1))
    chain = [x]
    for hk, wk in sizes[1:]:
        if chain[-1].size(-2) > 1:
            chain.append(F.interpolate(chain[-1], scale_factor=0.5, mode="area", recompute_scale_factor=False))
        else:
            chain.append(chain[-1].mean(dim=-1, keepdim=True))
        assert tuple(chain[-1].shape[-2:]) == (hk, wk)
    return chain


def blur(x, lod, chain_out=None, cut=None):
    """radially_varying_blur.py:111-140: out = up_K where lod >= K, else (1 - f) up_l + f up_{l+1}, l = floor(lod),
    f = fmod(lod, 1); up_k is level k bilinearly up-sampled straight to full size, up_K the constant.
    chain_out: a list that receives the mip chain [m_0 .. m_K] (the tensors of the graph: after backward() m_k.grad is the loss's
    gradient with respect to chain level k, what csrc/hvs_fov.hip keeps as g[k]).
    cut = (k, y0, y1): rows y0 .. y1 - 1 of up_k are detached, so those pixels pass nothing back to level k THROUGH up_k (the
    forward value is unchanged): the defect of a backward pass that skips those rows of level k's footprints."""
    chain = mip_chain(x)
    if chain_out is not None:
        for m in chain[1:]:
            if m.requires_grad:
                m.retain_grad()
        chain_out.append(chain)
    K = len(chain) - 1
    size = x.shape[-2:]
    up = [x] + [F.interpolate(m, size=size, mode="bilinear", align_corners=False) for m in chain[1:K]] + [chain[K].expand_as(x)]
    if cut is not None:
        k, y0, y1 = cut
        u = up[k]
        up[k] = torch.cat([u[..., :y0, :], u[..., y0:y1, :].detach(), u[..., y1:, :]], dim=-2)
    frac = torch.fmod(lod, 1.0)
    out = torch.zeros_like(x)
    for l in range(K + 1):
        if l == K:
            mask, blended = lod >= l, up[l]
        else:
            mask = (lod < l + 1) if l == 0 else ((lod >= l) & (lod < l + 1))
            blended = (1 - frac) * up[l] + frac * up[l + 1]
        out = torch.where(mask, blended, out)
    return out


def find_stats(x, lod, tap=None):
    """metameric_loss.py:101-109 -> (mean, std, var before the clamp). tap: see stats_maps"""
    cut = None if tap is None else tap.get("cut")
    mean = blur(x, lod, None if tap is None else tap["mean"], cut)
    var = blur(x * x, lod, None if tap is None else tap["square"], cut) - mean * mean
    std = torch.sqrt(torch.where(var < VAR_FLOOR, torch.full_like(var, VAR_FLOOR), var))
    return mean, std, var


def lod_maps(gaze, H, W, n_levels, alpha, width, distance, mode, dtype=torch.float64, device="cpu"):
    """one per band level, rebuilt at the level's own size (metameric_loss.py:97-99: one RadiallyVaryingBlur per level)"""
    return [lod_map(gaze, (H >> l, W >> l), alpha, width, distance, mode, dtype, device) for l in range(n_levels - 1)]


def stats_maps(x, filters, lods, n_levels, want_vars=False, taps=None):
    """metameric_loss.py:125-167: [mean h, std h, (mean, std) per band per level .., last lowpass]; h shares level 0's map.
    taps: {pyramid level: dict(mean=[], square=[], cut=None or (k, y0, y1))}: the lists receive, per map of that level in the
    library's order (h in front of level 0's bands), the chain of the map and the chain of its square (blur's chain_out); cut
    is handed to every blur of that level."""
    h, bands, low = hvs_ref.pyramid(x, filters, n_levels)
    taps = taps or {}
    out, variances = [], []
    m, s, v = find_stats(h, lods[0], taps.get(0))
    out += [m, s]
    variances.append(v)
    for l, (level, lod) in enumerate(zip(bands, lods)):
        for b in level:
            m, s, v = find_stats(b, lod, taps.get(l))
            out += [m, s]
            variances.append(v)
    out.append(low)
    return (out, variances) if want_vars else out


def fov_loss(image, target, filters, gaze=(0.5, 0.5), alpha=0.2, real_image_width=0.2, real_viewing_distance=0.7, n_pyramid_levels=5,
             mode="quadratic", loss_type="L1", image_colorspace="RGB", return_maps=False, lods=None, taps=None):
    """MetamericLoss.__call__ (:204-271) with use_l2_foveal_loss=False: image, target [1,3,H,W]; autograd to image only.
    taps: stats_maps's, for the image's side"""
    hvs_ref.check_size(image.size(2), image.size(3), n_pyramid_levels)
    target = target.detach()
    if image_colorspace == "RGB":
        image, target = hvs_ref.rgb_2_ycrcb(image), hvs_ref.rgb_2_ycrcb(target)
    if lods is None:
        lods = lod_maps(gaze, image.size(2), image.size(3), n_pyramid_levels, alpha, real_image_width, real_viewing_distance, mode,
                        image.dtype, image.device)
    a = stats_maps(image, filters, lods, n_pyramid_levels, taps=taps)
    with torch.no_grad():
        b = stats_maps(target, filters, lods, n_pyramid_levels)
    loss = 0.0
    for x, y in zip(a, b):
        loss = loss + (F.mse_loss(x, y) if loss_type == "MSE" else F.l1_loss(x, y))
    loss = loss / len(a)
    return (loss, a) if return_maps else loss


def variances_outside_band(image, target, filters, lods, n_levels, lo=2e-8, hi=5e-7, image_colorspace="RGB"):
    """number of blended variances of either picture in [lo, hi] (exact zeros where lod = 0 are outside it)"""
    n = 0
    with torch.no_grad():
        for x in (image, target):
            if image_colorspace == "RGB":
                x = hvs_ref.rgb_2_ycrcb(x)
            for v in stats_maps(x, filters, lods, n_levels, want_vars=True)[1]:
                n += int(((v >= lo) & (v <= hi)).sum())
    return n


def undecided_sign_gradient(image, target, filters, lods, n_levels, threshold=hvs_ref.UNDECIDED, image_colorspace="RGB"):
    """tests/hvs_ref.undecided_sign_gradient for this loss -> (statistics with |a - b| < threshold, the share of the largest
    gradient they carry)"""
    img = image.detach().clone().requires_grad_(True)
    x, t = (hvs_ref.rgb_2_ycrcb(img), hvs_ref.rgb_2_ycrcb(target)) if image_colorspace == "RGB" else (img, target)
    a = stats_maps(x, filters, lods, n_levels)
    with torch.no_grad():
        b = stats_maps(t, filters, lods, n_levels)
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


def chain_gradients(tap, k):
    """after backward(): [2, nmc, h_k, w_k] = the loss's gradient with respect to chain level k of a tapped pyramid level's maps,
    the mean chain first, then the chain of the square, the maps in the library's order (csrc/hvs_fov.hip: g[k])"""
    return torch.stack([torch.cat([chain[k].grad[0] for chain in tap[which]]) for which in ("mean", "square")])
