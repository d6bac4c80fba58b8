"""Golden vectors for the uniform metameric (HVS) loss from the REFERENCE's own code (run in the build container only):
    python tests/golden/make_hvs_golden.py   ->  tests/golden/ref_hvs.npz
imports /root/reference/metamer/odak_perception (MetamericLossUniform, get_steerable_pyramid_filters) on the CPU, in float32
as the reference runs, and stores
  filters{6,2}_{l0,h0,b}   the cropped 5x5 filter sets for 6 and 2 orientations (data the reference's programs read: the
                           tests and tools take their coefficients from here, no source file of this repository holds any)
  per case i: img_i, tgt_i (16-bit, decoded by tests/hvs_ref.decode_u16), loss_i, grad_i (autograd), case_i, mapidx_i
and, in ref_hvs_maps.npz (a second file, so that each stays under the size limit of a committed file), four statistic maps per
case: map0_i (mean of h), mapmid_i (a mid-pyramid mean), mapstd_i (a standard deviation of that level), maplow_i (the lowpass
residual), at the indices mapidx_i of the reference's list of statistics.
The inputs keep every pooled variance of both pictures out of [2e-8, 5e-7], so the clamp at 1e-7 is decided alike in every
precision (asserted here with the reference's own pyramid, in float64; seeds are tried until it holds). For the L1 cases
they also keep |a - b| away from its kink as far as seeds can (tests/hvs_ref.undecided_sign_gradient says why and how far): the
statistics that differ by less than 1e-9 together carry less than KINK_SHARE of the largest gradient, and the reference's own
float32 run flipped no sign against float64. Seeds are tried until both hold."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference/metamer")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from odak_perception import MetamericLossUniform  # noqa: E402
from odak_perception.steerable_pyramid_filters import get_steerable_pyramid_filters  # noqa: E402
from tests import hvs_ref  # noqa: E402

# (H, W, pooling, levels, orientations, type)
CASES = [(32, 64, 4, 5, 6, "L1"), (64, 96, 9, 5, 6, "L1"), (40, 56, 4, 3, 6, "MSE"), (32, 32, 1, 5, 6, "L1"),
         (64, 64, 16, 5, 6, "MSE"), (96, 160, 25, 5, 6, "L1"), (48, 80, 2, 4, 2, "L1")]


KINK_SHARE = 2e-7  # of max |gradient|: every such sign flipped costs twice this, 1/5 of the comparisons' floor of 16 fp32 epsilons; ONE element that matters costs 1e-4 or more (the border elements of odd bands alone come to ~4e-8)
REF_L2 = 2e-5      # the reference's float32 gradient within this of float64: no sign of its own flipped (one costs >= 1e-4)


def pictures(H, W, seed):
    """target: a smooth sinusoid picture (amplitude 0.2) plus uniform noise of width 0.5 per channel; image: target + N(0, 0.05^2)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 3, H), np.linspace(0, 2, W), indexing="ij")
    base = np.stack([0.5 + 0.2 * np.sin(xx * (c + 1) + yy) * np.cos(yy * 1.7 - c) for c in range(3)])
    tgt = np.clip(base + 0.5 * (rng.random(base.shape) - 0.5), 0, 1)
    img = np.clip(tgt + 0.05 * rng.standard_normal(base.shape), 0, 1)
    # 16-bit pictures (hvs_ref.decode_u16 gives the float32 values the reference ran on): half the bytes in the fixture
    return np.round(img * 65535).astype(np.uint16)[None], np.round(tgt * 65535).astype(np.uint16)[None]


def ref_variances_in_band(loss_fn, x64, pooling):
    """pooled variances in [2e-8, 5e-7], recomputed as find_stats does from the reference's own pyramid"""
    from odak_perception.color_conversion import rgb_2_ycrcb
    from odak_perception.metameric_loss_uniform import uniform_blur
    x = rgb_2_ycrcb(x64).double()
    loss_fn.calc_statsmaps(x.float(), pooling)  # builds pyramid_maker
    pm = loss_fn.pyramid_maker
    saved = (pm.filt_h0, pm.filt_l0, pm.band_filters)
    pm.filt_h0, pm.filt_l0, pm.band_filters = saved[0].double(), saved[1].double(), [b.double() for b in saved[2]]
    pyr = pm.construct_pyramid(x, loss_fn.n_pyramid_levels)
    pm.filt_h0, pm.filt_l0, pm.band_filters = saved
    n, p = 0, float(pooling)
    maps = [(pyr[0]["h"], p)]
    for lvl in pyr[:-1]:
        maps += [(b, p) for b in lvl["b"]]
        p /= 2
    for m, pp in maps:
        mean = uniform_blur(m, pp)
        var = uniform_blur(m * m, pp) - mean * mean
        n += int(((var >= 2e-8) & (var <= 5e-7)).sum())
    return n


out, out_maps = {}, {}
for no in (6, 2):
    f = get_steerable_pyramid_filters(5, no, "cropped")
    out[f"filters{no}_l0"] = f["l0"].numpy().astype(np.float32)
    out[f"filters{no}_h0"] = f["h0"].numpy().astype(np.float32)
    out[f"filters{no}_b"] = np.stack([b.numpy() for b in f["b"]]).astype(np.float32)

for ci, (H, W, pool, levels, no, kind) in enumerate(CASES):
    for seed in range(1000 * ci, 1000 * ci + 400):
        img_q, tgt_q = pictures(H, W, seed)
        img_np, tgt_np = hvs_ref.decode_u16(img_q), hvs_ref.decode_u16(tgt_q)
        fn = MetamericLossUniform(device=torch.device("cpu"), pooling_size=pool, n_pyramid_levels=levels, n_orientations=no,
                                  loss_type=kind, bilinear_downsampling=True)
        bad = ref_variances_in_band(fn, torch.tensor(img_np), pool) + ref_variances_in_band(fn, torch.tensor(tgt_np), pool)
        kink = ref_l2 = 0.0
        if bad == 0 and kind == "L1":
            # ... and |a - b| away from ITS kink: no statistic difference with a gradient that matters is below 1e-9, and the
            # reference's own float32 run took every sign as float64 does (else its distance, the allowance, means nothing)
            f64 = hvs_ref.filters_to(get_steerable_pyramid_filters(5, no, "cropped"), dtype=torch.float64)
            i64 = torch.tensor(img_np).double().requires_grad_(True)
            kink = hvs_ref.undecided_sign_gradient(i64, torch.tensor(tgt_np).double(), f64, pool, levels)[1]
            if kink <= KINK_SHARE:
                hvs_ref.hvs_loss(i64, torch.tensor(tgt_np).double(), f64, pool, levels, kind).backward()
                i32 = torch.tensor(img_np, requires_grad=True)
                fn(i32, torch.tensor(tgt_np)).backward()
                ref_l2 = float((i32.grad.double() - i64.grad).norm() / i64.grad.norm())
        if bad == 0 and kink <= KINK_SHARE and ref_l2 < REF_L2:
            break
    assert bad == 0 and kink <= KINK_SHARE and ref_l2 < REF_L2, (ci, bad, kink, ref_l2)
    fn = MetamericLossUniform(device=torch.device("cpu"), pooling_size=pool, n_pyramid_levels=levels, n_orientations=no,
                              loss_type=kind, bilinear_downsampling=True)
    img = torch.tensor(img_np, requires_grad=True)
    tgt = torch.tensor(tgt_np)
    loss = fn(img, tgt, image_colorspace="RGB")
    loss.backward()
    from odak_perception.color_conversion import rgb_2_ycrcb
    with torch.no_grad():
        maps = fn.calc_statsmaps(rgb_2_ycrcb(torch.tensor(img_np)), pool)
    assert len(maps) == hvs_ref.n_stats(levels, no)
    mid = 2 * (1 + no * ((levels - 1) // 2))          # the mean of the first band of a middle level
    std = mid + 3                                     # the std of the second band of that level
    idx = [0, mid, std, len(maps) - 1]
    assert idx[1] % 2 == 0 and idx[2] % 2 == 1
    out.update({f"img_{ci}": img_q, f"tgt_{ci}": tgt_q, f"loss_{ci}": np.float32(loss.item()), f"grad_{ci}": img.grad.numpy(),
                f"mapidx_{ci}": np.array(idx), f"seed_{ci}": seed,
                f"case_{ci}": np.array([H, W, pool, levels, no, 1 if kind == "MSE" else 0])})
    out_maps.update({f"map0_{ci}": maps[idx[0]].numpy(), f"mapmid_{ci}": maps[idx[1]].numpy(), f"mapstd_{ci}": maps[idx[2]].numpy(),
                     f"maplow_{ci}": maps[idx[3]].numpy()})
    print(ci, (H, W, pool, levels, no, kind), "seed", seed, "loss", loss.item())
out["n"] = len(CASES)
np.savez_compressed(os.path.join(HERE, "ref_hvs.npz"), **out)
np.savez_compressed(os.path.join(HERE, "ref_hvs_maps.npz"), **out_maps)  # (a file of its own: each stays under 1 MiB)
print("wrote", {f: os.path.getsize(os.path.join(HERE, f)) for f in ("ref_hvs.npz", "ref_hvs_maps.npz")})
