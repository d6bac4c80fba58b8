"""Edge-case golden vectors for the uniform metameric (HVS) loss from the REFERENCE's own code (run by hand in the build
container only, never by a test):
    python tests/golden/make_hvs_edge_golden.py   ->  tests/golden/ref_hvs_edges.npz, ref_hvs_edges_maps.npz
The second fixture beside make_hvs_golden.py's. Its cases (CASES below, named E0 .. E7) reach what the seven cases of
ref_hvs.npz do not: pooling sizes whose halving falls below 1 at a deeper level, so that the "pooled" map is LARGER than the band
(ph > h), pooled maps of one row or one column, one and eight orientations, two and six levels, an image smaller than a tile,
several remainders against the 16x16 tile, and ASYMMETRIC filters. The reference's own filters cannot tell a right tap order
from a wrong one (l0 and h0 equal their rotation by 180 degrees, their transpose and their flips exactly, every band filter is
the negative of its rotation by 180 degrees), so the cases marked "asymmetric" run the reference's MetamericLossUniform with its
pyramid maker's filt_l0, filt_h0 and band_filters REPLACED by the sets stored here as
  afilters{1,4,6,8}_{l0,h0,b}   float32, drawn from a seeded generator: every 5x5 block has unit L1 norm (l0 + 1/25, so that the
                                lowpass keeps a DC gain through six levels) and is re-drawn until it differs from its rotation
                                by 180 degrees, its transpose, its two flips and from minus its rotation by at least half its
                                maximum (tests/hvs_cases.asymmetry)
(eight orientations are beyond the reference's own tables; its pyramid code takes any number of band filters).
Per case i it stores what ref_hvs.npz stores: img_i, tgt_i (16-bit), loss_i, grad_i (the reference's float32 run, autograd),
case_i = [H, W, pooling, levels, orientations, MSE?, asymmetric?] (float64: a pooling size can be fractional), seed_i, mapidx_i;
for E5 also loss_5_ycrcb, grad_5_ycrcb (the same pictures taken as YCrCb). In ref_hvs_edges_maps.npz: map0_i (mean of h),
mapmid_i (the mean of the first band), mapstd_i (the std of the second band, of the first where there is one) of the DEEPEST
level that is pooled (not an identity level), maplow_i (the lowpass residual).
The inputs meet the conditions of make_hvs_golden.py, in every colour space the case is run in: no pooled variance of either
picture in [2e-8, 5e-7] (the reference's own pyramid in float64), for L1 the undecided share of the gradient <= KINK_SHARE and
the reference's float32 gradient within REF_L2 of float64. Seeds 0, 1, .. are tried until they hold.
No case had to be shrunk. The h0 and band blocks are drawn with ZERO MEAN (the mean is taken off before the block is normalised),
as a highpass and an oriented band have no DC gain. With a DC gain the band statistics are numbers of the size of the picture,
not of its detail, and the reference's float32 rounding of them decides signs of |a - b| and cancels in mean-square - mean^2:
its float32 gradient was then 3e-6 .. 8e-6 (rel. L2) off float64 on the small cases, a std map of E3 4e-4 and the gradient of E7
1.4e-4 (max/max) off, against the 1e-4 the CPU tests bound the reference's distance by, and E4 found no seed in 400 at 88x136
(nor at 56x72) that met the two L1 conditions. With zero-mean blocks the same figures are 2e-7 .. 6e-7 and E4 holds at seed 1."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference/metamer")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from odak_perception import MetamericLossUniform  # noqa: E402
from odak_perception.color_conversion import rgb_2_ycrcb  # noqa: E402
from odak_perception.metameric_loss_uniform import uniform_blur  # noqa: E402
from odak_perception.spatial_steerable_pyramid import SpatialSteerablePyramid  # noqa: E402
from odak_perception.steerable_pyramid_filters import get_steerable_pyramid_filters  # noqa: E402
from tests import hvs_cases as hc  # noqa: E402
from tests import hvs_ref  # noqa: E402

# (H, W, pooling, levels, orientations, type, asymmetric filters?, colour spaces)
CASES = [(32, 32, 5, 5, 2, "L1", False, ("RGB",)),          # E0: level 3 is 4x4 at p = 0.625 -> pooled 6x6
         (32, 32, 3, 5, 2, "MSE", False, ("RGB",)),         # E1: 8x8 -> 10x10 and 4x4 -> 10x10
         (16, 16, 3, 4, 1, "L1", True, ("RGB",)),           # E2: one orientation, 4x4 -> 5x5
         (8, 8, 0.75, 2, 1, "L1", True, ("RGB",)),          # E3: p < 1 at level 0 (8x8 -> 10x10), two levels, less than a tile
         (88, 136, 5, 3, 6, "L1", True, ("RGB",)),          # E4: tile remainders 8, 8 and (44x68) 12, 4; p = 5, 2.5
         (24, 72, 13, 3, 6, "L1", True, ("RGB", "YCrCb")),  # E5: pooled maps of one row (1x5 at both levels)
         (36, 20, 13, 2, 4, "L1", True, ("RGB",)),          # E6: pooled map 2x1, one column
         (64, 64, 16, 6, 8, "MSE", True, ("RGB",))]         # E7: six levels, eight orientations, identity at the 4x4 level
ASYM_ORIENTATIONS = (1, 4, 6, 8)
FILTER_SEED = 20261019
KINK_SHARE = 2e-7  # (make_hvs_golden.py says why)
REF_L2 = 2e-5


def pictures(H, W, seed):
    """make_hvs_golden.pictures: a smooth sinusoid picture plus uniform noise; image = target + N(0, 0.05^2); 16-bit"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 3, H), np.linspace(0, 2, W), indexing="ij")
    base = np.stack([0.5 + 0.2 * np.sin(xx * (c + 1) + yy) * np.cos(yy * 1.7 - c) for c in range(3)])
    tgt = np.clip(base + 0.5 * (rng.random(base.shape) - 0.5), 0, 1)
    img = np.clip(tgt + 0.05 * rng.standard_normal(base.shape), 0, 1)
    return np.round(img * 65535).astype(np.uint16)[None], np.round(tgt * 65535).astype(np.uint16)[None]


def asymmetric_sets():
    rng = np.random.default_rng(FILTER_SEED)

    def block(lowpass):
        while True:
            a = rng.standard_normal((5, 5))
            if not lowpass:
                a -= a.mean()  # no DC gain, as a highpass or an oriented band has none (see the head of this file)
            a /= np.abs(a).sum()
            if lowpass:
                a += 1.0 / 25
            a = a.astype(np.float32)
            if hc.asymmetry(a) >= hc.ASYMMETRY:
                return a

    out = {}
    for no in ASYM_ORIENTATIONS:
        out[f"afilters{no}_l0"] = block(True).reshape(1, 1, 5, 5)
        out[f"afilters{no}_h0"] = block(False).reshape(1, 1, 5, 5)
        out[f"afilters{no}_b"] = np.stack([block(False).reshape(1, 1, 5, 5) for _ in range(no)])
    return out


def reference_loss(pool, levels, no, kind, filters):
    """the reference's MetamericLossUniform; filters = None: its own, else its pyramid maker's three filter attributes replaced"""
    fn = MetamericLossUniform(device=torch.device("cpu"), pooling_size=pool, n_pyramid_levels=levels, n_orientations=no,
                              loss_type=kind, bilinear_downsampling=True)
    if filters is not None:
        def dense(f):  # spatial_steerable_pyramid.py:91-96
            d = torch.zeros(3, 3, 5, 5)
            for c in range(3):
                d[c, c] = f.reshape(5, 5)
            return d
        pm = SpatialSteerablePyramid(use_bilinear_downup=True, n_channels=3, device=torch.device("cpu"), n_orientations=6,
                                     filter_type="cropped", filter_size=5)
        pm.filt_l0, pm.filt_h0, pm.band_filters = dense(filters["l0"]), dense(filters["h0"]), [dense(b) for b in filters["b"]]
        fn.pyramid_maker = pm  # calc_statsmaps keeps it: device, number of band filters and channels are what it asks for
    return fn


def ref_variances_in_band(fn, x64, pooling, colorspace):
    """pooled variances in [2e-8, 5e-7], recomputed as find_stats does from the reference's own pyramid in float64"""
    x = (rgb_2_ycrcb(x64) if colorspace == "RGB" else x64).double()
    fn.calc_statsmaps(x.float(), pooling)  # builds pyramid_maker where it is not set
    pm = fn.pyramid_maker
    saved = (pm.filt_h0, pm.filt_l0, pm.band_filters)
    pm.filt_h0, pm.filt_l0, pm.band_filters = saved[0].double(), saved[1].double(), [b.double() for b in saved[2]]
    pyr = pm.construct_pyramid(x, fn.n_pyramid_levels)
    pm.filt_h0, pm.filt_l0, pm.band_filters = saved
    assert len(pyr[0]["b"]) == fn.n_orientations
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


def conditions(case, seed, f32, f64):
    """-> (pooled variances in the band, undecided share of the L1 gradient, the reference's float32 gradient against float64)"""
    H, W, pool, levels, no, kind, asym, spaces = case
    img_q, tgt_q = pictures(H, W, seed)
    img_np, tgt_np = hvs_ref.decode_u16(img_q), hvs_ref.decode_u16(tgt_q)
    fn = reference_loss(pool, levels, no, kind, f32 if asym else None)
    bad, kink, ref_l2 = 0, 0.0, 0.0
    for cs in spaces:
        bad += ref_variances_in_band(fn, torch.tensor(img_np), pool, cs) + ref_variances_in_band(fn, torch.tensor(tgt_np), pool, cs)
        # the restatement must count what the reference's pyramid counts: the CPU tests assert it with the restatement
        bad += hvs_ref.variances_outside_band(torch.tensor(img_np).double(), torch.tensor(tgt_np).double(), f64, pool, levels,
                                              image_colorspace=cs)
    if bad == 0 and kind == "L1":
        for cs in spaces:
            i64 = torch.tensor(img_np).double().requires_grad_(True)
            t64 = torch.tensor(tgt_np).double()
            kink = max(kink, hvs_ref.undecided_sign_gradient(i64, t64, f64, pool, levels, image_colorspace=cs)[1])
            if kink <= KINK_SHARE:
                hvs_ref.hvs_loss(i64, t64, f64, pool, levels, kind, image_colorspace=cs).backward()
                i32 = torch.tensor(img_np, requires_grad=True)
                reference_loss(pool, levels, no, kind, f32 if asym else None)(i32, torch.tensor(tgt_np), image_colorspace=cs).backward()
                ref_l2 = max(ref_l2, float((i32.grad.double() - i64.grad).norm() / i64.grad.norm()))
    return bad, kink, ref_l2


def case_filters(sets, no, asym):
    f32 = hvs_ref.filters_from_npz(sets, no, prefix="afilters") if asym else get_steerable_pyramid_filters(5, no, "cropped")
    return f32, hvs_ref.filters_to(f32, dtype=torch.float64)


def main():
    out, out_maps = asymmetric_sets(), {}
    for ci, case in enumerate(CASES):
        H, W, pool, levels, no, kind, asym, spaces = case
        f32, f64 = case_filters(out, no, asym)
        for seed in range(400):
            bad, kink, ref_l2 = conditions(case, seed, f32, f64)
            if bad == 0 and kink <= KINK_SHARE and ref_l2 < REF_L2:
                break
        assert bad == 0 and kink <= KINK_SHARE and ref_l2 < REF_L2, (ci, bad, kink, ref_l2)
        img_q, tgt_q = pictures(H, W, seed)
        img_np, tgt_np = hvs_ref.decode_u16(img_q), hvs_ref.decode_u16(tgt_q)
        for cs in spaces:
            fn = reference_loss(pool, levels, no, kind, f32 if asym else None)
            img = torch.tensor(img_np, requires_grad=True)
            loss = fn(img, torch.tensor(tgt_np), image_colorspace=cs)
            loss.backward()
            tag = "" if cs == "RGB" else "_ycrcb"
            out.update({f"loss_{ci}{tag}": np.float32(loss.item()), f"grad_{ci}{tag}": img.grad.numpy()})
        with torch.no_grad():
            maps = reference_loss(pool, levels, no, kind, f32 if asym else None).calc_statsmaps(rgb_2_ycrcb(torch.tensor(img_np)), pool)
        assert len(maps) == hvs_ref.n_stats(levels, no)
        idx = hc.edge_map_indices(pool, levels, no)
        out.update({f"img_{ci}": img_q, f"tgt_{ci}": tgt_q, f"mapidx_{ci}": np.array(idx), f"seed_{ci}": seed,
                    f"case_{ci}": np.array([H, W, pool, levels, no, 1 if kind == "MSE" else 0, 1 if asym else 0], dtype=np.float64)})
        out_maps.update({f"map0_{ci}": maps[idx[0]].numpy(), f"mapmid_{ci}": maps[idx[1]].numpy(), f"mapstd_{ci}": maps[idx[2]].numpy(),
                         f"maplow_{ci}": maps[idx[3]].numpy()})
        print(f"E{ci}", (H, W, pool, levels, no, kind, asym), "seed", seed, "kink", kink, "ref_l2", ref_l2, "idx", idx, flush=True)
    out["n"] = len(CASES)
    np.savez_compressed(os.path.join(HERE, "ref_hvs_edges.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "ref_hvs_edges_maps.npz"), **out_maps)
    print("wrote", {f: os.path.getsize(os.path.join(HERE, f)) for f in ("ref_hvs_edges.npz", "ref_hvs_edges_maps.npz")})


if __name__ == "__main__":
    main()
