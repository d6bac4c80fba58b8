"""Golden vectors for the foveated metameric (HVS) loss from the REFERENCE's own code (run in the build container only):
    python tests/golden/make_hvs_fov_golden.py   ->  tests/golden/ref_hvs_fov.npz, ref_hvs_fov_maps.npz
imports /root/reference/metamer/odak_perception (MetamericLoss) on the CPU, in float32 as the reference runs, with
use_l2_foveal_loss=False and use_bilinear_downup=True (what hvs_loss_calc.py:38-41 passes), and stores per case i
  img_i, tgt_i (16-bit, decoded by tests/hvs_ref.decode_u16), loss_i, grad_i (autograd), case_i, mapidx_i, seed_i, amp_i,
  lod_i_l   the reference's LOD map of every band level l (RadiallyVaryingBlur.lod_map of blurs[l])
and, in ref_hvs_fov_maps.npz (a second file, so that each stays under the size limit of a committed file), four statistic maps
per case: map0_i (mean of h), mapmid_i (a mid-pyramid mean), mapstd_i (a standard deviation of that level), maplow_i (the lowpass
residual), at the indices mapidx_i of the reference's list of statistics. The filters are those of ref_hvs.npz.
Seeds are tried until make_hvs_golden.py's two conditions hold (evaluated with the float64 restatement, tests/hvs_fov_ref.py,
which tests/test_hvs_fov_cpu.py pins to these vectors): no blended variance of either picture in [2e-8, 5e-7] (exact zeros where
lod = 0 are fine), and for L1 cases the kink share below KINK_SHARE with the reference's float32 gradient within REF_L2 of
float64. The blended variance rises continuously from 0 where the LOD leaves 0, so a ring of pixels can always come close to
the band: where no seed of a case clears it the picture's noise amplitude is changed (AMPLITUDES), never the band."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference/metamer")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from odak_perception import MetamericLoss  # noqa: E402
from tests import hvs_fov_ref, hvs_ref  # noqa: E402
from tests.hvs_fov_cases import pictures  # noqa: E402  (the noise width is a parameter)

# (H, W, levels, orientations, alpha, mode, type, gaze, width, distance, colour space)
CASES = [(32, 64, 5, 6, 0.05, "quadratic", "MSE", (0.5, 0.5), 1.0, 0.5, "RGB"),      # F0: HVSLoss's defaults; deeper levels all-identity
         (32, 64, 5, 6, 3.0, "quadratic", "L1", (0.3, 0.6), 1.0, 0.5, "RGB"),        # F1: chain ends 1x2, the appended mean is sampled
         (64, 96, 5, 6, 0.5, "quadratic", "L1", (0.5, 0.5), 1.0, 0.5, "RGB"),        # F2: LOD up to about 5 of a 7-level chain
         (96, 64, 5, 2, 0.5, "quadratic", "MSE", (0.5, 0.5), 1.0, 0.5, "YCrCb"),     # F3: tall; two orientations; YCrCb input
         (40, 56, 3, 6, 2.0, "linear", "L1", (0.2, 0.7), 1.0, 0.5, "RGB"),           # F4: odd mip sizes 5->2, 7->3; lod >= K reached
         (64, 64, 5, 6, 0.001, "quadratic", "L1", (0.5, 0.5), 1.0, 0.5, "RGB"),      # F5: lod = 0 everywhere, L1
         (64, 64, 5, 6, 0.001, "quadratic", "MSE", (0.5, 0.5), 1.0, 0.5, "RGB"),     #     ... and MSE
         (64, 96, 4, 6, 0.3, "quadratic", "MSE", (1.2, -0.1), 2.0, 1.0, "RGB")]      # F6: gaze outside the picture, the renderer's display geometry

KINK_SHARE = 2e-7  # make_hvs_golden.py's
REF_L2 = 2e-5
AMPLITUDES = (0.5, 1.0, 2.0, 4.0)   # (the picture is clipped to [0, 1]: the larger ones approach two-valued noise)
SEEDS = 40


def reference(case):
    H, W, levels, no, alpha, mode, kind, gaze, width, dist, space = case
    return MetamericLoss(device=torch.device("cpu"), alpha=alpha, real_image_width=width, real_viewing_distance=dist,
                         n_pyramid_levels=levels, mode=mode, n_orientations=no, use_l2_foveal_loss=False, loss_type=kind,
                         use_bilinear_downup=True)


z = np.load(os.path.join(HERE, "ref_hvs.npz"))
out, out_maps = {}, {}
for ci, case in enumerate(CASES):
    H, W, levels, no, alpha, mode, kind, gaze, width, dist, space = case
    f64 = hvs_ref.filters_to(hvs_ref.filters_from_npz(z, no), dtype=torch.float64)
    lods = hvs_fov_ref.lod_maps(gaze, H, W, levels, alpha, width, dist, mode)
    found = False
    for amp in AMPLITUDES:
        for seed in range(1000 * ci, 1000 * ci + SEEDS):
            img_q, tgt_q = pictures(H, W, seed, amp)
            img_np, tgt_np = hvs_ref.decode_u16(img_q), hvs_ref.decode_u16(tgt_q)
            i64, t64 = torch.tensor(img_np).double(), torch.tensor(tgt_np).double()
            bad = hvs_fov_ref.variances_outside_band(i64, t64, f64, lods, levels, image_colorspace=space)
            kink = ref_l2 = 0.0
            if bad == 0 and kind == "L1":
                kink = hvs_fov_ref.undecided_sign_gradient(i64, t64, f64, lods, levels, image_colorspace=space)[1]
                if kink <= KINK_SHARE:
                    x64 = i64.clone().requires_grad_(True)
                    hvs_fov_ref.fov_loss(x64, t64, f64, n_pyramid_levels=levels, loss_type=kind, image_colorspace=space, lods=lods).backward()
                    i32 = torch.tensor(img_np, requires_grad=True)
                    reference(case)(i32, torch.tensor(tgt_np), gaze=list(gaze), image_colorspace=space).backward()
                    ref_l2 = float((i32.grad.double() - x64.grad).norm() / x64.grad.norm())
            if bad == 0 and kink <= KINK_SHARE and ref_l2 < REF_L2:
                found = True
                break
        if found:
            break
        print("   case", ci, "amplitude", amp, "no seed: last", (bad, kink, ref_l2), flush=True)
    assert found, (ci, bad, kink, ref_l2)
    fn = reference(case)
    img = torch.tensor(img_np, requires_grad=True)
    loss = fn(img, torch.tensor(tgt_np), gaze=list(gaze), image_colorspace=space)   # (asserts that the reference completes)
    loss.backward()
    ref_lods = [fn.blurs[l].lod_map.numpy().astype(np.float32) for l in range(levels - 1)]
    assert all(m.shape == (H >> l, W >> l) for l, m in enumerate(ref_lods))
    from odak_perception.color_conversion import rgb_2_ycrcb
    with torch.no_grad():
        x = torch.tensor(img_np)
        maps = fn.calc_statsmaps(rgb_2_ycrcb(x) if space == "RGB" else x, gaze=list(gaze), alpha=alpha, real_image_width=width,
                                 real_viewing_distance=dist, mode=mode)
    assert len(maps) == hvs_ref.n_stats(levels, no)
    mid = 2 * (1 + no * ((levels - 1) // 2))          # the mean of the first band of a middle level
    idx = [0, mid, mid + 3, len(maps) - 1]            # ... and the std of the second band of that level
    out.update({f"img_{ci}": img_q, f"tgt_{ci}": tgt_q, f"loss_{ci}": np.float32(loss.item()), f"grad_{ci}": img.grad.numpy(),
                f"mapidx_{ci}": np.array(idx), f"seed_{ci}": seed, f"amp_{ci}": amp,
                f"case_{ci}": np.array([H, W, levels, no, alpha, 1 if mode == "quadratic" else 0, 1 if kind == "MSE" else 0,
                                        gaze[0], gaze[1], width, dist, 1 if space == "RGB" else 0], dtype=np.float64)})
    out.update({f"lod_{ci}_{l}": m for l, m in enumerate(ref_lods)})
    out_maps.update({f"map0_{ci}": maps[idx[0]].numpy(), f"mapmid_{ci}": maps[idx[1]].numpy(), f"mapstd_{ci}": maps[idx[2]].numpy(),
                     f"maplow_{ci}": maps[idx[3]].numpy()})
    print(ci, case, "seed", seed, "amp", amp, "loss", loss.item(), "lod max", [float(m.max()) for m in ref_lods], flush=True)
out["n"] = len(CASES)
np.savez_compressed(os.path.join(HERE, "ref_hvs_fov.npz"), **out)
np.savez_compressed(os.path.join(HERE, "ref_hvs_fov_maps.npz"), **out_maps)
print("wrote", {f: os.path.getsize(os.path.join(HERE, f)) for f in ("ref_hvs_fov.npz", "ref_hvs_fov_maps.npz")})
