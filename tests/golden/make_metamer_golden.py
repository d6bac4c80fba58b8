"""Golden vectors for the metamer from the REFERENCE's own code (run in the build container only, on the CPU):
    python tests/golden/make_metamer_golden.py   ->  tests/golden/ref_metamer.npz, ref_metamer_out.npz, ref_metamer_rt.npz
imports /root/reference/metamer/odak_perception (MetamerMSELoss) in float32 as the reference runs, with avg_pooling_downup=True
(the argument it hands to its pyramid as use_bilinear_downup), and stores per case i (tests/metamer_cases.py lists the cases)
  tgt_i, img_i (16-bit, decoded by tests/hvs_ref.decode_u16), noise_i (the noise the reference drew: torch.manual_seed(0),
  torch.rand_like on the CPU, caught at the call), case_i, loss_i (the reference's loss of img_i against its metamer of tgt_i)
and, in further files so that each stays under the size limit of a committed file,
  ref_metamer_out.npz: metamer_i (gen_metamer of tgt_i), grad_i (autograd of loss_i to img_i),
  ref_metamer_rt.npz:  roundtrip_i (the reference's reconstruct_from_pyramid(construct_pyramid(.)) of tgt_i, colour converted as
                       gen_metamer converts).
Per case it MEASURES the distance of the reference's float32 vectors from the float64 restatement (tests/metamer_ref.py) fed with
the same noise -- ref_max_abs_i, ref_rel_l2_i over the metamer, ref_rt_max_abs_i, ref_rt_rel_l2_i over the round trip -- and stores
it: 4 x that distance is what the library may differ from the restatement by (tests/metamer_cases.allowance).
Two things the reference cannot be told through its constructor are set on the object, and said here:
  mode: MetamerMSELoss accepts it and never passes it on (metamer_mse_loss.py:49-52); the linear case sets metameric_loss.mode.
  YCrCb input: gen_metamer always converts from RGB (:78); the YCrCb case replaces that module's rgb_2_ycrcb by the identity for
  its calls.
The filters are those of ref_hvs.npz (the reference's own get_steerable_pyramid_filters(5, n, "cropped"))."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference/metamer")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import odak_perception.metamer_mse_loss as ref_module  # noqa: E402
from odak_perception import MetamerMSELoss  # noqa: E402
from odak_perception.color_conversion import rgb_2_ycrcb, ycrcb_2_rgb  # noqa: E402
from tests import hvs_ref, metamer_ref  # noqa: E402
from tests.hvs_fov_cases import pictures  # noqa: E402

# (H, W, levels, orientations, alpha, mode, loss type, gaze, width, distance, colour space)
CASES = [(32, 64, 5, 2, 0.2, "quadratic", "L1", (0.5, 0.5), 0.2, 0.7, "RGB"),       # M0: the class's defaults; residual 2x4
         (40, 56, 3, 6, 2.0, "linear", "MSE", (0.2, 0.7), 1.0, 0.5, "RGB"),         # M1: no powers of two; linear
         (64, 96, 5, 6, 0.5, "quadratic", "L1", (0.5, 0.5), 1.0, 0.5, "RGB"),       # M2: LOD deep into the chains
         (64, 64, 5, 2, 0.001, "quadratic", "MSE", (0.5, 0.5), 1.0, 0.5, "RGB"),    # M3: LOD 0, the variance on its floor
         (64, 96, 4, 6, 0.3, "quadratic", "MSE", (1.2, -0.1), 2.0, 1.0, "YCrCb"),   # M4: gaze outside; YCrCb input
         (96, 160, 5, 2, 0.2, "quadratic", "L1", (0.4, 0.6), 1.0, 0.5, "RGB")]      # M5: several tiles on both axes


def distances(got, want):
    d = got.double() - want
    return float(d.abs().max()), float(d.norm() / want.norm())


z = np.load(os.path.join(HERE, "ref_hvs.npz"))
files = {"ref_metamer.npz": {}, "ref_metamer_out.npz": {}, "ref_metamer_rt.npz": {}}
main, outs, rts = files["ref_metamer.npz"], files["ref_metamer_out.npz"], files["ref_metamer_rt.npz"]
rand_like, to_ycrcb = torch.rand_like, ref_module.rgb_2_ycrcb
for ci, case in enumerate(CASES):
    H, W, levels, no, alpha, mode, kind, gaze, width, dist, space = case
    img_q, tgt_q = pictures(H, W, 5000 + ci, 1.0)
    img_np, tgt_np = hvs_ref.decode_u16(img_q), hvs_ref.decode_u16(tgt_q)
    ref_module.rgb_2_ycrcb = to_ycrcb if space == "RGB" else (lambda x: x)
    drawn = []

    def catching(*a, **k):
        drawn.append(rand_like(*a, **k))
        return drawn[-1]

    def make():
        fn = MetamerMSELoss(device=torch.device("cpu"), alpha=alpha, real_image_width=width, real_viewing_distance=dist, mode=mode,
                            n_pyramid_levels=levels, n_orientations=no, loss_type=kind, avg_pooling_downup=True)
        fn.metameric_loss.mode = mode
        return fn

    fn = make()
    torch.rand_like = catching
    try:
        with torch.no_grad():
            metamer = fn.gen_metamer(torch.tensor(tgt_np), list(gaze))
            again = make().gen_metamer(torch.tensor(tgt_np), list(gaze))
    finally:
        torch.rand_like = rand_like
    assert len(drawn) == 2 and torch.equal(drawn[0], drawn[1]) and torch.equal(metamer, again)   # the same bits twice
    noise = drawn[0]
    assert noise.dtype == torch.float32 and tuple(noise.shape) == (1, 3, H, W)
    img = torch.tensor(img_np, requires_grad=True)
    loss = make()(img, torch.tensor(tgt_np), gaze=list(gaze))
    loss.backward()
    with torch.no_grad():
        x = torch.tensor(tgt_np)
        maker = fn.metameric_loss.pyramid_maker
        rt = maker.reconstruct_from_pyramid(maker.construct_pyramid(rgb_2_ycrcb(x) if space == "RGB" else x, levels))
        rt = ycrcb_2_rgb(rt) if space == "RGB" else rt
        f64 = hvs_ref.filters_to(hvs_ref.filters_from_npz(z, no), dtype=torch.float64)
        y = metamer_ref.gen_metamer(torch.tensor(tgt_np).double(), noise.double(), f64, gaze=gaze, alpha=alpha, real_image_width=width,
                                    real_viewing_distance=dist, n_pyramid_levels=levels, mode=mode, image_colorspace=space)
        y_rt = metamer_ref.roundtrip(torch.tensor(tgt_np).double(), f64, levels, space)
        y_loss = metamer_ref.loss(torch.tensor(img_np).double(), y, kind)
    d, d_rt = distances(metamer, y), distances(rt, y_rt)
    main.update({f"tgt_{ci}": tgt_q, f"img_{ci}": img_q, f"noise_{ci}": noise.numpy(), f"loss_{ci}": np.float32(loss.item()),
                 f"ref_max_abs_{ci}": d[0], f"ref_rel_l2_{ci}": d[1], f"ref_rt_max_abs_{ci}": d_rt[0], f"ref_rt_rel_l2_{ci}": d_rt[1],
                 f"case_{ci}": np.array([H, W, levels, no, alpha, 1 if mode == "quadratic" else 0, 1 if kind == "MSE" else 0,
                                         gaze[0], gaze[1], width, dist, 1 if space == "RGB" else 0], dtype=np.float64)})
    outs.update({f"metamer_{ci}": metamer.numpy(), f"grad_{ci}": img.grad.numpy()})
    rts.update({f"roundtrip_{ci}": rt.numpy()})
    print(ci, case, "metamer range", float(metamer.min()), float(metamer.max()), "reference vs float64: metamer", d, "round trip", d_rt,
          "loss", loss.item(), "float64", float(y_loss), flush=True)
ref_module.rgb_2_ycrcb = to_ycrcb
main["n"] = len(CASES)
for name, arrays in files.items():
    np.savez_compressed(os.path.join(HERE, name), **arrays)
print("wrote", {f: os.path.getsize(os.path.join(HERE, f)) for f in files})
