"""Golden vectors for the RESIZED uniform metameric (HVS) loss from the REFERENCE's own code (run by hand in the build container
only, never by a test):
    python tests/golden/make_hvs_resize_golden.py   ->  tests/golden/ref_hvs_resize.npz
The third fixture, beside make_hvs_golden.py's and make_hvs_edge_golden.py's (whose helpers and constants it imports). What the
reference's scripts do on every step (metric_mask_learn.py:221-227, eff_finetune.py:116-122, prune.py:128-134) is run here as they
run it, in float32 on the CPU: F.interpolate(x, size=(H, W), mode='bilinear', align_corners=False) of both pictures, then the
reference's MetamericLossUniform, with torch autograd from the loss back to the SOURCE image. The cases are
tests/hvs_resize_cases.CASES (R0 .. R4; that file says what each reaches). Per case i it stores
  img_i, tgt_i    the 16-bit SOURCE pictures [1,3,Hs,Ws] (make_hvs_golden.pictures at the source size)
  loss_i, grad_i  the reference's float32 result; grad_i has the SOURCE shape. For R2 also loss_2_ycrcb, grad_2_ycrcb.
  case_i          [Hs, Ws, H, W, pooling, levels, orientations, MSE?, asymmetric?, also YCrCb?] (float64), seed_i
Asymmetric cases use the filter sets already stored in ref_hvs_edges.npz (tests/hvs_resize_cases.filters_of: for two orientations
l0, h0 and the first two bands of the set of four, as no set of two is stored); this fixture stores no filters.
The pictures meet make_hvs_golden.py's conditions ON THE RESIZED PICTURES, in every colour space the case runs in: no pooled
variance of either resized picture in [2e-8, 5e-7] (the reference's own pyramid in float64, and the restatement), for L1 the
undecided share of the gradient <= KINK_SHARE, and the reference's float32 gradient (to the source) within REF_L2 of float64.
Seeds 0, 1, .. are tried until they hold. No case had to be changed."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_hvs_edge_golden as edge  # noqa: E402  (puts the reference's metamer/ and the repository root on sys.path)
from tests import hvs_cases as hc  # noqa: E402
from tests import hvs_ref  # noqa: E402
from tests import hvs_resize_cases as rc  # noqa: E402

KINK_SHARE, REF_L2 = edge.KINK_SHARE, edge.REF_L2  # (make_hvs_golden.py's constants; it says why)


def reference_run(case, f32, img_np, tgt_np, colorspace):
    """the reference as its scripts call it, float32 -> (loss, gradient with respect to the source image)"""
    (Hs, Ws), (H, W), levels, no, pool, kind, asym, spaces = case
    fn = edge.reference_loss(pool, levels, no, kind, f32 if asym else None)
    img = torch.tensor(img_np, requires_grad=True)
    loss = fn(rc.resize(img, H, W), rc.resize(torch.tensor(tgt_np), H, W), image_colorspace=colorspace)
    loss.backward()
    return loss.item(), img.grad


def conditions(case, seed, f32, f64):
    """-> (pooled variances in the band, undecided share of the L1 gradient, the reference's float32 gradient against float64),
    the first two on the RESIZED pictures"""
    (Hs, Ws), (H, W), levels, no, pool, kind, asym, spaces = case
    img_q, tgt_q = edge.pictures(Hs, Ws, seed)
    img_np, tgt_np = hvs_ref.decode_u16(img_q), hvs_ref.decode_u16(tgt_q)
    i64, t64 = torch.tensor(img_np).double(), torch.tensor(tgt_np).double()
    ri, rt = rc.resize(i64, H, W), rc.resize(t64, H, W)
    fn = edge.reference_loss(pool, levels, no, kind, f32 if asym else None)
    bad, kink, ref_l2 = 0, 0.0, 0.0
    for cs in spaces:
        bad += edge.ref_variances_in_band(fn, ri, pool, cs) + edge.ref_variances_in_band(fn, rt, pool, cs)
        bad += hvs_ref.variances_outside_band(ri, rt, f64, pool, levels, image_colorspace=cs)
    if bad == 0:
        for cs in spaces:
            if kind == "L1":
                kink = max(kink, hvs_ref.undecided_sign_gradient(ri, rt, f64, pool, levels, image_colorspace=cs)[1])
            if kink <= KINK_SHARE:
                s64 = i64.clone().requires_grad_(True)
                hvs_ref.hvs_loss(rc.resize(s64, H, W), rt, f64, pool, levels, kind, image_colorspace=cs).backward()
                g32 = reference_run(case, f32, img_np, tgt_np, cs)[1]
                ref_l2 = max(ref_l2, float((g32.double() - s64.grad).norm() / s64.grad.norm()))
    return bad, kink, ref_l2


def main():
    out = {}
    for ci, case in enumerate(rc.CASES):
        (Hs, Ws), (H, W), levels, no, pool, kind, asym, spaces = case
        f32 = rc.asymmetric_filters(hc.edges(), no) if asym else edge.get_steerable_pyramid_filters(5, no, "cropped")
        f64 = hvs_ref.filters_to(f32, dtype=torch.float64)
        for seed in range(400):
            bad, kink, ref_l2 = conditions(case, seed, f32, f64)
            if bad == 0 and kink <= KINK_SHARE and ref_l2 < REF_L2:
                break
        assert bad == 0 and kink <= KINK_SHARE and ref_l2 < REF_L2, (ci, bad, kink, ref_l2)
        img_q, tgt_q = edge.pictures(Hs, Ws, seed)
        img_np, tgt_np = hvs_ref.decode_u16(img_q), hvs_ref.decode_u16(tgt_q)
        for cs in spaces:
            loss, grad = reference_run(case, f32, img_np, tgt_np, cs)
            tag = "" if cs == "RGB" else "_ycrcb"
            out.update({f"loss_{ci}{tag}": np.float32(loss), f"grad_{ci}{tag}": grad.numpy()})
        out.update({f"img_{ci}": img_q, f"tgt_{ci}": tgt_q, f"seed_{ci}": seed,
                    f"case_{ci}": np.array([Hs, Ws, H, W, pool, levels, no, 1 if kind == "MSE" else 0, 1 if asym else 0,
                                            1 if "YCrCb" in spaces else 0], dtype=np.float64)})
        print(f"R{ci}", case, "seed", seed, "kink", kink, "ref_l2", ref_l2, flush=True)
    out["n"] = len(rc.CASES)
    path = os.path.join(HERE, "ref_hvs_resize.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.getsize(path), "bytes; ref_hvs_edges.npz has", os.path.getsize(os.path.join(HERE, "ref_hvs_edges.npz")))


if __name__ == "__main__":
    main()
