"""Golden vectors for the quality metrics from the REFERENCE's own code (run in the build container only, on the CPU):
    python tests/golden/make_quality_golden.py   ->  tests/golden/ref_quality.npz
imports /root/reference/fov3dgs/utils/loss_utils.py (l1_loss :17-18, ssim :37-76) and utils/image_utils.py (mse :14-15, psnr
:17-19) and stores, for the four pictures of make_loss_golden.py (none a multiple of the kernels' 16x32 tile but the last, which
fills half of one), the reference's fp32 values AND the same expressions evaluated in float64 on the same fp32 inputs:
  ssim_i, l1_i, mse_i, psnr_i        fp32, of the [1,C,H,W] pair: one value per picture, what prune.py:137-174 adds up
  mse_ch_i, psnr_ch_i                fp32 [C], of the [C,H,W] pair: one value per channel
  *64_i                              the float64 evaluations
  psnr_gap_i, psnr_ch_gap_i          |fp32 - float64| of the PSNR values: the reference's own rounding distance"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference/fov3dgs")
from utils.image_utils import mse, psnr  # noqa: E402
from utils.loss_utils import l1_loss, ssim  # noqa: E402

rng = np.random.default_rng(2025)
out = {}
cases = [(3, 37, 53, "noise"), (3, 70, 33, "smooth"), (1, 9, 5, "noise"), (3, 16, 16, "equal")]
for ci, (C, H, W, kind) in enumerate(cases):
    if kind == "smooth":  # a smooth picture and a slightly degraded copy, like a render next to its ground truth
        yy, xx = np.meshgrid(np.linspace(0, 3, H), np.linspace(0, 2, W), indexing="ij")
        base = np.stack([0.5 + 0.4 * np.sin(xx * (c + 1) + yy) * np.cos(yy * 1.7 - c) for c in range(C)]).astype(np.float32)
        a_np = np.clip(base + 0.03 * rng.standard_normal(base.shape).astype(np.float32), 0, 1)
        b_np = base
    elif kind == "equal":
        a_np = rng.random((C, H, W)).astype(np.float32); b_np = a_np.copy()
    else:
        a_np = rng.random((C, H, W)).astype(np.float32); b_np = rng.random((C, H, W)).astype(np.float32)
    out[f"a{ci}"], out[f"b{ci}"] = a_np, b_np
    for suffix, dtype in (("", torch.float32), ("64", torch.float64)):
        a, b = torch.tensor(a_np).to(dtype), torch.tensor(b_np).to(dtype)
        out[f"ssim{suffix}_{ci}"] = ssim(a[None], b[None]).numpy()
        out[f"l1{suffix}_{ci}"] = l1_loss(a[None], b[None]).numpy()
        out[f"mse{suffix}_{ci}"] = mse(a[None], b[None]).numpy().reshape(())
        out[f"psnr{suffix}_{ci}"] = psnr(a[None], b[None]).numpy().reshape(())
        out[f"mse_ch{suffix}_{ci}"] = mse(a, b).numpy().reshape(C)
        out[f"psnr_ch{suffix}_{ci}"] = psnr(a, b).numpy().reshape(C)
        assert out[f"ssim{suffix}_{ci}"].dtype == (np.float32 if dtype == torch.float32 else np.float64)
    with np.errstate(invalid="ignore"):  # inf - inf for the equal pictures: their gap is 0
        out[f"psnr_gap_{ci}"] = np.nan_to_num(np.abs(out[f"psnr_{ci}"].astype(np.float64) - out[f"psnr64_{ci}"]), nan=0.0)
        out[f"psnr_ch_gap_{ci}"] = np.nan_to_num(np.abs(out[f"psnr_ch_{ci}"].astype(np.float64) - out[f"psnr_ch64_{ci}"]), nan=0.0)
out["n"] = len(cases)
np.savez_compressed(os.path.join(HERE, "ref_quality.npz"), **out)
print("wrote ref_quality.npz")
for ci in range(len(cases)):
    print(ci, {k: out[f"{k}_{ci}"] for k in ("ssim", "ssim64", "l1", "mse", "mse64", "psnr", "psnr64", "psnr_gap", "psnr_ch", "psnr_ch_gap")})
