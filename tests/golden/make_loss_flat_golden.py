"""Recorded results of the REFERENCE's own image losses on the flat, dark and stepped pictures of tests/loss_cases.py:
    python tests/golden/make_loss_flat_golden.py <path to the reference's fov3dgs directory>   ->  tests/golden/ref_loss3.npz
imports the reference's utils/loss_utils.py (l1_loss :17-18, ssim :37-76) on the CPU, feeds it every pair of loss_cases.pictures and
stores, per case, l1, ssim, loss (lam 0.2), the autograd gradients of loss and of ssim with respect to the first argument (on blob and
steps also the loss' gradient with respect to gt, from the same backward pass) and the CRC32 of the pair. No pictures are stored:
loss_cases.case() draws them again and checks the CRC."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import loss_cases as lc  # noqa: E402

sys.path.insert(0, sys.argv[1])
from utils.loss_utils import l1_loss, ssim  # noqa: E402

out = {}
for name in lc.NAMES:
    a_np, b_np = lc.pictures(name)
    with_gt = name in lc.GT_GRAD
    a = torch.tensor(a_np, requires_grad=True)
    b = torch.tensor(b_np, requires_grad=with_gt)
    l1, ss = l1_loss(a, b), ssim(a, b)
    loss = (1.0 - lc.LAM) * l1 + lc.LAM * (1.0 - ss)
    loss.backward()
    a2 = torch.tensor(a_np, requires_grad=True)
    ssim(a2, torch.tensor(b_np)).backward()
    out.update({f"l1_{name}": np.float64(l1.item()), f"ssim_{name}": np.float64(ss.item()), f"loss_{name}": np.float64(loss.item()),
                f"grad_{name}": a.grad.numpy(), f"ssim_grad_{name}": a2.grad.numpy(), f"crc_{name}": np.int64(lc.crc_of(a_np, b_np))})
    if with_gt:
        out[f"grad_gt_{name}"] = b.grad.numpy()
    print(name, a_np.shape, "l1", l1.item(), "ssim", ss.item(), "loss", loss.item(), "equal pixels", float((a_np == b_np).mean()))
path = os.path.join(HERE, "ref_loss3.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
