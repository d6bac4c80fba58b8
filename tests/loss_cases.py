"""Pictures on which SSIM's formula is fragile, and the yardsticks the fused L1 + SSIM loss (csrc/loss.hip, and its copy in
csrc/quality.hip) is judged by on them: tests/test_loss_flat_cpu.py and tests/test_loss_flat_gpu.py.

The suite's other loss pictures are white noise, where the local variance (~1/12) and mean^2 (~1/4) swamp the stabilisers
C1 = 1e-4 and C2 = 9e-4 and the cancellation E[x^2] - mu^2 costs nothing. A render next to its ground truth has black background
(mu^2 << C1), flat areas (sigma^2 << C2, the cancellation goes to the last bits) and regions with x == y exactly. The cases
(float32, drawn with numpy.random.default_rng in float64 and rounded once; tests/golden/ref_loss3.npz keeps a CRC32 of every pair and
case() checks it, the rule of tests/hvs_fov_large_cases.py):

  blob     3x70x50  gt = clamp(1.6 (1 - r / 0.35), 0, 1) (0.6 + 0.2 c), r the distance from the centre in units of the picture, 0 outside;
                    render = clamp(0.9 gt + 0.05 [r < 0.2] + 0.004 randn, 0, 1), exactly 0 where gt is 0 (~60 % of the pixels)
  flat     3x70x50  gt constant 0.0 / 1.0 / 0.5 per channel; render = clamp(gt + 0.01 randn, 0, 1), its upper half equal to gt bit for bit
  smooth   3x70x50  gt = 0.5 + 0.4 sin(6.3 ((c + 1) u + v)); render = clamp(gt + 0.02 randn, 0, 1)
  steps    3x70x50  render = 0.8 / 0.2 by (col >= 16) xor (row >= 32), + 0.1 c for col >= 37 (one edge on a tile seam in each direction, one
                    off it); gt = the render rolled one column, times 0.97
  dark     3x70x50  render = 0.02 rand; gt = clamp(render + 0.004 randn, 0, 1): mu^2 <~ C1 everywhere
  tiny     3x4x4    smaller than the halo: render 1.0, gt 0.98 with one element equal to the render's
  corner   1x33x17  one row and one column reach into the second tile; built like flat with the constant 1.0
  equal    3x70x50  x == y everywhere: the flat channels in the left half, the smooth ramp in the right. SSIM's true gradient is 0.

70 x 50 on the kernels' 16-wide x 32-tall tile with its 5-pixel halo is 4 tile columns (the last 2 wide) and 3 tile rows (the last 6
tall): every kind of seam, and small enough for the 121-tap oracle with autograd.

Per case, computed once per session and shared (the tests must leave it unchanged):
  the reference point   oracle/loss_oracle.py in float64: l1, ssim, loss (lam 0.2) and the gradients of loss and of ssim with respect to
                        the render; with respect to gt (swapped arguments: both losses are symmetric) on blob and steps
  a float32 family      (a) the reference's own loss_utils.py on the CPU (ref_loss3.npz, tests/golden/make_loss_flat_golden.py);
                        (b) - (d) restated() below in float32: explicit shifted sums over the float32 2-D window, taps taken row-major
                        ascending, row-major descending and column-major; gradients by autograd.
                        None of the four is the kernels' separable, fma-ordered scheme: the code under test and imitations of it are
                        not part of the yardstick.
  yardstick[stat]       the largest distance of the four members from float64
  allowance[stat]       MARGIN = 4 x the yardstick (lpips_cases.MARGIN, for the same reason: another summation order)

The statistics: |l1 - l1_64|, |ssim - ssim_64|, |loss(0.2) - loss_64| (absolute); for each gradient the largest
|g - g64| / (|g64| + rms g64) (lpips_cases.feature_ratio) and the relative L2 distance (lpips_grad_cases.grad_l2). On `equal` g64 is 0
(to 1e-17): its gradients are judged by n max |g| instead, and its values by rules of their own (test_loss_flat_gpu.py).

The L1 value is the exception: the family agrees with float64 to below one ulp, so its allowance is derived. The kernel rounds each
x - y once (<= u = eps32 / 2 relative; exact where the two are within a factor 2), adds the |x - y| of a 16 x 32 tile in float32 in a
fixed tree (two per thread, six shuffle levels, two levels over the four waves: nine additions deep, <= 9 u on a sum of non-negative
terms), the tiles in double, and rounds mean to float32 once (u): (1 + 9 + 1) u = 5.5 eps32, taken as L1_EPS = 6 eps32 times l1_64.
"""
import functools
import math
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss_oracle as lo
from tests.lpips_cases import MARGIN, feature_ratio
from tests.lpips_grad_cases import grad_l2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("blob", "flat", "smooth", "steps", "dark", "tiny", "corner", "equal")
GT_GRAD = ("blob", "steps")   # the cases whose gradient with respect to gt is judged too
C, H, W = 3, 70, 50
LAM = 0.2
EPS32 = 2.0 ** -23
L1_EPS = 6.0                  # the L1 value's allowance in eps32 of l1_64 (derived above)
C1, C2 = 0.01 ** 2, 0.03 ** 2
ORDERS = {"rows_up": [(i, j) for i in range(11) for j in range(11)],
          "rows_down": [(i, j) for i in reversed(range(11)) for j in reversed(range(11))],
          "columns": [(i, j) for j in range(11) for i in range(11)]}
VALUE_STATS = ("l1", "ssim", "loss")


def _flat(rng, consts, h, w):
    gt = np.stack([np.full((h, w), v) for v in consts])
    x = np.clip(gt + 0.01 * rng.standard_normal(gt.shape), 0, 1)
    x[:, :h // 2] = gt[:, :h // 2]
    return x, gt


def _smooth_ramp(h, w):
    v, u = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    return np.stack([0.5 + 0.4 * np.sin(6.3 * ((c + 1) * u + v)) for c in range(C)])


def pictures(name):
    """-> (render, gt): float32 [C,H,W] numpy arrays, read-only"""
    rng = np.random.default_rng([2026, NAMES.index(name)])
    if name == "blob":
        rows, cols = np.meshgrid((np.arange(H) - (H - 1) / 2) / H, (np.arange(W) - (W - 1) / 2) / W, indexing="ij")
        r = np.sqrt(rows ** 2 + cols ** 2)
        gt = np.stack([np.clip(1.6 * (1 - r / 0.35), 0, 1) * (0.6 + 0.2 * c) for c in range(C)])
        x = np.clip(0.9 * gt + 0.05 * (r < 0.2) + 0.004 * rng.standard_normal(gt.shape), 0, 1)
        x[gt == 0] = 0.0
    elif name == "flat":
        x, gt = _flat(rng, (0.0, 1.0, 0.5), H, W)
    elif name == "smooth":
        gt = _smooth_ramp(H, W)
        x = np.clip(gt + 0.02 * rng.standard_normal(gt.shape), 0, 1)
    elif name == "steps":
        rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        x = np.stack([np.where((cols >= 16) ^ (rows >= 32), 0.8, 0.2) + 0.1 * c * (cols >= 37) for c in range(C)])
        gt = np.roll(x.astype(np.float32).astype(np.float64), 1, axis=2) * 0.97
    elif name == "dark":
        x = 0.02 * rng.random((C, H, W))
        gt = np.clip(x + 0.004 * rng.standard_normal(x.shape), 0, 1)
    elif name == "tiny":
        x = np.full((3, 4, 4), 1.0)
        gt = np.full((3, 4, 4), 0.98)
        gt[1, 2, 1] = 1.0
    elif name == "corner":
        x, gt = _flat(rng, (1.0,), 33, 17)
    elif name == "equal":
        x = _flat(rng, (0.0, 1.0, 0.5), H, W)[1]
        x[:, :, W // 2:] = _smooth_ramp(H, W)[:, :, W // 2:]
        gt = x.copy()
    else:
        raise KeyError(name)
    x, gt = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(gt, np.float32)
    x.setflags(write=False)
    gt.setflags(write=False)
    return x, gt


def crc_of(x, gt):
    return zlib.crc32(np.ascontiguousarray(gt).tobytes(), zlib.crc32(np.ascontiguousarray(x).tobytes()))


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN, "ref_loss3.npz")))


def window_2d(dtype):
    g = lo.window_1d()
    return (g[:, None].float() @ g[None, :].float()).to(dtype)  # the reference forms the 2-D window in float32


def blur(img, w2d, order, pad="zero"):
    """correlation of every channel of img [C,H,W] with the 11 x 11 window, the taps added in `order`"""
    h, w = img.shape[1:]
    p = F.pad(img, (5, 5, 5, 5)) if pad == "zero" else F.pad(img[None], (5, 5, 5, 5), mode="replicate")[0]
    out = None
    for i, j in order:
        t = w2d[i, j] * p[:, i:i + h, j:j + w]
        out = t if out is None else out + t
    return out


def ssim_restated(x, y, order="rows_up", c1=C1, c2=C2, pad="zero"):
    """the reference's _ssim in x's dtype with explicit shifted sums; c1, c2, pad: the doctored variants of test_loss_flat_cpu.py"""
    w2d = window_2d(x.dtype)
    o = ORDERS[order]
    mu1, mu2 = blur(x, w2d, o, pad), blur(y, w2d, o, pad)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = blur(x * x, w2d, o, pad) - mu1_sq
    s2 = blur(y * y, w2d, o, pad) - mu2_sq
    s12 = blur(x * y, w2d, o, pad) - mu12
    return (((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))).mean()


def restated(x, y, dtype, order="rows_up", with_gt=False, **doctor):
    """-> dict(l1, ssim, loss, grad_loss, grad_ssim[, grad_gt]): the losses of the pair in `dtype`, gradients by autograd
    (grad_gt: of the loss with respect to gt, from the same backward pass)"""
    a = x.detach().to(dtype).clone().requires_grad_(True)
    b = y.detach().to(dtype).clone().requires_grad_(with_gt)
    l1, ss = (a - b).abs().mean(), ssim_restated(a, b, order, **doctor)
    loss = (1.0 - LAM) * l1 + LAM * (1.0 - ss)
    g = torch.autograd.grad(loss, [a, b] if with_gt else [a], retain_graph=True)
    out = dict(l1=l1.item(), ssim=ss.item(), loss=loss.item(), grad_loss=g[0], grad_ssim=torch.autograd.grad(ss, a)[0])
    if with_gt:
        out["grad_gt"] = g[1]
    return out


def statistics(c, got):
    """the statistics of `got` (a dict with any of l1, ssim, loss, grad_loss, grad_ssim, grad_gt) against case c's float64 point"""
    out = {}
    for k in VALUE_STATS:
        if k in got and not c["equal"]:
            out[k] = abs(float(got[k]) - c[k + "64"])
    for k in ("grad_loss", "grad_ssim", "grad_gt"):
        if k in got and got[k] is not None:
            g = got[k].detach().double().cpu().reshape(c["x"].shape)
            if c["equal"]:
                out[k + "_nmax"] = c["n"] * float(g.abs().max())
            else:
                out[k + "_max"] = feature_ratio(g, c[k + "64"])
                out[k + "_l2"] = grad_l2(g, c[k + "64"])
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, x, y (float32 CPU tensors), n, equal, crc, l1_64 .. grad_gt64, mse64, psnr64, members {a..d: statistics},
    yardstick {stat: value}, allowance {stat: value})"""
    xn, yn = pictures(name)
    z = golden()
    crc = crc_of(xn, yn)
    if crc != int(z[f"crc_{name}"]):
        raise AssertionError(f"loss case {name}: the pictures' CRC32 {crc} is not the fixture's {int(z[f'crc_{name}'])}")
    x, y = torch.tensor(xn), torch.tensor(yn)
    with_gt = name in GT_GRAD
    loss64, l164, ssim64, gl64 = lo.l1_ssim(x, y, LAM)
    c = dict(name=name, x=x, y=y, n=x.numel(), equal=name == "equal", crc=crc, l164=l164, ssim64=ssim64, loss64=loss64, grad_loss64=gl64,
             grad_ssim64=lo.ssim_with_grad(x, y)[1], grad_gt64=lo.l1_ssim(y, x, LAM)[3] if with_gt else None)
    d = x.double() - y.double()
    c["mse64"] = float((d * d).mean())
    c["psnr64"] = 20.0 * math.log10(1.0 / math.sqrt(c["mse64"])) if c["mse64"] > 0 else float("inf")
    a = dict(l1=float(z[f"l1_{name}"]), ssim=float(z[f"ssim_{name}"]), loss=float(z[f"loss_{name}"]),
             grad_loss=torch.from_numpy(z[f"grad_{name}"]), grad_ssim=torch.from_numpy(z[f"ssim_grad_{name}"]))
    if with_gt:
        a["grad_gt"] = torch.from_numpy(z[f"grad_gt_{name}"])
    members = {"a": statistics(c, a)}
    for m, order in zip("bcd", ORDERS):
        members[m] = statistics(c, restated(x, y, torch.float32, order, with_gt))
    c["members"] = members
    c["yardstick"] = {k: max(s[k] for s in members.values()) for k in members["a"]}
    c["allowance"] = {k: MARGIN * v for k, v in c["yardstick"].items()}
    if not c["equal"]:
        c["allowance"]["l1"] = L1_EPS * EPS32 * l164
    for t in (gl64, c["grad_ssim64"], c["grad_gt64"]):
        if t is not None:
            t.requires_grad_(False)
    return c


@functools.lru_cache(maxsize=None)
def half_case(name):
    """case `name` with the render rounded to float16: the float64 loss of the ROUNDED pair and the allowance of a loss value on it,
    MARGIN x the largest distance of members (b) - (d) (the reference's fixture holds no run on the rounded pair)"""
    c = case(name)
    x16 = c["x"].half()
    loss64 = lo.l1_ssim(x16.float(), c["y"], LAM)[0]
    yard = max(abs(restated(x16.float(), c["y"], torch.float32, order)["loss"] - loss64) for order in ORDERS)
    return dict(x16=x16, loss64=loss64, yardstick=yard, allowance=MARGIN * yard)


def ratios(c, measured):
    """{stat: measured / allowance} (inf where a positive figure meets an allowance of 0)"""
    out = {}
    for k, v in measured.items():
        a = c["allowance"][k]
        out[k] = v / a if a > 0 else (0.0 if v == 0 else float("inf"))
    return out
