"""The quality gate of the reference's pruning loop on the HIP library (csrc/quality.hip, include/fovraster.h: fr_quality_*).

``prune.py`` measures the model before every pruning round and after each of its final prunes (:284-290, :327-331, :345-349):
``test_ssim_loss`` and ``test_psnr_loss`` (:137-174) each render every camera, run the torch SSIM (five grouped 121-tap
convolutions) or ``psnr`` and add Python scalars, a host synchronisation per view; ``metric_mask_learn.py:120-143`` gates on the
mean uniform HVS loss in the same way. Here:

  QualityMeter     ``add(image, gt)`` enqueues ONE pass over the pair (SSIM map, squared and absolute error per tile) and a
                   one-workgroup finish that writes the view's (ssim, psnr, l1, mse) into its slot of a device array and adds
                   them to a device accumulator; ``result()`` is the one readback.
  evaluate_views   the drop-in for test_ssim_loss + test_psnr_loss (+ test_hvs_loss with ``hvs=``): ONE render per camera.

The means are over the views of the per-view values (prune.py's arithmetic), added in double in the order of the ``add`` calls,
with no float atomics: a second identical run gives the same bits. GPU tensors only: there is no CPU fallback. Use a meter from
one stream at a time."""
import torch

from . import image_utils


class QualityMeter:
    """Mean SSIM, PSNR and L1 over up to `capacity` views, accumulated on `device`."""

    def __init__(self, device, capacity):
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"capacity must be a positive int, got {capacity!r}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("fovraster QualityMeter needs a GPU device: there is no CPU fallback")
        self.device, self.capacity = device, capacity
        # one buffer, one readback: the accumulator (sum ssim, sum psnr, sum l1, views) as 4 doubles, then float32 [capacity,4]
        self._buf = torch.zeros(4 + 2 * capacity, dtype=torch.float64, device=device)
        self._accum = self._buf[:4]
        self._per_view = self._buf[4:].view(torch.float32).view(capacity, 4)
        self._partials = None
        self._n = 0

    def __len__(self):
        return self._n

    def reset(self):
        self._buf.zero_()
        self._n = 0

    def add(self, image, gt):
        """One view: image and gt are [C,H,W] or [1,C,H,W] pictures on the meter's device. Enqueues the two launches on the
        current stream and nothing else (a non-contiguous or non-fp32 input is converted first)."""
        for t, name in ((image, "image"), (gt, "gt")):
            if not torch.is_tensor(t):
                raise TypeError(f"fovraster QualityMeter.add expects torch tensors, got {type(t).__name__} for {name}")
        if image.dim() == 4 and image.shape[0] == 1:
            image = image[0]
        if gt.dim() == 4 and gt.shape[0] == 1:
            gt = gt[0]
        if image.dim() != 3 or image.shape != gt.shape:
            raise ValueError(f"image and gt must be [C,H,W] (or [1,C,H,W]) of one shape, got {tuple(image.shape)} and {tuple(gt.shape)}")
        x, y, _, C, H, W = image_utils._planes(image[None], gt[None], "QualityMeter.add")
        if x.device != self.device:
            raise RuntimeError(f"fovraster QualityMeter on {self.device}: the pictures are on {x.device}")
        if self._n >= self.capacity:
            raise RuntimeError(f"fovraster QualityMeter: more than capacity = {self.capacity} views")
        self._partials = image_utils._measure(x, y, 1, C, H, W, True, self._per_view, self._n, self._accum, self._partials)
        self._n += 1

    def result(self):
        """-> {"ssim", "psnr", "l1": means over the views (float), "n", "per_view": {"ssim", "psnr", "l1", "mse": float32 [n]}}:
        the one readback (it waits for the device)."""
        host = self._buf.cpu()
        sums, n = host[:4].tolist(), self._n
        if int(sums[3]) != n:
            raise RuntimeError(f"fovraster QualityMeter: the device counted {sums[3]} views, the host {n}")
        per = host[4:].view(torch.float32).view(self.capacity, 4)[:n]
        mean = (lambda s: s / n) if n else (lambda s: float("nan"))
        return {"ssim": mean(sums[0]), "psnr": mean(sums[1]), "l1": mean(sums[2]), "n": n,
                "per_view": {k: per[:, i].clone() for i, k in enumerate(("ssim", "psnr", "l1", "mse"))}}

    def passes(self, target_psnr, target_ssim):
        """The gate of prune.py:288-290: mean PSNR >= target_psnr and mean SSIM >= target_ssim."""
        r = self.result()
        return bool(r["psnr"] >= target_psnr) and bool(r["ssim"] >= target_ssim)


def evaluate_views(model, cameras, pipe, bg, render=None, hvs=None, resize="pyramid", lpips=None):
    """prune.py's test_ssim_loss and test_psnr_loss (:137-174) in one loop with ONE render per camera
    (``cuda_type="pcheck_obb"``, under no_grad) against ``camera.original_image``, and with ``hvs=`` a MetamericLossUniform also
    metric_mask_learn.py's test_hvs_loss (:120-135), the resize to the pyramid's size done inside its kernels (``resize=``).
    `render` defaults to fov3dgs_amd.gaussian_renderer.render. Returns QualityMeter.result(), plus "hvs" (the mean) and
    per_view["hvs"] when asked, and with ``lpips=`` an lpipsPyTorch.LPIPS object also "lpips" (the mean) and per_view["lpips"],
    the fourth figure of the reference's tables (quality_metrics.py:61-83, hvs_metrics.py:71-98: lpips(render, gt, net_type='vgg')). Nothing synchronises with the
    host between the first render and the readback."""
    if render is None:
        from .gaussian_renderer import render
    cameras = list(cameras)
    if not cameras:
        raise ValueError("evaluate_views: no cameras")
    xyz = model.get_xyz
    if not xyz.is_cuda:
        raise RuntimeError("fovraster evaluate_views needs a model on the GPU: there is no CPU fallback")
    dev = xyz.device
    meter = QualityMeter(dev, len(cameras))
    hvs_vals = torch.zeros(len(cameras), dtype=torch.float32, device=dev) if hvs is not None else None
    lpips_vals = torch.zeros(len(cameras), dtype=torch.float32, device=dev) if lpips is not None else None
    with torch.no_grad():
        for v, cam in enumerate(cameras):
            image = render(cam, model, pipe, bg, cuda_type="pcheck_obb")["render"]
            gt = cam.original_image.to(dev)
            meter.add(image, gt)
            if hvs is not None:
                hvs_vals[v] = hvs(image.unsqueeze(0), gt.unsqueeze(0), resize=resize)
            if lpips is not None:
                lpips_vals[v] = lpips(image.unsqueeze(0), gt.unsqueeze(0)).reshape(())
    out = meter.result()
    if hvs is not None:
        per = hvs_vals.cpu()
        out["per_view"]["hvs"] = per
        out["hvs"] = float(per.double().mean())
    if lpips is not None:
        per = lpips_vals.cpu()
        out["per_view"]["lpips"] = per
        out["lpips"] = float(per.double().mean())
    return out
