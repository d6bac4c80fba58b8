"""The pruning step of the Fov-3DGS loop on the HIP library (csrc/prune.hip): the per-view importance metric, the mask of
the k least important Gaussians, and the cut of those rows out of the model, its Adam moments and its side arrays.

Drops in for the reference's ``metric_pruning`` (fov3dgs/prune.py:71-110; the same loop in metric_mask_learn.py:72-111) and
for ``GaussianModel.prune`` / ``_prune_optimizer`` / ``prune_points`` (fov3dgs/scene/gaussian_model.py:192-198, :624-664):

  update_metric_   one kernel for prune.py:82-86 (ten elementwise torch passes, four of them boolean-mask indexings)
  lowest_k_mask    a radix select for prune.py:101-107 (a full torch.sort, an index slice, a float mask scatter)
  compact_rows     one plan and ONE gather launch for up to 32 tensors (gaussian_model.py:629-664: 21 ``tensor[mask]`` calls,
                   each with its own nonzero and host synchronisation)

The choice inside a run of equal metrics -- most metrics are exactly 0 -- is arbitrary in the reference (an unstable sort);
here the rows are ordered by (metric, index) as torch.sort(stable=True) orders them, so the lowest indices of a tied run go
first and the result is one bit pattern, run after run.

Two more steps of prune.py's loop live here (csrc/prune_step.hip): ``scale_decay_loss`` (prune.py:257-261) and the opacity cap
``reset_opacity_max`` / ``reset_opacity`` / ``reset_opacity_upper_bound`` (gaussian_model.py:421-431, :447-452). Its quality gate is
fov3dgs_amd.quality.

GPU tensors only: there is no CPU fallback. Everything runs on torch.cuda.current_stream() of the tensors' device. The
scratch memory is one grow-only tensor per device (use it from one stream at a time). Transient memory of a prune: the
outputs are allocated before the inputs are released, so for a moment the parameters and both moments exist twice (about
4.3 GB at 6 M Gaussians)."""
import ctypes as C
import math

import torch

from . import _native

_KINDS = {"max_comp_efficiency": _native.PRUNE_MAX_COMP_EFFICIENCY, "surface": _native.PRUNE_CONTRIB,
          "max_contrib": _native.PRUNE_CONTRIB}
# the rasterizer the reference renders each metric's statistics with (prune.py:81, :89, :94)
_CUDA_TYPES = {"max_comp_efficiency": "pcheck_obb_loss_weighted_max_count", "surface": "pcheck_obb_loss_weighted_max_count",
               "max_contrib": "pcheck_obb_max"}
# group name -> model attribute (gaussian_model.py:646-651)
_ATTRS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
          ("scaling", "_scaling"), ("rotation", "_rotation"))
_workspaces = {}


def _require_gpu(what, *tensors):
    for t in tensors:
        if not torch.is_tensor(t):
            raise TypeError(f"fovraster {what} expects torch tensors, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"fovraster {what} needs GPU tensors: there is no CPU fallback")
    for t in tensors[1:]:
        if t.device != tensors[0].device:
            raise RuntimeError(f"fovraster {what}: tensors on {tensors[0].device} and {t.device}")


def _workspace(lib, P, device):
    need = max(int(lib.fr_prune_workspace_bytes(P)), 16)
    ws = _workspaces.get(device)
    if ws is None or ws.numel() < need:  # (grows with the model, never shrinks)
        ws = _workspaces[device] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"fovraster {what} failed ({rc}): {_native.last_error()}")


def _flat(t, P, name):
    if t.dim() == 2 and t.shape[1] == 1:
        t = t.reshape(-1)
    if t.dim() != 1 or t.shape[0] != P:
        raise ValueError(f"{name}: expected [{P}] or [{P}, 1], got {list(t.shape)}")
    return t


@torch.no_grad()
def update_metric_(metrics, contribs, gs_count, metric="max_comp_efficiency"):
    """One view's update of the pruning metric, in place: ``metrics[metrics < cur] = cur[metrics < cur]`` (prune.py:86) with
    cur = contribs / (gs_count + 1e-7), 0 where gs_count < 1, for "max_comp_efficiency" (prune.py:82-85) and cur = contribs
    for "surface" and "max_contrib" (prune.py:90-91, :95-97; gs_count may be None). metrics, contribs: float32 [P] or [P,1];
    gs_count: the rasterizer's int32 counts. Bit for bit the torch expression; a NaN cur leaves the old value. Returns metrics."""
    if metric not in _KINDS:
        raise ValueError(f"unknown pruning metric {metric!r} (expected one of {sorted(_KINDS)})")
    kind = _KINDS[metric]
    needs_count = kind == _native.PRUNE_MAX_COMP_EFFICIENCY
    _require_gpu("update_metric_", metrics, contribs, *((gs_count,) if needs_count else ()))
    if metrics.dtype != torch.float32 or not metrics.is_contiguous():
        raise ValueError(f"metrics must be a contiguous float32 tensor (it is updated in place), got {metrics.dtype}")
    P = metrics.shape[0]
    _flat(metrics, P, "metrics")
    contribs = _flat(contribs, P, "contribs")
    if contribs.dtype != torch.float32:
        raise ValueError(f"contribs must be float32, got {contribs.dtype}")
    contribs = contribs.contiguous()
    counts = None
    if needs_count:
        counts = _flat(gs_count, P, "gs_count")
        if counts.dtype in (torch.int64, torch.int16, torch.int8, torch.uint8):
            counts = counts.to(torch.int32)
        if counts.dtype != torch.int32:
            raise ValueError(f"gs_count must be the rasterizer's int32 counts, got {counts.dtype}")
        counts = counts.contiguous()
    if P == 0:
        return metrics
    lib = _native.load()
    with torch.cuda.device(metrics.device):
        rc = lib.fr_prune_metric_max(P, kind, contribs.data_ptr(), None if counts is None else counts.data_ptr(),
                                     metrics.data_ptr(), _stream(metrics.device))
    _check(rc, "prune_metric_max")
    return metrics


@torch.no_grad()
def lowest_k_mask(metrics, k):
    """-> torch.bool [P] with exactly k ones: the k smallest metrics, ties and all, in the order of
    ``torch.sort(metrics, descending=False, dim=0, stable=True)`` (NaN last, -0 == +0, the lower index first among equals).
    Replaces prune.py:101-107. metrics: float32 [P] or [P,1]. No host synchronisation."""
    _require_gpu("lowest_k_mask", metrics)
    if metrics.dtype != torch.float32:
        raise ValueError(f"metrics must be float32, got {metrics.dtype}")
    P = metrics.shape[0]
    m = _flat(metrics, P, "metrics").contiguous()
    k = int(k)
    if not 0 <= k <= P:
        raise ValueError(f"k = {k} is not in 0..{P}")
    mask = torch.empty(P, dtype=torch.bool, device=m.device)
    if P == 0:
        return mask
    lib = _native.load()
    with torch.cuda.device(m.device):
        ws = _workspace(lib, P, m.device)
        rc = lib.fr_prune_select_lowest(P, m.data_ptr(), k, mask.data_ptr(), ws.data_ptr(), _stream(m.device))
    _check(rc, "prune_select_lowest")
    return mask


@torch.no_grad()
def compact_rows(keep_mask, tensors, n_keep=None, invert=False):
    """-> [t[keep_mask] for t in tensors], bit for bit, with one plan and one gather launch per 32 tensors.

    keep_mask: bool or uint8 [P]; invert=True keeps the rows where it is False (the result is ``t[~keep_mask]``). tensors: any
    number of GPU tensors with P rows, of a 4- or 8-byte dtype and any trailing shape ([P,0,3] included); anything else raises
    ValueError. n_keep=None reads the number of kept rows back once (the only synchronisation); with n_keep given -- it must
    be the number of kept rows -- nothing synchronises, and it is not checked (that would be the synchronisation): when it is
    smaller, the kept rows beyond n_keep are never written; when it is larger, the surplus rows at the end of each result are
    uninitialised memory."""
    tensors = list(tensors)
    _require_gpu("compact_rows", keep_mask, *tensors)
    if keep_mask.dim() != 1 or keep_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"keep_mask must be a bool or uint8 vector, got {keep_mask.dtype} {list(keep_mask.shape)}")
    P = keep_mask.shape[0]
    srcs = []
    for t in tensors:
        if t.dim() < 1 or t.shape[0] != P:
            raise ValueError(f"compact_rows: a tensor of shape {list(t.shape)} does not have the mask's {P} rows")
        if t.layout != torch.strided or t.element_size() not in (4, 8):
            raise ValueError(f"compact_rows: dtype {t.dtype} / layout {t.layout} (strided tensors of 4- or 8-byte elements)")
        srcs.append(t.detach().contiguous())
    dev = keep_mask.device
    if n_keep is not None:
        n_keep = int(n_keep)
        if not 0 <= n_keep <= P:
            raise ValueError(f"n_keep = {n_keep} is not in 0..{P}")
    if P == 0:
        return [s.new_empty(s.shape) for s in srcs]
    lib = _native.load()
    mask = keep_mask.contiguous()
    with torch.cuda.device(dev):
        ws = _workspace(lib, P, dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        _check(lib.fr_compact_plan(P, mask.data_ptr(), int(bool(invert)), count.data_ptr(), ws.data_ptr(), _stream(dev)), "compact_plan")
        if n_keep is None:
            n_keep = int(count.item())
        outs = [s.new_empty((n_keep,) + tuple(s.shape[1:])) for s in srcs]  # (allocated before any input is released)
        args = _native.CompactArgs()
        args.P, args.invert, args.mask, args.workspace = P, int(bool(invert)), mask.data_ptr(), ws.data_ptr()
        for lo in range(0, len(srcs), _native.COMPACT_MAX_TENSORS):
            chunk = list(zip(srcs, outs))[lo:lo + _native.COMPACT_MAX_TENSORS]
            args.num_tensors = len(chunk)
            for d, (s, o) in zip(args.tensors, chunk):
                row_bytes = s.element_size() * (s.numel() // P)
                d.src, d.dst, d.row_words, d.dst_rows = s.data_ptr() or None, o.data_ptr() or None, row_bytes // 4, n_keep
            _check(lib.fr_compact_rows(C.byref(args), _stream(dev)), "compact_rows")
    return outs


@torch.no_grad()
def prune_points(model, mask, n_pruned=None):
    """GaussianModel.prune_points (gaussian_model.py:642-664, with _prune_optimizer, :624-640) for any object with the
    reference's attributes: _xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation, optimizer,
    xyz_gradient_accum, denom, max_radii2D and, optionally, indexes. mask: bool [P], True = prune the row.

    Every group's parameter, the exp_avg / exp_avg_sq of the groups that have state (a group without state only gets its
    parameter cut), the three side arrays and `indexes` go through ONE plan and ONE gather launch. As in the reference: new
    nn.Parameters are installed in param_groups, in optimizer.state (the same state dict: `step` and every other key stay)
    and on the model; side arrays whose length is not the mask's are zeroed at the new size. Works with torch.optim.Adam
    and fov3dgs_amd.optim.Adam. n_pruned: the number of True entries of mask when the caller knows it (lowest_k_mask's k):
    then nothing synchronises with the host; None reads the count back once."""
    opt = model.optimizer
    groups = [(g, g["params"][0]) for g in opt.param_groups]
    if mask.dim() == 2 and mask.shape[1] == 1:
        mask = mask.reshape(-1)
    _require_gpu("prune_points", mask, *[p for _, p in groups])
    if mask.dtype not in (torch.bool, torch.uint8):
        mask = mask != 0
    P = mask.shape[0]
    table, slots = [], []   # what is gathered, and where each result goes
    for g, p in groups:
        st = opt.state.get(p, None)
        table.append(p)
        slots.append(("param", g, st))
        if st is not None:
            table += [st["exp_avg"], st["exp_avg_sq"]]
            slots += [("exp_avg", g, st), ("exp_avg_sq", g, st)]
    side = model.xyz_gradient_accum.shape[0] == P
    if side:
        table += [model.xyz_gradient_accum, model.denom, model.max_radii2D]
        slots += [("xyz_gradient_accum", None, None), ("denom", None, None), ("max_radii2D", None, None)]
    if hasattr(model, "indexes"):
        table.append(model.indexes)
        slots.append(("indexes", None, None))
    n_keep = None if n_pruned is None else P - int(n_pruned)
    outs = compact_rows(mask, table, n_keep=n_keep, invert=True)
    new = {}
    for (what, g, st), out in zip(slots, outs):
        if what == "param":
            old = g["params"][0]
            if st is not None:
                del opt.state[old]
            g["params"][0] = torch.nn.Parameter(out.requires_grad_(True))
            if st is not None:
                opt.state[g["params"][0]] = st
            new[g["name"]] = g["params"][0]
        elif g is not None:
            st[what] = out
        else:
            setattr(model, what, out)
    for name, attr in _ATTRS:
        setattr(model, attr, new[name])
    if not side:
        n, dev = model._xyz.shape[0], model._xyz.device
        model.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        model.denom = torch.zeros((n, 1), device=dev)
        model.max_radii2D = torch.zeros((n,), device=dev)


@torch.no_grad()
def prune(model, prune_method, threshold):
    """GaussianModel.prune (gaussian_model.py:192-198): "opacity" cuts the Gaussians whose opacity is below threshold. The
    allocator's cache is left alone (no empty_cache)."""
    if prune_method != "opacity":
        raise ValueError("Prune method not recognized")
    opacity = model.get_opacity if hasattr(model, "get_opacity") else torch.sigmoid(model._opacity)
    prune_points(model, (opacity < threshold).reshape(-1))


def metric_pruning(model, cameras, pipe, bg, prune_ratio=0.1, metric="max_comp_efficiency", render=None):
    """The reference's metric_pruning (prune.py:71-110): renders every camera with the statistics rasterizer of `metric`,
    keeps each Gaussian's largest per-view value, and prunes the int(P * prune_ratio) Gaussians with the smallest one.
    `render` defaults to fov3dgs_amd.gaussian_renderer.render. After the renders nothing synchronises with the host: the
    select, the plan and the gather are enqueued back to back. Returns model."""
    if metric not in _KINDS:
        raise ValueError(f"unknown pruning metric {metric!r} (expected one of {sorted(_KINDS)})")
    if render is None:
        from .gaussian_renderer import render
    xyz = model.get_xyz
    _require_gpu("metric_pruning", xyz)
    P, dev = xyz.shape[0], xyz.device
    metrics = torch.zeros(P, dtype=torch.float32, device=dev)
    ones = {}
    with torch.no_grad():
        for cam in cameras:
            kw = {}
            if _CUDA_TYPES[metric] == "pcheck_obb_loss_weighted_max_count":  # loss_map = 1 everywhere (prune.py:80, :88)
                shape = (3, int(cam.image_height), int(cam.image_width))
                if shape not in ones:
                    ones[shape] = torch.ones(shape, dtype=torch.float32, device=dev)
                kw["loss_map"] = ones[shape]
            # (prune.py:94 also passes only_train_shs_dc=True for "max_contrib"; it is left out on purpose: neither the
            # reference's render (gaussian_renderer/__init__.py:19-20) nor this package's takes that argument, and a choice
            # of what to train cannot change contribs under no_grad)
            pkg = render(cam, model, pipe, bg, cuda_type=_CUDA_TYPES[metric], **kw)
            update_metric_(metrics, pkg["contribs"], pkg["gs_count"], metric)
    k = int(P * prune_ratio)
    prune_points(model, lowest_k_mask(metrics, k), n_pruned=k)
    return model


# ---- the other steps of prune.py's loop (csrc/prune_step.hip) ------------------------------------------------------------
class _ScaleDecay(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, counts, threshold, raw):
        lib = _native.load()
        s = scaling.detach()
        if not s.is_contiguous():
            s = s.contiguous()
        P, dev = s.shape[0], s.device
        partials = torch.empty(int(lib.fr_scale_decay_blocks(P)), dtype=torch.float64, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.fr_scale_decay_forward(P, s.data_ptr(), counts.data_ptr(), threshold, int(raw), partials.data_ptr(), out.data_ptr(),
                                            _stream(dev))
        _check(rc, "scale_decay_forward")
        ctx.save_for_backward(s, counts)
        ctx.threshold, ctx.raw = threshold, raw
        return out[0]

    @staticmethod
    def backward(ctx, g):
        s, counts = ctx.saved_tensors
        lib = _native.load()
        P, dev = s.shape[0], s.device
        g = g.detach().reshape(-1)[:1].to(device=dev, dtype=torch.float32).contiguous()  # read by the kernel: no host round trip
        grad = torch.empty_like(s)
        with torch.cuda.device(dev):
            rc = lib.fr_scale_decay_backward(P, s.data_ptr(), counts.data_ptr(), ctx.threshold, int(ctx.raw), g.data_ptr(), grad.data_ptr(),
                                             _stream(dev))
        _check(rc, "scale_decay_backward")
        return grad, None, None, None


def scale_decay_loss(scaling, gs_count, threshold=4, raw=False):
    """The scale-decay term of prune.py:257-261, ``(max(scaling, dim=1) * (gs_count - 4) * (gs_count > 4)).mean()``, as one
    forward launch plus a one-workgroup finish and one backward launch instead of about eight elementwise / reduce kernels and
    their autograd graph: mean_p( max_j s[p,j] * max(gs_count[p] - threshold, 0) ), a device scalar.

    scaling: float32 [P,3] -- activated, as get_scaling returns it, or with raw=True the log-scales (``_scaling``; the exp is taken
    in the kernel). gs_count: int32 [P] or [P,1], as render_pkg["gs_count"]; it receives no gradient. The gradient is dense
    [P,3]: (count - threshold)+ / P in the column of the row's maximum (the lowest column among equals, torch.max's index), times
    exp(raw) there with raw=True, 0 elsewhere, times the upstream gradient, which the kernel reads on the device: ``loss +=
    scale_loss * scale_weight`` synchronises nothing. A row with count <= threshold adds exactly 0 and gets exactly 0, whatever
    its scale. Sums are double, in a fixed order: the same bits on every run."""
    for t in (scaling, gs_count):
        if not torch.is_tensor(t):
            raise TypeError(f"fovraster scale_decay_loss expects torch tensors, got {type(t).__name__}")
    if scaling.dim() != 2 or scaling.shape[1] != 3 or scaling.shape[0] == 0:
        raise ValueError(f"scaling: expected [P,3] with P > 0, got {list(scaling.shape)}")
    if scaling.dtype != torch.float32:
        raise ValueError(f"scaling must be float32, got {scaling.dtype}")
    P = scaling.shape[0]
    counts = _flat(gs_count, P, "gs_count")
    if counts.dtype != torch.int32:
        raise ValueError(f"gs_count must be the rasterizer's int32 counts, got {counts.dtype}")
    if isinstance(threshold, bool) or not isinstance(threshold, int) or not -2 ** 31 <= threshold < 2 ** 31:
        raise ValueError(f"threshold must be an int32 value, got {threshold!r}")
    _require_gpu("scale_decay_loss", scaling, counts)
    return _ScaleDecay.apply(scaling, counts.detach().contiguous(), threshold, bool(raw))


@torch.no_grad()
def _cap_opacity(model, cap, what):
    if isinstance(cap, bool) or not isinstance(cap, (int, float)) or not 0.0 < float(cap) < 1.0:
        raise ValueError(f"{what}: the cap must lie inside (0, 1), got {cap!r}")
    cap = float(cap)
    opt = model.optimizer
    groups = [g for g in opt.param_groups if g.get("name") == "opacity"]
    if len(groups) != 1:
        raise ValueError(f"{what}: the optimizer has {len(groups)} groups named 'opacity'")
    group = groups[0]
    old = group["params"][0]
    if old is not model._opacity:
        raise ValueError(f"{what}: the 'opacity' group's parameter is not model._opacity")
    if old.dim() not in (1, 2) or (old.dim() == 2 and old.shape[1] != 1):
        raise ValueError(f"{what}: _opacity must be [P,1] or [P], got {list(old.shape)}")
    if old.dtype != torch.float32:
        raise ValueError(f"{what}: _opacity must be float32, got {old.dtype}")
    _require_gpu(what, old)
    raw = old.detach().contiguous()
    P, dev = raw.shape[0], raw.device
    st = opt.state.get(old, None)
    new = torch.empty_like(raw)
    m1, m2 = (torch.empty_like(raw), torch.empty_like(raw)) if st is not None else (None, None)
    cap_logit = math.log(cap / (1.0 - cap))
    lib = _native.load()
    with torch.cuda.device(dev):
        rc = lib.fr_opacity_cap(P, raw.data_ptr() or None, cap, cap_logit, new.data_ptr() or None,
                                None if m1 is None else m1.data_ptr() or None, None if m2 is None else m2.data_ptr() or None, _stream(dev))
    _check(rc, "opacity_cap")
    # replace_tensor_to_optimizer (gaussian_model.py:609-622); a NEW tensor on purpose: the rasterizer's "unchanged inputs" and
    # packed-layout caches key on the tensors' identity and version
    param = torch.nn.Parameter(new.requires_grad_(True))
    if st is not None:
        st["exp_avg"], st["exp_avg_sq"] = m1, m2
        del opt.state[old]
        opt.state[param] = st
    group["params"][0] = param
    model._opacity = param
    return param


def reset_opacity_max(model, max=0.99):
    """GaussianModel.reset_opacity_max (gaussian_model.py:427-431, with replace_tensor_to_optimizer :609-622): every opacity above
    `max` becomes `max`. ONE launch reads ``model._opacity`` and writes the new raw opacities -- float32(logit(max)), evaluated
    in double, where sigmoid(raw) > max -- and the zeroed exp_avg / exp_avg_sq; then a new nn.Parameter goes into the "opacity"
    group, into optimizer.state (the same state dict: `step` and every other key stay; a group without state only gets its
    parameter replaced) and onto the model. Works with torch.optim.Adam and fov3dgs_amd.optim.Adam; nothing synchronises.

    A difference from the reference, on purpose: it passes EVERY row through logit(sigmoid(raw)), which moves the rows under the
    cap by rounding noise (and sends raw values beyond +-17 to +-inf); here those rows keep their bits, and a NaN stays NaN.
    Returns the new parameter."""
    return _cap_opacity(model, max, "reset_opacity_max")


def reset_opacity(model):
    """GaussianModel.reset_opacity (gaussian_model.py:421-424): reset_opacity_max with the cap 0.01."""
    return _cap_opacity(model, 0.01, "reset_opacity")


def reset_opacity_upper_bound(model, upper_bound):
    """GaussianModel.reset_opacity_upper_bound (gaussian_model.py:447-452): reset_opacity_max with the cap `upper_bound`."""
    return _cap_opacity(model, upper_bound, "reset_opacity_upper_bound")
