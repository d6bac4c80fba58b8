"""Densification on the HIP library (csrc/densify.hip): the steps of the training loop that add rows to the model, its Adam
moments and its side arrays.

Drops in for the reference's GaussianModel methods (fov3dgs/scene/gaussian_model.py), for any object with the attributes
``pruning.prune_points`` takes (_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation, optimizer,
xyz_gradient_accum, denom, max_radii2D, percent_dense and, optionally, indexes), with torch.optim.Adam and fov3dgs_amd.optim.Adam:

  add_densification_stats    :865-867, one kernel
  clone_rows / position_grad_densify / densify_and_clone                                    :803-818, :836-851
  split_rows / idx_densify_and_split / scale_densify_and_split / densify_and_split_big_size / densify_and_split
                                                                                            :709-801
  densify_and_prune          :820-834 -- in the reference two torch.cat and two prune_points over the whole training state (6
                             parameters and 12 Adam moments), each tensor[mask] and .sum() with its own nonzero and host
                             synchronisation; here ONE plan, ONE readback and ONE pass over the state

Every row-changing call: plan (a class byte per source row, per-tile counts, their running sums); ONE readback of four counts
-- the only host synchronisation --; the outputs are allocated, the noise drawn; one gather launch per 32 tensors; new
nn.Parameters are installed in param_groups, in optimizer.state (the same state dict object: `step` and every other key stay;
a group without state only gets its parameter) and on the model; xyz_gradient_accum, denom and max_radii2D become zeros of the
new size (:704-706).

Layout of every result, which is what the reference's cat / [mask] sequence produces: kept originals | surviving clones |
surviving children of copy 0 | ... | of copy N - 1, each in index order. Child c of the r-th split row (r in index order over
all split rows) is drawn with noise[c * n_split + r]. The noise is ``torch.randn((N * n_split, 3), generator=generator)``
unless the caller passes one: reproducible under torch.manual_seed, but not the reference's random stream (its torch.normal
calls are shaped by intermediate row counts that no longer exist here).

`indexes`, when the model has it with P rows, is copied in EVERY operation: clones and children inherit the parent's index.
The reference handles it only in idx_densify_and_split (:790-793) and prune_points; its other methods would leave `indexes`
short and raise at the next prune.

GPU tensors only: there is no CPU fallback. Everything runs on torch.cuda.current_stream() of the tensors' device. The
scratch memory is one grow-only tensor per device (use it from one stream at a time). Transient memory: the outputs are
allocated before any input is released, so for a moment the parameters and both moments exist twice (about 4.3 GB + the new
rows at 6 M Gaussians), as in pruning.py."""
import collections
import ctypes as C

import torch

from . import _native
from .pruning import _ATTRS, _check, _require_gpu, _stream

Counts = collections.namedtuple("Counts", "kept cloned split children_per_copy")
_ROLES = {"xyz": _native.DENSIFY_XYZ, "scaling": _native.DENSIFY_SCALING}
_workspaces = {}


def _workspace(lib, P, device):
    need = max(int(lib.fr_densify_workspace_bytes(P)), 16)
    ws = _workspaces.get(device)
    if ws is None or ws.numel() < need:  # (grows with the model, never shrinks)
        ws = _workspaces[device] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def _check_n(N):
    N = int(N)
    if not 1 <= N <= 4:
        raise ValueError(f"N = {N} is not in 1..4")
    return N


def _row_mask(mask, P, what):
    if not torch.is_tensor(mask):
        raise TypeError(f"fovraster {what} expects a torch tensor as mask, got {type(mask).__name__}")
    if mask.dim() == 2 and mask.shape[1] == 1:
        mask = mask.reshape(-1)
    if mask.dim() != 1 or mask.shape[0] != P:
        raise ValueError(f"{what}: the mask has shape {list(mask.shape)}, the model has {P} rows")
    if mask.dtype not in (torch.bool, torch.uint8):
        mask = mask != 0
    return mask


def _f32(t, name):
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    return t.detach().contiguous()


@torch.no_grad()
def add_densification_stats(model, viewspace_point_tensor, update_filter):
    """GaussianModel.add_densification_stats (gaussian_model.py:865-867), in place and in one launch: for the rows where
    update_filter is set, xyz_gradient_accum += |grad[:, :2]| and denom += 1. viewspace_point_tensor: the [P,3] screen-space
    points whose .grad the backward pass filled (a plain gradient tensor is taken as it is). No host synchronisation."""
    grad = getattr(viewspace_point_tensor, "grad", None)
    grad = viewspace_point_tensor if grad is None else grad
    accum, denom = model.xyz_gradient_accum, model.denom
    P = accum.shape[0]
    update_filter = _row_mask(update_filter, P, "add_densification_stats")
    if grad.dim() != 2 or grad.shape[0] != P or grad.shape[1] < 2:
        raise ValueError(f"add_densification_stats: the gradient has shape {list(grad.shape)}, expected [{P}, 3]")
    _require_gpu("add_densification_stats", accum, denom, grad, update_filter)
    for t, name in ((accum, "xyz_gradient_accum"), (denom, "denom")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != P:
            raise ValueError(f"{name} must be a contiguous float32 [{P}, 1] tensor (it is updated in place)")
    grad = _f32(grad, "the gradient")
    if grad.shape[1] != 3:
        grad = torch.nn.functional.pad(grad[:, :2], (0, 1))
    if P == 0:
        return
    lib = _native.load()
    with torch.cuda.device(accum.device):
        _check(lib.fr_densify_stats(P, grad.data_ptr(), update_filter.contiguous().data_ptr(), accum.data_ptr(), denom.data_ptr(),
                                    _stream(accum.device)), "densify_stats")


def _run(model, what, mode, N=2, mask=None, grads=None, max_grad=0.0, min_opacity=0.0, t_dense=0.0, t_world=0.0,
         use_world_size=False, noise=None, generator=None):
    """Plan, one readback, allocate, gather, install. -> Counts."""
    N = _check_n(N)
    opt = model.optimizer
    groups = [(g, g["params"][0]) for g in opt.param_groups]
    by_name = {g["name"]: p for g, p in groups}
    if set(by_name) != {n for n, _ in _ATTRS}:
        raise ValueError(f"{what}: the optimizer's groups are {sorted(by_name)}, expected {sorted(n for n, _ in _ATTRS)}")
    P = by_name["xyz"].shape[0]
    if mask is not None:
        mask = _row_mask(mask, P, what)
    if grads is not None:
        if not torch.is_tensor(grads):
            raise TypeError(f"fovraster {what} expects a torch tensor as grads, got {type(grads).__name__}")
        if grads.dim() == 2 and grads.shape[1] == 1:
            grads = grads.reshape(-1)
        if grads.dim() != 1 or grads.shape[0] > P:
            raise ValueError(f"{what}: grads has shape {list(grads.shape)}, expected [n] or [n, 1] with n <= {P}")
    _require_gpu(what, *[p for _, p in groups], *[t for t in (mask, grads, noise) if t is not None])
    dev = by_name["xyz"].device
    xyz, scaling, rotation, opacity = (_f32(by_name[n], "_" + n) for n in ("xyz", "scaling", "rotation", "opacity"))
    for n, p in by_name.items():
        if p.shape[0] != P:
            raise ValueError(f"{what}: _{n} has {p.shape[0]} rows, _xyz has {P}")
    if xyz.shape != (P, 3) or scaling.shape != (P, 3) or rotation.shape != (P, 4) or opacity.numel() != P:
        raise ValueError(f"{what}: expected _xyz [P,3], _scaling [P,3], _rotation [P,4] and _opacity [P,1]")
    # what is gathered, its role, and where each result goes
    table, slots = [], []
    srcs = {"xyz": xyz, "scaling": scaling, "rotation": rotation, "opacity": opacity}
    for g, p in groups:
        st = opt.state.get(p, None)
        table.append((srcs.get(g["name"], p), _ROLES.get(g["name"], _native.DENSIFY_COPY)))
        slots.append(("param", g, st))
        if st is not None:
            table += [(st["exp_avg"], _native.DENSIFY_ZERO_NEW), (st["exp_avg_sq"], _native.DENSIFY_ZERO_NEW)]
            slots += [("exp_avg", g, st), ("exp_avg_sq", g, st)]
    if hasattr(model, "indexes") and model.indexes.shape[0] == P:
        table.append((model.indexes, _native.DENSIFY_COPY))
        slots.append(("indexes", None, None))
    srcs_c = []
    for t, role in table:
        if t.shape[0] != P or t.layout != torch.strided or t.element_size() not in (4, 8):
            raise ValueError(f"{what}: a tensor of shape {list(t.shape)} and dtype {t.dtype} cannot be gathered ({P} rows of 4- or 8-byte elements)")
        srcs_c.append(t.detach().contiguous())
    counts = Counts(0, 0, 0, 0)
    if P > 0:
        lib = _native.load()
        with torch.cuda.device(dev):
            ws = _workspace(lib, P, dev)
            counts_dev = torch.empty(4, dtype=torch.int32, device=dev)
            pa = _native.DensifyPlanArgs()
            pa.P, pa.mode, pa.N, pa.use_world_size = P, mode, N, int(bool(use_world_size))
            pa.max_grad, pa.min_opacity, pa.t_dense, pa.t_world = float(max_grad), float(min_opacity), float(t_dense), float(t_world)
            keep_alive = []
            if mask is not None:
                mask = mask.contiguous()
                pa.mask = mask.data_ptr()
            elif grads is not None:
                grads = _f32(grads, "grads")
                pa.n_grad, pa.accum = grads.shape[0], grads.data_ptr() or None
            else:
                accum, denom = _f32(model.xyz_gradient_accum, "xyz_gradient_accum"), _f32(model.denom, "denom")
                if accum.numel() != P or denom.numel() != P:
                    raise ValueError(f"{what}: xyz_gradient_accum / denom do not have the model's {P} rows")
                keep_alive += [accum, denom]
                pa.n_grad, pa.accum, pa.denom = P, accum.data_ptr(), denom.data_ptr()
            pa.scaling, pa.opacity = scaling.data_ptr(), opacity.data_ptr()
            pa.counts_out, pa.workspace = counts_dev.data_ptr(), ws.data_ptr()
            _check(lib.fr_densify_plan(C.byref(pa), _stream(dev)), "densify_plan")
            counts = Counts(*counts_dev.tolist())  # the one synchronisation
            n_new = counts.kept + counts.cloned + N * counts.children_per_copy
            outs = [s.new_empty((n_new,) + tuple(s.shape[1:])) for s in srcs_c]  # (allocated before any input is released)
            if noise is None:
                noise = torch.randn((N * counts.split, 3), device=dev, generator=generator)
            elif noise.dtype != torch.float32 or tuple(noise.shape) != (N * counts.split, 3):
                raise ValueError(f"{what}: noise must be float32 [{N * counts.split}, 3] (N x the {counts.split} split rows), got "
                                 f"{noise.dtype} {list(noise.shape)}")
            noise = noise.contiguous()
            ra = _native.DensifyRowsArgs()
            ra.P, ra.N, ra.workspace = P, N, ws.data_ptr()
            ra.n_keep, ra.n_clone, ra.n_split, ra.n_child = counts
            ra.scaling, ra.rotation, ra.noise = scaling.data_ptr(), rotation.data_ptr(), noise.data_ptr() or None
            pairs = list(zip(srcs_c, outs, [role for _, role in table]))
            for lo in range(0, len(pairs), _native.COMPACT_MAX_TENSORS):
                chunk = pairs[lo:lo + _native.COMPACT_MAX_TENSORS]
                ra.num_tensors = len(chunk)
                for d, (s, o, role) in zip(ra.tensors, chunk):
                    row_bytes = s.element_size() * (s.numel() // P)
                    d.src, d.dst, d.row_words, d.role = s.data_ptr() or None, o.data_ptr() or None, row_bytes // 4, role
                _check(lib.fr_densify_rows(C.byref(ra), _stream(dev)), "densify_rows")
            del keep_alive
    else:
        outs = [s.new_empty(s.shape) for s in srcs_c]
    new = {}
    for (kind, g, st), out in zip(slots, outs):
        if kind == "param":
            old = g["params"][0]
            if st is not None:
                del opt.state[old]
            g["params"][0] = torch.nn.Parameter(out.requires_grad_(True))
            if st is not None:
                opt.state[g["params"][0]] = st
            new[g["name"]] = g["params"][0]
        elif g is not None:
            st[kind] = out
        else:
            setattr(model, kind, out)
    for name, attr in _ATTRS:
        setattr(model, attr, new[name])
    n = model._xyz.shape[0]
    model.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
    model.denom = torch.zeros((n, 1), device=dev)
    model.max_radii2D = torch.zeros((n,), device=dev)
    return counts


def _scaling_max(model):
    return torch.exp(model._scaling.detach()).max(dim=1).values


@torch.no_grad()
def clone_rows(model, mask):
    """Append a copy of every row where mask is set (the generic clone of densification_postfix, gaussian_model.py:688-706):
    parameters bitwise, moments zero, `indexes` inherited. One plan, one readback of the counts (the only synchronisation), one
    gather launch. -> Counts."""
    return _run(model, "clone_rows", _native.DENSIFY_CLONE_MASK, mask=mask)


@torch.no_grad()
def position_grad_densify(model, grad_threshold):
    """GaussianModel.position_grad_densify (gaussian_model.py:836-851): clone where |xyz_gradient_accum / denom| (NaN -> 0) is
    at least grad_threshold, whatever the size. The mask is three elementwise torch passes; the rest is clone_rows."""
    grads = model.xyz_gradient_accum / model.denom
    grads[grads.isnan()] = 0.0
    return clone_rows(model, torch.norm(grads, dim=-1) >= grad_threshold)


@torch.no_grad()
def split_rows(model, mask, N=2, noise=None, generator=None):
    """Replace every row where mask is set by N children (gaussian_model.py:780-801 without the mask's origin): child xyz =
    R (exp(scaling) * noise) + xyz, child scaling = log(exp(scaling) / (0.8 N)), everything else the parent's, moments zero.
    noise: float32 [N * n_split, 3] standard normal, row c * n_split + r for child c of the r-th split row; drawn with
    `generator` when None. One plan, one readback of the counts (the only synchronisation), one gather launch. -> Counts."""
    return _run(model, "split_rows", _native.DENSIFY_SPLIT_MASK, N=N, mask=mask, noise=noise, generator=generator)


@torch.no_grad()
def idx_densify_and_split(model, selected_pts_mask, N=2, noise=None, generator=None):
    """GaussianModel.idx_densify_and_split (gaussian_model.py:779-801): split the rows of the caller's mask."""
    return split_rows(model, selected_pts_mask, N=N, noise=noise, generator=generator)


@torch.no_grad()
def scale_densify_and_split(model, scene_extent, thresh_percent, N=2, noise=None, generator=None):
    """GaussianModel.scale_densify_and_split (gaussian_model.py:757-777): split where the largest scale exceeds
    thresh_percent * scene_extent."""
    _check_n(N)
    return split_rows(model, _scaling_max(model) > thresh_percent * scene_extent, N=N, noise=noise, generator=generator)


@torch.no_grad()
def densify_and_split_big_size(model, size_threshold, N=2, noise=None, generator=None):
    """GaussianModel.densify_and_split_big_size (gaussian_model.py:709-729): split where the largest scale exceeds size_threshold."""
    _check_n(N)
    return split_rows(model, _scaling_max(model) > size_threshold, N=N, noise=noise, generator=generator)


@torch.no_grad()
def densify_and_clone(model, grads, grad_threshold, scene_extent):
    """GaussianModel.densify_and_clone (gaussian_model.py:803-818): clone where |grads| >= grad_threshold and the largest scale is
    at most percent_dense * scene_extent; the mask is computed in the plan kernel. grads: float32 [P] or [P,1]. One readback of
    the counts (the only synchronisation). -> Counts."""
    if grads.shape[0] != model._xyz.shape[0]:
        raise ValueError(f"densify_and_clone: grads has {grads.shape[0]} rows, the model has {model._xyz.shape[0]}")
    return _run(model, "densify_and_clone", _native.DENSIFY_CLONE_GRAD, grads=grads, max_grad=grad_threshold,
                t_dense=model.percent_dense * scene_extent)


@torch.no_grad()
def densify_and_split(model, grads, grad_threshold, scene_extent, N=2, noise=None, generator=None):
    """GaussianModel.densify_and_split (gaussian_model.py:731-755): split where grads >= grad_threshold (signed, and 0 for the
    rows past len(grads): the reference's padded_grad) and the largest scale exceeds percent_dense * scene_extent; the mask is
    computed in the plan kernel. One readback of the counts (the only synchronisation). -> Counts."""
    return _run(model, "densify_and_split", _native.DENSIFY_SPLIT_GRAD, N=N, grads=grads, max_grad=grad_threshold,
                t_dense=model.percent_dense * scene_extent, noise=noise, generator=generator)


@torch.no_grad()
def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, N=2, noise=None, generator=None):
    """GaussianModel.densify_and_prune (gaussian_model.py:820-834) as ONE pass: clone, split, drop the split parents and cut the
    faint and the oversized rows, decided per source row from xyz_gradient_accum / denom, the scales and the opacity (the classes
    are spelled out in include/fovraster.h). One plan, one readback of the four counts -- the only synchronisation --, one gather
    launch. The allocator's cache is left alone (no empty_cache).

    Two quirks of the reference are kept: max_radii2D has been zeroed by the time of the final cut, so max_screen_size (when
    truthy, as the reference tests it) only switches the `largest scale > 0.1 * extent` test on; clones are never split.
    -> Counts."""
    return _run(model, "densify_and_prune", _native.DENSIFY_AND_PRUNE, N=N, max_grad=max_grad, min_opacity=min_opacity,
                t_dense=model.percent_dense * extent, t_world=0.1 * extent, use_world_size=bool(max_screen_size),
                noise=noise, generator=generator)
