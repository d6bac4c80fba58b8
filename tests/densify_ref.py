"""Reference restatements for fov3dgs_amd.densify (test infrastructure, not a test), written from the semantics of the
reference's GaussianModel (fov3dgs/scene/gaussian_model.py:666-851, :865-867), not from its text, in torch's own operations
(cat, boolean indexing, bmm). They run on tests/prune_ref.Model on any device and take an explicit `noise` where the
reference draws one: samples = exp(scaling).repeat(N, 1) * noise, which is what torch.normal(0, std) computes from a
standard normal draw.

  postfix                       cat_tensors_to_optimizer + densification_postfix (:666-706); `indexes` is extended too: clones
                                and children inherit the parent's index (the contract of fov3dgs_amd.densify)
  clone_rows / split_rows       the generic clone (:809-818) and split (:740-755) of a mask
  position_grad_densify, idx_densify_and_split, scale_densify_and_split, densify_and_split_big_size, densify_and_clone,
  densify_and_split, densify_and_prune
                                the reference's methods, literally: densify_and_prune is the four-pass sequence
  densify_and_prune_plan        the same result from ONE decision per source row (what the HIP kernels implement)
  add_densification_stats       :865-867
  children_f64                  the children's xyz and scaling in float64 from the float32 inputs, and the xyz error scale
  open_gaps                     nudges scales and opacities away from the decision thresholds (judged in float64)
"""
import torch

from tests import prune_ref
from tests.adam_ref import ATTRS, NAMES

GAP = 1e-4  # relative half-width of the gap open_gaps leaves around every threshold


def build_rotation(r):
    """utils/general_utils.py:78-99: rotation matrices [n,3,3] of raw quaternions [n,4] (w, x, y, z), divided by their norm."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device, dtype=r.dtype)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def postfix(model, new, new_indexes=None):
    """Append the rows of new = {group name: tensor} to every group's parameter, zeros to its exp_avg / exp_avg_sq where the
    group has state; new nn.Parameters in the group, in optimizer.state (same state dict) and on the model; the side arrays
    become zeros of the new size."""
    opt = model.optimizer
    for group in opt.param_groups:
        old = group["params"][0]
        ext = new[group["name"]]
        st = opt.state.get(old, None)
        if st is not None:
            st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0)
            st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
            del opt.state[old]
        group["params"][0] = torch.nn.Parameter(torch.cat((old.detach(), ext), dim=0).requires_grad_(True))
        if st is not None:
            opt.state[group["params"][0]] = st
        setattr(model, ATTRS[group["name"]], group["params"][0])
    if new_indexes is not None:
        model.indexes = torch.cat((model.indexes, new_indexes), dim=0)
    n, dev = model._xyz.shape[0], model._xyz.device
    model.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
    model.denom = torch.zeros((n, 1), device=dev)
    model.max_radii2D = torch.zeros((n,), device=dev)


def _has_indexes(model):
    return hasattr(model, "indexes") and model.indexes.shape[0] == model._xyz.shape[0]


def clone_rows(model, mask):
    mask = mask.reshape(-1).bool()
    idx = model.indexes[mask] if _has_indexes(model) else None
    postfix(model, {n: getattr(model, ATTRS[n]).detach()[mask] for n in NAMES}, idx)


def split_rows(model, mask, N, noise):
    mask = mask.reshape(-1).bool()
    n_split = int(mask.sum())
    assert noise.shape == (N * n_split, 3), (noise.shape, N, n_split)
    scaling = torch.exp(model._scaling.detach())
    samples = scaling[mask].repeat(N, 1) * noise
    rots = build_rotation(model._rotation.detach()[mask]).repeat(N, 1, 1)
    new = {n: getattr(model, ATTRS[n]).detach()[mask].repeat(N, *([1] * (getattr(model, ATTRS[n]).dim() - 1))) for n in NAMES}
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + model._xyz.detach()[mask].repeat(N, 1)
    new["scaling"] = torch.log(scaling[mask].repeat(N, 1) / (0.8 * N))
    idx = model.indexes[mask].repeat(N) if _has_indexes(model) else None
    postfix(model, new, idx)
    prune_ref.prune_points(model, torch.cat((mask, torch.zeros(N * n_split, device=mask.device, dtype=torch.bool))))
    # (prune_points cuts the zeroed side arrays; they stay zeros of the new size)


def _mean_grads(model):
    grads = model.xyz_gradient_accum / model.denom
    grads[grads.isnan()] = 0.0
    return grads


def position_grad_densify(model, grad_threshold):
    clone_rows(model, torch.norm(_mean_grads(model), dim=-1) >= grad_threshold)


def idx_densify_and_split(model, mask, N, noise):
    split_rows(model, mask, N, noise)


def scale_mask(model, threshold):
    return torch.max(torch.exp(model._scaling.detach()), dim=1).values > threshold


def scale_densify_and_split(model, scene_extent, thresh_percent, N, noise):
    split_rows(model, scale_mask(model, thresh_percent * scene_extent), N, noise)


def densify_and_split_big_size(model, size_threshold, N, noise):
    split_rows(model, scale_mask(model, size_threshold), N, noise)


def clone_mask(model, grads, grad_threshold, scene_extent):
    return (torch.norm(grads, dim=-1) >= grad_threshold) & ~scale_mask(model, model.percent_dense * scene_extent)


def split_mask(model, grads, grad_threshold, scene_extent):
    padded = torch.zeros(model._xyz.shape[0], device=model._xyz.device)
    padded[:grads.shape[0]] = grads.reshape(-1)
    return (padded >= grad_threshold) & scale_mask(model, model.percent_dense * scene_extent)


def densify_and_clone(model, grads, grad_threshold, scene_extent):
    clone_rows(model, clone_mask(model, grads, grad_threshold, scene_extent))


def densify_and_split(model, grads, grad_threshold, scene_extent, N, noise):
    split_rows(model, split_mask(model, grads, grad_threshold, scene_extent), N, noise)


def final_cut_mask(model, min_opacity, extent, max_screen_size):
    mask = (torch.sigmoid(model._opacity.detach()) < min_opacity).reshape(-1)
    if max_screen_size:
        mask = mask | (model.max_radii2D > max_screen_size) | scale_mask(model, 0.1 * extent)
    return mask


def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, N, noise):
    """The literal sequence of :820-834: clone (cat), split (cat, cut of the parents), final cut. -> (clones, split rows)."""
    grads = _mean_grads(model)
    cm = clone_mask(model, grads, max_grad, extent)
    clone_rows(model, cm)
    sm = split_mask(model, grads, max_grad, extent)
    split_rows(model, sm, N, noise)
    prune_ref.prune_points(model, final_cut_mask(model, min_opacity, extent, max_screen_size))
    return int(cm.sum()), int(sm.sum())


def plan_classes(model, max_grad, min_opacity, extent, max_screen_size, N):
    """The per-source-row classes of densify_and_prune: (keep, clone survives, split, children survive), bool [P] each."""
    g = _mean_grads(model).reshape(-1)
    s = torch.exp(model._scaling.detach())
    smax = s.max(dim=1).values
    t_d, t_w = model.percent_dense * extent, 0.1 * extent
    clone = (g.abs() >= max_grad) & (smax <= t_d)
    split = (g >= max_grad) & (smax > t_d)
    faint = (torch.sigmoid(model._opacity.detach()) < min_opacity).reshape(-1)
    cmax = torch.exp(torch.log(s / (0.8 * N))).max(dim=1).values
    world = bool(max_screen_size)
    dead = faint | ((smax > t_w) if world else torch.zeros_like(faint))
    child_dead = faint | ((cmax > t_w) if world else torch.zeros_like(faint))
    return ~split & ~dead, clone & ~dead, split, split & ~child_dead


def densify_and_prune_plan(model, max_grad, min_opacity, extent, max_screen_size, N, noise):
    """densify_and_prune from one decision per source row: every output is kept originals | surviving clones | surviving
    children of copy 0 | ... | of copy N - 1, each in index order; child c of the r-th split row uses noise[c * n_split + r]."""
    keep, clone, split, child = plan_classes(model, max_grad, min_opacity, extent, max_screen_size, N)
    n_split = int(split.sum())
    assert noise.shape == (N * n_split, 3)
    alive = child[split]  # per split row, in index order
    scaling = torch.exp(model._scaling.detach())
    samples = scaling[split].repeat(N, 1) * noise
    rots = build_rotation(model._rotation.detach()[split]).repeat(N, 1, 1)
    kids_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + model._xyz.detach()[split].repeat(N, 1)
    kids_scaling = torch.log(scaling[split].repeat(N, 1) / (0.8 * N))
    alive_n = alive.repeat(N)
    has_indexes = _has_indexes(model)
    opt = model.optimizer
    for group in opt.param_groups:
        old = group["params"][0]
        p = old.detach()
        reps = [1] * (p.dim() - 1)
        kids = {"xyz": kids_xyz, "scaling": kids_scaling}.get(group["name"])
        if kids is None:
            kids = p[split].repeat(N, *reps)
        out = torch.cat((p[keep], p[clone], kids[alive_n]), dim=0)
        st = opt.state.get(old, None)
        if st is not None:
            for k in ("exp_avg", "exp_avg_sq"):
                kept = st[k][keep]
                st[k] = torch.cat((kept, torch.zeros((out.shape[0] - kept.shape[0],) + tuple(kept.shape[1:]), dtype=kept.dtype, device=kept.device)))
            del opt.state[old]
        group["params"][0] = torch.nn.Parameter(out.requires_grad_(True))
        if st is not None:
            opt.state[group["params"][0]] = st
        setattr(model, ATTRS[group["name"]], group["params"][0])
    if has_indexes:
        i = model.indexes
        model.indexes = torch.cat((i[keep], i[clone], i[split].repeat(N)[alive_n]))
    n, dev = model._xyz.shape[0], model._xyz.device
    model.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
    model.denom = torch.zeros((n, 1), device=dev)
    model.max_radii2D = torch.zeros((n,), device=dev)
    return int(keep.sum()), int(clone.sum()), n_split, int(alive.sum())


def add_densification_stats(model, grad, update_filter):
    model.xyz_gradient_accum[update_filter] += torch.norm(grad[update_filter, :2], dim=-1, keepdim=True)
    model.denom[update_filter] += 1


def children_f64(xyz, scaling, rotation, noise, N):
    """The children of the given parent rows (float32 [n,3], [n,3], [n,4]; noise float32 [N * n, 3]) in float64 from the float32
    inputs, in the reference's repeat(N, 1) order. -> (xyz [N n, 3], scaling [N n, 3], xyz error scale [N n, 3] =
    |xyz_r| per component + sum_k |s_k|, which bounds the terms of every component since |R_jk| <= 1)."""
    xyz, scaling, rotation, noise = (t.detach().double().cpu() for t in (xyz, scaling, rotation, noise))
    s = torch.exp(scaling).repeat(N, 1) * noise
    R = build_rotation(rotation).repeat(N, 1, 1)
    kids = torch.bmm(R, s.unsqueeze(-1)).squeeze(-1) + xyz.repeat(N, 1)
    scale = xyz.repeat(N, 1).abs() + s.abs().sum(dim=1, keepdim=True)
    return kids, torch.log(torch.exp(scaling) / (0.8 * N)).repeat(N, 1), scale


def _in_gap(value, threshold):
    return (value / threshold - 1.0).abs() < GAP


def gap_rows(model, thresholds, min_opacity, Ns=(2, 3)):
    """(rows whose largest scale, their own or a child's for any N of Ns, lies within GAP relative of a threshold; rows whose
    opacity lies within GAP relative of min_opacity), judged in float64."""
    smax = torch.exp(model._scaling.detach().double().cpu()).max(dim=1).values
    bad = torch.zeros_like(smax, dtype=torch.bool)
    for t in thresholds:
        for div in (1.0,) + tuple(0.8 * N for N in Ns):
            bad |= _in_gap(smax / div, float(t))
    o = torch.sigmoid(model._opacity.detach().double().cpu()).reshape(-1)
    return bad, (_in_gap(o, float(min_opacity)) if min_opacity else torch.zeros_like(bad))


@torch.no_grad()
def open_gaps(model, thresholds, min_opacity, Ns=(2, 3)):
    """Move the scales (+0.01 in the log, all three of a row) and the opacity logits (+0.01) of the rows inside a gap until none
    is. -> the number of rows still inside a gap (the tests assert 0). Nothing is excluded from any comparison."""
    for _ in range(64):
        bad_s, bad_o = gap_rows(model, thresholds, min_opacity, Ns)
        if not bad_s.any() and not bad_o.any():
            break
        dev = model._scaling.device
        model._scaling.data[bad_s.to(dev)] += 0.01
        model._opacity.data[bad_o.to(dev)] += 0.01
    bad_s, bad_o = gap_rows(model, thresholds, min_opacity, Ns)
    return int(bad_s.sum()) + int(bad_o.sum())
