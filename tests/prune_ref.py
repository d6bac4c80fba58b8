"""Reference restatements for fov3dgs_amd.pruning (test infrastructure, not a test), written from the semantics of the
reference's code, not from its text:

  key / order / lowest_k_mask   the total order of the select, in numpy: (key(m), index) ascending, which is the order of
                                torch.sort(m, descending=False, dim=0, stable=True) (tests/test_prune_cpu.py checks that)
  metric_update                 prune.py:82-86 / :90-92 / :95-98, in numpy float32: one rounding per operation
  prune_points                  gaussian_model.py:624-664 with torch's own boolean indexing
  metric_pruning                prune.py:71-110 with torch's own operations; the sort is the STABLE one: inside a run of
                                equal metrics the reference's own choice is arbitrary, the contract here is the lowest indices
  Model                         an object with the attributes of the reference's GaussianModel that pruning touches, which
                                fov3dgs_amd.gaussian_renderer.render() can also draw
  metric_inputs                 one view's (contribs, counts) with every special value the metric kernel meets
"""
import copy

import numpy as np
import torch

from fov3dgs_amd import synthetic as syn
from tests.adam_ref import ATTRS, NAMES, TRAINING_ARGS

METRICS = ("max_comp_efficiency", "surface", "max_contrib")
CUDA_TYPES = {"max_comp_efficiency": "pcheck_obb_loss_weighted_max_count", "surface": "pcheck_obb_loss_weighted_max_count",
              "max_contrib": "pcheck_obb_max"}


def key(m):
    """uint32 sort key of float32 values: NaN -> 0xFFFFFFFF, +-0 -> 0x80000000, negative -> ~bits, else bits | 0x80000000."""
    b = np.ascontiguousarray(m, dtype=np.float32).reshape(-1).view(np.uint32)
    mag = b & np.uint32(0x7FFFFFFF)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    k = np.where(mag == 0, np.uint32(0x80000000), k)
    return np.where(mag > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def order(m):
    """Row indices by ascending (key, index)."""
    return np.argsort(key(m), kind="stable")


def lowest_k_mask(m, k, _order=None):
    mask = np.zeros(np.asarray(m).size, dtype=bool)
    mask[(order(m) if _order is None else _order)[:k]] = True
    return mask


def metric_update(metrics, contribs, counts, metric):
    """New metrics (numpy float32 [P]) after one view. counts: int32 [P] (ignored unless metric is max_comp_efficiency)."""
    metrics, cur = np.asarray(metrics, dtype=np.float32), np.asarray(contribs, dtype=np.float32)
    with np.errstate(all="ignore"):
        if metric == "max_comp_efficiency":
            counts = np.asarray(counts)
            den = counts.astype(np.float32) + np.float32(1e-7)
            cur = np.where(counts < 1, np.float32(0.0), (cur / den).astype(np.float32)).astype(np.float32)
        else:
            assert metric in ("surface", "max_contrib"), metric
        return np.where(metrics < cur, cur, metrics).astype(np.float32)


def metric_inputs(P, view, seed=0):
    """(contribs float32 [P], counts int32 [P]) of one "view": counts 0, 1, 2 and large ones; contribs with 0, denormals, NaN."""
    g = torch.Generator().manual_seed(1000 * seed + view)
    counts = torch.randint(0, 4, (P,), generator=g, dtype=torch.int32)
    big = torch.rand(P, generator=g) < 0.3
    counts = torch.where(big, torch.randint(3, 2_000_000, (P,), generator=g, dtype=torch.int32), counts)
    contribs = torch.rand(P, generator=g) * torch.exp(4 * torch.randn(P, generator=g))
    kind = torch.rand(P, generator=g)
    contribs = torch.where(kind < 0.1, torch.zeros(()), contribs)
    contribs = torch.where((kind >= 0.1) & (kind < 0.2), torch.full((), 1e-41), contribs)
    contribs = torch.where((kind >= 0.2) & (kind < 0.25), torch.full((), float("nan")), contribs)
    return contribs.float(), counts


class Model(syn.GaussianCloud):
    """A GaussianCloud (what render() draws) with the training state of the reference's GaussianModel: `optimizer` over the six
    groups of training_setup (gaussian_model.py:279-289), xyz_gradient_accum / denom [P,1], max_radii2D [P] and `indexes`."""

    def __init__(self, cloud, optimizer_cls, device="cpu", indexes=True):
        ps = [torch.nn.Parameter(p.detach().to(device).clone()) for p in
              (cloud._xyz, cloud._features_dc, cloud._features_rest, cloud._scaling, cloud._rotation, cloud._opacity)]
        super().__init__(*ps, sh_degree=cloud.active_sh_degree)
        from fov3dgs_amd import optim
        self.optimizer = optimizer_cls(optim.reference_param_groups(self, TRAINING_ARGS), lr=0.0, eps=1e-15)
        P = len(self)
        g = torch.Generator().manual_seed(P)
        self.xyz_gradient_accum = torch.rand(P, 1, generator=g).to(device)
        self.denom = torch.randint(0, 9, (P, 1), generator=g).float().to(device)
        self.max_radii2D = (100 * torch.rand(P, generator=g)).to(device)
        if indexes:
            self.indexes = torch.arange(P, dtype=torch.int64).to(device)


def clone_model(model):
    """A deep copy: own parameters, own optimizer of the same class with a copy of every state entry, own side arrays."""
    new = copy.copy(model)
    for n in NAMES:
        setattr(new, ATTRS[n], torch.nn.Parameter(getattr(model, ATTRS[n]).detach().clone()))
    from fov3dgs_amd import optim
    new.optimizer = type(model.optimizer)(optim.reference_param_groups(new, TRAINING_ARGS), lr=0.0, eps=1e-15)
    for go, gn in zip(model.optimizer.param_groups, new.optimizer.param_groups):
        assert go["name"] == gn["name"]
        gn["lr"] = go["lr"]
        st = model.optimizer.state.get(go["params"][0], None)
        if st is not None:
            new.optimizer.state[gn["params"][0]] = {k: (v.clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in st.items()}
    for a in ("xyz_gradient_accum", "denom", "max_radii2D", "indexes"):
        if hasattr(model, a):
            setattr(new, a, getattr(model, a).clone())
    return new


def prune_points(model, mask):
    """gaussian_model.py:642-664: cut the rows where mask is True out of every group's parameter (and out of exp_avg /
    exp_avg_sq where the group has state, keeping the state's other entries), install new nn.Parameters in the group, in
    optimizer.state and on the model; side arrays of the mask's length are cut too, others are zeroed at the new size;
    `indexes` is cut when the model has it."""
    keep = ~mask
    opt = model.optimizer
    new = {}
    for group in opt.param_groups:
        old = group["params"][0]
        st = opt.state.get(old, None)
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][keep], st["exp_avg_sq"][keep]
            del opt.state[old]
        group["params"][0] = torch.nn.Parameter(old.detach()[keep].requires_grad_(True))
        if st is not None:
            opt.state[group["params"][0]] = st
        new[group["name"]] = group["params"][0]
    for n in NAMES:
        setattr(model, ATTRS[n], new[n])
    if model.xyz_gradient_accum.shape[0] == keep.shape[0]:
        model.xyz_gradient_accum = model.xyz_gradient_accum[keep]
        model.denom = model.denom[keep]
        model.max_radii2D = model.max_radii2D[keep]
    else:
        n, dev = model._xyz.shape[0], model._xyz.device
        model.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        model.denom = torch.zeros((n, 1), device=dev)
        model.max_radii2D = torch.zeros((n,), device=dev)
    if hasattr(model, "indexes"):
        model.indexes = model.indexes[keep]


def metric_pruning(model, cameras, pipe, bg, prune_ratio, metric, render):
    """prune.py:71-110 in torch's own operations, with the stable sort."""
    P = model.get_xyz.shape[0]
    dev = model.get_xyz.device
    metrics = torch.zeros(P, device=dev)
    zero = torch.zeros((), device=dev)
    for cam in cameras:
        with torch.no_grad():
            kw = {}
            if CUDA_TYPES[metric].endswith("max_count"):
                kw["loss_map"] = torch.ones((3, int(cam.image_height), int(cam.image_width)), device=dev)
            pkg = render(cam, model, pipe, bg, cuda_type=CUDA_TYPES[metric], **kw)
            cur = pkg["contribs"].float()
            if metric == "max_comp_efficiency":  # per tile test; 0 where no tile tested the Gaussian (:84-85)
                tests = pkg["gs_count"].float()
                cur = torch.where(tests < 1, zero, cur / (tests + 1e-7))
            metrics = torch.where(metrics < cur, cur, metrics)  # (:86: a NaN cur leaves the old value)
    pruned = torch.zeros(P, dtype=torch.bool, device=dev)
    pruned[metrics.sort(stable=True).indices[:int(P * prune_ratio)]] = True  # (:101-107, ties by index)
    prune_points(model, pruned)
    return model


def state_tensors(model):
    """{name: tensor} of everything a prune touches: parameters, moments, steps, side arrays, indexes."""
    out = {}
    for g in model.optimizer.param_groups:
        p = g["params"][0]
        assert p is getattr(model, ATTRS[g["name"]]), g["name"]
        out[g["name"]] = p.detach()
        for k, v in model.optimizer.state.get(p, {}).items():
            out[f"{g['name']}.{k}"] = v if torch.is_tensor(v) else torch.tensor(v)
    for a in ("xyz_gradient_accum", "denom", "max_radii2D", "indexes"):
        if hasattr(model, a):
            out[a] = getattr(model, a)
    return out


def same_bits(a, b):
    """Bitwise equality of two tensors of the same dtype and shape (NaN payloads and signed zeros included)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.numel() == 0:
        return True
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    it = {4: torch.int32, 8: torch.int64}.get(a.element_size())
    return torch.equal(a.view(it), b.view(it)) if it is not None and a.dtype != torch.bool else torch.equal(a, b)


def assert_same_state(a, b, what=""):
    sa, sb = state_tensors(a), state_tensors(b)
    assert sa.keys() == sb.keys(), (what, sorted(sa), sorted(sb))
    for k in sa:
        assert same_bits(sa[k], sb[k]), f"{what} {k}: {tuple(sa[k].shape)} vs {tuple(sb[k].shape)}"
