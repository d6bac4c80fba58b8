"""Adam for a 3DGS model: one HIP kernel launch per step for all parameter groups (csrc/optim.hip, fr_adam_step).

Drops in for the reference's ``torch.optim.Adam(l, lr=0.0, eps=1e-15)`` (fov3dgs/scene/gaussian_model.py:289) and also takes
the rasterizer's row-sparse gradients (``row_sparse_grads = True``: torch.sparse_coo with one sparse dimension), which
torch.optim.Adam refuses. ``param_groups`` / ``state`` / ``state_dict()`` have torch.optim.Adam's layout, so checkpoints
interchange with it in both directions and the reference's model surgery (replace_tensor_to_optimizer, _prune_optimizer,
cat_tensors_to_optimizer) works unchanged: parameters, state tensors and learning rates are looked up afresh on every step.

GPU float32 contiguous parameters only: there is no CPU fallback (the constructor, state_dict and load_state_dict work on
CPU tensors, step() does not)."""
import ctypes as C

import torch

from . import _native

_SPARSE_MODES = {"exact": _native.ADAM_EXACT, "lazy": _native.ADAM_LAZY}
# torch.optim.Adam's own group keys at the only values this optimizer supports: torch's step() indexes them directly, so an
# exported state_dict must carry them to load into torch.optim.Adam and step there
_TORCH_KEYS = {"weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
               "differentiable": False, "fused": None, "decoupled_weight_decay": False}


def _check_group_values(group):
    if group.get("weight_decay", 0) != 0:
        raise ValueError(f"fovraster Adam has no weight decay (weight_decay={group['weight_decay']})")
    if group.get("amsgrad", False):
        raise ValueError("fovraster Adam has no amsgrad")
    if group.get("maximize", False):
        raise ValueError("fovraster Adam has no maximize")


class Adam(torch.optim.Optimizer):
    """``Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, sparse="exact")`` -- torch.optim.Adam without weight decay,
    amsgrad and maximize (the reference uses none), stepped by one kernel.

    Dense gradients: torch.optim.Adam's semantics in torch's order of operations, each operation rounded once
    (``m += (1-b1)(g-m); v = b2 v + (1-b2) g g; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)``; the bias corrections
    are computed on the host in double from the parameter's own ``step``). The two moment updates end in a fused multiply-add
    exactly where torch's float32 GPU kernels do, so exp_avg and exp_avg_sq equal torch.optim.Adam's on the GPU bit for bit.

    Row-sparse gradients (torch.sparse_coo, one sparse dimension; uncoalesced input is coalesced first):
      ``sparse="exact"`` (default)  a row without an entry has gradient zero: the result is torch.optim.Adam on
          ``grad.to_dense()`` -- every row's moments decay and every row moves by its momentum -- without materialising it.
      ``sparse="lazy"``  only the listed rows of the parameter and of both moments are read or written, with the same
          formula and the parameter's global ``step``; rows a view did not touch keep their bits, and their moments do not
          decay. That changes the training dynamics (a Gaussian seen again after k steps continues from moments that are k
          steps old, bias-corrected as if they were current), so it is opt-in. It differs from torch.optim.SparseAdam in the
          placement of eps: SparseAdam takes ``sqrt(v) + eps`` and folds ``sqrt(1-b2^t)`` into the step size, i.e. it
          divides by ``(sqrt(v) + eps) / sqrt(1-b2^t)``; this optimizer keeps Adam's ``sqrt(v)/sqrt(1-b2^t) + eps``. With
          the reference's eps = 1e-15 the two agree to rounding, with eps = 1e-8 and small second moments they do not.

    A parameter whose ``.grad`` is None is skipped and its ``step`` does not advance. step() runs on
    ``torch.cuda.current_stream()`` of the parameters' device with no synchronisation, no host <-> device copy and, after the
    first step (which creates the state), no allocation."""

    # how the exact mode finds the compact row of a Gaussian: "map" = an inverse map of 4 bytes per Gaussian (persistent
    # scratch, filled by a small kernel in front of the step), "search" = a binary search in the rows, no scratch, one launch
    # (2.1x the dense step's time at 6 M Gaussians / 2 M rows, the map 1.2x; tools/optim_bench.py times both)
    exact_lookup = "map"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, sparse="exact"):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if sparse not in _SPARSE_MODES:
            raise ValueError(f"Invalid sparse mode: {sparse!r} (expected 'exact' or 'lazy')")
        self.sparse = sparse
        self._args, self._row_maps = _native.AdamArgs(), {}
        defaults = dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps, **_TORCH_KEYS)
        super().__init__(params, defaults)
        for group in self.param_groups:
            _check_group_values(group)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("sparse", "exact")
        self._args, self._row_maps = _native.AdamArgs(), {}
        for group in self.param_groups:
            for k, v in _TORCH_KEYS.items():
                group.setdefault(k, v)

    def __getstate__(self):
        d = dict(super().__getstate__())
        d["sparse"] = self.sparse  # (self._args, a table of device pointers, and the scratch are rebuilt, never pickled)
        return d

    def add_param_group(self, param_group):
        _check_group_values(param_group)
        super().add_param_group(param_group)

    def load_state_dict(self, state_dict):
        """torch.optim.Adam's dicts load as they are. weight_decay != 0, amsgrad or maximize raise ValueError; a ``step`` kept
        on the GPU (torch's fused / capturable layouts) is moved to the CPU once, here."""
        for group in state_dict["param_groups"]:
            _check_group_values(group)
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for k, v in _TORCH_KEYS.items():
                group.setdefault(k, v)
            group["capturable"], group["fused"] = False, None  # (the layouts that keep `step` on the device)
        for st in self.state.values():
            s = st.get("step")
            if s is None:
                continue
            if not torch.is_tensor(s):
                st["step"] = torch.tensor(float(s), dtype=torch.float32)
            elif s.device.type != "cpu" or s.dtype != torch.float32:
                st["step"] = s.detach().to(device="cpu", dtype=torch.float32)

    def _describe(self, t, p, grad, state, group):
        """Fill descriptor t; returns the tensors it points into (kept alive until the launch) and, for a tensor that uses the
        row map, what the map is built from (one map serves the tensors of a launch that share their rows)."""
        if p.dtype != torch.float32:
            raise RuntimeError(f"fovraster Adam: parameter of dtype {p.dtype} (float32 only)")
        if not p.is_contiguous():
            raise RuntimeError(f"fovraster Adam: parameter of shape {tuple(p.shape)} is not contiguous")
        m, v = state["exp_avg"], state["exp_avg_sq"]
        for name, s in (("exp_avg", m), ("exp_avg_sq", v)):
            if s.shape != p.shape or s.dtype != torch.float32 or s.device != p.device or not s.is_contiguous():
                raise RuntimeError(f"fovraster Adam: state {name} ({tuple(s.shape)}, {s.dtype}, {s.device}) does not match its "
                                   f"parameter ({tuple(p.shape)}, float32, {p.device}, contiguous)")
        if grad.dtype != torch.float32 or grad.device != p.device or grad.shape != p.shape:
            raise RuntimeError(f"fovraster Adam: gradient ({tuple(grad.shape)}, {grad.dtype}, {grad.device}) does not match its "
                               f"parameter ({tuple(p.shape)}, float32, {p.device})")
        t.param, t.exp_avg, t.exp_avg_sq, t.numel = p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
        if grad.layout == torch.strided:
            if not grad.is_contiguous():
                raise RuntimeError(f"fovraster Adam: gradient of shape {tuple(grad.shape)} is not contiguous")
            t.grad, t.rows, t.row_map, t.n_rows, t.width, t.mode = grad.data_ptr(), None, None, 0, 1, _native.ADAM_DENSE
            keep, key = (grad,), None
        elif grad.layout == torch.sparse_coo:
            if grad.sparse_dim() != 1:
                raise RuntimeError(f"fovraster Adam: sparse gradient with {grad.sparse_dim()} sparse dimensions (row-sparse "
                                   "gradients have one)")
            if not grad.is_coalesced():
                grad = grad.coalesce()
            rows, vals = grad._indices(), grad._values()
            n = vals.shape[0]
            if n > 1 and rows.stride(1) != 1:
                rows = rows.contiguous()
            if not vals.is_contiguous():
                vals = vals.contiguous()
            t.grad, t.rows, t.n_rows = vals.data_ptr(), rows.data_ptr(), n
            t.width = p.numel() // p.shape[0] if p.shape[0] else 1
            t.mode = _SPARSE_MODES[self.sparse]
            t.row_map, key = None, None
            if t.mode == _native.ADAM_EXACT and n > 0 and self.exact_lookup == "map":
                scratch = self._row_maps.get(p.device)
                if scratch is None or scratch.numel() < p.shape[0]:  # (grows with the model, never shrinks)
                    scratch = self._row_maps[p.device] = torch.empty(p.shape[0], dtype=torch.int32, device=p.device)
                t.row_map, key = scratch.data_ptr(), (rows.data_ptr(), n, p.shape[0])
            keep = (rows, vals)
        else:
            raise RuntimeError(f"fovraster Adam: gradient layout {grad.layout} (strided or sparse_coo)")
        step = state["step"]
        step += 1
        k = float(step)
        beta1, beta2 = group["betas"]
        bc1 = 1 - beta1 ** k
        bc2 = 1 - beta2 ** k
        t.one_minus_beta1, t.beta2, t.one_minus_beta2 = 1 - beta1, beta2, 1 - beta2
        t.bias_correction2_sqrt, t.eps, t.neg_step_size = bc2 ** 0.5, group["eps"], -(float(group["lr"]) / bc1)
        return keep, key

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device.type != "cuda":
                    raise RuntimeError("fovraster Adam needs GPU tensors: there is no CPU fallback")
                work.append((group, p))
        if not work:
            return loss
        for group, p in work:  # every check that does not need the state comes before the first `step` advances
            _check_group_values(group)
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        lib = _native.load()
        args, keep = self._args, []  # `keep`: what the descriptors point into stays alive until everything is enqueued
        devices = []
        for _, p in work:
            if p.device not in devices:
                devices.append(p.device)

        def launch(n, dev):
            args.num_tensors = n
            with torch.cuda.device(dev):
                rc = lib.fr_adam_step(C.byref(args), torch.cuda.current_stream(dev).cuda_stream)
            if rc != 0:
                raise RuntimeError(f"fovraster adam_step failed ({rc}): {_native.last_error()}")
        for dev in devices:
            k, map_key, stepped = 0, None, []
            try:
                for group, p in work:
                    if p.device != dev:
                        continue
                    kept, key = self._describe(args.tensors[k], p, p.grad, self.state[p], group)
                    keep.append(kept)
                    stepped.append(p)
                    if k == _native.ADAM_MAX_TENSORS - 1 or (key is not None and map_key is not None and key != map_key):
                        # a full table, or rows the map of this launch was not built from: what is in the table goes first
                        full = key is None or map_key is None or key == map_key
                        launch(k + 1 if full else k, dev)
                        if full:
                            k, map_key, stepped = 0, None, []
                        else:
                            args.tensors[0] = args.tensors[k]
                            k, map_key, stepped = 1, key, [p]
                        continue
                    map_key = key if key is not None else map_key
                    k += 1
                if k:
                    launch(k, dev)
            except Exception:  # what was described but not launched did not step
                for p in stepped:
                    self.state[p]["step"] -= 1
                raise
        return loss


def reference_param_groups(model, training_args, spatial_lr_scale=1.0):
    """The six parameter groups of GaussianModel.training_setup (gaussian_model.py:279-286): names, order and learning
    rates. `model` carries _xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation (synthetic.GaussianCloud and the
    reference's GaussianModel do); training_args its position_lr_init, feature_lr, opacity_lr, scaling_lr, rotation_lr."""
    a = training_args
    return [
        {"params": [model._xyz], "lr": a.position_lr_init * spatial_lr_scale, "name": "xyz"},
        {"params": [model._features_dc], "lr": a.feature_lr, "name": "f_dc"},
        {"params": [model._features_rest], "lr": a.feature_lr / 20.0, "name": "f_rest"},
        {"params": [model._opacity], "lr": a.opacity_lr, "name": "opacity"},
        {"params": [model._scaling], "lr": a.scaling_lr, "name": "scaling"},
        {"params": [model._rotation], "lr": a.rotation_lr, "name": "rotation"},
    ]
