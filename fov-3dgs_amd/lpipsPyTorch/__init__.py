"""LPIPS (VGG16, version 0.1) on the HIP library (csrc/lpips.hip, include/fovraster.h: fr_lpips_*): a drop-in for the two names
of the reference's ``lpipsPyTorch`` package, ``lpips(x, y, net_type, version)`` and ``LPIPS(net_type, version)``.

The reference (lpipsPyTorch/__init__.py:6-21) builds torchvision's VGG16 and fetches two weight files for every picture pair.
This package holds no weights and fetches none: the caller hands them in,

    weights = dict(features=<vgg16().features.state_dict(), or the whole vgg16().state_dict()>,
                   lin=<the LPIPS v0.1 vgg.pth state dict: lin{k}.model.1.weight, or the renamed {k}.1.weight>)

either per object (``LPIPS('vgg', weights=weights)``), or once for the unchanged scripts:

    lpipsPyTorch.set_default_weights(lpipsPyTorch.load_weights("vgg16_features.pth", "lpips_vgg.pth"))
    ...  lpips(render, gt, net_type='vgg')

Semantics are the reference's (modules/networks.py:41-64, :89-96; modules/utils.py:6-8; modules/lpips.py:30-36): the z-score is
applied to the picture as handed in ([0, 1] pictures are not rescaled to [-1, 1]), and the result is ONE ``[1,1,1,1]`` value, the
sum over the five taps AND over the batch -- ``torch.sum(torch.cat(res, 0), 0, True)``; the scripts pass N = 1.

Only 'vgg' is built. ``lpips`` and ``LPIPS`` are the evaluation metric: they build no backward pass and refuse an input that
requires grad. GPU tensors only, there is no CPU fallback. The weights are packed once per object and device, the workspace (two
activation buffers of 2 N x 64 x H x W floats, 2.1 GB for one 1080 x 1920 pair) is kept per picture size; use an object from one
stream at a time.

The training loss is a pair of names of its own, ``lpips_loss(x, y, net_type='vgg', version='0.1', weights=None)`` and
``LPIPSLoss(net_type='vgg', version='0.1', weights=None)``: the same value, bit for bit, and when ``x`` requires grad a
``grad_fn`` whose backward pass is HIP as well (fr_lpips_forward_keep, fr_lpips_backward). ``y`` is the target and must not
require grad. A differentiable call keeps x's 13 post-ReLU maps and the five tap gradients in a buffer of its own, held by its
autograd node (3.25 GB for one 1080 x 1920 pair) and freed by ``backward()``; calls and their backward passes may interleave in
any order. The gradient follows torch's rules -- a ReLU passes it where the kept output is > 0, a 2 x 2 max pool sends it to the
first maximum of its window in row-major order -- with ONE stated deviation: at a pixel whose tap vector is entirely zero the
reference's ``sqrt`` backward yields inf * 0 = NaN and poisons the whole gradient; here the term a_c (sum_j u_j a_j) / (n^2 s)
is taken as 0 at s = 0, its limit, the ReLU rule zeroes the rest, and the gradient stays finite."""
import ctypes as C
import collections.abc
import weakref

import torch

from .. import _native

__all__ = ["lpips", "LPIPS", "lpips_loss", "LPIPSLoss", "set_default_weights", "load_weights", "pack_weights", "pack_backward_weights"]

CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)  # the convolutions of vgg16().features
CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)  # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (networks.py:93-94)
MIN_SIZE = 16  # below it the fourth pool has no output (the reference raises there too)

# the 18 stages between the 19 handles of fr_lpips_args.stage_events
STAGES = ("conv1_1", "conv1_2", "head1", "conv2_1", "conv2_2", "head2", "conv3_1", "conv3_2", "conv3_3", "head3", "conv4_1", "conv4_2",
          "conv4_3", "head4", "conv5_1", "conv5_2", "conv5_3", "head5")

# the 13 stages between the 14 handles of fr_lpips_backward_args.stage_events
BACKWARD_STAGES = ("conv5_3", "conv5_2", "conv5_1", "conv4_3", "conv4_2", "conv4_1", "conv3_3", "conv3_2", "conv3_1", "conv2_2", "conv2_1",
                   "conv1_2", "conv1_1")

PACK_COUNT = 0  # how often pack_weights has run (the tests check that a loop over views packs once)
_default_weights = None
_cache = {}  # id(weights object) -> (weights object, LPIPS): the functional form packs once per weights object and device
_loss_cache = {}  # the same for lpips_loss and LPIPSLoss


def _get(mapping, names, what):
    for n in names:
        if n in mapping:
            return mapping[n]
    raise KeyError(f"lpipsPyTorch: weights[{what!r}] has no key {names[0]!r} (nor {', '.join(repr(n) for n in names[1:])})")


def _f32(t, shape, name):
    if not torch.is_tensor(t):
        raise TypeError(f"lpipsPyTorch: {name} must be a tensor, got {type(t).__name__}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"lpipsPyTorch: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.detach().to(device="cpu", dtype=torch.float32).contiguous()


def _normalise(weights):
    """-> (13 conv weights, 13 biases, 5 lin vectors) as contiguous CPU float32 tensors, validated by name and shape"""
    if not isinstance(weights, collections.abc.Mapping):
        raise TypeError("lpipsPyTorch: weights must be dict(features=..., lin=...)")
    for k in ("features", "lin"):
        if k not in weights:
            raise KeyError(f"lpipsPyTorch: weights has no key {k!r} (expected dict(features=..., lin=...))")
    feats, lin = weights["features"], weights["lin"]
    for k, m in (("features", feats), ("lin", lin)):
        if not isinstance(m, collections.abc.Mapping):
            raise TypeError(f"lpipsPyTorch: weights[{k!r}] must be a mapping of names to tensors")
    ws, bs, ls = [], [], []
    for idx, (ci, co) in zip(CONV_INDICES, CONV_CHANNELS):
        w = _get(feats, (f"{idx}.weight", f"features.{idx}.weight"), "features")
        b = _get(feats, (f"{idx}.bias", f"features.{idx}.bias"), "features")
        ws.append(_f32(w, (co, ci, 3, 3), f"features {idx}.weight"))
        bs.append(_f32(b, (co,), f"features {idx}.bias"))
    for k, c in enumerate(TAP_CHANNELS):
        v = _get(lin, (f"lin{k}.model.1.weight", f"{k}.1.weight"), "lin")
        ls.append(_f32(v, (1, c, 1, 1), f"lin {k}").reshape(c))
    return ws, bs, ls


def pack_weights(weights):
    """weights (see the module's text) -> the packed weights, a CPU uint8 tensor of fr_lpips_packed_bytes (a host routine)"""
    global PACK_COUNT
    ws, bs, ls = _normalise(weights)
    lib = _native.load()
    packed = torch.empty(lib.fr_lpips_packed_bytes(), dtype=torch.uint8)

    def ptrs(ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    rc = lib.fr_lpips_pack_weights(ptrs(ws), ptrs(bs), ptrs(ls), packed.data_ptr())
    if rc != 0:
        raise RuntimeError(f"fovraster lpips_pack_weights failed ({rc}): {_native.last_error()}")
    PACK_COUNT += 1
    return packed


def pack_backward_weights(weights):
    """weights -> the backward pass's weights (the transposed, flipped slabs), a CPU uint8 tensor of fr_lpips_backward_packed_bytes"""
    ws, _, _ = _normalise(weights)
    lib = _native.load()
    packed = torch.empty(lib.fr_lpips_backward_packed_bytes(), dtype=torch.uint8)
    rc = lib.fr_lpips_pack_backward_weights((C.c_void_p * len(ws))(*[t.data_ptr() for t in ws]), packed.data_ptr())
    if rc != 0:
        raise RuntimeError(f"fovraster lpips_pack_backward_weights failed ({rc}): {_native.last_error()}")
    return packed


def set_default_weights(weights):
    """The weights of every later ``lpips(...)`` / ``LPIPS(...)`` without ``weights=`` (None: forget them). Validated here."""
    global _default_weights
    if weights is not None:
        _normalise(weights)
    _default_weights = weights


def load_weights(features_path, lin_path):
    """Read two LOCAL files: a state dict of vgg16().features (or of the whole vgg16()) and the LPIPS v0.1 vgg lin weights."""
    return dict(features=torch.load(features_path, map_location="cpu", weights_only=True),
                lin=torch.load(lin_path, map_location="cpu", weights_only=True))


def _check_net(net_type, version):
    if version != "0.1":
        raise AssertionError("v0.1 is only supported now")
    if net_type in ("alex", "squeeze"):
        raise NotImplementedError(f"lpipsPyTorch: net_type={net_type!r} is not built here; 'vgg' is the one supported "
                                  "(every call in the reference's scripts passes 'vgg')")
    if net_type != "vgg":
        raise NotImplementedError("choose net_type from [alex, squeeze, vgg]; 'vgg' is the one supported here.")


def _resolve(weights):
    if weights is None:
        weights = _default_weights
    if weights is None:
        raise RuntimeError("lpipsPyTorch: no weights -- this package holds none and downloads none: pass weights=dict(features=..., "
                           "lin=...) or call set_default_weights(load_weights(features_path, lin_path)) first")
    return weights


class LPIPS(torch.nn.Module):
    """The criterion of modules/lpips.py:8-36 for net_type='vgg' (the reference's default 'alex' is kept in the signature and
    refused). ``forward(x, y)`` -> [1,1,1,1]; ``taps(x, y)`` -> the five addends [5]; ``features(x)`` -> the five tap maps."""

    def __init__(self, net_type="alex", version="0.1", weights=None):
        super().__init__()
        _check_net(net_type, version)
        self._weights = _resolve(weights)
        _normalise(self._weights)  # a wrong or missing key is named now, not at the first call
        self._packed = {}  # device -> packed weights there
        self._work = {}    # device -> ((N, H, W), workspace)

    def _packed_on(self, dev):
        p = self._packed.get(dev)
        if p is None:
            p = self._packed[dev] = pack_weights(self._weights).to(dev)
        return p

    @staticmethod
    def _check(x, y):
        for t, name in ((x, "x"), (y, "y")):
            if not torch.is_tensor(t):
                raise TypeError(f"lpipsPyTorch: {name} must be a tensor, got {type(t).__name__}")
            if t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"lpipsPyTorch: {name} must be [N,3,H,W], got {tuple(t.shape)}")
            if t.dtype != torch.float32:
                raise ValueError(f"lpipsPyTorch: {name} must be float32, got {t.dtype}")
        if x.shape != y.shape:
            raise ValueError(f"lpipsPyTorch: x and y must have equal shapes, got {tuple(x.shape)} and {tuple(y.shape)}")
        if x.shape[0] < 1 or x.shape[2] < MIN_SIZE or x.shape[3] < MIN_SIZE:
            raise ValueError(f"lpipsPyTorch: pictures must be at least {MIN_SIZE} x {MIN_SIZE} (H < 16 or W < 16 leaves the fourth pool "
                             f"without an output), got {tuple(x.shape)}")
        for t, name in ((x, "x"), (y, "y")):
            if t.requires_grad:
                raise RuntimeError(f"lpipsPyTorch: {name} requires grad, but this is the evaluation metric: no backward pass is built "
                                   "(detach it first)")
        if not x.is_cuda or x.device != y.device:
            raise RuntimeError(f"fovraster LPIPS needs x and y on one GPU (got {x.device} and {y.device}): there is no CPU fallback")

    def _workspace(self, dev, N, H, W):
        lib = _native.load()
        key, work = self._work.get(dev, (None, None))
        if key != (N, H, W):
            nbytes = lib.fr_lpips_workspace_bytes(N, H, W)
            if nbytes < 0:
                raise ValueError(f"lpipsPyTorch: {_native.last_error()}")
            self._work.pop(dev, None)
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self._work[dev] = ((N, H, W), work)
        return work

    def _run(self, x, y, want_taps=False, want_features=False, stage_events=None):
        self._check(x, y)
        lib = _native.load()
        x, y = x.detach().contiguous(), y.detach().contiguous()
        dev = x.device
        N, _, H, W = x.shape
        packed = self._packed_on(dev)
        work = self._workspace(dev, N, H, W)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        taps = torch.empty(5, dtype=torch.float32, device=dev) if want_taps else None
        feats = [torch.empty((N, c, H >> k, W >> k), dtype=torch.float32, device=dev) for k, c in enumerate(TAP_CHANNELS)] if want_features else None
        a = _native.LpipsArgs(size=C.sizeof(_native.LpipsArgs), N=N, H=H, W=W, debug=0, x=x.data_ptr(), y=y.data_ptr(), packed=packed.data_ptr(),
                              workspace=work.data_ptr(), out=out.data_ptr(), out_taps=None if taps is None else taps.data_ptr(),
                              stream=torch.cuda.current_stream(dev).cuda_stream)
        if stage_events is not None:
            a.stage_events = stage_events
        if feats is not None:
            for k, f in enumerate(feats):
                a.out_features[k] = f.data_ptr()
        with torch.cuda.device(dev):
            rc = lib.fr_lpips_forward(C.byref(a))
        if rc != 0:
            raise RuntimeError(f"fovraster lpips_forward failed ({rc}): {_native.last_error()}")
        return out, taps, feats

    def forward(self, x, y):
        return self._run(x, y)[0].reshape(1, 1, 1, 1)

    def stage_times(self, x, y):
        """one call with an event between its stages -> {stage: ms} over STAGES (synchronises; for tools/lpips_bench.py)"""
        lib = _native.load()
        ev = (C.c_void_p * (len(STAGES) + 1))(*[lib.fr_event_create() for _ in range(len(STAGES) + 1)])
        try:
            self._run(x, y, stage_events=ev)
            torch.cuda.synchronize(x.device)
            out, ms = {}, C.c_float()
            for i, name in enumerate(STAGES):
                if lib.fr_event_elapsed_ms(ev[i], ev[i + 1], C.byref(ms)) != 0:
                    raise RuntimeError(f"fovraster: {_native.last_error()}")
                out[name] = ms.value
            return out
        finally:
            for e in ev:
                lib.fr_event_destroy(e)

    def taps(self, x, y):
        """the five per-tap values (each summed over the batch), float32 [5]; their sum is forward(x, y)"""
        return self._run(x, y, want_taps=True)[1]

    def features(self, x):
        """the five tap maps of x before the normalisation, [N,C_k,H >> k,W >> k]"""
        return self._run(x, x, want_features=True)[2]


def _events(lib, n):
    return (C.c_void_p * n)(*[lib.fr_event_create() for _ in range(n)])


def _elapsed(lib, ev, names):
    out, ms = {}, C.c_float()
    for i, name in enumerate(names):
        if lib.fr_event_elapsed_ms(ev[i], ev[i + 1], C.byref(ms)) != 0:
            raise RuntimeError(f"fovraster: {_native.last_error()}")
        out[name] = ms.value
    return out


class _LPIPSFunction(torch.autograd.Function):
    """value = LPIPS(x, y), differentiable in x. The kept state is saved with the node: it belongs to this call alone."""

    @staticmethod
    def forward(ctx, x, y, crit):
        lib = _native.load()
        xc, yc = x.detach().contiguous(), y.detach().contiguous()
        dev = xc.device
        N, _, H, W = xc.shape
        nbytes = lib.fr_lpips_keep_workspace_bytes(N, H, W)
        if nbytes < 0:
            raise ValueError(f"lpipsPyTorch: {_native.last_error()}")
        keep = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        a = _native.LpipsKeepArgs(size=C.sizeof(_native.LpipsKeepArgs), N=N, H=H, W=W, debug=0, x=xc.data_ptr(), y=yc.data_ptr(),
                                  packed=crit._packed_on(dev).data_ptr(), workspace=crit._workspace(dev, N, H, W).data_ptr(),
                                  keep=keep.data_ptr(), out=out.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        if crit._forward_events is not None:
            a.stage_events = crit._forward_events
        with torch.cuda.device(dev):
            rc = lib.fr_lpips_forward_keep(C.byref(a))
        if rc != 0:
            raise RuntimeError(f"fovraster lpips_forward_keep failed ({rc}): {_native.last_error()}")
        ctx.save_for_backward(keep)
        ctx.crit, ctx.shape = crit, (N, H, W)
        crit._last = (weakref.ref(keep), (N, H, W))
        return out.reshape(1, 1, 1, 1)

    @staticmethod
    def backward(ctx, grad_out):
        keep, = ctx.saved_tensors  # a second backward without retain_graph raises here, as torch does
        lib = _native.load()
        crit, (N, H, W) = ctx.crit, ctx.shape
        dev = keep.device
        grad_out = grad_out.detach().to(torch.float32).contiguous()
        grad_x = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
        a = _native.LpipsBackwardArgs(size=C.sizeof(_native.LpipsBackwardArgs), N=N, H=H, W=W, debug=0,
                                      packed_backward=crit._packed_backward_on(dev).data_ptr(), keep=keep.data_ptr(),
                                      workspace=crit._workspace(dev, N, H, W).data_ptr(), grad_out=grad_out.data_ptr(),
                                      grad_x=grad_x.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        if crit._backward_events is not None:
            a.stage_events = crit._backward_events
        with torch.cuda.device(dev):
            rc = lib.fr_lpips_backward(C.byref(a))
        if rc != 0:
            raise RuntimeError(f"fovraster lpips_backward failed ({rc}): {_native.last_error()}")
        return grad_x, None, None


class LPIPSLoss(LPIPS):
    """LPIPS as a training loss (see the module's text). ``forward(x, y)`` -> [1,1,1,1], with a ``grad_fn`` when x requires grad;
    without, it is LPIPS's call: nothing is kept. ``activations()`` -> the 13 post-ReLU maps of x the last differentiable forward
    kept."""

    def __init__(self, net_type="vgg", version="0.1", weights=None):
        super().__init__(net_type, version, weights)
        self._packed_backward = {}  # device -> backward weights there
        self._last = None           # (weak reference to the last kept state, (N, H, W))
        self._forward_events = self._backward_events = None

    def _packed_backward_on(self, dev):
        p = self._packed_backward.get(dev)
        if p is None:
            p = self._packed_backward[dev] = pack_backward_weights(self._weights).to(dev)
        return p

    def forward(self, x, y):
        if torch.is_tensor(y) and y.requires_grad:
            raise RuntimeError("lpipsPyTorch: y requires grad, but y is the target of LPIPSLoss: the gradient is built with respect "
                               "to x only (pass y.detach())")
        if not (torch.is_tensor(x) and x.requires_grad):
            return super().forward(x, y)
        if not torch.is_grad_enabled():  # under torch.no_grad() there is nothing to differentiate
            return super().forward(x.detach(), y)
        self._check(x.detach(), y)
        self._packed_backward_on(x.device)  # packed at the first differentiable call, not inside backward()
        return _LPIPSFunction.apply(x, y, self)

    def activations(self):
        """the 13 post-ReLU maps of x from the last differentiable forward, [N,C_l,H_l,W_l] float32 copies (relu1_1 .. relu5_3).
        The kept state lives as long as that forward's graph: call this before ``backward()`` frees it."""
        if self._last is None:
            raise RuntimeError("lpipsPyTorch: activations() needs a differentiable forward first (an x that requires grad)")
        keep, (N, H, W) = self._last[0](), self._last[1]
        if keep is None:
            raise RuntimeError("lpipsPyTorch: the last differentiable forward's kept state is gone (backward() freed it); call "
                               "activations() before backward(), or backward(retain_graph=True)")
        lib = _native.load()
        floats, out = keep.view(torch.float32), []
        for l, (_, c) in enumerate(CONV_CHANNELS):
            s = 0 if l < 2 else 1 if l < 4 else 2 if l < 7 else 3 if l < 10 else 4
            h, w = H >> s, W >> s
            off = lib.fr_lpips_keep_activation_offset(N, H, W, l) // 4
            m = floats[off:off + N * c * h * w].view(N, c // 8, h, w, 8)
            out.append(m.permute(0, 1, 4, 2, 3).reshape(N, c, h, w).clone())
        return out

    def stage_times(self, x, y):
        """one keeping forward and its backward with an event between the stages -> ({stage: ms} over STAGES, {stage: ms} over
        BACKWARD_STAGES) (synchronises; for tools/lpips_train_bench.py)"""
        lib = _native.load()
        self._forward_events, self._backward_events = _events(lib, len(STAGES) + 1), _events(lib, len(BACKWARD_STAGES) + 1)
        try:
            x = x.detach().clone().requires_grad_(True)
            self(x, y).backward()
            torch.cuda.synchronize(x.device)
            return _elapsed(lib, self._forward_events, STAGES), _elapsed(lib, self._backward_events, BACKWARD_STAGES)
        finally:
            for e in list(self._forward_events) + list(self._backward_events):
                lib.fr_event_destroy(e)
            self._forward_events = self._backward_events = None


def lpips_loss(x, y, net_type="vgg", version="0.1", weights=None):
    """LPIPSLoss as a function: the criterion is kept per weights object, as ``lpips`` keeps its own."""
    _check_net(net_type, version)
    weights = _resolve(weights)
    hit = _loss_cache.get(id(weights))
    if hit is None or hit[0] is not weights:
        hit = _loss_cache[id(weights)] = (weights, LPIPSLoss(net_type, version, weights=weights))
    return hit[1](x, y)


def lpips(x, y, net_type="alex", version="0.1", weights=None):
    """lpipsPyTorch/__init__.py:6-21. The criterion is kept per weights object (and packs once per device): a loop over views
    neither rebuilds the network nor repacks."""
    _check_net(net_type, version)
    weights = _resolve(weights)
    hit = _cache.get(id(weights))
    if hit is None or hit[0] is not weights:
        hit = _cache[id(weights)] = (weights, LPIPS(net_type, version, weights=weights))
    return hit[1](x, y)
