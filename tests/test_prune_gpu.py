"""fov3dgs_amd.pruning on the MI355X against tests/prune_ref.py. Every comparison is bit for bit.

The sizes are chosen against the kernels' tile constants (csrc/prune.hip): PRUNE_TILE = 1024 rows per workgroup (256 threads x
PRUNE_PER_THREAD = 4 consecutive rows), at most PRUNE_HIST_WGS = 256 workgroups per histogram pass, each taking
PRUNE_HIST_UNROLL = 4 tiles per round (whole tiles with vector loads, the last tile and unaligned input one by one), and
PRUNE_SCAN_CHUNK = 256 tiles per round of the one-workgroup scan. P = 300 001 has 293 tiles: more than one tile, histogram
workgroups with four whole tiles and others that reach the partial last tile, and two rounds of the scan; the select also runs
at P = 1 100 003 (1 075 tiles), where the histogram workgroups go round their tile loop twice. 63 / 64 / 65 and 255 / 256 / 257
sit around a wave and a workgroup's thread count; 65 537, 300 001 and 1 100 003 are odd, so the 4-row vector path has a scalar tail."""
import ctypes as C

import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native, optim, pruning
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.gaussian_renderer import render
from fov3dgs_amd.loss_utils import l1_ssim_loss
from tests import prune_ref
from tests.adam_ref import ATTRS, NAMES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRUNE_TILE, PRUNE_HIST_WGS, PRUNE_HIST_UNROLL, PRUNE_SCAN_CHUNK = 1024, 256, 4, 256
SIZES = (1, 63, 64, 65, 255, 256, 257, 65_537, 300_001)
SELECT_SIZES = SIZES + (1_100_003,)
assert -(-SIZES[-1] // PRUNE_TILE) > PRUNE_SCAN_CHUNK and SIZES[-1] // PRUNE_TILE > PRUNE_HIST_UNROLL
assert -(-SELECT_SIZES[-1] // PRUNE_TILE) > PRUNE_HIST_WGS * PRUNE_HIST_UNROLL


class Pipe:
    debug = False


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


# ---- metric ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (1, 63, 64, 65, 1000, 100_003))
def test_metric_update_matches_the_torch_expression(P):
    _need_gpu()
    for metric in prune_ref.METRICS:
        for shape in ((P,), (P, 1)):
            got = torch.zeros(shape, device=DEV)
            want = np.zeros(P, dtype=np.float32)
            for view in range(3):
                contribs, counts = prune_ref.metric_inputs(P, view, seed=P)
                if view == 0:
                    counts[:3] = torch.tensor([0, 1, 2], dtype=torch.int32)[:P]
                    contribs[:3] = 0.3
                out = pruning.update_metric_(got, contribs.to(DEV).reshape(shape), counts.to(DEV), metric)
                assert out is got
                want = prune_ref.metric_update(want, contribs.numpy(), counts.numpy(), metric)
                assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.int32), want.view(np.int32)), (metric, shape, view)
    # the counts are not read by the metrics that do not use them
    got = torch.zeros(P, device=DEV)
    pruning.update_metric_(got, torch.full((P,), 2.5, device=DEV), None, "surface")
    assert (got == 2.5).all()


# ---- select ----------------------------------------------------------------------------------------------------------
def _from_bits(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def metric_vectors(P):
    rng = np.random.default_rng(P)
    rnd = rng.random(P).astype(np.float32)
    out = {"all zeros": np.zeros(P, dtype=np.float32)}
    out["40 % zeros"] = np.where(rng.random(P) < 0.4, np.float32(0), rnd * np.exp(4 * rng.standard_normal(P)).astype(np.float32)).astype(np.float32)
    out["all distinct"] = rng.permutation(P).astype(np.float32) * np.float32(0.25) - np.float32(P // 8)  # exact in float32 for P < 2^24
    out["lowest byte"] = _from_bits(np.uint32(0x3F800000) | rng.integers(0, 256, P).astype(np.uint32))
    out["highest byte"] = _from_bits((rng.integers(0, 256, P).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456))
    out["signed zeros"] = np.where(rng.random(P) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    nan = out["40 % zeros"].copy()
    sel = rng.random(P) < 0.3
    nan[sel] = _from_bits(np.where(rng.random(P) < 0.5, np.uint32(0x7FC00000), np.uint32(0xFF800001) | rng.integers(0, 1 << 22, P).astype(np.uint32)))[sel]
    out["NaNs"] = nan
    neg = (rng.standard_normal(P) * 10).astype(np.float32)
    kind = rng.random(P)
    neg[kind < 0.1] = np.inf
    neg[(kind >= 0.1) & (kind < 0.2)] = -np.inf
    neg[(kind >= 0.2) & (kind < 0.3)] = -1e-42
    out["negatives and infinities"] = neg
    return out


@pytest.mark.parametrize("P", SELECT_SIZES)
def test_lowest_k_mask_is_the_stable_order(P):
    _need_gpu()
    ks = sorted({0, 1, int(0.02 * P), P // 2, P - 1, P})
    for name, m in metric_vectors(P).items():
        assert m.dtype == np.float32 and m.shape == (P,)
        order = prune_ref.order(m)
        dev = torch.from_numpy(m.copy()).to(DEV)
        if name == "NaNs" and P >= 63:
            n_nan = int(np.isnan(m).sum())
            assert 0 < n_nan and P - 1 > P - n_nan  # k = P - 1 reaches into the NaNs
        for k in ks:
            got = pruning.lowest_k_mask(dev if k != 1 else dev.unsqueeze(1), k)
            assert got.dtype == torch.bool and got.shape == (P,)
            got_bytes = got.view(torch.uint8).cpu().numpy()
            assert got_bytes.max(initial=0) <= 1, (name, k)  # a bool tensor holds 0 / 1 bytes
            assert int(got_bytes.sum(dtype=np.int64)) == k, (name, k)
            assert np.array_equal(got_bytes.astype(bool), prune_ref.lowest_k_mask(m, k, order)), (name, k)
    # an input that does not start on a 16-byte boundary (the scalar path of every thread)
    if P > 1:
        m = metric_vectors(P)["40 % zeros"]
        dev = torch.from_numpy(m.copy()).to(DEV)[1:]
        k = (P - 1) // 3
        assert dev.data_ptr() % 16 != 0
        assert np.array_equal(pruning.lowest_k_mask(dev, k).cpu().numpy(), prune_ref.lowest_k_mask(m[1:], k))
    with pytest.raises(ValueError):
        pruning.lowest_k_mask(dev, P + 1)


# ---- compaction ------------------------------------------------------------------------------------------------------
def model_tensors(P, seed=0):
    """The tensor set of one prune of the reference's model (gaussian_model.py:624-664) plus a zero-width tensor: payloads are
    random bit patterns, NaNs among them."""
    g = torch.Generator(device=DEV).manual_seed(seed)

    def bits(*shape):
        return torch.randint(-(1 << 31), 1 << 31, shape, generator=g, dtype=torch.int64, device=DEV).to(torch.int32).view(torch.float32)
    out = []
    for row in ((3,), (1, 3), (15, 3), (1,), (3,), (4,)):
        out += [bits(P, *row) for _ in range(3)]  # parameter, exp_avg, exp_avg_sq
    out += [bits(P, 1), bits(P, 1), bits(P)]
    out.append(torch.randint(-(1 << 62), 1 << 62, (P,), generator=g, dtype=torch.int64, device=DEV))
    out.append(torch.empty(P, 0, 3, device=DEV))
    return out


def keep_masks(P):
    g = torch.Generator().manual_seed(P)
    idx = torch.arange(P)
    out = {"keep all": torch.ones(P, dtype=torch.bool), "drop all": torch.zeros(P, dtype=torch.bool),
           "first row": idx == 0, "last row": idx == P - 1, "alternating": idx % 2 == 0}
    for frac in (0.02, 0.5, 0.98):
        out[f"random {frac}"] = torch.rand(P, generator=g) < frac
    out["one workgroup dropped, aligned"] = ~((idx >= PRUNE_TILE) & (idx < 2 * PRUNE_TILE))
    out["one workgroup dropped, unaligned"] = ~((idx >= PRUNE_TILE + 476) & (idx < 2 * PRUNE_TILE + 476))
    return out


def _bits_equal(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    it = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


@pytest.mark.parametrize("P", (0,) + SIZES)
def test_compact_rows_is_boolean_indexing(P):
    _need_gpu()
    tensors = model_tensors(P)
    assert len(tensors) == 23 <= _native.COMPACT_MAX_TENSORS
    for name, keep in keep_masks(P).items():
        keep = keep.to(DEV)
        for invert in (False, True):
            want_rows = ~keep if invert else keep
            n = int(want_rows.sum())
            got = pruning.compact_rows(keep, tensors, invert=invert)
            torch.cuda.set_sync_debug_mode("error")  # with the count given nothing synchronises
            try:
                again = pruning.compact_rows(keep, tensors, n_keep=n, invert=invert)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert len(got) == len(again) == len(tensors)
            for t, a, b in zip(tensors, got, again):
                want = t[want_rows]
                assert a.shape == want.shape == (n,) + tuple(t.shape[1:]) and a.dtype == t.dtype, (name, invert, tuple(t.shape))
                assert _bits_equal(a, want), (name, invert, tuple(t.shape))
                assert _bits_equal(b, want), (name, invert, tuple(t.shape), "n_keep given")
    # a uint8 mask, and more tensors than one launch takes
    if P:
        keep = (torch.arange(P) % 3 != 0)
        many = [tensors[0], tensors[9]] * 20
        assert len(many) > _native.COMPACT_MAX_TENSORS
        for a, t in zip(pruning.compact_rows(keep.to(torch.uint8).to(DEV) * 7, many), many):
            assert _bits_equal(a, t[keep.to(DEV)])


def test_compact_rows_rejects_what_it_cannot_copy():
    _need_gpu()
    keep = torch.ones(8, dtype=torch.bool, device=DEV)
    for bad in (torch.zeros(8, 3, dtype=torch.float16, device=DEV), torch.zeros(8, dtype=torch.uint8, device=DEV),
                torch.zeros(7, 3, device=DEV)):
        with pytest.raises(ValueError):
            pruning.compact_rows(keep, [bad])
    with pytest.raises(ValueError):
        pruning.compact_rows(keep.float(), [torch.zeros(8, 3, device=DEV)])
    with pytest.raises(ValueError):
        pruning.compact_rows(keep, [torch.zeros(8, 3, device=DEV)], n_keep=9)
    # a non-contiguous source is gathered by value
    t = torch.arange(48, dtype=torch.float32, device=DEV).reshape(6, 8).t()
    assert torch.equal(pruning.compact_rows(keep, [t])[0], t)


@pytest.mark.parametrize("P", (65, 300_001))
def test_a_count_one_too_small_leaves_the_surplus_row_unwritten(P):
    _need_gpu()
    lib = _native.load()
    keep = (torch.arange(P) % 5 != 1).to(DEV)
    n = int(keep.sum())
    ws = torch.empty(lib.fr_prune_workspace_bytes(P), dtype=torch.uint8, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    assert lib.fr_compact_plan(P, keep.data_ptr(), 0, count.data_ptr(), ws.data_ptr(), stream) == 0
    assert int(count) == n
    srcs = [torch.randn(P, 3, device=DEV), torch.randn(P, 45, device=DEV), torch.randn(P, device=DEV)]
    guard = -12345.0
    dsts = [torch.full((n,) + tuple(s.shape[1:]), guard, device=DEV) for s in srcs]  # row n - 1 is the guard behind n - 1 rows
    args = _native.CompactArgs()
    args.P, args.num_tensors, args.invert, args.mask, args.workspace = P, len(srcs), 0, keep.data_ptr(), ws.data_ptr()
    for d, s, o in zip(args.tensors, srcs, dsts):
        d.src, d.dst, d.row_words, d.dst_rows = s.data_ptr(), o.data_ptr(), s.numel() // P, n - 1
    assert lib.fr_compact_rows(C.byref(args), stream) == 0, _native.last_error()
    torch.cuda.synchronize()
    for s, o in zip(srcs, dsts):
        assert torch.equal(o[:n - 1], s[keep][:n - 1])
        assert (o[n - 1] == guard).all()


# ---- prune_points ----------------------------------------------------------------------------------------------------
_trained = {}


def trained_model(optimizer_cls):
    """A 3 000-Gaussian model after three training steps (cached: the tests clone it and leave it unchanged)."""
    if optimizer_cls not in _trained:
        torch.manual_seed(0)
        model = prune_ref.Model(syn.scene_1k(P=3000), optimizer_cls, device=DEV)
        cam, bg = syn.camera_1k(128, 128).to(DEV), torch.zeros(3, device=DEV)
        target = torch.rand(3, 128, 128, device=DEV)
        for _ in range(3):
            model.optimizer.zero_grad(set_to_none=True)
            l1_ssim_loss(render(cam, model, Pipe(), bg, cuda_type="pcheck_obb_sum")["render"], target, 0.2).backward()
            model.optimizer.step()
        model.optimizer.zero_grad(set_to_none=True)
        for n in NAMES:
            st = model.optimizer.state[getattr(model, ATTRS[n])]
            assert float(st["step"]) == 3 and st["exp_avg"].abs().max() > 0 and st["exp_avg_sq"].abs().max() > 0, n
        _trained[optimizer_cls] = model
    return prune_ref.clone_model(_trained[optimizer_cls])


def _step_with_random_grads(model, seed=5):
    g = torch.Generator().manual_seed(seed)
    for n in NAMES:
        p = getattr(model, ATTRS[n])
        p.grad = (1e-3 * torch.randn(p.shape, generator=g)).to(DEV)
    model.optimizer.step()
    model.optimizer.zero_grad(set_to_none=True)


@pytest.mark.parametrize("optimizer_cls", (optim.Adam, torch.optim.Adam), ids=("fused", "torch"))
def test_prune_points_is_the_reference_surgery(optimizer_cls):
    _need_gpu()
    P = 3000
    mask = (torch.rand(P, generator=torch.Generator().manual_seed(3)) < 0.3).to(DEV)
    for n_pruned in (None, int(mask.sum())):
        model, ref = trained_model(optimizer_cls), trained_model(optimizer_cls)
        old = {n: getattr(model, ATTRS[n]) for n in NAMES}
        pruning.prune_points(model, mask, n_pruned=n_pruned)
        prune_ref.prune_points(ref, mask)
        prune_ref.assert_same_state(model, ref, f"n_pruned={n_pruned}")  # (also: the groups' parameters are the model's)
        n = P - int(mask.sum())
        assert len(model.optimizer.state) == 6
        for name in NAMES:
            p = getattr(model, ATTRS[name])
            assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.shape[0] == n
            assert old[name] not in model.optimizer.state
            assert set(model.optimizer.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and float(model.optimizer.state[p]["step"]) == 3
        assert torch.equal(model.indexes, torch.arange(P, device=DEV)[~mask])
    # one further step: the same bits as an optimizer freshly built from the pruned state
    fresh = prune_ref.clone_model(model)
    _step_with_random_grads(model)
    _step_with_random_grads(fresh)
    prune_ref.assert_same_state(model, fresh, "the step after the prune")
    assert float(model.optimizer.state[model._xyz]["step"]) == 4 and not prune_ref.same_bits(model._xyz, ref._xyz)


def test_prune_points_side_arrays_of_another_length_and_groups_without_state():
    _need_gpu()
    P = 3000
    mask = (torch.arange(P) % 7 == 0).to(DEV)
    model, ref = trained_model(optim.Adam), trained_model(optim.Adam)
    for m in (model, ref):
        m.xyz_gradient_accum = torch.ones(5, 1, device=DEV)
        del m.indexes
    pruning.prune_points(model, mask)
    prune_ref.prune_points(ref, mask)
    prune_ref.assert_same_state(model, ref, "side arrays of another length")
    n = P - int(mask.sum())
    assert model.xyz_gradient_accum.shape == (n, 1) and model.denom.shape == (n, 1) and model.max_radii2D.shape == (n,)
    assert not model.xyz_gradient_accum.any() and not model.denom.any() and not model.max_radii2D.any()
    assert not hasattr(model, "indexes")
    # no state at all (no step yet), and state for some groups only
    for stepped in ((), ("xyz", "opacity")):
        model = prune_ref.Model(syn.scene_1k(P=P), optim.Adam, device=DEV)
        for n_ in stepped:
            p = getattr(model, ATTRS[n_])
            p.grad = torch.ones_like(p)
        if stepped:
            model.optimizer.step()
            model.optimizer.zero_grad(set_to_none=True)
        ref = prune_ref.clone_model(model)
        pruning.prune_points(model, mask, n_pruned=int(mask.sum()))
        prune_ref.prune_points(ref, mask)
        prune_ref.assert_same_state(model, ref, f"state for {stepped}")
        assert len(model.optimizer.state) == len(stepped) and model._features_rest.shape == (n, 15, 3)


def test_prune_by_opacity():
    _need_gpu()
    model, ref = trained_model(optim.Adam), trained_model(optim.Adam)
    mask = (torch.sigmoid(ref._opacity) < 0.4).squeeze()
    assert 0 < int(mask.sum()) < len(ref)
    pruning.prune(model, "opacity", 0.4)
    prune_ref.prune_points(ref, mask)
    prune_ref.assert_same_state(model, ref, "prune by opacity")
    assert (torch.sigmoid(model._opacity) >= 0.4).all()


# ---- metric_pruning end to end ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", prune_ref.METRICS)
def test_metric_pruning_end_to_end(metric):
    _need_gpu()
    model, ref = trained_model(optim.Adam), trained_model(optim.Adam)
    cams = [syn.camera_ring(i, width=128, height=128).to(DEV) for i in range(4)]
    bg = torch.zeros(3, device=DEV)
    seen = []

    def recording(cam, pc, pipe, bg_, **kw):
        assert kw["cuda_type"] == prune_ref.CUDA_TYPES[metric] and ("loss_map" in kw) == (metric != "max_contrib")
        if "loss_map" in kw:
            assert kw["loss_map"].shape == (3, 128, 128) and (kw["loss_map"] == 1).all()
        pkg = render(cam, pc, pipe, bg_, **kw)
        seen.append({"contribs": pkg["contribs"].clone(), "gs_count": pkg["gs_count"].clone()})
        return pkg

    replay = iter(seen)
    out = pruning.metric_pruning(model, cams, Pipe(), bg, prune_ratio=0.1, metric=metric, render=recording)
    assert out is model and len(seen) == 4 and len(model) == 3000 - 300
    assert sum(int((s["gs_count"] > 0).sum()) for s in seen) > 0
    prune_ref.metric_pruning(ref, cams, Pipe(), bg, 0.1, metric, lambda *a, **kw: next(replay))
    prune_ref.assert_same_state(model, ref, metric)
    with torch.no_grad():
        a = render(cams[0], model, Pipe(), bg, cuda_type="pcheck_obb_sum")["render"]
        b = render(cams[0], ref, Pipe(), bg, cuda_type="pcheck_obb_sum")["render"]
    assert torch.equal(a, b)
    # the default render is the package's own
    again = trained_model(optim.Adam)
    pruning.metric_pruning(again, cams, Pipe(), bg, prune_ratio=0.1, metric=metric)
    prune_ref.assert_same_state(again, ref, f"{metric}, default render")


def test_select_plan_and_rows_enqueue_without_synchronisation():
    _need_gpu()
    model, ref = trained_model(optim.Adam), trained_model(optim.Adam)
    P, k = len(model), 60
    metrics = torch.rand(P, generator=torch.Generator().manual_seed(9)).to(DEV)
    metrics[::3] = 0
    pruning.lowest_k_mask(metrics, k)  # (the workspace exists)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mask = pruning.lowest_k_mask(metrics, k)
        pruning.prune_points(model, mask, n_pruned=k)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    want = torch.from_numpy(prune_ref.lowest_k_mask(metrics.cpu().numpy(), k)).to(DEV)
    assert torch.equal(mask, want)
    prune_ref.prune_points(ref, want)
    prune_ref.assert_same_state(model, ref, "sync-free prune")


# ---- determinism -----------------------------------------------------------------------------------------------------
def test_select_and_compact_are_deterministic():
    _need_gpu()
    P = SIZES[-1]
    m = torch.from_numpy(metric_vectors(P)["40 % zeros"]).to(DEV)
    k = int(0.3 * P)  # inside the run of zeros
    a, b = pruning.lowest_k_mask(m, k), pruning.lowest_k_mask(m, k)
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and int(a.sum()) == k
    tensors = model_tensors(P, seed=1)
    x, y = pruning.compact_rows(a, tensors, invert=True), pruning.compact_rows(a, tensors, n_keep=P - k, invert=True)
    assert all(_bits_equal(p, q) for p, q in zip(x, y)) and x[0].shape[0] == P - k
    # on a side stream
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c = pruning.lowest_k_mask(m, k)
        z = pruning.compact_rows(c, tensors[:3], n_keep=P - k, invert=True)
    s.synchronize()
    assert torch.equal(a, c) and all(_bits_equal(p, q) for p, q in zip(x[:3], z))
