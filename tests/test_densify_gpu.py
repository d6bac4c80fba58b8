"""fov3dgs_amd.densify on the MI355X against tests/densify_ref.py, with the same noise on both sides.

Layout and copies are compared bit for bit: every parameter except the children's xyz and scaling, every exp_avg / exp_avg_sq,
`step`, the side arrays, `indexes`, the row counts. The children's xyz and scaling are compared with a float64 restatement of
the same expressions from the float32 inputs (densify_ref.children_f64):
    |d xyz| <= 32 * 2^-24 * (|xyz_r| + sum_k |s_k|) per component   (4 x the distance of torch's float32 arithmetic from
                                                                    float64, measured at 7.9 units over 2 M random rows on the
                                                                    CPU; the margin is for the device's expf and sqrtf)
    |d scaling| <= 2^-21 * max(1, |want|)                           (2 ulp expf, one rounding of the division, 2 ulp logf)
A transposed or unnormalised rotation, a missing 0.8 N or noise shared between copies misses these by orders of magnitude. The
measured maxima go to the parity report.

Decisions are exact by construction: the inputs are nudged on the CPU (densify_ref.open_gaps) so that, in float64, no largest
scale -- a parent's or a child's -- lies within relative 1e-4 of a size threshold and no sigmoid(opacity) within 1e-4 of
min_opacity; the tests assert that no row was left inside a gap, and nothing is excluded from any comparison.
xyz_gradient_accum / denom is a correctly rounded division and needs no gap. The inputs hold denom = 0 with accum = 0 (NaN ->
0), denom = 0 with accum > 0 (inf: hot) and negative accum (clone takes |g|, split the signed g).

The sizes are chosen against the tile constants (csrc/row_scan.h): 1024 rows per workgroup (256 threads x 4 rows), 256 tiles per
round of the one-workgroup scans. 63 / 64 / 65 and 255 / 256 / 257 sit around a wave and a workgroup's thread count, 1 025 is one
tile and one row, 65 537 is 64 tiles and one row, 300 001 has 293 tiles: two rounds of the scan, a partial last tile, an odd
length."""
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import densify, optim
from fov3dgs_amd import synthetic as syn
from fov3dgs_amd.gaussian_renderer import render
from fov3dgs_amd.loss_utils import l1_ssim_loss
from tests import checks, densify_ref, parity_report, prune_ref
from tests.adam_ref import ATTRS, NAMES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE, SCAN_CHUNK = 1024, 256
SIZES = (1, 63, 64, 65, 255, 256, 257, 1_025, 65_537, 300_001)
assert -(-SIZES[-1] // TILE) > SCAN_CHUNK and SIZES[-1] % TILE and SIZES[-1] % 2
PERCENT_DENSE, EXTENT = 0.08, 1.0        # t_dense = 0.08: about the median largest scale of scene_1k; t_world = 0.1
MAX_GRAD, MIN_OPACITY, MAX_SCREEN = 0.2, 0.1, 20
SCALE_PERCENT, BIG_SIZE = 0.12, 0.09     # scale_densify_and_split's and densify_and_split_big_size's thresholds
THRESHOLDS = (PERCENT_DENSE * EXTENT, 0.1 * EXTENT, SCALE_PERCENT * EXTENT, BIG_SIZE)
XYZ_UNITS, SCALING_UNITS = 32.0, 1.0     # of 2^-24 (|xyz_r| + sum |s_k|) and of 2^-21 max(1, |want|)


class Pipe:
    debug = False


def _need_gpu():
    assert torch.cuda.is_available(), "this test needs the MI355X"


_bases = {}


def base_model(P, optimizer_cls=optim.Adam, indexes=True, state=True):
    """A model of P Gaussians after one optimizer step (cached: the tests clone it and leave it unchanged), with the special
    gradient sums and the gaps around every threshold."""
    key = (P, optimizer_cls, indexes, state)
    if key not in _bases:
        model = prune_ref.Model(syn.scene_1k(P=P, seed=P % 97), optimizer_cls, device=DEV, indexes=indexes)
        model.percent_dense = PERCENT_DENSE
        g = torch.Generator().manual_seed(P)
        if state:
            for n in NAMES:
                p = getattr(model, ATTRS[n])
                p.grad = (1e-3 * torch.randn(p.shape, generator=g)).to(DEV)
            model.optimizer.step()
            model.optimizer.zero_grad(set_to_none=True)
        kind = torch.rand(P, generator=g).to(DEV)
        model.xyz_gradient_accum[kind < 0.1] *= -1.0
        zero = (kind >= 0.1) & (kind < 0.2)
        model.xyz_gradient_accum[zero] = 0.0
        model.denom[zero] = 0.0
        if indexes:
            model.indexes = torch.randint(-(1 << 62), 1 << 62, (P,), generator=g, dtype=torch.int64).to(DEV)
        assert densify_ref.open_gaps(model, THRESHOLDS, MIN_OPACITY) == 0  # no row is left inside a gap
        if P >= 1000:
            a, d = model.xyz_gradient_accum.reshape(-1), model.denom.reshape(-1)
            assert ((d == 0) & (a == 0)).any() and ((d == 0) & (a > 0)).any() and ((d > 0) & (a < 0)).any()
        _bases[key] = model
    return prune_ref.clone_model(_bases[key])


def _noise(n, seed=11):
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(seed)).to(DEV)


def check_children(base, model, split, alive, N, noise, what, ref=None):
    """The children's xyz and scaling against float64. -> the number of rows in front of the children."""
    parents = split & alive
    n_split, n_child = int(split.sum()), int(parents.sum())
    n_fixed = len(model) - N * n_child
    if n_child == 0:
        return n_fixed
    z = noise.view(N, n_split, 3)[:, alive[split]].reshape(-1, 3)
    xyz64, sc64, scale = densify_ref.children_f64(base._xyz[parents], base._scaling[parents], base._rotation[parents], z, N)
    units = {}
    for who, m in (("hip", model), ("torch", ref)):
        if m is None:
            continue
        dx = (m._xyz.detach()[n_fixed:].double().cpu() - xyz64).abs() / (2.0 ** -24 * scale)
        ds = (m._scaling.detach()[n_fixed:].double().cpu() - sc64).abs() / (2.0 ** -21 * sc64.abs().clamp(min=1.0))
        units[f"{who}_xyz_units"], units[f"{who}_scaling_units"] = float(dx.max()), float(ds.max())
    parity_report.record("densify", what, children=N * n_child, xyz_units_allowed=XYZ_UNITS, scaling_units_allowed=SCALING_UNITS, **units)
    print(what, units)
    assert units["hip_xyz_units"] <= XYZ_UNITS, (what, units)
    assert units["hip_scaling_units"] <= SCALING_UNITS, (what, units)
    return n_fixed


def check_state(base, model, ref, split, alive, N, noise, what):
    """model (grown by fov3dgs_amd.densify) against ref (grown by densify_ref): everything bit for bit except the children's
    xyz and scaling, which are held to their float64 bounds."""
    assert len(model) == len(ref), (what, len(model), len(ref))
    n_fixed = check_children(base, model, split, alive, N, noise, what, ref)
    sa, sb = prune_ref.state_tensors(model), prune_ref.state_tensors(ref)
    assert sa.keys() == sb.keys(), (what, sorted(sa), sorted(sb))
    for k in sa:
        if k in ("xyz", "scaling"):
            assert sa[k].shape == sb[k].shape and prune_ref.same_bits(sa[k][:n_fixed], sb[k][:n_fixed]), (what, k)
        else:
            assert prune_ref.same_bits(sa[k], sb[k]), f"{what} {k}: {tuple(sa[k].shape)} vs {tuple(sb[k].shape)}"
    n = len(model)
    assert model.xyz_gradient_accum.shape == (n, 1) and model.denom.shape == (n, 1) and model.max_radii2D.shape == (n,)
    assert not model.xyz_gradient_accum.any() and not model.denom.any() and not model.max_radii2D.any()
    for name in NAMES:
        p = getattr(model, ATTRS[name])
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.shape[0] == n, name


def run_composite(P, N, optimizer_cls=optim.Adam, max_screen_size=MAX_SCREEN, max_grad=MAX_GRAD, min_opacity=MIN_OPACITY, **kw):
    base, model, ref = (base_model(P, optimizer_cls, **kw) for _ in range(3))
    keep, clone, split, child = densify_ref.plan_classes(base, max_grad, min_opacity, EXTENT, max_screen_size, N)
    noise = _noise(N * int(split.sum()))
    old = {n: getattr(model, ATTRS[n]) for n in NAMES}
    counts = densify.densify_and_prune(model, max_grad, min_opacity, EXTENT, max_screen_size, N=N, noise=noise)
    densify_ref.densify_and_prune(ref, max_grad, min_opacity, EXTENT, max_screen_size, N, noise)
    assert tuple(counts) == (int(keep.sum()), int(clone.sum()), int(split.sum()), int(child.sum())), counts
    what = f"densify_and_prune P={P} N={N} {optimizer_cls.__module__.split('.')[0]} max_screen_size={max_screen_size}"
    check_state(base, model, ref, split, child, N, noise, what)
    for n in NAMES:
        assert getattr(model, ATTRS[n]) is not old[n] and old[n] not in model.optimizer.state
    return base, model, counts


# ---- the composite ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (2, 3))
@pytest.mark.parametrize("P", SIZES)
def test_densify_and_prune_is_the_reference_sequence(P, N):
    _need_gpu()
    base, model, counts = run_composite(P, N)
    if P >= 65_537:  # every class occurs; the world-size test cuts parents and children
        assert min(counts) > 100 and counts.children_per_copy < counts.split
        for n in NAMES:
            st = model.optimizer.state[getattr(model, ATTRS[n])]
            assert float(st["step"]) == 1 and st["exp_avg"][:counts.kept].any() and not st["exp_avg"][counts.kept:].any()


@pytest.mark.parametrize("optimizer_cls", (optim.Adam, torch.optim.Adam), ids=("fused", "torch"))
def test_densify_and_prune_with_both_optimizers_and_without_max_screen_size(optimizer_cls):
    _need_gpu()
    P = 4099  # four whole tiles and three rows
    for N in (2, 3):
        _, _, with_size = run_composite(P, N, optimizer_cls)
        _, _, without = run_composite(P, N, optimizer_cls, max_screen_size=None)
        _, _, zero = run_composite(P, N, optimizer_cls, max_screen_size=0)  # (falsy, as the reference tests it)
        assert without == zero and without.kept > with_size.kept and without.children_per_copy > with_size.children_per_copy
        assert without.split == with_size.split and without.children_per_copy <= without.split


# ---- the other operations --------------------------------------------------------------------------------------------
def _mean_grads(m):
    return densify_ref._mean_grads(m)


# name -> (split mask of the base model or None, the call on fov3dgs_amd.densify, the call on densify_ref)
OPERATIONS = {
    "clone_rows": (None, lambda m, a: densify.clone_rows(m, a["mask"]), lambda m, a: densify_ref.clone_rows(m, a["mask"])),
    "position_grad_densify": (None, lambda m, a: densify.position_grad_densify(m, MAX_GRAD),
                              lambda m, a: densify_ref.position_grad_densify(m, MAX_GRAD)),
    "densify_and_clone": (None, lambda m, a: densify.densify_and_clone(m, a["grads"], MAX_GRAD, EXTENT),
                          lambda m, a: densify_ref.densify_and_clone(m, a["grads"], MAX_GRAD, EXTENT)),
    "split_rows": (lambda b, a: a["mask"], lambda m, a: densify.split_rows(m, a["mask"], N=a["N"], noise=a["noise"]),
                   lambda m, a: densify_ref.split_rows(m, a["mask"], a["N"], a["noise"])),
    "idx_densify_and_split": (lambda b, a: a["mask"], lambda m, a: densify.idx_densify_and_split(m, a["mask"].unsqueeze(1), N=a["N"], noise=a["noise"]),
                              lambda m, a: densify_ref.idx_densify_and_split(m, a["mask"], a["N"], a["noise"])),
    "scale_densify_and_split": (lambda b, a: densify_ref.scale_mask(b, SCALE_PERCENT * EXTENT),
                                lambda m, a: densify.scale_densify_and_split(m, EXTENT, SCALE_PERCENT, N=a["N"], noise=a["noise"]),
                                lambda m, a: densify_ref.scale_densify_and_split(m, EXTENT, SCALE_PERCENT, a["N"], a["noise"])),
    "densify_and_split_big_size": (lambda b, a: densify_ref.scale_mask(b, BIG_SIZE),
                                   lambda m, a: densify.densify_and_split_big_size(m, BIG_SIZE, N=a["N"], noise=a["noise"]),
                                   lambda m, a: densify_ref.densify_and_split_big_size(m, BIG_SIZE, a["N"], a["noise"])),
    "densify_and_split": (lambda b, a: densify_ref.split_mask(b, a["grads"], MAX_GRAD, EXTENT),
                          lambda m, a: densify.densify_and_split(m, a["grads"], MAX_GRAD, EXTENT, N=a["N"], noise=a["noise"]),
                          lambda m, a: densify_ref.densify_and_split(m, a["grads"], MAX_GRAD, EXTENT, a["N"], a["noise"])),
    # the reference's padded_grad: grads shorter than the model
    "densify_and_split, short grads": (lambda b, a: densify_ref.split_mask(b, a["grads"][:-7], MAX_GRAD, EXTENT),
                                       lambda m, a: densify.densify_and_split(m, a["grads"][:-7], MAX_GRAD, EXTENT, N=a["N"], noise=a["noise"]),
                                       lambda m, a: densify_ref.densify_and_split(m, a["grads"][:-7], MAX_GRAD, EXTENT, a["N"], a["noise"])),
}


@pytest.mark.parametrize("optimizer_cls", (optim.Adam, torch.optim.Adam), ids=("fused", "torch"))
@pytest.mark.parametrize("name", sorted(OPERATIONS))
def test_every_operation_is_the_reference_surgery(name, optimizer_cls):
    _need_gpu()
    split_of, ours, theirs = OPERATIONS[name]
    for P in (257, 4099):
        for N in (2, 3) if split_of else (2,):
            base, model, ref = (base_model(P, optimizer_cls) for _ in range(3))
            a = {"N": N, "mask": (torch.rand(P, generator=torch.Generator().manual_seed(P + N)) < 0.3).to(DEV), "grads": _mean_grads(base)}
            split = split_of(base, a) if split_of else torch.zeros(P, dtype=torch.bool, device=DEV)
            assert split_of is None or 0 < int(split.sum()) < P
            a["noise"] = _noise(N * int(split.sum()), seed=P)
            counts = ours(model, a)
            theirs(ref, a)
            assert len(model) > P - int(split.sum()) and counts.split == counts.children_per_copy == int(split.sum())
            assert counts.kept == P - counts.split and len(model) == counts.kept + counts.cloned + N * counts.split
            check_state(base, model, ref, split, split, N, a["noise"], f"{name} P={P} N={N} {optimizer_cls.__module__.split('.')[0]}")
            assert float(model.optimizer.state[model._xyz]["step"]) == 1


# ---- edges -----------------------------------------------------------------------------------------------------------
def test_nothing_selected_changes_no_bit_but_installs_new_parameters():
    _need_gpu()
    P = 4099
    def composite(m):
        m.xyz_gradient_accum.zero_()  # g = 0 (0 / 0 -> NaN -> 0 included): nothing is hot; nothing is faint, no size test
        return densify.densify_and_prune(m, MAX_GRAD, 0.0, EXTENT, None)
    for call in (composite,
                 lambda m: densify.clone_rows(m, torch.zeros(P, dtype=torch.bool, device=DEV)),
                 lambda m: densify.split_rows(m, torch.zeros(P, dtype=torch.bool, device=DEV), N=3)):
        base, model = base_model(P), base_model(P)
        old = {n: getattr(model, ATTRS[n]) for n in NAMES}
        assert tuple(call(model)) == (P, 0, 0, 0)
        for n in NAMES:
            new = getattr(model, ATTRS[n])
            assert new is not old[n] and new.data_ptr() != old[n].data_ptr() and prune_ref.same_bits(new, getattr(base, ATTRS[n])), n
            assert any(g["params"][0] is new for g in model.optimizer.param_groups)
            st, st0 = model.optimizer.state[new], base.optimizer.state[getattr(base, ATTRS[n])]
            assert prune_ref.same_bits(st["exp_avg"], st0["exp_avg"]) and prune_ref.same_bits(st["exp_avg_sq"], st0["exp_avg_sq"])
        assert prune_ref.same_bits(model.indexes, base.indexes)
        assert not model.xyz_gradient_accum.any() and not model.denom.any() and not model.max_radii2D.any()  # (:704-706, whatever was selected)


@pytest.mark.parametrize("P", (65, 4099))
def test_everything_cloned_everything_split_everything_cut(P):
    _need_gpu()
    ones = torch.ones(P, dtype=torch.bool, device=DEV)
    base, model, ref = (base_model(P) for _ in range(3))
    assert tuple(densify.clone_rows(model, ones)) == (P, P, 0, 0)
    densify_ref.clone_rows(ref, ones)
    check_state(base, model, ref, ~ones, ~ones, 2, _noise(0), f"everything cloned P={P}")
    assert prune_ref.same_bits(model._xyz[P:], base._xyz) and prune_ref.same_bits(model.indexes[P:], base.indexes)
    for N in (1, 4):
        base, model, ref = (base_model(P) for _ in range(3))
        noise = _noise(N * P)
        assert tuple(densify.split_rows(model, ones, N=N, noise=noise)) == (0, 0, P, P)
        densify_ref.split_rows(ref, ones, N, noise)
        check_state(base, model, ref, ones, ones, N, noise, f"everything split P={P} N={N}")
        assert len(model) == N * P and not model.optimizer.state[model._xyz]["exp_avg"].any()
    # every row and every child is too faint: 0 rows are left
    base, model, ref = (base_model(P) for _ in range(3))
    split = densify_ref.plan_classes(base, MAX_GRAD, 2.0, EXTENT, MAX_SCREEN, 2)[2]
    noise = _noise(2 * int(split.sum()))
    counts = densify.densify_and_prune(model, MAX_GRAD, 2.0, EXTENT, MAX_SCREEN, noise=noise)
    densify_ref.densify_and_prune(ref, MAX_GRAD, 2.0, EXTENT, MAX_SCREEN, 2, noise)
    assert tuple(counts) == (0, 0, int(split.sum()), 0) and len(model) == 0
    check_state(base, model, ref, split, ~split, 2, noise, f"everything cut P={P}")
    # ... and an empty model goes in (nothing is launched)
    for call in (lambda m: densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN),
                 lambda m: densify.clone_rows(m, torch.zeros(0, dtype=torch.bool, device=DEV)),
                 lambda m: densify.split_rows(m, torch.zeros(0, dtype=torch.bool, device=DEV))):
        old = model._xyz
        assert tuple(call(model)) == (0, 0, 0, 0) and len(model) == 0 and model._xyz is not old
        assert model._features_rest.shape == (0, 15, 3) and model.denom.shape == (0, 1) and model.indexes.shape == (0,)
    torch.cuda.synchronize()


def test_an_optimizer_without_state_and_a_model_without_indexes():
    _need_gpu()
    P = 4099
    for kw in ({"state": False}, {"indexes": False}, {"state": False, "indexes": False}):
        _, model, _ = run_composite(P, 2, **kw)
        assert len(model.optimizer.state) == (0 if kw.get("state") is False else 6)
        assert hasattr(model, "indexes") == (kw.get("indexes") is not False)
    # state for some groups only; `indexes` of another length is left alone
    base = base_model(P, state=False)
    for n in ("xyz", "opacity"):
        p = getattr(base, ATTRS[n])
        p.grad = torch.ones_like(p)
    base.optimizer.step()
    base.optimizer.zero_grad(set_to_none=True)
    base.indexes = torch.arange(5, device=DEV)
    model, ref = prune_ref.clone_model(base), prune_ref.clone_model(base)
    mask = (torch.arange(P, device=DEV) % 7 == 0)
    noise = _noise(3 * int(mask.sum()))
    densify.split_rows(model, mask, N=3, noise=noise)
    del ref.indexes  # (the reference's prune_points would index it with the mask)
    densify_ref.split_rows(ref, mask, 3, noise)
    ref.indexes = torch.arange(5, device=DEV)
    check_state(base, model, ref, mask, mask, 3, noise, "state for xyz and opacity only")
    assert len(model.optimizer.state) == 2 and torch.equal(model.indexes, torch.arange(5, device=DEV))


def test_noise_is_checked_drawn_reproducibly_and_not_shared_between_copies():
    _need_gpu()
    P, N = 4099, 3
    mask = (torch.arange(P, device=DEV) % 5 == 0)
    n_split = int(mask.sum())
    for bad in (_noise(N * n_split + 1), _noise(n_split), _noise(N * n_split).double()):
        with pytest.raises(ValueError, match="noise"):
            densify.split_rows(base_model(P), mask, N=N, noise=bad)
    runs = []
    for seed in (1, 1, 2):
        model = base_model(P)
        densify.split_rows(model, mask, N=N, generator=torch.Generator(device=DEV).manual_seed(seed))
        runs.append(model._xyz.detach().clone())
    assert prune_ref.same_bits(runs[0], runs[1]) and not prune_ref.same_bits(runs[0], runs[2])
    kids = runs[0][P - n_split:].view(N, n_split, 3)
    assert not torch.equal(kids[0], kids[1]) and not torch.equal(kids[1], kids[2])
    a, b = base_model(P), base_model(P)
    torch.manual_seed(5)
    densify.split_rows(a, mask, N=N)
    torch.manual_seed(5)
    densify.split_rows(b, mask, N=N)
    prune_ref.assert_same_state(a, b, "torch.manual_seed")


# ---- still trainable afterwards --------------------------------------------------------------------------------------
def test_a_grown_model_trains_on_like_the_reference_grown_one():
    """render + l1_ssim_loss backward + one optim.Adam step after densify_and_prune on 20 000 Gaussians.

    The children's xyz and scaling of the two models agree within their float64 bounds (checked first), not bit for bit, so the
    reference-grown model takes those rows over from the HIP-grown one; from then on the two states are equal bit for bit. The
    backward pass sums with float atomics, whose order is not defined: two renders of the SAME state do not give the same bits
    (measured here: the two models' gradients are compared and recorded, and must agree as whole tensors within the suite's
    checks.GRAD_REL_L2). "The same step" is therefore the step with the same gradients: the reference-grown model steps with the
    gradients the HIP-grown model's render produced, and every tensor of the stepped states must be equal bit for bit."""
    _need_gpu()
    P, N = 20_000, 2
    torch.manual_seed(0)
    base = prune_ref.Model(syn.scene_1k(P=P), optim.Adam, device=DEV)
    base.percent_dense = PERCENT_DENSE
    cam, bg = syn.camera_1k(128, 128).to(DEV), torch.zeros(3, device=DEV)
    target = torch.rand(3, 128, 128, device=DEV)

    def backward(m):
        m.optimizer.zero_grad(set_to_none=True)
        l1_ssim_loss(render(cam, m, Pipe(), bg, cuda_type="pcheck_obb_sum")["render"], target, 0.2).backward()
        grads = {n: getattr(m, ATTRS[n]).grad for n in NAMES}
        return {n: (g.to_dense() if g.is_sparse else g).clone() for n, g in grads.items()}
    backward(base)
    base.optimizer.step()
    base.optimizer.zero_grad(set_to_none=True)
    assert densify_ref.open_gaps(base, THRESHOLDS, MIN_OPACITY) == 0
    model, ref = prune_ref.clone_model(base), prune_ref.clone_model(base)
    keep, clone, split, child = densify_ref.plan_classes(base, MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN, N)
    noise = _noise(N * int(split.sum()))
    counts = densify.densify_and_prune(model, MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN, N=N, noise=noise)
    densify_ref.densify_and_prune(ref, MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN, N, noise)
    assert min(counts) > 100
    check_state(base, model, ref, split, child, N, noise, "before the step, P=20000")
    n_fixed = counts.kept + counts.cloned
    with torch.no_grad():
        ref._xyz[n_fixed:] = model._xyz[n_fixed:]
        ref._scaling[n_fixed:] = model._scaling[n_fixed:]
    prune_ref.assert_same_state(model, ref, "before the step")
    before = model._xyz.detach().clone()
    ref_grads = backward(ref)
    grads = backward(model)
    for n in NAMES:
        st = checks.grad_stats(grads[n].cpu().numpy(), ref_grads[n].cpu().numpy())
        parity_report.record("densify", f"gradients of two renders of one grown state, {n}", rel_l2=st["rel_l2"], max_abs=st["max_abs"],
                             differing_values=int((grads[n] != ref_grads[n]).sum()), rel_l2_allowed=checks.GRAD_REL_L2)
        assert st["rel_l2"] <= checks.GRAD_REL_L2 and st["rows_with_gradient"] > 0, (n, st)
        getattr(ref, ATTRS[n]).grad = getattr(model, ATTRS[n]).grad.clone()
    model.optimizer.step()
    ref.optimizer.step()
    prune_ref.assert_same_state(model, ref, "the step after densify_and_prune")
    st = model.optimizer.state[model._xyz]
    assert float(st["step"]) == 2
    # new rows start from zero moments: exp_avg = (1 - beta1) g after their first step, and those with a gradient moved
    new_g = grads["xyz"][counts.kept:]
    assert new_g.any()
    assert torch.allclose(st["exp_avg"][counts.kept:], 0.1 * new_g, rtol=1e-6, atol=0)
    moved = (model._xyz.detach()[counts.kept:] != before[counts.kept:]).any(dim=1)
    assert torch.equal(moved, (new_g != 0).any(dim=1))


# ---- add_densification_stats -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (1, 257, 100_003))
def test_add_densification_stats(P):
    _need_gpu()
    g = torch.Generator().manual_seed(P)
    model = base_model(min(P, 257))
    grad = (torch.randn(P, 3, generator=g) * torch.exp(3 * torch.randn(P, 3, generator=g))).to(DEV)
    filt = (torch.rand(P, generator=g) < 0.6).to(DEV)
    filt[0] = True
    if P > 1:
        filt[1] = False
    accum0 = torch.randn(P, 1, generator=g).to(DEV)
    denom0 = torch.randint(0, 9, (P, 1), generator=g).float().to(DEV)
    want = torch.hypot(grad[:, 0].double(), grad[:, 1].double()).unsqueeze(1)
    # the increment itself: from zero sums
    model.xyz_gradient_accum, model.denom = torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV)
    densify.add_densification_stats(model, grad, filt)
    inc = model.xyz_gradient_accum.clone()
    rel = ((inc.double() - want).abs() / want)[filt]
    parity_report.record("densify", f"add_densification_stats P={P}", max_rel=float(rel.max()) if rel.numel() else 0.0, allowed=2.0 ** -22)
    assert (rel <= 2.0 ** -22).all(), float(rel.max())
    assert not inc[~filt].any() and torch.equal(model.denom, filt.float().unsqueeze(1))
    # ... added to what is there, through a tensor that carries the gradient as .grad; the other rows keep their bits
    model.xyz_gradient_accum, model.denom = accum0.clone(), denom0.clone()
    points = torch.zeros(P, 3, device=DEV, requires_grad=True)
    points.grad = grad
    densify.add_densification_stats(model, points, filt.unsqueeze(1))
    f = filt.unsqueeze(1)
    assert prune_ref.same_bits(torch.where(f, 0, model.xyz_gradient_accum), torch.where(f, 0, accum0))
    assert prune_ref.same_bits(model.xyz_gradient_accum, torch.where(f, accum0 + inc, accum0))
    assert prune_ref.same_bits(model.denom, torch.where(f, denom0 + 1, denom0))
    # ... which is what the reference's statement leaves, up to the rounding of its norm
    ref = base_model(min(P, 257))
    ref.xyz_gradient_accum, ref.denom = torch.zeros(P, 1, device=DEV), denom0.clone()
    densify_ref.add_densification_stats(ref, grad, filt)
    assert prune_ref.same_bits(model.denom, ref.denom) and torch.allclose(inc, ref.xyz_gradient_accum, rtol=1e-6, atol=0)


# ---- determinism -----------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bits():
    _need_gpu()
    P, N = SIZES[-1], 3
    split = densify_ref.plan_classes(base_model(P), MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN, N)[2]
    noise = _noise(N * int(split.sum()))
    a, b, c = base_model(P), base_model(P), base_model(P)
    ca = densify.densify_and_prune(a, MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN, N=N, noise=noise)
    cb = densify.densify_and_prune(b, MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN, N=N, noise=noise)
    assert ca == cb
    prune_ref.assert_same_state(a, b, "two runs")
    s = torch.cuda.Stream(device=DEV)  # on a side stream
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        cc = densify.densify_and_prune(c, MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN, N=N, noise=noise)
    s.synchronize()
    assert ca == cc
    prune_ref.assert_same_state(a, c, "a side stream")
