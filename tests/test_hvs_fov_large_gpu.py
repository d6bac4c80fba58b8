"""The fused foveated HVS loss (csrc/hvs_fov.hip) on the GPU where its backward pass cuts texel footprints into row slices, runs
one lane per texel, six pyramid levels or a single orientation: cases S0 .. S6 of tests/golden/ref_hvs_fov_large.npz
(tests/hvs_fov_large_cases.py; tests/test_hvs_fov_large_cpu.py proves on the library's own plan that each reaches what it is
named for, and that the figures below move beyond their allowance when a seam row or a slice is left out).
The yardstick is the float64 restatement (tests/hvs_fov_ref.py), computed once per case. The allowance is tests/hvs_cases.py's
rule, unchanged: 3 x the distance of the reference's OWN float32 run from that yardstick (stored in the fixture), floor 16 eps.
A wrong row at a slice seam is invisible in the image gradient, so the gradient of every chain level, g[k], is read from the
backward workspace at the plan's offset and compared too; the reference exposes no such tensor, so its allowance is 3 x the
float32 RESTATEMENT's own distance on the same quantity (the CPU half pins that restatement to the reference's vectors).
Every measured figure is recorded through tests/parity_report.py (kind "hvs_fov")."""
import numpy as np
import pytest
import torch

import fov3dgs_amd  # noqa: F401
from fov3dgs_amd import _native
from fov3dgs_amd.odak_perception import MetamericLoss, _native_hvs_fov, pack_filters
from tests import hvs_cases as hc
from tests import hvs_fov_cases as fc
from tests import hvs_fov_large_cases as lc
from tests import parity_report

pytestmark = pytest.mark.gpu
CASES = list(range(7))
DEV = "cuda:0"
S = lc.STRIDE


def _case(i):
    c = lc.case(i)
    assert c.crc == int(lc.golden()[f"crc_{i}"]), f"{c.name}: the pictures drawn from (seed {c.seed}, amplitude {c.amp}) are not the generator's"
    return c


def _loss_fn(c):
    return MetamericLoss(device=DEV, alpha=c.alpha, real_image_width=c.width, real_viewing_distance=c.distance,
                         n_pyramid_levels=c.levels, mode=c.mode, n_orientations=c.orientations, use_l2_foveal_loss=False,
                         loss_type=c.loss_type, use_bilinear_downup=True, filters=lc.filters_of(c))


def _run(fn, c, tgt=None):
    img = torch.tensor(c.img, device=DEV).requires_grad_(True)
    tgt = torch.tensor(c.tgt, device=DEV) if tgt is None else tgt
    loss = fn(img, tgt, gaze=list(c.gaze), image_colorspace=c.colorspace, resize="pyramid" if c.Hs else None)
    loss.backward()
    return loss.detach(), img.grad


@pytest.mark.parametrize("i", CASES)
def test_loss_and_gradient_match_the_float64_restatement(i):
    c, z, y = _case(i), lc.golden(), lc.yardstick(i)
    loss, grad = _run(_loss_fn(c), c)
    assert loss.dim() == 0 and grad.shape == (1, 3, c.Hs or c.H, c.Ws or c.W)
    grad = grad.cpu().numpy()
    ref_rel, ref_l2, ref_mx = (float(v) for v in z[f"refdist_{i}"])
    rel = abs(float(loss) - y["loss"]) / y["loss"]
    l2, mx = hc.distances(grad, y["grad"])
    parity_report.record("hvs_fov", c.name, rel_loss=rel, ref_rel_loss=ref_rel, grad_rel_l2=l2, ref_grad_rel_l2=ref_l2,
                         grad_max_over_max=mx, ref_grad_max_over_max=ref_mx)
    print(f"{c.name}: rel loss {rel:.3e} (reference {ref_rel:.3e}) grad rel L2 {l2:.3e} (reference {ref_l2:.3e}) "
          f"max/max {mx:.3e} (reference {ref_mx:.3e})")
    assert np.isfinite(grad).all()
    assert rel <= hc.allowance(ref_rel), (rel, ref_rel)
    assert l2 <= hc.allowance(ref_l2), (l2, ref_l2)
    assert mx <= hc.allowance(ref_mx), (mx, ref_mx)


@pytest.mark.parametrize("i", CASES)
def test_lod_maps_match_the_stored_ones(i):
    """the maps the kernels build against the yardstick on the stored stride, within the rule's allowance of the reference's own
    float32 maps there"""
    c, z, y = _case(i), lc.golden(), lc.yardstick(i)
    got = _loss_fn(c).lod_maps(c.H, c.W, gaze=list(c.gaze))
    assert len(got) == c.levels - 1
    for l, m in enumerate(got):
        assert m.dtype == torch.float64 and tuple(m.shape) == (c.H >> l, c.W >> l)
        want = y["lods"][l][::S, ::S]
        ref_d, d = fc.max_abs(z[f"lod_{i}_{l}"], want), fc.max_abs(m.cpu().numpy()[::S, ::S], want)
        parity_report.record("hvs_fov", f"{c.name}/lod{l}", max_abs=d, ref_max_abs=ref_d)
        print(f"{c.name} level {l}: LOD map max |d| {d:.3e} (reference {ref_d:.3e})")
        assert d <= hc.allowance(ref_d), (l, d, ref_d)


def _direct(c):
    """fr_hvs_fov_forward and fr_hvs_fov_backward called directly, the backward workspace and the gradient filled with NaN
    before the call -> (loss, gradient [1,3,H,W], workspace), device tensors"""
    lib = _native.load()
    st = _native_hvs_fov.Settings(c.H, c.W, c.alpha, c.width, c.distance, 1 if c.mode == "quadratic" else 0, c.gaze[0], c.gaze[1], c.levels,
                                  c.orientations, 1 if c.loss_type == "MSE" else 0, 1 if c.colorspace == "RGB" else 0)
    head = (0, 0, c.H, c.W, st.alpha, st.width, st.distance, st.mode, st.gaze_x, st.gaze_y, st.levels, st.orientations, st.mse, st.rgb)
    filters = pack_filters(lc.filters_of(c), c.orientations).to(DEV)
    img, tgt = torch.tensor(c.img[0], device=DEV).contiguous(), torch.tensor(c.tgt[0], device=DEV).contiguous()
    new = lambda n, dt=torch.float32: torch.full((n,), float("nan"), dtype=dt, device=DEV)
    state_i, state_t = new(_native_hvs_fov.floats(st, 0)), new(_native_hvs_fov.floats(st, 0))
    lod, partials, out = new(_native_hvs_fov.floats(st, 3) // 2, torch.float64), new(_native_hvs_fov.floats(st, 2)), new(1)
    work, grad, one = new(_native_hvs_fov.floats(st, 1)), new(3 * c.H * c.W), torch.ones(1, device=DEV)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    with torch.cuda.device(DEV):
        rc = lib.fr_hvs_fov_forward(*head, filters.data_ptr(), img.data_ptr(), tgt.data_ptr(), state_i.data_ptr(), state_t.data_ptr(),
                                    lod.data_ptr(), 0, partials.data_ptr(), out.data_ptr(), stream)
        assert rc == 0, _native.last_error()
        rc = lib.fr_hvs_fov_backward(*head, filters.data_ptr(), state_i.data_ptr(), state_t.data_ptr(), lod.data_ptr(), work.data_ptr(),
                                     one.data_ptr(), grad.data_ptr(), stream)
        assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    return out[0], grad.reshape(1, 3, c.H, c.W), work


@pytest.mark.parametrize("i", [0, 1, 2, 3, 4, 5])
def test_chain_level_gradients_match_the_float64_restatement(i):
    c, y, y32 = _case(i), lc.yardstick(i), lc.float32_restatement(i)
    loss, grad, work = _direct(c)
    want_loss, want_grad = _run(_loss_fn(c), c)
    assert bool(torch.isfinite(grad).all()) and torch.equal(loss, want_loss) and torch.equal(grad, want_grad)
    work = work.cpu().numpy()
    worst = [0.0, 0.0]
    for l, k, p in lc.chain_levels(c):
        nmc = 3 * (c.orientations + (1 if l == 0 else 0))
        got = work[p.g:p.g + 2 * nmc * p.h * p.w].reshape(2, nmc, p.h, p.w)
        part = work[p.gpart:p.gpart + p.S * 2 * nmc * p.h * p.w]
        want = y["chain"][(l, k)]
        assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(part).all(), (l, k)
        if np.floor(y["lods"][l].max()) + 1 < k:    # no pixel blends level k: every slice wrote zeros
            assert not want.any() and not got.any() and not part.any(), (l, k)
            parity_report.record("hvs_fov", f"{c.name}/level{l}/g{k}", unused=1, slices=p.S, lanes=p.G)
            continue
        ref_l2, ref_mx = hc.distances(y32["chain"][(l, k)], want)
        l2, mx = hc.distances(got, want)
        worst = [max(worst[0], l2 / hc.allowance(ref_l2)), max(worst[1], mx / hc.allowance(ref_mx))]
        parity_report.record("hvs_fov", f"{c.name}/level{l}/g{k}", rel_l2=l2, restatement32_rel_l2=ref_l2, max_over_max=mx,
                             restatement32_max_over_max=ref_mx, slices=p.S, lanes=p.G)
        print(f"{c.name} level {l} g[{k}] ({p.h}x{p.w}, S {p.S}, G {p.G}): rel L2 {l2:.3e} (float32 restatement {ref_l2:.3e}) "
              f"max/max {mx:.3e} ({ref_mx:.3e})")
        assert l2 <= hc.allowance(ref_l2), (l, k, l2, ref_l2)
        assert mx <= hc.allowance(ref_mx), (l, k, mx, ref_mx)
    print(f"{c.name}: largest share of an allowance used by a chain gradient: rel L2 {worst[0]:.3f} max/max {worst[1]:.3f}")
    if i == 3:   # HVSLoss's defaults: every sliced level is unused
        assert all(np.floor(y["lods"][l].max()) + 1 < k for l, k, p in lc.chain_levels(c) if p.S > 1)


def test_two_calls_are_bit_identical():
    c = _case(2)
    a, b = _direct(c), _direct(c)
    assert all(torch.equal(u, v) for u, v in zip(a[:2], b[:2]))
    for l, k, p in lc.chain_levels(c):   # ... and so is every chain level's gradient
        n = 2 * 3 * (c.orientations + (1 if l == 0 else 0)) * p.h * p.w
        assert torch.equal(a[2][p.g:p.g + n], b[2][p.g:p.g + n])


def test_kept_target_and_lod_maps_never_decide_a_result():
    c = _case(1)
    fn = _loss_fn(c)
    tgt = torch.tensor(c.tgt, device=DEV)
    first = _run(fn, c, tgt)
    assert fn._target is not None and fn._target[0]() is tgt and fn._lod[3]
    state, lod = fn._target[2], fn._lod[2]
    again = _run(fn, c, tgt)                        # the same object, unchanged, the same gaze: nothing is recomputed ...
    assert fn._target[2] is state and fn._lod[2] is lod
    fresh = _run(_loss_fn(c), c, tgt.clone())       # ... and the result is a fresh object's
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert torch.equal(first[0], fresh[0]) and torch.equal(first[1], fresh[1])
