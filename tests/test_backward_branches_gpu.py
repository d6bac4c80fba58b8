"""The backward pass judged on thousands of rows and on every branch: the GPU half of tests/backward_scenes.py (the scenes, their
census and the comparison; tests/test_backward_scenes_cpu.py asserts the census conditions and proves that the comparison rejects
a defect in every branch).

The small-frame tests of tests/test_gpu_parity.py draw their scene from helpers.small_case, where 67 of 3000 Gaussians carry a
gradient. Here every scene has 900 to 3000 live rows, and every branch of the per-Gaussian pass (csrc/backward.hip) -- a scale
modifier other than 1, a clamped x or y tangent, a colour channel clamped at zero, the tilted camera's transpose -- has at least 40
live rows that are ALSO judged on their own.

Per test: the instance lists equal the oracle's bit for bit; the loss gradient is zero on the pixels whose forward state differs
between the two passes (at most 1e-3 of the frame); all eight gradient tensors are held to the reference arithmetic's own noise
(checks.check_against_noise: the HIP gradients and the fp32 oracle both against the double-precision oracle on the same forward
state, factor 1.5 with 3.5 rows beside it for these thousand-row tensors, a tail and a gross clause: backward_scenes.judge) and, where the reference's own arithmetic is inside them, to
check_grad's whole-tensor bounds against the fp32 oracle; dL_dsh's DC coefficient is exactly zero on clamped channels. Every
comparison's measured shares (HIP vs double, fp32 oracle vs double) are kept in the parity report. Every gradient tensor starts as
NaN (tests/conftest.py)."""
import numpy as np
import pytest
import torch

from tests import backward_scenes as bs
from tests.checks import check_grad, grad_stats
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

MAX_FLIPPED = 1e-3  # share of the frame's pixels left out of the loss because their forward state differs between the two passes


def _need_gpu():
    if not torch.cuda.is_available():  # only reached by an explicit -m gpu run (tests/conftest.py skips otherwise)
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _both_passes(variant, scene, cam, tag, ref=None, hip_scene=None, raw=False):
    """HIP forward + backward and the oracle's fp32 / fp64 gradients for one loss gradient, which is zero on the pixels whose forward
    state differs between the two passes. ref: a cached backward_scenes.reference() of (variant, scene, cam) -- used as it is when
    no pixel differs. hip_scene: what the library is given when that is not `scene` (the raw parameters).
    -> (got, g32, g64, census, oracle forward)"""
    from tests.gpu_helpers import hip_backward, hip_forward
    want_f = ref["fwd"] if ref is not None else orc.forward(variant, scene, cam)
    got_f = hip_forward(variant, scene if hip_scene is None else hip_scene, cam, raw=raw)
    # the lists, before anything else is judged
    assert got_f["num_rendered"] == want_f["num_rendered"]
    np.testing.assert_array_equal(got_f["radii"], want_f["radii"])
    np.testing.assert_array_equal(got_f["ranges"], want_f["ranges"])
    np.testing.assert_array_equal(got_f["point_list"], want_f["point_list"])
    agree = (got_f["n_contrib"] == want_f["n_contrib"]) & ~(np.abs(got_f["final_T"] - want_f["final_T"]) > 1e-5 * np.abs(want_f["final_T"]) + 1e-9)
    left_out = bs.record_flipped_pixels(tag, agree)
    print(f"{tag}: {int((~agree).sum())} of {agree.size} pixels left out of the loss")
    assert left_out <= MAX_FLIPPED
    dpix = bs.loss_gradient(cam)
    if ref is not None and agree.all():
        g32, g64, cen = ref["g32"], ref["g64"], ref["census"]
    else:
        dpix = dpix * agree[None].astype(np.float32)
        g32, g64 = bs.oracle_gradients(variant, scene, cam, want_f, dpix)
        cen = bs.census(scene, cam, want_f, g32)
    got = hip_backward(variant, got_f, dpix)
    return got, g32, g64, cen, want_f


FACTORS = bs.FACTORS  # per-tensor exceptions to the factor 1.5, with their measurements (tests/backward_scenes.py)


@pytest.mark.parametrize("name", tuple(bs.SCENES))
def test_every_branch_on_its_own_rows(name):
    """All eight tensors on every scene of tests/backward_scenes.py, the whole tensor and the live rows of every branch the scene
    claims on their own: scale_modifier 2.5 and 0.4 (open-x*, close-wide-x*, open-original-x2.5), clamped x / y / both tangents
    (close-*), clamped colour channels, both training variants.
    Factor over the reference's own share: 1.5, except dL_dopacity on close-tall (3.125 = measured 5 rows against the reference's
    2, x 1.25) -- backward_scenes.FACTORS has the measurement."""
    _need_gpu()
    ref = bs.reference(name)
    got, g32, g64, cen, _ = _both_passes(ref["variant"], ref["scene"], ref["cam"], name, ref=ref)
    bs.record_census(name, cen, ref["fwd"])
    branches = bs.SCENES[name]["branches"]
    for br in branches:
        assert int(cen[br].sum()) >= bs.MIN_BRANCH, br
    bs.judge(got, g32, g64, cen, name, branches=branches, factors=FACTORS.get(name))


@pytest.mark.parametrize("sh_degree", (0, 1, 2))
def test_open_scene_at_lower_sh_degrees(sh_degree):
    """The open scene with the active SH degree below the allocated one: the coefficients beyond it get exactly zero."""
    _need_gpu()
    ref = bs.reference("open", sh_degree)
    tag = f"open degree {sh_degree}"
    got, g32, g64, cen, _ = _both_passes(ref["variant"], ref["scene"], ref["cam"], tag, ref=ref)
    assert int(cen["colour_clamped"].sum()) >= bs.MIN_BRANCH
    bs.judge(got, g32, g64, cen, tag, branches=("colour_clamped",), factors=FACTORS.get(tag))
    used = (sh_degree + 1) ** 2
    assert np.all(got["dL_dsh"].reshape(-1, 16, 3)[:, used:] == 0.0)
    assert np.abs(got["dL_dsh"].reshape(-1, 16, 3)[:, used - 1]).max() > 0


def test_open_scene_with_precomputed_colours_and_covariances():
    """colors_precomp + cov3D_precomp: dL_dcolor / dL_dcov3D are the inputs' gradients, the tensors of the absent inputs are zero."""
    _need_gpu()
    ref = bs.reference("open")
    pre = dict(ref["scene"])
    pre["colors_precomp"] = np.random.default_rng(3).random((len(pre["means3D"]), 3)).astype(np.float32)
    pre["cov3D_precomp"] = np.array(ref["fwd"]["cov3D"])
    for k in ("shs", "scales", "rotations"):
        pre.pop(k)
    got, g32, g64, cen, _ = _both_passes(ref["variant"], pre, ref["cam"], "open precomputed")
    assert int(cen["live"].sum()) >= bs.MIN_LIVE
    bs.judge(got, g32, g64, cen, "open precomputed", tensors=("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D"))
    for k in ("dL_dsh", "dL_dscale", "dL_drot"):
        assert got[k].size == 0 or not np.abs(got[k]).any(), k  # (NaN != 0: unwritten elements fail here too)
        assert np.isfinite(got[k]).all(), k


def test_open_scene_from_raw_parameters():
    """raw_activations: the kernels apply exp / normalize / sigmoid and return the gradients with respect to the RAW parameters.
    Judged against the chain rule applied in the test, in float64, to the oracle's gradients (fp32 and double) with respect to the
    activated values -- the activated values themselves are the library's own (activations.activate: the kernels' expressions), so
    that both passes see one forward state."""
    _need_gpu()
    from fov3dgs_amd.activations import activate
    from tests.helpers import small_cloud
    ref = bs.reference("open")
    cloud = small_cloud(3000, seed=3)
    o64 = bs.OPACITY_FACTOR / (1.0 + np.exp(-cloud._opacity.double().numpy()))  # the open scene's opacities: 0.1 sigmoid(raw)
    raw = dict(scales=cloud._scaling.numpy().astype(np.float32), rotations=cloud._rotation.numpy().astype(np.float32),
               opacities=np.log(o64 / (1.0 - o64)).astype(np.float32))
    with torch.no_grad():
        s, q, o = activate(*(torch.from_numpy(raw[k]).to("cuda:0") for k in ("scales", "rotations", "opacities")))
    scene = dict(ref["scene"], scales=s.cpu().numpy(), rotations=q.cpu().numpy(), opacities=o.cpu().numpy())
    np.testing.assert_allclose(scene["opacities"], ref["scene"]["opacities"], rtol=1e-5)  # (the open scene, to the activations' rounding)
    got, g32, g64, cen, _ = _both_passes(ref["variant"], scene, ref["cam"], "open raw", hip_scene=dict(scene, **raw), raw=True)
    assert int(cen["live"].sum()) >= bs.MIN_LIVE
    # the activations' derivatives in float64, from the raw values
    r64 = {k: v.astype(np.float64) for k, v in raw.items()}
    sig = 1.0 / (1.0 + np.exp(-r64["opacities"]))
    norm = np.linalg.norm(r64["rotations"], axis=1, keepdims=True)
    unit = r64["rotations"] / norm

    def chain(g):
        g = {k: np.asarray(v, np.float64) for k, v in g.items()}
        g["dL_dopacity"] = g["dL_dopacity"] * sig * (1.0 - sig)
        g["dL_dscale"] = g["dL_dscale"] * np.exp(r64["scales"])
        g["dL_drot"] = (g["dL_drot"] - unit * (unit * g["dL_drot"]).sum(axis=1, keepdims=True)) / norm
        return g
    bs.judge(got, chain(g32), chain(g64), cen, "open raw", branches=("colour_clamped",))


@pytest.mark.parametrize("variant", ("original", "pcheck_obb_sum"))
@pytest.mark.parametrize("P", bs.SHORT)
def test_short_lists_take_every_tail_of_the_full_fold(P, variant):
    """Lists of 1, 2, 3 and 5 entries through the FULL k_render_bwd (tests/test_appearance_backward_gpu.py covers the lean
    instantiation): the fold ends with one entry pending or none, after zero, one or two full folds. Judged against the
    DOUBLE-precision oracle, EVERY row within 1e-4 relative -- no outlier share: the rows outside 1e-4 of the large scenes are sums
    over long lists whose terms cancel and neighbours of flipped pairs; here a row sums at most a few hundred pixels of at most
    five entries and flipped pixels are out of the loss (the reference's own fp32 arithmetic is within 7.4e-6 of the double result
    on every row of these scenes) -- and a fold that dropped or doubled an entry is off by the entry."""
    _need_gpu()
    _, scene, cam = bs.build_short(P, variant)
    tag = f"P={P} {variant}"
    got, g32, g64, cen, want_f = _both_passes(variant, scene, cam, tag)
    n = want_f["ranges"][:, 1].astype(int) - want_f["ranges"][:, 0].astype(int)
    assert n.max() == P and (n == P).sum() >= 4 and cen["live"].all()
    for k in bs.TENSORS:
        g = got[k].reshape(g64[k].shape)
        st = grad_stats(g, g64[k])
        print(f"{tag} {k}: worst row {st['row_rel_max']:.2e} (fp32 oracle: {grad_stats(g32[k], g64[k])['row_rel_max']:.2e})")
        check_grad(g, g64[k], f"{tag} {k} vs the double-precision oracle", min_rows=P)
        assert st["frac_bad"] == 0.0, f"{tag} {k}: a row is {st['row_rel_max']:.2e} off the double-precision gradient"
