"""The CPU half of the backward-branch tests (tests/backward_scenes.py; the GPU half is tests/test_backward_branches_gpu.py).

For every scene: the CENSUS CONDITIONS (enough live rows in every branch the scene claims -- conditions, not measurements), the
reference arithmetic's own noise (fp32 oracle backward against the double-precision one on the same forward state: recorded through
tests/parity_report.py, asserted only against a loose sanity bound), and proof that the comparison the GPU half uses REJECTS a
defect in every branch: the fp32 oracle gradients with one defect injected must fail judge(), the untouched ones must pass.

Measured here (small_cloud(3000, seed 3), opacities x 0.1; live = rows with dL_dopacity != 0; clamp x / clamp y / both; rows with a
colour channel clamped at zero; longest tile list; instances):
  open                 2970 live    9 /  17 /  5   431   792  D 18 855
  open-x2.5            2222        13 /  21 /  8   306  1569    43 142
  open-x0.4            2958         2 /   8 /  1   430   453     8 477
  close-wide           1560        52 / 143 / 23   223   374    31 950
  close-tall           2324        77 /  17 /  6   331   464    30 736
  close-square          963       116 / 113 / 44   142   308    22 783
  close-wide-x2.5      1264       229 / 460 / 96   164  1009    91 375
  close-wide-x0.4      1242        10 /  38 /  7   180   141    10 721
  open-original        2970         9 /  17 /  5   431   922    26 708
  open-original-x2.5   2222        13 /  21 /  8   306  1936    56 470
  close-wide-original  1560        52 / 143 / 23   223   501    45 319
Share of the rows outside 1e-4 relative, fp32 oracle vs fp64 oracle (grad_stats): dL_dopacity 3.7e-3 (open; ABOVE checks.GRAD_OUTLIERS =
3e-3, which is why the GPU half judges against this noise and not against a fixed cap), 3.4e-3 (open-original), 2.6e-3 (close-wide);
every other tensor <= 1.8e-3 (dL_dcov3D / dL_dscale on open-x2.5)."""
import numpy as np
import pytest

from tests import backward_scenes as bs
from tests import parity_report
from tests.checks import grad_stats

# Sanity bounds on the reference's own noise (share of live rows outside 1e-4 of the double-precision result): the worst measured
# over the scenes x 2 -- dL_dopacity 3.7e-3 -> 7.4e-3, every other tensor 1.8e-3 -> 3.6e-3. Not a tolerance of the library: a guard
# against a scene change that makes the yardstick itself meaningless.
NOISE_SANITY = {"dL_dopacity": 7.4e-3}
NOISE_SANITY_OTHER = 3.6e-3
# (scene, tensor) whose whole-tensor bounds (cosine, relative L2 against the fp32 oracle) the GPU half does NOT apply, because the
# reference's own fp32 arithmetic is not well inside them: open-x0.4 has one near-camera row of huge, cancelling terms that carries
# the tensor's norm (relative L2 of the fp32 oracle against the double one 9.1e-4, 1 - cosine 4.1e-7).
WHOLE_TENSOR_EXCEPTIONS = {("open-x0.4", "dL_dopacity")}
# Share of ||dL_dmean3D|| carried by the rows with a clamped tangent, measured: close-square 0.39, close-wide 0.25, close-tall 0.13
CLAMPED_NORM_SHARE = ("close-square", 0.2)


@pytest.mark.parametrize("name", tuple(bs.SCENES))
def test_census_conditions(name):
    ref = bs.reference(name)
    cen, spec = ref["census"], bs.SCENES[name]
    n = bs.counts(cen)
    print(name, n, "longest list", bs.longest_list(ref["fwd"]), "instances", ref["fwd"]["num_rendered"])
    bs.record_census(name, cen, ref["fwd"])
    assert n["live"] >= bs.MIN_LIVE
    assert (ref["fwd"]["radii"][cen["live"]] > 0).all()
    if spec["scale_modifier"] != 1.0:
        assert "scale_modifier" in spec["branches"] and n["scale_modifier"] == n["live"]
    for br in spec["branches"]:
        assert n[br] >= bs.MIN_BRANCH, (br, n[br])
        # ten times as many live rows in the branch as the comparison lets be wrong within the branch's rows, tensor by tensor
        sel = cen[br]
        for k in bs.TENSORS:
            share = grad_stats(ref["g32"][k][sel], ref["g64"][k][sel])["frac_bad"]
            wrong = bs.allowed_wrong_rows(share, n[br], factor=bs.FACTORS.get(name, {}).get(k, bs.FACTOR))
            assert n[br] >= 10 * wrong, (br, k, n[br], wrong)


def test_clamped_rows_carry_the_position_gradient():
    """On close-square the rows with a clamped tangent carry 0.39 of ||dL_dmean3D|| (close-wide 0.25, close-tall 0.13): the clamped
    branch is not a corner of negligible rows."""
    name, least = CLAMPED_NORM_SHARE
    ref = bs.reference(name)
    g, cl = ref["g64"]["dL_dmean3D"], ref["census"]["clamp_x"] | ref["census"]["clamp_y"]
    share = float(np.linalg.norm(g[cl]) / np.linalg.norm(g))
    parity_report.record("census", f"{name}: share of |dL_dmean3D| on rows with a clamped tangent", share=share, rows=int(cl.sum()))
    print(name, "clamped rows' share of |dL_dmean3D|:", share)
    assert share >= least


@pytest.mark.parametrize("name", tuple(bs.SCENES))
def test_reference_noise_is_recorded_and_sane(name):
    """fp32 oracle backward vs the double-precision one on the same forward state, per tensor and per claimed branch: recorded, and
    below NOISE_SANITY (the worst measured x 2: dL_dopacity 7.4e-3, other tensors 3.6e-3). Also pins which tensors' whole-tensor
    bounds the GPU half applies (WHOLE_TENSOR_EXCEPTIONS)."""
    ref = bs.reference(name)
    for k in bs.TENSORS:
        st = grad_stats(ref["g32"][k], ref["g64"][k])
        parity_report.record("oracle_noise", f"{name} fp32 vs fp64 oracle backward {k}", **st)
        print(f"{name} {k}: outside 1e-4 {st['frac_bad']:.2e}, relative L2 {st['rel_l2']:.1e}, 1 - cosine {st['one_minus_cosine']:.1e}, rows {st['rows_with_gradient']}")
        assert st["frac_bad"] <= NOISE_SANITY.get(k, NOISE_SANITY_OTHER), (k, st["frac_bad"])
        assert bs.whole_tensor_judged(ref["g32"][k], ref["g64"][k]) == ((name, k) not in WHOLE_TENSOR_EXCEPTIONS), (name, k, st)
        for br in bs.SCENES[name]["branches"]:
            sel = ref["census"][br]
            sb = grad_stats(ref["g32"][k][sel], ref["g64"][k][sel])
            parity_report.record("oracle_noise", f"{name} fp32 vs fp64 oracle backward {k} [{br}]", **sb)


@pytest.mark.parametrize("variant", ("original", "pcheck_obb_sum"))
@pytest.mark.parametrize("P", bs.SHORT)
def test_short_scenes_hold_lists_of_every_length(P, variant):
    _, scene, cam = bs.build_short(P, variant)
    fwd = bs.orc.forward(variant, scene, cam)
    r = fwd["ranges"].astype(np.int64)
    n = r[:, 1] - r[:, 0]
    assert n.max() == P and (n == P).sum() >= 4  # several tiles hold all P splats
    g32, _ = bs.oracle_gradients(variant, scene, cam, fwd, bs.loss_gradient(cam))
    assert (g32["dL_dopacity"] != 0).all()


# ---- the comparison rejects a defect in every branch ---------------------------------------------------------------------------
def _scale_defect(ref, g):
    g["dL_dscale"] = g["dL_dscale"] / np.float32(ref["cam"]["scale_modifier"])  # the factor dropped from (or doubled in) dL_dscale


def _clamp_defect(which):
    def f(ref, g):
        g["dL_dmean3D"][ref["census"][which]] *= np.float32(1.01)  # stands for a tangent gradient that ignores the clamp
    return f


def _colour_defect(ref, g):
    ch = ref["census"]["channels_clamped"]
    g["dL_dsh"][:, 0][ch] = (bs.SH_C0 * g["dL_dcolor"][ch]).astype(np.float32)  # the DC gradient an unclamped channel would get


def _rot_defect(ref, g):
    g["dL_drot"] *= np.float32(1.01)


def _cases():
    out = []
    for name, s in bs.SCENES.items():
        if "scale_modifier" in s["branches"]:
            out.append(pytest.param(name, _scale_defect, "dL_dscale", id=f"{name}-scale"))
        for which in ("clamp_x", "clamp_y", "clamp_both"):
            if which in s["branches"]:
                out.append(pytest.param(name, _clamp_defect(which), "dL_dmean3D", id=f"{name}-{which}"))
        if "colour_clamped" in s["branches"]:
            out.append(pytest.param(name, _colour_defect, "dL_dsh", id=f"{name}-colour"))
        if name.startswith("close"):
            out.append(pytest.param(name, _rot_defect, "dL_drot", id=f"{name}-rot"))
    return out


@pytest.mark.parametrize("name,defect,tensor", _cases())
def test_the_comparison_rejects_a_defect(name, defect, tensor):
    """dL_dscale divided by the scale modifier; dL_dmean3D of the rows with a clamped tangent off by 1 %; a DC gradient on clamped
    colour channels; dL_drot off by 1 % on the close scenes: each fails the ROW comparison against the reference's noise (the
    whole-tensor bounds against the fp32 oracle are left out here: the doctored tensor IS the fp32 oracle's but for the defect)."""
    ref = bs.reference(name)
    branches = bs.SCENES[name]["branches"]
    g = {k: np.array(v) for k, v in ref["g32"].items()}
    defect(ref, g)
    assert not np.array_equal(g[tensor], ref["g32"][tensor])
    with parity_report.muted():  # (doctored inputs: nothing measured here belongs in the report)
        bs.judge(ref["g32"], ref["g32"], ref["g64"], ref["census"], f"{name} untouched", branches=branches)
        with pytest.raises(AssertionError, match=f"{tensor}.*outside"):
            bs.judge(g, ref["g32"], ref["g64"], ref["census"], f"{name} defect", branches=branches, against_f32=False)


def test_a_defect_confined_to_a_branch_is_caught_by_the_branch():
    """52 rows of a 1560-row tensor off by 1 %: 3.3 % of the rows. The branch's own comparison sees all of its rows wrong, also when
    the whole tensor's fraction is not asked (close-wide, the clamp-x rows' dL_dscale)."""
    ref = bs.reference("close-wide")
    g = {k: np.array(v) for k, v in ref["g32"].items()}
    g["dL_dscale"][ref["census"]["clamp_x"]] *= np.float32(1.01)
    with parity_report.muted(), pytest.raises(AssertionError, match=r"dL_dscale \[clamp_x"):
        for k in bs.TENSORS:  # (the branch rows alone)
            sel = ref["census"]["clamp_x"]
            bs.check_against_noise(g[k][sel], ref["g32"][k][sel], ref["g64"][k][sel], f"{k} [clamp_x", floor=bs.FLOOR, abs_rows=bs.ABS_ROWS)


def test_a_gradient_on_a_clamped_channel_is_not_exactly_zero():
    """A DC gradient of 1e-30 on the clamped channels is inside every relative tolerance: the exact-zero assertion catches it."""
    ref = bs.reference("open")
    g = {k: np.array(v) for k, v in ref["g32"].items()}
    g["dL_dsh"][:, 0][ref["census"]["channels_clamped"]] = np.float32(1e-30)
    with parity_report.muted(), pytest.raises(AssertionError, match="clamped channel"):
        bs.judge(g, ref["g32"], ref["g64"], ref["census"], "open 1e-30", branches=("colour_clamped",), against_f32=False)


def test_min_rows_guard():
    from tests.checks import check_grad
    ref = bs.reference("open")
    check_grad(ref["g32"]["dL_dopacity"], ref["g32"]["dL_dopacity"], "guard", min_rows=2970)
    with pytest.raises(AssertionError, match="rows carry a gradient"):
        check_grad(ref["g32"]["dL_dopacity"], ref["g32"]["dL_dopacity"], "guard", min_rows=2971)
