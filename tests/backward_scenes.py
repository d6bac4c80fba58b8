"""Named, seeded scenes for the backward pass, each with a CENSUS of which rows reach which branch, and the comparison the
CPU half (tests/test_backward_scenes_cpu.py) and the GPU half (tests/test_backward_branches_gpu.py) both judge with.

Why: tests/helpers.small_case adds 1.0 to every raw opacity, and at 200 x 120 its blend stops after the first few splats of a
tile: 67 of its 3000 Gaussians carry a gradient (14 with scale_modifier 2.5), so a branch of csrc/backward.hip that a few dozen
rows take is judged on next to none of them. The scenes here are small_cloud(3000, seed 3) with the opacities x 0.1 (every list
is consumed: thousands of live rows) under cameras that put many rows into each branch:

  open            small_camera() 200 x 120, tilted          -> clamped colour channels, the tilted transpose of dL_dmean3D
  open-x2.5/-x0.4 the same with scale_modifier 2.5 / 0.4    -> the factor in the recomputed covariance and in dL_dscale
  close-wide      eye (0.4, -0.3, 2.5), fovx 50, 200 x 120  -> clamped y (and x) tangents
  close-tall      the same eye, 120 x 200                   -> clamped x tangents
  close-square    eye (0, 0, 3), fovx 40, 136 x 136         -> clamped x and y tangents, both at once
  close-wide-x2.5/-x0.4                                     -> both factors on a close camera
  open-original, close-wide-original                        -> the `original` variant (no -4.5 cutoff, other rectangles)
  short-1/2/3/5   P = 1, 2, 3, 5 large splats of scene_1k   -> the short-list tails of the FULL k_render_bwd fold

A LIVE row is one with dL_dopacity != 0. The census conditions (at least 900 live rows, at least 40 live rows in every branch a
scene claims, ten times as many as the tolerance lets be wrong) are asserted by the CPU half; they are conditions, not
measurements. A plain module: not a conftest, nothing here is collected."""
import functools
import math

import numpy as np

from oracle import oracle as orc
from tests import parity_report
from tests.checks import GRAD_COSINE, GRAD_REL_L2, _where, check_against_noise, check_grad, grad_stats
from tests.helpers import cam_dict, scene_dict, small_camera, small_cloud, syn

TENSORS = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")
SH_C0 = 0.28209479177387814
MIN_LIVE = 900       # live rows every census scene must have
MIN_BRANCH = 40      # live rows in every branch a scene claims
ABS_ROWS = 3.5       # rows a tensor of about a thousand rows may hold outside rtol whatever the fraction says (check_grad's 3.5 / rows)
FACTOR = 1.5         # the project's margin over the reference arithmetic's own share (tests/checks.py check_against_noise)
FLOOR = 1e-4
TAIL_FLOOR = 0.5e-4  # half of rtol: all but 1 % (+ ABS_ROWS) of the rows lie within max(2 x the reference's p99, rtol / 2) (check_against_noise)
OPACITY_FACTOR = 0.1

# name -> variant, camera (None: small_camera(); else eye, fovx in degrees, width, height), background, scale_modifier and the
# branches the scene CLAIMS (census(...)[branch] is its mask of live rows)
SCENES = {
    "open": dict(variant="pcheck_obb_sum", camera=None, bg=(0.1, 0.2, 0.3), scale_modifier=1.0, branches=("colour_clamped",)),
    "open-x2.5": dict(variant="pcheck_obb_sum", camera=None, bg=(0.1, 0.2, 0.3), scale_modifier=2.5, branches=("colour_clamped", "scale_modifier")),
    "open-x0.4": dict(variant="pcheck_obb_sum", camera=None, bg=(0.1, 0.2, 0.3), scale_modifier=0.4, branches=("colour_clamped", "scale_modifier")),
    "close-wide": dict(variant="pcheck_obb_sum", camera=((0.4, -0.3, 2.5), 50.0, 200, 120), bg=(0.3, 0.1, 0.6), scale_modifier=1.0,
                       branches=("clamp_x", "clamp_y", "colour_clamped")),
    "close-tall": dict(variant="pcheck_obb_sum", camera=((0.4, -0.3, 2.5), 50.0, 120, 200), bg=(0.3, 0.1, 0.6), scale_modifier=1.0,
                       branches=("clamp_x", "colour_clamped")),
    "close-square": dict(variant="pcheck_obb_sum", camera=((0.0, 0.0, 3.0), 40.0, 136, 136), bg=(0.3, 0.1, 0.6), scale_modifier=1.0,
                         branches=("clamp_x", "clamp_y", "clamp_both", "colour_clamped")),
    "close-wide-x2.5": dict(variant="pcheck_obb_sum", camera=((0.4, -0.3, 2.5), 50.0, 200, 120), bg=(0.3, 0.1, 0.6), scale_modifier=2.5,
                            branches=("clamp_x", "clamp_y", "scale_modifier")),
    "close-wide-x0.4": dict(variant="pcheck_obb_sum", camera=((0.4, -0.3, 2.5), 50.0, 200, 120), bg=(0.3, 0.1, 0.6), scale_modifier=0.4,
                            branches=("scale_modifier",)),
    "open-original": dict(variant="original", camera=None, bg=(0.1, 0.2, 0.3), scale_modifier=1.0, branches=("colour_clamped",)),
    "open-original-x2.5": dict(variant="original", camera=None, bg=(0.1, 0.2, 0.3), scale_modifier=2.5, branches=("colour_clamped", "scale_modifier")),
    "close-wide-original": dict(variant="original", camera=((0.4, -0.3, 2.5), 50.0, 200, 120), bg=(0.3, 0.1, 0.6), scale_modifier=1.0,
                                branches=("clamp_x", "clamp_y", "colour_clamped")),
}
# Per-(scene, tensor) exceptions to the factor 1.5 (the rule: where a tensor needs more, measure both shares on the GPU, factor =
# measured ratio x 1.25, named in the test's docstring). One: close-tall dL_dopacity, 5 rows of the library's outside 1e-4 of the
# double-precision result in each of 13 runs on an MI355X against 2 of the fp32 oracle's (2.15e-3 / 8.61e-4 of 2324 rows, equal p99
# 2.3e-5 / 2.5e-5): ratio 2.5 -> 3.125, i.e. 9 rows allowed with ABS_ROWS where 1.5 would allow 6 -- one row above what was
# measured, and counts elsewhere moved by up to two rows between runs. Every other comparison stayed two rows or more below its
# limit at 1.5 in each of eight runs.
# (The fp32 oracle's own counts move by a row between hosts -- libm's expf -- and every allowance is computed at run time from the
# oracle of the host the test runs on; the counts quoted here and in DESIGN.md are one MI355X host's.)
FACTORS = {"close-tall": {"dL_dopacity": 3.125}}
CLAMP_SCENES = tuple(n for n, s in SCENES.items() if "clamp_x" in s["branches"] or "clamp_y" in s["branches"])
SHORT = (1, 2, 3, 5)


def camera(eye, fovx_deg, width, height):
    """look_at(eye, (0, 0, 4)) with a fovy that matches the aspect ratio, as tests/helpers.small_camera does."""
    fovx = math.radians(fovx_deg)
    fx = width / (2 * math.tan(fovx / 2))
    fovy = 2 * math.atan(height / (2 * fx))
    R, t = syn.look_at(eye, (0.0, 0.0, 4.0))
    return syn.MiniCam(R, t, fovx, fovy, width, height)


def build(name, sh_degree=3):
    """-> (variant, scene, cam): the oracle-style input dicts of the named scene."""
    s = SCENES[name]
    scene = scene_dict(small_cloud(3000, seed=3), s["variant"])
    scene["opacities"] = (scene["opacities"] * OPACITY_FACTOR).astype(np.float32)
    cam = small_camera() if s["camera"] is None else camera(*s["camera"])
    return s["variant"], scene, cam_dict(cam, bg=s["bg"], sh_degree=sh_degree, scale_modifier=s["scale_modifier"])


def build_short(P, variant):
    """P large splats of scene_1k that overlap in front of the identity camera: several tiles hold all P of them."""
    cloud = syn.scene_1k(P=P, seed=40 + P)
    cloud._scaling += 2.3
    cloud._xyz[:, :2] *= 0.3
    scene = scene_dict(cloud, variant)
    scene["opacities"] = np.clip(scene["opacities"], 0.3, 0.7).astype(np.float32)  # (neither skipped by the alpha test nor saturating at once)
    return variant, scene, cam_dict(syn.camera_1k(200, 120), bg=(0.2, 0.1, 0.0))


def loss_gradient(cam, seed=7):
    return np.random.default_rng(seed).normal(size=(3, int(cam["image_height"]), int(cam["image_width"]))).astype(np.float32)


def oracle_gradients(variant, scene, cam, fwd, dpix):
    """-> (g32, g64): the reference's fp32 arithmetic and the same arithmetic in double, both on the fp32 forward's state `fwd`."""
    g32 = orc.backward(variant, scene, cam, fwd, dpix)
    f64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in fwd.items()}
    s64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    g64 = orc.backward(variant, s64, cam, f64, dpix.astype(np.float64), dtype=np.float64)
    return g32, g64


@functools.lru_cache(maxsize=None)
def reference(name, sh_degree=3):
    """The named scene's oracle forward, loss gradient, fp32 / fp64 oracle gradients and census: computed once per session and shared
    (read-only: the arrays are locked)."""
    variant, scene, cam = build(name, sh_degree)
    fwd = orc.forward(variant, scene, cam)
    dpix = loss_gradient(cam)
    g32, g64 = oracle_gradients(variant, scene, cam, fwd, dpix)
    ref = dict(variant=variant, scene=scene, cam=cam, fwd=fwd, dpix=dpix, g32=g32, g64=g64, census=census(scene, cam, fwd, g32))
    for d in (scene, fwd, g32, g64, ref["census"]):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    dpix.setflags(write=False)
    return ref


def tangents(scene, cam):
    """-> (t.x / t.z, t.y / t.z, limx, limy) of every Gaussian, in float32 like forward.cu:82-87 / backward.cu:170-176."""
    vm = np.asarray(cam["viewmatrix"], np.float32).reshape(-1)
    p = np.asarray(scene["means3D"], np.float32)
    t = [p[:, 0] * vm[0 + i] + p[:, 1] * vm[4 + i] + p[:, 2] * vm[8 + i] + vm[12 + i] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return t[0] / t[2], t[1] / t[2], np.float32(1.3) * np.float32(cam["tanfovx"]), np.float32(1.3) * np.float32(cam["tanfovy"])


def census(scene, cam, fwd, grads):
    """Masks over the P rows, from the oracle's forward and backward outputs: which LIVE rows (dL_dopacity != 0) fall into which
    branch of the per-Gaussian backward pass.
      live            dL_dopacity != 0
      clamp_x         live, x tangent clamped (alone or with y)        clamp_y   likewise for y       clamp_both  both at once
      colour_clamped  live, at least one colour channel clamped at zero by the forward pass
      scale_modifier  live (every live row takes the factor) when the camera's scale_modifier is not 1, else empty
    and `channels_clamped` [P, 3]: the clamped channels of the live rows."""
    live = np.asarray(grads["dL_dopacity"]).reshape(-1) != 0
    ux, uy, limx, limy = tangents(scene, cam)
    cx, cy = (ux < -limx) | (ux > limx), (uy < -limy) | (uy > limy)
    clamped = np.asarray(fwd["clamped"]).astype(bool)
    mod = float(cam.get("scale_modifier", 1.0))
    return dict(live=live, clamp_x=live & cx, clamp_y=live & cy, clamp_both=live & cx & cy, colour_clamped=live & clamped.any(axis=1),
                scale_modifier=live & (mod != 1.0), channels_clamped=clamped & live[:, None])


def counts(cen):
    return {k: int(v.sum()) for k, v in cen.items() if k != "channels_clamped"}


def longest_list(fwd):
    r = np.asarray(fwd["ranges"]).astype(np.int64)
    return int((r[:, 1] - r[:, 0]).max()) if len(r) else 0


def allowed_wrong_rows(ref_share, rows, factor=FACTOR):
    """How many of `rows` live rows the comparison of judge() lets be outside rtol when the reference's own arithmetic leaves
    `ref_share` of them outside: (factor x share + FLOOR) x rows + ABS_ROWS, rounded down."""
    return int(math.floor((factor * ref_share + FLOOR) * rows + ABS_ROWS + 1e-9))


def whole_tensor_judged(f32, f64):
    """The whole-tensor bounds of check_grad (cosine, relative L2) against the fp32 oracle are applied only where the reference's
    own fp32 arithmetic is well inside them against its double-precision self (half of each bound)."""
    b = grad_stats(f32, f64)
    return b["rel_l2"] <= 0.5 * GRAD_REL_L2 and b["one_minus_cosine"] <= 0.5 * GRAD_COSINE


def judge(got, g32, g64, cen, tag, branches=(), min_rows=MIN_LIVE, factors=None, against_f32=True, tensors=TENSORS):
    """THE comparison of the branch tests. `got` (a dict of the eight gradient tensors: the HIP library's, or a doctored copy of the
    oracle's in the CPU half) is held to the reference arithmetic's own noise -- both `got` and the fp32 oracle `g32` against the
    double-precision oracle `g64` on the same forward state, factor 1.5 (`factors`: per-tensor exceptions, measured x 1.25) -- on all
    rows AND on the live rows of every branch in `branches` on their own (a defect confined to 50 rows must not hide in a 3000-row
    fraction); dL_dsh's DC coefficient is exactly 0 on clamped channels; and (against_f32) the tensor as a whole agrees with the
    fp32 oracle within check_grad's default cosine / relative-L2 bounds wherever the reference's own arithmetic does
    (whole_tensor_judged), with at least `min_rows` rows carrying a gradient.
    Allowances (check_against_noise with abs_rows and tail_floor; n = rows with a gradient in the tensor or branch):
      rows outside rtol                                  <= 1.5 x the reference's share x n + 1e-4 n + 3.5 rows
      rows beyond max(2 x the reference's p99, rtol / 2) <= 1 % of n + 3.5 rows
      rows outside 100 x rtol                            <= 1.5 x the reference's share x n + 1e-4 n + 1.5 rows
    The 3.5 rows are BESIDE the fractions, not instead of them: k_render_bwd sums with float atomics, whose order moves a row
    across a threshold from run to run, and with two to nine rows of the reference's own outside rtol a bound without rows of
    headroom fails one run in a few. The tail clause counts rows instead of comparing 99th percentiles because on 44 to 963 rows
    that percentile is the largest to tenth-largest value (measured: 2.0-3.9 x the reference's on the branches, 0.72-0.90 of the
    2 x limit from run to run on close-square's dL_dopacity); its floor of rtol / 2 says what the clause guards: a systematic error
    below rtol in a branch puts ALL of its rows beyond the threshold."""
    factors = factors or {}
    for k in tensors:
        g = np.asarray(got[k]).reshape(np.shape(g64[k]))
        assert np.isfinite(g).all(), f"{tag} {k}"
        check_against_noise(g, g32[k], g64[k], f"{tag} {k}", factor=factors.get(k, FACTOR), floor=FLOOR, abs_rows=ABS_ROWS, tail_floor=TAIL_FLOOR)
        for br in branches:
            sel = cen[br]
            check_against_noise(g[sel], g32[k][sel], g64[k][sel], f"{tag} {k} [{br}: {int(sel.sum())} rows]", factor=factors.get(k, FACTOR),
                                floor=FLOOR, abs_rows=ABS_ROWS, tail_floor=TAIL_FLOOR)
        if against_f32:
            whole = whole_tensor_judged(g32[k], g64[k])
            # (the ROWS are judged against the reference's noise above: its own fp32 arithmetic leaves more than GRAD_OUTLIERS of
            # dL_dopacity's rows outside 1e-4 on these scenes, so the fixed row budgets of check_grad cannot apply)
            check_grad(g, g32[k], f"{tag} {k} (whole tensor)", outlier_frac=1.0, cosine=GRAD_COSINE if whole else np.inf,
                       rel_l2=GRAD_REL_L2 if whole else np.inf, min_rows=min_rows)
    if "dL_dsh" in tensors and "channels_clamped" in cen:
        dc = np.asarray(got["dL_dsh"]).reshape(len(cen["live"]), -1, 3)[:, 0]
        assert np.all(dc[cen["channels_clamped"]] == 0.0), f"{tag}: a clamped channel passed a gradient to its DC coefficient"


def record_census(name, cen, fwd, extra=None):
    parity_report.record("census", f"{_where()} {name}", longest_list=longest_list(fwd), num_rendered=int(fwd["num_rendered"]), **counts(cen), **(extra or {}))


def record_flipped_pixels(tag, agree):
    """Records and returns the share of the frame's pixels left out of the loss because their forward state differs between the passes."""
    left_out = 1.0 - float(np.mean(agree))
    parity_report.record("flipped_pixels", f"{_where()} {tag}", share_left_out=left_out, pixels=int(np.size(agree)))
    return left_out
