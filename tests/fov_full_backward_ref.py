"""Reference, scenes and comparison of the foveated renderer's FULL backward pass (k_render_bwd_fov_full / k_fov_full_bwd,
fr_backward_fov): the gradients of means3D, scales, rotations, the rest SH coefficients, the viewspace points and the per-level
opacities / DC colours through the forward pass of the foveated renderer.

The reference is INDEPENDENT of the hand-derived moment formulas of csrc/backward.hip: torch.autograd through a frozen-decision
restatement of the foveated forward, in float64 (the reference) and in float32 (the same arithmetic on the same decisions, for
checks.check_against_noise):

  * decisions, lists, tile levels and `est` come from the forward dict exactly as tests/fov_backward_ref.FovBackwardRef takes them
    (its tiles: which (pixel, state, Gaussian) pairs are blended, which state-1 pixels start finished, the states' shares w1 / 1 - w1
    as CONSTANTS: float32 as the forward forms them, or the same expression in double);
  * projection, covariance, conic and SH colour are the expressions of tests/torch_rasterizer.py (restated in project() because
    rasterize() does not hand out its intermediates; sh_colour is imported), with detach_clamped_tangents=True: the reference's
    convention for a clamped tangent;
  * the saturation is straight-through: alpha = o G + (min(0.99, o G) - o G).detach() (backward.cu:497-541 does not differentiate
    the min);
  * per state and pixel: value = sum_j alpha_j T_j c_j + T_end bg with T_j = prod_{i<j} (1 - alpha_i) over the blended pairs.

Two stages, so that a frame of 20 000 Gaussians stays small: the per-Gaussian quantities (pixel position, conic, level colours,
opacities) are leaves of the tile stage, whose gradients are accumulated tile by tile; then one backward from them to the model.
dL_dlevel_colours (the gradient of the clamped level colour) and dL_dmeans2D (the gradient of the pixel position times (W/2, H/2),
third component 0: what the plain backward returns and densify.add_densification_stats reads) fall out of the first stage.

A LIVE Gaussian has a non-zero dL_dopacities row in the float64 reference. A plain module: not a conftest, nothing here is collected."""
import functools

import numpy as np
import torch

from tests import backward_scenes as bs
from tests import fov_backward_ref as R
from tests import fov_backward_scenes as fs
from tests import parity_report
from tests.checks import _where, check_grad, grad_stats
from tests.helpers import cam_dict, scene_dict, small_cloud, syn
from tests.torch_rasterizer import sh_colour

GEOMETRY = ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dshs_rest", "dL_dmeans2D")   # one row per Gaussian
LEVELLED = fs.TENSORS                                                                       # one row per (Gaussian, level)
MIN_LIVE, MIN_BRANCH = bs.MIN_LIVE, bs.MIN_BRANCH
SHORT_RTOL = fs.SHORT_RTOL
# two derivations of one number in float64 (FovBackwardRef's hand-written sums, autograd's tile stage here, both fed with the forward's
# float32 positions / conics / colours): they differ by the order of the sums only. The bound is relative to the tensor's largest
# entry; the observed agreement is printed by the CPU half and recorded in DESIGN.md.
F64_AGREEMENT = 1e-12
# Per-(scene, tensor) exceptions to the factor 1.5 (the rule of tests/backward_scenes.py: where a tensor needs more, measure both
# shares on the GPU, factor = measured ratio x 1.25, named with its measurement here and in DESIGN.md). None so far.
FACTORS = {}

# name -> the branches (census masks over the P Gaussians) judged on their own rows, each with >= MIN_BRANCH live rows
LARGE = {
    "faint": ("two_level", "colour_clamped"),
    "deep": ("two_level", "colour_clamped"),
    "faint-L2": ("two_level",),
    "close-wide-x2.5-fov": ("clamp_x", "clamp_y", "clamp_both", "scale_modifier"),
}
TINY = ("tiny-17x15", "tiny-8x8", "tiny-15x1")
SHORT_NAMES = fs.SHORT_NAMES
NOTHING = fs.NOTHING
DEGREES = (0, 1, 2)


def build(name, sh_degree=3):
    """-> (scene, cam, settings), as fov_backward_scenes.build; close-wide-x2.5-fov: small_cloud(3000, 3) with foveation_layers(seed 4),
    opacities x 0.1, under backward_scenes' close camera with scale_modifier 2.5 (clamped tangents of both kinds, the factor)."""
    if name == "close-wide-x2.5-fov":
        cloud = small_cloud(3000, 3)
        scene = fs._faint(scene_dict(cloud, fs.VARIANT, syn.foveation_layers(cloud, seed=4)))
        cam = cam_dict(bs.camera((0.4, -0.3, 2.5), 50.0, 200, 120), bg=R.BG, gaze=(0.4, 0.55), alpha=0.6, scale_modifier=2.5)
        return scene, cam, None
    scene, cam, settings = fs.build(name)
    if sh_degree != 3:
        cam = dict(cam, sh_degree=sh_degree)
    return scene, cam, settings


def project(means3D, scales, rotations, cam):
    """tests/torch_rasterizer.rasterize's projection (forward.cu:74-262, auxiliary.h:41-44) with detach_clamped_tangents=True
    -> pixel position [P,2] and conic [P,3] in the dtype of the inputs. Rows the frame does not list are never used."""
    F = means3D.dtype
    W, H = int(cam["image_width"]), int(cam["image_height"])
    vm = torch.as_tensor(np.asarray(cam["viewmatrix"], np.float64), dtype=F).reshape(4, 4)
    pm = torch.as_tensor(np.asarray(cam["projmatrix"], np.float64), dtype=F).reshape(4, 4)
    tanx, tany = float(cam["tanfovx"]), float(cam["tanfovy"])
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    mod = float(cam.get("scale_modifier", 1.0))
    P = means3D.shape[0]
    ones = torch.ones(P, 1, dtype=F)
    ph = torch.cat([means3D, ones], 1) @ pm
    pw = 1.0 / (ph[:, 3] + 1e-7)
    proj = ph[:, :3] * pw[:, None]
    t = torch.cat([means3D, ones], 1) @ vm
    tz = t[:, 2]
    r, x, y, z = rotations[:, 0], rotations[:, 1], rotations[:, 2], rotations[:, 3]
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
    Mm = Rm @ torch.diag_embed(mod * scales)
    Sigma = Mm @ Mm.transpose(1, 2)
    limx, limy = 1.3 * tanx, 1.3 * tany
    txc = torch.clamp(t[:, 0] / tz, -limx, limx) * tz
    tyc = torch.clamp(t[:, 1] / tz, -limy, limy) * tz
    with torch.no_grad():
        ux, uy = t[:, 0] / tz, t[:, 1] / tz
        cx, cy = (ux < -limx) | (ux > limx), (uy < -limy) | (uy > limy)
    txc, tyc = torch.where(cx, txc.detach(), txc), torch.where(cy, tyc.detach(), tyc)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * txc) / (tz * tz), zero, fy / tz, -(fy * tyc) / (tz * tz)], 1).reshape(P, 2, 3)
    Tm = J @ vm[:3, :3].T
    cov = Tm @ Sigma @ Tm.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c - b * b
    det_s = torch.where(det != 0, det, torch.ones_like(det))
    conic = torch.stack([c / det_s, -b / det_s, a / det_s], 1)
    pix = torch.stack([((proj[:, 0] + 1.0) * W - 1.0) * 0.5, ((proj[:, 1] + 1.0) * H - 1.0) * 0.5], 1)
    return pix, conic


class FovFullBackwardRef:
    """ref: a FovBackwardRef of the frame (the frozen decisions). image() and backward() in float64 or float32."""

    def __init__(self, ref, scene, cam):
        self.ref, self.scene, self.cam = ref, scene, cam
        self.P, self.L, self.W, self.H = ref.P, ref.L, ref.W, ref.H
        self.listed = np.zeros(self.P, bool)
        for tl in ref.tiles:
            self.listed[tl["g"]] = True

    def _model(self, dtype):
        F = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
        s = self.scene
        leaf = lambda k, shape: torch.tensor(np.asarray(s[k], np.float32).reshape(shape), dtype=F, requires_grad=True)
        P, L = self.P, self.L
        return F, dict(means3D=leaf("means3D", (P, 3)), scales=leaf("scales", (P, 3)), rotations=leaf("rotations", (P, 4)),
                       shs_rest=leaf("shs", (P, -1, 3)), shs_dcs=leaf("shs_dcs", (P, L, 3)), opacities=leaf("opacities", (P, L)))

    def _per_gaussian(self, m, F):
        """-> pix [P,2], conic [P,3], level colours [P,L,3] (clamped at 0), functions of the model"""
        pix, conic = project(m["means3D"], m["scales"], m["rotations"], self.cam)
        dirs = m["means3D"] - torch.as_tensor(np.asarray(self.cam["campos"], np.float64), dtype=F)
        deg = int(self.cam["sh_degree"])
        cols = torch.stack([sh_colour(deg, torch.cat([m["shs_dcs"][:, l:l + 1], m["shs_rest"]], 1), dirs) for l in range(self.L)], 1)
        return pix, conic, cols

    def _tile(self, tl, pix, conic, cols, opac, F, is64, offsets32=False):
        """one tile's pixel values [256,3] from the per-Gaussian quantities, decisions frozen
        offsets32: centre - pixel as the forward formed it in float32 (FovBackwardRef's input) instead of from `pix`"""
        g = torch.as_tensor(tl["g"])
        X, Y = torch.as_tensor(tl["X"], dtype=F), torch.as_tensor(tl["Y"], dtype=F)
        dx, dy = pix[g, 0:1] - X[None, :], pix[g, 1:2] - Y[None, :]
        if offsets32:
            dx, dy = torch.tensor(np.asarray(tl["dx"], np.float64), dtype=F), torch.tensor(np.asarray(tl["dy"], np.float64), dtype=F)
        power = -0.5 * (conic[g, 0:1] * dx * dx + conic[g, 2:3] * dy * dy) - conic[g, 1:2] * dx * dy
        bg = torch.as_tensor(self.ref.bg, dtype=F)
        val = torch.zeros(256, 3, dtype=F)
        for st in tl["states"]:
            acc = torch.as_tensor(st["acc"])
            if not bool(acc.any()):
                Tfin = torch.ones(256, dtype=F)
                val = val + torch.as_tensor(st["wgt"] if is64 else st["wgt32"], dtype=F)[:, None] * (Tfin[:, None] * bg[None, :])
                continue
            G = torch.exp(torch.where(acc, power, torch.zeros_like(power)))   # (pairs that are not blended: their G is not used)
            oG = opac[g, st["lev"]][:, None] * G
            alpha = oG + (torch.clamp_max(oG, 0.99) - oG).detach()
            alpha = torch.where(acc, alpha, torch.zeros_like(alpha))
            Tafter = torch.cumprod(1.0 - alpha, 0)
            Tbefore = torch.cat([torch.ones(1, 256, dtype=F), Tafter[:-1]], 0)
            w = alpha * Tbefore
            share = torch.as_tensor(st["wgt"] if is64 else st["wgt32"], dtype=F)
            val = val + share[:, None] * (w.T @ cols[g, st["lev"]] + Tafter[-1][:, None] * bg[None, :])
        return val

    def image(self, dtype=np.float64):
        F, m = self._model(dtype)
        is64 = F == torch.float64
        with torch.no_grad():
            pix, conic, cols = self._per_gaussian(m, F)
            img = torch.zeros(3, self.H, self.W, dtype=F)
            bg = torch.as_tensor(self.ref.bg, dtype=F)
            for tl in self.ref.tiles:
                ins = torch.as_tensor(tl["inside"])
                if len(tl["g"]) == 0:
                    val = bg[None, :].expand(256, 3)
                else:
                    val = self._tile(tl, pix, conic, cols, m["opacities"], F, is64)
                img[:, torch.as_tensor(tl["Y"])[ins], torch.as_tensor(tl["X"])[ins]] = val[ins].T
        return img.numpy()

    def _tile_stage(self, leaves, opac, dL_dpix, F, offsets32=False):
        """accumulates, tile by tile, the gradients of sum(dL_dpix * image) in the leaves (pix, conic, level colours) and `opac`"""
        is64 = F == torch.float64
        dpix = torch.tensor(np.array(dL_dpix), dtype=F)
        for tl in self.ref.tiles:
            if len(tl["g"]) == 0 or not any(st["acc"].any() for st in tl["states"]):
                continue
            ins = torch.as_tensor(tl["inside"])
            dl = torch.zeros(256, 3, dtype=F)
            dl[ins] = dpix[:, torch.as_tensor(tl["Y"])[ins], torch.as_tensor(tl["X"])[ins]].T
            (self._tile(tl, leaves[0], leaves[1], leaves[2], opac, F, is64, offsets32) * dl).sum().backward()

    def level_gradients_on(self, fwd, dL_dpix):
        """The tile stage alone, in float64, fed with the FORWARD's float32 pixel positions, conics and level colours -- the inputs
        FovBackwardRef takes: -> dict(dL_dopacities, dL_dlevel_colours, dL_dshs_dcs), the same numbers as FovBackwardRef.backward's
        by another derivation (autograd here, hand-written sums there)."""
        F = torch.float64
        colours = np.nan_to_num(np.asarray(self.ref.colours, np.float64), nan=0.0)
        leaves = [torch.tensor(np.asarray(x, np.float64), dtype=F, requires_grad=True) for x in (np.asarray(fwd["means2D"])[:, :2], fwd["conic"], colours)]
        opac = torch.tensor(np.asarray(self.ref.opac, np.float64), dtype=F, requires_grad=True)
        self._tile_stage(leaves, opac, dL_dpix, F, offsets32=True)
        gcol = np.zeros_like(colours) if leaves[2].grad is None else leaves[2].grad.numpy()
        gop = np.zeros((self.P, self.L)) if opac.grad is None else opac.grad.numpy()
        return dict(dL_dopacities=gop, dL_dlevel_colours=gcol, dL_dshs_dcs=np.where(colours > 0, R.SH_C0 * gcol, 0.0))

    def backward(self, dL_dpix, dtype=np.float64):
        """-> dict of the eight gradient tensors (numpy, `dtype`)"""
        F, m = self._model(dtype)
        pix, conic, cols = self._per_gaussian(m, F)
        leaves = [t.detach().requires_grad_(True) for t in (pix, conic, cols)]
        self._tile_stage(leaves, m["opacities"], dL_dpix, F)

        zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
        gpix, gconic, gcols = (zero(t) for t in leaves)
        torch.autograd.backward([pix, conic, cols], [gpix, gconic, gcols])
        out = {("dL_d" + k): zero(v).numpy() for k, v in m.items()}
        # dL_dscales follows the reference's CONVENTION, as every backward pass of the package does (tests/test_oracle_pins.py,
        # DESIGN.md): backward.cu:295-325 forms s = mod * scale and returns dL/ds, without the factor d s / d scale = mod that
        # autograd through diag(mod * scales) applies. The gradient with respect to s is autograd's divided by mod.
        out["dL_dscales"] = out["dL_dscales"] / out["dL_dscales"].dtype.type(float(self.cam.get("scale_modifier", 1.0)))
        out["dL_dlevel_colours"] = gcols.numpy()
        d2 = np.zeros((self.P, 3), out["dL_dmeans3D"].dtype)
        d2[:, 0], d2[:, 1] = gpix[:, 0].numpy() * (0.5 * self.W), gpix[:, 1].numpy() * (0.5 * self.H)
        out["dL_dmeans2D"] = d2
        # (Gaussians no tile lists took no part in the frame; a NaN of their projection -- behind the camera -- must not leak through a
        # zero gradient of the second stage)
        for k in GEOMETRY:
            out[k][~self.listed] = 0
        return out


def tangent_clamps(scene, cam):
    ux, uy, limx, limy = bs.tangents(scene, cam)
    return (ux < -limx) | (ux > limx), (uy < -limy) | (uy > limy)


def census(ref, scene, cam, g64):
    """Masks over the P Gaussians: live (any level's dL_dopacities != 0), two_level (live and blended by a state of a two-level tile),
    colour_clamped (live with a clamped channel at a level a tile used), clamp_x / clamp_y / clamp_both (live with a clamped tangent),
    scale_modifier (every live row when the factor is not 1)."""
    live = (np.asarray(g64["dL_dopacities"]) != 0).any(axis=1)
    cx, cy = tangent_clamps(scene, cam)
    used = ref.used_single | ref.used_blend
    clamped = ((np.nan_to_num(ref.colours, nan=1.0) == 0) & used[..., None]).any(axis=(1, 2))
    mod = float(cam.get("scale_modifier", 1.0))
    return dict(live=live, two_level=live & ref.used_blend.any(axis=1), colour_clamped=live & clamped, clamp_x=live & cx, clamp_y=live & cy,
                clamp_both=live & cx & cy, scale_modifier=live & (mod != 1.0))


@functools.lru_cache(maxsize=None)
def reference(name, sh_degree=3):
    """The named scene's forward, FovBackwardRef, autograd reference, loss gradient, float32 / float64 gradients and both censuses:
    computed once per session and shared (read-only: the arrays are locked)."""
    if name != "close-wide-x2.5-fov" and sh_degree == 3:
        r = fs.reference(name)   # (the forward and the frozen decisions are the appearance scenes': one computation per session)
        scene, cam, settings, fwd, ref, dpix = (r[k] for k in ("scene", "cam", "settings", "fwd", "ref", "dpix"))
    else:
        scene, cam, settings = build(name, sh_degree)
        fwd = fs.forward(scene, cam, settings)
        ref = fs.make_ref(fwd, scene, cam, settings)
        dpix = R.dL_for(cam)
    full = FovFullBackwardRef(ref, scene, cam)
    g32, g64 = full.backward(dpix, np.float32), full.backward(dpix, np.float64)
    out = dict(name=name, scene=scene, cam=cam, settings=settings, fwd=fwd, ref=ref, full=full, dpix=dpix, g32=g32, g64=g64, L=ref.L,
               census=census(ref, scene, cam, g64), level_census=fs.census(ref, fwd, scene, g64))
    fs._lock(scene, {k: v for k, v in fwd.items() if isinstance(v, np.ndarray)}, g32, g64, out["census"], out["level_census"])
    dpix.setflags(write=False)
    return out


def judge(got, g32, g64, cen, level_cen, tag, L, branches=(), min_rows=MIN_LIVE, factors=None, geometry=GEOMETRY):
    """THE comparison: fov_backward_scenes.judge on the three per-level tensors (whole, and the exact zeros), backward_scenes.judge on the
    five per-Gaussian tensors, whole and on the live rows of every branch in `branches`: the same clauses and constants (rtol 1e-4,
    FACTOR 1.5, FLOOR, ABS_ROWS, TAIL_FLOOR). Coefficients of dL_dshs_rest above the frame's degree are judged by the caller.
    geometry: the per-Gaussian tensors judged (a frame of SH degree 0 leaves dL_dshs_rest out: the reference's is all zeros, no row
    carries a gradient, and the caller asserts exact zeros instead)."""
    fs.judge(got, g32, g64, level_cen, tag, L, min_rows=min_rows, factors=factors)
    bs.judge(got, g32, g64, cen, tag, branches=branches, min_rows=min_rows, factors=factors, tensors=geometry)
    dead = ~cen["live"]
    allowed = fs.stray_allowance(g64)
    for k in geometry:
        x = np.asarray(got[k]).reshape(len(dead), -1)
        stray = int((x[dead] != 0).any(axis=1).sum())
        assert stray <= allowed, f"{tag} {k}: {stray} Gaussians the reference leaves at zero carry a gradient (allowed {allowed})"


def judge_short(got, g32, g64, level_cen, tag, L, min_rows):
    """Short scenes: EVERY row of every tensor within SHORT_RTOL of the float64 reference, no outlier share."""
    fs.judge_short(got, g32, g64, level_cen, tag, L, min_rows)
    for k in GEOMETRY:
        g, f64 = np.asarray(got[k]).reshape(np.shape(g64[k])), np.asarray(g64[k])
        st = grad_stats(g, f64, rtol=SHORT_RTOL)
        print(f"{tag} {k}: worst row {st['row_rel_max']:.2e} (float32 reference: {grad_stats(np.asarray(g32[k]), f64)['row_rel_max']:.2e})")
        check_grad(g, f64, f"{tag} {k} vs the double-precision reference", min_rows=min(min_rows, int((f64.reshape(len(f64), -1) != 0).any(axis=1).sum())))
        assert st["frac_bad"] == 0.0, f"{tag} {k}: a row is {st['row_rel_max']:.2e} off the double-precision gradient"


def record_census(name, cen, extra=None):
    parity_report.record("census", f"{_where()} {name}", **{k: int(v.sum()) for k, v in cen.items()}, **(extra or {}))
