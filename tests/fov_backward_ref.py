"""Reference of the foveated renderer's appearance backward pass (fr_backward_fov_appearance): the gradients of the per-level
opacities [P,L] and DC colours [P,L,3] through the forward pass of the foveated renderer.

The reference has no such backward; the definition is its RS / R0 backward arithmetic (backward.cu:399-557) applied to the foveated
forward pass. This file is a restatement of tests/numpy_fov_rasterizer.blend_fov, tile by tile:

  * FORWARD AND DECISIONS in fp32, with that function's operations in its order: which (pixel, state, Gaussian) pairs are blended
    (support test, alpha < 1/255, the upper state's existence skip), where a state stops (T (1 - alpha) < 1e-4; the stopping entry
    is not accumulated), which state-1 pixels of a two-level tile start finished (est > L2). Inputs: a forward dict of the C oracle
    (oracle.forward("fov_pcheck_obb", ...)) or of the numpy derivation under other settings -- point_list, ranges, means2D, conic,
    tile_min, tile_gx / gy, tile_blend, fov_colors, level_ranges -- and the scene's opacities / shs_dcs / highest_levels.
  * VALUES AND GRADIENTS in the dtype asked for (float64: the reference; float32: the same arithmetic for checks.check_against_noise)
    with the decisions FROZEN. Per state and pixel, entries j in list order with alpha_j = min(0.99, o_j G_j) where blended, else 0:
        T_j = prod_{i<j} (1 - alpha_i),  w_j = alpha_j T_j,  value = sum_j w_j c_j + T_end bg
        dL/dc_j      += w_j dL                                       (dL = the state's share of dL/dpixel: w1 or 1 - w1 or 1; w1 is
                                                                      a value like the others: in float32, or from the same fp32 `est`
                                                                      in double)
        dL/dalpha_j   = T_j (c_j . dL) - (sum_{i>j} w_i (c_i . dL) + T_end (bg . dL)) / (1 - alpha_j)
        dL/do_j      += G_j dL/dalpha_j                              (the min is not differentiated: backward.cu:497-541)
    and dL/dshs_dcs = SH_C0 dL/dcolour where the level colour is > 0, else 0 (clamped at that level).
  * frozen_loss(): sum(dL_dpix * image) as a function of (opacities, shs_dcs) with decisions, exponentials, rest-SH part and clamp
    flags held: multilinear in what is perturbed, so central differences are exact up to rounding (the CPU test's check (b)).
"""
import numpy as np

BLOCK = 16
SH_C0 = 0.28209479177387814


def _exp32(p):
    return np.exp(p.astype(np.float64)).astype(np.float32)   # expf, correctly rounded (numpy_fov_rasterizer._exp)


class FovBackwardRef:
    def __init__(self, fwd, scene, cam, levels=4, start_blend=0.5, blend_width=0.5):
        f32 = np.float32
        self.W, self.H = int(cam["image_width"]), int(cam["image_height"])
        self.gx, self.gy = (self.W + BLOCK - 1) // BLOCK, (self.H + BLOCK - 1) // BLOCK
        self.L = int(levels)
        self.bg = np.asarray(cam["bg"], f32)
        self.P = int(np.asarray(scene["means3D"]).shape[0])
        self.opac = np.asarray(scene["opacities"], f32).reshape(self.P, self.L)
        self.dcs = np.asarray(scene["shs_dcs"], f32).reshape(self.P, self.L, 3)
        self.colours = np.asarray(fwd["fov_colors"], f32)[:, :self.L]          # NaN where the level was never evaluated
        highest = np.asarray(scene["highest_levels"], f32).reshape(-1)
        mean2d, conic = np.asarray(fwd["means2D"], f32), np.asarray(fwd["conic"], f32)
        ranges, plist = np.asarray(fwd["ranges"]).astype(np.int64), np.asarray(fwd["point_list"]).astype(np.int64)
        tmin = np.asarray(fwd["tile_min"], f32)
        tgx, tgy = np.asarray(fwd["tile_gx"], f32), np.asarray(fwd["tile_gy"], f32)
        tblend = np.asarray(fwd["tile_blend"]).astype(bool)
        lx, ly = np.tile(np.arange(BLOCK), BLOCK), np.repeat(np.arange(BLOCK), BLOCK)
        self.tiles = []
        for t in range(self.gx * self.gy):
            s, e = ranges[t]
            X, Y = (t % self.gx) * BLOCK + lx, (t // self.gx) * BLOCK + ly
            inside = (X < self.W) & (Y < self.H)
            g = plist[s:e]
            blend = bool(tblend[t])
            with np.errstate(all="ignore"):
                L1 = int(tmin[t]) if np.isfinite(tmin[t]) else 0
            est = tmin[t] + (lx.astype(f32) * tgx[t] + ly.astype(f32) * tgy[t]) / f32(BLOCK)
            # the decisions, in fp32 (blend_fov)
            dx, dy = mean2d[g, 0:1] - X.astype(f32)[None, :], mean2d[g, 1:2] - Y.astype(f32)[None, :]
            power = -f32(0.5) * (conic[g, 0:1] * dx * dx + conic[g, 2:3] * dy * dy) - conic[g, 1:2] * dx * dy
            with np.errstate(all="ignore"):
                support = ~((power > 0) | (power < f32(-4.5)))
                e32 = _exp32(power)
            states = []
            if blend:
                with np.errstate(all="ignore"):
                    x = np.abs(est - (f32(L1) + f32(start_blend))) / f32(blend_width)
                    x = np.fmax(f32(0), np.fmin(f32(1), x))
                    w1 = f32(1) - (f32(3) * x * x - f32(2) * x * x * x)
                    # the same weight in double, from the tile map's fp32 numbers (tile_min, the gradient, the fp32 constants):
                    # w1 = 1 - smoothstep cancels where x is near 1 (w1 ~ 3 (1 - x)^2), so the fp32 rounding of est (2e-7) and of w1
                    # (6e-8 absolute) is a RELATIVE error of up to 1e-4 in the lower state's share of a pixel -- part of the fp32
                    # arithmetic's noise, not a decision to freeze (the decision est > L2 above stays the fp32 one)
                    est64 = np.float64(tmin[t]) + (lx * np.float64(tgx[t]) + ly * np.float64(tgy[t])) / BLOCK
                    x64 = np.abs(est64 - (np.float64(L1) + np.float64(f32(start_blend)))) / np.float64(f32(blend_width))
                    x64 = np.fmax(0.0, np.fmin(1.0, x64))
                    w1d = 1.0 - (3.0 * x64 * x64 - 2.0 * x64 * x64 * x64)
                exists = ~((highest[g] + f32(1)) < (tmin[t] + f32(1)))
                specs = [(L1, ~inside | (est > f32(L1 + 1)), (w1, w1d), None), (L1 + 1, ~inside, (f32(1) - w1, 1.0 - w1d), exists)]
            else:
                specs = [(L1, ~inside, (np.ones(256, f32), np.ones(256)), None)]
            for lev, done0, (wgt, wgt_d), exists in specs:
                lev = max(min(lev, self.L - 1), 0)   # (tile_min <= -1: level 0, as the oracle and the library index it)
                with np.errstate(all="ignore"):
                    a = np.fmin(f32(0.99), self.opac[g, lev][:, None] * e32)
                    cand = support & ~(a < f32(1) / f32(255))
                if exists is not None:
                    cand &= exists[:, None]
                T, done = np.ones(256, f32), done0.copy()
                acc = np.zeros((len(g), 256), bool)
                last = np.zeros(256, np.int64)
                for j in range(len(g)):
                    go = cand[j] & ~done
                    if not go.any():
                        if done.all():
                            break
                        continue
                    t1 = T * (f32(1) - a[j])
                    stop = go & (t1 < f32(0.0001))
                    ac = go & ~stop
                    T = np.where(ac, t1, T)
                    done |= stop
                    acc[j] = ac
                    last[ac] = j + 1
                states.append(dict(lev=lev, acc=acc, wgt32=np.where(inside, wgt, 0).astype(f32), wgt=np.where(inside, wgt_d, 0).astype(np.float64),
                                   final_T=T, n_contrib=last))
            self.tiles.append(dict(g=g, X=X, Y=Y, inside=inside, blend=blend, states=states, dx=dx, dy=dy, conic=conic[g]))
        # which levels of which Gaussians a tile of each kind used (for the tests' sampling): [P, L] bools
        self.used_single, self.used_blend = np.zeros((self.P, self.L), bool), np.zeros((self.P, self.L), bool)
        for tl in self.tiles:
            for st in tl["states"]:
                rows = tl["g"][st["acc"].any(axis=1)]
                (self.used_blend if tl["blend"] else self.used_single)[rows, st["lev"]] = True
        self.tiles_of = None

    # ---- values -------------------------------------------------------------------------------------------------------------
    def _G(self, tl, F):
        dx, dy, c = tl["dx"].astype(F), tl["dy"].astype(F), tl["conic"].astype(F)
        power = -F(0.5) * (c[:, 0:1] * dx * dx + c[:, 2:3] * dy * dy) - c[:, 1:2] * dx * dy
        with np.errstate(all="ignore"):
            return np.exp(np.where(power > 0, F(0), power))   # (never blended where power > 0: the value is not used)

    def _state(self, tl, st, G, opac, F):
        alpha = np.where(st["acc"], np.minimum(F(0.99), opac[tl["g"], st["lev"]].astype(F)[:, None] * G), F(0))
        om = F(1) - alpha
        Tafter = np.cumprod(om, axis=0) if len(alpha) else np.ones((0, 256), F)
        Tbefore = np.vstack([np.ones((1, 256), F), Tafter[:-1]]) if len(alpha) else Tafter
        Tfin = Tafter[-1] if len(alpha) else np.ones(256, F)
        return alpha, om, Tbefore, Tfin

    def _wgt(self, st, F):
        """the state's share of its pixels: float32 as the forward pass forms it, or the same expression in double"""
        return st["wgt32"] if F is np.float32 else st["wgt"].astype(F)

    def _colours(self, colours, F):
        return np.nan_to_num(np.asarray(colours, F), nan=0.0)

    def image(self, opac=None, colours=None, dtype=np.float64, tiles=None, pixels=False):
        """The image [3,H,W] from the frozen decisions (pixels=True: {tile: [256,3]} of the tiles asked for instead)."""
        F = np.dtype(dtype).type
        opac = self.opac if opac is None else opac
        col = self._colours(self.colours if colours is None else colours, F)
        bg = self.bg.astype(F)
        img = np.zeros((3, self.H, self.W), F)
        out = {}
        for t in (range(len(self.tiles)) if tiles is None else tiles):
            tl = self.tiles[t]
            G = self._G(tl, F)
            val = np.zeros((256, 3), F)
            for st in tl["states"]:
                alpha, om, Tb, Tfin = self._state(tl, st, G, opac, F)
                c = col[tl["g"], st["lev"]]
                val += self._wgt(st, F)[:, None] * ((alpha * Tb).T @ c + Tfin[:, None] * bg[None, :])
            if pixels:
                out[t] = val
            else:
                ins = tl["inside"]
                for ch in range(3):
                    img[ch][tl["Y"][ins], tl["X"][ins]] = val[ins, ch]
        return out if pixels else img

    def state_planes(self):
        """final_T [2,H,W] (fp32) and n_contrib [2,H,W] per level state as the state-keeping forward keeps them, and `single` [H,W]:
        the pixels of single-level tiles. Plane 1 is defined in two-level tiles only (elsewhere 1 / 0 here)."""
        fT, nc = np.ones((2, self.H, self.W), np.float32), np.zeros((2, self.H, self.W), np.int64)
        single = np.zeros((self.H, self.W), bool)
        for tl in self.tiles:
            ins = tl["inside"]
            for k, st in enumerate(tl["states"]):
                fT[k][tl["Y"][ins], tl["X"][ins]] = st["final_T"][ins]
                nc[k][tl["Y"][ins], tl["X"][ins]] = st["n_contrib"][ins]
            single[tl["Y"][ins], tl["X"][ins]] = not tl["blend"]
        return fT, nc, single

    # ---- gradients ----------------------------------------------------------------------------------------------------------
    def backward(self, dL_dpix, dtype=np.float64, opac=None, colours=None):
        """-> dict(dL_dopacities [P,L], dL_dlevel_colours [P,L,3], dL_dshs_dcs [P,L,3]) in `dtype`."""
        F = np.dtype(dtype).type
        opac = self.opac if opac is None else opac
        colraw = self.colours if colours is None else colours
        col = self._colours(colraw, F)
        bg = self.bg.astype(F)
        dpix = np.asarray(dL_dpix, F)
        d_op, d_col = np.zeros((self.P, self.L), F), np.zeros((self.P, self.L, 3), F)
        for tl in self.tiles:
            if len(tl["g"]) == 0:
                continue
            ins, g = tl["inside"], tl["g"]
            dl = np.zeros((256, 3), F)
            dl[ins] = dpix[:, tl["Y"][ins], tl["X"][ins]].T
            G = self._G(tl, F)
            for st in tl["states"]:
                if not st["acc"].any():
                    continue
                alpha, om, Tb, Tfin = self._state(tl, st, G, opac, F)
                dlw = dl * self._wgt(st, F)[:, None]
                c = col[g, st["lev"]]
                w = alpha * Tb
                cd = c @ dlw.T                                              # c_j . dL per pixel
                np.add.at(d_col[:, st["lev"]], g, w @ dlw)
                wc = w * cd
                behind = np.vstack([np.cumsum(wc[::-1], axis=0)[::-1][1:], np.zeros((1, 256), F)])
                dalpha = Tb * cd - (behind + (Tfin * (dlw @ bg))[None, :]) / om
                np.add.at(d_op[:, st["lev"]], g, np.where(st["acc"], G * dalpha, F(0)).sum(axis=1))
        with np.errstate(invalid="ignore"):
            open_ch = np.nan_to_num(np.asarray(colraw, np.float64), nan=0.0) > 0
        return dict(dL_dopacities=d_op, dL_dlevel_colours=d_col, dL_dshs_dcs=np.where(open_ch, F(SH_C0) * d_col, F(0)))

    # ---- the frozen function of check (b) -----------------------------------------------------------------------------------
    def tiles_with(self, gi):
        if self.tiles_of is None:
            self.tiles_of = {}
            for t, tl in enumerate(self.tiles):
                for q in np.unique(tl["g"]):
                    self.tiles_of.setdefault(int(q), []).append(t)
        return self.tiles_of.get(int(gi), [])

    def colours_from_dcs(self, dcs):
        """The level colours as a function of shs_dcs with the rest-SH part and the clamp flags of the forward state frozen."""
        base = np.nan_to_num(self.colours.astype(np.float64), nan=0.0)
        rest = base - SH_C0 * self.dcs.astype(np.float64)
        return np.where(base > 0, SH_C0 * np.asarray(dcs, np.float64) + rest, 0.0)

    def frozen_loss(self, dL_dpix, opac, dcs, tiles):
        """sum(dL_dpix * image) over `tiles`, in double, decisions frozen."""
        px = self.image(opac=opac, colours=self.colours_from_dcs(dcs), tiles=tiles, pixels=True)
        total = 0.0
        for t, val in px.items():
            tl = self.tiles[t]
            ins = tl["inside"]
            total += float((np.asarray(dL_dpix, np.float64)[:, tl["Y"][ins], tl["X"][ins]].T * val[ins]).sum())
        return total


def rows(x, L):
    """one row per (Gaussian, level): [P, L, ...] -> [P L, ...]"""
    x = np.asarray(x)
    return x.reshape((x.shape[0] * L,) + x.shape[2:]) if x.ndim > 2 else x.reshape(-1, 1)


# ---- the scenes both test files use ---------------------------------------------------------------------------------------------
MIN_ROWS_PER_LEVEL = 50    # (Gaussian, level) rows with a gradient at EACH level of the main scene
MIN_BLEND_TILES = 10       # two-level tiles of the main scene
MIN_ROWS_OTHER = 100       # ... and rows with a gradient, all levels together, of every other parity scene
# The main scene: small_case("fov_pcheck_obb") at 200x120 with alpha 0.6 and the gaze moved to (0.2, 0.35). The test cloud is dense
# (a pixel finishes a few splats deep), so the handful of level-0 tiles around the gaze see few Gaussians: at the default gaze
# (0.4, 0.55) the reference counts 43 / 271 / 227 / 149 rows with a gradient at the levels 0 / 1 / 2 / 3, here 53 / 230 / 206 / 401
# and 18 two-level tiles (a scan over gazes and alphas found no more than 57 rows at level 0).
MAIN = dict(alpha=0.6, gaze=(0.2, 0.35))
# the parity scenes of the GPU test: the main one, then alpha 0.6 / 0.05 at the gazes (0.4, 0.55) and (0.9, 0.1), and one ragged frame
PARITY = (MAIN, dict(alpha=0.6, gaze=(0.4, 0.55)), dict(alpha=0.05, gaze=(0.4, 0.55)), dict(alpha=0.6, gaze=(0.9, 0.1)),
          dict(alpha=0.05, gaze=(0.9, 0.1)), dict(alpha=0.6, gaze=(0.2, 0.35), width=203, height=131))
BG = (0.3, 0.1, 0.25)      # non-zero background


def dL_for(cam, seed=11):
    return np.random.default_rng(seed).standard_normal((3, int(cam["image_height"]), int(cam["image_width"]))).astype(np.float32)


_cache = {}


def case(alpha=0.6, gaze=(0.4, 0.55), width=200, height=120, mutate=None):
    """-> (scene, cam, oracle forward, FovBackwardRef, dL_dpix), computed once per key and shared (read-only).
    mutate: None, or the name of a scene variant: "clamp" (DCs shifted so that roughly four channels in ten clamp), "hl0" (every
    highest level 0), "sat" (every seventh Gaussian's opacities 1.0), "clip98" (opacities clipped to <= 0.98: check (b))."""
    key = (alpha, tuple(gaze), width, height, mutate)
    if key not in _cache:
        from oracle import oracle as orc
        from tests.helpers import small_case
        scene, cam = small_case("fov_pcheck_obb", bg=BG, gaze=gaze, alpha=alpha, width=width, height=height)
        scene = dict(scene)
        if mutate == "clamp":
            scene["shs_dcs"] = (scene["shs_dcs"] - np.float32(1.5)).astype(np.float32)
        elif mutate == "hl0":
            scene["highest_levels"] = np.zeros_like(scene["highest_levels"])
        elif mutate == "sat":
            op = scene["opacities"].copy()
            op[::7] = 1.0
            scene["opacities"] = op
        elif mutate == "clip98":
            scene["opacities"] = np.minimum(scene["opacities"], np.float32(0.98))
        fwd = orc.forward("fov_pcheck_obb", scene, cam)
        _cache[key] = (scene, cam, fwd, FovBackwardRef(fwd, scene, cam), dL_for(cam))
    return _cache[key]
