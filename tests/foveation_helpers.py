"""Helpers of the foveation-settings tests: the independent derivation (tests/numpy_fov_rasterizer.py) under a setting's constants,
and the HIP library through the entry points that take the settings (what tests/gpu_helpers.hip_forward does without them)."""
import numpy as np

from tests import numpy_fov_rasterizer as npr
from tests.helpers import cam_dict, scene_dict, small_camera, small_cloud, syn
from fov3dgs_amd.rasterizer import FoveationSettings

# The GPU parity cases: (settings, alpha, gaze). Frames of 640x368, where every level holds tiles, many tiles blend and no tile's
# tile_min lies within 1e-4 of a level boundary or of the blend threshold (asserted by the tests on the derivation's own values).
CASES = {
    "L5": (FoveationSettings(5, 9.0, 2.4, 1.2, 0.4, 0.6), 0.08, (0.7, 0.3)),
    "L6": (FoveationSettings(6, 16.0, 1.6, 0.8, 0.5, 0.5), 0.05, (0.3, 0.6)),
    "L8": (FoveationSettings(8, 25.0, 2.0, 1.0, 0.6, 0.4), 0.1, (0.3, 0.6)),
    "L3": (FoveationSettings(3, 12.0, 2.0, 1.0, 0.5, 0.5), 0.05, (0.62, 0.35)),
    "L4band": (FoveationSettings(4, 12.0, 2.0, 1.0, 0.35, 0.65), 0.05, (0.3, 0.6)),
    "L2": (FoveationSettings(2, 12.0, 2.0, 1.0, 0.5, 0.5), 0.05, (0.45, 0.5)),
}
WIDTH, HEIGHT, POINTS = 640, 368, 3000


def step_and_cap(settings):
    """the level step and cap of a setting, in the order of operations fr_foveation documents (floats)"""
    s = np.float32(np.sqrt(np.float64(np.float32(settings.max_pooling_size))))
    step = np.float32((np.float64(s) - 1.0) / np.float64(np.float32(settings.levels - 1)))
    cap = np.float32(np.float64(np.float32(settings.levels)) - 0.1)
    return step, cap


def set_constants(monkeypatch, settings):
    """the derivation reads its constants as module globals at call time: give it the setting's"""
    monkeypatch.setattr(npr, "FOV_NUM", int(settings.levels))
    monkeypatch.setattr(npr, "SQRT_MAX_PS", float(np.float32(np.sqrt(np.float64(np.float32(settings.max_pooling_size))))))
    monkeypatch.setattr(npr, "REAL_IMAGE_WIDTH", float(settings.real_image_width))
    monkeypatch.setattr(npr, "REAL_VIEWING_DISTANCE", float(settings.real_viewing_distance))
    monkeypatch.setattr(npr, "START_BLEND", float(settings.start_blend))
    monkeypatch.setattr(npr, "BLEND_WIDTH", float(settings.blend_width))


def level_map(monkeypatch, settings, cam):
    set_constants(monkeypatch, settings)
    return npr.tile_level_map(npr._Arith(np.float32), cam)


def derivation(monkeypatch, settings, scene, cam):
    set_constants(monkeypatch, settings)
    return npr.rasterize("fov_pcheck_obb", scene, cam, np.float32)


def fov_case(settings, alpha, gaze, width=WIDTH, height=HEIGHT, P=POINTS, seed=3, bg=(0.1, 0.2, 0.3)):
    """-> (scene, cam) dicts: helpers.small_cloud composed into settings.levels equally likely layers"""
    cloud = small_cloud(P, seed)
    L = int(settings.levels)
    fov = syn.foveation_layers(cloud, seed=seed + 1, fractions=(1.0 / L,) * L)
    return scene_dict(cloud, "fov_pcheck_obb", fov), cam_dict(small_camera(width, height), bg=bg, gaze=gaze, alpha=alpha)


def hip_forward_fov(scene, cam, settings, dev="cuda:0", debug=True, packed=False):
    """gpu_helpers.hip_forward("fov_pcheck_obb", ...) through the entry point that takes `settings` (None: the one without), plus
    the level rows and level ranges per Gaussian: level_colours [P,L,4] (NaN = not a cull survivor) and level_ranges [P,2]."""
    import torch
    from fov3dgs_amd import _native
    from fov3dgs_amd.rasterizer import _forward_native, pack_model
    from tests.gpu_helpers import _t, _view, settings_from, vis_list_of
    lib = _native.load()
    vid = _native.VARIANT_FOV_PCHECK_OBB
    rs = settings_from(cam, dev, debug)
    tens = {k: _t(scene.get(k), dev) for k in ("means3D", "shs", "opacities", "scales", "rotations", "shs_dcs", "highest_levels")}
    pk = None
    if packed:
        pk = pack_model(tens["means3D"], tens["scales"], tens["rotations"], tens["opacities"], shs=tens["shs"],
                        shs_dcs=tens["shs_dcs"], highest_levels=tens["highest_levels"])
    res = _forward_native(vid, rs, tens["means3D"], tens["shs"], None, tens["opacities"], tens["scales"], tens["rotations"], None,
                          tens["shs_dcs"], tens["highest_levels"], cam.get("gaze", (0.5, 0.5)), cam.get("alpha", 0.05), packed=pk,
                          foveation=settings)
    torch.cuda.synchronize()
    num_rendered, color, radii, geom, binb, img = res[:6]
    W, H = rs.image_width, rs.image_height
    T = ((W + 15) // 16) * ((H + 15) // 16)
    P = tens["means3D"].shape[0]
    L = 4 if settings is None else int(settings.levels)
    out = {"num_rendered": num_rendered, "color": color.cpu().numpy(), "radii": radii.cpu().numpy(), "_lease": res[-1],
           "visibility": getattr(radii, "_fovraster_visibility", None)}
    if P == 0 or img.numel() == 0:
        out["ranges"], out["point_list"] = np.zeros((T, 2), np.uint32), np.zeros(0, np.uint32)
        return out
    out["ranges"] = _view(img, lib.fr_image_ranges(vid, W, H, img.data_ptr()), 2 * T, torch.int32).cpu().numpy().astype(np.uint32).reshape(T, 2)
    vis = vis_list_of(lib, vid, P, geom)
    vl = vis.cpu().numpy().astype(np.int64)
    if num_rendered > 0:
        items = _view(binb, lib.fr_binning_point_list(vid, num_rendered, binb.data_ptr()), num_rendered, torch.int32).long()
        out["point_list"] = vis[items].cpu().numpy().astype(np.uint32)
    else:
        out["point_list"] = np.zeros(0, np.uint32)
    lv = _view(img, lib.fr_image_tile_levels(W, H, img.data_ptr()), 5 * T, torch.float32).cpu().numpy().reshape(5, T)
    out["tile_levels"], out["tile_min"], out["tile_gx"], out["tile_gy"] = lv[0], lv[1], lv[2], lv[3]
    out["tile_blend"] = (lv[4] != 0).astype(np.uint8)
    rows = np.full((P, max(L, 4), 4), np.nan, np.float32)
    rows[vl, :4] = _view(geom, lib.fr_geometry_level_colours(P, geom.data_ptr()), 16 * P, torch.float32).view(P, 4, 4).cpu().numpy()[:len(vl)]
    if L > 4:
        hi = lib.fr_geometry_level_colours_hi(P, L, geom.data_ptr())
        assert hi, "levels > 4: the library keeps the rows of the levels 4 .. 7"
        rows[vl, 4:] = _view(geom, hi, 16 * P, torch.float32).view(P, 4, 4).cpu().numpy()[:len(vl), :L - 4]
    out["level_colours"] = rows[:, :L]
    lr = np.zeros(P, np.int64)
    lr[vl] = _view(geom, lib.fr_geometry_level_ranges(P, geom.data_ptr()), P, torch.int32).cpu().numpy()[:len(vl)].astype(np.int64) & 0xffffffff
    out["level_ranges"] = np.stack([lr & 0xff, (lr >> 8) & 0xff], axis=1).astype(np.int32)
    return out
