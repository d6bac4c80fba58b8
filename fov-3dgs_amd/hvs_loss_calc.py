"""Drop-in for the reference's ``from hvs_loss_calc import HVSLoss`` (fov3dgs/hvs_loss_calc.py:21-75), the object hvs_metrics.py and
quality_metrics*.py compute "HVS Uniform" and "HVS FOV" with: both losses as fused HIP (fov3dgs_amd.odak_perception).

    from fov3dgs_amd.hvs_loss_calc import HVSLoss
    hvs = HVSLoss()                                     # the reference's defaults
    uniform = hvs.calc_uniform_loss(img, gt, pooling_size=1)
    fov = hvs.calc_fov_loss(img, gt, gaze=[0.5, 0.5])

The constructor is the reference's plus ``filters=`` (the steerable-pyramid coefficients are an input of this library: see
fov3dgs_amd.odak_perception). Both calls take the UN-resized pictures: where the reference's resize_img (:51-64) interpolates
them to the next multiple of 2 ** n_pyramid_levels first, the kernels sample them in their first load (resize="pyramid") and
the gradient has the pictures' own shape.
"""
from .odak_perception import MetamericLoss, MetamericLossUniform


class HVSLoss:
    def __init__(self, n_pyramid_levels=5, n_orientations=6, device="cuda", loss_type="MSE", bilinear_downsampling=True, alpha=0.05,
                 real_image_width=1.0, real_viewing_distance=0.5, uniform_pooling_size=1, filters=None):
        self.n_pyramid_levels = n_pyramid_levels
        self.n_orientations = n_orientations
        self.device = device
        self.bilinear_downsampling = bilinear_downsampling
        self.loss_type = loss_type
        self.uniform_loss = MetamericLossUniform(n_pyramid_levels=n_pyramid_levels, n_orientations=n_orientations,
                                                 pooling_size=uniform_pooling_size, device=device, loss_type=loss_type,
                                                 bilinear_downsampling=bilinear_downsampling, filters=filters)
        self.alpha = alpha
        self.fov_loss = MetamericLoss(device=device, alpha=alpha, real_image_width=real_image_width,
                                      real_viewing_distance=real_viewing_distance, n_pyramid_levels=n_pyramid_levels, mode="quadratic",
                                      n_orientations=n_orientations, use_l2_foveal_loss=False, fovea_weight=False, use_radial_weight=False,
                                      use_fullres_l0=False, equi=False, loss_type=loss_type, use_bilinear_downup=bilinear_downsampling,
                                      filters=filters)

    def calc_uniform_loss(self, img1, img2, pooling_size=1):
        """hvs_loss_calc.py:66-70: the pooling size is assigned per call (the uniform class reads it at call time)"""
        self.uniform_loss.pooling_size = pooling_size
        return self.uniform_loss(img1, img2, resize="pyramid")

    def calc_fov_loss(self, img1, img2, gaze=[0.5, 0.5]):
        """hvs_loss_calc.py:72-75"""
        return self.fov_loss(img1, img2, gaze=gaze, resize="pyramid")
