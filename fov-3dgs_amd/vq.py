"""Drop-in for LightGaussian/vectree/vq.py: ``from vq import VectorQuantize`` becomes ``from fov3dgs_amd.vq import VectorQuantize``.
Only the configuration vectree.py:44-51 uses exists (fov3dgs_amd.vectree); every other argument value raises ValueError."""
from .vectree import EuclideanCodebook, VectorQuantize, nearest_code  # noqa: F401
