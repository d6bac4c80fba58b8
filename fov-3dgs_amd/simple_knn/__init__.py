"""Drop-in for the reference package fov3dgs/submodules/simple-knn (imported as `simple_knn._C`).

Switch: `from simple_knn._C import distCUDA2` -> `from fov3dgs_amd.simple_knn._C import distCUDA2`.
"""
