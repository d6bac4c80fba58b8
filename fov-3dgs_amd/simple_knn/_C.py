"""distCUDA2 of simple-knn (fov3dgs/submodules/simple-knn/spatial.cu:15-25) on the HIP library (csrc/knn.hip).

distCUDA2(points [P,3] fp32, ROCm GPU) -> [P] fp32: the mean squared distance of each point to its three nearest
neighbours, ((b0 + b1) + b2) / 3 with a missing neighbour counting as FLT_MAX (include/fovraster.h, fr_knn_mean_dist2).
The search is exact: the result has one bit pattern for a given input. Runs on the current stream, no host sync;
the workspace comes from torch's caching allocator. GPU tensors only (no CPU fallback)."""
import torch

from .. import _native
from ..rasterizer import _require_gpu


def distCUDA2(points):
    if not torch.is_tensor(points):
        raise TypeError(f"distCUDA2 expects a torch.Tensor, got {type(points).__name__}")
    _require_gpu(points)
    if points.dtype != torch.float32:
        raise RuntimeError(f"distCUDA2 expects float32 points, got {points.dtype}")
    if points.dim() != 2 or points.size(1) != 3:
        raise RuntimeError(f"distCUDA2 expects points of shape [P, 3], got {list(points.shape)}")
    lib = _native.load()
    pts = points.detach().contiguous()
    P = pts.size(0)
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    if P == 0:
        return out
    with torch.cuda.device(pts.device):
        ws = torch.empty(lib.fr_knn_workspace_bytes(P), dtype=torch.uint8, device=pts.device)
        rc = lib.fr_knn_mean_dist2(P, pts.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                   torch.cuda.current_stream(pts.device).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"fovraster knn_mean_dist2 failed ({rc}): {_native.last_error()}")
    return out
