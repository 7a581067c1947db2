"""lattice_from_params on the GPU (reference: diffusion/lattice_helpers.py:55-105); matrix_to_params on the host (:16-35)."""
import torch

from .. import _hip


def lattice_from_params(lengths: torch.Tensor, angles: torch.Tensor) -> torch.Tensor:
    """lengths [B,3], angles [B,3] (consumed as radians) on a cuda device -> [B,3,3] fp32."""
    _hip.require_gpu()
    lengths = lengths.to(torch.float32).contiguous()
    angles = angles.to(device=lengths.device, dtype=torch.float32).contiguous()
    B = lengths.shape[0]
    out = torch.empty((B, 3, 3), device=lengths.device, dtype=torch.float32)
    _hip.check(_hip.lib().arreau_lattice_from_params(_hip.ptr(lengths), _hip.ptr(angles), B, _hip.ptr(out),
                                                      _hip.stream_ptr(lengths.device)), "arreau_lattice_from_params")
    return out


def matrix_to_params(matrix):
    """Host matrix_to_params (diffusion/lattice_helpers.py:16-35) in float64: cell matrices [B,3,3] (rows a, b, c; numpy or
    torch) -> (lengths [B,3], angles [B,3] in radians) as numpy arrays.  Angle i lies between the other two vectors."""
    import numpy as np
    m = np.asarray(matrix.detach().cpu() if isinstance(matrix, torch.Tensor) else matrix, dtype=np.float64).reshape(-1, 3, 3)
    lengths = np.sqrt((m ** 2).sum(-1))
    angles = np.zeros((m.shape[0], 3))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        cosv = (m[:, j, :] * m[:, k, :]).sum(-1) / (lengths[:, j] * lengths[:, k])
        angles[:, i] = np.arccos(np.clip(cosv, -1.0, 1.0))
    return lengths, angles
