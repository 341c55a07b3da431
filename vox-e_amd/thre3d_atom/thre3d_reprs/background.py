"""Learned environment-map background behind the voxel grid (new in this build).

A real capture has neither a black nor a white background: every pixel whose ray leaves the grid without saturating is
supervised against whatever stood behind the object.  `EnvMapBackground` gives the optimiser a place for that colour that is not
density inside the box: an equirectangular map of logits that depends on the ray direction only, composited behind the render
with the ray's leftover transmittance 1 - acc (voxe_background_fwd / voxe_background_bwd)."""
from typing import Any, Dict

import torch
from torch import Tensor

from voxe_hip import ops as _ops


class EnvMapBackground(torch.nn.Module):
    """texels [height, width, 3] of logits (zeros: a mid-grey sky); longitude wraps, the poles clamp (include/voxe.h)"""

    def __init__(self, height: int, width: int) -> None:
        super().__init__()
        if height < 2 or width < 2:
            raise ValueError(f"an environment map needs at least 2 x 2 texels; got {height} x {width}")
        self.texels = torch.nn.Parameter(torch.zeros((int(height), int(width), 3), dtype=torch.float32))

    @property
    def resolution(self):
        return int(self.texels.shape[0]), int(self.texels.shape[1])

    def get_save_config_dict(self) -> Dict[str, Any]:
        return {"height": self.resolution[0], "width": self.resolution[1]}

    def forward(self, colour: Tensor, acc: Tensor, directions: Tensor) -> Tensor:
        """colour [R,3] + (1 - acc) * sigmoid(map at directions [R,3]); differentiable w.r.t. every argument and the texels"""
        return _ops.background_composite(colour, acc, directions, self.texels)

    def extra_repr(self) -> str:
        return f"height: {self.resolution[0]}, width: {self.resolution[1]}"
