"""Per-image exposure compensation (new in this build).

A hand-held capture with auto-exposure and auto white balance does not see the scene with one exposure: without a place for the
difference the grid explains it with view-dependent colour and semi-transparent floaters, because the photometric loss demands
them.  `PerImageExposure` gives the optimiser that place: a 3 x 4 affine colour transform per training image (3D Gaussian
Splatting's exposure optimisation, URF's exposure term), applied to the rendered colour inside the loss only
(voxe_exposure_fwd_bwd).  Renders are never altered; held-out views are scored after a closed-form least-squares affine instead
(voxe_hip.ops.fit_affine_colour, the colour-corrected metrics of mip-NeRF 360 and RawNeRF)."""
from typing import Any, Dict, Optional

import torch
from torch import Tensor

from voxe_hip import ops as _ops


class PerImageExposure(torch.nn.Module):
    """delta [num_images, 12]: per image dA (3 x 3, row-major) then db (3), with c' = (I + dA) c + db; zeros = the identity"""

    def __init__(self, num_images: int) -> None:
        super().__init__()
        if int(num_images) < 1:
            raise ValueError(f"exposure compensation needs at least one image; got {num_images}")
        self.delta = torch.nn.Parameter(torch.zeros((int(num_images), 12), dtype=torch.float32))

    @property
    def num_images(self) -> int:
        return int(self.delta.shape[0])

    def get_save_config_dict(self) -> Dict[str, Any]:
        return {"num_images": self.num_images}

    def check_image_ids(self, image_ids: Tensor) -> None:
        """once per dataset, not per call (the kernel clamps ids out of range instead of reading them back)"""
        if image_ids.numel() and not (0 <= int(image_ids.min()) and int(image_ids.max()) < self.num_images):
            raise ValueError(f"image ids must lie in [0, {self.num_images}); got {int(image_ids.min())} .. {int(image_ids.max())}")

    def forward(self, colour: Tensor, target: Tensor, image_ids: Tensor, kind: str = "l1", ray_weight: Optional[Tensor] = None,
                return_corrected: bool = False):
        """(loss, mse[, corrected]) of voxe_hip.ops.exposure_loss under this module's transforms: the photometric loss of
        rendered colours [R,3] against targets [R,3] of the images image_ids [R]; differentiable w.r.t. `colour` and the
        parameters"""
        return _ops.exposure_loss(colour, target, image_ids, self.delta, kind=kind, ray_weight=ray_weight,
                                  return_corrected=return_corrected)

    def corrected(self, colour: Tensor, image_ids: Tensor) -> Tensor:
        """the transformed colours alone, no gradient"""
        with torch.no_grad():
            return _ops.exposure_apply(colour, image_ids, self.delta)

    def regulariser(self) -> Tensor:
        """mean of delta^2 (plain torch: 12 numbers per image): holds the gauge that scene colour and one affine common to all
        images share"""
        return (self.delta * self.delta).mean()

    def extra_repr(self) -> str:
        return f"num_images: {self.num_images}"
