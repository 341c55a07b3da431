"""PSNR helper (reference: thre3d_atom/utils/metric_utils.py:10-21)."""
import math
from typing import Any

import torch

from thre3d_atom.utils.constants import INFINITY


def mse2psnr(x: Any) -> Any:
    """-10 log10(mse); an exact zero maps to the reference's INFINITY sentinel (tensor) / inf (float)."""
    if isinstance(x, torch.Tensor):
        if float(x) == 0.0:
            return torch.full((1,), INFINITY, dtype=x.dtype, device=x.device)
        return -10.0 * torch.log10(x)
    return math.inf if x == 0.0 else -10.0 * math.log10(x)


SSIM_MIN_SIDE = 11   # the window: smaller images have no valid window


def ssim(image_a: torch.Tensor, image_b: torch.Tensor) -> float:
    """SSIM of two images in [0, 1], [H,W,C] or [C,H,W] with C in 1..4, on the GPU (voxe_hip.ops.ssim: 11 x 11 Gaussian window of
    sigma 1.5, valid windows only, data range 1 -- the number a paper's table reports; not in the reference, which has LPIPS)."""
    from voxe_hip import ops

    if image_a.shape != image_b.shape or image_a.dim() != 3:
        raise ValueError(f"ssim: two images of one shape [H,W,C] or [C,H,W]; got {tuple(image_a.shape)} and {tuple(image_b.shape)}")
    if image_a.shape[-1] > 4 and image_a.shape[0] <= 4:   # channel-first
        image_a, image_b = image_a.permute(1, 2, 0), image_b.permute(1, 2, 0)
    with torch.no_grad():
        mean, _ = ops.ssim(image_a.detach().float().contiguous()[None], image_b.detach().float().contiguous()[None], data_range=1.0)
    return float(mean)
