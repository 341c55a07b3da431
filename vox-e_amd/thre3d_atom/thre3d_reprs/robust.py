"""Robust photometric loss for captures with transient objects (new in this build).

Something is in some photographs and not in others: a passer-by, a car, the photographer's shadow.  A plain L1 treats those
pixels like any others and the grid explains them with view-dependent floaters, because that is what the data asks for.
RobustNeRF (Sabour et al. 2023) trims the loss instead: a pixel whose residual is above a quantile of the batch's residuals is
an outlier, an outlier is forgiven when its 3 x 3 neighbourhood or the patch around it is mostly inliers, and the mask gets no
gradient (voxe_robust_fwd_bwd).  The batch is therefore drawn as pixel patches, as it is for the SSIM term."""
from typing import Dict, Optional, Tuple

from torch import Tensor

from voxe_hip import ops as _ops

MIN_PATCH, MAX_PATCH = 4, 64


def check_robust_options(patch_size: int, inlier_quantile: float, patch_inlier_fraction: float) -> None:
    """the trainer's options, before any work"""
    if int(patch_size) != patch_size or patch_size % 2 or not MIN_PATCH <= patch_size <= MAX_PATCH:
        raise ValueError(f"robust_patch_size must be an even integer in {MIN_PATCH}..{MAX_PATCH}; got {patch_size}")
    if not 0.0 < inlier_quantile <= 1.0:
        raise ValueError(f"robust_inlier_quantile must lie in (0, 1]; got {inlier_quantile}")
    if not 0.0 <= patch_inlier_fraction <= 1.0:
        raise ValueError(f"robust_patch_inlier_fraction must lie in [0, 1]; got {patch_inlier_fraction}")


def robust_patch_side(patch_size: int, height: int, width: int) -> int:
    """side of the patches drawn from images of [height x width]: min(patch_size, height, width) rounded down to even; 0 when
    that is below 4 (no robust loss at this size)"""
    side = min(int(patch_size), int(height), int(width)) // 2 * 2
    return side if side >= MIN_PATCH else 0


def as_patches(colour: Tensor, num_patches: int, side: int) -> Tensor:
    """a patch-major batch [num_patches * side^2, C] (patch, row, column: the samplers' order) viewed as [N,P,P,C]"""
    return colour.contiguous().view(num_patches, side, side, colour.shape[-1])


def robust_loss_on_patches(colour: Tensor, pixels: Tensor, num_patches: int, side: int, inlier_quantile: float = 0.5,
                           patch_inlier_fraction: Optional[float] = 0.6, mask: Optional[Tensor] = None,
                           kind: str = "l1") -> Tuple[Tensor, Tensor, Tensor, Dict]:
    """voxe_hip.ops.robust_loss of a render's colour [R,C] against the photographs' pixels [R,C], R = num_patches * side^2 in the
    samplers' patch-major order: (loss, mse, mask [N,P,P] uint8, info); with `mask` another call's mask is applied instead"""
    return _ops.robust_loss(as_patches(colour, num_patches, side), as_patches(pixels.detach(), num_patches, side),
                            inlier_quantile=inlier_quantile, patch_inlier_fraction=patch_inlier_fraction, kind=kind, mask=mask)


def robust_mask_on_patches(colour: Tensor, pixels: Tensor, num_patches: int, side: int, inlier_quantile: float = 0.5,
                           patch_inlier_fraction: Optional[float] = 0.6) -> Tuple[Tensor, Dict]:
    """the mask alone (voxe_hip.ops.robust_mask), for a loss that takes it as per-ray weights: (mask [N,P,P] uint8, info)"""
    return _ops.robust_mask(as_patches(colour.detach(), num_patches, side), as_patches(pixels.detach(), num_patches, side),
                            inlier_quantile=inlier_quantile, patch_inlier_fraction=patch_inlier_fraction)


def inlier_fractions(info: Dict, num_pixels: int) -> Tuple[float, float, float]:
    """(raw inliers, forgiven pixels, final mask) as fractions of the batch's pixels; reads the counts back from the device"""
    a, c, w = (int(v) for v in info["stats"].tolist())
    return a / num_pixels, c / num_pixels, w / num_pixels
