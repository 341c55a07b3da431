"""Depth supervision of a VoxelGrid on a batch of rays.  Not in the reference.

The ray-termination term of DS-NeRF (Deng et al., CVPR 2022): a sparse structure-from-motion point seen in an image is a depth
measurement D on the ray of its keypoint, with an uncertainty s.  Per ray, with the samples z_k and weights w_k = T_k alpha_k of
the colour forward and dz_k = z_{k+1} - z_k,

    L_r = -sum_k exp(-(z_k - D)^2 / (2 s^2)) dz_k log(w_k + eps)

pulls the distribution of the ray's termination towards a Gaussian around D, and the loss is the (weighted) mean over the rays.
Value and gradient (to the raw densities only) come from one fused kernel call (voxe_depth.hip); the per-sample weights are
never materialised.
"""
import dataclasses
from typing import Optional

import torch
from torch import Tensor

from thre3d_atom.rendering.volumetric.render_interface import Rays
from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, _check_flat, _render_params
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid
from thre3d_atom.utils.imaging_utils import CameraBounds
from voxe_hip import ops as _ops


@torch.no_grad()
def depth_targets_on_rays(rays: Rays, points_xyz: Tensor) -> Tensor:
    """t* = <P - o, d> / <d, d> of world points [R,3] on flat rays: the ray parameter of closest approach, in the units of the
    sample depths z_k (p = o + d z) whatever the length of d.  Detached."""
    _check_flat(rays)
    o, d = rays.origins.detach(), rays.directions.detach()
    p = points_xyz.detach().to(device=o.device, dtype=o.dtype)
    return ((p - o) * d).sum(dim=-1) / (d * d).sum(dim=-1)


def depth_loss_on_rays(voxel_grid: VoxelGrid, rays: Rays, target_depth: Tensor, target_sigma: Tensor,
                       render_config: SHVoxGridRenderConfig, ray_weight: Optional[Tensor] = None, eps: float = 1e-5,
                       camera_bounds: Optional[CameraBounds] = None) -> Tensor:
    """Mean ray-termination loss of flat `rays` through `voxel_grid` towards `target_depth` [R] with widths `target_sigma` [R]
    (> 0) and optional weights `ray_weight` [R] (>= 0): a scalar tensor, differentiable w.r.t. voxel_grid.densities.  The
    samples are those render_sh_voxel_grid takes for `render_config` (a fresh jitter stream when it perturbs the samples);
    `camera_bounds` (default: the config's) are the (near, far) the rays are sampled with."""
    _check_flat(rays)
    if camera_bounds is not None:
        render_config = dataclasses.replace(render_config, camera_bounds=camera_bounds)
    params = _render_params(voxel_grid, rays, render_config, attn=False)
    return _ops.depth_loss(voxel_grid.voxe_grid_spec(attn=False), params, voxel_grid.densities, rays.origins, rays.directions,
                           target_depth, target_sigma, ray_weight, eps=eps)
