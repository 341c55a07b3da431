"""Orientation loss of a VoxelGrid on a batch of rays.  Not in the reference.

The regulariser of Ref-NeRF (Verbin et al., CVPR 2022, eq. 11) against "foggy" surfaces -- semi-transparent shells whose density
gradient points away from the camera while they still carry weight, which show as noisy normal maps and as rough or doubled
surfaces in the mesh.  Per ray, with the samples and weights w_k = T_k alpha_k of the colour forward, the unit ray direction u
and the density-gradient normal n_k = -G_k / sqrt(|G_k|^2 + normal_eps^2) of the sample's cell (the field
thre3d_reprs.geometry.render_normals composites),

    L_r = sum_k w_k max(0, n_k . u)^2

and the loss is the (weighted) mean over the rays.  Value and gradient come from one fused kernel call (voxe_orientation.hip);
the gradient reaches the raw densities through the weights and through the normals, the samples and the rays are constants.
"""
import dataclasses
from typing import Optional

from torch import Tensor

from thre3d_atom.rendering.volumetric.render_interface import Rays
from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, _check_flat, _render_params
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid
from thre3d_atom.utils.imaging_utils import CameraBounds
from voxe_hip import ops as _ops


def orientation_loss_on_rays(voxel_grid: VoxelGrid, rays: Rays, render_config: SHVoxGridRenderConfig,
                             ray_weight: Optional[Tensor] = None, normal_eps: float = 1e-2,
                             camera_bounds: Optional[CameraBounds] = None) -> Tensor:
    """Mean orientation loss of flat `rays` through `voxel_grid` with optional weights `ray_weight` [R] (>= 0): a scalar tensor,
    differentiable w.r.t. voxel_grid.densities.  The samples are those render_sh_voxel_grid takes for `render_config` (a fresh
    jitter stream when it perturbs the samples); `camera_bounds` (default: the config's) are the (near, far) the rays are
    sampled with.  `normal_eps` >= 0 guards the normal's length, in the units of the density gradient.  The default 1e-2 is
    a guard, not a tuned value: about 2e-4 of a unit density step across one voxel of a 160^3 grid over [-1.5, 1.5]."""
    _check_flat(rays)
    if camera_bounds is not None:
        render_config = dataclasses.replace(render_config, camera_bounds=camera_bounds)
    params = _render_params(voxel_grid, rays, render_config, attn=False)
    return _ops.orientation_loss(voxel_grid.voxe_grid_spec(attn=False), params, voxel_grid.densities, rays.origins,
                                 rays.directions, ray_weight, normal_eps=normal_eps)
