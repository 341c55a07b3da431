"""Distortion loss of a VoxelGrid on a batch of rays (DESIGN.md section 4 "Distortion").  Not in the reference.

The regulariser of mip-NeRF 360 against floaters -- semi-transparent density smeared along rays in front of the surface -- in
the O(S) evaluation of DVGOv2: per ray, with the samples and weights w_k = T_k alpha_k of the colour forward and the sample
intervals [s_k, s_k + d_k] normalised by the camera bounds,

    L_r = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i,    m_k = s_k + d_k / 2

and the loss is the mean over the rays.  Value and gradient (to the raw densities only: the samples are constants, the features
are not involved) come from one fused kernel call (voxe_distortion.hip); the per-sample weights are never materialised.
"""
import dataclasses
from typing import Optional

from torch import Tensor

from thre3d_atom.rendering.volumetric.render_interface import Rays
from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, _check_flat, _render_params
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid
from thre3d_atom.utils.imaging_utils import CameraBounds
from voxe_hip import ops as _ops


def distortion_loss_on_rays(voxel_grid: VoxelGrid, rays: Rays, render_config: SHVoxGridRenderConfig,
                            camera_bounds: Optional[CameraBounds] = None) -> Tensor:
    """Mean distortion loss of flat `rays` through `voxel_grid`: a scalar tensor, differentiable w.r.t. voxel_grid.densities.
    The samples are those render_sh_voxel_grid takes for `render_config` (a fresh jitter stream when it perturbs the samples);
    `camera_bounds` (default: the config's) are the (near, far) the rays are sampled and the depths normalised with."""
    _check_flat(rays)
    if camera_bounds is not None:
        render_config = dataclasses.replace(render_config, camera_bounds=camera_bounds)
    params = _render_params(voxel_grid, rays, render_config, attn=False)
    return _ops.distortion_loss(voxel_grid.voxe_grid_spec(attn=False), params, voxel_grid.densities, rays.origins,
                                rays.directions)
