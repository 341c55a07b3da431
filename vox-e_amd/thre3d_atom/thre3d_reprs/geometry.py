"""Geometry views of a VoxelGrid: density-gradient normals, rendered normal maps, and the per-frame buffers of the render tool's
geometry mode (DESIGN.md section 4 "Normals").  Not in the reference.

The normal of a point is n = -grad V / |grad V| of the trilinear pre-activated density VoxelGrid.forward interpolates (toward
lower density: outward on a solid).  A rendered normal is sum_k w_k n(p_k) over the forward's own samples and weights, so it
is not renormalised (|N| <= acc).  All of it runs in voxe_normals.hip; nothing here is differentiable.
"""
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from thre3d_atom.rendering.volumetric.render_interface import Rays
from thre3d_atom.rendering.volumetric.utils.misc import cast_rays, flatten_rays
from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, _check_flat, _render_params
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid
from thre3d_atom.utils.imaging_utils import CameraIntrinsics, CameraPose, to8b
from voxe_hip import ops as _ops


class GeometryFrame(NamedTuple):
    colour: Tensor          # [H,W,3] the colour render (the forward of VolumetricModel.render)
    depth: Tensor           # [H,W,1]
    acc: Tensor             # [H,W,1]
    normal_world: Tensor    # [H,W,3] sum_k w_k n(p_k), world space
    normal_camera: Tensor   # [H,W,3] the same in camera space (R^T N: a surface facing the camera is (0,0,+1))


def render_normals(voxel_grid: VoxelGrid, rays: Rays, render_config: SHVoxGridRenderConfig,
                   rng: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(normals [R,3], depth [R,1], acc [R,1]) of flat rays, with the kernel parameters render_sh_voxel_grid would use for
    (voxel_grid, rays, render_config).  `rng` follows ops.render's rule; pass the rng of a colour render to get the normals
    of exactly its samples."""
    _check_flat(rays)
    params = _render_params(voxel_grid, rays, render_config, attn=False)
    return _ops.render_normals(voxel_grid.voxe_grid_spec(attn=False), params, voxel_grid.densities, rays.origins,
                               rays.directions, rng=rng)


def render_geometry(vol_mod, camera_pose: CameraPose, camera_intrinsics: CameraIntrinsics,
                    num_samples_per_ray: Optional[int] = None) -> GeometryFrame:
    """Colour, depth, acc and normals of one camera of an SH voxel-grid VolumetricModel.  Colour comes from the fused forward
    and normals from the normals kernel, both on ONE jitter stream, so both are integrals over the same samples."""
    grid = vol_mod.thre3d_repr
    overrides = {} if num_samples_per_ray is None else {"num_samples_per_ray": int(num_samples_per_ray)}
    config = vol_mod._update_render_config(vol_mod.render_config, overrides)
    rays = flatten_rays(cast_rays(camera_intrinsics, camera_pose, device=vol_mod.device))
    params = _render_params(grid, rays, config, attn=False)
    spec = grid.voxe_grid_spec(attn=False)
    rng = _ops.resolve_rng(params, None, None)
    with torch.no_grad():
        colour, _, _, _ = _ops.render(spec, params, grid.densities, grid.features, rays.origins, rays.directions,
                                      workspace=grid.voxe_workspace("sh"), rng=rng)
        normal, depth, acc = _ops.render_normals(spec, params, grid.densities, rays.origins, rays.directions, rng=rng)
    H, W = int(camera_intrinsics.height), int(camera_intrinsics.width)
    normal = normal.view(H, W, 3)
    return GeometryFrame(colour.view(H, W, -1), depth.view(H, W, 1), acc.view(H, W, 1), normal,
                         normals_to_camera(normal, camera_pose))


def normals_to_camera(normal: Tensor, pose: CameraPose) -> Tensor:
    """n_cam = R^T n for the pose's camera-to-world rotation R (cast_rays' convention: the camera looks down -z, y is up), on
    the last axis of `normal` [..., 3]"""
    rot = torch.as_tensor(np.asarray(pose.rotation) if not isinstance(pose.rotation, Tensor) else pose.rotation)
    rot = rot.to(device=normal.device, dtype=normal.dtype)
    return normal @ rot     # (R^T n)^T = n^T R


def normals_to_rgb(normal_camera, acc) -> np.ndarray:
    """display colour to8b(0.5 n + 0.5 acc + (1 - acc)): the premultiplied normal map over white (uint8 [..., 3])"""
    n = normal_camera.detach().cpu().numpy() if isinstance(normal_camera, Tensor) else np.asarray(normal_camera)
    a = acc.detach().cpu().numpy() if isinstance(acc, Tensor) else np.asarray(acc)
    return to8b(0.5 * n + 0.5 * a + (1.0 - a))


def vertex_normals(voxel_grid: VoxelGrid, vertices: Tensor) -> Tensor:
    """unit normals n(p) [V,3] at world points [V,3] (e.g. the vertices of thre3d_reprs.mesh.extract_mesh)"""
    spec = voxel_grid.voxe_grid_spec()   # raises exactly where rendering would
    return _ops.query_normals(spec, voxel_grid.densities, vertices.to(voxel_grid.densities.device))
