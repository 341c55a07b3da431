"""Per-voxel visibility of a VoxelGrid under a set of cameras, and pruning by it (DESIGN.md section 4 "Visibility").  Not in the
reference.

For every sample k a camera's rays take through the grid -- exactly the samples, transmittances T_k and weights
w_k = T_k alpha_k of the colour forward -- and every corner c of the sample's trilinear footprint with gather weight t_c:

    max_weight[c] = max over (rays, k) of w_k * t_c      how much the voxel ever mattered to a pixel (Plenoxels / DVGO pruning)
    max_trans[c]  = max over (rays, k) of T_k            how open the best line of sight to the voxel is (1: seen through empty
                                                         space, ~0: occluded, exactly 0: never sampled)

Both run in voxe_visibility.hip as unsigned-integer atomic maxima over the float bits, so the grids are the same bit for bit
whatever the order of cameras, rays or launches.  Nothing here is differentiable.
"""
from pathlib import Path
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from thre3d_atom.rendering.volumetric.utils.misc import cast_rays, flatten_rays
from thre3d_atom.thre3d_reprs.renderers import _render_params
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, density_activation_codes
from thre3d_atom.utils.constants import CAMERA_INTRINSICS, HEMISPHERICAL_RADIUS
from thre3d_atom.utils.imaging_utils import CameraIntrinsics, CameraPose, get_thre360_animation_poses, novel_view_camera
from voxe_hip import abi
from voxe_hip import ops as _ops

# softplus(-20) = 2e-9: below every density the renderer can tell from empty space
_SOFTPLUS_EMPTY = -20.0


class Visibility(NamedTuple):
    max_weight: Tensor   # [X,Y,Z] float32
    max_trans: Tensor    # [X,Y,Z] float32


def accumulate_visibility(vol_mod, poses: Sequence[CameraPose], camera_intrinsics: CameraIntrinsics,
                          **render_overrides) -> Visibility:
    """Visibility grids of an SH voxel-grid VolumetricModel over `poses` (one launch per camera; by the kernel's contract the
    result equals a single multi-view launch bit for bit).  The render parameters are those render_sh_voxel_grid would use for
    the model's render config with `render_overrides` applied, except that stratified jitter is off unless
    perturb_sampled_points=True is passed."""
    grid = vol_mod.thre3d_repr
    overrides = {"perturb_sampled_points": False, **render_overrides}
    config = vol_mod._update_render_config(vol_mod.render_config, overrides)
    spec = grid.voxe_grid_spec(attn=False)
    dens = grid.densities.detach()
    vis = Visibility(*(torch.zeros(dens.shape[:3], dtype=torch.float32, device=dens.device) for _ in range(2)))
    for pose in poses:
        rays = flatten_rays(cast_rays(camera_intrinsics, pose, device=vol_mod.device))
        params = _render_params(grid, rays, config, attn=False)
        _ops.visibility_accumulate_(spec, params, dens, rays.origins, rays.directions, vis.max_weight, vis.max_trans)
    return vis


def visibility_cameras(extra_info: Dict[str, Any], data_path: Optional[str] = None, num_views: int = 36,
                       camera_pitch: float = 60.0) -> Tuple[List[CameraPose], CameraIntrinsics]:
    """The cameras the entry points judge visibility by: the training split of `data_path`, or `num_views` poses of the
    checkpoint's own 360 degree animation path (saved hemispherical radius and intrinsics, as the render tool uses them)."""
    if data_path is not None:
        from thre3d_atom.data.datasets import PosedImagesDataset

        data = PosedImagesDataset(Path(data_path) / "train", Path(data_path) / "train_camera_params.json", rgba_white_bkgd=True)
        return [CameraPose(p[:, :3], p[:, 3:]) for p in data.poses], data.camera_intrinsics
    return (get_thre360_animation_poses(extra_info[HEMISPHERICAL_RADIUS], camera_pitch, num_views),
            novel_view_camera(extra_info[CAMERA_INTRINSICS]))


def empty_raw_density(pre_act: int, post_act: int, density_scale: float) -> float:
    """The raw density E a pruned voxel is lowered to, for the kernel's activation codes: 0 for Identity / ReLU
    post-activation, -20 / density_scale for Softplus (softplus(-20) = 2e-9).  With the abs pre-activation 0 is the only raw
    value that lowers the field, and a Softplus field on top of abs has no empty value at all (softplus(|x|) >= ln 2):
    ValueError."""
    if post_act == abi.ACT_SOFTPLUS:
        if pre_act == abi.ACT_ABS:
            raise ValueError("a grid with abs pre-activation and Softplus post-activation has no empty density value "
                             "(softplus(|x|) >= ln 2): it cannot be pruned")
        return _SOFTPLUS_EMPTY / float(density_scale)
    return 0.0


def pruned_densities(densities: Tensor, keep_mask: Tensor, pre_act: int, post_act: int, density_scale: float) -> Tensor:
    """raw' of prune_voxel_grid_ as a new tensor (any device): raw where keep_mask != 0, else min(raw, E) -- or E = 0 outright
    under the abs pre-activation, where |raw'| <= |raw| is what lowers the field."""
    empty = empty_raw_density(pre_act, post_act, density_scale)
    keep = (keep_mask != 0).reshape(densities.shape)
    if pre_act == abi.ACT_ABS:
        lowered = torch.zeros_like(densities)
    else:
        lowered = torch.minimum(densities, torch.full_like(densities, empty))
    return torch.where(keep, densities, lowered)


def prune_voxel_grid_(voxel_grid: VoxelGrid, keep_mask: Tensor) -> int:
    """Lower, in place, the raw density of every voxel with keep_mask == 0 ([X,Y,Z] or [X,Y,Z,1], bool / uint8) to the field's
    empty value E and never raise one: raw' = min(raw, E), E = 0 for an Identity / ReLU post-activation and -20 / density_scale
    for Softplus; with the abs pre-activation raw' = 0 (Identity / ReLU) and ValueError for Softplus, which has no empty value.
    Features are untouched.  Returns the number of voxels whose value changed.

    Pruning can only remove density: the pre-activated value of no voxel rises, the trilinear interpolant is monotone in its
    corner values (all weights are >= 0) and the post-activations are monotone, so sigma(p) <= its old value at every point."""
    pre, post = density_activation_codes(voxel_grid._density_preactivation, voxel_grid._density_postactivation)
    old = voxel_grid.densities.detach()
    if keep_mask.numel() != old.numel() or tuple(keep_mask.shape[:3]) != tuple(old.shape[:3]):
        raise ValueError(f"keep_mask must be [X,Y,Z]={tuple(old.shape[:3])}; got {tuple(keep_mask.shape)}")
    new = pruned_densities(old, keep_mask.to(old.device), pre, post, float(voxel_grid._expected_density_scale))
    changed = int((new != old).sum())
    with torch.no_grad():
        voxel_grid.densities.copy_(new)
    return changed
