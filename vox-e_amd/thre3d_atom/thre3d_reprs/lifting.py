"""Lifting 2-D images (masks, colours, one-hot labels) into a VoxelGrid by weighted back-projection, and the region a lifted
mask selects (DESIGN.md section 4.16 "Lifting").  Not in the reference.

For every sample k a camera's rays take through the grid -- exactly the samples and weights w_k = T_k alpha_k of the colour
forward -- and every corner c of the sample's trilinear footprint with gather weight t_c:

    sum_w[c]      += w_k t_c                 how much rendering weight the cameras put on the voxel
    sum_wv[c, ch] += w_k t_c image[ch, pixel]

The ratio sum_wv / sum_w is the weighted vote of the pixels that saw the voxel.  Both sums run in voxe_lift.hip in 64-bit fixed
point (32 fraction bits) through integer atomics, so they are the same bit for bit whatever the order of cameras, rays or
launches -- which a thresholded vote needs.  Nothing here is differentiable.
"""
from typing import Any, Dict, NamedTuple, Optional, Sequence

import torch
from torch import Tensor

from thre3d_atom.rendering.volumetric.utils.misc import cast_rays, flatten_rays
from thre3d_atom.thre3d_reprs.renderers import _render_params
from thre3d_atom.utils.imaging_utils import CameraIntrinsics, CameraPose
from voxe_hip import ops as _ops

LABEL_UNSEEN, LABEL_OUT, LABEL_IN = 0, 1, 2
_ONE = float(1 << 32)     # the fixed-point unit of the sums


class Lifted(NamedTuple):
    sum_wv: Tensor   # [X,Y,Z,C] int64, 32 fraction bits
    sum_w: Tensor    # [X,Y,Z] int64, 32 fraction bits

    def weight(self) -> Tensor:
        """float32 [X,Y,Z]: sum_w * 2^-32 (through float64)"""
        return (self.sum_w.to(torch.float64) / _ONE).to(torch.float32)

    def mean(self, min_weight: float = 0.0) -> Tensor:
        """float32 [X,Y,Z,C]: sum_wv / sum_w (in float64) where weight() > min_weight, NaN elsewhere"""
        ratio = self.sum_wv.to(torch.float64) / self.sum_w.to(torch.float64)[..., None]
        seen = (self.weight() > min_weight)[..., None]
        return torch.where(seen, ratio, torch.full_like(ratio, float("nan"))).to(torch.float32)


def lift_images(vol_mod, poses: Sequence[CameraPose], camera_intrinsics: CameraIntrinsics, images: Tensor,
                **render_overrides) -> Lifted:
    """Lift `images` ([N,C,H,W], C in 1..8, values in [-1, 1], one per pose) into the grid of an SH voxel-grid VolumetricModel:
    one launch per camera, rays cast exactly as accumulate_visibility casts them (lens models included).  The render parameters
    are those render_sh_voxel_grid would use for the model's render config with `render_overrides` applied, except that
    stratified jitter is off unless perturb_sampled_points=True is passed."""
    grid = vol_mod.thre3d_repr
    if images.dim() != 4 or images.shape[0] != len(poses) or not 1 <= images.shape[1] <= 8:
        raise ValueError(f"images must be [N,C,H,W] with N = {len(poses)} poses and C in 1..8; got {tuple(images.shape)}")
    if images.numel() > 0 and not bool((images.abs() <= 1.0).all()):     # (False for NaN too)
        raise ValueError("images must be finite with |v| <= 1")
    overrides = {"perturb_sampled_points": False, **render_overrides}
    config = vol_mod._update_render_config(vol_mod.render_config, overrides)
    spec = grid.voxe_grid_spec(attn=False)
    dens = grid.densities.detach()
    channels = int(images.shape[1])
    lifted = Lifted(torch.zeros((*dens.shape[:3], channels), dtype=torch.int64, device=dens.device),
                    torch.zeros(dens.shape[:3], dtype=torch.int64, device=dens.device))
    for pose, image in zip(poses, images):
        rays = cast_rays(camera_intrinsics, pose, device=vol_mod.device)
        if tuple(rays.image_shape) != tuple(image.shape[1:]):
            raise ValueError(f"image size {tuple(image.shape[1:])} is not the camera's {tuple(rays.image_shape)}")
        rays = flatten_rays(rays)
        params = _render_params(grid, rays, config, attn=False)
        values = image.to(device=dens.device, dtype=torch.float32).permute(1, 2, 0).reshape(-1, channels).contiguous()
        _ops.lift_accumulate_(spec, params, dens, rays.origins, rays.directions, values, lifted.sum_wv, lifted.sum_w)
    return lifted


def region_labels(lifted: Lifted, threshold: float = 0.5, min_weight: float = 1e-3) -> Tensor:
    """uint8 [X,Y,Z]: 0 = unseen (weight <= min_weight), 1 = voted out (channel-0 mean < threshold), 2 = voted in"""
    seen = lifted.weight() > min_weight
    vote = lifted.sum_wv[..., 0].to(torch.float64) / lifted.sum_w.to(torch.float64)
    labels = torch.where(vote < threshold, LABEL_OUT, LABEL_IN).to(torch.uint8)
    return torch.where(seen, labels, torch.zeros_like(labels))


def _grid_geometry(grid) -> Dict[str, Any]:
    spec = grid.voxe_grid_spec(attn=False)
    return {"dims": tuple(int(n) for n in grid.densities.shape[:3]),
            "aabb": tuple(tuple(float(v) for v in axis) for axis in spec.aabb)}


def save_region(path, labels: Tensor, lifted: Lifted, meta: Dict[str, Any]) -> None:
    """Write a region file: a torch.save dict of labels, weight, mean, dims, aabb, threshold, min_weight and num_views.  `meta`
    holds the last five (dims / aabb as _grid_geometry gives them, or a "grid" to take them from)."""
    meta = dict(meta)
    if "grid" in meta:
        meta.update(_grid_geometry(meta.pop("grid")))
    min_weight = float(meta["min_weight"])
    dims = tuple(int(n) for n in meta["dims"])
    if tuple(labels.shape) != dims:
        raise ValueError(f"labels {tuple(labels.shape)} do not match dims {dims}")
    torch.save({"labels": labels.to(device="cpu", dtype=torch.uint8), "weight": lifted.weight().cpu(),
                "mean": lifted.mean(min_weight).cpu(), "dims": dims,
                "aabb": tuple(tuple(float(v) for v in axis) for axis in meta["aabb"]), "threshold": float(meta["threshold"]),
                "min_weight": min_weight, "num_views": int(meta["num_views"])}, path)


def load_region(path, grid) -> Dict[str, Any]:
    """Read a region file back for `grid` (a VoxelGrid); ValueError when its dims or AABB are not the grid's"""
    region = torch.load(path, map_location="cpu", weights_only=False)
    want = _grid_geometry(grid)
    if tuple(region["dims"]) != want["dims"]:
        raise ValueError(f"{path}: region dims {tuple(region['dims'])} are not the grid's {want['dims']}")
    got = torch.tensor(region["aabb"], dtype=torch.float64)
    if got.shape != (3, 2) or not torch.allclose(got, torch.tensor(want["aabb"], dtype=torch.float64), rtol=0.0, atol=1e-6):
        raise ValueError(f"{path}: region AABB {region['aabb']} is not the grid's {want['aabb']}")
    return region


def remove_mask(labels: Tensor, dilate: int = 1) -> Tensor:
    """uint8 [X,Y,Z]: 1 where the label is 1 (voted out) and no label-2 voxel lies within Chebyshev distance `dilate` (0..3,
    through ops.visibility_mask, on the device; dilate = 0 needs no pass: a voxel carries one label).  Unseen voxels -- object
    interiors among them -- are never removed."""
    if int(dilate) == 0:
        return (labels == LABEL_OUT).to(torch.uint8)
    near_in = _ops.visibility_mask((labels == LABEL_IN).to(torch.float32), 0.5, int(dilate))
    return ((labels == LABEL_OUT) & (near_in == 0)).to(torch.uint8)


def prune_region_(voxel_grid, labels: Tensor, dilate: int = 1) -> int:
    """Lower, in place, the density of the voxels of remove_mask(labels, dilate) through prune_voxel_grid_; returns how many
    values changed"""
    from thre3d_atom.thre3d_reprs.visibility import prune_voxel_grid_

    labels = labels.to(voxel_grid.densities.device)
    return prune_voxel_grid_(voxel_grid, remove_mask(labels, dilate) == 0)


def mesh_mask(labels: Tensor, mask: Optional[Tensor] = None) -> Tensor:
    """uint8 [X,Y,Z]: labels != 1, ANDed with `mask` when there is one"""
    keep = (labels != LABEL_OUT).to(torch.uint8)
    return keep if mask is None else keep * (mask.to(keep.device) != 0).to(torch.uint8)
