"""Per-voxel Fisher information of a VoxelGrid under a set of cameras, the predictive variance of a rendered pixel and the
expected information gain of a candidate camera (DESIGN.md section 4 "Fisher information"; FisherRF, Jiang et al., ECCV 2024).
Not in the reference.

With J_{r,ch}[v] = d colour_{r,ch} / d raw density_v of ray r -- exactly the samples, weights and SH colours of the colour
forward -- the diagonal Fisher information of a set of rays is

    H[v] = sum over (rays, ch) of J_{r,ch}[v]^2                          how well the rays pin the voxel's density down

and, with a prior precision lambda > 0 and P = 1 / (H + lambda) as the (diagonal Laplace) posterior variance of the densities,

    var[r]  = sum_v P[v] sum_ch J_{r,ch}[v]^2                           predictive variance of a pixel, summed over the channels
    gain    = sum_r var[r] = sum_v H_candidate[v] / (H_train[v] + lambda)   expected information gain of a candidate camera

Both run in voxe_fisher.hip.  The square sits inside the sum over rays, so no number of backward passes over several rays gives
H; the kernel carries every voxel's sum along the ray and squares it when the ray leaves the voxel.  Nothing here is
differentiable.  Only the densities get a Fisher term; the features do not.  The kernel always marches the whole ray: the
early termination of the renderer (term_eps of the render parameters) is ignored, so where a render stops early the Fisher
terms of the samples behind the cut are still counted (they carry a transmittance below term_eps).

`prior_precision` defaults to PRIOR_PRECISION_SCALE x H.max() of the grid handed in: an untuned guard against the division by
zero in voxels no ray constrains, not a measured choice."""
import math
from typing import List, NamedTuple, Optional, Sequence

import torch
from torch import Tensor

from thre3d_atom.rendering.volumetric.utils.misc import cast_rays, flatten_rays
from thre3d_atom.thre3d_reprs.renderers import _render_params
from thre3d_atom.utils.imaging_utils import CameraIntrinsics, CameraPose
from voxe_hip import ops as _ops

PRIOR_PRECISION_SCALE = 1e-6


class Selection(NamedTuple):
    indices: List[int]            # the chosen candidates in the order they were chosen
    gains: List[float]            # gain of each at the moment it was chosen
    gains_after: List[float]      # its gain again once its own information is part of the running total
    rounds: List[List[float]]     # per round, the gain of every candidate (NaN for those already chosen)


def _launch_inputs(vol_mod, pose: CameraPose, camera_intrinsics: CameraIntrinsics, render_overrides):
    grid = vol_mod.thre3d_repr
    overrides = {"perturb_sampled_points": False, **render_overrides}
    config = vol_mod._update_render_config(vol_mod.render_config, overrides)
    rays = flatten_rays(cast_rays(camera_intrinsics, pose, device=vol_mod.device))
    params = _render_params(grid, rays, config, attn=False)
    return grid.voxe_grid_spec(attn=False), params, grid.densities.detach(), grid.features.detach(), rays


def default_prior_precision(fisher: Tensor) -> float:
    """PRIOR_PRECISION_SCALE x the largest entry of `fisher`: an untuned guard, not a measured choice"""
    return PRIOR_PRECISION_SCALE * float(fisher.max())


def _resolve_prior(fisher: Tensor, prior_precision: Optional[float]) -> float:
    lam = default_prior_precision(fisher) if prior_precision is None else float(prior_precision)
    if not (lam > 0.0) or not math.isfinite(lam):
        raise ValueError(f"prior_precision must be a finite number above 0 (an all-zero Fisher grid has no default); got {lam}")
    return lam


def accumulate_fisher(vol_mod, poses: Sequence[CameraPose], camera_intrinsics: CameraIntrinsics, **render_overrides) -> Tensor:
    """H [X,Y,Z] float32 of an SH voxel-grid VolumetricModel over `poses`: one launch per camera.  The render parameters are
    those render_sh_voxel_grid would use for the model's render config with `render_overrides` applied, except that stratified
    jitter is off unless perturb_sampled_points=True is passed."""
    dens = vol_mod.thre3d_repr.densities.detach()
    fisher = torch.zeros(dens.shape[:3], dtype=torch.float32, device=dens.device)
    for pose in poses:
        spec, params, dens, feat, rays = _launch_inputs(vol_mod, pose, camera_intrinsics, render_overrides)
        _ops.fisher_rays_(spec, params, dens, feat, rays.origins, rays.directions, fisher=fisher)
    return fisher


def uncertainty_map(vol_mod, pose: CameraPose, camera_intrinsics: CameraIntrinsics, fisher: Tensor,
                    prior_precision: Optional[float] = None, **render_overrides) -> Tensor:
    """[H,W] float32: the predictive variance sum_v J^2 / (fisher[v] + prior_precision) of every pixel of the camera, summed over
    the colour channels; exactly 0 where the ray misses the grid.  One gather pass, no grid is written."""
    lam = _resolve_prior(fisher, prior_precision)
    spec, params, dens, feat, rays = _launch_inputs(vol_mod, pose, camera_intrinsics, render_overrides)
    voxel_var = (1.0 / (fisher.to(device=dens.device, dtype=torch.float32) + lam)).contiguous()
    var = _ops.fisher_rays_(spec, params, dens, feat, rays.origins, rays.directions, voxel_var=voxel_var, want_ray_var=True)
    return var.reshape(int(camera_intrinsics.height), int(camera_intrinsics.width))


def information_gain(vol_mod, pose: CameraPose, camera_intrinsics: CameraIntrinsics, fisher: Tensor,
                     prior_precision: Optional[float] = None, **render_overrides) -> float:
    """sum of uncertainty_map = sum_v H_candidate[v] / (fisher[v] + prior_precision): the expected information gain of taking
    this photograph, given what `fisher` already holds"""
    return float(uncertainty_map(vol_mod, pose, camera_intrinsics, fisher, prior_precision, **render_overrides).double().sum())


def select_next_views(vol_mod, train_poses: Sequence[CameraPose], candidate_poses: Sequence[CameraPose],
                      camera_intrinsics: CameraIntrinsics, k: int, prior_precision: Optional[float] = None,
                      train_fisher: Optional[Tensor] = None, **render_overrides) -> Selection:
    """Greedy next-best-view selection: score every remaining candidate by information_gain against the running Fisher grid
    (the training set's at first), take the best (the lowest index among equal gains), add its own Fisher information to the
    running total, repeat k times.  `prior_precision` defaults to default_prior_precision of the TRAINING set's grid and stays
    fixed over the rounds.  `train_fisher`: the training set's grid when the caller already has it."""
    if k < 0:
        raise ValueError(f"k must be >= 0; got {k}")
    total = accumulate_fisher(vol_mod, train_poses, camera_intrinsics, **render_overrides) if train_fisher is None \
        else train_fisher.clone()
    lam = _resolve_prior(total, prior_precision)
    remaining = list(range(len(candidate_poses)))
    picked, gains, after, rounds = [], [], [], []
    for _ in range(min(int(k), len(remaining))):
        scores = {i: information_gain(vol_mod, candidate_poses[i], camera_intrinsics, total, lam, **render_overrides)
                  for i in remaining}
        best = max(remaining, key=lambda i: (scores[i], -i))
        rounds.append([scores.get(i, float("nan")) for i in range(len(candidate_poses))])
        total = total + accumulate_fisher(vol_mod, [candidate_poses[best]], camera_intrinsics, **render_overrides)
        picked.append(best)
        gains.append(scores[best])
        after.append(information_gain(vol_mod, candidate_poses[best], camera_intrinsics, total, lam, **render_overrides))
        remaining.remove(best)
    return Selection(picked, gains, after, rounds)
