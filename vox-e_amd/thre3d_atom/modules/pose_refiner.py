"""Refine the camera poses of a posed-image dataset against a trained, frozen voxel grid (DESIGN.md section 4 "Ray gradients").
Not in the reference.

What iNeRF does for one photograph and BARF / NeRF-- do while training, here as a stage of its own: the grid is a constant, the
unknowns are six numbers per camera (thre3d_reprs/poses.py).  Each iteration draws a random pixel batch over a cache of cameras,
casts those rays from the corrected poses (ops.cast_rays_from_poses), renders them (vol_mod.render_rays), and steps Adam on the
mean squared error against the pixels; the gradient reaches the deltas through voxe_render_bwd_rays and voxe_cast_rays_bwd."""
from pathlib import Path
from typing import Any, List, Tuple

import torch
from torch import Tensor

from thre3d_atom.modules.volumetric_model import VolumetricModel
from thre3d_atom.rendering.volumetric.utils.misc import sample_random_rays_and_pixels_from_cameras
from thre3d_atom.thre3d_reprs.poses import CameraPoseDeltas, LearnedIntrinsics, write_camera_params
from thre3d_atom.utils.logging import log


def refine_camera_poses(vol_mod: VolumetricModel, dataset: Any, output_dir: Path, num_iterations: int = 200,
                        learning_rate: float = 3e-3, ray_batch_size: int = 32768, image_batch_cache_size: int = 8,
                        split: str = "train", summary_freq: int = 10, intrinsics_learning_rate: float = 0.0,
                        pose_learning: bool = True, learned: dict = None) -> Tuple[Tensor, List[float]]:
    """-> (refined poses [N,3,4] on the model's device, the logged losses).  Writes <output_dir>/refined_<split>_camera_params.json
    in the schema PosedImagesDataset reads.  The grid is frozen for the duration and restored afterwards.
    intrinsics_learning_rate > 0: fx, fy, cx, cy of the dataset's shared camera are learned too (a second parameter group of the
    same Adam) and written back with the poses; the distortion coefficients stay fixed.  pose_learning=False keeps the poses
    exact (only the intrinsics move).  `learned` (a dict) receives the refined PinholeCamera under "camera"."""
    device = vol_mod.device
    data = dataset.to(device)
    intr = data.camera_intrinsics
    grid_params = list(vol_mod.thre3d_repr.parameters())
    was_trainable = [p.requires_grad for p in grid_params]
    for p in grid_params:
        p.requires_grad_(False)
    deltas = CameraPoseDeltas(len(data)).to(device)
    groups = [{"params": list(deltas.parameters()), "lr": learning_rate if pose_learning else 0.0}]
    intrinsics = None
    if intrinsics_learning_rate > 0.0:
        intrinsics = LearnedIntrinsics(intr)   # (a host parameter: thre3d_reprs/poses.py)
        groups.append({"params": list(intrinsics.parameters()), "lr": intrinsics_learning_rate})
    elif not pose_learning:
        raise ValueError("nothing to refine: pose_learning is off and intrinsics_learning_rate is 0")
    optimizer = torch.optim.Adam(groups)
    gen = torch.Generator().manual_seed(torch.initial_seed() % (2 ** 31))
    cache = min(int(image_batch_cache_size), len(data))
    losses: List[float] = []
    try:
        for it in range(1, num_iterations + 1):
            picks = torch.randint(0, len(data), (cache,), generator=gen).to(device)
            rays, pixels = sample_random_rays_and_pixels_from_cameras(
                intr, deltas.apply(data.poses[picks], picks), data.images, ray_batch_size, image_ids=picks, fast_subset=True,
                differentiable=True, intrinsics=None if intrinsics is None else intrinsics.values)
            # (the poses do not move the samples' jitter: a fixed quadrature keeps the loss a smooth function of the pose)
            loss = torch.nn.functional.mse_loss(vol_mod.render_rays(rays, perturb_sampled_points=False).colour, pixels)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            if it % summary_freq == 0 or it in (1, num_iterations):
                losses.append(float(loss.detach()))
                log.info(f"pose refinement iteration {it}: mse {losses[-1]: .6f}")
    finally:
        for p, flag in zip(grid_params, was_trainable):
            p.requires_grad_(flag)
    refined = deltas.apply(data.poses).detach()
    camera = None if intrinsics is None else intrinsics.camera()
    if learned is not None:
        learned["camera"] = camera
    path = write_camera_params(Path(output_dir) / f"refined_{split}_camera_params.json", dataset, refined, camera=camera)
    log.info(f"refined poses of {len(data)} cameras -> {path}"
             + ("" if camera is None else f"; refined intrinsics fx {camera.fx:.3f} fy {camera.fy:.3f} cx {camera.cx:.3f} cy {camera.cy:.3f}"))
    return refined, losses
