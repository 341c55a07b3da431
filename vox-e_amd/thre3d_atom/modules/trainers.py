"""Coarse-to-fine reconstruction of an SH voxel grid from posed images.

Entry point of the reference's thre3d_atom/modules/trainers.py (`train_sh_vox_grid_vol_mod_with_posed_images`
:55-506): `num_stages` stages, the grid doubling each stage (trilinear upsampling, HIP kernel), images
down-sampled by the matching factor, per iteration a random batch of rays over `image_batch_cache_size`
images, L1 loss on the specular render plus (optionally) on the diffuse render, Adam with a per-stage decay.
Rendering and its backward are the fused HIP kernels; the optimiser is the fused HIP Adam.
"""
import time
from functools import partial
from pathlib import Path
from typing import Any, Callable, Optional

import torch
from torch import Tensor

from thre3d_atom.modules.optim import FusedGridAdam, VoxeAdam
from thre3d_atom.modules.testers import test_sh_vox_grid_vol_mod_with_posed_images
from thre3d_atom.modules.volumetric_model import VolumetricModel
from thre3d_atom.rendering.volumetric.utils.misc import (_cast_and_gather, is_general_camera,
                                                          sample_random_patches_and_pixels_from_cameras,
                                                          sample_random_rays_and_pixels_from_cameras)
from thre3d_atom.thre3d_reprs.background import EnvMapBackground
from thre3d_atom.thre3d_reprs.depth import depth_targets_on_rays
from thre3d_atom.thre3d_reprs.exposure import PerImageExposure
from thre3d_atom.thre3d_reprs.poses import CameraPoseDeltas, LearnedIntrinsics, write_camera_params
from thre3d_atom.thre3d_reprs.renderers import _render_params, render_sh_voxel_grid
from thre3d_atom.thre3d_reprs.robust import (check_robust_options, inlier_fractions, robust_loss_on_patches, robust_mask_on_patches,
                                             robust_patch_side)
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, scale_voxel_grid_with_required_output_size
from thre3d_atom.utils.constants import CAMERA_BOUNDS, CAMERA_INTRINSICS, HEMISPHERICAL_RADIUS
from thre3d_atom.utils.imaging_utils import CameraPose, to8b
from thre3d_atom.utils.logging import log
from thre3d_atom.utils.metric_utils import mse2psnr
from thre3d_atom.utils.misc import compute_thre3d_grid_sizes
from voxe_hip import ops as _ops
from voxe_hip.ops import _next_rng


_SSIM_MIN_PATCH = 11   # SSIM's window: a smaller patch has no valid window


def _depth_batch(data: Any, intr: Any, poses_batch: Tensor, picks: Tensor, batch_size: int, sigma_scale: float,
                 min_sigma: float, refine: dict):
    """One batch of depth measurements for the depth term: `batch_size` observations drawn uniformly (with replacement) from the
    sparse points seen by the picked cameras, each cast at the nearest pixel of its keypoint through `poses_batch` (the poses of
    `picks`, refined or not: `refine` holds _cast_and_gather's differentiable / intrinsics arguments).  Returns (rays, D, s,
    omega): the target depth of each ray (depth_targets_on_rays), s = max(sigma_scale * error * D / fx, min_sigma) -- the
    lateral size of the point's reprojection error at that depth, but no narrower than the mean sample spacing, below which
    the Gaussian falls between samples -- and omega = 1 (0 for every ray when the picked cameras see no point).  No host
    synchronisation."""
    sp = data.sparse_points
    device = picks.device
    height, width = int(intr.height), int(intr.width)
    counts = sp.offsets[picks + 1] - sp.offsets[picks]
    ends = torch.cumsum(counts, dim=0)
    total = ends[-1]
    flat = (torch.rand(int(batch_size), device=device) * total).long().clamp_(max=(total - 1).clamp_min(0))
    cam = torch.searchsorted(ends, flat, right=True).clamp_(max=picks.numel() - 1)
    row = (sp.offsets[picks[cam]] + (flat - (ends[cam] - counts[cam]))).clamp_(0, max(sp.xy.shape[0] - 1, 0))
    # (the centre of the top-left pixel is at (0.5, 0.5): the nearest pixel of a keypoint is the floor of its position)
    px = sp.xy[row, 0].floor().long().clamp_(0, width - 1)
    py = sp.xy[row, 1].floor().long().clamp_(0, height - 1)
    rays, _ = _cast_and_gather(intr, poses_batch, data.images, (cam * height + py) * width + px, picks,
                               refine.get("differentiable", False), refine.get("intrinsics"))
    D = depth_targets_on_rays(rays, sp.xyz[row])
    fx = float(getattr(intr, "fx", intr.focal))
    s = (sigma_scale * sp.error[row] * D.clamp_min(0.0) / fx).clamp_min(min_sigma)
    return rays, D, s, (total > 0).to(torch.float32).expand(int(batch_size)).contiguous()


class _PinnedStaging:
    """Host -> device copies of the per-iteration camera picks that do not stall the host: a pageable tensor's .to(device) waits for
    the stream (every kernel of the previous iterations) before it returns, which makes the loop host-paced; a small ring of pinned
    buffers + non_blocking copies does not.  A buffer is reused only once its copy has completed (event per buffer)."""

    def __init__(self, n: int, device, depth: int = 4):
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.bufs = [torch.empty(n, dtype=torch.int64, pin_memory=self.cuda) for _ in range(depth)]
        self.events = [None] * depth
        self.turn = 0

    def to_device(self, fill) -> Tensor:
        i = self.turn % len(self.bufs)
        self.turn += 1
        if self.events[i] is not None:
            self.events[i].synchronize()
        fill(self.bufs[i])
        if not self.cuda:
            return self.bufs[i].clone()
        out = self.bufs[i].to(self.device, non_blocking=True)
        self.events[i] = torch.cuda.Event()
        self.events[i].record()
        return out


def train_sh_vox_grid_vol_mod_with_posed_images(
    vol_mod: VolumetricModel,
    train_dataset: Any,
    output_dir: Path,
    random_initializer: Callable[[Tensor], Tensor] = partial(torch.nn.init.uniform_, a=-1.0, b=1.0),
    test_dataset: Optional[Any] = None,
    image_batch_cache_size: int = 8,
    ray_batch_size: int = 32768,
    num_stages: int = 4,
    num_iterations_per_stage: int = 2000,
    scale_factor: float = 2.0,
    learning_rate: float = 0.03,
    lr_decay_gamma_per_stage: float = 0.1,
    lr_decay_steps_per_stage: int = 1000,
    stagewise_lr_decay_gamma: float = 0.9,
    render_feedback_pose: Optional[CameraPose] = None,
    save_freq: int = 1000,
    test_freq: int = 1000,
    feedback_freq: int = 100,
    summary_freq: int = 10,
    apply_diffuse_render_regularization: bool = True,
    num_workers: int = 4,
    verbose_rendering: bool = True,
    fast_debug_mode: bool = False,
    lpips_weight: float = 0.0,
    fused_grid_step: bool = True,      # addition of this build: FusedGridAdam (gradient stays in the kernels' workspace)
    fused_iteration: bool = True,      # addition of this build: the whole iteration (batch, 2 renders, L1, backward, Adam) as
                                       # ONE library call (voxe_recon_step) -- needs fused_grid_step; same arithmetic
    prefetch_batches: bool = True,     # addition of this build (fused_iteration only): the next iteration's pixel batch and its
                                       # segment tables are assembled while this iteration's backward / Adam run
                                       # (voxe_recon_prefetch); same batches, same arithmetic
    distortion_weight: float = 0.0,    # addition of this build: weight of the distortion loss on the ray batch (mip-NeRF 360's
                                       # regulariser against floaters, thre3d_reprs/distortion.py); 0 = off, nothing changes.
                                       # Above 0 the iteration is not the one-call one (voxe_recon_step has no such term)
    pose_learning_rate: float = 0.0,   # addition of this build: > 0 refines the training cameras while training (BARF / NeRF--):
                                       # one CameraPoseDeltas over all training cameras, shared across the stages, stepped by a
                                       # second Adam at this rate; the refined poses are saved next to the checkpoints.  0 = off,
                                       # nothing changes.  Above 0 the iteration is not the one-call one either
    intrinsics_learning_rate: float = 0.0,   # addition of this build: > 0 also learns fx, fy, cx, cy of the shared camera (in
                                             # full-resolution pixels, scaled to each stage's images) by a second parameter group
                                             # of the pose optimiser; needs pose_learning_rate > 0.  0 = off, nothing changes
    background_resolution: int = 0,    # addition of this build: N > 0 learns an environment-map background of [N, 2N] texels
                                       # behind the grid (thre3d_reprs/background.py), fixed across the stages and saved with the
                                       # checkpoints; needs white_bkgd=False.  0 = off, nothing changes.  Above 0 the iteration
                                       # is not the one-call one either (voxe_recon_step knows no background)
    background_learning_rate: Optional[float] = None,   # Adam rate of the background's texels; None = `learning_rate`, with the
                                                        # same stage decay
    ssim_weight: float = 0.0,          # addition of this build: weight of a D-SSIM term, ssim_weight * (1 - SSIM) on pixel patches
                                       # (voxe_hip.ops.ssim); 0 = off, nothing changes.  Above 0 the batch is
                                       # floor(ray_batch_size / P^2) random P x P patches instead of a random pixel set (the L1
                                       # terms run over the same pixels) and the iteration is not the one-call one either
    ssim_patch_size: int = 32,         # P; a stage whose images are smaller uses min(H, W), and skips the term below 11
    depth_weight: float = 0.0,         # addition of this build: weight of the depth supervision from the dataset's sparse
                                       # structure-from-motion points (DS-NeRF's ray-termination loss, thre3d_reprs/depth.py,
                                       # DESIGN.md 4.19); 0 = off, nothing changes.  Above 0 the dataset must carry
                                       # `sparse_points` and the iteration is not the one-call one either
    depth_ray_batch_size: int = 4096,  # keypoint rays per iteration, drawn from the observations of the picked cameras
    depth_sigma_scale: float = 1.0,    # multiplies the width s_r = error_r * D_r / fx of each measurement
    orientation_weight: float = 0.0,   # addition of this build: weight of the orientation loss on the ray batch (Ref-NeRF's
                                       # regulariser against weight on samples whose density-gradient normal faces away from the
                                       # viewer, thre3d_reprs/orientation.py); 0 = off, nothing changes.  Above 0
                                       # the iteration is not the one-call one either
    orientation_normal_eps: float = 1e-2,   # the guard under the normal's length, in the units of the density gradient.  A guard,
                                            # not a tuned value: about 2e-4 of a unit density step across one voxel of a 160^3
                                            # grid over [-1.5, 1.5]
    exposure_learning_rate: float = 0.0,    # addition of this build: > 0 learns a 3 x 4 affine colour transform per training image
                                            # with the scene (thre3d_reprs/exposure.py): one PerImageExposure over
                                            # all training images, shared across the stages, stepped by its own Adam at this rate
                                            # and saved with the checkpoints; the L1 terms (and the SSIM term) see the transformed
                                            # render.  0 = off, nothing changes.  Above 0 the iteration is not the one-call one
                                            # either, and the images must have 3 channels
    exposure_regularization: float = 1e-3,  # weight of mean(delta^2) on the transforms: a guard against the gauge that scene
                                            # colour and one affine common to all images share.  Untuned: nobody has measured it
    robust_loss: bool = False,              # addition of this build: True replaces the L1 terms by RobustNeRF's trimmed loss
                                            # (thre3d_reprs/robust.py) for captures with transient objects: the
                                            # batch is floor(ray_batch_size / P^2) random P x P patches, a pixel above the
                                            # quantile of the batch's residuals is left out unless its 3 x 3 neighbourhood or its
                                            # patch is mostly inliers, and the mask gets no gradient.  False = off, nothing
                                            # changes.  On, the iteration is not the one-call one either, and ssim_weight must be 0
    robust_patch_size: int = 16,            # P, even, 4..64; a stage whose images are smaller uses min(H, W) rounded down to even,
                                            # and the plain L1 below 4
    robust_inlier_quantile: float = 0.5,    # the quantile of the residuals at and below which a pixel is an inlier
    robust_patch_inlier_fraction: float = 0.6,   # share of forgiven pixels at which a patch's inner half is forgiven as a whole
) -> VolumetricModel:
    if not isinstance(vol_mod.thre3d_repr, VoxelGrid) or vol_mod.render_procedure != render_sh_voxel_grid:
        raise AssertionError("this train procedure needs an SH-based VoxelGrid volumetric model")
    if lpips_weight != 0.0:
        raise NotImplementedError("LPIPS needs the external `lpips` network; not part of this build")
    if ssim_weight < 0.0 or (ssim_weight > 0.0 and ssim_patch_size < _SSIM_MIN_PATCH):
        raise ValueError(f"ssim_weight must not be negative and ssim_patch_size at least {_SSIM_MIN_PATCH} (SSIM's window); got "
                         f"{ssim_weight} and {ssim_patch_size}")
    if depth_weight < 0.0 or (depth_weight > 0.0 and (depth_ray_batch_size < 1 or not depth_sigma_scale > 0.0)):
        raise ValueError(f"depth_weight must not be negative, depth_ray_batch_size at least 1 and depth_sigma_scale positive; got "
                         f"{depth_weight}, {depth_ray_batch_size} and {depth_sigma_scale}")
    if orientation_weight < 0.0 or not (0.0 <= orientation_normal_eps < float("inf")):
        raise ValueError(f"orientation_weight must not be negative and orientation_normal_eps finite and not negative; got "
                         f"{orientation_weight} and {orientation_normal_eps}")
    if exposure_learning_rate < 0.0 or exposure_regularization < 0.0:
        raise ValueError(f"exposure_learning_rate and exposure_regularization must not be negative; got {exposure_learning_rate} "
                         f"and {exposure_regularization}")
    if robust_loss:
        check_robust_options(robust_patch_size, robust_inlier_quantile, robust_patch_inlier_fraction)
        if ssim_weight > 0.0:
            raise ValueError("robust_loss and ssim_weight > 0 do not combine: an SSIM term without the mask would let the "
                             "transient objects back in, and a per-patch-weighted SSIM is not part of this build")
    if depth_weight > 0.0 and getattr(train_dataset, "sparse_points", None) is None:
        from thre3d_atom.data.datasets import SPARSE_POINTS_SUFFIX, sparse_points_path

        config = train_dataset.get_config_dict() if hasattr(train_dataset, "get_config_dict") else {}
        missing = sparse_points_path(config["camera_params_json"]) if "camera_params_json" in config else f"<split>{SPARSE_POINTS_SUFFIX}"
        raise ValueError(f"depth_weight > 0 needs the dataset's sparse points, and {missing} does not exist: "
                         f"tools/convert_from_colmap_text.py writes it next to the camera parameters when the model has a "
                         f"points3D.txt")
    if depth_weight > 0.0 and train_dataset.sparse_points.xy.shape[0] == 0:
        raise ValueError("depth_weight > 0, and the dataset's sparse points hold no observation")
    if background_resolution < 0 or background_resolution == 1:
        raise ValueError(f"background_resolution must be 0 (off) or at least 2; got {background_resolution}")
    if background_resolution > 0:
        if vol_mod.render_config.white_bkgd:
            raise ValueError("background_resolution > 0 needs white_bkgd=False: the white background is already composited by the "
                             "renderer")
        vol_mod.background = EnvMapBackground(background_resolution, 2 * background_resolution).requires_grad_(True)
    device = vol_mod.device
    output_dir = Path(output_dir)
    model_dir = output_dir / "saved_models"
    model_dir.mkdir(exist_ok=True, parents=True)

    grid_sizes = compute_thre3d_grid_sizes(vol_mod.thre3d_repr.grid_dims, num_stages, scale_factor)
    stage_datasets = [train_dataset.downsampled(scale_factor ** (num_stages - 1 - s)).to(device) for s in range(num_stages)]

    exposure_optimizer = None
    if exposure_learning_rate > 0.0:
        if stage_datasets[0].images.shape[1] != 3:
            raise ValueError(f"exposure_learning_rate > 0 needs images of 3 channels (the transform is 3 x 4); got "
                             f"{stage_datasets[0].images.shape[1]}")
        vol_mod.exposure = PerImageExposure(len(train_dataset)).requires_grad_(True)
        # (once per dataset, not per call: a batch's image ids are drawn from these indices, and the kernel clamps)
        vol_mod.exposure.check_image_ids(torch.arange(len(train_dataset)))
        exposure_optimizer = torch.optim.Adam(vol_mod.exposure.parameters(), lr=exposure_learning_rate)

    with torch.no_grad():
        vol_mod.thre3d_repr = scale_voxel_grid_with_required_output_size(vol_mod.thre3d_repr, grid_sizes[0])
        random_initializer(vol_mod.thre3d_repr.densities)
        random_initializer(vol_mod.thre3d_repr.features)

    extra_info = {CAMERA_BOUNDS: train_dataset.camera_bounds, CAMERA_INTRINSICS: train_dataset.camera_intrinsics,
                  HEMISPHERICAL_RADIUS: train_dataset.get_hemispherical_radius_estimate()}
    # rendered feedback (trainers.py:164-175,409-432 of the reference): the given pose, else the first held-out / training
    # view; stills go to training_logs/rendered_output as [specular | diffuse] PNGs
    render_dir = output_dir / "training_logs" / "rendered_output"
    if not fast_debug_mode:
        render_dir.mkdir(exist_ok=True, parents=True)
    if render_feedback_pose is None:
        first = (test_dataset if test_dataset is not None else train_dataset).poses[0].to(device)
        render_feedback_pose = CameraPose(rotation=first[:, :3], translation=first[:, 3:])

    def rendered_feedback(step: int) -> None:
        from PIL import Image

        intr_full = train_dataset.camera_intrinsics
        views = [vol_mod.render(render_feedback_pose, intr_full, gpu_render=True, verbose=verbose_rendering,
                                render_diffuse=diffuse).colour for diffuse in (False, True)]
        Image.fromarray(to8b(torch.cat(views, dim=1).cpu().numpy())).save(render_dir / f"default_{step}.png")

    pose_deltas = pose_optimizer = learned_intrinsics = None
    if intrinsics_learning_rate > 0.0 and not pose_learning_rate > 0.0:
        raise ValueError("intrinsics_learning_rate > 0 needs pose_learning_rate > 0 (the intrinsics are a parameter group of the "
                         "pose optimiser)")
    if pose_learning_rate > 0.0:
        pose_deltas = CameraPoseDeltas(len(train_dataset)).to(device)
        groups = [{"params": list(pose_deltas.parameters()), "lr": pose_learning_rate}]
        if intrinsics_learning_rate > 0.0:
            learned_intrinsics = LearnedIntrinsics(train_dataset.camera_intrinsics)   # (a host parameter)
            groups.append({"params": list(learned_intrinsics.parameters()), "lr": intrinsics_learning_rate})
        pose_optimizer = torch.optim.Adam(groups)

    def save_refined_poses() -> None:
        refined = pose_deltas.apply(train_dataset.poses.to(device)).detach()
        camera = None if learned_intrinsics is None else learned_intrinsics.camera()
        if camera is not None and hasattr(train_dataset, "get_config_dict"):
            # (a PosedImagesDataset's file holds the camera of the images on disk, before its own downsample factor)
            factor = float(train_dataset.get_config_dict().get("downsample_factor", 1.0))
            if factor != 1.0:
                first = next(iter(train_dataset.camera_parameters.values()))["intrinsic"]
                camera = type(camera)(int(first["height"]), int(first["width"]), camera.fx * factor, camera.fy * factor,
                                      camera.cx * factor, camera.cy * factor, camera.distortion)
        write_camera_params(model_dir / "refined_train_camera_params.json", train_dataset, refined, camera=camera)

    global_step, trained = 0, 0.0
    gen = torch.Generator().manual_seed(torch.initial_seed() % (2 ** 31))
    for stage in range(1, num_stages + 1):
        data = stage_datasets[stage - 1]
        intr = data.camera_intrinsics
        lr = learning_rate * (stagewise_lr_decay_gamma ** (stage - 1))
        if fused_grid_step:
            optimizer = FusedGridAdam(vol_mod.thre3d_repr, lr=lr, betas=(0.9, 0.999))
        else:
            optimizer = VoxeAdam([{"params": vol_mod.thre3d_repr.parameters(), "lr": lr}], betas=(0.9, 0.999))
        scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=lr_decay_gamma_per_stage)
        background_optimizer = background_scheduler = None
        if background_resolution > 0:
            # a second Adam on the texels (their state does not survive a stage, like the grid's: the reference builds a fresh
            # optimiser per stage)
            background_lr = (learning_rate if background_learning_rate is None else background_learning_rate) \
                * (stagewise_lr_decay_gamma ** (stage - 1))
            background_optimizer = VoxeAdam([{"params": vol_mod.background.parameters(), "lr": background_lr}], betas=(0.9, 0.999))
            background_scheduler = torch.optim.lr_scheduler.ExponentialLR(background_optimizer, gamma=lr_decay_gamma_per_stage)
        # (the one-call iteration reads RGB targets straight from the image stack)
        one_call = fused_grid_step and fused_iteration and data.images.shape[1] == 3 and data.images.is_contiguous()
        if distortion_weight > 0.0:
            if one_call and stage == 1:
                log.info("distortion_weight > 0: the iterations render, add the term and step separately (no one-call iteration)")
            one_call = False
        if pose_deltas is not None:
            if one_call and stage == 1:
                log.info("pose_learning_rate > 0: the iterations cast, render and step separately (no one-call iteration)")
            one_call = False
        if background_resolution > 0:
            if one_call and stage == 1:
                log.info("background_resolution > 0: the iterations render, composite the background and step separately (no "
                         "one-call iteration)")
            one_call = False
        if depth_weight > 0.0:
            if one_call and stage == 1:
                log.info("depth_weight > 0: the iterations render, cast the keypoint rays, add the term and step separately (no "
                         "one-call iteration)")
            one_call = False
        if orientation_weight > 0.0:
            if one_call and stage == 1:
                log.info("orientation_weight > 0: the iterations render, add the term and step separately (no one-call iteration)")
            one_call = False
        if exposure_optimizer is not None:
            if one_call and stage == 1:
                log.info("exposure_learning_rate > 0: the iterations render, take the losses under the per-image colour transforms "
                         "and step separately (no one-call iteration)")
            one_call = False
        patch = 0   # side of this stage's SSIM patches; 0: the term is off and the batch is the random pixel set
        if ssim_weight > 0.0:
            if one_call and stage == 1:
                log.info("ssim_weight > 0: the iterations draw pixel patches, render, add the term and step separately (no one-call "
                         "iteration)")
            one_call = False
            patch = min(int(ssim_patch_size), int(intr.height), int(intr.width))
            if patch < _SSIM_MIN_PATCH:
                log.info(f"stage {stage}: images [{intr.height} x {intr.width}] are smaller than SSIM's {_SSIM_MIN_PATCH} x "
                         f"{_SSIM_MIN_PATCH} window: no SSIM term in this stage")
                patch = 0
            elif patch * patch > ray_batch_size:
                raise ValueError(f"ray_batch_size {ray_batch_size} holds no {patch} x {patch} patch")
        robust_side = 0   # side of this stage's robust-loss patches; 0: the L1 terms are the plain ones
        if robust_loss:
            if one_call and stage == 1:
                log.info("robust_loss: the iterations draw pixel patches, render, take the trimmed L1 and step separately (no "
                         "one-call iteration)")
            one_call = False
            robust_side = robust_patch_side(robust_patch_size, intr.height, intr.width)
            if robust_side == 0:
                log.info(f"stage {stage}: images [{intr.height} x {intr.width}] hold no 4 x 4 patch: the plain L1 in this stage")
            elif robust_side * robust_side > ray_batch_size:
                raise ValueError(f"ray_batch_size {ray_batch_size} holds no {robust_side} x {robust_side} patch")
        if is_general_camera(intr):
            # voxe_recon_step casts (height, width, focal) cameras only: fx != fy, an off-centre principal point or a lens model
            # takes the composed iteration with voxe_cast_rays_camera
            if one_call and stage == 1:
                log.info("general camera (fx, fy, cx, cy, distortion): the iterations cast with voxe_cast_rays_camera, render and "
                         "step separately (no one-call iteration)")
            one_call = False
        stage_factor = float(scale_factor ** (num_stages - stage))   # (the factor stage_datasets were downsampled by)
        fused_losses = torch.zeros(4, dtype=torch.float32, device=device)
        log.info(f"stage {stage}: grid {vol_mod.thre3d_repr.grid_dims}, images [{intr.height} x {intr.width}], lr {lr:.4f}")

        staging = _PinnedStaging(min(image_batch_cache_size, len(data)), device)

        def draw_batch():
            # a cache of `image_batch_cache_size` random views; the batch is a random subset of ALL their pixels
            # (cast + collate + randperm of the reference, restricted to the pixels that are kept)
            picks = staging.to_device(lambda out: torch.randint(0, len(data), (out.numel(),), generator=gen, out=out))
            if not one_call:
                return picks, None, None
            return picks, data.poses[picks].contiguous(), _next_rng()

        try:
            # (the one-call loop draws an iteration's cameras / streams one iteration AHEAD -- before the previous step is
            #  enqueued -- whether or not the hint below is given: the batches do not depend on `prefetch_batches`)
            upcoming = draw_batch()
            for it in range(1, num_iterations_per_stage + 1):
                t0 = time.perf_counter()
                picks, poses_it, rng_it = upcoming
                upcoming = draw_batch() if it < num_iterations_per_stage else None
                if one_call:
                    # ONE library call: random pixel batch over the picked cameras -> specular (+ diffuse) render -> L1 ->
                    # backward -> Adam with this optimiser's state and learning rate (voxe_recon_step).  The loss values stay
                    # on the device until they are logged.
                    params_it = _render_params(vol_mod.thre3d_repr, None, vol_mod.render_config, attn=False)
                    batch_it = min(ray_batch_size, picks.numel() * intr.height * intr.width)
                    optimizer.reconstruction_step(params_it, intr.height, intr.width, float(intr.focal), poses_it, picks, data.images,
                                                  batch_it, apply_diffuse_render_regularization, fused_losses, rng_it)
                    if prefetch_batches and upcoming is not None:
                        optimizer.reconstruction_prefetch(params_it, intr.height, intr.width, float(intr.focal), upcoming[1], upcoming[0],
                                                          data.images, batch_it, apply_diffuse_render_regularization, fused_losses,
                                                          upcoming[2])
                else:
                    poses_batch = data.poses[picks]
                    refine = {}
                    if pose_deltas is not None:
                        # (the rays carry the render's gradient back to the deltas of the picked cameras)
                        poses_batch, refine = pose_deltas.apply(poses_batch, picks), {"differentiable": True}
                        if learned_intrinsics is not None:
                            refine["intrinsics"] = learned_intrinsics.values / stage_factor
                    exposed = exposure_optimizer is not None
                    if patch or robust_side:
                        # (the SSIM term and the robust loss exclude each other: one of the two sides is 0)
                        side = patch or robust_side
                        num_patches = ray_batch_size // (side * side)
                        rays_batch, pixels_batch, *ids_batch = sample_random_patches_and_pixels_from_cameras(
                            intr, poses_batch, data.images, num_patches, side, image_ids=picks, **refine, return_image_ids=exposed)
                    else:
                        rays_batch, pixels_batch, *ids_batch = sample_random_rays_and_pixels_from_cameras(
                            intr, poses_batch, data.images, ray_batch_size, image_ids=picks, **refine,
                            # (sorting the batch by (camera, row, column) helps the ray-ordered gather of small batches; batches of
                            #  16384+ rays take the space-binned render, which does not care about the order: skip the sort)
                            memory_order=ray_batch_size < 16384, fast_subset=True, return_image_ids=exposed)
                    specular = vol_mod.render_rays(rays_batch).colour
                    robust_weight = robust_mask = None
                    if robust_side and exposed:
                        # (the mask of the colours as the loss sees them, a constant; then the loss under the transforms with the
                        #  mask as per-ray weights: its normalisation, 1 / 3R sum omega, is the robust loss's)
                        corrected = vol_mod.exposure.corrected(specular.detach(), ids_batch[0])
                        robust_mask, robust_info = robust_mask_on_patches(corrected, pixels_batch, num_patches, robust_side,
                                                                          robust_inlier_quantile, robust_patch_inlier_fraction)
                        robust_weight = robust_mask.view(-1).to(torch.float32)
                    if exposed:
                        # (value, mse and both gradients of the L1 under each ray's image transform in one call)
                        loss, mse = vol_mod.exposure(specular, pixels_batch, ids_batch[0], ray_weight=robust_weight)
                        psnr = mse2psnr(mse)
                    elif robust_side:
                        # (value, the unmasked mse, the mask and the gradient in one call)
                        loss, mse, robust_mask, robust_info = robust_loss_on_patches(
                            specular, pixels_batch, num_patches, robust_side, robust_inlier_quantile, robust_patch_inlier_fraction)
                        psnr = mse2psnr(mse)
                    else:
                        loss = torch.nn.functional.l1_loss(specular, pixels_batch)
                        psnr = mse2psnr(torch.nn.functional.mse_loss(specular.detach(), pixels_batch))
                    if apply_diffuse_render_regularization:
                        diffuse = vol_mod.render_rays(rays_batch, render_diffuse=True).colour
                        if exposed:
                            loss = loss + vol_mod.exposure(diffuse, pixels_batch, ids_batch[0], ray_weight=robust_weight)[0]
                        elif robust_side:
                            # (the diffuse term under the specular term's mask)
                            loss = loss + robust_loss_on_patches(diffuse, pixels_batch, num_patches, robust_side,
                                                                 mask=robust_mask)[0]
                        else:
                            loss = loss + torch.nn.functional.l1_loss(diffuse, pixels_batch)
                    if exposed and exposure_regularization > 0.0:
                        loss = loss + exposure_regularization * vol_mod.exposure.regulariser()
                    if distortion_weight > 0.0:
                        # (under FusedGridAdam the renders' gradient stays in the workspace and this term's arrives as
                        #  densities.grad, which step() adds; under VoxeAdam plain autograd sums both)
                        distortion = vol_mod.distortion_loss(rays_batch)
                        loss = loss + distortion_weight * distortion
                    if depth_weight > 0.0:
                        # (keypoint rays of the picked cameras, through the same poses and intrinsics as the batch's; the
                        #  gradient reaches the densities as the distortion term's does)
                        config = vol_mod.render_config
                        bounds = config.camera_bounds
                        depth_rays, depth_target, depth_sigma, depth_omega = _depth_batch(
                            data, intr, poses_batch, picks, depth_ray_batch_size, depth_sigma_scale,
                            (bounds.far - bounds.near) / config.num_samples_per_ray, refine)
                        depth = vol_mod.depth_loss(depth_rays, depth_target, depth_sigma, ray_weight=depth_omega)
                        loss = loss + depth_weight * depth
                    if orientation_weight > 0.0:
                        # (on the ray batch; the gradient reaches the densities as the distortion term's does)
                        orientation = vol_mod.orientation_loss(rays_batch, normal_eps=orientation_normal_eps)
                        loss = loss + orientation_weight * orientation
                    if patch:
                        # (the batch is patch-major, row, column: the render's colour viewed as channel-last patches)
                        shape = (num_patches, patch, patch, specular.shape[-1])
                        # (under exposure compensation the term sees the transformed colours, like the L1 terms)
                        seen = _ops.exposure_apply(specular, ids_batch[0], vol_mod.exposure.delta) if exposed else specular
                        ssim, _ = _ops.ssim(seen.view(shape), pixels_batch.contiguous().view(shape))
                        loss = loss + ssim_weight * (1.0 - ssim)
                    optimizer.zero_grad()
                    if pose_optimizer is not None:
                        pose_optimizer.zero_grad()
                    if background_optimizer is not None:
                        background_optimizer.zero_grad()
                    if exposure_optimizer is not None:
                        exposure_optimizer.zero_grad()
                    loss.backward()
                    optimizer.step()
                    if pose_optimizer is not None:
                        pose_optimizer.step()
                    if background_optimizer is not None:
                        background_optimizer.step()
                    if exposure_optimizer is not None:
                        exposure_optimizer.step()
                global_step += 1
                trained += time.perf_counter() - t0
                if global_step % summary_freq == 0 or it in (1, num_iterations_per_stage):
                    if one_call:
                        l1_spec, mse_spec, l1_diff, _ = fused_losses.tolist()
                        loss = torch.tensor(l1_spec + (l1_diff if apply_diffuse_render_regularization else 0.0))
                        psnr = mse2psnr(torch.tensor(mse_spec))
                    log.info(f"Stage: {stage} Global Iteration: {global_step} Stage Iteration: {it} "
                             f"loss: {float(loss.detach()): .3f} psnr: {float(psnr): .3f}"
                             + (f" distortion: {float(distortion.detach()): .6f}" if distortion_weight > 0.0 else "")
                             + (f" ssim: {float(ssim.detach()): .4f}" if patch else "")
                             + (f" depth: {float(depth.detach()): .6f}" if depth_weight > 0.0 else "")
                             + (f" orientation: {float(orientation.detach()): .6f}" if orientation_weight > 0.0 else "")
                             + (" inliers: {:.3f} / {:.3f} / {:.3f}".format(
                                 *inlier_fractions(robust_info, num_patches * robust_side * robust_side)) if robust_side else ""))
                if it % lr_decay_steps_per_stage == 0:
                    scheduler.step()
                    if background_scheduler is not None:
                        background_scheduler.step()
                last = it == num_iterations_per_stage
                if not fast_debug_mode and (global_step % feedback_freq == 0 or it == 1 or last):
                    log.info(f"TIME CHECK: time spent actually training till now: {trained:.1f} s")
                    rendered_feedback(global_step)
                if test_dataset is not None and not fast_debug_mode and (global_step % test_freq == 0 or last):
                    test_sh_vox_grid_vol_mod_with_posed_images(vol_mod, test_dataset, parallel_rays_chunk_size=ray_batch_size,
                                                               global_step=global_step)
                if it % save_freq == 0 and not fast_debug_mode:
                    torch.save(vol_mod.get_save_info(extra_info), model_dir / f"model_stage_{stage}_iter_{it}.pth")
                    if pose_deltas is not None:
                        save_refined_poses()
        finally:
            if fused_grid_step:   # leave the deferred-gradient mode even when the loop raised (renders would return no .grad)
                optimizer.detach()
        if stage != num_stages:
            with torch.no_grad():
                vol_mod.thre3d_repr = scale_voxel_grid_with_required_output_size(vol_mod.thre3d_repr, grid_sizes[stage])
    torch.save(vol_mod.get_save_info(extra_info), model_dir / "model_final.pth")
    if pose_deltas is not None:
        save_refined_poses()
    log.info(f"Training complete; time spent actually training: {trained:.1f} s")
    return vol_mod
