#!/usr/bin/env python3
"""Reconstruct an SH voxel grid (ReLU / softplus field) from posed images (entry point kept from the
reference's train_sh_based_voxel_grid_with_posed_images.py:142-267; same option names for the options kept)."""
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.data.datasets import PosedImagesDataset  # noqa: E402
from thre3d_atom.modules.trainers import train_sh_vox_grid_vol_mod_with_posed_images  # noqa: E402
from thre3d_atom.modules.volumetric_model import VolumetricModel  # noqa: E402
from thre3d_atom.rendering.volumetric.utils.misc import compute_expected_density_scale_for_relu_field_grid  # noqa: E402
from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelGridLocation, VoxelSize  # noqa: E402
from thre3d_atom.utils.constants import NUM_COLOUR_CHANNELS  # noqa: E402
from thre3d_atom.utils.cli_compat import accepted_options, report_unused  # noqa: E402
from thre3d_atom.utils.logging import log  # noqa: E402
from thre3d_atom.utils.misc import log_config_to_disk  # noqa: E402

# options of the reference's script that this build has no use for (the dataset is cached on the GPU: no loader workers)
COMPAT_ONLY = [("--num_workers", click.INT, 4, 1)]


def density_activations(use_relu_field: bool, use_softplus_field: bool, grid_world_size):
    """Activation table of the reference CLI (:177-200).  NB: there the `else` of the softplus test also
    overrides the ReLU branch, so (relu=True, softplus=False) yields the abs/Identity field; reproduced."""
    scale = compute_expected_density_scale_for_relu_field_grid(grid_world_size)
    if use_softplus_field:
        return dict(density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.Softplus(), expected_density_scale=scale)
    return dict(density_preactivation=torch.abs, density_postactivation=torch.nn.Identity(), expected_density_scale=1.0)


@click.command()
@click.option("-d", "--data_path", type=click.Path(file_okay=False, dir_okay=True), required=True)
@click.option("-o", "--output_path", type=click.Path(file_okay=False, dir_okay=True), required=True)
@click.option("--data_downsample_factor", type=click.FloatRange(min=1.0), default=1.0, show_default=True)
@click.option("--grid_dims", type=click.INT, nargs=3, default=(160, 160, 160), show_default=True)
@click.option("--grid_location", type=click.FLOAT, nargs=3, default=(0.0, 0.0, 0.0), show_default=True)
@click.option("--grid_world_size", type=click.FLOAT, nargs=3, default=(3.0, 3.0, 3.0), show_default=True)
@click.option("--sh_degree", type=click.INT, default=0, show_default=True)
@click.option("--use_relu_field", type=click.BOOL, default=True, show_default=True)
@click.option("--use_softplus_field", type=click.BOOL, default=True, show_default=True)
@click.option("--white_bkgd", type=click.BOOL, default=True, show_default=True)
@click.option("--ray_batch_size", type=click.INT, default=32768, show_default=True)
@click.option("--train_num_samples_per_ray", type=click.INT, default=256, show_default=True)
@click.option("--render_num_samples_per_ray", type=click.INT, default=1024, show_default=True)
@click.option("--num_stages", type=click.INT, default=4, show_default=True)
@click.option("--num_iterations_per_stage", type=click.INT, default=500, show_default=True)
@click.option("--scale_factor", type=click.FLOAT, default=2.0, show_default=True)
@click.option("--learning_rate", type=click.FLOAT, default=0.03, show_default=True)
@click.option("--lr_decay_steps_per_stage", type=click.INT, default=400, show_default=True)
@click.option("--lr_decay_gamma_per_stage", type=click.FLOAT, default=0.1, show_default=True)
@click.option("--stagewise_lr_decay_gamma", type=click.FLOAT, default=0.9, show_default=True)
@click.option("--apply_diffuse_render_regularization", type=click.BOOL, default=True)
@click.option("--optimized_sampling", type=click.BOOL, default=False, show_default=True)
@click.option("--linear_disparity_sampling", type=click.BOOL, default=False, show_default=True)
@click.option("--fast_debug_mode", type=click.BOOL, default=False, show_default=True)
@click.option("--separate_train_test_folders", type=click.BOOL, default=True, show_default=True,
              help="<data_path>/train + train_camera_params.json (else <data_path>/images + camera_params.json)")
@click.option("--normalize_scene_scale", type=click.BOOL, default=False, show_default=True)
@click.option("--parallel_rays_chunk_size", type=click.INT, default=32768, show_default=True)
@click.option("--save_frequency", type=click.INT, default=250, show_default=True)
@click.option("--test_frequency", type=click.INT, default=250, show_default=True)
@click.option("--feedback_frequency", type=click.INT, default=100, show_default=True)
@click.option("--summary_frequency", type=click.INT, default=50, show_default=True)
@click.option("--verbose_rendering", type=click.BOOL, default=False, show_default=True)
@click.option("--lpips_weight", type=click.FLOAT, default=0.0, show_default=True)
@click.option("--distortion_weight", type=click.FloatRange(min=0.0), default=0.0, show_default=True,
              help="weight of the distortion loss on the ray batch (against floaters); 0 = off")
@click.option("--pose_learning_rate", type=click.FloatRange(min=0.0), default=0.0, show_default=True,
              help="> 0: refine the training cameras while training (Adam at this rate on per-camera pose deltas); 0 = off")
@click.option("--intrinsics_learning_rate", type=click.FloatRange(min=0.0), default=0.0, show_default=True,
              help="> 0 (with --pose_learning_rate): also learn fx, fy, cx, cy of the shared camera at this rate; 0 = off")
@click.option("--background_resolution", type=click.IntRange(min=0), default=0, show_default=True,
              help="N > 0: learn an environment-map background of N x 2N texels behind the grid (needs --white_bkgd False); 0 = off")
@click.option("--background_learning_rate", type=click.FloatRange(min=0.0), default=None,
              help="Adam rate of the background's texels (default: --learning_rate)")
@click.option("--ssim_weight", type=click.FloatRange(min=0.0), default=0.0, show_default=True,
              help="weight of a D-SSIM term, weight * (1 - SSIM), on random pixel patches instead of a random pixel set; 0 = off")
@click.option("--ssim_patch_size", type=click.IntRange(min=11), default=32, show_default=True,
              help="side of the SSIM term's pixel patches (a stage with smaller images uses its smaller side)")
@click.option("--depth_weight", type=click.FloatRange(min=0.0), default=0.0, show_default=True,
              help="weight of the depth supervision from the sparse points the COLMAP importer wrote (<split>_sparse_points.npz); "
                   "0 = off")
@click.option("--depth_ray_batch_size", type=click.IntRange(min=1), default=4096, show_default=True,
              help="keypoint rays of the depth term per iteration")
@click.option("--depth_sigma_scale", type=click.FloatRange(min=0.0, min_open=True), default=1.0, show_default=True,
              help="multiplies the width of each depth measurement (its reprojection error at its depth)")
@click.option("--orientation_weight", type=click.FloatRange(min=0.0), default=0.0, show_default=True,
              help="weight of the orientation loss on each ray batch (penalises weight on samples whose normal faces away from "
                   "the viewer); 0 = off")
@click.option("--orientation_normal_eps", type=click.FloatRange(min=0.0), default=1e-2, show_default=True,
              help="guard under the length of the density gradient in the orientation loss, in the gradient's units")
@click.option("--exposure_learning_rate", type=click.FloatRange(min=0.0), default=0.0, show_default=True,
              help="Adam rate of a learned 3x4 affine colour transform per training image (exposure / white-balance "
                   "compensation, applied inside the loss only; needs RGB images); 0 = off")
@click.option("--exposure_regularization", type=click.FloatRange(min=0.0), default=1e-3, show_default=True,
              help="weight of mean(delta^2) on the per-image colour transforms: an untuned guard against the gauge that scene "
                   "colour and one affine common to all images share (nobody has measured it)")
@click.option("--robust_loss", type=click.BOOL, default=False, show_default=True,
              help="replace the L1 terms by RobustNeRF's trimmed loss on random pixel patches, for captures with transient objects "
                   "(a passer-by, a car, a shadow); does not combine with --ssim_weight")
@click.option("--robust_patch_size", type=click.IntRange(min=4, max=64), default=16, show_default=True,
              help="side of the robust loss's pixel patches, even (a stage with smaller images uses its smaller side)")
@click.option("--robust_inlier_quantile", type=click.FloatRange(min=0.0, max=1.0, min_open=True), default=0.5, show_default=True,
              help="quantile of the batch's residuals at and below which a pixel is an inlier")
@click.option("--robust_patch_inlier_fraction", type=click.FloatRange(min=0.0, max=1.0), default=0.6, show_default=True,
              help="share of forgiven pixels at which the inner half of a patch is forgiven as a whole")
@accepted_options(COMPAT_ONLY)
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    device = torch.device("cuda")
    data_path, output_path = Path(cfg.data_path), Path(cfg.output_path)
    log_config_to_disk(kwargs, output_path)
    report_unused(kwargs, COMPAT_ONLY, log)
    separate = cfg.separate_train_test_folders and (data_path / "train").is_dir()
    train_dir = data_path / "train" if separate else data_path / "images"
    params = data_path / ("train_camera_params.json" if separate and (data_path / "train_camera_params.json").exists() else "camera_params.json")
    dataset = PosedImagesDataset(train_dir, params, normalize_scene_scale=cfg.normalize_scene_scale,
                                 downsample_factor=cfg.data_downsample_factor, rgba_white_bkgd=cfg.white_bkgd)
    test_dataset = None
    if separate and (data_path / "test").is_dir() and (data_path / "test_camera_params.json").exists():
        test_dataset = PosedImagesDataset(data_path / "test", data_path / "test_camera_params.json",
                                          normalize_scene_scale=cfg.normalize_scene_scale,
                                          downsample_factor=cfg.data_downsample_factor, rgba_white_bkgd=cfg.white_bkgd)
    densities = torch.empty((*cfg.grid_dims, 1), dtype=torch.float32, device=device).uniform_(-1.0, 1.0)
    num_sh = NUM_COLOUR_CHANNELS * ((cfg.sh_degree + 1) ** 2)
    features = torch.empty((*cfg.grid_dims, num_sh), dtype=torch.float32, device=device).uniform_(-1.0, 1.0)
    voxel_size = VoxelSize(*[w / n for w, n in zip(cfg.grid_world_size, cfg.grid_dims)])
    grid = VoxelGrid(densities, features, voxel_size, VoxelGridLocation(*cfg.grid_location), tunable=True,
                     **density_activations(cfg.use_relu_field, cfg.use_softplus_field, cfg.grid_world_size))
    vol_mod = VolumetricModel(grid, render_sh_voxel_grid, SHVoxGridRenderConfig(
        num_samples_per_ray=cfg.train_num_samples_per_ray, camera_bounds=dataset.camera_bounds, white_bkgd=cfg.white_bkgd,
        render_num_samples_per_ray=cfg.render_num_samples_per_ray, optimized_sampling=cfg.optimized_sampling,
        linear_disparity_sampling=cfg.linear_disparity_sampling, parallel_rays_chunk_size=cfg.parallel_rays_chunk_size),
        device=device)
    train_sh_vox_grid_vol_mod_with_posed_images(
        vol_mod, dataset, output_path, test_dataset=test_dataset, ray_batch_size=cfg.ray_batch_size, num_stages=cfg.num_stages,
        num_iterations_per_stage=cfg.num_iterations_per_stage, scale_factor=cfg.scale_factor,
        learning_rate=cfg.learning_rate, lr_decay_gamma_per_stage=cfg.lr_decay_gamma_per_stage,
        lr_decay_steps_per_stage=cfg.lr_decay_steps_per_stage, stagewise_lr_decay_gamma=cfg.stagewise_lr_decay_gamma,
        apply_diffuse_render_regularization=cfg.apply_diffuse_render_regularization, fast_debug_mode=cfg.fast_debug_mode,
        save_freq=cfg.save_frequency, test_freq=cfg.test_frequency, feedback_freq=cfg.feedback_frequency,
        summary_freq=cfg.summary_frequency, verbose_rendering=cfg.verbose_rendering, lpips_weight=cfg.lpips_weight,
        num_workers=cfg.num_workers, distortion_weight=cfg.distortion_weight, pose_learning_rate=cfg.pose_learning_rate,
        intrinsics_learning_rate=cfg.intrinsics_learning_rate, background_resolution=cfg.background_resolution,
        background_learning_rate=cfg.background_learning_rate, ssim_weight=cfg.ssim_weight, ssim_patch_size=cfg.ssim_patch_size,
        depth_weight=cfg.depth_weight, depth_ray_batch_size=cfg.depth_ray_batch_size, depth_sigma_scale=cfg.depth_sigma_scale,
        orientation_weight=cfg.orientation_weight, orientation_normal_eps=cfg.orientation_normal_eps,
        exposure_learning_rate=cfg.exposure_learning_rate, exposure_regularization=cfg.exposure_regularization,
        robust_loss=cfg.robust_loss, robust_patch_size=cfg.robust_patch_size, robust_inlier_quantile=cfg.robust_inlier_quantile,
        robust_patch_inlier_fraction=cfg.robust_patch_inlier_fraction)


if __name__ == "__main__":
    main()
