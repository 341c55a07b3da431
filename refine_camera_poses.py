#!/usr/bin/env python3
"""Refine the camera poses of a dataset split against a trained voxel grid: the grid is frozen, per-camera pose corrections
(axis-angle + translation) are optimised with Adam on the photometric error of random pixel batches, and the refined cameras are
written as refined_<split>_camera_params.json in the dataset's own schema.  The gradient to the cameras comes from the GPU
(vox-e_amd/csrc/voxe_render_rays_bwd.hip, voxe_cast_rays_bwd; for a dataset with fx, fy, cx, cy and lens distortion
vox-e_amd/csrc/voxe_camera.hip, voxe_cast_rays_camera_bwd, which --intrinsics_learning_rate also uses to learn fx, fy, cx, cy)."""
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.data.datasets import PosedImagesDataset  # noqa: E402
from thre3d_atom.modules.pose_refiner import refine_camera_poses  # noqa: E402
from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict  # noqa: E402


def split_paths(data_path: Path, split: str):
    """(images dir, camera-parameter file) of a split: <data>/<split> + <split>_camera_params.json, else <data>/images +
    camera_params.json"""
    if (data_path / split).is_dir() and (data_path / f"{split}_camera_params.json").exists():
        return data_path / split, data_path / f"{split}_camera_params.json"
    return data_path / "images", data_path / "camera_params.json"


@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained model")
@click.option("-d", "--data_path", type=click.Path(file_okay=False, dir_okay=True), required=True, help="dataset whose cameras are refined")
@click.option("-o", "--output_path", type=click.Path(file_okay=False, dir_okay=True), required=True, help="directory for the refined camera parameters")
@click.option("--num_iterations", type=click.IntRange(min=1), default=200, show_default=True)
@click.option("--learning_rate", type=click.FloatRange(min=0.0, min_open=True), default=3e-3, show_default=True)
@click.option("--intrinsics_learning_rate", type=click.FloatRange(min=0.0), default=0.0, show_default=True,
              help="> 0: also learn fx, fy, cx, cy of the shared camera (pixels) at this rate and write them back; 0 = off")
@click.option("--ray_batch_size", type=click.IntRange(min=1), default=32768, show_default=True)
@click.option("--split", type=click.STRING, default="train", show_default=True)
@click.option("--white_bkgd", type=click.BOOL, default=True, show_default=True, help="composite RGBA images over white")
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    device = torch.device("cuda")
    vol_mod, _ = create_volumetric_model_from_saved_model(Path(cfg.model_path), create_voxel_grid_from_saved_info_dict, device=device)
    images_dir, params = split_paths(Path(cfg.data_path), cfg.split)
    dataset = PosedImagesDataset(images_dir, params, rgba_white_bkgd=cfg.white_bkgd)
    _, losses = refine_camera_poses(vol_mod, dataset, Path(cfg.output_path), num_iterations=cfg.num_iterations,
                                    learning_rate=cfg.learning_rate, ray_batch_size=cfg.ray_batch_size, split=cfg.split,
                                    intrinsics_learning_rate=cfg.intrinsics_learning_rate)
    print(f"{len(dataset)} cameras, {cfg.num_iterations} iterations: mse {losses[0]:.6f} -> {losses[-1]:.6f}  -> "
          f"{Path(cfg.output_path) / ('refined_' + cfg.split + '_camera_params.json')}")


if __name__ == "__main__":
    main()
