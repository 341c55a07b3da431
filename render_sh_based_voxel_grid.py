#!/usr/bin/env python3
"""Render a camera path of a trained SH voxel grid (entry point kept from the reference's
render_sh_based_voxel_grid.py:74-170; same option names).  Every frame is one fused HIP forward launch.
Frames are written as PNGs, plus rendered_video.mp4 when `imageio` is installed (an animated PNG otherwise).
--render_geometry also writes geometry_NNNN.png = colour | depth | normals | 1 - acc per frame (the reference's output_only=False
layout of animations.py with a camera-space normal map inserted) and rendered_geometry_video next to rendered_video."""
import os
import sys
from pathlib import Path

import click
import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model  # noqa: E402
from thre3d_atom.thre3d_reprs.geometry import normals_to_rgb, render_geometry  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict  # noqa: E402
from thre3d_atom.utils.constants import CAMERA_INTRINSICS, HEMISPHERICAL_RADIUS, NUM_COLOUR_CHANNELS  # noqa: E402
from thre3d_atom.utils.imaging_utils import (  # noqa: E402
    CameraPose,
    get_thre360_animation_poses,
    get_thre360_spiral_animation_poses,
    novel_view_camera,
    postprocess_depth_map,
    scale_camera_intrinsics,
    to8b,
)


@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained (reconstructed) model")
@click.option("-o", "--output_path", type=click.Path(file_okay=False, dir_okay=True), required=True, help="path for saving rendered output")
@click.option("-r", "--ref_path", type=click.Path(file_okay=True, dir_okay=False), default=None, help="reference model whose camera info is used")
@click.option("-d", "--data_path", type=click.Path(file_okay=False, dir_okay=True), default=None, help="dataset (camera_path=dataset)")
@click.option("--overridden_num_samples_per_ray", type=click.IntRange(min=1), default=512, show_default=True)
@click.option("--render_scale_factor", type=click.FLOAT, default=2.0, show_default=True)
@click.option("--camera_path", type=click.Choice(["thre360", "spiral", "dataset"]), default="thre360", show_default=True)
@click.option("--camera_pitch", type=click.FLOAT, default=60.0, show_default=True)
@click.option("--num_frames", type=click.IntRange(min=1), default=180, show_default=True)
@click.option("--vertical_camera_height", type=click.FLOAT, default=3.0, show_default=True)
@click.option("--num_spiral_rounds", type=click.IntRange(min=1), default=2, show_default=True)
@click.option("--fps", type=click.IntRange(min=1), default=60, show_default=True)
@click.option("--save_freq", type=click.INT, default=None, help="write every n-th frame as PNG (default: all)")
@click.option("-p", "--sds_prompt", type=click.STRING, required=False, default=None)
@click.option("--render_geometry", is_flag=True, default=False,
              help="also write geometry frames: colour | depth | normals | 1 - acc, and rendered_geometry_video")
@click.option("--ignore_background", is_flag=True, default=False,
              help="do not composite the checkpoint's learned background (render over white, as for a checkpoint without one)")
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    device = torch.device("cuda")
    out = Path(cfg.output_path)
    out.mkdir(exist_ok=True, parents=True)
    if cfg.sds_prompt is not None:
        (out / "prompt.txt").write_text(cfg.sds_prompt)
    vol_mod, extra = create_volumetric_model_from_saved_model(Path(cfg.model_path), create_voxel_grid_from_saved_info_dict, device=device)
    if cfg.ignore_background:
        vol_mod.background = None
    if vol_mod.background is None:
        vol_mod.render_config.white_bkgd = True  # the reference forces a white background at inference (:97-98)
    # (a checkpoint trained with a learned background renders over that background: white_bkgd stays off)
    if cfg.ref_path is not None:
        _, extra = create_volumetric_model_from_saved_model(Path(cfg.ref_path), create_voxel_grid_from_saved_info_dict, device=device)
    radius, intrinsics = extra[HEMISPHERICAL_RADIUS], extra[CAMERA_INTRINSICS]
    if cfg.camera_path == "thre360":
        poses = get_thre360_animation_poses(radius, cfg.camera_pitch, cfg.num_frames)
    elif cfg.camera_path == "spiral":
        poses = get_thre360_spiral_animation_poses((radius / 8.0, radius), cfg.vertical_camera_height, cfg.num_spiral_rounds, cfg.num_frames)
    else:
        from thre3d_atom.data.datasets import PosedImagesDataset

        data = PosedImagesDataset(Path(cfg.data_path) / "train", Path(cfg.data_path) / "train_camera_params.json",
                                  rgba_white_bkgd=True)
        poses = [CameraPose(p[:, :3], p[:, 3:]) for p in data.poses]
    intrinsics = scale_camera_intrinsics(novel_view_camera(intrinsics), cfg.render_scale_factor)   # (no lens on a novel view)
    frames, geometry = [], []
    for n, pose in enumerate(poses):
        if cfg.render_geometry:
            geo = render_geometry(vol_mod, pose, intrinsics, num_samples_per_ray=cfg.overridden_num_samples_per_ray)
            frames.append(to8b(geo.colour.cpu().numpy()))
            acc = geo.acc.cpu().numpy()
            geometry.append(np.concatenate([frames[-1], postprocess_depth_map(geo.depth.cpu().numpy(), acc_map=acc),
                                            normals_to_rgb(geo.normal_camera, acc),
                                            to8b(1.0 - np.tile(acc, (1, 1, NUM_COLOUR_CHANNELS)))], axis=1))
        else:
            rendered = vol_mod.render(pose, intrinsics, gpu_render=True, num_samples_per_ray=cfg.overridden_num_samples_per_ray)
            frames.append(to8b(rendered.colour.cpu().numpy()))
        if cfg.save_freq is None or n % cfg.save_freq == 0:
            from PIL import Image

            Image.fromarray(frames[-1]).save(out / f"frame_{n:04d}.png")
            if geometry:
                Image.fromarray(geometry[-1]).save(out / f"geometry_{n:04d}.png")
    write_video(out, "rendered_video", frames, cfg.fps)
    if geometry:
        write_video(out, "rendered_geometry_video", geometry, cfg.fps)


def write_video(out: Path, name: str, frames, fps: int) -> None:
    """`name`.mp4 when imageio is installed, an animated PNG of the same frames (plays in browsers) otherwise"""
    try:
        import imageio

        imageio.mimwrite(out / f"{name}.mp4", frames, fps=fps)
    except ImportError:
        from PIL import Image

        stills = [Image.fromarray(f) for f in frames]
        stills[0].save(out / f"{name}.png", save_all=True, append_images=stills[1:], duration=int(1000 / fps), loop=0)
        print(f"imageio not installed: wrote {len(frames)} PNG frames and {name}.png (APNG) to {out} instead of an mp4")


if __name__ == "__main__":
    main()
