#!/usr/bin/env python3
"""Lift per-image 2-D masks of a posed capture into a trained voxel grid and write the region they select: every sample of every
masked ray deposits its rendering weight, and its weight times the mask value, into the 8 voxels of its trilinear footprint; the
per-voxel ratio is the vote (vox-e_amd/csrc/voxe_lift.hip, 64-bit fixed point: the same bits whatever the order of cameras).
-m holds one image per image of <data>/<split>/, with the same file names: greyscale, or RGBA whose alpha is used; value / 255 is
the soft mask.  The region file (labels 0 = unseen, 1 = voted out, 2 = voted in, plus weight and mean) is what
prune_voxel_grid_by_region.py and export_mesh.py --region read."""
import os
import sys
from pathlib import Path

import click
import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.data.datasets import PosedImagesDataset  # noqa: E402
from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model  # noqa: E402
from thre3d_atom.thre3d_reprs.lifting import lift_images, region_labels, save_region  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict  # noqa: E402
from thre3d_atom.utils.imaging_utils import CameraPose  # noqa: E402


def read_masks(masks_dir: Path, images_dir: Path, camera_parameters) -> torch.Tensor:
    """[N,1,H,W] float32 in [0, 1]: the mask of every image PosedImagesDataset reads from `images_dir`, in its order"""
    from PIL import Image

    files = sorted(p for p in images_dir.iterdir() if p.suffix.lower() in (".png", ".jpg", ".jpeg"))
    files = [p for p in files if p.name in camera_parameters] or files
    masks = []
    for p in files:
        path = masks_dir / p.name
        if not path.is_file():
            raise click.UsageError(f"no mask for {p.name}: {path} is missing")
        img = np.asarray(Image.open(path))
        if img.ndim == 3:   # RGBA / LA: the alpha channel; RGB: its first channel
            img = img[..., -1] if img.shape[-1] in (2, 4) else img[..., 0]
        masks.append(torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32) / 255.0)[None])
    return torch.stack(masks)


@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained model")
@click.option("-d", "--data_path", type=click.Path(file_okay=False, dir_okay=True), required=True, help="dataset whose cameras took the masks")
@click.option("-m", "--masks_path", type=click.Path(file_okay=False, dir_okay=True), required=True, help="one mask per image of the split, same file names")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="region file (.pth)")
@click.option("--split", type=click.STRING, default="train", show_default=True, help="<data>/<split>/ and <data>/<split>_camera_params.json")
@click.option("--threshold", type=click.FLOAT, default=0.5, show_default=True, help="a seen voxel is voted in when its mean mask value reaches this")
@click.option("--min_weight", type=click.FLOAT, default=1e-3, show_default=True, help="a voxel is seen when its summed rendering weight exceeds this")
@click.option("--overridden_num_samples_per_ray", type=click.IntRange(min=1), default=None, help="samples per ray (default: the model's)")
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    device = torch.device("cuda")
    vol_mod, _ = create_volumetric_model_from_saved_model(Path(cfg.model_path), create_voxel_grid_from_saved_info_dict, device=device)
    data_path = Path(cfg.data_path)
    data = PosedImagesDataset(data_path / cfg.split, data_path / f"{cfg.split}_camera_params.json", rgba_white_bkgd=True)
    masks = read_masks(Path(cfg.masks_path), data_path / cfg.split, data.camera_parameters)
    poses = [CameraPose(p[:, :3], p[:, 3:]) for p in data.poses]
    overrides = {}
    if cfg.overridden_num_samples_per_ray is not None:
        overrides["num_samples_per_ray"] = int(cfg.overridden_num_samples_per_ray)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    masks = masks.to(device)
    start.record()
    lifted = lift_images(vol_mod, poses, data.camera_intrinsics, masks, **overrides)
    labels = region_labels(lifted, cfg.threshold, cfg.min_weight)
    end.record()
    torch.cuda.synchronize()
    out = Path(cfg.output_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    save_region(out, labels, lifted, {"grid": vol_mod.thre3d_repr, "threshold": cfg.threshold, "min_weight": cfg.min_weight,
                                      "num_views": len(poses)})
    counts = torch.bincount(labels.flatten().long(), minlength=3).tolist()
    print(f"{len(poses)} views: unseen {counts[0]}  voted out {counts[1]}  voted in {counts[2]} of {labels.numel()} voxels  "
          f"lift {start.elapsed_time(end):.2f} ms  -> {out}")


if __name__ == "__main__":
    main()
