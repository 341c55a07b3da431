#!/usr/bin/env python3
"""Prune a voxel grid by a lifted region (lift_masks_to_grid.py): every voxel the masks voted out (label 1) that has no voted-in
voxel (label 2) within --region_dilate voxels has its density lowered to the field's empty value, through the rule of
prune_voxel_grid.py (prune_voxel_grid_: densities only fall, features are untouched).  Unseen voxels -- object interiors among
them -- are never removed.  The output is a checkpoint the existing loaders read; run prune_voxel_grid.py on it for the
visibility rule.  (prune_voxel_grid.py keeps the options it has: this rule has an entry point of its own.)"""
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model  # noqa: E402
from thre3d_atom.thre3d_reprs.constants import STATE_DICT, THRE3D_REPR, u_DENSITIES  # noqa: E402
from thre3d_atom.thre3d_reprs.lifting import load_region, prune_region_, remove_mask  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict  # noqa: E402


@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained / edited / refined model")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="pruned checkpoint (.pth)")
@click.option("--region", type=click.Path(file_okay=True, dir_okay=False), required=True, help="region file of lift_masks_to_grid.py")
@click.option("--region_dilate", type=click.IntRange(min=0, max=3), default=1, show_default=True, help="keep voted-out voxels this close to a voted-in one")
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    device = torch.device("cuda")
    path = Path(cfg.model_path)
    vol_mod, _ = create_volumetric_model_from_saved_model(path, create_voxel_grid_from_saved_info_dict, device=device)
    grid = vol_mod.thre3d_repr
    labels = load_region(cfg.region, grid)["labels"].to(device)
    removed = int(remove_mask(labels, cfg.region_dilate).sum())
    changed = prune_region_(grid, labels, cfg.region_dilate)
    # the checkpoint as it was loaded, with the densities replaced (as prune_voxel_grid.py writes it)
    data = torch.load(path, map_location="cpu", weights_only=False)
    state = data[THRE3D_REPR][STATE_DICT]
    state[u_DENSITIES] = grid.densities.detach().to(device="cpu", dtype=state[u_DENSITIES].dtype)
    out = Path(cfg.output_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    torch.save(data, out)
    print(f"region {cfg.region}: removed {removed} of {labels.numel()} voxels ({changed} densities lowered)  -> {out}")


if __name__ == "__main__":
    main()
