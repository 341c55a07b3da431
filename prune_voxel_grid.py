#!/usr/bin/env python3
"""Prune a trained, edited or refined voxel grid by visibility: every voxel whose maximum rendering weight over a set of cameras
stays at or below --weight_threshold (and has no such neighbour within --dilate voxels) has its density lowered to the field's
empty value; features are untouched and the output is a checkpoint the existing loaders read.  The cameras are the training
split of -d, or --num_views poses of the checkpoint's own 360 degree animation path.  The visibility pass runs on the GPU
(vox-e_amd/csrc/voxe_visibility.hip)."""
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model  # noqa: E402
from thre3d_atom.thre3d_reprs.compression import load_uncompressed_checkpoint  # noqa: E402
from thre3d_atom.thre3d_reprs.constants import STATE_DICT, THRE3D_REPR, u_DENSITIES  # noqa: E402
from thre3d_atom.thre3d_reprs.visibility import accumulate_visibility, prune_voxel_grid_, visibility_cameras  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict  # noqa: E402
from voxe_hip import ops  # noqa: E402


@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained / edited / refined model")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="pruned checkpoint (.pth)")
@click.option("-d", "--data_path", type=click.Path(file_okay=False, dir_okay=True), default=None, help="dataset whose training cameras are used")
@click.option("--num_views", type=click.IntRange(min=1), default=36, show_default=True, help="poses of the 360 degree path (without -d)")
@click.option("--weight_threshold", type=click.FLOAT, default=0.0, show_default=True, help="keep voxels whose max rendering weight exceeds this")
@click.option("--dilate", type=click.IntRange(min=0, max=3), default=1, show_default=True, help="also keep voxels this close to a kept one")
@click.option("--overridden_num_samples_per_ray", type=click.IntRange(min=1), default=None, help="samples per ray (default: the model's)")
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    device = torch.device("cuda")
    path = Path(cfg.model_path)
    # the checkpoint as it is on disk: its densities are replaced below and every other entry (features, keep grid, configs,
    # extra info) is written back untouched (a compressed checkpoint is refused here, before any work)
    data = load_uncompressed_checkpoint(path)
    vol_mod, extra = create_volumetric_model_from_saved_model(path, create_voxel_grid_from_saved_info_dict, device=device)
    poses, intrinsics = visibility_cameras(extra, cfg.data_path, cfg.num_views)
    overrides = {}
    if cfg.overridden_num_samples_per_ray is not None:
        overrides["num_samples_per_ray"] = int(cfg.overridden_num_samples_per_ray)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    vis = accumulate_visibility(vol_mod, poses, intrinsics, **overrides)
    keep = ops.visibility_mask(vis.max_weight, cfg.weight_threshold, cfg.dilate)
    end.record()
    torch.cuda.synchronize()
    grid = vol_mod.thre3d_repr
    changed = prune_voxel_grid_(grid, keep)
    kept = int(keep.sum())
    state = data[THRE3D_REPR][STATE_DICT]
    state[u_DENSITIES] = grid.densities.detach().to(device="cpu", dtype=state[u_DENSITIES].dtype)
    out = Path(cfg.output_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    torch.save(data, out)
    print(f"{len(poses)} views: kept {kept}  pruned {keep.numel() - kept} of {keep.numel()} voxels ({changed} densities lowered)  "
          f"visibility {start.elapsed_time(end):.2f} ms  -> {out}")


if __name__ == "__main__":
    main()
