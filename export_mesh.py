#!/usr/bin/env python3
"""Export the density iso-surface of a trained, edited or refined voxel grid as a closed, coloured triangle mesh (binary
PLY, opens in Blender / MeshLab / slicers).  Marching cubes runs on the GPU (vox-e_amd/csrc/voxe_mesh.hip); vertex
colours are the diffuse (DC) colour of the field at each vertex; --vertex_normals adds unit density-gradient normals (smooth
shading, vox-e_amd/csrc/voxe_normals.hip).  --edit_region_only keeps the voxels a refined model
marks as its edit region (keep-grid value 0) and caps the mesh where that region cuts the object.  --visible_only keeps the
voxels some camera actually weighs (vox-e_amd/csrc/voxe_visibility.hip): the training cameras of -d, or --num_views poses of the
checkpoint's own 360 degree path.  --region leaves out the voxels the masks of a lifted region voted out
(lift_masks_to_grid.py, vox-e_amd/csrc/voxe_lift.hip)."""
import os
import sys
import time
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model_attn  # noqa: E402
from thre3d_atom.thre3d_reprs.compression import load_uncompressed_checkpoint  # noqa: E402
from thre3d_atom.thre3d_reprs.constants import STATE_DICT, THRE3D_REPR, u_ATTN  # noqa: E402
from thre3d_atom.thre3d_reprs.geometry import vertex_normals  # noqa: E402
from thre3d_atom.thre3d_reprs.mesh import default_level, extract_mesh, save_ply  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict_attn  # noqa: E402


@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained / edited / refined model")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="output mesh (.ply)")
@click.option("--level", type=click.FLOAT, default=None,
              help="iso-level of the (post-activated) density; default ln 2 / voxel size: a one-voxel slab absorbs half the light")
@click.option("--edit_region_only", is_flag=True, default=False, help="refined models: mesh only the edit region (keep grid == 0)")
@click.option("--vertex_normals", is_flag=True, default=False, help="write unit vertex normals (nx ny nz) from the density gradient")
@click.option("--visible_only", is_flag=True, default=False,
              help="mesh only the voxels whose maximum rendering weight over the cameras exceeds --visibility_threshold (1 voxel dilated)")
@click.option("--visibility_threshold", type=click.FLOAT, default=0.0, show_default=True)
@click.option("--num_views", type=click.IntRange(min=1), default=36, show_default=True, help="--visible_only: poses of the 360 degree path (without -d)")
@click.option("-d", "--data_path", type=click.Path(file_okay=False, dir_okay=True), default=None,
              help="--visible_only: dataset whose training cameras are used")
@click.option("--region", type=click.Path(file_okay=True, dir_okay=False), default=None,
              help="region file of lift_masks_to_grid.py: leave out the voxels its masks voted out (label 1)")
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    device = torch.device("cuda")
    path = Path(cfg.model_path)
    has_attn = u_ATTN in load_uncompressed_checkpoint(path)[THRE3D_REPR][STATE_DICT]
    if cfg.edit_region_only and not has_attn:
        raise click.UsageError(f"{path} holds no keep grid (attn): --edit_region_only needs a refined model")
    vol_mod, extra = create_volumetric_model_from_saved_model_attn(path, create_voxel_grid_from_saved_info_dict_attn,
                                                                   device=device, load_attn=has_attn)
    grid = vol_mod.thre3d_repr
    mask = (grid.attn.detach()[..., 0] == 0) if cfg.edit_region_only else None
    if cfg.visible_only:
        mask = visible_mask(vol_mod, extra, cfg, mask)
    if cfg.region is not None:
        mask = region_mask(grid, cfg.region, mask)
    level = cfg.level if cfg.level is not None else default_level(grid)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh = extract_mesh(grid, level=level, mask=mask)
    normals = vertex_normals(grid, mesh.vertices) if cfg.vertex_normals else None
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    out = Path(cfg.output_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    save_ply(mesh, out, normals=normals)
    print(f"level {level:.6g}: V = {len(mesh.vertices)}  T = {len(mesh.faces)}  extract {ms:.2f} ms  -> {out}")


def visible_mask(vol_mod, extra, cfg, mask):
    """u8 [X,Y,Z]: the voxels whose max rendering weight over the cameras exceeds the threshold, dilated by one voxel, ANDed
    with `mask` when there is one"""
    from thre3d_atom.thre3d_reprs.visibility import accumulate_visibility, visibility_cameras
    from voxe_hip import ops

    poses, intrinsics = visibility_cameras(extra, cfg.data_path, cfg.num_views)
    vis = accumulate_visibility(vol_mod, poses, intrinsics)
    seen = ops.visibility_mask(vis.max_weight, cfg.visibility_threshold, 1)
    return seen if mask is None else seen * mask.to(torch.uint8)


def region_mask(grid, region_path, mask):
    """u8 [X,Y,Z]: the voxels the region's masks did not vote out (labels != 1), ANDed with `mask` when there is one"""
    from thre3d_atom.thre3d_reprs.lifting import load_region, mesh_mask

    labels = load_region(region_path, grid)["labels"].to(grid.densities.device)
    return mesh_mask(labels, mask)


if __name__ == "__main__":
    main()
