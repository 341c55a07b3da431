#!/usr/bin/env python3
"""Move a trained, edited or refined voxel grid: rotate it about an axis, turn it by quarter turns, mirror it, translate it,
scale it, re-grid it to another resolution (--output_dims keeps the world extent), or drop it into another checkpoint's scene
(--into: CSG union on that grid's lattice).  The map is p' = scale * R p + translation in world units; SH coefficients of
view-dependent grids are rotated with the geometry.  The output is the loaded checkpoint with only the grid tensors (and, when
the lattice changes, its voxel size) replaced, so the existing loaders read it; the cameras stored in it are not moved.  Scale
is geometric only: densities are not compensated.  The resampling runs on the GPU (vox-e_amd/csrc/voxe_transform.hip)."""
import os
import sys
from pathlib import Path

import click
import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.thre3d_reprs.compression import load_uncompressed_checkpoint  # noqa: E402
from thre3d_atom.thre3d_reprs.constants import CONFIG_DICT, STATE_DICT, THRE3D_REPR, u_ATTN, u_DENSITIES, u_FEATURES  # noqa: E402
from thre3d_atom.thre3d_reprs.transform import compose_voxel_grids_, default_output_lattice, transform_voxel_grid  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid  # noqa: E402

AXES = click.Choice(["x", "y", "z"])
_QUARTER = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]   # (cos, sin) of n quarter turns, exactly


def _about(axis: str, c: float, s: float) -> np.ndarray:
    a = "xyz".index(axis)
    i, j = (a + 1) % 3, (a + 2) % 3
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def rotation_from_options(rotate_axis=None, rotate_degrees=None, quarter_turns=None, mirror=None) -> np.ndarray:
    """the orthogonal matrix of the (mutually exclusive) rotation options; quarter turns and mirrors are exact integer
    matrices"""
    given = [rotate_axis is not None or rotate_degrees is not None, quarter_turns is not None, mirror is not None]
    if sum(given) > 1:
        raise click.UsageError("--rotate_axis/--rotate_degrees, --quarter_turns and --mirror exclude each other")
    if given[0]:
        if rotate_axis is None or rotate_degrees is None:
            raise click.UsageError("--rotate_axis and --rotate_degrees go together")
        return _about(rotate_axis, float(np.cos(np.radians(rotate_degrees))), float(np.sin(np.radians(rotate_degrees))))
    if given[1]:
        axis, n = quarter_turns
        if axis not in ("x", "y", "z"):
            raise click.UsageError("--quarter_turns takes an axis (x, y or z) and a count")
        return _about(axis, *_QUARTER[int(n) % 4])
    if given[2]:
        R = np.eye(3)
        R["xyz".index(mirror), "xyz".index(mirror)] = -1.0
        return R
    return np.eye(3)


def _grid_of(data, device) -> VoxelGrid:
    state = data[THRE3D_REPR][STATE_DICT]
    config = dict(data[THRE3D_REPR][CONFIG_DICT], tunable=False)
    on = dict(device=device, dtype=torch.float32)
    attn = state[u_ATTN].to(**on) if u_ATTN in state else None
    return VoxelGrid(densities=state[u_DENSITIES].to(**on), features=state[u_FEATURES].to(**on), attn=attn, **config)


def _write_back(data, grid: VoxelGrid) -> None:
    state, config = data[THRE3D_REPR][STATE_DICT], data[THRE3D_REPR][CONFIG_DICT]
    for key, tensor in ((u_DENSITIES, grid.densities), (u_FEATURES, grid.features), (u_ATTN, grid.attn)):
        if key in state and tensor is not None:
            state[key] = tensor.detach().to(device="cpu", dtype=state[key].dtype)
    if tuple(config["voxel_size"]) != tuple(grid.voxel_size):
        config["voxel_size"] = grid.voxel_size
    if tuple(config["grid_location"]) != tuple(grid._grid_location):
        config["grid_location"] = grid._grid_location


@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained / edited / refined model")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="transformed checkpoint (.pth)")
@click.option("--rotate_axis", type=AXES, default=None, help="axis of --rotate_degrees")
@click.option("--rotate_degrees", type=click.FLOAT, default=None, help="rotation about --rotate_axis, counter-clockwise, degrees")
@click.option("--quarter_turns", type=(str, int), default=None, help="AXIS N: N exact quarter turns about AXIS (the lattice is permuted)")
@click.option("--mirror", type=AXES, default=None, help="mirror this coordinate")
@click.option("--translate", type=(float, float, float), default=(0.0, 0.0, 0.0), show_default=True, help="translation, world units")
@click.option("--scale", type=click.FloatRange(min=0.0, min_open=True), default=1.0, show_default=True, help="uniform scale (geometric only)")
@click.option("--output_dims", type=(int, int, int), default=None, help="voxels of the output lattice (same world extent)")
@click.option("--into", type=click.Path(file_okay=True, dir_okay=False), default=None, help="compose into this checkpoint's grid; it is what gets written")
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    device = torch.device("cuda")
    R = rotation_from_options(cfg.rotate_axis, cfg.rotate_degrees, cfg.quarter_turns, cfg.mirror)
    data = load_uncompressed_checkpoint(Path(cfg.model_path))
    grid = _grid_of(data, device)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if cfg.into is not None:
        if cfg.output_dims is not None:
            raise click.UsageError("--output_dims does not apply with --into: the other checkpoint's lattice is kept")
        data = load_uncompressed_checkpoint(Path(cfg.into))
        out_grid = _grid_of(data, device)
        start.record()
        taken = compose_voxel_grids_(out_grid, grid, R, cfg.translate, cfg.scale)
        end.record()
        what = f"composed into {cfg.into}: {int(taken.sum())} of {taken.numel()} voxels taken"
    else:
        dims = edges = None
        if cfg.output_dims is not None:
            dims = tuple(int(n) for n in cfg.output_dims)
            edges = tuple((n * e) / m for n, e, m in zip(*default_output_lattice(grid, R), dims))
        start.record()
        out_grid = transform_voxel_grid(grid, R, cfg.translate, cfg.scale, output_dims=dims, output_voxel_size=edges)
        end.record()
        what = f"{grid.grid_dims} -> {out_grid.grid_dims} voxels"
    torch.cuda.synchronize()
    _write_back(data, out_grid)
    out = Path(cfg.output_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    torch.save(data, out)
    print(f"{what}  {start.elapsed_time(end):.2f} ms  -> {out}")


if __name__ == "__main__":
    main()
