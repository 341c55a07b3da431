#!/usr/bin/env python3
"""Import a closed triangle mesh (binary or ASCII PLY, e.g. an export_mesh.py result touched up in a mesh editor, a CAD or scan
asset, a visual hull) as a voxel-grid checkpoint.  The voxeliser runs on the GPU (vox-e_amd/csrc/voxe_voxelize.hip): an exact
inside / outside decision and a narrow band of distances around the surface, turned into densities whose iso-surface at --level
is the mesh, and vertex colours into the diffuse (DC) colour.  --like takes the lattice, activations, SH degree, render settings
and cameras of an existing checkpoint; --grid_dims makes a cubic lattice around the mesh with the trainer's default (softplus)
field.  The result loads in render_sh_based_voxel_grid.py, export_mesh.py and transform_voxel_grid.py --into like any other."""
import os
import sys
from pathlib import Path

import click
import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.rendering.volumetric.utils.misc import compute_expected_density_scale_for_relu_field_grid  # noqa: E402
from thre3d_atom.thre3d_reprs.constants import CONFIG_DICT, STATE_DICT, THRE3D_REPR, u_ATTN, u_DENSITIES, u_FEATURES  # noqa: E402
from thre3d_atom.thre3d_reprs.mesh import load_ply, mesh_to_voxel_grid  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelGridLocation, VoxelSize  # noqa: E402


def cubic_lattice(vertices: np.ndarray, dims, band_voxels: float):
    """(voxel size, grid location) of a lattice with cubic voxels around the mesh bounds, padded by band + 1 voxels per side on
    the axis that binds"""
    lo, hi = vertices.min(axis=0).astype(np.float64), vertices.max(axis=0).astype(np.float64)
    pad = float(band_voxels) + 1.0
    usable = [n - 2.0 * pad for n in dims]
    if min(usable) <= 0:
        raise click.UsageError(f"--grid_dims {tuple(dims)} leave no room inside a pad of {pad} voxels per side")
    edge = max(float(e) / u for e, u in zip(hi - lo, usable))
    if not edge > 0:
        raise click.UsageError("the mesh has no extent")
    return VoxelSize(edge, edge, edge), VoxelGridLocation(*[float(c) for c in (lo + hi) / 2])


def fresh_checkpoint(vertices: np.ndarray, dims, sh_degree: int, band_voxels: float, device):
    """(checkpoint dict without tensors, empty grid on `device`) of --grid_dims: the trainer's default field (Identity / Softplus,
    the density scale of the lattice's world size), a camera circle that sees the whole lattice"""
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.utils.constants import CAMERA_BOUNDS, CAMERA_INTRINSICS, HEMISPHERICAL_RADIUS
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

    voxel_size, location = cubic_lattice(vertices, dims, band_voxels)
    world = [n * e for n, e in zip(dims, voxel_size)]
    grid = VoxelGrid(torch.zeros((*dims, 1), device=device), torch.zeros((*dims, 3 * (sh_degree + 1) ** 2), device=device), voxel_size,
                     location, tunable=True, density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.Softplus(),
                     expected_density_scale=compute_expected_density_scale_for_relu_field_grid(world))
    half_diagonal = 0.5 * float(np.linalg.norm(world))
    reach = float(np.linalg.norm(location)) + half_diagonal       # (the camera circle is about the origin)
    radius = 2.7 * reach                                          # (the proportions of the synthetic scenes: 4.03 for 1.5)
    bounds = CameraBounds(max(radius - reach, 1e-3), radius + reach)
    side = 400
    intrinsics = CameraIntrinsics(side, side, 0.5 * side / float(np.tan(0.5 * 0.6911112)))
    vol_mod = VolumetricModel(grid, render_sh_voxel_grid, SHVoxGridRenderConfig(num_samples_per_ray=256, camera_bounds=bounds,
                                                                                white_bkgd=True), device=device)
    extra = {CAMERA_BOUNDS: bounds, CAMERA_INTRINSICS: intrinsics, HEMISPHERICAL_RADIUS: radius}
    return vol_mod.get_save_info(extra), grid


@click.command()
@click.option("-i", "--mesh_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="input mesh (.ply, binary or ASCII)")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="output checkpoint (.pth)")
@click.option("--like", type=click.Path(file_okay=True, dir_okay=False), default=None,
              help="checkpoint whose lattice, activations, SH degree, render settings and cameras the output takes")
@click.option("--grid_dims", type=click.IntRange(min=1), nargs=3, default=None,
              help="without --like: voxels of a cubic-voxel lattice around the mesh (padded by band + 1 voxels)")
@click.option("--sh_degree", type=click.IntRange(min=0, max=3), default=0, show_default=True, help="with --grid_dims")
@click.option("--level", type=click.FLOAT, default=None,
              help="density at which the imported field has the mesh as its iso-surface; default ln 2 / voxel size, export_mesh.py's")
@click.option("--band_voxels", type=click.FloatRange(min=0.0, min_open=True), default=2.0, show_default=True,
              help="half-width of the band around the surface over which the density falls to empty, in voxels")
@click.option("--inside_ratio", type=click.FloatRange(min=1.0), default=2.0, show_default=True,
              help="the density saturates this many times further above empty than the level is")
@click.option("--allow_open", is_flag=True, default=False, help="import a mesh that is not closed (its inside is then not well defined)")
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    if (cfg.like is None) == (not cfg.grid_dims):
        raise click.UsageError("give exactly one of --like and --grid_dims")
    device = torch.device("cuda")
    mesh = load_ply(cfg.mesh_path)
    if cfg.like is not None:
        data = torch.load(Path(cfg.like), map_location="cpu", weights_only=False)
        state = data[THRE3D_REPR][STATE_DICT]
        config = dict(data[THRE3D_REPR][CONFIG_DICT], tunable=False)
        like = VoxelGrid(densities=state[u_DENSITIES].to(device=device, dtype=torch.float32),
                         features=state[u_FEATURES].to(device=device, dtype=torch.float32), **config)
        state.pop(u_ATTN, None)      # (a keep grid describes the old content)
    else:
        if len(mesh.vertices) == 0:
            raise click.UsageError("the mesh has no vertices: --grid_dims cannot place a lattice around it")
        data, like = fresh_checkpoint(mesh.vertices.numpy(), tuple(int(n) for n in cfg.grid_dims), cfg.sh_degree, cfg.band_voxels, device)
        state = data[THRE3D_REPR][STATE_DICT]
    try:
        grid, stats = mesh_to_voxel_grid(mesh, like, level=cfg.level, band_voxels=cfg.band_voxels, inside_ratio=cfg.inside_ratio,
                                         allow_open=cfg.allow_open, return_stats=True)
    except ValueError as err:
        raise click.ClickException(str(err)) from err
    for key, tensor in ((u_DENSITIES, grid.densities), (u_FEATURES, grid.features)):
        state[key] = tensor.detach().to(device="cpu", dtype=state[key].dtype)
    out = Path(cfg.output_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    torch.save(data, out)
    print(f"V = {len(mesh.vertices)}  T = {len(mesh.faces)}  grid {grid.grid_dims}: {stats[2]} voxels in the band, "
          f"{stats[0]} odd columns  -> {out}")


if __name__ == "__main__":
    main()
