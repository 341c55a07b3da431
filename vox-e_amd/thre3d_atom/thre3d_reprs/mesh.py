"""Triangle-mesh export of a VoxelGrid's density iso-surface (marching cubes on the GPU; DESIGN.md section 4 "Mesh export").

The surface is where the density VoxelGrid.forward returns equals `level`; it is closed and its triangles wind
counter-clockwise seen from outside.  Vertex colours are what a diffuse render shows for an opaque sample there:
sigmoid(C0 * f_dc) of the trilinear DC coefficients, queried through the same point-query kernel as VoxelGrid.forward.
`save_ply` writes a binary little-endian PLY with numpy only.
"""
import math
from pathlib import Path
from typing import NamedTuple, Optional, Union

import numpy as np
import torch
from torch import Tensor

from thre3d_atom.rendering.volumetric.utils.spherical_harmonics import C0
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid
from voxe_hip import ops as _ops


class Mesh(NamedTuple):
    vertices: Tensor   # [V,3] float32, world space
    faces: Tensor      # [T,3] int32 vertex ids
    colours: Tensor    # [V,3] float32 in [0, 1]


def default_level(voxel_grid: VoxelGrid) -> float:
    """ln 2 / min(voxel size): the density at which a slab one voxel thick absorbs half the light
    (density2occupancy_pb(level, min voxel size) == 0.5)"""
    return math.log(2.0) / min(float(s) for s in voxel_grid.voxel_size)


def extract_mesh(voxel_grid: VoxelGrid, level: Optional[float] = None, mask: Optional[Tensor] = None) -> Mesh:
    """Iso-surface {density == level} of `voxel_grid` (default level: default_level()).  `mask` ([X,Y,Z], 0 = excluded)
    turns the excluded voxels into outside; the mesh is then capped where the mask cuts the object."""
    spec = voxel_grid.voxe_grid_spec()   # raises exactly where rendering would
    if level is None:
        level = default_level(voxel_grid)
    densities = voxel_grid.densities.detach()
    if mask is not None:
        mask = mask.to(densities.device)
    vertices, faces = _ops.extract_mesh(spec, densities, float(level), mask)
    features = voxel_grid.features.detach()
    ncoef = features.shape[-1] // 3      # [..., 3, (deg+1)^2]: the DC coefficient of channel c is at c * ncoef
    if len(vertices) == 0:
        colours = torch.empty((0, 3), dtype=torch.float32, device=densities.device)
    else:
        with torch.no_grad():
            out = voxel_grid(vertices)
            if out.dim() == 1:       # (a single point loses its axis, like the reference's squeeze)
                out = out[None]
            colours = torch.sigmoid(C0 * out[:, 0:3 * ncoef:ncoef])
    return Mesh(vertices, faces, colours)


def save_ply(mesh: Mesh, path: Union[str, Path], normals: Optional[Tensor] = None) -> None:
    """binary little-endian PLY: float x y z (then float nx ny nz when `normals` [V,3] is given, e.g.
    geometry.vertex_normals), uchar red green blue per vertex; a uchar-counted int32 list per face"""
    v = mesh.vertices.detach().cpu().numpy().astype("<f4")
    f = mesh.faces.detach().cpu().numpy().astype("<i4")
    c = np.clip(np.rint(mesh.colours.detach().cpu().numpy().astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    n = None if normals is None else normals.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
    if n is not None and len(n) != len(v):
        raise ValueError(f"save_ply: {len(n)} normals for {len(v)} vertices")
    header = (
        "ply\nformat binary_little_endian 1.0\ncomment vox-e mesh export\n"
        f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
        + ("" if n is None else "property float nx\nproperty float ny\nproperty float nz\n")
        + "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n"
    )
    vrec = np.empty(len(v), dtype=[("xyz", "<f4", 3)] + ([] if n is None else [("nxyz", "<f4", 3)]) + [("rgb", "u1", 3)])
    vrec["xyz"], vrec["rgb"] = v, c
    if n is not None:
        vrec["nxyz"] = n
    frec = np.empty(len(f), dtype=[("n", "u1"), ("idx", "<i4", 3)])
    frec["n"], frec["idx"] = 3, f
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
