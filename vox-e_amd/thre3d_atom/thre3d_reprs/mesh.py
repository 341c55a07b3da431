"""Triangle-mesh export of a VoxelGrid's density iso-surface (marching cubes on the GPU; DESIGN.md section 4 "Mesh export").

The surface is where the density VoxelGrid.forward returns equals `level`; it is closed and its triangles wind
counter-clockwise seen from outside.  Vertex colours are what a diffuse render shows for an opaque sample there:
sigmoid(C0 * f_dc) of the trilinear DC coefficients, queried through the same point-query kernel as VoxelGrid.forward.
`save_ply` writes a binary little-endian PLY with numpy only.

The way back: `load_ply` reads binary and ASCII PLY, `mesh_to_voxel_grid` voxelises a closed mesh on
the GPU (signed-distance band, exact inside / outside) into a grid whose iso-surface at a level is the mesh.
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


# ---- mesh import --------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _ply_header(blob: bytes):
    """-> (format, elements, offset of the data): elements = [(name, count, [property, ...])], a property is (name, type) or
    (name, count type, item type) for a list.  ValueError for anything that is not a PLY header this reader understands."""
    if not blob.startswith(b"ply"):
        raise ValueError("load_ply: not a PLY file (no 'ply' magic)")
    end = blob.find(b"end_header")
    if end < 0:
        raise ValueError("load_ply: the header has no end_header")
    nl = blob.find(b"\n", end)
    if nl < 0:
        raise ValueError("load_ply: the header's last line is not terminated")
    try:
        lines = blob[:end].decode("ascii").split("\n")
    except UnicodeDecodeError as err:
        raise ValueError("load_ply: the header is not ASCII") from err
    fmt, elements = None, []
    for line in lines[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            if len(tok) != 3 or tok[1] not in ("ascii", "binary_little_endian"):
                raise ValueError(f"load_ply: unsupported format line {line.strip()!r} (ascii | binary_little_endian)")
            fmt = tok[1]
        elif tok[0] == "element":
            if len(tok) != 3 or not tok[2].isdigit():
                raise ValueError(f"load_ply: malformed element line {line.strip()!r}")
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError("load_ply: a property before any element")
            types = tok[2:4] if len(tok) == 5 and tok[1] == "list" else tok[1:2] if len(tok) == 3 else None
            if types is None or any(t not in _PLY_TYPES for t in types):
                raise ValueError(f"load_ply: malformed property line {line.strip()!r}")
            elements[-1][2].append((tok[-1], *[_PLY_TYPES[t] for t in types]))
        else:
            raise ValueError(f"load_ply: unknown header line {line.strip()!r}")
    if fmt is None:
        raise ValueError("load_ply: the header has no format line")
    return fmt, elements, nl + 1


def _fan(polygons) -> np.ndarray:
    """triangles (v0, vi, vi+1) of every polygon"""
    tris = [(p[0], p[i], p[i + 1]) for p in polygons for i in range(1, len(p) - 1)]
    return np.array(tris, dtype=np.int64).reshape(-1, 3)


def load_ply(path: Union[str, Path]) -> Mesh:
    """A triangle mesh from a binary little-endian or ASCII PLY file, numpy only: vertex x y z, optional nx ny nz (read over),
    optional red green blue [alpha] (uchar: / 255); faces as a list property (polygons are fan-triangulated).  Everything
    save_ply writes loads back.  CPU tensors; `colours` is None when the file has none.  ValueError for a malformed file."""
    blob = Path(path).read_bytes()
    fmt, elements, pos = _ply_header(blob)
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise ValueError("load_ply: no vertex element")
    tokens = blob[pos:].split() if fmt == "ascii" else None
    tpos = 0
    vertex, polygons = None, []
    for name, count, props in elements:
        scalar_only = all(len(p) == 2 for p in props)
        if scalar_only:
            if fmt == "ascii":
                need = count * len(props)
                if tpos + need > len(tokens):
                    raise ValueError(f"load_ply: element {name} is truncated")
                try:
                    table = np.array(tokens[tpos:tpos + need], dtype=np.float64).reshape(count, len(props))
                except ValueError as err:
                    raise ValueError(f"load_ply: element {name} holds a non-numeric value") from err
                tpos += need
                rec = {p[0]: table[:, i] for i, p in enumerate(props)}
            else:
                dt = np.dtype([(p[0], "<" + p[1]) for p in props])
                if pos + count * dt.itemsize > len(blob):
                    raise ValueError(f"load_ply: element {name} is truncated")
                arr = np.frombuffer(blob, dtype=dt, count=count, offset=pos)
                pos += count * dt.itemsize
                rec = {p[0]: arr[p[0]] for p in props}
            if name == "vertex":
                vertex = (rec, {p[0]: p[1] for p in props})
            continue
        # an element with list properties (the faces): record by record
        lists = []
        uniform = (fmt != "ascii" and len(props) == 1 and count > 0 and pos < len(blob)
                   and (len(blob) - pos) >= count * (np.dtype(props[0][1]).itemsize + blob[pos] * np.dtype(props[0][2]).itemsize))
        if uniform and props[0][1] == "u1":
            n0 = blob[pos]
            dt = np.dtype([("n", "u1"), ("idx", "<" + props[0][2], (n0,))])
            arr = np.frombuffer(blob, dtype=dt, count=count, offset=pos)
            if np.all(arr["n"] == n0):      # every polygon has the first one's size: one strided read
                lists = arr["idx"].astype(np.int64)
                pos += count * dt.itemsize
            else:
                uniform = False
        else:
            uniform = False
        if not uniform:
            for _ in range(count):
                for p in props:
                    if len(p) == 2:
                        if fmt == "ascii":
                            tpos += 1
                        else:
                            pos += np.dtype(p[1]).itemsize
                        continue
                    if fmt == "ascii":
                        if tpos >= len(tokens):
                            raise ValueError(f"load_ply: element {name} is truncated")
                        n = int(tokens[tpos])
                        if tpos + 1 + n > len(tokens):
                            raise ValueError(f"load_ply: element {name} is truncated")
                        item = [int(t) for t in tokens[tpos + 1:tpos + 1 + n]]
                        tpos += 1 + n
                    else:
                        cdt, idt = np.dtype("<" + p[1]), np.dtype("<" + p[2])
                        if pos + cdt.itemsize > len(blob):
                            raise ValueError(f"load_ply: element {name} is truncated")
                        n = int(np.frombuffer(blob, dtype=cdt, count=1, offset=pos)[0])
                        pos += cdt.itemsize
                        if pos + n * idt.itemsize > len(blob):
                            raise ValueError(f"load_ply: element {name} is truncated")
                        item = np.frombuffer(blob, dtype=idt, count=n, offset=pos).astype(np.int64).tolist()
                        pos += n * idt.itemsize
                    if name == "face" and p[0] in ("vertex_indices", "vertex_index"):
                        lists.append(item)
        if name == "face":
            polygons = lists
    rec, types = vertex
    if not all(k in rec for k in "xyz"):
        raise ValueError("load_ply: the vertex element lacks x, y or z")
    v = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32)
    colours = None
    if all(k in rec for k in ("red", "green", "blue")):
        c = np.stack([rec["red"], rec["green"], rec["blue"]], axis=1).astype(np.float64)
        colours = torch.from_numpy((c / 255.0 if types["red"] == "u1" else c).astype(np.float32))
    if isinstance(polygons, np.ndarray) and polygons.ndim == 2 and polygons.shape[1] == 3:
        f = polygons
    else:
        f = _fan([p for p in polygons if len(p) >= 3])
    if f.size and (f.min() < -2 ** 31 or f.max() >= 2 ** 31):
        raise ValueError("load_ply: a vertex index does not fit an int32")
    return Mesh(torch.from_numpy(v.reshape(-1, 3).copy()), torch.from_numpy(f.astype(np.int32).reshape(-1, 3)), colours)


def iso_value(post_act: int, level: float) -> Optional[float]:
    """L = post^-1(level) in the domain the density pre-activation maps into, as the mesh export computes it (float32); None
    when level <= post(0)"""
    from voxe_hip import abi

    level = float(np.float32(level))
    if post_act == abi.ACT_SOFTPLUS:
        if not level > float(np.float32(math.log(2.0))):
            return None
        return float(np.float32(level if level > 20.0 else math.log(math.expm1(level))))
    return level if level > 0.0 else None


def mesh_to_voxel_grid(mesh: Mesh, like: VoxelGrid, level: Optional[float] = None, band_voxels: float = 2.0,
                       inside_ratio: float = 2.0, allow_open: bool = False, return_stats: bool = False):
    """A new VoxelGrid with `like`'s dims, AABB, activations, density scale and SH degree whose density iso-surface at `level`
    (default default_level(like)) is the mesh: with sd the signed distance of a voxel centre (negative inside, clamped to the
    band h = band_voxels * min(voxel size)), L = iso_value(post, level) and e the field's empty value before the
    post-activation (0, or -20 under Softplus), the pre-activated density is v = L - (L - e) clamp(sd / h, -(inside_ratio - 1), 1)
    -- L on the surface, e from h outside on, saturating inside -- and the raw density v / density scale.  Vertex colours go
    into the DC coefficients inside the band (logit(clamp(c, 1/510, 1 - 1/510)) / C0; mid grey without colours); every other
    feature is 0.  ValueError: a field without an empty value (abs + Softplus), level at or below it, a malformed triangle,
    or -- unless allow_open -- a mesh that is not closed (columns with an odd number of crossings).  Not differentiable."""
    from thre3d_atom.thre3d_reprs.visibility import empty_raw_density
    from voxe_hip import abi

    spec = like.voxe_grid_spec()
    pre, post, scale = spec.density_pre_act, spec.density_post_act, float(spec.density_scale)
    empty = scale * empty_raw_density(pre, post, scale)       # (ValueError: abs + Softplus)
    e = abs(empty) if pre == abi.ACT_ABS else empty
    if level is None:
        level = default_level(like)
    L = iso_value(post, level)
    if L is None or not L > e:
        raise ValueError(f"mesh_to_voxel_grid: level {level} is not above the field's empty value")
    if not band_voxels > 0 or not inside_ratio >= 1:
        raise ValueError("mesh_to_voxel_grid: band_voxels must be > 0 and inside_ratio >= 1")
    device = like.densities.device
    h = float(band_voxels) * min(float(s) for s in like.voxel_size)
    colours = None if mesh.colours is None else mesh.colours.to(device)
    sdf, nearest, cols, _, stats = _ops.voxelize_mesh(mesh.vertices.to(device), mesh.faces.to(device), colours, like.grid_dims,
                                                       spec.aabb, h)
    if stats[1]:
        raise ValueError(f"mesh_to_voxel_grid: {stats[1]} malformed triangles (an index outside the vertices, a non-finite "
                         "vertex or one more than 1024 voxels from the grid's origin)")
    if stats[0] and not allow_open:
        raise ValueError(f"mesh_to_voxel_grid: the mesh is not closed ({stats[0]} columns with an odd number of crossings); "
                         "allow_open=True imports it regardless")
    with torch.no_grad():
        # (python scalars: torch rounds each to float32 and every operation on its own, like tests/voxelize_ref.fields)
        s = torch.clamp(sdf / float(np.float32(h)), min=-(float(inside_ratio) - 1.0), max=1.0)
        v = float(L) - float(np.float32(L - e)) * s
        densities = (v / float(np.float32(scale)))[..., None].contiguous()
        features = torch.zeros_like(like.features.detach(), dtype=torch.float32, device=device)
        ncoef = features.shape[-1] // 3
        if colours is not None:
            dc = torch.logit(torch.clamp(cols.double(), 1.0 / 510.0, 1.0 - 1.0 / 510.0)) / C0
            features[..., 0:3 * ncoef:ncoef] = torch.where((nearest >= 0)[..., None], dc, torch.zeros_like(dc)).float()
    grid = VoxelGrid(densities, features, like.voxel_size, **like.get_config_dict())
    return (grid, stats) if return_stats else grid
