"""Rigid transform, re-gridding and composition of VoxelGrids (DESIGN.md section 4.12 "Transform").  Not in the reference.

The scene-frame map is  p' = s R p + t  with R orthogonal (det +1 or -1: mirrors are allowed), s > 0 and t in world units.
Every voxel of a destination lattice samples the source grid trilinearly at the pre-image of its centre
(voxe_transform.hip, one pass over the destination); the SH coefficients of degree 1..3 grids are rotated band by band with
the geometry, so view-dependent colour moves with the object.  The map between the two lattices is

    u = A i + b,    A = diag(1/v_s) (R^T / s) diag(v_d),    b = diag(1/v_s) ((R^T / s)(lo_d + v_d / 2 - t) - lo_s) - 1/2

(i the destination voxel index, u the continuous source index with voxel centres at the integers), computed here in float64.

Uniform scale is geometric only: raw values are not compensated, so the optical depth through a scaled object scales by s.
Nothing here is differentiable.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from thre3d_atom.thre3d_reprs.visibility import empty_raw_density
from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelGridLocation, VoxelSize, density_activation_codes
from voxe_hip import abi
from voxe_hip import ops as _ops

_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435)
_NUM_FIT_DIRECTIONS = 256


def sh_basis(degree: int, v: np.ndarray) -> np.ndarray:
    """[N, (degree+1)^2] float64 values of the renderer's real SH basis (voxe_device.hpp sh_basis, signs included) at the unit
    directions v [N,3]."""
    v = np.asarray(v, dtype=np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    out = [np.full_like(x, 0.28209479177387814)]
    if degree > 0:
        out += [-_C1 * y, _C1 * z, -_C1 * x]
    if degree > 1:
        xx, yy, zz = x * x, y * y, z * z
        out += [_C2[0] * x * y, _C2[1] * y * z, _C2[2] * (2.0 * zz - xx - yy), _C2[3] * x * z, _C2[4] * (xx - yy)]
    if degree > 2:
        out += [_C3[0] * y * (3 * xx - yy), _C3[1] * x * y * z, _C3[2] * y * (4 * zz - xx - yy),
                _C3[3] * z * (2 * zz - 3 * xx - 3 * yy), _C3[4] * x * (4 * zz - xx - yy), _C3[5] * z * (xx - yy),
                _C3[6] * x * (xx - 3 * yy)]
    return np.stack(out, axis=-1)


def _orthogonal(rotation) -> np.ndarray:
    R = np.asarray(rotation.detach().cpu() if isinstance(rotation, Tensor) else rotation, dtype=np.float64)
    if R.shape != (3, 3) or not np.allclose(R @ R.T, np.eye(3), atol=1e-6):
        raise ValueError(f"rotation must be an orthogonal 3x3 matrix (a rotation or a mirror); got\n{R}")
    return R


def sh_rotation_matrices(R, degree: int) -> List[np.ndarray]:
    """[M_0 .. M_degree], float64, M_l of shape (2l+1, 2l+1) with  b_l(R^T v)^T = b_l(v)^T M_l  for every unit v: the
    coefficients of a scene moved by R are c'_l = M_l c_l per colour channel.  Obtained by least squares over fixed-seed unit
    directions and the same directions times R (the bands are rotation invariant and the directions over-determine every
    block, so the fit is exact to rounding); no Wigner formulas.  degree -1 gives an empty list."""
    if not -1 <= degree <= 3:
        raise ValueError("only SH degrees 0..3 (or -1: no SH) are supported")
    R = _orthogonal(R)
    v = np.random.default_rng(20240229).normal(size=(_NUM_FIT_DIRECTIONS, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if degree < 0:
        return []
    here, there = sh_basis(degree, v), sh_basis(degree, v @ R)   # rows of v @ R are (R^T v)^T
    blocks = []
    for l in range(degree + 1):
        band = slice(l * l, (l + 1) * (l + 1))
        blocks.append(np.linalg.lstsq(here[:, band], there[:, band], rcond=None)[0])
    return blocks


def _edges_and_low_corner(grid: VoxelGrid) -> Tuple[np.ndarray, np.ndarray]:
    lo = np.array([float(r[0]) for r in grid.aabb], dtype=np.float64)
    hi = np.array([float(r[1]) for r in grid.aabb], dtype=np.float64)
    return (hi - lo) / np.array(grid.grid_dims, dtype=np.float64), lo


def resample_index_map(src_grid: VoxelGrid, dst_dims: Sequence[int], dst_voxel_size: Sequence[float],
                       dst_location: Sequence[float], R, t: Sequence[float] = (0.0, 0.0, 0.0),
                       s: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """(A [3,3], b [3]) in float64 of the map from destination voxel indices to continuous source indices for the scene-frame
    map p' = s R p + t; the destination lattice has `dst_dims` voxels of edges `dst_voxel_size` centred at `dst_location`."""
    R = _orthogonal(R)
    if not float(s) > 0.0:
        raise ValueError(f"scale must be positive; got {s}")
    v_s, lo_s = _edges_and_low_corner(src_grid)
    v_d = np.array([float(e) for e in dst_voxel_size], dtype=np.float64)
    dims = np.array([int(n) for n in dst_dims], dtype=np.float64)
    lo_d = np.array([float(c) for c in dst_location], dtype=np.float64) - (dims * v_d) / 2
    inv = R.T / float(s)
    A = (inv * v_d[None, :]) / v_s[:, None]
    b = (inv @ (lo_d + 0.5 * v_d - np.array([float(c) for c in t], dtype=np.float64)) - lo_s) / v_s - 0.5
    return A, b


def _axis_permutation(R: np.ndarray) -> Optional[List[int]]:
    """source axis feeding each destination axis when R is exactly a signed permutation (quarter turns, mirrors), else None"""
    if not np.all((R == 0) | (np.abs(R) == 1)):
        return None
    return [int(np.argmax(np.abs(R[a]))) for a in range(3)]


def default_output_lattice(grid: VoxelGrid, R) -> Tuple[Tuple[int, int, int], Tuple[float, float, float]]:
    """(dims, voxel edges) transform_voxel_grid gives its output by default: the source's own, permuted along when R is
    exactly a signed permutation"""
    perm = _axis_permutation(_orthogonal(R))
    dims, edges = grid.grid_dims, tuple(float(e) for e in grid.voxel_size)
    if perm is not None:
        dims, edges = tuple(dims[k] for k in perm), tuple(edges[k] for k in perm)
    return dims, edges


def _density_fill(grid: VoxelGrid) -> Tuple[int, float]:
    pre, post = density_activation_codes(grid._density_preactivation, grid._density_postactivation)
    return pre, empty_raw_density(pre, post, float(grid._expected_density_scale))


def _sh_degree_of(features: Tensor) -> int:
    n = int(features.shape[-1])
    for deg in range(4):
        if n == 3 * (deg + 1) ** 2:
            return deg
    raise ValueError(f"features with {n} channels are not SH coefficients of degree 0..3 (3, 12, 27 or 48 channels)")


def transform_voxel_grid(grid: VoxelGrid, rotation, translation: Sequence[float] = (0.0, 0.0, 0.0), scale: float = 1.0,
                         output_dims: Optional[Sequence[int]] = None, output_voxel_size: Optional[Sequence[float]] = None,
                         output_location: Optional[Sequence[float]] = None) -> VoxelGrid:
    """A new VoxelGrid holding `grid` moved by p' = scale * rotation @ p + translation, SH coefficients rotated along; `grid` is
    not changed.  The output lattice defaults to the source's own (dims, voxel size, location); when `rotation` is exactly a
    signed permutation (quarter turns, mirrors) the default dims and voxel edges are the permuted ones, so the turn maps the
    lattice onto itself.  Space the source does not cover gets the field's empty density (0 for Identity / ReLU, -20 / density
    scale for Softplus; ValueError for Softplus on abs, which has none -- the rule of prune_voxel_grid_) and zero features.
    Under the abs pre-activation the stored densities are the interpolated |raw| values.  An attention grid is carried along
    (plain channel, fill 0)."""
    R = _orthogonal(rotation)
    pre, fill = _density_fill(grid)
    degree = _sh_degree_of(grid.features)
    src_dims, src_edges = default_output_lattice(grid, R)
    dims = tuple(int(n) for n in (output_dims if output_dims is not None else src_dims))
    edges = tuple(float(e) for e in (output_voxel_size if output_voxel_size is not None else src_edges))
    location = tuple(float(c) for c in (output_location if output_location is not None else grid._grid_location))
    A, b = resample_index_map(grid, dims, edges, location, R, translation, scale)
    xf = _ops.make_resample(A, b, sh_rotation_matrices(R, degree), degree, pre, fill, abi.RESAMPLE_REPLACE)
    densities, features, _ = _ops.grid_resample(grid.densities, grid.features, xf, dst_dims=dims)
    attn = None
    if grid.attn is not None:
        plain = _ops.make_resample(A, b, None, -1, abi.ACT_IDENTITY, 0.0, abi.RESAMPLE_REPLACE)
        attn = _ops.grid_resample(None, grid.attn, plain, dst_dims=dims)[1]
    config = grid.get_config_dict()
    config["grid_location"] = VoxelGridLocation(*location)
    return VoxelGrid(densities=densities, features=features, voxel_size=VoxelSize(*edges), attn=attn, **config)


def compose_voxel_grids_(dst_grid: VoxelGrid, src_grid: VoxelGrid, rotation, translation: Sequence[float] = (0.0, 0.0, 0.0),
                         scale: float = 1.0) -> Tensor:
    """Drop `src_grid`, moved by p' = scale * rotation @ p + translation, into `dst_grid` in place: the CSG union of the two
    pre-activation density fields on the destination's lattice.  A destination voxel is replaced -- density and all features
    -- where the source sample lies wholly inside the source lattice and is strictly denser than the destination; every other
    voxel keeps its bits.  Returns `taken`, uint8 [X,Y,Z] of the destination: 1 where the source won.  When both grids carry
    an attention grid, the destination's takes the source's values where taken.  Both grids must agree on the density
    activations, the density scale and the SH degree: ValueError otherwise."""
    R = _orthogonal(rotation)
    if dst_grid is src_grid:
        raise ValueError("source and destination must be different grids")
    pre, _ = _density_fill(src_grid)
    acts = [density_activation_codes(g._density_preactivation, g._density_postactivation) for g in (dst_grid, src_grid)]
    if acts[0] != acts[1]:
        raise ValueError(f"the grids disagree on the density activations (codes {acts[0]} vs {acts[1]})")
    if float(dst_grid._expected_density_scale) != float(src_grid._expected_density_scale):
        raise ValueError(f"the grids disagree on the density scale ({dst_grid._expected_density_scale} vs "
                         f"{src_grid._expected_density_scale})")
    degree = _sh_degree_of(src_grid.features)
    if _sh_degree_of(dst_grid.features) != degree:
        raise ValueError(f"the grids disagree on the SH degree ({_sh_degree_of(dst_grid.features)} vs {degree})")
    A, b = resample_index_map(src_grid, dst_grid.grid_dims, dst_grid.voxel_size, dst_grid._grid_location, R, translation, scale)
    xf = _ops.make_resample(A, b, sh_rotation_matrices(R, degree), degree, pre, 0.0, abi.RESAMPLE_UNION)
    # the kernel runs in place on private copies, which are then copied back through torch: the tensors' version counters move,
    # so nothing keyed on them (packed grids, forward records) outlives the edit
    densities = dst_grid.densities.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
    features = dst_grid.features.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
    _, _, taken = _ops.grid_resample(src_grid.densities, src_grid.features, xf, dst_densities=densities, dst_features=features,
                                     want_taken=True)
    with torch.no_grad():
        dst_grid.densities.copy_(densities)
        dst_grid.features.copy_(features)
        if dst_grid.attn is not None and src_grid.attn is not None:
            plain = _ops.make_resample(A, b, None, -1, abi.ACT_IDENTITY, 0.0, abi.RESAMPLE_REPLACE)
            moved = _ops.grid_resample(None, src_grid.attn, plain, dst_dims=dst_grid.grid_dims)[1]
            dst_grid.attn.copy_(torch.where(taken[..., None] != 0, moved, dst_grid.attn.detach()))
    return taken
