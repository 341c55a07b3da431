"""CPU checks of the grid transform feature: the SH rotation blocks, the float64 restatement
tests/transform_ref.py against analytic affine fields and against numpy's transpose / flip / shift on lattice-preserving maps,
the conventions end to end on the CPU oracle (a moved grid rendered from moved rays gives the same image), and the C ABI's
declarations and argument validation.  tests/test_transform_gpu.py builds its inputs with the functions below."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import transform_ref as T
from conftest import ROOT
from voxe_hip import abi, workload
from voxe_hip.desc import make_render_cfg

ORTHOGONALS = [(seed, det) for seed in range(5) for det in (1, -1)]   # ten random orthogonal matrices of both determinants
GENERIC_R = T.rotation_about("z", 31.0) @ T.rotation_about("x", -17.0) @ T.rotation_about("y", 52.0)


def _product():
    from thre3d_atom.thre3d_reprs import transform

    return transform


# ---- 1: SH rotation blocks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_rotation_matrices(degree):
    tr = _product()
    n = (degree + 1) ** 2
    fresh = T.unit_directions(500, seed=77)
    rng = np.random.default_rng(degree)
    worst = 0.0
    for seed, det in ORTHOGONALS:
        R = T.random_orthogonal(seed, det)
        assert np.sign(np.linalg.det(R)) == det
        blocks = tr.sh_rotation_matrices(R, degree)
        assert [m.shape for m in blocks] == [(2 * l + 1, 2 * l + 1) for l in range(degree + 1)]
        M = np.zeros((n, n))
        for l, m in enumerate(blocks):
            M[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = m
            assert np.abs(m @ m.T - np.eye(2 * l + 1)).max() <= 1e-12            # every block orthogonal
        c = rng.normal(size=(n,))
        # b(R^T v) . c = b(v) . (M c) on directions the fit has not seen (rows of fresh @ R are (R^T v)^T)
        err = np.abs(T.sh_basis(degree, fresh @ R) @ c - T.sh_basis(degree, fresh) @ (M @ c)).max()
        worst = max(worst, err)
        assert err <= 1e-12
        R2 = T.random_orthogonal(seed + 100, -det)
        both, second = tr.sh_rotation_matrices(R @ R2, degree), tr.sh_rotation_matrices(R2, degree)
        for l in range(degree + 1):
            assert np.abs(both[l] - blocks[l] @ second[l]).max() <= 1e-12       # M(R1 R2) = M(R1) M(R2)
    print(f"degree {degree}: max |b(R^T v).c - b(v).(M c)| {worst:.2e}")
    for l, m in enumerate(tr.sh_rotation_matrices(np.eye(3), degree)):
        assert np.abs(m - np.eye(2 * l + 1)).max() <= 1e-13
    assert np.abs(tr.sh_basis(degree, fresh) - T.sh_basis(degree, fresh)).max() <= 1e-15
    with pytest.raises(ValueError):
        tr.sh_rotation_matrices(np.diag([1.0, 2.0, 1.0]), degree)


# ---- 2: affine fields ---------------------------------------------------------------------------------------------------------
AFFINE = dict(dims_s=(13, 9, 17), v_s=(0.21, 0.33, 0.17), loc_s=(0.1, -0.2, 0.05), dims_d=(11, 15, 10), v_d=(0.19, 0.14, 0.26),
              loc_d=(0.15, 0.0, -0.1), t=(0.12, -0.08, 0.05), s=1.3)


def _lo(dims, edges, loc):
    return tuple(c - (n * e) / 2 for n, e, c in zip(dims, edges, loc))


def _centres(dims, lo, edges):
    g = np.meshgrid(*(lo[a] + (np.arange(dims[a]) + 0.5) * edges[a] for a in range(3)), indexing="ij")
    return np.stack(g, axis=-1)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_affine_fields_are_reproduced_with_rotated_coefficients(degree):
    tr = _product()
    k = AFFINE
    n = 3 * (degree + 1) ** 2
    rng = np.random.default_rng(10 + degree)
    g_d, c_d = rng.normal(size=3), rng.normal()
    g_f, c_f = rng.normal(size=(n, 3)), rng.normal(size=n)
    lo_s, lo_d = _lo(k["dims_s"], k["v_s"], k["loc_s"]), _lo(k["dims_d"], k["v_d"], k["loc_d"])
    p = _centres(k["dims_s"], lo_s, k["v_s"])
    src_d = torch.from_numpy(p @ g_d + c_d)[..., None]
    src_f = torch.from_numpy(p @ g_f.T + c_f)
    A, b = T.index_map(k["dims_s"], lo_s, k["v_s"], k["dims_d"], lo_d, k["v_d"], GENERIC_R, k["t"], k["s"])
    blocks = tr.sh_rotation_matrices(GENERIC_R, degree)
    out = T.resample(src_d, src_f, k["dims_d"], A, b, blocks, degree, fill=-3.0)
    # the analytic answer: the fields at the pre-image of every destination centre, coefficients rotated analytically
    q = (_centres(k["dims_d"], lo_d, k["v_d"]) - np.array(k["t"])) @ GENERIC_R / k["s"]        # rows: (R^T (p' - t) / s)^T
    want_d = torch.from_numpy(q @ g_d + c_d)
    want_f = T.rotate_coefficients(torch.from_numpy(q @ g_f.T + c_f), blocks, degree)
    u = out["u"]
    whole = torch.ones(k["dims_d"], dtype=torch.bool)
    for a in range(3):
        whole &= (u[..., a] >= 0) & (u[..., a] <= k["dims_s"][a] - 1)
    assert bool(out["valid"][whole].all())
    assert int(whole.sum()) * 3 >= whole.numel(), f"only {int(whole.sum())} of {whole.numel()} footprints lie in the lattice"
    err_d = float((out["densities"][..., 0] - want_d)[whole].abs().max())
    err_f = float((out["features"] - want_f)[whole].abs().max())
    print(f"degree {degree}: {int(whole.sum())}/{whole.numel()} voxels, max err density {err_d:.2e} features {err_f:.2e}")
    assert err_d <= 1e-9 and err_f <= 1e-9
    # the product's index map is the contract's
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelGridLocation, VoxelSize

    grid = VoxelGrid(src_d.float(), src_f.float(), VoxelSize(*k["v_s"]), VoxelGridLocation(*k["loc_s"]))
    A2, b2 = tr.resample_index_map(grid, k["dims_d"], k["v_d"], k["loc_d"], GENERIC_R, k["t"], k["s"])
    assert np.abs(A2 - A).max() <= 1e-13 and np.abs(b2 - b).max() <= 1e-12


# ---- 3: lattice-preserving maps -----------------------------------------------------------------------------------------------
LATTICE_DIMS, LATTICE_EDGES = (7, 5, 6), (0.3, 0.21, 0.17)


def lattice_inputs(degree=0, seed=4):
    g = torch.Generator().manual_seed(seed)
    dens = torch.randn((*LATTICE_DIMS, 1), generator=g)
    feat = torch.randn((*LATTICE_DIMS, 3 * (degree + 1) ** 2), generator=g)
    return dens, feat


@pytest.mark.parametrize("case", T.lattice_cases(), ids=lambda c: c[0])
def test_lattice_preserving_maps_are_exact_permutations(case):
    _, R, shift = case
    dens, feat = lattice_inputs()
    dims_d, _, _, A, b = T.lattice_setup(LATTICE_DIMS, LATTICE_EDGES, R, shift)
    assert set(np.unique(A)) <= {-1.0, 0.0, 1.0} and np.abs(b - np.round(b)).max() < 1e-12
    A32, b32 = T.as_kernel_args(A, b)
    fill = -1.5
    want_d, want_f = T.permute_by(dens.numpy(), R, shift, fill), T.permute_by(feat.numpy(), R, shift, 0.0)
    assert want_d.shape[:3] == dims_d and int((want_d == fill).sum()) > 0
    # in the kernel's number format every step of the contract is exact on these maps
    out = T.resample(dens, feat, dims_d, A32, b32, [np.eye(1)], 0, fill=fill, dtype=torch.float32)
    assert np.array_equal(out["densities"].numpy(), want_d) and np.array_equal(out["features"].numpy(), want_f)
    assert np.array_equal(out["taken"].numpy(), T.permute_by(np.ones((*LATTICE_DIMS, 1), np.float32), R, shift, 0.0)[..., 0] == 1)
    # in float64 the rounding tails of b (|b - round(b)| ~ 1e-16) stay visible at that size
    out64 = T.resample(dens, feat, dims_d, A32, b32, [np.eye(1)], 0, fill=fill)
    assert float((out64["densities"].numpy() - want_d).__abs__().max()) <= 1e-12
    assert float((out64["features"].numpy() - want_f).__abs__().max()) <= 1e-12


# ---- 4: the conventions end to end, on the oracle -----------------------------------------------------------------------------
ORACLE_DIMS, ORACLE_EDGE, ORACLE_HW, ORACLE_S = (12, 10, 14), 0.25, 32, 96
ORACLE_CASES = [("quarter_z", T.quarter_turn("z", 1), (1, -1, 1)), ("quarter_x", T.quarter_turn("x", 1), (-1, 1, 0))]


def oracle_grid(degree):
    """ReLU grid (empty value 0, so content may be shifted: the renderer pads the lattice with raw 0), random N(0,1) features,
    density carved to 0 outside |normalised coordinate| < 0.6: every non-empty voxel is >= 2 voxels off every face"""
    g = torch.Generator().manual_seed(21 + degree)
    dens = torch.empty((*ORACLE_DIMS, 1)).uniform_(1.0, 6.0, generator=g)
    feat = torch.randn((*ORACLE_DIMS, 3 * (degree + 1) ** 2), generator=g)
    keep = torch.ones(ORACLE_DIMS, dtype=torch.bool)
    for a, n in enumerate(ORACLE_DIMS):
        c = (2 * (torch.arange(n) + 0.5) / n - 1).abs() < 0.6
        keep &= c.reshape([-1 if k == a else 1 for k in range(3)])
    dens[~keep] = 0.0
    return dens, feat


def oracle_rays():
    from oracle import voxe_oracle as vo
    from thre3d_atom.utils.imaging_utils import pose_spherical

    pose = pose_spherical(*workload.synth_pose_angles(1, 8), workload.RADIUS)
    return vo.cast_rays(ORACLE_HW, ORACLE_HW, workload.focal_for(ORACLE_HW), pose.rotation.numpy(), pose.translation.numpy())


def moved_rays(o, d, R, t):
    return ((o.astype(np.float64) @ R.T + np.asarray(t)).astype(np.float32), (d.astype(np.float64) @ R.T).astype(np.float32))


def aabb_of(dims, edges):
    return tuple((-(n * e) / 2, (n * e) / 2) for n, e in zip(dims, edges))


def _oracle_render(dens, feat, dims, edges, degree, o, d):
    from oracle import voxe_oracle as vo

    grid = vo.Grid(dens.numpy(), feat.numpy(), aabb_of(dims, edges), 1.0, abi.ACT_IDENTITY, abi.ACT_RELU)
    cfg = make_render_cfg(ORACLE_S, workload.NEAR, workload.FAR, sh_degree=degree)
    out = vo.render_fwd(grid, cfg, o, d)
    return out["colour"], out["acc"]


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: c[0])
def test_moved_grid_renders_the_same_image_from_moved_rays(case, degree):
    tr = _product()
    _, R, shift = case
    dens, feat = oracle_grid(degree)
    edges = (ORACLE_EDGE,) * 3
    o, d = oracle_rays()
    colour, acc = _oracle_render(dens, feat, ORACLE_DIMS, edges, degree, o, d)
    assert float(acc.mean()) >= 0.05 and float(colour.std()) >= 0.05      # something is seen, and it is not flat
    dims_d, v_d, t, A, b = T.lattice_setup(ORACLE_DIMS, edges, R, shift)
    A32, b32 = T.as_kernel_args(A, b)
    o2, d2 = moved_rays(o, d, R, t)

    def moved(blocks):
        out = T.resample(dens, feat, dims_d, A32, b32, blocks, degree, fill=0.0)
        return _oracle_render(out["densities"].float(), out["features"].float(), dims_d, v_d, degree, o2, d2)

    colour2, acc2 = moved(tr.sh_rotation_matrices(R, degree))
    err_c, err_a = float(np.abs(colour2 - colour).max()), float(np.abs(acc2 - acc).max())
    print(f"{case[0]} degree {degree}: colour {err_c:.2e} acc {err_a:.2e}  (mean acc {acc.mean():.3f}, colour std {colour.std():.3f})")
    assert err_c <= 2e-6 and err_a <= 2e-6
    if degree >= 1:   # the transposition matters: with M(R^T) the view-dependent part lands in the wrong frame
        wrong, _ = moved(tr.sh_rotation_matrices(R.T, degree))
        assert float(np.abs(wrong - colour).max()) > 1e-3


# ---- 5: C ABI -----------------------------------------------------------------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


def test_resample_symbol_is_declared_with_no_cpu_twin_and_abi_13():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    assert re.search(r"\bvoxe_grid_resample\s*\(", text) and "voxe_grid_resample" in abi.hip_symbols()
    assert not re.search(r"\bvoxe_cpu_\w*resample", text) and not any("resample" in s for s in abi.cpu_symbols())
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text
    L = _lib()
    assert L.voxe_abi_version() == 13 and hasattr(L, "voxe_grid_resample")
    assert "voxe_transform.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    assert ctypes.sizeof(abi.VoxeResample) == 4 * (9 + 3 + 84 + 4)


def test_validation_without_a_device():
    from voxe_hip import ops

    L = _lib()
    P = ctypes.c_void_p(16)
    xf = ops.make_resample(np.eye(3), np.zeros(3))

    def call(sd=P, sf=P, dims=(4, 5, 6), C=3, dd=P, df=P, dims2=(3, 3, 3), x=xf, **fields):
        saved = {k: getattr(x, k) for k in fields} if x is not None else {}
        for k, v in fields.items():
            setattr(x, k, v)
        try:
            return L.voxe_grid_resample(sd, sf, *dims, C, dd, df, *dims2, ctypes.byref(x) if x is not None else None, None, None)
        finally:
            for k, v in saved.items():
                setattr(x, k, v)

    assert call(x=None) == abi.ERR_NULL_POINTER
    assert call(sd=None) == abi.ERR_NULL_POINTER and call(df=None) == abi.ERR_NULL_POINTER      # half a pair
    assert call(sd=None, dd=None, sf=None, df=None) == abi.ERR_NULL_POINTER
    assert call(sd=None, dd=None, mode=abi.RESAMPLE_UNION) == abi.ERR_NULL_POINTER               # UNION needs the densities
    assert call(mode=2) == abi.ERR_UNSUPPORTED and call(density_pre_act=abi.ACT_RELU) == abi.ERR_UNSUPPORTED
    assert call(sh_degree=4) == abi.ERR_UNSUPPORTED and call(sh_degree=-2) == abi.ERR_UNSUPPORTED
    assert call(C=3, sh_degree=1) == abi.ERR_BAD_SHAPE and call(C=65) == abi.ERR_BAD_SHAPE and call(C=0) == abi.ERR_BAD_SHAPE
    assert call(dims=(0, 5, 6)) == abi.ERR_BAD_SHAPE and call(dims2=(3, -1, 3)) == abi.ERR_BAD_SHAPE
    assert call(dims=(4096, 4096, 2)) == abi.ERR_BAD_SHAPE and call(dims2=(1024, 1024, 1024)) == abi.ERR_BAD_SHAPE
    with pytest.raises(ops.VoxeError):
        ops.make_resample(np.eye(3), np.zeros(3), None, 2)
    # make_resample fills identity blocks and the given ones at their offsets
    blocks = [np.eye(1), 2 * np.eye(3), 3 * np.eye(5)]
    x2 = ops.make_resample(np.eye(3), [1, 2, 3], blocks, 2, abi.ACT_ABS, -4.0, abi.RESAMPLE_UNION)
    rot = np.array(x2.sh_rot[:])
    assert rot[0] == 1 and np.array_equal(rot[1:10].reshape(3, 3), blocks[1]) and np.array_equal(rot[10:35].reshape(5, 5), blocks[2])
    assert np.array_equal(rot[35:].reshape(7, 7), np.eye(7))
    assert (x2.sh_degree, x2.density_pre_act, x2.mode, x2.density_fill, list(x2.b)) == (2, abi.ACT_ABS, 1, -4.0, [1.0, 2.0, 3.0])
