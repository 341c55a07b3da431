"""CPU checks of the density-gradient normals: the C ABI's declarations and argument validation (no device work), the float64
restatement tests/normals_ref.py on an analytic field, the camera-space / display helpers, the PLY writer's normals and the
new entry-point options."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import torch

import normals_ref
from conftest import ROOT
from test_mesh_host import parse_ply
from voxe_hip import abi
from voxe_hip.desc import make_grid_desc, make_render_cfg

AABB = [(-1.0, 1.4), (-0.6, 0.9), (-1.2, 0.3)]


def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


def test_normals_symbols_are_declared_with_no_cpu_twin_and_abi_13():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    for name in ("voxe_query_normals", "voxe_render_normals"):
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols()
    assert not re.search(r"\bvoxe_cpu_\w*normals", text)
    assert not any("normals" in s for s in abi.cpu_symbols())
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text
    L = _lib()
    assert L.voxe_abi_version() == 13
    assert hasattr(L, "voxe_query_normals") and hasattr(L, "voxe_render_normals")


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    g = make_grid_desc(16, 0, (8, 6, 5), 3, AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)   # features NULL: not read
    c = make_render_cfg(32, 1.0, 4.0)
    q = lambda g_, pts=P, n=4, out=P: L.voxe_query_normals(ctypes.byref(g_) if g_ else None, pts, n, out, None)  # noqa: E731

    def r(g_=g, c_=c, ro=P, rd=P, R=4, nrm=P):
        return L.voxe_render_normals(ctypes.byref(g_) if g_ else None, ctypes.byref(c_) if c_ else None, ro, rd, R, None, nrm,
                                     None, None, None)

    # NULL pointers
    assert q(None) == abi.ERR_NULL_POINTER and r(g_=None) == abi.ERR_NULL_POINTER
    assert r(c_=None) == abi.ERR_NULL_POINTER
    assert q(g, pts=None) == abi.ERR_NULL_POINTER and q(g, out=None) == abi.ERR_NULL_POINTER
    for kw in ({"ro": None}, {"rd": None}, {"nrm": None}):
        assert r(**kw) == abi.ERR_NULL_POINTER, kw
    g.densities = 0
    assert q(g) == abi.ERR_NULL_POINTER and r(g) == abi.ERR_NULL_POINTER
    g.densities = 16
    # shapes
    assert q(g, n=-1) == abi.ERR_BAD_SHAPE and r(R=-1) == abi.ERR_BAD_SHAPE
    for dims in ((0, 6, 5), (8, -1, 5), (1300, 1300, 1300), (1 << 12, 1 << 12, 2), (2, 2, 1 << 24)):
        g.X, g.Y, g.Z = dims
        assert q(g) == abi.ERR_BAD_SHAPE and r(g) == abi.ERR_BAD_SHAPE, dims
    g.X, g.Y, g.Z = 8, 6, 5
    c.num_samples = 0
    assert r(c_=c) == abi.ERR_BAD_SHAPE
    c.num_samples = 32
    # activations
    g.density_post_act = 9
    assert q(g) == abi.ERR_UNSUPPORTED and r(g) == abi.ERR_UNSUPPORTED
    g.density_post_act, g.density_pre_act = abi.ACT_RELU, 5
    assert q(g) == abi.ERR_UNSUPPORTED and r(g) == abi.ERR_UNSUPPORTED
    g.density_pre_act = abi.ACT_ABS
    # empty calls: no launch, NULL buffers allowed
    assert q(g, pts=None, n=0, out=None) == abi.OK
    assert L.voxe_render_normals(ctypes.byref(g), ctypes.byref(c), None, None, 0, None, None, None, None, None) == abi.OK
    # feature kind / F are not read
    g.feature_kind, g.F = 7, 0
    assert q(g, pts=None, n=0, out=None) == abi.OK


def test_restatement_reproduces_a_linear_ramp_on_an_anisotropic_grid():
    dims = (9, 13, 6)
    a = torch.tensor([0.7, -1.9, 0.4], dtype=torch.float64)
    size = [(hi - lo) / n for (lo, hi), n in zip(AABB, dims)]
    axes = [torch.tensor([AABB[k][0] + (i + 0.5) * size[k] for i in range(dims[k])], dtype=torch.float64) for k in range(3)]
    x, y, z = torch.meshgrid(*axes, indexing="ij")
    v = (a[0] * x + a[1] * y + a[2] * z + 0.3).to(torch.float32)
    gen = torch.Generator().manual_seed(3)
    # points whose cell has all 8 corners inside the grid (voxel centres span u in [0, N-1])
    lo = torch.tensor([AABB[k][0] + 0.5 * size[k] for k in range(3)])
    span = torch.tensor([(dims[k] - 1) * size[k] for k in range(3)])
    pts = lo + torch.rand((4000, 3), generator=gen) * span * 0.999
    V, G = normals_ref.value_and_gradient(v, pts, AABB)
    assert torch.allclose(G, a.expand_as(G), atol=1e-5), (G - a).abs().max()
    n = normals_ref.point_normals(v, pts, AABB)
    assert torch.allclose(n, (-a / a.norm()).expand_as(n), atol=1e-6)
    ref = (pts.to(torch.float64) @ a + 0.3)
    assert torch.allclose(V, ref, atol=1e-5)
    # a constant grid has no gradient anywhere inside: exact zeros
    n0 = normals_ref.point_normals(torch.full(dims, 0.8), pts, AABB)
    assert bool((n0 == 0).all())


def test_camera_space_and_display_colour():
    from thre3d_atom.thre3d_reprs.geometry import normals_to_camera, normals_to_rgb
    from thre3d_atom.utils.imaging_utils import pose_spherical, to8b

    pose = pose_spherical(30.0, 20.0, 4.0)
    rot = torch.as_tensor(pose.rotation, dtype=torch.float32)
    # the world direction toward the camera centre (its +z axis) is a facing surface normal: (0, 0, 1) in camera space
    facing = rot[:, 2][None]
    cam = normals_to_camera(facing, pose)
    assert torch.allclose(cam, torch.tensor([[0.0, 0.0, 1.0]]), atol=1e-6)
    rgb = normals_to_rgb(torch.tensor([[0.0, 0.0, 1.0]]), torch.ones(1, 1))
    assert np.array_equal(rgb, to8b(np.array([[0.5, 0.5, 1.0]])))
    white = normals_to_rgb(torch.zeros(1, 3), torch.zeros(1, 1))
    assert np.array_equal(white, np.full((1, 3), 255, np.uint8))


def test_save_ply_with_and_without_normals(tmp_path):
    from thre3d_atom.thre3d_reprs.mesh import Mesh, save_ply

    rng = np.random.default_rng(4)
    v = rng.random((17, 3)).astype(np.float32)
    f = rng.integers(0, 17, (9, 3)).astype(np.int32)
    col = rng.random((17, 3)).astype(np.float32)
    nrm = rng.standard_normal((17, 3)).astype(np.float32)
    mesh = Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(col))
    save_ply(mesh, tmp_path / "a.ply")
    save_ply(mesh, tmp_path / "b.ply", normals=None)
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes()
    save_ply(mesh, tmp_path / "n.ply", normals=torch.from_numpy(nrm))
    xyz, n, rgb, idx = parse_ply_normals(tmp_path / "n.ply")
    assert np.array_equal(xyz, v) and np.array_equal(n, nrm) and np.array_equal(idx, f)
    assert np.array_equal(rgb, np.rint(col * 255).astype(np.uint8))
    assert np.array_equal(parse_ply(tmp_path / "a.ply")[0], v)


def parse_ply_normals(path):
    """x y z nx ny nz (float) red green blue (uchar) per vertex, as save_ply(normals=...) writes them"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode().splitlines()
    props = [h.split()[-1] for h in header if h.startswith("property float") or h.startswith("property uchar")]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"], props
    nv = int(next(h for h in header if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in header if h.startswith("element face")).split()[-1])
    vt = np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    ft = np.dtype([("c", "u1"), ("idx", "<i4", 3)])
    assert len(data) == end + nv * vt.itemsize + nf * ft.itemsize
    verts = np.frombuffer(data, vt, nv, end)
    faces = np.frombuffer(data, ft, nf, end + nv * vt.itemsize)
    return verts["xyz"], verts["n"], verts["rgb"], faces["idx"]


def _cli(name):
    spec = importlib.util.spec_from_file_location(name[:-3], os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_new_entry_point_options_exist_and_default_off():
    for script, flag in (("render_sh_based_voxel_grid.py", "render_geometry"), ("export_mesh.py", "vertex_normals")):
        opts = {p.name: p for p in _cli(script).main.params}
        assert flag in opts, (script, flag)
        assert opts[flag].is_flag and opts[flag].default is False, (script, flag)
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "--render_geometry" in text and "--vertex_normals" in text, doc
    assert "4.9" in open(os.path.join(ROOT, "DESIGN.md")).read()
