"""CPU checks of the mesh export: the generated case table (byte for byte, crack-free, wound outward), the numpy
restatement on analytic fields, the PLY writer, and the C ABI's declarations and argument validation (no device work)."""
import ctypes
import math
import os
import re
from collections import Counter

import numpy as np
import torch

import mesh_ref
from conftest import ROOT
from voxe_hip import abi, mc_table
from voxe_hip.desc import make_grid_desc


# ---- case table ---------------------------------------------------------------------------------------------------------
def test_generator_reproduces_committed_header():
    assert open(mc_table.HEADER).read() == mc_table.header_text()
    assert "voxe_mc_table.hpp" in open(os.path.join(ROOT, "vox-e_amd", "voxe_hip", "build.py")).read()


def _boundary(tris):
    """directed edges of the triangles that occur without their reverse (fan diagonals cancel): the loops' segments"""
    d = Counter()
    for t in tris:
        for q in range(3):
            d[(t[q], t[(q + 1) % 3])] += 1
    out = Counter()
    for (a, b), n in d.items():
        net = n - d.get((b, a), 0)
        if net > 0:
            out[(a, b)] += net
    return out


def _on_face(seg, face):
    fe = set(mc_table.face_edges(face))
    return seg[0] in fe and seg[1] in fe


def _face_boundary(case, face):
    return sorted(s for s, n in _boundary(mc_table.case_triangles(case)).items() for _ in range(n) if _on_face(s, face))


def test_every_loop_segment_lies_on_one_face_and_matches_the_face_rule():
    for case in range(256):
        bnd = _boundary(mc_table.case_triangles(case))
        assert all(n == 1 for n in bnd.values()), case
        for seg in bnd:
            assert sum(_on_face(seg, f) for f in mc_table.FACES) == 1, (case, seg)
        for face in mc_table.FACES:
            assert _face_boundary(case, face) == sorted(mc_table.face_segments(case, face)), (case, face)


def test_neighbouring_cells_leave_opposite_segments_on_their_shared_face():
    """cell A's face (a, 1) is cell B's face (a, 0): for every pair of cases that agree on those 4 corners, B's segments
    are A's, mapped across and reversed -- no cracks, consistent orientation"""
    def mapped(e, a):
        c0, _ = mc_table.edge_corners(e)
        return next(f for f in range(12) if f >> 2 == e >> 2 and mc_table.edge_corners(f)[0] == c0 ^ (1 << a))

    for a in range(3):
        hi = [c for c in range(8) if (c >> a) & 1]
        for ca in range(256):
            seg_a = sorted((mapped(y, a), mapped(x, a)) for x, y in _face_boundary(ca, (a, 1)))
            for cb in range(256):
                if all(((ca >> c) & 1) == ((cb >> (c ^ (1 << a))) & 1) for c in hi):
                    assert _face_boundary(cb, (a, 0)) == seg_a, (a, ca, cb)


def test_loops_wind_with_the_inside_on_the_correct_side():
    """walking a segment along d on a face with outward normal n, n x d points away from the inside corner(s) it bounds"""
    pos = lambda c: np.array(mc_table.corner_pos(c), float)  # noqa: E731
    for case in range(256):
        for face in mc_table.FACES:
            n = np.array(mc_table.face_normal(face))
            corners = mc_table.face_corners(face)
            inside = [c for c in corners if (case >> c) & 1]
            for ea, eb in _face_boundary(case, face):
                A, B = np.array(mc_table.edge_mid(ea)), np.array(mc_table.edge_mid(eb))
                side = np.cross(n, B - A)
                ends = set(mc_table.edge_corners(ea)) | set(mc_table.edge_corners(eb))
                if len(inside) == 2 and bin(inside[0] ^ inside[1]).count("1") == 2:   # diagonal: ambiguous face
                    cut = [c for c in inside if c in ends]   # ambiguous face: the one inside corner this segment cuts off
                    assert len(cut) == 1
                    assert np.dot(pos(cut[0]) - A, side) < 0, (case, face)
                    continue
                for c in corners:
                    s = np.dot(pos(c) - A, side)
                    assert (s < 0) if c in inside else (s > 0), (case, face, c)


def test_table_shape():
    assert mesh_ref.K == int(re.search(r"#define VOXE_MC_MAX_TRIS (\d+)", mc_table.header_text()).group(1))
    assert mesh_ref.TRI_COUNT[0] == 0 and mesh_ref.TRI_COUNT[255] == 0
    for case in range(256):   # one fan of len - 2 triangles per loop
        assert len(mc_table.case_triangles(case)) == sum(len(lp) - 2 for lp in mc_table.case_loops(case))


# ---- numpy restatement on analytic fields -------------------------------------------------------------------------------
AABB = [(-1.0, 1.0)] * 3


def test_sphere_is_closed_with_the_analytic_volume_and_area():
    n, r = 96, 0.6                     # surface radius 0.6 = 28.8 voxels
    v, f = mesh_ref.extract(mesh_ref.sphere_field(n, 2 * r), AABB, 0.5)
    assert mesh_ref.is_closed(f)
    assert mesh_ref.euler_characteristic(f) == 2
    assert abs(mesh_ref.volume(v, f) / (4.0 / 3.0 * math.pi * r ** 3) - 1) < 0.01
    assert abs(mesh_ref.area(v, f) / (4.0 * math.pi * r * r) - 1) < 0.02
    assert np.abs(np.linalg.norm(v, axis=1) - r).max() < 2.0 / n


def test_torus_and_two_spheres_topology():
    v, f = mesh_ref.extract(mesh_ref.torus_field(64), AABB, 0.5)
    assert mesh_ref.is_closed(f) and mesh_ref.euler_characteristic(f) == 0
    two = np.maximum(mesh_ref.sphere_field(64, 0.6, (-0.45, 0, 0)), mesh_ref.sphere_field(64, 0.6, (0.45, 0, 0)))
    v, f = mesh_ref.extract(two, AABB, 0.5)
    assert mesh_ref.is_closed(f) and mesh_ref.euler_characteristic(f) == 4
    assert mesh_ref.volume(v, f) > 0


def test_noisy_field_mask_and_activations():
    from voxe_hip import workload

    dens, _ = workload.random_grid(20)
    raw = dens.numpy()
    v, f = mesh_ref.extract(raw, [(-1.5, 1.5)] * 3, 0.4, scale=1.5, pre=abi.ACT_ABS)
    assert len(f) > 1000 and mesh_ref.is_closed(f) and mesh_ref.volume(v, f) > 0
    assert np.unique(f).size == len(v)           # every vertex is used
    mask = np.random.default_rng(0).random(raw.shape[:3]) > 0.3
    vm, fm = mesh_ref.extract(raw, [(-1.5, 1.5)] * 3, 0.4, scale=1.5, pre=abi.ACT_ABS, mask=mask)
    vz, fz = mesh_ref.extract(np.where(mask[..., None], raw, 0), [(-1.5, 1.5)] * 3, 0.4, scale=1.5, pre=abi.ACT_ABS)
    assert np.array_equal(fm, fz) and np.array_equal(vm, vz) and mesh_ref.is_closed(fm)
    # softplus: the surface is where softplus(trilerp v) == level
    v, f = mesh_ref.extract(raw, [(-1.5, 1.5)] * 3, 1.0, scale=3.0, post=abi.ACT_SOFTPLUS)
    assert mesh_ref.is_closed(f)
    assert mesh_ref.iso_value(abi.ACT_SOFTPLUS, math.log(2.0)) is None and mesh_ref.iso_value(abi.ACT_RELU, 0.0) is None


def test_default_level_halves_the_light_through_one_voxel():
    from thre3d_atom.rendering.volumetric.accumulate import density2occupancy_pb
    from thre3d_atom.thre3d_reprs.mesh import default_level
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    g = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.02, 0.01, 0.03))
    lv = default_level(g)
    assert abs(float(density2occupancy_pb(torch.tensor(lv), torch.tensor(0.01))) - 0.5) < 1e-6


# ---- PLY ----------------------------------------------------------------------------------------------------------------
def parse_ply(path):
    """minimal binary little-endian PLY reader for the writer's layout -> xyz [V,3], rgb [V,3], faces [T,3]"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    nv = int(next(h for h in header if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in header if h.startswith("element face")).split()[-1])
    vt = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
    ft = np.dtype([("n", "u1"), ("idx", "<i4", 3)])
    assert len(data) == end + nv * vt.itemsize + nf * ft.itemsize
    verts = np.frombuffer(data, vt, nv, end)
    faces = np.frombuffer(data, ft, nf, end + nv * vt.itemsize)
    assert (faces["n"] == 3).all()
    return verts["xyz"], verts["rgb"], faces["idx"]


def test_save_ply_round_trips(tmp_path):
    from thre3d_atom.thre3d_reprs.mesh import Mesh, save_ply

    v, f = mesh_ref.extract(mesh_ref.sphere_field(24, 1.2), AABB, 0.5)
    col = np.random.default_rng(1).random((len(v), 3)).astype(np.float32)
    save_ply(Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(col)), tmp_path / "m.ply")
    xyz, rgb, idx = parse_ply(tmp_path / "m.ply")
    assert np.array_equal(xyz, v) and np.array_equal(idx, f)
    assert np.array_equal(rgb, np.rint(col * 255).astype(np.uint8))
    save_ply(Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3)), tmp_path / "e.ply")
    assert len(parse_ply(tmp_path / "e.ply")[0]) == 0


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_mesh_symbols_are_declared_and_validated_without_a_device():
    from voxe_hip import build

    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    for name in ("voxe_mesh_scratch_bytes", "voxe_mesh_count", "voxe_mesh_emit"):
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols()
    assert not re.search(r"\bvoxe_cpu_mesh", text)
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text
    L = abi.declare(ctypes.CDLL(build.build()), "voxe_")
    assert L.voxe_abi_version() == 13
    need = L.voxe_mesh_scratch_bytes(8, 8, 8)
    assert need >= 10 ** 3 * 9 and L.voxe_mesh_scratch_bytes(0, 8, 8) == 0 and L.voxe_mesh_scratch_bytes(2000, 2000, 2000) == 0
    g = make_grid_desc(8, 8, (8, 8, 8), 3, AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_RELU)
    tot = ctypes.c_void_p(8)
    count = lambda g_, lv, sc=8, nb=need: L.voxe_mesh_count(ctypes.byref(g_) if g_ else None, lv, None, tot, sc, nb, None)  # noqa: E731
    assert count(None, 1.0) == abi.ERR_NULL_POINTER
    assert L.voxe_mesh_count(ctypes.byref(g), 1.0, None, None, 8, need, None) == abi.ERR_NULL_POINTER
    g.densities = 0
    assert count(g, 1.0) == abi.ERR_NULL_POINTER
    g.densities = 8
    g.Y = 0
    assert count(g, 1.0) == abi.ERR_BAD_SHAPE
    g.Y = 8
    for post, bad, good in ((abi.ACT_RELU, 0.0, 1e-3), (abi.ACT_IDENTITY, -1.0, 0.5), (abi.ACT_SOFTPLUS, 0.69, 0.7)):
        g.density_post_act = post
        assert count(g, bad) == abi.ERR_BAD_SHAPE
        assert count(g, float("nan")) == abi.ERR_BAD_SHAPE
        assert count(g, good, None, 0) == abi.ERR_WORKSPACE       # (the level passed: the scratch is checked next)
    g.density_post_act = 9
    assert count(g, 1.0) == abi.ERR_UNSUPPORTED
    g.density_post_act, g.density_pre_act = abi.ACT_RELU, 5
    assert count(g, 1.0) == abi.ERR_UNSUPPORTED
    g.density_pre_act, g.feature_kind = abi.ACT_ABS, 7
    assert count(g, 1.0) == abi.ERR_UNSUPPORTED
    g.feature_kind = abi.FEAT_ATTN
    assert count(g, 1.0, 8, need - 1) == abi.ERR_WORKSPACE
    emit = lambda vp, nv, fp, nf: L.voxe_mesh_emit(ctypes.byref(g), 1.0, None, vp, nv, fp, nf, 8, need, None)  # noqa: E731
    assert emit(8, -1, 8, 4) == abi.ERR_BAD_SHAPE
    assert emit(None, 4, 8, 4) == abi.ERR_NULL_POINTER
    assert emit(8, 4, None, 4) == abi.ERR_NULL_POINTER
    assert L.voxe_mesh_emit(ctypes.byref(g), 0.0, None, 8, 4, 8, 4, 8, need, None) == abi.ERR_BAD_SHAPE
    assert L.voxe_mesh_emit(ctypes.byref(g), 1.0, None, 8, 4, 8, 4, 8, 16, None) == abi.ERR_WORKSPACE


def test_export_entry_point_is_documented():
    assert os.path.exists(os.path.join(ROOT, "export_mesh.py"))
    for doc in ("README.md", "INTEGRATION.md"):
        assert "export_mesh.py" in open(os.path.join(ROOT, doc)).read(), doc
