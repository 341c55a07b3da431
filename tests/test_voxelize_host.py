"""CPU checks of the mesh import: the numpy restatement tests/voxelize_ref.py against analytic bodies
(exact inside sets, lattice cubes, invariance under face order / vertex rotation / winding, open meshes), its round trip through
the mesh export's restatement, the PLY reader, the density and feature mapping of mesh_to_voxel_grid (on the restatement's
voxelisation: no GPU here), the C ABI's prototypes and the CLI's options."""
import ctypes as C
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import mesh_ref
import voxelize_ref as vr
from conftest import ROOT
from voxe_hip import abi

H = 0.2   # two voxels of the 20^3 lattice over [-1, 1]^3


@functools.lru_cache(maxsize=None)
def _body(name):
    v, f = vr.body_mesh(name)
    return v, f, vr.voxelize(v, f, vr.position_colours(v), vr.N20, vr.AABB, H)


def _same(a, b, keys=("sdf", "nearest", "inside", "colours", "stats", "d2")):
    return [k for k in keys if not np.array_equal(a[k], b[k])]


# ---- inside / outside ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "torus", "offcentre"])
def test_parity_is_the_analytic_inside_set(name):
    """0 mismatches on every voxel, 0 odd columns, no malformed triangle (the fixed-point parity decides like the field the mesh
    was extracted from: the mesh separates the voxel centres above the level from those below it)"""
    field, level = vr.body_fields()[name]
    v, f, r = _body(name)
    assert len(f) > 300 and mesh_ref.is_closed(f)
    assert np.array_equal(r["inside"] != 0, field > np.float32(level))
    assert r["stats"][0] == 0 and r["stats"][1] == 0 and r["stats"][2] == int((r["nearest"] >= 0).sum()) > 0
    assert np.all(np.abs(r["sdf"]) <= np.float32(H)) and np.array_equal(r["sdf"] < 0, r["inside"] != 0)
    assert np.all(r["sdf"][r["nearest"] < 0] == np.where(r["inside"][r["nearest"] < 0] != 0, -np.float32(H), np.float32(H)))


@pytest.mark.parametrize("name", ["sphere", "offcentre"])
def test_unchanged_by_face_order_vertex_rotation_and_winding(name):
    v, f, r = _body(name)
    col = vr.position_colours(v)
    for shift in (1, 2):
        assert _same(vr.voxelize(v, np.roll(f, shift, axis=1), col, vr.N20, vr.AABB, H), r) == []
    assert _same(vr.voxelize(v, f[:, ::-1], col, vr.N20, vr.AABB, H), r) == []
    perm = np.random.default_rng(3).permutation(len(f))
    rp = vr.voxelize(v, f[perm], col, vr.N20, vr.AABB, H)
    # the distance, the sign and the statistics are the same bits; the winner among equidistant triangles (a closest point on a
    # shared edge or vertex) is the lowest id of the order given, so `nearest` maps back wherever the winner is alone
    assert _same(rp, r, ("sdf", "inside", "stats", "d2")) == []
    back = np.where(rp["nearest"] >= 0, perm[rp["nearest"]], -1)
    differ = np.argwhere(back != r["nearest"])
    assert len(differ) < (r["nearest"] >= 0).sum()
    lo, step = vr.lattice(vr.N20, vr.AABB)
    tri = np.sort(f[back[tuple(differ.T)]], axis=1)
    d2, _, _ = vr.closest(v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]], vr._centres(differ, lo, step, np.float32))
    assert np.array_equal(d2, r["d2"][tuple(differ.T)])


def _covering_triangle(v, f):
    """a triangle whose (y, z) projection holds a column centre -- moved by (eps, eps^2) as the top-left rule does: the vertices of
    a marching-cubes mesh on x edges project exactly onto column centres"""
    lo, step = vr.lattice(vr.N20, vr.AABB)
    u = (v.astype(np.float64) - lo) / step - 0.5
    for t, (a, b, c) in enumerate(u[f][:, :, 1:]):
        m = np.array([b - a, c - a]).T
        if abs(np.linalg.det(m)) < 1e-2:
            continue
        for p in (np.floor((a + b + c) / 3) + np.array(o) for o in ((0, 0), (0, 1), (1, 0), (1, 1))):
            s = np.linalg.solve(m, p + np.array([1e-3, 1e-6]) - a)
            if s[0] > 1e-8 and s[1] > 1e-8 and s[0] + s[1] < 1 - 1e-8:
                return t
    raise AssertionError("no triangle covers a column centre")


def test_open_mesh_has_odd_columns():
    v, f, r = _body("sphere")
    t = _covering_triangle(v, f)
    ro = vr.voxelize(v, np.delete(f, t, axis=0), None, vr.N20, vr.AABB, H)
    assert ro["stats"][0] > 0 and r["stats"][0] == 0


@pytest.mark.parametrize("name", ["cube_centres", "cube_bounds"])
@pytest.mark.parametrize("sub", [1, 2])
def test_lattice_cubes_give_their_cells_exactly(name, sub):
    """faces exactly on voxel centres (every crossing is a lattice hit) / exactly on voxel boundaries, as 12 triangles and with
    every face cut 2 x 2 (column centres on shared edges and on shared vertices): the half-open cells [lo, hi) per axis"""
    v, f = vr.cube_mesh(name, sub)
    assert len(f) == 12 * sub * sub
    r = vr.voxelize(v, f, None, vr.N20, vr.AABB, 0.15)
    assert np.array_equal(r["inside"], vr.cube_cells(name)) and r["inside"].sum() == 512
    assert r["stats"][0] == 0 and r["stats"][1] == 0


def test_distance_is_the_float64_brute_force_distance():
    v, f, r = _body("torus")
    band = r["nearest"] >= 0
    lo, step = vr.lattice(vr.N20, vr.AABB)
    centres = vr._centres(np.argwhere(band), lo, step, np.float64)
    d = vr.point_mesh_distance(centres, v, f)
    assert np.abs(np.abs(r["sdf"][band].astype(np.float64)) - np.minimum(d, np.float32(H))).max() < 1e-6
    # (every voxel within the band is in it)
    far = vr.point_mesh_distance(vr._centres(np.argwhere(~band), lo, step, np.float64), v, f)
    assert far.min() > H * (1 - 1e-6)


# ---- round trip --------------------------------------------------------------------------------------------------------------------
# measured on the restatement (band 1.5, 2 and 3 voxels alike): largest distance of a re-extracted vertex to the source mesh in
# voxels, enclosed volume over the source's
ROUND_TRIP = {"sphere": (0.0325, 0.9878), "torus": (0.0491, 0.9766), "offcentre": (0.0461, 0.9780)}
COLOUR_ROUND_TRIP = 0.0054      # largest |re-exported vertex colour - colour of the position| over the three bodies


def round_trip(name, band_voxels=2.0):
    """mesh -> restatement import into a ReLU field -> the export's restatement at the same level"""
    v, f = vr.body_mesh(name)
    h = band_voxels * 0.1
    r = _body(name)[2] if band_voxels == 2.0 else vr.voxelize(v, f, vr.position_colours(v), vr.N20, vr.AABB, h)
    level = np.log(2.0) / 0.1
    raw, feats = vr.fields(r["sdf"], r["nearest"], r["colours"], h, vr.iso_value(abi.ACT_RELU, level), abi.ACT_IDENTITY,
                           abi.ACT_RELU, 1.0, 0)
    v2, f2 = mesh_ref.extract(raw, vr.AABB, level, 1.0, abi.ACT_IDENTITY, abi.ACT_RELU)
    return v, f, v2, f2, raw, feats


@pytest.mark.parametrize("name", ["sphere", "torus", "offcentre"])
def test_round_trip_through_the_export(name):
    """Measured on the restatement: vertex-to-source distance 0.0325 / 0.0491 / 0.0461 voxel and volume ratio 0.9878 / 0.9766 /
    0.9780 for the sphere / torus / off-centre sphere (the same to four digits at bands of 1.5, 2 and 3 voxels); the bounds are
    those with a 1.5x margin.  V and T come back unchanged: 360 / 716, 648 / 1296, 230 / 456."""
    v, f, v2, f2, _, feats = round_trip(name)
    assert mesh_ref.is_closed(f2) and mesh_ref.euler_characteristic(f2) == mesh_ref.euler_characteristic(f)
    assert (len(v2), len(f2)) == (len(v), len(f))
    dist = vr.point_mesh_distance(v2, v, f).max() / 0.1
    ratio = mesh_ref.volume(v2, f2) / mesh_ref.volume(v, f)
    colour = 1.0 / (1.0 + np.exp(-vr.C0 * vr.trilinear(feats.astype(np.float64), vr.AABB, v2)))
    cerr = np.abs(colour - vr.position_colours(v2).astype(np.float64)).max()
    print(f"{name}: distance {dist:.4f} voxel, volume ratio {ratio:.4f}, colour {cerr:.4f}")
    bound_d, measured_ratio = ROUND_TRIP[name]
    assert dist <= 1.5 * bound_d and abs(1.0 - ratio) <= 1.5 * (1.0 - measured_ratio)
    assert cerr <= 1.5 * COLOUR_ROUND_TRIP


def test_round_trip_at_another_band():
    v, f, v2, f2, _, _ = round_trip("offcentre", 3.0)
    assert mesh_ref.is_closed(f2) and len(f2) == len(f)
    assert vr.point_mesh_distance(v2, v, f).max() / 0.1 <= 1.5 * ROUND_TRIP["offcentre"][0]


# ---- mesh_to_voxel_grid on the restatement's voxelisation -----------------------------------------------------------------------
def _like(pre, post, scale=1.0, sh_degree=0):
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    return VoxelGrid(torch.zeros(*vr.N20, 1), torch.zeros(*vr.N20, 3 * (sh_degree + 1) ** 2), VoxelSize(0.1, 0.1, 0.1),
                     density_preactivation=pre, density_postactivation=post, expected_density_scale=scale)


@pytest.fixture
def restated_voxeliser(monkeypatch):
    """thre3d_reprs.mesh with the device call replaced by the restatement (CPU tensors)"""
    from thre3d_atom.thre3d_reprs import mesh as mesh_mod

    def voxelize_mesh(vertices, faces, colours, dims, aabb, band):
        r = vr.voxelize(vertices.numpy(), faces.numpy(), None if colours is None else colours.numpy(), dims, aabb, band)
        return (torch.from_numpy(r["sdf"]), torch.from_numpy(r["nearest"]), torch.from_numpy(r["colours"]),
                torch.from_numpy(r["inside"]), tuple(int(s) for s in r["stats"]))

    monkeypatch.setattr(mesh_mod._ops, "voxelize_mesh", voxelize_mesh)
    return mesh_mod


@pytest.mark.parametrize("pre,post,scale,deg", [(torch.nn.Identity(), torch.nn.ReLU(), 1.0, 0), (torch.nn.Identity(), torch.nn.Softplus(), 30.0, 1),
                                                (torch.abs, torch.nn.Identity(), 1.0, 0)])
def test_mesh_to_voxel_grid_mapping(restated_voxeliser, pre, post, scale, deg):
    from thre3d_atom.thre3d_reprs.voxels import density_activation_codes

    m = restated_voxeliser
    v, f, r = _body("offcentre")
    mesh = m.Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(vr.position_colours(v)))
    like = _like(pre, post, scale, deg)
    grid = m.mesh_to_voxel_grid(mesh, like)
    pre_c, post_c = density_activation_codes(pre, post)
    L = vr.iso_value(post_c, m.default_level(like))
    raw, feats = vr.fields(r["sdf"], r["nearest"], r["colours"], H, L, pre_c, post_c, scale, deg)
    assert grid.grid_dims == like.grid_dims and tuple(grid.aabb) == tuple(like.aabb) and grid.features.shape == like.features.shape
    assert grid._expected_density_scale == scale and grid._density_postactivation is post
    got = grid.densities.numpy()
    assert np.abs(got - raw).max() <= 4 * np.spacing(np.abs(raw).max())      # (three float32 operations)
    assert np.abs(grid.features.numpy() - feats).max() < 1e-5
    # L on the surface side, the empty value from h outside on, saturated deep inside
    e = np.float32(-20.0 if post_c == abi.ACT_SOFTPLUS else 0.0)
    pre_act = np.abs(got[..., 0] * np.float32(scale)) if pre_c == abi.ACT_ABS else got[..., 0] * np.float32(scale)
    assert np.allclose(pre_act[r["sdf"] == np.float32(H)], e, atol=1e-5)
    assert np.allclose(pre_act[r["sdf"] == -np.float32(H)], L + (L - e), rtol=1e-6)
    assert np.array_equal(pre_act > L, r["sdf"] < 0) or np.array_equal(pre_act >= L, r["sdf"] <= 0)
    # without colours: mid grey, every feature 0
    grey = m.mesh_to_voxel_grid(m.Mesh(mesh.vertices, mesh.faces, None), like)
    assert float(grey.features.abs().max()) == 0.0 and torch.equal(grey.densities, grid.densities)


def test_mesh_to_voxel_grid_refusals(restated_voxeliser):
    m = restated_voxeliser
    v, f, _ = _body("sphere")
    mesh = m.Mesh(torch.from_numpy(v), torch.from_numpy(f), None)
    relu = _like(torch.nn.Identity(), torch.nn.ReLU())
    with pytest.raises(ValueError, match="empty"):
        m.mesh_to_voxel_grid(mesh, _like(torch.abs, torch.nn.Softplus()))
    with pytest.raises(ValueError, match="level"):
        m.mesh_to_voxel_grid(mesh, relu, level=0.0)
    with pytest.raises(ValueError, match="level"):       # softplus^-1(level) <= -20
        m.mesh_to_voxel_grid(mesh, _like(torch.nn.Identity(), torch.nn.Softplus()), level=0.5)
    opened = m.Mesh(mesh.vertices, torch.from_numpy(np.delete(f, _covering_triangle(v, f), axis=0)), None)
    with pytest.raises(ValueError, match="not closed"):
        m.mesh_to_voxel_grid(opened, relu)
    grid, stats = m.mesh_to_voxel_grid(opened, relu, allow_open=True, return_stats=True)
    assert stats[0] > 0 and grid.densities.shape == (20, 20, 20, 1)
    bad = f.copy()
    bad[7, 1] = len(v)
    with pytest.raises(ValueError, match="malformed"):
        m.mesh_to_voxel_grid(m.Mesh(mesh.vertices, torch.from_numpy(bad), None), relu, allow_open=True)


# ---- PLY ---------------------------------------------------------------------------------------------------------------------------
def _write_ascii(path, v, f, c=None, normals=False, polygons=None):
    lines = ["ply", "format ascii 1.0", "comment a test file", f"element vertex {len(v)}", "property float x", "property float y",
             "property float z"]
    if normals:
        lines += ["property float nx", "property float ny", "property float nz"]
    if c is not None:
        lines += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    polygons = [list(t) for t in f] if polygons is None else polygons
    lines += [f"element face {len(polygons)}", "property list uchar uint vertex_indices", "end_header"]
    for i, p in enumerate(v):
        row = [repr(float(x)) for x in p] + (["0", "0", "1"] if normals else [])
        row += [] if c is None else [str(int(x)) for x in c[i]] + ["255"]
        lines.append(" ".join(row))
    lines += [" ".join(str(x) for x in [len(p), *p]) for p in polygons]
    path.write_text("\n".join(lines) + "\n")


def test_load_ply_reads_back_what_save_ply_writes(tmp_path):
    from thre3d_atom.thre3d_reprs.mesh import Mesh, load_ply, save_ply

    v, f = vr.body_mesh("offcentre")
    col = vr.position_colours(v)
    mesh = Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(col))
    for normals in (None, torch.ones(len(v), 3)):
        save_ply(mesh, tmp_path / "m.ply", normals=normals)
        back = load_ply(tmp_path / "m.ply")
        assert torch.equal(back.vertices, mesh.vertices) and torch.equal(back.faces, mesh.faces) and back.faces.dtype == torch.int32
        assert float((back.colours - mesh.colours).abs().max()) <= 0.5 / 255 + 1e-7
    c8 = np.rint(col * 255).astype(np.uint8)
    for normals in (False, True):
        _write_ascii(tmp_path / "a.ply", v, f, c8, normals=normals)
        back = load_ply(tmp_path / "a.ply")
        assert torch.equal(back.vertices, mesh.vertices) and torch.equal(back.faces, mesh.faces)
        assert np.array_equal(np.rint(back.colours.numpy() * 255).astype(np.uint8), c8)
    _write_ascii(tmp_path / "n.ply", v, f)
    assert load_ply(tmp_path / "n.ply").colours is None
    save_ply(Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3)), tmp_path / "e.ply")
    empty = load_ply(tmp_path / "e.ply")
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)


def test_load_ply_fan_triangulates_polygons(tmp_path):
    from thre3d_atom.thre3d_reprs.mesh import load_ply

    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 1.5, 0]], dtype=np.float32)
    _write_ascii(tmp_path / "q.ply", v, None, polygons=[[0, 1, 2, 3], [3, 2, 4], [0, 1, 2, 4, 3]])
    want = [[0, 1, 2], [0, 2, 3], [3, 2, 4], [0, 1, 2], [0, 2, 4], [0, 4, 3]]
    assert load_ply(tmp_path / "q.ply").faces.tolist() == want
    # binary, quads only (one strided read) and mixed (record by record)
    for polys in ([[0, 1, 2, 3], [1, 2, 4, 3]], [[0, 1, 2, 3], [3, 2, 4]]):
        head = ("ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty double x\nproperty double y\nproperty double z\n"
                f"element face {len(polys)}\nproperty list uchar int vertex_index\nend_header\n").encode()
        body = v.astype("<f8").tobytes() + b"".join(bytes([len(p)]) + np.array(p, "<i4").tobytes() for p in polys)
        (tmp_path / "b.ply").write_bytes(head + body)
        got = load_ply(tmp_path / "b.ply")
        assert got.faces.tolist() == [[p[0], p[i], p[i + 1]] for p in polys for i in range(1, len(p) - 1)]
        assert np.array_equal(got.vertices.numpy(), v)


@pytest.mark.parametrize("blob", [
    b"plx\nformat ascii 1.0\nelement vertex 0\nend_header\n",
    b"ply\nelement vertex 0\nproperty float x\nend_header\n",                                         # no format
    b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n",
    b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n",    # no end_header
    b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n0 0\n",   # no z
    b"ply\nformat ascii 1.0\nelement vertex 1\nproperty quad x\nend_header\n0\n",                       # unknown type
    b"ply\nformat ascii 1.0\nelement vertex x\nend_header\n",
    b"ply\nformat ascii 1.0\nproperty float x\nend_header\n",                                         # property without element
    b"ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n",  # no vertex element
    b"ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n",   # truncated
    b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n\0\0\0\0",
])
def test_load_ply_refuses_malformed_files(tmp_path, blob):
    from thre3d_atom.thre3d_reprs.mesh import load_ply

    (tmp_path / "bad.ply").write_bytes(blob)
    with pytest.raises(ValueError):
        load_ply(tmp_path / "bad.ply")


# ---- C ABI and CLI -----------------------------------------------------------------------------------------------------------------
_CTYPES = {"float*": C.c_void_p, "int32_t*": C.c_void_p, "uint8_t*": C.c_void_p, "int64_t*": C.c_void_p, "void*": C.c_void_p,
           "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "size_t": C.c_size_t, "int": C.c_int}


def _prototype(name):
    """(restype, argtypes) of a function as include/voxe.h declares it"""
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*)\);", text, re.M)
    assert m, f"{name} is not declared in include/voxe.h"
    args = []
    for a in m.group(2).split(","):
        words = a.replace("const", " ").replace("*", " * ").split()
        args.append("".join(words[:-1]))          # (the last word is the parameter's name)
    return _CTYPES[m.group(1)], [_CTYPES[a] for a in args]


def test_abi_declares_the_voxeliser_as_the_header_does():
    assert abi.ABI_VERSION == 13
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    assert re.search(r"#define VOXE_ABI_VERSION 13\b", text)
    assert not re.search(r"voxe_cpu_voxelize", text)
    for name in ("voxelize_scratch_bytes", "voxelize_mesh"):
        assert "voxe_" + name in abi.hip_symbols()
        res, args = _prototype("voxe_" + name)
        got_res, got_args = abi.HIP_ONLY[name]
        # (aabb_lo / aabb_hi are host float[3]: POINTER(c_float) on the ctypes side)
        norm = [C.c_void_p if a is C.POINTER(C.c_float) else a for a in got_args]
        assert got_res is res and norm == args, name
    assert len(abi.HIP_ONLY["voxelize_mesh"][1]) == 19


def test_library_validates_before_any_device_work():
    """the status codes in the header's order, on a machine without a GPU (no call gets as far as a launch)"""
    from voxe_hip import build

    lib = abi.declare(C.CDLL(build.build()), "voxe_")
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    call = lambda **kw: lib.voxe_voxelize_mesh(*[{**dict(  # noqa: E731
        vertices=8, V=4, faces=8, T=4, colours=None, X=8, Y=8, Z=8, lo=lo, hi=hi, h=0.5, sdf=8, nearest=None, cols=None, inside=None,
        stats=None, scratch=8, scratch_bytes=1 << 20, stream=None), **kw}[k] for k in (
        "vertices", "V", "faces", "T", "colours", "X", "Y", "Z", "lo", "hi", "h", "sdf", "nearest", "cols", "inside", "stats",
        "scratch", "scratch_bytes", "stream")])
    assert call(sdf=None) == abi.ERR_NULL_POINTER and call(vertices=None) == abi.ERR_NULL_POINTER
    assert call(faces=None) == abi.ERR_NULL_POINTER and call(lo=None) == abi.ERR_NULL_POINTER
    assert call(sdf=None, X=0) == abi.ERR_NULL_POINTER                       # (the order: pointers first)
    for bad in (dict(X=0), dict(Y=-1), dict(Z=1025), dict(h=0.0), dict(h=-1.0), dict(h=float("nan")), dict(h=float("inf")),
                dict(T=-1), dict(V=1 << 31), dict(hi=lo)):
        assert call(**bad) == abi.ERR_BAD_SHAPE, bad
    need = lib.voxe_voxelize_scratch_bytes(8, 8, 8, 4)
    assert need >= 8 * 8 * 8 * 12 + 4 * 12 and lib.voxe_voxelize_scratch_bytes(8, 8, 1025, 4) == 0
    assert lib.voxe_voxelize_scratch_bytes(1024, 1024, 1024, 1 << 20) > (1 << 30) * 12
    assert call(scratch_bytes=need - 1) == abi.ERR_WORKSPACE and call(scratch=None) == abi.ERR_WORKSPACE
    assert call(h=0.0, scratch_bytes=0) == abi.ERR_BAD_SHAPE                 # (the order: shape before workspace)
    # the bound grows by 12 bytes per triangle, whatever their size: no work item is stored
    assert lib.voxe_voxelize_scratch_bytes(8, 8, 8, 4 + 64000) - need == 64000 * 12


def test_cli_option_table():
    spec = importlib.util.spec_from_file_location("import_mesh_cli", os.path.join(ROOT, "import_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opts = {p.name: p for p in mod.main.params}
    assert set(opts) == {"mesh_path", "output_path", "like", "grid_dims", "sh_degree", "level", "band_voxels", "inside_ratio", "allow_open"}
    assert opts["mesh_path"].required and "-i" in opts["mesh_path"].opts and "-o" in opts["output_path"].opts
    assert opts["band_voxels"].default == 2.0 and opts["inside_ratio"].default == 2.0 and opts["sh_degree"].default == 0
    assert opts["grid_dims"].nargs == 3 and opts["level"].default is None and opts["allow_open"].is_flag
    from click.testing import CliRunner

    res = CliRunner().invoke(mod.main, ["-i", "m.ply", "-o", "m.pth"])
    assert res.exit_code == 2 and "exactly one of --like and --grid_dims" in res.output
    res = CliRunner().invoke(mod.main, ["-i", "m.ply", "-o", "m.pth", "--like", "a.pth", "--grid_dims", "8", "8", "8"])
    assert res.exit_code == 2
    # the lattice of --grid_dims: cubic voxels, the mesh inside a pad of band + 1 voxels
    size, centre = mod.cubic_lattice(np.array([[-1.0, 0.0, 0.0], [1.0, 0.5, 0.25]]), (26, 26, 26), 2.0)
    assert size[0] == size[1] == size[2] == pytest.approx(2.0 / 20) and tuple(centre) == (0.0, 0.25, 0.125)
