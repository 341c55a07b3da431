"""GPU checks of the mesh import (voxe_voxelize_mesh, thre3d_reprs.mesh.mesh_to_voxel_grid).  Every
call goes through the C ABI with each buffer at its documented size between the guard bands of tests/arena.py (tests/contract.py),
and is compared with the numpy restatement tests/voxelize_ref.py: the integer outputs bit for bit, and so are the float ones -- the
restatement performs the kernel's float32 operations in the kernel's order.  Then determinism under face order, malformed
faces, the buffer contract, and the import end to end: re-export, render, colours."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref
import voxelize_ref as vr
from contract import DEV, K, P, run_contract, run_short
from voxe_hip import abi

pytestmark = pytest.mark.gpu
OPTIONAL = ("nearest", "colours", "inside", "stats")


def _lib():
    from voxe_hip.runtime import lib

    return lib()


def _stream():
    from voxe_hip.runtime import stream_ptr

    return stream_ptr(DEV)


def voxelize_case(k, case, want=OPTIONAL):
    """one voxe_voxelize_mesh call on arena buffers of exactly the documented sizes; records every output"""
    import ctypes as C

    v, f, c, dims, aabb, h = case
    X, Y, Z = dims
    N = X * Y * Z
    L = _lib()
    bv = k.inp("vertices", np.asarray(v, np.float32).reshape(-1, 3))
    bf = k.inp("faces", np.asarray(f, np.int32).reshape(-1, 3))
    bc = None if c is None else k.inp("vertex_colours", np.asarray(c, np.float32).reshape(-1, 3))
    out = {"sdf": k.out("sdf", N)}
    if "nearest" in want:
        out["nearest"] = k.out("nearest", N, torch.int32)
    if "colours" in want:
        out["colours"] = k.out("colours", 3 * N)
    if "inside" in want:
        out["inside"] = k.out("inside", N, torch.uint8)
    if "stats" in want:
        out["stats"] = k.out("stats", 4, torch.int64)
    need = L.voxe_voxelize_scratch_bytes(X, Y, Z, len(f))
    assert need > 0
    sc = k.scratch("scratch", need)
    k.begin()
    lo, hi = (C.c_float * 3)(*[a[0] for a in aabb]), (C.c_float * 3)(*[a[1] for a in aabb])
    k.call(L.voxe_voxelize_mesh, P(bv) if len(v) else None, len(v), P(bf) if len(f) else None, len(f), P(bc), X, Y, Z, lo, hi, float(h),
           P(out["sdf"]), P(out.get("nearest")), P(out.get("colours")), P(out.get("inside")), P(out.get("stats")), P(sc),
           k.size(sc, "scratch"), _stream())
    for name, b in out.items():
        k.bits(b, minus_one_ok=name == "nearest")
    return out


def _gpu(case, want=OPTIONAL, pattern=0xFF):
    """-> name -> numpy array of one guarded run"""
    k = K(pattern)
    out = voxelize_case(k, case, want)
    shape = {"sdf": case[3], "nearest": case[3], "inside": case[3], "colours": (*case[3], 3), "stats": (4,)}
    return {n: b.cpu().numpy().reshape(shape[n]) for n, b in out.items()}


@functools.lru_cache(maxsize=None)
def _cases():
    return vr.gpu_cases()


@functools.lru_cache(maxsize=None)
def _ref(name, dtype=np.float32):
    return vr.voxelize(*_cases()[name], dtype=dtype)


def _equal_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "torus", "offcentre", "cube_centres", "cube_bounds", "tetrahedron", "sphere_out",
                                  "sphere_huge", "degenerate", "empty", "z65"])
def test_matches_the_restatement_bit_for_bit(name):
    """inside, nearest and stats: integers, bit-identical.  sdf and colours: the float32 restatement's bits (it performs the same
    operations in the same order, and division and square root are correctly rounded on both sides); the float64 restatement
    bounds what float32 costs."""
    case = _cases()[name]
    runs = run_contract(voxelize_case, case)               # (0xFF and 0x00 fills: every promised element is written)
    got = {n: t.numpy() for n, t in runs[0].bits_out.items()}
    ref = _ref(name)
    dims = case[3]
    sdf = got["sdf"].reshape(dims)
    print(f"{name}: stats {got['stats'].tolist()}  max |sdf - restatement| {np.abs(sdf - ref['sdf']).max():.3e}  "
          f"nearest differing {(got['nearest'].reshape(dims) != ref['nearest']).sum()}")
    assert np.array_equal(got["stats"], ref["stats"])
    assert np.array_equal(got["inside"].reshape(dims), ref["inside"])
    assert np.array_equal(got["nearest"].reshape(dims), ref["nearest"])
    assert _equal_bits(sdf, ref["sdf"])
    assert _equal_bits(got["colours"].reshape(*dims, 3), ref["colours"].astype(np.float32))
    if len(case[1]):
        r64 = _ref(name, np.float64)
        same = ref["nearest"] == r64["nearest"]
        err = np.abs(ref["sdf"].astype(np.float64) - r64["sdf"]).max()
        print(f"{name}: float32 restatement against float64: max |sdf| error {err:.3e}, {(~same).sum()} other winners among equals")
        assert np.abs(sdf.astype(np.float64) - r64["sdf"]).max() <= 2 * err + 1e-12
    if name in vr.CUBES:
        assert np.array_equal(got["inside"].reshape(dims), vr.cube_cells(name))
    if name == "empty":
        assert np.all(sdf == np.float32(case[5])) and not got["stats"].any() and np.all(got["nearest"] == -1)
    if name == "degenerate":
        # the ten collinear triangles take no part: the sphere's own result, ids moved past them
        base = _ref("sphere")
        ids = np.where(base["nearest"] >= 300, base["nearest"] + 10, base["nearest"])
        assert np.array_equal(ids, ref["nearest"]) and _equal_bits(base["sdf"], ref["sdf"]) and got["stats"][1] == 0


def test_body_meshes_give_the_analytic_inside_set():
    for name, (field, level) in vr.body_fields().items():
        got = _gpu(_cases()[name], want=("inside", "stats"))
        assert np.array_equal(got["inside"] != 0, field > np.float32(level)), name
        assert got["stats"][0] == 0 and got["stats"][1] == 0


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_same_bits_whatever_the_face_order_and_from_run_to_run():
    v, f, c, dims, aabb, h = _cases()["torus"]
    first, again = _gpu(_cases()["torus"]), _gpu(_cases()["torus"], pattern=0x00)
    for n in first:
        assert _equal_bits(first[n], again[n]), n
    lo, step = vr.lattice(dims, aabb)
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(len(f))
        got = _gpu((v, f[perm], c, dims, aabb, h))
        for n in ("sdf", "inside", "stats"):
            assert _equal_bits(got[n], first[n]), (seed, n)
        # `nearest` is the lowest id of the order given: it maps back wherever the winner is alone, and where it does not the other
        # triangle is exactly as far (a closest point on a shared edge or vertex, or two triangles that mirror each other across a
        # symmetry plane of mesh and lattice through the voxel centre -- then the colours are those of another point)
        back = np.where(got["nearest"] >= 0, perm[got["nearest"]], -1)
        differ = np.argwhere(back != first["nearest"])
        assert np.array_equal(back >= 0, first["nearest"] >= 0) and len(differ) < (back >= 0).sum()
        tri = np.sort(f[back[tuple(differ.T)]], axis=1)
        d2, _, _ = vr.closest(v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]], vr._centres(differ, lo, step, np.float32))
        assert _equal_bits(np.minimum(np.sqrt(d2), np.float32(h)), np.abs(first["sdf"][tuple(differ.T)]))
        same = back == first["nearest"]
        assert _equal_bits(got["colours"][same], first["colours"][same])
        if seed == 1:
            ref = vr.voxelize(v, f[perm], c, dims, aabb, h)
            assert np.array_equal(got["nearest"], ref["nearest"]) and _equal_bits(got["colours"], ref["colours"].astype(np.float32))


# ---- malformed faces ---------------------------------------------------------------------------------------------------------------
def test_malformed_triangles_are_skipped_and_counted():
    """a face index equal to V, one equal to -1, a non-finite vertex and one outside the fixed-point range: four triangles skipped
    and counted, everything else as without them.  (The vertex buffer sits inside the arena: even a read through the bad index
    would stay in memory the test owns.)"""
    v, f, c, dims, aabb, h = _cases()["offcentre"]
    V = len(v)
    v2 = np.concatenate([v, [[np.nan, 0, 0], [0, 0, 120.0]]]).astype(np.float32)      # (u_z = 1209.5 > 1024)
    c2 = np.concatenate([c, [[1, 0, 0], [0, 1, 0]]]).astype(np.float32)
    bad = np.array([[3, V + 2, 5], [-1, 4, 6], [7, 8, V], [V + 1, 9, 10]], dtype=np.int32)
    f2 = np.concatenate([f[:100], bad[:2], f[100:250], bad[2:], f[250:]]).astype(np.int32)
    got, clean = _gpu((v2, f2, c2, dims, aabb, h)), _gpu(_cases()["offcentre"])
    assert got["stats"][1] == 4 and clean["stats"][1] == 0
    assert np.array_equal(got["stats"][[0, 2, 3]], clean["stats"][[0, 2, 3]])
    ids = clean["nearest"] + 2 * (clean["nearest"] >= 100) + 2 * (clean["nearest"] >= 250)
    assert np.array_equal(got["nearest"], ids)
    for n in ("sdf", "inside", "colours"):
        assert _equal_bits(got[n], clean[n]), n
    ref = vr.voxelize(v2, f2, c2, dims, aabb, h)
    assert np.array_equal(ref["stats"], got["stats"]) and np.array_equal(ref["nearest"], got["nearest"])


# ---- buffer contract ---------------------------------------------------------------------------------------------------------------
def test_optional_outputs_in_every_combination():
    case = _cases()["cube_bounds"]
    full = _gpu(case)
    for mask in range(15):
        want = tuple(n for i, n in enumerate(OPTIONAL) if (mask >> i) & 1)
        got = _gpu(case, want=want)
        assert set(got) == {"sdf", *want}
        for n in got:
            assert _equal_bits(got[n], full[n]), (want, n)


def test_short_scratch_is_refused_with_nothing_written():
    run_short(voxelize_case, "scratch", _cases()["cube_centres"])
    # ... and so are the other refusals the header lists, with real buffers
    import ctypes as C

    k = K(0xFF)
    sdf, sc = k.out("sdf", 8 * 8 * 8), k.scratch("scratch", _lib().voxe_voxelize_scratch_bytes(8, 8, 8, 0))
    k.begin()
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    snap = k.a.mem.clone()
    L = _lib()
    assert L.voxe_voxelize_mesh(None, 0, None, 0, None, 8, 8, 8, lo, hi, 0.0, P(sdf), None, None, None, None, P(sc), sc.nbytes,
                                _stream()) == abi.ERR_BAD_SHAPE
    assert L.voxe_voxelize_mesh(None, 0, None, 3, None, 8, 8, 8, lo, hi, 0.5, P(sdf), None, None, None, None, P(sc), sc.nbytes,
                                _stream()) == abi.ERR_NULL_POINTER
    torch.cuda.synchronize()
    assert torch.equal(k.a.mem, snap)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _relu_like(deg=0):
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    return VoxelGrid(torch.zeros(*vr.N20, 1, device=DEV), torch.zeros(*vr.N20, 3 * (deg + 1) ** 2, device=DEV), VoxelSize(0.1, 0.1, 0.1),
                     density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.ReLU())


@functools.lru_cache(maxsize=None)
def _imported(name="sphere"):
    from thre3d_atom.thre3d_reprs.mesh import Mesh, mesh_to_voxel_grid

    v, f, c, _, _, _ = _cases()[name]
    mesh = Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c))
    grid, stats = mesh_to_voxel_grid(mesh, _relu_like(), return_stats=True)
    return grid, stats


def test_import_then_export_is_the_restatements_round_trip():
    from test_voxelize_host import COLOUR_ROUND_TRIP, round_trip
    from thre3d_atom.thre3d_reprs.mesh import extract_mesh

    grid, stats = _imported()
    v, f, rv, rf, raw, feats = round_trip("sphere")
    assert stats[0] == 0 and stats[1] == 0 and stats[2] == _ref("sphere")["stats"][2]
    dens = grid.densities.detach().cpu().numpy()
    print(f"densities: max |import - restatement| {np.abs(dens - raw).max():.3e}")
    assert np.abs(dens - raw).max() <= 4 * np.spacing(np.abs(raw).max())
    assert np.abs(grid.features.detach().cpu().numpy() - feats).max() < 1e-5
    mesh = extract_mesh(grid)           # (default level: the level the import aimed at)
    gv, gf = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    assert np.array_equal(gf, rf)
    assert gv.shape == rv.shape and bool(np.all(np.abs(gv - rv) <= 2 * np.spacing(np.maximum(np.abs(gv), np.abs(rv)))))
    assert mesh_ref.is_closed(gf) and mesh_ref.euler_characteristic(gf) == 2
    # imported colours: a mesh coloured by position comes back coloured by position
    cerr = np.abs(mesh.colours.cpu().numpy().astype(np.float64) - vr.position_colours(gv)).max()
    print(f"re-exported colours: max error {cerr:.4f} (restatement's round trip: {COLOUR_ROUND_TRIP})")
    assert cerr <= 1.5 * COLOUR_ROUND_TRIP


def test_render_of_the_imported_grid():
    import gpu_helpers as gh
    from oracle import voxe_oracle as vo
    from thre3d_atom.utils.imaging_utils import pose_spherical
    from voxe_hip.desc import make_render_cfg

    grid, _ = _imported()
    v = _cases()["sphere"][0]
    dens, feat = grid.densities.detach().cpu().numpy(), grid.features.detach().cpu().numpy()
    og = vo.Grid(dens, feat, grid.voxe_grid_spec().aabb, 1.0, abi.ACT_IDENTITY, abi.ACT_RELU)
    H = W = 40
    pose = pose_spherical(30.0, -25.0, 3.0)
    o, d = vo.cast_rays(H, W, 0.5 * W / np.tan(0.5 * 0.9), pose.rotation.numpy(), pose.translation.numpy())
    cfg = make_render_cfg(96, 1.2, 4.8, white_bkgd=False)
    out, ref = gh.hip_forward(og, cfg, o, d), vo.render_fwd(og, cfg, o, d)
    np.testing.assert_allclose(out["colour"], ref["colour"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(out["acc"], ref["acc"], rtol=0, atol=5e-6)
    # a ray that stays further than h + one voxel per axis from the mesh meets no density at all: acc is exactly 0.  A sample
    # gathers the eight voxels of its cell, up to one voxel away on EVERY axis -- one cell diagonal, sqrt(3) voxels, in Euclidean
    # distance -- and a voxel carries density when it is closer than h to the mesh.  (The mesh lies within max |vertex| of the
    # origin; the ray's distance from the origin bounds its distance from the mesh from below.)
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    miss = np.linalg.norm(np.cross(o, dn), axis=1) - np.linalg.norm(v, axis=1).max() > 0.2 + np.sqrt(3.0) * 0.1
    acc = out["acc"].reshape(-1)
    assert 50 < miss.sum() < len(miss) - 50 and np.all(acc[miss] == 0.0)
    assert acc.max() > 0.99                                # (and the object is opaque)


def test_cli_writes_checkpoints_the_other_tools_load(tmp_path):
    """import_mesh.py on a fresh cubic lattice (--grid_dims) and on another checkpoint's lattice (--like): the results load like
    any checkpoint and their iso-surface is the mesh"""
    import importlib.util
    import os

    from click.testing import CliRunner
    from conftest import ROOT
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.mesh import Mesh, extract_mesh, save_ply
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict

    spec = importlib.util.spec_from_file_location("import_mesh_cli_gpu", os.path.join(ROOT, "import_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    v, f, c, _, _, _ = _cases()["offcentre"]
    save_ply(Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c)), tmp_path / "m.ply")
    res = CliRunner().invoke(mod.main, ["-i", str(tmp_path / "m.ply"), "-o", str(tmp_path / "fresh.pth"), "--grid_dims", "28", "28", "28",
                                        "--sh_degree", "1"])
    assert res.exit_code == 0, (res.output, res.exception)
    assert f"V = {len(v)}  T = {len(f)}" in res.output and "0 odd columns" in res.output
    res = CliRunner().invoke(mod.main, ["-i", str(tmp_path / "m.ply"), "-o", str(tmp_path / "like.pth"), "--like", str(tmp_path / "fresh.pth"),
                                        "--band_voxels", "3"])
    assert res.exit_code == 0, (res.output, res.exception)
    for name in ("fresh.pth", "like.pth"):
        vm, extra = create_volumetric_model_from_saved_model(tmp_path / name, create_voxel_grid_from_saved_info_dict, device=DEV)
        grid = vm.thre3d_repr
        assert grid.grid_dims == (28, 28, 28) and grid.features.shape[-1] == 12 and extra is not None
        mesh = extract_mesh(grid)
        gv, gf = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
        assert len(gf) > 300 and mesh_ref.is_closed(gf) and mesh_ref.euler_characteristic(gf) == 2
        edge = float(grid.voxel_size[0])
        assert vr.point_mesh_distance(gv, v, f).max() < 0.25 * edge      # (a marching-cubes surface between two lattices)
        assert 0.9 < mesh_ref.volume(gv, gf) / mesh_ref.volume(v, f) < 1.05
    # an open mesh is refused unless asked for
    save_ply(Mesh(torch.from_numpy(v), torch.from_numpy(f[40:]), torch.from_numpy(c)), tmp_path / "open.ply")
    res = CliRunner().invoke(mod.main, ["-i", str(tmp_path / "open.ply"), "-o", str(tmp_path / "o.pth"), "--like", str(tmp_path / "fresh.pth")])
    assert res.exit_code == 1 and "not closed" in res.output
    res = CliRunner().invoke(mod.main, ["-i", str(tmp_path / "open.ply"), "-o", str(tmp_path / "o.pth"), "--like", str(tmp_path / "fresh.pth"),
                                        "--allow_open"])
    assert res.exit_code == 0, (res.output, res.exception)
