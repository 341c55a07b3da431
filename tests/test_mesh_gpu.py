"""GPU checks of the mesh export (voxe_mesh_count / voxe_mesh_emit, thre3d_reprs.mesh, export_mesh.py): face-for-face
agreement with the numpy restatement tests/mesh_ref.py, vertices on the renderer's iso-surface (through the independent
point-query kernel), closedness / orientation / topology, colours, masks, determinism, capacity guards, rejections."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import mesh_ref
from conftest import GOLDEN, ROOT
from test_mesh_host import parse_ply
from voxe_hip import abi, ops, workload
from voxe_hip.desc import make_grid_desc
from voxe_hip.runtime import VoxeError

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C0 = 0.28209479177387814


def _grid(dens, feat, aabb, scale=1.0, pre=None, post=None):
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelGridLocation, VoxelSize

    side = [(hi - lo) / n for (lo, hi), n in zip(aabb, dens.shape[:3])]
    centre = [(lo + hi) / 2 for lo, hi in aabb]
    return VoxelGrid(dens.to(DEV), feat.to(DEV), VoxelSize(*side), VoxelGridLocation(*centre),
                     density_preactivation=pre if pre is not None else torch.nn.Identity(),
                     density_postactivation=post if post is not None else torch.nn.Identity(),
                     expected_density_scale=scale)


def _ulp_close(a, b, ulps=2):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))))


def _cases():
    d24, f24 = workload.random_grid(24)
    d48, f48 = workload.random_grid(48, nfeat=27, seed=3)
    sph = torch.from_numpy(mesh_ref.sphere_field(64, 1.2))[..., None]
    g = torch.Generator().manual_seed(7)
    d_sh2 = torch.empty(20, 22, 18, 1).uniform_(-1, 1, generator=g)
    f_sh2 = torch.empty(20, 22, 18, 27).uniform_(-2, 2, generator=g)
    return {
        "random24": (d24, f24, [(-1.5, 1.5)] * 3, 1.5, abi.ACT_ABS, abi.ACT_IDENTITY, 0.45),
        "random48": (d48, f48, [(-1.5, 1.5)] * 3, 1.0, abi.ACT_ABS, abi.ACT_IDENTITY, 0.3),
        "sphere64": (sph, torch.rand(64, 64, 64, 3, generator=g), [(-1.0, 1.0)] * 3, 1.0, abi.ACT_IDENTITY, abi.ACT_IDENTITY, 0.5),
        "sh2_softplus": (d_sh2, f_sh2, [(-1.0, 1.2), (-0.9, 1.1), (-1.3, 0.7)], 3.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, 1.2),
    }


_ACT = {abi.ACT_IDENTITY: torch.nn.Identity(), abi.ACT_ABS: torch.abs, abi.ACT_RELU: torch.nn.ReLU(),
        abi.ACT_SOFTPLUS: torch.nn.Softplus()}


@pytest.mark.parametrize("name", ["random24", "random48", "sphere64", "sh2_softplus"])
def test_matches_numpy_restatement_and_lies_on_the_render_surface(name):
    from thre3d_atom.thre3d_reprs.mesh import extract_mesh

    dens, feat, aabb, scale, pre, post, level = _cases()[name]
    vg = _grid(dens, feat, aabb, scale, _ACT[pre], _ACT[post])
    aabb = vg.voxe_grid_spec().aabb          # (centre -/+ half extent, as the grid computes it)
    mesh = extract_mesh(vg, level=level)
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    rv, rf = mesh_ref.extract(dens.numpy(), aabb, level, scale, pre, post)
    assert len(f) > 100
    assert np.array_equal(f, rf)
    assert v.shape == rv.shape and _ulp_close(v, rv)
    assert mesh_ref.is_closed(f) and mesh_ref.volume(v, f) > 0
    # every vertex is on the renderer's iso-surface: the point-query kernel's density there equals the level
    # (in the pre-post domain: trilerp(v) = L, tolerance relative to max|v|)
    out = vg(mesh.vertices)
    L = float(mesh_ref.iso_value(post, level))
    vmax = float(np.abs(mesh_ref.node_values(dens.numpy(), scale, pre)).max())
    dens_q = out[:, -1].detach().double().cpu().numpy()
    if post == abi.ACT_SOFTPLUS:
        pre_q = np.where(dens_q > 20, dens_q, np.log(np.expm1(np.maximum(dens_q, 1e-30))))
    else:
        pre_q = dens_q
    assert np.abs(pre_q - L).max() < 1e-4 * vmax
    # colours: sigmoid(C0 * DC) of a float64 trilinear of the DC channels (index c * (deg+1)^2)
    ncoef = feat.shape[-1] // 3
    dc = _trilerp64(feat.numpy()[..., 0::ncoef], aabb, v)
    assert np.abs(mesh.colours.cpu().numpy() - 1 / (1 + np.exp(-C0 * dc))).max() < 1e-5


def _trilerp64(grid, aabb, p):
    """grid_sample(align_corners=False, zero padding) of grid [X,Y,Z,C] at world points p, in float64"""
    N = np.array(grid.shape[:3])
    lo, hi = np.array([a[0] for a in aabb]), np.array([a[1] for a in aabb])
    u = (p.astype(np.float64) - lo) / (hi - lo) * N - 0.5
    i0 = np.floor(u).astype(np.int64)
    w1 = u - i0
    out = np.zeros((len(p), grid.shape[-1]))
    for c in range(8):
        o = np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])
        idx = i0 + o
        ok = np.all((idx >= 0) & (idx < N), axis=1)
        w = np.prod(np.where(o == 1, w1, 1 - w1), axis=1) * ok
        ic = np.clip(idx, 0, N - 1)
        out += w[:, None] * grid[ic[:, 0], ic[:, 1], ic[:, 2]]
    return out


def test_checkpoint_mesh_lies_on_its_surface():
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.mesh import extract_mesh
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict

    vm, _ = create_volumetric_model_from_saved_model(os.path.join(GOLDEN, "ref_checkpoint.pth"),
                                                     create_voxel_grid_from_saved_info_dict, device=DEV)
    vg = vm.thre3d_repr
    sigma = torch.nn.functional.softplus(vg.densities.detach() * float(vg._expected_density_scale))
    level = float(torch.quantile(sigma.flatten().cpu(), 0.8))
    mesh = extract_mesh(vg, level=level)
    assert len(mesh.faces) > 0 and mesh_ref.is_closed(mesh.faces.cpu().numpy())
    q = vg(mesh.vertices)[:, -1].detach().double().cpu().numpy()
    L = float(mesh_ref.iso_value(abi.ACT_SOFTPLUS, level))
    pre = np.where(q > 20, q, np.log(np.expm1(q)))
    vmax = float(vg.densities.detach().abs().max()) * float(vg._expected_density_scale)
    assert np.abs(pre - L).max() < 1e-4 * vmax


def test_sphere_160_closed_oriented_with_the_analytic_volume():
    n, r = 160, 0.6
    field = torch.from_numpy(mesh_ref.sphere_field(n, 2 * r))[..., None].to(DEV)
    spec = ops.GridSpec(aabb=((-1.0, 1.0),) * 3, density_post_act=abi.ACT_IDENTITY)
    v, f = ops.extract_mesh(spec, field, 0.5)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert mesh_ref.is_closed(f) and mesh_ref.euler_characteristic(f) == 2
    assert abs(mesh_ref.volume(v, f) / (4.0 / 3.0 * math.pi * r ** 3) - 1) < 0.01   # > 0: outward normals
    two = np.maximum(mesh_ref.sphere_field(96, 0.6, (-0.45, 0, 0)), mesh_ref.sphere_field(96, 0.6, (0.45, 0, 0)))
    _, f2 = ops.extract_mesh(spec, torch.from_numpy(two)[..., None].to(DEV), 0.5)
    assert mesh_ref.euler_characteristic(f2.cpu().numpy()) == 4
    _, f3 = ops.extract_mesh(spec, torch.from_numpy(mesh_ref.torus_field(96))[..., None].to(DEV), 0.5)
    assert mesh_ref.is_closed(f3.cpu().numpy()) and mesh_ref.euler_characteristic(f3.cpu().numpy()) == 0


def test_masks():
    dens, _ = workload.random_grid(32, seed=11)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_pre_act=abi.ACT_ABS, density_post_act=abi.ACT_RELU)
    d = dens.to(DEV)
    v0, f0 = ops.extract_mesh(spec, d, 0.4)
    v1, f1 = ops.extract_mesh(spec, d, 0.4, mask=torch.ones(32, 32, 32, dtype=torch.bool, device=DEV))
    assert torch.equal(v0, v1) and torch.equal(f0, f1)
    mask = torch.rand(32, 32, 32, generator=torch.Generator().manual_seed(2)) > 0.4
    vm, fm = ops.extract_mesh(spec, d, 0.4, mask=mask.to(DEV))
    vz, fz = ops.extract_mesh(spec, torch.where(mask[..., None], dens, 0.0).to(DEV), 0.4)
    assert torch.equal(vm, vz) and torch.equal(fm, fz)
    assert mesh_ref.is_closed(fm.cpu().numpy())
    rv, rf = mesh_ref.extract(dens.numpy(), spec.aabb, 0.4, 1.0, abi.ACT_ABS, abi.ACT_RELU, mask=mask.numpy())
    assert np.array_equal(fm.cpu().numpy(), rf)


def test_edit_region_mask_of_refine_scene():
    from thre3d_atom.thre3d_reprs.mesh import extract_mesh

    side = 48
    dens, col, edit, _ = workload.refine_scene(side)
    vg = _grid(dens, col, [(-1.5, 1.5)] * 3)
    mesh = extract_mesh(vg, level=0.5, mask=torch.from_numpy(edit))
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    assert len(f) > 0 and mesh_ref.is_closed(f) and mesh_ref.volume(v, f) > 0
    idx = np.argwhere(edit)
    vox = 3.0 / side
    lo = -1.5 + (idx.min(0) - 1) * vox
    hi = -1.5 + (idx.max(0) + 2) * vox     # bounding box of the region dilated by one voxel
    assert np.all(v >= lo - 1e-5) and np.all(v <= hi + 1e-5)


def test_deterministic_and_capacity_guard():
    dens, _ = workload.random_grid(40, seed=5)
    spec = ops.GridSpec(aabb=((-1.0, 1.0),) * 3, density_pre_act=abi.ACT_ABS, density_post_act=abi.ACT_IDENTITY)
    d = dens.to(DEV)
    va, fa = ops.extract_mesh(spec, d, 0.35)
    vb, fb = ops.extract_mesh(spec, d, 0.35)
    assert torch.equal(va.view(torch.int32), vb.view(torch.int32)) and torch.equal(fa, fb)
    V, T = len(va), len(fa)
    L = ops.lib()
    g = make_grid_desc(d.data_ptr(), d.data_ptr(), (40, 40, 40), 1, spec.aabb, 1.0, abi.ACT_ABS, abi.ACT_IDENTITY)
    nb = L.voxe_mesh_scratch_bytes(40, 40, 40)
    sc = torch.empty(nb, dtype=torch.uint8, device=DEV)
    tot = torch.empty(2, dtype=torch.int64, device=DEV)
    guard = 4096
    vbuf = torch.full(((V - 1) * 3 + guard,), 7.0, device=DEV)
    fbuf = torch.full(((T - 1) * 3 + guard,), -7, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert L.voxe_mesh_count(ctypes.byref(g), 0.35, None, tot.data_ptr(), sc.data_ptr(), nb, st) == 0
    assert tot.tolist() == [V, T]
    assert L.voxe_mesh_emit(ctypes.byref(g), 0.35, None, vbuf.data_ptr(), V - 1, fbuf.data_ptr(), T - 1,
                            sc.data_ptr(), nb, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(vbuf[:(V - 1) * 3], va[:V - 1].flatten()) and torch.equal(fbuf[:(T - 1) * 3], fa[:T - 1].flatten())
    assert bool((vbuf[(V - 1) * 3:] == 7.0).all()) and bool((fbuf[(T - 1) * 3:] == -7).all())


def test_stress_256_and_count_agreement():
    dens, _ = workload.random_grid(256, nfeat=1)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_pre_act=abi.ACT_ABS, density_post_act=abi.ACT_IDENTITY)
    v, f = ops.extract_mesh(spec, dens.to(DEV), 0.5)
    assert len(f) > 10_000_000 and int(f.min()) >= 0 and int(f.max()) == len(v) - 1
    small, _ = workload.random_grid(72, nfeat=1, seed=9)
    vs, fs = ops.extract_mesh(spec, small.to(DEV), 0.5)
    rv, rf = mesh_ref.extract(small.numpy(), spec.aabb, 0.5, 1.0, abi.ACT_ABS, abi.ACT_IDENTITY)
    assert len(fs) == len(rf) and len(vs) == len(rv)


def test_rejections():
    from thre3d_atom.thre3d_reprs.mesh import extract_mesh
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    dens, feat = workload.random_grid(8)
    vg = VoxelGrid(dens.to(DEV), feat.to(DEV), VoxelSize(0.1, 0.1, 0.1), feature_postactivation=torch.nn.Sigmoid())
    with pytest.raises(VoxeError):
        extract_mesh(vg, level=0.5)
    sp = _grid(dens, feat, [(-1, 1)] * 3, post=torch.nn.Softplus())
    with pytest.raises(VoxeError):
        extract_mesh(sp, level=math.log(2.0))
    with pytest.raises(VoxeError):
        extract_mesh(_grid(dens, feat, [(-1, 1)] * 3), level=0.0)
    with pytest.raises(VoxeError):
        extract_mesh(_grid(dens, feat, [(-1, 1)] * 3), level=0.5, mask=torch.ones(8, 8, 7, dtype=torch.bool))


def _cli():
    spec = importlib.util.spec_from_file_location("export_mesh_cli", os.path.join(ROOT, "export_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_on_checkpoint_and_refined_model(tmp_path):
    import copy

    from click.testing import CliRunner

    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict

    mod = _cli()
    out = tmp_path / "ref.ply"
    ckpt = os.path.join(GOLDEN, "ref_checkpoint.pth")
    res = CliRunner().invoke(mod.main, ["-i", ckpt, "-o", str(out)])
    assert res.exit_code == 0, (res.output, res.exception)
    xyz, rgb, faces = parse_ply(out)
    assert len(faces) > 0 and mesh_ref.is_closed(faces) and "T = " in res.output
    # a refined model: keep grid (attn) 0 on a slab of the object, -5 / -10 elsewhere
    vm, extra = create_volumetric_model_from_saved_model(ckpt, create_voxel_grid_from_saved_info_dict, device=DEV)
    refined = copy.deepcopy(vm)
    keep = torch.full_like(refined.thre3d_repr.densities.detach(), -10.0)
    keep[:, :, 2:5] = 0.0
    refined.thre3d_repr.add_attn_params(keep)
    path = tmp_path / "refined.pth"
    torch.save(refined.get_save_info(extra), path)
    out2 = tmp_path / "edit.ply"
    res = CliRunner().invoke(mod.main, ["-i", str(path), "-o", str(out2), "--edit_region_only"])
    assert res.exit_code == 0, (res.output, res.exception)
    xyz2, _, faces2 = parse_ply(out2)
    assert len(faces2) > 0 and mesh_ref.is_closed(faces2)
    assert xyz2[:, 2].min() >= -1.0 - 1e-5      # inside the slab dilated by one voxel (z voxels 1..5 of [-1.5, 1.5])
    res = CliRunner().invoke(mod.main, ["-i", ckpt, "-o", str(tmp_path / "x.ply"), "--edit_region_only"])
    assert res.exit_code != 0
