"""GPU checks of the density-gradient normals (voxe_query_normals / voxe_render_normals, thre3d_reprs.geometry, the entry points'
new options): agreement with the float64 restatement tests/normals_ref.py, depth / acc against the colour forward, an analytic
sphere, the mesh export's winding, determinism, no interference with a forward / backward or a recon step, edge cases."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_ref
import normals_ref
from conftest import GOLDEN, ROOT
from test_normals_host import parse_ply_normals
from voxe_hip import abi, ops, workload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
AABB = ((-1.1, 1.3), (-0.8, 0.9), (-1.25, 0.7))      # unequal voxel sizes with the non-cubic dims below


def _rand_grid(dims, F=3, seed=0, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    d = torch.empty((*dims, 1)).uniform_(lo, hi, generator=g)
    f = torch.empty((*dims, F)).uniform_(-1, 1, generator=g)
    return d.to(DEV), f.to(DEV)


def _test_points(dims, aabb, n, seed):
    """random points inside and around the grid, within one voxel of every face, outside it and exactly on lattice planes"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.tensor([a[0] for a in aabb], dtype=torch.float64)
    hi = torch.tensor([a[1] for a in aabb], dtype=torch.float64)
    size = (hi - lo) / torch.tensor(dims, dtype=torch.float64)
    inner = lo + torch.rand((n, 3), generator=g, dtype=torch.float64) * (hi - lo)
    around = lo - 1.5 * size + torch.rand((n, 3), generator=g, dtype=torch.float64) * (hi - lo + 3 * size)
    face = inner.clone()[: 6 * (n // 6)].view(6, -1, 3)
    for f in range(6):
        a, side = f // 2, f % 2
        t = torch.rand(face.shape[1], generator=g, dtype=torch.float64) * size[a]
        face[f, :, a] = (lo[a] + t) if side == 0 else (hi[a] - t)
    lattice = inner[: n // 2].clone()
    idx = torch.randint(-1, max(dims) + 1, (n // 2, 3), generator=g)
    for a in range(3):   # voxel centres (u integer) on one axis per point
        ax = torch.randint(0, 3, (n // 2,), generator=g) == a
        u = idx[:, a].clamp(-1, dims[a]).to(torch.float64)
        lattice[ax, a] = lo[a] + (u[ax] + 0.5) * size[a]
    pts = torch.cat([inner, around, face.reshape(-1, 3), lattice]).to(torch.float32)
    return pts.to(DEV)


def _well_conditioned(v, pts, aabb, G):
    """points where |G| stands out of the float32 rounding of the weighted corner values (~1e-7 max|v| per voxel size): below
    1e-2 of that scale a 1e-5 direction error is rounding, not a wrong normal"""
    vmax = float(v.abs().max())
    scale = max(n * (aabb[a][1] - aabb[a][0]) ** -1 for a, n in enumerate(v.shape))
    return G.norm(dim=1) > 1e-2 * vmax * scale


@pytest.mark.parametrize("pre,post", [(abi.ACT_IDENTITY, abi.ACT_IDENTITY), (abi.ACT_ABS, abi.ACT_RELU),
                                      (abi.ACT_IDENTITY, abi.ACT_SOFTPLUS), (abi.ACT_ABS, abi.ACT_SOFTPLUS)])
def test_query_normals_match_the_restatement(pre, post):
    dims = (19, 11, 14)
    dens, feat = _rand_grid(dims, seed=pre * 7 + post)
    spec = ops.GridSpec(aabb=AABB, density_scale=1.7, density_pre_act=pre, density_post_act=post)
    pts = _test_points(dims, AABB, 6000, seed=post)
    got = ops.query_normals(spec, dens, pts).double()
    v = normals_ref.field(dens, spec.density_scale, pre)
    V, G = normals_ref.value_and_gradient(v, pts, AABB)
    # the restatement's axis order and field, through the point-query kernel VoxelGrid.forward uses
    q = ops.query_points(spec, dens, feat, pts)[:, -1].double()
    assert torch.allclose(q, normals_ref.post(post, V), atol=2e-6, rtol=1e-6)
    ref = normals_ref.normals_from_gradient(G)
    ok = _well_conditioned(v, pts, AABB, G)
    assert float(ok.float().sum() / (G.norm(dim=1) > 0).float().sum()) > 0.9
    assert float((got - ref)[ok].abs().max()) <= 1e-5
    assert bool(((got.norm(dim=1) - 1).abs() < 1e-5)[ok].all())
    assert bool((got[G.norm(dim=1) == 0] == 0).all())   # outside the grid: exact zeros
    assert int((G.norm(dim=1) == 0).sum()) > 100
    # a constant grid: exact zeros inside, and the faces' zero padding gives outward normals in the boundary cells only
    const = torch.full_like(dens, 0.6)
    n0 = ops.query_normals(spec, const, pts)
    _, G0 = normals_ref.value_and_gradient(normals_ref.field(const, spec.density_scale, pre), pts, AABB)
    assert bool((n0[G0.norm(dim=1) == 0] == 0).all()) and int((G0.norm(dim=1) == 0).sum()) > 1000


def _cameras(hw, n, first=0):
    from thre3d_atom.utils.imaging_utils import pose_spherical

    rays = [ops.cast_rays(hw, hw, workload.focal_for(hw), *pose_spherical(*workload.synth_pose_angles(i, 8), workload.RADIUS), DEV)
            for i in range(first, first + n)]
    return torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays])


def _render_cases():
    # (name, sh degree, hw, views, perturb, jitter kind, aabb_clip, lindisp, order)
    return [
        ("sh0_plain", 0, 48, 1, False, None, False, False, "image"),
        ("sh0_hash_clip", 0, 40, 1, True, None, True, False, "image"),
        ("sh0_hash_lindisp_multiview", 0, 24, 3, True, None, False, True, "multiview"),
        ("sh2_jitter_shuffled", 2, 32, 1, True, "caller", False, False, "shuffled"),
        ("sh2_hash_clip_lindisp_linear", 2, 36, 1, True, None, True, True, "linear"),
        # the host's lanes per ray (lanes_per_ray): 8 below 262 144 rays, 4 below 524 288, 2 below 1 048 576, then 1
        ("sh0_400_g8", 0, 400, 1, False, None, True, False, "image"),
        ("sh0_600_g4_jitter", 0, 600, 1, True, "caller", False, False, "linear"),
        ("sh0_800_g2", 0, 800, 1, False, None, False, False, "image"),
        ("sh0_1040_g1", 0, 1040, 1, False, None, True, False, "linear"),
    ]


@pytest.mark.parametrize("case", _render_cases(), ids=lambda c: c[0])
def test_render_normals_match_the_restatement_and_the_forward(case):
    name, deg, hw, views, perturb, jkind, clip, lindisp, order = case
    dims = (26, 20, 23)
    F = 3 * (deg + 1) ** 2
    g = torch.Generator().manual_seed(len(name))
    dens = (torch.empty((*dims, 1)).uniform_(-1, 1, generator=g) * 1.5).to(DEV)
    feat = torch.empty((*dims, F)).uniform_(-1, 1, generator=g).to(DEV)
    aabb = ((-1.3, 1.2), (-1.0, 1.1), (-1.4, 1.0))
    spec = ops.GridSpec(aabb=aabb, density_scale=2.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS)
    ro, rd = _cameras(hw, views)
    R = ro.shape[0]
    S = 96 if R < 100000 else 64
    width = height = 0
    if order in ("image", "multiview"):
        width = hw
        height = hw if order == "multiview" else 0
    elif order == "shuffled":
        perm = torch.randperm(R, generator=g).to(DEV)
        ro, rd = ro[perm].contiguous(), rd[perm].contiguous()
    params = ops.RenderParams(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=perturb, linear_disparity=lindisp,
                              aabb_clip=clip, white_bkgd=True, sh_degree=deg, image_width=width, image_height=height)
    jitter = torch.rand((R, S), generator=g).to(DEV) if jkind == "caller" else None
    rng = (1234, 77) if perturb and jitter is None else (0, 0)
    N, depth, acc = ops.render_normals(spec, params, dens, ro, rd, jitter=jitter, rng=rng)
    assert not N.requires_grad and N.shape == (R, 3) and depth.shape == (R, 1) and acc.shape == (R, 1)
    # the restatement on (a subset of) the rays: the probe needs the same ray indices for the hash stream
    sub = torch.arange(R, device=DEV) if R <= 20000 else torch.randperm(R, generator=g)[:8000].to(DEV)
    if R > 20000:
        assert jitter is not None or not perturb
        p_sub = ops.RenderParams(**{**vars(params), "image_width": 0, "image_height": 0})
        args = (ro[sub].contiguous(), rd[sub].contiguous(), None if jitter is None else jitter[sub].contiguous())
    else:
        p_sub, args = params, (ro, rd, jitter)
    rN, rdepth, racc = normals_ref.render_normals(spec, p_sub, dens, feat, *args, rng=rng)
    assert float((N[sub].double() - rN).abs().max()) <= 1e-4
    assert float((acc[sub, 0].double() - racc).abs().max()) <= 1e-5
    assert bool((N.norm(dim=1) <= acc[:, 0] * (1 + 1e-5) + 1e-6).all())
    assert float(acc.max()) > 0.5 and float(N.norm(dim=1).max()) > 0.1
    # depth and acc: the colour forward's, same cfg and rng
    with torch.no_grad():
        _, fdepth, facc, _ = ops.render(spec, params, dens, feat, ro, rd, jitter=jitter, rng=rng)
    assert float((acc - facc).abs().max()) <= 2e-6
    assert float(((depth - fdepth).abs() / fdepth.abs().clamp_min(1e-3)).max()) <= 1e-5


def test_analytic_sphere_normals_are_radial():
    from thre3d_atom.utils.imaging_utils import pose_spherical

    dims = (70, 58, 64)
    aabb = ((-1.2, 1.3), (-1.0, 1.1), (-1.1, 1.2))
    centre = torch.tensor([0.15, -0.1, 0.05], dtype=torch.float64)
    r0 = 0.7
    axes = [torch.tensor([aabb[a][0] + (i + 0.5) * (aabb[a][1] - aabb[a][0]) / dims[a] for i in range(dims[a])],
                         dtype=torch.float64) for a in range(3)]
    x, y, z = torch.meshgrid(*axes, indexing="ij")
    dist = torch.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    dens = (40.0 * (r0 - dist)).to(torch.float32)[..., None].to(DEV)   # linear radial field, softplus: an opaque ball
    spec = ops.GridSpec(aabb=aabb, density_scale=1.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS)
    hw = 96
    pose = pose_spherical(35.0, 25.0, 4.0)
    ro, rd = ops.cast_rays(hw, hw, workload.focal_for(hw), pose.rotation, pose.translation, DEV)
    params = ops.RenderParams(num_samples=384, near=1.5, far=6.5, image_width=hw)
    N, depth, acc = ops.render_normals(spec, params, dens, ro, rd)
    m = acc[:, 0] > 0.99
    assert int(m.sum()) > 500
    p = (ro + rd * (depth / acc))[m].double().cpu()
    radial = (p - centre) / (p - centre).norm(dim=1, keepdim=True)
    n = N[m].double().cpu()
    cos = (n * radial).sum(dim=1) / n.norm(dim=1)
    assert float(torch.rad2deg(torch.arccos(cos.clamp(-1, 1))).max()) <= 3.0
    # a camera aimed at the centre: its centre pixel sees the sphere head on, (0, 0, 1) in camera space
    from thre3d_atom.thre3d_reprs.geometry import normals_to_camera

    rot = torch.as_tensor(pose.rotation, dtype=torch.float64)
    eye = centre + 4.0 * rot[:, 2]
    aim = type(pose)(pose.rotation, eye.to(torch.float32)[:, None])
    o1, d1 = ops.cast_rays(hw, hw, workload.focal_for(hw), aim.rotation, aim.translation, DEV)
    N1, _, a1 = ops.render_normals(spec, params, dens, o1, d1)
    c = (hw // 2) * hw + hw // 2
    cam = normals_to_camera(N1[c:c + 1].double(), aim)[0]
    assert float(a1[c]) > 0.99
    assert float(torch.rad2deg(torch.arccos((cam / cam.norm())[2].clamp(-1, 1)))) <= 3.0


def test_vertex_normals_agree_with_the_mesh_winding():
    from test_mesh_gpu import _grid
    from thre3d_atom.thre3d_reprs.geometry import vertex_normals
    from thre3d_atom.thre3d_reprs.mesh import extract_mesh

    d48, f48 = workload.random_grid(40, seed=9)
    sph = torch.from_numpy(mesh_ref.sphere_field(48, 1.1))[..., None]
    for dens, feat, level, post in ((d48, f48, 0.35, torch.nn.Identity()), (sph, torch.rand(48, 48, 48, 3), 0.9, torch.nn.Softplus())):
        vg = _grid(dens, feat, [(-1.0, 1.2), (-0.9, 1.0), (-1.1, 0.8)], 1.0, torch.nn.Identity(), post)
        mesh = extract_mesh(vg, level=level)
        v, f = mesh.vertices.double().cpu(), mesh.faces.long().cpu()
        fn = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)   # area-weighted, outward
        acc = torch.zeros_like(v).index_add_(0, f[:, 0], fn).index_add_(0, f[:, 1], fn).index_add_(0, f[:, 2], fn)
        n = vertex_normals(vg, mesh.vertices).double().cpu()
        agree = ((n * acc).sum(dim=1) > 0).double().mean()
        assert len(f) > 200 and float(agree) >= 0.99, float(agree)
        assert float((n.norm(dim=1) - 1).abs().max()) < 1e-5


def test_deterministic_and_edge_cases():
    dens, feat = _rand_grid((32, 24, 28), seed=5)
    spec = ops.GridSpec(aabb=AABB, density_scale=2.0)
    ro, rd = _cameras(64, 2)
    params = ops.RenderParams(num_samples=128, near=workload.NEAR, far=workload.FAR, perturb=True, image_width=64,
                              image_height=64)
    a = ops.render_normals(spec, params, dens, ro, rd, rng=(5, 6))
    b = ops.render_normals(spec, params, dens, ro, rd, rng=(5, 6))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    pts = _test_points((32, 24, 28), AABB, 3000, 1)
    assert torch.equal(ops.query_normals(spec, dens, pts), ops.query_normals(spec, dens, pts))
    # R = 0 / N = 0
    e = torch.zeros((0, 3), device=DEV)
    n0, d0, a0 = ops.render_normals(spec, params, dens, e, e)
    assert n0.shape == (0, 3) and d0.shape == (0, 1) and ops.query_normals(spec, dens, e).shape == (0, 3)
    # S = 2048
    p2 = ops.RenderParams(num_samples=2048, near=workload.NEAR, far=workload.FAR, perturb=True)
    n2, dd2, a2 = ops.render_normals(spec, p2, dens, ro[:3000], rd[:3000], rng=(1, 2))
    _, fd2, fa2, _ = ops.render(spec, p2, dens, feat, ro[:3000], rd[:3000], rng=(1, 2))
    assert bool(torch.isfinite(n2).all()) and float((a2 - fa2).abs().max()) <= 2e-6
    # 256^3 at 800 x 800, S = 512
    d256, _ = workload.random_grid(256, nfeat=1, seed=2)
    big = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=2.0)
    o8, r8 = _cameras(800, 1, first=3)
    p8 = ops.RenderParams(num_samples=512, near=workload.NEAR, far=workload.FAR, perturb=True, image_width=800)
    n8, dp8, a8 = ops.render_normals(big, p8, d256.to(DEV), o8, r8)
    assert all(bool(torch.isfinite(t).all()) for t in (n8, dp8, a8)) and float(a8.max()) > 0.5


def _prefetch_stats():
    import ctypes

    out = (ctypes.c_int64 * 3)()
    assert ops.lib().voxe_recon_prefetch_stats(out) == 0
    return list(out)


def test_no_interference_with_forward_backward_and_recon_step():
    dens0, feat0 = _rand_grid((40, 40, 40), seed=8)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=3.0)
    ro, rd = _cameras(64, 1)
    # (the fixed-point backward: two backward passes of the same forward give the same bits)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, image_width=64,
                              deterministic=True)
    g_col = torch.rand((ro.shape[0], 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    grads = []
    for with_normals in (False, True):
        d, f = dens0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
        ws = ops.Workspace()
        col = ops.render(spec, params, d, f, ro, rd, workspace=ws, rng=(3, 4))[0]
        if with_normals:
            ops.render_normals(spec, params, d, ro, rd, rng=(3, 4))
            ops.query_normals(spec, d, ro)
        (col * g_col).sum().backward()
        grads.append((d.grad.clone(), f.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    # recon_step -> recon_prefetch -> (render_normals) -> recon_step: the hint is taken either way, the iterations agree
    from thre3d_atom.utils.imaging_utils import pose_spherical

    hw, K, batch = 64, 6, 20000
    poses = torch.stack([torch.cat([p.rotation, p.translation], dim=-1) for p in
                         (pose_spherical(*workload.synth_pose_angles(i, K), workload.RADIUS) for i in range(K))]).to(DEV)
    images = torch.rand(K, 3, hw, hw, generator=torch.Generator().manual_seed(1)).to(DEV)
    rows = torch.arange(K, device=DEV)
    rp = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True)
    results = []
    for with_normals in (False, True):
        d, f = dens0.clone(), feat0.clone()
        st_d = (torch.zeros_like(d), torch.zeros_like(d))
        st_f = (torch.zeros_like(f), torch.zeros_like(f))
        wa, wb = ops.Workspace(), ops.Workspace()
        losses = torch.zeros(4, device=DEV)
        common = (spec, rp, d, f, wa, wb, hw, hw, workload.focal_for(hw), poses, rows, images, batch, True)
        ops.recon_step_(*common, st_d, st_f, 1, 1, 2e-2, losses, (11, 0), zero_gradient_first=True)
        first = losses.tolist()
        ops.recon_prefetch_(*common, losses, (11, 1000))
        s0 = _prefetch_stats()
        if with_normals:
            ops.render_normals(spec, params, d, ro, rd, rng=(3, 4))
            ops.query_normals(spec, d, ro)
        ops.recon_step_(*common, st_d, st_f, 2, 2, 2e-2, losses, (11, 1000), zero_gradient_first=False)
        torch.cuda.synchronize()
        s1 = _prefetch_stats()
        assert s1[1] - s0[1] == 1 and s1[2] == s0[2], (with_normals, s0, s1)   # the hint was taken, not dropped
        results.append((first, losses.tolist(), d.clone(), f.clone()))
    (a_first, a_loss, a_d, a_f), (b_first, b_loss, b_d, b_f) = results
    assert a_first == b_first
    for x, y in zip(a_loss, b_loss):
        assert abs(x - y) < 2e-6 + 2e-5 * abs(x), (a_loss, b_loss)
    for a, b, x0 in ((a_d, b_d, dens0), (a_f, b_f, feat0)):
        assert float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(a - x0)) < 0.05


def test_render_geometry_on_the_checkpoint():
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.geometry import render_geometry
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict
    from thre3d_atom.utils.constants import CAMERA_INTRINSICS, HEMISPHERICAL_RADIUS
    from thre3d_atom.utils.imaging_utils import get_thre360_animation_poses

    vm, extra = create_volumetric_model_from_saved_model(os.path.join(GOLDEN, "ref_checkpoint.pth"),
                                                         create_voxel_grid_from_saved_info_dict, device=DEV)
    intr = extra[CAMERA_INTRINSICS]
    pose = get_thre360_animation_poses(extra[HEMISPHERICAL_RADIUS], 60.0, 4)[1]
    geo = render_geometry(vm, pose, intr, num_samples_per_ray=96)
    H, W = int(intr.height), int(intr.width)
    assert geo.colour.shape == (H, W, 3) and geo.depth.shape == (H, W, 1) and geo.acc.shape == (H, W, 1)
    assert geo.normal_world.shape == (H, W, 3) and geo.normal_camera.shape == (H, W, 3)
    # the colour path's acc (one forward with the same rng and config) matches the normals path's
    from thre3d_atom.rendering.volumetric.utils.misc import cast_rays, flatten_rays
    from thre3d_atom.thre3d_reprs.renderers import _render_params

    grid = vm.thre3d_repr
    cfg = vm._update_render_config(vm.render_config, {"num_samples_per_ray": 96})
    rays = flatten_rays(cast_rays(intr, pose, device=DEV))
    params = _render_params(grid, rays, cfg, attn=False)
    torch.manual_seed(5)
    geo = render_geometry(vm, pose, intr, num_samples_per_ray=96)
    torch.manual_seed(5)
    rng = ops._next_rng() if params.perturb else (0, 0)
    with torch.no_grad():
        colour, _, facc, _ = ops.render(grid.voxe_grid_spec(), params, grid.densities, grid.features, rays.origins,
                                        rays.directions, rng=rng)
    assert torch.equal(colour.view(H, W, 3), geo.colour)
    assert float((facc.view(H, W, 1) - geo.acc).abs().max()) <= 2e-6
    assert float((geo.normal_world.norm(dim=-1) - geo.acc[..., 0]).max()) <= 1e-5


def _load_cli(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_geometry_frames_and_vertex_normals(tmp_path):
    from click.testing import CliRunner
    from PIL import Image

    ckpt = os.path.join(GOLDEN, "ref_checkpoint.pth")
    mod = _load_cli("render_sh_based_voxel_grid.py")
    base = ["-i", ckpt, "--num_frames", "4", "--render_scale_factor", "1.0", "--overridden_num_samples_per_ray", "64"]
    plain, geo = tmp_path / "plain", tmp_path / "geo"
    res = CliRunner().invoke(mod.main, base + ["-o", str(plain)])
    assert res.exit_code == 0, (res.output, res.exception)
    res = CliRunner().invoke(mod.main, base + ["-o", str(geo), "--render_geometry"])
    assert res.exit_code == 0, (res.output, res.exception)
    frames = sorted(geo.glob("geometry_*.png"))
    assert len(frames) == 3
    col = np.asarray(Image.open(sorted(geo.glob("frame_*.png"))[0]))
    img = np.asarray(Image.open(frames[0]))
    H, W = col.shape[:2]
    assert img.shape == (H, 4 * W, 3) and np.array_equal(img[:, :W], col)
    names = {p.name for p in plain.iterdir()}
    assert not any(n.startswith("geometry") or "geometry" in n for n in names)
    assert {p.name for p in geo.iterdir()} - names == {f.name for f in frames} | {
        n.replace("rendered_video", "rendered_geometry_video") for n in names if n.startswith("rendered_video")}
    # export_mesh.py --vertex_normals
    exp = _load_cli("export_mesh.py")
    out = tmp_path / "m.ply"
    res = CliRunner().invoke(exp.main, ["-i", ckpt, "-o", str(out), "--vertex_normals"])
    assert res.exit_code == 0, (res.output, res.exception)
    xyz, n, _, idx = parse_ply_normals(out)
    assert len(xyz) > 0 and float(np.abs(np.linalg.norm(n, axis=1) - 1).max()) < 1e-5
