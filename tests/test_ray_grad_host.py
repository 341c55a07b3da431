"""CPU checks of the ray and camera-pose gradients: the float64 restatement tests/ray_grad_ref.py against
the oracle's forward, against the reference's own autograd (tests/golden/ray_grads.npz) and against finite differences; the
definition of voxe_cast_rays_bwd by hand; CameraPoseDeltas; the C ABI's declarations and argument validation (no device work);
the entry points; and pose recovery on the restatement.  tests/test_ray_grad_gpu.py builds its inputs with the functions below."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ray_grad_ref as RR
import test_distortion_host as TD
import test_visibility_host as H
from conftest import ROOT
from voxe_hip import abi, ops, workload
from voxe_hip.desc import make_grid_desc, make_render_cfg

CPU = torch.device("cpu")
GOLDEN = os.path.join(ROOT, "tests", "golden")
GRAD_REL_L2 = 1e-4          # the project's gradient bound
COLOUR_ABS = 5e-6           # the project's colour bound
KINDS = {   # make_grid's kinds in tools/gen_golden.py: (pre, post, density scale)
    "softplus": (abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, 100.0 / 3.0),
    "softplus_soft": (abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, 2.0),
    "relu": (abi.ACT_IDENTITY, abi.ACT_RELU, 100.0 / 3.0),
    "abs": (abi.ACT_ABS, abi.ACT_IDENTITY, 1.0),
}


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ---- inputs shared with the GPU tests ---------------------------------------------------------------------------------
def golden_cases():
    return [f"{kind}_{mode}" for kind in ("softplus", "relu", "abs") for mode in ("plain", "jit")] + \
           [f"deg{deg}_{mode}" for deg in (1, 2, 3) for mode in ("full", "diffuse")]


_npz = {}


def _load(name):
    if name not in _npz:
        with np.load(os.path.join(GOLDEN, name)) as z:
            _npz[name] = {k: z[k] for k in z.files}
    return _npz[name]


def golden_inputs(case, device):
    """dict of one case of tests/golden/ray_grads.npz: spec, params, dens, feat, ro, rd, jitter, g_col, g_dep, g_acc and the
    reference's d_o, d_d, colour.  The grids are those of render_sh0.npz / render_shdeg.npz (the generator asserts it)."""
    G = _load("ray_grads.npz")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    near, far = (float(v) for v in G["bounds"])
    if case.startswith("deg"):
        deg, mode = int(case[3]), case.split("_")[1]
        grids, prefix, kind, rays = _load("render_shdeg.npz"), f"deg{deg}_", "softplus_soft", "deg"
        params = ops.RenderParams(num_samples=32, near=near, far=far, white_bkgd=True, sh_degree=deg, render_diffuse=mode == "diffuse")
    else:
        kind, mode = case.split("_")
        grids, prefix, rays = _load("render_sh0.npz"), kind + "_", "sh0"
        params = ops.RenderParams(num_samples=64, near=near, far=far, white_bkgd=True, perturb=mode == "jit")
    pre, post, scale = KINDS[kind]
    aabb = tuple((float(lo), float(hi)) for lo, hi in grids[prefix + "aabb"])
    spec = ops.GridSpec(aabb=aabb, density_scale=scale, density_pre_act=pre, density_post_act=post)
    key = case + "_"
    return dict(spec=spec, params=params, dens=t(grids[prefix + "densities"]), feat=t(grids[prefix + "features"]),
                ro=t(G[rays + "_rays_o"]), rd=t(G[rays + "_rays_d"]), jitter=t(G[key + "jitter"]) if key + "jitter" in G else None,
                rng=(0, 0), g_col=t(G[key + "g_colour"]), g_dep=t(G[key + "g_depth"]), g_acc=t(G[key + "g_acc"]),
                d_o=t(G[key + "d_rays_o"]), d_d=t(G[key + "d_rays_d"]), colour=t(G[key + "colour"]))


def upstream(R, device, seed=43):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((R, 3), generator=g).to(device), (torch.randn((R,), generator=g) * 0.25).to(device),
            (torch.randn((R,), generator=g) * 0.25).to(device))


def agreement_cases():
    """(name of the distortion tests' case, SH degree): the DIMS = (26, 20, 23) anisotropic grid with the four image cases, linear
    batches R in {1, 63, 65} and S in {1, 2, 37}, each with SH-0 and SH-2 features"""
    return [(c, deg) for c in TD.agreement_cases() for deg in (0, 2)]


def agreement_inputs(case, deg, pre, post, device):
    """the distortion tests' inputs of `case` (densities carved to a central box: border rays see nothing) with SH-`deg`
    features and the colour + depth + acc upstream gradients"""
    spec, params, dens, feat, ro, rd, jitter, rng = TD.agreement_inputs(case, pre, post, device)
    if deg > 0:
        g = torch.Generator().manual_seed(100 + deg)
        feat = torch.empty((*H.DIMS, 3 * (deg + 1) ** 2)).uniform_(-1, 1, generator=g).to(device)
    params = ops.RenderParams(**{**vars(params), "sh_degree": deg, "white_bkgd": True})
    if params.num_samples == 1:
        # (the only sample of a ray sits at `near`: the S sweep's 3.0 is in front of the carved box -- every gradient would be 0;
        #  4.0 puts it inside the box for the central rays)
        params = ops.RenderParams(**{**vars(params), "near": 4.0})
    g_col, g_dep, g_acc = upstream(ro.shape[0], device)
    return dict(spec=spec, params=params, dens=dens, feat=feat, ro=ro, rd=rd, jitter=jitter, rng=rng, g_col=g_col, g_dep=g_dep,
                g_acc=g_acc)


def restatement(p, samples, dtype=torch.float64, g=("g_col", "g_dep", "g_acc")):
    ups = [p[k] if k in g else None for k in ("g_col", "g_dep", "g_acc")]
    return RR.ray_gradients(samples, p["dens"], p["feat"], p["ro"], p["rd"], p["spec"], p["params"], *ups, dtype=dtype)


def host_samples(p):
    return RR.probe_host(p["spec"], p["params"], p["dens"], p["feat"], p["ro"], p["rd"], p["jitter"], p["rng"])


# The pose-recovery scene (the GPU test optimises it with the kernels, the host test with the restatement)
POSE_HW, POSE_S, POSE_CAMERAS, POSE_STEPS, POSE_LR = 24, 48, (0, 3, 5), 100, 3e-3


def pose_scene(device):
    """(spec, params, densities, features): 16^3 over +-1.5, softplus at density scale 100 / 3; a ball at (0.3, 0.1, -0.2) with a
    soft skin and a box, smooth colours"""
    n = 16
    ax = (torch.arange(n, dtype=torch.float64) + 0.5) / n * 3.0 - 1.5
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt((x - 0.3) ** 2 + (y - 0.1) ** 2 + (z + 0.2) ** 2)
    box = ((x + 0.6).abs() < 0.35) & ((y + 0.5).abs() < 0.5) & ((z - 0.4).abs() < 0.3)
    one = torch.ones_like(r)
    raw = 0.3 * torch.clamp(torch.maximum(0.25 * (0.8 - r) / (3.0 / 16.0), torch.where(box, one, -one)), -1.0, 1.0)
    feat = 3.0 * torch.stack([torch.sin(2.0 * x + 1.0), torch.cos(3.0 * y), torch.sin(2.5 * z + 1.0)], dim=-1)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0)
    params = ops.RenderParams(num_samples=POSE_S, near=1.8, far=6.6, white_bkgd=True)
    return spec, params, raw.float()[..., None].contiguous().to(device), feat.float().contiguous().to(device)


def pose_cameras(device):
    """(true poses [3,3,4], perturbed poses [3,3,4], focal)"""
    from thre3d_atom.thre3d_reprs.poses import axis_angle_to_matrix
    from thre3d_atom.utils.imaging_utils import pose_spherical

    true = []
    for i in POSE_CAMERAS:
        pose = pose_spherical(*workload.synth_pose_angles(i, 8), workload.RADIUS)
        true.append(torch.cat([torch.as_tensor(pose.rotation).float(), torch.as_tensor(pose.translation).float().reshape(3, 1)], dim=1))
    true = torch.stack(true)
    g = torch.Generator().manual_seed(5)
    w = torch.randn(3, 3, generator=g)
    w = w / w.norm(dim=1, keepdim=True) * float(np.radians(3.0))
    dt = torch.randn(3, 3, generator=g)
    dt = dt / dt.norm(dim=1, keepdim=True) * 0.08
    noisy = torch.cat([axis_angle_to_matrix(w) @ true[:, :, :3], true[:, :, 3:] + dt[:, :, None]], dim=2)
    return true.to(device), noisy.to(device), workload.focal_for(POSE_HW)


def assert_pose_recovery(losses, rot0, rot1, tr0, tr1):
    """the three conditions of the pose-recovery tests"""
    print(f"pose recovery: loss {losses[0]:.4e} -> {losses[-1]:.4e} (x {losses[-1] / losses[0]:.2e});  rotation error "
          f"{[round(float(v), 3) for v in rot0]} -> {[round(float(v), 3) for v in rot1]} deg;  translation error "
          f"{[round(float(v), 4) for v in tr0]} -> {[round(float(v), 4) for v in tr1]}")
    assert losses[-1] <= losses[0] / 100.0
    assert float(rot1.mean()) <= 0.5 * float(rot0.mean())
    assert bool((rot1 <= rot0).all()) and float(tr1.mean()) <= float(tr0.mean())


# ---- the restatement against the oracle, the reference and finite differences -----------------------------------------
@pytest.mark.parametrize("case", golden_cases())
def test_restatement_forward_is_the_renderers(case):
    """the float64 restatement renders what voxe_cpu_render_fwd renders (and the reference): it differentiates the renderer's
    function"""
    from oracle import voxe_oracle as vo

    p = golden_inputs(case, CPU)
    spec, params = p["spec"], p["params"]
    with torch.no_grad():
        colour, depth, acc = RR.render_from_samples(*host_samples(p), p["dens"], p["feat"], p["ro"], p["rd"], spec, params)
    grid = vo.Grid(p["dens"].numpy(), p["feat"].numpy(), spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act)
    cfg = make_render_cfg(params.num_samples, params.near, params.far, params.perturb, white_bkgd=True, sh_degree=params.sh_degree,
                          render_diffuse=params.render_diffuse)
    want = vo.render_fwd(grid, cfg, p["ro"].numpy(), p["rd"].numpy(), None if p["jitter"] is None else p["jitter"].numpy())
    err = float((colour - torch.from_numpy(want["colour"]).double()).abs().max())
    err_ref = float((colour - p["colour"].double()).abs().max())
    print(f"{case}: colour max abs error vs the oracle {err:.3e}, vs the reference {err_ref:.3e}")
    assert err <= COLOUR_ABS and err_ref <= COLOUR_ABS
    assert float((acc - torch.from_numpy(want["acc"]).double()).abs().max()) <= COLOUR_ABS


@pytest.mark.parametrize("case", golden_cases())
def test_restatement_gradients_match_the_references_autograd(case):
    """bound: max(4 x yardstick, 1e-4) rel-L2 over [R,3], the yardstick being the restatement's own float32 run against its
    float64 run.  Measured (float64 restatement against the reference's float32 autograd): 3.9e-7 .. 2.9e-6 for d_o and for d_d,
    each within 7 % of its yardstick (3.8e-7 .. 3.0e-6)."""
    p = golden_inputs(case, CPU)
    samples = host_samples(p)
    o64, d64 = restatement(p, samples)
    o32, d32 = restatement(p, samples, dtype=torch.float32)
    for name, got, f32, want in (("d_o", o64, o32, p["d_o"]), ("d_d", d64, d32, p["d_d"])):
        yard = rel_l2(f32, got)
        err = rel_l2(got, want)
        print(f"{case} {name}: rel_l2 vs the reference {err:.3e} (float32 restatement vs float64: {yard:.3e})")
        assert err <= max(4.0 * yard, GRAD_REL_L2)
        assert float(want.norm()) > 0
    if not case.startswith("deg"):
        # the ray that misses the box: exactly 0 on both sides
        miss = (p["d_o"] == 0).all(dim=1) & (p["d_d"] == 0).all(dim=1)
        assert int(miss.sum()) >= 1
        assert bool((o64[miss] == 0).all()) and bool((d64[miss] == 0).all())


def test_autograd_agrees_with_central_differences():
    """a wrong definition would show here, independent of the reference: central differences (step 1e-6) of the float64
    restatement, on rays whose samples all stay strictly inside their cells under the step"""
    p = golden_inputs("deg2_full", CPU)
    samples = host_samples(p)
    z, inside, idx = samples
    spec, params = p["spec"], p["params"]
    # fraction of every sample inside its cell (float64), and the rays whose samples keep 1e-3 from every cell face
    o, d = p["ro"].double(), p["rd"].double()
    pts = o[:, None, :] + d[:, None, :] * z.double()[:, :, None]
    from voxe_hip.desc import norm_constants

    scale, bias = norm_constants(spec.aabb)
    ok = torch.ones(o.shape[0], dtype=torch.bool)
    for a in range(3):
        u = (((pts[..., a] * float(scale[a]) + float(bias[a])) + 1.0) * p["dens"].shape[a] - 1.0) * 0.5
        f = u - idx[..., a].double()
        lo = (pts[..., a] - spec.aabb[a][0]).abs()
        hi = (pts[..., a] - spec.aabb[a][1]).abs()
        ok &= ((f > 1e-3) & (f < 1.0 - 1e-3) & (lo > 1e-3) & (hi > 1e-3)).all(dim=1)
    rays = torch.nonzero(ok).reshape(-1)[:4]
    assert len(rays) == 4
    sub = dict(p, ro=p["ro"][rays], rd=p["rd"][rays], g_col=p["g_col"][rays], g_dep=p["g_dep"][rays], g_acc=p["g_acc"][rays])
    ssub = tuple(s[rays] for s in samples)
    d_o, d_d = restatement(sub, ssub)

    def loss(ro, rd):
        colour, depth, acc = RR.render_from_samples(*ssub, p["dens"], p["feat"], ro, rd, spec, params)
        return float((colour * sub["g_col"]).sum() + (depth * sub["g_dep"]).sum() + (acc * sub["g_acc"]).sum())

    h = 1e-6
    for which, grad in (("o", d_o), ("d", d_d)):
        for r in range(4):
            for a in range(3):
                vals = []
                for sgn in (1.0, -1.0):
                    ro, rd = sub["ro"].double().clone(), sub["rd"].double().clone()
                    (ro if which == "o" else rd)[r, a] += sgn * h
                    vals.append(loss(ro, rd))
                fd = (vals[0] - vals[1]) / (2 * h)
                assert abs(fd - float(grad[r, a])) <= 1e-6 * max(1.0, float(grad[r].abs().max())), (which, r, a, fd, float(grad[r, a]))


def test_cast_rays_backward_by_hand():
    """a 2 x 2 image, focal 2, one camera: dir_cam = ((x - 1) / 2, -(y - 1) / 2, -1) for x, y in {0.5, 1.5}"""
    rot = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    pose = torch.cat([rot, torch.tensor([[1.0], [2.0], [3.0]], dtype=torch.float64)], dim=1)[None].requires_grad_(True)
    focal = torch.tensor(2.0, dtype=torch.float64, requires_grad=True)
    ro, rd = RR.cast_rays(2, 2, focal, pose)
    dirs = torch.tensor([[-0.25, 0.25, -1.0], [0.25, 0.25, -1.0], [-0.25, -0.25, -1.0], [0.25, -0.25, -1.0]], dtype=torch.float64)
    assert torch.allclose(rd.detach(), dirs @ rot.T, atol=1e-15) and torch.equal(ro.detach(), pose.detach()[0, :, 3].expand(4, 3))
    g = torch.Generator().manual_seed(0)
    g_o, g_d = torch.randn(4, 3, generator=g, dtype=torch.float64), torch.randn(4, 3, generator=g, dtype=torch.float64)
    d_pose, d_focal = torch.autograd.grad((ro * g_o).sum() + (rd * g_d).sum(), (pose, focal))
    assert torch.allclose(d_pose[0, :, 3], g_o.sum(dim=0), atol=1e-14)                        # d_trans = sum d_o
    assert torch.allclose(d_pose[0, :, :3], g_d.T @ dirs, atol=1e-14)                          # d_rot[a][b] = sum d_d[a] dir_cam[b]
    ddirs = torch.cat([-dirs[:, :2] / 2.0, torch.zeros(4, 1, dtype=torch.float64)], dim=1)     # d dir_cam / d focal
    assert abs(float(d_focal) - float((g_d * (ddirs @ rot.T)).sum())) < 1e-14
    # the indexed form picks the same rays
    idx = torch.tensor([3, 0])
    ro2, rd2 = RR.cast_rays(2, 2, 2.0, pose.detach(), idx)
    assert torch.equal(rd2, rd.detach()[idx]) and torch.equal(ro2, ro.detach()[idx])


# ---- CameraPoseDeltas -------------------------------------------------------------------------------------------------
def test_camera_pose_deltas():
    from thre3d_atom.thre3d_reprs.poses import CameraPoseDeltas, axis_angle_to_matrix, rotation_error_degrees, translation_error

    g = torch.Generator().manual_seed(1)
    q, _ = torch.linalg.qr(torch.randn(5, 3, 3, generator=g))
    q = q * torch.linalg.det(q)[:, None, None]
    poses = torch.cat([q, torch.randn(5, 3, 1, generator=g)], dim=2)
    m = CameraPoseDeltas(5)
    assert tuple(m.deltas.shape) == (5, 6) and int(m.deltas.count_nonzero()) == 0
    assert torch.equal(m.apply(poses), poses)                                                  # identity at zero
    assert torch.equal(m.apply(poses[[3, 1]], torch.tensor([3, 1])), poses[[3, 1]])
    # finite, non-zero gradient at w = 0: d/dw of exp(w^) R at 0 is the generator
    out = m.apply(poses)
    (out * torch.randn(out.shape, generator=g)).sum().backward()
    assert bool(torch.isfinite(m.deltas.grad).all()) and float(m.deltas.grad[:, :3].abs().min()) > 0
    with torch.no_grad():
        m.deltas.copy_(torch.randn(5, 6, generator=g) * 0.5)
        m.deltas[0, :3] = 1e-6 * torch.tensor([1.0, -2.0, 0.5])                                 # the series branch
    out = m.apply(poses).detach()
    rot = out[:, :, :3].double()
    assert float((rot @ rot.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
    assert float((torch.linalg.det(rot) - 1.0).abs().max()) < 1e-6
    assert torch.allclose(out[:, :, 3], poses[:, :, 3] + m.deltas.detach()[:, 3:], atol=1e-7)
    # (camera 0's 1e-4 degrees are below what float32 rotation matrices resolve: acos near 1)
    angle = rotation_error_degrees(out, poses)
    assert torch.allclose(angle[1:], torch.rad2deg(m.deltas.detach()[1:, :3].norm(dim=1)).double(), atol=1e-3) and float(angle[0]) < 0.1
    assert torch.allclose(translation_error(out, poses), m.deltas.detach()[:, 3:].norm(dim=1).double(), atol=1e-6)
    # a known quarter turn about z composed on the left: x -> y
    quarter = axis_angle_to_matrix(torch.tensor([[0.0, 0.0, np.pi / 2]], dtype=torch.float64))[0]
    assert torch.allclose(quarter, torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64), atol=1e-15)
    one = CameraPoseDeltas(1)
    with torch.no_grad():
        one.deltas[0, 2] = np.pi / 2
    eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1)[None]
    assert torch.allclose(one.apply(eye)[0, :, 0], torch.tensor([0.0, 1.0, 0.0]), atol=1e-6)
    # the series and the closed form meet
    a = axis_angle_to_matrix(torch.tensor([[0.9e-4, 0.0, 0.0]], dtype=torch.float64))
    b = axis_angle_to_matrix(torch.tensor([[1.1e-4, 0.0, 0.0]], dtype=torch.float64))
    assert float((a - b).abs().max()) < 1e-4


def test_write_camera_params_round_trip(tmp_path):
    from PIL import Image

    from thre3d_atom.data.datasets import InMemoryPosedImages, PosedImagesDataset
    from thre3d_atom.thre3d_reprs.poses import write_camera_params
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

    g = torch.Generator().manual_seed(2)
    poses = torch.randn(3, 3, 4, generator=g)
    data = InMemoryPosedImages(torch.rand(3, 3, 6, 8, generator=g), poses, CameraIntrinsics(6, 8, 11.5), CameraBounds(1.0, 4.0))
    images = tmp_path / "images"
    images.mkdir()
    for i in range(3):
        Image.fromarray((data.images[i].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(images / f"{i:04d}.png")
    path = write_camera_params(tmp_path / "refined_train_camera_params.json", data, poses + 0.25)
    back = PosedImagesDataset(images, path)
    assert torch.allclose(back.poses, poses + 0.25, atol=1e-6) and back.camera_intrinsics == CameraIntrinsics(6, 8, 11.5)
    # ... and from a dataset that was read from disk: names and intrinsics are kept, the poses replaced
    path2 = write_camera_params(tmp_path / "again.json", back, poses - 1.0)
    again = PosedImagesDataset(images, path2)
    assert torch.allclose(again.poses, poses - 1.0, atol=1e-6) and set(again.camera_parameters) == set(back.camera_parameters)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


SYMBOLS = ("voxe_render_bwd_rays", "voxe_render_bwd_rays_debug_lanes", "voxe_cast_rays_bwd_scratch_bytes", "voxe_cast_rays_bwd")


def _proto_names(text, name):
    proto = re.search(rf"\b{name}\((.*?)\);", text, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    return [a.split()[-1].lstrip("*") for a in proto.split(",")]


def test_symbols_are_declared_with_no_cpu_twin_and_abi_13():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    L = _lib()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols() and hasattr(L, name)
    assert not re.search(r"\bvoxe_cpu_(render_bwd_rays|cast_rays_bwd)", text)
    assert not any("bwd_rays" in s or "cast_rays_bwd" in s for s in abi.cpu_symbols())
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text and L.voxe_abi_version() == 13
    assert "voxe_render_rays_bwd.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    assert _proto_names(text, "int voxe_render_bwd_rays") == ["grid", "cfg", "rays_o", "rays_d", "R", "jitter", "d_colour", "d_depth",
                                                              "d_acc", "d_rays_o", "d_rays_d", "accumulate", "stream"]
    assert _proto_names(text, "int voxe_cast_rays_bwd") == ["H", "W", "focal", "poses", "K", "flat_index", "B", "d_rays_o", "d_rays_d",
                                                            "d_poses", "d_focal", "accumulate", "scratch", "scratch_bytes", "stream"]
    assert len(L.voxe_render_bwd_rays.argtypes) == 13 and L.voxe_render_bwd_rays.argtypes[11] is ctypes.c_int32
    assert len(L.voxe_cast_rays_bwd.argtypes) == 15 and L.voxe_cast_rays_bwd.argtypes[2] is ctypes.c_float
    # the binding passes them in the prototype's order
    src = inspect.getsource(ops.render_bwd_rays)
    assert re.search(r"voxe_render_bwd_rays\(C\.byref\(g\), C\.byref\(c\), ptr\(ro\), ptr\(rd\), R, ptr\(jit\)", src)


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    g = make_grid_desc(16, 16, (8, 6, 5), 3, H.AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)
    c = make_render_cfg(32, 1.0, 4.0)

    def call(g_=g, c_=c, ro=P, rd=P, R=4, d_o=None, d_d=None):
        return L.voxe_render_bwd_rays(ctypes.byref(g_) if g_ else None, ctypes.byref(c_) if c_ else None, ro, rd, R, None, P, None, None,
                                      d_o, d_d, 0, None)

    assert call(g_=None) == abi.ERR_NULL_POINTER and call(c_=None) == abi.ERR_NULL_POINTER
    assert call(ro=None) == abi.ERR_NULL_POINTER and call(rd=None) == abi.ERR_NULL_POINTER
    g.densities = 0
    assert call(g) == abi.ERR_NULL_POINTER
    g.densities, g.features = 16, 0
    assert call(g) == abi.ERR_NULL_POINTER
    g.features = 16
    assert call(R=-1) == abi.ERR_BAD_SHAPE and call(R=1 << 31) == abi.ERR_BAD_SHAPE
    for dims in ((0, 6, 5), (8, -1, 5), (1300, 1300, 1300), (1 << 12, 1 << 12, 2), (2, 2, 1 << 24), (700, 700, 1100)):
        g.X, g.Y, g.Z = dims                                      # (the last: X Y Z < 2^31 <= X Y Z (F + 1))
        assert call(g) == abi.ERR_BAD_SHAPE, dims
    g.X, g.Y, g.Z = 8, 6, 5
    c.num_samples = 0
    assert call(c_=c) == abi.ERR_BAD_SHAPE
    c.num_samples = 32
    g.density_post_act = 9
    assert call(g) == abi.ERR_UNSUPPORTED
    g.density_post_act = abi.ACT_RELU
    # F == 3 (deg + 1)^2
    c.sh_degree = 1
    assert call(c_=c) == abi.ERR_BAD_SHAPE
    g.F = 12
    assert call(g, c) == abi.OK
    c.sh_degree = 4
    assert call(c_=c) == abi.ERR_UNSUPPORTED
    c.sh_degree, g.F = 0, 3
    g.feature_kind, g.F = abi.FEAT_ATTN, 1
    assert call(g) == abi.ERR_UNSUPPORTED
    g.feature_kind, g.F = abi.FEAT_SH, 3
    # no launch: R == 0 (NULL rays allowed) or both outputs NULL
    assert call(ro=None, rd=None, R=0, d_o=P, d_d=P) == abi.OK and call() == abi.OK
    for lanes in (1, 2, 4, 8, 0):
        assert L.voxe_render_bwd_rays_debug_lanes(lanes) == abi.OK
    assert L.voxe_render_bwd_rays_debug_lanes(3) == abi.ERR_BAD_SHAPE and L.voxe_render_bwd_rays_debug_lanes(16) == abi.ERR_BAD_SHAPE

    need = L.voxe_cast_rays_bwd_scratch_bytes(3)
    assert need >= 3 * 13 * 8 and L.voxe_cast_rays_bwd_scratch_bytes(1000) >= 1000 * 13 * 8

    def cast(H_=4, W=5, focal=3.0, poses=P, K=3, idx=P, B=7, d_poses=P, sc=P, nbytes=need):
        return L.voxe_cast_rays_bwd(H_, W, focal, poses, K, idx, B, P, P, d_poses, None, 0, sc, nbytes, None)

    assert cast(H_=0) == abi.ERR_BAD_SHAPE and cast(W=-1) == abi.ERR_BAD_SHAPE and cast(K=0) == abi.ERR_BAD_SHAPE
    assert cast(B=-1) == abi.ERR_BAD_SHAPE and cast(focal=0.0) == abi.ERR_BAD_SHAPE
    assert cast(idx=None, B=59) == abi.ERR_BAD_SHAPE                      # whole images: B == K H W
    assert cast(poses=None) == abi.ERR_NULL_POINTER and cast(d_poses=None) == abi.ERR_NULL_POINTER
    assert cast(sc=None) == abi.ERR_WORKSPACE and cast(nbytes=need - 1) == abi.ERR_WORKSPACE


def test_operators_refuse_host_tensors():
    from voxe_hip.runtime import VoxeError

    spec = ops.GridSpec(aabb=H.AABB)
    params = ops.RenderParams(num_samples=8, near=1.0, far=4.0)
    z = torch.zeros(2, 3)
    with pytest.raises(VoxeError):
        ops.render_bwd_rays(spec, params, torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), z, z, None, (0, 0), z, None, None)
    with pytest.raises(VoxeError):
        ops.cast_rays_from_poses(4, 4, 5.0, torch.zeros(1, 3, 4))
    with pytest.raises(VoxeError):
        ops.cast_rays_bwd(4, 4, 5.0, torch.zeros(1, 3, 4), None, None, None)


# ---- pose recovery on the restatement ---------------------------------------------------------------------------------
def test_pose_recovery_on_the_restatement():
    """the scene of the GPU test, optimised with the restatement's gradients (float64, the oracle's samples): the reference's own
    autograd on these inputs goes 3.4e-2 -> 2.3e-5 in loss, 3.0 -> 1.06 / 0.98 / 0.24 degrees, 0.080 -> 0.064 / 0.046 / 0.017"""
    from thre3d_atom.thre3d_reprs.poses import CameraPoseDeltas, rotation_error_degrees, translation_error

    spec, params, dens, feat = pose_scene(CPU)
    true, noisy, focal = pose_cameras(CPU)
    per = POSE_HW * POSE_HW

    def render(poses):
        ro, rd = RR.cast_rays(POSE_HW, POSE_HW, focal, poses)
        samples = RR.probe_host(spec, params, dens, feat, ro, rd)
        return RR.render_from_samples(*samples, dens, feat, ro, rd, spec, params)[0]

    with torch.no_grad():
        target = render(true)
    deltas = CameraPoseDeltas(3).double()
    opt = torch.optim.Adam(deltas.parameters(), lr=POSE_LR)
    losses = []
    for _ in range(POSE_STEPS + 1):
        opt.zero_grad()
        colour = render(deltas.apply(noisy.double()))
        loss = ((colour - target) ** 2).reshape(3, per, 3).mean(dim=(1, 2)).sum()
        losses.append(float(loss.detach()))
        if len(losses) <= POSE_STEPS:
            loss.backward()
            opt.step()
    final = deltas.apply(noisy.double()).detach()
    assert_pose_recovery(losses, rotation_error_degrees(noisy, true), rotation_error_degrees(final, true),
                         translation_error(noisy, true), translation_error(final, true))


# ---- the inputs of the GPU agreement test are not vacuous (oracle probe -> restatement, no device) ---------------------
NEGLIGIBLE = 1e-100


def blind_rays(d_o, d_d):
    """rays that see nothing, per the float64 restatement: (gradient exactly 0, gradient below 1e-100)"""
    mag = d_o.abs().sum(dim=1) + d_d.abs().sum(dim=1)
    return mag == 0, mag < NEGLIGIBLE


def assert_agreement_not_vacuous(case, post, d_o, d_d):
    """both gradients are non-zero and, in the image cases, some rays see nothing.  Under abs + ReLU those rays' gradient is
    exactly 0 in the restatement.  Under identity + Softplus it cannot be, by definition: no ray of these frusta misses the box,
    and where an empty ray crosses the grid's outer faces the zero padding blends the empty raw value (-800 after scaling)
    towards 0, which leaves softplus'(v) = e^v at 1e-260 or so in float64 (0 in float32).  That pair is held to what it can
    meet: rays whose float64 gradient is below 1e-100 -- on which the kernel must still return exact zeros."""
    assert float(d_o.norm()) > 0 and float(d_d.norm()) > 0
    if case[8] is None:
        exact, negligible = blind_rays(d_o, d_d)
        assert int((negligible if post == abi.ACT_SOFTPLUS else exact).sum()) >= 1


@pytest.mark.parametrize("pre,post", TD.ACTS)
@pytest.mark.parametrize("case", TD.agreement_cases(), ids=lambda c: c[0])
def test_agreement_inputs_are_not_vacuous(case, pre, post):
    p = agreement_inputs(case, 0, pre, post, CPU)
    d_o, d_d = restatement(p, host_samples(p))
    print(f"{case[0]}: R {len(d_o)}  |d_o| {float(d_o.norm()):.4g}  |d_d| {float(d_d.norm()):.4g}  rays with an exact 0: "
          f"{int(((d_o == 0).all(dim=1) & (d_d == 0).all(dim=1)).sum())}")
    assert_agreement_not_vacuous(case, post, d_o, d_d)


# ---- entry points and documents ---------------------------------------------------------------------------------------
def _cli(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_ray_grad_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_options_trainer_argument_and_documents():
    train = {p.name: p for p in _cli("train_sh_based_voxel_grid_with_posed_images.py").main.params}
    assert train["pose_learning_rate"].default == 0.0 and "--pose_learning_rate" in train["pose_learning_rate"].opts
    refine = {p.name: p for p in _cli("refine_camera_poses.py").main.params}
    assert refine["model_path"].required and refine["data_path"].required and refine["output_path"].required
    assert "-i" in refine["model_path"].opts and "-d" in refine["data_path"].opts and "-o" in refine["output_path"].opts
    assert refine["num_iterations"].default == 200 and refine["learning_rate"].default == 3e-3
    assert refine["ray_batch_size"].default == 32768 and refine["split"].default == "train"
    from thre3d_atom.modules import pose_refiner, trainers

    sig = inspect.signature(trainers.train_sh_vox_grid_vol_mod_with_posed_images)
    assert sig.parameters["pose_learning_rate"].default == 0.0
    assert callable(pose_refiner.refine_camera_poses) and callable(ops.cast_rays_from_poses) and callable(ops.render_bwd_rays)
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "--pose_learning_rate" in text and "refine_camera_poses.py" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.13" in design and "voxe_render_bwd_rays" in design
    assert "ray_grad_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "ray_grads.npz" in design and "g19_ray_grads" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_pose_learning_rate_zero_leaves_the_one_call_iteration(tmp_path, monkeypatch):
    """pose_learning_rate = 0 takes the trainer's code path as it was: the one-call iteration runs (voxe_recon_step through
    FusedGridAdam.reconstruction_step), no pose deltas exist and no refined cameras are written; above 0 the iteration casts
    differentiable rays, renders and steps separately, and the refined cameras are saved next to the checkpoints"""
    from thre3d_atom.modules import trainers
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

    calls = {"one_call": 0, "render": 0, "differentiable": 0, "plain": 0}

    class FakeOpt(torch.optim.Optimizer):
        def __init__(self, grid, lr, betas):
            super().__init__(list(grid.parameters()), dict(lr=lr))

        def reconstruction_step(self, *a, **k):
            calls["one_call"] += 1

        def reconstruction_prefetch(self, *a, **k):
            pass

        def detach(self):
            pass

        def step(self, closure=None):
            pass

    class Data:
        def __init__(self):
            self.images = torch.rand(4, 3, 8, 8)
            self.poses = torch.eye(4)[None, :3].repeat(4, 1, 1)
            self.camera_intrinsics = CameraIntrinsics(8, 8, 10.0)
            self.camera_bounds = CameraBounds(1.0, 4.0)

        def downsampled(self, f):
            return self

        def to(self, device):
            return self

        def __len__(self):
            return 4

        def get_hemispherical_radius_estimate(self):
            return 4.0

    def fake_render_rays(self, rays, **kw):
        calls["render"] += 1
        return type("Out", (), {"colour": self.thre3d_repr.features.sum() * 0 + rays.origins.sum() * 0 + torch.zeros(16, 3)})()

    def fake_sample(intr, poses, images, n, differentiable=False, **k):
        calls["differentiable" if differentiable else "plain"] += 1
        assert poses.requires_grad == differentiable
        return type("R", (), {"origins": poses[:, :, 3].sum() * 0 + torch.zeros(16, 3)})(), torch.zeros(16, 3)

    monkeypatch.setattr(trainers, "FusedGridAdam", FakeOpt)
    monkeypatch.setattr(trainers, "scale_voxel_grid_with_required_output_size", lambda grid, size: grid)
    monkeypatch.setattr(trainers, "_render_params", lambda *a, **k: None)
    monkeypatch.setattr(trainers, "_next_rng", lambda: (0, 0))
    monkeypatch.setattr(VolumetricModel, "render_rays", fake_render_rays)
    monkeypatch.setattr(trainers, "sample_random_rays_and_pixels_from_cameras", fake_sample)
    for rate, want in ((0.0, {"one_call": 3, "render": 0, "differentiable": 0, "plain": 0}),
                       (1e-3, {"one_call": 0, "render": 6, "differentiable": 3, "plain": 0})):
        for k in calls:
            calls[k] = 0
        vg = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.1, 0.1, 0.1), tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(8, CameraBounds(1.0, 4.0)), device=CPU)
        out = tmp_path / f"rate_{rate}"
        trainers.train_sh_vox_grid_vol_mod_with_posed_images(vm, Data(), out, num_stages=1, num_iterations_per_stage=3,
                                                             fast_debug_mode=True, pose_learning_rate=rate)
        assert calls == want, (rate, calls)
        assert (out / "saved_models" / "refined_train_camera_params.json").exists() == (rate > 0)
