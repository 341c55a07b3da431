"""CPU checks of the distortion loss on rays: the C ABI's declarations and argument validation (no device work), self-checks of
the float64 restatement tests/distortion_ref.py (a hand-computed ray, the O(S) prefix form, the kernel's lane-split evaluation,
finite differences), the trainer's option, and -- with the oracle's sample probe feeding the restatement -- that the inputs of
the GPU tests (tests/test_distortion_gpu.py builds them with the functions below) are not vacuous."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import distortion_ref as DR
import test_visibility_host as H
from conftest import ROOT
from voxe_hip import abi, ops, workload
from voxe_hip.desc import make_grid_desc, make_render_cfg

CPU = torch.device("cpu")
ACTS = H.ACTS
# the voxels that carry density in the agreement inputs: a central box of the visibility tests' grid; everything else is EMPTY
BOX = ((6, 20), (4, 16), (5, 18))


# ---- inputs shared with the GPU tests ---------------------------------------------------------------------------------
def empty_raw(pre, post):
    """a raw density whose sigma is exactly 0 in float64 and in the kernel: 0 under abs + ReLU; under identity + Softplus
    softplus(2 * -400) = log1p(exp(-800)) = 0 (exp underflows in both precisions)"""
    return -400.0 if post == abi.ACT_SOFTPLUS else 0.0


def carve(dens, pre, post):
    """the visibility tests' random densities inside BOX, empty outside: border rays of every camera see nothing (L_r == 0
    exactly), central rays cross random density"""
    out = torch.full_like(dens, empty_raw(pre, post))
    (x0, x1), (y0, y1), (z0, z1) = BOX
    out[x0:x1, y0:y1, z0:z1] = dens[x0:x1, y0:y1, z0:z1]
    return out


def agreement_cases():
    """the four image cases of the visibility tests, then R in {1, 63, 65} linear rays and S in {1, 2, 37} (blocks over the G
    lanes uneven, some empty): (name, hw, views, perturb, jitter kind, aabb_clip, lindisp, order, R or None, S)"""
    cases = [c + (None, 96) for c in H.agreement_cases()]
    for R in (1, 63, 65):
        cases.append((f"linear_R{R}", 48, 1, True, None, False, False, "linear", R, 96))
    for S in (1, 2, 37):
        cases.append((f"linear_S{S}", 48, 1, True, None, False, False, "linear", 200, S))
    return cases


def agreement_inputs(case, pre, post, device):
    """(spec, params, densities, features, rays_o, rays_d, jitter, rng) of one agreement case"""
    name, hw, views, perturb, jkind, clip, lindisp, order, R, S = case
    if order != "linear":
        spec, params, dens, feat, ro, rd, jitter, rng = H.agreement_inputs(case[:8], pre, post, device)
        return spec, params, carve(dens, pre, post), feat, ro, rd, jitter, rng
    spec, _, dens, feat, ro, rd, _, _ = H.agreement_inputs(("plain", hw, 1, False, None, False, False, "image"), pre, post, device)
    # R rays spread over the lower three quarters of the image (the centre that hits the box, and the corners of the last rows
    # that miss it); R == 1: the centre pixel
    pick = torch.tensor([hw * (hw // 2) + hw // 2]) if R == 1 else torch.linspace(hw * hw // 4, hw * hw - 1, R).round().long()
    ro, rd = ro[pick.to(device)].contiguous(), rd[pick.to(device)].contiguous()
    # (the S sweep samples [3, 5] only: with the workload's [2, 6] the two samples of S = 2 both fall inside the box on one ray
    #  in six, and nearly every L_r would be 0)
    near, far = (workload.NEAR, workload.FAR) if S == 96 else (3.0, 5.0)
    params = ops.RenderParams(num_samples=S, near=near, far=far, perturb=perturb, linear_disparity=lindisp, aabb_clip=clip)
    return spec, params, carve(dens, pre, post), feat, ro, rd, None, (4321, 5)


def assert_agreement_not_vacuous(case, L, grad):
    """the three conditions on the float64 restatement's per-ray loss and gradient.  Two of the edge cases cannot meet all of
    them BY DEFINITION, and are held to what they can: a single ray (R == 1) cannot both weigh and be empty -- it must weigh --
    and crosses at most ~20 cells of the 14-voxel-wide box, whose footprints hold fewer than 100 voxels (30 are asked for);
    a single sample (S == 1) has d_0 = 0 and one m, so L_r = 0 and the gradient vanishes for every ray -- the case checks that
    the kernel says exactly that."""
    R, S = case[8], case[9]
    if S == 1:
        assert float(L.abs().max()) == 0.0 and int((grad != 0).sum()) == 0
        return
    assert float((L > 1e-4).double().mean()) >= 0.25
    assert int((grad != 0).sum()) > (30 if R == 1 else 100)
    if R != 1:
        assert int((L == 0).sum()) >= 1


# The descent fixture: the floater.  A dense ball (softplus field, raw 10 at scale 2: sigma 20) and, between the cameras and
# the ball, a faint shell of raw -0.5 (sigma 0.31) around it; everything else is empty (raw -6: sigma 6e-6).  30 Adam steps of
# FLOATER_LR move no voxel by more than 0.9, i.e. 9 % of the ball's raw density.
FLOATER_LR, FLOATER_STEPS = 0.03, 30
FLOATER_DIMS = (32, 32, 32)
FLOATER_AABB = ((-1.5, 1.5),) * 3
FLOATER_BALL, FLOATER_SHELL = 0.45, (0.9, 1.2)


def floater_field():
    """(densities [X,Y,Z,1], ball mask [X,Y,Z], shell mask [X,Y,Z])"""
    n = FLOATER_DIMS[0]
    ax = (torch.arange(n, dtype=torch.float32) + 0.5) / n * 3.0 - 1.5
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    ball, shell = r < FLOATER_BALL, (r > FLOATER_SHELL[0]) & (r < FLOATER_SHELL[1])
    dens = torch.full((n, n, n), -6.0)
    dens[shell] = -0.5
    dens[ball] = 10.0
    return dens[..., None].contiguous(), ball, shell


def floater_inputs(device):
    """(spec, params, densities, features, rays_o, rays_d, ball, shell): 2 cameras at 24 x 24, S = 64, no jitter"""
    dens, ball, shell = floater_field()
    spec = ops.GridSpec(aabb=FLOATER_AABB, density_scale=2.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS)
    ro, rd = H.cameras(24, 2, device)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, image_width=24, image_height=24)
    feat = torch.zeros((*FLOATER_DIMS, 3))
    return spec, params, dens.to(device), feat.to(device), ro, rd, ball.to(device), shell.to(device)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


def test_distortion_symbols_are_declared_with_no_cpu_twin_and_abi_13():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    for name in ("voxe_distortion_scratch_bytes", "voxe_distortion_fwd_bwd", "voxe_distortion_debug_lanes"):
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols()
    assert not re.search(r"\bvoxe_cpu_\w*distortion", text)
    assert not any("distortion" in s for s in abi.cpu_symbols())
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text
    L = _lib()
    assert L.voxe_abi_version() == 13
    assert hasattr(L, "voxe_distortion_fwd_bwd") and hasattr(L, "voxe_distortion_scratch_bytes")
    assert "voxe_distortion.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    # the header's prototype has the arguments the binding passes, in order
    proto = re.search(r"int voxe_distortion_fwd_bwd\((.*?)\);", text, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    names = [a.split()[-1].lstrip("*") for a in proto.split(",")]
    assert names == ["grid", "cfg", "rays_o", "rays_d", "R", "jitter", "grad_scale", "loss_out", "ray_loss", "d_densities",
                     "accumulate", "scratch", "scratch_bytes", "stream"]
    assert len(L.voxe_distortion_fwd_bwd.argtypes) == len(names)
    assert L.voxe_distortion_fwd_bwd.argtypes[6] is ctypes.c_float and L.voxe_distortion_fwd_bwd.argtypes[10] is ctypes.c_int32


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    g = make_grid_desc(16, 0, (8, 6, 5), 3, H.AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)   # features NULL: not read
    c = make_render_cfg(32, 1.0, 4.0)
    need = L.voxe_distortion_scratch_bytes(4)
    assert need >= 8 * 4 and L.voxe_distortion_scratch_bytes(1 << 20) >= 8 << 20

    def call(g_=g, c_=c, ro=P, rd=P, R=4, loss=None, ray=None, d=None, acc=1, sc=P, nbytes=need):
        return L.voxe_distortion_fwd_bwd(ctypes.byref(g_) if g_ else None, ctypes.byref(c_) if c_ else None, ro, rd, R, None, 1.0,
                                         loss, ray, d, acc, sc, nbytes, None)

    assert call(g_=None) == abi.ERR_NULL_POINTER and call(c_=None) == abi.ERR_NULL_POINTER
    assert call(ro=None) == abi.ERR_NULL_POINTER and call(rd=None) == abi.ERR_NULL_POINTER
    g.densities = 0
    assert call(g) == abi.ERR_NULL_POINTER
    g.densities = 16
    assert call(R=-1) == abi.ERR_BAD_SHAPE and call(R=1 << 31) == abi.ERR_BAD_SHAPE
    for dims in ((0, 6, 5), (8, -1, 5), (1300, 1300, 1300), (1 << 12, 1 << 12, 2), (2, 2, 1 << 24)):
        g.X, g.Y, g.Z = dims
        assert call(g) == abi.ERR_BAD_SHAPE, dims
    g.X, g.Y, g.Z = 8, 6, 5
    c.num_samples = 0
    assert call(c_=c) == abi.ERR_BAD_SHAPE
    c.num_samples = 32
    g.density_post_act = 9
    assert call(g) == abi.ERR_UNSUPPORTED
    g.density_post_act, g.density_pre_act = abi.ACT_RELU, 5
    assert call(g) == abi.ERR_UNSUPPORTED
    g.density_pre_act = abi.ACT_ABS
    # the loss needs the scratch
    assert call(loss=P, sc=None) == abi.ERR_WORKSPACE and call(loss=P, nbytes=need - 1) == abi.ERR_WORKSPACE
    # no launch: R == 0 (NULL rays allowed), or all three outputs NULL (accumulate != 0: d_densities is not touched either)
    assert call(ro=None, rd=None, R=0, loss=P, ray=P, d=P) == abi.OK and call(ro=None, rd=None, R=0) == abi.OK
    assert call() == abi.OK and call(sc=None, nbytes=0) == abi.OK
    # feature kind / F are not read
    g.feature_kind, g.F = 7, 0
    assert call() == abi.OK
    for lanes in (1, 2, 4, 8, 0):
        assert L.voxe_distortion_debug_lanes(lanes) == abi.OK
    assert L.voxe_distortion_debug_lanes(3) == abi.ERR_BAD_SHAPE and L.voxe_distortion_debug_lanes(16) == abi.ERR_BAD_SHAPE


def test_operator_refuses_host_tensors():
    from voxe_hip.runtime import VoxeError

    spec = ops.GridSpec(aabb=H.AABB)
    params = ops.RenderParams(num_samples=8, near=1.0, far=4.0)
    with pytest.raises(VoxeError):
        ops.distortion_loss(spec, params, torch.zeros(4, 4, 4, 1), torch.zeros(2, 3), torch.zeros(2, 3))


# ---- the restatement checks itself ------------------------------------------------------------------------------------
def test_two_point_masses_by_hand():
    """S = 4 samples at z = 2, 3, 4, 6 on [near, far] = [2, 6], weights only on samples 1 and 2"""
    z = torch.tensor([[2.0, 3.0, 4.0, 6.0]])
    m, d = DR.intervals(z, 2.0, 6.0)
    assert torch.allclose(d, torch.tensor([[0.25, 0.25, 0.5, 0.0]], dtype=torch.float64), atol=1e-15)
    assert torch.allclose(m, torch.tensor([[0.125, 0.375, 0.75, 1.0]], dtype=torch.float64), atol=1e-15)
    w1, w2 = 0.3, 0.45
    w = torch.tensor([[0.0, w1, w2, 0.0]], dtype=torch.float64)
    want = 2 * w1 * w2 * abs(0.375 - 0.75) + (w1 * w1 * 0.25 + w2 * w2 * 0.5) / 3.0
    assert abs(float(DR.pair_sum(w, m, d)) - want) < 1e-15
    # ... and through weights(): sigma picked so that alpha_1 = 0.3 and alpha_2 T_2 = 0.45 for a unit direction
    a1, a2 = w1, w2 / (1 - w1)
    sigma = torch.tensor([[0.0, -np.log(1 - a1) / 1.0, -np.log(1 - a2) / 2.0, 0.0]], dtype=torch.float64)
    got = DR.weights(sigma, z, torch.tensor([[0.0, 0.0, 1.0]]))
    assert torch.allclose(got, w, atol=1e-15)


def _random_ray(S, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.sort(torch.rand(1, S, generator=g) * 4.0 + 2.0, dim=1).values
    x = torch.rand(S, generator=g, dtype=torch.float64) * (torch.rand(S, generator=g) < 0.7) * 0.4   # optical depths, some 0
    m, d = DR.intervals(z, 2.0, 6.0)
    return x, m[0], d[0]


@pytest.mark.parametrize("S", [1, 2, 37, 96])
def test_prefix_and_lane_split_forms_equal_the_double_sum(S):
    """the O(S) prefix evaluation and the kernel's G-lane evaluation (local marches + scans + the closed-form prefix of
    sum g w, in float64) give the O(S^2) sum to 1e-12, and the lane-split q_k = dL/dx_k equals autograd's"""
    x, m, d = _random_ray(S, 11 + S)
    x.requires_grad_(True)
    alpha = 1.0 - torch.exp(-x)
    T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1.0 - alpha[:-1]]), dim=0)
    w = (alpha * T)[None]
    L = DR.pair_sum(w, m[None], d[None])[0]
    assert abs(float(DR.prefix_sum(w, m[None], d[None])[0].detach()) - float(L.detach())) < 1e-12
    (q_ref,) = torch.autograd.grad(L, x)
    for G in (1, 2, 4, 8):
        Lg, q = DR.lane_split(x.detach(), m, d, G)
        assert abs(Lg - float(L.detach())) < 1e-12, G
        assert float((q - q_ref).abs().max()) < 1e-12, G
    assert S == 1 or float(L.detach()) > 1e-3


def test_autograd_gradient_against_central_differences():
    case = agreement_cases()[0]
    pre, post = ACTS[0]
    spec, params, dens, feat, ro, rd, jitter, rng = agreement_inputs(case, pre, post, CPU)
    keep = torch.linspace(0, ro.shape[0] - 1, 300).round().long()       # 300 rays of the image are enough
    ro, rd = ro[keep].contiguous(), rd[keep].contiguous()
    params = ops.RenderParams(num_samples=params.num_samples, near=params.near, far=params.far)
    dens = dens.double()
    # (the restatement takes float64 densities as they are: finite differences need the resolution)
    d0 = dens.clone().requires_grad_(True)
    L = DR.distortion_host(spec, params, d0, feat, ro, rd).mean()
    (g,) = torch.autograd.grad(L, d0)
    nz = torch.nonzero(g.reshape(-1).abs() > 0.05 * g.abs().max()).reshape(-1)
    pick = nz[torch.randperm(len(nz), generator=torch.Generator().manual_seed(0))[:20]]
    assert len(pick) == 20
    from oracle import voxe_oracle as vo

    grid = vo.Grid(dens.float().numpy(), feat.numpy(), spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act)
    cfg = make_render_cfg(params.num_samples, params.near, params.far)
    probe = vo.sample_probe(grid, cfg, ro.numpy(), rd.numpy(), None)
    z, inside = torch.from_numpy(probe["z"]), torch.from_numpy(probe["inside"])
    h = 1e-4
    for i in pick.tolist():
        vals = []
        for sgn in (1.0, -1.0):
            dd = dens.clone()
            dd.view(-1)[i] += sgn * h
            vals.append(float(DR.from_samples(z, inside, dd, ro, rd, spec, params.near, params.far).mean()))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - float(g.view(-1)[i])) <= 1e-6 * abs(float(g.view(-1)[i])), (i, fd, float(g.view(-1)[i]))


# ---- the inputs are not vacuous (oracle probe -> restatement, no device) ----------------------------------------------
@pytest.mark.parametrize("pre,post", ACTS)
@pytest.mark.parametrize("case", agreement_cases(), ids=lambda c: c[0])
def test_agreement_inputs_are_not_vacuous(case, pre, post):
    spec, params, dens, feat, ro, rd, jitter, rng = agreement_inputs(case, pre, post, CPU)
    L, grad = DR.loss_and_gradient(DR.distortion_host, spec, params, dens, feat, ro, rd, jitter, rng)
    print(f"{case[0]}: R {len(L)}  L_r > 1e-4: {float((L > 1e-4).double().mean()):.3f}  L_r == 0: {int((L == 0).sum())}  "
          f"grad != 0: {int((grad != 0).sum())}  loss {float(L.mean()):.6f}")
    assert_agreement_not_vacuous(case, L, grad)


def test_floater_fixture_descends_in_the_restatement():
    """the fixture of the GPU descent test behaves as that test expects, in float64 on the host: a small plain step lowers
    the loss, the gradient sits on the shell and the ball's side facing the cameras, and the ball outweighs nothing"""
    spec, params, dens, feat, ro, rd, ball, shell = floater_inputs(CPU)
    L, grad = DR.loss_and_gradient(DR.distortion_host, spec, params, dens, feat, ro, rd)
    loss0 = float(L.mean())
    assert loss0 > 1e-3 and float((L > 1e-4).double().mean()) > 0.25
    eta = 0.05 * loss0 / float((grad * grad).sum())         # first order: lowers the loss by 5 %
    stepped = (dens.double() - eta * grad).float()
    loss1 = float(DR.distortion_host(spec, params, stepped, feat, ro, rd).mean())
    print(f"floater: loss {loss0:.6f} -> {loss1:.6f} after one step of eta {eta:.3g}")
    assert loss1 < loss0
    assert float(grad[shell].abs().sum()) > 0.0
    # ... and FLOATER_STEPS Adam steps on the term alone more than halve it while the ball keeps its peak within 10 %
    d = dens.clone().requires_grad_(True)
    opt = torch.optim.Adam([d], lr=FLOATER_LR)
    for _ in range(FLOATER_STEPS):
        opt.zero_grad()
        DR.distortion_host(spec, params, d, feat, ro, rd).mean().backward()
        opt.step()
    loss30 = float(DR.distortion_host(spec, params, d.detach(), feat, ro, rd).mean())
    peak0, peak30 = float(dens[ball].max()), float(d.detach()[ball].max())
    print(f"floater: loss {loss0:.6f} -> {loss30:.6f} after {FLOATER_STEPS} Adam steps; ball peak {peak0:.3f} -> {peak30:.3f}")
    assert loss30 < 0.5 * loss0 and abs(peak30 - peak0) <= 0.1 * peak0


# ---- trainer option ---------------------------------------------------------------------------------------------------
def test_cli_option_and_trainer_argument():
    spec = importlib.util.spec_from_file_location("train_dist_cli", os.path.join(ROOT, "train_sh_based_voxel_grid_with_posed_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opt = {p.name: p for p in mod.main.params}["distortion_weight"]
    assert opt.default == 0.0 and "--distortion_weight" in opt.opts
    from thre3d_atom.modules import trainers

    sig = inspect.signature(trainers.train_sh_vox_grid_vol_mod_with_posed_images)
    assert sig.parameters["distortion_weight"].default == 0.0
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.distortion import distortion_loss_on_rays

    assert callable(distortion_loss_on_rays) and callable(VolumetricModel.distortion_loss)
    for doc in ("README.md", "INTEGRATION.md"):
        assert "--distortion_weight" in open(os.path.join(ROOT, doc)).read(), doc
    assert "4.11" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_weight_zero_leaves_the_one_call_iteration(tmp_path, monkeypatch):
    """distortion_weight = 0 takes the trainer's code path as it was: the one-call iteration runs (voxe_recon_step through
    FusedGridAdam.reconstruction_step) and the distortion term is never evaluated; above 0 it is the other way round"""
    from thre3d_atom.modules import trainers
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

    calls = {"one_call": 0, "distortion": 0, "render": 0}

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
        return type("Out", (), {"colour": self.thre3d_repr.features.sum() * 0 + torch.zeros(rays.origins.shape[0], 3)})()

    def fake_distortion(self, rays, **kw):
        calls["distortion"] += 1
        return self.thre3d_repr.densities.sum() * 0

    monkeypatch.setattr(trainers, "FusedGridAdam", FakeOpt)
    monkeypatch.setattr(trainers, "scale_voxel_grid_with_required_output_size", lambda grid, size: grid)
    monkeypatch.setattr(trainers, "_render_params", lambda *a, **k: None)
    monkeypatch.setattr(trainers, "_next_rng", lambda: (0, 0))
    monkeypatch.setattr(VolumetricModel, "render_rays", fake_render_rays)
    monkeypatch.setattr(VolumetricModel, "distortion_loss", fake_distortion)
    monkeypatch.setattr(trainers, "sample_random_rays_and_pixels_from_cameras",
                        lambda intr, poses, images, n, **k: (type("R", (), {"origins": torch.zeros(16, 3)})(), torch.zeros(16, 3)))
    for weight, want in ((0.0, {"one_call": 3, "distortion": 0, "render": 0}), (0.01, {"one_call": 0, "distortion": 3, "render": 6})):
        for k in calls:
            calls[k] = 0
        vg = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.1, 0.1, 0.1), tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(8, CameraBounds(1.0, 4.0)), device=CPU)
        trainers.train_sh_vox_grid_vol_mod_with_posed_images(vm, Data(), tmp_path, num_stages=1, num_iterations_per_stage=3,
                                                             fast_debug_mode=True, distortion_weight=weight)
        assert calls == want, (weight, calls)
