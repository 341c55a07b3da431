"""CPU checks of the depth supervision (the ray-termination loss towards sparse structure-from-motion points): the C ABI's
declarations and argument validation (no device work), self-checks of the float64 restatement tests/depth_ref.py (the kernel's
lane-split evaluation, the closed-form gradient, the tail behind an opaque wall), the targets on rays, the importer's sparse-point
sidecar and the dataset that carries it, the trainer's options, and -- with the oracle's sample probe feeding the restatement --
that the inputs of the GPU tests (tests/test_depth_gpu.py builds them with the functions below) are not vacuous."""
import ctypes
import importlib.util
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import depth_ref as PR
import test_distortion_host as T
import test_visibility_host as H
from conftest import ROOT
from voxe_hip import abi, ops, workload
from voxe_hip.desc import make_grid_desc, make_render_cfg

CPU = torch.device("cpu")
ACTS = T.ACTS
# an opaque wall inside test_distortion_host.BOX (raw 400: sigma 800, T reaches 0 within three samples): targets behind it
WALL = ((11, 15), (8, 12), (9, 14))
WALL_RAW = 400.0


# ---- inputs shared with the GPU tests ---------------------------------------------------------------------------------
def agreement_cases():
    """test_distortion_host's: plain 48 x 48, hash jitter + aabb_clip 40 x 40, linear_disparity over 3 views of 24 x 24, shuffled
    rays with caller jitter, R in {1, 63, 65} and S in {1, 2, 37}"""
    return T.agreement_cases()


def _box_world():
    lo, hi = [], []
    for (a, b), n, (i0, i1) in zip(H.AABB, H.DIMS, T.BOX):
        lo.append(a + (b - a) * i0 / n)
        hi.append(a + (b - a) * i1 / n)
    return torch.tensor(lo, dtype=torch.float64), torch.tensor(hi, dtype=torch.float64)


def targets(params, rays_o, rays_d):
    """(D, s, omega) [R] float32 on the host.  By ray index r: r % 5 picks the target -- 0 on the surface of the dense box,
    1 in the empty space 0.6 in front of it, 2 behind it (behind the opaque wall for the rays that cross it), 3 behind `far`
    (narrow: every c_k underflows to exactly 0, also in float64), 4 in front of `near`; s runs from one nominal sample spacing
    (far - near) / S to ten; omega is 0 for r % 6 == 5, else 0.5 .. 2.  A single ray takes the first kind with omega 1."""
    o, d = rays_o.cpu().double(), rays_d.cpu().double()
    R = o.shape[0]
    lo, hi = _box_world()
    inv = 1.0 / d
    ta, tb = (lo - o) * inv, (hi - o) * inv
    t0, t1 = torch.minimum(ta, tb).amax(dim=1), torch.maximum(ta, tb).amin(dim=1)
    closest = -(o * d).sum(dim=1) / (d * d).sum(dim=1)
    hit = t0 < t1
    t0, t1 = torch.where(hit, t0, closest), torch.where(hit, t1, closest)
    r = torch.arange(R)
    kind = r % 5 if R > 1 else torch.zeros(1, dtype=torch.long)
    spacing = (params.far - params.near) / params.num_samples
    D = torch.stack([t0 + 0.05, t0 - 0.6, t1 + 0.3, torch.full_like(t0, params.far + 2.5), torch.full_like(t0, params.near - 0.3)])
    D = D.gather(0, kind[None])[0]
    s = spacing * (1.0 + (7 * r + 5) % 10).double()
    s = torch.where(kind == 3, torch.full_like(s, min(spacing, 0.05)), s)
    omega = torch.where(r % 6 == 5, torch.zeros(R, dtype=torch.float64), 0.5 + 0.5 * (r % 4).double()) if R > 1 else torch.ones(1)
    return D.float(), s.float(), omega.float()


def agreement_inputs(case, pre, post, device):
    """(spec, params, densities, features, rays_o, rays_d, jitter, rng, D, s, omega) of one agreement case"""
    spec, params, dens, feat, ro, rd, jitter, rng = T.agreement_inputs(case, pre, post, device)
    (x0, x1), (y0, y1), (z0, z1) = WALL
    dens = dens.clone()
    dens[x0:x1, y0:y1, z0:z1] = WALL_RAW
    D, s, omega = (t.to(device) for t in targets(params, ro, rd))
    return spec, params, dens, feat, ro, rd, jitter, rng, D, s, omega


def targets_inside(rays_o, rays_d, D):
    p = rays_o.cpu().double() + rays_d.cpu().double() * D.cpu().double()[:, None]
    lo, hi = (torch.tensor([a[i] for a in H.AABB], dtype=torch.float64) for i in (0, 1))
    return ((p > lo) & (p < hi)).all(dim=1)


def assert_agreement_not_vacuous(case, params, z, rays_o, rays_d, D, s, L, grad):
    """the conditions on the float64 restatement: at least a quarter of the rays have their target inside the grid's box and
    sum_k c_k > 0.1 s_r; at least one ray's target lies behind `far` with every c_k == 0, so that L_r and its gradient are
    exactly 0; the gradient lands on more than 100 voxels.  Two edge cases are held to what they can meet BY DEFINITION, as in
    test_distortion_host: a single ray (R == 1) is of the first kind and ends at the opaque wall a few cells into the dense box (20 voxels are
    asked for); a single sample (S == 1) has dz_0 = 0, so L_r = 0 and the gradient vanishes for every ray -- the case checks that
    the kernel says exactly that."""
    R, S = case[8], case[9]
    if S == 1:
        assert float(L.abs().max()) == 0.0 and int((grad != 0).sum()) == 0
        return
    csum = PR.coefficients(z.cpu(), D.cpu(), s.cpu()).sum(dim=1)
    good = targets_inside(rays_o, rays_d, D) & (csum > 0.1 * s.cpu().double())
    assert float(good.double().mean()) >= 0.25
    assert int((grad != 0).sum()) > (20 if R == 1 else 100)
    if R != 1:
        behind = D.cpu() >= params.far + 2.0     # (the fourth kind of targets())
        assert int(behind.sum()) >= 1 and bool((L.cpu()[behind] == 0).all())


# The near-empty case: a softplus field of raw -10 +- 0.5 at scale 1 (sigma 4.5e-5, x = sigma delta = 3e-6 at S = 64), targets at
# the closest approach to the origin with s = one sample spacing: w sits far below eps, where alpha = 1 - exp(-x) in float32
# carries an error of 1e-2 relative to w straight into log(w + eps) and 1 / (w + eps).
def near_empty_inputs(device):
    """(spec, params, densities, features, rays_o, rays_d, jitter, rng, D, s, omega): one 24 x 24 camera, S = 64"""
    g = torch.Generator().manual_seed(19)
    dens = -10.0 + (torch.rand((*H.DIMS, 1), generator=g) - 0.5)
    feat = torch.zeros((*H.DIMS, 3))
    spec = ops.GridSpec(aabb=H.AABB, density_scale=1.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS)
    ro, rd = H.cameras(24, 1, device)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, image_width=24)
    o, d = ro.cpu().double(), rd.cpu().double()
    D = (-(o * d).sum(dim=1) / (d * d).sum(dim=1)).float()
    s = torch.full_like(D, (workload.FAR - workload.NEAR) / 64)
    return spec, params, dens.to(device), feat.to(device), ro, rd, None, (0, 0), D.to(device), s.to(device), None


# The descent fixture: a faint uniform fog (softplus field, raw -3 at scale 2: sigma 2.5e-3) and no surface; the targets lie on
# a sphere of radius 0.5 around the origin, seen by 2 cameras of 24 x 24 at S = 64.  Rays that miss the sphere have weight 0.
FOG_LR, FOG_STEPS = 0.03, 30
# (the float64 restatement: loss 0.2894 -> 0.2299, mean |E[z] - D| of the supervised rays 0.3885 -> 0.3246)
FOG_LOSS_RATIO, FOG_DEPTH_RATIO = 0.85, 0.9
FOG_DIMS, FOG_AABB, FOG_RADIUS = (32, 32, 32), ((-1.5, 1.5),) * 3, 0.5


def fog_inputs(device):
    """(spec, params, densities, features, rays_o, rays_d, D, s, omega)"""
    spec = ops.GridSpec(aabb=FOG_AABB, density_scale=2.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS)
    ro, rd = H.cameras(24, 2, device)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, image_width=24, image_height=24)
    o, d = ro.cpu().double(), rd.cpu().double()
    a, b, c = (d * d).sum(dim=1), (o * d).sum(dim=1), (o * o).sum(dim=1) - FOG_RADIUS ** 2
    disc = b * b - a * c
    hit = disc > 0
    D = torch.where(hit, (-b - disc.clamp_min(0).sqrt()) / a, -b / a).float()
    s = torch.full_like(D, 2.0 * (workload.FAR - workload.NEAR) / 64)
    dens = torch.full((*FOG_DIMS, 1), -3.0)
    feat = torch.zeros((*FOG_DIMS, 3))
    return spec, params, dens.to(device), feat.to(device), ro, rd, D.to(device), s.to(device), hit.float().to(device)


def expected_depth(z, w):
    """sum_k w_k z_k / sum_k w_k per ray"""
    return (w * z.to(w.dtype)).sum(dim=1) / w.sum(dim=1).clamp_min(1e-300)


def fog_descent_reference(fn, spec, params, dens, feat, ro, rd, D, s, omega):
    """the float64 restatement's FOG_STEPS Adam steps on the term alone: the loss before every step and after the last"""
    d = dens.detach().double().clone().requires_grad_(True)
    opt = torch.optim.Adam([d], lr=FOG_LR)
    om = omega.double()
    losses = []
    for _ in range(FOG_STEPS):
        opt.zero_grad()
        loss = (fn(spec, params, d, feat, ro, rd, D, s) * om).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    losses.append(float((fn(spec, params, d.detach(), feat, ro, rd, D, s) * om).mean()))
    return losses, d.detach()


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


NAMES = ["grid", "cfg", "rays_o", "rays_d", "R", "jitter", "target_depth", "target_sigma", "ray_weight", "eps", "grad_scale",
         "loss_out", "ray_loss", "d_densities", "accumulate", "scratch", "scratch_bytes", "stream"]
CTYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def test_depth_symbols_are_declared_with_no_cpu_twin_and_abi_13():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    for name in ("voxe_depth_scratch_bytes", "voxe_depth_fwd_bwd", "voxe_depth_debug_lanes"):
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols()
    assert not re.search(r"\bvoxe_cpu_\w*depth_fwd", text)
    assert not any("depth_fwd" in s or "depth_scratch" in s for s in abi.cpu_symbols())
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text
    L = _lib()
    assert L.voxe_abi_version() == 13
    for name in ("voxe_depth_scratch_bytes", "voxe_depth_fwd_bwd", "voxe_depth_debug_lanes"):
        assert hasattr(L, name)
    assert "voxe_depth.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    # the header's prototype has the arguments the binding passes, in order and of the same types
    proto = re.search(r"int voxe_depth_fwd_bwd\((.*?)\);", text, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    args = [a.split() for a in proto.split(",")]
    assert [a[-1].lstrip("*") for a in args] == NAMES
    argtypes = L.voxe_depth_fwd_bwd.argtypes
    assert len(argtypes) == len(NAMES)
    for a, ct in zip(args, argtypes):
        pointer = "*" in "".join(a)
        if pointer:
            assert ct not in CTYPES.values(), a
        else:
            assert ct is CTYPES[a[-2]], a
    assert L.voxe_depth_scratch_bytes.argtypes == [ctypes.c_int64] and L.voxe_depth_debug_lanes.argtypes == [ctypes.c_int32]


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    g = make_grid_desc(16, 0, (8, 6, 5), 3, H.AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)   # features NULL: not read
    c = make_render_cfg(32, 1.0, 4.0)
    need = L.voxe_depth_scratch_bytes(4)
    assert need >= 8 * 4 and L.voxe_depth_scratch_bytes(1 << 20) >= 8 << 20

    def call(g_=g, c_=c, ro=P, rd=P, R=4, D=P, s=P, w=None, eps=1e-5, loss=None, ray=None, d=None, acc=1, sc=P, nbytes=need):
        return L.voxe_depth_fwd_bwd(ctypes.byref(g_) if g_ else None, ctypes.byref(c_) if c_ else None, ro, rd, R, None, D, s, w, eps,
                                    1.0, loss, ray, d, acc, sc, nbytes, None)

    assert call(g_=None) == abi.ERR_NULL_POINTER and call(c_=None) == abi.ERR_NULL_POINTER
    assert call(ro=None) == abi.ERR_NULL_POINTER and call(rd=None) == abi.ERR_NULL_POINTER
    assert call(D=None) == abi.ERR_NULL_POINTER and call(s=None) == abi.ERR_NULL_POINTER
    g.densities = 0
    assert call(g) == abi.ERR_NULL_POINTER
    g.densities = 16
    assert call(R=-1) == abi.ERR_BAD_SHAPE and call(R=1 << 31) == abi.ERR_BAD_SHAPE
    for eps in (0.0, -1e-5, float("inf"), float("nan")):
        assert call(eps=eps) == abi.ERR_BAD_SHAPE, eps
    for dims in ((0, 6, 5), (8, -1, 5), (1300, 1300, 1300)):
        g.X, g.Y, g.Z = dims
        assert call(g) == abi.ERR_BAD_SHAPE, dims
    g.X, g.Y, g.Z = 8, 6, 5
    c.num_samples = 0
    assert call(c_=c) == abi.ERR_BAD_SHAPE
    c.num_samples = 32
    g.density_post_act = 9
    assert call(g) == abi.ERR_UNSUPPORTED
    g.density_post_act = abi.ACT_RELU
    # the loss needs the scratch
    assert call(loss=P, sc=None) == abi.ERR_WORKSPACE and call(loss=P, nbytes=need - 1) == abi.ERR_WORKSPACE
    # no launch: R == 0 (NULL rays and targets allowed), or all three outputs NULL (accumulate != 0: d_densities is not touched)
    assert call(ro=None, rd=None, D=None, s=None, R=0, loss=P, ray=P, d=P) == abi.OK
    assert call() == abi.OK and call(w=P) == abi.OK and call(sc=None, nbytes=0) == abi.OK
    for lanes in (1, 2, 4, 8, 0):
        assert L.voxe_depth_debug_lanes(lanes) == abi.OK
    assert L.voxe_depth_debug_lanes(3) == abi.ERR_BAD_SHAPE and L.voxe_depth_debug_lanes(16) == abi.ERR_BAD_SHAPE


def test_operator_refuses_host_tensors_and_bad_arguments():
    from voxe_hip.runtime import VoxeError

    spec = ops.GridSpec(aabb=H.AABB)
    params = ops.RenderParams(num_samples=8, near=1.0, far=4.0)
    z2, z3 = torch.zeros(2), torch.zeros(2, 3)
    with pytest.raises(VoxeError):
        ops.depth_loss(spec, params, torch.zeros(4, 4, 4, 1), z3, z3, z2, z2 + 1)
    with pytest.raises(VoxeError):
        ops.depth_loss(spec, params, torch.zeros(4, 4, 4, 1), z3, z3, z2, z2 + 1, eps=0.0)
    with pytest.raises(VoxeError):
        ops.depth_loss(spec, params, torch.zeros(4, 4, 4, 1), z3, z3, z2.clone().requires_grad_(True), z2 + 1)


# ---- the restatement checks itself ------------------------------------------------------------------------------------
def _random_ray(S, seed):
    """optical depths x (some 0, as outside the box), depths z and c for a target inside the ray, float64"""
    g = torch.Generator().manual_seed(seed)
    z = torch.sort(torch.rand(1, S, generator=g) * 4.0 + 2.0, dim=1).values
    x = torch.rand(S, generator=g, dtype=torch.float64) * (torch.rand(S, generator=g) < 0.7) * 0.4
    c = PR.coefficients(z, torch.tensor([3.7]), torch.tensor([0.6]))[0]
    return x, z, c


def _literal(x, c):
    alpha = 1.0 - torch.exp(-x)
    T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1.0 - alpha[:-1]]), dim=0)
    return PR.literal_sum((alpha * T)[None], c[None])[0]


@pytest.mark.parametrize("S", [1, 2, 37, 96])
def test_lane_split_and_closed_form_equal_the_literal_sum(S):
    """the kernel's G-lane evaluation (phases 0 - 3, in float64) and the closed-form dL/dx give the literal sum and autograd's
    gradient to 1e-12"""
    x, _, c = _random_ray(S, 23 + S)
    x.requires_grad_(True)
    L = _literal(x, c)
    (q_ref,) = torch.autograd.grad(L, x) if S > 1 else (torch.zeros_like(x),)
    Lc, qc = PR.closed_form(x.detach(), c)
    assert abs(float(Lc) - float(L.detach())) < 1e-12 and float((qc - q_ref).abs().max()) < 1e-12
    for G in (1, 2, 4, 8):
        Lg, q = PR.lane_split(x.detach(), c, G)
        assert abs(Lg - float(L.detach())) < 1e-12, G
        assert float((q - q_ref).abs().max()) < 1e-12, G
    assert float(L.detach()) > 1e-2 if S > 2 else float(L.detach()) >= 0.0
    if S == 1:
        assert float(L.detach()) == 0.0 and float(c.abs().max()) == 0.0


def test_the_constants_behind_an_opaque_wall_are_in_the_value():
    """a wall of optical depth 2000 at sample 10 of 40 (T reaches exactly 0 behind it, in float64 too), the target behind it at
    sample 25: every sample behind the wall has w = 0 and adds -c_k log(eps); a march that stops at the wall loses them"""
    S = 40
    z = torch.linspace(2.0, 6.0, S)[None]
    x = torch.full((S,), 1e-3, dtype=torch.float64)
    x[10] = 2000.0
    c = PR.coefficients(z, z[:, 25], torch.tensor([0.15]))[0]
    L = float(_literal(x, c))
    behind = float(-np.log(PR._eps(PR.EPS)) * c[11:].sum())
    assert float(c[11:].sum()) > 0.3 and float(c[:11].sum()) < 1e-12
    assert abs(L - behind) < 1e-9 and L > 4.0
    for G in (1, 2, 4, 8):
        Lg, q = PR.lane_split(x, c, G)
        assert abs(Lg - L) < 1e-12 and float(q[11:].abs().max()) == 0.0, G


# ---- targets on rays --------------------------------------------------------------------------------------------------
def test_depth_targets_on_hand_made_rays():
    from thre3d_atom.rendering.volumetric.render_interface import Rays
    from thre3d_atom.thre3d_reprs.depth import depth_targets_on_rays

    o = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [0.0, 0.0, -4.0], [0.0, 0.0, 0.0]])
    d = torch.tensor([[0.0, 0.0, 1.0], [0.0, 2.0, 0.0], [0.0, 0.0, 0.5], [1.0, 1.0, 0.0]])
    p = torch.tensor([[0.3, -0.2, 2.5], [1.0, 7.0, 3.5], [0.0, 0.0, 1.0], [-1.0, -1.0, 5.0]], requires_grad=True)
    t = depth_targets_on_rays(Rays(o, d), p)
    assert not t.requires_grad
    assert torch.allclose(t, torch.tensor([2.5, 2.5, 10.0, -1.0]), atol=1e-6)
    # the point of the ray at t* is the foot of the perpendicular from P
    foot = o + d * t[:, None]
    assert float(((p.detach() - foot) * d).sum(dim=1).abs().max()) < 1e-5


# ---- the inputs are not vacuous (oracle probe -> restatement, no device) ----------------------------------------------
@pytest.mark.parametrize("pre,post", ACTS)
@pytest.mark.parametrize("case", agreement_cases(), ids=lambda c: c[0])
def test_agreement_inputs_are_not_vacuous(case, pre, post):
    spec, params, dens, feat, ro, rd, jitter, rng, D, s, omega = agreement_inputs(case, pre, post, CPU)
    z, _ = PR.host_samples(spec, params, dens, feat, ro, rd, jitter, rng)
    L, grad = PR.loss_and_gradient(PR.depth_host, spec, params, dens, feat, ro, rd, D, s, omega, jitter=jitter, rng=rng)
    print(f"{case[0]}: R {len(L)}  L_r > 0: {float((L > 0).double().mean()):.3f}  L_r == 0: {int((L == 0).sum())}  "
          f"grad != 0: {int((grad != 0).sum())}  loss {float((L * omega.double()).mean()):.6f}")
    assert bool(torch.isfinite(L).all()) and bool(torch.isfinite(grad).all())
    assert_agreement_not_vacuous(case, params, z, ro, rd, D, s, L, grad)


def test_near_empty_inputs_sit_below_eps_and_separate_the_two_alphas():
    """in float32 torch on these inputs, alpha = 1 - exp(-x) misses the GPU test's gradient bound and alpha = -expm1(-x) meets it"""
    spec, params, dens, feat, ro, rd, jitter, rng, D, s, _ = near_empty_inputs(CPU)
    z, inside = PR.host_samples(spec, params, dens, feat, ro, rd)

    def grad(dtype, weights):
        d = dens.clone().requires_grad_(True)
        R, S = z.shape
        p = ro[:, None, :] + rd[:, None, :] * z[:, :, None]
        sigma = PR.DR.sigma_from_raw(d, p.reshape(-1, 3), spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act,
                                     dtype).reshape(R, S)
        sigma = torch.where(inside.bool(), sigma, torch.zeros_like(sigma))
        w = weights(sigma, z, rd, dtype)
        L = PR.literal_sum(w, PR.coefficients(z, D, s, dtype))
        (g,) = torch.autograd.grad(L.mean(), d)
        return w.detach(), g.double()

    w64, g64 = grad(torch.float64, PR.DR.weights)
    _, g_exp = grad(torch.float32, PR.DR.weights)
    _, g_expm1 = grad(torch.float32, PR.weights_expm1)
    rel = lambda a: float((a - g64).norm() / g64.norm())
    print(f"near-empty: median w {float(w64[inside.bool()].median()):.3e}  float32 1 - exp: {rel(g_exp):.3e}  float32 expm1: {rel(g_expm1):.3e}")
    assert float(w64[inside.bool()].median()) < PR.EPS and int((g64 != 0).sum()) > 100
    assert rel(g_exp) > 1e-4 > 10 * rel(g_expm1)


def test_fog_fixture_descends_in_the_restatement():
    """the fixture of the GPU descent test behaves as that test expects, in float64 on the host: 30 Adam steps on the term
    alone lower the loss at every step and move the expected depth of the supervised rays towards the targets"""
    spec, params, dens, feat, ro, rd, D, s, omega = fog_inputs(CPU)
    assert float(omega.mean()) > 0.05
    z, inside = PR.host_samples(spec, params, dens, feat, ro, rd)
    fn = lambda sp, pa, d, f, o, dd, D_, s_: PR.from_samples(z, inside, d, o, dd, sp, D_, s_)
    losses, final = fog_descent_reference(fn, spec, params, dens, feat, ro, rd, D, s, omega)
    err = []
    for d in (dens.double(), final):
        p = ro[:, None, :] + rd[:, None, :] * z[:, :, None]
        sigma = PR.DR.sigma_from_raw(d, p.reshape(-1, 3), spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act)
        w = PR.DR.weights(torch.where(inside.bool(), sigma.reshape(z.shape), torch.zeros(z.shape, dtype=torch.float64)), z, rd)
        # (the last sample's weight is what is left of T: the background, not a termination inside the fog)
        e = expected_depth(z[:, :-1], w[:, :-1])
        err.append(float(((e - D.double()).abs() * omega.double()).sum() / omega.double().sum()))
    print(f"fog: loss {losses[0]:.5f} -> {losses[-1]:.5f}; |E[z] - D| of the supervised rays {err[0]:.4f} -> {err[1]:.4f}")
    assert all(b < a for a, b in zip(losses, losses[1:]))
    assert losses[-1] < FOG_LOSS_RATIO * losses[0] and err[1] < FOG_DEPTH_RATIO * err[0]


# ---- the importer's sparse-point sidecar and the dataset that carries it ----------------------------------------------
SFM_EYES = ((3.0, 0.5, 1.0), (-1.0, 3.0, 1.5), (0.5, -3.0, 2.0))
SFM_CAMERA = (64, 48, 60.0, 57.0, 31.5, 24.5)                      # width, height, fx, fy, cx, cy (PINHOLE)
SFM_CLOUD = np.random.default_rng(6).uniform(-0.5, 0.5, size=(30, 3))
SFM_BEHIND = np.array([6.0, 1.0, 2.0])                              # behind the first camera (which looks at the origin from x = 3)
SFM_ERRORS = np.random.default_rng(7).uniform(0.2, 1.5, size=31)


def _look_at(eye):
    """COLMAP's world-to-camera (R, t) of a camera at `eye` looking at the origin: x right, y down, z forward"""
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ eye


def _quaternion(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def _pixel(R, t, point):
    width, height, fx, fy, cx, cy = SFM_CAMERA
    pc = R @ np.asarray(point, np.float64) + t
    return float(fx * pc[0] / pc[2] + cx), float(fy * pc[1] / pc[2] + cy), float(pc[2])


@pytest.fixture()
def colmap_model(tmp_path):
    """a synthetic COLMAP text model: 3 cameras looking at a cloud of 30 points around the origin; every image observes every
    point at its exact projection, plus -- in the first image -- a point behind the camera (id 31), an observation outside the
    image (of point 1, at x = 70) and a keypoint without a 3D point (id -1)"""
    path = tmp_path / "sparse"
    path.mkdir()
    width, height, fx, fy, cx, cy = SFM_CAMERA
    (path / "cameras.txt").write_text(f"# Camera list\n1 PINHOLE {width} {height} {fx} {fy} {cx} {cy}\n")
    lines, kept = ["# Image list with two lines of data per image:"], {}
    for i, eye in enumerate(SFM_EYES):
        R, t = _look_at(eye)
        obs = []
        for j, p in enumerate(SFM_CLOUD):
            x, y, depth = _pixel(R, t, p)
            assert depth > 0 and 0 <= x < width and 0 <= y < height
            obs.append((x, y, j + 1))
        kept[f"img_{i}.png"] = list(obs)
        if i == 0:
            obs += [(20.0, 20.0, 31), (70.0, 10.0, 1), (5.0, 5.0, -1)]
        lines.append(f"{i + 1} {' '.join(repr(float(v)) for v in _quaternion(R))} {' '.join(repr(float(v)) for v in t)} 1 img_{i}.png")
        lines.append(" ".join(f"{x!r} {y!r} {pid}" for x, y, pid in obs))
    (path / "images.txt").write_text("\n".join(lines) + "\n")
    cloud = list(SFM_CLOUD) + [SFM_BEHIND]
    (path / "points3D.txt").write_text("# 3D point list\n" + "".join(
        f"{j + 1} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r} 128 128 128 {float(SFM_ERRORS[j])!r} 1 0\n"
        for j, p in enumerate(cloud)))
    return path, kept


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_importer_writes_the_sparse_points_and_they_project_back(colmap_model, tmp_path):
    import camera_ref as CR

    model, kept = colmap_model
    tool = _tool("convert_from_colmap_text")
    assert tool.main(["-m", str(model), "-o", str(tmp_path / "scene")]) == 0
    entries = json.loads((tmp_path / "scene" / "train_camera_params.json").read_text())
    with np.load(tmp_path / "scene" / "train_sparse_points.npz") as f:
        side = {k: f[k] for k in f.files}
    assert sorted(side) == ["error", "names", "offsets", "xy", "xyz"]
    assert side["names"].tolist() == list(entries) == [f"img_{i}.png" for i in range(3)]
    # 30 observations per image: the point behind the first camera, the observation outside the image and the keypoint
    # without a 3D point are dropped
    assert side["offsets"].tolist() == [0, 30, 60, 90] and side["offsets"].dtype == np.int64
    assert side["xy"].shape == (90, 2) and side["xyz"].shape == (90, 3) and side["error"].shape == (90,)
    assert all(side[k].dtype == np.float32 for k in ("xy", "xyz", "error"))
    for i, name in enumerate(side["names"].tolist()):
        rows = slice(side["offsets"][i], side["offsets"][i + 1])
        assert np.allclose(side["xy"][rows], np.array([(x, y) for x, y, _ in kept[name]]), atol=1e-4)
        assert np.allclose(side["xyz"][rows], SFM_CLOUD, atol=1e-6) and np.allclose(side["error"][rows], SFM_ERRORS[:30], atol=1e-6)
        # projecting xyz with the camera the tool wrote reproduces xy
        e = entries[name]
        intr = e["intrinsic"]
        cam = CR.Camera(intr["height"], intr["width"], intr["fx"], intr["fy"], intr["cx"], intr["cy"], tuple(intr["distortion"]))
        pose = np.concatenate([np.array(e["extrinsic"]["rotation"]), np.array(e["extrinsic"]["translation"])], axis=1)
        for xy, xyz in zip(side["xy"][rows], side["xyz"][rows]):
            got = CR.project(cam, pose, xyz.astype(np.float64))
            assert abs(got[0] - xy[0]) <= 1e-3 and abs(got[1] - xy[1]) <= 1e-3
    # --no_sparse_points writes the cameras only
    assert tool.main(["-m", str(model), "-o", str(tmp_path / "bare"), "--no_sparse_points"]) == 0
    assert (tmp_path / "bare" / "train_camera_params.json").exists() and not (tmp_path / "bare" / "train_sparse_points.npz").exists()


def test_importer_recentre_shifts_the_points_with_the_cameras(colmap_model, tmp_path):
    model, _ = colmap_model
    # move the whole model: the optical axes then meet at `offset`, which --recentre takes back out
    offset = np.array([0.7, -0.4, 0.25])
    lines = (model / "points3D.txt").read_text().splitlines()
    moved = [lines[0]] + [" ".join([p[0]] + [repr(float(v) + float(o)) for v, o in zip(p[1:4], offset)] + p[4:]) for p in
                          (line.split() for line in lines[1:])]
    (model / "points3D.txt").write_text("\n".join(moved) + "\n")
    images = (model / "images.txt").read_text().splitlines()
    for n, eye in enumerate(SFM_EYES):
        R, _ = _look_at(eye)
        head = images[1 + 2 * n].split()
        head[5:8] = [repr(float(v)) for v in -R @ (np.asarray(eye) + offset)]
        images[1 + 2 * n] = " ".join(head)
    (model / "images.txt").write_text("\n".join(images) + "\n")
    tool = _tool("convert_from_colmap_text")
    plain, centred = tool.sparse_points(model), tool.sparse_points(model, recentre=True)
    assert np.allclose(plain["xyz"][:30], SFM_CLOUD + offset, atol=1e-6)
    assert np.allclose(centred["xyz"][:30], SFM_CLOUD, atol=1e-5) and np.array_equal(plain["xy"], centred["xy"])
    entries = tool.convert(model, recentre=True)
    assert np.allclose(np.array(entries["img_0.png"]["extrinsic"]["translation"]).reshape(3), SFM_EYES[0], atol=1e-5)


def _write_images(folder, names, height=48, width=64):
    from PIL import Image

    folder.mkdir(parents=True, exist_ok=True)
    for n in names:
        Image.fromarray(np.full((height, width, 3), 128, np.uint8)).save(folder / n)


def test_dataset_carries_the_sparse_points(colmap_model, tmp_path):
    from thre3d_atom.data.datasets import PosedImagesDataset, sparse_points_path

    model, kept = colmap_model
    tool = _tool("convert_from_colmap_text")
    scene = tmp_path / "scene"
    assert tool.main(["-m", str(model), "-o", str(scene)]) == 0
    # the image folder holds two of the three images, in another order than the file's: matched by name
    _write_images(scene / "train", ["img_2.png", "img_0.png"])
    params = scene / "train_camera_params.json"
    assert sparse_points_path(params) == scene / "train_sparse_points.npz"
    data = PosedImagesDataset(scene / "train", params)
    sp = data.sparse_points
    assert sp.offsets.tolist() == [0, 30, 60] and sp.offsets.dtype == torch.int64
    assert np.allclose(sp.xy[:30].numpy(), np.array([(x, y) for x, y, _ in kept["img_0.png"]]), atol=1e-4)
    assert np.allclose(sp.xy[30:].numpy(), np.array([(x, y) for x, y, _ in kept["img_2.png"]]), atol=1e-4)
    assert np.allclose(sp.xyz[:30].numpy(), SFM_CLOUD, atol=1e-6) and np.allclose(sp.error[30:].numpy(), SFM_ERRORS[:30], atol=1e-6)
    # downsampled(2): pixel coordinates and pixel errors halve, the points stay; to() carries them
    half = data.downsampled(2.0)
    assert torch.allclose(half.sparse_points.xy, sp.xy / 2) and torch.allclose(half.sparse_points.error, sp.error / 2)
    assert torch.equal(half.sparse_points.xyz, sp.xyz) and torch.equal(half.sparse_points.offsets, sp.offsets)
    assert torch.equal(half.to("cpu").sparse_points.xy, half.sparse_points.xy)
    built_small = PosedImagesDataset(scene / "train", params, downsample_factor=2.0)
    assert torch.allclose(built_small.sparse_points.xy, sp.xy / 2) and built_small.camera_intrinsics.width == 32
    # normalize_scene_scale: the points scale with the camera centres (the farthest camera of the file lands at radius 1)
    scale = 1.0 / max(np.linalg.norm(e) for e in SFM_EYES)
    unit = PosedImagesDataset(scene / "train", params, normalize_scene_scale=True)
    assert np.allclose(unit.sparse_points.xyz.numpy(), sp.xyz.numpy() * scale, atol=1e-6)
    assert np.allclose(unit.poses[0, :, 3].numpy(), np.array(SFM_EYES[0]) * scale, atol=1e-6)
    # no sidecar: None, also after downsampled() and to()
    (scene / "train_sparse_points.npz").unlink()
    bare = PosedImagesDataset(scene / "train", params)
    assert bare.sparse_points is None and bare.downsampled(2.0).sparse_points is None and bare.to("cpu").sparse_points is None


def test_in_memory_dataset_takes_optional_sparse_points():
    from thre3d_atom.data.datasets import InMemoryPosedImages, SparsePoints
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

    images, poses = torch.rand(2, 3, 8, 8), torch.eye(4)[None, :3].repeat(2, 1, 1)
    intr, bounds = CameraIntrinsics(8, 8, 10.0), CameraBounds(1.0, 4.0)
    assert InMemoryPosedImages(images, poses, intr, bounds).sparse_points is None
    assert inspect.signature(InMemoryPosedImages.__init__).parameters["sparse_points"].default is None
    sp = SparsePoints(torch.tensor([0, 1, 3]), torch.rand(3, 2) * 8, torch.rand(3, 3), torch.rand(3))
    assert InMemoryPosedImages(images, poses, intr, bounds, sparse_points=sp).downsampled(2.0).sparse_points.xy.shape == (3, 2)
    with pytest.raises(ValueError):
        InMemoryPosedImages(images, poses, intr, bounds, sparse_points=SparsePoints(torch.tensor([0, 3]), *sp[1:]))


# ---- trainer options --------------------------------------------------------------------------------------------------
def test_cli_options_trainer_arguments_and_documents():
    spec = importlib.util.spec_from_file_location("train_depth_cli", os.path.join(ROOT, "train_sh_based_voxel_grid_with_posed_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opts = {p.name: p for p in mod.main.params}
    for name, default in (("depth_weight", 0.0), ("depth_ray_batch_size", 4096), ("depth_sigma_scale", 1.0)):
        assert opts[name].default == default and f"--{name}" in opts[name].opts
    from thre3d_atom.modules import trainers

    sig = inspect.signature(trainers.train_sh_vox_grid_vol_mod_with_posed_images)
    assert sig.parameters["depth_weight"].default == 0.0 and sig.parameters["depth_ray_batch_size"].default == 4096
    assert sig.parameters["depth_sigma_scale"].default == 1.0
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.depth import depth_loss_on_rays, depth_targets_on_rays

    assert callable(depth_loss_on_rays) and callable(depth_targets_on_rays) and callable(VolumetricModel.depth_loss)
    assert inspect.signature(depth_loss_on_rays).parameters["eps"].default == 1e-5
    assert callable(ops.depth_loss) and callable(ops.depth_fwd_bwd)
    for doc in ("README.md", "INTEGRATION.md"):
        assert "--depth_weight" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.19" in design and "profiles/depth_bench.txt" in design and "expm1" in design
    assert "voxe_depth_fwd_bwd" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the attention and SDS trainers do not take the term
    from thre3d_atom.modules import attn_grid_trainer, sds_trainer

    for module in (attn_grid_trainer, sds_trainer):
        assert "depth_weight" not in open(module.__file__).read()


def test_weight_zero_leaves_the_one_call_iteration_and_a_missing_sidecar_is_named(tmp_path, monkeypatch):
    """depth_weight = 0 takes the trainer's code path as it was, sparse points or not: the one-call iteration runs and the depth
    term is never evaluated; above 0 it is the other way round; above 0 without sparse points the trainer names the file"""
    from thre3d_atom.data.datasets import SparsePoints
    from thre3d_atom.modules import trainers
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

    calls = {"one_call": 0, "depth": 0, "render": 0}
    seen = {}

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
        def __init__(self, sparse):
            self.images = torch.rand(4, 3, 8, 8)
            self.poses = torch.eye(4)[None, :3].repeat(4, 1, 1)
            self.poses[:, 2, 3] = 3.0
            self.camera_intrinsics = CameraIntrinsics(8, 8, 10.0)
            self.camera_bounds = CameraBounds(1.0, 4.0)
            self.sparse_points = sparse

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

    def fake_depth(self, rays, target_depth, target_sigma, ray_weight=None, **kw):
        calls["depth"] += 1
        seen.update(R=rays.origins.shape[0], D=target_depth, s=target_sigma, w=ray_weight)
        return self.thre3d_repr.densities.sum() * 0

    def fake_cast(intr, poses, images, flat_index, image_ids, differentiable, intrinsics):
        # rays down -z from the camera centres, one unit per unit of depth: the target of a point is its distance along -z
        from thre3d_atom.rendering.volumetric.render_interface import Rays

        cam = flat_index // (8 * 8)
        assert int(flat_index.min()) >= 0 and int(cam.max()) < poses.shape[0]
        return Rays(poses[cam, :, 3], torch.tensor([0.0, 0.0, -1.0]).expand(len(cam), 3)), None

    monkeypatch.setattr(trainers, "FusedGridAdam", FakeOpt)
    monkeypatch.setattr(trainers, "scale_voxel_grid_with_required_output_size", lambda grid, size: grid)
    monkeypatch.setattr(trainers, "_render_params", lambda *a, **k: None)
    monkeypatch.setattr(trainers, "_next_rng", lambda: (0, 0))
    monkeypatch.setattr(trainers, "_cast_and_gather", fake_cast)
    monkeypatch.setattr(VolumetricModel, "render_rays", fake_render_rays)
    monkeypatch.setattr(VolumetricModel, "depth_loss", fake_depth)
    monkeypatch.setattr(trainers, "sample_random_rays_and_pixels_from_cameras",
                        lambda intr, poses, images, n, **k: (type("R", (), {"origins": torch.zeros(16, 3)})(), torch.zeros(16, 3)))
    # 5 observations per camera, 1.5 in front of it; reprojection errors of 2 px (-> s = 2 * 1.5 / 10 = 0.3) and 0.01 px (-> the floor)
    sparse = SparsePoints(torch.arange(5) * 5, torch.rand(20, 2) * 8, torch.tensor([[0.0, 0.0, 1.5]]).repeat(20, 1),
                          torch.tensor([2.0, 0.01]).repeat(10))

    def run(weight, data):
        for k in calls:
            calls[k] = 0
        vg = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.1, 0.1, 0.1), tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(8, CameraBounds(1.0, 4.0)), device=CPU)
        trainers.train_sh_vox_grid_vol_mod_with_posed_images(vm, data, tmp_path, num_stages=1, num_iterations_per_stage=3,
                                                             fast_debug_mode=True, depth_weight=weight, depth_ray_batch_size=64)

    for data in (Data(sparse), Data(None)):
        run(0.0, data)
        assert calls == {"one_call": 3, "depth": 0, "render": 0}, calls
    run(0.5, Data(sparse))
    assert calls == {"one_call": 0, "depth": 3, "render": 6}, calls
    assert seen["R"] == 64 and torch.allclose(seen["D"], torch.full((64,), 1.5)) and bool((seen["w"] == 1).all())
    floor = (4.0 - 1.0) / 8
    assert set(round(float(v), 5) for v in seen["s"]) <= {round(floor, 5), round(max(0.3, floor), 5)} and float(seen["s"].min()) >= floor
    with pytest.raises(ValueError, match="_sparse_points.npz"):
        run(0.5, Data(None))
