"""CPU checks of the orientation loss on rays: the C ABI's declarations and argument validation (no device work), self-checks of
the float64 restatement tests/orientation_ref.py (its cell gradient against normals_ref and against autograd of the interpolant,
the closed-form gradient, the kernel's lane-split evaluation), the trainer's options, and -- with the oracle's sample probe
feeding the restatement -- that the inputs of the GPU tests (tests/test_orientation_gpu.py builds them with the functions
below) are well conditioned and not vacuous.

Conditioning of the agreement inputs.  The GPU tests hold the kernel's gradient to rel_l2 < 1e-4 against float64; an input on
which float32 arithmetic itself cannot do much better says nothing about the kernel.  Every agreement input must therefore let
the restatement's own float32 evaluation reach 2.5e-5 (a quarter of the bound), at both values of normal_eps.  The random
corner values of O(1) of the inputs below do, with 2e-7 to 3e-6 (the figures are printed).  A nearly flat field (0.5 +- 0.001),
whose slope differences cancel, is not among the inputs."""
import ctypes
import importlib.util
import inspect
import os
import re

import pytest
import torch

import distortion_ref as DR
import normals_ref
import orientation_ref as OR
import test_distortion_host as T
import test_visibility_host as H
from conftest import ROOT
from voxe_hip import abi, ops, workload
from voxe_hip.desc import make_grid_desc, make_render_cfg

CPU = torch.device("cpu")
ACTS = T.ACTS
EPS = (0.0, 1e-2)
YARDSTICK_GATE = 2.5e-5     # a quarter of the GPU tests' gradient bound


# ---- inputs shared with the GPU tests ---------------------------------------------------------------------------------
def agreement_cases():
    """the cases of the distortion tests (carved densities: rays that see nothing, rays behind opaque voxels), then one case
    DENSE TO THE GRID FACES: the uncarved random densities, so that the cells with i0 == -1 and i0 == N - 1, whose slope is not
    the difference of the gather weights, carry weight; 8 rays that miss the grid keep an exact L_r == 0 among them"""
    return T.agreement_cases() + [("dense_faces", 48, 1, False, None, False, False, "dense", None, 96)]


def agreement_inputs(case, pre, post, device):
    """(spec, params, densities, features, rays_o, rays_d, jitter, rng) of one agreement case"""
    if case[7] != "dense":
        spec, params, dens, feat, ro, rd, jitter, rng = T.agreement_inputs(case, pre, post, device)
        if case[9] == 1:
            # (the one sample of S = 1 sits at `near`: 3.9 puts it inside the carved box for the central rays -- at the distortion
            #  tests' 3.0 it is in front of the box on every ray and every L_r would be 0.  Its interval is the last one, 1e10:
            #  w is 1 or 0 and the whole gradient comes through the normals)
            params = ops.RenderParams(num_samples=1, near=3.9, far=5.0, perturb=params.perturb)
        return spec, params, dens, feat, ro, rd, jitter, rng
    spec, params, dens, feat, ro, rd, jitter, rng = H.agreement_inputs(("plain", case[1], 1, False, None, False, False, "image"),
                                                                       pre, post, device)
    # (no image layout: the rays that look away from the grid follow the image's)
    ro, rd = torch.cat([ro, ro[:8]]).contiguous(), torch.cat([rd, -rd[:8]]).contiguous()
    params = ops.RenderParams(num_samples=case[9], near=workload.NEAR, far=workload.FAR)
    return spec, params, dens, feat, ro, rd, jitter, rng


def ray_weights(R, device):
    """omega [R] >= 0 of the weighted runs, a fifth of them 0"""
    g = torch.Generator().manual_seed(R)
    return (torch.rand(R, generator=g) * 2.0 * (torch.rand(R, generator=g) > 0.2)).to(device)


def assert_agreement_not_vacuous(case, L, grad, grad_normals):
    """the conditions on the float64 restatement's per-ray loss, its gradient and the part of it that comes through the normals.
    A single ray (R == 1) cannot both weigh and be empty -- it must weigh -- and its footprints hold fewer than 100 voxels (30
    are asked for)."""
    R = case[8]
    assert float((L > 1e-4).double().mean()) >= 0.25
    assert int((grad != 0).sum()) > (30 if R == 1 else 100)
    if R != 1:
        assert int((L == 0).sum()) >= 1
    assert float(grad_normals.norm()) >= 0.1 * float(grad.norm())


# The analytic fixture: v = pre-activated density is a ramp in x only (identity + Softplus), so G = (g, 0, 0) with g > 0 in every
# interior cell and n = (-1, 0, 0): rays that travel towards -x see the normal's back, c = -u_x; rays towards +x see its front
RAMP_DIMS = (32, 32, 32)
RAMP_AABB = ((-1.5, 1.5),) * 3


def ramp_inputs(device):
    """(spec, params, densities, features, rays_o [72,3], rays_d [72,3]): the first 36 rays have u_x < 0, the others u_x > 0;
    every sample lies in [-1.3, 1.3]^3, i.e. in interior cells (the face cells are the outer 0.047)"""
    n = RAMP_DIMS[0]
    x = (torch.arange(n, dtype=torch.float32) + 0.5) / n * 3.0 - 1.5
    dens = (0.7 * x)[:, None, None, None].expand(n, n, n, 1).contiguous()      # v = 2 raw in [-2, 2]
    spec = ops.GridSpec(aabb=RAMP_AABB, density_scale=2.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS)
    params = ops.RenderParams(num_samples=64, near=0.1, far=1.2)
    a = torch.linspace(-0.9, -0.4, 6)
    yy, zz = torch.meshgrid(a, a, indexing="ij")
    ro, rd = [], []
    for sx in (-1.0, 1.0):
        ro.append(torch.stack([torch.full_like(yy, -0.9 * sx), yy, zz], dim=-1).reshape(-1, 3))
        rd.append(torch.tensor([0.6 * sx, 0.48, 0.64]).mul(1.3).expand(36, 3))
    ro, rd = torch.cat(ro).contiguous(), torch.cat(rd).contiguous()
    end = ro + rd * 1.2
    assert float(torch.maximum(ro.abs().max(), end.abs().max())) < 1.3
    return spec, params, dens.to(device), torch.zeros((*RAMP_DIMS, 3), device=device), ro.to(device), rd.to(device)


# The descent fixture: the fuzzy ball.  A smooth radial falloff under a Softplus, semi-transparent, so that the hemisphere
# that faces away from a camera carries weight with its normal pointing away from it.  FUZZY_STEPS Adam steps on the term alone;
# the two constants are the float64 restatement's (test_fuzzy_ball_descends_in_the_restatement computes them again).
FUZZY_LR, FUZZY_STEPS = 0.05, 30
FUZZY_DIMS = (32, 32, 32)
FUZZY_AABB = ((-1.5, 1.5),) * 3
FUZZY_LOSS_RATIO = 0.1104     # last / first loss of the restatement's descent
FUZZY_MAX_MOVE = 1.4344       # its largest |raw - raw_0| over the voxels


def fuzzy_inputs(device):
    """(spec, params, densities, features, rays_o, rays_d): 2 cameras at 24 x 24, S = 64, no jitter"""
    n = FUZZY_DIMS[0]
    ax = (torch.arange(n, dtype=torch.float32) + 0.5) / n * 3.0 - 1.5
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(x * x + y * y + z * z)
    dens = (1.0 - 2.5 * r)[..., None].contiguous()             # v = 2 raw: 2 at the centre, 0 at r = 0.4, -3 at r = 1
    spec = ops.GridSpec(aabb=FUZZY_AABB, density_scale=2.0, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS)
    ro, rd = H.cameras(24, 2, device)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, image_width=24, image_height=24)
    return spec, params, dens.to(device), torch.zeros((*FUZZY_DIMS, 3), device=device), ro, rd


def fuzzy_descent(loss_fn, dens, dtype):
    """FUZZY_STEPS Adam steps of loss_fn(densities) -> scalar: (the loss before every step and after the last, final densities)"""
    d = dens.detach().to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([d], lr=FUZZY_LR)
    losses = []
    for _ in range(FUZZY_STEPS):
        opt.zero_grad()
        loss = loss_fn(d)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    with torch.no_grad():
        losses.append(float(loss_fn(d.detach())))
    return losses, d.detach()


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


NAMES = ["grid", "cfg", "rays_o", "rays_d", "R", "jitter", "ray_weight", "normal_eps", "grad_scale", "loss_out", "ray_loss",
         "d_densities", "accumulate", "scratch", "scratch_bytes", "stream"]
SYMBOLS = ("voxe_orientation_scratch_bytes", "voxe_orientation_fwd_bwd", "voxe_orientation_debug_lanes")
CTYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def test_orientation_symbols_are_declared_with_no_cpu_twin_and_abi_13():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols()
    assert not re.search(r"\bvoxe_cpu_\w*orientation", text)
    assert not any("orientation" in s for s in abi.cpu_symbols())
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text
    L = _lib()
    assert L.voxe_abi_version() == 13
    for name in SYMBOLS:
        assert hasattr(L, name)
    assert "voxe_orientation.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    # the header's prototype has the arguments the binding passes, in order and of the same types
    proto = re.search(r"int voxe_orientation_fwd_bwd\((.*?)\);", text, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    args = [a.split() for a in proto.split(",")]
    assert [a[-1].lstrip("*") for a in args] == NAMES
    argtypes = L.voxe_orientation_fwd_bwd.argtypes
    assert len(argtypes) == len(NAMES)
    for a, ct in zip(args, argtypes):
        if "*" in "".join(a):
            assert ct not in CTYPES.values(), a
        else:
            assert ct is CTYPES[a[-2]], a
    assert L.voxe_orientation_scratch_bytes.argtypes == [ctypes.c_int64]
    assert L.voxe_orientation_debug_lanes.argtypes == [ctypes.c_int32]


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    g = make_grid_desc(16, 0, (8, 6, 5), 3, H.AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)   # features NULL: not read
    c = make_render_cfg(32, 1.0, 4.0)
    need = L.voxe_orientation_scratch_bytes(4)
    assert need >= 8 * 4 and L.voxe_orientation_scratch_bytes(1 << 20) >= 8 << 20

    def call(g_=g, c_=c, ro=P, rd=P, R=4, w=None, eps=1e-2, loss=None, ray=None, d=None, acc=1, sc=P, nbytes=need):
        return L.voxe_orientation_fwd_bwd(ctypes.byref(g_) if g_ else None, ctypes.byref(c_) if c_ else None, ro, rd, R, None, w, eps,
                                          1.0, loss, ray, d, acc, sc, nbytes, None)

    assert call(g_=None) == abi.ERR_NULL_POINTER and call(c_=None) == abi.ERR_NULL_POINTER
    assert call(ro=None) == abi.ERR_NULL_POINTER and call(rd=None) == abi.ERR_NULL_POINTER
    g.densities = 0
    assert call(g) == abi.ERR_NULL_POINTER
    g.densities = 16
    assert call(R=-1) == abi.ERR_BAD_SHAPE and call(R=1 << 31) == abi.ERR_BAD_SHAPE
    for eps in (-1e-5, float("inf"), float("-inf"), float("nan")):
        assert call(eps=eps) == abi.ERR_BAD_SHAPE, eps
    assert call(eps=0.0) == abi.OK
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
    assert call() == abi.OK and call(w=P) == abi.OK and call(sc=None, nbytes=0) == abi.OK
    for lanes in (1, 2, 4, 8, 0):
        assert L.voxe_orientation_debug_lanes(lanes) == abi.OK
    assert L.voxe_orientation_debug_lanes(3) == abi.ERR_BAD_SHAPE and L.voxe_orientation_debug_lanes(16) == abi.ERR_BAD_SHAPE


def test_operator_refuses_host_tensors_and_bad_arguments():
    from voxe_hip.runtime import VoxeError

    spec = ops.GridSpec(aabb=H.AABB)
    params = ops.RenderParams(num_samples=8, near=1.0, far=4.0)
    z3 = torch.zeros(2, 3)
    with pytest.raises(VoxeError):
        ops.orientation_loss(spec, params, torch.zeros(4, 4, 4, 1), z3, z3)
    for eps in (-1.0, float("inf"), float("nan")):
        with pytest.raises(VoxeError):
            ops.orientation_loss(spec, params, torch.zeros(4, 4, 4, 1), z3, z3, normal_eps=eps)
    with pytest.raises(VoxeError):
        ops.orientation_loss(spec, params, torch.zeros(4, 4, 4, 1), z3, z3, torch.ones(2, requires_grad=True))


# ---- the restatement checks itself ------------------------------------------------------------------------------------
def _points(n, seed, margin):
    """world points [n,3] inside H.AABB, `margin` voxels away from the faces (negative: up to that far outside the last voxel
    centres, i.e. in the face cells)"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.tensor([a[0] for a in H.AABB])
    hi = torch.tensor([a[1] for a in H.AABB])
    vox = (hi - lo) / torch.tensor(H.DIMS, dtype=torch.float32)
    lo, hi = lo + (0.5 + margin) * vox, hi - (0.5 + margin) * vox
    return lo + (hi - lo) * torch.rand((n, 3), generator=g)


@pytest.mark.parametrize("pre", [abi.ACT_IDENTITY, abi.ACT_ABS])
def test_cell_gradient_equals_the_normals_restatement(pre):
    """-G / |G| of the restatement's cell gradient is normals_ref's normal, in the face cells too (points up to the box faces)"""
    dens = torch.empty((*H.DIMS, 1)).uniform_(-1.5, 1.5, generator=torch.Generator().manual_seed(3))
    p = _points(4000, 5, -0.499)
    G = OR.cell_gradient(dens, p, H.AABB, 2.0, pre)
    _, i0, _, _ = normals_ref.index_coords(p, H.DIMS, H.AABB)
    face = ((i0 < 0) | (i0 >= torch.tensor(H.DIMS) - 1)).any(dim=1)
    assert int(face.sum()) > 200 and int((~face).sum()) > 2000
    v = normals_ref.field(dens, 2.0, pre)
    _, G_ref = normals_ref.value_and_gradient(v, p, H.AABB)
    assert float((G - G_ref).abs().max()) <= 1e-5 * float(G_ref.abs().max())
    n_ref = normals_ref.point_normals(v, p, H.AABB)
    n = normals_ref.normals_from_gradient(G)
    assert float((n - n_ref).abs().max()) < 1e-5
    # eps = 0: c = max(0, n . u)
    u = torch.nn.functional.normalize(torch.randn((4000, 3), generator=torch.Generator().manual_seed(6), dtype=torch.float64), dim=1)
    assert float((OR.facing(G, u, 0.0) - torch.relu((n_ref * u).sum(dim=1))).abs().max()) < 1e-5


def test_cell_gradient_of_interior_samples_is_the_gradient_of_the_interpolant():
    """for points in interior cells, G is autograd's gradient of V with respect to the position"""
    from voxe_hip.desc import norm_constants

    dens = torch.empty((*H.DIMS, 1)).uniform_(-1.5, 1.5, generator=torch.Generator().manual_seed(4))
    p = _points(2000, 7, 0.01)
    G = OR.cell_gradient(dens, p, H.AABB, 2.0, abi.ACT_IDENTITY)
    v = normals_ref.field(dens, 2.0, abi.ACT_IDENTITY).double()
    _, i0, _, _ = normals_ref.index_coords(p, H.DIMS, H.AABB)
    assert bool(((i0 >= 0) & (i0 < torch.tensor(H.DIMS) - 1)).all())
    scale, bias = norm_constants(H.AABB)
    pp = p.double().requires_grad_(True)
    u = ((pp * torch.tensor(scale, dtype=torch.float64) + torch.tensor(bias, dtype=torch.float64) + 1.0)
         * torch.tensor(H.DIMS, dtype=torch.float64) - 1.0) * 0.5
    t = u - i0.double()
    V = 0.0
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                wgt = (t[:, 0] if dx else 1 - t[:, 0]) * (t[:, 1] if dy else 1 - t[:, 1]) * (t[:, 2] if dz else 1 - t[:, 2])
                V = V + wgt * v[i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz]
    (dV,) = torch.autograd.grad(V.sum(), pp)
    assert float((G - dV).abs().max()) <= 2e-5 * float(dV.abs().max())


def _random_ray(S, seed):
    """optical depths x (some 0, as outside the box), cell gradients G (some 0, some tiny) and a unit direction, float64"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(S, generator=g, dtype=torch.float64) * (torch.rand(S, generator=g) < 0.7) * 0.4
    G = torch.randn((S, 3), generator=g, dtype=torch.float64) * (torch.rand(S, generator=g) < 0.9)[:, None]
    G[::5] *= 1e-3
    u = torch.nn.functional.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0)
    return x, G, u


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("S", [1, 2, 37, 96])
def test_closed_form_and_lane_split_equal_the_literal_sum(S, eps):
    """the header's closed-form gradient (through the weights and through the normals) and the kernel's G-lane evaluation (in
    float64) give the literal sum and autograd's gradient to 1e-12"""
    x, G, u = _random_ray(S, 31 + S)
    if S <= 2:
        side = torch.linalg.cross(u, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
        G[:] = (-u + 0.8 * side) * torch.tensor([[1.0], [0.5]], dtype=torch.float64)[:S]      # (the few samples face away, askew)
        x[:] = 0.3
    x.requires_grad_(True)
    G.requires_grad_(True)
    alpha = 1.0 - torch.exp(-x)
    T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1.0 - alpha[:-1]]), dim=0)
    c = OR.facing(G, u, eps)
    L = OR.literal_sum((alpha * T)[None], c[None])[0]
    q_ref, dG_ref = torch.autograd.grad(L, (x, G))
    Lc, qc, dGc = OR.closed_form(x.detach(), G.detach(), u, eps)
    assert abs(float(Lc) - float(L.detach())) < 1e-12
    assert float((qc - q_ref).abs().max()) < 1e-12 and float((dGc - dG_ref).abs().max()) < 1e-12
    assert float(dG_ref.abs().max()) > 1e-3 and bool((dGc[c.detach() == 0] == 0).all())
    for lanes in (1, 2, 4, 8):
        Lg, q = OR.lane_split(x.detach(), c.detach(), lanes)
        assert abs(Lg - float(L.detach())) < 1e-12, lanes
        assert float((q - q_ref).abs().max()) < 1e-12, lanes
    assert float(L.detach()) > 1e-2


def test_lane_split_leaves_exact_zeros_behind_the_last_contributing_sample():
    """samples that carry weight but face the viewer, behind the last one that faces away: their dL/dx is exactly 0 in every
    split, as autograd has it (a suffix taken as total - running sum leaves its rounding there)"""
    S = 41
    g = torch.Generator().manual_seed(2)
    x = torch.rand(S, generator=g, dtype=torch.float64) * 0.1 + 0.01
    c = torch.rand(S, generator=g, dtype=torch.float64)
    c[17:] = 0.0
    for lanes in (1, 2, 4, 8):
        _, q = OR.lane_split(x, c, lanes)
        assert bool((q[17:] == 0).all()) and bool((q[:17] != 0).all()), lanes


# ---- the inputs are well conditioned and not vacuous (oracle probe -> restatement, no device) -------------------------
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("pre,post", ACTS)
@pytest.mark.parametrize("case", agreement_cases(), ids=lambda c: c[0])
def test_agreement_inputs_are_conditioned_and_not_vacuous(case, pre, post, eps):
    spec, params, dens, feat, ro, rd, jitter, rng = agreement_inputs(case, pre, post, CPU)
    z, inside = OR.host_samples(spec, params, dens, feat, ro, rd, jitter, rng)

    def grad_of(dtype, part="both"):
        d = dens.clone().requires_grad_(True)
        L = OR.from_samples(z, inside, d, ro, rd, spec, eps, dtype, part)
        (g,) = torch.autograd.grad(L.mean(), d)
        return L.detach(), g.double()

    L, grad = grad_of(torch.float64)
    _, grad_n = grad_of(torch.float64, "normals")
    _, grad32 = grad_of(torch.float32)
    yard = float((grad32 - grad).norm() / grad.norm())
    print(f"{case[0]} pre {pre} post {post} eps {eps}: R {len(L)}  L_r > 1e-4: {float((L > 1e-4).double().mean()):.3f}  L_r == 0: "
          f"{int((L == 0).sum())}  grad != 0: {int((grad != 0).sum())}  normals part {float(grad_n.norm() / grad.norm()):.3f}  "
          f"loss {float(L.mean()):.6f}  float32 yardstick's gradient rel_l2 {yard:.2e}")
    assert yard <= YARDSTICK_GATE
    assert_agreement_not_vacuous(case, L, grad, grad_n)
    if case[7] == "dense":
        # the face cells carry weight
        p = (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).reshape(-1, 3)
        _, i0, _, _ = normals_ref.index_coords(p, H.DIMS, H.AABB)
        face = ((i0 == -1) | (i0 == torch.tensor(H.DIMS) - 1)).any(dim=1).reshape(z.shape) & inside.bool()
        sigma = DR.sigma_from_raw(dens, p, spec.aabb, spec.density_scale, pre, post).reshape(z.shape)
        w = DR.weights(torch.where(inside.bool(), sigma, torch.zeros_like(sigma)), z, rd)
        assert int((face & (w > 1e-3)).sum()) > 100


def test_ramp_fixture_by_hand():
    """the analytic fixture in the restatement: L_r = u_x^2 * acc_r for the rays towards -x, exactly 0 towards +x"""
    spec, params, dens, feat, ro, rd = ramp_inputs(CPU)
    z, inside = OR.host_samples(spec, params, dens, feat, ro, rd)
    assert bool(inside.bool().all())
    L, grad = OR.loss_and_gradient(OR.orientation_host, spec, params, dens, feat, ro, rd, eps=0.0)
    p = (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).reshape(-1, 3)
    sigma = DR.sigma_from_raw(dens, p, spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act).reshape(z.shape)
    acc = DR.weights(sigma, z, rd).sum(dim=1)
    ux = OR.unit_directions(rd)[:, 0]
    assert float(((L[:36] - ux[:36] ** 2 * acc[:36]).abs() / L[:36]).max()) < 1e-6 and float(L[:36].min()) > 1e-2
    assert bool((L[36:] == 0).all())
    _, grad_pos = OR.loss_and_gradient(OR.orientation_host, spec, params, dens, feat, ro[36:], rd[36:], eps=0.0)
    assert int((grad_pos != 0).sum()) == 0 and int((grad != 0).sum()) > 100


def test_fuzzy_ball_descends_in_the_restatement():
    """the fixture of the GPU descent test in float64 on the host: the far hemisphere weighs (most rays have L_r > 1e-4), Adam on
    the term alone lowers it to the ratio the GPU test is measured against, and no voxel moves further than FUZZY_MAX_MOVE"""
    spec, params, dens, feat, ro, rd = fuzzy_inputs(CPU)
    z, inside = OR.host_samples(spec, params, dens, feat, ro, rd)
    L = OR.from_samples(z, inside, dens, ro, rd, spec)
    assert float((L > 1e-4).double().mean()) > 0.25 and float(L.mean()) > 1e-3
    losses, final = fuzzy_descent(lambda d: OR.from_samples(z, inside, d, ro, rd, spec).mean(), dens, torch.float64)
    ratio, move = losses[-1] / losses[0], float((final - dens.double()).abs().max())
    print(f"fuzzy ball: loss {losses[0]:.6f} -> {losses[-1]:.6f} (ratio {ratio:.4f}) after {FUZZY_STEPS} Adam steps; largest move "
          f"{move:.4f}")
    assert ratio < 0.9
    assert abs(ratio - FUZZY_LOSS_RATIO) <= 1e-3 and abs(move - FUZZY_MAX_MOVE) <= 1e-3 * FUZZY_MAX_MOVE


# ---- trainer options --------------------------------------------------------------------------------------------------
def test_cli_options_trainer_arguments_and_documents():
    spec = importlib.util.spec_from_file_location("train_orient_cli", os.path.join(ROOT, "train_sh_based_voxel_grid_with_posed_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opts = {p.name: p for p in mod.main.params}
    for name, default in (("orientation_weight", 0.0), ("orientation_normal_eps", 1e-2)):
        assert opts[name].default == default and f"--{name}" in opts[name].opts
    from thre3d_atom.modules import trainers

    sig = inspect.signature(trainers.train_sh_vox_grid_vol_mod_with_posed_images)
    assert sig.parameters["orientation_weight"].default == 0.0 and sig.parameters["orientation_normal_eps"].default == 1e-2
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.orientation import orientation_loss_on_rays

    assert callable(orientation_loss_on_rays) and callable(VolumetricModel.orientation_loss)
    assert inspect.signature(orientation_loss_on_rays).parameters["normal_eps"].default == 1e-2
    assert "guard, not a tuned value" in orientation_loss_on_rays.__doc__ and "guard, not a tuned value" in ops.orientation_loss.__doc__
    assert callable(ops.orientation_loss) and callable(ops.orientation_fwd_bwd)
    for doc in ("README.md", "INTEGRATION.md"):
        assert "--orientation_weight" in open(os.path.join(ROOT, doc)).read(), doc
    assert "voxe_orientation.hip" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.20" in design and "profiles/orientation_bench.txt" in design
    assert "voxe_orientation_fwd_bwd" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "orientation_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    # the attention and SDS trainers do not take the term
    from thre3d_atom.modules import attn_grid_trainer, sds_trainer

    for module in (attn_grid_trainer, sds_trainer):
        assert "orientation_weight" not in open(module.__file__).read()


def test_weight_zero_leaves_the_one_call_iteration(tmp_path, monkeypatch):
    """orientation_weight = 0 takes the trainer's code path as it was: the one-call iteration runs (voxe_recon_step through
    FusedGridAdam.reconstruction_step, with its prefetch) and the term is never evaluated; above 0 it is the other way round, and
    the term receives the trainer's normal_eps"""
    from thre3d_atom.modules import trainers
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics

    calls = {"one_call": 0, "prefetch": 0, "orientation": 0, "distortion": 0, "render": 0}
    seen = {}

    class FakeOpt(torch.optim.Optimizer):
        def __init__(self, grid, lr, betas):
            super().__init__(list(grid.parameters()), dict(lr=lr))

        def reconstruction_step(self, *a, **k):
            calls["one_call"] += 1

        def reconstruction_prefetch(self, *a, **k):
            calls["prefetch"] += 1

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

    def fake_orientation(self, rays, **kw):
        calls["orientation"] += 1
        seen.update(kw)
        return self.thre3d_repr.densities.sum() * 0

    def fake_distortion(self, rays, **kw):
        calls["distortion"] += 1
        return self.thre3d_repr.densities.sum() * 0

    monkeypatch.setattr(trainers, "FusedGridAdam", FakeOpt)
    monkeypatch.setattr(trainers, "scale_voxel_grid_with_required_output_size", lambda grid, size: grid)
    monkeypatch.setattr(trainers, "_render_params", lambda *a, **k: None)
    monkeypatch.setattr(trainers, "_next_rng", lambda: (0, 0))
    monkeypatch.setattr(VolumetricModel, "render_rays", fake_render_rays)
    monkeypatch.setattr(VolumetricModel, "orientation_loss", fake_orientation)
    monkeypatch.setattr(VolumetricModel, "distortion_loss", fake_distortion)
    monkeypatch.setattr(trainers, "sample_random_rays_and_pixels_from_cameras",
                        lambda intr, poses, images, n, **k: (type("R", (), {"origins": torch.zeros(16, 3)})(), torch.zeros(16, 3)))

    def run(**kw):
        for k in calls:
            calls[k] = 0
        vg = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.1, 0.1, 0.1), tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(8, CameraBounds(1.0, 4.0)), device=CPU)
        trainers.train_sh_vox_grid_vol_mod_with_posed_images(vm, Data(), tmp_path, num_stages=1, num_iterations_per_stage=3,
                                                             fast_debug_mode=True, **kw)

    run(orientation_weight=0.0)
    assert calls == {"one_call": 3, "prefetch": 2, "orientation": 0, "distortion": 0, "render": 0}, calls
    run(orientation_weight=0.01, orientation_normal_eps=0.25)
    assert calls == {"one_call": 0, "prefetch": 0, "orientation": 3, "distortion": 0, "render": 6}, calls
    assert seen == {"normal_eps": 0.25}
    run(orientation_weight=0.01, distortion_weight=0.01)
    assert calls == {"one_call": 0, "prefetch": 0, "orientation": 3, "distortion": 3, "render": 6}, calls
    assert seen == {"normal_eps": 1e-2}
    for bad in (dict(orientation_weight=-1.0), dict(orientation_weight=0.1, orientation_normal_eps=-1.0),
                dict(orientation_weight=0.1, orientation_normal_eps=float("inf"))):
        with pytest.raises(ValueError, match="orientation"):
            run(**bad)
