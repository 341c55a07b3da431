"""GPU checks of the per-voxel Fisher information (voxe_fisher_rays, ops.fisher_rays_, thre3d_reprs/fisher.py).

The reference is tests/fisher_ref.py: float64 autograd Jacobians, one backward per ray and channel, through
ray_grad_ref.render_from_samples on the device's own probed samples.  The same formulas in float32 are the yardstick of ray_var.
The cases, variants and inputs are tests/test_fisher_host.py's, which shows on the CPU that none of them is vacuous: on the dense
cases a kernel that squared every sample's deposit would miss the reference by 0.24 - 0.85 rel-L2.

Bounds.
  fisher   rel-L2 < 2e-4 against float64: twice the project's 1e-4 gradient bound, because squaring doubles a relative error.
  ray_var  max abs error <= 4 x the float32 restatement's own, floor 1e-6 x the case's largest value (16 float32 ulps of it: a
           per-ray sum of up to a few hundred squared float32 terms cannot be asked for less); the precedent is test_depth_gpu.py.
  tie      fisher of ONE ray against sum_ch (d_densities of voxe_render_bwd for d_colour = e_ch)^2: rel-L2 < 2e-4.
  modes    sum_r ray_var(P) against sum_c P[c] fisher[c]: 1e-5 relative (the same emits, summed in double and in float atomics).

Measured on an MI355X, worst of the ten variants of each case (fisher rel-L2 | ray_var error / its bound at P = 1, at a random P |
sum_r ray_var against sum_c P fisher); the whole log is profiles/fisher_pytest_gpu.log:
  dense8 (R 65)        4.7e-7 | 0.27 0.31 | 2.3e-8      dense12 (R 63)       2.4e-6 | 0.40 0.29 | 9.4e-9
  skip24 (R 65)        7.8e-6 | 0.30 0.27 | 1.3e-8      aniso (R 98)         3.9e-6 | 0.28 0.30 | 7.9e-9
  aniso_jitter (R 63)  6.5e-6 | 0.37 0.27 | 9.2e-9      dense12_clip (R 65)  1.7e-6 | 0.34 0.36 | 9.8e-9
  lattice_row (R 25)   1.9e-7 | 0.27 0.22 | 2.5e-8      lattice_tie (R 49)   2.0e-6 | 0.33 0.27 | 1.2e-8
  diagonal (R 49)      1.2e-6 | 0.30 0.28 | 1.2e-8      single (R 1)         1.5e-6 | 0.46 0.28 | 4.5e-8
  all_miss (R 17)      exact zeros
tie to voxe_render_bwd (ten single rays, the route asserted through voxe_render_route), worst rel-L2 over the three variants:
  plain scatter 2.3e-5   line-dense scatter 1.7e-5   LDS window 1.7e-5   space-binned 6.7e-6   deterministic 1.7e-5"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fisher_ref as FR
import ray_grad_ref as RG
import test_fisher_host as T
import test_visibility_host as H
from voxe_hip import abi, dispatch, ops, workload

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FISHER_TOL = T.FISHER_TOL
MODES_TOL = 1e-5


def _rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _run(spec, params, dens, feat, ro, rd, jitter=None, rng=(0, 0), fisher=True, voxel_var=None, ray_var=False, into=None):
    """(fisher [X,Y,Z] or None, ray_var [R] or None) of one call"""
    buf = into if into is not None else (torch.zeros(dens.shape[:3], device=DEV) if fisher else None)
    rv = ops.fisher_rays_(spec, params, dens, feat, ro, rd, fisher=buf, voxel_var=voxel_var, want_ray_var=ray_var, jitter=jitter, rng=rng)
    return buf, rv


@functools.lru_cache(maxsize=None)
def _reference(case_name, variant):
    """(inputs, J float64, J float32, probed samples) of one case under one variant, computed once"""
    inp = T.inputs(T.case_named(case_name), variant, DEV)
    spec, params, dens, feat, ro, rd, jitter, rng = inp
    samples = RG.probe_device(spec, params, dens, feat, ro, rd, jitter, rng)
    J64 = FR.jacobians(samples, dens, feat, ro, rd, spec, params)
    J32 = FR.jacobians(samples, dens, feat, ro, rd, spec, params, dtype=torch.float32)
    return inp, J64, J32, samples


# ---- 1, 2, 4: agreement with the restatement, both modes ---------------------------------------------------------------
@pytest.mark.parametrize("variant", T.variants(), ids=T.variant_id)
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c[0])
def test_fisher_and_ray_var_match_the_restatement(case, variant):
    (spec, params, dens, feat, ro, rd, jitter, rng), J64, J32, samples = _reference(case[0], variant)
    R = ro.shape[0]
    P = T.voxel_var(dens.shape[:3], DEV)
    H64 = FR.fisher_of(J64)
    fisher, rv1 = _run(spec, params, dens, feat, ro, rd, jitter, rng, ray_var=True)                 # both outputs, P = NULL
    _, rvP = _run(spec, params, dens, feat, ro, rd, jitter, rng, fisher=False, voxel_var=P, ray_var=True)
    _, rvP2 = _run(spec, params, dens, feat, ro, rd, jitter, rng, fisher=False, voxel_var=P, ray_var=True)
    fisher_only, none = _run(spec, params, dens, feat, ro, rd, jitter, rng)
    assert none is None and bool(torch.isfinite(fisher).all()) and bool(torch.isfinite(rvP).all())
    # 2 (part): the same bits on every run
    assert torch.equal(rvP, rvP2)
    missed = ~samples[1].bool().any(dim=1)
    assert bool((rv1[missed] == 0).all()) and bool((rvP[missed] == 0).all())
    if case[0] == "all_miss":
        assert int(fisher.count_nonzero()) == 0 and int(rv1.count_nonzero()) == 0 and int(H64.count_nonzero()) == 0
        return
    # 1: fisher
    err = _rel_l2(fisher, H64)
    err_only = _rel_l2(fisher_only, H64)
    zeros = (H64 == 0).reshape(fisher.shape)
    stray = int((fisher[zeros] != 0).sum())
    # 2: ray_var, P = 1 and a random P
    lines = []
    for name, got, Pv in (("P=1", rv1, None), ("P", rvP, P)):
        want = FR.ray_var_of(J64, Pv)
        yard = float((FR.ray_var_of(J32, Pv).double() - want).abs().max())
        bound = max(4.0 * yard, 1e-6 * float(want.max()))
        e = float((got.double() - want).abs().max())
        lines.append((name, e, yard, bound, float(want.max())))
    # 4: two modes, one Jacobian
    modes1 = abs(float(rv1.double().sum()) - float(fisher.double().sum())) / float(fisher.double().sum())
    modesP = abs(float(rvP.double().sum()) - float((P.double() * fisher.double()).sum())) / float((P.double() * fisher.double()).sum())
    print(f"{case[0]} {T.variant_id(variant)}: R {R}  fisher rel_l2 {err:.2e} (alone {err_only:.2e})  stray non-zeros {stray}  "
          + "  ".join(f"ray_var[{n}] err {e:.2e} f32 torch {y:.2e} bound {b:.2e} max {m:.2e}" for n, e, y, b, m in lines)
          + f"  modes {modes1:.1e} {modesP:.1e}")
    assert err < FISHER_TOL and err_only < FISHER_TOL
    assert stray == 0 and int(zeros.sum()) > 0
    for name, e, yard, bound, _ in lines:
        assert e <= bound, (name, e, yard, bound)
    assert modes1 <= MODES_TOL and modesP <= MODES_TOL


# ---- 3: the tie to the shipped backward --------------------------------------------------------------------------------
# every backward route the binding can pin for a one-ray launch: name -> (RenderParams fields, the route voxe_render_route must
# report).  A 1 x 1 image gives the image-ordered routes their order; the space-binned route takes unordered rays from
# region_min_rays on; the deterministic route has one channel group: SH degree 0 or the diffuse flag
ROUTES = {"scatter": (dict(dispatch=dispatch.Dispatch(bwd_mode=1)), abi.ROUTE_SCATTER),
          "line_dense": (dict(dispatch=dispatch.Dispatch(bwd_mode=2)), abi.ROUTE_PACKED_SCATTER),
          "tile": (dict(image_width=1, dispatch=dispatch.Dispatch(tile_min_rays=-1)), abi.ROUTE_TILE),
          "region": (dict(image_width=0, dispatch=dispatch.Dispatch(region_min_rays=1)), abi.ROUTE_REGION),
          "deterministic": (dict(image_width=1, deterministic=True), abi.ROUTE_DETERMINISTIC)}
TIE_VARIANTS = [T.variants()[1], T.variants()[7], T.variants()[4]]          # sh2 | abs + ReLU, white, sh0 | sh2 diffuse, white
TIE = [(v, r) for v in TIE_VARIANTS for r in sorted(ROUTES) if r != "deterministic" or v[3] == 0 or v[4]]


@pytest.mark.parametrize("variant,route", TIE, ids=lambda x: x if isinstance(x, str) else T.variant_id(x))
def test_single_ray_fisher_is_the_squared_gradient_of_the_shipped_backward(variant, route):
    """R = 1 launches: fisher = sum_ch (d_densities of voxe_render_bwd with d_colour = e_ch, no depth / acc gradient)^2"""
    import dataclasses

    spec, params, dens, feat, _, _, _, _ = T.inputs(T.case_named("aniso"), variant, DEV)
    params = dataclasses.replace(params, image_width=0, image_height=0)
    ros, rds = T.single_rays(DEV)
    fields, want_route = ROUTES[route]
    pinned = dataclasses.replace(params, **fields)
    # the launch takes the route it is named after (a changed threshold must not quietly turn the routes into one)
    g, c = ops._descs(spec, pinned, dens, feat, 0, 0, False)
    assert ops._route(g, c, 1) == want_route
    worst, touched = 0.0, 0
    for i in range(ros.shape[0]):
        ro, rd = ros[i:i + 1].contiguous(), rds[i:i + 1].contiguous()
        fisher, _ = _run(spec, params, dens, feat, ro, rd)
        want = torch.zeros_like(fisher, dtype=torch.float64)
        for ch in range(3):
            d = dens.clone().requires_grad_(True)
            colour = ops.render(spec, pinned, d, feat, ro, rd, workspace=ops.Workspace())[0]
            (g,) = torch.autograd.grad(colour[0, ch], d)
            want += g[..., 0].double() ** 2
        touched += int(want.count_nonzero())
        worst = max(worst, _rel_l2(fisher, want))
    print(f"{T.variant_id(variant)} {route}: worst rel_l2 over {ros.shape[0]} single rays {worst:.2e}; {touched} voxels touched")
    assert touched > 300 and worst < FISHER_TOL


# ---- 5: batch independence ---------------------------------------------------------------------------------------------
def test_launch_split_and_ray_order_do_not_matter():
    variant = T.variants()[3]
    spec, params, dens, feat, ro, rd, _, _ = T.inputs(T.case_named("aniso"), variant, DEV)      # two 7 x 7 cameras, image order
    P = T.voxel_var(dens.shape[:3], DEV)
    whole, rv = _run(spec, params, dens, feat, ro, rd, voxel_var=P, ray_var=True)
    import dataclasses

    one = dataclasses.replace(params, image_height=0)
    parts = torch.zeros_like(whole)
    rvs = []
    for k in range(2):
        sl = slice(49 * k, 49 * (k + 1))
        rvs.append(_run(spec, one, dens, feat, ro[sl].contiguous(), rd[sl].contiguous(), voxel_var=P, ray_var=True, into=parts)[1])
    perm = torch.randperm(ro.shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)
    flat = dataclasses.replace(params, image_width=0, image_height=0)
    shuffled, rv_s = _run(spec, flat, dens, feat, ro[perm].contiguous(), rd[perm].contiguous(), voxel_var=P, ray_var=True)
    assert _rel_l2(parts, whole) < 2 * FISHER_TOL and _rel_l2(shuffled, whole) < 2 * FISHER_TOL and float(whole.max()) > 0
    assert torch.equal(torch.cat(rvs), rv) and torch.equal(rv_s, rv[perm])


# ---- 6, 7: semantics and error codes -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return T.inputs(T.case_named("dense12"), T.variants()[3], DEV)


def test_fisher_accumulates_and_ray_var_is_overwritten(base):
    spec, params, dens, feat, ro, rd, jitter, rng = base
    fresh, _ = _run(spec, params, dens, feat, ro, rd)
    start = torch.rand(dens.shape[:3], generator=torch.Generator().manual_seed(1)).to(DEV) * float(fresh.max())
    on_top, _ = _run(spec, params, dens, feat, ro, rd, into=start.clone())
    assert _rel_l2(on_top - start, fresh) < 1e-5 and float(fresh.max()) > 0
    untouched = fresh == 0
    assert int(untouched.sum()) > 0 and torch.equal(on_top[untouched], start[untouched])
    # ray_var: what the buffer held before does not matter (the binding hands the call an uninitialised tensor; the contract test
    # below poisons it)
    _, a = _run(spec, params, dens, feat, ro, rd, fisher=False, ray_var=True)
    _, b = _run(spec, params, dens, feat, ro, rd, fisher=False, ray_var=True)
    assert torch.equal(a, b) and float(a.max()) > 0


def test_null_outputs_and_no_rays(base):
    from voxe_hip.desc import make_grid_desc, make_render_cfg
    from voxe_hip.runtime import lib, stream_ptr

    spec, params, dens, feat, ro, rd, jitter, rng = base
    L, st = lib(), stream_ptr(DEV)
    R, nvox = ro.shape[0], dens.numel()
    g = make_grid_desc(dens.data_ptr(), feat.data_ptr(), tuple(int(n) for n in dens.shape[:3]), int(feat.shape[-1]), spec.aabb, spec.density_scale, spec.density_pre_act,
                       spec.density_post_act)
    c = make_render_cfg(params.num_samples, params.near, params.far, white_bkgd=params.white_bkgd, sh_degree=params.sh_degree)
    fisher = torch.full((nvox,), 7.0, device=DEV)
    ray = torch.full((R,), 7.0, device=DEV)
    P = torch.ones(nvox, device=DEV)

    def call(R_=R, f=None, p=None, r=None, ro_=ro.data_ptr(), rd_=rd.data_ptr()):
        status = L.voxe_fisher_rays(C.byref(g), C.byref(c), ro_, rd_, R_, None, f, p, r, st)
        torch.cuda.synchronize()
        return status

    # both outputs NULL (with or without voxel_var), R == 0 (rays may be NULL): VOXE_OK and nothing is written
    assert call() == abi.OK and call(p=P.data_ptr()) == abi.OK
    assert call(R_=0, f=fisher.data_ptr(), p=P.data_ptr(), r=ray.data_ptr(), ro_=None, rd_=None) == abi.OK
    assert bool((fisher == 7.0).all()) and bool((ray == 7.0).all())
    # fisher alone leaves ray_var's buffer alone, and the other way round; voxel_var is ignored without ray_var
    assert call(f=fisher.data_ptr(), p=None) == abi.OK and bool((ray == 7.0).all()) and float(fisher.max()) > 7.0
    before = fisher.clone()
    assert call(r=ray.data_ptr()) == abi.OK and torch.equal(fisher, before) and not bool((ray == 7.0).any())
    ones = ray.clone()
    assert call(p=P.data_ptr(), r=ray.data_ptr()) == abi.OK and torch.equal(ray, ones)             # P = 1 is P = NULL
    # 7: error codes with real pointers (tests/test_fisher_host.py walks the whole table without a device)
    assert call(R_=-1, f=fisher.data_ptr()) == abi.ERR_BAD_SHAPE
    assert call(f=fisher.data_ptr(), ro_=None) == abi.ERR_NULL_POINTER
    c.sh_degree = 1
    assert call(f=fisher.data_ptr()) == abi.ERR_BAD_SHAPE
    c.sh_degree = 5
    assert call(f=fisher.data_ptr()) == abi.ERR_UNSUPPORTED
    c.sh_degree = params.sh_degree
    g.feature_kind = abi.FEAT_ATTN
    assert call(f=fisher.data_ptr()) == abi.ERR_UNSUPPORTED
    g.feature_kind = abi.FEAT_SH
    g.features = 0
    assert call(f=fisher.data_ptr()) == abi.ERR_NULL_POINTER
    assert torch.equal(fisher, before)


def test_operator_checks_its_buffers(base):
    from voxe_hip.runtime import VoxeError

    spec, params, dens, feat, ro, rd, jitter, rng = base
    for bad in (torch.zeros(dens.shape[:3], dtype=torch.float64, device=DEV), torch.zeros((5, 5, 5), device=DEV),
                torch.zeros(dens.shape[:3])):
        with pytest.raises(VoxeError):
            ops.fisher_rays_(spec, params, dens, feat, ro, rd, fisher=bad)
    with pytest.raises(VoxeError):
        ops.fisher_rays_(spec, params, dens, feat, ro, rd, voxel_var=torch.zeros((5, 5, 5), device=DEV), want_ray_var=True)
    assert ops.fisher_rays_(spec, params, dens, feat, ro, rd) is None                                # neither output: no launch
    four = torch.zeros(dens.shape, device=DEV)                                                       # [X,Y,Z,1] is accepted
    ops.fisher_rays_(spec, params, dens, feat, ro, rd, fisher=four)
    assert float(four.max()) > 0


# ---- 8: the buffer contract (tests/contract.py, tests/arena.py) ----------------------------------------------------------
def fisher_case(k, name, mode):
    from contract import P as ptr_of
    from voxe_hip.runtime import lib, stream_ptr
    import test_buffer_contract_gpu as BC

    L, sc, st = lib(), BC.scene(name), stream_ptr(DEV)
    R = sc.R
    dens, feat = k.inp("densities", sc.dens), k.inp("features", sc.feat)
    ro, rd = k.inp("rays_o", sc.ro), k.inp("rays_d", sc.rd)
    var = k.inp("voxel_var", T.voxel_var(sc.dims, "cpu").numpy())
    g, c = sc.desc(dens.ptr, feat.ptr), sc.cfg()
    fisher = k.inout("fisher", np.zeros(sc.nvox, np.float32)) if mode != "gather" else None
    ray = k.out("ray_var", R) if mode != "accumulate" else None
    k.begin()
    k.call(L.voxe_fisher_rays, C.byref(g), C.byref(c), ro.ptr, rd.ptr, k.count(R), None, ptr_of(fisher), var.ptr, ptr_of(ray), st)
    if ray is not None:
        k.bits(ray)
        assert float(ray.t.max()) > 0
    if fisher is not None:
        k.pair(fisher, 2 * FISHER_TOL)
        assert float(fisher.t.max()) > 0
    if mode == "both":
        a = float(ray.t.double().sum())
        b = float((var.t.double() * fisher.t.double()).sum())
        assert abs(a - b) <= MODES_TOL * b, (a, b)


@pytest.mark.parametrize("name,mode", [("packed_scatter", "both"), ("tile_sh2_tiny", "both"), ("tile_sh3_views", "gather"),
                                       ("views_tile", "accumulate")])
def test_buffer_contract(name, mode):
    from contract import run_contract

    run_contract(fisher_case, name, mode)


def test_buffer_contract_no_rays():
    from contract import run_empty

    run_empty(fisher_case, "packed_scatter", "both")


def test_no_interference_with_a_forward_and_its_deterministic_backward():
    g = torch.Generator().manual_seed(8)
    dens0 = torch.empty((40, 40, 40, 1)).uniform_(-1, 1, generator=g).to(DEV)
    feat0 = torch.empty((40, 40, 40, 3)).uniform_(-1, 1, generator=g).to(DEV)
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=3.0)
    ro, rd = H.cameras(64, 1, DEV)
    params = ops.RenderParams(num_samples=64, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, image_width=64,
                              deterministic=True)
    g_col = torch.rand((ro.shape[0], 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    grads = []
    for with_call in (False, True):
        d, f = dens0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
        ws = ops.Workspace()
        col = ops.render(spec, params, d, f, ro, rd, workspace=ws, rng=(3, 4))[0]
        if with_call:
            fisher, rv = _run(spec, params, d, f, ro, rd, rng=(3, 4), ray_var=True)
            assert float(fisher.max()) > 0 and float(rv.max()) > 0
        (col * g_col).sum().backward()
        grads.append((col.detach().clone(), d.grad.clone(), f.grad.clone()))
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    assert float(grads[0][1].abs().max()) > 0


# ---- 9: the library layer --------------------------------------------------------------------------------------------------
def _scene_model():
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelGridLocation, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics, pose_spherical

    spec, params, dens, feat = T.scene_inputs(DEV)
    side, centre, aabb = T.scene_geometry()
    vg = VoxelGrid(dens, feat, VoxelSize(*side), VoxelGridLocation(*centre), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=T.SCENE_SCALE, tunable=True)
    assert vg.voxe_grid_spec() == spec
    vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(T.SCENE_S, CameraBounds(H.BALL_NEAR, H.BALL_FAR)), device=DEV)
    intr = CameraIntrinsics(T.SCENE_HW, T.SCENE_HW, workload.focal_for(T.SCENE_HW))
    pose = lambda yaw: pose_spherical(yaw, T.SCENE_PITCH, H.BALL_RADIUS)      # noqa: E731
    return vm, intr, [pose(y) for y in T.SCENE_TRAIN_YAWS], [pose(y) for y in T.SCENE_CANDIDATE_YAWS]


def test_library_layer_prefers_the_unseen_side():
    from thre3d_atom.thre3d_reprs import fisher as F

    vm, intr, train, cands = _scene_model()
    spec, params, dens, feat = T.scene_inputs(DEV)
    total = F.accumulate_fisher(vm, train, intr)
    # one launch per camera over the kernel's own rays: the same grid as the operator on test_fisher_host.scene_rays
    by_hand = torch.zeros_like(total)
    for yaw in T.SCENE_TRAIN_YAWS:
        ro, rd = T.scene_rays(yaw, DEV)
        ops.fisher_rays_(spec, params, dens, feat, ro, rd, fisher=by_hand)
    assert _rel_l2(total, by_hand) < 2 * FISHER_TOL and total.shape == T.SCENE_DIMS and total.dtype == torch.float32
    lam = F.default_prior_precision(total)
    assert lam == pytest.approx(1e-6 * float(total.max()))
    near_map, far_map = (F.uncertainty_map(vm, p, intr, total) for p in cands)
    assert near_map.shape == (T.SCENE_HW, T.SCENE_HW)
    gains = [F.information_gain(vm, p, intr, total) for p in cands]
    assert gains[0] == pytest.approx(float(near_map.double().sum())) and gains[1] == pytest.approx(float(far_map.double().sum()))
    # gain == sum_v H_candidate / (H_train + lambda)
    for p, gain in zip(cands, gains):
        Hc = F.accumulate_fisher(vm, [p], intr)
        assert gain == pytest.approx(float((Hc.double() / (total.double() + lam)).sum()), rel=1e-4)
    print(f"gain near side {gains[0]:.4g}  far side {gains[1]:.4g}  ratio {gains[1] / gains[0]:.2f}")
    assert gains[1] >= T.SCENE_MIN_RATIO * gains[0] > 0
    # pixels: the unseen side is the less certain one, and a ray that misses the grid has variance exactly 0
    hit_near, hit_far = near_map > 0, far_map > 0
    assert float(far_map[hit_far].mean()) > float(near_map[hit_near].mean()) > 0
    for yaw, m in zip(T.SCENE_CANDIDATE_YAWS, (near_map, far_map)):
        ro, rd = T.scene_rays(yaw, DEV)
        inside = RG.probe_device(spec, params, dens, feat, ro, rd)[1].bool().any(dim=1).reshape(m.shape)
        assert int((~inside).sum()) >= 4 and bool((m[~inside] == 0).all())
    sel = F.select_next_views(vm, train, cands, intr, 2)
    assert sel.indices == [1, 0] and sel.gains[0] == pytest.approx(gains[1], rel=1e-4)
    assert sel.gains_after[0] < sel.gains[0]                                  # its own information is in the total now
    assert sel.rounds[0] == pytest.approx(gains, rel=1e-4) and sel.rounds[1][1] != sel.rounds[1][1]


def test_select_next_views_command_line(tmp_path):
    """the entry point end to end on the view-selection scene: a saved checkpoint, a dataset directory whose training cameras are
    read back through visibility_cameras, candidates from a camera file and from the checkpoint's 360 degree path, the real
    ray casting and kernel calls"""
    import importlib.util
    import json
    import os

    from click.testing import CliRunner
    from PIL import Image

    from conftest import ROOT
    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.thre3d_reprs import fisher as F
    from thre3d_atom.thre3d_reprs.poses import write_camera_params
    from thre3d_atom.utils.constants import CAMERA_BOUNDS, CAMERA_INTRINSICS, HEMISPHERICAL_RADIUS
    from thre3d_atom.utils.imaging_utils import CameraBounds

    vm, intr, train, cands = _scene_model()
    bounds = CameraBounds(H.BALL_NEAR, H.BALL_FAR)
    torch.save(vm.get_save_info({CAMERA_BOUNDS: bounds, CAMERA_INTRINSICS: intr, HEMISPHERICAL_RADIUS: H.BALL_RADIUS}), tmp_path / "model.pth")
    (tmp_path / "data" / "train").mkdir(parents=True)

    def stack(poses):
        return torch.stack([torch.cat([torch.as_tensor(p.rotation), torch.as_tensor(p.translation).reshape(3, 1)], dim=1) for p in poses]).cpu()

    blank = np.zeros((T.SCENE_HW, T.SCENE_HW, 3), np.uint8)
    for i in range(len(train)):
        Image.fromarray(blank).save(tmp_path / "data" / "train" / f"{i:04d}.png")
    for name, poses in (("data/train_camera_params.json", train), ("candidates_camera_params.json", cands)):
        images = torch.zeros((len(poses), 3, T.SCENE_HW, T.SCENE_HW))
        write_camera_params(tmp_path / name, InMemoryPosedImages(images, stack(poses), intr, bounds), stack(poses))
    spec = importlib.util.spec_from_file_location("select_next_views_gpu_cli", os.path.join(ROOT, "select_next_views.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["-i", str(tmp_path / "model.pth"), "-d", str(tmp_path / "data")]
    res = CliRunner().invoke(mod.main, base + ["-o", str(tmp_path / "file"), "--candidates", str(tmp_path / "candidates_camera_params.json"),
                                               "--num_select", "2", "--uncertainty_maps"])
    assert res.exit_code == 0, (res.output, res.exception)
    rep = json.loads((tmp_path / "file" / "next_views.json").read_text())
    total = F.accumulate_fisher(vm, train, intr)
    want = [F.information_gain(vm, p, intr, total) for p in cands]
    assert rep["num_train_views"] == len(train) and rep["num_candidates"] == 2
    assert rep["prior_precision"] == pytest.approx(1e-6 * float(total.max()), rel=1e-4)
    assert [s["candidate"] for s in rep["selected"]] == [1, 0] and rep["rounds"][0]["gains"] == pytest.approx(want, rel=1e-3)
    assert rep["selected"][0]["gain_after"] < rep["selected"][0]["gain"]
    assert np.allclose(rep["selected"][0]["extrinsic"]["translation"], np.asarray(torch.as_tensor(cands[1].translation).cpu()).reshape(3, 1),
                       atol=1e-5)
    saved = torch.load(tmp_path / "file" / "fisher.pth")
    assert _rel_l2(saved["fisher"].to(DEV), total) < 2 * FISHER_TOL
    for n in range(2):
        assert Image.open(tmp_path / "file" / f"uncertainty_{n:04d}.png").size == (2 * T.SCENE_HW, T.SCENE_HW)
    # the checkpoint's own 360 degree path
    res = CliRunner().invoke(mod.main, base + ["-o", str(tmp_path / "path"), "--num_candidates", "4", "--camera_pitch", str(T.SCENE_PITCH),
                                               "--num_select", "1", "--prior_precision", "1e-12"])
    assert res.exit_code == 0, (res.output, res.exception)
    rep = json.loads((tmp_path / "path" / "next_views.json").read_text())
    from thre3d_atom.utils.imaging_utils import get_thre360_animation_poses

    ring = list(get_thre360_animation_poses(H.BALL_RADIUS, T.SCENE_PITCH, 5))
    want = [F.information_gain(vm, p, intr, total, 1e-12) for p in ring]
    best = max(range(4), key=lambda i: want[i])
    assert rep["num_candidates"] == 4 and rep["prior_precision"] == 1e-12
    assert rep["rounds"][0]["gains"] == pytest.approx(want, rel=1e-3)
    assert rep["selected"][0]["candidate"] == best and rep["selected"][0]["name"] == f"thre360_{best:04d}"
