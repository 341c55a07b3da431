"""CPU checks of the per-voxel Fisher information: the C ABI's declarations and argument validation (no device work), the float64
restatement tests/fisher_ref.py against the header's closed form, the greedy view selection on hand-made grids, the entry
point's options and JSON schema with the kernel calls replaced, and -- with the oracle's sample probe feeding the restatement --
that every input of the GPU tests (tests/test_fisher_gpu.py builds them with the functions below) is not vacuous.

What "not vacuous" means here.  The kernel under test carries a voxel's sum along the ray and squares it once; the cheap
alternative squares every sample's deposit.  An input on which both give the same number says nothing, so on the dense cases
the per-sample-squares variant of fisher_ref must miss the restatement by more than 10 x the GPU tolerance (it misses by 0.3 -
0.9 rel-L2, printed).  The carry rule has its branches -- one, two and three axes changing at once, jumps of more than one cell,
footprint corners outside the grid -- and the case list must reach each of them (counts printed)."""
import ctypes
import importlib.util
import inspect
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import degenerate_cases as DC
import fisher_ref as FR
import ray_grad_ref as RG
import test_visibility_host as H
from conftest import ROOT
from voxe_hip import abi, ops, workload
from voxe_hip.desc import make_grid_desc, make_render_cfg

CPU = torch.device("cpu")
ACTS = H.ACTS
FISHER_TOL = 2e-4           # rel-L2 of fisher against float64: twice the project's 1e-4 gradient bound (squaring doubles a relative error)
CUBE = ((-1.5, 1.5),) * 3


# ---- inputs shared with the GPU tests ---------------------------------------------------------------------------------
def variants():
    """(pre, post, white, sh_degree, diffuse): both activation pairs x white on / off x degree 0 / 2, plus the diffuse flag on
    a degree-2 grid"""
    out = []
    for pre, post in ACTS:
        for white in (False, True):
            for deg in (0, 2):
                out.append((pre, post, white, deg, False))
        out.append((pre, post, True, 2, True))
    return out


def variant_id(v):
    return f"pre{v[0]}post{v[1]}-{'white' if v[2] else 'black'}-sh{v[3]}{'-diffuse' if v[4] else ''}"


# (name, dims, aabb, S, rays, R, dense): `rays` names the builder below; `dense` = the per-sample-squares variant must be far off
CASES = [
    ("dense8", (8, 8, 8), CUBE, 64, "camera", 65, True),              # many samples per cell
    ("dense12", (12, 12, 12), CUBE, 24, "camera+miss", 63, True),     # ~1 sample per cell; 8 rays look away from the grid
    ("skip24", (24, 24, 24), CUBE, 8, "camera", 65, False),           # 5 cells per sample: jumps
    ("aniso", H.DIMS, H.AABB, 40, "views", 98, True),                 # 26 x 20 x 23, two 7 x 7 cameras in image order
    ("aniso_jitter", H.DIMS, H.AABB, 40, "camera", 63, True),         # the in-kernel jitter stream
    ("dense12_clip", (12, 12, 12), CUBE, 24, "camera", 65, True),     # aabb_clip: per-ray bounds
    ("lattice_row", None, None, None, "row_image", 25, False),        # axis-aligned rays, samples exactly on voxel planes
    ("lattice_tie", None, None, None, "tie_xy", 49, False),           # two march axes tie exactly
    ("diagonal", None, None, None, "tie_xyz", 49, False),             # rays along the cell diagonals
    ("all_miss", None, None, None, "all_miss", 17, False),            # no ray meets the grid
    ("single", (8, 8, 8), CUBE, 64, "camera_centre", 1, True),        # R = 1
]


def case_named(name):
    return next(c for c in CASES if c[0] == name)


def _features(dims, deg, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.empty((*dims, 3 * (deg + 1) ** 2)).uniform_(-1, 1, generator=g)


def inputs(case, variant, device):
    """(spec, params, densities, features, rays_o, rays_d, jitter, rng) of one case under one variant"""
    name, dims, aabb, S, kind, R, _ = case
    pre, post, white, deg, diffuse = variant
    jitter, rng, perturb, clip, width, height = None, (0, 0), False, False, 0, 0
    if kind in ("row_image", "tie_xy", "tie_xyz", "all_miss"):
        c = DC.case(kind)
        o, d = DC.rays(c)
        n = o.shape[0]
        pick = np.arange(n) if n == R else np.arange(0, n, {"tie_xy": 6, "tie_xyz": 6, "all_miss": 25}[kind])
        assert len(pick) == R and (kind not in ("tie_xy", "tie_xyz") or (n // 2) in pick)      # (the central ray is among them)
        ro, rd = torch.from_numpy(o[pick].copy()).to(device), torch.from_numpy(d[pick].copy()).to(device)
        dens = torch.from_numpy(c.grid.densities.copy())
        dims, aabb, S = tuple(dens.shape[:3]), tuple(tuple(float(v) for v in r) for r in c.grid.aabb), c.S
        near, far = c.near, c.far
    else:
        g = torch.Generator().manual_seed(len(name) + 10 * pre + post)
        dens = torch.empty((*dims, 1)).uniform_(-1, 1, generator=g) * 1.5
        near, far = workload.NEAR, workload.FAR
        if kind == "views":
            ro, rd = H.cameras(7, 2, device)
            width = height = 7
        else:
            ro, rd = H.cast(9, *workload.synth_pose_angles(3, 8), workload.RADIUS, device)
            if kind == "camera_centre":
                ro, rd = ro[40:41].contiguous(), rd[40:41].contiguous()
            elif kind == "camera+miss":
                ro, rd = torch.cat([ro[:R - 8], ro[:8]]).contiguous(), torch.cat([rd[:R - 8], -rd[:8]]).contiguous()
            else:
                ro, rd = ro[:R].contiguous(), rd[:R].contiguous()
        if name == "aniso_jitter":
            perturb, rng = True, (1234, 77)
        clip = name == "dense12_clip"
    assert ro.shape[0] == R
    spec = ops.GridSpec(aabb=aabb, density_scale=2.0, density_pre_act=pre, density_post_act=post)
    params = ops.RenderParams(num_samples=S, near=near, far=far, perturb=perturb, aabb_clip=clip, white_bkgd=white, sh_degree=deg,
                              render_diffuse=diffuse, image_width=width, image_height=height)
    return spec, params, dens.to(device), _features(dims, deg, 7 + deg).to(device), ro, rd, jitter, rng


def voxel_var(dims, device):
    """a random positive P [X,Y,Z] over three decades"""
    g = torch.Generator().manual_seed(int(np.prod(dims)))
    return torch.exp(torch.empty(dims).uniform_(-3.0, 3.0, generator=g)).to(device)


def single_rays(device):
    """the ten single rays of the tie to the shipped backward: spread over the 26 x 20 x 23 grid's first camera"""
    ro, rd = H.cameras(12, 1, device)
    pick = torch.tensor([5, 18, 31, 44, 57, 66, 77, 90, 103, 130], device=ro.device)
    return ro[pick].contiguous(), rd[pick].contiguous()


# The view-selection scene: a fuzzy ball (test_visibility_host.ball_field at every second voxel, v = 10 (r0 - dist) under a
# Softplus: opaque through the middle, soft at the rim), five training cameras 15 degrees apart on one side, two candidates.
# The training cameras have to be that close: with the default prior precision a voxel NO training ray crosses weighs 1e6 times
# a well-seen one, so a candidate between two sparse cameras gains from the gaps between their rays as much as the far side
# does from the occluded half (float64 restatement, 8 x 8 pixels, three cameras 40 degrees apart: ratio 0.7; this layout: 31)
SCENE_DIMS = (35, 29, 32)
SCENE_SCALE = 0.25
SCENE_HW, SCENE_S = 12, 96
SCENE_PITCH = 70.0
SCENE_TRAIN_YAWS = (-30.0, -15.0, 0.0, 15.0, 30.0)
SCENE_CANDIDATE_YAWS = (5.0, 180.0)           # index 0: among the training cameras; index 1: the far side
SCENE_MIN_RATIO = 2.0


def scene_geometry():
    """(voxel sizes, centre, aabb as VoxelGrid derives it: centre -/+ count * edge / 2)"""
    side = [(hi - lo) / n for (lo, hi), n in zip(H.BALL_AABB, SCENE_DIMS)]
    centre = [(lo + hi) / 2 for lo, hi in H.BALL_AABB]
    aabb = tuple((c - (n * e) / 2, c + (n * e) / 2) for c, e, n in zip(centre, side, SCENE_DIMS))
    return side, centre, aabb


def scene_inputs(device):
    """(spec, params, densities, features) of the scene"""
    dens = H.ball_field()[0][::2, ::2, ::2].contiguous()
    assert tuple(dens.shape[:3]) == SCENE_DIMS
    spec = ops.GridSpec(aabb=scene_geometry()[2], density_scale=SCENE_SCALE, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    params = ops.RenderParams(num_samples=SCENE_S, near=H.BALL_NEAR, far=H.BALL_FAR, image_width=SCENE_HW)
    return spec, params, dens.to(device), _features(SCENE_DIMS, 0, 5).to(device)


def scene_rays(yaw, device):
    return H.cast(SCENE_HW, yaw, SCENE_PITCH, H.BALL_RADIUS, device)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


NAMES = ["grid", "cfg", "rays_o", "rays_d", "R", "jitter", "fisher", "voxel_var", "ray_var", "stream"]


def test_fisher_symbol_is_declared_with_no_cpu_twin_and_abi_13():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    L = _lib()
    assert re.search(r"\bvoxe_fisher_rays\s*\(", text) and "voxe_fisher_rays" in abi.hip_symbols() and hasattr(L, "voxe_fisher_rays")
    assert not re.search(r"\bvoxe_cpu_\w*fisher", text) and not any("fisher" in s for s in abi.cpu_symbols())
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text and L.voxe_abi_version() == 13
    assert "voxe_fisher.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    proto = re.search(r"int voxe_fisher_rays\((.*?)\);", text, re.S).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == NAMES
    argtypes = L.voxe_fisher_rays.argtypes
    assert len(argtypes) == len(NAMES) and argtypes[4] is ctypes.c_int64
    src = inspect.getsource(ops.fisher_rays_)
    assert re.search(r"voxe_fisher_rays\(C\.byref\(g\), C\.byref\(c\), ptr\(ro\), ptr\(rd\), R, ptr\(jit\), ptr\(fisher\)", src)
    # the definition is in the header
    assert "fisher[c]  += sum_ch J_{r,ch}[c]^2" in text and "ray_var[r]  = sum_c P[c] sum_ch J_{r,ch}[c]^2" in text


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    g = make_grid_desc(16, 16, (8, 6, 5), 3, H.AABB, 1.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)
    c = make_render_cfg(32, 1.0, 4.0)

    def call(g_=g, c_=c, ro=P, rd=P, R=4, fisher=None, var=None, ray=None):
        return L.voxe_fisher_rays(ctypes.byref(g_) if g_ else None, ctypes.byref(c_) if c_ else None, ro, rd, R, None, fisher, var, ray,
                                  None)

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
    g.density_post_act, g.density_pre_act = abi.ACT_RELU, 5
    assert call(g) == abi.ERR_UNSUPPORTED
    g.density_pre_act = abi.ACT_ABS
    c.sh_degree = 1
    assert call(c_=c) == abi.ERR_BAD_SHAPE                      # F == 3 (deg + 1)^2
    g.F = 12
    assert call(g, c) == abi.OK
    c.sh_degree = 4
    assert call(c_=c) == abi.ERR_UNSUPPORTED
    c.sh_degree, g.F = 0, 3
    g.feature_kind, g.F = abi.FEAT_ATTN, 1
    assert call(g) == abi.ERR_UNSUPPORTED
    g.feature_kind, g.F = abi.FEAT_SH, 3
    # no launch: R == 0 (NULL rays allowed), or both outputs NULL (voxel_var alone asks for nothing)
    assert call(ro=None, rd=None, R=0, fisher=P, var=P, ray=P) == abi.OK and call(ro=None, rd=None, R=0) == abi.OK
    assert call() == abi.OK and call(var=P) == abi.OK


def test_operator_refuses_host_tensors_and_bad_buffers():
    from voxe_hip.runtime import VoxeError

    spec = ops.GridSpec(aabb=H.AABB)
    params = ops.RenderParams(num_samples=8, near=1.0, far=4.0)
    z = torch.zeros(2, 3)
    d, f = torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3)
    with pytest.raises(VoxeError):
        ops.fisher_rays_(spec, params, d, f, z, z, fisher=torch.zeros(4, 4, 4))
    with pytest.raises(VoxeError):
        ops.fisher_rays_(spec, params, d, f, z, z, want_ray_var=True)
    assert ops.fisher_rays_.__module__ == ops.render_bwd_rays.__module__ == "voxe_hip.ops"      # with its sibling that reads features


# ---- the restatement checks itself ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [variants()[0], variants()[3], variants()[7], variants()[9]], ids=variant_id)
def test_autograd_jacobian_equals_the_closed_form_on_one_ray(variant):
    """J of autograd through render_from_samples is the header's closed form sum_k delta_k E_{k,ch} post'(v_k) t_c pre' scale"""
    spec, params, dens, feat, ro, rd, jitter, rng = inputs(case_named("single"), variant, CPU)
    samples = RG.probe_host(spec, params, dens, feat, ro, rd, jitter, rng)
    J = FR.jacobians(samples, dens, feat, ro, rd, spec, params)
    Jc = FR.closed_form_jacobians(FR.sample_terms(samples, dens, feat, ro, rd, spec, params), dens.numel())
    assert J.shape == (1, 3, dens.numel()) and int((J != 0).sum()) > 100
    assert float((J - Jc).abs().max()) <= 1e-12 * float(J.abs().max())
    # and the two reductions are what they say
    P = voxel_var(dens.shape[:3], CPU)
    assert torch.equal(FR.fisher_of(J), (J ** 2).sum(dim=(0, 1)))
    assert abs(float(FR.ray_var_of(J, P)[0]) - float((FR.fisher_of(J) * P.reshape(-1).double()).sum())) <= 1e-12 * float(FR.ray_var_of(J, P)[0])
    assert float(FR.ray_var_of(J)[0]) == float(FR.fisher_of(J).sum())


# ---- the GPU tests' inputs are not vacuous (oracle probe -> restatement, no device) -----------------------------------
_facts = {}


@pytest.mark.parametrize("variant", variants(), ids=variant_id)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_gpu_cases_are_not_vacuous(case, variant):
    spec, params, dens, feat, ro, rd, jitter, rng = inputs(case, variant, CPU)
    samples = RG.probe_host(spec, params, dens, feat, ro, rd, jitter, rng)
    facts = FR.carry_facts(samples, dens.shape[:3])
    _facts[(case[0], variant)] = facts
    terms = FR.sample_terms(samples, dens, feat, ro, rd, spec, params)
    H64 = FR.fisher_of(FR.closed_form_jacobians(terms, dens.numel()))
    wrong = FR.per_sample_squares(terms, dens.numel())
    miss = float((wrong - H64).norm() / H64.norm()) if float(H64.norm()) > 0 else 0.0
    print(f"{case[0]} {variant_id(variant)}: R {ro.shape[0]}  {facts}  fisher != 0: {int((H64 != 0).sum())} of {H64.numel()}  "
          f"per-sample-squares rel_l2 {miss:.3f}")
    if case[0] == "all_miss":
        assert facts["inside"] == 0 and int((H64 != 0).sum()) == 0
        return
    assert int((H64 != 0).sum()) > (30 if ro.shape[0] == 1 else 100) and bool(torch.isfinite(H64).all())
    assert int((H64 == 0).sum()) > 0                                          # exact zeros exist to be kept
    if case[6]:
        assert miss > 10 * FISHER_TOL and miss > 0.1, miss                     # (i)
    if case[0] == "skip24":
        assert facts["jumps"] > 100                                            # (iii)
    if case[0] == "dense12":
        assert facts["missed_rays"] == 8
    if case[0] in ("dense8", "dense12", "aniso"):
        assert facts["two_axes"] > 10 and facts["three_axes"] >= 1, facts      # (ii)
        assert facts["outside_corners"] > 10                                   # (iv)
        assert facts["same_cell"] > 100 or case[0] != "dense8"
    if case[0] == "diagonal":
        assert facts["three_axes"] >= 1, facts


def test_lattice_cases_still_are_what_their_names_say():
    for kind in ("row_image", "tie_xy", "tie_xyz", "all_miss"):
        DC.check_preconditions(DC.case(kind))


def _scene_fisher(yaw):
    spec, params, dens, feat = scene_inputs(CPU)
    ro, rd = scene_rays(yaw, CPU)
    samples = RG.probe_host(spec, params, dens, feat, ro, rd)
    J = FR.closed_form_jacobians(FR.sample_terms(samples, dens, feat, ro, rd, spec, params), dens.numel())
    return FR.fisher_of(J), FR.carry_facts(samples, SCENE_DIMS)


def test_view_selection_scene_ranks_the_far_side_first_in_the_restatement():
    """(v): with the default prior precision the float64 restatement gives the far-side candidate at least SCENE_MIN_RATIO times
    the gain of the candidate among the training cameras; some pixels of every camera miss the grid"""
    train = sum(_scene_fisher(y)[0] for y in SCENE_TRAIN_YAWS)
    lam = 1e-6 * float(train.max())
    gains = []
    for yaw in SCENE_CANDIDATE_YAWS:
        Hc, facts = _scene_fisher(yaw)
        gains.append(float((Hc / (train + lam)).sum()))
        assert 4 <= facts["missed_rays"] <= SCENE_HW * SCENE_HW - 16, facts
    print(f"view-selection scene: gain near side {gains[0]:.4g}  far side {gains[1]:.4g}  ratio {gains[1] / gains[0]:.2f}  lambda {lam:.3e}")
    assert gains[1] >= SCENE_MIN_RATIO * gains[0] > 0


# ---- greedy selection on hand-made grids ------------------------------------------------------------------------------
def _fake_library(monkeypatch, grids):
    """the library layer with the kernel calls replaced: pose i has the Fisher grid grids[i]"""
    from thre3d_atom.thre3d_reprs import fisher as F

    calls = {"accumulate": [], "gain": []}

    def accumulate(vol_mod, poses, intrinsics, **kw):
        calls["accumulate"].append(list(poses))
        return sum((grids[p] for p in poses), torch.zeros_like(grids[0]))

    def gain(vol_mod, pose, intrinsics, fisher, prior_precision=None, **kw):
        calls["gain"].append((pose, float(prior_precision)))
        return float((grids[pose].double() / (fisher.double() + prior_precision)).sum())

    monkeypatch.setattr(F, "accumulate_fisher", accumulate)
    monkeypatch.setattr(F, "information_gain", gain)
    return F, calls


def test_select_next_views_on_hand_made_grids(monkeypatch):
    e = torch.eye(4)
    # poses 0, 1: training (voxels 0 and 1 well seen); candidates 2 .. 6
    grids = {0: 100.0 * e[0], 1: 100.0 * e[1], 2: 50.0 * e[0], 3: 4.0 * e[2], 4: 4.0 * e[2], 5: 3.0 * e[3], 6: 1.0 * e[2] + 1.0 * e[3]}
    F, calls = _fake_library(monkeypatch, grids)
    sel = F.select_next_views(None, [0, 1], [2, 3, 4, 5, 6], None, 3, prior_precision=1.0)
    # round 0: gains 50/101, 4, 4, 3, 2 -> candidates 1 and 2 tie: the lower index.  Its grid joins the total: voxel 2 now holds 4
    # round 1: 50/101, -, 4/5, 3, 1/5 + 1 -> candidate 3.  round 2: 50/101, -, 4/5, -, 1/5 + 1/4 -> candidate 2
    assert sel.indices == [1, 3, 2]
    assert sel.gains == pytest.approx([4.0, 3.0, 0.8]) and sel.gains_after == pytest.approx([0.8, 0.75, 4.0 / 9.0])
    assert sel.rounds[0] == pytest.approx([50.0 / 101.0, 4.0, 4.0, 3.0, 2.0])
    assert math.isnan(sel.rounds[1][1]) and sel.rounds[1][4] == pytest.approx(1.2) and sel.rounds[2][4] == pytest.approx(0.45)
    assert calls["accumulate"][0] == [0, 1] and calls["accumulate"][1:] == [[3], [5], [4]]
    assert all(lam == 1.0 for _, lam in calls["gain"])
    # the default prior precision: 1e-6 x the TRAINING set's largest entry, fixed over the rounds
    F, calls = _fake_library(monkeypatch, grids)
    sel = F.select_next_views(None, [0, 1], [2, 3, 4, 5, 6], None, 9)
    assert sorted(sel.indices) == [0, 1, 2, 3, 4] and len(sel.rounds) == 5 and sel.indices[:2] == [1, 3]
    assert len({lam for _, lam in calls["gain"]}) == 1 and calls["gain"][0][1] == pytest.approx(1e-4)
    assert F.select_next_views(None, [0], [2, 3], None, 0, train_fisher=grids[0]).indices == []
    with pytest.raises(ValueError):
        F.select_next_views(None, [0], [2], None, 1, train_fisher=torch.zeros(4))       # no default for an all-zero grid
    with pytest.raises(ValueError):
        F.select_next_views(None, [0], [2], None, 1, prior_precision=0.0)
    assert "untuned guard" in F.__doc__ and "untuned guard" in F.default_prior_precision.__doc__


# ---- the entry point ----------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("select_next_views_cli", os.path.join(ROOT, "select_next_views.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_point_options_and_documents():
    opts = {p.name: p for p in _cli().main.params}
    assert set(opts) == {"model_path", "data_path", "output_path", "candidates", "num_candidates", "camera_pitch", "num_select",
                         "prior_precision", "uncertainty_maps", "overridden_num_samples_per_ray"}
    assert opts["model_path"].required and opts["data_path"].required and opts["output_path"].required
    assert "-i" in opts["model_path"].opts and "-d" in opts["data_path"].opts and "-o" in opts["output_path"].opts
    assert opts["num_candidates"].default == 72 and opts["camera_pitch"].default == 60.0 and opts["num_select"].default == 5
    assert opts["candidates"].default is None and opts["prior_precision"].default is None
    assert opts["uncertainty_maps"].is_flag and opts["uncertainty_maps"].default is False
    assert opts["overridden_num_samples_per_ray"].default is None
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "select_next_views.py" in readme and "voxe_fisher.hip" in readme and "fisher.py" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.24" in design and "profiles/fisher_bench.txt" in design and "untuned guard" in design
    assert "fisher_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


@pytest.mark.parametrize("from_file", [False, True])
def test_entry_point_writes_the_ranking_with_the_kernel_calls_replaced(from_file, tmp_path, monkeypatch):
    from click.testing import CliRunner

    from thre3d_atom.data.constants import BOUNDS, EXTRINSIC, INTRINSIC, ROTATION, TRANSLATION
    from thre3d_atom.thre3d_reprs import fisher as F
    from thre3d_atom.utils.constants import HEMISPHERICAL_RADIUS
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics, pose_spherical

    mod = _cli()
    intr = CameraIntrinsics(6, 8, 10.0)
    train = [pose_spherical(y, 60.0, 4.0) for y in (0.0, 30.0)]
    vol_mod = type("V", (), {"render_config": type("C", (), {"camera_bounds": CameraBounds(2.0, 6.0)})(),
                             "render": lambda self, pose, intrinsics, **kw: type("O", (), {"colour": torch.full((6, 8, 3), 0.5)})()})()
    seen = {}
    monkeypatch.setattr(mod, "create_volumetric_model_from_saved_model", lambda *a, **k: (vol_mod, {HEMISPHERICAL_RADIUS: 4.0}))
    monkeypatch.setattr(mod, "visibility_cameras", lambda extra, data_path: (train, intr))

    def yaw_of(pose):
        t = torch.as_tensor(pose.translation).reshape(3)
        return float(torch.atan2(t[1], t[0]))

    def fake_accumulate(vm, poses, intrinsics, **kw):
        seen.setdefault("overrides", kw)
        return torch.full((2, 2, 2), float(len(poses)))

    def fake_select(vm, train_poses, cands, intrinsics, k, lam, train_fisher=None, **kw):
        seen.update(k=k, lam=lam, n=len(cands), train_fisher=train_fisher)
        order = list(range(len(cands)))[::-1][:k]
        return F.Selection(order, [10.0 - n for n in range(k)], [1.0] * k,
                           [[float("nan") if i in order[:n] else 1.0 + i for i in range(len(cands))] for n in range(k)])

    monkeypatch.setattr(mod.F, "accumulate_fisher", fake_accumulate)
    monkeypatch.setattr(mod.F, "select_next_views", fake_select)
    monkeypatch.setattr(mod.F, "uncertainty_map", lambda vm, pose, intrinsics, fisher, lam, **kw: torch.rand(6, 8) * (torch.rand(6, 8) > 0.3))
    args = ["-i", "model.pth", "-d", "data", "-o", str(tmp_path), "--num_select", "2", "--uncertainty_maps",
            "--overridden_num_samples_per_ray", "64"]
    if from_file:
        cams = {f"c{n}.png": {EXTRINSIC: {ROTATION: np.asarray(p.rotation).tolist(), TRANSLATION: np.asarray(p.translation).tolist()},
                              INTRINSIC: {"height": 6, "width": 8, "focal": 10.0, BOUNDS: [2.0, 6.0]}}
                for n, p in enumerate(pose_spherical(y, 50.0, 4.0) for y in (90.0, 180.0, 270.0))}
        (tmp_path / "cams.json").write_text(json.dumps(cams))
        args += ["--candidates", str(tmp_path / "cams.json")]
    else:
        args += ["--num_candidates", "6", "--prior_precision", "0.5"]
    res = CliRunner().invoke(mod.main, args)
    assert res.exit_code == 0, (res.output, res.exception)
    n_cand = 3 if from_file else 6
    assert seen["k"] == 2 and seen["n"] == n_cand and seen["overrides"] == {"num_samples_per_ray": 64}
    assert seen["lam"] == (pytest.approx(2e-6) if from_file else 0.5) and float(seen["train_fisher"].max()) == 2.0
    rep = json.loads((tmp_path / "next_views.json").read_text())
    assert rep["num_train_views"] == 2 and rep["num_candidates"] == n_cand and rep["prior_precision"] == pytest.approx(seen["lam"])
    assert [s["candidate"] for s in rep["selected"]] == [n_cand - 1, n_cand - 2] and [s["rank"] for s in rep["selected"]] == [0, 1]
    assert [s["gain"] for s in rep["selected"]] == [10.0, 9.0] and rep["selected"][0]["gain_after"] == 1.0
    for s in rep["selected"]:
        assert np.asarray(s[EXTRINSIC][ROTATION]).shape == (3, 3) and np.asarray(s[EXTRINSIC][TRANSLATION]).shape == (3, 1)
        assert s[INTRINSIC]["height"] == 6 and s[INTRINSIC]["width"] == 8 and s[INTRINSIC][BOUNDS] == [2.0, 6.0]
    if from_file:
        assert rep["selected"][0]["name"] == "c2.png"
        assert np.allclose(rep["selected"][0][EXTRINSIC][TRANSLATION], np.asarray(pose_spherical(270.0, 50.0, 4.0).translation), atol=1e-6)
    assert len(rep["rounds"]) == 2 and rep["rounds"][1]["gains"][n_cand - 1] is None and rep["rounds"][0]["gains"][0] == 1.0
    saved = torch.load(tmp_path / "fisher.pth")
    assert saved["fisher"].shape == (2, 2, 2) and saved["num_train_views"] == 2
    from PIL import Image

    for n in range(2):
        assert Image.open(tmp_path / f"uncertainty_{n:04d}.png").size == (16, 6)
