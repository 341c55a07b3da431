"""CPU checks of tests/iteration_ref.py, the float64 restatement of the trainer's composed iteration, against itself:

1. with one term on, its value and gradient are what that term's own restatement returns on the same inputs (distortion_ref,
   depth_ref, orientation_ref .loss_and_gradient, ssim_ref.ssim64_grad, exposure_ref.fwd_bwd, robust_ref.fwd_bwd,
   background_ref.autograd_gradients), to float64 rounding;
2. a central finite difference in float64 on a handful of elements of every parameter tensor agrees with the autograd gradient
   of the full sum (the glue: weights, means, the affine colour, the mask as a constant, the depth targets, the casts);
3. the conditions that keep tests/test_iteration_gpu.py honest hold on a host-drawn batch of every case: every active term holds
   at least 1 % of the gradient of every grid tensor it reaches, dropping or doubling a term moves the sum by more than the bound,
   and the robust mask does not sit on an edge.  The GPU test asserts the same on the batches its runs drew.

The 3 x 3 rule's cut is an integer count (5 of 9) that many pixels of any batch reach; a count moves only when an inlier flag
flips, which the gap around the quantile excludes, so the conditions asserted are: no residual within 1e-4 (relative) of the
threshold, no patch's count of forgiven pixels equal to its cut, and the patch cut f P^2 itself not an integer."""
import functools

import numpy as np
import pytest
import torch

import background_ref as BR
import depth_ref as PR
import distortion_ref as DR
import exposure_ref as ER
import iteration_ref as IR
import orientation_ref as OR
import ray_grad_ref as RR
import robust_ref as BRF
import ssim_ref as SR

F64 = 1e-10        # float64 rounding through a few hundred sums: relative agreement of two float64 evaluations
F32_LEAF = 2.0 ** -23   # the ray losses' loss_and_gradient differentiate a float32 leaf: autograd rounds their gradient to float32


@functools.lru_cache(maxsize=None)
def _images():
    return IR.truth_images_host()


def _scene(name):
    return IR.make_scene(_images(), IR.CASES[name][1])


@functools.lru_cache(maxsize=None)
def _case(name):
    scene = _scene(name)
    batch = IR.host_batch(name, scene)
    return scene, batch, IR.evaluate(scene, IR.options_of(IR.CASES[name][3]), IR.initial_params(name), batch)


def _perturbed_params(name, seed=11):
    """the case's parameters away from their zero start: texels, exposure, pose deltas and intrinsics as after a few steps"""
    g = torch.Generator().manual_seed(seed)
    p = IR.initial_params(name)
    for key, scale in (("texels", 0.5), ("exposure", 0.05), ("poses", 0.01), ("intrinsics", 0.3)):
        if p[key] is not None:
            p[key] = p[key] + scale * torch.randn(p[key].shape, generator=g)
    return p


def _rays32(scene, batch, key="flat_index"):
    o, d = IR.cast(scene, scene.poses[batch["picks"]].double(), batch[key])
    return o.float(), d.float()


# ---- 1: one term on: the composed reference is that term's own restatement ----------------------------------------------
@pytest.mark.parametrize("term", ["distortion", "depth", "orientation"])
def test_a_ray_loss_alone_is_its_own_restatement(term):
    name = "one_" + term
    scene, batch, res = _case(name)
    kw = IR.CASES[name][3]
    p = IR.initial_params(name)
    dens, feat = p["densities"], p["features"]
    params = IR.render_params(scene, feat)
    if term == "depth":
        ro, rd = _rays32(scene, batch, "depth_flat_index")
        D, s, omega = res["aux"]["depth_targets"]
        assert float(s.min()) == (IR.FAR - IR.NEAR) / IR.SAMPLES and float(s.max()) > 1.2 * float(s.min())    # both sides of the max
        L, g = PR.loss_and_gradient(PR.depth_host, scene.spec, params, dens, feat, ro, rd, D, s, omega)
        value, weight = float((L * omega).mean()), kw["depth_weight"]
    elif term == "distortion":
        ro, rd = _rays32(scene, batch)
        L, g = DR.loss_and_gradient(DR.distortion_host, scene.spec, params, dens, feat, ro, rd)
        value, weight = float(L.mean()), kw["distortion_weight"]
    else:
        ro, rd = _rays32(scene, batch)
        L, g = OR.loss_and_gradient(OR.orientation_host, scene.spec, params, dens, feat, ro, rd, eps=1e-2)
        value, weight = float(L.mean()), kw["orientation_weight"]
    assert value > 0 and float(g.norm()) > 0
    assert abs(res["values"][term] - weight * value) <= F64 * weight * value
    assert IR.rel_l2(res["grads"][term]["densities"], weight * g) <= F32_LEAF
    assert all(float(res["grads"][term][k].norm()) == 0.0 for k in res["sum"] if k != "densities")


def _graph(name, params=None, fixed=None):
    scene = _scene(name)
    batch = IR.host_batch(name, scene)
    leaves = IR.make_leaves(params if params is not None else IR.initial_params(name))
    out, aux = IR.terms(scene, IR.options_of(IR.CASES[name][3]), leaves, batch, fixed=fixed)
    return scene, batch, leaves, out, aux


def test_the_ssim_term_alone_is_ssim64():
    _, _, _, out, aux = _graph("one_ssim")
    weight, patch = IR.CASES["one_ssim"][3]["ssim_weight"], 12
    x, y = aux["specular"].reshape(-1, patch, patch, 3), aux["pixels"].reshape(-1, patch, patch, 3)
    assert x.shape[0] == 4
    (got,) = torch.autograd.grad(out["ssim"], aux["specular_graph"])
    assert abs(float(out["ssim"].detach()) - weight * (1.0 - float(SR.ssim64(x, y)[0]))) <= F64
    assert IR.rel_l2(got.reshape(x.shape), -weight * SR.ssim64_grad(x, y)) <= F64


def test_the_l1_under_exposure_is_exposure_ref():
    name = "one_exposure"
    scene, batch, leaves, out, aux = _graph(name, _perturbed_params(name))
    got_x, got_delta = torch.autograd.grad(out["l1"], (aux["specular_graph"], leaves["exposure"]))
    ref = ER.fwd_bwd(aux["specular"].numpy(), aux["pixels"].numpy(), aux["image_ids"].numpy(), leaves["exposure"].detach().numpy(), "l1")
    assert abs(float(out["l1"]) - ref["loss"][0]) <= F64 * ref["loss"][0]
    assert abs(aux["mse"] - ref["mse"][0]) <= F64 * ref["mse"][0]
    assert IR.rel_l2(got_x, torch.from_numpy(ref["d_x"][0])) <= F64
    assert IR.rel_l2(got_delta, torch.from_numpy(ref["d_delta"][0])) <= F64
    assert int(ref["used"].sum()) >= 4 and not ref["flip"].any()
    reg = IR.CASES[name][3].get("exposure_regularization", 1e-3)
    assert abs(float(out["exposure_reg"]) - reg * float((leaves["exposure"].detach() ** 2).mean())) <= F64 * float(out["exposure_reg"])


def test_the_robust_l1_under_exposure_is_robust_ref_with_the_mask_as_ray_weight():
    name = "all_robust"
    scene, batch, leaves, out, aux = _graph(name, _perturbed_params(name))
    side = 8
    seen = IR.affine_colour(aux["specular"], aux["image_ids"], leaves["exposure"].detach())
    x, y = seen.reshape(-1, side, side, 3).float().numpy(), aux["pixels"].reshape(-1, side, side, 3).float().numpy()
    rank, patch_min = BRF.rank_of_quantile(0.5, x.shape[0] * side * side), BRF.patch_min_of_fraction(0.6, side)
    ref = BRF.fwd_bwd(x, y, rank, 5, patch_min)
    info = aux["robust"]
    assert info["gap"] > 1e-4 and ref["stats"] == info["stats"] and info["stats"][2] > info["stats"][0]     # both rules forgive
    assert np.array_equal(ref["mask"].reshape(-1), aux["mask"].numpy().astype(np.uint8))
    assert abs(float(out["l1"]) - ref["loss"]) <= 1e-6          # (robust_ref takes x - y in float32)
    # the same value and gradients from exposure_ref with the mask as per-ray weights: the trainer's `robust_side and exposed`
    got_x, got_delta = torch.autograd.grad(out["l1"], (aux["specular_graph"], leaves["exposure"]))
    ex = ER.fwd_bwd(aux["specular"].numpy(), aux["pixels"].numpy(), aux["image_ids"].numpy(), leaves["exposure"].detach().numpy(), "l1",
                    w=aux["mask"].numpy())
    assert abs(float(out["l1"]) - ex["loss"][0]) <= F64 * ex["loss"][0]
    assert IR.rel_l2(got_x, torch.from_numpy(ex["d_x"][0])) <= F64 and IR.rel_l2(got_delta, torch.from_numpy(ex["d_delta"][0])) <= F64
    # the diffuse term under the same mask: an SH-0 grid's diffuse render is its specular one
    assert float(out["diffuse"]) == float(out["l1"])


def test_the_background_behind_the_l1_is_background_ref():
    name = "one_background"
    scene, batch, leaves, out, aux = _graph(name, _perturbed_params(name))
    o, d = aux["rays"]
    dens, feat = leaves["densities"].detach(), leaves["features"].detach()
    colour, _, acc = RR.render_from_samples(aux["z"], aux["inside"], RR.probe_host(
        scene.spec, IR.render_params(scene, feat), dens.float(), feat.float(), o.float(), d.float())[2], dens, feat, o, d, scene.spec,
        IR.render_params(scene, feat))
    g = torch.sign(aux["specular"] - aux["pixels"]) / aux["pixels"].numel()
    composite, d_acc, d_tex, d_d = BR.autograd_gradients(colour, acc, d, leaves["texels"].detach(), g)
    assert float((composite - aux["specular"]).abs().max()) <= 1e-14
    (got,) = torch.autograd.grad(out["l1"], leaves["texels"])
    assert float(d_tex.norm()) > 0 and IR.rel_l2(got, d_tex) <= F64


# ---- 2: finite differences of the full sum ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_ssim", "all_robust"])
def test_autograd_of_the_sum_agrees_with_central_differences(name):
    scene = _scene(name)
    batch = IR.host_batch(name, scene)
    options = IR.options_of(IR.CASES[name][3])
    params = _perturbed_params(name)
    base = IR.evaluate(scene, options, params, batch)
    aux = base["aux"]
    # what the trainer holds constant: the float32 rays the samples come from, the mask, the depth targets
    o, d = aux["rays"]
    fixed = {"rays32": (o.float(), d.float())}
    if "mask" in aux:
        fixed["mask"] = aux["mask"]
    if "depth_targets" in aux:
        fixed["depth_targets"] = aux["depth_targets"]
        fixed["depth_rays32"] = _depth_rays32(scene, params, batch)

    def total(p):
        with torch.no_grad():
            out, _ = IR.terms(scene, options, {k: v.double() for k, v in p.items() if v is not None}, batch, fixed=fixed)
        return float(sum(out.values()))

    worst = 0.0
    for key, grad in base["sum"].items():
        flat = grad.reshape(-1)
        for i in torch.topk(flat.abs(), min(3, flat.numel())).indices.tolist():
            h = 1e-6 * max(1.0, abs(float(params[key].reshape(-1)[i])))
            vals = []
            for sign in (1.0, -1.0):
                p = {k: (None if v is None else v.double().clone()) for k, v in params.items()}
                p[key].reshape(-1)[i] += sign * h
                vals.append(total(p))
            fd = (vals[0] - vals[1]) / (2.0 * h)
            err = abs(fd - float(flat[i])) / abs(float(flat[i]))
            worst = max(worst, err)
            print(f"{name} {key}[{i}]: autograd {float(flat[i]):+.6e}  central difference {fd:+.6e}  rel {err:.2e}")
            # h^2 f''' / 6 and the rounding 2^-53 |L| / h, both relative to gradients of 1e-3 .. 1: well below 1e-5
            assert err <= 1e-5, (key, i, err)
    assert worst > 0.0


def _depth_rays32(scene, params, batch):
    from thre3d_atom.thre3d_reprs.poses import CameraPoseDeltas

    poses = scene.poses[batch["picks"]].double()
    if params["poses"] is not None:
        module = CameraPoseDeltas(scene.poses.shape[0]).double()
        module.deltas.data.copy_(params["poses"])
        poses = module.apply(poses, batch["picks"]).detach()
    intr = None if params["intrinsics"] is None else params["intrinsics"].double()
    o, d = IR.cast(scene, poses, batch["depth_flat_index"], intr)
    return o.float(), d.float()


# ---- 3: the conditions on the inputs ---------------------------------------------------------------------------------------
def assert_every_term_is_visible(name, res, run=None):
    """every active term holds VISIBLE of each grid tensor's gradient it reaches (the ray losses reach the densities only: their
    kernels have no feature gradient), and the sum without or with twice a term is outside the bound of `run` (default: of the
    sum itself)"""
    kw = IR.CASES[name][3]
    active = {"l1"} | ({"diffuse"} if kw.get("apply_diffuse_render_regularization", True) else set()) \
        | {t for t in ("distortion", "depth", "orientation", "ssim") if kw.get(t + "_weight", 0.0) > 0.0}
    assert active <= set(res["grads"])
    for tensor in IR.GRID:
        share = IR.shares(res, tensor)
        print(f"{name} shares of d_{tensor}: " + "  ".join(f"{t} {v:.3f}" for t, v in share.items()))
        reach = {t for t in active if tensor == "densities" or t not in IR.DENSITY_ONLY}
        assert reach <= set(share), (tensor, reach, share)
        target = res["sum"][tensor] if run is None else run[tensor]
        for t in reach:
            assert share[t] >= IR.VISIBLE, (name, tensor, t, share[t])
            g = res["grads"][t][tensor]
            assert IR.rel_l2(res["sum"][tensor] - g, target) > IR.BOUND and IR.rel_l2(res["sum"][tensor] + g, target) > IR.BOUND


def assert_mask_is_off_the_edges(info):
    assert info["gap"] > 1e-4, info
    assert not (info["patch_counts"] == info["patch_min"]).any(), info
    assert info["patch_cut"] != round(info["patch_cut"])


@pytest.mark.parametrize("name", list(IR.CASES))
def test_the_cases_keep_every_term_visible(name):
    scene, batch, res = _case(name)
    assert_every_term_is_visible(name, res)
    assert res["aux"]["min_abs_residual"] > 0.0
    if "robust" in res["aux"]:
        assert_mask_is_off_the_edges(res["aux"]["robust"])
        a, c, w = res["aux"]["robust"]["stats"]
        assert a < w < batch["flat_index"].numel()           # the mask trims, and the rules forgive


def test_first_moments():
    g1, g2 = torch.tensor([1.0, -2.0]), torch.tensor([0.5, 4.0])
    m1, m2 = IR.first_moments(g1, g2)
    assert torch.allclose(m1, 0.1 * g1) and torch.allclose(m2, 0.9 * m1 + 0.1 * g2)
