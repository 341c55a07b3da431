"""float64 torch restatement of ONE composed (not one-call) iteration of train_sh_vox_grid_vol_mod_with_posed_images
(thre3d_atom/modules/trainers.py, the `else` branch of the iteration), on the CPU, and the cases the host and GPU tests share.

Nothing of the terms is derived here: the render with autograd to grid and rays is ray_grad_ref.render_from_samples, the rays are
ray_grad_ref.cast_rays (camera_ref.cast_rays_torch under learned intrinsics) of CameraPoseDeltas(...).double() applied to the picked
poses, the background is background_ref.composite, the ray losses are distortion_ref / depth_ref / orientation_ref.from_samples,
SSIM is ssim_ref.ssim64 and the robust mask is robust_ref's rank, threshold and mask_from_inliers.  What is written here is the
glue the trainer itself adds:
  * the L1 mean of the specular render and of the diffuse second render against the batch's pixels;
  * under exposure compensation c' = (I + dA) c + db per ray's image (checked against exposure_ref.fwd_bwd by the host test) and
    exposure_regularization * mean(delta^2);
  * the robust mask as a constant, taken of the colours as the loss sees them, shared by the diffuse term; the loss is
    sum_r w_r |e_r| / (3 R), which is also what `ray_weight` gives under exposure;
  * weight * (1 - SSIM) on the channel-last patch view of the (transformed) specular colours;
  * the depth batch: D = <P - o, d> / <d, d> (detached), s = max(sigma_scale * error * max(D, 0) / fx, (far - near) / S), omega = 1;
  * the weights, and the sum.
As in the ray-loss restatements the sample depths, inside flags and cell indices are the renderer's own (a sample probe of the
float32 rays: the oracle's on the host, ops.sample_probe on the device); the render config does not perturb the samples.

`evaluate` returns, per term, its value and its gradient to every parameter tensor (already multiplied by the weight), and the sums.
"""
import dataclasses
from typing import Any, Dict, Optional

import numpy as np
import torch

import background_ref as BR
import camera_ref as CR
import depth_ref as PR
import distortion_ref as DR
import orientation_ref as OR
import ray_grad_ref as RR
import robust_ref as BRF
import ssim_ref as SR
from voxe_hip import abi, ops

TERMS = ("l1", "diffuse", "exposure_reg", "distortion", "depth", "orientation", "ssim")
PARAMS = ("densities", "features", "texels", "exposure", "poses", "intrinsics")
GRID = ("densities", "features")
# the terms whose gradient reaches only the densities (their kernels have no feature, ray or colour gradient)
DENSITY_ONLY = ("distortion", "depth", "orientation")
BETA1 = 0.9


@dataclasses.dataclass
class Scene:
    """what an iteration reads besides the parameters and the batch"""
    spec: Any                 # ops.GridSpec
    num_samples: int
    near: float
    far: float
    white_bkgd: bool
    height: int
    width: int
    focal: float
    images: torch.Tensor      # [N,3,H,W] float32
    poses: torch.Tensor       # [N,3,4] float32
    sparse: Optional[tuple] = None   # (offsets, xy, xyz, error) of SparsePoints


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def render_params(scene: Scene, features, diffuse=False):
    degree = int(round((features.shape[-1] // 3) ** 0.5)) - 1
    return ops.RenderParams(num_samples=scene.num_samples, near=scene.near, far=scene.far, white_bkgd=scene.white_bkgd,
                            sh_degree=degree, render_diffuse=diffuse)


def cast(scene: Scene, poses64, flat_index, intrinsics=None):
    """(rays_o, rays_d) float64 of flat (camera, row, column) indices into the K poses; differentiable w.r.t. both.  (One stage:
    the images are the full-resolution ones, and the learned intrinsics are used as they are.)"""
    if intrinsics is None:
        return RR.cast_rays(scene.height, scene.width, scene.focal, poses64, flat_index)
    cam = CR.Camera(scene.height, scene.width, scene.focal, scene.focal, scene.width * 0.5, scene.height * 0.5)
    return CR.cast_rays_torch(cam, intrinsics, poses64, flat_index)


def affine_colour(colour, ids, delta):
    """c' = (I + dA) c + db of each ray's image: delta [N,12] = dA row-major, then db"""
    A = delta[:, :9].reshape(-1, 3, 3) + torch.eye(3, dtype=delta.dtype)
    return (A[ids] * colour[:, None, :]).sum(dim=-1) + delta[ids, 9:]


def robust_mask(seen, pixels, num_patches, side, quantile, patch_fraction):
    """(mask [R] float64, info) of the float64 colours: robust_ref's rank, order statistic and neighbourhood / patch rules on
    float64 residuals e = sum_c d_c^2.  info: the sorted residuals around the rank and the counts the edge conditions need"""
    d = (seen.detach() - pixels).reshape(num_patches, side, side, -1).numpy()
    e = (d * d).sum(axis=-1)
    M = e.size
    rank = BRF.rank_of_quantile(quantile, M)
    tau = BRF.threshold(e, rank)
    a = (e <= tau).astype(np.int64)
    patch_min = BRF.patch_min_of_fraction(patch_fraction, side)
    c, w, _ = BRF.mask_from_inliers(a, 5, patch_min)
    others = np.delete(np.sort(e.reshape(-1)), rank)
    info = {"tau": float(tau), "rank": rank, "gap": float(np.abs(others - tau).min() / tau),
            "patch_counts": c.reshape(num_patches, -1).sum(axis=1), "patch_min": patch_min,
            "patch_cut": None if patch_fraction is None else float(patch_fraction) * side * side,
            "stats": (int(a.sum()), int(c.sum()), int(w.sum()))}
    return torch.from_numpy(w.reshape(-1).astype(np.float64)), info


def depth_targets(scene: Scene, options, rows, rays_o, rays_d):
    """(D, s, omega) [R] float64 of the keypoint rows: the glue of the trainer's _depth_batch"""
    _, _, xyz, error = scene.sparse
    o, d = rays_o.detach(), rays_d.detach()
    D = ((xyz[rows].double() - o) * d).sum(dim=-1) / (d * d).sum(dim=-1)
    s = (float(options.get("depth_sigma_scale", 1.0)) * error[rows].double() * D.clamp_min(0.0) / float(scene.focal)) \
        .clamp_min((scene.far - scene.near) / scene.num_samples)
    return D, s, torch.ones_like(D)


def depth_flat_index(scene: Scene, cam, rows):
    """the flat index of the nearest pixel of each keypoint row, in camera `cam` of the picks (the centre of the top-left pixel
    is at (0.5, 0.5))"""
    xy = scene.sparse[1]
    px = xy[rows, 0].floor().long().clamp_(0, scene.width - 1)
    py = xy[rows, 1].floor().long().clamp_(0, scene.height - 1)
    return (cam * scene.height + py) * scene.width + px


def terms(scene: Scene, options: Dict, leaves: Dict, batch: Dict, probe=RR.probe_host, fixed: Optional[Dict] = None):
    """({term: scalar with a graph to `leaves`}, aux) of one iteration.  leaves: float64 tensors by PARAMS name (absent / None:
    the option is off).  batch: flat_index, picks, and for the depth term depth_flat_index / depth_rows; optional rays32 /
    depth_rays32 (the float32 rays the samples are probed with and the ray losses march: default the float64 rays rounded).
    `fixed` holds constants a finite difference must not move: rays32, depth_rays32, mask, depth_targets."""
    fixed = fixed or {}
    dens, feat = leaves["densities"], leaves["features"]
    texels, delta, pose_deltas, intrinsics = (leaves.get(k) for k in ("texels", "exposure", "poses", "intrinsics"))
    picks, flat = batch["picks"].long(), batch["flat_index"].long()
    per = scene.height * scene.width
    cam = torch.div(flat, per, rounding_mode="floor")
    rem = flat - cam * per
    ids = picks[cam]
    pixels = scene.images[ids, :, torch.div(rem, scene.width, rounding_mode="floor"), rem % scene.width].double()
    poses64 = scene.poses[picks].double()
    if pose_deltas is not None:
        from thre3d_atom.thre3d_reprs.poses import CameraPoseDeltas

        module = CameraPoseDeltas(scene.poses.shape[0]).double()
        module._parameters["deltas"] = pose_deltas            # (the leaf itself: the gradient arrives at it)
        poses64 = module.apply(poses64, picks)
    o, d = cast(scene, poses64, flat, intrinsics)
    o32, d32 = fixed.get("rays32") or batch.get("rays32") or (o.detach().float(), d.detach().float())
    dens32, feat32 = dens.detach().float(), feat.detach().float()
    p_spec, p_diff = render_params(scene, feat), render_params(scene, feat, diffuse=True)
    z, inside, idx = (t.cpu() for t in probe(scene.spec, p_spec, dens32, feat32, o32, d32))
    R = flat.numel()

    def render(params):
        colour, _, acc = RR.render_from_samples(z, inside, idx, dens, feat, o, d, scene.spec, params)
        return colour if texels is None else BR.composite(colour, acc, d, texels)

    def seen_by_loss(colour):
        return colour if delta is None else affine_colour(colour, ids, delta)

    aux = {"pixels": pixels, "image_ids": ids, "rays": (o.detach(), d.detach()), "z": z, "inside": inside}
    specular = render(p_spec)
    seen = seen_by_loss(specular)
    aux["specular"], aux["specular_graph"], aux["seen_graph"] = specular.detach(), specular, seen
    weight = None
    side = int(options.get("robust_side", 0))
    if side:
        num_patches = R // (side * side)
        weight, aux["robust"] = robust_mask(seen, pixels, num_patches, side, options.get("robust_inlier_quantile", 0.5),
                                            options.get("robust_patch_inlier_fraction", 0.6))
        if "mask" in fixed:
            weight = fixed["mask"]
        aux["mask"] = weight

    def photometric(colour_seen):
        e = colour_seen - pixels
        if weight is None:
            return e.abs().mean(), e
        return (weight[:, None] * e.abs()).sum() / (3.0 * R), e

    out = {}
    out["l1"], e_spec = photometric(seen)
    # (the L1 gradient is the residual's sign: the smallest |e| among the rays that meet the grid says how far a float32 render
    #  is from flipping one; a ray that misses the grid renders its background exactly in either precision)
    hit = inside.bool().any(dim=1)
    aux["min_abs_residual"] = float(e_spec.detach()[hit].abs().min())
    aux["mse"] = float((e_spec.detach() ** 2).mean())
    if options.get("diffuse", True):
        diffuse = render(p_diff)
        aux["diffuse_colour"] = diffuse.detach()
        out["diffuse"], e_diff = photometric(seen_by_loss(diffuse))
        aux["min_abs_residual"] = min(aux["min_abs_residual"], float(e_diff.detach()[hit].abs().min()))
    if delta is not None and options.get("exposure_regularization", 1e-3) > 0.0:
        out["exposure_reg"] = float(options.get("exposure_regularization", 1e-3)) * (delta * delta).mean()
    if options.get("distortion_weight", 0.0) > 0.0:
        L = DR.from_samples(z, inside, dens, o32, d32, scene.spec, scene.near, scene.far)
        aux["distortion"] = float(L.detach().mean())
        out["distortion"] = float(options["distortion_weight"]) * L.mean()
    if options.get("depth_weight", 0.0) > 0.0:
        dflat, rows = batch["depth_flat_index"].long(), batch["depth_rows"].long()
        od, dd = cast(scene, poses64, dflat, intrinsics)
        od32, dd32 = fixed.get("depth_rays32") or batch.get("depth_rays32") or (od.detach().float(), dd.detach().float())
        zd, ind, _ = (t.cpu() for t in probe(scene.spec, p_spec, dens32, feat32, od32, dd32))
        D, s, omega = fixed.get("depth_targets") or depth_targets(scene, options, rows, od, dd)
        L = PR.from_samples(zd, ind, dens, od32, dd32, scene.spec, D, s)
        aux["depth"], aux["depth_targets"] = float((L.detach() * omega).mean()), (D, s, omega)
        out["depth"] = float(options["depth_weight"]) * (L * omega).mean()
    if options.get("orientation_weight", 0.0) > 0.0:
        L = OR.from_samples(z, inside, dens, o32, d32, scene.spec, float(options.get("orientation_normal_eps", 1e-2)))
        aux["orientation"] = float(L.detach().mean())
        out["orientation"] = float(options["orientation_weight"]) * L.mean()
    patch = int(options.get("ssim_patch", 0))
    if patch and options.get("ssim_weight", 0.0) > 0.0:
        shape = (R // (patch * patch), patch, patch, 3)
        ssim = SR.ssim64(seen.reshape(shape), pixels.reshape(shape))[0]
        aux["ssim"] = float(ssim.detach())
        out["ssim"] = float(options["ssim_weight"]) * (1.0 - ssim)
    return out, aux


def make_leaves(params: Dict):
    """float64 leaves of the parameter tensors (None entries dropped)"""
    return {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in params.items() if v is not None}


def evaluate(scene: Scene, options: Dict, params: Dict, batch: Dict, probe=RR.probe_host, fixed: Optional[Dict] = None):
    """dict: values {term: float}, total, grads {term: {param: tensor}}, sum {param: tensor}, aux"""
    leaves = make_leaves(params)
    out, aux = terms(scene, options, leaves, batch, probe, fixed)
    names = list(leaves)
    grads = {}
    for term, value in out.items():
        gs = torch.autograd.grad(value, [leaves[n] for n in names], retain_graph=True, allow_unused=True)
        grads[term] = {n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(names, gs)}
    total = {n: sum(grads[t][n] for t in grads) for n in names}
    if "ssim" in out and "exposure" in leaves:
        # (what the SSIM term hands the affine colour's backward: tests/test_iteration_gpu.py builds the exposure bound from it)
        (aux["ssim_d_seen"],) = torch.autograd.grad(out["ssim"], aux["seen_graph"], retain_graph=True)
    return {"values": {t: float(v.detach()) for t, v in out.items()}, "total": float(sum(v.detach() for v in out.values())),
            "grads": grads, "sum": total, "aux": aux}


def shares(result, name):
    """{term: |g_term| / |sum of the terms|} on parameter tensor `name`, of the terms that reach it at all"""
    whole = float(result["sum"][name].norm())
    return {t: float(g[name].norm()) / whole for t, g in result["grads"].items() if float(g[name].norm()) > 0.0}


# float32 roundings of a d_delta term, + 2, as tests/test_exposure_gpu.py counts them (K_DDELTA["l1"], K_BWD_DDELTA)
K_DDELTA_L1, K_BWD_DDELTA, U24 = 4, 4, 2.0 ** -24
SSIM_GRAD_REL = 1e-4       # what tests/test_ssim_gpu.py holds the SSIM gradient to (ssim_ref.reference: bound_grad_rel's floor)


def exposure_gradient_bound(result, delta, colour_abs):
    """[N,12]: how far a float32 run's gradient to the exposure deltas may lie from `result`'s, element by element, built from
    what tests/test_exposure_gpu.py asserts and one named source it does not have.  Per L1 term (specular, diffuse):
    K 2^-24 sum|terms| + the fixed point's 2^-33 per ray, test_exposure_gpu's own bound for exact float32 inputs; plus the
    render's colour error `colour_abs` pushed through the backward d_delta[n, 3c + j] = gs sum_r w_r sign(e_rc) x_rj, which is
    |gs| sum_r w_r colour_abs on the nine dA columns and nothing on the three db columns (they do not read x).  For the SSIM
    term through voxe_exposure_apply_bwd, d_delta = sum_r g_r x_r^T: K 2^-24 sum|terms|, sum_r |g_r| colour_abs on the dA
    columns, and SSIM_GRAD_REL of sum|terms| for the error of g itself.  A residual whose sign a float32 render flips is not
    covered: the GPU test prints the smallest |residual|."""
    import exposure_ref as ER

    aux = result["aux"]
    delta = np.asarray(delta, np.float64).reshape(-1, 12)
    N = delta.shape[0]
    ids, y = aux["image_ids"].numpy(), aux["pixels"].numpy()
    w = aux["mask"].numpy() if "mask" in aux else None
    weights = np.ones(y.shape[0]) if w is None else w
    eps_x = np.full(y.shape, float(colour_abs))
    dA = np.concatenate([np.ones(9), np.zeros(3)])
    bound = np.zeros((N, 12))
    for key in ("specular", "diffuse_colour"):
        if key in aux:
            ref = ER.fwd_bwd(aux[key].numpy(), y, ids, delta, "l1", w)
            bound += K_DDELTA_L1 * U24 * ref["d_delta"][1] + abs(ref["gs"]) * ref["count"][:, None] * 2.0 ** -33
            bound += ER._segment(ids, N, weights[:, None] * np.ones_like(y), eps_x, abs(ref["gs"])) * dA
    if "ssim_d_seen" in aux:
        g = aux["ssim_d_seen"].numpy()
        back = ER.apply_bwd(aux["specular"].numpy(), ids, delta, g)
        bound += (K_BWD_DDELTA * U24 + SSIM_GRAD_REL) * back["d_delta"][1] + ER._segment(ids, N, np.abs(g), eps_x, 1.0) * dA
    return torch.from_numpy(bound)


def first_moments(g1, g2):
    """Adam's exp_avg after one and after two steps from zero state"""
    return (1.0 - BETA1) * g1, BETA1 * (1.0 - BETA1) * g1 + (1.0 - BETA1) * g2


# ---- the scene and the cases of tests/test_iteration_host.py and tests/test_iteration_gpu.py ----------------------------------
DIMS, VOXEL = (14, 12, 10), 0.2          # an anisotropic grid: its box is 2.8 x 2.4 x 2.0
DENSITY_SCALE = 10.0
HW, VIEWS, SAMPLES, NEAR, FAR = 32, 16, 32, 1.8, 6.6
FOCAL = 0.5 * HW / float(np.tan(0.5 * 0.6911112))
KEYPOINTS = 24                           # per camera
TRUTH_RADIUS = 0.9                       # the sphere the synthetic views show (test_trainers_gpu._sphere_model)
BOUND = 1e-4                             # global rel-L2 of a gradient against its reference (tests/test_hip_configs.py)
VISIBLE = 100.0 * BOUND                  # the share every active term must have of a grid tensor's gradient


def grid_spec():
    aabb = tuple((-0.5 * n * VOXEL, 0.5 * n * VOXEL) for n in DIMS)
    return ops.GridSpec(aabb=aabb, density_scale=DENSITY_SCALE, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS)


def initial_grid(degree, seed=3):
    """(densities [14,12,10,1], features [14,12,10,3 (deg+1)^2]) float32, uniform in [-1, 1]"""
    g = torch.Generator().manual_seed(seed)
    return (torch.empty(*DIMS, 1).uniform_(-1, 1, generator=g), torch.empty(*DIMS, 3 * (degree + 1) ** 2).uniform_(-1, 1, generator=g))


def view_poses():
    from thre3d_atom.utils.imaging_utils import pose_spherical

    poses = []
    for i in range(VIEWS):
        pose = pose_spherical(360.0 * i / VIEWS, 20.0 + 50.0 * ((i * 0.618) % 1.0), 4.0311)
        poses.append(torch.cat([pose.rotation, pose.translation], dim=1))
    return torch.stack(poses).float()


def sparse_points(poses, seed=9):
    """(offsets, xy, xyz, error): KEYPOINTS pixels per camera whose rays hit the truth's sphere, the world point where they do,
    and reprojection errors in [0.5, 4] pixels -- on both sides of the width's floor (far - near) / S"""
    gen = torch.Generator().manual_seed(seed)
    offsets, xy, xyz = [0], [], []
    for pose in poses:
        ro, rd = RR.cast_rays(HW, HW, FOCAL, pose[None])
        a, b, c = (rd * rd).sum(dim=1), (ro * rd).sum(dim=1), (ro * ro).sum(dim=1) - TRUTH_RADIUS ** 2
        disc = b * b - a * c
        hit = torch.nonzero(disc > 0).reshape(-1)
        pick = hit[torch.randperm(len(hit), generator=gen)[:KEYPOINTS]]
        depth = ((-b - disc.clamp_min(0).sqrt()) / a)[pick]
        xy.append(torch.stack([(pick % HW).float() + 0.5, (pick // HW).float() + 0.5], dim=1))
        xyz.append((ro[pick] + rd[pick] * depth[:, None]).float())
        offsets.append(offsets[-1] + len(pick))
    error = torch.empty(offsets[-1]).uniform_(0.5, 4.0, generator=gen)
    return torch.tensor(offsets), torch.cat(xy), torch.cat(xyz), error


def make_scene(images, white_bkgd):
    poses = view_poses()
    return Scene(grid_spec(), SAMPLES, NEAR, FAR, bool(white_bkgd), HW, HW, FOCAL, images.float().cpu(), poses, sparse_points(poses))


def truth_images_host():
    """the synthetic views in float64 on the host: the truth's 24^3 sphere grid through the restatement's render (the GPU test
    renders them with the kernels; the two differ by the renderer's float32 error, which conditions on the inputs do not see)"""
    side, samples = 24, 64
    ax = (torch.arange(side, dtype=torch.float32) + 0.5) / side * 3.0 - 1.5
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    dens = torch.where(torch.sqrt(x * x + y * y + z * z) < TRUTH_RADIUS, torch.tensor(1.0), torch.tensor(-1.0))[..., None].contiguous()
    feat = torch.stack([2.0 * torch.sin(2 * x), 2.0 * torch.cos(3 * y), 2.0 * torch.sin(2.5 * z + 1)], dim=-1).contiguous()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=100.0 / 3.0)
    params = ops.RenderParams(num_samples=samples, near=NEAR, far=FAR, white_bkgd=True)
    poses = view_poses()
    ro, rd = RR.cast_rays(HW, HW, FOCAL, poses)
    ro, rd = ro.float(), rd.float()
    with torch.no_grad():
        colour, _, _ = RR.render_from_samples(*RR.probe_host(spec, params, dens, feat, ro, rd), dens, feat, ro, rd, spec, params)
    return colour.reshape(VIEWS, HW, HW, 3).permute(0, 3, 1, 2).float().contiguous()


# name -> (SH degree, white_bkgd, ray_batch_size, trainer keyword arguments).  The weights are chosen so that every active term
# holds at least VISIBLE of the gradient of every grid tensor it reaches (test_iteration_host asserts it on a host batch,
# test_iteration_gpu on the batches the runs drew).
_ALL_SSIM = dict(apply_diffuse_render_regularization=True, distortion_weight=0.05, depth_weight=0.02, depth_ray_batch_size=64,
                 orientation_weight=0.05, exposure_learning_rate=1e-3, background_resolution=4, pose_learning_rate=1e-3,
                 intrinsics_learning_rate=1e-2, ssim_weight=0.2, ssim_patch_size=12)
_ALL_ROBUST = dict(apply_diffuse_render_regularization=True, robust_loss=True, robust_patch_size=8, exposure_learning_rate=1e-3,
                   distortion_weight=0.05, background_resolution=4)
CASES = {
    "all_ssim": (1, False, 4 * 12 * 12, _ALL_SSIM),
    "all_robust": (0, False, 8 * 8 * 8, _ALL_ROBUST),
    "one_distortion": (0, True, 300, dict(apply_diffuse_render_regularization=False, distortion_weight=0.2)),
    "one_depth": (0, True, 300, dict(apply_diffuse_render_regularization=False, depth_weight=0.02, depth_ray_batch_size=64)),
    "one_orientation": (0, True, 300, dict(apply_diffuse_render_regularization=False, orientation_weight=0.05)),
    "one_ssim": (0, True, 4 * 12 * 12, dict(apply_diffuse_render_regularization=False, ssim_weight=0.2, ssim_patch_size=12)),
    "one_exposure": (0, True, 300, dict(apply_diffuse_render_regularization=False, exposure_learning_rate=1e-3)),
    "one_background": (0, False, 300, dict(apply_diffuse_render_regularization=False, background_resolution=4)),
    "one_pose": (0, True, 300, dict(apply_diffuse_render_regularization=False, pose_learning_rate=1e-3)),
    # L1, diffuse and distortion over every pixel of 16 picked views: the batch size at which the render takes its other route
    "plain_large": (0, True, 16 * HW * HW, dict(apply_diffuse_render_regularization=True, distortion_weight=0.2,
                                               image_batch_cache_size=16)),
}
ONE_TERM = tuple(k for k in CASES if k.startswith("one_"))


def options_of(kwargs):
    """the restatement's options of the trainer's keyword arguments (one stage at 32 x 32: the patch sides are the given ones)"""
    opts = {"diffuse": kwargs.get("apply_diffuse_render_regularization", True)}
    for k in ("distortion_weight", "depth_weight", "depth_sigma_scale", "orientation_weight", "orientation_normal_eps", "ssim_weight",
              "exposure_regularization", "robust_inlier_quantile", "robust_patch_inlier_fraction"):
        if k in kwargs:
            opts[k] = kwargs[k]
    if kwargs.get("ssim_weight", 0.0) > 0.0:
        opts["ssim_patch"] = min(int(kwargs.get("ssim_patch_size", 32)), HW)
    if kwargs.get("robust_loss", False):
        opts["robust_side"] = min(int(kwargs.get("robust_patch_size", 16)), HW) // 2 * 2
    return opts


def initial_params(name):
    """the parameter tensors as the trainer creates them for case `name` (float32; None: the option is off)"""
    degree, _, _, kw = CASES[name]
    dens, feat = initial_grid(degree)
    n = int(kw.get("background_resolution", 0))
    return {"densities": dens, "features": feat,
            "texels": torch.zeros(n, 2 * n, 3) if n else None,
            "exposure": torch.zeros(VIEWS, 12) if kw.get("exposure_learning_rate", 0.0) > 0.0 else None,
            "poses": torch.zeros(VIEWS, 6) if kw.get("pose_learning_rate", 0.0) > 0.0 else None,
            "intrinsics": torch.tensor([FOCAL, FOCAL, HW * 0.5, HW * 0.5]) if kw.get("intrinsics_learning_rate", 0.0) > 0.0 else None}


def host_batch(name, scene, seed=0):
    """a batch drawn on the host the way the trainer draws it (its own generator: the GPU runs draw theirs on the device)"""
    _, _, ray_batch, kw = CASES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    K = min(int(kw.get("image_batch_cache_size", 8)), VIEWS)
    picks = torch.randint(0, VIEWS, (K,), generator=g)
    opts = options_of(kw)
    side = opts.get("ssim_patch", 0) or opts.get("robust_side", 0)
    per = HW * HW
    if side:
        n = ray_batch // (side * side)
        cams = torch.randint(0, K, (n,), generator=g)
        top, left = torch.randint(0, HW - side + 1, (n,), generator=g), torch.randint(0, HW - side + 1, (n,), generator=g)
        offs = torch.arange(side)
        flat = ((cams[:, None, None] * HW + top[:, None, None] + offs[None, :, None]) * HW + left[:, None, None]
                + offs[None, None, :]).reshape(-1)
    else:
        flat = torch.sort(torch.randperm(K * per, generator=g)[:min(ray_batch, K * per)]).values
    batch = {"picks": picks, "flat_index": flat}
    if kw.get("depth_weight", 0.0) > 0.0:
        offsets = scene.sparse[0]
        n = int(kw.get("depth_ray_batch_size", 4096))
        cam = torch.randint(0, K, (n,), generator=g)
        rows = offsets[picks[cam]] + (torch.rand(n, generator=g) * (offsets[picks[cam] + 1] - offsets[picks[cam]])).long()
        batch["depth_rows"], batch["depth_flat_index"] = rows, depth_flat_index(scene, cam, rows)
    return batch
