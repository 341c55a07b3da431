"""Losses over libvoxe_hip.so (the scalar regularisers of the SDS edit, the masked attention L1, the distortion loss, the depth
supervision and the orientation loss on rays, the per-image exposure compensation, the robust loss on patches, SSIM) and Adam on one tensor.  No workspace; reached through voxe_hip.ops, which re-exports every name here."""
import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import abi
from .args import GridSpec, RenderParams, _check_rays, _require_buffer, resolve_rng
from .gridops import _check_densities, _sampling_inputs
from .runtime import VoxeError, check, ensure_gfx950, f32c, lib, ptr, require_device, stream_ptr
from .workspace import _scratch_for, wrote


class _ScalarLossFn(torch.autograd.Function):
    """loss = entry(x[, other]) by one library call that writes the value and -- for an upstream gradient of 1.0, scaled in the
    backward -- the gradient w.r.t. `x` in one launch sequence.  `plan(x, other)` (both dense float32) checks the shapes and
    returns ((scratch-size query, its arguments), the call's leading arguments)."""

    @staticmethod
    def forward(ctx, x, other, entry, symbol, plan):
        require_device(x, entry)
        a = f32c(x.detach())
        b = None if other is None else f32c(other.detach())
        (scratch_query, scratch_args), lead = plan(a, b)
        device = a.device
        ensure_gfx950(device)
        L = lib()
        with torch.cuda.device(device):
            sc = _scratch_for(device, getattr(L, scratch_query)(*scratch_args))
            loss = torch.empty((), dtype=torch.float32, device=device)
            d_a = torch.empty_like(a) if ctx.needs_input_grad[0] else None
            check(getattr(L, symbol)(*lead, 1.0, ptr(loss), ptr(d_a), 0, ptr(sc), sc.numel(), stream_ptr(device)), symbol)
        ctx.save_for_backward(d_a)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_a,) = ctx.saved_tensors
        return (None if d_a is None else d_a * g), None, None, None, None


def density_correlation_loss(sds_density: torch.Tensor, regular_density: torch.Tensor) -> torch.Tensor:
    """1 - corr(sds, regular)  (thre3d_atom/modules/sds_trainer.py:507-524); differentiable w.r.t. sds."""
    def plan(a, b):
        if a.numel() != b.numel():
            raise VoxeError("density_correlation_loss: shape mismatch")
        return ("voxe_dcl_scratch_bytes", (a.numel(),)), (ptr(a), ptr(b), a.numel())
    return _ScalarLossFn.apply(sds_density, regular_density, "density_correlation_loss", "voxe_dcl_fwd_bwd", plan)


def density_diff_loss(sds_density: torch.Tensor, regular_density: torch.Tensor, l2_mode: bool) -> torch.Tensor:
    """mse_loss (l2_mode) / l1_loss of the two density grids (thre3d_atom/modules/sds_trainer.py:494-503); differentiable w.r.t. sds."""
    kind = abi.DREG_L2 if l2_mode else abi.DREG_L1

    def plan(a, b):
        if a.numel() != b.numel():
            raise VoxeError("density_diff_loss: shape mismatch")
        return ("voxe_dcl_scratch_bytes", (a.numel(),)), (ptr(a), ptr(b), a.numel(), int(kind))
    return _ScalarLossFn.apply(sds_density, regular_density, "density_diff_loss", "voxe_density_diff_fwd_bwd", plan)


def feature_correlation_loss(sds_features: torch.Tensor, regular_features: torch.Tensor) -> torch.Tensor:
    """sum_v (sum_c sigmoid(f_vc) - sigmoid(r_vc))^2 (thre3d_atom/modules/sds_trainer.py:526-534); differentiable w.r.t. sds."""
    def plan(f, r):
        if f.shape != r.shape or f.dim() < 1:
            raise VoxeError("feature_correlation_loss: shape mismatch")
        F = int(f.shape[-1])
        nvox = f.numel() // F
        return ("voxe_dcl_scratch_bytes", (nvox,)), (ptr(f), ptr(r), nvox, F)
    return _ScalarLossFn.apply(sds_features, regular_features, "feature_correlation_loss", "voxe_feature_correlation_fwd_bwd", plan)


def tv_loss_on_grid(grid: torch.Tensor) -> torch.Tensor:
    """(mean|dx| + mean|dy| + mean|dz|)/3  (thre3d_atom/modules/sds_trainer.py:563-567)."""
    def plan(gr, _):
        if gr.dim() != 4:
            raise VoxeError("tv_loss_on_grid expects [X,Y,Z,C]")
        return ("voxe_tv_scratch_bytes", tuple(gr.shape)), (ptr(gr), *gr.shape)
    return _ScalarLossFn.apply(grid, None, "tv_loss_on_grid", "voxe_tv_fwd_bwd", plan)


@torch.no_grad()
def adam_step_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
               step: int, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8) -> None:
    """In-place torch.optim.Adam update of one tensor (weight_decay=0, amsgrad=False)."""
    for name, t in (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        _require_buffer("adam_step_", name, t, numel=param.numel())
    device = param.device
    ensure_gfx950(device)
    with torch.cuda.device(device):
        check(lib().voxe_adam_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(),
                                   float(lr), float(beta1), float(beta2), float(eps), int(step),
                                   stream_ptr(device)), "voxe_adam_step")
    wrote(param, exp_avg, exp_avg_sq)


@torch.no_grad()
def attn_masked_l1(render: torch.Tensor, attn_map: torch.Tensor):
    """voxe_attn_masked_l1: calc_loss_on_attn_grid (modules/refinement_functions.py:42-77) and its gradient w.r.t. the render.
    Returns (loss [scalar tensor], d_render like `render`)."""
    require_device(render, "attn_masked_l1 (render)")
    require_device(attn_map, "attn_masked_l1 (attn_map)")
    r, m = f32c(render.detach()).reshape(-1), f32c(attn_map.detach()).reshape(-1)
    if r.numel() != m.numel():
        raise VoxeError(f"attn_masked_l1: render ({r.numel()}) and map ({m.numel()}) differ in size")
    device = r.device
    ensure_gfx950(device)
    L = lib()
    d_r = torch.empty_like(r)
    loss = torch.zeros((), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        sc = _scratch_for(device, L.voxe_attn_masked_l1_scratch_bytes())
        check(L.voxe_attn_masked_l1(ptr(r), ptr(m), r.numel(), ptr(d_r), ptr(loss), ptr(sc), sc.numel(), stream_ptr(device)),
              "voxe_attn_masked_l1")
    return loss, d_r.reshape(render.shape)


# ------------------------------------------------------------------------------------------------
# distortion loss on rays (DESIGN.md section 4 "Distortion"): reads the raw densities only, no workspace; differentiable w.r.t.
# the densities
# ------------------------------------------------------------------------------------------------
def distortion_fwd_bwd(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor,
                       jitter: Optional[torch.Tensor] = None, rng: Tuple[int, int] = (0, 0), grad_scale: float = 1.0,
                       want_loss: bool = True, want_ray_loss: bool = False, d_densities: Optional[torch.Tensor] = None,
                       accumulate: bool = False, lanes: int = 0):
    """voxe_distortion_fwd_bwd as it stands: (loss [] or None, ray_loss [R] or None); `d_densities` (contiguous float32 of the
    densities' shape, or None) receives grad_scale * dloss/draw, added to its contents when `accumulate`.  `lanes` (test aid):
    1 / 2 / 4 / 8 pins the kernel's lanes per ray for this call, 0 = chosen by R."""
    _check_densities(densities, "distortion_loss")
    _check_rays("distortion_loss", rays_o, rays_d, jitter, params.num_samples)
    device = densities.device
    if d_densities is not None:
        _require_buffer("distortion_loss", "d_densities", d_densities, shape=densities.shape, device=device)
    g, c, dens, ro, rd, jit = _sampling_inputs(spec, params, densities, rays_o, rays_d, jitter, rng)
    R = ro.shape[0]
    L = lib()
    with torch.cuda.device(device):
        loss = torch.zeros((), dtype=torch.float32, device=device) if want_loss else None
        ray_loss = torch.empty((R,), dtype=torch.float32, device=device) if want_ray_loss else None
        sc = _scratch_for(device, L.voxe_distortion_scratch_bytes(R)) if want_loss else None
        if lanes:
            check(L.voxe_distortion_debug_lanes(int(lanes)), "voxe_distortion_debug_lanes")
        try:
            check(L.voxe_distortion_fwd_bwd(C.byref(g), C.byref(c), ptr(ro), ptr(rd), R, ptr(jit), float(grad_scale), ptr(loss),
                                            ptr(ray_loss), ptr(d_densities), 1 if accumulate else 0, ptr(sc),
                                            sc.numel() if sc is not None else 0, stream_ptr(device)), "voxe_distortion_fwd_bwd")
        finally:
            if lanes:
                L.voxe_distortion_debug_lanes(0)
    wrote(d_densities)
    return loss, ray_loss


class _DistortionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, densities, spec, params, rays_o, rays_d, jitter, rng, return_ray_loss, lanes):
        d_d = torch.empty_like(f32c(densities.detach())) if ctx.needs_input_grad[0] else None
        loss, ray_loss = distortion_fwd_bwd(spec, params, densities, rays_o, rays_d, jitter, rng, want_ray_loss=return_ray_loss,
                                            d_densities=d_d, lanes=lanes)
        ctx.save_for_backward(d_d)
        if return_ray_loss:
            ctx.mark_non_differentiable(ray_loss)
            return loss, ray_loss
        return loss

    @staticmethod
    def backward(ctx, g, *_):
        (d_d,) = ctx.saved_tensors
        return (None if d_d is None else d_d * g,) + (None,) * 8


def distortion_loss(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor,
                    jitter: Optional[torch.Tensor] = None, rng: Optional[Tuple[int, int]] = None, return_ray_loss: bool = False,
                    _lanes: int = 0):
    """Distortion loss of flat rays (mip-NeRF 360; DVGOv2's O(S) evaluation): the mean over rays of
    L_r = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i on depths normalised by params.near / params.far, with the samples
    and weights `render` uses for the same params, jitter and rng (`rng` follows render's rule: None = a fresh stream when
    params.perturb and no jitter is given).  A scalar tensor, differentiable w.r.t. `densities` (the gradient is computed in the
    forward, only when it is needed); return_ray_loss=True: (loss, L_r [R], not differentiable)."""
    rng = resolve_rng(params, jitter, rng)
    return _DistortionFn.apply(densities, spec, params, rays_o, rays_d, jitter, rng, bool(return_ray_loss), int(_lanes))


# ------------------------------------------------------------------------------------------------
# depth supervision: ray-termination loss towards per-ray depth targets: reads the raw densities only,
# no workspace; differentiable w.r.t. the densities
# ------------------------------------------------------------------------------------------------
DEPTH_EPS = 1e-5   # DS-NeRF's


def _per_ray(entry: str, name: str, t: Optional[torch.Tensor], R: int, device) -> Optional[torch.Tensor]:
    """a per-ray input [R] as dense float32 on the rays' device"""
    if t is None:
        return None
    require_device(t, f"{entry} ({name})")
    if t.numel() != R or t.device != device:
        raise VoxeError(f"{entry}: {name} must hold one value per ray ({R}) on {device}; got {tuple(t.shape)} on {t.device}")
    return f32c(t.detach().reshape(R))


def depth_fwd_bwd(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor,
                  target_depth: torch.Tensor, target_sigma: torch.Tensor, ray_weight: Optional[torch.Tensor] = None,
                  jitter: Optional[torch.Tensor] = None, rng: Tuple[int, int] = (0, 0), eps: float = DEPTH_EPS,
                  grad_scale: float = 1.0, want_loss: bool = True, want_ray_loss: bool = False,
                  d_densities: Optional[torch.Tensor] = None, accumulate: bool = False, lanes: int = 0):
    """voxe_depth_fwd_bwd as it stands: (loss [] or None, ray_loss [R] or None); `d_densities` (contiguous float32 of the
    densities' shape, or None) receives grad_scale * dloss/draw, added to its contents when `accumulate`.  `lanes` (test aid):
    1 / 2 / 4 / 8 pins the kernel's lanes per ray for this call, 0 = chosen by R."""
    _check_densities(densities, "depth_loss")
    _check_rays("depth_loss", rays_o, rays_d, jitter, params.num_samples)
    device = densities.device
    if d_densities is not None:
        _require_buffer("depth_loss", "d_densities", d_densities, shape=densities.shape, device=device)
    g, c, dens, ro, rd, jit = _sampling_inputs(spec, params, densities, rays_o, rays_d, jitter, rng)
    R = ro.shape[0]
    td, ts, rw = (_per_ray("depth_loss", n, t, R, device) for n, t in (("target_depth", target_depth), ("target_sigma", target_sigma),
                                                                       ("ray_weight", ray_weight)))
    if td is None or ts is None:
        raise VoxeError("depth_loss: target_depth and target_sigma are required")
    L = lib()
    with torch.cuda.device(device):
        loss = torch.zeros((), dtype=torch.float32, device=device) if want_loss else None
        ray_loss = torch.empty((R,), dtype=torch.float32, device=device) if want_ray_loss else None
        sc = _scratch_for(device, L.voxe_depth_scratch_bytes(R)) if want_loss else None
        if lanes:
            check(L.voxe_depth_debug_lanes(int(lanes)), "voxe_depth_debug_lanes")
        try:
            check(L.voxe_depth_fwd_bwd(C.byref(g), C.byref(c), ptr(ro), ptr(rd), R, ptr(jit), ptr(td), ptr(ts), ptr(rw), float(eps),
                                       float(grad_scale), ptr(loss), ptr(ray_loss), ptr(d_densities), 1 if accumulate else 0,
                                       ptr(sc), sc.numel() if sc is not None else 0, stream_ptr(device)), "voxe_depth_fwd_bwd")
        finally:
            if lanes:
                L.voxe_depth_debug_lanes(0)
    wrote(d_densities)
    return loss, ray_loss


class _DepthFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, densities, spec, params, rays_o, rays_d, target_depth, target_sigma, ray_weight, jitter, rng, eps,
                return_ray_loss, lanes):
        d_d = torch.empty_like(f32c(densities.detach())) if ctx.needs_input_grad[0] else None
        loss, ray_loss = depth_fwd_bwd(spec, params, densities, rays_o, rays_d, target_depth, target_sigma, ray_weight, jitter, rng,
                                       eps=eps, want_ray_loss=return_ray_loss, d_densities=d_d, lanes=lanes)
        ctx.save_for_backward(d_d)
        if return_ray_loss:
            ctx.mark_non_differentiable(ray_loss)
            return loss, ray_loss
        return loss

    @staticmethod
    def backward(ctx, g, *_):
        (d_d,) = ctx.saved_tensors
        return (None if d_d is None else d_d * g,) + (None,) * 12


def depth_loss(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor,
               target_depth: torch.Tensor, target_sigma: torch.Tensor, ray_weight: Optional[torch.Tensor] = None,
               jitter: Optional[torch.Tensor] = None, rng: Optional[Tuple[int, int]] = None, eps: float = DEPTH_EPS,
               return_ray_loss: bool = False, _lanes: int = 0):
    """Ray-termination loss of flat rays towards depth targets (DS-NeRF): the mean over rays of
    omega_r L_r, L_r = -sum_k exp(-(z_k - D_r)^2 / (2 s_r^2)) dz_k log(w_k + eps), with the samples and weights `render` uses for
    the same params, jitter and rng (`rng` follows render's rule).  target_depth D, target_sigma s > 0 (both in the units of the
    sample depths) and ray_weight omega >= 0 (None = 1) hold one value per ray and receive no gradient.  A scalar tensor,
    differentiable w.r.t. `densities` (the gradient is computed in the forward, only when it is needed);
    return_ray_loss=True: (loss, L_r [R], not differentiable)."""
    for name, t in (("target_depth", target_depth), ("target_sigma", target_sigma), ("ray_weight", ray_weight)):
        if t is not None and t.requires_grad:
            raise VoxeError(f"depth_loss: {name} receives no gradient; detach it")
    if not (eps > 0.0 and eps < float("inf")):
        raise VoxeError(f"depth_loss: eps must be finite and > 0; got {eps}")
    rng = resolve_rng(params, jitter, rng)
    return _DepthFn.apply(densities, spec, params, rays_o, rays_d, target_depth, target_sigma, ray_weight, jitter, rng, float(eps),
                          bool(return_ray_loss), int(_lanes))


# ------------------------------------------------------------------------------------------------
# orientation loss on rays: reads the raw densities only, no workspace; differentiable w.r.t. the
# densities
# ------------------------------------------------------------------------------------------------
ORIENTATION_NORMAL_EPS = 1e-2   # a guard, not a tuned value (see orientation_loss)


def orientation_fwd_bwd(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor,
                        ray_weight: Optional[torch.Tensor] = None, jitter: Optional[torch.Tensor] = None,
                        rng: Tuple[int, int] = (0, 0), normal_eps: float = ORIENTATION_NORMAL_EPS, grad_scale: float = 1.0,
                        want_loss: bool = True, want_ray_loss: bool = False, d_densities: Optional[torch.Tensor] = None,
                        accumulate: bool = False, lanes: int = 0):
    """voxe_orientation_fwd_bwd as it stands: (loss [] or None, ray_loss [R] or None); `d_densities` (contiguous float32 of the
    densities' shape, or None) receives grad_scale * dloss/draw, added to its contents when `accumulate`.  `lanes` (test aid):
    1 / 2 / 4 / 8 pins the kernel's lanes per ray for this call, 0 = chosen by R."""
    _check_densities(densities, "orientation_loss")
    _check_rays("orientation_loss", rays_o, rays_d, jitter, params.num_samples)
    device = densities.device
    if d_densities is not None:
        _require_buffer("orientation_loss", "d_densities", d_densities, shape=densities.shape, device=device)
    g, c, dens, ro, rd, jit = _sampling_inputs(spec, params, densities, rays_o, rays_d, jitter, rng)
    R = ro.shape[0]
    rw = _per_ray("orientation_loss", "ray_weight", ray_weight, R, device)
    L = lib()
    with torch.cuda.device(device):
        loss = torch.zeros((), dtype=torch.float32, device=device) if want_loss else None
        ray_loss = torch.empty((R,), dtype=torch.float32, device=device) if want_ray_loss else None
        sc = _scratch_for(device, L.voxe_orientation_scratch_bytes(R)) if want_loss else None
        if lanes:
            check(L.voxe_orientation_debug_lanes(int(lanes)), "voxe_orientation_debug_lanes")
        try:
            check(L.voxe_orientation_fwd_bwd(C.byref(g), C.byref(c), ptr(ro), ptr(rd), R, ptr(jit), ptr(rw), float(normal_eps),
                                             float(grad_scale), ptr(loss), ptr(ray_loss), ptr(d_densities), 1 if accumulate else 0,
                                             ptr(sc), sc.numel() if sc is not None else 0, stream_ptr(device)),
                  "voxe_orientation_fwd_bwd")
        finally:
            if lanes:
                L.voxe_orientation_debug_lanes(0)
    wrote(d_densities)
    return loss, ray_loss


class _OrientationFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, densities, spec, params, rays_o, rays_d, ray_weight, jitter, rng, normal_eps, return_ray_loss, lanes):
        d_d = torch.empty_like(f32c(densities.detach())) if ctx.needs_input_grad[0] else None
        loss, ray_loss = orientation_fwd_bwd(spec, params, densities, rays_o, rays_d, ray_weight, jitter, rng, normal_eps=normal_eps,
                                             want_ray_loss=return_ray_loss, d_densities=d_d, lanes=lanes)
        ctx.save_for_backward(d_d)
        if return_ray_loss:
            ctx.mark_non_differentiable(ray_loss)
            return loss, ray_loss
        return loss

    @staticmethod
    def backward(ctx, g, *_):
        (d_d,) = ctx.saved_tensors
        return (None if d_d is None else d_d * g,) + (None,) * 10


def orientation_loss(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor,
                     ray_weight: Optional[torch.Tensor] = None, jitter: Optional[torch.Tensor] = None,
                     rng: Optional[Tuple[int, int]] = None, normal_eps: float = ORIENTATION_NORMAL_EPS,
                     return_ray_loss: bool = False, _lanes: int = 0):
    """Orientation loss of flat rays (Ref-NeRF): the mean over rays of omega_r L_r, L_r = sum_k w_k max(0, n_k . u_r)^2, with the
    samples and weights `render` uses for the same params, jitter and rng (`rng` follows render's rule), u_r the unit ray
    direction and n_k = -G_k / sqrt(|G_k|^2 + normal_eps^2) the density-gradient normal `render_normals` composites, guarded by
    `normal_eps` >= 0 in the units of the gradient G.  The default 1e-2 is a guard, not a tuned value: about 2e-4 of a unit
    density step across one voxel of a 160^3 grid over [-1.5, 1.5].  ray_weight omega >= 0 (None = 1) holds one value per ray
    and receives no gradient, nor do the rays.  A scalar tensor, differentiable w.r.t. `densities` through the weights and
    through the normals (the gradient is computed in the forward, only when it is needed); return_ray_loss=True:
    (loss, L_r [R], not differentiable)."""
    if ray_weight is not None and ray_weight.requires_grad:
        raise VoxeError("orientation_loss: ray_weight receives no gradient; detach it")
    if not (normal_eps >= 0.0 and normal_eps < float("inf")):
        raise VoxeError(f"orientation_loss: normal_eps must be finite and >= 0; got {normal_eps}")
    rng = resolve_rng(params, jitter, rng)
    return _OrientationFn.apply(densities, spec, params, rays_o, rays_d, ray_weight, jitter, rng, float(normal_eps),
                                bool(return_ray_loss), int(_lanes))


# ------------------------------------------------------------------------------------------------
# per-image exposure compensation: no grid, no workspace; differentiable w.r.t. the colours and the
# parameters
# ------------------------------------------------------------------------------------------------
_EXPOSURE_KINDS = {"l1": abi.DREG_L1, "l2": abi.DREG_L2}
EXPOSURE_FIT_SUMS = 25


def _exposure_inputs(entry: str, colour: torch.Tensor, target: Optional[torch.Tensor], image_ids: torch.Tensor, delta: torch.Tensor):
    """(x [R,3], y [R,3] or None, ids [R] int32, delta [N,12]) as dense tensors on the colours' device"""
    require_device(colour, f"{entry} (colour)")
    device = colour.device
    if colour.dim() != 2 or colour.shape[1] != 3:
        raise VoxeError(f"{entry}: colour must be [R,3]; got {tuple(colour.shape)}")
    R = colour.shape[0]
    if target is not None and (target.shape != colour.shape or target.device != device):
        raise VoxeError(f"{entry}: target must be {tuple(colour.shape)} on {device}; got {tuple(target.shape)} on {target.device}")
    if image_ids.dtype not in (torch.int32, torch.int64) or image_ids.numel() != R or image_ids.device != device:
        raise VoxeError(f"{entry}: image_ids must hold one integer per ray ({R}) on {device}; got {image_ids.dtype} "
                        f"{tuple(image_ids.shape)} on {image_ids.device}")
    if delta.dim() != 2 or delta.shape[1] != 12 or delta.shape[0] < 1 or delta.device != device:
        raise VoxeError(f"{entry}: delta must be [N,12], N >= 1, on {device}; got {tuple(delta.shape)} on {delta.device}")
    ids = image_ids.detach().reshape(R).to(torch.int32).contiguous()
    return f32c(colour.detach()), (None if target is None else f32c(target.detach())), ids, f32c(delta.detach())


def exposure_fwd_bwd(colour: torch.Tensor, target: torch.Tensor, image_ids: torch.Tensor, delta: torch.Tensor, kind: str = "l1",
                     ray_weight: Optional[torch.Tensor] = None, grad_scale: float = 1.0, want_loss: bool = True,
                     want_mse: bool = False, want_corrected: bool = False, d_colour: Optional[torch.Tensor] = None,
                     d_delta: Optional[torch.Tensor] = None, accumulate: bool = False):
    """voxe_exposure_fwd_bwd as it stands: (loss [] or None, mse [] or None, corrected [R,3] or None); `d_colour` (contiguous
    float32 [R,3], or None) receives grad_scale * dloss/dcolour, `d_delta` (contiguous float32 [N,12], or None)
    grad_scale * dloss/ddelta, added to its contents when `accumulate`.  image_ids outside [0, N) are clamped on the device:
    check a dataset's ids once, not per call."""
    if kind not in _EXPOSURE_KINDS:
        raise VoxeError(f"exposure_loss: kind must be 'l1' or 'l2'; got {kind!r}")
    x, y, ids, dl = _exposure_inputs("exposure_loss", colour, target, image_ids, delta)
    device = x.device
    R, N = x.shape[0], dl.shape[0]
    if d_colour is not None:
        _require_buffer("exposure_loss", "d_colour", d_colour, shape=x.shape, device=device)
    if d_delta is not None:
        _require_buffer("exposure_loss", "d_delta", d_delta, shape=dl.shape, device=device)
    rw = _per_ray("exposure_loss", "ray_weight", ray_weight, R, device)
    ensure_gfx950(device)
    L = lib()
    with torch.cuda.device(device):
        loss = torch.empty((), dtype=torch.float32, device=device) if want_loss else None
        mse = torch.empty((), dtype=torch.float32, device=device) if want_mse else None
        corrected = torch.empty((R, 3), dtype=torch.float32, device=device) if want_corrected else None
        sc = _scratch_for(device, L.voxe_exposure_scratch_bytes(R, N)) if (want_loss or want_mse or d_delta is not None) else None
        check(L.voxe_exposure_fwd_bwd(ptr(x), ptr(y), ptr(ids), R, ptr(dl), N, _EXPOSURE_KINDS[kind], ptr(rw), float(grad_scale),
                                      ptr(loss), ptr(mse), ptr(corrected), ptr(d_colour), ptr(d_delta), 1 if accumulate else 0,
                                      ptr(sc), sc.numel() if sc is not None else 0, stream_ptr(device)),
              "voxe_exposure_fwd_bwd")
    wrote(d_colour)
    wrote(d_delta)
    return loss, mse, corrected


class _ExposureFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colour, delta, target, image_ids, kind, ray_weight, return_corrected):
        d_c = torch.empty_like(f32c(colour.detach())) if ctx.needs_input_grad[0] else None
        d_d = torch.empty_like(f32c(delta.detach())) if ctx.needs_input_grad[1] else None
        loss, mse, corrected = exposure_fwd_bwd(colour, target, image_ids, delta, kind, ray_weight, want_mse=True,
                                                want_corrected=return_corrected, d_colour=d_c, d_delta=d_d)
        ctx.save_for_backward(d_c, d_d)
        if return_corrected:
            ctx.mark_non_differentiable(mse, corrected)
            return loss, mse, corrected
        ctx.mark_non_differentiable(mse)
        return loss, mse

    @staticmethod
    def backward(ctx, g, *_):
        d_c, d_d = ctx.saved_tensors
        return (None if d_c is None else d_c * g, None if d_d is None else d_d * g) + (None,) * 5


def exposure_loss(colour: torch.Tensor, target: torch.Tensor, image_ids: torch.Tensor, delta: torch.Tensor, kind: str = "l1",
                  ray_weight: Optional[torch.Tensor] = None, return_corrected: bool = False):
    """Photometric loss under a per-image affine colour transform: with A = I + dA_n, c' = A colour + db_n for the image
    n = image_ids[r] of ray r and delta[n] = (dA row-major, db), the mean over the 3R elements of omega_r |c' - target| ('l1',
    sign(0) = 0 like torch's l1_loss) or omega_r (c' - target)^2 ('l2').  Returns (loss [], mse []), with return_corrected
    (loss, mse, corrected [R,3]): `loss` is differentiable w.r.t. `colour` and `delta` (both gradients are computed in the forward,
    each only when its input requires one; d_delta is a fixed-point segmented reduction, bit-reproducible); `mse`, the plain mean
    of (c' - target)^2 for a PSNR line, and `corrected` are not.  target, image_ids and ray_weight (omega >= 0, None = 1) receive
    no gradient.  image_ids (int32 or int64, [R]) outside [0, N) are clamped on the device."""
    for name, t in (("target", target), ("image_ids", image_ids), ("ray_weight", ray_weight)):
        if t is not None and t.requires_grad:
            raise VoxeError(f"exposure_loss: {name} receives no gradient; detach it")
    if kind not in _EXPOSURE_KINDS:
        raise VoxeError(f"exposure_loss: kind must be 'l1' or 'l2'; got {kind!r}")
    _exposure_inputs("exposure_loss", colour, target, image_ids, delta)
    return _ExposureFn.apply(colour, delta, target, image_ids, kind, ray_weight, bool(return_corrected))


def exposure_apply_bwd(colour: torch.Tensor, image_ids: torch.Tensor, delta: torch.Tensor, d_corrected: torch.Tensor,
                       d_colour: Optional[torch.Tensor] = None, d_delta: Optional[torch.Tensor] = None,
                       accumulate: bool = False) -> None:
    """voxe_exposure_apply_bwd as it stands: `d_colour` [R,3] receives A^T d_corrected, `d_delta` [N,12] the per-image sums of
    (d_corrected x^T, d_corrected), added to its contents when `accumulate`.  Range of the fixed point: see exposure_apply."""
    x, g, ids, dl = _exposure_inputs("exposure_apply", colour, d_corrected, image_ids, delta)
    device = x.device
    R, N = x.shape[0], dl.shape[0]
    if d_colour is not None:
        _require_buffer("exposure_apply", "d_colour", d_colour, shape=x.shape, device=device)
    if d_delta is not None:
        _require_buffer("exposure_apply", "d_delta", d_delta, shape=dl.shape, device=device)
    ensure_gfx950(device)
    L = lib()
    with torch.cuda.device(device):
        sc = _scratch_for(device, L.voxe_exposure_scratch_bytes(R, N)) if d_delta is not None else None
        check(L.voxe_exposure_apply_bwd(ptr(x), ptr(ids), R, ptr(dl), N, ptr(g), ptr(d_colour), ptr(d_delta), 1 if accumulate else 0,
                                        ptr(sc), sc.numel() if sc is not None else 0, stream_ptr(device)), "voxe_exposure_apply_bwd")
    wrote(d_colour)
    wrote(d_delta)


class _ExposureApplyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colour, delta, image_ids):
        x, _, ids, dl = _exposure_inputs("exposure_apply", colour, None, image_ids, delta)
        device = x.device
        ensure_gfx950(device)
        R = x.shape[0]
        with torch.cuda.device(device):
            corrected = torch.empty((R, 3), dtype=torch.float32, device=device)
            # (the target is read for the residual only; with every reduction skipped the colours stand in for it)
            check(lib().voxe_exposure_fwd_bwd(ptr(x), ptr(x), ptr(ids), R, ptr(dl), dl.shape[0], abi.DREG_L2, None, 1.0, None, None,
                                              ptr(corrected), None, None, 0, None, 0, stream_ptr(device)), "voxe_exposure_fwd_bwd")
        ctx.save_for_backward(x, dl, ids)
        return corrected

    @staticmethod
    def backward(ctx, g):
        x, dl, ids = ctx.saved_tensors
        d_c = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        d_d = torch.empty_like(dl) if ctx.needs_input_grad[1] else None
        if d_c is not None or d_d is not None:
            exposure_apply_bwd(x, ids, dl, g, d_colour=d_c, d_delta=d_d)
        return d_c, d_d, None


def exposure_apply(colour: torch.Tensor, image_ids: torch.Tensor, delta: torch.Tensor) -> torch.Tensor:
    """c' = (I + dA_n) colour + db_n per ray, n = image_ids[r]: the `corrected` output of voxe_exposure_fwd_bwd alone, [R,3],
    for a loss that sees the corrected colours themselves (the trainer's SSIM term); differentiable w.r.t. `colour` and `delta`
    (voxe_exposure_apply_bwd, the same fixed-point reduction).  The backward's fixed point assumes the upstream gradient of a
    mean over the batch, entries near 1 / R: per image the sums of |dL/dc'| and of |dL/dc' x| must stay below 2^31 / R',
    R' = R rounded up to a power of two, or d_delta wraps -- a loss summed, not averaged, over 2^20 rays and more does not fit,
    and entries below 2^-33 / R' are lost."""
    if image_ids.requires_grad:
        raise VoxeError("exposure_apply: image_ids receives no gradient")
    _exposure_inputs("exposure_apply", colour, None, image_ids, delta)
    return _ExposureApplyFn.apply(colour, delta, image_ids)


def exposure_fit_sums(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """voxe_exposure_fit_sums as it stands: x, y [N,P,3] float32 -> sums [N,25] float64 (include/voxe.h names the 25)"""
    for name, t in (("x", x), ("y", y)):
        require_device(t, f"fit_affine_colour ({name})")
    if x.dim() != 3 or x.shape[2] != 3 or x.shape[0] < 1 or x.shape[1] < 1 or x.shape != y.shape or x.device != y.device:
        raise VoxeError(f"fit_affine_colour: x and y must be [N,P,3] of one shape on one device, N, P >= 1; got {tuple(x.shape)} "
                        f"and {tuple(y.shape)}")
    device = x.device
    ensure_gfx950(device)
    xd, yd = f32c(x.detach()), f32c(y.detach())
    N, P = int(x.shape[0]), int(x.shape[1])
    L = lib()
    with torch.cuda.device(device):
        sums = torch.empty((N, EXPOSURE_FIT_SUMS), dtype=torch.float64, device=device)
        need = L.voxe_exposure_fit_scratch_bytes(N, P)
        if need == 0:
            raise VoxeError(f"fit_affine_colour: {tuple(x.shape)} is outside the limits of voxe_exposure_fit_sums")
        sc = _scratch_for(device, need)
        check(L.voxe_exposure_fit_sums(ptr(xd), ptr(yd), N, P, ptr(sums), ptr(sc), sc.numel(), stream_ptr(device)),
              "voxe_exposure_fit_sums")
    return sums


_FIT_UPPER = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
FIT_RIDGE = 1e-11   # relative to the largest eigenvalue of an image's 4 x 4 system


def solve_affine_colour(sums: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(A [N,3,3], b [N,3]) in float64 on the CPU from sums [N,25]: per image the least-squares affine y ~ A x + b.  The 4 x 4
    system is solved through its eigenvalues w_i as w_i / (w_i^2 + (FIT_RIDGE w_max)^2): a ridge that changes a well-posed image
    by (FIT_RIDGE cond)^2, below rounding up to cond 1e4, and keeps a degenerate one (constant colour, P < 4) finite, at the
    solution of least norm."""
    s = sums.detach().to("cpu", torch.float64)
    N = s.shape[0]
    G = torch.zeros((N, 4, 4), dtype=torch.float64)
    for k, (i, j) in enumerate(_FIT_UPPER):
        G[:, i, j] = s[:, k]
        G[:, j, i] = s[:, k]
    h = s[:, 10:22].reshape(N, 4, 3)
    w, V = torch.linalg.eigh(G)
    lam = FIT_RIDGE * w[:, -1:].clamp_min(torch.finfo(torch.float64).tiny)
    inv = w / (w * w + lam * lam)
    theta = V @ (inv.unsqueeze(-1) * (V.transpose(1, 2) @ h))   # [N,4,3]: rows A^T then b
    return theta[:, :3, :].transpose(1, 2).contiguous(), theta[:, 3, :].contiguous()


def fit_affine_colour(x: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The least-squares affine colour transform of each image, y ~ A x + b over its P pixels (the colour correction of
    mip-NeRF 360's and RawNeRF's colour-corrected metrics): x, y [N,P,3] float32 on the device -> (A [N,3,3], b [N,3]) float64 on
    the device.  The sums are formed on the device in double (voxe_exposure_fit_sums, bit-reproducible), the 4 x 4 systems are
    solved on the host in float64 (solve_affine_colour); no gradient."""
    sums = exposure_fit_sums(x, y)
    A, b = solve_affine_colour(sums)
    return A.to(x.device), b.to(x.device)


# ------------------------------------------------------------------------------------------------
# robust photometric loss on pixel patches: no grid, no workspace; differentiable w.r.t. x
# ------------------------------------------------------------------------------------------------
ROBUST_MIN_PATCH, ROBUST_MAX_PATCH = 4, 64


def robust_parameters(M: int, P: int, inlier_quantile: float = 0.5, smooth_min_count: int = 5,
                      patch_inlier_fraction: Optional[float] = 0.6) -> Tuple[int, int, int]:
    """(rank, smooth_min, patch_min) of voxe_robust_fwd_bwd for M = N P^2 pixels in patches of side P: the 0-based rank
    min(M - 1, max(0, ceil(q M) - 1)) of the quantile q (in double), the 3x3 count as it stands, and ceil(f P^2) of the patch
    fraction f, at least 1; f = None switches the patch rule off (P^2 + 1)."""
    q = float(inlier_quantile)
    if not 0.0 <= q <= 1.0:
        raise VoxeError(f"robust_loss: inlier_quantile must lie in [0, 1]; got {inlier_quantile}")
    if int(smooth_min_count) != smooth_min_count or not 1 <= smooth_min_count <= 9:
        raise VoxeError(f"robust_loss: smooth_min_count must be an integer in 1..9; got {smooth_min_count}")
    if patch_inlier_fraction is not None and not 0.0 <= float(patch_inlier_fraction) <= 1.0:
        raise VoxeError(f"robust_loss: patch_inlier_fraction must lie in [0, 1] or be None (off); got {patch_inlier_fraction}")
    rank = min(M - 1, max(0, math.ceil(q * M) - 1))
    patch_min = P * P + 1 if patch_inlier_fraction is None else max(1, math.ceil(float(patch_inlier_fraction) * (P * P)))
    return rank, int(smooth_min_count), patch_min


def _check_robust_patches(entry: str, x: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor]) -> None:
    if x.dim() != 4 or x.shape != y.shape or x.device != y.device:
        raise VoxeError(f"{entry}: x and y must be [N,P,P,C] of one shape on one device; got {tuple(x.shape)} on {x.device} and "
                        f"{tuple(y.shape)} on {y.device}")
    N, P, P2, Cn = x.shape
    if (N < 1 or P != P2 or P % 2 or not ROBUST_MIN_PATCH <= P <= ROBUST_MAX_PATCH or not 1 <= Cn <= 4
            or N * P * P >= 1 << 31):
        raise VoxeError(f"{entry}: needs N >= 1 square patches of an even side in {ROBUST_MIN_PATCH}..{ROBUST_MAX_PATCH}, 1..4 "
                        f"channels (channel-last) and fewer than 2^31 pixels; got {tuple(x.shape)}")
    for name, t in (("x", x), ("y", y)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise VoxeError(f"{entry}: {name} must be a contiguous float32 tensor; got {t.dtype}, contiguous={t.is_contiguous()}")
        require_device(t, f"{entry} ({name})")
    if mask is not None:
        _require_buffer(entry, "mask", mask, shape=(N, P, P), device=x.device, dtype=torch.uint8)


def robust_fwd_bwd(x: torch.Tensor, y: torch.Tensor, rank: int = 0, smooth_min: int = 5, patch_min: int = 1, kind: str = "l1",
                   mask: Optional[torch.Tensor] = None, grad_scale: float = 1.0, want_loss: bool = True, want_mse: bool = True,
                   want_tau: bool = True, want_mask: bool = True, want_stats: bool = True, d_x: Optional[torch.Tensor] = None):
    """voxe_robust_fwd_bwd as it stands: (loss [] or None, mse [] or None, tau [] or None, mask [N,P,P] uint8 or None,
    stats [3] int64 or None); `d_x` (contiguous float32 of x's shape, or None) receives grad_scale * dloss/dx.  With `mask`
    (uint8 [N,P,P]) the weights are (mask != 0), rank / smooth_min / patch_min are ignored and tau and stats are zeros."""
    if kind not in _EXPOSURE_KINDS:
        raise VoxeError(f"robust_loss: kind must be 'l1' or 'l2'; got {kind!r}")
    _check_robust_patches("robust_loss", x, y, mask)
    device = x.device
    if d_x is not None:
        _require_buffer("robust_loss", "d_x", d_x, shape=x.shape, device=device)
    N, P, _, Cn = (int(v) for v in x.shape)
    if mask is None and not (0 <= rank < N * P * P and 1 <= smooth_min <= 9 and 1 <= patch_min <= P * P + 1):
        raise VoxeError(f"robust_loss: needs 0 <= rank < {N * P * P}, smooth_min in 1..9 and 1 <= patch_min <= {P * P + 1}; got "
                        f"{rank}, {smooth_min}, {patch_min}")
    ensure_gfx950(device)
    xd, yd = x.detach(), y.detach()
    L = lib()
    with torch.cuda.device(device):
        loss = torch.empty((), dtype=torch.float32, device=device) if want_loss else None
        mse = torch.empty((), dtype=torch.float32, device=device) if want_mse else None
        tau = torch.empty((), dtype=torch.float32, device=device) if want_tau else None
        mask_out = torch.empty((N, P, P), dtype=torch.uint8, device=device) if want_mask else None
        stats = torch.empty((3,), dtype=torch.int64, device=device) if want_stats else None
        sc = _scratch_for(device, L.voxe_robust_scratch_bytes(N, P, Cn))
        check(L.voxe_robust_fwd_bwd(ptr(xd), ptr(yd), N, P, Cn, _EXPOSURE_KINDS[kind], int(rank), int(smooth_min), int(patch_min),
                                    ptr(mask), float(grad_scale), ptr(loss), ptr(mse), ptr(tau), ptr(mask_out), ptr(stats), ptr(d_x),
                                    ptr(sc), sc.numel(), stream_ptr(device)), "voxe_robust_fwd_bwd")
    wrote(d_x)
    return loss, mse, tau, mask_out, stats


class _RobustFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, rank, smooth_min, patch_min, kind, mask):
        d_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        loss, mse, tau, mask_out, stats = robust_fwd_bwd(x, y, rank, smooth_min, patch_min, kind, mask, d_x=d_x)
        ctx.save_for_backward(d_x)
        ctx.mark_non_differentiable(mse, tau, mask_out, stats)
        return loss, mse, tau, mask_out, stats

    @staticmethod
    def backward(ctx, g, *_):
        (d_x,) = ctx.saved_tensors
        return (None if d_x is None else d_x * g,) + (None,) * 6


def _robust_info(tau, stats, rank, smooth_min, patch_min):
    return {"tau": tau, "stats": stats, "rank": rank, "smooth_min": smooth_min, "patch_min": patch_min}


def robust_loss(x: torch.Tensor, y: torch.Tensor, *, inlier_quantile: float = 0.5, smooth_min_count: int = 5,
                patch_inlier_fraction: Optional[float] = 0.6, kind: str = "l1", mask: Optional[torch.Tensor] = None):
    """RobustNeRF's trimmed photometric loss (Sabour et al. 2023) of two channel-last batches of patches [N,P,P,C], P even in
    4..64, C in 1..4, float32 contiguous on the device -- a render's colour viewed as patches against the photographs.  A pixel
    is an inlier when its squared residual (summed over the channels) is at most the `inlier_quantile` order statistic of the
    batch; an outlier is forgiven when at least `smooth_min_count` of its 3x3 neighbourhood (inside its patch) are inliers, or,
    in the inner half of a patch, when at least `patch_inlier_fraction` of the patch is forgiven (None: rule off).  The loss is
    the mean over all C N P^2 elements of w |x - y| ('l1') or w (x - y)^2 ('l2') with the 0 / 1 mask w a constant.  Returns
    (loss [], mse [], mask [N,P,P] uint8, info): `loss` is differentiable w.r.t. `x` (the gradient is computed in the forward,
    only when x requires one); `mse` is the unmasked mean of (x - y)^2 for a PSNR line; info holds "tau" (the threshold, []),
    "stats" (int64 [3]: the counts of raw inliers, of forgiven pixels, of the mask) and the three integers the call used.  With
    `mask` (uint8 [N,P,P], another call's) the weights are (mask != 0), nothing is selected and tau and stats are zeros.  `y`
    and `mask` receive no gradient."""
    if y.requires_grad:
        raise VoxeError("robust_loss: the target y receives no gradient; detach it")
    if kind not in _EXPOSURE_KINDS:
        raise VoxeError(f"robust_loss: kind must be 'l1' or 'l2'; got {kind!r}")
    _check_robust_patches("robust_loss", x, y, mask)
    N, P = int(x.shape[0]), int(x.shape[1])
    rank, smooth_min, patch_min = robust_parameters(N * P * P, P, inlier_quantile, smooth_min_count, patch_inlier_fraction)
    loss, mse, tau, mask_out, stats = _RobustFn.apply(x, y, rank, smooth_min, patch_min, kind, mask)
    return loss, mse, mask_out, _robust_info(tau, stats, rank, smooth_min, patch_min)


def robust_mask(x: torch.Tensor, y: torch.Tensor, *, inlier_quantile: float = 0.5, smooth_min_count: int = 5,
                patch_inlier_fraction: Optional[float] = 0.6):
    """The mask of robust_loss alone, for composing with other losses: (mask [N,P,P] uint8, info) from the same call with only
    mask_out, tau_out and stats; no gradient."""
    _check_robust_patches("robust_mask", x, y, None)
    N, P = int(x.shape[0]), int(x.shape[1])
    rank, smooth_min, patch_min = robust_parameters(N * P * P, P, inlier_quantile, smooth_min_count, patch_inlier_fraction)
    _, _, tau, mask_out, stats = robust_fwd_bwd(x, y, rank, smooth_min, patch_min, want_loss=False, want_mse=False)
    return mask_out, _robust_info(tau, stats, rank, smooth_min, patch_min)


# ------------------------------------------------------------------------------------------------
# SSIM of channel-last images: no grid, no workspace; differentiable w.r.t. x
# ------------------------------------------------------------------------------------------------
SSIM_WINDOW = 11   # valid windows only: [N,H,W,C] gives an [N,H-10,W-10,C] map


def _check_ssim_images(x: torch.Tensor, y: torch.Tensor) -> None:
    for name, t in (("x", x), ("y", y)):
        require_device(t, f"ssim ({name})")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise VoxeError(f"ssim: {name} must be a contiguous float32 tensor; got {t.dtype}, contiguous={t.is_contiguous()}")
    if x.dim() != 4 or x.shape != y.shape or x.device != y.device:
        raise VoxeError(f"ssim: x and y must be [N,H,W,C] of one shape on one device; got {tuple(x.shape)} and {tuple(y.shape)}")
    N, H, W, Cn = x.shape
    if N < 1 or H < SSIM_WINDOW or W < SSIM_WINDOW or not 1 <= Cn <= 4:
        raise VoxeError(f"ssim: needs N >= 1, H and W >= {SSIM_WINDOW} and 1..4 channels (channel-last); got {tuple(x.shape)}")


def ssim_fwd_bwd(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, grad_scale: float = 1.0, want_mean: bool = True,
                 want_per_image: bool = True, want_map: bool = False, d_x: Optional[torch.Tensor] = None,
                 accumulate: bool = False):
    """voxe_ssim_fwd_bwd as it stands: (mean [] or None, per_image [N] or None, ssim_map [N,H-10,W-10,C] or None); `d_x`
    (contiguous float32 of x's shape, or None) receives grad_scale * dssim/dx, added to its contents when `accumulate`."""
    _check_ssim_images(x, y)
    if not data_range > 0:
        raise VoxeError(f"ssim: data_range must be positive; got {data_range}")
    device = x.device
    if d_x is not None:
        _require_buffer("ssim", "d_x", d_x, shape=x.shape, device=device)
    ensure_gfx950(device)
    N, H, W, Cn = (int(v) for v in x.shape)
    xd, yd = x.detach(), y.detach()
    L = lib()
    with torch.cuda.device(device):
        mean = torch.empty((), dtype=torch.float32, device=device) if want_mean else None
        per_image = torch.empty((N,), dtype=torch.float32, device=device) if want_per_image else None
        ssim_map = (torch.empty((N, H - SSIM_WINDOW + 1, W - SSIM_WINDOW + 1, Cn), dtype=torch.float32, device=device)
                    if want_map else None)
        need = L.voxe_ssim_scratch_bytes(N, H, W, Cn, 1 if d_x is not None else 0)
        if need == 0:
            raise VoxeError(f"ssim: {tuple(x.shape)} has more tiles than one launch holds")
        sc = _scratch_for(device, need)
        check(L.voxe_ssim_fwd_bwd(ptr(xd), ptr(yd), N, H, W, Cn, float(data_range), float(grad_scale), ptr(mean), ptr(per_image),
                                  ptr(ssim_map), ptr(d_x), 1 if accumulate else 0, ptr(sc), sc.numel(), stream_ptr(device)),
              "voxe_ssim_fwd_bwd")
    wrote(d_x)
    return mean, per_image, ssim_map


class _SsimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, data_range):
        d_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        mean, per_image, _ = ssim_fwd_bwd(x, y, data_range, d_x=d_x)
        ctx.save_for_backward(d_x)
        ctx.mark_non_differentiable(per_image)
        return mean, per_image

    @staticmethod
    def backward(ctx, g, *_):
        (d_x,) = ctx.saved_tensors
        return (None if d_x is None else d_x * g), None, None


def ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0):
    """SSIM (Wang et al. 2004: 11 x 11 Gaussian window of sigma 1.5, valid windows only, C1 = (0.01 L)^2, C2 = (0.03 L)^2 with
    L = data_range) of two channel-last batches [N,H,W,C], C in 1..4, float32 contiguous on the device -- a render's colour viewed
    as patches or as an image.  Returns (mean [], per_image [N]): the mean of the (H-10) x (W-10) x C map over the batch and per
    image.  `mean` is differentiable w.r.t. `x` (the gradient is computed in the forward, only when x requires one); `y` is a
    target and receives no gradient, `per_image` is not differentiable."""
    if y.requires_grad:
        raise VoxeError("ssim: the target y receives no gradient; detach it")
    _check_ssim_images(x, y)
    return _SsimFn.apply(x, y, float(data_range))
