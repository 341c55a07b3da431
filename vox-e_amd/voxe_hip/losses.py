"""Losses over libvoxe_hip.so (the scalar regularisers of the SDS edit, the masked attention L1, the distortion loss, the depth
supervision and the orientation loss on rays, SSIM) and Adam on one tensor.  No workspace; reached through voxe_hip.ops, which re-exports every name here."""
import ctypes as C
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
