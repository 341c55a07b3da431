"""torch-level operators over libvoxe_hip.so, the one import surface of the binding.  What runs in a Workspace lives here (render, point
query, fused steps, reconstruction iteration; workspace.py holds the cache protocol); cameras.py, losses.py and gridops.py are
re-exported.  Tensors are plumbing; all compute is in the HIP library.  Nothing here falls back to torch ops or to the CPU oracle."""
import ctypes as C
import dataclasses
from typing import Optional, Tuple

import torch

from . import abi
from . import dispatch as _dispatch
from .args import GridSpec, RenderParams, _check_rays, _moments, _next_rng, _require_buffer, resolve_rng  # noqa: F401
from .background import background_bwd, background_composite, background_fwd_into  # noqa: F401
from .cameras import (cast_rays, cast_rays_bwd, cast_rays_camera, cast_rays_camera_bwd, cast_rays_from_camera,  # noqa: F401
                      cast_rays_from_poses, cast_rays_indexed, random_subset)
from .desc import make_grid_desc, make_render_cfg
from .gridops import (LIFT_MERGE_PER_LANE, LIFT_MERGE_SHIPPED, LIFT_MERGE_WAVE, LIFT_ONE, cc_largest_k, extract_mesh,  # noqa: F401
                      graph_build, graphcut, grid_resample, lift_accumulate_, lift_debug_merge, make_resample, query_normals,
                      render_normals, upsample_trilinear, visibility_accumulate_, visibility_mask, voxelize_mesh,
                      VQ_MERGE_PER_LANE, VQ_MERGE_RUNS, VQ_MERGE_SHIPPED, vq_accumulate_, vq_assign_, vq_debug_merge)
from .losses import (adam_step_, attn_masked_l1, density_correlation_loss, density_diff_loss, depth_fwd_bwd,  # noqa: F401
                     depth_loss, distortion_fwd_bwd, distortion_loss, exposure_apply, exposure_apply_bwd, exposure_fit_sums, exposure_fwd_bwd,
                     exposure_loss, feature_correlation_loss, fit_affine_colour, orientation_fwd_bwd, orientation_loss,
                     robust_fwd_bwd, robust_loss, robust_mask, robust_parameters, solve_affine_colour, ssim, ssim_fwd_bwd,
                     tv_loss_on_grid)
from .runtime import VoxeError, check, ensure_gfx950, f32c, lib, ptr, require_device, stream_ptr
from .workspace import DROPPED, DeferredGrad, ReconRecord, Workspace, wrote, _pack_key, _scratch_for, _state_key  # noqa: F401


def _render_ws_bytes(L, g, c, R) -> int:
    """workspace of a render call: what the library asks for plus, behind it, room for the per-tile plan of the lean tile kernels
    (voxe.h: voxe_tile_plan_bytes; 0 where none is built)"""
    return L.voxe_workspace_bytes(C.byref(g), C.byref(c), R) + L.voxe_tile_plan_bytes(C.byref(g), C.byref(c), R)


def _route(g, c, R) -> int:
    return int(lib().voxe_render_route(C.byref(g), C.byref(c), int(R)))


def _descs(spec: GridSpec, params: RenderParams, densities, features, seed, rng_offset, reuse):
    X, Y, Z, F = features.shape
    g = make_grid_desc(densities.data_ptr(), features.data_ptr(), (X, Y, Z), F, spec.aabb,
                       spec.density_scale, spec.density_pre_act, spec.density_post_act, spec.feature_kind)
    c = make_render_cfg(params.num_samples, params.near, params.far, params.perturb,
                        params.linear_disparity, params.aabb_clip, params.white_bkgd, params.sh_degree,
                        params.render_diffuse, params.term_eps, seed, rng_offset, reuse, params.image_width,
                        image_height=params.image_height, deterministic=params.deterministic,
                        linear_grad=params.linear_grad,
                        dispatch=(params.dispatch if params.dispatch is not None else _dispatch.current()).struct())
    return g, c


def _validate_inputs(densities, features, rays_o, rays_d, jitter, params: RenderParams):
    for name, t in (("densities", densities), ("features", features)):
        require_device(t, f"voxe render ({name})")
    if densities.dim() != 4 or features.dim() != 4 or densities.shape[:3] != features.shape[:3] or densities.shape[3] != 1:
        raise VoxeError(f"grid tensors must be [X,Y,Z,1] and [X,Y,Z,F]; got {tuple(densities.shape)}, {tuple(features.shape)}")
    _check_rays("voxe render", rays_o, rays_d, jitter, params.num_samples)


def render_fwd_into(spec: GridSpec, params: RenderParams, densities, features, rays_o, rays_d, jitter,
                    colour, depth, acc, disparity, workspace: Workspace, rng=(0, 0), keep_for_backward: bool = True,
                    source=None) -> None:
    """voxe_render_fwd on caller-provided output tensors (contiguous float32 on one device, no autograd).
    keep_for_backward=False (inference): the forward skips what only a backward of the same rays would read (the per-sample
    values of view-dependent grids); a later backward on this workspace re-marches.
    `source` = (densities, features) as the caller holds them, when `densities` / `features` are dense float32 conversions of
    those: the packed-grid cache is keyed on the source, never on a temporary."""
    device = densities.device
    ensure_gfx950(device)
    L = lib()
    R = rays_o.shape[0]
    src_d, src_f = source if source is not None else (densities, features)
    g, c = _descs(spec, params, densities, features, rng[0], rng[1], False)
    with torch.cuda.device(device):
        c.ray_state_valid = 0 if keep_for_backward else -1     # (-1: the size query leaves out everything only a backward reads)
        ws, c.reuse_packed_grid, _, _ = workspace.before_call(spec, src_d, src_f, _render_ws_bytes(L, g, c, R), device)
        check(L.voxe_render_fwd(C.byref(g), C.byref(c), ptr(rays_o), ptr(rays_d), R, ptr(jitter), ptr(colour),
                                ptr(depth), ptr(acc), ptr(disparity), ptr(ws), ws.numel(),
                                stream_ptr(device)), "voxe_render_fwd")
    workspace.after_call(spec, src_d, src_f, (params, rays_o, rays_d, jitter, rng, _route(g, c, R)) if keep_for_backward else DROPPED)


def render_bwd_into(spec: GridSpec, params: RenderParams, densities, features, rays_o, rays_d, jitter,
                    colour, depth, acc, g_colour, g_depth, g_acc, d_densities, d_features,
                    workspace: Workspace, rng=(0, 0), accumulate: bool = False, source=None) -> None:
    """voxe_render_bwd into caller-provided gradient tensors (either may be None to skip it).  `source`: as in render_fwd_into."""
    device = densities.device
    L = lib()
    R = rays_o.shape[0]
    src_d, src_f = source if source is not None else (densities, features)
    g, c = _descs(spec, params, densities, features, rng[0], rng[1], False)
    with torch.cuda.device(device):
        ws, c.reuse_packed_grid, _, key = workspace.before_call(spec, src_d, src_f, _render_ws_bytes(L, g, c, R), device)
        c.ray_state_valid = int(workspace.holds_states(_state_key(key, params, rays_o, rays_d, jitter, rng, _route(g, c, R))))
        check(L.voxe_render_bwd(C.byref(g), C.byref(c), ptr(rays_o), ptr(rays_d), R, ptr(jitter), ptr(colour),
                                ptr(depth), ptr(acc), ptr(g_colour), ptr(g_depth), ptr(g_acc),
                                ptr(d_densities), ptr(d_features), int(accumulate), ptr(ws), ws.numel(),
                                stream_ptr(device)), "voxe_render_bwd")
    workspace.after_call(spec, src_d, src_f)


class _RenderFn(torch.autograd.Function):
    """colour, depth, acc, disparity = render(densities, features | rays)  with the fused HIP kernels."""

    @staticmethod
    def forward(ctx, densities, features, rays_o, rays_d, jitter, spec, params, workspace, rng):
        ctx.set_materialize_grads(False)
        device = densities.device
        ensure_gfx950(device)
        dens, feat = f32c(densities.detach()), f32c(features.detach())
        ro, rd = f32c(rays_o.detach()), f32c(rays_d.detach())
        jit = None if jitter is None else f32c(jitter.detach())
        R = ro.shape[0]
        cout = 1 if spec.feature_kind == abi.FEAT_ATTN else 3
        colour = torch.empty((R, cout), dtype=torch.float32, device=device)
        depth = torch.empty((R, 1), dtype=torch.float32, device=device)
        acc = torch.empty((R, 1), dtype=torch.float32, device=device)
        disp = torch.empty((R, 1), dtype=torch.float32, device=device)
        ctx.main_workspace = workspace
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:  # (grad mode itself is off inside Function.forward)
            version = (densities._version, features._version)
            workspace = workspace.for_differentiable_forward(version)
            workspace.forward_pending(version)
        render_fwd_into(spec, params, dens, feat, ro, rd, jit, colour, depth, acc, disp, workspace, rng,
                        keep_for_backward=bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1]), source=(densities, features))
        ctx.spec, ctx.params, ctx.workspace, ctx.rng = spec, params, workspace, rng
        ctx.save_for_backward(densities, features, ro, rd, jit, colour, depth, acc)
        return colour, depth, acc, disp

    @staticmethod
    def backward(ctx, g_colour, g_depth, g_acc, g_disp):
        densities, features, ro, rd, jit, colour, depth, acc = ctx.saved_tensors
        need_d, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_ro, need_rd = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if not (need_d or need_f or need_ro or need_rd):
            return (None,) * 9
        if need_ro or need_rd:
            # the gradient to the rays is a call of its own on the raw tensors (no workspace, no forward record); the grid's
            # gradient below is computed exactly as without it
            grid_grads = _RenderFn._backward_grid(ctx, g_colour, g_depth, g_acc, g_disp) if (need_d or need_f) else (None, None)
            gd, ga = _upstream_depth_acc(depth, acc, g_depth, g_acc, g_disp)
            d_ro, d_rd = render_bwd_rays(ctx.spec, ctx.params, densities.detach(), features.detach(), ro, rd, jit, ctx.rng,
                                         None if g_colour is None else f32c(g_colour), gd, ga,
                                         want_o=bool(need_ro), want_d=bool(need_rd))
            return grid_grads + (d_ro, d_rd) + (None,) * 5
        return _RenderFn._backward_grid(ctx, g_colour, g_depth, g_acc, g_disp) + (None,) * 7

    @staticmethod
    def _backward_grid(ctx, g_colour, g_depth, g_acc, g_disp):
        """(d_densities, d_features) of a backward whose grid needs a gradient (None, None in the deferred-gradient mode)"""
        densities, features, ro, rd, jit, colour, depth, acc = ctx.saved_tensors
        need_d, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        device = densities.device
        spec, params, workspace = ctx.spec, ctx.params, ctx.workspace
        g_depth, g_acc = _upstream_depth_acc(depth, acc, g_depth, g_acc, g_disp)
        if g_colour is None:
            g_colour = torch.zeros_like(colour)
        g_colour = f32c(g_colour)
        dens, feat = f32c(densities.detach()), f32c(features.detach())
        main = ctx.main_workspace
        deferred = main.deferred
        if deferred is not None and main.buf is not None and dens.data_ptr() == densities.data_ptr() \
                and feat.data_ptr() == features.data_ptr():
            # deferred-gradient mode: the gradient stays in the MAIN workspace's gradient region (kernel layout) for the
            # fused grid step; autograd sees no gradient for the two grid tensors
            if not params.linear_grad:   # every render of the step writes the SAME (linear) gradient layout
                params = dataclasses.replace(params, linear_grad=True)
            layout = render_bwd_acc(spec, params, dens, feat, ro, rd, jit, colour, depth, acc, g_colour, g_depth, g_acc,
                                    workspace, ctx.rng, zero_first=deferred.must_clear(main.buf),
                                    want_densities=bool(need_d and deferred.want_densities),
                                    want_features=bool(need_f and deferred.want_features),
                                    grad_workspace=(main if workspace is not main else None),
                                    expect_layout=deferred.expected_layout(), source=(densities, features))
            if layout is not None:
                deferred.accumulated(main.buf, layout)
                workspace.backward_ran()
                return None, None
            # (the kernel that fits this render writes another gradient layout than what the region holds -- cannot happen
            #  with linear_grad -- : ordinary path; its un-pack leaves a gradient in ITS workspace's region)
            if workspace is main:
                deferred.overwritten()
        d_dens = torch.empty_like(dens) if need_d else None
        d_feat = torch.empty_like(feat) if need_f else None
        render_bwd_into(spec, params, dens, feat, ro, rd, jit, colour, depth, acc, g_colour, g_depth, g_acc,
                        d_dens, d_feat, workspace, ctx.rng, source=(densities, features))
        workspace.backward_ran()
        return d_dens, d_feat


def _upstream_depth_acc(depth, acc, g_depth, g_acc, g_disp):
    """(g_depth, g_acc) as dense float32, the disparity's gradient (1 / max(1e-10, depth / acc), accumulate.py:85-88) chained in"""
    g_depth = None if g_depth is None else f32c(g_depth)
    g_acc = None if g_acc is None else f32c(g_acc)
    return (g_depth, g_acc) if g_disp is None else disparity_bwd(depth, acc, f32c(g_disp), g_depth, g_acc)


def render(spec: GridSpec, params: RenderParams, densities: torch.Tensor, features: torch.Tensor,
           rays_o: torch.Tensor, rays_d: torch.Tensor, jitter: Optional[torch.Tensor] = None,
           workspace: Optional[Workspace] = None, rng: Optional[Tuple[int, int]] = None):
    """Fused volumetric render.  Returns (colour [R,Cout], depth [R,1], acc [R,1], disparity [R,1]);
    differentiable w.r.t. `densities` and `features` when they require grad."""
    _validate_inputs(densities, features, rays_o, rays_d, jitter, params)
    if workspace is None:
        workspace = Workspace()
    rng = resolve_rng(params, jitter, rng)
    if params.dispatch is None:
        # resolve the dispatch HERE, once: the backward runs on autograd's engine thread, where a `dispatch.override()` of the
        # calling context is not visible, and forward and backward of one render must use the same routes
        params = dataclasses.replace(params, dispatch=_dispatch.current())
    return _RenderFn.apply(densities, features, rays_o, rays_d, jitter, spec, params, workspace, rng)


def sample_probe(spec: GridSpec, params: RenderParams, densities, features, rays_o, rays_d, jitter=None,
                 rng=(0, 0), outputs=("idx", "inside", "z", "sigma", "rad")):
    """Per-sample probe (index math test hook): dict of the requested outputs
    idx [R,S,3] int32, inside [R,S] bool, z [R,S], sigma [R,S], rad [R,S,Cout]."""
    _validate_inputs(densities, features, rays_o, rays_d, jitter, params)
    device = densities.device
    ensure_gfx950(device)
    L = lib()
    dens, feat, ro, rd = f32c(densities.detach()), f32c(features.detach()), f32c(rays_o), f32c(rays_d)
    jit = None if jitter is None else f32c(jitter)
    R, S = ro.shape[0], params.num_samples
    cout = 1 if spec.feature_kind == abi.FEAT_ATTN else 3
    g, c = _descs(spec, params, dens, feat, rng[0], rng[1], False)
    shapes = {"idx": ((R, S, 3), torch.int32), "inside": ((R, S), torch.uint8), "z": ((R, S), torch.float32),
              "sigma": ((R, S), torch.float32), "rad": ((R, S, cout), torch.float32)}
    with torch.cuda.device(device):
        ws = torch.empty(L.voxe_workspace_bytes(C.byref(g), C.byref(c), R), dtype=torch.uint8, device=device)
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=device) for k in outputs}
        check(L.voxe_sample_probe(C.byref(g), C.byref(c), ptr(ro), ptr(rd), R, ptr(jit), ptr(out.get("idx")),
                                  ptr(out.get("inside")), ptr(out.get("z")), ptr(out.get("sigma")),
                                  ptr(out.get("rad")), ptr(ws), ws.numel(), stream_ptr(device)),
              "voxe_sample_probe")
    if "inside" in out:
        out["inside"] = out["inside"].bool()
    return out


class _QueryFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, densities, features, points, spec, workspace):
        device = densities.device
        ensure_gfx950(device)
        L = lib()
        dens, feat, pts = f32c(densities.detach()), f32c(features.detach()), f32c(points.detach())
        N, F = pts.shape[0], feat.shape[-1]
        g, _ = _descs(spec, RenderParams(1, 0.0, 1.0), dens, feat, 0, 0, False)
        with torch.cuda.device(device):
            # (keyed on the caller's tensors: `dens` / `feat` may be temporaries of the conversion above)
            ws, reuse, _, _ = workspace.before_call(spec, densities, features, L.voxe_workspace_bytes(C.byref(g), None, 0), device)
            out = torch.empty((N, F + 1), dtype=torch.float32, device=device)
            check(L.voxe_query_fwd(C.byref(g), ptr(pts), N, ptr(out), reuse, ptr(ws), ws.numel(), stream_ptr(device)),
                  "voxe_query_fwd")
        workspace.after_call(spec, densities, features)
        ctx.spec, ctx.workspace = spec, workspace
        ctx.save_for_backward(densities, features, pts)
        return out

    @staticmethod
    def backward(ctx, g_out):
        densities, features, pts = ctx.saved_tensors
        need_d, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_d or need_f):
            return None, None, None, None, None
        device = densities.device
        L = lib()
        dens, feat = f32c(densities.detach()), f32c(features.detach())
        g, _ = _descs(ctx.spec, RenderParams(1, 0.0, 1.0), dens, feat, 0, 0, False)
        with torch.cuda.device(device):
            ws, reuse, _, _ = ctx.workspace.before_call(ctx.spec, densities, features, L.voxe_workspace_bytes(C.byref(g), None, 0), device)
            d_dens = torch.empty_like(dens) if need_d else None
            d_feat = torch.empty_like(feat) if need_f else None
            check(L.voxe_query_bwd(C.byref(g), ptr(pts), pts.shape[0], ptr(f32c(g_out)), ptr(d_dens), ptr(d_feat), 0, reuse, ptr(ws),
                                   ws.numel(), stream_ptr(device)), "voxe_query_bwd")
        ctx.workspace.after_call(ctx.spec, densities, features, DROPPED)   # (the gradient region of the workspace was reused)
        return d_dens, d_feat, None, None, None


def query_points(spec: GridSpec, densities: torch.Tensor, features: torch.Tensor, points: torch.Tensor,
                 workspace: Optional[Workspace] = None) -> torch.Tensor:
    """Un-masked trilinear point query [N,3] -> [N,F+1] = (features, post(pre(density*scale)));
    VoxelGrid.forward semantics (thre3d_atom/thre3d_reprs/voxels.py:287-342), differentiable w.r.t. the grid."""
    for name, t in (("densities", densities), ("features", features), ("points", points)):
        require_device(t, f"query_points ({name})")
    if points.dim() != 2 or points.shape[1] != 3:
        raise VoxeError(f"points must be [N,3]; got {tuple(points.shape)}")
    return _QueryFn.apply(densities, features, points, spec, workspace or Workspace())


def render_bwd_acc(spec: GridSpec, params: RenderParams, densities, features, rays_o, rays_d, jitter,
                   colour, depth, acc, g_colour, g_depth, g_acc, workspace: Workspace, rng=(0, 0),
                   zero_first: bool = True, want_densities: bool = True, want_features: bool = True,
                   grad_workspace: Optional[Workspace] = None, expect_layout: int = abi.GRAD_ANY, source=None) -> Optional[int]:
    """voxe_render_bwd_acc(_into): the backward of one render, its gradient LEFT in the workspace (kernel layout) for
    `grid_adam_step_` -- in `grad_workspace`'s gradient region when given (a second render of the same step that ran in
    its own workspace).  Returns the layout (abi.GRAD_*); renders accumulated into one step must agree on it:
    with `expect_layout` set, a render whose kernel writes the other layout is NOT run and None is returned.
    `source`: as in render_fwd_into."""
    device = densities.device
    L = lib()
    R = rays_o.shape[0]
    src_d, src_f = source if source is not None else (densities, features)
    g, c = _descs(spec, params, densities, features, rng[0], rng[1], False)
    layout = C.c_int32(abi.GRAD_ANY)
    if expect_layout != abi.GRAD_ANY and R > 0 and expect_layout != predicted_grad_layout(spec, params, densities, features, R):
        return None
    with torch.cuda.device(device):
        ws, c.reuse_packed_grid, _, key = workspace.before_call(spec, src_d, src_f, _render_ws_bytes(L, g, c, R), device)
        c.ray_state_valid = int(workspace.holds_states(_state_key(key, params, rays_o, rays_d, jitter, rng, _route(g, c, R))))
        gws = None if grad_workspace is None else grad_workspace.buf
        check(L.voxe_render_bwd_acc_into(C.byref(g), C.byref(c), ptr(rays_o), ptr(rays_d), R, ptr(jitter), ptr(colour),
                                         ptr(depth), ptr(acc), ptr(g_colour), ptr(g_depth), ptr(g_acc),
                                         int(want_densities), int(want_features), int(zero_first), C.byref(layout),
                                         ptr(ws), ws.numel(), ptr(gws), 0 if gws is None else gws.numel(),
                                         stream_ptr(device)), "voxe_render_bwd_acc_into")
    workspace.after_call(spec, src_d, src_f)
    return int(layout.value)


def predicted_grad_layout(spec: GridSpec, params: RenderParams, densities, features, R: int) -> int:
    """which gradient layout the backward of this render writes (voxe_render_bwd_layout)"""
    g, c = _descs(spec, params, densities, features, 0, 0, False)
    return int(lib().voxe_render_bwd_layout(C.byref(g), C.byref(c), int(R)))


def workspace_grad_view(spec: GridSpec, densities, features, workspace: Workspace) -> torch.Tensor:
    """float32 view of the workspace's gradient region (what a data-parallel job all-reduces between
    `render_bwd_acc` and `grid_adam_step_`)."""
    g, _ = _descs(spec, RenderParams(num_samples=1, near=0.0, far=1.0), densities, features, 0, 0, False)
    L = lib()
    off, nbytes = L.voxe_workspace_grad_offset(C.byref(g)), L.voxe_workspace_grad_bytes(C.byref(g))
    if workspace.buf is None or workspace.buf.numel() < off + nbytes:
        raise VoxeError("workspace_grad_view: the workspace holds no gradient region yet")
    return workspace.buf[off:off + nbytes].view(torch.float32)


def workspace_packed_view(spec: GridSpec, densities, features, workspace: Workspace) -> torch.Tensor:
    """float32 view [X*Y*Z*(F+1)] of the workspace's packed grid (what the next render samples): a sharded optimiser
    all-gathers the x-slabs of THIS instead of the raw parameters."""
    n = densities.numel() + features.numel()
    if workspace.buf is None or workspace.buf.numel() < 4 * n:
        raise VoxeError("workspace_packed_view: the workspace holds no packed grid yet")
    return workspace.buf[: 4 * n].view(torch.float32)


@torch.no_grad()
def grid_adam_step_(spec: GridSpec, densities, features, grad_layout: int, workspace: Workspace, step: int, lr: float,
                    state_densities=None, state_features=None, extra_d_densities=None, extra_d_features=None,
                    beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                    x_range: Optional[Tuple[int, int]] = None, step_features: Optional[int] = None,
                    dcl_reference: Optional[torch.Tensor] = None, dcl_weight: float = 0.0,
                    dcl_loss: Optional[torch.Tensor] = None, density_kind: int = 0,
                    feat_reference: Optional[torch.Tensor] = None, feat_weight: float = 0.0,
                    feat_loss: Optional[torch.Tensor] = None) -> None:
    """voxe_grid_adam_step: consume the workspace gradient (+ optional extra gradients in tensor layout), update
    densities / features in place with torch.optim.Adam arithmetic, leave the NEW grid packed and a zeroed gradient
    region in the workspace.  state_* = (exp_avg, exp_avg_sq) or None to freeze that tensor.  x_range = (x_begin, x_end)
    restricts the step to a slab of x-planes (sharded optimiser: the caller exchanges the other slabs of the packed grid
    before the next render).  `step` / `step_features`: the 1-based Adam step of the densities / of the features
    (torch.optim.Adam counts per parameter; `step_features` None = the same as `step`).
    `dcl_reference` (densities of the pretrained field, same shape as `densities`): the density-correlation regulariser of the
    SDS edit (modules/sds_trainer.py:507-524) with weight `dcl_weight` is evaluated INSIDE the step -- its moments by two small
    launches on the current parameters, its gradient per voxel in the Adam pass -- and `dcl_loss` (float32 scalar tensor on the
    device) receives the unweighted loss value.  `density_kind` (abi.DREG_*): the same three arguments as the l2_mode / l1_mode
    regulariser (sds_trainer.py:494-503: per-voxel terms, no reduction unless `dcl_loss` is given).  `feat_reference` /
    `feat_weight` / `feat_loss`: _feature_correlation_loss (sds_trainer.py:526-534) against the pretrained field's features,
    evaluated per voxel inside the step (SH-0 / attention grids)."""
    device = densities.device
    ensure_gfx950(device)
    (m_d, v_d), (m_f, v_f) = _moments(state_densities), _moments(state_features)
    for nm, t, ref in (("densities", densities, densities), ("features", features, features), ("state_densities", m_d, densities),
                       ("state_densities", v_d, densities), ("state_features", m_f, features), ("state_features", v_f, features),
                       ("extra_d_densities", extra_d_densities, densities), ("extra_d_features", extra_d_features, features),
                       ("dcl_reference", dcl_reference, densities), ("feat_reference", feat_reference, features)):
        if t is not None:
            _require_buffer("grid_adam_step_", nm, t, numel=ref.numel())
    if workspace.buf is None:
        raise VoxeError("grid_adam_step_: the workspace holds no gradient (call render_bwd_acc first)")
    g, _ = _descs(spec, RenderParams(num_samples=1, near=0.0, far=1.0), densities, features, 0, 0, False)
    with torch.cuda.device(device):
        ws = workspace.buf
        x0, x1 = (0, int(densities.shape[0])) if x_range is None else (int(x_range[0]), int(x_range[1]))
        reg = None
        if dcl_reference is not None or feat_reference is not None:
            for nm, t in (("dcl_loss", dcl_loss), ("feat_loss", feat_loss)):
                if t is not None:
                    _require_buffer("grid_adam_step_", nm, t, numel=1)
            sc = _scratch_for(device, lib().voxe_dcl_scratch_bytes(densities.numel()))
            reg = abi.VoxeGridRegularisers()
            if dcl_reference is not None:
                reg.dcl_reference, reg.dcl_weight, reg.dcl_loss = ptr(dcl_reference), float(dcl_weight), ptr(dcl_loss)
                reg.density_kind = int(density_kind)
            if feat_reference is not None:
                reg.feat_reference, reg.feat_weight, reg.feat_loss = ptr(feat_reference), float(feat_weight), ptr(feat_loss)
            reg.scratch, reg.scratch_bytes = ptr(sc), sc.numel()
        check(lib().voxe_grid_adam_step(C.byref(g), int(grad_layout), x0, x1, ptr(extra_d_densities), ptr(extra_d_features),
                                        ptr(m_d), ptr(v_d), ptr(m_f), ptr(v_f), float(lr), float(beta1), float(beta2),
                                        float(eps), int(step), int(step if step_features is None else step_features),
                                        None if reg is None else C.byref(reg), ptr(ws), ws.numel(), stream_ptr(device)),
              "voxe_grid_adam_step")
    # (a frozen tensor -- no Adam state -- was not written: its version stays, so other workspaces that hold it packed, e.g. the
    #  two attention grids of the refinement stage over ONE density tensor, keep their packed copies)
    wrote(densities if m_d is not None else None, features if m_f is not None else None, m_d, v_d, m_f, v_f)
    workspace.after_call(spec, densities, features, DROPPED)          # the workspace holds the updated grid packed


@torch.no_grad()
def attn_refine_step_(spec: GridSpec, params: RenderParams, densities, attn, rays_o, rays_d, attn_map, workspace: Workspace,
                      step: int, lr: float, state, tv_weight: float, losses: Optional[torch.Tensor] = None, rng=(0, 0),
                      beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, attn_render: Optional[torch.Tensor] = None,
                      zero_gradient_first: bool = False, tv_loss_always: bool = True) -> None:
    """voxe_attn_refine_step: one attention grid's share of a refinement iteration (modules/attn_grid_trainer.py:335-378) in ONE
    library call -- attention render -> masked L1 against `attn_map` + `tv_weight` x TV -> backward -> Adam step of `attn` in place
    (`state` = (exp_avg, exp_avg_sq); the densities are frozen).  `losses` [2] (device) receives masked L1 and TV (unweighted),
    `attn_render` [R] the rendered attention image."""
    device = densities.device
    if spec.feature_kind != abi.FEAT_ATTN:
        raise VoxeError("attn_refine_step_ needs an attention grid spec (feature_kind = FEAT_ATTN)")
    R = int(rays_o.shape[0])
    for nm, t, n in (("densities", densities, densities.numel()), ("attn", attn, densities.numel()),
                     ("exp_avg", state[0], densities.numel()), ("exp_avg_sq", state[1], densities.numel()),
                     ("rays_o", rays_o, 3 * R), ("rays_d", rays_d, 3 * R), ("attn_map", attn_map, R)):
        _require_buffer("attn_refine_step_", nm, t, numel=n)
    for nm, t, n in (("losses", losses, 2), ("attn_render", attn_render, R)):
        if t is not None:
            _require_buffer("attn_refine_step_", nm, t, numel=n)
    ensure_gfx950(device)      # (behind the tensor checks: CPU tensors are refused with a VoxeError, GPU or not)
    L = lib()
    if losses is None and tv_weight != 0.0:
        # the TV pass writes its loss value wherever it runs, and it runs for the gradient whenever tv_weight != 0: the library
        # is never handed NULL there (a null store on the device otherwise); the values go to a scratch pair nobody reads
        losses = workspace.recon.scratch("refine_losses", 2, torch.float32, device)
        # (`tv_loss_always` asks for the TV VALUE when tv_weight == 0; nobody reads the value here, and tv_weight != 0 runs the
        #  pass anyway: off, so that the flag never becomes the reason for a launch)
        tv_loss_always = False
    g, c = _descs(spec, params, densities, attn, rng[0], rng[1], False)
    rs = abi.VoxeAttnRefineStep()
    rs.attn_map, rs.tv_weight, rs.tv_loss_always = ptr(attn_map), float(tv_weight), int(bool(tv_loss_always))
    rs.lr, rs.beta1, rs.beta2, rs.eps, rs.step = float(lr), float(beta1), float(beta2), float(eps), int(step)
    rs.exp_avg, rs.exp_avg_sq = ptr(state[0]), ptr(state[1])
    rs.losses, rs.attn_render = ptr(losses), ptr(attn_render)
    with torch.cuda.device(device):
        ws, c.reuse_packed_grid, fresh, _ = workspace.before_call(spec, densities, attn, _render_ws_bytes(L, g, c, R), device)
        # (a buffer this call allocated holds whatever torch.empty returned in its gradient region)
        rs.zero_gradient_first = int(bool(zero_gradient_first) or fresh)
        sc = workspace.recon.scratch("refine", L.voxe_attn_refine_scratch_bytes(C.byref(g), R), torch.uint8, device)
        check(L.voxe_attn_refine_step(C.byref(g), C.byref(c), C.byref(rs), ptr(rays_o), ptr(rays_d), R, ptr(ws), ws.numel(),
                                      ptr(sc), sc.numel(), stream_ptr(device)), "voxe_attn_refine_step")
    wrote(attn, state[0], state[1])
    workspace.after_call(spec, densities, attn, DROPPED)              # the workspace holds the updated grid packed


@torch.no_grad()
def _recon_call(entry: str, spec: GridSpec, params: RenderParams, densities, features, workspace: Workspace, workspace2: Workspace,
                height: int, width: int, focal: float, poses: torch.Tensor, image_rows: Optional[torch.Tensor],
                images: torch.Tensor, batch: int, diffuse_regularisation: bool, state_densities, state_features,
                step_densities: int, step_features: int, lr: float, losses: torch.Tensor, rng: Tuple[int, int],
                beta1: float, beta2: float, eps: float, zero_gradient_first: bool):
    """argument marshalling shared by voxe_recon_step and voxe_recon_prefetch (the hint must announce EXACTLY what the step
    will pass: same descriptors, same buffers, same sizes)"""
    device = densities.device
    ensure_gfx950(device)
    for nm, t in (("densities", densities), ("features", features), ("poses", poses), ("images", images), ("losses", losses)):
        _require_buffer(entry, nm, t)
    if images.dim() != 4 or images.shape[1] != 3 or tuple(images.shape[2:]) != (height, width):
        raise VoxeError(f"{entry}: images must be [N,3,{height},{width}], got {tuple(images.shape)}")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or losses.numel() < 4:
        raise VoxeError(f"{entry}: poses must be [K,3,4] and losses hold 4 floats")
    if image_rows is not None and (image_rows.dtype != torch.int64 or image_rows.numel() != poses.shape[0] or not image_rows.is_cuda):
        raise VoxeError(f"{entry}: image_rows must be int64 [K] on the device")
    L = lib()
    p = dataclasses.replace(params, linear_grad=True, image_width=0, image_height=0)
    g, c = _descs(spec, p, densities, features, rng[0], rng[1], False)
    rs = abi.VoxeReconStep()
    rs.H, rs.W, rs.focal = int(height), int(width), float(focal)
    rs.poses, rs.images, rs.image_rows = ptr(poses), ptr(images), ptr(image_rows)
    rs.num_images = int(images.shape[0])
    rs.K, rs.batch, rs.diffuse_regularisation = int(poses.shape[0]), int(batch), int(bool(diffuse_regularisation))
    moments = _recon_optimiser(rs, densities, features, state_densities, state_features, step_densities, step_features, lr, beta1,
                               beta2, eps)
    rs.losses = ptr(losses)
    with torch.cuda.device(device):
        nbytes = L.voxe_workspace_bytes(C.byref(g), C.byref(c), int(batch))
        if diffuse_regularisation and p.sh_degree == 0:
            # SH-0: the library runs both renders as ONE launch of 2 * batch rays when the first workspace holds that launch
            nbytes = max(nbytes, L.voxe_workspace_bytes(C.byref(g), C.byref(c), 2 * int(batch)))
        ws, c.reuse_packed_grid, fresh, _ = workspace.before_call(spec, densities, features, nbytes, device)
        # (a buffer this call allocated holds whatever torch.empty returned in its gradient region)
        rs.zero_gradient_first = int(bool(zero_gradient_first) or fresh)
        ws2 = None
        if diffuse_regularisation:
            # the second workspace runs the DIFFUSE render: for view-dependent grids that render may take another route (and
            # need other scratch) than the specular one -- size it with the diffuse cfg, and never below the first workspace
            # (SH-0: it holds the second set of segment tables, the one voxe_recon_prefetch fills ahead)
            _, c2 = _descs(spec, dataclasses.replace(p, render_diffuse=True), densities, features, rng[0], rng[1], False)
            ws2 = workspace2.ensure(max(nbytes, L.voxe_workspace_bytes(C.byref(g), C.byref(c2), int(batch))), device)
        sc = workspace.recon.scratch("step", L.voxe_recon_scratch_bytes(int(batch)), torch.uint8, device, hinted=workspace)
    return L, g, c, rs, ws, ws2, sc, moments


def _recon_optimiser(rs, densities, features, state_densities, state_features, step_densities, step_features, lr, beta1, beta2, eps):
    """fill in the optimiser's share of a VoxeReconStep; -> (exp_avg, exp_avg_sq) of the densities and of the features.  The grid
    step writes every moment tensor through its raw pointer, one value per parameter: checked on every call, cached path or not"""
    (m_d, v_d), (m_f, v_f) = _moments(state_densities), _moments(state_features)
    for nm, t, p in (("state_densities", m_d, densities), ("state_densities", v_d, densities), ("state_features", m_f, features),
                     ("state_features", v_f, features)):
        if t is not None:
            _require_buffer("recon_step_", nm, t, numel=p.numel(), device=p.device)
    rs.lr, rs.beta1, rs.beta2, rs.eps = float(lr), float(beta1), float(beta2), float(eps)
    rs.step_densities, rs.step_features = int(step_densities), int(step_features)
    rs.exp_avg_densities, rs.exp_avg_sq_densities = ptr(m_d), ptr(v_d)
    rs.exp_avg_features, rs.exp_avg_sq_features = ptr(m_f), ptr(v_f)
    return m_d, v_d, m_f, v_f


def _recon_key(spec, params, densities, features, height, width, focal, images, batch, diffuse_regularisation, losses):
    """what has to be unchanged for the descriptors of the last recon_step_ to describe this call too (everything but the cameras,
    the streams, the optimiser's state / hyper-parameters and the flags)"""
    return (spec, params, params.dispatch if params.dispatch is not None else _dispatch.current(), densities.data_ptr(),
            tuple(densities.shape), densities.dtype, densities.is_contiguous(), features.data_ptr(), tuple(features.shape), features.dtype,
            features.is_contiguous(), int(height), int(width), float(focal), images.data_ptr(), tuple(images.shape), images.dtype,
            images.is_contiguous(), int(batch), bool(diffuse_regularisation), losses.data_ptr(), losses.dtype, losses.numel())


def recon_step_(spec: GridSpec, params: RenderParams, densities, features, workspace: Workspace, workspace2: Workspace,
                height: int, width: int, focal: float, poses: torch.Tensor, image_rows: Optional[torch.Tensor],
                images: torch.Tensor, batch: int, diffuse_regularisation: bool, state_densities, state_features,
                step_densities: int, step_features: int, lr: float, losses: torch.Tensor, rng: Tuple[int, int],
                beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, zero_gradient_first: bool = True) -> None:
    """voxe_recon_step: one reconstruction iteration (random pixel batch over the K cameras `poses` -> specular
    [+ diffuse] render -> L1 loss(es) against `images` -> backward -> Adam on both grid tensors) in ONE library call.
    `losses` [4] float32 on the device receives (L1 specular, MSE specular, L1 diffuse, MSE diffuse).  The jitter /
    subset streams derive from `rng` (subset: offset, specular: offset + 1, diffuse: offset + 2).  Afterwards
    `workspace` holds the updated grid packed and a cleared gradient region."""
    device = densities.device
    key = _recon_key(spec, params, densities, features, height, width, focal, images, batch, diffuse_regularisation, losses)
    cached = workspace.recon.descriptors(key, workspace.buf, workspace2.buf, poses, image_rows, rng)
    if cached is not None:
        # the same loop as the last call: only the optimiser's state and the flags are filled in -- the trainer's loop is paced by
        # this function's host time
        L = lib()
        g, c, rs, ws, ws2, sc = cached
        c.reuse_packed_grid = int(workspace.holds(spec, densities, features))
        moments = _recon_optimiser(rs, densities, features, state_densities, state_features, step_densities, step_features, lr,
                                   beta1, beta2, eps)
        rs.zero_gradient_first = int(bool(zero_gradient_first))
    else:
        L, g, c, rs, ws, ws2, sc, moments = _recon_call(
            "recon_step_", spec, params, densities, features, workspace, workspace2, height, width, focal, poses, image_rows, images,
            batch, diffuse_regularisation, state_densities, state_features, step_densities, step_features, lr, losses, rng, beta1,
            beta2, eps, zero_gradient_first)
    with torch.cuda.device(device):
        check(L.voxe_recon_step(C.byref(g), C.byref(c), C.byref(rs), ptr(ws), ws.numel(), ptr(ws2),
                                0 if ws2 is None else ws2.numel(), ptr(sc), sc.numel(), stream_ptr(device)), "voxe_recon_step")
    # what a hint for the NEXT iteration has to repeat (recon_prefetch_ copies these descriptors instead of building them again:
    # the hint's host time is on the iteration's critical path once the device work is hidden)
    workspace.recon.step_enqueued(workspace, workspace2, ReconRecord(key, g, c, rs, ws, ws2, sc))
    wrote(densities, features, *moments)
    workspace.after_call(spec, densities, features, DROPPED)          # the workspace holds the updated grid packed
    workspace2.forget_grid()                               # (its packed grid is the previous iteration's)


def recon_prefetch_(spec: GridSpec, params: RenderParams, densities, features, workspace: Workspace, workspace2: Workspace,
                    height: int, width: int, focal: float, poses: torch.Tensor, image_rows: Optional[torch.Tensor],
                    images: torch.Tensor, batch: int, diffuse_regularisation: bool, losses: torch.Tensor, rng: Tuple[int, int]) -> None:
    """voxe_recon_prefetch: announce the NEXT recon_step_ (same arguments; `poses`, `image_rows` and `rng` are the next
    iteration's; everything else must equal the last recon_step_ of this workspace, otherwise nothing is announced).  The library
    assembles that iteration's batch and segment tables on a stream of its own while the current iteration's backward and grid
    step run; the next recon_step_ takes them iff its arguments are the announced ones.  A hint: results never depend on it, and
    no buffer is ever allocated, grown or moved by it.  Call it right after recon_step_ (both workspaces and the scratch exist by then and keep
    their addresses); `poses` / `image_rows` are kept alive until the next recon_step_ of this workspace, and the caller must not
    modify them in between: the step recognises its hint by their addresses, not by their values."""
    device = densities.device
    if workspace.buf is None:
        return                                             # (no step has sized the buffers yet: nothing to announce against)
    key = _recon_key(spec, params, densities, features, height, width, focal, images, batch, diffuse_regularisation, losses)
    cached = workspace.recon.descriptors(key, workspace.buf, workspace2.buf, poses, image_rows, rng)
    if cached is None:
        # Anything else (another batch size, grid, image stack, ... than the last step's) is not announced: marshalling it afresh
        # could regrow a workspace, and a hint must never move a buffer -- the caller's knowledge of what its workspace holds
        # (packed grid, cleared gradient region: `zero_gradient_first`) would silently go stale.  The next step bins inline.
        return
    L = lib()
    g, c, rs, ws, ws2, sc = cached
    with torch.cuda.device(device):
        check(L.voxe_recon_prefetch(C.byref(g), C.byref(c), C.byref(rs), ptr(ws), ws.numel(), ptr(ws2),
                                    0 if ws2 is None else ws2.numel(), ptr(sc), sc.numel(), stream_ptr(device)), "voxe_recon_prefetch")
    workspace.recon.hint_issued(workspace, workspace2, (poses, image_rows, images))


@torch.no_grad()
def disparity_bwd(depth: torch.Tensor, acc: torch.Tensor, g_disp: torch.Tensor, g_depth: Optional[torch.Tensor] = None,
                  g_acc: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """voxe_disparity_bwd: (g_depth + d disparity/d depth * g_disp, g_acc + d disparity/d acc * g_disp), all [R, 1]"""
    require_device(depth, "disparity_bwd")
    out_d, out_a = torch.empty_like(depth), torch.empty_like(acc)
    with torch.cuda.device(depth.device):
        check(lib().voxe_disparity_bwd(ptr(depth), ptr(acc), ptr(g_disp), ptr(g_depth), ptr(g_acc), ptr(out_d), ptr(out_a),
                                       depth.numel(), stream_ptr(depth.device)), "voxe_disparity_bwd")
    return out_d, out_a


def clock_probe(device, spin: int = 0) -> float:
    """sustained shader clock in Hz (voxe_clock_probe: enqueued on the current stream, then waited for)"""
    hz = C.c_double(0.0)
    with torch.cuda.device(device):
        check(lib().voxe_clock_probe(int(spin), C.byref(hz), stream_ptr(device)), "voxe_clock_probe")
    return float(hz.value)


def region_debug_tables(spec: GridSpec, params: RenderParams, densities, features, R: int, workspace: Workspace) -> dict:
    """views of the space-binned route's segment tables in `workspace` (as the last forward of these R rays left them):
    test aid, see voxe_region_debug_layout"""
    g, c = _descs(spec, params, densities, features, 0, 0, False)
    out = (C.c_int64 * 17)()
    check(lib().voxe_region_debug_layout(C.byref(g), C.byref(c), int(R), out), "voxe_region_debug_layout")
    base, (o_region, o_pos, o_seg, o_sorted, o_lane_n, o_count, o_start, nslots, nlanes, nreg, per_lane, bx, by, bz, ncls,
           chunk) = int(out[0]), [int(v) for v in out[1:]]
    buf = workspace.buf

    def view(off, n, dtype, width=1):
        nbytes = n * width * torch.empty((), dtype=dtype).element_size()
        return buf[base + off: base + off + nbytes].view(dtype).view(n, width) if width > 1 else \
            buf[base + off: base + off + nbytes].view(dtype)

    ncnt = (nreg + 1) * ncls + 1
    return {"slot_region": view(o_region, nslots, torch.int32), "slot_pos": view(o_pos, nslots, torch.int32),
            "slot_seg": view(o_seg, nslots, torch.int32, 2), "sorted": view(o_sorted, nslots, torch.int32, 4),
            "lane_n": view(o_lane_n, nlanes, torch.int32), "count": view(o_count, ncnt, torch.int32),
            "start": view(o_start, ncnt, torch.int32), "nreg": nreg, "slots_per_lane": per_lane,
            "region_cells": (bx, by, bz), "len_classes": ncls, "chunk": chunk}


def profile_enable(on: bool = True) -> None:
    check(lib().voxe_profile_enable(int(on)), "voxe_profile_enable")


def profile_read() -> dict:
    p = abi.VoxeProfile()
    check(lib().voxe_profile_read(C.byref(p)), "voxe_profile_read")
    return {name: getattr(p, name) for name, _ in abi.VoxeProfile._fields_}


# ------------------------------------------------------------------------------------------------
# ray and camera-pose gradients (DESIGN.md section 4 "Ray gradients"): the render's gradient w.r.t. its rays reads the raw grid
# tensors only (no workspace); the ray casting's backward carries it on to the poses and the focal length
# ------------------------------------------------------------------------------------------------
def render_bwd_rays(spec: GridSpec, params: RenderParams, densities: torch.Tensor, features: torch.Tensor, rays_o: torch.Tensor,
                    rays_d: torch.Tensor, jitter: Optional[torch.Tensor], rng: Tuple[int, int], g_colour: Optional[torch.Tensor],
                    g_depth: Optional[torch.Tensor], g_acc: Optional[torch.Tensor], lanes: int = 0, want_o: bool = True,
                    want_d: bool = True, d_rays_o: Optional[torch.Tensor] = None, d_rays_d: Optional[torch.Tensor] = None,
                    accumulate: bool = False):
    """voxe_render_bwd_rays: (d_rays_o [R,3], d_rays_d [R,3]) of the render of these rays for the upstream gradients g_colour
    [R,3], g_depth [R] / [R,1], g_acc [R] / [R,1] (each may be None = 0).  want_o / want_d = False skips that output (None);
    d_rays_o / d_rays_d: caller's buffers (contiguous float32 [R,3]), added to when `accumulate`.  `lanes` (test aid): 1 / 2 /
    4 / 8 pins the kernel's lanes per ray for this call, 0 = chosen by R."""
    _validate_inputs(densities, features, rays_o, rays_d, jitter, params)
    device = densities.device
    ensure_gfx950(device)
    dens, feat = f32c(densities.detach()), f32c(features.detach())
    ro, rd = f32c(rays_o.detach()), f32c(rays_d.detach())
    jit = None if jitter is None else f32c(jitter.detach())
    R = ro.shape[0]
    ups = []
    for name, t, n in (("g_colour", g_colour, 3 * R), ("g_depth", g_depth, R), ("g_acc", g_acc, R)):
        if t is not None:
            require_device(t, f"render_bwd_rays ({name})")
            if t.numel() != n:
                raise VoxeError(f"render_bwd_rays: {name} must hold {n} values; got {tuple(t.shape)}")
            t = f32c(t.detach())
        ups.append(t)
    for name, t in (("d_rays_o", d_rays_o), ("d_rays_d", d_rays_d)):
        if t is not None:
            _require_buffer("render_bwd_rays", name, t, shape=(R, 3), device=device)
    g, c = _descs(spec, params, dens, feat, rng[0], rng[1], False)
    L = lib()
    with torch.cuda.device(device):
        d_o = d_rays_o if d_rays_o is not None else (torch.empty((R, 3), dtype=torch.float32, device=device) if want_o else None)
        d_d = d_rays_d if d_rays_d is not None else (torch.empty((R, 3), dtype=torch.float32, device=device) if want_d else None)
        if lanes:
            check(L.voxe_render_bwd_rays_debug_lanes(int(lanes)), "voxe_render_bwd_rays_debug_lanes")
        try:
            check(L.voxe_render_bwd_rays(C.byref(g), C.byref(c), ptr(ro), ptr(rd), R, ptr(jit), ptr(ups[0]), ptr(ups[1]),
                                         ptr(ups[2]), ptr(d_o), ptr(d_d), 1 if accumulate else 0, stream_ptr(device)),
                  "voxe_render_bwd_rays")
        finally:
            if lanes:
                L.voxe_render_bwd_rays_debug_lanes(0)
    wrote(d_rays_o, d_rays_d)
    return d_o, d_d


# ------------------------------------------------------------------------------------------------
# per-voxel Fisher information: reads the raw grid tensors only, no workspace, not differentiable
# ------------------------------------------------------------------------------------------------
def fisher_rays_(spec: GridSpec, params: RenderParams, densities: torch.Tensor, features: torch.Tensor, rays_o: torch.Tensor,
                 rays_d: torch.Tensor, fisher: Optional[torch.Tensor] = None, voxel_var: Optional[torch.Tensor] = None,
                 want_ray_var: bool = False, jitter: Optional[torch.Tensor] = None, rng: Tuple[int, int] = (0, 0)):
    """voxe_fisher_rays: add, in place, to `fisher` ([X,Y,Z] or [X,Y,Z,1] float32, contiguous; zero it before the first call)
    the diagonal Fisher information sum_rays sum_ch (d colour_{r,ch} / d raw density)^2 of the flat rays, with the samples,
    weights and SH colours `render` uses for the same params, jitter and rng.  want_ray_var: also return ray_var [R] =
    sum_c voxel_var[c] sum_ch J_{r,ch}[c]^2 (voxel_var [X,Y,Z] or [X,Y,Z,1]; None = 1), bit-reproducible; otherwise None.
    With neither output nothing is launched."""
    _validate_inputs(densities, features, rays_o, rays_d, jitter, params)
    device = densities.device
    ensure_gfx950(device)
    for name, t in (("fisher", fisher), ("voxel_var", voxel_var)):
        if t is not None:
            _require_buffer("fisher_rays_", name, t, shape=densities.shape if t.dim() == 4 else densities.shape[:3],
                            numel=densities.numel(), device=device)
    dens, feat = f32c(densities.detach()), f32c(features.detach())
    ro, rd = f32c(rays_o.detach()), f32c(rays_d.detach())
    jit = None if jitter is None else f32c(jitter.detach())
    R = ro.shape[0]
    g, c = _descs(spec, params, dens, feat, rng[0], rng[1], False)
    with torch.cuda.device(device):
        ray_var = torch.empty((R,), dtype=torch.float32, device=device) if want_ray_var else None
        check(lib().voxe_fisher_rays(C.byref(g), C.byref(c), ptr(ro), ptr(rd), R, ptr(jit), ptr(fisher),
                                     ptr(voxel_var) if want_ray_var else None, ptr(ray_var), stream_ptr(device)),
              "voxe_fisher_rays")
    wrote(fisher)
    return ray_var
