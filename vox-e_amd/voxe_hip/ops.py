"""torch-level operators over libvoxe_hip.so: the fused render (autograd.Function), ray casting and
the whole-grid passes.  Tensors are plumbing (device memory + streams); all compute is in the HIP
library.  Nothing here falls back to torch ops or to the CPU oracle."""
import ctypes as C
import dataclasses
import weakref
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import abi
from . import dispatch as _dispatch
from .desc import make_grid_desc, make_render_cfg
from .runtime import VoxeError, check, ensure_gfx950, f32c, lib, ptr, require_device, stream_ptr


@dataclass(frozen=True)
class GridSpec:
    """Static (non-tensor) description of a voxel grid: what VoxeGridDesc needs besides pointers."""
    aabb: Tuple[Tuple[float, float], Tuple[float, float], Tuple[float, float]]
    density_scale: float = 1.0
    density_pre_act: int = abi.ACT_IDENTITY
    density_post_act: int = abi.ACT_SOFTPLUS
    feature_kind: int = abi.FEAT_SH


@dataclass
class RenderParams:
    """Everything VoxeRenderCfg holds except the RNG stream and the packed-grid reuse flag."""
    num_samples: int
    near: float
    far: float
    perturb: bool = False
    linear_disparity: bool = False
    aabb_clip: bool = False
    white_bkgd: bool = False
    sh_degree: int = 0
    render_diffuse: bool = False
    term_eps: float = 0.0
    image_width: int = 0
    image_height: int = 0     # > 0 (with image_width): the rays are K = R / (H * W) images, one after the other
    deterministic: bool = False   # backward in 64-bit fixed point: bit-reproducible (test / race-check mode)
    linear_grad: bool = False     # render_bwd_acc: write VOXE_GRAD_LINEAR whatever kernel runs (deferred-gradient mode)
    dispatch: Optional[_dispatch.Dispatch] = None   # kernel routes / tuning of THIS call (VoxeDispatch); None = dispatch.current()


@dataclass
class DeferredGrad:
    """state of the deferred-gradient mode of one grid: which layout the accumulated gradient has and whether the region
    holds anything since the last optimiser step"""
    layout: int = abi.GRAD_ANY
    dirty: bool = False
    want_densities: bool = True
    want_features: bool = True
    clean_ptr: int = 0        # data_ptr of the workspace buffer whose gradient region is known to be cleared / in use


class Workspace:
    """Caller-owned scratch of the render entry points: [packed grid | packed gradient].
    Remembers which grid values it holds packed so consecutive calls can skip the pack pass."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.key = None        # which grid values are packed in the buffer (_pack_key of the SOURCE tensors)
        self.state_key = None  # which forward call's per-ray depth-segment states it holds
        # weak references to the storages behind the two keys.  An address and a version counter name a tensor's values only
        # while its storage lives: a freed block goes back to the caching allocator, and the next tensor of that size gets the
        # same data_ptr with a fresh counter at the same value.  A dead reference therefore ends the key it belongs to.
        self._sources = ()
        self._state_sources = ()
        # A differentiable forward leaves its per-ray states here for its backward.  When a second differentiable
        # forward arrives before that backward (two renders in one loss: specular + diffuse), it runs in `sibling`
        # (own buffers) instead of overwriting the states -- otherwise the first backward must re-march its rays.
        self.pending = False
        self.pending_version = None   # (densities._version, features._version) of the forward that set `pending`
        self.sibling: Optional["Workspace"] = None
        # deferred-gradient mode (FusedGridAdam): backward passes of renders through this workspace (or its sibling)
        # LEAVE the grid gradient in this workspace's gradient region instead of returning .grad tensors
        self.deferred: Optional["DeferredGrad"] = None
        self.recon_scratch: dict = {}   # device scratch of recon_step_ (rays, targets, outputs of one fused iteration)
        # recon_prefetch_: the library's side stream may be writing into this buffer (and reading `prefetch_keepalive`) until the
        # next recon_step_ of the owning workspace has been enqueued
        self.prefetch_inflight = False
        self.prefetch_keepalive = None
        self.recon_cache = None         # descriptors of the last recon_step_ (what a hint for the next one repeats)

    def __del__(self):
        # a hint in flight (recon_prefetch_) writes this buffer from a stream torch's caching allocator knows nothing about
        try:
            if self.prefetch_inflight and self.buf is not None:
                torch.cuda.synchronize(self.buf.device)
        except Exception:
            pass

    def for_differentiable_forward(self, version=None) -> "Workspace":
        """the workspace a differentiable forward should run in.  A pending forward whose backward never came (the caller
        dropped the graph: the parameters have moved on since) no longer blocks this workspace."""
        if self.pending and version is not None and self.pending_version != version:
            self.pending = False
        if not self.pending:
            return self
        if self.sibling is None:
            self.sibling = Workspace()
        if self.sibling.pending and version is not None and self.sibling.pending_version != version:
            self.sibling.pending = False
        return self.sibling if not self.sibling.pending else self

    def ensure(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            old = self.buf
            if old is not None and self.prefetch_inflight:
                torch.cuda.synchronize(old.device)   # (a stream torch's allocator knows nothing about is still using the old buffer)
                self.prefetch_inflight = False
            self.recon_cache = None                  # (its descriptors point into the old buffer -- and would keep it alive)
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
            keep = (old is not None and self.deferred is not None and self.deferred.dirty
                    and old.device == self.buf.device)
            if keep:
                # deferred-gradient mode: an accumulated gradient (and the packed grid in front of it) lives at fixed
                # offsets from the start of the buffer -- a render that needs a bigger workspace must not lose it
                self.buf[: old.numel()].copy_(old)
                self.deferred.clean_ptr = self.buf.data_ptr()
            else:
                self.key = None
            self.state_key = None
        return self.buf

    def invalidate(self):
        """forget what the buffer holds: the next call packs the grid and marches its rays again.  For writes that neither
        torch's version counters nor this module can see (`tensor.data`, another library's kernel, a DLPack view)."""
        self.key = None
        self.state_key = None
        if self.sibling is not None:
            self.sibling.invalidate()

    def holds(self, spec: "GridSpec", densities: torch.Tensor, features: torch.Tensor) -> bool:
        """THE decision "skip the pack pass": does the buffer hold the values of these grid tensors, packed for `spec`?
        `densities` / `features` are the caller's tensors, BEFORE any conversion to dense float32 (the converted copy is a
        temporary whose address and version say nothing about the source)."""
        if self.key is None:
            return False
        if not _alive(self._sources):
            self.key = self.state_key = None
            return False
        return self.key == _pack_key(spec, densities, features)

    def remember(self, spec: "GridSpec", densities: torch.Tensor, features: torch.Tensor) -> None:
        """the buffer now holds these (source) tensors' values packed for `spec`"""
        self.key = _pack_key(spec, densities, features)
        self._sources = (_storage_ref(densities), _storage_ref(features))

    def holds_states(self, state_key) -> bool:
        """THE decision "ray_state_valid = 1": does the buffer hold the per-ray states of exactly the forward `state_key`
        (_state_key) describes, marched through the packed grid it still holds?"""
        if self.state_key is None:
            return False
        if not (_alive(self._sources) and _alive(self._state_sources)):
            self.state_key = None
            return False
        return self.state_key == state_key

    def remember_states(self, state_key, rays_o, rays_d, jitter) -> None:
        self.state_key = state_key
        self._state_sources = tuple(_storage_ref(t) for t in (rays_o, rays_d, jitter) if t is not None)


def _render_ws_bytes(L, g, c, R) -> int:
    """workspace of a render call: what the library asks for plus, behind it, room for the per-tile plan of the lean tile kernels
    (voxe.h: voxe_tile_plan_bytes; 0 where none is built)"""
    return L.voxe_workspace_bytes(C.byref(g), C.byref(c), R) + L.voxe_tile_plan_bytes(C.byref(g), C.byref(c), R)


def _storage_ref(t: torch.Tensor):
    return weakref.ref(t.untyped_storage())


def _alive(refs) -> bool:
    for r in refs:
        if r() is None:
            return False
    return True


def _pack_key(spec: GridSpec, densities: torch.Tensor, features: torch.Tensor):
    """which values a packed grid holds -- of the caller's tensors as they are (any dtype, any strides).  Complete only together
    with Workspace._sources: equal addresses and versions mean equal values while the storages behind them are alive.
    (density_post_act is applied per sample, not by the pack: not part of the key.)"""
    return (densities.data_ptr(), densities._version, features.data_ptr(), features._version,
            tuple(features.shape), spec.density_scale, spec.density_pre_act, spec.feature_kind,
            densities.dtype, densities.stride(), features.dtype, features.stride())


def _state_key(pack_key, params: RenderParams, rays_o, rays_d, jitter, rng, route=None):
    """identity of a forward call: the backward may consume the ray states only of exactly this call -- and only when it
    resolves to the same kernels (`route` = voxe_render_route: ray-ordered and space-binned renders keep different
    tables, and the choice also depends on process-level tuning switches that may change between the two calls)"""
    fwd = tuple((k, v) for k, v in vars(params).items() if k not in ("linear_grad", "deterministic", "dispatch"))   # backward-only knobs
    fwd += (("dispatch", params.dispatch if params.dispatch is not None else _dispatch.current()),)
    # (the rays' and the jitter's version counters too: the trainers reuse their ray buffers, rewriting them in place)
    return (pack_key, fwd, rays_o.data_ptr(), rays_o._version, rays_d.data_ptr(), rays_d._version, rays_o.shape[0],
            None if jitter is None else (jitter.data_ptr(), jitter._version), tuple(rng), route)


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
    for name, t in (("densities", densities), ("features", features), ("rays_o", rays_o), ("rays_d", rays_d)):
        require_device(t, f"voxe render ({name})")
    if densities.dim() != 4 or features.dim() != 4 or densities.shape[:3] != features.shape[:3] or densities.shape[3] != 1:
        raise VoxeError(f"grid tensors must be [X,Y,Z,1] and [X,Y,Z,F]; got {tuple(densities.shape)}, {tuple(features.shape)}")
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_o.shape != rays_d.shape:
        raise VoxeError(f"rays must be flat [R,3]; got {tuple(rays_o.shape)}, {tuple(rays_d.shape)}")
    if jitter is not None and tuple(jitter.shape) != (rays_o.shape[0], params.num_samples):
        raise VoxeError(f"jitter must be [R,S]={rays_o.shape[0], params.num_samples}; got {tuple(jitter.shape)}")


def _next_rng():
    """(seed, offset) of the in-kernel counter-hash jitter stream, tied to torch's CPU generator so that
    torch.manual_seed() makes renders reproducible (no device sync involved)."""
    seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
    offset = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    return seed, offset


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
        ws = workspace.ensure(_render_ws_bytes(L, g, c, R), device)
        c.reuse_packed_grid = int(workspace.holds(spec, src_d, src_f))
        check(L.voxe_render_fwd(C.byref(g), C.byref(c), ptr(rays_o), ptr(rays_d), R, ptr(jitter), ptr(colour),
                                ptr(depth), ptr(acc), ptr(disparity), ptr(ws), ws.numel(),
                                stream_ptr(device)), "voxe_render_fwd")
    workspace.remember(spec, src_d, src_f)
    if keep_for_backward:
        workspace.remember_states(_state_key(workspace.key, params, rays_o, rays_d, jitter, rng, _route(g, c, R)), rays_o, rays_d, jitter)
    else:
        workspace.state_key = None


def render_bwd_into(spec: GridSpec, params: RenderParams, densities, features, rays_o, rays_d, jitter,
                    colour, depth, acc, g_colour, g_depth, g_acc, d_densities, d_features,
                    workspace: Workspace, rng=(0, 0), accumulate: bool = False, source=None) -> None:
    """voxe_render_bwd into caller-provided gradient tensors (either may be None to skip it).  `source`: as in render_fwd_into."""
    device = densities.device
    L = lib()
    R = rays_o.shape[0]
    src_d, src_f = source if source is not None else (densities, features)
    key = _pack_key(spec, src_d, src_f)
    g, c = _descs(spec, params, densities, features, rng[0], rng[1], False)
    with torch.cuda.device(device):
        ws = workspace.ensure(_render_ws_bytes(L, g, c, R), device)
        c.reuse_packed_grid = int(workspace.holds(spec, src_d, src_f))
        c.ray_state_valid = int(workspace.holds_states(_state_key(key, params, rays_o, rays_d, jitter, rng, _route(g, c, R))))
        check(L.voxe_render_bwd(C.byref(g), C.byref(c), ptr(rays_o), ptr(rays_d), R, ptr(jitter), ptr(colour),
                                ptr(depth), ptr(acc), ptr(g_colour), ptr(g_depth), ptr(g_acc),
                                ptr(d_densities), ptr(d_features), int(accumulate), ptr(ws), ws.numel(),
                                stream_ptr(device)), "voxe_render_bwd")
    workspace.remember(spec, src_d, src_f)


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
            workspace.pending, workspace.pending_version = True, version
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
            gd = None if g_depth is None else f32c(g_depth)
            ga = None if g_acc is None else f32c(g_acc)
            if g_disp is not None:
                gd, ga = disparity_bwd(depth, acc, f32c(g_disp), gd, ga)
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
        g_depth = None if g_depth is None else f32c(g_depth)
        g_acc = None if g_acc is None else f32c(g_acc)
        if g_disp is not None:
            # disparity = 1 / max(1e-10, depth / acc)  (accumulate.py:85-88): chained into d_depth and d_acc by one kernel
            g_depth, g_acc = disparity_bwd(depth, acc, f32c(g_disp), g_depth, g_acc)
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
            # (the region of a buffer this mode has not written yet holds whatever torch.empty returned)
            fresh = (not deferred.dirty) and deferred.clean_ptr != main.buf.data_ptr()
            if not params.linear_grad:   # every render of the step writes the SAME (linear) gradient layout
                params = dataclasses.replace(params, linear_grad=True)
            layout = render_bwd_acc(spec, params, dens, feat, ro, rd, jit, colour, depth, acc, g_colour, g_depth, g_acc,
                                    workspace, ctx.rng, zero_first=fresh,
                                    want_densities=bool(need_d and deferred.want_densities),
                                    want_features=bool(need_f and deferred.want_features),
                                    grad_workspace=(main if workspace is not main else None),
                                    expect_layout=deferred.layout if deferred.dirty else abi.GRAD_ANY, source=(densities, features))
            if layout is not None:
                deferred.clean_ptr = main.buf.data_ptr()
                if layout != abi.GRAD_ANY:
                    deferred.layout = layout
                    deferred.dirty = True
                workspace.pending = False
                return None, None
            # (the kernel that fits this render writes another gradient layout than what the region holds -- cannot happen
            #  with linear_grad -- : ordinary path; its un-pack leaves a gradient in ITS workspace's region)
            if workspace is main:
                if deferred.dirty:
                    raise VoxeError("deferred-gradient mode: a render with another gradient layout would overwrite the "
                                    "accumulated gradient")
                deferred.clean_ptr = 0
        d_dens = torch.empty_like(dens) if need_d else None
        d_feat = torch.empty_like(feat) if need_f else None
        render_bwd_into(spec, params, dens, feat, ro, rd, jit, colour, depth, acc, g_colour, g_depth, g_acc,
                        d_dens, d_feat, workspace, ctx.rng, source=(densities, features))
        workspace.pending = False
        return d_dens, d_feat


def render(spec: GridSpec, params: RenderParams, densities: torch.Tensor, features: torch.Tensor,
           rays_o: torch.Tensor, rays_d: torch.Tensor, jitter: Optional[torch.Tensor] = None,
           workspace: Optional[Workspace] = None, rng: Optional[Tuple[int, int]] = None):
    """Fused volumetric render.  Returns (colour [R,Cout], depth [R,1], acc [R,1], disparity [R,1]);
    differentiable w.r.t. `densities` and `features` when they require grad."""
    _validate_inputs(densities, features, rays_o, rays_d, jitter, params)
    if workspace is None:
        workspace = Workspace()
    if rng is None:
        rng = _next_rng() if (params.perturb and jitter is None) else (0, 0)
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
            ws = workspace.ensure(L.voxe_workspace_bytes(C.byref(g), None, 0), device)
            out = torch.empty((N, F + 1), dtype=torch.float32, device=device)
            # (keyed on the caller's tensors: `dens` / `feat` may be temporaries of the conversion above)
            check(L.voxe_query_fwd(C.byref(g), ptr(pts), N, ptr(out), int(workspace.holds(spec, densities, features)), ptr(ws),
                                   ws.numel(), stream_ptr(device)), "voxe_query_fwd")
        workspace.remember(spec, densities, features)
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
            ws = ctx.workspace.ensure(L.voxe_workspace_bytes(C.byref(g), None, 0), device)
            d_dens = torch.empty_like(dens) if need_d else None
            d_feat = torch.empty_like(feat) if need_f else None
            check(L.voxe_query_bwd(C.byref(g), ptr(pts), pts.shape[0], ptr(f32c(g_out)), ptr(d_dens), ptr(d_feat), 0,
                                   int(ctx.workspace.holds(ctx.spec, densities, features)), ptr(ws), ws.numel(),
                                   stream_ptr(device)), "voxe_query_bwd")
        ctx.workspace.remember(ctx.spec, densities, features)
        ctx.workspace.state_key = None  # the gradient region of the workspace was reused
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


def cast_rays(height: int, width: int, focal: float, rotation, translation, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """rays_o, rays_d [H*W,3] on `device` (thre3d_atom/rendering/volumetric/utils/misc.py:12-50)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise VoxeError("cast_rays runs on the GPU only (no CPU fallback in the product path)")
    ensure_gfx950(device)
    rot = torch.as_tensor(rotation).detach().to("cpu", torch.float32).reshape(9).contiguous()
    tr = torch.as_tensor(translation).detach().to("cpu", torch.float32).reshape(3).contiguous()
    fp = C.POINTER(C.c_float)
    n = int(height) * int(width)
    with torch.cuda.device(device):
        ro = torch.empty((n, 3), dtype=torch.float32, device=device)
        rd = torch.empty((n, 3), dtype=torch.float32, device=device)
        check(lib().voxe_cast_rays(int(height), int(width), float(focal), C.cast(rot.data_ptr(), fp),
                                   C.cast(tr.data_ptr(), fp), ptr(ro), ptr(rd), stream_ptr(device)),
              "voxe_cast_rays")
    return ro, rd


def cast_rays_indexed(height: int, width: int, focal: float, poses: torch.Tensor,
                      flat_index: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rays of selected pixels of K cameras: poses [K,3,4] and flat_index int64 [B] = (camera*H + y)*W + x, both on
    the GPU; -> rays_o, rays_d [B,3].  No host synchronisation, no full-image ray buffers."""
    require_device(poses, "cast_rays_indexed")
    require_device(flat_index, "cast_rays_indexed")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or flat_index.dtype != torch.int64 or flat_index.dim() != 1:
        raise VoxeError("cast_rays_indexed: poses must be [K,3,4] float, flat_index int64 [B]")
    device = poses.device
    ensure_gfx950(device)
    p = f32c(poses)
    idx = flat_index.contiguous()
    n = int(idx.shape[0])
    with torch.cuda.device(device):
        ro = torch.empty((n, 3), dtype=torch.float32, device=device)
        rd = torch.empty((n, 3), dtype=torch.float32, device=device)
        check(lib().voxe_cast_rays_indexed(int(height), int(width), float(focal), ptr(p), int(p.shape[0]), ptr(idx), n,
                                           ptr(ro), ptr(rd), stream_ptr(device)), "voxe_cast_rays_indexed")
    return ro, rd


def random_subset(n: int, count: int, device, rng: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """`count` distinct pseudo-random indices of [0, n) (int64, random order) -- the role of torch.randperm(n)[:count]
    without permuting all n.  Reproducible: (seed, counter) come from torch's CPU generator state like the jitter."""
    device = torch.device(device)
    if device.type != "cuda":
        raise VoxeError("random_subset runs on the GPU only (no CPU fallback in the product path)")
    ensure_gfx950(device)
    seed, offset = rng if rng is not None else _next_rng()
    with torch.cuda.device(device):
        out = torch.empty((int(count),), dtype=torch.int64, device=device)
        check(lib().voxe_random_subset(int(n), int(count), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), ptr(out),
                                       stream_ptr(device)), "voxe_random_subset")
    return out


# ------------------------------------------------------------------------------------------------
# whole-grid passes
# ------------------------------------------------------------------------------------------------
_scratch = {}


def _scratch_for(device, nbytes: int) -> torch.Tensor:
    key = (torch.device(device).index, torch.cuda.current_stream(device).cuda_stream)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
        _scratch[key] = buf
    return buf


class _DclFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sds_density, regular_density):
        require_device(sds_density, "density_correlation_loss")
        a, b = f32c(sds_density.detach()), f32c(regular_density.detach())
        if a.numel() != b.numel():
            raise VoxeError("density_correlation_loss: shape mismatch")
        device = a.device
        ensure_gfx950(device)
        L = lib()
        with torch.cuda.device(device):
            sc = _scratch_for(device, L.voxe_dcl_scratch_bytes(a.numel()))
            loss = torch.empty((), dtype=torch.float32, device=device)
            d_a = torch.empty_like(a) if ctx.needs_input_grad[0] else None
            # gradient for upstream 1.0 is produced in the same launch sequence and scaled in backward
            check(L.voxe_dcl_fwd_bwd(ptr(a), ptr(b), a.numel(), 1.0, ptr(loss), ptr(d_a), 0, ptr(sc),
                                     sc.numel(), stream_ptr(device)), "voxe_dcl_fwd_bwd")
        ctx.save_for_backward(d_a)
        ctx.shape = sds_density.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_a,) = ctx.saved_tensors
        if d_a is None:
            return None, None
        return (d_a * g).reshape(ctx.shape), None


def density_correlation_loss(sds_density: torch.Tensor, regular_density: torch.Tensor) -> torch.Tensor:
    """1 - corr(sds, regular)  (thre3d_atom/modules/sds_trainer.py:507-524); differentiable w.r.t. sds."""
    return _DclFn.apply(sds_density, regular_density)


class _DiffFn(torch.autograd.Function):
    """density_correlation_loss_fn's l2_mode / l1_mode (sds_trainer.py:494-503): value + gradient in one launch sequence"""

    @staticmethod
    def forward(ctx, sds_density, regular_density, kind):
        require_device(sds_density, "density_diff_loss")
        a, b = f32c(sds_density.detach()), f32c(regular_density.detach())
        if a.numel() != b.numel():
            raise VoxeError("density_diff_loss: shape mismatch")
        device = a.device
        ensure_gfx950(device)
        L = lib()
        with torch.cuda.device(device):
            sc = _scratch_for(device, L.voxe_dcl_scratch_bytes(a.numel()))
            loss = torch.empty((), dtype=torch.float32, device=device)
            d_a = torch.empty_like(a) if ctx.needs_input_grad[0] else None
            check(L.voxe_density_diff_fwd_bwd(ptr(a), ptr(b), a.numel(), int(kind), 1.0, ptr(loss), ptr(d_a), 0, ptr(sc),
                                              sc.numel(), stream_ptr(device)), "voxe_density_diff_fwd_bwd")
        ctx.save_for_backward(d_a)
        ctx.shape = sds_density.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_a,) = ctx.saved_tensors
        if d_a is None:
            return None, None, None
        return (d_a * g).reshape(ctx.shape), None, None


def density_diff_loss(sds_density: torch.Tensor, regular_density: torch.Tensor, l2_mode: bool) -> torch.Tensor:
    """mse_loss (l2_mode) / l1_loss of the two density grids (thre3d_atom/modules/sds_trainer.py:494-503); differentiable w.r.t. sds."""
    return _DiffFn.apply(sds_density, regular_density, abi.DREG_L2 if l2_mode else abi.DREG_L1)


class _FeatCorrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sds_features, regular_features):
        require_device(sds_features, "feature_correlation_loss")
        f, r = f32c(sds_features.detach()), f32c(regular_features.detach())
        if f.shape != r.shape or f.dim() < 1:
            raise VoxeError("feature_correlation_loss: shape mismatch")
        device = f.device
        ensure_gfx950(device)
        L = lib()
        F = int(f.shape[-1])
        nvox = f.numel() // F
        with torch.cuda.device(device):
            sc = _scratch_for(device, L.voxe_dcl_scratch_bytes(nvox))
            loss = torch.empty((), dtype=torch.float32, device=device)
            d_f = torch.empty_like(f) if ctx.needs_input_grad[0] else None
            check(L.voxe_feature_correlation_fwd_bwd(ptr(f), ptr(r), nvox, F, 1.0, ptr(loss), ptr(d_f), 0, ptr(sc), sc.numel(),
                                                     stream_ptr(device)), "voxe_feature_correlation_fwd_bwd")
        ctx.save_for_backward(d_f)
        ctx.shape = sds_features.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_f,) = ctx.saved_tensors
        if d_f is None:
            return None, None
        return (d_f * g).reshape(ctx.shape), None


def feature_correlation_loss(sds_features: torch.Tensor, regular_features: torch.Tensor) -> torch.Tensor:
    """sum_v (sum_c sigmoid(f_vc) - sigmoid(r_vc))^2 (thre3d_atom/modules/sds_trainer.py:526-534); differentiable w.r.t. sds."""
    return _FeatCorrFn.apply(sds_features, regular_features)


class _TvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid):
        require_device(grid, "tv_loss_on_grid")
        gr = f32c(grid.detach())
        if gr.dim() != 4:
            raise VoxeError("tv_loss_on_grid expects [X,Y,Z,C]")
        device = gr.device
        ensure_gfx950(device)
        L = lib()
        X, Y, Z, Cn = gr.shape
        with torch.cuda.device(device):
            sc = _scratch_for(device, L.voxe_tv_scratch_bytes(X, Y, Z, Cn))
            loss = torch.empty((), dtype=torch.float32, device=device)
            d_g = torch.empty_like(gr) if ctx.needs_input_grad[0] else None
            check(L.voxe_tv_fwd_bwd(ptr(gr), X, Y, Z, Cn, 1.0, ptr(loss), ptr(d_g), 0, ptr(sc), sc.numel(),
                                    stream_ptr(device)), "voxe_tv_fwd_bwd")
        ctx.save_for_backward(d_g)
        return loss

    @staticmethod
    def backward(ctx, g):
        (d_g,) = ctx.saved_tensors
        return None if d_g is None else d_g * g


def tv_loss_on_grid(grid: torch.Tensor) -> torch.Tensor:
    """(mean|dx| + mean|dy| + mean|dz|)/3  (thre3d_atom/modules/sds_trainer.py:563-567)."""
    return _TvFn.apply(grid)


@torch.no_grad()
def adam_step_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
               step: int, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8) -> None:
    """In-place torch.optim.Adam update of one tensor (weight_decay=0, amsgrad=False)."""
    for name, t in (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        require_device(t, f"adam_step_ ({name})")
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != param.numel():
            raise VoxeError(f"adam_step_: {name} must be contiguous float32 of the parameter's size")
    device = param.device
    ensure_gfx950(device)
    with torch.cuda.device(device):
        check(lib().voxe_adam_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(),
                                   float(lr), float(beta1), float(beta2), float(eps), int(step),
                                   stream_ptr(device)), "voxe_adam_step")
    # the library wrote through raw pointers: tell autograd (and the packed-grid cache keyed on
    # Tensor._version) that these tensors changed in place
    for t in (param, exp_avg, exp_avg_sq):
        torch.autograd.graph.increment_version(t)


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
    key = _pack_key(spec, src_d, src_f)
    g, c = _descs(spec, params, densities, features, rng[0], rng[1], False)
    layout = C.c_int32(abi.GRAD_ANY)
    if expect_layout != abi.GRAD_ANY and R > 0 and expect_layout != predicted_grad_layout(spec, params, densities, features, R):
        return None
    with torch.cuda.device(device):
        ws = workspace.ensure(_render_ws_bytes(L, g, c, R), device)
        c.reuse_packed_grid = int(workspace.holds(spec, src_d, src_f))
        c.ray_state_valid = int(workspace.holds_states(_state_key(key, params, rays_o, rays_d, jitter, rng, _route(g, c, R))))
        gws = None if grad_workspace is None else grad_workspace.buf
        check(L.voxe_render_bwd_acc_into(C.byref(g), C.byref(c), ptr(rays_o), ptr(rays_d), R, ptr(jitter), ptr(colour),
                                         ptr(depth), ptr(acc), ptr(g_colour), ptr(g_depth), ptr(g_acc),
                                         int(want_densities), int(want_features), int(zero_first), C.byref(layout),
                                         ptr(ws), ws.numel(), ptr(gws), 0 if gws is None else gws.numel(),
                                         stream_ptr(device)), "voxe_render_bwd_acc_into")
    workspace.remember(spec, src_d, src_f)
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
    tensors = [("densities", densities, densities), ("features", features, features)]
    for nm, st, ref in (("state_densities", state_densities, densities), ("state_features", state_features, features)):
        if st is not None:
            tensors += [(nm, st[0], ref), (nm, st[1], ref)]
    for nm, t, ref in (("extra_d_densities", extra_d_densities, densities), ("extra_d_features", extra_d_features, features),
                       ("dcl_reference", dcl_reference, densities), ("feat_reference", feat_reference, features)):
        if t is not None:
            tensors.append((nm, t, ref))
    for nm, t, ref in tensors:
        require_device(t, f"grid_adam_step_ ({nm})")
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != ref.numel():
            raise VoxeError(f"grid_adam_step_: {nm} must be contiguous float32 of its parameter's size")
    if workspace.buf is None:
        raise VoxeError("grid_adam_step_: the workspace holds no gradient (call render_bwd_acc first)")
    g, _ = _descs(spec, RenderParams(num_samples=1, near=0.0, far=1.0), densities, features, 0, 0, False)
    m_d, v_d = state_densities if state_densities is not None else (None, None)
    m_f, v_f = state_features if state_features is not None else (None, None)
    with torch.cuda.device(device):
        ws = workspace.buf
        x0, x1 = (0, int(densities.shape[0])) if x_range is None else (int(x_range[0]), int(x_range[1]))
        reg = None
        if dcl_reference is not None or feat_reference is not None:
            for nm, t in (("dcl_loss", dcl_loss), ("feat_loss", feat_loss)):
                if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.numel() != 1):
                    raise VoxeError(f"grid_adam_step_: {nm} must be a float32 scalar tensor on the device")
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
    for t in (densities if m_d is not None else None, features if m_f is not None else None, m_d, v_d, m_f, v_f):
        if t is not None:
            torch.autograd.graph.increment_version(t)
    workspace.remember(spec, densities, features)          # the workspace holds the updated grid packed
    workspace.state_key = None


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
        require_device(t, f"attn_refine_step_ ({nm})")
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise VoxeError(f"attn_refine_step_: {nm} must be contiguous float32 with {n} elements")
    for nm, t, n in (("losses", losses, 2), ("attn_render", attn_render, R)):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n):
            raise VoxeError(f"attn_refine_step_: {nm} must be contiguous float32 with {n} elements on the device")
    ensure_gfx950(device)      # (behind the tensor checks: CPU tensors are refused with a VoxeError, GPU or not)
    L = lib()
    if losses is None and tv_weight != 0.0:
        # the TV pass writes its loss value wherever it runs, and it runs for the gradient whenever tv_weight != 0: the library
        # is never handed NULL there (a null store on the device otherwise); the values go to a scratch pair nobody reads
        losses = workspace.recon_scratch.get("refine_losses")
        if losses is None or losses.device != device:
            losses = workspace.recon_scratch["refine_losses"] = torch.empty(2, dtype=torch.float32, device=device)
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
        had = workspace.buf
        ws = workspace.ensure(_render_ws_bytes(L, g, c, R), device)
        # (a buffer this call allocated holds whatever torch.empty returned in its gradient region)
        rs.zero_gradient_first = int(bool(zero_gradient_first) or ws is not had)
        c.reuse_packed_grid = int(workspace.holds(spec, densities, attn))
        need = L.voxe_attn_refine_scratch_bytes(C.byref(g), R)
        sc = workspace.recon_scratch.get("refine")
        if sc is None or sc.numel() < need or sc.device != ws.device:
            sc = workspace.recon_scratch["refine"] = torch.empty(need, dtype=torch.uint8, device=device)
        check(L.voxe_attn_refine_step(C.byref(g), C.byref(c), C.byref(rs), ptr(rays_o), ptr(rays_d), R, ptr(ws), ws.numel(),
                                      ptr(sc), sc.numel(), stream_ptr(device)), "voxe_attn_refine_step")
    for t in (attn, state[0], state[1]):
        torch.autograd.graph.increment_version(t)
    workspace.remember(spec, densities, attn)              # the workspace holds the updated grid packed
    workspace.state_key = None


@torch.no_grad()
def _recon_call(entry: str, spec: GridSpec, params: RenderParams, densities, features, workspace: Workspace, workspace2: Workspace,
                height: int, width: int, focal: float, poses: torch.Tensor, image_rows: Optional[torch.Tensor],
                images: torch.Tensor, batch: int, diffuse_regularisation: bool, state_densities, state_features,
                step_densities: int, step_features: int, lr: float, losses: torch.Tensor, rng: Tuple[int, int],
                beta1: float, beta2: float, eps: float, zero_gradient_first: bool, scratch_holder: Optional[dict]):
    """argument marshalling shared by voxe_recon_step and voxe_recon_prefetch (the hint must announce EXACTLY what the step
    will pass: same descriptors, same buffers, same sizes)"""
    device = densities.device
    ensure_gfx950(device)
    for nm, t in (("densities", densities), ("features", features), ("poses", poses), ("images", images), ("losses", losses)):
        require_device(t, f"{entry} ({nm})")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise VoxeError(f"{entry}: {nm} must be contiguous float32")
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
    rs.lr, rs.beta1, rs.beta2, rs.eps = float(lr), float(beta1), float(beta2), float(eps)
    rs.step_densities, rs.step_features = int(step_densities), int(step_features)
    m_d, v_d = state_densities if state_densities is not None else (None, None)
    m_f, v_f = state_features if state_features is not None else (None, None)
    rs.exp_avg_densities, rs.exp_avg_sq_densities = ptr(m_d), ptr(v_d)
    rs.exp_avg_features, rs.exp_avg_sq_features = ptr(m_f), ptr(v_f)
    rs.losses = ptr(losses)
    holder = scratch_holder if scratch_holder is not None else workspace.recon_scratch
    with torch.cuda.device(device):
        nbytes = L.voxe_workspace_bytes(C.byref(g), C.byref(c), int(batch))
        if diffuse_regularisation and p.sh_degree == 0:
            # SH-0: the library runs both renders as ONE launch of 2 * batch rays when the first workspace holds that launch
            nbytes = max(nbytes, L.voxe_workspace_bytes(C.byref(g), C.byref(c), 2 * int(batch)))
        had = workspace.buf
        ws = workspace.ensure(nbytes, device)
        # (a buffer this call allocated holds whatever torch.empty returned in its gradient region)
        rs.zero_gradient_first = int(bool(zero_gradient_first) or ws is not had)
        c.reuse_packed_grid = int(workspace.holds(spec, densities, features))
        ws2 = None
        if diffuse_regularisation:
            # the second workspace runs the DIFFUSE render: for view-dependent grids that render may take another route (and
            # need other scratch) than the specular one -- size it with the diffuse cfg, and never below the first workspace
            # (SH-0: it holds the second set of segment tables, the one voxe_recon_prefetch fills ahead)
            _, c2 = _descs(spec, dataclasses.replace(p, render_diffuse=True), densities, features, rng[0], rng[1], False)
            ws2 = workspace2.ensure(max(nbytes, L.voxe_workspace_bytes(C.byref(g), C.byref(c2), int(batch))), device)
        need = L.voxe_recon_scratch_bytes(int(batch))
        sc = holder.get("buf")
        if sc is None or sc.numel() < need or sc.device != ws.device:
            if sc is not None and workspace.prefetch_inflight:
                torch.cuda.synchronize(device)     # (the library's side stream may still be writing the old buffer)
                workspace.prefetch_inflight = False
            sc = holder["buf"] = torch.empty(need, dtype=torch.uint8, device=device)
    return L, g, c, rs, ws, ws2, sc, (m_d, v_d, m_f, v_f)


def _recon_key(spec, params, densities, features, height, width, focal, images, batch, diffuse_regularisation, losses):
    """what has to be unchanged for the descriptors of the last recon_step_ to describe this call too (everything but the cameras,
    the streams, the optimiser's state / hyper-parameters and the flags)"""
    return (spec, params, params.dispatch if params.dispatch is not None else _dispatch.current(), densities.data_ptr(),
            tuple(densities.shape), densities.dtype, densities.is_contiguous(), features.data_ptr(), tuple(features.shape), features.dtype,
            features.is_contiguous(), int(height), int(width), float(focal), images.data_ptr(), tuple(images.shape), images.dtype,
            images.is_contiguous(), int(batch), bool(diffuse_regularisation), losses.data_ptr(), losses.dtype, losses.numel())


def _recon_cameras_ok(poses, image_rows, K) -> bool:
    return (poses.is_cuda and poses.dtype == torch.float32 and poses.is_contiguous() and tuple(poses.shape) == (K, 3, 4)
            and (image_rows is None or (image_rows.is_cuda and image_rows.dtype == torch.int64 and image_rows.numel() == K)))


def recon_step_(spec: GridSpec, params: RenderParams, densities, features, workspace: Workspace, workspace2: Workspace,
                height: int, width: int, focal: float, poses: torch.Tensor, image_rows: Optional[torch.Tensor],
                images: torch.Tensor, batch: int, diffuse_regularisation: bool, state_densities, state_features,
                step_densities: int, step_features: int, lr: float, losses: torch.Tensor, rng: Tuple[int, int],
                beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, zero_gradient_first: bool = True,
                scratch_holder: Optional[dict] = None) -> None:
    """voxe_recon_step: one reconstruction iteration (random pixel batch over the K cameras `poses` -> specular
    [+ diffuse] render -> L1 loss(es) against `images` -> backward -> Adam on both grid tensors) in ONE library call.
    `losses` [4] float32 on the device receives (L1 specular, MSE specular, L1 diffuse, MSE diffuse).  The jitter /
    subset streams derive from `rng` (subset: offset, specular: offset + 1, diffuse: offset + 2).  Afterwards
    `workspace` holds the updated grid packed and a cleared gradient region."""
    device = densities.device
    cache = workspace.recon_cache
    key = _recon_key(spec, params, densities, features, height, width, focal, images, batch, diffuse_regularisation, losses)
    if (cache is not None and scratch_holder is None and cache[0] == key and cache[4] is workspace.buf and workspace.buf is not None
            and cache[5] is workspace2.buf and _recon_cameras_ok(poses, image_rows, cache[3].K)):
        # the same loop as the last call (grid, cameras' shape, images, batch, buffers): its descriptors with this iteration's
        # cameras, streams, optimiser state and flags -- the trainer's loop is paced by this function's host time
        L = lib()
        _, g, c0, rs0, ws, ws2, sc = cache
        c = type(c0).from_buffer_copy(c0)
        rs = type(rs0).from_buffer_copy(rs0)
        c.seed, c.rng_offset = int(rng[0]) & 0xFFFFFFFFFFFFFFFF, int(rng[1]) & 0xFFFFFFFFFFFFFFFF
        c.reuse_packed_grid = int(workspace.holds(spec, densities, features))
        rs.poses, rs.image_rows = ptr(poses), ptr(image_rows)
        rs.lr, rs.beta1, rs.beta2, rs.eps = float(lr), float(beta1), float(beta2), float(eps)
        rs.step_densities, rs.step_features = int(step_densities), int(step_features)
        m_d, v_d = state_densities if state_densities is not None else (None, None)
        m_f, v_f = state_features if state_features is not None else (None, None)
        rs.exp_avg_densities, rs.exp_avg_sq_densities = ptr(m_d), ptr(v_d)
        rs.exp_avg_features, rs.exp_avg_sq_features = ptr(m_f), ptr(v_f)
        rs.zero_gradient_first = int(bool(zero_gradient_first))
    else:
        L, g, c, rs, ws, ws2, sc, (m_d, v_d, m_f, v_f) = _recon_call(
            "recon_step_", spec, params, densities, features, workspace, workspace2, height, width, focal, poses, image_rows, images,
            batch, diffuse_regularisation, state_densities, state_features, step_densities, step_features, lr, losses, rng, beta1,
            beta2, eps, zero_gradient_first, scratch_holder)
    with torch.cuda.device(device):
        check(L.voxe_recon_step(C.byref(g), C.byref(c), C.byref(rs), ptr(ws), ws.numel(), ptr(ws2),
                                0 if ws2 is None else ws2.numel(), ptr(sc), sc.numel(), stream_ptr(device)), "voxe_recon_step")
    workspace.prefetch_inflight = False                    # (the step waited for the side stream, hint taken or not)
    workspace2.prefetch_inflight = False
    # what a hint for the NEXT iteration has to repeat (recon_prefetch_ copies these descriptors instead of building them again:
    # the hint's host time is on the iteration's critical path once the device work is hidden)
    workspace.recon_cache = (key, g, c, rs, ws, ws2, sc)
    workspace.prefetch_keepalive = None
    for t in (densities, features, m_d, v_d, m_f, v_f):
        if t is not None:
            torch.autograd.graph.increment_version(t)
    workspace.remember(spec, densities, features)          # the workspace holds the updated grid packed
    workspace.state_key = None
    workspace2.key = None                                  # (its packed grid is the previous iteration's)
    workspace2.state_key = None


def recon_prefetch_(spec: GridSpec, params: RenderParams, densities, features, workspace: Workspace, workspace2: Workspace,
                    height: int, width: int, focal: float, poses: torch.Tensor, image_rows: Optional[torch.Tensor],
                    images: torch.Tensor, batch: int, diffuse_regularisation: bool, losses: torch.Tensor, rng: Tuple[int, int],
                    scratch_holder: Optional[dict] = None) -> None:
    """voxe_recon_prefetch: announce the NEXT recon_step_ (same arguments; `poses`, `image_rows` and `rng` are the next
    iteration's; everything else must equal the last recon_step_ of this workspace, otherwise nothing is announced).  The library
    assembles that iteration's batch and segment tables on a stream of its own while the current iteration's backward and grid
    step run; the next recon_step_ takes them iff its arguments are the announced ones.  A hint: results never depend on it, and
    no buffer is ever allocated, grown or moved by it.  Call it right after recon_step_ (both workspaces and the scratch exist by then and keep
    their addresses); `poses` / `image_rows` are kept alive until the next recon_step_ of this workspace."""
    device = densities.device
    if workspace.buf is None:
        return                                             # (no step has sized the buffers yet: nothing to announce against)
    cache = workspace.recon_cache
    key = _recon_key(spec, params, densities, features, height, width, focal, images, batch, diffuse_regularisation, losses)
    if (cache is not None and scratch_holder is None and cache[0] == key and cache[4] is workspace.buf and cache[5] is workspace2.buf
            and _recon_cameras_ok(poses, image_rows, cache[3].K)):
        # the descriptors of the last step with the next iteration's cameras and streams
        L = lib()
        _, g, c0, rs0, ws, ws2, sc = cache
        c = type(c0).from_buffer_copy(c0)
        rs = type(rs0).from_buffer_copy(rs0)
        c.seed, c.rng_offset = int(rng[0]) & 0xFFFFFFFFFFFFFFFF, int(rng[1]) & 0xFFFFFFFFFFFFFFFF
        rs.poses, rs.image_rows = ptr(poses), ptr(image_rows)
    else:
        # Anything else (another batch size, grid, image stack, ... than the last step's) is not announced: marshalling it afresh
        # could regrow a workspace, and a hint must never move a buffer -- the caller's knowledge of what its workspace holds
        # (packed grid, cleared gradient region: `zero_gradient_first`) would silently go stale.  The next step bins inline.
        return
    with torch.cuda.device(device):
        check(L.voxe_recon_prefetch(C.byref(g), C.byref(c), C.byref(rs), ptr(ws), ws.numel(), ptr(ws2),
                                    0 if ws2 is None else ws2.numel(), ptr(sc), sc.numel(), stream_ptr(device)), "voxe_recon_prefetch")
    workspace.prefetch_inflight = True
    if workspace2 is not None:
        workspace2.prefetch_inflight = True
    workspace.prefetch_keepalive = (poses, image_rows, images)


@torch.no_grad()
def upsample_trilinear(src: torch.Tensor, out_size: Sequence[int]) -> torch.Tensor:
    """[X,Y,Z,C] -> [X2,Y2,Z2,C], F.interpolate(trilinear, align_corners=False) semantics
    (thre3d_atom/thre3d_reprs/voxels.py:409-447)."""
    require_device(src, "upsample_trilinear")
    s = f32c(src)
    X, Y, Z, Cn = s.shape
    X2, Y2, Z2 = (int(v) for v in out_size)
    device = s.device
    ensure_gfx950(device)
    with torch.cuda.device(device):
        dst = torch.empty((X2, Y2, Z2, Cn), dtype=torch.float32, device=device)
        check(lib().voxe_upsample_trilinear(ptr(s), X, Y, Z, Cn, ptr(dst), X2, Y2, Z2, stream_ptr(device)),
              "voxe_upsample_trilinear")
    return dst


# ---- refinement stage: grid graph cut / connected components -----------------------------------------------
def graph_build(density_grid: torch.Tensor, feature_grid: torch.Tensor, sigma: float = 0.1,
                dilate_yz: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Nodes and quantised n-link capacities of the refinement graph
    (thre3d_atom/modules/refinement_functions.py:182-287).  density_grid [X,Y,Z(,1)], feature_grid [X,Y,Z,F]
    -> node_mask uint8 [X,Y,Z], cap int32 [6,X,Y,Z] (abi.DIR_* planes, abi.GRAPH_CAP_ONE units)."""
    require_device(density_grid, "graph_build")
    require_device(feature_grid, "graph_build")
    dens = f32c(density_grid)
    feat = f32c(feature_grid)
    X, Y, Z = (int(v) for v in dens.shape[:3])
    if dens.numel() != X * Y * Z or feat.dim() != 4 or tuple(feat.shape[:3]) != (X, Y, Z):
        raise VoxeError(f"graph_build: density grid {tuple(dens.shape)} / feature grid {tuple(feat.shape)} mismatch")
    device = dens.device
    ensure_gfx950(device)
    with torch.cuda.device(device):
        node = torch.empty((X, Y, Z), dtype=torch.uint8, device=device)
        cap = torch.empty((6, X, Y, Z), dtype=torch.int32, device=device)
        check(lib().voxe_graph_build(ptr(dens), ptr(feat), X, Y, Z, int(feat.shape[3]), float(sigma),
                                     int(bool(dilate_yz)), ptr(node), ptr(cap), stream_ptr(device)),
              "voxe_graph_build")
    return node, cap


def graphcut(node_mask: torch.Tensor, terminal: torch.Tensor, cap: torch.Tensor):
    """Exact minimum cut of the voxel graph (g.maxflow() + get_segment, refinement_functions.py:289-294).
    terminal int8 [X,Y,Z]: +1 edit (source) seed, -1 object (sink) seed.  `cap` is not modified.
    -> segment uint8 [X,Y,Z] (0 edit / 1 object / 255 no node), flow value (python int, capacity units)."""
    for t, name in ((node_mask, "node_mask"), (terminal, "terminal"), (cap, "cap")):
        require_device(t, f"graphcut({name})")
    X, Y, Z = (int(v) for v in node_mask.shape)
    if node_mask.dtype != torch.uint8 or terminal.dtype != torch.int8 or cap.dtype != torch.int32:
        raise VoxeError("graphcut: expected uint8 node_mask, int8 terminal, int32 cap")
    if tuple(terminal.shape) != (X, Y, Z) or tuple(cap.shape) != (6, X, Y, Z):
        raise VoxeError("graphcut: shape mismatch")
    device = node_mask.device
    ensure_gfx950(device)
    with torch.cuda.device(device):
        residual = cap.contiguous().clone()
        node, term = node_mask.contiguous(), terminal.contiguous()
        segment = torch.empty((X, Y, Z), dtype=torch.uint8, device=device)
        flow = torch.zeros((1,), dtype=torch.int64, device=device)
        nbytes = int(lib().voxe_graphcut_scratch_bytes(X, Y, Z))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        check(lib().voxe_graphcut(ptr(node), ptr(term), ptr(residual), X, Y, Z, ptr(segment), ptr(flow),
                                  ptr(scratch), nbytes, stream_ptr(device)), "voxe_graphcut")
    return segment, int(flow.item())


def cc_largest_k(mask: torch.Tensor, k: int) -> Tuple[torch.Tensor, int]:
    """cc3d.largest_k(mask, k, connectivity=26) (edit_pretrained_relu_field.py:384-389): int32 labels [X,Y,Z]
    (the M = min(k, N) largest components numbered 1..M by ascending size) and N."""
    require_device(mask, "cc_largest_k")
    m = (mask != 0).to(torch.uint8).contiguous()
    if m.dim() != 3:
        raise VoxeError(f"cc_largest_k: expected a [X,Y,Z] mask, got {tuple(m.shape)}")
    X, Y, Z = (int(v) for v in m.shape)
    device = m.device
    ensure_gfx950(device)
    with torch.cuda.device(device):
        labels = torch.empty((X, Y, Z), dtype=torch.int32, device=device)
        ncomp = torch.zeros((1,), dtype=torch.int32, device=device)
        nbytes = int(lib().voxe_cc_scratch_bytes(X, Y, Z, int(k)))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        check(lib().voxe_cc_largest_k(ptr(m), X, Y, Z, int(k), ptr(labels), ptr(ncomp), ptr(scratch), nbytes,
                                      stream_ptr(device)), "voxe_cc_largest_k")
    return labels, int(ncomp.item())


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
# mesh export (marching cubes over the density iso-surface; DESIGN.md section 4 "Mesh export")
# ------------------------------------------------------------------------------------------------
def extract_mesh(spec: GridSpec, densities: torch.Tensor, level: float,
                 mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Closed, outward-wound triangle mesh of {density == level} on the device: vertices [V,3] float32 (world space),
    faces [T,3] int32.  `mask` ([X,Y,Z] or [X,Y,Z,1], bool / uint8, 0 = excluded) turns voxels into outside.  The count
    pass's totals are read back once (one synchronisation) to size the outputs."""
    require_device(densities, "extract_mesh (densities)")
    if densities.dim() != 4 or densities.shape[-1] != 1:
        raise VoxeError(f"extract_mesh: densities must be [X,Y,Z,1]; got {tuple(densities.shape)}")
    dens = f32c(densities.detach())
    device = dens.device
    X, Y, Z = (int(s) for s in dens.shape[:3])
    m = None
    if mask is not None:
        require_device(mask, "extract_mesh (mask)")
        if tuple(mask.shape[:3]) != (X, Y, Z) or mask.numel() != X * Y * Z:
            raise VoxeError(f"extract_mesh: mask must be [X,Y,Z]=({X},{Y},{Z}); got {tuple(mask.shape)}")
        m = (mask.reshape(X, Y, Z) != 0).to(torch.uint8).contiguous()
    ensure_gfx950(device)
    L = lib()
    g = make_grid_desc(dens.data_ptr(), dens.data_ptr(), (X, Y, Z), 1, spec.aabb, spec.density_scale,
                       spec.density_pre_act, spec.density_post_act, spec.feature_kind)
    with torch.cuda.device(device):
        nbytes = L.voxe_mesh_scratch_bytes(X, Y, Z)
        if nbytes == 0:
            raise VoxeError(f"extract_mesh: grid {X}x{Y}x{Z} is too large for int32 vertex / triangle ids")
        sc = _scratch_for(device, nbytes)
        totals = torch.empty(2, dtype=torch.int64, device=device)
        st = stream_ptr(device)
        check(L.voxe_mesh_count(C.byref(g), float(level), ptr(m), ptr(totals), ptr(sc), sc.numel(), st), "voxe_mesh_count")
        V, T = (int(v) for v in totals.cpu())
        if V >= 2 ** 31 or T >= 2 ** 31:
            raise VoxeError(f"extract_mesh: {V} vertices / {T} triangles exceed int32 ids")
        vertices = torch.empty((V, 3), dtype=torch.float32, device=device)
        faces = torch.empty((T, 3), dtype=torch.int32, device=device)
        check(L.voxe_mesh_emit(C.byref(g), float(level), ptr(m), ptr(vertices), V, ptr(faces), T, ptr(sc), sc.numel(), st),
              "voxe_mesh_emit")
    return vertices, faces


# ------------------------------------------------------------------------------------------------
# density-gradient normals (DESIGN.md section 4 "Normals"): read the raw densities only, no workspace, not differentiable
# ------------------------------------------------------------------------------------------------
def _normals_grid_desc(spec: GridSpec, dens: torch.Tensor):
    X, Y, Z = (int(s) for s in dens.shape[:3])
    # (features, F and feature_kind are not read by the normals entry points: no feature tensor is needed)
    return make_grid_desc(dens.data_ptr(), 0, (X, Y, Z), 0, spec.aabb, spec.density_scale, spec.density_pre_act,
                          spec.density_post_act, spec.feature_kind)


def _check_densities(densities: torch.Tensor, what: str) -> None:
    require_device(densities, f"{what} (densities)")
    if densities.dim() != 4 or densities.shape[-1] != 1:
        raise VoxeError(f"{what}: densities must be [X,Y,Z,1]; got {tuple(densities.shape)}")


def query_normals(spec: GridSpec, densities: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """n(p) = -grad V / |grad V| at world points [N,3] -> [N,3] float32 ((0,0,0) where the gradient vanishes, e.g. outside the
    grid).  V is the trilinear pre-activated density VoxelGrid.forward interpolates; no gradient flows through the result."""
    _check_densities(densities, "query_normals")
    require_device(points, "query_normals (points)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise VoxeError(f"query_normals: points must be [N,3]; got {tuple(points.shape)}")
    device = densities.device
    ensure_gfx950(device)
    dens, pts = f32c(densities.detach()), f32c(points.detach().to(device))
    g = _normals_grid_desc(spec, dens)
    N = pts.shape[0]
    with torch.cuda.device(device):
        out = torch.empty((N, 3), dtype=torch.float32, device=device)
        check(lib().voxe_query_normals(C.byref(g), ptr(pts), N, ptr(out), stream_ptr(device)), "voxe_query_normals")
    return out


def render_normals(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor,
                   jitter: Optional[torch.Tensor] = None, rng: Optional[Tuple[int, int]] = None):
    """Rendered normals of flat rays: (normals [R,3] = sum_k w_k n(p_k) in world space, not renormalised; depth [R,1];
    acc [R,1]) with the samples and weights `render` uses for the same params, jitter and rng (`rng` follows render's rule:
    None = a fresh stream when params.perturb and no jitter is given).  The background and white_bkgd do not apply.
    Not differentiable."""
    _check_densities(densities, "render_normals")
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        require_device(t, f"render_normals ({name})")
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_o.shape != rays_d.shape:
        raise VoxeError(f"rays must be flat [R,3]; got {tuple(rays_o.shape)}, {tuple(rays_d.shape)}")
    if jitter is not None and tuple(jitter.shape) != (rays_o.shape[0], params.num_samples):
        raise VoxeError(f"jitter must be [R,S]={rays_o.shape[0], params.num_samples}; got {tuple(jitter.shape)}")
    if rng is None:
        rng = _next_rng() if (params.perturb and jitter is None) else (0, 0)
    device = densities.device
    ensure_gfx950(device)
    dens, ro, rd = f32c(densities.detach()), f32c(rays_o.detach()), f32c(rays_d.detach())
    jit = None if jitter is None else f32c(jitter.detach())
    g = _normals_grid_desc(spec, dens)
    c = make_render_cfg(params.num_samples, params.near, params.far, params.perturb, params.linear_disparity, params.aabb_clip,
                        seed=rng[0], rng_offset=rng[1], image_width=params.image_width, image_height=params.image_height)
    R = ro.shape[0]
    with torch.cuda.device(device):
        normals = torch.empty((R, 3), dtype=torch.float32, device=device)
        depth = torch.empty((R, 1), dtype=torch.float32, device=device)
        acc = torch.empty((R, 1), dtype=torch.float32, device=device)
        check(lib().voxe_render_normals(C.byref(g), C.byref(c), ptr(ro), ptr(rd), R, ptr(jit), ptr(normals), ptr(depth),
                                        ptr(acc), stream_ptr(device)), "voxe_render_normals")
    return normals, depth, acc


# ------------------------------------------------------------------------------------------------
# per-voxel visibility (DESIGN.md section 4 "Visibility"): reads the raw densities only, no workspace, not differentiable
# ------------------------------------------------------------------------------------------------
def visibility_accumulate_(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor,
                           rays_d: torch.Tensor, max_weight: Optional[torch.Tensor] = None,
                           max_trans: Optional[torch.Tensor] = None, jitter: Optional[torch.Tensor] = None,
                           rng: Optional[Tuple[int, int]] = None) -> None:
    """Raise, in place, max_weight[c] to w_k * t_c and max_trans[c] to T_k over every sample k of the flat rays and every
    corner c of its trilinear footprint (t_c the gather weight, w_k = T_k alpha_k, T_k the transmittance on arrival), with the
    samples and weights `render` uses for the same params, jitter and rng (`rng` follows render's rule).  The buffers
    ([X,Y,Z] or [X,Y,Z,1] float32, contiguous, either may be None) ACCUMULATE: zero them before the first call.  The result is
    the same bit for bit however the rays are split over calls or ordered."""
    _check_densities(densities, "visibility_accumulate_")
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        require_device(t, f"visibility_accumulate_ ({name})")
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_o.shape != rays_d.shape:
        raise VoxeError(f"rays must be flat [R,3]; got {tuple(rays_o.shape)}, {tuple(rays_d.shape)}")
    if jitter is not None and tuple(jitter.shape) != (rays_o.shape[0], params.num_samples):
        raise VoxeError(f"jitter must be [R,S]={rays_o.shape[0], params.num_samples}; got {tuple(jitter.shape)}")
    device = densities.device
    nvox = densities.numel()
    for name, t in (("max_weight", max_weight), ("max_trans", max_trans)):
        if t is None:
            continue
        require_device(t, f"visibility_accumulate_ ({name})")
        if (t.dtype != torch.float32 or not t.is_contiguous() or t.device != device or t.numel() != nvox
                or tuple(t.shape[:3]) != tuple(densities.shape[:3])):
            raise VoxeError(f"visibility_accumulate_: {name} must be a contiguous float32 [X,Y,Z] buffer on the grid's device; "
                            f"got {tuple(t.shape)} {t.dtype}")
    if rng is None:
        rng = _next_rng() if (params.perturb and jitter is None) else (0, 0)
    ensure_gfx950(device)
    dens, ro, rd = f32c(densities.detach()), f32c(rays_o.detach()), f32c(rays_d.detach())
    jit = None if jitter is None else f32c(jitter.detach())
    g = _normals_grid_desc(spec, dens)
    c = make_render_cfg(params.num_samples, params.near, params.far, params.perturb, params.linear_disparity, params.aabb_clip,
                        seed=rng[0], rng_offset=rng[1], image_width=params.image_width, image_height=params.image_height)
    with torch.cuda.device(device):
        check(lib().voxe_visibility_accumulate(C.byref(g), C.byref(c), ptr(ro), ptr(rd), ro.shape[0], ptr(jit), ptr(max_weight),
                                               ptr(max_trans), stream_ptr(device)), "voxe_visibility_accumulate")


def visibility_mask(vis: torch.Tensor, threshold: float, dilate: int = 0) -> torch.Tensor:
    """uint8 [X,Y,Z]: 1 where some voxel within Chebyshev distance `dilate` (0..3) has vis > threshold (strict; NaN never)."""
    require_device(vis, "visibility_mask (vis)")
    if vis.dim() == 4 and vis.shape[-1] == 1:
        vis = vis[..., 0]
    if vis.dim() != 3:
        raise VoxeError(f"visibility_mask: vis must be [X,Y,Z]; got {tuple(vis.shape)}")
    v = f32c(vis.detach())
    device = v.device
    ensure_gfx950(device)
    X, Y, Z = (int(s) for s in v.shape)
    with torch.cuda.device(device):
        mask = torch.empty((X, Y, Z), dtype=torch.uint8, device=device)
        check(lib().voxe_visibility_mask(ptr(v), X, Y, Z, float(threshold), int(dilate), ptr(mask), stream_ptr(device)),
              "voxe_visibility_mask")
    return mask


# ------------------------------------------------------------------------------------------------
# rigid transform / re-gridding / composition of grids: no workspace, not differentiable
# ------------------------------------------------------------------------------------------------
def make_resample(A, b, sh_rot=None, sh_degree: int = -1, density_pre_act: int = abi.ACT_IDENTITY, density_fill: float = 0.0,
                  mode: int = abi.RESAMPLE_REPLACE) -> abi.VoxeResample:
    """VoxeResample from host values: A (3x3) and b (3) in any float type (cast to float32 here), sh_rot the list of band
    blocks M_0..M_deg ((2l+1) x (2l+1) each, as thre3d_reprs.transform.sh_rotation_matrices returns them) or None."""
    xf = abi.VoxeResample()
    flat = [float(v) for row in A for v in row]
    if len(flat) != 9 or len(b) != 3:
        raise VoxeError("grid_resample: A must be 3x3 and b of length 3")
    xf.A[:] = flat
    xf.b[:] = [float(v) for v in b]
    xf.sh_rot[0] = 1.0
    for l in range(1, 4):   # identity blocks where none is given
        for j in range(2 * l + 1):
            xf.sh_rot[abi.SH_ROT_OFFSETS[l] + j * (2 * l + 2)] = 1.0
    if sh_degree >= 0:
        if sh_rot is None or len(sh_rot) < sh_degree + 1:
            raise VoxeError(f"grid_resample: sh_degree {sh_degree} needs the rotation blocks M_0..M_{sh_degree}")
        for l in range(1, sh_degree + 1):   # (band 0 is the identity by definition)
            n = 2 * l + 1
            vals = [float(v) for row in sh_rot[l] for v in row]
            if len(vals) != n * n:
                raise VoxeError(f"grid_resample: M_{l} must be {n}x{n}")
            xf.sh_rot[abi.SH_ROT_OFFSETS[l]:abi.SH_ROT_OFFSETS[l + 1]] = vals
    xf.sh_degree, xf.density_pre_act, xf.mode, xf.density_fill = int(sh_degree), int(density_pre_act), int(mode), float(density_fill)
    return xf


@torch.no_grad()
def grid_resample(src_densities: Optional[torch.Tensor], src_features: Optional[torch.Tensor], xf: abi.VoxeResample,
                  dst_dims: Optional[Sequence[int]] = None, dst_densities: Optional[torch.Tensor] = None,
                  dst_features: Optional[torch.Tensor] = None, want_taken: bool = False):
    """voxe_grid_resample (include/voxe.h): sample the source grid ([X,Y,Z,1] densities and / or [X,Y,Z,C] features) at
    u = A i + b for every voxel i of the destination.  REPLACE: new float32 tensors of `dst_dims` are returned.  UNION:
    `dst_densities` (and `dst_features` when the source has features) are updated in place -- contiguous float32 tensors that do
    not alias the source.  Returns (densities, features, taken): taken is a uint8 [X2,Y2,Z2] tensor when want_taken, else
    None."""
    union = xf.mode == abi.RESAMPLE_UNION
    srcs = [t for t in (src_densities, src_features) if t is not None]
    if not srcs:
        raise VoxeError("grid_resample: neither densities nor features given")
    for t in srcs:
        require_device(t, "grid_resample")
        if t.dim() != 4:
            raise VoxeError(f"grid_resample: source tensors must be [X,Y,Z,C]; got {tuple(t.shape)}")
    device = srcs[0].device
    X, Y, Z = (int(v) for v in srcs[0].shape[:3])
    if any(tuple(t.shape[:3]) != (X, Y, Z) or t.device != device for t in srcs):
        raise VoxeError("grid_resample: source densities and features must share dims and device")
    if src_densities is not None and src_densities.shape[-1] != 1:
        raise VoxeError(f"grid_resample: densities must be [X,Y,Z,1]; got {tuple(src_densities.shape)}")
    Cn = int(src_features.shape[-1]) if src_features is not None else 1
    sd = None if src_densities is None else f32c(src_densities.detach())
    sf = None if src_features is None else f32c(src_features.detach())
    ensure_gfx950(device)
    with torch.cuda.device(device):
        if union:
            if dst_densities is None or sd is None or (sf is not None and dst_features is None):
                raise VoxeError("grid_resample: UNION runs in place on dst_densities (and dst_features) and needs the densities")
            dd, df = dst_densities, (dst_features if sf is not None else None)
            dims2 = tuple(int(v) for v in dd.shape[:3])
            for name, t, ch, s_ in (("dst_densities", dd, 1, sd), ("dst_features", df, Cn, sf)):
                if t is None:
                    continue
                require_device(t, f"grid_resample ({name})")
                if (t.dtype != torch.float32 or not t.is_contiguous() or t.device != device or t.dim() != 4
                        or tuple(t.shape) != (*dims2, ch)):
                    raise VoxeError(f"grid_resample: {name} must be a contiguous float32 {(*dims2, ch)} tensor on the source's "
                                    f"device; got {tuple(t.shape)} {t.dtype}")
                if t.untyped_storage().data_ptr() == s_.untyped_storage().data_ptr():
                    raise VoxeError("grid_resample: source and destination must not alias")
        else:
            if dst_dims is None or dst_densities is not None or dst_features is not None:
                raise VoxeError("grid_resample: REPLACE allocates its outputs: pass dst_dims and no destination tensors")
            dims2 = tuple(int(v) for v in dst_dims)
            if len(dims2) != 3 or min(dims2) <= 0:
                raise VoxeError(f"grid_resample: dst_dims must be three positive ints; got {dims2}")
            dd = None if sd is None else torch.empty((*dims2, 1), dtype=torch.float32, device=device)
            df = None if sf is None else torch.empty((*dims2, Cn), dtype=torch.float32, device=device)
        taken = torch.empty(dims2, dtype=torch.uint8, device=device) if want_taken else None
        check(lib().voxe_grid_resample(ptr(sd), ptr(sf), X, Y, Z, Cn, ptr(dd), ptr(df), *dims2, C.byref(xf), ptr(taken),
                                       stream_ptr(device)), "voxe_grid_resample")
    if union:
        # the library wrote the destination through raw pointers: tell autograd and the packed-grid caches
        for t in (dd, df):
            if t is not None:
                torch.autograd.graph.increment_version(t)
    return dd, df, taken


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
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        require_device(t, f"distortion_loss ({name})")
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_o.shape != rays_d.shape:
        raise VoxeError(f"rays must be flat [R,3]; got {tuple(rays_o.shape)}, {tuple(rays_d.shape)}")
    if jitter is not None and tuple(jitter.shape) != (rays_o.shape[0], params.num_samples):
        raise VoxeError(f"jitter must be [R,S]={rays_o.shape[0], params.num_samples}; got {tuple(jitter.shape)}")
    device = densities.device
    if d_densities is not None:
        require_device(d_densities, "distortion_loss (d_densities)")
        if (d_densities.dtype != torch.float32 or not d_densities.is_contiguous() or d_densities.device != device
                or d_densities.shape != densities.shape):
            raise VoxeError("distortion_loss: d_densities must be a contiguous float32 buffer of the densities' shape on the "
                            f"grid's device; got {tuple(d_densities.shape)} {d_densities.dtype}")
    ensure_gfx950(device)
    dens, ro, rd = f32c(densities.detach()), f32c(rays_o.detach()), f32c(rays_d.detach())
    jit = None if jitter is None else f32c(jitter.detach())
    g = _normals_grid_desc(spec, dens)
    c = make_render_cfg(params.num_samples, params.near, params.far, params.perturb, params.linear_disparity, params.aabb_clip,
                        seed=rng[0], rng_offset=rng[1], image_width=params.image_width, image_height=params.image_height)
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
    if d_densities is not None:
        torch.autograd.graph.increment_version(d_densities)
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
    if rng is None:
        rng = _next_rng() if (params.perturb and jitter is None) else (0, 0)
    return _DistortionFn.apply(densities, spec, params, rays_o, rays_d, jitter, rng, bool(return_ray_loss), int(_lanes))


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
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != device or tuple(t.shape) != (R, 3)):
            raise VoxeError(f"render_bwd_rays: {name} must be a contiguous float32 [R,3] buffer on the grid's device")
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
    for t in (d_rays_o, d_rays_d):
        if t is not None:
            torch.autograd.graph.increment_version(t)
    return d_o, d_d


def cast_rays_bwd(height: int, width: int, focal: float, poses: torch.Tensor, flat_index: Optional[torch.Tensor],
                  g_rays_o: Optional[torch.Tensor], g_rays_d: Optional[torch.Tensor], want_focal: bool = False,
                  d_poses: Optional[torch.Tensor] = None, d_focal: Optional[torch.Tensor] = None, accumulate: bool = False):
    """voxe_cast_rays_bwd: (d_poses [K,3,4], d_focal [] or None) of the rays cast_rays_indexed(height, width, focal, poses,
    flat_index) returns -- flat_index None: the K whole images, ray i = pixel i -- for the upstream gradients g_rays_o / g_rays_d
    [B,3] (either may be None = 0).  d_poses / d_focal: caller's buffers, added to when `accumulate`."""
    require_device(poses, "cast_rays_bwd")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise VoxeError("cast_rays_bwd: poses must be [K,3,4]")
    device = poses.device
    ensure_gfx950(device)
    p = f32c(poses.detach())
    K = int(p.shape[0])
    if flat_index is not None:
        require_device(flat_index, "cast_rays_bwd")
        if flat_index.dtype != torch.int64 or flat_index.dim() != 1:
            raise VoxeError("cast_rays_bwd: flat_index must be int64 [B]")
        idx = flat_index.contiguous()
        B = int(idx.shape[0])
    else:
        idx, B = None, K * int(height) * int(width)
    ups = []
    for name, t in (("g_rays_o", g_rays_o), ("g_rays_d", g_rays_d)):
        if t is not None:
            require_device(t, f"cast_rays_bwd ({name})")
            if tuple(t.shape) != (B, 3):
                raise VoxeError(f"cast_rays_bwd: {name} must be [B,3]={B, 3}; got {tuple(t.shape)}")
            t = f32c(t.detach())
        ups.append(t)
    L = lib()
    with torch.cuda.device(device):
        if d_poses is None:
            d_poses = torch.empty((K, 3, 4), dtype=torch.float32, device=device)
        if d_focal is None and want_focal:
            d_focal = torch.empty((), dtype=torch.float32, device=device)
        sc = _scratch_for(device, L.voxe_cast_rays_bwd_scratch_bytes(K))
        check(L.voxe_cast_rays_bwd(int(height), int(width), float(focal), ptr(p), K, ptr(idx), B, ptr(ups[0]), ptr(ups[1]),
                                   ptr(d_poses), ptr(d_focal), 1 if accumulate else 0, ptr(sc), sc.numel(), stream_ptr(device)),
              "voxe_cast_rays_bwd")
    return d_poses, d_focal


class _CastRaysFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, poses, focal_tensor, flat_index, height, width, focal):
        ctx.set_materialize_grads(False)
        if flat_index is None:
            # whole images through the indexed kernel: per pixel the arithmetic of voxe_cast_rays, bit for bit
            index = torch.arange(poses.shape[0] * height * width, dtype=torch.int64, device=poses.device)
        else:
            index = flat_index
        ro, rd = cast_rays_indexed(height, width, focal, poses.detach(), index)
        ctx.save_for_backward(poses, flat_index)
        ctx.geometry = (height, width, focal)
        ctx.focal_like = focal_tensor
        return ro, rd

    @staticmethod
    def backward(ctx, g_o, g_d):
        poses, flat_index = ctx.saved_tensors
        height, width, focal = ctx.geometry
        want_focal = ctx.focal_like is not None and ctx.needs_input_grad[1]
        if not (ctx.needs_input_grad[0] or want_focal) or (g_o is None and g_d is None):
            return (None,) * 6
        d_poses, d_focal = cast_rays_bwd(height, width, focal, poses, flat_index, g_o, g_d, want_focal=want_focal)
        if want_focal:
            d_focal = d_focal.to(device=ctx.focal_like.device, dtype=ctx.focal_like.dtype).reshape(ctx.focal_like.shape)
        return (d_poses.to(poses.dtype) if ctx.needs_input_grad[0] else None), (d_focal if want_focal else None), None, None, None, None


def cast_rays_from_poses(height: int, width: int, focal, poses: torch.Tensor,
                         flat_index: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """rays_o, rays_d [B,3] of poses [K,3,4] (rotation | translation, on the GPU), differentiable w.r.t. `poses` and, when
    `focal` is a 0-dim tensor, w.r.t. the focal length.  flat_index (int64 [B], (camera * H + y) * W + x) picks pixels as
    cast_rays_indexed does; None: the K whole images one after the other.  The forward's bits are those of cast_rays /
    cast_rays_indexed."""
    require_device(poses, "cast_rays_from_poses")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise VoxeError("cast_rays_from_poses: poses must be [K,3,4]")
    focal_tensor = focal if isinstance(focal, torch.Tensor) else None
    if focal_tensor is not None and focal_tensor.dim() != 0:
        raise VoxeError("cast_rays_from_poses: focal must be a number or a 0-dim tensor")
    value = float(focal) if focal_tensor is None else float(focal_tensor.detach())
    return _CastRaysFn.apply(poses, focal_tensor, flat_index, int(height), int(width), value)


# ------------------------------------------------------------------------------------------------
# real-capture cameras: intrinsics + lens distortion
# ------------------------------------------------------------------------------------------------
def _camera_struct(camera, intrinsics=None) -> abi.VoxeCamera:
    """abi.VoxeCamera of `camera`: an abi.VoxeCamera, or any object with height, width, fx, fy, cx, cy and distortion (k1 k2 p1 p2
    k3) such as thre3d_atom's PinholeCamera, or a plain (height, width, focal) tuple (centred, no distortion).  `intrinsics`
    (4 numbers fx fy cx cy) replaces the camera's own."""
    if isinstance(camera, abi.VoxeCamera):
        c = abi.VoxeCamera.from_buffer_copy(camera)
    elif hasattr(camera, "fx"):
        k = [float(v) for v in camera.distortion] + [0.0] * 5
        c = abi.VoxeCamera(int(camera.height), int(camera.width), float(camera.fx), float(camera.fy), float(camera.cx),
                           float(camera.cy), *k[:5])
    else:
        height, width, focal = camera
        c = abi.VoxeCamera(int(height), int(width), float(focal), float(focal), int(width) * 0.5, int(height) * 0.5, 0, 0, 0, 0, 0)
    if intrinsics is not None:
        c.fx, c.fy, c.cx, c.cy = (float(v) for v in intrinsics)
    return c


def _camera_call_inputs(name: str, poses: torch.Tensor, flat_index: Optional[torch.Tensor], cam: abi.VoxeCamera):
    require_device(poses, name)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise VoxeError(f"{name}: poses must be [K,3,4]")
    ensure_gfx950(poses.device)
    p = f32c(poses.detach())
    K = int(p.shape[0])
    if flat_index is not None:
        require_device(flat_index, name)
        if flat_index.dtype != torch.int64 or flat_index.dim() != 1:
            raise VoxeError(f"{name}: flat_index must be int64 [B]")
        idx = flat_index.contiguous()
        B = int(idx.shape[0])
        if B == 0:   # (an empty tensor has no address, and a NULL index means whole images)
            idx = torch.zeros((1,), dtype=torch.int64, device=p.device)
    else:
        idx, B = None, K * int(cam.H) * int(cam.W)
    return p, K, idx, B


def cast_rays_camera(camera, poses: torch.Tensor, flat_index: Optional[torch.Tensor] = None,
                     intrinsics=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """voxe_cast_rays_camera: rays_o, rays_d [B,3] of `camera` (see _camera_struct) at poses [K,3,4] (GPU).  flat_index (int64
    [B], (camera * H + y) * W + x) picks pixels; None: the K whole images one after the other."""
    cam = _camera_struct(camera, intrinsics)
    p, K, idx, B = _camera_call_inputs("cast_rays_camera", poses, flat_index, cam)
    device = p.device
    with torch.cuda.device(device):
        ro = torch.empty((B, 3), dtype=torch.float32, device=device)
        rd = torch.empty((B, 3), dtype=torch.float32, device=device)
        check(lib().voxe_cast_rays_camera(C.byref(cam), ptr(p), K, ptr(idx), B, ptr(ro), ptr(rd), stream_ptr(device)),
              "voxe_cast_rays_camera")
    return ro, rd


def cast_rays_camera_bwd(camera, poses: torch.Tensor, flat_index: Optional[torch.Tensor], g_rays_o: Optional[torch.Tensor],
                         g_rays_d: Optional[torch.Tensor], want_poses: bool = True, want_intrinsics: bool = False,
                         want_distortion: bool = False, d_poses: Optional[torch.Tensor] = None,
                         d_intrinsics: Optional[torch.Tensor] = None, d_distortion: Optional[torch.Tensor] = None,
                         accumulate: bool = False, intrinsics=None):
    """voxe_cast_rays_camera_bwd: (d_poses [K,3,4], d_intrinsics [4] fx fy cx cy, d_distortion [5] k1 k2 p1 p2 k3) of the rays
    cast_rays_camera(camera, poses, flat_index) returns, for the upstream gradients g_rays_o / g_rays_d [B,3] (either may be None
    = 0).  An output is None unless wanted or given as the caller's buffer, which is added to when `accumulate`."""
    cam = _camera_struct(camera, intrinsics)
    p, K, idx, B = _camera_call_inputs("cast_rays_camera_bwd", poses, flat_index, cam)
    device = p.device
    ups = []
    for name, t in (("g_rays_o", g_rays_o), ("g_rays_d", g_rays_d)):
        if t is not None:
            require_device(t, f"cast_rays_camera_bwd ({name})")
            if tuple(t.shape) != (B, 3):
                raise VoxeError(f"cast_rays_camera_bwd: {name} must be [B,3]={B, 3}; got {tuple(t.shape)}")
            t = f32c(t.detach())
        ups.append(t)
    for name, t, shape in (("d_poses", d_poses, (K, 3, 4)), ("d_intrinsics", d_intrinsics, (4,)), ("d_distortion", d_distortion, (5,))):
        if t is not None:
            require_device(t, f"cast_rays_camera_bwd ({name})")
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
                raise VoxeError(f"cast_rays_camera_bwd: {name} must be contiguous float32 {shape}")
    L = lib()
    with torch.cuda.device(device):
        if d_poses is None and want_poses:
            d_poses = torch.empty((K, 3, 4), dtype=torch.float32, device=device)
        if d_intrinsics is None and want_intrinsics:
            d_intrinsics = torch.empty((4,), dtype=torch.float32, device=device)
        if d_distortion is None and want_distortion:
            d_distortion = torch.empty((5,), dtype=torch.float32, device=device)
        sc = _scratch_for(device, L.voxe_cast_rays_camera_bwd_scratch_bytes(K))
        check(L.voxe_cast_rays_camera_bwd(C.byref(cam), ptr(p), K, ptr(idx), B, ptr(ups[0]), ptr(ups[1]), ptr(d_poses),
                                          ptr(d_intrinsics), ptr(d_distortion), 1 if accumulate else 0, ptr(sc), sc.numel(),
                                          stream_ptr(device)), "voxe_cast_rays_camera_bwd")
    return d_poses, d_intrinsics, d_distortion


class _CastRaysCameraFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, poses, intrinsics, distortion, flat_index, cam):
        ctx.set_materialize_grads(False)
        ro, rd = cast_rays_camera(cam, poses.detach(), flat_index)
        ctx.save_for_backward(poses, flat_index)
        ctx.cam = cam
        ctx.like = [None if t is None else (t.device, t.dtype, t.shape) for t in (intrinsics, distortion)]
        return ro, rd

    @staticmethod
    def backward(ctx, g_o, g_d):
        poses, flat_index = ctx.saved_tensors
        want = [bool(n) for n in ctx.needs_input_grad[:3]]
        if not any(want) or (g_o is None and g_d is None):
            return (None,) * 5
        outs = cast_rays_camera_bwd(ctx.cam, poses, flat_index, g_o, g_d, want_poses=want[0], want_intrinsics=want[1],
                                    want_distortion=want[2])
        grads = [outs[0].to(poses.dtype) if want[0] else None]
        for got, like, w in zip(outs[1:], ctx.like, want[1:]):
            grads.append(got.to(device=like[0], dtype=like[1]).reshape(like[2]) if w else None)
        return (*grads, None, None)


def cast_rays_from_camera(camera, poses: torch.Tensor, flat_index: Optional[torch.Tensor] = None,
                          intrinsics: Optional[torch.Tensor] = None,
                          distortion: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """rays_o, rays_d [B,3] of `camera` at poses [K,3,4] (GPU), differentiable w.r.t. `poses` and the optional tensors
    `intrinsics` [4] (fx fy cx cy) and `distortion` [5] (k1 k2 p1 p2 k3), whose VALUES replace the camera's own.  The forward's
    bits are those of cast_rays_camera.  The camera travels by value in the call's arguments, so the two tensors are read on the
    host: keep them there (as LearnedIntrinsics does), a device tensor costs a synchronisation per call."""
    cam = _camera_struct(camera)
    if intrinsics is not None:
        if not isinstance(intrinsics, torch.Tensor) or tuple(intrinsics.shape) != (4,):
            raise VoxeError("cast_rays_from_camera: intrinsics must be a tensor [4] = fx fy cx cy")
        cam.fx, cam.fy, cam.cx, cam.cy = (float(v) for v in intrinsics.detach().cpu())
    if distortion is not None:
        if not isinstance(distortion, torch.Tensor) or tuple(distortion.shape) != (5,):
            raise VoxeError("cast_rays_from_camera: distortion must be a tensor [5] = k1 k2 p1 p2 k3")
        cam.k1, cam.k2, cam.p1, cam.p2, cam.k3 = (float(v) for v in distortion.detach().cpu())
    require_device(poses, "cast_rays_from_camera")
    return _CastRaysCameraFn.apply(poses, intrinsics, distortion, flat_index, cam)
