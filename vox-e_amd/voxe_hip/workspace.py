"""The caller-owned workspace of the render, query and fused-step entry points and the protocols that live on it.  Plain Python
over tensors: no library call is made here, and nothing outside this module assigns an attribute of its classes.
* the two caches, "the buffer still holds this grid packed" (VoxeRenderCfg::reuse_packed_grid) and "it still holds this forward's ray
  states" (::ray_state_valid): an entry point of voxe_hip.ops asks `Workspace.before_call`, calls the library, tells `after_call`;
* the deferred-gradient mode (`DeferredGrad`, `Workspace.attach_deferred` / `detach_deferred` / `call_failed`): must the gradient
  region be cleared before a backward accumulates into it;
* the reconstruction loop (`ReconLoop` = `Workspace.recon`): the last step's descriptors, named scratch, a hint in flight;
* a differentiable forward waiting for its backward (`forward_pending`, `backward_ran`, `partner`)."""
import weakref
from collections import namedtuple
from dataclasses import dataclass
from operator import attrgetter
from typing import Optional

import torch

from . import abi
from . import dispatch as _dispatch
from .runtime import VoxeError, ptr

# what a library call did to the ray states (Workspace.after_call; a tuple names the forward whose states it left)
UNTOUCHED, DROPPED = "untouched", "dropped"


@dataclass
class DeferredGrad:
    """state of the deferred-gradient mode of one grid: which layout the accumulated gradient has and whether the region
    holds anything since the last optimiser step"""
    layout: int = abi.GRAD_ANY
    dirty: bool = False
    want_densities: bool = True
    want_features: bool = True
    clean_ptr: int = 0        # data_ptr of the workspace buffer whose gradient region is known to be cleared / in use

    def must_clear(self, buf) -> bool:
        """THE question "clear the region first" (a buffer this mode has not written holds whatever torch.empty returned)"""
        return not self.dirty and (buf is None or self.clean_ptr != buf.data_ptr())

    def expected_layout(self) -> int:
        return self.layout if self.dirty else abi.GRAD_ANY

    def accumulated(self, buf, layout: int) -> None:
        """a backward left a gradient of `layout` in the region of `buf` (GRAD_ANY: no rays, nothing but the clearing)"""
        self.clean_ptr = buf.data_ptr()
        if layout != abi.GRAD_ANY:
            self.layout, self.dirty = layout, True

    def consumed(self, buf) -> None:
        """an optimiser step (or zero_grad) took the gradient and left the region of `buf` cleared"""
        self.clean_ptr = buf.data_ptr()
        self.dirty, self.layout = False, abi.GRAD_ANY

    def overwritten(self) -> None:
        """a backward of the ordinary path is about to un-pack ANOTHER gradient layout through the region"""
        if self.dirty:
            raise VoxeError("deferred-gradient mode: a render with another gradient layout would overwrite the "
                            "accumulated gradient")
        self.clean_ptr = 0


# what the last recon_step_ handed the library: its descriptors (the next call of the same loop copies them) and its buffers
ReconRecord = namedtuple("ReconRecord", "key grid cfg step ws ws2 scratch")


class ReconLoop:
    """Python state of the fused iterations (recon_step_ / recon_prefetch_, attn_refine_step_) that run in one workspace"""

    def __init__(self):
        self.last: Optional[ReconRecord] = None   # of the last recon_step_ (what a hint for the next one repeats)
        self.buffers = {}                         # name -> device scratch of the fused iterations
        self.keepalive = None                     # what the library's side stream reads until the next step is enqueued

    def scratch(self, name: str, numel: int, dtype, device, hinted: Optional["Workspace"] = None) -> torch.Tensor:
        """the scratch tensor `name`, at least `numel` x `dtype` on `device`, grown on demand (`hinted`: a workspace whose hint uses it)"""
        buf = self.buffers.get(name)
        if buf is None or buf.numel() < numel or buf.dtype != dtype or buf.device != torch.device(device):
            if buf is not None and hinted is not None and hinted.hint_inflight:
                torch.cuda.synchronize(buf.device)     # (the side stream of `hinted`'s hint may still be writing the old buffer)
                hinted.hint_inflight = False
            buf = self.buffers[name] = torch.empty(numel, dtype=dtype, device=device)
        return buf

    def descriptors(self, key, buf, buf2, poses, image_rows, rng):
        """(g, c, rs, ws, ws2, sc) of the last recon_step_ -- copies of its descriptors with this call's cameras and streams, its
        buffers -- when that step ran the same loop (`key`: grid, images, batch; the cameras' shape; the two workspaces' buffers
        `buf` / `buf2` still in place), else None: the full marshalling is then the step's business, and a hint announces nothing"""
        last = self.last
        if not (last is not None and last.key == key and last.ws is buf and last.ws2 is buf2):
            return None
        K = last.step.K      # (the cameras: another K, dtype or layout than the descriptors were built for)
        if not (poses.is_cuda and poses.dtype == torch.float32 and poses.is_contiguous() and tuple(poses.shape) == (K, 3, 4)
                and (image_rows is None or (image_rows.is_cuda and image_rows.dtype == torch.int64 and image_rows.numel() == K))):
            return None
        c, rs = type(last.cfg).from_buffer_copy(last.cfg), type(last.step).from_buffer_copy(last.step)
        c.seed, c.rng_offset = int(rng[0]) & 0xFFFFFFFFFFFFFFFF, int(rng[1]) & 0xFFFFFFFFFFFFFFFF
        rs.poses, rs.image_rows = ptr(poses), ptr(image_rows)
        return last.grid, c, rs, last.ws, last.ws2, last.scratch

    def hint_issued(self, workspace: "Workspace", workspace2: "Workspace", keepalive) -> None:
        """until the next step is enqueued the library's side stream may be writing both buffers and reading `keepalive`"""
        workspace.hint_inflight = workspace2.hint_inflight = True
        self.keepalive = keepalive

    def step_enqueued(self, workspace: "Workspace", workspace2: "Workspace", record: ReconRecord) -> None:
        """(the step waited for the side stream, hint taken or not)"""
        workspace.hint_inflight = workspace2.hint_inflight = False
        self.last, self.keepalive = record, None


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
        self.recon = ReconLoop()
        self.hint_inflight = False      # set and cleared by ReconLoop.hint_issued / step_enqueued on both workspaces of the pair

    def __del__(self):
        # a hint in flight (recon_prefetch_) writes this buffer from a stream torch's caching allocator knows nothing about
        try:
            if self.hint_inflight and self.buf is not None:
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
        sibling = self.partner()
        if sibling.pending and version is not None and sibling.pending_version != version:
            sibling.pending = False
        return sibling if not sibling.pending else self

    def partner(self) -> "Workspace":
        """the second workspace of this one (own buffers), created on first use"""
        if self.sibling is None:
            self.sibling = Workspace()
        return self.sibling

    def forward_pending(self, version) -> None:
        """a differentiable forward of the parameters at `version` left its ray states here for its backward"""
        self.pending, self.pending_version = True, version

    def backward_ran(self) -> None:
        self.pending = False

    def attach_deferred(self, want_densities: bool, want_features: bool) -> DeferredGrad:
        if self.deferred is not None:
            raise RuntimeError("FusedGridAdam: this grid is already in deferred-gradient mode (another FusedGridAdam is "
                               "attached to it); detach() that optimiser first")
        self.deferred = DeferredGrad(want_densities=want_densities, want_features=want_features)
        return self.deferred

    def detach_deferred(self, mine: Optional[DeferredGrad] = None) -> bool:
        """leave the deferred-gradient mode (`mine`, the finalizer: only while it is still that optimiser's) -> an unconsumed gradient
        stays behind.  It must not leak into a later fused step: its region is unknown to whoever attaches next, and detach(), which
        unlike the finalizer may run a kernel, zeroes it as well"""
        d = self.deferred
        if d is None or (mine is not None and d is not mine):
            return False
        if d.dirty:
            self.call_failed()
        self.deferred = None
        return d.dirty

    def call_failed(self) -> None:
        """a fused call may have failed BEHIND its first backward: the gradient region then holds a partial gradient and the
        packed grid may be stale -- the next call must clear / re-pack first"""
        if self.deferred is not None:
            self.deferred.clean_ptr = 0
        self.invalidate()

    def before_call(self, spec, densities, features, nbytes: int, device):
        """THE question before a library call on the grid `densities` / `features` (the caller's SOURCE tensors, see `holds`):
        -> (buffer of at least `nbytes`, reuse_packed_grid, fresh, pack key).  `fresh`: this call allocated the buffer, its gradient
        region holds whatever torch.empty returned.  The pack key is taken before a regrow can clear the workspace's own: a
        backward builds from it the _state_key it then asks `holds_states` about."""
        had = self.buf
        key = _pack_key(spec, densities, features)
        buf = self.ensure(nbytes, device)
        return buf, int(self._holds_key(key)), buf is not had, key

    def after_call(self, spec, densities, features, states=UNTOUCHED) -> None:
        """THE statement after it: the buffer holds these (source) tensors' values packed for `spec`, and the ray states are
        UNTOUCHED, DROPPED (their region was reused, or rays were marched without keeping them) or those of the forward
        states = (params, rays_o, rays_d, jitter, rng, route) through the grid just remembered"""
        self.remember(spec, densities, features)
        if states is DROPPED:
            self.state_key = None
        elif states is not UNTOUCHED:
            params, rays_o, rays_d, jitter, rng, route = states
            self.remember_states(_state_key(self.key, params, rays_o, rays_d, jitter, rng, route), rays_o, rays_d, jitter)

    def forget_states(self) -> None:
        """the buffer no longer holds any forward's ray states; the packed grid stays"""
        self.state_key = None

    def forget_grid(self) -> None:
        """the buffer no longer holds a current grid (nor, then, ray states marched through it); the sibling keeps its own"""
        self.key = None
        self.state_key = None

    def invalidate(self):
        """forget what the buffer holds: the next call packs the grid and marches its rays again.  For writes that neither
        torch's version counters nor this module can see (`tensor.data`, another library's kernel, a DLPack view)."""
        self.forget_grid()
        if self.sibling is not None:
            self.sibling.invalidate()

    def ensure(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            old = self.buf
            if old is not None and self.hint_inflight:
                torch.cuda.synchronize(old.device)   # (a stream torch's allocator knows nothing about is still using the old buffer)
                self.hint_inflight = False
            self.recon.last = None                   # (its descriptors point into the old buffer -- and would keep it alive)
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

    def holds(self, spec, densities: torch.Tensor, features: torch.Tensor) -> bool:
        """THE decision "skip the pack pass": does the buffer hold the values of these grid tensors, packed for `spec`?
        `densities` / `features` are the caller's tensors, BEFORE any conversion to dense float32 (the converted copy is a
        temporary whose address and version say nothing about the source)."""
        return self._holds_key(_pack_key(spec, densities, features))

    def _holds_key(self, key) -> bool:
        if self.key is None:
            return False
        if not _alive(self._sources):
            self.key = self.state_key = None
            return False
        return self.key == key

    def remember(self, spec, densities: torch.Tensor, features: torch.Tensor) -> None:
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


def wrote(*tensors) -> None:
    """the library wrote these tensors (None: skipped) through raw pointers: tell autograd -- and the packed-grid caches, which are
    keyed on Tensor._version -- that they changed in place"""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


def _storage_ref(t: torch.Tensor):
    return weakref.ref(t.untyped_storage())


def _alive(refs) -> bool:
    for r in refs:
        if r() is None:
            return False
    return True


def _pack_key(spec, densities: torch.Tensor, features: torch.Tensor):
    """which values a packed grid holds -- of the caller's tensors as they are (any dtype, any strides).  Complete only together
    with Workspace._sources: equal addresses and versions mean equal values while the storages behind them are alive.
    (density_post_act is applied per sample, not by the pack: not part of the key.)"""
    return (densities.data_ptr(), densities._version, features.data_ptr(), features._version,
            tuple(features.shape), spec.density_scale, spec.density_pre_act, spec.feature_kind,
            densities.dtype, densities.stride(), features.dtype, features.stride())


_forward_fields = {}   # type of the params -> getter of the values a forward depends on


def _state_key(pack_key, params, rays_o, rays_d, jitter, rng, route=None):
    """identity of a forward call: the backward may consume the ray states only of exactly this call -- and only when it
    resolves to the same kernels (`route` = voxe_render_route, asked by the caller: ray-ordered and space-binned renders keep
    different tables, and the choice also depends on process-level tuning switches that may change between the two calls)"""
    get = _forward_fields.get(type(params))
    if get is None:   # (every field but the backward-only knobs and the dispatch, which is resolved below)
        names = [k for k in vars(params) if k not in ("linear_grad", "deterministic", "dispatch")]
        get = _forward_fields[type(params)] = attrgetter(*names)
    fwd = get(params) + (params.dispatch if params.dispatch is not None else _dispatch.current(),)
    # (the rays' and the jitter's version counters too: the trainers reuse their ray buffers, rewriting them in place)
    return (pack_key, fwd, rays_o.data_ptr(), rays_o._version, rays_d.data_ptr(), rays_d._version, rays_o.shape[0],
            None if jitter is None else (jitter.data_ptr(), jitter._version), tuple(rng), route)


_scratch = {}   # device scratch of the whole-grid passes: one buffer per (device, stream), grown on demand


def _scratch_for(device, nbytes: int) -> torch.Tensor:
    key = (torch.device(device).index, torch.cuda.current_stream(device).cuda_stream)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
        _scratch[key] = buf
    return buf
