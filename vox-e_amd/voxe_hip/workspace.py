"""The caller-owned workspace of the render, query and fused-step entry points and the protocol of its two caches: "the buffer still
holds this grid packed" (VoxeRenderCfg::reuse_packed_grid) and "it still holds this forward's ray states" (::ray_state_valid).
Plain Python over tensors: no library call is made here.  An entry point of voxe_hip.ops prepares its arguments, asks
`Workspace.before_call`, calls the library and tells `Workspace.after_call`."""
import weakref
from dataclasses import dataclass
from operator import attrgetter
from typing import Optional

import torch

from . import abi
from . import dispatch as _dispatch

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
