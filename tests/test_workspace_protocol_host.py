"""The two operations every workspace-using entry point of voxe_hip.ops is built from -- `Workspace.before_call` (size the buffer,
decide reuse_packed_grid and ray_state_valid) and `Workspace.after_call` (what the buffer holds now) -- with `forget_states`,
`forget_grid` and the announcement of tensors the library wrote.  Driven directly with CPU tensors, as
tests/test_cache_keys_host.py drives the pieces underneath; the grids are those of tests/cache_cases.py."""
import torch

import cache_cases as cc
from voxe_hip import ops
from voxe_hip.workspace import DROPPED, UNTOUCHED, DeferredGrad, wrote

PARAMS = ops.RenderParams(num_samples=6, near=1.0, far=4.0, perturb=True)
NBYTES = 4096


def _rays(R=50):
    g = torch.Generator().manual_seed(3)
    return {"rays_o": cc.host_tensor(torch.rand((R, 3), generator=g)), "rays_d": cc.host_tensor(torch.rand((R, 3), generator=g)),
            "jitter": cc.host_tensor(torch.rand((R, PARAMS.num_samples), generator=g))}


RNG, ROUTE = (4, 2), 0


def _before(ws, o, r=None, nbytes=NBYTES):
    """(buffer, reuse_packed_grid, ray_state_valid, fresh) as a backward entry point decides them: the state key of the forward on
    the rays `r` is built from the pack key `before_call` took before it could regrow the buffer"""
    buf, reuse, fresh, key = ws.before_call(o.spec, o.densities, o.features, nbytes, "cpu")
    assert key == ops._pack_key(o.spec, o.densities, o.features)
    valid = r is not None and ws.holds_states(ops._state_key(key, PARAMS, r["rays_o"], r["rays_d"], r["jitter"], RNG, ROUTE))
    return buf, reuse, int(valid), fresh


def _after(ws, o, r=None, states=UNTOUCHED):
    if r is not None:
        states = (PARAMS, r["rays_o"], r["rays_d"], r["jitter"], RNG, ROUTE)
    ws.after_call(o.spec, o.densities, o.features, states)


def test_first_call_repacks_and_the_same_grid_is_reused():
    o, r, ws = cc.make_owner("sh0"), _rays(), ops.Workspace()
    buf, reuse, valid, fresh = _before(ws, o, r)
    assert (reuse, valid, fresh) == (0, 0, True) and buf is ws.buf and buf.numel() >= NBYTES
    _after(ws, o)
    buf2, reuse, valid, fresh = _before(ws, o, r)
    assert buf2 is buf and (reuse, valid, fresh) == (1, 0, False)           # the grid is held; nobody left ray states
    assert _before(ws, o)[1:] == (1, 0, False)                             # (no state key: no claim)
    cc.BY_NAME["add_"].apply(o)
    assert _before(ws, o, r)[1:] == (0, 0, False)


def test_kept_states_are_valid_for_exactly_that_forward():
    o, r, ws = cc.make_owner("sh0"), _rays(), ops.Workspace()
    _before(ws, o)
    _after(ws, o, r)
    assert _before(ws, o, r)[1:] == (1, 1, False)
    assert _before(ws, o, _rays(R=51))[1:] == (1, 0, False)
    # the kept key is built on the pack key `after_call` has just taken, with the route the caller asked
    assert ws.state_key == ops._state_key(ws.key, PARAMS, r["rays_o"], r["rays_d"], r["jitter"], RNG, ROUTE)
    ws.after_call(o.spec, o.densities, o.features, (PARAMS, r["rays_o"], r["rays_d"], r["jitter"], RNG, ROUTE + 1))
    assert _before(ws, o, r)[1:] == (1, 0, False)          # (the same rays through other kernels: another forward)
    _after(ws, o, r)
    # a call that says nothing about the states leaves them; one that dropped them ends the claim and nothing else
    _after(ws, o)
    assert _before(ws, o, r)[1:] == (1, 1, False)
    _after(ws, o, states=DROPPED)
    assert _before(ws, o, r)[1:] == (1, 0, False)


def test_forget_states_ends_only_the_state_claim_and_forget_grid_both():
    o, r, ws = cc.make_owner("sh0"), _rays(), ops.Workspace()
    _before(ws, o)
    _after(ws, o, r)
    ws.forget_states()
    assert ws.state_key is None and ws.key is not None
    assert _before(ws, o, r)[1:] == (1, 0, False)
    _after(ws, o, r)
    ws.forget_grid()
    assert ws.key is None and ws.state_key is None
    assert _before(ws, o, r)[1:] == (0, 0, False)
    # forget_grid is this workspace's alone; invalidate() reaches the sibling
    _after(ws, o, r)
    ws.pending, ws.pending_version = True, (0, 0)
    sib = ws.for_differentiable_forward((0, 0))
    _before(sib, o)
    _after(sib, o, r)
    ws.forget_grid()
    assert _before(sib, o, r)[1:] == (1, 1, False)
    ws.invalidate()
    assert _before(sib, o, r)[1:] == (0, 0, False) and _before(ws, o)[1:] == (0, 0, False)


def test_regrow_reports_a_new_buffer_and_drops_both_keys():
    o, r, ws = cc.make_owner("sh0"), _rays(), ops.Workspace()
    old = _before(ws, o)[0]
    _after(ws, o, r)
    ws.recon_cache = ("descriptors into the old buffer",)
    buf, reuse, valid, fresh = _before(ws, o, r, nbytes=2 * NBYTES)
    assert buf is not old and buf is ws.buf and buf.numel() >= 2 * NBYTES
    assert (reuse, valid, fresh) == (0, 0, True)
    assert ws.key is None and ws.state_key is None and ws.recon_cache is None
    # a smaller request keeps the buffer
    _after(ws, o, r)
    assert _before(ws, o, r, nbytes=NBYTES) == (buf, 1, 1, False)


def test_regrow_with_a_deferred_gradient_keeps_the_grid_key():
    """deferred-gradient mode with an accumulated gradient: the packed grid and the gradient are copied into the new buffer (on the
    device; here the key logic alone), so the grid is still held -- the ray states are not -- and `clean_ptr` follows the buffer"""
    o, r, ws = cc.make_owner("sh0"), _rays(), ops.Workspace()
    old = _before(ws, o)[0]
    _after(ws, o, r)
    ws.deferred = DeferredGrad(dirty=True, clean_ptr=old.data_ptr())
    key = ws.key
    buf, reuse, valid, fresh = _before(ws, o, r, nbytes=2 * NBYTES)
    assert buf is not old and fresh
    assert (reuse, valid) == (1, 0) and ws.key == key and ws.state_key is None
    assert ws.deferred.clean_ptr == buf.data_ptr()
    # not dirty: nothing to keep
    ws.deferred.dirty = False
    assert _before(ws, o, nbytes=4 * NBYTES)[1:] == (0, 0, True) and ws.key is None


def test_wrote_bumps_exactly_the_tensors_given():
    a, b, c = torch.zeros(3), torch.zeros(3), torch.zeros(3)
    versions = (a._version, b._version, c._version)
    wrote(a, None, b)
    assert (a._version, b._version, c._version) == (versions[0] + 1, versions[1] + 1, versions[2])
    wrote()
    wrote(None)
    assert (a._version, b._version, c._version) == (versions[0] + 1, versions[1] + 1, versions[2])
    # ... which is what ends a pack claim on a tensor the library wrote through its raw pointer
    o, ws = cc.make_owner("sh0"), ops.Workspace()
    _before(ws, o)
    _after(ws, o)
    wrote(o.features)
    assert _before(ws, o)[1] == 0
