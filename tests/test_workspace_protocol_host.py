"""The two operations every workspace-using entry point of voxe_hip.ops is built from -- `Workspace.before_call` (size the buffer,
decide reuse_packed_grid and ray_state_valid) and `Workspace.after_call` (what the buffer holds now) -- with `forget_states`,
`forget_grid` and the announcement of tensors the library wrote.  Driven directly with CPU tensors, as
tests/test_cache_keys_host.py drives the pieces underneath; the grids are those of tests/cache_cases.py."""
import pytest
import torch

import cache_cases as cc
from voxe_hip import abi, ops
from voxe_hip.runtime import VoxeError
from voxe_hip.workspace import DROPPED, UNTOUCHED, ReconRecord, wrote

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
    ws.forward_pending((0, 0))
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
    ws.recon.step_enqueued(ws, ops.Workspace(), ReconRecord("descriptors into the old buffer", None, None, None, old, None, None))
    assert ws.recon.last.ws is old
    buf, reuse, valid, fresh = _before(ws, o, r, nbytes=2 * NBYTES)
    assert buf is not old and buf is ws.buf and buf.numel() >= 2 * NBYTES
    assert (reuse, valid, fresh) == (0, 0, True)
    assert ws.key is None and ws.state_key is None and ws.recon.last is None
    # a smaller request keeps the buffer
    _after(ws, o, r)
    assert _before(ws, o, r, nbytes=NBYTES) == (buf, 1, 1, False)


def test_regrow_with_a_deferred_gradient_keeps_the_grid_key():
    """deferred-gradient mode with an accumulated gradient: the packed grid and the gradient are copied into the new buffer (on the
    device; here the key logic alone), so the grid is still held -- the ray states are not -- and the known region follows the buffer"""
    o, r, ws = cc.make_owner("sh0"), _rays(), ops.Workspace()
    old = _before(ws, o)[0]
    _after(ws, o, r)
    ws.attach_deferred(True, True).accumulated(old, abi.GRAD_LINEAR)
    key = ws.key
    buf, reuse, valid, fresh = _before(ws, o, r, nbytes=2 * NBYTES)
    assert buf is not old and fresh
    assert (reuse, valid) == (1, 0) and ws.key == key and ws.state_key is None
    assert not ws.deferred.must_clear(buf) and ws.deferred.dirty
    # not dirty: nothing to keep
    ws.deferred.consumed(buf)
    assert _before(ws, o, nbytes=4 * NBYTES)[1:] == (0, 0, True) and ws.key is None


def test_deferred_gradient_state_machine_through_every_transition():
    """attach -> accumulate -> step -> failed call -> overwritten region -> second attach -> release: after each transition the
    three questions the entry points ask (clear first? which layout must the next render write? is a gradient waiting?)"""
    o, ws = cc.make_owner("sh0"), ops.Workspace()
    buf = _before(ws, o)[0]
    _after(ws, o)
    d = ws.attach_deferred(True, False)

    def state(b=buf):
        return d.must_clear(b), d.expected_layout(), d.dirty

    assert ws.deferred is d and (d.want_densities, d.want_features) == (True, False)
    assert state(None) == (True, abi.GRAD_ANY, False) and state() == (True, abi.GRAD_ANY, False)
    d.accumulated(buf, abi.GRAD_LINEAR)
    assert state() == (False, abi.GRAD_LINEAR, True) and state(None) == (False, abi.GRAD_LINEAR, True)
    d.consumed(buf)
    assert state() == (False, abi.GRAD_ANY, False) and state(None)[0] and state(torch.empty_like(buf))[0]
    ws.call_failed()                                       # ... the region holds a partial gradient, the packed grid may be stale
    assert state() == (True, abi.GRAD_ANY, False) and ws.key is None and ws.state_key is None
    d.accumulated(buf, abi.GRAD_ANY)                       # a backward without rays: cleared, nothing accumulated
    assert state() == (False, abi.GRAD_ANY, False)
    d.overwritten()                                        # clean: allowed, and the region is no longer known
    assert state() == (True, abi.GRAD_ANY, False)
    d.accumulated(buf, abi.GRAD_LINEAR)
    with pytest.raises(VoxeError, match="would overwrite the accumulated gradient"):
        d.overwritten()
    assert state() == (False, abi.GRAD_LINEAR, True)
    with pytest.raises(RuntimeError, match="already in deferred-gradient mode"):
        ws.attach_deferred(True, True)
    assert ws.deferred is d
    # the finalizer's release: of its own mode only; a dirty region is unknown to whoever attaches next, the grid is re-packed
    _after(ws, o)
    assert not ws.detach_deferred(mine=ops.DeferredGrad()) and ws.deferred is d and ws.key is not None
    assert ws.detach_deferred(mine=d) and ws.deferred is None and ws.key is None
    nxt = ws.attach_deferred(True, True)
    assert nxt is not d and nxt.must_clear(buf) and nxt.expected_layout() == abi.GRAD_ANY and not nxt.dirty
    nxt.consumed(buf)
    assert not ws.detach_deferred() and ws.deferred is None          # nothing accumulated: nothing left behind


def test_recon_scratch_grows_on_demand_and_names_do_not_alias():
    recon, cpu = ops.Workspace().recon, torch.device("cpu")
    a = recon.scratch("step", 100, torch.uint8, cpu)
    assert a.numel() >= 100 and a.dtype == torch.uint8
    assert recon.scratch("step", 100, torch.uint8, cpu) is a and recon.scratch("step", 40, torch.uint8, cpu) is a
    b = recon.scratch("step", 101, torch.uint8, cpu)
    assert b is not a and b.numel() >= 101 and recon.scratch("step", 100, torch.uint8, cpu) is b
    c = recon.scratch("refine", 101, torch.uint8, cpu)
    assert c is not b and c.data_ptr() != b.data_ptr() and recon.scratch("step", 101, torch.uint8, cpu) is b
    f = recon.scratch("refine_losses", 2, torch.float32, cpu)
    assert f.dtype == torch.float32 and f.numel() == 2 and recon.scratch("refine", 101, torch.uint8, cpu) is c


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
