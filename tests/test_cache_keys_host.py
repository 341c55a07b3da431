"""What the binding decides about its two caches -- the packed grid (`Workspace.holds`) and the forward's ray states
(`Workspace.holds_states`) -- for every way a grid or a ray batch can change between two calls through one workspace
(tests/cache_cases.py).  Plain Python over data_ptr / _version / storage lifetimes: CPU tensors, no GPU.  The call sites of
voxe_hip.ops ask the same two functions, so what is decided here is what the kernels are told
(tests/test_cache_coherence_gpu.py checks the values that then reach them).

A false hit raises nothing: the kernels would run correctly on the previous grid.  Every row therefore first shows the HIT on the
unchanged grid (a cache that never hits would pass everything else) and then the miss after the change."""
import pytest
import torch

import cache_cases as cc
from voxe_hip import abi, ops


def _remember(ws, o):
    ws.remember(o.spec, o.densities, o.features)


def _holds(ws, o):
    return ws.holds(o.spec, o.densities, o.features)


@pytest.mark.parametrize("name,kind", cc.rows())
def test_change_forces_a_repack(name, kind):
    change = cc.BY_NAME[name]
    o = cc.make_owner(kind, change.source)
    ws = ops.Workspace()
    assert not _holds(ws, o)                               # nothing packed yet
    _remember(ws, o)
    assert _holds(ws, o) and _holds(ws, o)                 # the unchanged grid hits, as often as it is asked
    change.apply(o)
    assert _holds(ws, o) == (not change.repack), name
    # a call that packed the new values makes them the held ones
    _remember(ws, o)
    assert _holds(ws, o)


@pytest.mark.parametrize("source", ["f64", "f16", "permuted"])
@pytest.mark.parametrize("which", ["densities", "features"])
def test_converted_source_is_keyed_on_the_source_not_on_the_temporary(source, which):
    """the dense float32 copy a call makes of a float64 / float16 / permuted tensor is a temporary: a storage of its own, version 0
    whatever happened to the source, freed when the call returns (that the next call's copy then lands on the same address is the
    caching allocator's doing: tests/test_cache_coherence_gpu.py asserts it where it happens; the host's malloc does it in some
    process states and not in others).  The key of the source sees the change -- and a source that did not change still hits,
    although every call converts it again."""
    from voxe_hip.runtime import f32c

    o = cc.make_owner("sh0", source)
    t = getattr(o, which)
    ws = ops.Workspace()
    _remember(ws, o)
    assert _holds(ws, o)
    with torch.no_grad():
        t.add_(0.5)
    copy = f32c(t.detach())
    assert copy.untyped_storage().data_ptr() != t.untyped_storage().data_ptr() and copy._version == 0 and t._version > 0
    assert not _holds(ws, o)
    _remember(ws, o)
    del copy
    assert _holds(ws, o)


def test_the_same_storage_under_another_handle_still_hits():
    """no over-invalidation: `detach()` (what every autograd entry point does to its inputs), a Parameter wrapped around the
    tensor and the tensors autograd saved for a backward are new Python objects over the same storage and version counter"""
    o = cc.make_owner("sh0")
    ws = ops.Workspace()
    _remember(ws, o)
    assert ws.holds(o.spec, o.densities.detach(), o.features.detach())
    assert ws.holds(o.spec, torch.nn.Parameter(o.densities.detach()), o.features)
    assert _holds(ws, o)


def test_dead_source_ends_both_keys_and_invalidate_reaches_the_sibling():
    o = cc.make_owner("sh0")
    ws = ops.Workspace()
    _remember(ws, o)
    rays = _rays()
    ws.remember_states(_state_key(ws, rays), rays["rays_o"], rays["rays_d"], rays["jitter"])
    assert ws.holds_states(_state_key(ws, rays))
    key = ws.key
    del o._features
    assert ws.key == key                                   # (nothing ran yet: the keys end when they are asked)
    assert not ws.holds_states(_state_key(ws, rays)) and ws.state_key is None
    o = cc.make_owner("sh0")
    assert not _holds(ws, o) and ws.key is None
    # invalidate(): the sibling a second differentiable forward ran in is a cache of the same grid
    _remember(ws, o)
    ws.forward_pending((0, 0))
    sib = ws.for_differentiable_forward((0, 0))
    assert sib is ws.sibling and sib is not ws
    _remember(sib, o)
    ws.invalidate()
    assert not _holds(ws, o) and not _holds(sib, o)


# ---- rays and jitter ------------------------------------------------------------------------------------------------------------
PARAMS = ops.RenderParams(num_samples=6, near=1.0, far=4.0, perturb=True)


def _rays(R=50):
    g = torch.Generator().manual_seed(3)
    return {"rays_o": cc.host_tensor(torch.rand((R, 3), generator=g)), "rays_d": cc.host_tensor(torch.rand((R, 3), generator=g)),
            "jitter": cc.host_tensor(torch.rand((R, PARAMS.num_samples), generator=g))}


def _state_key(ws, r):
    return ops._state_key(ws.key, PARAMS, r["rays_o"], r["rays_d"], r["jitter"], (4, 2), 0)


@pytest.mark.parametrize("name", sorted(cc.RAY_CHANGES))
def test_ray_change_ends_the_state_claim(name):
    o = cc.make_owner("sh0")
    ws = ops.Workspace()
    _remember(ws, o)
    r = _rays()
    assert not ws.holds_states(_state_key(ws, r))
    ws.remember_states(_state_key(ws, r), r["rays_o"], r["rays_d"], r["jitter"])
    assert ws.holds_states(_state_key(ws, r)) and ws.holds_states(_state_key(ws, r))
    cc.RAY_CHANGES[name](r)
    assert not ws.holds_states(_state_key(ws, r)), name


def test_state_claim_ends_with_the_grid_and_survives_saved_tensor_handles():
    o = cc.make_owner("sh0")
    ws = ops.Workspace()
    _remember(ws, o)
    r = _rays()
    ws.remember_states(_state_key(ws, r), r["rays_o"], r["rays_d"], r["jitter"])
    # the backward sees the rays as autograd unpacked them: other Python objects over the same storages
    alias = {k: v.detach() for k, v in r.items()}
    assert ws.holds_states(_state_key(ws, alias))
    with torch.no_grad():
        o.densities.add_(0.5)
    assert not _holds(ws, o)
    _remember(ws, o)                                       # a call packed the new grid: the states were marched through the old one
    assert not ws.holds_states(_state_key(ws, r))


# ---- VoxelGrid: the setters tell the workspaces; what bypasses them is caught by the workspaces themselves --------------------------
def _voxel_grid(kind="sh0"):
    return cc.make_voxel_grid(kind)


def _grid_tensors(grid, tag):
    if tag in ("sh", "query"):
        return grid.voxe_grid_spec(attn=False), grid.densities, grid.features
    return grid.voxe_grid_spec(attn=True), grid.densities, grid.attn


TAGS = ("sh", "attn", "query", "query_attn")


def _remember_all(grid):
    for tag in TAGS:
        grid.voxe_workspace(tag).remember(*_grid_tensors(grid, tag))
        assert grid.voxe_workspace(tag).holds(*_grid_tensors(grid, tag))


@pytest.mark.parametrize("name", [n for n, k in cc.rows(grid_only=True) if k == "sh0" and cc.BY_NAME[n].source == "f32"])
def test_change_on_a_voxel_grid_reaches_every_workspace_that_held_the_tensor(name):
    grid = _voxel_grid()
    _remember_all(grid)
    cc.BY_NAME[name].apply(grid)
    changed_densities = name != "del_then_fresh_features"
    for tag in TAGS:
        if changed_densities or tag in ("sh", "query"):
            assert not grid.voxe_workspace(tag).holds(*_grid_tensors(grid, tag)), (name, tag)


def test_add_attn_params_twice_at_one_address():
    grid = _voxel_grid()
    _remember_all(grid)
    ptr, version = grid.attn.data_ptr(), grid.attn._version
    grid.add_attn_params(grid.attn.detach() + 0.25)
    first = grid.attn.detach()
    grid.add_attn_params(cc.alloc_at(ptr, lambda: first + 0.25))
    assert (grid.attn.data_ptr(), grid.attn._version) == (ptr, version), "hazard not built"
    for tag in ("attn", "query_attn"):
        assert not grid.voxe_workspace(tag).holds(*_grid_tensors(grid, tag)), tag


def test_update_orig_densities_tells_the_workspaces():
    """forward_attn(orig_densities=True) reads a snapshot that update_orig_densities() REPLACES by a fresh clone (version 0 like
    every clone, and on the device soon at the address of the one before last: tests/test_cache_coherence_gpu.py)"""
    grid = _voxel_grid()
    spec = grid.voxe_grid_spec(attn=True)
    ws = grid.voxe_workspace("query_attn")
    ws.remember(spec, grid.orig_densities, grid.attn)
    assert ws.holds(spec, grid.orig_densities.detach(), grid.attn)
    with torch.no_grad():
        grid.densities.add_(0.5)
    assert ws.holds(spec, grid.orig_densities.detach(), grid.attn)          # the snapshot did not move
    grid.update_orig_densities()
    assert not ws.holds(spec, grid.orig_densities.detach(), grid.attn)


def test_invalidate_voxe_caches_is_the_remedy_for_writes_torch_cannot_see():
    """`.data` hands out a tensor with a version counter of its own: the write below is invisible by construction (the contract
    INTEGRATION.md states), and VoxelGrid.invalidate_voxe_caches() is what the caller then owes"""
    grid = _voxel_grid()
    _remember_all(grid)
    before = grid.densities._version
    grid.densities.data.add_(1.0)
    assert grid.densities._version == before
    assert all(grid.voxe_workspace(tag).holds(*_grid_tensors(grid, tag)) for tag in TAGS)      # undetectable
    grid.invalidate_voxe_caches()
    assert not any(grid.voxe_workspace(tag).holds(*_grid_tensors(grid, tag)) for tag in TAGS)


def test_pack_key_names_what_the_pack_reads():
    o = cc.make_owner("sh0")
    base = ops._pack_key(o.spec, o.densities, o.features)
    import dataclasses

    for field, value in (("density_scale", 1.0), ("density_pre_act", abi.ACT_ABS), ("feature_kind", abi.FEAT_ATTN)):
        assert ops._pack_key(dataclasses.replace(o.spec, **{field: value}), o.densities, o.features) != base, field
    # (applied per sample, not by the pack; tests/test_cache_coherence_gpu.py renders it)
    assert ops._pack_key(dataclasses.replace(o.spec, density_post_act=abi.ACT_RELU), o.densities, o.features) == base
    # one storage under other strides or another dtype holds other values
    sq = torch.zeros((4, 4, 4, 1))
    assert ops._pack_key(o.spec, sq, sq) != ops._pack_key(o.spec, sq.permute(1, 0, 2, 3), sq)
    assert ops._pack_key(o.spec, sq, sq) != ops._pack_key(o.spec, sq.view(torch.int32), sq)
