"""Which library calls each workspace-using entry point of voxe_hip.ops makes, in which order, and what it tells the kernels about the
two caches (VoxeRenderCfg::reuse_packed_grid, ::ray_state_valid).  The expected traces are literals recorded from the binding as it
was BEFORE the workspace protocol moved into voxe_hip/workspace.py: the same calls, no extra size or route queries, the same flags.

Shapes: the 20 x 24 x 28 grids of tests/cache_cases.py, the 32 x 40 ray batch (S = 48) of tests/test_cache_coherence_gpu.py; the
fused reconstruction iteration on 4 views of 24 x 32 pixels with a batch of 512."""
import dataclasses

import pytest
import torch

import cache_cases as cc
from synth import FAR, NEAR, RADIUS, focal_for, synth_pose_angles
from voxe_hip import abi

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import gpu_helpers as gh
    import test_cache_coherence_gpu as tcc
    from thre3d_atom.utils.imaging_utils import pose_spherical
    from voxe_hip import ops

    DEV = gh.DEV


class _LibSpy:
    """voxe_hip.ops.lib() recording every voxe_* entry that is fetched and called: (name,), or (name, reuse_packed_grid,
    ray_state_valid) where the second argument is a VoxeRenderCfg by reference"""

    def __init__(self, real):
        self._real, self.trace = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("voxe_"):
            return fn

        def spy(*args):
            cfg = getattr(args[1], "_obj", None) if len(args) > 1 else None
            if isinstance(cfg, abi.VoxeRenderCfg):
                self.trace.append((name, int(cfg.reuse_packed_grid), int(cfg.ray_state_valid)))
            else:
                self.trace.append((name,))
            return fn(*args)
        return spy


@pytest.fixture
def spy(monkeypatch):
    s = _LibSpy(ops.lib())
    monkeypatch.setattr(ops, "lib", lambda: s)
    return s


def _adam_state(t):
    return (torch.zeros_like(t), torch.zeros_like(t))


def _check(spy, name):
    torch.cuda.synchronize()
    assert spy.trace == EXPECTED[name], name


def test_raw_entry_points_on_one_workspace(spy):
    """render_fwd_into -> render_bwd_into -> render_bwd_acc -> grid_adam_step_ -> render_fwd_into"""
    o = cc.make_owner("sh0", "f32", DEV)
    r, p, ws = tcc._rays(), tcc._params(o), ops.Workspace()
    dens, feat = o.densities.detach(), o.features.detach()
    gc_, gd_, ga_ = tcc._upstream(3)
    outs = tcc._outs(o)
    rays = (r["rays_o"], r["rays_d"], r["jitter"])
    ops.render_fwd_into(o.spec, p, dens, feat, *rays, *outs, ws, tcc.RNG)
    dd, df = torch.empty_like(dens), torch.empty_like(feat)
    ops.render_bwd_into(o.spec, p, dens, feat, *rays, outs[0], outs[1], outs[2], gc_, gd_, ga_, dd, df, ws, tcc.RNG)
    layout = ops.render_bwd_acc(o.spec, p, dens, feat, *rays, outs[0], outs[1], outs[2], gc_, gd_, ga_, ws, tcc.RNG, zero_first=True)
    ops.grid_adam_step_(o.spec, dens, feat, layout, ws, 1, 0.5, _adam_state(dens), _adam_state(feat))
    ops.render_fwd_into(o.spec, p, dens, feat, *rays, *outs, ws, tcc.RNG)
    _check(spy, "raw")


def test_autograd_render(spy):
    """ops.render with grad -> .backward()"""
    o = cc.make_owner("sh0", "f32", DEV)
    tcc._render_forward_backward(o, ops.Workspace(), tcc._rays())
    _check(spy, "render")


def test_query_then_render(spy):
    """query_points with grad -> .backward() -> render_fwd_into on the same workspace"""
    o = cc.make_owner("sh0", "f32", DEV)
    ws = ops.Workspace()
    tcc._query(o, ws)
    r = tcc._rays()
    ops.render_fwd_into(o.spec, tcc._params(o), o.densities.detach(), o.features.detach(), r["rays_o"], r["rays_d"], r["jitter"],
                        *tcc._outs(o), ws, tcc.RNG)
    _check(spy, "query")


def test_recon_steps_with_hints(spy):
    """three recon_step_ calls with a recon_prefetch_ after the first two: the second and third step take the cached-descriptor
    path"""
    o = cc.make_owner("sh0", "f32", DEV)
    K, h, w, batch = 4, 24, 32, 512
    poses = torch.stack([torch.cat([p.rotation, p.translation], dim=-1) for p in
                         (pose_spherical(*synth_pose_angles(i, 100), RADIUS) for i in (3, 38, 12, 58))]).float().to(DEV)
    images = torch.rand(K, 3, h, w, generator=torch.Generator().manual_seed(1)).to(DEV)
    d, f = o.densities.detach(), o.features.detach()
    st_d, st_f = _adam_state(d), _adam_state(f)
    losses = torch.zeros(4, device=DEV)
    p = ops.RenderParams(num_samples=tcc.S, near=NEAR, far=FAR, perturb=True, white_bkgd=True)
    wa, wb = ops.Workspace(), ops.Workspace()
    common = (o.spec, p, d, f, wa, wb, h, w, focal_for(w), poses, None, images, batch, True)
    for n in (1, 2, 3):
        cached = wa.recon.last
        ops.recon_step_(*common, st_d, st_f, n, n, 1e-2, losses, (11, 10 * n), zero_gradient_first=(n == 1))
        if n > 1:     # (the shortcut hands the library copies of the cached descriptors and keeps the buffers)
            assert cached is not None and wa.recon.last.ws is cached.ws and wa.recon.last.grid is cached.grid
        if n < 3:
            ops.recon_prefetch_(*common, losses, (11, 10 * (n + 1)))
    _check(spy, "recon")


def test_attn_refine_steps(spy):
    """attn_refine_step_ twice on one workspace"""
    a = cc.make_owner("attn", "f32", DEV)
    r = tcc._rays()
    amap = torch.rand(tcc.R, generator=torch.Generator().manual_seed(2)).to(DEV)
    attn = a.features.detach()
    p = dataclasses.replace(tcc._params(a), deterministic=False)        # (the fused iteration has no fixed-point mode)
    ws, state = ops.Workspace(), _adam_state(attn)
    for step in (1, 2):
        ops.attn_refine_step_(a.spec, p, a.densities.detach(), attn, r["rays_o"], r["rays_d"], amap, ws, step, 0.5, state, 0.01,
                              rng=tcc.RNG, zero_gradient_first=(step == 1))
    _check(spy, "attn_refine")


def test_visibility_buffers_that_are_not_the_grid_are_refused():
    """visibility_accumulate_ writes X * Y * Z floats through the raw pointer of each buffer: anything but [X,Y,Z] / [X,Y,Z,1]
    float32 on the grid's device is an error before any launch -- a buffer of fewer dimensions included"""
    from voxe_hip.runtime import VoxeError

    o, r = cc.make_owner("sh0", "f32", DEV), tcc._rays()
    X, Y, Z = cc.DIMS
    p = ops.RenderParams(num_samples=tcc.S, near=NEAR, far=FAR)
    for shape in ((X, Y), (X,), (), (X, Y, Z - 1), (X, Y, Z, 2), (X * Y * Z,), (1, X, Y, Z)):
        for which in ("max_weight", "max_trans"):
            with pytest.raises(VoxeError, match=which):
                ops.visibility_accumulate_(o.spec, p, o.densities.detach(), r["rays_o"], r["rays_d"],
                                           **{which: torch.zeros(shape, device=DEV)})
    for shape in ((X, Y, Z), (X, Y, Z, 1)):
        mw = torch.zeros(shape, device=DEV)
        ops.visibility_accumulate_(o.spec, p, o.densities.detach(), r["rays_o"], r["rays_d"], max_weight=mw)
        assert float(mw.max()) > 0
    torch.cuda.synchronize()


# recorded by running this file against the binding before the refactor (the commit before this file's), then pasted
EXPECTED = {
    "raw": [
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_tile_plan_bytes', 0, 0),
        ('voxe_render_fwd', 0, 0),
        ('voxe_render_route', 0, 0),
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_tile_plan_bytes', 0, 0),
        ('voxe_render_route', 1, 0),
        ('voxe_render_bwd', 1, 1),
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_tile_plan_bytes', 0, 0),
        ('voxe_render_route', 1, 0),
        ('voxe_render_bwd_acc_into', 1, 1),
        ('voxe_grid_adam_step',),
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_tile_plan_bytes', 0, 0),
        ('voxe_render_fwd', 1, 0),
        ('voxe_render_route', 1, 0),
    ],
    "render": [
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_tile_plan_bytes', 0, 0),
        ('voxe_render_fwd', 0, 0),
        ('voxe_render_route', 0, 0),
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_tile_plan_bytes', 0, 0),
        ('voxe_render_route', 1, 0),
        ('voxe_render_bwd', 1, 1),
    ],
    "query": [
        ('voxe_workspace_bytes',),
        ('voxe_query_fwd',),
        ('voxe_workspace_bytes',),
        ('voxe_query_bwd',),
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_tile_plan_bytes', 0, 0),
        ('voxe_render_fwd', 0, 0),
        ('voxe_render_route', 0, 0),
    ],
    "recon": [
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_recon_scratch_bytes',),
        ('voxe_recon_step', 0, 0),
        ('voxe_recon_prefetch', 0, 0),
        ('voxe_recon_step', 1, 0),
        ('voxe_recon_prefetch', 1, 0),
        ('voxe_recon_step', 1, 0),
    ],
    "attn_refine": [
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_tile_plan_bytes', 0, 0),
        ('voxe_attn_refine_scratch_bytes',),
        ('voxe_attn_refine_step', 0, 0),
        ('voxe_workspace_bytes', 0, 0),
        ('voxe_tile_plan_bytes', 0, 0),
        ('voxe_attn_refine_scratch_bytes',),
        ('voxe_attn_refine_step', 1, 0),
    ],
}
