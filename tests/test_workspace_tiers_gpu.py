"""Workspace tiers through the C ABI: what a render call does when the caller's `workspace_bytes` is the full size
(voxe_workspace_bytes with ray_state_valid = 0), the inference size (ray_state_valid = -1: packed grid, gradient, states and
segment partials -- none of the backward's optional buffers) or 256 bytes short of that.

The buffer handed over is always the large one; only the `workspace_bytes` argument shrinks, and the library checks every size
before it launches anything.  Tolerances are those of tests/test_hip_parity.py for the same routes (FWD_ATOL on colour / acc,
rtol 3e-6 on depth, GRAD_REL_L2 on gradients): the kernels of two tiers may differ, and atomics make gradients non-bitwise."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import rel_l2
from voxe_hip import abi

pytestmark = pytest.mark.gpu

FWD_ATOL = 5e-6        # tests/test_hip_parity.py
DEPTH_RTOL = 3e-6
GRAD_REL_L2 = 1e-4

DIMS = (24, 24, 24)
# name -> (sh_degree, image side or 0, rays, samples, expected route, depth segments expected > 1 (None: not read))
RENDERS = {
    "tile_segmented": (0, 96, 96 * 96, 64, abi.ROUTE_TILE, True),
    "tile_one_segment": (0, 96, 96 * 96, 16, abi.ROUTE_TILE, False),
    "tile_two_phase": (1, 96, 96 * 96, 64, abi.ROUTE_TILE, True),
    "region": (0, 0, 16384, 64, abi.ROUTE_REGION, None),
    "packed_scatter": (0, 0, 2048, 64, abi.ROUTE_PACKED_SCATTER, None),
}


def _rays(side, R, dev):
    from thre3d_atom.utils.imaging_utils import pose_spherical
    from voxe_hip import ops

    if side:
        pose = pose_spherical(40.0, 35.0, 4.0311)
        return ops.cast_rays(side, side, 0.5 * side / np.tan(0.5 * 0.6911112), pose.rotation, pose.translation, dev)
    gen = torch.Generator().manual_seed(7)
    o = torch.randn(R, 3, generator=gen)
    o = 4.0311 * o / o.norm(dim=1, keepdim=True)
    target = torch.empty(R, 3).uniform_(-1.2, 1.2, generator=gen)
    d = target - o
    return o.to(dev).contiguous(), (d / d.norm(dim=1, keepdim=True)).to(dev).contiguous()


class _Render:
    """one render of RENDERS at the three workspace sizes: forward outputs, statuses and gradients per tier"""

    def __init__(self, name):
        from voxe_hip import ops
        from voxe_hip.runtime import lib, ptr, stream_ptr

        deg, side, R, S, _, _ = RENDERS[name]
        dev = torch.device("cuda:0")
        gen = torch.Generator().manual_seed(42)
        F = 3 * (deg + 1) ** 2
        self.dens = torch.empty((*DIMS, 1)).uniform_(-1, 1, generator=gen).to(dev)
        self.feat = torch.empty((*DIMS, F)).uniform_(-1, 1, generator=gen).to(dev)
        self.ro, self.rd = _rays(side, R, dev)
        self.R = R
        d_colour = torch.randn(R, 3, generator=gen).to(dev)
        d_depth = (0.2 * torch.randn(R, generator=gen)).to(dev)
        spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=2.0)
        params = ops.RenderParams(num_samples=S, near=1.8, far=6.6, white_bkgd=True, sh_degree=deg, image_width=side,
                                  image_height=side)
        L = lib()
        g, c = ops._descs(spec, params, self.dens, self.feat, 0, 0, False)
        gp, cp = C.byref(g), C.byref(c)
        self.route = L.voxe_render_route(gp, cp, R)
        sched = (C.c_int64 * 4)()
        assert L.voxe_tile_sched_debug_layout(gp, cp, R, sched) == abi.OK
        self.segments = sched[2] // sched[3] if sched[3] else None
        c.ray_state_valid = -1
        total = L.voxe_workspace_bytes(gp, cp, R)
        c.ray_state_valid = 0
        full = L.voxe_workspace_bytes(gp, cp, R)
        self.sizes = {"full": full, "total": total, "short": total - 256}
        ws = torch.empty(full, dtype=torch.uint8, device=dev)
        self.fwd, self.fwd_status, self.bwd_status, self.grads = {}, {}, {}, {}
        st = stream_ptr(dev)
        for tier, nbytes in self.sizes.items():
            colour, depth, acc = (torch.zeros(R, n, device=dev) for n in (3, 1, 1))
            c.ray_state_valid = 0
            self.fwd_status[tier] = L.voxe_render_fwd(gp, cp, ptr(self.ro), ptr(self.rd), R, None, ptr(colour), ptr(depth),
                                                      ptr(acc), None, ptr(ws), nbytes, st)
            torch.cuda.synchronize()
            self.fwd[tier] = tuple(x.cpu().numpy() for x in (colour, depth, acc))
            # the backward twice: on what the forward above left in the workspace (claim checked by the library), then re-marching
            for mode, valid in (("kept", 1), ("remarch", 0)):
                gd, gf = torch.zeros_like(self.dens), torch.zeros_like(self.feat)
                c.ray_state_valid = valid
                status = L.voxe_render_bwd(gp, cp, ptr(self.ro), ptr(self.rd), R, None, ptr(colour), ptr(depth), ptr(acc),
                                           ptr(d_colour), ptr(d_depth), None, ptr(gd), ptr(gf), 0, ptr(ws), nbytes, st)
                torch.cuda.synchronize()
                self.bwd_status[tier, mode] = status
                self.grads[tier, mode] = (gd.cpu().numpy(), gf.cpu().numpy())


_cache = {}


@pytest.fixture(params=sorted(RENDERS))
def render(request):
    if request.param not in _cache:
        _cache[request.param] = _Render(request.param)
    return request.param, _cache[request.param]


def test_render_takes_the_route_and_segment_count_it_is_meant_to(render):
    name, r = render
    _, _, _, _, route, segmented = RENDERS[name]
    assert r.route == route
    if segmented is not None:
        assert (r.segments > 1) == segmented, r.segments
    assert r.sizes["full"] >= r.sizes["total"] > 256
    if name in ("tile_two_phase", "region"):
        assert r.sizes["full"] > r.sizes["total"]     # (per-sample sources / binning scratch behind `total`)


def test_forward_succeeds_at_every_tier_and_agrees_with_the_full_workspace(render):
    name, r = render
    assert r.fwd_status == {"full": abi.OK, "total": abi.OK, "short": abi.OK}
    ref = r.fwd["full"]
    assert np.abs(ref[0]).max() > 0.1 and ref[2].max() > 0.5      # (the rays do hit the volume)
    for tier in ("total", "short"):
        colour, depth, acc = r.fwd[tier]
        print(f"{name} {tier}: max|d colour| {np.abs(colour - ref[0]).max():.2e} |d depth| {np.abs(depth - ref[1]).max():.2e} "
              f"|d acc| {np.abs(acc - ref[2]).max():.2e}")
        np.testing.assert_allclose(colour, ref[0], rtol=0, atol=FWD_ATOL)
        np.testing.assert_allclose(acc, ref[2], rtol=0, atol=FWD_ATOL)
        np.testing.assert_allclose(depth, ref[1], rtol=DEPTH_RTOL, atol=FWD_ATOL)


def test_backward_needs_total_bytes_and_agrees_with_the_full_workspace(render):
    name, r = render
    for mode in ("kept", "remarch"):
        assert r.bwd_status["short", mode] == abi.ERR_WORKSPACE
        assert r.bwd_status["total", mode] == abi.OK and r.bwd_status["full", mode] == abi.OK
        assert not r.grads["short", mode][0].any() and not r.grads["short", mode][1].any()    # (refused: nothing written)
    ref_d, ref_f = r.grads["full", "kept"]
    assert np.abs(ref_d).max() > 0 and np.abs(ref_f).max() > 0
    for key in (("full", "remarch"), ("total", "kept"), ("total", "remarch")):
        gd, gf = r.grads[key]
        print(f"{name} {key}: rel-L2 densities {rel_l2(gd, ref_d):.2e} features {rel_l2(gf, ref_f):.2e}")
        assert rel_l2(gd, ref_d) < GRAD_REL_L2 and rel_l2(gf, ref_f) < GRAD_REL_L2, key
