"""GPU check of the thread -> ray mapping the lanes-per-ray kernels share (voxe_ray_march.hpp: group_ray over a GroupTile): what
render_normals, distortion_fwd_bwd (ray_loss) and render_bwd_rays give for a ray depends on the ray, the cfg and the lanes per
ray, not on where the mapper put the ray.  The shape is ragged on purpose: 21 x 13 pixels (no side a multiple of a tile side of
any split) x 3 views, S = 33 (a ragged last block of samples per lane).  The three outputs involve no atomics, so the
comparison is bit for bit: image order with image_height set == the same rays in linear order == the rays shuffled."""
import pytest
import torch

from thre3d_atom.utils.imaging_utils import pose_spherical
from voxe_hip import abi, ops, workload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
W, H, VIEWS, S = 21, 13, 3, 33


@pytest.fixture(scope="module")
def scene():
    g = torch.Generator().manual_seed(6)
    dims = (26, 20, 23)
    dens = (torch.empty((*dims, 1)).uniform_(-1, 1, generator=g) * 1.5).to(DEV)
    feat = torch.empty((*dims, 12)).uniform_(-1, 1, generator=g).to(DEV)
    spec = ops.GridSpec(aabb=((-1.3, 1.2), (-1.0, 1.1), (-1.4, 1.0)), density_scale=2.0, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    rays = [ops.cast_rays(H, W, workload.focal_for(W), *pose_spherical(*workload.synth_pose_angles(i, 8), workload.RADIUS), DEV)
            for i in range(VIEWS)]
    ro, rd = torch.cat([r[0] for r in rays]).contiguous(), torch.cat([r[1] for r in rays]).contiguous()
    R = ro.shape[0]
    return dict(spec=spec, dens=dens, feat=feat, ro=ro, rd=rd, jitter=torch.rand((R, S), generator=g).to(DEV),
                perm=torch.randperm(R, generator=g).to(DEV), g_col=torch.randn((R, 3), generator=g).to(DEV),
                g_dep=torch.randn((R, 1), generator=g).to(DEV), g_acc=torch.randn((R, 1), generator=g).to(DEV))


def _normals(s, params, pick, lanes):
    return ops.render_normals(s["spec"], params, s["dens"], pick(s["ro"]), pick(s["rd"]), jitter=pick(s["jitter"]), rng=(0, 0))


def _distortion(s, params, pick, lanes):
    return ops.distortion_fwd_bwd(s["spec"], params, s["dens"], pick(s["ro"]), pick(s["rd"]), pick(s["jitter"]), (0, 0),
                                  want_loss=False, want_ray_loss=True, lanes=lanes)[1:]


def _rays(s, params, pick, lanes):
    return ops.render_bwd_rays(s["spec"], params, s["dens"], s["feat"], pick(s["ro"]), pick(s["rd"]), pick(s["jitter"]), (0, 0),
                               pick(s["g_col"]), pick(s["g_dep"]), pick(s["g_acc"]), lanes=lanes)


# (render_normals takes its lanes per ray from R alone, which the three orders share)
@pytest.mark.parametrize("call,splits", [(_normals, (0,)), (_distortion, (1, 2, 4, 8)), (_rays, (1, 2, 4, 8))],
                         ids=["normals", "distortion", "rays"])
def test_a_rays_result_does_not_depend_on_where_the_mapper_put_it(scene, call, splits):
    fields = dict(num_samples=S, near=workload.NEAR, far=workload.FAR, perturb=True, white_bkgd=True, sh_degree=1)
    image = ops.RenderParams(**fields, image_width=W, image_height=H)
    linear = ops.RenderParams(**fields)
    perm = scene["perm"]
    for lanes in splits:
        a = call(scene, image, lambda t: t, lanes)
        b = call(scene, linear, lambda t: t, lanes)
        c = call(scene, linear, lambda t: t[perm].contiguous(), lanes)
        for x, y, z in zip(a, b, c):
            assert float(x.abs().max()) > 0 and bool(torch.isfinite(x).all())
            assert torch.equal(x, y), (call.__name__, lanes, "image order against linear order")
            assert torch.equal(x[perm], z), (call.__name__, lanes, "image order against shuffled")
