"""float64 torch restatement of the render as a function of its RAYS, differentiated by torch autograd.

What the definition takes from the renderer as constants comes from a sample probe (ops.sample_probe on the device, the oracle's
voxe_cpu_sample_probe on the host: both bit-exact to the forward): the sample depths z, the inside flags and the cell index
i0 = floor(u).  Everything else is recomputed here from the rays: p = o + d z, the fraction f = u(p) - i0 inside that cell, the 8
corners with zero padding (also for the slope: a corner outside the grid is 0), pre / post activations, the SH basis of d / |d|,
sigmoid, delta = dl |d| (last dl = 1e10), w = T alpha, colour (+ white background), depth, acc.  `dtype=torch.float32` runs the
same formulas in float32: the yardstick of what float32 can deliver on these inputs."""
import numpy as np
import torch
import torch.nn.functional as F

from voxe_hip import abi
from voxe_hip.desc import norm_constants

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)


def sh_basis(v, ncu):
    """[R,ncu] real SH basis of unit directions v [R,3] (the renderer's own: spherical_harmonics.py)"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    b = [torch.full_like(x, C0)]
    if ncu > 1:
        b += [-C1 * y, C1 * z, -C1 * x]
    if ncu > 4:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [C2[0] * xy, C2[1] * yz, C2[2] * (2.0 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    if ncu > 9:
        b += [C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
              C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)]
    return torch.stack(b, dim=1)


def _post(act, x):
    if act == abi.ACT_SOFTPLUS:
        return F.softplus(x)
    if act == abi.ACT_RELU:
        return torch.relu(x)
    return x


def render_from_samples(z, inside, idx, densities, features, rays_o, rays_d, spec, params, dtype=torch.float64):
    """(colour [R,3], depth [R], acc [R]) in `dtype` of the probed samples z / inside [R,S], idx [R,S,3]; differentiable w.r.t.
    rays_o / rays_d (and the grid)"""
    R, S = z.shape
    dev = z.device
    X, Y, Z = (int(n) for n in densities.shape[:3])
    Fc = int(features.shape[-1])
    ncm = Fc // 3
    ncu = 1 if params.render_diffuse else (params.sh_degree + 1) ** 2
    assert Fc == 3 * (params.sh_degree + 1) ** 2
    o, d, zz = rays_o.to(dtype), rays_d.to(dtype), z.to(dtype)
    p = o[:, None, :] + d[:, None, :] * zz[:, :, None]
    scale, bias = norm_constants(spec.aabb)
    dims = (X, Y, Z)
    i0 = idx.to(torch.int64)
    w = []
    for a in range(3):
        u = (((p[..., a] * float(scale[a]) + float(bias[a])) + 1.0) * float(dims[a]) - 1.0) * 0.5
        f = u - i0[..., a].to(dtype)
        w.append(torch.stack([1.0 - f, f], dim=-1))
    v = densities.reshape(-1).to(dtype) * float(np.float32(spec.density_scale))
    if spec.density_pre_act == abi.ACT_ABS:
        v = v.abs()
    feat = features.reshape(-1, 3, ncm).to(dtype)[:, :, :ncu]
    dnorm = torch.sqrt((d * d).sum(dim=1))
    basis = sh_basis(d / dnorm[:, None], ncu)                      # [R,ncu]
    vv = torch.zeros((R, S), dtype=dtype, device=dev)
    x = torch.zeros((R, S, 3), dtype=dtype, device=dev)
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                i, j, k = i0[..., 0] + dx, i0[..., 1] + dy, i0[..., 2] + dz
                ok = (i >= 0) & (i < X) & (j >= 0) & (j < Y) & (k >= 0) & (k < Z)
                flat = (i.clamp(0, X - 1) * Y + j.clamp(0, Y - 1)) * Z + k.clamp(0, Z - 1)
                t = (w[0][..., dx] * w[1][..., dy]) * w[2][..., dz]
                t = torch.where(ok, t, torch.zeros_like(t))
                vv = vv + t * v[flat]
                x = x + t[..., None] * (feat[flat] * basis[:, None, None, :]).sum(dim=-1)
    sigma = _post(spec.density_post_act, vv)
    sigma = torch.where(inside.bool(), sigma, torch.zeros_like(sigma))
    rad = torch.sigmoid(x)
    dl = torch.cat([zz[:, 1:] - zz[:, :-1], torch.full((R, 1), 1e10, dtype=dtype, device=dev)], dim=1)
    delta = dl * dnorm[:, None]
    alpha = 1.0 - torch.exp(-sigma * delta)
    T = torch.cumprod(torch.cat([torch.ones((R, 1), dtype=dtype, device=dev), 1.0 - alpha[:, :-1]], dim=1), dim=1)
    wgt = alpha * T
    colour = (wgt[..., None] * rad).sum(dim=1)
    acc = wgt.sum(dim=1)
    depth = (wgt * zz).sum(dim=1)
    if params.white_bkgd:
        colour = colour + (1.0 - acc)[:, None]
    return colour, depth, acc


def probe_device(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0)):
    """(z, inside, idx) of the device forward's own samples"""
    from voxe_hip import ops

    pr = ops.sample_probe(spec, params, densities.detach(), features.detach(), rays_o.detach(), rays_d.detach(), jitter, rng=rng,
                          outputs=("z", "inside", "idx"))
    return pr["z"], pr["inside"], pr["idx"]


def probe_host(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0)):
    """the same from the oracle, on the host (no device)"""
    from oracle import voxe_oracle as vo
    from voxe_hip.desc import make_render_cfg

    grid = vo.Grid(densities.detach().cpu().float().numpy(), features.detach().cpu().float().numpy(), spec.aabb, spec.density_scale,
                   spec.density_pre_act, spec.density_post_act, spec.feature_kind)
    cfg = make_render_cfg(params.num_samples, params.near, params.far, params.perturb, params.linear_disparity, params.aabb_clip,
                          sh_degree=params.sh_degree, render_diffuse=params.render_diffuse, seed=rng[0], rng_offset=rng[1])
    pr = vo.sample_probe(grid, cfg, rays_o.detach().cpu().float().numpy(), rays_d.detach().cpu().float().numpy(),
                         None if jitter is None else jitter.cpu().numpy())
    return tuple(torch.from_numpy(np.ascontiguousarray(pr[k])) for k in ("z", "inside", "idx"))


def ray_gradients(samples, densities, features, rays_o, rays_d, spec, params, g_colour, g_depth, g_acc, dtype=torch.float64):
    """(d_rays_o, d_rays_d) [R,3] in `dtype`: autograd of sum(colour g_colour) + sum(depth g_depth) + sum(acc g_acc) through
    render_from_samples over the probed `samples` = (z, inside, idx); an upstream gradient may be None (= 0)"""
    z, inside, idx = samples
    o = rays_o.detach().to(dtype).clone().requires_grad_(True)
    d = rays_d.detach().to(dtype).clone().requires_grad_(True)
    colour, depth, acc = render_from_samples(z, inside, idx, densities.detach(), features.detach(), o, d, spec, params, dtype)
    L = (o * 0).sum() + (d * 0).sum()
    if g_colour is not None:
        L = L + (colour * g_colour.to(dtype)).sum()
    if g_depth is not None:
        L = L + (depth * g_depth.reshape(-1).to(dtype)).sum()
    if g_acc is not None:
        L = L + (acc * g_acc.reshape(-1).to(dtype)).sum()
    d_o, d_d = torch.autograd.grad(L, (o, d))
    return d_o, d_d


def cast_rays(height, width, focal, poses, flat_index=None):
    """float64 restatement of cast_rays / cast_rays_indexed: (rays_o, rays_d) [B,3] of poses [K,3,4]; differentiable w.r.t.
    poses and focal (a 0-dim tensor or a number)"""
    poses = poses.to(torch.float64)
    K = poses.shape[0]
    per = height * width
    f = torch.arange(K * per, device=poses.device) if flat_index is None else flat_index.to(poses.device)
    cam, rem = f // per, f % per
    py, px = rem // width, rem % width
    x, y = px.to(torch.float64) + 0.5, py.to(torch.float64) + 0.5
    focal = focal if isinstance(focal, torch.Tensor) else torch.tensor(float(focal), dtype=torch.float64)
    focal = focal.to(torch.float64)
    dirs = torch.stack([(x - width * 0.5) / focal, -(y - height * 0.5) / focal, -torch.ones_like(x)], dim=1)     # [B,3]
    rot, trans = poses[cam, :, :3], poses[cam, :, 3]
    return trans, (rot * dirs[:, None, :]).sum(dim=-1)
