"""float64 torch restatement of the per-voxel visibility grids (DESIGN.md section 4 "Visibility"), independent of the kernel
except for what the definitions take from the renderer as given: the sample depths, inside flags and sigma come from a sample
probe (ops.sample_probe on the device, the oracle's voxe_cpu_sample_probe on the host: both bit-exact to the forward), and the
index coordinate u is computed in float32 with footprint()'s operation order (normals_ref.index_coords).

Per sample k of ray r: alpha = 1 - exp(-sigma delta), T_k = prod_{j<k} (1 - alpha_j), w_k = T_k alpha_k (normals_ref's weights);
for each of the 8 corners c = floor(u) + {0,1}^3 inside the grid with weight t_c = (wx * wy) * wz (float32, the forward's gather
weight):  max_weight[c] = max(.., w_k t_c),  max_trans[c] = max(.., T_k) where t_c > 0.  Only samples that pass the strict AABB
test have a footprint."""
import numpy as np
import torch

import normals_ref


def from_samples(z, inside, sigma, rays_o, rays_d, dims, aabb, out=None):
    """(max_weight, max_trans) float64 [X,Y,Z] of the probed samples z / inside / sigma [R,S] of rays [R,3]; `out` = a pair to
    accumulate into"""
    dev = z.device
    X, Y, Z = (int(n) for n in dims)
    R, S = z.shape
    o, d = rays_o.to(torch.float32), rays_d.to(torch.float32)
    p = o[:, None, :] + d[:, None, :] * z[:, :, None]          # sample.py:67, two roundings in float32
    dnorm = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    dl = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=dev)], dim=1)
    delta = (dl * dnorm[:, None]).to(torch.float64)
    alpha = 1.0 - torch.exp(-sigma.to(torch.float64) * delta)
    T = torch.cumprod(torch.cat([torch.ones((R, 1), dtype=torch.float64, device=dev), 1.0 - alpha[:, :-1]], dim=1), dim=1)
    w = (alpha * T).reshape(-1)
    T = T.reshape(-1)
    _, i0, w0, w1 = normals_ref.index_coords(p.reshape(-1, 3), (X, Y, Z), aabb)
    ax = torch.stack([w0, w1], dim=-1)                          # [N,3,2] float32
    mw, mt = out if out is not None else (torch.zeros(X * Y * Z, dtype=torch.float64, device=dev) for _ in range(2))
    mw, mt = mw.view(-1), mt.view(-1)
    ins = inside.reshape(-1).bool()
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                i, j, k = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
                t = (ax[:, 0, dx] * ax[:, 1, dy]) * ax[:, 2, dz]           # float32, the forward's product order
                ok = ins & (i >= 0) & (i < X) & (j >= 0) & (j < Y) & (k >= 0) & (k < Z)
                flat = ((i.clamp(0, X - 1) * Y + j.clamp(0, Y - 1)) * Z + k.clamp(0, Z - 1))
                cw = torch.where(ok, w * t.to(torch.float64), torch.zeros_like(w))
                ct = torch.where(ok & (t > 0), T, torch.zeros_like(T))
                mw.scatter_reduce_(0, flat, cw.clamp_min(0.0), "amax", include_self=True)
                mt.scatter_reduce_(0, flat, ct.clamp_min(0.0), "amax", include_self=True)
    return mw.view(X, Y, Z), mt.view(X, Y, Z)


def visibility(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0), out=None):
    """the restatement over the device forward's own samples (ops.sample_probe)"""
    from voxe_hip import ops

    probe = ops.sample_probe(spec, params, densities, features, rays_o, rays_d, jitter, rng=rng, outputs=("z", "inside", "sigma"))
    return from_samples(probe["z"], probe["inside"], probe["sigma"], rays_o, rays_d, densities.shape[:3], spec.aabb, out=out)


def visibility_host(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0), out=None):
    """the same over the oracle's samples, on the host (no device): what a test's inputs are checked with before they are used"""
    from oracle import voxe_oracle as vo
    from voxe_hip.desc import make_render_cfg

    grid = vo.Grid(densities.cpu().numpy(), features.cpu().numpy(), spec.aabb, spec.density_scale, spec.density_pre_act,
                   spec.density_post_act, spec.feature_kind)
    cfg = make_render_cfg(params.num_samples, params.near, params.far, params.perturb, params.linear_disparity, params.aabb_clip,
                          seed=rng[0], rng_offset=rng[1])
    ro, rd = rays_o.cpu(), rays_d.cpu()
    probe = vo.sample_probe(grid, cfg, ro.numpy(), rd.numpy(), None if jitter is None else jitter.cpu().numpy())
    z, inside, sigma = (torch.from_numpy(np.ascontiguousarray(probe[k])) for k in ("z", "inside", "sigma"))
    return from_samples(z, inside, sigma, ro, rd, densities.shape[:3], spec.aabb, out=out)
