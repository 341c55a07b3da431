"""float64 torch restatement of the lifting sums (DESIGN.md section 4.16 "Lifting"): tests/visibility_ref.from_samples with
index_add_ in place of amax.  It takes from the renderer what visibility_ref takes -- the sample depths, inside flags and sigma of
a sample probe (ops.sample_probe on the device, the oracle's on the host: both bit-exact to the forward) and the float32 index
coordinate of footprint() -- and restates the rest in float64:

    alpha = 1 - exp(-sigma delta),  T_k = prod_{j<k} (1 - alpha_j),  w_k = T_k alpha_k
    sum_w[c]      += w_k t_c                     t_c = (wx * wy) * wz, float32, the forward's gather weight
    sum_wv[c, ch] += w_k t_c values[r, ch]
    n_c[c]        += 1                            for every contribution with w_k t_c > 0

in real units (the kernel's integers times 2^-32).  `mutant` breaks the restatement on purpose, for the tests that show the
error budget of tests/test_lift_gpu.py has teeth: "drop_last" leaves out each ray's last inside sample, "drop_corner" one fixed
corner of every footprint, "stuck_T" does not advance T past each ray's first inside sample."""
import numpy as np
import torch

import normals_ref

MUTANTS = ("drop_last", "drop_corner", "stuck_T")
QUANTUM = 2.0 ** -32


def from_samples(z, inside, sigma, rays_o, rays_d, values, dims, aabb, out=None, mutant=None):
    """(sum_wv [X,Y,Z,C], sum_w [X,Y,Z], n_c [X,Y,Z]) float64 / float64 / int64 of the probed samples z / inside / sigma [R,S] of
    rays [R,3] carrying values [R,C]; `out` = such a triple to accumulate into"""
    assert mutant is None or mutant in MUTANTS
    dev = z.device
    X, Y, Z = (int(n) for n in dims)
    R, S = z.shape
    C = int(values.shape[1])
    o, d = rays_o.to(torch.float32), rays_d.to(torch.float32)
    p = o[:, None, :] + d[:, None, :] * z[:, :, None]          # sample.py:67, two roundings in float32
    dnorm = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    dl = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=dev)], dim=1)
    delta = (dl * dnorm[:, None]).to(torch.float64)
    alpha = 1.0 - torch.exp(-sigma.to(torch.float64) * delta)
    ins2 = inside.bool()
    step = torch.arange(S, device=dev)[None, :].expand(R, S)
    om = 1.0 - alpha
    if mutant == "stuck_T":
        first = torch.where(ins2, step, torch.full_like(step, S)).amin(dim=1, keepdim=True)
        om = torch.where(step == first, torch.ones_like(om), om)
    T = torch.cumprod(torch.cat([torch.ones((R, 1), dtype=torch.float64, device=dev), om[:, :-1]], dim=1), dim=1)
    w = (alpha * T).reshape(-1)
    if mutant == "drop_last":
        last = torch.where(ins2, step, torch.full_like(step, -1)).amax(dim=1, keepdim=True)
        ins2 = ins2 & (step != last)
    _, i0, w0, w1 = normals_ref.index_coords(p.reshape(-1, 3), (X, Y, Z), aabb)
    ax = torch.stack([w0, w1], dim=-1)                          # [N,3,2] float32
    if out is not None:
        swv, sw, nc = out
    else:
        swv = torch.zeros((X * Y * Z, C), dtype=torch.float64, device=dev)
        sw = torch.zeros(X * Y * Z, dtype=torch.float64, device=dev)
        nc = torch.zeros(X * Y * Z, dtype=torch.int64, device=dev)
    swv, sw, nc = swv.view(-1, C), sw.view(-1), nc.view(-1)
    ins = ins2.reshape(-1)
    v = values.to(torch.float64)[:, None, :].expand(R, S, C).reshape(-1, C)
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                if mutant == "drop_corner" and (dx, dy, dz) == (1, 0, 1):
                    continue
                i, j, k = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
                t = (ax[:, 0, dx] * ax[:, 1, dy]) * ax[:, 2, dz]           # float32, the forward's product order
                ok = ins & (i >= 0) & (i < X) & (j >= 0) & (j < Y) & (k >= 0) & (k < Z)
                flat = ((i.clamp(0, X - 1) * Y + j.clamp(0, Y - 1)) * Z + k.clamp(0, Z - 1))
                cw = torch.where(ok, w * t.to(torch.float64), torch.zeros_like(w)).clamp_min(0.0)
                sw.index_add_(0, flat, cw)
                swv.index_add_(0, flat, cw[:, None] * v)
                nc.index_add_(0, flat, (cw > 0).to(torch.int64))
    return swv.view(X, Y, Z, C), sw.view(X, Y, Z), nc.view(X, Y, Z)


def budget(n_c, vmax):
    """the per-voxel bound |kernel - restatement| <= n_c (1e-5 max|v| + 2^-33): 1e-5 is the absolute bound
    tests/test_visibility_gpu.py holds one w_k t_c to, 2^-33 half a quantum of the fixed point"""
    return n_c.to(torch.float64) * (1e-5 * float(vmax) + 2.0 ** -33)


def worst_ratio(got, ref, n_c, vmax):
    """max over the voxels of |got - ref| / budget (0 / 0 = 0; an error where the budget is 0 counts as infinite)"""
    err = (got - ref).abs()
    b = budget(n_c, vmax)
    if err.dim() == 4:
        b = b[..., None].expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    return float(ratio.max())


def lift(spec, params, densities, features, rays_o, rays_d, values, jitter=None, rng=(0, 0), out=None, mutant=None):
    """the restatement over the device forward's own samples (ops.sample_probe)"""
    from voxe_hip import ops

    probe = ops.sample_probe(spec, params, densities, features, rays_o, rays_d, jitter, rng=rng, outputs=("z", "inside", "sigma"))
    return from_samples(probe["z"], probe["inside"], probe["sigma"], rays_o, rays_d, values, densities.shape[:3], spec.aabb,
                        out=out, mutant=mutant)


def host_probe(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0)):
    """(z, inside, sigma) of the oracle's sample probe, on the host (no device)"""
    from oracle import voxe_oracle as vo
    from voxe_hip.desc import make_render_cfg

    grid = vo.Grid(densities.cpu().numpy(), features.cpu().numpy(), spec.aabb, spec.density_scale, spec.density_pre_act,
                   spec.density_post_act, spec.feature_kind)
    cfg = make_render_cfg(params.num_samples, params.near, params.far, params.perturb, params.linear_disparity, params.aabb_clip,
                          seed=rng[0], rng_offset=rng[1])
    probe = vo.sample_probe(grid, cfg, rays_o.cpu().numpy(), rays_d.cpu().numpy(), None if jitter is None else jitter.cpu().numpy())
    return tuple(torch.from_numpy(np.ascontiguousarray(probe[k])) for k in ("z", "inside", "sigma"))


def lift_host(spec, params, densities, features, rays_o, rays_d, values, jitter=None, rng=(0, 0), out=None, mutant=None,
              probe=None):
    """the same over the oracle's samples, on the host: what a test's inputs are checked with before they are used"""
    z, inside, sigma = probe if probe is not None else host_probe(spec, params, densities, features, rays_o, rays_d, jitter, rng)
    return from_samples(z, inside, sigma, rays_o.cpu(), rays_d.cpu(), values.cpu(), densities.shape[:3], spec.aabb, out=out,
                        mutant=mutant)
