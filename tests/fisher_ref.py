"""float64 torch restatement of the per-voxel Fisher information, independent of the kernel.

The colours are ray_grad_ref.render_from_samples on probed samples (ray_grad_ref.probe_device / probe_host: bit-exact to the
forward); the per-ray Jacobians J [R,3,V] = d colour_{r,ch} / d raw density come from torch autograd, one backward per ray and
channel (the GPU tests keep R <= ~100).  Then

    fisher[c]  = sum_r sum_ch J[r,ch,c]^2          ray_var[r] = sum_c P[c] sum_ch J[r,ch,c]^2

`dtype=torch.float32` runs the same formulas in float32: the yardstick of what float32 can deliver on an input.

sample_terms() is the header's closed form written out per sample (what the kernel sums): test_fisher_host.py holds it against
autograd, and it yields the DELIBERATELY WRONG variant per_sample_squares(), which squares every sample's deposit on its own instead
of the sum of a voxel's run of samples: what a kernel without the carry would compute.  The non-vacuousness checks measure how
far that variant is from the truth on every input."""
import numpy as np
import torch

import ray_grad_ref as RG
from voxe_hip import abi
from voxe_hip.desc import norm_constants


def jacobians(samples, densities, features, rays_o, rays_d, spec, params, dtype=torch.float64):
    """J [R,3,V] in `dtype`: autograd of colour[r,ch] through render_from_samples, one backward per ray and channel"""
    z, inside, idx = samples
    d = densities.detach().to(dtype).clone().requires_grad_(True)
    colour, _, _ = RG.render_from_samples(z, inside, idx, d, features.detach(), rays_o.detach(), rays_d.detach(), spec, params, dtype)
    R = colour.shape[0]
    J = torch.zeros((R, 3, d.numel()), dtype=dtype, device=d.device)
    for r in range(R):
        for ch in range(3):
            (g,) = torch.autograd.grad(colour[r, ch], d, retain_graph=True)
            J[r, ch] = g.reshape(-1)
    return J


def fisher_of(J):
    """H [V] = sum_r sum_ch J^2"""
    return (J * J).sum(dim=(0, 1))


def ray_var_of(J, voxel_var=None):
    """[R] = sum_c P[c] sum_ch J^2 (P = 1 when None)"""
    s = (J * J).sum(dim=1)
    return s.sum(dim=1) if voxel_var is None else (s * voxel_var.reshape(1, -1).to(J.dtype)).sum(dim=1)


def sample_terms(samples, densities, features, rays_o, rays_d, spec, params, dtype=torch.float64):
    """The closed form per sample: (a [R,S,3], flat [R,S,8], cf [R,S,8]) with a_{k,ch} = delta_k E_{k,ch} post'(v_k) (0 for a
    sample outside the box), `flat` the voxel of corner q = 4 x + 2 y + z of the sample's footprint (clamped where outside) and
    cf = t_c pre'(scale raw_c) scale (0 for a corner outside the grid): J[r,ch,c] = sum over (k, q) with flat == c of a cf"""
    z, inside, idx = samples
    R, S = z.shape
    dev = z.device
    X, Y, Z = (int(n) for n in densities.shape[:3])
    ncm = int(features.shape[-1]) // 3
    ncu = 1 if params.render_diffuse else (params.sh_degree + 1) ** 2
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
    ds = float(np.float32(spec.density_scale))
    pre = densities.reshape(-1).to(dtype) * ds
    dpre = torch.full_like(pre, ds)
    if spec.density_pre_act == abi.ACT_ABS:
        dpre = torch.sign(pre) * ds
        pre = pre.abs()
    feat = features.reshape(-1, 3, ncm).to(dtype)[:, :, :ncu]
    dnorm = torch.sqrt((d * d).sum(dim=1))
    basis = RG.sh_basis(d / dnorm[:, None], ncu)
    vv = torch.zeros((R, S), dtype=dtype, device=dev)
    x = torch.zeros((R, S, 3), dtype=dtype, device=dev)
    flats, cfs = [], []
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                i, j, k = i0[..., 0] + dx, i0[..., 1] + dy, i0[..., 2] + dz
                ok = (i >= 0) & (i < X) & (j >= 0) & (j < Y) & (k >= 0) & (k < Z)
                flat = (i.clamp(0, X - 1) * Y + j.clamp(0, Y - 1)) * Z + k.clamp(0, Z - 1)
                t = (w[0][..., dx] * w[1][..., dy]) * w[2][..., dz]
                t = torch.where(ok, t, torch.zeros_like(t))
                vv = vv + t * pre[flat]
                x = x + t[..., None] * (feat[flat] * basis[:, None, None, :]).sum(dim=-1)
                flats.append(flat)
                cfs.append(t * dpre[flat])
    ins = inside.bool()
    if spec.density_post_act == abi.ACT_SOFTPLUS:
        sigma, dpost = torch.nn.functional.softplus(vv), torch.sigmoid(vv)
    elif spec.density_post_act == abi.ACT_RELU:
        sigma, dpost = torch.relu(vv), (vv > 0).to(dtype)
    else:
        sigma, dpost = vv, torch.ones_like(vv)
    sigma = torch.where(ins, sigma, torch.zeros_like(sigma))
    q = torch.sigmoid(x) - (1.0 if params.white_bkgd else 0.0)
    dl = torch.cat([zz[:, 1:] - zz[:, :-1], torch.full((R, 1), 1e10, dtype=dtype, device=dev)], dim=1)
    delta = dl * dnorm[:, None]
    e = torch.exp(-sigma * delta)
    T = torch.cumprod(torch.cat([torch.ones((R, 1), dtype=dtype, device=dev), e[:, :-1]], dim=1), dim=1)
    wq = ((1.0 - e) * T)[..., None] * q
    suffix = wq.flip(1).cumsum(dim=1).flip(1) - wq                    # sum over i > k
    E = q * (T * e)[..., None] - suffix                                  # T e = T - w
    a = (delta * dpost)[..., None] * E
    a = torch.where(ins[..., None], a, torch.zeros_like(a))
    return a, torch.stack(flats, dim=-1), torch.stack(cfs, dim=-1)


def closed_form_jacobians(terms, V):
    """J [R,3,V] of sample_terms(): every voxel's deposits summed per ray"""
    a, flat, cf = terms
    R, S = flat.shape[:2]
    J = torch.zeros((R, 3, V), dtype=a.dtype, device=a.device)
    dep = a[:, :, None, :] * cf[..., None]                               # [R,S,8,3]
    for ch in range(3):
        J[:, ch].scatter_add_(1, flat.reshape(R, -1), dep[..., ch].reshape(R, -1))
    return J


def per_sample_squares(terms, V):
    """the WRONG fisher [V]: sum over rays, samples, corners and channels of the squared deposit (no carry along the ray)"""
    a, flat, cf = terms
    dep = a[:, :, None, :] * cf[..., None]
    H = torch.zeros(V, dtype=a.dtype, device=a.device)
    H.scatter_add_(0, flat.reshape(-1), (dep * dep).sum(dim=-1).reshape(-1))
    return H


def carry_facts(samples, dims):
    """what the carry rule meets along the rays, from the probed samples: the clamped cell of every inside sample (the kernel's
    Cell: low corner moved into [0, N-2]) and, between consecutive inside samples of a ray, how many axes change at once and whether
    a jump exceeds one cell; plus the number of inside samples with a footprint corner outside the grid"""
    z, inside, idx = samples
    ins = inside.bool()
    N = torch.tensor(dims, device=idx.device)
    i0 = idx.to(torch.int64)
    cell = torch.minimum(i0.clamp(min=0), (N - 2).clamp(min=0))
    both = ins[:, 1:] & ins[:, :-1]
    d = (cell[:, 1:] - cell[:, :-1]).abs()
    step = both & (d.max(dim=-1).values == 1)
    naxes = (d != 0).sum(dim=-1)
    outside = ins & ((i0 < 0) | (i0 >= N - 1)).any(dim=-1)
    return {"two_axes": int((step & (naxes == 2)).sum()), "three_axes": int((step & (naxes == 3)).sum()),
            "jumps": int((both & (d.max(dim=-1).values > 1)).sum()), "same_cell": int((both & (naxes == 0)).sum()),
            "outside_corners": int(outside.sum()), "inside": int(ins.sum()),
            "missed_rays": int((~ins.any(dim=1)).sum())}
