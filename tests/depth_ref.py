"""float64 torch restatement of the ray-termination loss towards depth targets, independent of the kernel
except for what the definition takes from the renderer as given: the sample depths and inside flags come from a sample probe
(ops.sample_probe on the device, the oracle's voxe_cpu_sample_probe on the host), and sigma is recomputed from the raw
densities by distortion_ref.sigma_from_raw so that torch autograd carries the gradient to the densities.

Per ray, with a target depth D, a width s and a weight omega:
    w_k = T_k alpha_k (distortion_ref.weights),  dz_k = z_{k+1} - z_k (0 for the last sample)
    c_k = exp(-(z_k - D)^2 / (2 s^2)) dz_k,   L_r = -sum_k c_k log(w_k + eps)  -- the literal sum;   loss = mean_r omega_r L_r
dtype=torch.float32 is the yardstick of the GPU tests: the same formula in float32 torch with alpha = -expm1(-x)."""
import math

import numpy as np
import torch

import distortion_ref as DR

EPS = 1e-5


def _eps(eps):
    return float(np.float32(eps))


def coefficients(z, D, s, dtype=torch.float64):
    """c [R,S] of depths z [R,S] (float32) and targets D, s [R] (float32)"""
    zz = z.to(dtype)
    dz = torch.cat([zz[:, 1:] - zz[:, :-1], torch.zeros_like(zz[:, :1])], dim=1)
    t = (zz - D.to(dtype)[:, None]) / s.to(dtype)[:, None]
    return torch.exp(-0.5 * t * t) * dz


def weights_expm1(sigma, z, rays_d, dtype):
    """distortion_ref.weights with alpha = -expm1(-sigma delta): what a float32 evaluation needs where w is at or below eps"""
    R = z.shape[0]
    d = rays_d.to(torch.float32)
    dnorm = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    dl = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=z.device)], dim=1)
    alpha = -torch.expm1(-sigma * (dl * dnorm[:, None]).to(dtype))
    T = torch.cumprod(torch.cat([torch.ones((R, 1), dtype=dtype, device=z.device), 1.0 - alpha[:, :-1]], dim=1), dim=1)
    return alpha * T


def literal_sum(w, c, eps=EPS):
    """L_r [R] of weights w and coefficients c [R,S]"""
    return -(c * torch.log(w + _eps(eps))).sum(dim=1)


def closed_form(x, c, eps=EPS):
    """(L, dL/dx [S]) of ONE ray from its optical depths x [S] and coefficients c [S] (float64) by the header's formulas:
    g_k = -c_k / (w_k + eps), dL/dx_k = g_k (T_k - w_k) - sum_{i>k} g_i w_i"""
    eps = _eps(eps)
    alpha = -torch.expm1(-x)
    T = torch.cumprod(torch.cat([torch.ones(1, dtype=x.dtype), 1.0 - alpha[:-1]]), dim=0)
    w = alpha * T
    g = -c / (w + eps)
    gw = g * w
    suffix = gw.sum() - torch.cumsum(gw, dim=0)
    return -(c * torch.log(w + eps)).sum(), g * (T - w) - suffix


def lane_split(x, c, G, eps=EPS):
    """The kernel's evaluation of ONE ray, in float64: G contiguous blocks of the S samples; phase 0 sums c over each block,
    phase 1 takes each block's transmittance product, phase 2 marches it with the true T (stopping where T reaches 0: the
    constants of the samples behind are in phase 0's sum) for sum c log1p(w / eps) and sum g w, phase 3 takes the suffix as
    (the blocks behind) + (the block's sum - its running sum).  Returns (L, q) with q_k = dL/dx_k."""
    eps = _eps(eps)
    S = x.shape[0]
    alpha = (-torch.expm1(-x)).tolist()
    c = c.tolist()
    size = (S + G - 1) // G
    blocks = [range(j * size, min(S, (j + 1) * size)) for j in range(G)]
    Csum = [sum(c[k] for k in blk) for blk in blocks]                                  # phase 0
    Tb = [math.prod(1.0 - alpha[k] for k in blk) for blk in blocks]                    # phase 1
    Ts, t = [], 1.0
    for tb in Tb:
        Ts.append(t)
        t *= tb
    Lw, GW = [0.0] * G, [0.0] * G
    for j, blk in enumerate(blocks):                                                   # phase 2
        T = Ts[j]
        for k in blk:
            if not T > 0.0:
                break
            w = T * alpha[k]
            Lw[j] += c[k] * math.log1p(w / eps)
            GW[j] += (-c[k] / (w + eps)) * w
            T *= 1.0 - alpha[k]
    L = sum(-math.log(eps) * Csum[j] - Lw[j] for j in range(G))
    q = [0.0] * S
    for j, blk in enumerate(blocks):                                                   # phase 3
        T, run, behind = Ts[j], 0.0, sum(GW[j + 1:])
        for k in blk:
            if not T > 0.0:
                break
            w = T * alpha[k]
            g = -c[k] / (w + eps)
            run += g * w
            om = 1.0 - alpha[k]
            suffix = 0.0 if (k == S - 1 or not om > 0.0) else behind + (GW[j] - run)
            q[k] = g * (T * om) - suffix
            T *= om
    return L, torch.tensor(q, dtype=torch.float64)


def from_samples(z, inside, densities, rays_o, rays_d, spec, D, s, eps=EPS, dtype=torch.float64):
    """L_r [R] (dtype) of the probed samples z / inside [R,S] of rays [R,3]; differentiable w.r.t. `densities`"""
    R, S = z.shape
    o, d = rays_o.to(torch.float32), rays_d.to(torch.float32)
    p = o[:, None, :] + d[:, None, :] * z[:, :, None]          # sample.py:67, two roundings in float32
    sigma = DR.sigma_from_raw(densities, p.reshape(-1, 3), spec.aabb, spec.density_scale, spec.density_pre_act,
                              spec.density_post_act, dtype).reshape(R, S)
    sigma = torch.where(inside.bool(), sigma, torch.zeros_like(sigma))
    w = DR.weights(sigma, z, rays_d, dtype) if dtype == torch.float64 else weights_expm1(sigma, z, rays_d, dtype)
    return literal_sum(w, coefficients(z, D, s, dtype), eps)


def depth(spec, params, densities, features, rays_o, rays_d, D, s, jitter=None, rng=(0, 0), eps=EPS, dtype=torch.float64):
    """the restatement over the device forward's own samples (ops.sample_probe)"""
    from voxe_hip import ops

    probe = ops.sample_probe(spec, params, densities.detach(), features, rays_o, rays_d, jitter, rng=rng, outputs=("z", "inside"))
    return from_samples(probe["z"], probe["inside"], densities, rays_o, rays_d, spec, D, s, eps, dtype)


def host_samples(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0)):
    """(z, inside) [R,S] of the oracle's sample probe, on the host (no device)"""
    from oracle import voxe_oracle as vo
    from voxe_hip.desc import make_render_cfg

    grid = vo.Grid(densities.detach().float().cpu().numpy(), features.cpu().numpy(), spec.aabb, spec.density_scale,
                   spec.density_pre_act, spec.density_post_act, spec.feature_kind)
    cfg = make_render_cfg(params.num_samples, params.near, params.far, params.perturb, params.linear_disparity, params.aabb_clip,
                          seed=rng[0], rng_offset=rng[1])
    probe = vo.sample_probe(grid, cfg, rays_o.cpu().numpy(), rays_d.cpu().numpy(), None if jitter is None else jitter.cpu().numpy())
    return tuple(torch.from_numpy(np.ascontiguousarray(probe[k])) for k in ("z", "inside"))


def depth_host(spec, params, densities, features, rays_o, rays_d, D, s, jitter=None, rng=(0, 0), eps=EPS, dtype=torch.float64):
    """the same over the oracle's samples, on the host: what a test's inputs are checked with before they are used"""
    z, inside = host_samples(spec, params, densities, features, rays_o, rays_d, jitter, rng)
    return from_samples(z, inside, densities, rays_o.cpu(), rays_d.cpu(), spec, D.cpu(), s.cpu(), eps, dtype)


def loss_and_gradient(fn, spec, params, densities, features, rays_o, rays_d, D, s, omega=None, **kw):
    """(L_r [R] float64, dloss/draw [X,Y,Z,1] float64) of fn = depth or depth_host, loss = mean_r omega_r L_r (omega None = 1)"""
    if omega is None:
        return DR.loss_and_gradient(fn, spec, params, densities, features, rays_o, rays_d, D, s, **kw)
    d = densities.detach().clone().requires_grad_(True)
    L = fn(spec, params, d, features, rays_o, rays_d, D, s, **kw)
    (g,) = torch.autograd.grad((L * omega.to(device=L.device, dtype=L.dtype)).mean(), d)
    return L.detach(), g.to(torch.float64)
