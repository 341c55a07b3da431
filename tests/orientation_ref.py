"""float64 torch restatement of the orientation loss on rays, independent of the kernel except for what
the definition takes from the renderer as given: the sample depths and inside flags come from a sample probe (ops.sample_probe
on the device, the oracle's voxe_cpu_sample_probe on the host), sigma is recomputed from the raw densities by
distortion_ref.sigma_from_raw and the weights by distortion_ref.weights, so that torch autograd carries the gradient to the
densities -- through the weights and through the normals.

Per ray, with u = d / |d| and G_k the world gradient of the trilinear interpolant of v = pre(scale * raw) (zero padding) in the
cell of sample k:
    rho_k = sqrt(|G_k|^2 + eps^2),  c_k = max(0, -(G_k . u)) / rho_k  (0 where rho_k == 0),  L_r = sum_k w_k c_k^2
    loss = mean_r omega_r L_r
G is an explicit gather of the 8 corners, the differences along each axis formed first and then blended over the two other axes:
dtype=torch.float32, the yardstick of the GPU tests, then has the kernel's conditioning."""
import numpy as np
import torch

import distortion_ref as DR
import normals_ref
from voxe_hip import abi
from voxe_hip.desc import norm_constants

NORMAL_EPS = 1e-2


def _eps(eps):
    return float(np.float32(eps))


def cell_gradient(densities, points, aabb, density_scale, pre, dtype=torch.float64):
    """G [N,3] (dtype, world units) at world points [N,3] (float32); differentiable w.r.t. densities"""
    X, Y, Z = (int(n) for n in densities.shape[:3])
    _, i0, w0, w1 = normals_ref.index_coords(points, (X, Y, Z), aabb)
    w = torch.stack([w0, w1], dim=-1).to(dtype)                 # [N,3,2]
    v = densities.reshape(-1).to(dtype) * float(np.float32(density_scale))
    if pre == abi.ACT_ABS:
        v = v.abs()
    c = [[[None, None], [None, None]], [[None, None], [None, None]]]
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                i, j, k = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
                ok = (i >= 0) & (i < X) & (j >= 0) & (j < Y) & (k >= 0) & (k < Z)
                flat = (i.clamp(0, X - 1) * Y + j.clamp(0, Y - 1)) * Z + k.clamp(0, Z - 1)
                c[dx][dy][dz] = torch.where(ok, v[flat], torch.zeros((), dtype=dtype, device=v.device))
    gx = sum((w[:, 1, b0] * w[:, 2, b1]) * (c[1][b0][b1] - c[0][b0][b1]) for b1 in range(2) for b0 in range(2))
    gy = sum((w[:, 0, b0] * w[:, 2, b1]) * (c[b0][1][b1] - c[b0][0][b1]) for b1 in range(2) for b0 in range(2))
    gz = sum((w[:, 0, b0] * w[:, 1, b1]) * (c[b0][b1][1] - c[b0][b1][0]) for b1 in range(2) for b0 in range(2))
    scale, _ = norm_constants(aabb)
    gs = [float(np.float32(np.float32(n) * np.float32(scale[a])) * np.float32(0.5)) for a, n in enumerate((X, Y, Z))]
    return torch.stack([gx * gs[0], gy * gs[1], gz * gs[2]], dim=1)


def unit_directions(rays_d, dtype=torch.float64):
    d = rays_d.to(torch.float32)
    dnorm = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return (d / dnorm[:, None]).to(dtype)


def facing(G, u, eps=NORMAL_EPS):
    """c [...]: max(0, -(G . u)) / sqrt(|G|^2 + eps^2), 0 where the root is 0; G [...,3], u broadcastable"""
    eps = _eps(eps)
    rho2 = (G * G).sum(dim=-1) + eps * eps
    ok = rho2 > 0
    rho = torch.sqrt(torch.where(ok, rho2, torch.ones_like(rho2)))      # (no sqrt'(0) in the graph)
    return torch.where(ok, torch.relu(-(G * u).sum(dim=-1)) / rho, torch.zeros_like(rho))


def literal_sum(w, c):
    """L_r [R] of weights w and facing terms c [R,S]"""
    return (w * c * c).sum(dim=1)


def closed_form(x, G, u, eps=NORMAL_EPS):
    """(L, dL/dx [S], dL/dG [S,3]) of ONE ray from its optical depths x [S], cell gradients G [S,3] and unit direction u [3]
    (float64) by the header's formulas: dL/dx_k = c_k^2 (T_k - w_k) - sum_{i>k} c_i^2 w_i,
    dL/dG_k = 2 w_k c_k (-u / rho_k - c_k G_k / rho_k^2) for c_k > 0, else 0"""
    eps = _eps(eps)
    alpha = 1.0 - torch.exp(-x)
    T = torch.cumprod(torch.cat([torch.ones(1, dtype=x.dtype), 1.0 - alpha[:-1]]), dim=0)
    w = alpha * T
    c = facing(G, u, eps)
    cw = c * c * w
    suffix = cw.sum() - torch.cumsum(cw, dim=0)
    rho = torch.sqrt((G * G).sum(dim=-1) + eps * eps)
    safe = torch.where(rho > 0, rho, torch.ones_like(rho))
    dG = (2.0 * w * c)[:, None] * (-u[None, :] / safe[:, None] - (c / (safe * safe))[:, None] * G)
    dG = torch.where((c > 0)[:, None], dG, torch.zeros_like(dG))
    return cw.sum(), c * c * (T - w) - suffix, dG


def lane_split(x, c, G):
    """The kernel's evaluation of ONE ray, in float64, of optical depths x [S] and facing terms c [S]: G contiguous blocks of
    the S samples; march 1 takes each block with a local T = 1 (transmittance product, A = sum w~ c^2, the last sample that adds
    to A), the blocks are folded front to back, march 2 takes the block with the true T and the suffix as (the blocks behind) +
    (the block's total - its running sum), nothing of the block at and behind its last contributing sample.  Returns (L, q) with
    q_k = dL/dx_k at constant c."""
    S = x.shape[0]
    alpha = (1.0 - torch.exp(-x)).tolist()
    c = c.tolist()
    size = (S + G - 1) // G
    blocks = [range(j * size, min(S, (j + 1) * size)) for j in range(G)]
    loc = []
    for blk in blocks:                                         # march 1
        T, A, last = 1.0, 0.0, -1
        for k in blk:
            if not T > 0.0:
                break
            w = alpha[k] * T
            cw = c[k] * c[k] * w
            A += cw
            if cw != 0.0:
                last = k
            T *= 1.0 - alpha[k]
        loc.append((T, A, last))
    Ts, t = [], 1.0
    for T, _, _ in loc:
        Ts.append(t)
        t *= T
    Ablk = [Ts[j] * loc[j][1] for j in range(G)]
    L = sum(Ablk)
    q = [0.0] * S
    for j, blk in enumerate(blocks):                           # march 2
        T, run, behind, last = Ts[j], 0.0, sum(Ablk[j + 1:]), loc[j][2]
        for k in blk:
            if not T > 0.0:
                break
            w = alpha[k] * T
            run += c[k] * c[k] * w
            om = 1.0 - alpha[k]
            if k == S - 1 or not om > 0.0:
                suffix = 0.0
            else:
                suffix = behind if k >= last else behind + (Ablk[j] - run)
            q[k] = c[k] * c[k] * (T * om) - suffix
            T *= om
    return L, torch.tensor(q, dtype=torch.float64)


def from_samples(z, inside, densities, rays_o, rays_d, spec, eps=NORMAL_EPS, dtype=torch.float64, part="both"):
    """L_r [R] (dtype) of the probed samples z / inside [R,S] of rays [R,3]; differentiable w.r.t. `densities`.  part =
    "weights" / "normals" lets the gradient through that path only (the value is the same)."""
    R, S = z.shape
    o, d = rays_o.to(torch.float32), rays_d.to(torch.float32)
    p = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)   # sample.py:67, two roundings in float32
    dens_w = densities.detach() if part == "normals" else densities
    dens_n = densities.detach() if part == "weights" else densities
    sigma = DR.sigma_from_raw(dens_w, p, spec.aabb, spec.density_scale, spec.density_pre_act, spec.density_post_act, dtype).reshape(R, S)
    sigma = torch.where(inside.bool(), sigma, torch.zeros_like(sigma))
    w = DR.weights(sigma, z, rays_d, dtype)
    G = cell_gradient(dens_n, p, spec.aabb, spec.density_scale, spec.density_pre_act, dtype).reshape(R, S, 3)
    c = facing(G, unit_directions(rays_d, dtype)[:, None, :], eps)
    return literal_sum(w, c)


def orientation(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0), eps=NORMAL_EPS, dtype=torch.float64,
                part="both"):
    """the restatement over the device forward's own samples (ops.sample_probe)"""
    from voxe_hip import ops

    probe = ops.sample_probe(spec, params, densities.detach(), features, rays_o, rays_d, jitter, rng=rng, outputs=("z", "inside"))
    return from_samples(probe["z"], probe["inside"], densities, rays_o, rays_d, spec, eps, dtype, part)


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


def orientation_host(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0), eps=NORMAL_EPS,
                     dtype=torch.float64, part="both"):
    """the same over the oracle's samples, on the host: what a test's inputs are checked with before they are used"""
    z, inside = host_samples(spec, params, densities, features, rays_o, rays_d, jitter, rng)
    return from_samples(z, inside, densities, rays_o.cpu(), rays_d.cpu(), spec, eps, dtype, part)


def loss_and_gradient(fn, spec, params, densities, features, rays_o, rays_d, omega=None, **kw):
    """(L_r [R], dloss/draw [X,Y,Z,1] float64) of fn = orientation or orientation_host, loss = mean_r omega_r L_r (omega None
    = 1)"""
    d = densities.detach().clone().requires_grad_(True)
    L = fn(spec, params, d, features, rays_o, rays_d, **kw)
    mean = L.mean() if omega is None else (L * omega.to(device=L.device, dtype=L.dtype)).mean()
    (g,) = torch.autograd.grad(mean, d)
    return L.detach(), g.to(torch.float64)
