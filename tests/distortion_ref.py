"""float64 torch restatement of the distortion loss on rays, independent of the kernel except for what the
definition takes from the renderer as given: the sample depths and inside flags come from a sample probe (ops.sample_probe on the
device, the oracle's voxe_cpu_sample_probe on the host: both bit-exact to the forward).  sigma is RECOMPUTED here from the raw
densities -- pre(scale * raw) at the 8 corners of floor(u), blended with normals_ref.index_coords' float32 weights in the
forward's product order, zero padding, then the post-activation -- so that torch autograd carries the gradient to the densities.

Per ray: alpha = 1 - exp(-sigma delta) (last dl = 1e10), T_k = prod_{j<k} (1 - alpha_j), w_k = T_k alpha_k;
s_k = (z_k - near) / (far - near), d_k = s_{k+1} - s_k (0 for the last sample), m_k = s_k + d_k / 2;
L_r = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i  -- the literal O(S^2) double sum;  loss = mean_r L_r."""
import numpy as np
import torch
import torch.nn.functional as F

import normals_ref
from voxe_hip import abi

_CHUNK = 512   # rays per slice of the [R,S,S] pair sum


def sigma_from_raw(densities, points, aabb, density_scale, pre, post, dtype=torch.float64):
    """sigma [N] (dtype) of world points [N,3] (float32) from the raw densities [X,Y,Z,1]; differentiable w.r.t. densities"""
    X, Y, Z = (int(n) for n in densities.shape[:3])
    _, i0, w0, w1 = normals_ref.index_coords(points, (X, Y, Z), aabb)
    ax = torch.stack([w0, w1], dim=-1)                          # [N,3,2] float32
    v = densities.reshape(-1).to(dtype) * float(np.float32(density_scale))
    if pre == abi.ACT_ABS:
        v = v.abs()
    out = torch.zeros(points.shape[0], dtype=dtype, device=points.device)
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                i, j, k = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
                t = (ax[:, 0, dx] * ax[:, 1, dy]) * ax[:, 2, dz]           # float32, the forward's product order
                ok = (i >= 0) & (i < X) & (j >= 0) & (j < Y) & (k >= 0) & (k < Z)
                flat = (i.clamp(0, X - 1) * Y + j.clamp(0, Y - 1)) * Z + k.clamp(0, Z - 1)
                out = out + torch.where(ok, v[flat] * t.to(dtype), torch.zeros_like(out))
    if post == abi.ACT_SOFTPLUS:
        return F.softplus(out)
    if post == abi.ACT_RELU:
        return torch.relu(out)
    return out


def weights(sigma, z, rays_d, dtype=torch.float64):
    """w [R,S] = T alpha of sigma [R,S] (0 where the sample is outside) at depths z [R,S] (float32)"""
    R = z.shape[0]
    d = rays_d.to(torch.float32)
    dnorm = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    dl = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=z.device)], dim=1)
    delta = (dl * dnorm[:, None]).to(dtype)
    alpha = 1.0 - torch.exp(-sigma * delta)
    T = torch.cumprod(torch.cat([torch.ones((R, 1), dtype=dtype, device=z.device), 1.0 - alpha[:, :-1]], dim=1), dim=1)
    return alpha * T


def intervals(z, near, far, dtype=torch.float64):
    """(m, d) [R,S] of depths z [R,S]"""
    near, far = float(np.float32(near)), float(np.float32(far))
    s = (z.to(dtype) - near) / (far - near)
    d = torch.cat([s[:, 1:] - s[:, :-1], torch.zeros_like(s[:, :1])], dim=1)
    return s + d / 2, d


def pair_sum(w, m, d):
    """L_r [R]: the literal double sum"""
    out = []
    for a in range(0, w.shape[0], _CHUNK):
        ww, mm, dd = w[a:a + _CHUNK], m[a:a + _CHUNK], d[a:a + _CHUNK]
        pair = (ww[:, :, None] * ww[:, None, :] * (mm[:, :, None] - mm[:, None, :]).abs()).sum(dim=(1, 2))
        out.append(pair + (ww * ww * dd).sum(dim=1) / 3.0)
    return torch.cat(out) if out else w.new_zeros((0,))


def prefix_sum(w, m, d):
    """L_r [R] in O(S) for non-decreasing m: 2 sum_i w_i (m_i W_i - WM_i) + (1/3) sum_i w_i^2 d_i with exclusive prefixes"""
    W = torch.cumsum(w, dim=1) - w
    WM = torch.cumsum(w * m, dim=1) - w * m
    return 2.0 * (w * (m * W - WM)).sum(dim=1) + (w * w * d).sum(dim=1) / 3.0


def lane_split(x, m, d, G):
    """The kernel's evaluation of ONE ray, in float64: alpha = 1 - exp(-x) [S] split into G contiguous blocks that are marched
    with a local T = 1 and folded by scans.  Returns (L, q) with q_k = g_k (T_k - w_k) - sum_{i>k} g_i w_i,
    i.e. dL/dx_k."""
    S = x.shape[0]
    alpha = (1.0 - torch.exp(-x)).tolist()
    m, d = m.tolist(), d.tolist()
    size = (S + G - 1) // G
    blocks = [range(j * size, min(S, (j + 1) * size)) for j in range(G)]
    loc = []
    for blk in blocks:                                         # march 1
        T, A, B, P, U = 1.0, 0.0, 0.0, 0.0, 0.0
        for k in blk:
            w = alpha[k] * T
            P += w * (m[k] * A - B)
            A += w
            B += w * m[k]
            U += w * w * d[k]
            T *= 1.0 - alpha[k]
        loc.append((T, A, B, 2.0 * P + U / 3.0))
    Ts, W0, WM0, Lpre = [], [], [], []
    t, w0, wm0, l = 1.0, 0.0, 0.0, 0.0
    for T, A, B, Lb in loc:                                    # the scans
        Ts.append(t); W0.append(w0); WM0.append(wm0); Lpre.append(l)
        a, b = t * A, t * B
        l += t * t * Lb + 2.0 * (b * w0 - a * wm0)
        w0 += a
        wm0 += b
        t *= T
    Wtot, WMtot, Ltot = w0, wm0, l
    q = [0.0] * S
    for j, blk in enumerate(blocks):                           # march 2
        T, W, WM = Ts[j], W0[j], WM0[j]
        GW = 2.0 * Lpre[j] + 2.0 * (W0[j] * (WMtot - WM0[j]) - WM0[j] * (Wtot - W0[j]))
        for k in blk:
            w = alpha[k] * T
            g = 2.0 * ((m[k] * W - WM) + ((WMtot - WM - w * m[k]) - m[k] * (Wtot - W - w))) + (2.0 / 3.0) * w * d[k]
            W += w
            WM += w * m[k]
            GW += g * w
            q[k] = g * (T - w) - (2.0 * Ltot - GW)
            T *= 1.0 - alpha[k]
    return Ltot, torch.tensor(q, dtype=torch.float64)


def from_samples(z, inside, densities, rays_o, rays_d, spec, near, far, dtype=torch.float64):
    """L_r [R] (dtype) of the probed samples z / inside [R,S] of rays [R,3]; differentiable w.r.t. `densities`"""
    R, S = z.shape
    o, d = rays_o.to(torch.float32), rays_d.to(torch.float32)
    p = o[:, None, :] + d[:, None, :] * z[:, :, None]          # sample.py:67, two roundings in float32
    sigma = sigma_from_raw(densities, p.reshape(-1, 3), spec.aabb, spec.density_scale, spec.density_pre_act,
                           spec.density_post_act, dtype).reshape(R, S)
    sigma = torch.where(inside.bool(), sigma, torch.zeros_like(sigma))
    w = weights(sigma, z, rays_d, dtype)
    m, dd = intervals(z, near, far, dtype)
    return pair_sum(w, m, dd)


def distortion(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0), dtype=torch.float64):
    """the restatement over the device forward's own samples (ops.sample_probe)"""
    from voxe_hip import ops

    probe = ops.sample_probe(spec, params, densities.detach(), features, rays_o, rays_d, jitter, rng=rng, outputs=("z", "inside"))
    return from_samples(probe["z"], probe["inside"], densities, rays_o, rays_d, spec, params.near, params.far, dtype)


def distortion_host(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0), dtype=torch.float64):
    """the same over the oracle's samples, on the host (no device): what a test's inputs are checked with before they are used"""
    from oracle import voxe_oracle as vo
    from voxe_hip.desc import make_render_cfg

    grid = vo.Grid(densities.detach().cpu().numpy(), features.cpu().numpy(), spec.aabb, spec.density_scale, spec.density_pre_act,
                   spec.density_post_act, spec.feature_kind)
    cfg = make_render_cfg(params.num_samples, params.near, params.far, params.perturb, params.linear_disparity, params.aabb_clip,
                          seed=rng[0], rng_offset=rng[1])
    ro, rd = rays_o.cpu(), rays_d.cpu()
    probe = vo.sample_probe(grid, cfg, ro.numpy(), rd.numpy(), None if jitter is None else jitter.cpu().numpy())
    z, inside = (torch.from_numpy(np.ascontiguousarray(probe[k])) for k in ("z", "inside"))
    return from_samples(z, inside, densities, ro, rd, spec, params.near, params.far, dtype)


def loss_and_gradient(fn, spec, params, densities, *args, **kw):
    """(L_r [R] float64, dloss/draw [X,Y,Z,1] float64) of fn = distortion or distortion_host, loss = mean_r L_r"""
    d = densities.detach().clone().requires_grad_(True)
    L = fn(spec, params, d, *args, **kw)
    (g,) = torch.autograd.grad(L.mean(), d)
    return L.detach(), g.to(torch.float64)
