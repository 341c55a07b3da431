"""float64 torch restatement of the density-gradient normals (DESIGN.md section 4 "Normals"), independent of the kernels except
for what the definitions take from the renderer as given: the index coordinate u is computed in float32 with footprint()'s
operation order, and the render's sample depths / inside flags / sigma come from ops.sample_probe (bit-exact to the forward).

Per voxel v_i = pre(s * raw_i) (float32), V(p) = trilinear interpolant with zero padding, dV/du_a = the slope of exactly that
interpolant in the cell floor(u) selects (corners outside the grid are 0), G_a = dV/du_a * (N_a * scale_a / 2),
n = -G / |G| ((0,0,0) where G == 0), N_r = sum_k w_k n(p_k)."""
import numpy as np
import torch

from voxe_hip import abi
from voxe_hip.desc import norm_constants


def field(densities: torch.Tensor, scale: float, pre: int) -> torch.Tensor:
    """v [X,Y,Z] float32, as the pack kernel stores it"""
    v = densities.reshape(densities.shape[:3]).to(torch.float32) * torch.tensor(np.float32(scale), device=densities.device)
    return v.abs() if pre == abi.ACT_ABS else v


def index_coords(points: torch.Tensor, dims, aabb):
    """u [N,3] float32 with footprint()'s rounding, floor index i0 [N,3] int64, weights (w0, w1) [N,3] float32"""
    scale, bias = norm_constants(aabb)
    p = points.to(torch.float32)
    us = []
    for a in range(3):
        n = p[:, a] * torch.tensor(scale[a], device=p.device)
        n = n + torch.tensor(bias[a], device=p.device)
        u = n + 1.0
        u = u * float(dims[a])
        u = u - 1.0
        u = u * 0.5
        us.append(u)
    u = torch.stack(us, dim=1)
    fl = torch.floor(u)
    return u, fl.to(torch.int64), (fl + 1.0) - u, u - fl


def _corner(v: torch.Tensor, i: torch.Tensor, j: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    X, Y, Z = v.shape
    ok = (i >= 0) & (i < X) & (j >= 0) & (j < Y) & (k >= 0) & (k < Z)
    out = v[i.clamp(0, X - 1), j.clamp(0, Y - 1), k.clamp(0, Z - 1)].to(torch.float64)
    return torch.where(ok, out, torch.zeros_like(out))


def value_and_gradient(v: torch.Tensor, points: torch.Tensor, aabb):
    """V(p) [N] and the world gradient G(p) [N,3], float64"""
    dims = v.shape
    _, i0, w0, w1 = index_coords(points, dims, aabb)
    w = torch.stack([w0, w1], dim=-1).to(torch.float64)       # [N,3,2]
    c = torch.empty((points.shape[0], 2, 2, 2), dtype=torch.float64, device=points.device)
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                c[:, dx, dy, dz] = _corner(v, i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz)
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    V = torch.einsum("nx,ny,nz,nxyz->n", wx, wy, wz, c)
    gx = torch.einsum("ny,nz,nyz->n", wy, wz, c[:, 1] - c[:, 0])
    gy = torch.einsum("nx,nz,nxz->n", wx, wz, c[:, :, 1] - c[:, :, 0])
    gz = torch.einsum("nx,ny,nxy->n", wx, wy, c[:, :, :, 1] - c[:, :, :, 0])
    scale, _ = norm_constants(aabb)
    gs = torch.tensor([dims[a] * float(scale[a]) / 2.0 for a in range(3)], dtype=torch.float64, device=points.device)
    return V, torch.stack([gx, gy, gz], dim=1) * gs


def normals_from_gradient(G: torch.Tensor) -> torch.Tensor:
    nrm = G.norm(dim=1, keepdim=True)
    return torch.where(nrm > 0, -G / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.zeros_like(G))


def point_normals(v: torch.Tensor, points: torch.Tensor, aabb) -> torch.Tensor:
    return normals_from_gradient(value_and_gradient(v, points, aabb)[1])


def post(act: int, x: torch.Tensor) -> torch.Tensor:
    if act == abi.ACT_SOFTPLUS:
        return torch.nn.functional.softplus(x)
    if act == abi.ACT_RELU:
        return torch.relu(x)
    return x


def render_normals(spec, params, densities, features, rays_o, rays_d, jitter=None, rng=(0, 0)):
    """(N [R,3], depth [R], acc [R]) float64 over the forward's own samples (ops.sample_probe)"""
    from voxe_hip import ops

    probe = ops.sample_probe(spec, params, densities, features, rays_o, rays_d, jitter, rng=rng, outputs=("z", "inside", "sigma"))
    z, sigma = probe["z"], probe["sigma"].to(torch.float64)
    R, S = z.shape
    o, d = rays_o.to(torch.float32), rays_d.to(torch.float32)
    p = o[:, None, :] + d[:, None, :] * z[:, :, None]          # sample.py:67, two roundings in float32
    dnorm = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    dl = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=z.device)], dim=1)
    delta = (dl * dnorm[:, None]).to(torch.float64)
    alpha = 1.0 - torch.exp(-sigma * delta)
    T = torch.cumprod(torch.cat([torch.ones((R, 1), dtype=torch.float64, device=z.device), 1.0 - alpha[:, :-1]], dim=1), dim=1)
    w = alpha * T
    v = field(densities, spec.density_scale, spec.density_pre_act)
    n = point_normals(v, p.reshape(-1, 3), spec.aabb).reshape(R, S, 3)
    N = (w[..., None] * n).sum(dim=1)
    return N, (w * z.to(torch.float64)).sum(dim=1), w.sum(dim=1)
