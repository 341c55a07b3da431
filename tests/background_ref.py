"""Restatement of the environment-map background (include/voxe.h) in torch, float64 by default, and the inputs
the tests share.  Nothing here comes from the library: the forward is written with differentiable torch ops (so autograd gives a
second opinion on the gradients), `analytic_gradients` writes the header's chain rule out by hand, and `directions_from_uv` builds
ray directions that land on chosen map coordinates."""
import math

import torch

MAPS = ((2, 2), (4, 8), (5, 7))          # (He, We): 2 x 2 has every tap wrapped or clamped
RAY_COUNTS = (1, 63, 64, 65, 4096)


def angles(d):
    """(phi, theta, r2, usable) of directions [R,3]; phi = 0 where dx = dy = 0, usable = finite and not of zero length"""
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    usable = torch.isfinite(d).all(dim=1) & ((d * d).sum(dim=1) > 0)
    safe = torch.where(usable[:, None], d, torch.tensor([1.0, 0.0, 0.0], dtype=d.dtype, device=d.device).expand_as(d))
    dx, dy, dz = safe[:, 0], safe[:, 1], safe[:, 2]
    r2 = dx * dx + dy * dy
    axis = r2 == 0
    # (atan2 and sqrt have no finite derivative on the axis: evaluate them off it, then put the convention's values in)
    dx_ = torch.where(axis, torch.ones_like(dx), dx)
    phi = torch.where(axis, torch.zeros_like(dx), torch.atan2(dy, dx_))
    r = torch.sqrt(torch.where(axis, torch.ones_like(r2), r2))
    theta = torch.where(axis, torch.where(dz > 0, torch.zeros_like(dz), torch.full_like(dz, math.pi)), torch.atan2(r, dz))
    return phi, theta, r2, usable


def map_coords(d, He, We):
    """(u, v, usable) of directions [R,3]"""
    phi, theta, _, usable = angles(d)
    return (phi / (2 * math.pi) + 0.5) * We - 0.5, (theta / math.pi) * He - 0.5, usable


def taps(u, v, He, We):
    """(rows [R,2], columns [R,2], fx, fy, x0, y0): the four taps of every ray; fx / fy keep the graph of u / v"""
    x0, y0 = torch.floor(u.detach()), torch.floor(v.detach())
    fx, fy = u - x0, v - y0
    x0, y0 = x0.long(), y0.long()
    cols = torch.stack([x0 % We, (x0 + 1) % We], dim=1)
    rows = torch.stack([y0.clamp(0, He - 1), (y0 + 1).clamp(0, He - 1)], dim=1)
    return rows, cols, fx, fy, x0, y0


def background(texels, d):
    """b [R,3] = sigmoid(bilinear(E)) at directions d; 0 for unusable directions"""
    He, We = texels.shape[:2]
    u, v, usable = map_coords(d, He, We)
    rows, cols, fx, fy, _, _ = taps(u, v, He, We)
    e00, e01 = texels[rows[:, 0], cols[:, 0]], texels[rows[:, 0], cols[:, 1]]
    e10, e11 = texels[rows[:, 1], cols[:, 0]], texels[rows[:, 1], cols[:, 1]]
    fx, fy = fx[:, None], fy[:, None]
    t = (1 - fx) * (1 - fy) * e00 + fx * (1 - fy) * e01 + (1 - fx) * fy * e10 + fx * fy * e11
    return torch.sigmoid(t) * usable[:, None].to(t.dtype)


def composite(colour, acc, d, texels, dtype=torch.float64):
    """out [R,3] = colour + (1 - acc) b, every input converted to `dtype` first"""
    colour, acc, d, texels = (t.to(dtype) for t in (colour, acc, d, texels))
    return colour + (1 - acc.reshape(-1, 1)) * background(texels, d)


def autograd_gradients(colour, acc, d, texels, g):
    """(out, d_acc [R], d_texels, d_rays_d) of (composite * g).sum() by float64 autograd"""
    acc64 = acc.double().reshape(-1).clone().requires_grad_(True)
    d64 = d.double().clone().requires_grad_(True)
    t64 = texels.double().clone().requires_grad_(True)
    out = composite(colour, acc64, d64, t64)
    d_acc, d_d, d_t = torch.autograd.grad((out * g.double()).sum(), (acc64, d64, t64), allow_unused=True)
    zero = lambda x, like: torch.zeros_like(like) if x is None else x
    return out.detach(), zero(d_acc, acc64), zero(d_t, t64), torch.nan_to_num(zero(d_d, d64), nan=0.0, posinf=0.0, neginf=0.0)


@torch.no_grad()
def analytic_gradients(acc, d, texels, g):
    """(d_acc [R], d_texels, d_rays_d, s [R,3]) by the header's formulas, float64"""
    acc, d, E, g = acc.double().reshape(-1), d.double(), texels.double(), g.double()
    He, We = E.shape[:2]
    u, v, usable = map_coords(d, He, We)
    rows, cols, fx, fy, _, _ = taps(u, v, He, We)
    e = [[E[rows[:, j], cols[:, i]] for i in (0, 1)] for j in (0, 1)]       # e[row][column]
    fx_, fy_ = fx[:, None], fy[:, None]
    w = [[(1 - fx_) * (1 - fy_), fx_ * (1 - fy_)], [(1 - fx_) * fy_, fx_ * fy_]]
    t = sum(w[j][i] * e[j][i] for j in (0, 1) for i in (0, 1))
    ok = usable[:, None].double()
    b = torch.sigmoid(t) * ok
    d_acc = -(g * b).sum(dim=1)
    s = (1 - acc)[:, None] * g * b * (1 - b) * ok
    d_E = torch.zeros_like(E)
    for j in (0, 1):
        for i in (0, 1):
            d_E.index_put_((rows[:, j], cols[:, i]), w[j][i] * s, accumulate=True)
    d_u = (We / (2 * math.pi)) * (s * ((1 - fy_) * (e[0][1] - e[0][0]) + fy_ * (e[1][1] - e[1][0]))).sum(dim=1)
    d_v = (He / math.pi) * (s * ((1 - fx_) * (e[1][0] - e[0][0]) + fx_ * (e[1][1] - e[0][1]))).sum(dim=1)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    r2 = dx * dx + dy * dy
    on = usable & (r2 > 0)
    r2s = torch.where(on, r2, torch.ones_like(r2))
    r, n2 = torch.sqrt(r2s), r2s + dz * dz
    zero = torch.zeros_like(dx)
    dphi = torch.stack([-dy / r2s, dx / r2s, zero], dim=1)
    dtheta = torch.stack([dx * dz / r, dy * dz / r, -r], dim=1) / n2[:, None]
    d_d = torch.where(on[:, None], d_u[:, None] * dphi + d_v[:, None] * dtheta, torch.zeros_like(d))
    return d_acc, d_E, d_d, s


def directions_from_uv(u, v, He, We, length=None):
    """float64 directions [R,3] that map to (u, v): u in [-0.5, We - 0.5), v in (-0.5, He - 0.5); scaled by `length` [R]"""
    u, v = torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(v, dtype=torch.float64)
    phi = ((u + 0.5) / We - 0.5) * (2 * math.pi)
    theta = (v + 0.5) / He * math.pi
    d = torch.stack([torch.sin(theta) * torch.cos(phi), torch.sin(theta) * torch.sin(phi), torch.cos(theta)], dim=1)
    return d if length is None else d * torch.as_tensor(length, dtype=torch.float64)[:, None]


# ---- the inputs of the agreement tests ----------------------------------------------------------------------------------------
def tap_kinds(x0, y0, He, We):
    """per ray: column kind (0 interior, 1 x0 == -1, 2 x0 == We - 1) and row kind (0 interior, 1 y0 == -1, 2 y0 == He - 1)"""
    ck = torch.where(x0 == -1, 1, torch.where(x0 == We - 1, 2, 0))
    rk = torch.where(y0 == -1, 1, torch.where(y0 == He - 1, 2, 0))
    return ck, rk


def agreement_case(He, We, R, seed=0):
    """(texels, d, colour, acc, g, u, v) on the CPU, float32 (u, v float64: what d was built from).  (u, v) cycle through every
    cell of the extended map x0 in [-1, We - 1], y0 in [-1, He - 1] -- the wrap column from both sides and both clamped rows --
    with fractions in [0.05, 0.95]; directions have lengths in [0.25, 4]; acc holds exact 0 and 1, g all-zero rows."""
    gen = torch.Generator().manual_seed(1000 * He + 10 * We + R + seed)
    k = torch.arange(R) + int(torch.randint(0, 1 << 20, (1,), generator=gen))
    cx, cy = k % (We + 1) - 1, (k // (We + 1)) % (He + 1) - 1
    fu = 0.05 + 0.9 * torch.rand(R, generator=gen, dtype=torch.float64)
    fv = 0.05 + 0.9 * torch.rand(R, generator=gen, dtype=torch.float64)
    # (the extended cells at the rim are half cells: u in [-0.5, We - 0.5), v in (-0.5, He - 0.5))
    u = torch.where(cx == -1, -0.45 + 0.4 * fu, torch.where(cx == We - 1, We - 0.95 + 0.4 * fu, cx + fu))
    v = torch.where(cy == -1, -0.45 + 0.4 * fv, torch.where(cy == He - 1, He - 0.95 + 0.4 * fv, cy + fv))
    length = 0.25 * 16.0 ** torch.rand(R, generator=gen, dtype=torch.float64)
    d = directions_from_uv(u, v, He, We, length).float()
    texels = torch.randn(He, We, 3, generator=gen) * 1.5
    colour = torch.rand(R, 3, generator=gen)
    acc = torch.rand(R, generator=gen)
    g = torch.randn(R, 3, generator=gen)
    if R >= 8:
        acc[0::7], acc[3::7] = 0.0, 1.0
        g[5::11] = 0.0
    return texels, d, colour, acc, g, u, v


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ---- contention cases: (texels, d, colour, acc, g) on the CPU, float32 ----------------------------------------------------------
def _contention(He, We, d, seed):
    gen = torch.Generator().manual_seed(seed)
    R = d.shape[0]
    return (torch.randn(He, We, 3, generator=gen), d.float().contiguous(), torch.rand(R, 3, generator=gen),
            torch.rand(R, generator=gen) * 0.9, torch.randn(R, 3, generator=gen))


def one_cell_case(R=4096, He=4, We=8):
    """every ray in the cell (x0, y0) = (5, 2)"""
    gen = torch.Generator().manual_seed(7)
    u = 5 + 0.05 + 0.9 * torch.rand(R, generator=gen, dtype=torch.float64)
    v = 2 + 0.05 + 0.9 * torch.rand(R, generator=gen, dtype=torch.float64)
    return _contention(He, We, directions_from_uv(u, v, He, We), 8)


def two_cell_case(R=4096, He=4, We=8):
    """rays alternate between the cells (5, 2) and (1, 0): a run is broken at every lane"""
    gen = torch.Generator().manual_seed(9)
    odd = torch.arange(R) % 2 == 1
    u = torch.where(odd, 1.0, 5.0) + 0.05 + 0.9 * torch.rand(R, generator=gen, dtype=torch.float64)
    v = torch.where(odd, 0.0, 2.0) + 0.05 + 0.9 * torch.rand(R, generator=gen, dtype=torch.float64)
    return _contention(He, We, directions_from_uv(u, v, He, We), 10)


def camera_directions(hw, focal, yaw=0.7, pitch=0.4):
    """directions [hw * hw, 3] of a pinhole camera in image order (rows of pixels), float64, not normalised"""
    ys, xs = torch.meshgrid(torch.arange(hw, dtype=torch.float64), torch.arange(hw, dtype=torch.float64), indexing="ij")
    cam = torch.stack([(xs + 0.5 - hw / 2) / focal, -(ys + 0.5 - hw / 2) / focal, -torch.ones_like(xs)], dim=-1).reshape(-1, 3)
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    rot = torch.tensor([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]], dtype=torch.float64) @ \
        torch.tensor([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]], dtype=torch.float64)
    return cam @ rot.T


def camera_case(hw=48, He=4, We=8):
    """a 48 x 48 camera in image order into a 4 x 8 map: long runs of lanes per cell"""
    return _contention(He, We, camera_directions(hw, 1.2 * hw), 11)


def run_lengths(d, He, We):
    """lengths of the runs of consecutive rays that share a cell"""
    u, v, _ = map_coords(d.double(), He, We)
    key = torch.floor(u) * 1000 + torch.floor(v)
    change = torch.nonzero(key[1:] != key[:-1]).reshape(-1) + 1
    edges = torch.cat([torch.zeros(1, dtype=torch.long), change, torch.tensor([len(key)])])
    return edges[1:] - edges[:-1]
