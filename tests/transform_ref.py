"""Restatement of voxe_grid_resample (include/voxe.h) in torch on the CPU, written from the contract and not from
the kernel: float64 by default (the reference of the tests), float32 on request (the yardstick of the GPU tests: what the
same formula costs in the kernel's number format).  Also a float64 SH basis written from voxe_device.hpp, the analytic helpers
of the host tests and the inputs the host and GPU tests share."""
import numpy as np
import torch

REPLACE, UNION = 0, 1
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)


def sh_basis(degree, v):
    """[N, (degree+1)^2] float64, the renderer's basis (voxe_device.hpp sh_basis) at unit directions v [N,3]"""
    v = np.asarray(v, dtype=np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    b = [np.full_like(x, 0.28209479177387814)]
    if degree >= 1:
        b += [-(C1 * y), C1 * z, -(C1 * x)]
    if degree >= 2:
        b += [C2[0] * (x * y), C2[1] * (y * z), C2[2] * (2 * z * z - x * x - y * y), C2[3] * (x * z), C2[4] * (x * x - y * y)]
    if degree >= 3:
        xx, yy, zz = x * x, y * y, z * z
        b += [(C3[0] * y) * (3 * xx - yy), (C3[1] * x * y) * z, (C3[2] * y) * (4 * zz - xx - yy),
              (C3[3] * z) * (2 * zz - 3 * xx - 3 * yy), (C3[4] * x) * (4 * zz - xx - yy), (C3[5] * z) * (xx - yy),
              (C3[6] * x) * (xx - 3 * yy)]
    return np.stack(b, axis=-1)


def unit_directions(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def random_orthogonal(seed, det):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) * det < 0:
        q[:, 0] = -q[:, 0]
    return q


def rotation_about(axis, degrees):
    a, c, s = "xyz".index(axis), np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    i, j = (a + 1) % 3, (a + 2) % 3
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def quarter_turn(axis, n):
    """exact integer matrix of n quarter turns about an axis"""
    a = "xyz".index(axis)
    i, j = (a + 1) % 3, (a + 2) % 3
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][n % 4]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def mirror(axis):
    R = np.eye(3)
    R["xyz".index(axis), "xyz".index(axis)] = -1.0
    return R


def index_map(dims_s, lo_s, v_s, dims_d, lo_d, v_d, R, t, s):
    """(A, b) float64 of the contract's formula, from the lattices' low corners and voxel edges"""
    v_s, lo_s, v_d, lo_d, t = (np.asarray(a, dtype=np.float64) for a in (v_s, lo_s, v_d, lo_d, t))
    inv = np.asarray(R, dtype=np.float64).T / s
    # (the diagonal factors as element-wise products and quotients: v / v is exactly 1, which (1 / v) * v need not be)
    A = inv * v_d[None, :] / v_s[:, None]
    b = (inv @ (lo_d + 0.5 * v_d - t) - lo_s) / v_s - 0.5
    return A, b


def as_kernel_args(A, b):
    """what the kernel receives: the float32 casts, returned as float64 arrays holding exactly those values"""
    return np.asarray(A, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)


def rotate_coefficients(feat, blocks, degree):
    """[..., 3 ncoef] features -> rotated, c'_l = M_l c_l per colour channel and band (any float dtype of `feat`)"""
    n = (degree + 1) ** 2
    c = feat.reshape(*feat.shape[:-1], 3, n)
    out = c.clone()
    for l in range(1, degree + 1):
        band = slice(l * l, (l + 1) * (l + 1))
        M = torch.as_tensor(np.asarray(blocks[l]), dtype=feat.dtype)
        out[..., band] = torch.einsum("jk,...k->...j", M, c[..., band])
    return out.reshape(feat.shape)


def resample(src_d, src_f, dst_dims, A, b, blocks=None, sh_degree=-1, pre_abs=False, fill=0.0, mode=REPLACE, dst_d=None,
             dst_f=None, dtype=torch.float64):
    """The contract, every step in `dtype` (A, b: the values the kernel receives).  src_d [X,Y,Z,1] or None, src_f [X,Y,Z,C] or
    None.  Returns a dict: densities, features (None where the source has none), taken (bool), valid (bool), u [X2,Y2,Z2,3],
    new_density (the sample before the UNION choice)."""
    src = src_d if src_d is not None else src_f
    N = tuple(int(n) for n in src.shape[:3])
    A = torch.as_tensor(np.asarray(A), dtype=dtype)
    b = torch.as_tensor(np.asarray(b), dtype=dtype)
    grids = torch.meshgrid(*(torch.arange(n, dtype=dtype) for n in dst_dims), indexing="ij")
    u, i0, w = [], [], []
    for a in range(3):
        ua = A[a, 0] * grids[0]
        ua = ua + A[a, 1] * grids[1]
        ua = ua + A[a, 2] * grids[2]
        ua = ua + b[a]
        fl = torch.floor(ua)
        f = ua - fl
        u.append(ua)
        i0.append(torch.nan_to_num(fl, nan=-2.0).clamp(-2, N[a]).long())
        w.append((1 - f, f))
    dens = torch.zeros(tuple(dst_dims), dtype=dtype)
    feat = None if src_f is None else torch.zeros((*dst_dims, src_f.shape[-1]), dtype=dtype)
    valid = torch.ones(tuple(dst_dims), dtype=torch.bool)
    some = torch.zeros(tuple(dst_dims), dtype=torch.bool)
    none_inside = torch.ones(tuple(dst_dims), dtype=torch.bool)
    sd = None if src_d is None else src_d[..., 0].to(dtype)
    sf = None if src_f is None else src_f.to(dtype)
    for q in range(8):
        bits = (q & 1, (q >> 1) & 1, q >> 2)
        idx = [i0[a] + bits[a] for a in range(3)]
        inside = torch.ones(tuple(dst_dims), dtype=torch.bool)
        for a in range(3):
            inside &= (idx[a] >= 0) & (idx[a] < N[a])
        cl = [idx[a].clamp(0, N[a] - 1) for a in range(3)]
        t = (w[0][bits[0]] * w[1][bits[1]]) * w[2][bits[2]]
        nz = t != 0
        valid &= inside | ~nz
        some |= inside & nz
        none_inside &= ~inside
        if sd is not None:
            raw = sd[cl[0], cl[1], cl[2]]
            val = torch.where(inside, raw.abs() if pre_abs else raw, torch.full_like(raw, fill))
            dens = dens + val * t
        if sf is not None:
            val = torch.where(inside[..., None], sf[cl[0], cl[1], cl[2]], torch.zeros((), dtype=dtype))
            feat = feat + val * t[..., None]
    dens = torch.where(none_inside, torch.full_like(dens, fill), dens)
    if feat is not None:
        feat = torch.where(none_inside[..., None], torch.zeros((), dtype=dtype), feat)
        if sh_degree >= 1:
            feat = rotate_coefficients(feat, blocks, sh_degree)
    out = {"valid": valid, "u": torch.stack(u, dim=-1), "new_density": dens}
    if mode == UNION:
        old = dst_d[..., 0].to(dtype)
        take = valid & (dens > (old.abs() if pre_abs else old))
        out["taken"] = take
        out["densities"] = torch.where(take, dens, old)[..., None]
        out["features"] = None if feat is None else torch.where(take[..., None], feat, dst_f.to(dtype))
    else:
        out["taken"] = some
        out["densities"] = None if sd is None else dens[..., None]
        out["features"] = feat
    return out


def near_hull(u, src_dims, eps=1e-4):
    """bool [X2,Y2,Z2]: some component of u lies within eps of a value where a corner enters or leaves the source lattice or
    its weight becomes zero there (u = -1, 0, N-1, N)"""
    close = torch.zeros(u.shape[:-1], dtype=torch.bool)
    for a in range(3):
        for edge in (-1.0, 0.0, src_dims[a] - 1.0, float(src_dims[a])):
            close |= (u[..., a] - edge).abs() < eps
    return close


# ---- lattice-preserving maps: what numpy says the result is -------------------------------------------------------------------
def lattice_cases():
    """(name, R, integer voxel shift of the moved content along the destination axes)"""
    return [
        ("quarter_x", quarter_turn("x", 1), (1, -2, 0)),
        ("quarter_y", quarter_turn("y", 1), (0, 1, -1)),
        ("quarter_z", quarter_turn("z", 1), (-1, 0, 2)),
        ("half_z", quarter_turn("z", 2), (2, 1, 0)),
        ("three_quarter_y", quarter_turn("y", 3), (0, 0, 1)),
        ("mirror_x", mirror("x"), (1, 0, -1)),
        ("mirror_z", mirror("z"), (0, -1, 0)),
    ]


def permute_by(arr, R, shift, fill):
    """numpy's answer for a lattice-preserving map of a [X,Y,Z,C] array about the grid centre followed by a shift of `shift`
    voxels: transpose + flip (np.rot90 written out for any signed permutation) + shift with fill"""
    R = np.asarray(R)
    perm = [int(np.argmax(np.abs(R[a]))) for a in range(3)]
    out = np.transpose(arr, perm + [3])
    for a in range(3):
        if R[a, perm[a]] < 0:
            out = np.flip(out, axis=a)
    res = np.full_like(out, fill)
    src = [slice(max(0, -s), out.shape[a] - max(0, s)) for a, s in enumerate(shift)]
    dst = [slice(max(0, s), out.shape[a] - max(0, -s)) for a, s in enumerate(shift)]
    res[tuple(dst)] = out[tuple(src)]
    return np.ascontiguousarray(res)


def lattice_setup(dims, edges, R, shift):
    """destination dims / edges of the permuted lattice (both centred at the origin), t of the shift, and (A, b) in float64"""
    R = np.asarray(R, dtype=np.float64)
    perm = [int(np.argmax(np.abs(R[a]))) for a in range(3)]
    dims_d = tuple(dims[k] for k in perm)
    v_d = tuple(edges[k] for k in perm)
    t = tuple(shift[a] * v_d[a] for a in range(3))
    lo_s = tuple(-(n * e) / 2 for n, e in zip(dims, edges))
    lo_d = tuple(-(n * e) / 2 for n, e in zip(dims_d, v_d))
    A, b = index_map(dims, lo_s, edges, dims_d, lo_d, v_d, R, t, 1.0)
    return dims_d, v_d, t, A, b
