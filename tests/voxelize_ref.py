"""Numpy restatement of the mesh import, test infrastructure for tests/test_voxelize_host.py and
tests/test_voxelize_gpu.py.  The inside / outside decision is integer arithmetic exactly as include/voxe.h specifies it; the
distance is float32 in the operation order of vox-e_amd/csrc/voxe_voxelize.hip (dtype=np.float64 evaluates the same formulas in
double, for error bounds); then the density and feature mapping of thre3d_reprs.mesh.mesh_to_voxel_grid."""
import numpy as np

from voxe_hip import abi

FRAC = 8
ONE = 1 << FRAC
RANGE = 1024.0
DIST_CHUNK = (8, 8, 64)
SIGN_CHUNK = (16, 64)
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
C0 = 0.28209479177387814


def lattice(dims, aabb):
    """float32 (lo, step) per axis, as the library computes them"""
    lo = np.array([np.float32(a[0]) for a in aabb], dtype=np.float32)
    hi = np.array([np.float32(a[1]) for a in aabb], dtype=np.float32)
    return lo, ((hi - lo) / np.array(dims, dtype=np.float32)).astype(np.float32)


def snap(vertices, dims, aabb):
    """-> q [V,3] int64 (rint(256 u), u = (p - lo) / step - 0.5 in float32), ok [V] (|u| < 1024 on every axis)"""
    lo, step = lattice(dims, aabb)
    with np.errstate(all="ignore"):
        u = (np.asarray(vertices, dtype=np.float32).reshape(-1, 3) - lo) / step - np.float32(0.5)
        ok = np.all(np.abs(u) < np.float32(RANGE), axis=1)   # (False for NaN)
        q = np.where(ok[:, None], np.rint(u * np.float32(ONE)), 0.0).astype(np.int64)
    return q, ok


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest(A, B, C, P):
    """closest point of triangles (A, B, C) to points P (broadcast, [...,3], one dtype) by Voronoi regions -> d^2, v, w with the
    point A + v AB + w AC"""
    one, zero = A.dtype.type(1), A.dtype.type(0)
    ab, ac, ap, bp, cp = B - A, C - A, P - A, P - B, P - C
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    with np.errstate(all="ignore"):
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e43 / (e43 + e56)
        denom = one / ((va + vb) + vc)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        z, o = np.zeros_like(d1), np.ones_like(d1)
        v = np.select(conds, [z, o, v_ab, z, z, one - w_bc], vb * denom)
        w = np.select(conds, [z, z, z, o, w_ac, w_bc], vc * denom)
        diff = P - ((A + ab * v[..., None]) + ac * w[..., None])
        return _dot(diff, diff), v, w


def _chunks(lo, hi, size):
    return 0 if hi < lo else (hi - lo) // size + 1


def _centres(idx, lo, step, dtype):
    """voxel centres lo + (i + 0.5) step of integer indices [...,3]"""
    return lo.astype(dtype) + (idx.astype(dtype) + dtype(0.5)) * step.astype(dtype)


def voxelize(vertices, faces, colours, dims, aabb, h, dtype=np.float32):
    """-> dict(sdf, nearest, colours, inside, stats, d2): what voxe_voxelize_mesh writes, plus d2 (the winning squared distance,
    inf outside the band).  dtype=np.float64: the same distance formulas in double on the float32 inputs (sign and boxes are
    integer either way)."""
    dtype = np.dtype(dtype).type
    X, Y, Z = (int(d) for d in dims)
    verts = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, T = len(verts), len(faces)
    h32 = np.float32(h)
    out_col = np.zeros((X, Y, Z, 3), dtype=np.float32)
    if T == 0:
        return dict(sdf=np.full((X, Y, Z), h32, dtype=np.float32), nearest=np.full((X, Y, Z), -1, dtype=np.int32), colours=out_col,
                    inside=np.zeros((X, Y, Z), dtype=np.uint8), stats=np.zeros(4, dtype=np.int64),
                    d2=np.full((X, Y, Z), np.inf))
    lo, step = lattice(dims, aabb)
    q_all, ok_all = snap(verts, dims, aabb)
    with np.errstate(all="ignore"):
        r = [int(min(np.ceil(h32 / s), np.float32(2048))) for s in step]
    h2 = dtype(h32) * dtype(h32)
    N = (X, Y, Z)
    keys_d2 = np.full(N, np.inf, dtype=dtype)          # (d^2, id) minimum, lexicographic: the 64-bit key of the kernel
    keys_id = np.full(N, -1, dtype=np.int64)
    counters = np.zeros((X + 1, Y, Z), dtype=np.int64)
    malformed = items = 0
    fverts = verts.astype(dtype)
    for t in range(T):
        ids = faces[t]
        if np.any(ids < 0) or np.any(ids >= V) or not np.all(ok_all[ids]):
            malformed += 1
            continue
        ids = np.sort(ids)
        q = q_all[ids]
        e1, e2 = q[1] - q[0], q[2] - q[0]
        nrm = (int(e1[1]) * int(e2[2]) - int(e1[2]) * int(e2[1]), int(e1[2]) * int(e2[0]) - int(e1[0]) * int(e2[2]),
               int(e1[0]) * int(e2[1]) - int(e1[1]) * int(e2[0]))
        if nrm == (0, 0, 0):
            continue
        mn, mx = q.min(axis=0), q.max(axis=0)
        d0 = [max(0, int(mn[a] >> FRAC) - r[a]) for a in range(3)]
        d1 = [min(N[a] - 1, int(-((-mx[a]) >> FRAC)) + r[a]) for a in range(3)]
        s0 = [max(0, int(-((-mn[a]) >> FRAC))) for a in (1, 2)]
        s1 = [min(N[a] - 1, int(mx[a] >> FRAC)) for a in (1, 2)]
        # ---- sign: columns the triangle covers, crossing charged to the first voxel at or behind it ----
        if nrm[0] != 0:
            items += _chunks(s0[0], s1[0], SIGN_CHUNK[0]) * _chunks(s0[1], s1[1], SIGN_CHUNK[1])
            if s1[0] >= s0[0] and s1[1] >= s0[1]:
                A, B, C = (np.array([p[1], p[2], p[0]], dtype=np.int64) for p in q)
                area = nrm[0]
                if area < 0:
                    B, C, area = C, B, -area
                j, k = np.meshgrid(np.arange(s0[0], s1[0] + 1), np.arange(s0[1], s1[1] + 1), indexing="ij")
                py, pz = j.astype(np.int64) * ONE, k.astype(np.int64) * ONE
                cover = np.ones(j.shape, dtype=bool)
                E = []
                for S, D in ((B, C), (C, A), (A, B)):
                    dy, dz = int(D[0] - S[0]), int(D[1] - S[1])
                    e = dy * (pz - S[1]) - dz * (py - S[0])
                    cover &= (e > 0) | ((e == 0) & bool(dz < 0 or (dz == 0 and dy > 0)))
                    E.append(e)
                num = E[0] * A[2] + E[1] * B[2] + E[2] * C[2]
                i = np.clip(-((-num) // (area * ONE)), 0, X)
                np.add.at(counters, (i[cover], j[cover], k[cover]), 1)
        # ---- distance: cells of the dilated box ----
        items += np.prod([_chunks(d0[a], d1[a], DIST_CHUNK[a]) for a in range(3)])
        if all(d1[a] >= d0[a] for a in range(3)):
            sl = tuple(slice(d0[a], d1[a] + 1) for a in range(3))
            idx = np.stack(np.meshgrid(*[np.arange(d0[a], d1[a] + 1) for a in range(3)], indexing="ij"), axis=-1)
            dd, _, _ = closest(fverts[ids[0]], fverts[ids[1]], fverts[ids[2]], _centres(idx, lo, step, dtype))
            with np.errstate(invalid="ignore"):
                take = (dd <= h2) & ((dd < keys_d2[sl]) | ((dd == keys_d2[sl]) & (t < keys_id[sl])))
            keys_d2[sl] = np.where(take, dd, keys_d2[sl])
            keys_id[sl] = np.where(take, t, keys_id[sl])
    run = np.cumsum(counters, axis=0)
    inside = (run[:X] & 1).astype(np.uint8)
    odd = int((run[X] & 1).sum())
    band = keys_id >= 0
    d = np.where(band, np.minimum(np.sqrt(np.where(band, keys_d2, 0)), dtype(h32)), dtype(h32))
    sdf = np.where(inside != 0, -d, d)
    if colours is not None and band.any():
        cols = np.asarray(colours, dtype=np.float32).reshape(-1, 3).astype(dtype)
        where = np.argwhere(band)
        tri = np.sort(faces[keys_id[band]], axis=1)
        _, v, w = closest(fverts[tri[:, 0]], fverts[tri[:, 1]], fverts[tri[:, 2]], _centres(where, lo, step, dtype))
        u = (dtype(1) - v) - w
        out_col = out_col.astype(dtype)
        out_col[band] = (cols[tri[:, 0]] * u[:, None] + cols[tri[:, 1]] * v[:, None]) + cols[tri[:, 2]] * w[:, None]
    stats = np.array([odd, malformed, int(band.sum()), int(items)], dtype=np.int64)
    return dict(sdf=sdf.astype(dtype), nearest=keys_id.astype(np.int32), colours=out_col, inside=inside, stats=stats,
                d2=keys_d2)


# ---- density and feature mapping (thre3d_reprs.mesh.mesh_to_voxel_grid) ---------------------------------------------------------
def iso_value(post, level):
    """L = post^-1(level) in float32; None when level <= post(0)"""
    level = float(np.float32(level))
    if post == abi.ACT_SOFTPLUS:
        if not level > float(np.float32(np.log(2.0))):
            return None
        return np.float32(level if level > 20.0 else np.log(np.expm1(level)))
    return np.float32(level) if level > 0.0 else None


def fields(sdf, nearest, colours, h, L, pre, post, scale, sh_degree, inside_ratio=2.0):
    """-> raw densities [X,Y,Z,1], features [X,Y,Z,3 (deg+1)^2] in float32: v = L - (L - e) clamp(sd / h, -(ratio - 1), 1),
    raw = v / scale; DC feature logit(clamp(c, 1/510, 1 - 1/510)) / C0 inside the band, every other feature 0"""
    if post == abi.ACT_SOFTPLUS and pre == abi.ACT_ABS:
        raise ValueError("no empty value")
    e = np.float32(-20.0 if post == abi.ACT_SOFTPLUS else 0.0)
    L = np.float32(L)
    if not L > e:
        raise ValueError("level at or below the empty value")
    s = np.clip(np.asarray(sdf, dtype=np.float32) / np.float32(h), np.float32(-(inside_ratio - 1.0)), np.float32(1.0))
    v = L - (L - e) * s
    raw = (v / np.float32(scale)).astype(np.float32)[..., None]
    ncoef = (sh_degree + 1) ** 2
    feats = np.zeros((*np.shape(sdf), 3 * ncoef), dtype=np.float32)
    band = np.asarray(nearest) >= 0
    c = np.clip(np.asarray(colours, dtype=np.float64), 1.0 / 510.0, 1.0 - 1.0 / 510.0)
    dc = np.log(c / (1.0 - c)) / C0
    for ch in range(3):
        feats[..., ch * ncoef] = np.where(band, dc[..., ch], 0.0)
    return raw, feats


# ---- analytic test bodies -----------------------------------------------------------------------------------------------------
def box_mesh(lo, hi, sub=1):
    """closed, outward-wound triangle mesh of the axis-aligned box [lo, hi], each face cut into sub x sub quads of two triangles
    -> vertices [V,3] float32, faces [T,3] int32 (vertices shared between faces)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    index, verts, faces = {}, [], []

    def vid(p):
        key = tuple(np.round(p, 9))
        if key not in index:
            index[key] = len(verts)
            verts.append(p)
        return index[key]

    for ax in range(3):
        a1, a2 = (ax + 1) % 3, (ax + 2) % 3
        for side in (0, 1):
            for i in range(sub):
                for j in range(sub):
                    corner = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = np.empty(3)
                        p[ax] = hi[ax] if side else lo[ax]
                        p[a1] = lo[a1] + (hi[a1] - lo[a1]) * (i + di) / sub
                        p[a2] = lo[a2] + (hi[a2] - lo[a2]) * (j + dj) / sub
                        corner.append(vid(p))
                    quad = corner if side else corner[::-1]   # (a1, a2, ax) is right-handed: counter-clockwise seen from +ax
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int32)


def point_mesh_distance(points, verts, faces):
    """float64 distance of every point to the mesh (brute force) -> [N]"""
    p = np.asarray(points, dtype=np.float64)
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    best = np.full(len(p), np.inf)
    for lo_ in range(0, len(f), 256):
        tri = f[lo_:lo_ + 256]
        dd, _, _ = closest(v[tri[:, 0]][None], v[tri[:, 1]][None], v[tri[:, 2]][None], p[:, None, :])
        best = np.minimum(best, np.nanmin(dd, axis=1))
    return np.sqrt(best)


def trilinear(grid, aabb, points):
    """float64 trilinear interpolant of grid [X,Y,Z,C] (values at voxel centres, clamped at the border) at world points [N,3]"""
    dims = np.array(grid.shape[:3])
    lo, step = lattice(dims, aabb)
    u = (np.asarray(points, dtype=np.float64) - lo) / step - 0.5
    i0 = np.floor(u).astype(np.int64)
    t = u - i0
    out = np.zeros((len(u), grid.shape[-1]))
    for c in range(8):
        o = np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])
        idx = np.clip(i0 + o, 0, dims - 1)
        out += np.prod(np.where(o == 1, t, 1 - t), axis=1)[:, None] * grid[idx[:, 0], idx[:, 1], idx[:, 2]]
    return out


# ---- the meshes of the tests ------------------------------------------------------------------------------------------------------
AABB = [(-1.0, 1.0)] * 3
N20 = (20, 20, 20)


def position_colours(verts, aabb=AABB):
    lo, hi = np.array([a[0] for a in aabb]), np.array([a[1] for a in aabb])
    return np.clip((np.asarray(verts, dtype=np.float64) - lo) / (hi - lo), 0.0, 1.0).astype(np.float32)


def body_fields():
    """name -> (20^3 field, level): the analytic bodies whose marching-cubes meshes the tests import"""
    import mesh_ref

    return {"sphere": (mesh_ref.sphere_field(20, 0.6), 0.25), "torus": (mesh_ref.torus_field(20), 0.5),
            "offcentre": (mesh_ref.sphere_field(20, 0.5, (0.17, -0.12, 0.08)), 0.3)}


def body_mesh(name):
    import mesh_ref

    field, level = body_fields()[name]
    return mesh_ref.extract(field[..., None], AABB, level)


# the lattice cubes in index space [lo, hi) per axis: faces exactly on voxel centres / exactly on voxel boundaries
CUBES = {"cube_centres": ((5.0, 5.0, 5.0), (13.0, 13.0, 13.0)), "cube_bounds": ((4.5, 5.5, 6.5), (12.5, 13.5, 14.5))}


def cube_mesh(name, sub):
    lo, hi = CUBES[name]
    world = lambda u: (np.array(u) + 0.5) * 0.1 - 1.0   # noqa: E731  (exact enough: the snap takes rint(256 u))
    return box_mesh(world(lo), world(hi), sub)


def cube_cells(name):
    """the voxels of a lattice cube: centres with lo <= i < hi per axis (a centre on a face belongs to the side x + eps falls
    on, on every axis)"""
    lo, hi = CUBES[name]
    ax = [np.arange(20) for _ in range(3)]
    i, j, k = np.meshgrid(*ax, indexing="ij")
    inside = np.ones(N20, dtype=bool)
    for a, c in enumerate((i, j, k)):
        inside &= (c >= lo[a]) & (c < hi[a])
    return inside.astype(np.uint8)


def gpu_cases():
    """name -> (vertices, faces, colours or None, dims, aabb, h) of tests/test_voxelize_gpu.py"""
    out = {}
    for name in ("sphere", "torus", "offcentre"):
        v, f = body_mesh(name)
        out[name] = (v, f, position_colours(v), N20, AABB, 0.2)
    for name in CUBES:
        v, f = cube_mesh(name, 2)
        out[name] = (v, f, position_colours(v), N20, AABB, 0.15)
    # one tetrahedron across an anisotropic lattice: large triangles, many work items each
    aabb = [(-1.0, 1.0), (-0.6, 0.9), (-1.5, 1.0)]
    v = np.array([[-0.9, -0.5, -1.4], [0.9, -0.45, -1.2], [-0.2, 0.85, -1.3], [0.1, 0.1, 0.95]], dtype=np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32)
    out["tetrahedron"] = (v, f, position_colours(v, aabb), (16, 12, 20), aabb, 0.3)
    # spheres that leave the lattice through two of its faces: box clipping, crossings in front of and behind the grid
    sv, sf = body_mesh("sphere")
    v = (sv * np.float32(1.3) + np.array([-0.7, 0.1, 0.75], dtype=np.float32)).astype(np.float32)
    out["sphere_out"] = (v, sf, position_colours(v), N20, AABB, 0.2)
    # ... the same with a radius of 590 voxels about u = (-400, 10, -400): vertices up to |u| = 990 of the admissible 1024
    # (u = 10 p + 9.5 here)
    v = (sv * np.float32(59.0 / 0.45) + np.array([-40.95, 0.05, -40.95], dtype=np.float32)).astype(np.float32)
    out["sphere_huge"] = (v, sf, position_colours(v), N20, AABB, 0.2)
    # zero-area and repeated-vertex triangles among the sphere's
    rng = np.random.default_rng(5)
    v = np.concatenate([sv, [sv[10] + (sv[20] - sv[10]) * np.float32(2.0)]]).astype(np.float32)   # (a copy-free extra vertex)
    extra = [[3, 3, 7], [9, 4, 4], [5, 5, 5], [10, 20, 10], [8, 1, 8]]
    extra += [[int(a), int(a), int(b)] for a, b in rng.integers(0, len(sv), (5, 2))]
    f = np.concatenate([sf[:300], np.array(extra, dtype=np.int32), sf[300:]]).astype(np.int32)
    out["degenerate"] = (v, f, position_colours(v), N20, AABB, 0.2)
    out["empty"] = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, (12, 13, 14), AABB, 0.25)
    # a dimension of 65: the cells of a work item along z do not fill whole waves
    aabb = [(-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.6)]
    v, f = box_mesh((-0.7, -0.6, -0.8), (0.6, 0.7, 1.35), 1)
    out["z65"] = (v, f, None, (12, 14, 65), aabb, 0.25)
    return out
