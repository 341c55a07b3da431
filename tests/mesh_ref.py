"""Vectorised numpy restatement of the mesh export ("Mesh export"), test infrastructure for
tests/test_mesh_host.py and tests/test_mesh_gpu.py.  It uses the generated case table (voxe_hip.mc_table) and the same
float32 arithmetic, operation for operation, as vox-e_amd/csrc/voxe_mesh.hip, so that the GPU output can be compared
face for face and nearly bit for bit.  Also the mesh checks (closedness, Euler characteristic, volume, area)."""
import numpy as np

from voxe_hip import abi
from voxe_hip.mc_table import edge_corners, table

_TAB = table()
K = max(len(t) for t in _TAB)
TRI_COUNT = np.array([len(t) for t in _TAB], dtype=np.int64)
TRI_EDGES = np.full((256, K, 3), -1, dtype=np.int64)
for _c, _tris in enumerate(_TAB):
    for _i, _t in enumerate(_tris):
        TRI_EDGES[_c, _i] = _t
# cube edge e -> (offset of its owning node (base corner) inside the cell, axis)
EDGE_OFF = np.array([[(edge_corners(e)[0] >> a) & 1 for a in range(3)] for e in range(12)], dtype=np.int64)
EDGE_AXIS = np.array([e >> 2 for e in range(12)], dtype=np.int64)


def post_act(post, v):
    v = np.asarray(v, dtype=np.float64)
    if post == abi.ACT_SOFTPLUS:
        return np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 20.0))))
    if post == abi.ACT_RELU:
        return np.maximum(v, 0.0)
    return v


def iso_value(post, level):
    """L = post^-1(level) as a float32 (the library takes level as a float, computes in double and rounds once); None when
    level <= post(0)"""
    level = float(np.float32(level))
    if post == abi.ACT_SOFTPLUS:
        if not level > float(np.float32(np.log(2.0))):   # softplus(0) in float32
            return None
        return np.float32(level if level > 20.0 else np.log(np.expm1(level)))
    if not level > 0.0:
        return None
    return np.float32(level)


def node_values(raw, scale, pre, mask=None):
    """v = pre(scale * raw) per voxel in float32, 0 outside the mask, zero-padded by one node per side"""
    v = np.asarray(raw, dtype=np.float32).reshape(np.shape(raw)[:3]) * np.float32(scale)
    if pre == abi.ACT_ABS:
        v = np.abs(v)
    if mask is not None:
        v = np.where(np.asarray(mask).reshape(v.shape) != 0, v, np.float32(0.0)).astype(np.float32)
    return np.pad(v, 1)


def extract(raw, aabb, level, scale=1.0, pre=abi.ACT_IDENTITY, post=abi.ACT_IDENTITY, mask=None):
    """-> vertices [V,3] float32, faces [T,3] int32 (same numbering as the library)"""
    L = iso_value(post, level)
    assert L is not None, "level <= post(0)"
    P = node_values(raw, scale, pre, mask)
    ins = P > L
    S = P.shape
    # crossing +x/+y/+z edges per node
    emask = np.zeros(S, dtype=np.int64)
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        cr = ins[tuple(lo)] != ins[tuple(hi)]
        emask[tuple(lo)] |= cr.astype(np.int64) << a
    emask = emask.reshape(-1)
    vcount = (emask & 1) + ((emask >> 1) & 1) + ((emask >> 2) & 1)
    vbase = np.concatenate([[0], np.cumsum(vcount)[:-1]])
    # vertices, numbered by (node, axis): id = vbase[node] + number of crossing edges of the node on lower axes
    strides = np.array([S[1] * S[2], S[2], 1], dtype=np.int64)
    Pf = P.reshape(-1)
    V = int(vcount.sum())
    verts = np.zeros((V, 3), dtype=np.float32)
    for a in range(3):
        nn = np.nonzero((emask >> a) & 1)[0]
        below = emask[nn] & ((1 << a) - 1)
        ids = vbase[nn] + (below & 1) + ((below >> 1) & 1)
        va = Pf[nn]
        vb = Pf[nn + strides[a]]
        t = (L - va) / (vb - va)
        idx = np.stack([nn // strides[0], (nn // strides[1]) % S[1], nn % S[2]], axis=1) - 1   # lattice index -1..N
        u = idx.astype(np.float32)
        u[:, a] = u[:, a] + t
        verts[ids] = world(u, aabb, np.shape(raw)[:3])
    # cells: min node at lattice -1..N-1
    case = np.zeros((S[0] - 1, S[1] - 1, S[2] - 1), dtype=np.int64)
    for c in range(8):
        ox, oy, oz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= ins[ox:ox + S[0] - 1, oy:oy + S[1] - 1, oz:oz + S[2] - 1].astype(np.int64) << c
    cell_nodes = (np.arange(S[0] - 1)[:, None, None] * strides[0] + np.arange(S[1] - 1)[None, :, None] * strides[1]
                  + np.arange(S[2] - 1)[None, None, :]).reshape(-1)
    case = case.reshape(-1)
    cnt = TRI_COUNT[case]
    cells = np.repeat(np.arange(len(case)), cnt)
    slot = np.arange(len(cells)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    edges = TRI_EDGES[case[cells], slot]                                 # [T,3] cube edges
    owner = cell_nodes[cells][:, None] + (EDGE_OFF[edges] * strides).sum(-1)
    ax = EDGE_AXIS[edges]
    below = emask[owner] & ((1 << ax) - 1)
    faces = vbase[owner] + (below & 1) + ((below >> 1) & 1)
    return verts.astype(np.float32), faces.astype(np.int32)


def world(u, aabb, dims):
    """index-space u -> world: f32(lo) + (u + 0.5f) * ((f32(hi) - f32(lo)) / N), per axis, in float32"""
    out = np.empty_like(u, dtype=np.float32)
    for a in range(3):
        lo, hi = np.float32(aabb[a][0]), np.float32(aabb[a][1])
        step = (hi - lo) / np.float32(dims[a])
        out[:, a] = lo + (u[:, a] + np.float32(0.5)) * step
    return out


# ---- mesh checks -------------------------------------------------------------------------------------------------------
def is_closed(faces):
    """every undirected edge an even number of times; each directed edge as often as its reverse"""
    f = np.asarray(faces, dtype=np.int64)
    if len(f) == 0:
        return True
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    fwd = d[:, 0] * n + d[:, 1]
    rev = d[:, 1] * n + d[:, 0]
    keys, counts = np.unique(fwd, return_counts=True)
    rkeys, rcounts = np.unique(rev, return_counts=True)
    if not (np.array_equal(keys, rkeys) and np.array_equal(counts, rcounts)):
        return False
    und = np.unique(np.minimum(fwd, rev), return_counts=True)[1]
    return bool(np.all(und % 2 == 0))


def euler_characteristic(faces):
    f = np.asarray(faces, dtype=np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    E = len(np.unique(e[:, 0] * (int(f.max()) + 1) + e[:, 1]))
    V = len(np.unique(f))
    return V - E + len(f)


def volume(verts, faces):
    """signed enclosed volume (divergence theorem); > 0 for outward-facing normals"""
    p = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def area(verts, faces):
    p = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum() / 2.0)


def grid_points(n, lo=-1.0, hi=1.0):
    """voxel-centre coordinates of an n^3 grid over [lo, hi]^3 -> x, y, z [n,n,n] float64"""
    ax = (np.arange(n) + 0.5) / n * (hi - lo) + lo
    return np.meshgrid(ax, ax, ax, indexing="ij")


def sphere_field(n, r0, centre=(0.0, 0.0, 0.0), lo=-1.0, hi=1.0):
    x, y, z = grid_points(n, lo, hi)
    return (1.0 - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) / r0).astype(np.float32)


def torus_field(n, R=0.55, r=0.22, lo=-1.0, hi=1.0):
    """1 - dist(p, circle of radius R in the xy plane) / (2 r): level 0.5 is the torus of tube radius r"""
    x, y, z = grid_points(n, lo, hi)
    d = np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z)
    return (1.0 - d / (2.0 * r)).astype(np.float32)
