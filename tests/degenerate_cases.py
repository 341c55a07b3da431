"""Case table of the degenerate ray geometry (numpy only, no GPU): axis-aligned views, samples exactly on voxel planes and on AABB
faces, exact ties between march axes, cameras on a face / on a lattice point inside the box, launches in which no ray meets the
grid, 1xN / Nx1 / 1x1 images.  Every number of the lattice grid and of its cameras is exact in float32, so a float64 restatement
and a float32 kernel have to agree on every floor().

`case(name)` returns a Case; its first ten fields are (grid, cfg kwargs, H, W, focal, rot, eye, S, near, far).  `rays(case)` casts
the rays with the oracle (pixel centres are j + 0.5: an odd W or H gives a central column / row with dx / dy exactly 0),
`jitter_of(case)` gives the caller's jitter tensor of the one case that has one, `check_preconditions(case)` asserts on the ORACLE
alone that the case still is what its name says (so that a later edit cannot turn it generic without anyone noticing).

Preconditions per case (Case.need):
  integer_u   inside samples whose index coordinate u is an exact integer on some axis (footprint weights exactly 0 and 1)
  half_u      inside samples with u an exact half-integer on all three axes (weights exactly 0.5: a voxel corner)
  on_face     samples exactly on an AABB face, all of which the strict test must call outside
  zero_dir    rays with a direction component that is exactly 0
  tie         the central ray's |d| components named here are equal bit for bit
  miss        no ray has an inside sample: acc = 0, colour = background, exact-zero gradients
The axis cameras' bounds (>= 1000 integer-u samples, >= 100 on-face samples) are the issue's; the measured counts are 3 100 - 4 000
and 380 - 710.  Bounds of the smaller images follow from one ray: a ray that crosses the whole box along z has 65 samples half a
voxel apart, 32 of them (the odd ones) on a voxel-centre plane and inside, and its first and last sample on a face."""
import dataclasses
import functools
from typing import Optional

import numpy as np

from voxe_hip import abi
from voxe_hip.desc import make_render_cfg, norm_constants

from oracle import voxe_oracle as vo

H_IMG, W_IMG, FOCAL = 17, 25, 16.0
LATTICE_DIMS, LATTICE_AABB = (16, 8, 32), [(-2.0, 2.0), (-1.0, 1.0), (-4.0, 4.0)]      # voxel size 0.25
GENERIC_DIMS, GENERIC_AABB = (16, 12, 20), [(-2.0, 2.0)] * 3                            # voxel sizes 0.25 / 0.333 / 0.2
STEP = 0.125                                                                            # sample spacing: half a lattice voxel
SH_CASES = ("axis-z", "axis+x", "tie_xy", "eye_on_face", "all_miss")
SIDE_CASES = ("axis-z", "axis-z_clip", "tie_xy", "all_miss")


@dataclasses.dataclass
class Case:
    grid: vo.Grid
    kw: dict
    H: int
    W: int
    focal: float
    rot: np.ndarray          # [3,3], or [K,3,3] for K views in one launch
    eye: np.ndarray          # [3] / [K,3]
    S: int
    near: float
    far: float
    name: str = ""
    jitter_seed: Optional[int] = None        # a caller's jitter tensor U(0,1) [R,S] from this seed
    need: dict = dataclasses.field(default_factory=dict)

    def __iter__(self):
        return iter((self.grid, self.kw, self.H, self.W, self.focal, self.rot, self.eye, self.S, self.near, self.far))

    @property
    def views(self):
        return 1 if self.rot.ndim == 2 else self.rot.shape[0]

    @property
    def rng(self):
        return (int(self.kw.get("seed", 0)), int(self.kw.get("rng_offset", 0)))

    def cfg(self, **over):
        return make_render_cfg(self.S, self.near, self.far, **{**self.kw, **over})


def _grid(dims, aabb, relu=False, features=3, seed=18):
    rng = np.random.default_rng(seed)
    dens = rng.uniform(-1, 1, dims + (1,)).astype(np.float32)
    feat = rng.uniform(-1, 1, dims + (features,)).astype(np.float32)
    if relu:
        return vo.Grid(dens, feat, aabb, 100.0 / 3.0, abi.ACT_IDENTITY, abi.ACT_RELU)
    return vo.Grid(dens, feat, aabb, 2.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS)      # translucent: rays integrate through the whole box


def lattice_grid(relu=False, features=3):
    return _grid(LATTICE_DIMS, LATTICE_AABB, relu, features)


def generic_grid():
    return _grid(GENERIC_DIMS, GENERIC_AABB, seed=19)


def look(fwd, up):
    """rotation [right, up, -fwd] as columns: the camera looks down -z_cam"""
    fwd, up = np.asarray(fwd, np.float32), np.asarray(up, np.float32)
    right = np.cross(fwd, up).astype(np.float32)
    return np.stack([right, up, -fwd], axis=1).astype(np.float32)


def axis_camera(axis, sign, aabb):
    """the eye on the +-axis at hi + 2, looking at the centre: a signed permutation matrix; (rot, eye, near, far, S)"""
    hi = aabb[axis][1]
    extent = aabb[axis][1] - aabb[axis][0]
    eye = np.zeros(3, np.float32)
    eye[axis] = sign * (hi + 2.0)
    fwd = np.zeros(3, np.float32)
    fwd[axis] = -sign
    up = np.zeros(3, np.float32)
    up[1 if axis == 2 else 2] = 1.0
    rot = look(fwd, up)
    assert np.array_equal(np.abs(rot).sum(0), np.ones(3)) and np.array_equal(np.abs(rot).sum(1), np.ones(3))
    return rot, eye, 2.0, 2.0 + extent, int(round(extent / STEP)) + 1


_AXES = {"x": 0, "y": 1, "z": 2}
_LATTICE_NEED = dict(integer_u=1000, on_face=100, zero_dir=H_IMG + W_IMG - 1)


def _axis_case(name, grid=None, h=H_IMG, w=W_IMG, need=None, **kw):
    axis, sign = _AXES[name[5]], (1.0 if name[4] == "+" else -1.0)
    rot, eye, near, far, S = axis_camera(axis, sign, LATTICE_AABB)
    return Case(grid or lattice_grid(), kw, h, w, FOCAL, rot, eye, S, near, far, need=dict(_LATTICE_NEED if need is None else need))


def _build(name):
    if name in ("axis+x", "axis-x", "axis+y", "axis-y", "axis+z", "axis-z"):
        return _axis_case(name, white_bkgd=name[4] == "+")
    if name == "axis-z_relu":
        return _axis_case(name, grid=lattice_grid(relu=True))
    if name == "axis-z_clip":
        # the clipped range of a ray starts and ends ON the faces it crosses (measured: 3 718 face samples)
        return _axis_case(name, need=dict(on_face=100, zero_dir=H_IMG + W_IMG - 1), aabb_clip=True)
    if name == "axis-z_lindisp":
        return _axis_case(name, need=dict(zero_dir=H_IMG + W_IMG - 1), linear_disparity=True)
    if name == "axis-z_jitter":      # jitter removes the lattice hits and keeps the zero direction components
        c = _axis_case(name, need=dict(zero_dir=H_IMG + W_IMG - 1), perturb=True)
        c.jitter_seed = 7
        return c
    if name == "axis-z_hash":        # the in-kernel counter-hash jitter stream
        return _axis_case(name, need=dict(zero_dir=H_IMG + W_IMG - 1), perturb=True, seed=5, rng_offset=9)
    if name in ("eye_on_face", "eye_on_face_clip"):
        # o_z == hi_z: (hi - o) == 0 in the slab test; sample 0 of every ray is the eye itself, on the face, outside
        rot, _, _, _, _ = axis_camera(2, 1.0, LATTICE_AABB)
        return Case(lattice_grid(), dict(aabb_clip=name.endswith("clip")), H_IMG, W_IMG, FOCAL, rot, np.array([0, 0, 4.0], np.float32),
                    65, 0.0, 8.0, need=dict(on_face=H_IMG * W_IMG, integer_u=1000, zero_dir=H_IMG + W_IMG - 1))
    if name in ("eye_inside_corner", "eye_inside_corner_clip"):
        # a voxel corner (every coordinate a multiple of the voxel size): sample 0 has u half-integer on all three axes
        rot, _, _, _, _ = axis_camera(2, 1.0, LATTICE_AABB)
        return Case(lattice_grid(), dict(aabb_clip=name.endswith("clip"), white_bkgd=True), H_IMG, W_IMG, FOCAL, rot,
                    np.array([0.5, -0.25, 1.0], np.float32), 41, 0.0, 5.0, need=dict(half_u=H_IMG * W_IMG, zero_dir=H_IMG + W_IMG - 1))
    if name == "tie_xy":
        c = np.float32(np.sqrt(0.5))
        return Case(lattice_grid(), {}, 17, 17, FOCAL, look([-c, -c, 0], [0, 0, 1]), np.array([3, 3, 0], np.float32), 49, 1.0, 7.0,
                    need=dict(tie=(0, 1), zero_dir=17))
    if name == "tie_xy_relu":
        c = _build("tie_xy")
        c.grid = lattice_grid(relu=True)
        return c
    if name == "tie_xyz":
        c = np.float32(np.sqrt(1.0 / 3.0))
        up = (np.array([-1, -1, 2]) / np.sqrt(6.0)).astype(np.float32)
        return Case(lattice_grid(), dict(white_bkgd=True), 17, 17, FOCAL, look([-c, -c, -c], up), np.array([3, 3, 3], np.float32), 49, 1.0, 7.0,
                    need=dict(tie=(0, 1, 2)))
    if name in ("all_miss", "all_miss_clip"):
        # the axis-z camera behind the box, looking away from it
        rot, _, near, far, S = axis_camera(2, 1.0, LATTICE_AABB)
        return Case(lattice_grid(), dict(aabb_clip=name.endswith("clip"), white_bkgd=name.endswith("clip")), H_IMG, W_IMG, FOCAL, rot,
                    np.array([0, 0, -6.0], np.float32), S, near, far, need=dict(miss=True, zero_dir=H_IMG + W_IMG - 1))
    if name == "row_image":
        return _axis_case("axis-z", h=1, need=dict(integer_u=32 * 5, on_face=2 * 5, zero_dir=W_IMG))
    if name == "col_image":
        return _axis_case("axis-z", w=1, need=dict(integer_u=32 * 5, on_face=2 * 5, zero_dir=H_IMG))
    if name == "one_pixel":
        return _axis_case("axis-z", h=1, w=1, need=dict(integer_u=32, on_face=2, zero_dir=1))
    if name == "six_views":
        # pixel tiles of different march axes share one launch (image_width = 25, image_height = 17, K = 6)
        cams = [axis_camera(a, s, GENERIC_AABB) for a in range(3) for s in (1.0, -1.0)]
        return Case(generic_grid(), dict(white_bkgd=True), H_IMG, W_IMG, FOCAL, np.stack([c[0] for c in cams]),
                    np.stack([c[1] for c in cams]), 33, 2.0, 6.0, need=dict(zero_dir=6 * (H_IMG + W_IMG - 1), integer_u=1000, on_face=100))
    raise KeyError(name)


NAMES = ("axis+x", "axis-x", "axis+y", "axis-y", "axis+z", "axis-z", "axis-z_relu", "axis-z_clip", "axis-z_lindisp", "axis-z_jitter",
         "axis-z_hash", "eye_on_face", "eye_on_face_clip", "eye_inside_corner", "eye_inside_corner_clip", "tie_xy", "tie_xy_relu",
         "tie_xyz", "all_miss", "all_miss_clip", "row_image", "col_image", "one_pixel", "six_views")


def case(name) -> Case:
    c = _build(name)
    c.name = name
    return c


def rays(c: Case):
    if c.views == 1:
        return vo.cast_rays(c.H, c.W, c.focal, c.rot, c.eye)
    parts = [vo.cast_rays(c.H, c.W, c.focal, c.rot[k], c.eye[k]) for k in range(c.views)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def jitter_of(c: Case):
    if c.jitter_seed is None:
        return None
    return np.random.default_rng(c.jitter_seed).uniform(0, 1, (c.views * c.H * c.W, c.S)).astype(np.float32)


def index_coords(grid: vo.Grid, p):
    """u [..., 3] float32 of world points p [..., 3] float32, with footprint()'s operation order"""
    scale, bias = norm_constants(grid.aabb)
    dims = grid.densities.shape[:3]
    f = np.float32
    return np.stack([(((p[..., a] * scale[a] + bias[a]) + f(1.0)) * f(dims[a]) - f(1.0)) * f(0.5) for a in range(3)], axis=-1).astype(f)


def sample_facts(c: Case, o, d, probe):
    """counts of the exact lattice events among the oracle's samples"""
    p = (o[:, None, :] + d[:, None, :] * probe["z"][:, :, None]).astype(np.float32)       # sample.py:67
    u = index_coords(c.grid, p)
    inside = probe["inside"]
    lo = np.array([r[0] for r in c.grid.aabb], np.float32)
    hi = np.array([r[1] for r in c.grid.aabb], np.float32)
    face = ((p == lo) | (p == hi)).any(-1) & (p >= lo).all(-1) & (p <= hi).all(-1)
    return dict(integer_u=int((inside & (u == np.floor(u)).any(-1)).sum()),
                half_u=int((inside & (u - np.floor(u) == np.float32(0.5)).all(-1)).sum()),
                on_face=int(face.sum()), on_face_inside=int((face & inside).sum()),
                zero_dir=int((d == 0).any(-1).sum()), inside=int(inside.sum()))


def check_preconditions(c: Case, o=None, d=None, probe=None):
    if o is None:
        o, d = rays(c)
    if probe is None:
        probe = vo.sample_probe(c.grid, c.cfg(), o, d, jitter_of(c))
    facts = sample_facts(c, o, d, probe)
    for key in ("integer_u", "half_u", "on_face", "zero_dir"):
        assert facts[key] >= c.need.get(key, 0), (c.name, key, facts[key], c.need.get(key, 0))
    assert facts["on_face_inside"] == 0, (c.name, facts)            # the strict p > lo && p < hi test
    if "tie" in c.need:
        mid = d[(c.H // 2) * c.W + c.W // 2]
        mags = np.abs(mid[list(c.need["tie"])])
        assert c.H % 2 == 1 and c.W % 2 == 1 and np.all(mags == mags[0]) and mags[0] > 0, (c.name, mid)
        if len(c.need["tie"]) == 2:
            assert mid[3 - sum(c.need["tie"])] == 0, (c.name, mid)
    if c.need.get("miss"):
        assert facts["inside"] == 0, (c.name, facts)
    else:
        assert facts["inside"] >= 16 * c.views, (c.name, facts)
    return facts


@functools.lru_cache(maxsize=None)
def sh_grid(deg):
    """the lattice grid's shape with 12 / 27 / 48 feature channels"""
    return lattice_grid(features=3 * (deg + 1) ** 2)
