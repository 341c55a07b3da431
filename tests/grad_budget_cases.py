"""Case table of the per-voxel gradient check (numpy + the oracle only, no GPU), shared by tests/test_grad_budget_host.py (CPU:
the table's preconditions, the bite of the bound) and tests/test_hip_grad_per_voxel.py (GPU: every backward route).

A case is a grid, one or two cameras of the 100-view synthetic set (voxe_hip.workload; camera 3 is the bench camera, camera 38 an
oblique one), an image and a sample count.  The world box is [-1.5, 1.5]^3, jitter comes from the in-kernel stream (one case hands
the kernels a jitter tensor), the background is white.  Shapes are small and not trivial: several 8x8 pixel tiles, three depth
segments of 32 with a ragged end (S = 96 is six segments of 16 below 20 000 rays; S = 80 leaves a ragged 32-block), an odd-dimension
grid for the bricked gradient layout.

`reference(name, order)` holds, per upstream set ("colour": a colour gradient alone; "all": colour + depth + accumulated weight),
the oracle's gradient and the budget twin's (mag, budget, count) for it -- computed once and shared; nobody writes into them.
`corruptions(...)` are the three faults a global rel-L2 at 1e-4 does not see (a zeroed grid face, one lost trilinear corner of the
faint voxels, 0.1 % of the voxels scaled by 1.01)."""
import dataclasses
import functools

import numpy as np

import term_eps_cases as tc
from voxe_hip import abi
from voxe_hip.desc import make_render_cfg
from voxe_hip.workload import FAR, NEAR, RADIUS, focal_for, random_grid, sphere_grid, synth_pose_angles

from oracle import voxe_oracle as vo

AABB = [(-1.5, 1.5)] * 3
SETS = ("colour", "all")


@dataclasses.dataclass
class Case:
    name: str
    scene: str               # "random" | "sphere" | "odd" | "sh"
    scale: float = 2.0
    H: int = 64
    W: int = 64
    S: int = 96
    cams: tuple = (38,)      # more than one: K views in one launch (image_height set)
    post: int = abi.ACT_SOFTPLUS
    pre: int = abi.ACT_IDENTITY
    attn: bool = False
    deg: int = 0
    diffuse: bool = False
    clip: bool = False
    lindisp: bool = False
    jitter_seed: int = -1    # >= 0: a caller's jitter tensor U(0,1) [R,S] from this seed instead of the in-kernel stream
    eps: float = 0.0         # term_eps: the twin and the oracle get the cut tests/term_eps_cases.py derives
    seed: int = 42
    rng_offset: int = 7

    @property
    def rng(self):
        return (self.seed, self.rng_offset)

    @property
    def views(self):
        return len(self.cams)

    def cfg(self):
        return make_render_cfg(self.S, NEAR, FAR, perturb=True, white_bkgd=True, aabb_clip=self.clip, linear_disparity=self.lindisp,
                               sh_degree=self.deg, render_diffuse=self.diffuse, seed=self.seed, rng_offset=self.rng_offset)


ODD_DIMS, SH_DIMS = (37, 40, 33), (24, 20, 28)
_TABLE = [
    # the four scenes of the route table and the two sampling variants of the soft one
    Case("soft", "random", cams=(38,)),
    Case("dense", "random", scale=100.0 / 3.0, cams=(3,)),
    Case("sphere", "sphere", scale=100.0 / 3.0, cams=(38,)),
    Case("odd", "odd", H=56, W=72, S=80, cams=(3,)),
    Case("soft_clip", "random", clip=True, cams=(3,)),
    Case("soft_lindisp", "random", lindisp=True, cams=(3,)),
    # other fields, channel kinds and launches
    Case("relu", "random", scale=100.0 / 3.0, post=abi.ACT_RELU, cams=(3,)),
    Case("abs", "random", pre=abi.ACT_ABS, post=abi.ACT_IDENTITY, cams=(38,)),
    Case("attn", "random", attn=True, cams=(38,)),
    Case("jitter_tensor", "random", jitter_seed=7, cams=(3,)),
    Case("two_views", "random", cams=(3, 38)),
    Case("dense_eps1e-2", "random", scale=100.0 / 3.0, cams=(3,), eps=1e-2),
    # seven samples across an opaque field: INTERIOR samples saturate (om = 1 - alpha = 0 in float32 while e = exp(-x) is not), where
    # the reference's cumprod backward takes the product that leaves the sample out and a `suffix / om` form has nothing left
    Case("saturated", "random", scale=100.0 / 3.0, S=7, cams=(3,)),
    # view-dependent grids
    Case("sh1", "sh", H=48, W=48, S=64, deg=1),
    Case("sh2", "sh", H=48, W=48, S=64, deg=2),
    Case("sh3", "sh", H=48, W=48, S=64, deg=3),
    Case("sh2_diffuse", "sh", H=48, W=48, S=64, deg=2, diffuse=True),
]
CASES = {c.name: c for c in _TABLE}
SCENES = ("soft", "dense", "sphere", "odd", "soft_clip", "soft_lindisp")       # the rows every SH-0 route runs
SH_CASES = ("sh1", "sh2", "sh3", "sh2_diffuse")
# Preconditions per scene, checked on the oracle alone (tests/test_grad_budget_host.py), (densities, features) where two figures:
#   touched  share of the elements with budget > 0: at least 50 %;
#   exempt   share of the touched elements held only to the absolute floor (tests/helpers.py): at most 1 %;
#   tight    share of the touched elements whose bound lies below 1e-2 |ref|: at least 90 % / 99 % -- below that the GPU check would be
#            passing on slack.  (Measured: soft 92.3 - 93.0 % / 99.8 %, odd 90.2 - 90.7 % / 99.7 %, soft_lindisp 90.9 - 91.1 % / 99.8 %.)
# Three scenes cannot meet a figure for a reason of the scene itself; each floor sits just under what the oracle measures, so a change
# of the budget or of the scene that loosens the check further fails here:
#   dense      opaque within a few samples: behind the surface the block suffix divided by a tiny om dwarfs the gradient.  Densities
#              24.9 - 30.8 % tight (43 % with the uncertainties A, B, C alone).  Kept for its feature gradient and its faces.
#   sphere     opaque (scale 100/3: the scene the blindness of the global norm was measured on).  The exempt share is a property of mag
#              alone: the voxels behind the sphere are seen through exp(-66) and fall below 1e-20 x the largest mag -- 23.5 % of the
#              touched densities, 17.9 % of the touched feature values.  Outside the sphere x < 2^-26 and alpha = 0 exactly, so only
#              19.8 % of the feature values are touched at all.  Tight 52.4 - 53.9 % / 80.7 % (55.9 % / 82.3 % with A, B, C alone).
#   soft_clip  with the clipped range the closing 1e10 interval lies INSIDE the box: the last sample is opaque and every sample in front
#              of it carries the cancellation against its weight.  Densities 17.8 % tight under a colour gradient alone, 67 % with depth
#              and acc gradients (46 % / 75 % with A, B, C alone).
_DEFAULT_NEED = dict(touched=(0.50, 0.50), exempt=(0.01, 0.01), tight=(0.90, 0.99))
NEED = {name: dict(_DEFAULT_NEED) for name in SCENES}
NEED["dense"]["tight"] = (0.24, 0.99)
NEED["sphere"].update(touched=(0.50, 0.19), exempt=(0.24, 0.18), tight=(0.52, 0.80))
NEED["soft_clip"]["tight"] = (0.17, 0.99)


def case(name) -> Case:
    return CASES[name]


@functools.lru_cache(maxsize=None)
def grid_of(name):
    c = case(name)
    kind = abi.FEAT_ATTN if c.attn else abi.FEAT_SH
    F = 1 if c.attn else 3 * (c.deg + 1) ** 2
    if c.scene == "sphere":
        dens, feat = (t.numpy() for t in sphere_grid(48))
    elif c.scene == "random":
        dens, feat = (t.numpy() for t in random_grid(48, F))
    else:
        dims = ODD_DIMS if c.scene == "odd" else SH_DIMS
        rng = np.random.default_rng(61 + F)
        dens = rng.uniform(-1, 1, dims + (1,)).astype(np.float32)
        feat = rng.uniform(-1, 1, dims + (F,)).astype(np.float32)
    return vo.Grid(dens, feat, AABB, c.scale, c.pre, c.post, kind)


def pose(i, n=100):
    """(rot [3,3], eye [3]) of camera i of the n-view set, as tests/test_hip_configs.py builds them"""
    from thre3d_atom.utils.imaging_utils import pose_spherical

    p = pose_spherical(*synth_pose_angles(i, n), RADIUS)
    return p.rotation.numpy().astype(np.float32), p.translation.numpy().reshape(3).astype(np.float32)


def rays(c: Case):
    parts = [vo.cast_rays(c.H, c.W, focal_for(c.W), *pose(i)) for i in c.cams]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def reference(name, order="image"):
    """order "permuted": the same rays shuffled, as an unordered batch (the in-kernel jitter stream is indexed by a ray's position)"""
    c = case(name)
    grid, cfg = grid_of(name), c.cfg()
    o, d = rays(c)
    R = o.shape[0]
    rng = np.random.default_rng(_seed_of(name))
    gc = rng.standard_normal((R, grid.cout)).astype(np.float32)
    gdep = (0.2 * rng.standard_normal(R)).astype(np.float32)
    gacc = (0.2 * rng.standard_normal(R)).astype(np.float32)
    jit = np.random.default_rng(c.jitter_seed).uniform(0, 1, (R, c.S)).astype(np.float32) if c.jitter_seed >= 0 else None
    if order == "permuted":
        perm = rng.permutation(R)
        o, d, gc, gdep, gacc = (np.ascontiguousarray(a[perm]) for a in (o, d, gc, gdep, gacc))
        jit = None if jit is None else np.ascontiguousarray(jit[perm])
    cut = None
    if c.eps > 0:           # tests/term_eps_cases.py: the cut in float64 from the probe; rays it cannot decide carry no gradient
        T = tc.transmittance(vo.sample_probe(grid, cfg, o, d, jit), d)
        cut = tc.cut_of(T, c.eps)
        amb = tc.cut_of(T, c.eps * (1 + tc.DELTA)) != tc.cut_of(T, c.eps * (1 - tc.DELTA))
        assert amb.mean() <= tc.AMBIGUOUS_CAP and (cut < c.S).mean() >= tc.MIN_CUT_SHARE, (name, amb.mean(), (cut < c.S).mean())
        gc[amb], gdep[amb], gacc[amb] = 0.0, 0.0, 0.0
    out = dict(case=c, order=order, grid=grid, cfg=cfg, o=o, d=d, jit=jit, cut=cut, sets={},
               over=dict(image_width=c.W, image_height=c.H if c.views > 1 else 0) if order == "image" else dict(image_width=0))
    for which in SETS:
        if which == "all" and c.deg:        # view-dependent grids: colour gradients only, as everywhere in the suite
            continue
        up = dict(gc=gc, gdep=gdep if which == "all" else None, gacc=gacc if which == "all" else None)
        up["bwd"] = vo.render_bwd(grid, cfg, o, d, gc, d_depth=up["gdep"], d_acc=up["gacc"], jitter=jit, cut=cut)
        up["budget"] = vo.render_bwd_budget(grid, cfg, o, d, gc, d_depth=up["gdep"], d_acc=up["gacc"], jitter=jit, cut=cut)
        out["sets"][which] = up
    return out


def corruptions(ref_g, rng_seed=5):
    """{name: (corrupted copy of the gradient, mask of the elements it changed)} -- the three faults of a deposit kernel that a
    1e-4 rel-L2 passes: the x = X-1 plane zeroed, every element below 1e-4 x max loses one eighth (a trilinear corner), 0.1 % of
    the elements (of those below 1e-2 x max) scaled by 1.01"""
    out = {}
    g = ref_g.copy()
    g[-1] = 0.0
    out["zeroed_face"] = (g, (ref_g != 0) & (g == 0))
    faint = (np.abs(ref_g) < 1e-4 * float(np.abs(ref_g).max())) & (ref_g != 0)
    g = ref_g.copy()
    g[faint] *= np.float32(0.875)
    out["lost_eighth"] = (g, faint)
    # (drawn among the elements below 1e-2 x max: on the sphere a draw over all of them hits surface voxels that carry 1e-4 of the
    # gradient's energy each, which the norm does see: 1.5e-4)
    pick = (np.random.default_rng(rng_seed).random(ref_g.shape) < 1e-3) & (ref_g != 0) & (np.abs(ref_g) < 1e-2 * float(np.abs(ref_g).max()))
    g = ref_g.copy()
    g[pick] *= np.float32(1.01)
    out["scaled_1.01"] = (g, pick)
    return out


# ---- the checking functions of tests/test_hip_grad_per_voxel.py (importable without a GPU: the CPU mutation check feeds them) ------
def global_check(r, which, got, what=""):
    """what the suite asserted before: tests/test_hip_fuzz.py's _close (1e-4 rel-L2 + its absolute floor, x max(1, far) on the
    density gradient under a depth gradient)"""
    from test_hip_fuzz import _close

    up = r["sets"][which]
    for i, name in enumerate(("densities", "features")):
        ref_g = up["bwd"][i]
        err = float(np.linalg.norm(np.asarray(got[i], np.float64) - ref_g.astype(np.float64)))
        print(f"{r['case'].name} {what} {which} {name}: |err| {err:.3e}  |ref| {float(np.linalg.norm(ref_g)):.3e}")
        _close(name, got[i], ref_g, far=r["cfg"].far if (name == "densities" and up["gdep"] is not None) else 1.0)


@functools.lru_cache(maxsize=None)
def whole_ray_budget(name, order, which):
    """the twin with the whole ray as ONE block: the plain scatter kernel forms the suffix as `total - prefix` from the forward's outputs,
    its own, weaker, contract"""
    r = reference(name, order)
    up = r["sets"][which]
    return vo.render_bwd_budget(r["grid"], r["cfg"], r["o"], r["d"], up["gc"], d_depth=up["gdep"], d_acc=up["gacc"], jitter=r["jit"], cut=r["cut"],
                                segment=r["case"].S)


DET_BITS = 37       # the deterministic backward: 64-bit fixed point, the launch's largest contribution scaled to [2^37, 2^38)


def per_voxel(r, which, got, what="", route=""):
    """every density voxel and every feature value against its own bound; -> the exempt shares (densities, features).
    route "plain_scatter": the twin with the whole ray as one block; "deterministic": the fixed point's truncation on top"""
    from helpers import per_voxel_check

    up = r["sets"][which]
    budget = whole_ray_budget(r["case"].name, r["order"], which) if route == "plain_scatter" else up["budget"]
    return tuple(per_voxel_check(got[i], up["bwd"][i], *budget[name], f"{r['case'].name} {what} {which} {name}",
                                 fixed_point_bits=DET_BITS if route == "deterministic" else None)
                 for i, name in enumerate(("densities", "features")))


def check_gradients(r, which, got, what="", route=""):
    global_check(r, which, got, what)
    return per_voxel(r, which, got, what, route)
