"""Case table of the gradient truncation (VoxeRenderCfg::term_eps; numpy + the oracle only, no GPU), shared by
tests/test_oracle_term_eps.py (CPU) and tests/test_hip_term_eps.py (GPU).

The rule under test (include/voxe.h): sample k of a ray receives its exact gradient iff the transmittance in front of it,
T_k (accumulate.py's exclusive cumprod, T_0 = 1), is >= term_eps.  The oracle does not read term_eps: for every case this module
works out, from the oracle's sample probe alone,
  T[r,k]   in float64: sigma masked by `inside`, delta = diff(z) * |d| (the last, infinite, delta never enters an exclusive sum),
           T = exp(-exclusive cumsum(sigma * delta));
  cut(eps) the first k with T[r,k] < eps, S when there is none; the reference gradient is vo.render_bwd(..., cut=cut(eps));
  ambiguous rays: cut(eps * (1 + DELTA)) != cut(eps * (1 - DELTA)), DELTA = 1e-3.  A float32 running product of at most S factors,
           each a few ulp off between the three exp implementations (libm expf, the kernels' fast exp, float64 here), is within
           4 * 6e-8 * S ~ 3e-5 relative at S = 128; DELTA is 30 x that.  The upstream gradients (colour, depth, acc) of those rays
           are ZERO: they contribute nothing whichever side of the threshold a kernel lands on.

`check_conditions(ref)` asserts what makes a case worth running (and returns the figures):
  - at most 5 % of the rays are ambiguous (a cap: faint fields, where T hovers around the threshold, are unsuitable inputs);
  - at least 25 % of the rays are cut (cut < S) and at least 5 % are not;
  - with the launch's depth-segment length L (16 up to 20 000 rays, 32 above: VOXE_SEG16_MAX_RAYS), the non-ambiguous cut rays include
    cuts with cut % L == 0 (a segment that is skipped by its saved start state), == 1 and == L - 1;
  - sensitivity: |G(cut) - G(cut - 1)| and |G(cut) - G(min(cut + 1, S))|, the cut moved on the cut rays only, are each at least 10 x
    the tolerance the GPU comparison allows (tests/test_hip_fuzz.py's _close: 1e-4 |ref| + 5e-5, x max(1, far) for the density
    gradient under a depth gradient), on densities and on features: an off-by-one kernel fails the comparison, shown on the reference
    alone.  The same holds with the cut moved ONLY on the rays cut at k % L = 0, at 1 and at L - 1 (six figures per tensor; measured
    23 x and more): an off-by-one confined to a segment-start skip or to a segment's last sample fails too.
    The eps = 1e-3 cases (the realistic setting, Case.realistic) are EXEMPT from these sensitivity conditions: one sample at
    T ~ 1e-3 moves the gradient by 1.5e-4 ... 9e-4 rel-L2, which no 1e-4 comparison can be 10 x away from; they are kept as the
    setting the trainers use.

Scenes: a 32^3 grid on [-1,1]^3, densities U(-1,1), features U(-2,2); post-activation softplus with scale 100/3 ("sp") or ReLU
with scale 20 ("relu"): dense fields, a ray's transmittance crosses the threshold within a few samples.  Cameras at distance 3 looking
at the centre, focal 1.2 W, near / far 1.5 / 4.5, jitter on (the in-kernel stream; one case hands the kernels a jitter tensor)."""
import dataclasses
import functools

import numpy as np

from voxe_hip import abi
from voxe_hip.desc import make_render_cfg

from oracle import voxe_oracle as vo

DELTA = 1e-3
AMBIGUOUS_CAP, MIN_CUT_SHARE, MIN_UNCUT_SHARE, MARGIN_FACTOR = 0.05, 0.25, 0.05, 10.0
SEG16_MAX_RAYS = 20000          # VOXE_SEG16_MAX_RAYS (csrc/voxe_render_common.hpp)
DIMS, AABB, NEAR, FAR, DIST = (32, 32, 32), [(-1.0, 1.0)] * 3, 1.5, 4.5, 3.0
EYES = {"a": (0.55, 0.40, 0.73), "b": (-0.20, 0.91, 0.36), "c": (0.80, -0.58, 0.15)}       # eye directions (normalised below)


@dataclasses.dataclass
class Case:
    name: str
    field: str               # "sp" | "relu"
    S: int
    eps: float
    clip: bool = False
    hw: int = 40
    eyes: tuple = ("a",)     # more than one: K views in one launch (image_height set)
    attn: bool = False       # attention grid (one feature channel, one output channel)
    white: bool = True
    seed: int = 3
    jitter_seed: int = -1    # >= 0: a caller's jitter tensor U(0,1) [R,S] from this seed instead of the in-kernel stream

    @property
    def realistic(self):
        return self.eps <= 1e-3

    @property
    def views(self):
        return len(self.eyes)

    @property
    def rng(self):
        return (self.seed, 11)

    @property
    def R(self):
        return self.views * self.hw * self.hw

    @property
    def seg_len(self):
        return 16 if self.R <= SEG16_MAX_RAYS else 32

    def cfg(self, deg=0, **over):
        kw = dict(perturb=True, aabb_clip=self.clip, white_bkgd=self.white, seed=self.rng[0], rng_offset=self.rng[1], sh_degree=deg)
        return make_render_cfg(self.S, NEAR, FAR, **{**kw, **over})


_TABLE = [
    Case("sp_s64_e0.1", "sp", 64, 0.1),
    Case("relu_s97_clip_e0.5", "relu", 97, 0.5, clip=True, eyes=("b",), white=False),
    Case("sp_s33_e0.5", "sp", 33, 0.5, eyes=("c",)),
    Case("relu_s64_e0.5", "relu", 64, 0.5, eyes=("c",), white=False),
    Case("sp_s97_clip_e0.1", "sp", 97, 0.1, clip=True),
    Case("relu_s64_clip_e0.1", "relu", 64, 0.1, clip=True, eyes=("b",)),
    Case("attn_relu_s64_e0.1", "relu", 64, 0.1, attn=True, eyes=("b",)),
    Case("sp_s64_jitter_tensor_e0.1", "sp", 64, 0.1, eyes=("c",), jitter_seed=7),
    Case("sp_s64_e1e-3", "sp", 64, 1e-3),
    Case("sp_s97_clip_e1e-3", "sp", 97, 1e-3, clip=True, eyes=("b",)),
    Case("two_views_s64_e0.5", "sp", 64, 0.5, eyes=("a", "c")),
    Case("big_144_s64_e0.1", "sp", 64, 0.1, hw=144),
]
CASES = {c.name: c for c in _TABLE}
NAMES = tuple(CASES)
ROUTE_CASES = ("sp_s64_e0.1", "relu_s97_clip_e0.5", "sp_s33_e0.5", "sp_s64_e1e-3")      # both eps, clip on / off, S 64 / 97 / 33
SH_CASES = ("sp_s64_e0.1", "relu_s97_clip_e0.5", "sp_s64_e1e-3")


def case(name) -> Case:
    return CASES[name]


@functools.lru_cache(maxsize=None)
def grid_of(field, attn=False, deg=0):
    """the one density tensor of a field with 3 (SH-0), 1 (attention) or 3 (deg + 1)^2 feature channels"""
    rng = np.random.default_rng(29)
    dens = rng.uniform(-1, 1, DIMS + (1,)).astype(np.float32)
    F = 1 if attn else 3 * (deg + 1) ** 2
    feat = np.random.default_rng(31 + F).uniform(-2, 2, DIMS + (F,)).astype(np.float32)
    kind = abi.FEAT_ATTN if attn else abi.FEAT_SH
    if field == "relu":
        return vo.Grid(dens, feat, AABB, 20.0, abi.ACT_IDENTITY, abi.ACT_RELU, kind)
    return vo.Grid(dens, feat, AABB, 100.0 / 3.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, kind)


def camera(eye_dir):
    """(rot, eye): at distance DIST along eye_dir, looking at the origin; columns of rot are [right, up, -forward]"""
    e = np.asarray(eye_dir, np.float64)
    e = e / np.linalg.norm(e)
    fwd = -e
    up = np.array([0.0, 0.0, 1.0]) - fwd[2] * fwd
    up = up / np.linalg.norm(up)
    right = np.cross(fwd, up)
    return np.stack([right, up, -fwd], axis=1).astype(np.float32), (DIST * e).astype(np.float32)


def rays(c: Case):
    parts = [vo.cast_rays(c.hw, c.hw, 1.2 * c.hw, *camera(EYES[k])) for k in c.eyes]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def transmittance(probe, d):
    """T [R,S] float64 in front of every sample, from the oracle's probe"""
    sigma = np.where(probe["inside"], probe["sigma"].astype(np.float64), 0.0)
    dnorm = np.linalg.norm(d.astype(np.float64), axis=1)
    delta = np.diff(probe["z"].astype(np.float64), axis=1) * dnorm[:, None]
    x = np.cumsum(sigma[:, :-1] * delta, axis=1)
    return np.exp(-np.concatenate([np.zeros((x.shape[0], 1)), x], axis=1))


def cut_of(T, eps):
    below = T < eps
    return np.where(below.any(1), below.argmax(1), T.shape[1]).astype(np.int32)


def tolerance(ref_g, far=1.0):
    """what tests/test_hip_fuzz.py's _close allows on |got - ref|"""
    return 1e-4 * float(np.linalg.norm(ref_g)) + 5e-5 * max(1.0, float(far))


def _seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def reference(name, order="image", deg=0, diffuse=False):
    """everything the comparisons of one case need, computed once on the oracle and shared (nobody writes into it).  order
    "permuted": the same rays shuffled, as an unordered batch -- the in-kernel jitter stream is indexed by a ray's position, so
    T, the cuts and the ambiguous set are worked out for that order anew"""
    c = case(name)
    grid = grid_of(c.field, c.attn, deg)
    cfg = c.cfg(deg, render_diffuse=diffuse)
    o, d = rays(c)
    R = o.shape[0]
    rng = np.random.default_rng(_seed_of(name))
    gc = rng.standard_normal((R, grid.cout)).astype(np.float32)
    side = not deg          # view-dependent grids: colour gradients only
    gdep = (0.2 * rng.standard_normal(R)).astype(np.float32) if side else None
    gacc = (0.2 * rng.standard_normal(R)).astype(np.float32) if side else None
    jit = np.random.default_rng(c.jitter_seed).uniform(0, 1, (R, c.S)).astype(np.float32) if c.jitter_seed >= 0 else None
    if order == "permuted":
        perm = rng.permutation(R)
        o, d, gc = (np.ascontiguousarray(a[perm]) for a in (o, d, gc))
        jit = None if jit is None else np.ascontiguousarray(jit[perm])
        if side:
            gdep, gacc = np.ascontiguousarray(gdep[perm]), np.ascontiguousarray(gacc[perm])
    probe = vo.sample_probe(grid, cfg, o, d, jit)
    T = transmittance(probe, d)
    cut = cut_of(T, c.eps)
    amb = cut_of(T, c.eps * (1 + DELTA)) != cut_of(T, c.eps * (1 - DELTA))
    gc[amb] = 0.0
    if side:
        gdep[amb] = 0.0
        gacc[amb] = 0.0
    out = dict(case=c, grid=grid, cfg=cfg, deg=deg, o=o, d=d, jit=jit, gc=gc, gdep=gdep, gacc=gacc, probe=probe, T=T, cut=cut, amb=amb,
               over=dict(image_width=c.hw, image_height=c.hw if c.views > 1 else 0) if order == "image" else dict(image_width=0))
    out["bwd"] = bwd_with_cut(out, cut)
    out["tol"] = (tolerance(out["bwd"][0], FAR if side else 1.0), tolerance(out["bwd"][1]))
    return out


def bwd_with_cut(ref, cut):
    return vo.render_bwd(ref["grid"], ref["cfg"], ref["o"], ref["d"], ref["gc"], d_depth=ref["gdep"], d_acc=ref["gacc"], jitter=ref["jit"],
                         cut=cut)


def margins(ref):
    """(|G(cut) - G(cut - 1)|, |G(cut) - G(min(cut + 1, S))|) per tensor, the cut moved on the cut rays only; cached in ref"""
    if "margins" not in ref:
        cut, S = ref["cut"], ref["case"].S
        is_cut = cut < S
        ref["margins"] = tuple(_moved(ref, m) for m in (np.where(is_cut, np.maximum(cut - 1, 0), cut), np.where(is_cut, np.minimum(cut + 1, S), cut)))
    return ref["margins"]


def _moved(ref, cut):
    g = bwd_with_cut(ref, cut.astype(np.int32))
    return tuple(float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64))) for a, b in zip(g, ref["bwd"]))


def boundary_margins(ref):
    """{(k % L, +-1): per-tensor |G(cut) - G(cut +- 1)|}, the cut moved ONLY on the non-ambiguous rays cut at k % L = 0, 1, L - 1: what
    an off-by-one confined to a segment-start skip or to the last sample of a segment would change; cached in ref"""
    if "boundary_margins" not in ref:
        cut, S, L = ref["cut"], ref["case"].S, ref["case"].seg_len
        out = {}
        for res in (0, 1, L - 1):
            sel = (cut < S) & (cut > 0) & (cut % L == res) & ~ref["amb"]
            for step in (-1, 1):
                out[(res, step)] = _moved(ref, np.where(sel, np.clip(cut + step, 0, S), cut))
        ref["boundary_margins"] = out
    return ref["boundary_margins"]


def facts(ref):
    c, cut, amb = ref["case"], ref["cut"], ref["amb"]
    L = c.seg_len
    sure_cut = cut[(~amb) & (cut < c.S)]
    f = dict(rays=int(cut.size), seg_len=L, ambiguous=float(amb.mean()), cut=float((cut < c.S).mean()), uncut=float((cut == c.S).mean()),
             at_segment_start=int(((sure_cut % L == 0) & (sure_cut > 0)).sum()), one_past_start=int((sure_cut % L == 1).sum()),
             at_segment_end=int((sure_cut % L == L - 1).sum()), tol=ref["tol"])
    f["minus_one"], f["plus_one"] = margins(ref)
    f["boundary"] = min(m / t for ms in boundary_margins(ref).values() for m, t in zip(ms, ref["tol"]))
    return f


def describe(ref, f=None):
    f = f or facts(ref)
    return (f"{ref['case'].name} deg {ref['deg']}: R {f['rays']} L {f['seg_len']}  ambiguous {f['ambiguous']:.2%}  cut {f['cut']:.1%}  "
            f"uncut {f['uncut']:.1%}  cuts at k%L = 0 / 1 / L-1: {f['at_segment_start']} / {f['one_past_start']} / {f['at_segment_end']}  "
            f"tol (dens, feat) {f['tol'][0]:.2e} {f['tol'][1]:.2e}  |G(cut)-G(cut-1)| {f['minus_one'][0]:.2e} {f['minus_one'][1]:.2e}  "
            f"|G(cut)-G(cut+1)| {f['plus_one'][0]:.2e} {f['plus_one'][1]:.2e}  smallest boundary-only margin / tol {f['boundary']:.1f}")


def check_conditions(ref):
    """asserts the conditions of the module docstring on the oracle's figures alone; returns them"""
    c, f = ref["case"], facts(ref)
    what = describe(ref, f)
    assert f["ambiguous"] <= AMBIGUOUS_CAP, what
    assert f["cut"] >= MIN_CUT_SHARE and f["uncut"] >= MIN_UNCUT_SHARE, what
    assert f["at_segment_start"] > 0 and f["one_past_start"] > 0 and f["at_segment_end"] > 0, what
    if not c.realistic:      # (exempt: see the module docstring)
        for side in ("minus_one", "plus_one"):
            for margin, tol in zip(f[side], f["tol"]):
                assert margin >= MARGIN_FACTOR * tol, (side, what)
        assert f["boundary"] >= MARGIN_FACTOR, what
    return f
