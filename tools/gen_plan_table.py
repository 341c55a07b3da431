"""Record what the host side of libvoxe_hip.so plans for a table of render calls (tests/plan_table.json).

Route, gradient layout, workspace sizes and offsets, scratch sizes and the status of the entry points that return before any
device work -- for a few hundred (grid, cfg, dispatch, R) cases.  Nothing here touches a GPU: the pointers in the descriptors are
fake non-null values and every call returns from its argument / workspace checks.  tests/test_render_plan_host.py re-evaluates
every recorded case against the current build and asserts equality, so the table pins the planning code across refactors.

    python tools/gen_plan_table.py            # rebuild the library if needed and rewrite tests/plan_table.json
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "vox-e_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from voxe_hip import abi  # noqa: E402
from voxe_hip.desc import make_grid_desc, make_render_cfg  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "plan_table.json")
FAKE = 0x1000          # a non-null "device pointer" (never dereferenced: every call returns before device work)
SENTINEL = -12345      # pre-fill of the debug outputs

# grids: (X, Y, Z)
CUBE, SMALL, ODD, BIG = (24, 24, 24), (8, 8, 8), (33, 17, 9), (160, 160, 160)
# feature kinds: name -> (feature_kind, F, sh_degree, render_diffuse)
KINDS = {"attn": (abi.FEAT_ATTN, 1, 0, 0)}
for _d in range(4):
    KINDS[f"sh{_d}"] = (abi.FEAT_SH, 3 * (_d + 1) ** 2, _d, 0)
    KINDS[f"sh{_d}d"] = (abi.FEAT_SH, 3 * (_d + 1) ** 2, _d, 1)
# ray orders: (image_width, image_height, R) on both sides of tile_min_rays (8192) and region_min_rays (16384)
ORDERS = [(0, 0, 0), (0, 0, 2048), (0, 0, 8192), (0, 0, 16383), (0, 0, 16384), (64, 0, 4096), (90, 0, 8190), (96, 96, 9216),
          (96, 96, 18432), (100, 200, 20000), (400, 400, 160000), (800, 0, 640000)]
FEW = [(0, 0, 2048), (0, 0, 16384), (96, 96, 9216), (400, 400, 160000)]
# the scalar results of a case, in the order the table stores them
KEYS = ["workspace_bytes", "workspace_bytes_inference", "route", "bwd_layout", "grad_offset", "grad_bytes", "recon_scratch_bytes",
        "attn_refine_scratch_bytes", "render_fwd", "render_bwd", "render_bwd_acc", "render_bwd_acc_into", "sample_probe"]


def _case(kind, order, S, dims=CUBE, **more):
    """a case as the table stores it: only what differs from a 24^3 grid with valid activations and a default cfg.
    more: det, disp (VoxeDispatch fields), cfg / grid (fields overwritten after construction), null (a pointer left NULL)"""
    c = {"kind": kind, "order": list(order), "S": S}
    if tuple(dims) != CUBE:
        c["dims"] = list(dims)
    c.update(more)
    return c


def cases():
    out = []
    # feature kind x ray order x depth segments (16 samples: one segment at every R; 256: several)
    for kind, order, S in itertools.product(("attn", "sh0", "sh1"), ORDERS, (16, 256)):
        out.append(_case(kind, order, S))
    out += [_case("sh3", order, 256) for order in FEW]
    for kind, order in itertools.product(("sh0d", "sh1d", "sh2", "sh2d", "sh3d"), [(0, 0, 16384), (96, 96, 9216)]):
        out.append(_case(kind, order, 256))
    # deterministic mode (image-ordered single-group renders are supported, the others are refused by the backward)
    for kind, order in itertools.product(("attn", "sh0", "sh1", "sh1d"), [(0, 0, 0), (0, 0, 16384), (96, 96, 9216)]):
        out.append(_case(kind, order, 128, det=1))
    # dispatch overrides, one at a time and the pairs that interact
    overrides = [dict(bwd_mode=1), dict(bwd_mode=2), dict(tile_two_phase=-1), dict(precise_grad=1), dict(tile_min_rays=-1),
                 dict(region_min_rays=-1), dict(tile_map=1), dict(tile_map=2), dict(tile_map=3), dict(tile_map=4),
                 dict(tile_min_rays=-1, region_min_rays=-1), dict(precise_grad=1, tile_min_rays=-1),
                 dict(region_min_rays=4096), dict(tile_min_rays=100000), dict(region_image_ratio=-1.0),
                 dict(fwd_segments_per_thread=2, precise_grad=1)]
    for d in overrides:
        out += [_case("sh0", order, 256, disp=d) for order in FEW[1:]] + [_case("sh1", (96, 96, 9216), 256, disp=d)]
    # grids: anisotropic with odd extents (brick rounding of the gradient region), tiny, large (image-ordered region route)
    for dims, kind, order in itertools.product((ODD, SMALL, BIG), ("sh0", "sh1"),
                                               [(0, 0, 2048), (0, 0, 16384), (96, 96, 9216), (100, 200, 20000)]):
        out.append(_case(kind, order, 200, dims=dims))
    out += [_case("attn", (0, 0, 16384), 200, dims=dims) for dims in (ODD, SMALL, BIG)]
    # cfg switches that enter a plan: linear_grad, term_eps (switches the region route off), aabb_clip (precise sums), negative R
    for order in FEW:
        out.append(_case("sh0", order, 256, cfg=dict(linear_grad=1)))
        out.append(_case("sh0", order, 256, cfg=dict(term_eps=1e-3)))
        out.append(_case("sh0", order, 256, cfg=dict(aabb_clip=1), disp=dict(precise_grad=1)))
    out.append(_case("sh0", (0, 0, -5), 64))
    # the limits of validate(): 31-bit element count, 24-bit index products (each just below and at the limit)
    for dims in [(1024, 1024, 512), (1024, 1024, 511), (4096, 4096, 1), (4095, 4096, 1), (1, 4096, 4096), (1, 1, 1 << 24),
                 (1, 1, (1 << 24) - 1), (0, 8, 8), (8, 8, -1)]:
        out.append(_case("sh0", (0, 0, 16384), 64, dims=dims))
    out += [_case("sh0", (96, 96, 9216), 64, dims=dims) for dims in [(1024, 1024, 512), (4095, 4096, 1), (0, 8, 8)]]
    # status precedence: invalid activations, F / degree mismatch, unknown feature kind, bad degree, bad image fields, NULLs
    # (all of them on image-ordered rays, the first few of each list on unordered rays too)
    grid_patches = [dict(pre=7), dict(post=9), dict(F=5), dict(F=5, post=9), dict(feature_kind=5), dict(feature_kind=5, pre=7),
                    dict(F=0), dict(F=0, post=9)]
    cfg_patches = [dict(sh_degree=4), dict(sh_degree=-1), dict(num_samples=0), dict(image_width=-3), dict(image_width=7),
                   dict(image_width=0, image_height=5), dict(image_height=-1), dict(image_height=7)]
    for order, n in (((96, 96, 9216), 8), ((0, 0, 2048), 3)):
        out += [_case("sh0", order, 64, grid=patch) for patch in grid_patches[:n]]
        out += [_case("sh0", order, 64, cfg=patch) for patch in cfg_patches[:n]]
        out.append(_case("attn", order, 64, grid=dict(F=3)))
        out += [_case("sh0", order, 64, null=null) for null in ("densities", "features", "cfg")]
    return out


def load_library():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


def _structs(case, ray_state_valid):
    fk, F, deg, diffuse = KINDS[case["kind"]]
    W, H, _ = case["order"]
    grid = make_grid_desc(FAKE, FAKE, (1, 1, 1), F, [(-1.5, 1.5)] * 3, 2.0, abi.ACT_IDENTITY, abi.ACT_SOFTPLUS, fk)
    grid.X, grid.Y, grid.Z = case.get("dims", CUBE)
    for k, v in case.get("grid", {}).items():
        setattr(grid, {"pre": "density_pre_act", "post": "density_post_act"}.get(k, k), v)
    null = case.get("null")
    if null in ("densities", "features"):
        setattr(grid, null, None)
    if null == "cfg":
        return grid, None
    dispatch = None
    if "disp" in case:
        dispatch = abi.VoxeDispatch()
        for k, v in case["disp"].items():
            setattr(dispatch, k, v)
    cfg = make_render_cfg(case["S"], 1.8, 6.6, sh_degree=deg, render_diffuse=diffuse, image_width=W, image_height=H,
                          deterministic=case.get("det", 0), dispatch=dispatch)
    for k, v in case.get("cfg", {}).items():
        setattr(cfg, k, v)
    cfg.ray_state_valid = ray_state_valid
    return grid, cfg


def evaluate(lib, case):
    """everything the table records for one case (JSON-ready: ints and lists of ints)"""
    R = case["order"][2]
    res = {}
    for name, valid in (("workspace_bytes", 0), ("workspace_bytes_inference", -1)):
        grid, cfg = _structs(case, valid)
        res[name] = lib.voxe_workspace_bytes(ctypes.byref(grid), ctypes.byref(cfg) if cfg else None, R)
    grid, cfg = _structs(case, 0)
    gp, cp = ctypes.byref(grid), (ctypes.byref(cfg) if cfg else None)
    res["route"] = lib.voxe_render_route(gp, cp, R)
    res["bwd_layout"] = lib.voxe_render_bwd_layout(gp, cp, R)
    for name, fn, n in (("sched", lib.voxe_tile_sched_debug_layout, 4), ("region", lib.voxe_region_debug_layout, 17)):
        out = (ctypes.c_int64 * n)(*([SENTINEL] * n))
        st = fn(gp, cp, R, out)
        res[name] = [st] + (list(out) if st == abi.OK else [])
    res["grad_offset"] = lib.voxe_workspace_grad_offset(gp)
    res["grad_bytes"] = lib.voxe_workspace_grad_bytes(gp)
    res["recon_scratch_bytes"] = lib.voxe_recon_scratch_bytes(R)
    res["attn_refine_scratch_bytes"] = lib.voxe_attn_refine_scratch_bytes(gp, R)
    # the entry points with a NULL workspace: argument checks, then VOXE_ERR_WORKSPACE -- before any device work
    P = FAKE
    layout = ctypes.c_int32(SENTINEL)
    res["render_fwd"] = lib.voxe_render_fwd(gp, cp, P, P, R, None, P, P, P, None, None, 0, None)
    res["render_bwd"] = lib.voxe_render_bwd(gp, cp, P, P, R, None, P, P, P, P, None, None, P, P, 0, None, 0, None)
    res["render_bwd_acc"] = lib.voxe_render_bwd_acc(gp, cp, P, P, R, None, P, P, P, P, None, None, 1, 1, 1, ctypes.byref(layout),
                                                    None, 0, None)
    res["render_bwd_acc_into"] = lib.voxe_render_bwd_acc_into(gp, cp, P, P, R, None, P, P, P, P, None, None, 1, 1, 1,
                                                              ctypes.byref(layout), None, 0, None, 0, None)
    res["sample_probe"] = lib.voxe_sample_probe(gp, cp, P, P, R, None, None, None, None, None, None, None, 0, None)
    assert layout.value == SENTINEL
    return res


def row(case, plan):
    """one table row: the case, its scalar results in the order of KEYS, then the two debug layouts (status, values when OK)"""
    return [case, [plan[k] for k in KEYS], plan["sched"], plan["region"]]


def main():
    lib = load_library()
    rows = [row(c, evaluate(lib, c)) for c in cases()]
    with open(TABLE, "w") as f:
        f.write('{"keys": %s, "rows": [\n' % json.dumps(KEYS))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]}\n")
    print(f"{len(rows)} cases -> {TABLE}; routes {sorted({r[1][2] for r in rows})}; {os.path.getsize(TABLE)} bytes")


if __name__ == "__main__":
    main()
