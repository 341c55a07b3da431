"""Whole-grid passes over libvoxe_hip.so that need no workspace: upsampling, refinement graph and cut, connected components, mesh
export, density-gradient normals, per-voxel visibility, rigid resampling.  Reached through voxe_hip.ops, which re-exports them."""
import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import abi
from .args import GridSpec, RenderParams, _check_rays, _require_buffer, resolve_rng
from .desc import make_grid_desc, make_render_cfg
from .runtime import VoxeError, check, ensure_gfx950, f32c, lib, ptr, require_device, stream_ptr
from .workspace import _scratch_for, wrote


@torch.no_grad()
def upsample_trilinear(src: torch.Tensor, out_size: Sequence[int]) -> torch.Tensor:
    """[X,Y,Z,C] -> [X2,Y2,Z2,C], F.interpolate(trilinear, align_corners=False) semantics
    (thre3d_atom/thre3d_reprs/voxels.py:409-447)."""
    require_device(src, "upsample_trilinear")
    s = f32c(src)
    X, Y, Z, Cn = s.shape
    X2, Y2, Z2 = (int(v) for v in out_size)
    device = s.device
    ensure_gfx950(device)
    with torch.cuda.device(device):
        dst = torch.empty((X2, Y2, Z2, Cn), dtype=torch.float32, device=device)
        check(lib().voxe_upsample_trilinear(ptr(s), X, Y, Z, Cn, ptr(dst), X2, Y2, Z2, stream_ptr(device)),
              "voxe_upsample_trilinear")
    return dst


# ---- refinement stage: grid graph cut / connected components -----------------------------------------------
def graph_build(density_grid: torch.Tensor, feature_grid: torch.Tensor, sigma: float = 0.1,
                dilate_yz: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Nodes and quantised n-link capacities of the refinement graph
    (thre3d_atom/modules/refinement_functions.py:182-287).  density_grid [X,Y,Z(,1)], feature_grid [X,Y,Z,F]
    -> node_mask uint8 [X,Y,Z], cap int32 [6,X,Y,Z] (abi.DIR_* planes, abi.GRAPH_CAP_ONE units)."""
    require_device(density_grid, "graph_build")
    require_device(feature_grid, "graph_build")
    dens = f32c(density_grid)
    feat = f32c(feature_grid)
    X, Y, Z = (int(v) for v in dens.shape[:3])
    if dens.numel() != X * Y * Z or feat.dim() != 4 or tuple(feat.shape[:3]) != (X, Y, Z):
        raise VoxeError(f"graph_build: density grid {tuple(dens.shape)} / feature grid {tuple(feat.shape)} mismatch")
    device = dens.device
    ensure_gfx950(device)
    with torch.cuda.device(device):
        node = torch.empty((X, Y, Z), dtype=torch.uint8, device=device)
        cap = torch.empty((6, X, Y, Z), dtype=torch.int32, device=device)
        check(lib().voxe_graph_build(ptr(dens), ptr(feat), X, Y, Z, int(feat.shape[3]), float(sigma),
                                     int(bool(dilate_yz)), ptr(node), ptr(cap), stream_ptr(device)),
              "voxe_graph_build")
    return node, cap


def graphcut(node_mask: torch.Tensor, terminal: torch.Tensor, cap: torch.Tensor):
    """Exact minimum cut of the voxel graph (g.maxflow() + get_segment, refinement_functions.py:289-294).
    terminal int8 [X,Y,Z]: +1 edit (source) seed, -1 object (sink) seed.  `cap` is not modified.
    -> segment uint8 [X,Y,Z] (0 edit / 1 object / 255 no node), flow value (python int, capacity units)."""
    for t, name in ((node_mask, "node_mask"), (terminal, "terminal"), (cap, "cap")):
        require_device(t, f"graphcut({name})")
    X, Y, Z = (int(v) for v in node_mask.shape)
    if node_mask.dtype != torch.uint8 or terminal.dtype != torch.int8 or cap.dtype != torch.int32:
        raise VoxeError("graphcut: expected uint8 node_mask, int8 terminal, int32 cap")
    if tuple(terminal.shape) != (X, Y, Z) or tuple(cap.shape) != (6, X, Y, Z):
        raise VoxeError("graphcut: shape mismatch")
    device = node_mask.device
    ensure_gfx950(device)
    with torch.cuda.device(device):
        residual = cap.contiguous().clone()
        node, term = node_mask.contiguous(), terminal.contiguous()
        segment = torch.empty((X, Y, Z), dtype=torch.uint8, device=device)
        flow = torch.zeros((1,), dtype=torch.int64, device=device)
        nbytes = int(lib().voxe_graphcut_scratch_bytes(X, Y, Z))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        check(lib().voxe_graphcut(ptr(node), ptr(term), ptr(residual), X, Y, Z, ptr(segment), ptr(flow),
                                  ptr(scratch), nbytes, stream_ptr(device)), "voxe_graphcut")
    return segment, int(flow.item())


def cc_largest_k(mask: torch.Tensor, k: int) -> Tuple[torch.Tensor, int]:
    """cc3d.largest_k(mask, k, connectivity=26) (edit_pretrained_relu_field.py:384-389): int32 labels [X,Y,Z]
    (the M = min(k, N) largest components numbered 1..M by ascending size) and N."""
    require_device(mask, "cc_largest_k")
    m = (mask != 0).to(torch.uint8).contiguous()
    if m.dim() != 3:
        raise VoxeError(f"cc_largest_k: expected a [X,Y,Z] mask, got {tuple(m.shape)}")
    X, Y, Z = (int(v) for v in m.shape)
    device = m.device
    ensure_gfx950(device)
    with torch.cuda.device(device):
        labels = torch.empty((X, Y, Z), dtype=torch.int32, device=device)
        ncomp = torch.zeros((1,), dtype=torch.int32, device=device)
        nbytes = int(lib().voxe_cc_scratch_bytes(X, Y, Z, int(k)))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        check(lib().voxe_cc_largest_k(ptr(m), X, Y, Z, int(k), ptr(labels), ptr(ncomp), ptr(scratch), nbytes,
                                      stream_ptr(device)), "voxe_cc_largest_k")
    return labels, int(ncomp.item())


# ------------------------------------------------------------------------------------------------
# mesh export (marching cubes over the density iso-surface; DESIGN.md section 4 "Mesh export")
# ------------------------------------------------------------------------------------------------
def extract_mesh(spec: GridSpec, densities: torch.Tensor, level: float,
                 mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Closed, outward-wound triangle mesh of {density == level} on the device: vertices [V,3] float32 (world space),
    faces [T,3] int32.  `mask` ([X,Y,Z] or [X,Y,Z,1], bool / uint8, 0 = excluded) turns voxels into outside.  The count
    pass's totals are read back once (one synchronisation) to size the outputs."""
    require_device(densities, "extract_mesh (densities)")
    if densities.dim() != 4 or densities.shape[-1] != 1:
        raise VoxeError(f"extract_mesh: densities must be [X,Y,Z,1]; got {tuple(densities.shape)}")
    dens = f32c(densities.detach())
    device = dens.device
    X, Y, Z = (int(s) for s in dens.shape[:3])
    m = None
    if mask is not None:
        require_device(mask, "extract_mesh (mask)")
        if tuple(mask.shape[:3]) != (X, Y, Z) or mask.numel() != X * Y * Z:
            raise VoxeError(f"extract_mesh: mask must be [X,Y,Z]=({X},{Y},{Z}); got {tuple(mask.shape)}")
        m = (mask.reshape(X, Y, Z) != 0).to(torch.uint8).contiguous()
    ensure_gfx950(device)
    L = lib()
    g = make_grid_desc(dens.data_ptr(), dens.data_ptr(), (X, Y, Z), 1, spec.aabb, spec.density_scale,
                       spec.density_pre_act, spec.density_post_act, spec.feature_kind)
    with torch.cuda.device(device):
        nbytes = L.voxe_mesh_scratch_bytes(X, Y, Z)
        if nbytes == 0:
            raise VoxeError(f"extract_mesh: grid {X}x{Y}x{Z} is too large for int32 vertex / triangle ids")
        sc = _scratch_for(device, nbytes)
        totals = torch.empty(2, dtype=torch.int64, device=device)
        st = stream_ptr(device)
        check(L.voxe_mesh_count(C.byref(g), float(level), ptr(m), ptr(totals), ptr(sc), sc.numel(), st), "voxe_mesh_count")
        V, T = (int(v) for v in totals.cpu())
        if V >= 2 ** 31 or T >= 2 ** 31:
            raise VoxeError(f"extract_mesh: {V} vertices / {T} triangles exceed int32 ids")
        vertices = torch.empty((V, 3), dtype=torch.float32, device=device)
        faces = torch.empty((T, 3), dtype=torch.int32, device=device)
        check(L.voxe_mesh_emit(C.byref(g), float(level), ptr(m), ptr(vertices), V, ptr(faces), T, ptr(sc), sc.numel(), st),
              "voxe_mesh_emit")
    return vertices, faces


# ------------------------------------------------------------------------------------------------
# mesh import (signed-distance band of a triangle mesh): no workspace, not differentiable
# ------------------------------------------------------------------------------------------------
@torch.no_grad()
def voxelize_mesh(vertices: torch.Tensor, faces: torch.Tensor, colours: Optional[torch.Tensor], dims: Sequence[int], aabb,
                  band: float):
    """voxe_voxelize_mesh (include/voxe.h): vertices [V,3] float32 (world space), faces [T,3] int32 and optional vertex colours
    [V,3] on the device; `dims` (X, Y, Z) and `aabb` ((lo, hi) per axis) the lattice, `band` the half-width h > 0 in world units.
    -> (sdf [X,Y,Z] float32, negative inside, clamped to +-h; nearest [X,Y,Z] int32, -1 outside the band; colours [X,Y,Z,3];
    inside [X,Y,Z] uint8; stats: python ints (odd columns, malformed triangles, voxels in the band, work items), read back
    once).  The same bits whatever the order of the faces."""
    require_device(vertices, "voxelize_mesh (vertices)")
    require_device(faces, "voxelize_mesh (faces)")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise VoxeError(f"voxelize_mesh: vertices must be [V,3] and faces [T,3]; got {tuple(vertices.shape)}, {tuple(faces.shape)}")
    device = vertices.device
    v = f32c(vertices.detach())
    f = faces.detach().to(device=device, dtype=torch.int32).contiguous()
    c = None
    if colours is not None:
        require_device(colours, "voxelize_mesh (colours)")
        if tuple(colours.shape) != tuple(v.shape):
            raise VoxeError(f"voxelize_mesh: colours must be [V,3]={tuple(v.shape)}; got {tuple(colours.shape)}")
        c = f32c(colours.detach())
    X, Y, Z = (int(d) for d in dims)
    lo = (C.c_float * 3)(*[float(a[0]) for a in aabb])
    hi = (C.c_float * 3)(*[float(a[1]) for a in aabb])
    ensure_gfx950(device)
    L = lib()
    V, T = int(v.shape[0]), int(f.shape[0])
    with torch.cuda.device(device):
        nbytes = int(L.voxe_voxelize_scratch_bytes(X, Y, Z, T))
        if nbytes == 0:
            raise VoxeError(f"voxelize_mesh: a {X}x{Y}x{Z} lattice / {T} triangles are outside the limits of voxe_voxelize_mesh")
        sc = _scratch_for(device, nbytes)
        sdf = torch.empty((X, Y, Z), dtype=torch.float32, device=device)
        nearest = torch.empty((X, Y, Z), dtype=torch.int32, device=device)
        cols = torch.empty((X, Y, Z, 3), dtype=torch.float32, device=device)
        inside = torch.empty((X, Y, Z), dtype=torch.uint8, device=device)
        stats = torch.empty(4, dtype=torch.int64, device=device)
        check(L.voxe_voxelize_mesh(ptr(v), V, ptr(f), T, ptr(c), X, Y, Z, lo, hi, float(band), ptr(sdf), ptr(nearest), ptr(cols),
                                   ptr(inside), ptr(stats), ptr(sc), sc.numel(), stream_ptr(device)), "voxe_voxelize_mesh")
        stats = tuple(int(s) for s in stats.cpu())
    return sdf, nearest, cols, inside, stats


# ------------------------------------------------------------------------------------------------
# density-gradient normals (DESIGN.md section 4 "Normals"): read the raw densities only, no workspace, not differentiable
# ------------------------------------------------------------------------------------------------
def _normals_grid_desc(spec: GridSpec, dens: torch.Tensor):
    X, Y, Z = (int(s) for s in dens.shape[:3])
    # (features, F and feature_kind are not read by the normals entry points: no feature tensor is needed)
    return make_grid_desc(dens.data_ptr(), 0, (X, Y, Z), 0, spec.aabb, spec.density_scale, spec.density_pre_act,
                          spec.density_post_act, spec.feature_kind)


def _sampling_cfg(params: RenderParams, rng):
    """VoxeRenderCfg of the entries that only place samples along the rays (no colour, no workspace)"""
    return make_render_cfg(params.num_samples, params.near, params.far, params.perturb, params.linear_disparity, params.aabb_clip,
                           seed=rng[0], rng_offset=rng[1], image_width=params.image_width, image_height=params.image_height)


def _sampling_inputs(spec: GridSpec, params: RenderParams, densities, rays_o, rays_d, jitter, rng):
    """(grid desc, cfg, densities, rays_o, rays_d, jitter) of a density-only call on checked inputs: the tensors as dense float32
    (keep them alive over the call: the descriptor holds an address)"""
    ensure_gfx950(densities.device)
    dens, ro, rd = f32c(densities.detach()), f32c(rays_o.detach()), f32c(rays_d.detach())
    jit = None if jitter is None else f32c(jitter.detach())
    return _normals_grid_desc(spec, dens), _sampling_cfg(params, rng), dens, ro, rd, jit


def _check_densities(densities: torch.Tensor, what: str) -> None:
    require_device(densities, f"{what} (densities)")
    if densities.dim() != 4 or densities.shape[-1] != 1:
        raise VoxeError(f"{what}: densities must be [X,Y,Z,1]; got {tuple(densities.shape)}")


def query_normals(spec: GridSpec, densities: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """n(p) = -grad V / |grad V| at world points [N,3] -> [N,3] float32 ((0,0,0) where the gradient vanishes, e.g. outside the
    grid).  V is the trilinear pre-activated density VoxelGrid.forward interpolates; no gradient flows through the result."""
    _check_densities(densities, "query_normals")
    require_device(points, "query_normals (points)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise VoxeError(f"query_normals: points must be [N,3]; got {tuple(points.shape)}")
    device = densities.device
    ensure_gfx950(device)
    dens, pts = f32c(densities.detach()), f32c(points.detach().to(device))
    g = _normals_grid_desc(spec, dens)
    N = pts.shape[0]
    with torch.cuda.device(device):
        out = torch.empty((N, 3), dtype=torch.float32, device=device)
        check(lib().voxe_query_normals(C.byref(g), ptr(pts), N, ptr(out), stream_ptr(device)), "voxe_query_normals")
    return out


def render_normals(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor,
                   jitter: Optional[torch.Tensor] = None, rng: Optional[Tuple[int, int]] = None):
    """Rendered normals of flat rays: (normals [R,3] = sum_k w_k n(p_k) in world space, not renormalised; depth [R,1];
    acc [R,1]) with the samples and weights `render` uses for the same params, jitter and rng (`rng` follows render's rule:
    None = a fresh stream when params.perturb and no jitter is given).  The background and white_bkgd do not apply.
    Not differentiable."""
    _check_densities(densities, "render_normals")
    _check_rays("render_normals", rays_o, rays_d, jitter, params.num_samples)
    rng = resolve_rng(params, jitter, rng)
    device = densities.device
    g, c, dens, ro, rd, jit = _sampling_inputs(spec, params, densities, rays_o, rays_d, jitter, rng)
    R = ro.shape[0]
    with torch.cuda.device(device):
        normals = torch.empty((R, 3), dtype=torch.float32, device=device)
        depth = torch.empty((R, 1), dtype=torch.float32, device=device)
        acc = torch.empty((R, 1), dtype=torch.float32, device=device)
        check(lib().voxe_render_normals(C.byref(g), C.byref(c), ptr(ro), ptr(rd), R, ptr(jit), ptr(normals), ptr(depth),
                                        ptr(acc), stream_ptr(device)), "voxe_render_normals")
    return normals, depth, acc


# ------------------------------------------------------------------------------------------------
# per-voxel visibility (DESIGN.md section 4 "Visibility"): reads the raw densities only, no workspace, not differentiable
# ------------------------------------------------------------------------------------------------
def visibility_accumulate_(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor,
                           rays_d: torch.Tensor, max_weight: Optional[torch.Tensor] = None,
                           max_trans: Optional[torch.Tensor] = None, jitter: Optional[torch.Tensor] = None,
                           rng: Optional[Tuple[int, int]] = None) -> None:
    """Raise, in place, max_weight[c] to w_k * t_c and max_trans[c] to T_k over every sample k of the flat rays and every
    corner c of its trilinear footprint (t_c the gather weight, w_k = T_k alpha_k, T_k the transmittance on arrival), with the
    samples and weights `render` uses for the same params, jitter and rng (`rng` follows render's rule).  The buffers
    ([X,Y,Z] or [X,Y,Z,1] float32, contiguous, either may be None) ACCUMULATE: zero them before the first call.  The result is
    the same bit for bit however the rays are split over calls or ordered."""
    _check_densities(densities, "visibility_accumulate_")
    _check_rays("visibility_accumulate_", rays_o, rays_d, jitter, params.num_samples)
    device = densities.device
    for name, t in (("max_weight", max_weight), ("max_trans", max_trans)):
        if t is not None:     # ([X,Y,Z] or [X,Y,Z,1]: the kernel writes X * Y * Z floats whatever it is handed)
            _require_buffer("visibility_accumulate_", name, t, shape=densities.shape if t.dim() == 4 else densities.shape[:3],
                            numel=densities.numel(), device=device)
    rng = resolve_rng(params, jitter, rng)
    g, c, dens, ro, rd, jit = _sampling_inputs(spec, params, densities, rays_o, rays_d, jitter, rng)
    with torch.cuda.device(device):
        check(lib().voxe_visibility_accumulate(C.byref(g), C.byref(c), ptr(ro), ptr(rd), ro.shape[0], ptr(jit), ptr(max_weight),
                                               ptr(max_trans), stream_ptr(device)), "voxe_visibility_accumulate")


def visibility_mask(vis: torch.Tensor, threshold: float, dilate: int = 0) -> torch.Tensor:
    """uint8 [X,Y,Z]: 1 where some voxel within Chebyshev distance `dilate` (0..3) has vis > threshold (strict; NaN never)."""
    require_device(vis, "visibility_mask (vis)")
    if vis.dim() == 4 and vis.shape[-1] == 1:
        vis = vis[..., 0]
    if vis.dim() != 3:
        raise VoxeError(f"visibility_mask: vis must be [X,Y,Z]; got {tuple(vis.shape)}")
    v = f32c(vis.detach())
    device = v.device
    ensure_gfx950(device)
    X, Y, Z = (int(s) for s in v.shape)
    with torch.cuda.device(device):
        mask = torch.empty((X, Y, Z), dtype=torch.uint8, device=device)
        check(lib().voxe_visibility_mask(ptr(v), X, Y, Z, float(threshold), int(dilate), ptr(mask), stream_ptr(device)),
              "voxe_visibility_mask")
    return mask


# ------------------------------------------------------------------------------------------------
# lifting per-ray values into the grid: reads the raw densities only, no workspace, not differentiable
# ------------------------------------------------------------------------------------------------
LIFT_ONE = 1 << 32                                       # the fixed-point unit of sum_w / sum_wv (32 fraction bits)
LIFT_MERGE_SHIPPED, LIFT_MERGE_PER_LANE, LIFT_MERGE_WAVE = 0, 1, 2   # voxe_lift_debug_merge


def lift_accumulate_(spec: GridSpec, params: RenderParams, densities: torch.Tensor, rays_o: torch.Tensor, rays_d: torch.Tensor,
                     values: Optional[torch.Tensor], sum_wv: Optional[torch.Tensor], sum_w: Optional[torch.Tensor],
                     jitter: Optional[torch.Tensor] = None, rng: Optional[Tuple[int, int]] = (0, 0)) -> None:
    """Add, in place, q(w_k t_c) to sum_w[c] and q(w_k t_c values[r, ch]) to sum_wv[c, ch] over every sample k of the flat rays
    and every corner c of its trilinear footprint, q(x) = rint(x * 2^32), with the samples and weights visibility_accumulate_
    uses for the same params, jitter and rng.  values [R,C] float32 (C in 1..8, finite, |v| <= 1) and sum_wv [X,Y,Z,C] int64
    come together or are both None (coverage only); sum_w [X,Y,Z] int64 may be None.  The buffers ACCUMULATE: zero them before
    the first call.  The result is the same bit for bit however the rays are split over calls or ordered."""
    _check_densities(densities, "lift_accumulate_")
    _check_rays("lift_accumulate_", rays_o, rays_d, jitter, params.num_samples)
    device = densities.device
    X, Y, Z = (int(s) for s in densities.shape[:3])
    if (values is None) != (sum_wv is None):
        raise VoxeError("lift_accumulate_: values and sum_wv come together or not at all")
    Cn = 0
    if values is not None:
        require_device(values, "lift_accumulate_ (values)")
        if values.dim() != 2 or values.shape[0] != rays_o.shape[0] or not 1 <= values.shape[1] <= 8:
            raise VoxeError(f"lift_accumulate_: values must be [R,C]=({rays_o.shape[0]}, 1..8); got {tuple(values.shape)}")
        Cn = int(values.shape[1])
        _require_buffer("lift_accumulate_", "sum_wv", sum_wv, shape=(X, Y, Z, Cn), device=device, dtype=torch.int64)
    if sum_w is not None:
        _require_buffer("lift_accumulate_", "sum_w", sum_w, shape=(X, Y, Z), device=device, dtype=torch.int64)
    rng = resolve_rng(params, jitter, rng)
    g, c, dens, ro, rd, jit = _sampling_inputs(spec, params, densities, rays_o, rays_d, jitter, rng)
    vals = None if values is None else f32c(values.detach())
    with torch.cuda.device(device):
        check(lib().voxe_lift_accumulate(C.byref(g), C.byref(c), ptr(ro), ptr(rd), ro.shape[0], ptr(jit), ptr(vals), Cn,
                                         ptr(sum_wv), ptr(sum_w), stream_ptr(device)), "voxe_lift_accumulate")


def lift_debug_merge(mode: int) -> None:
    """test aid: pin the calling thread's later lift_accumulate_ calls to one kernel variant (LIFT_MERGE_*); 0 = shipped"""
    check(lib().voxe_lift_debug_merge(int(mode)), "voxe_lift_debug_merge")


# ------------------------------------------------------------------------------------------------
# vector quantisation against a codebook: plain buffers, no workspace, not differentiable
# ------------------------------------------------------------------------------------------------
VQ_MERGE_SHIPPED, VQ_MERGE_PER_LANE, VQ_MERGE_RUNS = 0, 1, 2   # voxe_vq_debug_merge
VQ_MAX_CHANNELS, VQ_MAX_CODEWORDS = 64, 65536


def _vq_points(entry: str, points: torch.Tensor) -> Tuple[int, int]:
    require_device(points, f"{entry} (points)")
    if points.dim() != 2:
        raise VoxeError(f"{entry}: points must be [N,F]; got {tuple(points.shape)}")
    _require_buffer(entry, "points", points, device=points.device)
    return int(points.shape[0]), int(points.shape[1])


def vq_assign_(points: torch.Tensor, codebook: torch.Tensor, index: Optional[torch.Tensor] = None,
               dist: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """voxe_vq_assign: index[n] = the codeword of `codebook` ([K,F] float32) nearest to points[n] ([N,F] float32) by the float32
    score |c|^2 - 2 x.c on the matrix cores, lowest k among bit-equal scores; dist[n] = the plain float32 squared distance to it.
    `index` (int32 [N]) and `dist` (float32 [N]) are written in place when given; index is allocated when None, dist is left
    out when None.  Returns (index, dist).  F in 1..64, K in 1..65536; all values finite."""
    N, F = _vq_points("vq_assign_", points)
    device = points.device
    if codebook.dim() != 2 or codebook.shape[1] != F:
        raise VoxeError(f"vq_assign_: codebook must be [K,F={F}]; got {tuple(codebook.shape)}")
    _require_buffer("vq_assign_", "codebook", codebook, device=device)
    K = int(codebook.shape[0])
    ensure_gfx950(device)
    with torch.cuda.device(device):
        if index is None:
            index = torch.empty((N,), dtype=torch.int32, device=device)
        _require_buffer("vq_assign_", "index", index, shape=(N,), device=device, dtype=torch.int32)
        if dist is not None:
            _require_buffer("vq_assign_", "dist", dist, shape=(N,), device=device)
        code_norm = torch.empty((max(K, 1),), dtype=torch.float32, device=device)
        check(lib().voxe_vq_assign(ptr(points), N, F, ptr(codebook), K, ptr(code_norm), ptr(index), ptr(dist),
                                   stream_ptr(device)), "voxe_vq_assign")
    return index, dist


def vq_accumulate_(points: torch.Tensor, weights: torch.Tensor, index: torch.Tensor, sum_wx: torch.Tensor,
                   sum_w: torch.Tensor, check_index: bool = True) -> None:
    """voxe_vq_accumulate: add, in place, q(w_n) to sum_w[index[n]] and q(w_n x_nj) to sum_wx[index[n], j], q(x) = rint(x * 2^32)
    (LIFT_ONE units).  points [N,F] float32 with |x| <= 1, weights [N] float32 in [0, 1], index [N] int32, sum_wx [K,F] and
    sum_w [K] int64.  The buffers ACCUMULATE: zero them before the first call.  The result is the same bit for bit however the
    points are ordered or split over calls.  The library skips a point whose index is outside 0..K-1 and cannot say so; with
    check_index (one host synchronisation) such an index is refused here with the library's bad-shape status instead."""
    N, F = _vq_points("vq_accumulate_", points)
    device = points.device
    if sum_wx.dim() != 2 or sum_wx.shape[1] != F:
        raise VoxeError(f"vq_accumulate_: sum_wx must be [K,F={F}]; got {tuple(sum_wx.shape)}")
    K = int(sum_wx.shape[0])
    _require_buffer("vq_accumulate_", "weights", weights, shape=(N,), device=device)
    _require_buffer("vq_accumulate_", "index", index, shape=(N,), device=device, dtype=torch.int32)
    _require_buffer("vq_accumulate_", "sum_wx", sum_wx, shape=(K, F), device=device, dtype=torch.int64)
    _require_buffer("vq_accumulate_", "sum_w", sum_w, shape=(K,), device=device, dtype=torch.int64)
    if check_index and N > 0:
        lo, hi = (int(v) for v in torch.aminmax(index))
        if lo < 0 or hi >= K:
            check(abi.ERR_BAD_SHAPE, f"voxe_vq_accumulate: index spans {lo}..{hi}, outside 0..{K - 1}")
    ensure_gfx950(device)
    with torch.cuda.device(device):
        check(lib().voxe_vq_accumulate(ptr(points), ptr(weights), ptr(index), N, F, K, ptr(sum_wx), ptr(sum_w),
                                       stream_ptr(device)), "voxe_vq_accumulate")


def vq_debug_merge(mode: int) -> None:
    """test aid: pin the calling thread's later vq_accumulate_ calls to one kernel variant (VQ_MERGE_*); 0 = shipped"""
    check(lib().voxe_vq_debug_merge(int(mode)), "voxe_vq_debug_merge")


# ------------------------------------------------------------------------------------------------
# rigid transform / re-gridding / composition of grids: no workspace, not differentiable
# ------------------------------------------------------------------------------------------------
def make_resample(A, b, sh_rot=None, sh_degree: int = -1, density_pre_act: int = abi.ACT_IDENTITY, density_fill: float = 0.0,
                  mode: int = abi.RESAMPLE_REPLACE) -> abi.VoxeResample:
    """VoxeResample from host values: A (3x3) and b (3) in any float type (cast to float32 here), sh_rot the list of band
    blocks M_0..M_deg ((2l+1) x (2l+1) each, as thre3d_reprs.transform.sh_rotation_matrices returns them) or None."""
    xf = abi.VoxeResample()
    flat = [float(v) for row in A for v in row]
    if len(flat) != 9 or len(b) != 3:
        raise VoxeError("grid_resample: A must be 3x3 and b of length 3")
    xf.A[:] = flat
    xf.b[:] = [float(v) for v in b]
    xf.sh_rot[0] = 1.0
    for l in range(1, 4):   # identity blocks where none is given
        for j in range(2 * l + 1):
            xf.sh_rot[abi.SH_ROT_OFFSETS[l] + j * (2 * l + 2)] = 1.0
    if sh_degree >= 0:
        if sh_rot is None or len(sh_rot) < sh_degree + 1:
            raise VoxeError(f"grid_resample: sh_degree {sh_degree} needs the rotation blocks M_0..M_{sh_degree}")
        for l in range(1, sh_degree + 1):   # (band 0 is the identity by definition)
            n = 2 * l + 1
            vals = [float(v) for row in sh_rot[l] for v in row]
            if len(vals) != n * n:
                raise VoxeError(f"grid_resample: M_{l} must be {n}x{n}")
            xf.sh_rot[abi.SH_ROT_OFFSETS[l]:abi.SH_ROT_OFFSETS[l + 1]] = vals
    xf.sh_degree, xf.density_pre_act, xf.mode, xf.density_fill = int(sh_degree), int(density_pre_act), int(mode), float(density_fill)
    return xf


@torch.no_grad()
def grid_resample(src_densities: Optional[torch.Tensor], src_features: Optional[torch.Tensor], xf: abi.VoxeResample,
                  dst_dims: Optional[Sequence[int]] = None, dst_densities: Optional[torch.Tensor] = None,
                  dst_features: Optional[torch.Tensor] = None, want_taken: bool = False):
    """voxe_grid_resample (include/voxe.h): sample the source grid ([X,Y,Z,1] densities and / or [X,Y,Z,C] features) at
    u = A i + b for every voxel i of the destination.  REPLACE: new float32 tensors of `dst_dims` are returned.  UNION:
    `dst_densities` (and `dst_features` when the source has features) are updated in place -- contiguous float32 tensors that do
    not alias the source.  Returns (densities, features, taken): taken is a uint8 [X2,Y2,Z2] tensor when want_taken, else
    None."""
    union = xf.mode == abi.RESAMPLE_UNION
    srcs = [t for t in (src_densities, src_features) if t is not None]
    if not srcs:
        raise VoxeError("grid_resample: neither densities nor features given")
    for t in srcs:
        require_device(t, "grid_resample")
        if t.dim() != 4:
            raise VoxeError(f"grid_resample: source tensors must be [X,Y,Z,C]; got {tuple(t.shape)}")
    device = srcs[0].device
    X, Y, Z = (int(v) for v in srcs[0].shape[:3])
    if any(tuple(t.shape[:3]) != (X, Y, Z) or t.device != device for t in srcs):
        raise VoxeError("grid_resample: source densities and features must share dims and device")
    if src_densities is not None and src_densities.shape[-1] != 1:
        raise VoxeError(f"grid_resample: densities must be [X,Y,Z,1]; got {tuple(src_densities.shape)}")
    Cn = int(src_features.shape[-1]) if src_features is not None else 1
    sd = None if src_densities is None else f32c(src_densities.detach())
    sf = None if src_features is None else f32c(src_features.detach())
    ensure_gfx950(device)
    with torch.cuda.device(device):
        if union:
            if dst_densities is None or sd is None or (sf is not None and dst_features is None):
                raise VoxeError("grid_resample: UNION runs in place on dst_densities (and dst_features) and needs the densities")
            dd, df = dst_densities, (dst_features if sf is not None else None)
            dims2 = tuple(int(v) for v in dd.shape[:3])
            for name, t, ch, s_ in (("dst_densities", dd, 1, sd), ("dst_features", df, Cn, sf)):
                if t is None:
                    continue
                _require_buffer("grid_resample", name, t, shape=(*dims2, ch), device=device)
                if t.untyped_storage().data_ptr() == s_.untyped_storage().data_ptr():
                    raise VoxeError("grid_resample: source and destination must not alias")
        else:
            if dst_dims is None or dst_densities is not None or dst_features is not None:
                raise VoxeError("grid_resample: REPLACE allocates its outputs: pass dst_dims and no destination tensors")
            dims2 = tuple(int(v) for v in dst_dims)
            if len(dims2) != 3 or min(dims2) <= 0:
                raise VoxeError(f"grid_resample: dst_dims must be three positive ints; got {dims2}")
            dd = None if sd is None else torch.empty((*dims2, 1), dtype=torch.float32, device=device)
            df = None if sf is None else torch.empty((*dims2, Cn), dtype=torch.float32, device=device)
        taken = torch.empty(dims2, dtype=torch.uint8, device=device) if want_taken else None
        check(lib().voxe_grid_resample(ptr(sd), ptr(sf), X, Y, Z, Cn, ptr(dd), ptr(df), *dims2, C.byref(xf), ptr(taken),
                                       stream_ptr(device)), "voxe_grid_resample")
    if union:
        wrote(dd, df)
    return dd, df, taken
