// voxe_api.hip -- the extern "C" boundary of libvoxe_hip.so (see include/voxe.h).
// Validation + argument marshalling only; kernels live in voxe_render.hip / voxe_grid_ops.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>

#include <mutex>
#include <unordered_map>

#include "../../include/voxe.h"
#include "voxe_launch.hpp"
#include "voxe_render_common.hpp"

using namespace voxe;

namespace {

// The dispatch of a call: VoxeRenderCfg::dispatch, or the shipped defaults (all fields 0) when it is NULL.  Nothing on the
// render path reads the environment (ABI v7).
const VoxeDispatch kDefaultDispatch = {};
const VoxeDispatch& disp_of(const VoxeRenderCfg* c) { return (c && c->dispatch) ? *c->dispatch : kDefaultDispatch; }
// bwd_mode 1 forces the plain global-atomic backward, 2 the line-dense scatter backward (A/B measurements, debugging)
bool force_scatter_bwd(const VoxeDispatch& d) { return d.bwd_mode == 1; }
bool force_no_tile_bwd(const VoxeDispatch& d) { return d.bwd_mode != 0; }
// tile_two_phase -1: view-dependent grids run the single-kernel channel groups even when the workspace has room for the
// per-sample sources
bool two_phase_disabled(const VoxeDispatch& d) { return d.tile_two_phase < 0; }

// block -> tile mapping (see logical_tile_of()).  Default: image-ordered rays are interleaved over the XCDs (load
// balance wins: neighbouring pixels share their voxels inside a wave anyway); rays in arbitrary order run in bands
// (a batch kept in memory order then gives every XCD's L2 a compact part of the volume: forward -22 % at 32768
// random rays).  VoxeDispatch::tile_map = 1 interleave | 2 band | 3 rows overrides both (A/B runs).
int tile_map_mode(int image_width, const VoxeDispatch& d) {
  if (d.tile_map >= 1 && d.tile_map <= 3) return d.tile_map - 1;
  return image_width > 0 ? 0 : 1;
}

struct Variant {
  int cout, ncoef_mem, C;
  bool attn;
};

// the checks every grid-taking entry point shares: extents and index widths of a grid read with `channels` floats per voxel ...
int grid_extent_status(const VoxeGridDesc* g, int channels) {
  if (g->X <= 0 || g->Y <= 0 || g->Z <= 0 || channels <= 0) return VOXE_ERR_BAD_SHAPE;
  if ((long long)g->X * g->Y * g->Z * channels >= (1LL << 31)) return VOXE_ERR_BAD_SHAPE;
  if ((long long)g->X * g->Y >= (1LL << 24) || (long long)g->Y * g->Z >= (1LL << 24) || g->Z >= (1 << 24)) return VOXE_ERR_BAD_SHAPE;  // 24-bit index multiplies (cell addresses; strides in the window flush)
  return VOXE_OK;
}
// ... of a call that reads densities and features ...
int grid_shape_status(const VoxeGridDesc* g) {
  if (!g || !g->densities || !g->features) return VOXE_ERR_NULL_POINTER;
  return g->F <= 0 ? VOXE_ERR_BAD_SHAPE : grid_extent_status(g, g->F + 1);
}
// ... and the density activations
int grid_acts_status(const VoxeGridDesc* g) {
  if (g->density_pre_act != VOXE_ACT_IDENTITY && g->density_pre_act != VOXE_ACT_ABS) return VOXE_ERR_UNSUPPORTED;
  if (g->density_post_act != VOXE_ACT_IDENTITY && g->density_post_act != VOXE_ACT_RELU &&
      g->density_post_act != VOXE_ACT_SOFTPLUS)
    return VOXE_ERR_UNSUPPORTED;
  return VOXE_OK;
}

int validate(const VoxeGridDesc* g, const VoxeRenderCfg* c, int64_t R, Variant* v) {
  if (!g || !c) return VOXE_ERR_NULL_POINTER;
  if (const int st = grid_shape_status(g)) return st;
  if (R < 0 || c->num_samples <= 0) return VOXE_ERR_BAD_SHAPE;
  if (g->feature_kind == VOXE_FEAT_ATTN) {
    if (g->F != 1) return VOXE_ERR_BAD_SHAPE;
    v->cout = 1; v->ncoef_mem = 1; v->attn = true;
  } else if (g->feature_kind == VOXE_FEAT_SH) {
    if (c->sh_degree < 0 || c->sh_degree > 3) return VOXE_ERR_UNSUPPORTED;
    const int nc = (c->sh_degree + 1) * (c->sh_degree + 1);
    if (g->F != 3 * nc) return VOXE_ERR_BAD_SHAPE;
    v->cout = 3; v->ncoef_mem = nc; v->attn = false;
  } else {
    return VOXE_ERR_UNSUPPORTED;
  }
  v->C = g->F + 1;
  if (const int st = grid_acts_status(g)) return st;
  if (c->image_width < 0 || (c->image_width > 0 && R % c->image_width != 0))
    return VOXE_ERR_BAD_SHAPE;
  if (c->image_height < 0 || (c->image_height > 0 && (c->image_width <= 0 || R % ((int64_t)c->image_height * c->image_width) != 0)))
    return VOXE_ERR_BAD_SHAPE;
  return VOXE_OK;
}

// a call that takes a grid and no render cfg (point queries): the shared checks + a channel count the pack kernels know
int validate_grid_only(const VoxeGridDesc* g) {
  if (const int st = grid_shape_status(g)) return st;
  const int C = g->F + 1;
  if (C != 2 && C != 4 && C != 13 && C != 28 && C != 49) return VOXE_ERR_BAD_SHAPE;
  return grid_acts_status(g);
}

// voxe_recon_step's paired render (two renders of the same batch with independent jitter streams in ONE launch of 2 B rays): an
// argument of plan_render(), kept by the plan; the space-binned kernels read DevCfg::pair_R.  rays = 0: an ordinary render
struct PairSpec { int64_t rays = 0; uint64_t rng_offset = 0; };

void grid_to_dev(const VoxeGridDesc* g, DevGrid* dg) {
  dg->X = g->X; dg->Y = g->Y; dg->Z = g->Z;
  for (int a = 0; a < 3; ++a) {
    dg->lo[a] = g->aabb_lo[a]; dg->hi[a] = g->aabb_hi[a];
    dg->scale[a] = g->norm_scale[a]; dg->bias[a] = g->norm_bias[a];
  }
  dg->density_scale = g->density_scale;
  dg->pre_act = g->density_pre_act; dg->post_act = g->density_post_act;
}

void make_dev(const VoxeGridDesc* g, const VoxeRenderCfg* c, int64_t R, const Variant& v, const PairSpec& pair, DevGrid* dg,
              HostCfg* dc) {
  dc->disp = disp_of(c);
  dc->pair_R = 0; dc->key0b = dc->key1b = 0;
  if (pair.rays) {
    dc->pair_R = pair.rays;
    dc->key0b = (uint32_t)c->seed ^ ((uint32_t)pair.rng_offset * 0x9E3779B1u);
    dc->key1b = (uint32_t)(c->seed >> 32) ^ (uint32_t)(pair.rng_offset >> 32) ^ 0x7F4A7C15u;
  }
  grid_to_dev(g, dg);
  dc->S = c->num_samples;
  dc->near = c->near; dc->far = c->far;
  dc->perturb = c->perturb; dc->lindisp = c->linear_disparity; dc->aabb_clip = c->aabb_clip;
  dc->white = c->white_bkgd; dc->attn = v.attn ? 1 : 0;
  dc->term_eps = c->term_eps;
  dc->key0 = (uint32_t)c->seed ^ ((uint32_t)c->rng_offset * 0x9E3779B1u);
  dc->key1 = (uint32_t)(c->seed >> 32) ^ (uint32_t)(c->rng_offset >> 32) ^ 0x7F4A7C15u;
  dc->image_width = c->image_width;
  dc->image_height = c->image_width > 0 ? (c->image_height > 0 ? c->image_height : (int)(R / c->image_width)) : 0;
  dc->map_mode = tile_map_mode(c->image_width, dc->disp);
  dc->R = R;
  dc->linear_grad = c->linear_grad;
  dc->seg_len = seg_len_for(R);
}

// ---- carving bytes: the one way this file lays buffers out in a caller's workspace / scratch ---------------------------------
// take() hands out the offset of the next buffer and moves on by its size rounded up to 256 bytes (a size of 0 takes nothing)
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t here = off; off += (bytes + 255) / 256 * 256; return here; }
};
template <class T> T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }

// workspace = [ packed grid | packed gradient | per-ray depth-segment states | segment partials | precise sums | schedule list ]
//             (`total`) [ two-phase sources | forward values | planar gradient | deterministic scratch | region scratch ]
// (`total_with_src`).  A call with a NULL cfg (grid step, point queries) has the first two only.
struct WsLayout {
  size_t packed_off, grad_off, state_off, seg_off, prec_off, sched_off, src_off, fwdval_off, planar_off, det_off, det_scale_off, region_off;
  size_t det_bytes;                          // fixed-point gradient + its scales (contiguous from det_off)
  size_t fwd_total, total, total_with_src;   // what a forward alone / a backward / every optional buffer needs
  // per-tile plan of the lean tile kernels, BEHIND everything voxe_workspace_bytes asks for: a caller that adds
  // voxe_tile_plan_bytes() to its workspace gets the planned kernels, every other caller the list alone (plan_render fills these)
  size_t plan_off, plan_bytes;
  bool has_precise, has_sched, has_src;      // the layout holds precise_grad sums / a schedule list / two-phase sources
  size_t grad_bytes() const { return state_off - grad_off; }
};
// `region`: the space-binned route applies to (grid, cfg, R) -- its scratch is part of the workspace.  A grid without extents: all 0.
WsLayout ws_layout(const VoxeGridDesc* g, const VoxeRenderCfg* c, int64_t R, bool region) {
  if (!g || g->X <= 0 || g->Y <= 0 || g->Z <= 0 || g->F <= 0) return WsLayout{};
  const size_t nvox = (size_t)g->X * g->Y * g->Z, C = (size_t)(g->F + 1), rays = (size_t)(R > 0 ? R : 0);
  const bool attn = g->feature_kind == VOXE_FEAT_ATTN;
  const size_t per_ray = (size_t)(attn ? 1 : 3) + 3;   // floats of one state / one segment partial
  const size_t nseg = c ? (size_t)num_segments(c->num_samples, seg_len_for(R)) : 1;
  WsLayout l{};
  Carve cv;
  l.packed_off = cv.take(nvox * C * sizeof(float));
  l.fwd_total = cv.off;  // the forward alone needs only the packed grid (states / segments are used when they fit)
  // the gradient region also fits the 2x2x2-bricked layout of the scatter backward (dims rounded up to even)
  const size_t bvox = (size_t)((g->X + 1) / 2) * ((g->Y + 1) / 2) * ((g->Z + 1) / 2) * 8;
  l.grad_off = cv.take(bvox * C * sizeof(float));
  l.state_off = cv.take((nseg - 1) * per_ray * rays * sizeof(float));
  // partial results of the depth-segmented forward: nseg x (cout + 3) floats per ray
  l.seg_off = cv.take(nseg * per_ray * rays * sizeof(float));
  // VoxeDispatch::precise_grad: segment-local sums of the forward in double, nseg x 5 doubles per ray (lean tile kernels)
  const bool precise = c && disp_of(c).precise_grad > 0 && c->image_width > 0 && !attn;
  const size_t prec = precise ? nseg * 5 * rays * sizeof(double) : 0;
  l.prec_off = cv.take(prec);
  l.has_precise = prec > 0;
  // cost-ordered block list of the lean tile kernels, next to the states it is valid with
  const size_t sched = c ? tile_sched_bytes(R, c->image_width, c->image_height, c->num_samples) : 0;
  l.sched_off = cv.take(sched);
  l.has_sched = sched > 0;
  l.total = cv.off;
  // per-sample gradient sources of the two-phase backward of view-dependent grids (optional: without it the channel
  // groups re-march the segment) ...
  const size_t srcb = c ? tile_src_bytes(R, c->image_width, c->image_height, c->num_samples, c->sh_degree, c->render_diffuse, attn) : 0;
  l.has_src = srcb > 0;
  l.src_off = cv.take(srcb);
  // ... and, behind the sources, the forward's per-sample (rad, v) in the same layout (r04: the source pass reads them instead of
  // gathering the wide texels again)
  l.fwdval_off = cv.take(srcb);
  // ... and the group-planar staging gradient of the lean deposit passes (r05: [group][voxel][4], 16 bytes per voxel and group)
  l.planar_off = cv.take(srcb ? tile_planar_bytes((long long)nvox, g->F + 1) : 0);
  // deterministic mode: the fixed-point gradient and, in its last 256 bytes, its scales behind everything else
  l.det_bytes = (c && c->deterministic) ? det_bytes((long long)nvox, g->F + 1) : 0;
  l.det_off = cv.take(l.det_bytes ? l.det_bytes - 256 : 0);
  l.det_scale_off = cv.take(l.det_bytes ? 256 : 0);
  // space-binned backward (voxe_render_region.hip): per-sample sources + segment tables
  l.region_off = cv.take(region ? region_scratch_bytes(g->X, g->Y, g->Z, R, c->num_samples, !attn && c->sh_degree > 0 && !c->render_diffuse) : 0);
  l.total_with_src = cv.off;
  return l;
}
// the part every call on a grid shares (grid step, point queries): packed grid + gradient region
WsLayout grid_layout(const VoxeGridDesc* g) { return ws_layout(g, nullptr, 0, false); }

// Every launching entry point ends here, and touches a thread-local of this library on the way.  glibc before 2.39 (BZ 19924) brings a
// thread's TLS table up to date only when the thread reads a thread-local of the NEWEST module loaded; until then every thread-local
// access of a dlopen()ed HIP runtime takes the slow path: measured 40 ns per HIP call, 1 - 2 us per entry point of this library, in a
// Python process (profiles/recon_args_host_time.txt).  The thread-local arguments this file used to read per call hid that.
thread_local volatile int tl_tls_current = 0;
int finish() { tl_tls_current = 1; return hipGetLastError() == hipSuccess ? VOXE_OK : VOXE_ERR_LAUNCH; }

// ---- the plan of one render call -----------------------------------------------------------------------------------------------
// Everything the entry points decide about a call -- which route it takes, how the workspace is carved, which optional buffers
// exist -- is decided ONCE, in plan_render(); the forward, the backward, its re-march and the query functions read the plan.  The
// forward and the backward of one render therefore agree on every buffer: both ask the same plan with the same workspace_bytes.
//
// Nominal vs effective: `route` / `region` are what the call does given the workspace voxe_workspace_bytes asks for.  A caller
// may pass less; tier() says what a workspace of `workspace_bytes` holds and which route the call then takes: states and segment
// partials need `total`, the region route, the two-phase buffers and the deterministic scratch need `total_with_src`.
struct RenderPlan {
  Variant v; DevGrid dg; HostCfg dc; WsLayout l;
  PairSpec pair;                 // the paired render of voxe_recon_step, or rays = 0
  int route = VOXE_ROUTE_NONE;   // nominal VOXE_ROUTE_*
  int nseg = 1;                  // depth segments of a march
  bool det = false, region = false, tiled = false, packed_bwd = false;   // deterministic | space-binned | LDS-window | line-dense scatter backward
  bool two_phase_ok = false;     // view-dependent grid on the tile route with room planned for the per-sample sources
  // VoxeDispatch::precise_grad: the double segment sums exist only when the forward of these rays is
  // render_fwd_tile4_kernel<3, true> (launch_fwd_t's condition): a depth-segmented march (nseg > 1), one segment per task, the lean
  // forward's own conditions.  Everywhere else (S <= one segment, fwd_segments_per_thread > 1, caller jitter, AABB clip, ...) the
  // backward runs its default suffix arithmetic.
  bool precise_sums_apply = false;

  struct Tier {
    bool full, with_src;         // workspace_bytes >= total | >= total_with_src
    bool region, two_phase;      // the region route / the two-phase buffers are live
    int route;                   // effective VOXE_ROUTE_*
    bool plan;                   // workspace_bytes >= total_with_src + the per-tile plan of this configuration
  };
  Tier tier(size_t workspace_bytes) const {
    const bool full = workspace_bytes >= l.total, with_src = workspace_bytes >= l.total_with_src;
    Tier t{full, with_src, region && with_src, two_phase_ok && with_src, 0, l.plan_bytes > 0 && workspace_bytes >= l.plan_off + l.plan_bytes};
    t.route = dc.R == 0 ? VOXE_ROUTE_NONE : det ? VOXE_ROUTE_DETERMINISTIC : t.region ? VOXE_ROUTE_REGION : tiled ? VOXE_ROUTE_TILE
              : packed_bwd ? VOXE_ROUTE_PACKED_SCATTER : VOXE_ROUTE_SCATTER;
    return t;
  }
  // layout of the gradient the backward leaves in the workspace (given the workspace voxe_workspace_bytes asks for)
  int grad_layout() const {
    if (dc.R == 0) return VOXE_GRAD_ANY;
    return (route == VOXE_ROUTE_PACKED_SCATTER && !dc.linear_grad) ? VOXE_GRAD_BRICKED : VOXE_GRAD_LINEAR;
  }
};

// Status of validate(); on VOXE_OK the whole plan is filled, otherwise only the layout (voxe_workspace_bytes answers for
// descriptors a render call would refuse).  `jitter`: the caller's jitter array (the lean forward, hence the precise sums, exist
// only without one).  `pair` (nullable): the paired render of voxe_recon_step.
int plan_render(const VoxeGridDesc* g, const VoxeRenderCfg* c, int64_t R, const float* jitter, const PairSpec* pair, RenderPlan* p) {
  *p = RenderPlan();   // (zeroes dg / dc: a plan that was refused has R = 0)
  if (pair) p->pair = *pair;
  const int st = validate(g, c, R, &p->v);
  if (st == VOXE_OK) {
    make_dev(g, c, R, p->v, p->pair, &p->dg, &p->dc);
    const VoxeDispatch& d = p->dc.disp;
    p->nseg = num_segments(c->num_samples, p->dc.seg_len);
    p->det = c->deterministic != 0;
    p->tiled = tile_bwd_supported(p->dc, c->sh_degree) && !force_no_tile_bwd(d);
    p->packed_bwd = !p->tiled && packed_scatter_supported(c->sh_degree) && !force_scatter_bwd(d);
    p->region = R > 0 && !p->det && !force_no_tile_bwd(d) && region_bwd_supported(p->dg, p->dc, c->sh_degree, c->render_diffuse, p->tiled);
  }
  p->l = ws_layout(g, c, R, p->region);
  if (st != VOXE_OK) return st;
  p->l.plan_off = p->l.total_with_src;
  p->l.plan_bytes = p->l.has_sched ? tile_plan_bytes(p->dc) : 0;
  p->route = p->tier(p->l.total_with_src).route;
  p->two_phase_ok = p->tiled && p->l.has_src && !two_phase_disabled(p->dc.disp);
  if (p->l.has_precise && c->sh_degree == 0 && !p->dc.attn && p->nseg > 1 && p->dc.disp.fwd_segments_per_thread <= 1) {
    FwdArgs probe{};
    probe.jitter = jitter;
    probe.segbuf = reinterpret_cast<float*>(1);   // (the segment partials live in the same workspace tier as the sums)
    p->precise_sums_apply = fwd_tile4_supported(p->dg, p->dc, probe, 3, 1);
  }
  return VOXE_OK;
}

// The FwdArgs of one march of the plan's rays through `workspace`: the forward itself (`out` = its outputs; keep = the caller
// keeps the workspace for a backward of these rays) or a re-march of the backward (`out` = null: no outputs, everything a backward
// reads is rebuilt).  One function, so that the two cannot disagree about sample_fwd, segsum_d, sched, ray_state or segbuf.
struct FwdOutputs { float *colour, *depth, *acc, *disparity; };
// what every function that runs a planned render is given, besides the plan
struct RenderCall {
  const VoxeGridDesc* grid; const VoxeRenderCfg* cfg;
  const float *rays_o, *rays_d; int64_t R; const float* jitter;
  void* workspace; size_t workspace_bytes; hipStream_t s;
  // voxe_recon_step on the space-binned route: where the segment tables live (null: in the workspace's own region scratch) and
  // whether voxe_recon_prefetch already filled them for these rays
  void* region_tables = nullptr; bool prebinned = false;
  bool drop_hint = false;   // a public render entry's call: once it is known to run, a hint pending on the workspace is dropped
};
FwdArgs fwd_args(const RenderPlan& p, const RenderPlan::Tier& t, const RenderCall& c, const FwdOutputs* out, bool keep) {
  const WsLayout& l = p.l;
  void* const workspace = c.workspace;
  const FwdOutputs o = out ? *out : FwdOutputs{};
  FwdArgs a{at<float>(workspace, l.packed_off), c.rays_o, c.rays_d, c.jitter, o.colour, o.depth, o.acc, o.disparity, nullptr, nullptr};
  a.keep_samples = keep;
  a.region_tables = c.region_tables; a.prebinned = c.prebinned;
  if (t.region) return a;   // (the region kernels keep their states and tables in their own scratch)
  // depth-segment states for the segmented backward, when that backward applies (a re-march runs only for a backward that reads them)
  if (t.full && (p.tiled || p.packed_bwd || !out)) a.ray_state = at<float>(workspace, l.state_off);
  if (t.full) a.segbuf = at<float>(workspace, l.seg_off);
  if (t.full && keep && p.precise_sums_apply) a.segsum_d = at<double>(workspace, l.prec_off);
  if (t.full && l.has_sched) a.sched = at<int>(workspace, l.sched_off);
  if (a.sched && t.plan) a.plan = at<int2>(workspace, l.plan_off);
  if (keep && t.two_phase) a.sample_fwd = at<float>(workspace, l.fwdval_off);   // (what the two-phase backward will read)
  return a;
}

// ---- what the last forward left in a workspace --------------------------------------------------------------------
// VoxeRenderCfg::ray_state_valid = 1 is a CLAIM by the caller ("this workspace still holds what voxe_render_fwd wrote for exactly
// these rays / cfg / jitter").  The library checks the claim instead of trusting it: every forward leaves a host-side record of
// what it rendered into the workspace it was given (keyed by the workspace address; calls on one workspace are ordered by the
// caller's stream, the record by the order of the calls), and a backward whose claim does not match the record re-marches the rays
// exactly as if it had been called with 0.  In particular a forward with ray_state_valid = -1 (inference: per-sample values not
// kept) followed by a backward with 1 is served by a re-march, not by stale per-sample values.  The record is a cache of facts
// about buffers, not dispatch state: losing it (more than kMaxStamps workspaces) only costs a re-march.
struct FwdStamp {
  const void *densities, *features, *rays_o, *rays_d, *jitter;
  int64_t R, pair_rays;
  uint64_t seed, rng_offset, pair_offset, wsbytes;
  int32_t X, Y, Z, F, feature_kind, pre_act, post_act, S, perturb, lindisp, clip, white, deg, diffuse, width, height, det, kept;
  float near_, far_, density_scale, lo[3], hi[3];
  // the dispatch fields (VoxeDispatch, field by field: the struct's padding is the caller's)
  int64_t d_tile_min_rays, d_region_min_rays;
  int32_t d_bwd_mode, d_tile_map, d_two_phase, d_qsplit, d_kl, d_fwd_window, d_fwd_spt, d_lean, d_precise, d_lds_ranks, d_phases;
  float d_fit_m, d_fit_lat, d_ffit_lat, d_ffit_m, d_zdom, d_max_adv, d_image_ratio;
};
FwdStamp make_stamp(const VoxeGridDesc* g, const VoxeRenderCfg* c, const float* rays_o, const float* rays_d, int64_t R,
                    const float* jitter, size_t wsbytes, const PairSpec& pair) {
  FwdStamp k;
  memset(&k, 0, sizeof(k));   // (padding included: stamps are compared with memcmp)
  k.densities = g->densities; k.features = g->features; k.rays_o = rays_o; k.rays_d = rays_d; k.jitter = jitter;
  k.R = R; k.pair_rays = pair.rays; k.seed = c->seed; k.rng_offset = c->rng_offset; k.pair_offset = pair.rng_offset; k.wsbytes = wsbytes;
  k.X = g->X; k.Y = g->Y; k.Z = g->Z; k.F = g->F; k.feature_kind = g->feature_kind; k.pre_act = g->density_pre_act;
  k.post_act = g->density_post_act; k.S = c->num_samples; k.perturb = c->perturb; k.lindisp = c->linear_disparity;
  k.clip = c->aabb_clip; k.white = c->white_bkgd; k.deg = c->sh_degree; k.diffuse = c->render_diffuse; k.width = c->image_width;
  k.height = c->image_height; k.det = c->deterministic;
  k.near_ = c->near; k.far_ = c->far; k.density_scale = g->density_scale;
  for (int a = 0; a < 3; ++a) { k.lo[a] = g->aabb_lo[a]; k.hi[a] = g->aabb_hi[a]; }
  const VoxeDispatch& d = disp_of(c);
  k.d_tile_min_rays = d.tile_min_rays; k.d_region_min_rays = d.region_min_rays; k.d_bwd_mode = d.bwd_mode; k.d_tile_map = d.tile_map;
  k.d_two_phase = d.tile_two_phase; k.d_qsplit = d.tile_qsplit; k.d_kl = d.tile_kl; k.d_fwd_window = d.fwd_window;
  k.d_fwd_spt = d.fwd_segments_per_thread; k.d_lean = d.tile_lean; k.d_precise = d.precise_grad; k.d_lds_ranks = d.region_lds_ranks; k.d_phases = d.tile_phases;
  k.d_fit_m = d.tile_fit_m; k.d_fit_lat = d.tile_fit_lat; k.d_ffit_lat = d.fwd_fit_lat; k.d_ffit_m = d.fwd_fit_m; k.d_zdom = d.fwd_zdom;
  k.d_max_adv = d.fwd_max_adv; k.d_image_ratio = d.region_image_ratio;
  return k;
}
FwdStamp make_stamp(const RenderPlan& p, const RenderCall& c) {
  return make_stamp(c.grid, c.cfg, c.rays_o, c.rays_d, c.R, c.jitter, c.workspace_bytes, p.pair);
}
constexpr size_t kMaxStamps = 256;
std::mutex g_stamp_mu;
std::unordered_map<const void*, FwdStamp> g_stamps;
void record_stamp(const void* workspace, const FwdStamp& k) {
  std::lock_guard<std::mutex> lock(g_stamp_mu);
  if (g_stamps.size() >= kMaxStamps && g_stamps.find(workspace) == g_stamps.end()) g_stamps.clear();
  g_stamps[workspace] = k;
}
void forget_stamp(const void* workspace) {
  std::lock_guard<std::mutex> lock(g_stamp_mu);
  g_stamps.erase(workspace);
}
// the tensor at `param` is about to be rewritten in place: no workspace's record of a forward over it describes the grid any more
void forget_stamps_of(const void* param) {
  if (!param) return;
  std::lock_guard<std::mutex> lock(g_stamp_mu);
  for (auto it = g_stamps.begin(); it != g_stamps.end();)
    it = (it->second.densities == param || it->second.features == param) ? g_stamps.erase(it) : std::next(it);
}
// does `workspace` hold the forward of exactly this render, per-sample values included?
bool stamp_matches(const void* workspace, FwdStamp k) {
  k.kept = 1;
  std::lock_guard<std::mutex> lock(g_stamp_mu);
  const auto it = g_stamps.find(workspace);
  return it != g_stamps.end() && memcmp(&it->second, &k, sizeof(k)) == 0;
}

// ---- voxe_recon_prefetch: the batch and the segment tables of the NEXT iteration, assembled on a side stream ---------------------
// Batch assembly and binning read the cameras, the images and the jitter streams -- never the grid -- so iteration i + 1's can run
// while iteration i's backward and grid step occupy the memory system (binning is index arithmetic; the grid step is a pure
// HBM stream).  Two sets of tables / batch buffers alternate: set 0 = (region scratch of `workspace`, front of `scratch`), set 1 =
// (the same offsets of `workspace2`, ReconLayout::batch2).  A prefetch is a HINT recorded per workspace: the step that follows
// uses it iff the arguments that decide the batch and the tables are the ones it was made for (ReconKey, compared field by
// field); otherwise it waits for the side stream and assembles its own, exactly as without the hint.
struct ReconKey {
  FwdStamp fwd;                  // grid geometry, cfg, dispatch, jitter streams, ray buffers of the paired render
  const void *poses, *image_rows, *images, *workspace2, *scratch;
  uint64_t subset_offset, ws2bytes, scbytes;
  int64_t batch;
  int32_t H, W, K, num_images;
  float focal;
};
// The hints on record -- one per workspace, with the side stream it is assembled on -- and their protocol.  Each method is one step
// of it and takes the lock once.  Each finds its record by workspace: a record that another thread's issue() recycled between two
// steps of one call is simply absent (or fresh) for the later step, which then has nothing to do.
class ReconHints {
 public:
  // voxe_recon_prefetch: `enqueue(slot, side)` puts the work of a hint for table set `slot` on the side stream and returns what the
  // hint was made for.  The side work starts behind the forward of the last step on this workspace: launched in front of the
  // backward, the segment pass would take a quarter of its slots; behind it, it shares the machine with the grid step, an HBM stream
  // that leaves the CUs idle (profiles/r06_recon_prefetch.txt; the schedules that lost are in DESIGN.md's table).
  template <class Enqueue>
  int issue(const void* workspace, hipStream_t s, Enqueue enqueue) {
    std::lock_guard<std::mutex> lock(mu_);
    if (recs_.size() >= kMaxRecords && recs_.find(workspace) == recs_.end()) {
      // (workspaces come and go with their trainers: records without a hint in flight give their stream and events back)
      for (auto it = recs_.begin(); it != recs_.end();) {
        Record& o = it->second;
        if (o.hint.valid) { ++it; continue; }          // (a hint in flight: its events are still waited for)
        if (o.side) { (void)hipStreamSynchronize(o.side); (void)hipStreamDestroy(o.side); }
        if (o.fork) (void)hipEventDestroy(o.fork);
        if (o.done) (void)hipEventDestroy(o.done);
        it = recs_.erase(it);
      }
    }
    Record& r = recs_[workspace];
    if (!r.side) {
      // (lowest priority: the side stream's kernels fill what the iteration's own kernels leave idle, they do not queue in front of them)
      int prio_lo = 0, prio_hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
      if (hipStreamCreateWithPriority(&r.side, hipStreamNonBlocking, prio_lo) != hipSuccess) return VOXE_ERR_LAUNCH;
      if (hipEventCreateWithFlags(&r.fork, hipEventDisableTiming) != hipSuccess) return VOXE_ERR_LAUNCH;
      if (hipEventCreateWithFlags(&r.done, hipEventDisableTiming) != hipSuccess) return VOXE_ERR_LAUNCH;
    }
    const int slot = 1 - r.last_slot;   // (a hint never consumed: its tables are overwritten -- in stream order on the side stream)
    if (!r.forked) (void)hipEventRecord(r.fork, s);   // no step has run on this workspace yet (or the last one took another route): behind whatever is on `s`
    (void)hipStreamWaitEvent(r.side, r.fork, 0);
    r.hint = Pending{true, slot, enqueue(slot, r.side)};
    (void)hipEventRecord(r.done, r.side);
    ++stats_[0];
    return VOXE_OK;
  }
  // voxe_recon_step begins: `s` waits for a hint pending on the workspace whether or not the step takes its tables (it may be about
  // to write that set); the hint is handed over.  Until forward_enqueued() a new hint is ordered behind everything on the stream.
  struct Pending { bool valid = false; int slot = 0; ReconKey key{}; };
  Pending begin_step(const void* workspace, hipStream_t s) {
    std::lock_guard<std::mutex> lock(mu_);
    const auto it = recs_.find(workspace);
    if (it == recs_.end()) return Pending();
    Record& r = it->second;
    const Pending p = r.hint;
    if (p.valid) (void)hipStreamWaitEvent(s, r.done, 0);
    r.hint.valid = false;
    r.last_slot = 0;
    r.forked = false;
    return p;
  }
  // the forward of a step that rendered from table set `slot` is on `s`: from here on the other set may be rewritten
  void forward_enqueued(const void* workspace, int slot, hipStream_t s) {
    std::lock_guard<std::mutex> lock(mu_);
    const auto it = recs_.find(workspace);
    if (it == recs_.end() || !it->second.side) return;
    it->second.last_slot = slot;
    (void)hipEventRecord(it->second.fork, s);
    it->second.forked = true;
  }
  // a step took the hint it was handed / assembled its own batch and tables instead
  void count(bool taken) { std::lock_guard<std::mutex> lock(mu_); ++stats_[taken ? 1 : 2]; }
  // a call other than the step is about to write `ptr` beyond the gradient region on `s`: a hint whose tables may live there (its workspace
  // or workspace2) is dropped, `s` waits for the side stream, and the next hint there is ordered behind everything on its stream
  void workspace_written(const void* ptr, hipStream_t s) {
    std::lock_guard<std::mutex> lock(mu_);
    for (auto& rec : recs_) {
      Record& r = rec.second;
      if (rec.first != ptr && r.hint.key.workspace2 != ptr) continue;   // (the key of the last hint issued, pending or not)
      r.forked = false;
      if (!r.hint.valid) continue;
      (void)hipStreamWaitEvent(s, r.done, 0);
      r.hint.valid = false; ++stats_[2];
    }
  }
  void stats(int64_t out[3]) { std::lock_guard<std::mutex> lock(mu_); for (int i = 0; i < 3; ++i) out[i] = stats_[i]; }
 private:
  struct Record {
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr;     // on the caller's stream, behind a step's forward (fold pass): from here on the side work of a hint may run
    hipEvent_t done = nullptr;     // on the side stream, behind the pending hint's work
    bool forked = false; int last_slot = 0;   // set the last step of this workspace rendered from
    Pending hint;                  // awaits the next step on this workspace
  };
  static constexpr size_t kMaxRecords = 16;
  std::mutex mu_;
  std::unordered_map<const void*, Record> recs_;     // by workspace
  int64_t stats_[3] = {0, 0, 0};                     // hints issued | taken by the following step | dropped (voxe_recon_prefetch_stats)
};
ReconHints g_hints;

// ---- per-phase timing (voxe_profile_*) ----------------------------------------------------------
enum Phase { PH_PACK = 0, PH_FWD, PH_MEMSET, PH_BWD, PH_UNPACK, PH_COUNT };
struct Profiler {
  static constexpr int kMax = 512;
  bool on = false, created = false;
  hipEvent_t ev[kMax][2];
  int phase[kMax];
  int count = 0, dropped = 0;
} g_prof;

struct PhaseTimer {  // records start/stop events around one phase when profiling is enabled
  int slot = -1;
  hipStream_t st;
  PhaseTimer(Phase ph, hipStream_t s) : st(s) {
    if (!g_prof.on) return;
    if (g_prof.count >= Profiler::kMax) { ++g_prof.dropped; return; }
    slot = g_prof.count++;
    g_prof.phase[slot] = ph;
    (void)hipEventRecord(g_prof.ev[slot][0], st);
  }
  ~PhaseTimer() {
    if (slot >= 0) (void)hipEventRecord(g_prof.ev[slot][1], st);
  }
};

}  // namespace

extern "C" {

int voxe_abi_version(void) { return VOXE_ABI_VERSION; }

const char* voxe_strerror(int status) {
  switch (status) {
    case VOXE_OK: return "ok";
    case VOXE_ERR_NULL_POINTER: return "null pointer";
    case VOXE_ERR_BAD_SHAPE: return "bad shape";
    case VOXE_ERR_UNSUPPORTED: return "unsupported activation / mode";
    case VOXE_ERR_WORKSPACE: return "workspace missing or too small";
    case VOXE_ERR_LAUNCH: return "kernel launch failed";
    case VOXE_ERR_NO_DEVICE: return "no gfx950 HIP device";
    default: return "unknown voxe status";
  }
}

int voxe_device_check(char* name, size_t name_len) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return VOXE_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return VOXE_ERR_NO_DEVICE;
  if (name && name_len) {
    strncpy(name, prop.gcnArchName, name_len - 1);
    name[name_len - 1] = 0;
  }
  return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? VOXE_OK : VOXE_ERR_NO_DEVICE;
}

int voxe_profile_enable(int32_t on) {
  if (on && !g_prof.created) {
    for (int i = 0; i < Profiler::kMax; ++i)
      for (int j = 0; j < 2; ++j)
        if (hipEventCreate(&g_prof.ev[i][j]) != hipSuccess) return VOXE_ERR_LAUNCH;
    g_prof.created = true;
  }
  g_prof.on = on != 0;
  g_prof.count = 0;
  g_prof.dropped = 0;
  return VOXE_OK;
}

int voxe_profile_read(VoxeProfile* out) {
  if (!out) return VOXE_ERR_NULL_POINTER;
  memset(out, 0, sizeof(*out));
  double* ms[PH_COUNT] = {&out->ms_pack, &out->ms_fwd, &out->ms_memset, &out->ms_bwd, &out->ms_unpack};
  int32_t* n[PH_COUNT] = {&out->n_pack, &out->n_fwd, &out->n_memset, &out->n_bwd, &out->n_unpack};
  for (int i = 0; i < g_prof.count; ++i) {
    if (hipEventSynchronize(g_prof.ev[i][1]) != hipSuccess) return VOXE_ERR_LAUNCH;
    float t = 0.f;
    if (hipEventElapsedTime(&t, g_prof.ev[i][0], g_prof.ev[i][1]) != hipSuccess) return VOXE_ERR_LAUNCH;
    *ms[g_prof.phase[i]] += (double)t;
    *n[g_prof.phase[i]] += 1;
  }
  out->n_dropped = g_prof.dropped;
  g_prof.count = 0;
  g_prof.dropped = 0;
  return VOXE_OK;
}

int voxe_cast_rays(int32_t H, int32_t W, float focal, const float* rot, const float* trans,
                   float* rays_o, float* rays_d, void* stream) {
  if (!rot || !trans || !rays_o || !rays_d) return VOXE_ERR_NULL_POINTER;
  if (H <= 0 || W <= 0) return VOXE_ERR_BAD_SHAPE;
  launch_cast_rays(H, W, focal, rot, trans, rays_o, rays_d, (hipStream_t)stream);
  return finish();
}

int voxe_cast_rays_indexed(int32_t H, int32_t W, float focal, const float* poses, int32_t K,
                           const int64_t* flat_index, int64_t B, float* rays_o, float* rays_d, void* stream) {
  if (!poses || !flat_index || !rays_o || !rays_d) return VOXE_ERR_NULL_POINTER;
  if (H <= 0 || W <= 0 || K <= 0 || B < 0) return VOXE_ERR_BAD_SHAPE;
  if (B == 0) return VOXE_OK;
  launch_cast_rays_indexed(H, W, focal, poses, K, (const long long*)flat_index, B, rays_o, rays_d,
                           (hipStream_t)stream);
  return finish();
}

int voxe_random_subset(int64_t n, int64_t count, uint64_t seed, uint64_t rng_offset, int64_t* out, void* stream) {
  if (!out) return VOXE_ERR_NULL_POINTER;
  if (n <= 0 || n > (1ll << 31) || count < 0 || count > n) return VOXE_ERR_BAD_SHAPE;
  if (count == 0) return VOXE_OK;
  launch_random_subset(n, count, seed, rng_offset, (long long*)out, (hipStream_t)stream);
  return finish();
}

// test aid (not part of voxe.h): where the cost-ordered block list of the lean tile kernels lives in the workspace of this render --
// out = (1 when launches of this configuration build one, byte offset, blocks of a launch, tile slots of a launch)
int voxe_tile_sched_debug_layout(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R, int64_t out[4]) {
  RenderPlan p;
  const int st = plan_render(grid, cfg, R, nullptr, nullptr, &p);
  if (st) return st;
  if (!out) return VOXE_ERR_NULL_POINTER;
  const HostCfg& dc = p.dc;
  const int64_t ntp = dc.image_width > 0 ? blocks_for_tiles(dc.map_mode, (dc.image_width + 7) / 8, tile_rows_total(dc, 8)) : 0;
  out[0] = (p.l.has_sched && tile_sched_applies(dc)) ? 1 : 0;
  out[1] = (int64_t)p.l.sched_off;
  out[2] = ntp * p.nseg;
  out[3] = ntp;
  return VOXE_OK;
}

// test aids (not part of voxe.h): byte offset in the workspace of this render's per-tile plan, one 8-byte record per block in list
// order (voxe_render_tile4.hip: PlanCfg), -1 when launches of this configuration build none; and how many launches of the planned
// forward / backward kernels this process has made so far
int voxe_tile_plan_debug_offset(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R, int64_t* out) {
  RenderPlan p;
  const int st = plan_render(grid, cfg, R, nullptr, nullptr, &p);
  if (st) return st;
  if (!out) return VOXE_ERR_NULL_POINTER;
  *out = p.l.plan_bytes > 0 ? (int64_t)p.l.plan_off : -1;
  return VOXE_OK;
}
int voxe_tile_plan_debug_launches(int64_t out[2]) {
  if (!out) return VOXE_ERR_NULL_POINTER;
  tile_plan_launch_counts(out);
  return VOXE_OK;
}

size_t voxe_tile_plan_bytes(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R) {
  RenderPlan p;
  if (plan_render(grid, cfg, R, nullptr, nullptr, &p) != VOXE_OK || !cfg || cfg->ray_state_valid < 0) return 0;
  return p.l.plan_bytes;
}

size_t voxe_workspace_bytes(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R) {
  RenderPlan p;
  (void)plan_render(grid, cfg, R, nullptr, nullptr, &p);   // (sizes are answered for descriptors a render call would refuse, too)
  // ray_state_valid = -1 (inference: no backward of these rays follows): the packed grid and the segmented forward's states /
  // partials -- none of the backward's per-sample sources, staging gradient or binning scratch (gigabytes at large R)
  return (cfg && cfg->ray_state_valid < 0) ? p.l.total : p.l.total_with_src;
}

}  // extern "C" (reopened below)

namespace {
// ---- running a planned render ------------------------------------------------------------------------------------------------------
// The public render entries plan their call and hand the plan to the functions below with RenderCall::drop_hint set: behind the
// checks that can refuse the call, in front of its first launch, a prefetch hint pending on the workspace is dropped
// (ReconHints::workspace_written).  voxe_recon_step and voxe_attn_refine_step plan each of their renders once and run its forward
// and backward from that plan (which reads neither cfg->ray_state_valid nor cfg->reuse_packed_grid: the steps change both in
// between); voxe_recon_step leaves drop_hint off, so a step never drops its own hint.
int render_fwd(const RenderPlan& p, const RenderCall& c, const FwdOutputs& out) {
  const VoxeRenderCfg* cfg = c.cfg; void* const workspace = c.workspace; hipStream_t s = c.s;
  if (c.R > 0 && (!c.rays_o || !c.rays_d || !out.colour)) return VOXE_ERR_NULL_POINTER;
  if (!workspace || c.workspace_bytes < p.l.fwd_total) return VOXE_ERR_WORKSPACE;
  if (c.drop_hint) g_hints.workspace_written(workspace, s);
  if (!cfg->reuse_packed_grid) { PhaseTimer t(PH_PACK, s); launch_pack_any(c.grid, at<float>(workspace, p.l.packed_off), s); }
  if (c.R == 0) return finish();
  {
    // what this workspace holds from now on (a backward's ray_state_valid = 1 is checked against it)
    FwdStamp k = make_stamp(p, c);
    k.kept = cfg->ray_state_valid >= 0 ? 1 : 0;
    record_stamp(workspace, k);
  }
  const RenderPlan::Tier tier = p.tier(c.workspace_bytes);
  const FwdArgs a = fwd_args(p, tier, c, &out, cfg->ray_state_valid >= 0);
  PhaseTimer t(PH_FWD, s);
  // space-binned path (unordered / sparse rays): forward through the region kernels; the segment tables and per-segment
  // states stay in the workspace for the backward of the same call (cfg->ray_state_valid)
  if (tier.region) launch_fwd_region(p.dg, p.dc, cfg->sh_degree, cfg->render_diffuse, a, at<char>(workspace, p.l.region_off), s);
  else launch_fwd(p.dg, p.dc, cfg->sh_degree, cfg->render_diffuse, a, s);
  return finish();
}

// what the three backward entry points check before anything else; on VOXE_OK *p is the plan of the call
int plan_bwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R, const float* jitter, const float* rays_o,
             const float* rays_d, const float* colour, const float* depth, const float* acc, const float* d_colour, RenderPlan* p) {
  const int st = plan_render(grid, cfg, R, jitter, nullptr, p);
  if (st) return st;
  if (R > 0 && (!rays_o || !rays_d || !colour || !depth || !acc || !d_colour)) return VOXE_ERR_NULL_POINTER;
  return VOXE_OK;
}

// memset (optional) + backward kernel into the packed gradient region of the workspace (or `grad_workspace`'s); *grad_layout = its layout
int render_bwd(const RenderPlan& p, const RenderCall& c, const float* colour, const float* depth, const float* acc,
               const float* d_colour, const float* d_depth, const float* d_acc, bool want_d, bool want_f, bool zero_first,
               int32_t* grad_layout, void* grad_workspace, size_t grad_workspace_bytes) {
  const VoxeRenderCfg* cfg = c.cfg; void* const workspace = c.workspace; hipStream_t s = c.s;
  const WsLayout& l = p.l;
  if (!workspace || c.workspace_bytes < l.total) return VOXE_ERR_WORKSPACE;
  if (grad_workspace && grad_workspace_bytes < l.state_off) return VOXE_ERR_WORKSPACE;   // (packed grid + gradient region)
  // (every refusal comes before the first launch: a refused call leaves the workspace as it found it)
  if (p.det && c.R > 0) {
    if (!det_bwd_supported(p.dc, cfg->sh_degree, cfg->render_diffuse)) return VOXE_ERR_UNSUPPORTED;
    if (!p.tier(c.workspace_bytes).with_src) return VOXE_ERR_WORKSPACE;
  }
  if (c.drop_hint) g_hints.workspace_written(workspace, s);
  float* packed = at<float>(workspace, l.packed_off);
  float* gpacked = at<float>(grad_workspace ? grad_workspace : workspace, l.grad_off);
  if (!cfg->reuse_packed_grid) { PhaseTimer t(PH_PACK, s); launch_pack_any(c.grid, packed, s); }
  if (zero_first) {
    PhaseTimer t(PH_MEMSET, s);
    if (hipMemsetAsync(gpacked, 0, l.grad_bytes(), s) != hipSuccess) return VOXE_ERR_LAUNCH;
  }
  if (c.R == 0) { *grad_layout = VOXE_GRAD_ANY; return finish(); }
  const DevGrid& dg = p.dg; const HostCfg& dc = p.dc;
  const RenderPlan::Tier tier = p.tier(c.workspace_bytes);
  float* state = at<float>(workspace, l.state_off);
  BwdArgs a{packed, c.rays_o, c.rays_d, c.jitter, colour, depth, acc, d_colour, d_depth, d_acc, gpacked,
            want_d, want_f, (p.tiled || p.packed_bwd) ? state : nullptr};
  a.region_tables = c.region_tables;
  // (the forward of these rays -- voxe_render_fwd with this workspace or the re-march below -- wrote the sums, the list and its
  // per-sample values under the same plan: fwd_args())
  if (p.precise_sums_apply) a.segsum_d = at<const double>(workspace, l.prec_off);
  if (l.has_sched) a.sched = at<const int>(workspace, l.sched_off);
  if (a.sched && tier.plan) a.plan = at<const int2>(workspace, l.plan_off);
  if (tier.two_phase) {
    a.sample_src = at<float>(workspace, l.src_off);
    if (p.nseg > 1) a.sample_fwd = at<const float>(workspace, l.fwdval_off);   // (only the depth-segmented forward writes them)
    a.grad_planar = at<float>(workspace, l.planar_off);
  }
  if (p.det) {   // (supported and sized: checked above)
    a.gdet = at<unsigned long long>(workspace, l.det_off);
    a.det_scale = at<float>(workspace, l.det_scale_off);
    a.ray_state = state;
  }
  // the caller's claim that the workspace holds this render's forward is only believed when the forward's record says so
  const FwdStamp stamp = make_stamp(p, c);
  const bool states_valid = cfg->ray_state_valid > 0 && stamp_matches(workspace, stamp);
  if (!states_valid) {
    // (the re-march below writes everything a backward reads: from here on the workspace holds THIS render)
    FwdStamp k = stamp;
    k.kept = 1;
    record_stamp(workspace, k);
  }
  if (!states_valid && tier.route != VOXE_ROUTE_SCATTER) {
    // the caller's workspace does not hold this call's forward states (region route: segment tables too): re-march, no outputs
    PhaseTimer t(PH_FWD, s);
    const FwdArgs f = fwd_args(p, tier, c, nullptr, true);
    if (tier.region) launch_fwd_region(dg, dc, cfg->sh_degree, cfg->render_diffuse, f, at<char>(workspace, l.region_off), s);
    else launch_fwd(dg, dc, cfg->sh_degree, cfg->render_diffuse, f, s);
  }
  bool bricked = false;
  PhaseTimer t(PH_BWD, s);
  if (tier.route == VOXE_ROUTE_DETERMINISTIC) {
    // (the fixed-point region must start cleared: the finalize pass leaves it so, the first use clears it here)
    if (hipMemsetAsync(a.gdet, 0, l.det_bytes, s) != hipSuccess) return VOXE_ERR_LAUNCH;
    launch_bwd_tile(dg, dc, cfg->sh_degree, cfg->render_diffuse, a, s);
  } else if (tier.route == VOXE_ROUTE_REGION) {
    launch_bwd_region(dg, dc, cfg->sh_degree, cfg->render_diffuse, a, at<char>(workspace, l.region_off), s);
  } else if (tier.route == VOXE_ROUTE_TILE) {
    launch_bwd_tile(dg, dc, cfg->sh_degree, cfg->render_diffuse, a, s);
  } else if (tier.route == VOXE_ROUTE_PACKED_SCATTER) {
    launch_bwd_packed_scatter(dg, dc, cfg->sh_degree, cfg->render_diffuse, a, s);
    bricked = !cfg->linear_grad;  // that kernel accumulates into the bricked layout unless asked otherwise
  } else {
    launch_bwd(dg, dc, cfg->sh_degree, cfg->render_diffuse, a, s);
  }
  *grad_layout = bricked ? VOXE_GRAD_BRICKED : VOXE_GRAD_LINEAR;
  return finish();
}
}  // namespace

extern "C" {

int voxe_render_fwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o,
                    const float* rays_d, int64_t R, const float* jitter, float* colour, float* depth,
                    float* acc, float* disparity, void* workspace, size_t workspace_bytes,
                    void* stream) {
  RenderPlan p;
  const int st = plan_render(grid, cfg, R, jitter, nullptr, &p);
  if (st) return st;
  return render_fwd(p, RenderCall{grid, cfg, rays_o, rays_d, R, jitter, workspace, workspace_bytes, (hipStream_t)stream, nullptr, false, /*drop_hint=*/true},
                    FwdOutputs{colour, depth, acc, disparity});
}

int voxe_render_bwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o,
                    const float* rays_d, int64_t R, const float* jitter, const float* colour,
                    const float* depth, const float* acc, const float* d_colour, const float* d_depth,
                    const float* d_acc, float* d_densities, float* d_features, int32_t accumulate,
                    void* workspace, size_t workspace_bytes, void* stream) {
  RenderPlan p;
  const int st = plan_bwd(grid, cfg, R, jitter, rays_o, rays_d, colour, depth, acc, d_colour, &p);
  if (st) return st;
  if (!d_densities && !d_features) return VOXE_OK;
  hipStream_t s = (hipStream_t)stream;
  int32_t layout = VOXE_GRAD_ANY;
  const int rc = render_bwd(p, RenderCall{grid, cfg, rays_o, rays_d, R, jitter, workspace, workspace_bytes, s, nullptr, false, /*drop_hint=*/true}, colour, depth, acc,
                            d_colour, d_depth, d_acc, d_densities != nullptr, d_features != nullptr, true, &layout, nullptr, 0);
  if (rc) return rc;
  { PhaseTimer t(PH_UNPACK, s); launch_unpack_any(grid, at<const float>(workspace, p.l.grad_off), d_densities, d_features, accumulate, layout == VOXE_GRAD_BRICKED ? 1 : 0, s); }
  return finish();
}

int voxe_render_bwd_acc(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o, const float* rays_d,
                        int64_t R, const float* jitter, const float* colour, const float* depth, const float* acc,
                        const float* d_colour, const float* d_depth, const float* d_acc, int32_t want_densities,
                        int32_t want_features, int32_t zero_first, int32_t* grad_layout, void* workspace,
                        size_t workspace_bytes, void* stream) {
  return voxe_render_bwd_acc_into(grid, cfg, rays_o, rays_d, R, jitter, colour, depth, acc, d_colour, d_depth, d_acc, want_densities,
                                  want_features, zero_first, grad_layout, workspace, workspace_bytes, nullptr, 0, stream);
}

int voxe_render_bwd_acc_into(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o, const float* rays_d,
                             int64_t R, const float* jitter, const float* colour, const float* depth, const float* acc,
                             const float* d_colour, const float* d_depth, const float* d_acc, int32_t want_densities,
                             int32_t want_features, int32_t zero_first, int32_t* grad_layout, void* workspace,
                             size_t workspace_bytes, void* grad_workspace, size_t grad_workspace_bytes, void* stream) {
  RenderPlan p;
  const int st = plan_bwd(grid, cfg, R, jitter, rays_o, rays_d, colour, depth, acc, d_colour, &p);
  if (st) return st;
  if (!grad_layout) return VOXE_ERR_NULL_POINTER;
  return render_bwd(p, RenderCall{grid, cfg, rays_o, rays_d, R, jitter, workspace, workspace_bytes, (hipStream_t)stream, nullptr, false, /*drop_hint=*/true}, colour, depth,
                    acc, d_colour, d_depth, d_acc, want_densities != 0, want_features != 0, zero_first != 0, grad_layout, grad_workspace,
                    grad_workspace_bytes);
}

// the two answers below are nominal: given the workspace voxe_workspace_bytes asks for
int voxe_render_bwd_layout(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R) {
  RenderPlan p;
  const int st = plan_render(grid, cfg, R, nullptr, nullptr, &p);
  if (st) return st < -1 ? st : VOXE_ERR_BAD_SHAPE;
  return p.grad_layout();
}

int voxe_render_route(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R) {
  RenderPlan p;
  const int st = plan_render(grid, cfg, R, nullptr, nullptr, &p);
  if (st) return st < -1 ? st : VOXE_ERR_BAD_SHAPE;
  return p.route;
}

int voxe_disparity_bwd(const float* depth, const float* acc, const float* d_disparity, const float* d_depth_in,
                       const float* d_acc_in, float* d_depth_out, float* d_acc_out, int64_t R, void* stream) {
  if (R < 0) return VOXE_ERR_BAD_SHAPE;
  if (R > 0 && (!depth || !acc || !d_disparity || !d_depth_out || !d_acc_out)) return VOXE_ERR_NULL_POINTER;
  launch_disparity_bwd(depth, acc, d_disparity, d_depth_in, d_acc_in, d_depth_out, d_acc_out, R, (hipStream_t)stream);
  return finish();
}

namespace {
struct ReconLayout { size_t subset, rays_o, rays_d, target, out[2], d_colour[2], partial, out2, d_colour2, batch2, total; };
ReconLayout recon_layout(int64_t B) {
  ReconLayout l;
  Carve cv;
  const size_t b = (size_t)(B > 0 ? B : 0);
  l.subset = cv.take(b * sizeof(int64_t));
  l.rays_o = cv.take(b * 3 * sizeof(float));
  l.rays_d = cv.take(b * 3 * sizeof(float));
  l.target = cv.take(b * 3 * sizeof(float));
  const size_t batch_bytes = cv.off;
  for (int i = 0; i < 2; ++i) l.out[i] = cv.take(b * 5 * sizeof(float));        // colour [B,3] | depth [B] | acc [B]
  for (int i = 0; i < 2; ++i) l.d_colour[i] = cv.take(b * 3 * sizeof(float));
  l.partial = cv.take(l1_scratch_bytes());
  // paired render: colour [2B,3] | depth [2B] | acc [2B], d_colour [2B,3]
  l.out2 = cv.take(2 * b * 5 * sizeof(float));
  l.d_colour2 = cv.take(2 * b * 3 * sizeof(float));
  // the same four buffers again, behind everything else: the batch voxe_recon_prefetch assembles ahead of its iteration
  l.batch2 = cv.take(batch_bytes);
  l.total = cv.off;
  return l;
}

ReconKey recon_key(const VoxeGridDesc* grid, const VoxeRenderCfg* pc, const PairSpec& pair, const VoxeRenderCfg* cfg, const VoxeReconStep* rs,
                   const float* rays_o, const float* rays_d, size_t workspace_bytes, const void* workspace2, size_t workspace2_bytes,
                   const void* scratch, size_t scratch_bytes) {
  ReconKey k;
  memset(&k, 0, sizeof(k));
  k.fwd = make_stamp(grid, pc, rays_o, rays_d, 2 * rs->batch, nullptr, workspace_bytes, pair);
  k.poses = rs->poses; k.image_rows = rs->image_rows; k.images = rs->images; k.workspace2 = workspace2; k.scratch = scratch;
  k.subset_offset = cfg->rng_offset; k.ws2bytes = workspace2_bytes; k.scbytes = scratch_bytes;
  k.batch = rs->batch; k.H = rs->H; k.W = rs->W; k.K = rs->K; k.num_images = rs->num_images; k.focal = rs->focal;
  return k;
}
// the paired render's cfg / jitter pair of an iteration whose caller passed `cfg`
VoxeRenderCfg recon_pair_cfg(const VoxeRenderCfg* cfg) {
  VoxeRenderCfg pc = *cfg;
  pc.ray_state_valid = 0;
  pc.rng_offset = cfg->rng_offset + 1;
  pc.render_diffuse = 0;
  pc.linear_grad = 1;
  pc.reuse_packed_grid = 0;      // (not part of any key; the step sets it itself)
  return pc;
}
struct ReconBatchPtrs { int64_t* subset; float *rays_o, *rays_d, *target; };
ReconBatchPtrs recon_batch_ptrs(const ReconLayout& l, void* scratch, int slot) {
  void* sc = at<char>(scratch, slot ? l.batch2 : 0);
  return ReconBatchPtrs{at<int64_t>(sc, l.subset), at<float>(sc, l.rays_o), at<float>(sc, l.rays_d), at<float>(sc, l.target)};
}
// batch assembly: keyed subset of the K * H * W pixels -> rays + target pixels (one launch; same streams as voxe_random_subset,
// voxe_cast_rays_indexed and the pixel gather)
void assemble_recon_batch(const VoxeRenderCfg* cfg, const VoxeReconStep* rs, const ReconBatchPtrs& bp, hipStream_t st) {
  launch_recon_batch(rs->batch, cfg->seed, cfg->rng_offset, rs->H, rs->W, rs->focal, rs->K, rs->poses, rs->images,
                     (const long long*)rs->image_rows, rs->num_images, (long long*)bp.subset, bp.rays_o, bp.rays_d, bp.target, st);
}
int recon_check(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const VoxeReconStep* rs) {
  if (!grid || !cfg || !rs || !rs->poses || !rs->images || !rs->losses) return VOXE_ERR_NULL_POINTER;
  if (grid->feature_kind != VOXE_FEAT_SH) return VOXE_ERR_UNSUPPORTED;
  if (rs->H <= 0 || rs->W <= 0 || rs->K <= 0 || rs->batch <= 0 || rs->batch > (int64_t)rs->K * rs->H * rs->W)
    return VOXE_ERR_BAD_SHAPE;
  if (rs->num_images <= 0 || (!rs->image_rows && rs->K > rs->num_images)) return VOXE_ERR_BAD_SHAPE;
  if (cfg->image_width != 0 || cfg->image_height != 0 || cfg->deterministic) return VOXE_ERR_UNSUPPORTED;   // a random batch has no image order
  if ((int64_t)rs->K * rs->H * rs->W > (1ll << 31)) return VOXE_ERR_BAD_SHAPE;
  return VOXE_OK;
}
}  // namespace

size_t voxe_recon_scratch_bytes(int64_t batch) { return batch > 0 ? recon_layout(batch).total : 0; }

int voxe_recon_prefetch(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const VoxeReconStep* rs, void* workspace,
                        size_t workspace_bytes, void* workspace2, size_t workspace2_bytes, void* scratch, size_t scratch_bytes,
                        void* stream) {
  const int chk = recon_check(grid, cfg, rs);
  if (chk) return chk;
  // only the paired render of SH-0 grids has tables worth assembling ahead; everything else: the hint is dropped
  if (!(rs->diffuse_regularisation && cfg->sh_degree == 0) || !workspace || !workspace2 || !scratch) return VOXE_OK;
  const int64_t B = rs->batch;
  const ReconLayout l = recon_layout(B);
  if (scratch_bytes < l.total) return VOXE_ERR_WORKSPACE;
  const VoxeRenderCfg pc = recon_pair_cfg(cfg);
  const PairSpec pair{B, cfg->rng_offset + 2};
  RenderPlan plan;
  (void)plan_render(grid, &pc, 2 * B, nullptr, &pair, &plan);   // (a render the plan refuses takes no region route: the hint is dropped)
  if (!plan.tier(workspace_bytes).region || !plan.tier(workspace2_bytes).region) return VOXE_OK;
  const int st = g_hints.issue(workspace, (hipStream_t)stream, [&](int slot, hipStream_t side) {
    const ReconBatchPtrs bp = recon_batch_ptrs(l, scratch, slot);
    assemble_recon_batch(cfg, rs, bp, side);
    launch_bin_region(plan.dg, plan.dc, bp.rays_o, bp.rays_d, nullptr, at<char>(slot ? workspace2 : workspace, plan.l.region_off), side);
    return recon_key(grid, &pc, pair, cfg, rs, bp.rays_o, bp.rays_d, workspace_bytes, workspace2, workspace2_bytes, scratch, scratch_bytes);
  });
  return st ? st : finish();
}

int voxe_recon_prefetch_stats(int64_t* out) {
  if (!out) return VOXE_ERR_NULL_POINTER;
  g_hints.stats(out);
  return VOXE_OK;
}

int voxe_recon_step(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const VoxeReconStep* rs, void* workspace,
                    size_t workspace_bytes, void* workspace2, size_t workspace2_bytes, void* scratch, size_t scratch_bytes,
                    void* stream) {
  const int chk = recon_check(grid, cfg, rs);
  if (chk) return chk;
  const int nrender = rs->diffuse_regularisation ? 2 : 1;
  if (nrender == 2 && !workspace2) return VOXE_ERR_WORKSPACE;
  const ReconLayout l = recon_layout(rs->batch);
  if (!scratch || scratch_bytes < l.total) return VOXE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t B = rs->batch;
  int st = VOXE_OK;
  const auto adam_step = [&]() {
    return voxe_grid_adam_step(grid, VOXE_GRAD_LINEAR, 0, grid->X, nullptr, nullptr, rs->exp_avg_densities,
                               rs->exp_avg_sq_densities, rs->exp_avg_features, rs->exp_avg_sq_features, rs->lr, rs->beta1,
                               rs->beta2, rs->eps, rs->step_densities, rs->step_features, nullptr, workspace, workspace_bytes, stream);
  };
  // a prefetch pending on this workspace: taken iff it was made for exactly this call
  const ReconHints::Pending pend = g_hints.begin_step(workspace, s);
  // SH-0 grids: the diffuse render is the specular kernel with another jitter stream -- both renders as ONE launch of 2 B
  // rays on the space-binned route (one binning pass, one forward, one backward; no second packed grid).  32 768-ray
  // batches leave the chip half empty and the binning / scan / fold passes are launch-latency sized: r04, 160^3,
  // 1.15 -> see profiles/r04_recon_bench.txt.  Needs `workspace` sized for 2 B rays (voxe_workspace_bytes(grid, cfg, 2 B)).
  if (nrender == 2 && cfg->sh_degree == 0) {
    VoxeRenderCfg pc = recon_pair_cfg(cfg);
    pc.reuse_packed_grid = cfg->reuse_packed_grid;
    const PairSpec pair{B, cfg->rng_offset + 2};
    RenderPlan plan;
    (void)plan_render(grid, &pc, 2 * B, nullptr, &pair, &plan);   // (refused: no region route, the general route below reports it)
    if (plan.tier(workspace_bytes).region) {
      bool prebinned = false;
      if (pend.valid) {
        const ReconBatchPtrs pp = recon_batch_ptrs(l, scratch, pend.slot);
        const ReconKey k = recon_key(grid, &pc, pair, cfg, rs, pp.rays_o, pp.rays_d, workspace_bytes, workspace2, workspace2_bytes, scratch, scratch_bytes);
        prebinned = memcmp(&k, &pend.key, sizeof(k)) == 0;
        g_hints.count(prebinned);
      }
      const int slot = prebinned ? pend.slot : 0;
      const ReconBatchPtrs bp = recon_batch_ptrs(l, scratch, slot);
      if (!prebinned) assemble_recon_batch(cfg, rs, bp, s);
      float* colour = at<float>(scratch, l.out2);
      float *depth = colour + 6 * B, *acc = depth + 2 * B;
      float* d_colour = at<float>(scratch, l.d_colour2);
      const RenderCall call{grid, &pc, bp.rays_o, bp.rays_d, 2 * B, nullptr, workspace, workspace_bytes, s,
                            /*region_tables=*/slot ? at<void>(workspace2, plan.l.region_off) : nullptr, prebinned};
      st = render_fwd(plan, call, FwdOutputs{colour, depth, acc, nullptr});
      if (st) return st;
      g_hints.forward_enqueued(workspace, slot, s);
      launch_l1_loss_grad_n(colour, bp.target, 3 * B, 2, d_colour, rs->losses, at<char>(scratch, l.partial), s);   // both renders, one launch pair
      pc.ray_state_valid = 1;
      pc.reuse_packed_grid = 1;
      int32_t layout = VOXE_GRAD_ANY;
      st = render_bwd(plan, call, colour, depth, acc, d_colour, nullptr, nullptr, rs->exp_avg_densities != nullptr,
                      rs->exp_avg_features != nullptr, rs->zero_gradient_first != 0, &layout, nullptr, 0);
      if (st) return st;
      if (layout != VOXE_GRAD_LINEAR) return VOXE_ERR_UNSUPPORTED;
      return adam_step();
    }
  }
  const ReconBatchPtrs bp = recon_batch_ptrs(l, scratch, 0);
  VoxeRenderCfg rc[2] = {*cfg, *cfg};
  RenderPlan plan[2]; RenderCall call[2];
  // plan both renders and check what their forward and backward will ask of the workspaces BEFORE the first launch: a refused
  // step leaves the scratch, the losses and both workspaces as it found them
  for (int i = 0; i < nrender; ++i) {
    rc[i].rng_offset = cfg->rng_offset + 1 + (uint64_t)i;
    rc[i].ray_state_valid = 0;
    rc[i].render_diffuse = i == 1 ? 1 : cfg->render_diffuse;
    rc[i].linear_grad = 1;                         // both renders write ONE gradient layout, whatever kernel runs
    if (i == 1) rc[i].reuse_packed_grid = 0;       // the second workspace still holds the previous iteration's grid
    st = plan_render(grid, &rc[i], B, nullptr, nullptr, &plan[i]);
    if (st) return st;
    void* const ws = i == 0 ? workspace : workspace2;
    if (!ws || (i == 0 ? workspace_bytes : workspace2_bytes) < plan[i].l.total) return VOXE_ERR_WORKSPACE;
  }
  assemble_recon_batch(cfg, rs, bp, s);
  for (int i = 0; i < nrender; ++i) {
    float* colour = at<float>(scratch, l.out[i]);
    float *depth = colour + 3 * B, *acc = depth + B;
    call[i] = RenderCall{grid, &rc[i], bp.rays_o, bp.rays_d, B, nullptr, i == 0 ? workspace : workspace2, i == 0 ? workspace_bytes : workspace2_bytes, s};
    st = render_fwd(plan[i], call[i], FwdOutputs{colour, depth, acc, nullptr});
    if (st) return st;
    launch_l1_loss_grad(colour, bp.target, 3 * B, at<float>(scratch, l.d_colour[i]), rs->losses + 2 * i, at<char>(scratch, l.partial), s);
  }
  for (int i = 0; i < nrender; ++i) {
    float* colour = at<float>(scratch, l.out[i]);
    float *depth = colour + 3 * B, *acc = depth + B;
    rc[i].ray_state_valid = 1;                     // the forward above left this render's states in its workspace
    rc[i].reuse_packed_grid = 1;
    int32_t layout = VOXE_GRAD_ANY;
    st = render_bwd(plan[i], call[i], colour, depth, acc, at<const float>(scratch, l.d_colour[i]), nullptr, nullptr,
                    rs->exp_avg_densities != nullptr, rs->exp_avg_features != nullptr,
                    /*zero_first=*/i == 0 && rs->zero_gradient_first, &layout, i == 0 ? nullptr : workspace, i == 0 ? 0 : workspace_bytes);
    if (st) return st;
    if (layout != VOXE_GRAD_LINEAR) return VOXE_ERR_UNSUPPORTED;
  }
  return adam_step();
}

namespace {
struct RefineLayout { size_t out, d_render, tv_grad, tv_scratch, l1_scratch, total; };
RefineLayout refine_layout(const VoxeGridDesc* g, int64_t R) {
  RefineLayout l;
  Carve cv;
  const size_t r = (size_t)(R > 0 ? R : 0);
  l.out = cv.take(r * 4 * sizeof(float));          // attn [R] | depth [R] | acc [R] | (spare)
  l.d_render = cv.take(r * sizeof(float));
  l.tv_grad = cv.take((size_t)g->X * g->Y * g->Z * sizeof(float));
  l.tv_scratch = cv.take(tv_scratch_bytes(g->X, g->Y, g->Z, 1));
  l.l1_scratch = cv.take(attn_l1_scratch_bytes());
  l.total = cv.off;
  return l;
}
}  // namespace

size_t voxe_attn_masked_l1_scratch_bytes(void) { return attn_l1_scratch_bytes(); }

int voxe_attn_masked_l1(const float* render, const float* attn_map, int64_t n, float* d_render, float* loss_out, void* scratch,
                        size_t scratch_bytes, void* stream) {
  if (n < 0) return VOXE_ERR_BAD_SHAPE;
  if (n == 0) return VOXE_OK;
  if (!render || !attn_map || !d_render) return VOXE_ERR_NULL_POINTER;
  if (!scratch || scratch_bytes < attn_l1_scratch_bytes()) return VOXE_ERR_WORKSPACE;
  launch_attn_masked_l1(render, attn_map, n, d_render, loss_out, scratch, (hipStream_t)stream);
  return finish();
}

size_t voxe_attn_refine_scratch_bytes(const VoxeGridDesc* grid, int64_t R) {
  if (!grid || grid->X <= 0 || grid->Y <= 0 || grid->Z <= 0 || R <= 0) return 0;
  return refine_layout(grid, R).total;
}

int voxe_attn_refine_step(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const VoxeAttnRefineStep* rs, const float* rays_o,
                          const float* rays_d, int64_t R, void* workspace, size_t workspace_bytes, void* scratch,
                          size_t scratch_bytes, void* stream) {
  if (!grid || !cfg || !rs || !rays_o || !rays_d || !rs->attn_map || !rs->exp_avg || !rs->exp_avg_sq) return VOXE_ERR_NULL_POINTER;
  if (grid->feature_kind != VOXE_FEAT_ATTN) return VOXE_ERR_UNSUPPORTED;
  if (R <= 0) return VOXE_ERR_BAD_SHAPE;
  if (cfg->deterministic) return VOXE_ERR_UNSUPPORTED;
  const RefineLayout l = refine_layout(grid, R);
  if (!scratch || scratch_bytes < l.total) return VOXE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* attn = rs->attn_render ? rs->attn_render : at<float>(scratch, l.out);
  float *depth = at<float>(scratch, l.out) + R, *acc = depth + R;
  float* d_render = at<float>(scratch, l.d_render);
  float* tv_grad = at<float>(scratch, l.tv_grad);
  VoxeRenderCfg rc = *cfg;
  rc.ray_state_valid = 0;
  RenderPlan plan;
  int st = plan_render(grid, &rc, R, nullptr, nullptr, &plan);
  if (st) return st;
  // (the backward's need, checked before the forward runs: a refused step has written nothing)
  if (!workspace || workspace_bytes < plan.l.total) return VOXE_ERR_WORKSPACE;
  const RenderCall call{grid, &rc, rays_o, rays_d, R, nullptr, workspace, workspace_bytes, s, nullptr, false, /*drop_hint=*/true};
  st = render_fwd(plan, call, FwdOutputs{attn, depth, acc, nullptr});
  if (st) return st;
  launch_attn_masked_l1(attn, rs->attn_map, R, d_render, rs->losses, at<char>(scratch, l.l1_scratch), s);
  rc.ray_state_valid = 1;
  rc.reuse_packed_grid = 1;
  int32_t layout = VOXE_GRAD_ANY;
  st = render_bwd(plan, call, attn, depth, acc, d_render, nullptr, nullptr, /*want_d=*/false, /*want_f=*/true,
                  rs->zero_gradient_first != 0, &layout, nullptr, 0);
  if (st) return st;
  // the TV stencil reads the parameters BEFORE the step overwrites them: its gradient goes through the step's extra-gradient input
  const float* extra = nullptr;
  if (rs->tv_weight != 0.0f || (rs->losses && rs->tv_loss_always)) {
    launch_tv(grid->features, grid->X, grid->Y, grid->Z, 1, rs->tv_weight, rs->losses ? rs->losses + 1 : nullptr,
              rs->tv_weight != 0.0f ? tv_grad : nullptr, 0, at<char>(scratch, l.tv_scratch), s);
    if (rs->tv_weight != 0.0f) extra = tv_grad;
  }
  return voxe_grid_adam_step(grid, layout, 0, grid->X, nullptr, extra, nullptr, nullptr, rs->exp_avg, rs->exp_avg_sq, rs->lr,
                             rs->beta1, rs->beta2, rs->eps, rs->step, rs->step, nullptr, workspace, workspace_bytes, stream);
}

int voxe_clock_probe(int32_t spin, double* shader_hz, void* stream) {
  if (!shader_hz) return VOXE_ERR_NULL_POINTER;
  *shader_hz = run_clock_probe(spin, (hipStream_t)stream);
  return *shader_hz > 0.0 ? finish() : VOXE_ERR_LAUNCH;
}

int voxe_region_debug_layout(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R, int64_t out[17]) {
  if (!out) return VOXE_ERR_NULL_POINTER;
  RenderPlan p;
  const int st = plan_render(grid, cfg, R, nullptr, nullptr, &p);
  if (st) return st;
  if (!p.region) return VOXE_ERR_UNSUPPORTED;   // (grid, cfg, R) does not take the space-binned route
  long long t[16];
  region_debug_layout(grid->X, grid->Y, grid->Z, R, cfg->num_samples, t);
  out[0] = (int64_t)p.l.region_off;
  for (int i = 0; i < 16; ++i) out[1 + i] = t[i];
  return VOXE_OK;
}

size_t voxe_workspace_grad_offset(const VoxeGridDesc* grid) { return grid_layout(grid).grad_off; }
size_t voxe_workspace_grad_bytes(const VoxeGridDesc* grid) { return grid_layout(grid).grad_bytes(); }

int voxe_grid_adam_step(const VoxeGridDesc* grid, int32_t grad_layout, int32_t x_begin, int32_t x_end,
                        const float* extra_d_densities,
                        const float* extra_d_features, float* exp_avg_d, float* exp_avg_sq_d, float* exp_avg_f,
                        float* exp_avg_sq_f, float lr, float beta1, float beta2, float eps, int64_t step,
                        int64_t step_features, const VoxeGridRegularisers* reg, void* workspace, size_t workspace_bytes,
                        void* stream) {
  if (!grid || !grid->densities || !grid->features) return VOXE_ERR_NULL_POINTER;
  if (grid->X <= 0 || grid->Y <= 0 || grid->Z <= 0 || grid->F <= 0 || step < 1 || step_features < 0) return VOXE_ERR_BAD_SHAPE;
  if ((long long)grid->X * grid->Y * grid->Z * (grid->F + 1) >= (1LL << 31)) return VOXE_ERR_BAD_SHAPE;
  if (x_begin < 0 || x_end > grid->X || x_begin > x_end) return VOXE_ERR_BAD_SHAPE;
  if (grad_layout == VOXE_GRAD_BRICKED && (x_begin & 1) && x_begin != x_end) return VOXE_ERR_BAD_SHAPE;
  if ((exp_avg_d == nullptr) != (exp_avg_sq_d == nullptr) || (exp_avg_f == nullptr) != (exp_avg_sq_f == nullptr))
    return VOXE_ERR_NULL_POINTER;
  if (grad_layout != VOXE_GRAD_LINEAR && grad_layout != VOXE_GRAD_BRICKED && grad_layout != VOXE_GRAD_ANY)
    return VOXE_ERR_UNSUPPORTED;
  const WsLayout l = grid_layout(grid);
  if (!workspace || workspace_bytes < l.state_off) return VOXE_ERR_WORKSPACE;
  DclTerm dcl;
  const long long nvox_all = (long long)grid->X * grid->Y * grid->Z;
  if (reg && reg->dcl_reference && reg->density_kind == VOXE_DREG_CORRELATION) {
    // moments over the WHOLE grid of the current parameters; the gradient is evaluated inside the step
    const long long n = nvox_all;
    if (x_begin != 0 || x_end != grid->X || !exp_avg_d) return VOXE_ERR_UNSUPPORTED;
    if (!reg->scratch || reg->scratch_bytes < dcl_scratch_bytes(n)) return VOXE_ERR_WORKSPACE;
    dcl.b = reg->dcl_reference;
    dcl.stats = launch_dcl_moments(grid->densities, reg->dcl_reference, n, reg->dcl_weight, reg->dcl_loss, reg->scratch,
                                   (hipStream_t)stream);
  } else if (reg && reg->dcl_reference) {
    // l2_mode / l1_mode (sds_trainer.py:494-503): per-voxel terms, no statistics; a reduction only for the logged value
    if (reg->density_kind != VOXE_DREG_L2 && reg->density_kind != VOXE_DREG_L1) return VOXE_ERR_UNSUPPORTED;
    if (!exp_avg_d) return VOXE_ERR_UNSUPPORTED;
    const long long plane = (long long)grid->Y * grid->Z;
    if (reg->dcl_loss) {
      if (!reg->scratch || reg->scratch_bytes < dcl_scratch_bytes(nvox_all)) return VOXE_ERR_WORKSPACE;
      if (x_begin == x_end && hipMemsetAsync(reg->dcl_loss, 0, sizeof(float), (hipStream_t)stream) != hipSuccess) return VOXE_ERR_LAUNCH;
      if (x_begin < x_end)
        launch_density_diff(grid->densities + x_begin * plane, reg->dcl_reference + x_begin * plane, (x_end - x_begin) * plane,
                            reg->density_kind, 0.0f, reg->dcl_loss, (float)(1.0 / (double)nvox_all), nullptr, 0, reg->scratch,
                            (hipStream_t)stream);
    }
    dcl.b = reg->dcl_reference;
    dcl.kind = reg->density_kind;
    dcl.k = (float)((reg->density_kind == VOXE_DREG_L2 ? 2.0 : 1.0) * (double)reg->dcl_weight / (double)nvox_all);
  }
  if (reg && reg->feat_reference) {
    // _feature_correlation_loss (sds_trainer.py:526-534): per voxel inside the step (texels of up to 4 channels)
    if (grid->F > 3 || !exp_avg_f) return VOXE_ERR_UNSUPPORTED;
    const long long plane = (long long)grid->Y * grid->Z;
    if (reg->feat_loss) {
      if (!reg->scratch || reg->scratch_bytes < dcl_scratch_bytes(nvox_all)) return VOXE_ERR_WORKSPACE;
      if (x_begin == x_end && hipMemsetAsync(reg->feat_loss, 0, sizeof(float), (hipStream_t)stream) != hipSuccess) return VOXE_ERR_LAUNCH;
      if (x_begin < x_end)
        launch_feature_correlation(grid->features + x_begin * plane * grid->F, reg->feat_reference + x_begin * plane * grid->F,
                                   (x_end - x_begin) * plane, grid->F, 0.0f, reg->feat_loss, nullptr, 0, reg->scratch,
                                   (hipStream_t)stream);
    }
    dcl.fref = reg->feat_reference;
    dcl.fk = 2.0f * reg->feat_weight;
  }
  if (x_begin == x_end) return VOXE_OK;
  // the parameters move: the per-ray states a forward left in this workspace no longer describe the grid -- a backward that still
  // claims ray_state_valid = 1 afterwards is served by a re-march
  forget_stamp(workspace);
  forget_stamps_of(grid->densities);   // (sibling workspaces / a grad_workspace's owner rendered the same tensors)
  forget_stamps_of(grid->features);
  if (!launch_grid_adam(grid, grad_layout == VOXE_GRAD_BRICKED, x_begin, x_end, at<float>(workspace, l.grad_off),
                        extra_d_densities, extra_d_features, exp_avg_d, exp_avg_sq_d, exp_avg_f, exp_avg_sq_f, lr, beta1,
                        beta2, eps, step, step_features > 0 ? step_features : step,
                        at<float>(workspace, l.packed_off), (hipStream_t)stream, dcl))
    return VOXE_ERR_UNSUPPORTED;
  return finish();
}

int voxe_sample_probe(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o,
                      const float* rays_d, int64_t R, const float* jitter, int32_t* idx,
                      uint8_t* inside, float* zvals, float* sigma, float* rad, void* workspace,
                      size_t workspace_bytes, void* stream) {
  RenderPlan p;
  const int st = plan_render(grid, cfg, R, jitter, nullptr, &p);
  if (st) return st;
  if (R > 0 && (!rays_o || !rays_d)) return VOXE_ERR_NULL_POINTER;
  if (!workspace || workspace_bytes < p.l.fwd_total) return VOXE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* packed = at<float>(workspace, p.l.packed_off);
  if (!cfg->reuse_packed_grid) launch_pack_any(grid, packed, s);
  if (R == 0) return finish();
  ProbeArgs a{packed, rays_o, rays_d, jitter, idx, inside, zvals, sigma, rad};
  launch_probe(p.dg, p.dc, cfg->sh_degree, cfg->render_diffuse, a, s);
  return finish();
}

int voxe_query_fwd(const VoxeGridDesc* grid, const float* points, int64_t N, float* out,
                   int32_t reuse_packed_grid, void* workspace, size_t workspace_bytes, void* stream) {
  const int st = validate_grid_only(grid);
  if (st) return st;
  if (N < 0) return VOXE_ERR_BAD_SHAPE;
  if (N > 0 && (!points || !out)) return VOXE_ERR_NULL_POINTER;
  const WsLayout l = grid_layout(grid);
  if (!workspace || workspace_bytes < l.fwd_total) return VOXE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* packed = at<float>(workspace, l.packed_off);
  if (!reuse_packed_grid) launch_pack_any(grid, packed, s);
  if (N == 0) return finish();
  DevGrid dg;
  grid_to_dev(grid, &dg);
  launch_query(dg, grid->F + 1, packed, points, N, out, nullptr, nullptr, false, false, s);
  return finish();
}

int voxe_query_bwd(const VoxeGridDesc* grid, const float* points, int64_t N, const float* d_out,
                   float* d_densities, float* d_features, int32_t accumulate, int32_t reuse_packed_grid,
                   void* workspace, size_t workspace_bytes, void* stream) {
  const int st = validate_grid_only(grid);
  if (st) return st;
  if (N < 0) return VOXE_ERR_BAD_SHAPE;
  if (N > 0 && (!points || !d_out)) return VOXE_ERR_NULL_POINTER;
  if (!d_densities && !d_features) return VOXE_OK;
  const WsLayout l = grid_layout(grid);
  if (!workspace || workspace_bytes < l.total) return VOXE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* packed = at<float>(workspace, l.packed_off);
  float* gpacked = at<float>(workspace, l.grad_off);
  if (!reuse_packed_grid) launch_pack_any(grid, packed, s);
  if (hipMemsetAsync(gpacked, 0, l.grad_bytes(), s) != hipSuccess) return VOXE_ERR_LAUNCH;
  if (N > 0) {
    DevGrid dg;
    grid_to_dev(grid, &dg);
    launch_query(dg, grid->F + 1, packed, points, N, nullptr, d_out, gpacked, d_densities != nullptr,
                 d_features != nullptr, s);
  }
  launch_unpack_any(grid, gpacked, d_densities, d_features, accumulate, 0, s);
  return finish();
}

size_t voxe_dcl_scratch_bytes(int64_t n) { return dcl_scratch_bytes(n); }

int voxe_dcl_fwd_bwd(const float* a, const float* b, int64_t n, float grad_scale, float* loss_out,
                     float* d_a, int32_t accumulate, void* scratch, size_t scratch_bytes,
                     void* stream) {
  if (!a || !b || !loss_out) return VOXE_ERR_NULL_POINTER;
  if (n <= 0) return VOXE_ERR_BAD_SHAPE;
  if (!scratch || scratch_bytes < dcl_scratch_bytes(n)) return VOXE_ERR_WORKSPACE;
  launch_dcl(a, b, n, grad_scale, loss_out, d_a, accumulate, scratch, (hipStream_t)stream);
  return finish();
}

int voxe_density_diff_fwd_bwd(const float* a, const float* b, int64_t n, int32_t kind, float grad_scale, float* loss_out,
                              float* d_a, int32_t accumulate, void* scratch, size_t scratch_bytes, void* stream) {
  if (!a || !b) return VOXE_ERR_NULL_POINTER;
  if (n <= 0) return VOXE_ERR_BAD_SHAPE;
  if (kind != VOXE_DREG_L2 && kind != VOXE_DREG_L1) return VOXE_ERR_UNSUPPORTED;
  if (loss_out && (!scratch || scratch_bytes < dcl_scratch_bytes(n))) return VOXE_ERR_WORKSPACE;
  if (!loss_out && !d_a) return VOXE_OK;
  launch_density_diff(a, b, n, kind, grad_scale, loss_out, (float)(1.0 / (double)n), d_a, accumulate, scratch, (hipStream_t)stream);
  return finish();
}

int voxe_feature_correlation_fwd_bwd(const float* f, const float* r, int64_t nvox, int32_t F, float grad_scale, float* loss_out,
                                     float* d_f, int32_t accumulate, void* scratch, size_t scratch_bytes, void* stream) {
  if (!f || !r) return VOXE_ERR_NULL_POINTER;
  if (nvox <= 0 || F < 1 || F > 64) return VOXE_ERR_BAD_SHAPE;
  if (loss_out && (!scratch || scratch_bytes < dcl_scratch_bytes(nvox))) return VOXE_ERR_WORKSPACE;
  if (!loss_out && !d_f) return VOXE_OK;
  launch_feature_correlation(f, r, nvox, F, grad_scale, loss_out, d_f, accumulate, scratch, (hipStream_t)stream);
  return finish();
}

size_t voxe_tv_scratch_bytes(int32_t X, int32_t Y, int32_t Z, int32_t C) {
  return tv_scratch_bytes(X, Y, Z, C);
}

int voxe_tv_fwd_bwd(const float* grid, int32_t X, int32_t Y, int32_t Z, int32_t C, float grad_scale,
                    float* loss_out, float* d_grid, int32_t accumulate, void* scratch,
                    size_t scratch_bytes, void* stream) {
  if (!grid || !loss_out) return VOXE_ERR_NULL_POINTER;
  if (X <= 0 || Y <= 0 || Z <= 0 || C <= 0) return VOXE_ERR_BAD_SHAPE;
  if ((long long)Y * Z * C >= (1ll << 31) - 256) return VOXE_ERR_BAD_SHAPE;   // (32-bit index arithmetic inside an x-plane)
  if (!scratch || scratch_bytes < tv_scratch_bytes(X, Y, Z, C)) return VOXE_ERR_WORKSPACE;
  launch_tv(grid, X, Y, Z, C, grad_scale, loss_out, d_grid, accumulate, scratch, (hipStream_t)stream);
  return finish();
}

int voxe_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, int64_t step, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq) return VOXE_ERR_NULL_POINTER;
  if (n < 0 || step < 1) return VOXE_ERR_BAD_SHAPE;
  forget_stamps_of(param);   // (a later ray_state_valid = 1 over this tensor re-marches)
  launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, (hipStream_t)stream);
  return finish();
}

int voxe_upsample_trilinear(const float* src, int32_t X, int32_t Y, int32_t Z, int32_t C, float* dst,
                            int32_t X2, int32_t Y2, int32_t Z2, void* stream) {
  if (!src || !dst) return VOXE_ERR_NULL_POINTER;
  if (X <= 0 || Y <= 0 || Z <= 0 || C <= 0 || X2 <= 0 || Y2 <= 0 || Z2 <= 0) return VOXE_ERR_BAD_SHAPE;
  if (X2 > 65535 || (long long)Y2 * Z2 * C >= (1ll << 31) - 256) return VOXE_ERR_BAD_SHAPE;   // (grid.y / 32-bit plane index)
  launch_upsample(src, X, Y, Z, C, dst, X2, Y2, Z2, (hipStream_t)stream);
  return finish();
}

// ---- refinement stage ------------------------------------------------------------------------------
static bool refine_dims_ok(int32_t X, int32_t Y, int32_t Z) {
  return X > 0 && Y > 0 && Z > 0 && (long long)X * Y * Z < (1ll << 30);
}

int voxe_graph_build(const float* density_grid, const float* feature_grid, int32_t X, int32_t Y, int32_t Z,
                     int32_t F, float sigma, int32_t dilate_yz, uint8_t* node_mask, int32_t* cap, void* stream) {
  if (!density_grid || !feature_grid || !node_mask || !cap) return VOXE_ERR_NULL_POINTER;
  if (!refine_dims_ok(X, Y, Z) || F <= 0 || !(sigma > 0.0f)) return VOXE_ERR_BAD_SHAPE;
  launch_graph_build(density_grid, feature_grid, X, Y, Z, F, sigma, dilate_yz ? 1 : 0, node_mask, cap,
                     (hipStream_t)stream);
  return finish();
}

size_t voxe_graphcut_scratch_bytes(int32_t X, int32_t Y, int32_t Z) {
  return refine_dims_ok(X, Y, Z) ? graphcut_scratch_bytes(X, Y, Z) : 0;
}

int voxe_graphcut(const uint8_t* node_mask, const int8_t* terminal, int32_t* cap, int32_t X, int32_t Y, int32_t Z,
                  uint8_t* segment, int64_t* flow, void* scratch, size_t scratch_bytes, void* stream) {
  if (!node_mask || !terminal || !cap || !segment || !flow) return VOXE_ERR_NULL_POINTER;
  if (!refine_dims_ok(X, Y, Z)) return VOXE_ERR_BAD_SHAPE;
  if (!scratch || scratch_bytes < graphcut_scratch_bytes(X, Y, Z)) return VOXE_ERR_WORKSPACE;
  if (run_graphcut(node_mask, terminal, cap, X, Y, Z, segment, flow, scratch, (hipStream_t)stream) != hipSuccess)
    return VOXE_ERR_LAUNCH;
  return finish();
}

size_t voxe_cc_scratch_bytes(int32_t X, int32_t Y, int32_t Z, int32_t k) {
  return refine_dims_ok(X, Y, Z) && k >= 0 ? cc_scratch_bytes(X, Y, Z, k) : 0;
}

int voxe_cc_largest_k(const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t k, int32_t* labels,
                      int32_t* num_components, void* scratch, size_t scratch_bytes, void* stream) {
  if (!mask || !labels || !num_components) return VOXE_ERR_NULL_POINTER;
  if (!refine_dims_ok(X, Y, Z) || k < 0 || k > 4096) return VOXE_ERR_BAD_SHAPE;
  if (!scratch || scratch_bytes < cc_scratch_bytes(X, Y, Z, k)) return VOXE_ERR_WORKSPACE;
  launch_cc_largest_k(mask, X, Y, Z, k, labels, num_components, scratch, (hipStream_t)stream);
  return finish();
}

// ---- mesh export ---------------------------------------------------------------------------------------------------
namespace {
// L = post^-1(level) in the pre-post domain; false when level <= post(0) (the zero-padded ring would not be outside)
bool mesh_iso_value(int post, float level, float* L) {
  if (!(level < INFINITY)) return false;   // (NaN, +inf)
  if (post == VOXE_ACT_SOFTPLUS) {
    if (!(level > 0.693147182464599609375f)) return false;   // softplus(0) in float
    *L = level > 20.0f ? level : (float)log(expm1((double)level));
    return *L > 0.0f;
  }
  if (!(level > 0.0f)) return false;
  *L = level;
  return true;
}

int validate_mesh(const VoxeGridDesc* g, float level, void* scratch, size_t scratch_bytes, float* L) {
  if (!g || !g->densities) return VOXE_ERR_NULL_POINTER;
  if (!mesh_dims_ok(g->X, g->Y, g->Z)) return VOXE_ERR_BAD_SHAPE;
  if (g->feature_kind != VOXE_FEAT_SH && g->feature_kind != VOXE_FEAT_ATTN) return VOXE_ERR_UNSUPPORTED;
  if (const int st = grid_acts_status(g)) return st;
  if (!mesh_iso_value(g->density_post_act, level, L)) return VOXE_ERR_BAD_SHAPE;
  if (!scratch || scratch_bytes < mesh_scratch_bytes(g->X, g->Y, g->Z)) return VOXE_ERR_WORKSPACE;
  return VOXE_OK;
}
}  // namespace

size_t voxe_mesh_scratch_bytes(int32_t X, int32_t Y, int32_t Z) {
  return mesh_dims_ok(X, Y, Z) ? mesh_scratch_bytes(X, Y, Z) : 0;
}

int voxe_mesh_count(const VoxeGridDesc* grid, float level, const uint8_t* mask, int64_t* totals, void* scratch,
                    size_t scratch_bytes, void* stream) {
  if (!totals) return VOXE_ERR_NULL_POINTER;
  float L;
  const int st = validate_mesh(grid, level, scratch, scratch_bytes, &L);
  if (st) return st;
  launch_mesh_count(grid, L, mask, totals, scratch, (hipStream_t)stream);
  return finish();
}

int voxe_mesh_emit(const VoxeGridDesc* grid, float level, const uint8_t* mask, float* vertices, int64_t max_vertices,
                   int32_t* faces, int64_t max_faces, void* scratch, size_t scratch_bytes, void* stream) {
  if (max_vertices < 0 || max_faces < 0) return VOXE_ERR_BAD_SHAPE;
  if ((max_vertices > 0 && !vertices) || (max_faces > 0 && !faces)) return VOXE_ERR_NULL_POINTER;
  float L;
  const int st = validate_mesh(grid, level, scratch, scratch_bytes, &L);
  if (st) return st;
  launch_mesh_emit(grid, L, mask, vertices, max_vertices, faces, max_faces, scratch, (hipStream_t)stream);
  return finish();
}


// ---- density-gradient normals ------------------------------------------------------------------------
// the grid checks of validate_grid_only() for a call that reads `densities` only (features / F / feature_kind are ignored)
static int validate_normals_grid(const VoxeGridDesc* g) {
  if (!g || !g->densities) return VOXE_ERR_NULL_POINTER;
  if (const int st = grid_extent_status(g, 1)) return st;
  return grid_acts_status(g);
}

// DevCfg of a call that marches the forward's samples without rendering (normals, visibility): the sampling fields make_dev()
// copies, with make_dev()'s expressions (the forward's depths and jitter stream); everything else 0
static void sampling_cfg_to_dev(const VoxeRenderCfg* cfg, int64_t R, DevCfg* out) {
  DevCfg& dc = *out;
  memset(&dc, 0, sizeof(dc));
  dc.S = cfg->num_samples;
  dc.near = cfg->near; dc.far = cfg->far;
  dc.perturb = cfg->perturb; dc.lindisp = cfg->linear_disparity; dc.aabb_clip = cfg->aabb_clip;
  dc.key0 = (uint32_t)cfg->seed ^ ((uint32_t)cfg->rng_offset * 0x9E3779B1u);
  dc.key1 = (uint32_t)(cfg->seed >> 32) ^ (uint32_t)(cfg->rng_offset >> 32) ^ 0x7F4A7C15u;
  dc.R = R;
  // image order (pixel tiles) only when the image fields describe R exactly; otherwise (or when absent) linear order
  const int64_t W = cfg->image_width, H = cfg->image_height > 0 ? cfg->image_height : (W > 0 ? R / W : 0);
  if (W > 0 && H > 0 && H <= INT32_MAX && R % (W * H) == 0) {
    dc.image_width = (int)W;
    dc.image_height = (int)H;
  }
}

// The prologue of the calls that march the forward's samples over the raw densities (voxe_ray_march.hpp lists them), in two steps
// so that a call can put checks of its own between them: the grid, cfg and the R / num_samples range ...
static int sampling_call_shape(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R) {
  const int st = validate_normals_grid(grid);
  if (st) return st;
  if (!cfg) return VOXE_ERR_NULL_POINTER;
  if (R < 0 || R >= (1LL << 31) || cfg->num_samples <= 0) return VOXE_ERR_BAD_SHAPE;
  return VOXE_OK;
}
// ... then the rays (R == 0: nothing is read, they may be NULL -- an empty tensor has no address) and the device structs
static int sampling_call_rays(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R, const float* rays_o,
                              const float* rays_d, DevGrid* dg, DevCfg* dc) {
  if (R > 0 && (!rays_o || !rays_d)) return VOXE_ERR_NULL_POINTER;
  grid_to_dev(grid, dg);
  sampling_cfg_to_dev(cfg, R, dc);
  return VOXE_OK;
}
static int sampling_call(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R, const float* rays_o, const float* rays_d,
                         DevGrid* dg, DevCfg* dc) {
  const int st = sampling_call_shape(grid, cfg, R);
  return st ? st : sampling_call_rays(grid, cfg, R, rays_o, rays_d, dg, dc);
}
// a *_debug_lanes test aid: the lanes per ray it may pin (0: the library's choice) into that call's pin
static int pin_lanes(int* pin, int32_t lanes) {
  if (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 4 && lanes != 8) return VOXE_ERR_BAD_SHAPE;
  *pin = lanes;
  return VOXE_OK;
}

int voxe_query_normals(const VoxeGridDesc* grid, const float* points, int64_t N, float* normals, void* stream) {
  const int st = validate_normals_grid(grid);
  if (st) return st;
  if (N < 0) return VOXE_ERR_BAD_SHAPE;
  if (N > 0 && (!points || !normals)) return VOXE_ERR_NULL_POINTER;
  if (N == 0) return VOXE_OK;
  DevGrid dg;
  grid_to_dev(grid, &dg);
  launch_query_normals(dg, grid->densities, points, N, normals, (hipStream_t)stream);
  return finish();
}

int voxe_render_normals(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o, const float* rays_d, int64_t R,
                        const float* jitter, float* normals, float* depth, float* acc, void* stream) {
  DevGrid dg;
  DevCfg dc;
  const int st = sampling_call(grid, cfg, R, rays_o, rays_d, &dg, &dc);
  if (st) return st;
  if (R > 0 && !normals) return VOXE_ERR_NULL_POINTER;
  if (R == 0) return VOXE_OK;
  launch_render_normals(dg, dc, grid->densities, rays_o, rays_d, jitter, normals, depth, acc, (hipStream_t)stream);
  return finish();
}

// ---- per-voxel visibility ----------------------------------------------------------------------------
int voxe_visibility_accumulate(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o, const float* rays_d,
                               int64_t R, const float* jitter, float* max_weight, float* max_trans, void* stream) {
  DevGrid dg;
  DevCfg dc;
  const int st = sampling_call(grid, cfg, R, rays_o, rays_d, &dg, &dc);
  if (st) return st;
  if (R == 0 || (!max_weight && !max_trans)) return VOXE_OK;
  launch_visibility_accumulate(dg, dc, grid->densities, rays_o, rays_d, jitter, max_weight, max_trans, (hipStream_t)stream);
  return finish();
}

int voxe_visibility_mask(const float* vis, int32_t X, int32_t Y, int32_t Z, float threshold, int32_t dilate, uint8_t* mask,
                         void* stream) {
  if (X <= 0 || Y <= 0 || Z <= 0 || (long long)X * Y * Z >= (1LL << 31)) return VOXE_ERR_BAD_SHAPE;
  if (dilate < 0 || dilate > 3) return VOXE_ERR_BAD_SHAPE;
  if (!vis || !mask) return VOXE_ERR_NULL_POINTER;
  launch_visibility_mask(vis, X, Y, Z, threshold, dilate, mask, (hipStream_t)stream);
  return finish();
}

// ---- lifting per-ray values into the grid ----------------------------------------------------------------
int voxe_lift_accumulate(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o, const float* rays_d, int64_t R,
                         const float* jitter, const float* values, int32_t C, int64_t* sum_wv, int64_t* sum_w, void* stream) {
  if (const int st = sampling_call_shape(grid, cfg, R)) return st;
  if ((values || sum_wv) && (C < 1 || C > 8)) return VOXE_ERR_BAD_SHAPE;
  DevGrid dg;
  DevCfg dc;
  if (const int st = sampling_call_rays(grid, cfg, R, rays_o, rays_d, &dg, &dc)) return st;
  if (R > 0 && (values == nullptr) != (sum_wv == nullptr)) return VOXE_ERR_NULL_POINTER;   // (R == 0: values may be NULL too)
  if (R == 0 || (!sum_wv && !sum_w)) return VOXE_OK;
  launch_lift_accumulate(dg, dc, grid->densities, rays_o, rays_d, jitter, values, C, reinterpret_cast<long long*>(sum_wv),
                         reinterpret_cast<long long*>(sum_w), (hipStream_t)stream);
  return finish();
}

int voxe_lift_debug_merge(int32_t mode) {
  if (mode < 0 || mode > 2) return VOXE_ERR_BAD_SHAPE;
  tl_lift_merge = mode;
  return VOXE_OK;
}

// ---- vector quantisation against a codebook ----------------------------------------------------------------
static bool vq_shape_ok(int64_t N, int32_t F, int32_t K) {
  return N >= 0 && N < (1LL << 31) && F >= 1 && F <= 64 && K >= 1 && K <= 65536;
}

int voxe_vq_assign(const float* points, int64_t N, int32_t F, const float* codebook, int32_t K, float* code_norm, int32_t* index,
                   float* dist, void* stream) {
  if (!vq_shape_ok(N, F, K)) return VOXE_ERR_BAD_SHAPE;
  if (N == 0) return VOXE_OK;
  if (!points || !codebook || !code_norm || !index) return VOXE_ERR_NULL_POINTER;
  launch_vq_assign(points, N, F, codebook, K, code_norm, index, dist, (hipStream_t)stream);
  return finish();
}

int voxe_vq_accumulate(const float* points, const float* weights, const int32_t* index, int64_t N, int32_t F, int32_t K,
                       int64_t* sum_wx, int64_t* sum_w, void* stream) {
  if (!vq_shape_ok(N, F, K)) return VOXE_ERR_BAD_SHAPE;
  if (N == 0) return VOXE_OK;
  if (!points || !weights || !index || !sum_wx || !sum_w) return VOXE_ERR_NULL_POINTER;
  launch_vq_accumulate(points, weights, index, N, F, K, reinterpret_cast<long long*>(sum_wx), reinterpret_cast<long long*>(sum_w),
                       (hipStream_t)stream);
  return finish();
}

int voxe_vq_debug_merge(int32_t mode) {
  if (mode < 0 || mode > 2) return VOXE_ERR_BAD_SHAPE;
  tl_vq_merge = mode;
  return VOXE_OK;
}

// ---- the density ray losses ("What the ray losses share") ---------------------------------------------------
// The common tail of their entries, behind an entry's own checks: the scratch of the mean, the clear of d_densities when the
// call does not accumulate, and the call that has nothing to launch.  *done: the entry returns the status
static int ray_loss_outputs_ready(const VoxeGridDesc* grid, int64_t R, const float* loss_out, const float* ray_loss,
                                  float* d_densities, int32_t accumulate, const void* scratch, size_t scratch_bytes, void* stream,
                                  bool* done) {
  *done = true;
  if (R > 0 && loss_out && (!scratch || scratch_bytes < ray_loss_scratch_bytes(R))) return VOXE_ERR_WORKSPACE;
  const bool clear = d_densities && !accumulate;
  if (clear && hipMemsetAsync(d_densities, 0, sizeof(float) * (size_t)grid->X * grid->Y * grid->Z, (hipStream_t)stream) != hipSuccess)
    return VOXE_ERR_LAUNCH;
  if (R == 0 || (!loss_out && !ray_loss && !d_densities)) return clear ? finish() : VOXE_OK;
  *done = false;
  return VOXE_OK;
}

// ---- distortion loss on rays -----------------------------------------------------------------------
size_t voxe_distortion_scratch_bytes(int64_t R) { return ray_loss_scratch_bytes(R); }

int voxe_distortion_fwd_bwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o, const float* rays_d, int64_t R,
                            const float* jitter, float grad_scale, float* loss_out, float* ray_loss, float* d_densities,
                            int32_t accumulate, void* scratch, size_t scratch_bytes, void* stream) {
  DevGrid dg;
  DevCfg dc;
  const int st = sampling_call(grid, cfg, R, rays_o, rays_d, &dg, &dc);
  if (st) return st;
  bool done;
  const int sr = ray_loss_outputs_ready(grid, R, loss_out, ray_loss, d_densities, accumulate, scratch, scratch_bytes, stream, &done);
  if (done) return sr;
  launch_distortion(dg, dc, grid->densities, rays_o, rays_d, jitter, grad_scale, loss_out, ray_loss, d_densities, scratch,
                    (hipStream_t)stream);
  return finish();
}

int voxe_distortion_debug_lanes(int32_t lanes) { return pin_lanes(&tl_lane_pins.distortion, lanes); }

// ---- ray-termination loss towards depth targets --------------------------------------------------------
size_t voxe_depth_scratch_bytes(int64_t R) { return ray_loss_scratch_bytes(R); }

int voxe_depth_fwd_bwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o, const float* rays_d, int64_t R,
                       const float* jitter, const float* target_depth, const float* target_sigma, const float* ray_weight, float eps,
                       float grad_scale, float* loss_out, float* ray_loss, float* d_densities, int32_t accumulate, void* scratch,
                       size_t scratch_bytes, void* stream) {
  DevGrid dg;
  DevCfg dc;
  const int st = sampling_call(grid, cfg, R, rays_o, rays_d, &dg, &dc);
  if (st) return st;
  if (!(eps > 0.0f) || !std::isfinite(eps)) return VOXE_ERR_BAD_SHAPE;
  if (R > 0 && (!target_depth || !target_sigma)) return VOXE_ERR_NULL_POINTER;
  bool done;
  const int sr = ray_loss_outputs_ready(grid, R, loss_out, ray_loss, d_densities, accumulate, scratch, scratch_bytes, stream, &done);
  if (done) return sr;
  launch_depth(dg, dc, grid->densities, rays_o, rays_d, jitter, target_depth, target_sigma, ray_weight, eps, grad_scale, loss_out,
               ray_loss, d_densities, scratch, (hipStream_t)stream);
  return finish();
}

int voxe_depth_debug_lanes(int32_t lanes) { return pin_lanes(&tl_lane_pins.depth, lanes); }

// ---- orientation loss on rays -----------------------------------------------------------------------------
size_t voxe_orientation_scratch_bytes(int64_t R) { return ray_loss_scratch_bytes(R); }

int voxe_orientation_fwd_bwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o, const float* rays_d,
                             int64_t R, const float* jitter, const float* ray_weight, float normal_eps, float grad_scale,
                             float* loss_out, float* ray_loss, float* d_densities, int32_t accumulate, void* scratch,
                             size_t scratch_bytes, void* stream) {
  DevGrid dg;
  DevCfg dc;
  const int st = sampling_call(grid, cfg, R, rays_o, rays_d, &dg, &dc);
  if (st) return st;
  if (!(normal_eps >= 0.0f) || !std::isfinite(normal_eps)) return VOXE_ERR_BAD_SHAPE;
  bool done;
  const int sr = ray_loss_outputs_ready(grid, R, loss_out, ray_loss, d_densities, accumulate, scratch, scratch_bytes, stream, &done);
  if (done) return sr;
  launch_orientation(dg, dc, grid->densities, rays_o, rays_d, jitter, ray_weight, normal_eps, grad_scale, loss_out, ray_loss,
                     d_densities, scratch, (hipStream_t)stream);
  return finish();
}

int voxe_orientation_debug_lanes(int32_t lanes) { return pin_lanes(&tl_lane_pins.orientation, lanes); }

// ---- per-image exposure compensation ----------------------------------------------------------------------
namespace {
bool exposure_shape_ok(int64_t R, int64_t N) { return R >= 0 && R < (1LL << 31) && N >= 1 && N < (1LL << 24); }
bool exposure_fit_shape_ok(int64_t N, int64_t P) { return N >= 1 && N <= 65535 && P >= 1 && P < (1LL << 31); }
}  // namespace

size_t voxe_exposure_scratch_bytes(int64_t R, int64_t N) { return exposure_shape_ok(R, N) ? exposure_scratch_bytes(R, N) : 0; }

int voxe_exposure_fwd_bwd(const float* x, const float* y, const int32_t* image_id, int64_t R, const float* delta, int64_t N,
                          int32_t kind, const float* ray_weight, float grad_scale, float* loss_out, float* mse_out,
                          float* corrected, float* d_x, float* d_delta, int32_t accumulate, void* scratch, size_t scratch_bytes,
                          void* stream) {
  if (!delta || (R > 0 && (!x || !y || !image_id))) return VOXE_ERR_NULL_POINTER;
  if (!exposure_shape_ok(R, N)) return VOXE_ERR_BAD_SHAPE;
  if (kind != VOXE_DREG_L1 && kind != VOXE_DREG_L2) return VOXE_ERR_UNSUPPORTED;
  const bool reduces = loss_out || mse_out || d_delta;
  if (R > 0 && reduces && (!scratch || scratch_bytes < exposure_scratch_bytes(R, N))) return VOXE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (R == 0) {
    // outputs that exist are zeroed (d_delta unless it accumulates), nothing else is touched
    if (loss_out && hipMemsetAsync(loss_out, 0, sizeof(float), s) != hipSuccess) return VOXE_ERR_LAUNCH;
    if (mse_out && hipMemsetAsync(mse_out, 0, sizeof(float), s) != hipSuccess) return VOXE_ERR_LAUNCH;
    if (d_delta && !accumulate && hipMemsetAsync(d_delta, 0, sizeof(float) * 12 * (size_t)N, s) != hipSuccess) return VOXE_ERR_LAUNCH;
    return (loss_out || mse_out || (d_delta && !accumulate)) ? finish() : VOXE_OK;
  }
  if (!reduces && !corrected && !d_x) return VOXE_OK;
  if (!launch_exposure(x, y, image_id, delta, ray_weight, R, (int)N, kind == VOXE_DREG_L1, grad_scale, loss_out, mse_out, corrected,
                       d_x, d_delta, accumulate, scratch, s))
    return VOXE_ERR_LAUNCH;
  return finish();
}

int voxe_exposure_apply_bwd(const float* x, const int32_t* image_id, int64_t R, const float* delta, int64_t N,
                            const float* d_corrected, float* d_x, float* d_delta, int32_t accumulate, void* scratch,
                            size_t scratch_bytes, void* stream) {
  if (!delta || (R > 0 && (!x || !image_id || !d_corrected))) return VOXE_ERR_NULL_POINTER;
  if (!exposure_shape_ok(R, N)) return VOXE_ERR_BAD_SHAPE;
  if (R > 0 && d_delta && (!scratch || scratch_bytes < exposure_scratch_bytes(R, N))) return VOXE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (R == 0) {
    if (!d_delta || accumulate) return VOXE_OK;
    return hipMemsetAsync(d_delta, 0, sizeof(float) * 12 * (size_t)N, s) == hipSuccess ? finish() : VOXE_ERR_LAUNCH;
  }
  if (!d_x && !d_delta) return VOXE_OK;
  if (!launch_exposure_apply_bwd(x, image_id, delta, d_corrected, R, (int)N, d_x, d_delta, accumulate, scratch, s))
    return VOXE_ERR_LAUNCH;
  return finish();
}

size_t voxe_exposure_fit_scratch_bytes(int64_t N, int64_t P) {
  return exposure_fit_shape_ok(N, P) ? exposure_fit_scratch_bytes(N, P) : 0;
}

int voxe_exposure_fit_sums(const float* x, const float* y, int64_t N, int64_t P, double* sums, void* scratch, size_t scratch_bytes,
                           void* stream) {
  if (!x || !y || !sums) return VOXE_ERR_NULL_POINTER;
  if (!exposure_fit_shape_ok(N, P)) return VOXE_ERR_BAD_SHAPE;
  if (!scratch || scratch_bytes < exposure_fit_scratch_bytes(N, P)) return VOXE_ERR_WORKSPACE;
  launch_exposure_fit(x, y, N, P, sums, scratch, (hipStream_t)stream);
  return finish();
}

// ---- robust photometric loss on pixel patches -------------------------------------------------------------
namespace {
bool robust_shape_ok(int32_t N, int32_t P, int32_t C) {
  return N >= 1 && P >= 4 && P <= 64 && (P & 1) == 0 && C >= 1 && C <= 4 && (int64_t)N * P * P < (1LL << 31);
}
}  // namespace

size_t voxe_robust_scratch_bytes(int32_t N, int32_t P, int32_t C) { return robust_shape_ok(N, P, C) ? robust_scratch_bytes(N, P) : 0; }

int voxe_robust_fwd_bwd(const float* x, const float* y, int32_t N, int32_t P, int32_t C, int32_t kind, int64_t rank,
                        int32_t smooth_min, int32_t patch_min, const uint8_t* mask_in, float grad_scale, float* loss_out,
                        float* mse_out, float* tau_out, uint8_t* mask_out, int64_t* stats, float* d_x, void* scratch,
                        size_t scratch_bytes, void* stream) {
  if (!x || !y || !scratch) return VOXE_ERR_NULL_POINTER;
  if (!robust_shape_ok(N, P, C)) return VOXE_ERR_BAD_SHAPE;
  if (!mask_in && (rank < 0 || rank >= (int64_t)N * P * P || smooth_min < 1 || smooth_min > 9 || patch_min < 1 ||
                   patch_min > P * P + 1))
    return VOXE_ERR_BAD_SHAPE;
  if (kind != VOXE_DREG_L1 && kind != VOXE_DREG_L2) return VOXE_ERR_UNSUPPORTED;
  if (scratch_bytes < robust_scratch_bytes(N, P)) return VOXE_ERR_WORKSPACE;
  if (!loss_out && !mse_out && !tau_out && !mask_out && !stats && !d_x) return VOXE_OK;
  if (!launch_robust(x, y, N, P, C, kind == VOXE_DREG_L1, rank, smooth_min, patch_min, mask_in, grad_scale, loss_out, mse_out,
                     tau_out, mask_out, (long long*)stats, d_x, scratch, (hipStream_t)stream))
    return VOXE_ERR_LAUNCH;
  return finish();
}

// ---- SSIM of channel-last images --------------------------------------------------------------------------
namespace {
bool ssim_shape_ok(int32_t N, int32_t H, int32_t W, int32_t C) { return N >= 1 && H >= 11 && W >= 11 && C >= 1 && C <= 4; }
}  // namespace

size_t voxe_ssim_scratch_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t with_grad) {
  return ssim_shape_ok(N, H, W, C) ? ssim_scratch_bytes(N, H, W, C, with_grad) : 0;
}

int voxe_ssim_fwd_bwd(const float* x, const float* y, int32_t N, int32_t H, int32_t W, int32_t C, float data_range, float grad_scale,
                      float* mean_out, float* per_image, float* ssim_map, float* d_x, int32_t accumulate, void* scratch,
                      size_t scratch_bytes, void* stream) {
  if (!x || !y || !scratch) return VOXE_ERR_NULL_POINTER;
  if (!ssim_shape_ok(N, H, W, C) || !(data_range > 0.0f)) return VOXE_ERR_BAD_SHAPE;
  const size_t need = ssim_scratch_bytes(N, H, W, C, d_x != nullptr);
  if (need == 0) return VOXE_ERR_BAD_SHAPE;   // more 16 x 16 tiles than one launch holds
  if (scratch_bytes < need) return VOXE_ERR_WORKSPACE;
  if (!mean_out && !per_image && !ssim_map && !d_x) return VOXE_OK;
  launch_ssim(x, y, N, H, W, C, data_range, grad_scale, mean_out, per_image, ssim_map, d_x, accumulate, scratch,
              (hipStream_t)stream);
  return finish();
}

// ---- environment-map background behind the grid ----------------------------------------------------------
namespace {
// the checks the two background calls share; *done: the call ends here with the returned status
int validate_background(const VoxeEnvMap* env, int64_t R, bool* done) {
  *done = true;
  if (!env || !env->texels) return VOXE_ERR_NULL_POINTER;
  if (env->height < 2 || env->width < 2 || R < 0 || R >= (1LL << 31)) return VOXE_ERR_BAD_SHAPE;
  *done = R == 0;
  return VOXE_OK;
}
}  // namespace

int voxe_background_fwd(const VoxeEnvMap* env, const float* rays_d, int64_t R, const float* colour_in, const float* acc,
                        float* colour_out, void* stream) {
  bool done;
  const int st = validate_background(env, R, &done);
  if (done) return st;
  if (!rays_d || !colour_in || !acc || !colour_out) return VOXE_ERR_NULL_POINTER;
  launch_background_fwd(env->texels, env->height, env->width, rays_d, R, colour_in, acc, colour_out, (hipStream_t)stream);
  return finish();
}

int voxe_background_bwd(const VoxeEnvMap* env, const float* rays_d, int64_t R, const float* acc, const float* d_colour_out,
                        float* d_acc, float* d_texels, float* d_rays_d, int32_t accumulate, void* stream) {
  bool done;
  const int st = validate_background(env, R, &done);
  if (done) return st;
  if (!rays_d || !acc || !d_colour_out) return VOXE_ERR_NULL_POINTER;
  if (!d_acc && !d_texels && !d_rays_d) return VOXE_OK;
  if (d_texels && !accumulate &&
      hipMemsetAsync(d_texels, 0, sizeof(float) * 3 * (size_t)env->height * (size_t)env->width, (hipStream_t)stream) != hipSuccess)
    return VOXE_ERR_LAUNCH;
  launch_background_bwd(env->texels, env->height, env->width, rays_d, R, acc, d_colour_out, d_acc, d_texels, d_rays_d,
                        accumulate != 0, (hipStream_t)stream);
  return finish();
}

int voxe_background_debug_merge(int32_t mode) {
  if (mode < 0 || mode > 2) return VOXE_ERR_BAD_SHAPE;
  tl_background_merge = mode;
  return VOXE_OK;
}

// ---- ray and camera-pose gradients -------------------------------------------------------------------------
int voxe_render_bwd_rays(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o, const float* rays_d, int64_t R,
                         const float* jitter, const float* d_colour, const float* d_depth, const float* d_acc, float* d_rays_o,
                         float* d_rays_d, int32_t accumulate, void* stream) {
  if (const int st = sampling_call_shape(grid, cfg, R)) return st;
  if (grid->feature_kind != VOXE_FEAT_SH || cfg->sh_degree < 0 || cfg->sh_degree > 3) return VOXE_ERR_UNSUPPORTED;
  if (grid->F != 3 * (cfg->sh_degree + 1) * (cfg->sh_degree + 1)) return VOXE_ERR_BAD_SHAPE;
  if (const int se = grid_extent_status(grid, grid->F + 1)) return se;
  if (!grid->features) return VOXE_ERR_NULL_POINTER;
  DevGrid dg;
  DevCfg dc;
  if (const int st = sampling_call_rays(grid, cfg, R, rays_o, rays_d, &dg, &dc)) return st;
  if (R == 0 || (!d_rays_o && !d_rays_d)) return VOXE_OK;
  dc.white = cfg->white_bkgd;
  launch_render_rays_bwd(dg, dc, cfg->sh_degree, cfg->render_diffuse, grid->densities, grid->features, rays_o, rays_d, jitter,
                         d_colour, d_depth, d_acc, d_rays_o, d_rays_d, accumulate, (hipStream_t)stream);
  return finish();
}

int voxe_render_bwd_rays_debug_lanes(int32_t lanes) { return pin_lanes(&tl_lane_pins.rays_bwd, lanes); }

// ---- per-voxel Fisher information ---------------------------------------------------------------------------
int voxe_fisher_rays(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const float* rays_o, const float* rays_d, int64_t R,
                     const float* jitter, float* fisher, const float* voxel_var, float* ray_var, void* stream) {
  if (const int st = sampling_call_shape(grid, cfg, R)) return st;
  if (grid->feature_kind != VOXE_FEAT_SH || cfg->sh_degree < 0 || cfg->sh_degree > 3) return VOXE_ERR_UNSUPPORTED;
  if (grid->F != 3 * (cfg->sh_degree + 1) * (cfg->sh_degree + 1)) return VOXE_ERR_BAD_SHAPE;
  if (const int se = grid_extent_status(grid, grid->F + 1)) return se;
  if (!grid->features) return VOXE_ERR_NULL_POINTER;
  DevGrid dg;
  DevCfg dc;
  if (const int st = sampling_call_rays(grid, cfg, R, rays_o, rays_d, &dg, &dc)) return st;
  if (R == 0 || (!fisher && !ray_var)) return VOXE_OK;
  dc.white = cfg->white_bkgd;
  launch_fisher_rays(dg, dc, cfg->sh_degree, cfg->render_diffuse, grid->densities, grid->features, rays_o, rays_d, jitter, fisher,
                     voxel_var, ray_var, (hipStream_t)stream);
  return finish();
}

size_t voxe_cast_rays_bwd_scratch_bytes(int32_t K) { return cast_rays_bwd_scratch_bytes(K); }

int voxe_cast_rays_bwd(int32_t H, int32_t W, float focal, const float* poses, int32_t K, const int64_t* flat_index, int64_t B,
                       const float* d_rays_o, const float* d_rays_d, float* d_poses, float* d_focal, int32_t accumulate,
                       void* scratch, size_t scratch_bytes, void* stream) {
  if (H <= 0 || W <= 0 || K <= 0 || B < 0 || !(focal > 0.0f)) return VOXE_ERR_BAD_SHAPE;
  if (K > (1 << 24) || (int64_t)K * H * W >= (1LL << 40)) return VOXE_ERR_BAD_SHAPE;
  if (!flat_index && B != (int64_t)K * H * W) return VOXE_ERR_BAD_SHAPE;
  if (!poses || !d_poses) return VOXE_ERR_NULL_POINTER;
  if (!scratch || scratch_bytes < cast_rays_bwd_scratch_bytes(K)) return VOXE_ERR_WORKSPACE;
  if (launch_cast_rays_bwd(H, W, focal, poses, K, (const long long*)flat_index, B, d_rays_o, d_rays_d, d_poses, d_focal,
                           accumulate, scratch, (hipStream_t)stream) != hipSuccess)
    return VOXE_ERR_LAUNCH;
  return finish();
}

// ---- real-capture cameras -------------------------------------------------------------------------------------
static bool camera_ok(const VoxeCamera* c) {
  if (c->H <= 0 || c->W <= 0) return false;
  if (!(c->fx > 0.0f) || !(c->fy > 0.0f) || !std::isfinite(c->fx) || !std::isfinite(c->fy)) return false;
  const float rest[7] = {c->cx, c->cy, c->k1, c->k2, c->p1, c->p2, c->k3};
  for (float v : rest)
    if (!std::isfinite(v)) return false;
  return true;
}

static int camera_call_ok(const VoxeCamera* cam, const float* poses, int32_t K, const int64_t* flat_index, int64_t B) {
  if (!cam) return VOXE_ERR_NULL_POINTER;
  if (!camera_ok(cam) || K <= 0 || B < 0) return VOXE_ERR_BAD_SHAPE;
  if (K > (1 << 24) || (int64_t)K * cam->H * cam->W >= (1LL << 40)) return VOXE_ERR_BAD_SHAPE;
  if (!flat_index && B != (int64_t)K * cam->H * cam->W) return VOXE_ERR_BAD_SHAPE;
  if (!poses) return VOXE_ERR_NULL_POINTER;
  return VOXE_OK;
}

int voxe_cast_rays_camera(const VoxeCamera* cam, const float* poses, int32_t K, const int64_t* flat_index, int64_t B,
                          float* rays_o, float* rays_d, void* stream) {
  const int ok = camera_call_ok(cam, poses, K, flat_index, B);
  if (ok != VOXE_OK) return ok;
  if (B == 0) return VOXE_OK;   // (nothing is written: the outputs of an empty batch may have no address)
  if (!rays_o || !rays_d) return VOXE_ERR_NULL_POINTER;
  launch_cast_rays_camera(*cam, poses, K, (const long long*)flat_index, B, rays_o, rays_d, (hipStream_t)stream);
  return finish();
}

size_t voxe_cast_rays_camera_bwd_scratch_bytes(int32_t K) { return cast_rays_camera_bwd_scratch_bytes(K); }

int voxe_cast_rays_camera_bwd(const VoxeCamera* cam, const float* poses, int32_t K, const int64_t* flat_index, int64_t B,
                              const float* d_rays_o, const float* d_rays_d, float* d_poses, float* d_intrinsics,
                              float* d_distortion, int32_t accumulate, void* scratch, size_t scratch_bytes, void* stream) {
  const int ok = camera_call_ok(cam, poses, K, flat_index, B);
  if (ok != VOXE_OK) return ok;
  if (!d_poses && !d_intrinsics && !d_distortion) return VOXE_OK;
  if (!scratch || scratch_bytes < cast_rays_camera_bwd_scratch_bytes(K)) return VOXE_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {   // nothing to sum: an overwriting call leaves exact zeros, no kernel runs
    if (!accumulate) {
      if (d_poses && hipMemsetAsync(d_poses, 0, sizeof(float) * 12 * (size_t)K, st) != hipSuccess) return VOXE_ERR_LAUNCH;
      if (d_intrinsics && hipMemsetAsync(d_intrinsics, 0, sizeof(float) * 4, st) != hipSuccess) return VOXE_ERR_LAUNCH;
      if (d_distortion && hipMemsetAsync(d_distortion, 0, sizeof(float) * 5, st) != hipSuccess) return VOXE_ERR_LAUNCH;
    }
    return VOXE_OK;
  }
  if (launch_cast_rays_camera_bwd(*cam, poses, K, (const long long*)flat_index, B, d_rays_o, d_rays_d, d_poses, d_intrinsics,
                                  d_distortion, accumulate, scratch, st) != hipSuccess)
    return VOXE_ERR_LAUNCH;
  return finish();
}

// ---- rigid transform / re-gridding / composition ------------------------------------------------------------
static bool resample_dims_ok(int32_t X, int32_t Y, int32_t Z, int32_t C) {
  if (X <= 0 || Y <= 0 || Z <= 0) return false;
  if ((long long)X * Y * Z * (C + 1) >= (1LL << 31)) return false;
  return (long long)X * Y < (1LL << 24) && (long long)Y * Z < (1LL << 24) && Z < (1 << 24);   // 24-bit index multiplies
}

int voxe_grid_resample(const float* src_densities, const float* src_features, int32_t X, int32_t Y, int32_t Z, int32_t C,
                       float* dst_densities, float* dst_features, int32_t X2, int32_t Y2, int32_t Z2, const VoxeResample* xf,
                       uint8_t* taken, void* stream) {
  if (!xf) return VOXE_ERR_NULL_POINTER;
  if ((src_densities == nullptr) != (dst_densities == nullptr) || (src_features == nullptr) != (dst_features == nullptr))
    return VOXE_ERR_NULL_POINTER;
  if (!src_densities && !src_features) return VOXE_ERR_NULL_POINTER;
  if (xf->mode != VOXE_RESAMPLE_REPLACE && xf->mode != VOXE_RESAMPLE_UNION) return VOXE_ERR_UNSUPPORTED;
  if (xf->mode == VOXE_RESAMPLE_UNION && !src_densities) return VOXE_ERR_NULL_POINTER;
  if (xf->density_pre_act != VOXE_ACT_IDENTITY && xf->density_pre_act != VOXE_ACT_ABS) return VOXE_ERR_UNSUPPORTED;
  if (xf->sh_degree < -1 || xf->sh_degree > 3) return VOXE_ERR_UNSUPPORTED;
  const int32_t Cf = src_features ? C : 1;   // (C is not read without features)
  if (src_features) {
    if (xf->sh_degree < 0 ? (C < 1 || C > 64) : C != 3 * (xf->sh_degree + 1) * (xf->sh_degree + 1)) return VOXE_ERR_BAD_SHAPE;
  }
  if (!resample_dims_ok(X, Y, Z, Cf) || !resample_dims_ok(X2, Y2, Z2, Cf)) return VOXE_ERR_BAD_SHAPE;
  launch_grid_resample(src_densities, src_features, X, Y, Z, Cf, dst_densities, dst_features, X2, Y2, Z2, *xf, taken,
                       (hipStream_t)stream);
  return finish();
}

// ---- mesh import ----------------------------------------------------------------------------------------------
size_t voxe_voxelize_scratch_bytes(int32_t X, int32_t Y, int32_t Z, int64_t T) {
  return voxelize_dims_ok(X, Y, Z, T) ? voxelize_scratch_bytes(X, Y, Z, T) : 0;
}

int voxe_voxelize_mesh(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const float* vertex_colours,
                       int32_t X, int32_t Y, int32_t Z, const float* aabb_lo, const float* aabb_hi, float h, float* sdf,
                       int32_t* nearest, float* colours, uint8_t* inside, int64_t* stats, void* scratch, size_t scratch_bytes,
                       void* stream) {
  if (!sdf || !aabb_lo || !aabb_hi || (V > 0 && !vertices) || (T > 0 && !faces)) return VOXE_ERR_NULL_POINTER;
  if (!voxelize_dims_ok(X, Y, Z, T) || V < 0 || V >= (1ll << 31)) return VOXE_ERR_BAD_SHAPE;
  for (int d = 0; d < 3; ++d)
    if (!(aabb_hi[d] > aabb_lo[d]) || !(aabb_hi[d] - aabb_lo[d] < INFINITY)) return VOXE_ERR_BAD_SHAPE;
  if (!(h > 0.0f) || !(h < INFINITY)) return VOXE_ERR_BAD_SHAPE;
  if (!scratch || scratch_bytes < voxelize_scratch_bytes(X, Y, Z, T)) return VOXE_ERR_WORKSPACE;
  launch_voxelize(vertices, V, faces, T, vertex_colours, X, Y, Z, aabb_lo, aabb_hi, h, sdf, nearest, colours, inside, stats,
                  scratch, (hipStream_t)stream);
  return finish();
}

}  // extern "C"
