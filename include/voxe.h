/*
 * voxe.h -- C ABI of the MI355X-native voxel-grid volumetric renderer (libvoxe_hip.so)
 *           and of its CPU twin, the test oracle (oracle/libvoxe_oracle.so, voxe_cpu_*).
 *
 * The reference (TAU-VAILab/Vox-E, thre3d_atom) has NO native ABI: its hot path is a chain of
 * ATen ops reached through autograd.  This header is the boundary a maintainer would bind from
 * Python (ctypes stub in INTEGRATION.md); each entry point names the reference code it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain C, no torch / HIP types: `stream` is a hipStream_t passed as void* (NULL = default
 *     stream); every pointer of a voxe_* function is a DEVICE pointer on the current HIP device,
 *     every pointer of a voxe_cpu_* function is a HOST pointer;
 *   - all buffers are caller-owned, contiguous, float32 unless stated; nothing is allocated inside;
 *   - every function returns 0 on success or a negative VoxeStatus; nothing throws;
 *   - functions are asynchronous w.r.t. the host (they enqueue on `stream`) and thread-safe for
 *     distinct (stream, workspace) pairs.
 *
 * Grid memory layout (reference: thre3d_atom/thre3d_reprs/voxels.py:46-136)
 *   densities [X,Y,Z,1], features [X,Y,Z,F]  (C innermost, Z fastest spatial axis);
 *   element (ix,iy,iz,c) lives at ((ix*Y + iy)*Z + iz)*C + c.
 */
#ifndef VOXE_H_
#define VOXE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VOXE_ABI_VERSION 13

typedef enum VoxeStatus {
  VOXE_OK = 0,
  VOXE_ERR_NULL_POINTER = -1,
  VOXE_ERR_BAD_SHAPE = -2,       /* non-positive grid dims / R / S, F not 3*(deg+1)^2 ...        */
  VOXE_ERR_UNSUPPORTED = -3,     /* activation / mode the HIP path does not implement            */
  VOXE_ERR_WORKSPACE = -4,       /* workspace NULL or smaller than voxe_workspace_bytes()        */
  VOXE_ERR_LAUNCH = -5,          /* hipGetLastError() after a launch was not hipSuccess          */
  VOXE_ERR_NO_DEVICE = -6        /* no HIP device / wrong architecture                           */
} VoxeStatus;

/* density activations (voxels.py:55-57; CLI table train_sh_based_voxel_grid_with_posed_images.py:177-200) */
typedef enum VoxeAct {
  VOXE_ACT_IDENTITY = 0,
  VOXE_ACT_ABS = 1,        /* torch.abs            (pre-activation of the non-softplus field)     */
  VOXE_ACT_RELU = 2,       /* torch.nn.ReLU        (post)                                         */
  VOXE_ACT_SOFTPLUS = 3    /* torch.nn.Softplus(beta=1, threshold=20) (post; the CLI default)     */
} VoxeAct;

/* What the "feature" channels are. */
typedef enum VoxeFeatureKind {
  VOXE_FEAT_SH = 0,    /* RGB spherical-harmonic coefficients, F = 3*(deg+1)^2; Cout = 3
                          (process.py:20-96, accumulate.py:31-113)                                */
  VOXE_FEAT_ATTN = 1   /* one attention channel, F = 1; Cout = 1; background multiplied by 0
                          (voxels.py:344-406, process.py:98-174, accumulate.py:115-198)           */
} VoxeFeatureKind;

typedef struct VoxeGridDesc {
  const float* densities;   /* [X,Y,Z,1]  VoxelGrid._densities (or .orig_densities)               */
  const float* features;    /* [X,Y,Z,F]  VoxelGrid._features  (or .attn for VOXE_FEAT_ATTN)      */
  int32_t X, Y, Z, F;
  float aabb_lo[3];         /* float32(aabb.{x,y,z}_range[0])  voxels.py:196-223                  */
  float aabb_hi[3];         /* float32(aabb.{x,y,z}_range[1])                                     */
  float norm_scale[3];      /* adjust_dynamic_range(slack=True): np.float32(2)/(f32(hi)-f32(lo))  */
  float norm_bias[3];       /*   np.float32(-1) - f32(lo)*scale   (imaging_utils.py:57-63)        */
  float density_scale;      /* expected_density_scale (voxels.py:303-305)                         */
  int32_t density_pre_act;  /* VoxeAct: IDENTITY | ABS                                            */
  int32_t density_post_act; /* VoxeAct: IDENTITY | RELU | SOFTPLUS                                */
  int32_t feature_kind;     /* VoxeFeatureKind                                                    */
} VoxeGridDesc;

/* Which kernels render a call, and with which tuning parameters (ABI v7).  Every field: 0 = the shipped default, so a
 * zero-initialised struct -- or VoxeRenderCfg::dispatch == NULL -- is the shipped dispatch.  The struct is read on every call
 * from the caller's memory: there is no process-global dispatch state in the library and nothing reads the environment on
 * the render path (the Python binding resolves its VOXE_* environment switches ONCE into one of these, voxe_hip/dispatch.py).
 * Forward and backward of one render must be given the same values (the per-ray states a forward leaves in the workspace
 * belong to one route: voxe_render_route).  Results never depend on these fields beyond float summation order. */
typedef struct VoxeDispatch {
  int32_t bwd_mode;            /* 0 auto | 1 plain global-atomic scatter (the A/B baseline) | 2 line-dense scatter            */
  int32_t tile_map;            /* block -> pixel-tile map: 0 auto | 1 interleaved over the XCDs | 2 XCD bands | 3 tile rows    */
  int64_t tile_min_rays;       /* image-ordered renders below this many rays take the line-dense scatter backward instead of
                                  the LDS-window one: 0 = 8192 | > 0 explicit | -1 no minimum                                 */
  int32_t tile_two_phase;      /* view-dependent grids: 0 two-phase backward when the workspace holds the per-sample sources |
                                  -1 always the single-kernel channel groups                                                  */
  int32_t tile_qsplit;         /* parts of a tile that does not fit the window: 0 auto (by launch size) | 1 consecutive passes
                                  of one block | 4 sibling blocks                                                             */
  int32_t tile_kl;             /* lateral edge of the backward's LDS window (voxels): 0 auto | 8 | 10                          */
  float tile_fit_m;            /* a pass fits the window when its spread along the march axis is below this many layers:
                                  0 = by launch size (4.0 ... 5.5)                                                            */
  float tile_fit_lat;          /* ... and its lateral extent below this many voxels: 0 = window edge - 2.5                     */
  int32_t fwd_window;          /* LDS texel window of the image-ordered forward (SH-0: 16-byte texels; r06: SH 1 - 3, whole texels):
                                  0 on | -1 off (ray-ordered forward) | 2 test aid (SH 1 - 3): samples the window did not serve
                                  render as NaN                                                                               */
  float fwd_fit_lat, fwd_fit_m;/* window forward: fit bounds of a tile (0 = 5.5 voxels / 4.5 layers; SH 1 - 3: 5.5 / 12 -- its
                                  lanes wait for a layer instead of leaving the window)                                       */
  float fwd_zdom;              /* a tile is z-dominant when |d_z| >= |this| x max(|d_x|, |d_y|); > 0: such tiles march ray by ray,
                                  < 0: along z through the window.  0 = 1.0 for SH-0, -1.0 for SH 1 - 3 (4.4)    */
  float fwd_max_adv;           /* layers a window tile may advance per sample: 0 = 1.7                                         */
  int32_t fwd_segments_per_thread; /* depth segments one thread of the ray-ordered forward walks: 0 = 1                        */
  int64_t region_min_rays;     /* space-binned route for unordered / sparse rays from this many rays on: 0 = 16384 | > 0
                                  explicit | -1 route off                                                                     */
  float region_image_ratio;    /* image-ordered launches take the space-binned route when grid side >= this x image width:
                                  0 = 1.3 | < 0: every image-ordered launch the route accepts                                 */
  int32_t tile_lean;           /* ABI v8.  SH-0 image-ordered backward: 0 = the lean LDS-window kernel (voxe_render_tile4.hip)
                                  wherever it applies | -1 always the general kernel (A/B runs, parity tests)                 */
  int32_t precise_grad;        /* ABI v8.  0 = float running sums inside a depth segment (density gradients ~1e-5 median
                                  relative error against a double-precision backward) | 1 = the suffix sums of the
                                  image-ordered SH-0 backward are carried in double (~2e-6, a few percent slower).  Forward
                                  and backward of one render must agree on it (the forward saves the segment states).       */
  int32_t region_lds_ranks;    /* ABI v9.  Space-binned route, segment pass: 0 = segments are ranked per block in an LDS table
                                  (no global atomic; grids up to ~200^3) | -1 one returning global atomic per segment (r02)   */
  int32_t tile_phases;         /* ABI v11.  SH-0 image-ordered backward, tiles that do not fit the window and run as 2 / 4 parts:
                                  0 = the lanes outside a part take the other SAMPLE PHASES of the part's rays (32 rays x 2
                                  consecutive samples, 16 rays x 4: every wave instruction works on 64 lanes) | -1 = one
                                  sample per ray and iteration, the other lanes idle (r05).  Read only by a library built with
                                  -DVOXE_T4_PHASES_KL8=1 / -DVOXE_T4_PHASES_KL10=1: the shipped kernels carry no phased march
                                  (inside one kernel it cost the one-sample march 8 % at 400x400 and won nothing over the
                                  views at 100 .. 266 px: csrc/voxe_render_tile4.hip, profiles/r06_phases_kl8.txt).          */
} VoxeDispatch;

typedef struct VoxeRenderCfg {
  int32_t num_samples;        /* S   SHVoxGridRenderConfig.num_samples_per_ray (renderers.py:32)  */
  float near, far;            /* CameraBounds (sample.py:38-41)                                   */
  int32_t perturb;            /* stratified jitter (sample.py:55-64). jitter==NULL -> in-kernel
                                 counter hash keyed by (seed, rng_offset, ray, sample)             */
  int32_t linear_disparity;   /* sample.py:48-51                                                  */
  int32_t aabb_clip;          /* optimized_sampling: per-ray bounds from the ray/AABB slab test
                                 (sample.py:71-202)                                               */
  int32_t white_bkgd;         /* accumulate.py:77-81 (for VOXE_FEAT_ATTN the term is *0.0, :166)  */
  int32_t sh_degree;          /* 0..3 ; F == 3*(sh_degree+1)^2 for VOXE_FEAT_SH                   */
  int32_t render_diffuse;     /* use only the degree-0 coefficient (process.py:59-63)             */
  float term_eps;             /* gradient truncation (NOT in the reference; 0 = off).  The forward always integrates all S
                                 samples exactly like the reference; with term_eps > 0 the BACKWARD stops marching a ray once
                                 its transmittance is below term_eps: samples behind that point get no gradient (their
                                 contributions scale with T < term_eps), the samples in front keep their EXACT gradient
                                 (the suffix sums come from the full forward).  -20 % backward time on surface-like scenes.
                                 The rule: sample k receives its exact gradient iff the transmittance IN FRONT of it, T_k (the
                                 exclusive product, T_0 = 1), is >= term_eps.  Meaningful for 0 < term_eps < 1; at >= 1 the
                                 kernels still differentiate sample 0 of the first segment: neither tested nor promised.     */
  uint64_t seed, rng_offset;  /* in-kernel jitter stream                                          */
  int32_t reuse_packed_grid;  /* 1: workspace already holds this grid packed by a previous call
                                 on the same workspace (grid values unchanged)                    */
  int32_t image_width;        /* 0 = unknown. >0: rays are a row-major H x W image (ray r is
                                 pixel (r / W, r % W)); lets the kernels use 2-D pixel tiles      */
  int32_t image_height;       /* 0 = one image (H = R / image_width).  >0 with image_width > 0: the rays are K =
                                 R / (image_height * image_width) row-major images of the same size, one after
                                 the other (ray r = (camera * H + y) * W + x): ONE launch renders a multi-view
                                 batch; pixel tiles never straddle two cameras.  R must be a multiple of H * W.  */
  int32_t deterministic;      /* backward only, test / race-check mode (SURVEY 8(b) `deterministic`).  1: the gradient
                                 is accumulated in 64-bit FIXED POINT (integer adds are associative, so the result
                                 does not depend on the order lanes, waves and blocks meet on a voxel): two calls on
                                 the same inputs return identical bits.  Costs an extra measuring pass (per-call
                                 power-of-two scales from max |contribution|) and 8 bytes per gradient value of
                                 workspace (voxe_workspace_bytes accounts for it).  Image-ordered rays
                                 (image_width > 0), SH degree 0 / render_diffuse / attention grids; other
                                 configurations return VOXE_ERR_UNSUPPORTED.  0: float atomics (default).          */
  int32_t linear_grad;        /* voxe_render_bwd_acc(_into) only.  1: the gradient region is written in
                                 VOXE_GRAD_LINEAR whatever backward kernel runs (the line-dense scatter of small
                                 unordered batches otherwise prefers VOXE_GRAD_BRICKED, -7 % on that kernel): lets a
                                 caller accumulate ANY mix of renders into one optimiser step.                     */
  int32_t ray_state_valid;    /* backward only. 1: `workspace` still holds the per-ray depth-segment
                                 states (transmittance + partial sums every VOXE_SEGMENT_SAMPLES
                                 samples) written by voxe_render_fwd for EXACTLY these rays / cfg /
                                 jitter, so the depth-segmented backward starts from them.
                                 0: the backward first re-marches the rays to rebuild them.
                                 voxe_render_fwd reads it too: -1 = no backward of these rays will follow
                                 (inference): the forward skips what only that backward would read (the per-sample
                                 values of view-dependent image-ordered renders, r04), and
                                 voxe_workspace_bytes() leaves out the backward's scratch.  The 1 is a CLAIM the
                                 library checks (r05): every forward records, per workspace address, what it
                                 rendered there (grid, rays, jitter, cfg, dispatch, whether the per-sample values
                                 were kept); a backward whose claim does not match the record -- after a forward
                                 with -1, a forward of other rays in between, or a voxe_grid_adam_step on this
                                 workspace (the parameters moved) -- re-marches as if given 0.  voxe_grid_adam_step
                                 and voxe_adam_step also drop the record of EVERY workspace whose forward read the
                                 tensors they rewrite (r06).  What the record compares is identity -- pointers,
                                 shapes, AABB, cfg, dispatch -- never CONTENTS: a caller that rewrites the grid, the
                                 rays or the jitter in place by other means (its own kernels, a copy into the same
                                 buffer) must pass 0.                                                            */
  const VoxeDispatch* dispatch; /* HOST pointer, NULL = the shipped dispatch; read during the call only (ABI v7)      */
} VoxeRenderCfg;

/* depth-segment length of the segmented kernels (samples per segment); launches of at most 20000 rays use 16: they
 * leave the chip under-filled, and shorter dependent chains then matter more than the extra boundary states     */
#ifndef VOXE_SEGMENT_SAMPLES
#define VOXE_SEGMENT_SAMPLES 32
#endif

/* ------------------------------------------------------------------------------------------------
 * Library / device
 * ---------------------------------------------------------------------------------------------- */
int voxe_abi_version(void);
const char* voxe_strerror(int status);
/* 0 when a gfx950 device is current; VOXE_ERR_NO_DEVICE otherwise. Fills name (may be NULL). */
int voxe_device_check(char* name, size_t name_len);

/* ------------------------------------------------------------------------------------------------
 * Per-phase device timing (measurement hook used by bench.py; no reference counterpart).
 * While enabled, every render call brackets its phases with hipEvents ON THE CALLER'S STREAM
 * (pack, forward kernel, gradient memset, backward kernel, unpack).  voxe_profile_read() waits for
 * the recorded events and returns the summed milliseconds / launch counts since voxe_profile_enable(1).
 * At most 512 phase records are kept between enable and read; later ones are dropped (n_dropped).
 * ---------------------------------------------------------------------------------------------- */
typedef struct VoxeProfile {
  double ms_pack, ms_fwd, ms_memset, ms_bwd, ms_unpack;
  int32_t n_pack, n_fwd, n_memset, n_bwd, n_unpack, n_dropped;
} VoxeProfile;
int voxe_profile_enable(int32_t on);
int voxe_profile_read(VoxeProfile* out);

/* ------------------------------------------------------------------------------------------------
 * Ray casting -- rendering/volumetric/utils/misc.py:12-50 (cast_rays)
 *   rot[9] row-major 3x3, trans[3] : HOST pointers (12 floats, copied by value into the launch)
 *   rays_o, rays_d : [H*W,3]
 * ---------------------------------------------------------------------------------------------- */
int voxe_cast_rays(int32_t H, int32_t W, float focal, const float* rot, const float* trans,
                   float* rays_o, float* rays_d, void* stream);

/* Rays of SELECTED pixels of K cameras sharing (H, W, focal): what the reconstruction trainer keeps of
 *   cast_rays x K -> collate_rays -> randperm subset   (modules/trainers.py:290-313, misc.py:60-70,126-138)
 * without materialising the K full images of rays.  poses: DEVICE [K,3,4] (rotation | translation);
 * flat_index: DEVICE int64 [B], value = (camera * H + y) * W + x;  rays_o, rays_d: [B,3].  Arithmetic per pixel
 * identical to voxe_cast_rays (bit-exact same rays).                                                       */
int voxe_cast_rays_indexed(int32_t H, int32_t W, float focal, const float* poses, int32_t K,
                           const int64_t* flat_index, int64_t B, float* rays_o, float* rays_d, void* stream);

/* A uniformly random SUBSET of `count` distinct indices of [0, n), in random order: what `torch.randperm(n)[:count]`
 * is used for in the ray-batch samplers (rendering/volumetric/utils/misc.py:126-138) without permuting all n
 * (n = 1.28 M pixels for a 32768-ray batch).  out[i] = P(i), P a keyed 4-round Feistel permutation of [0, 2^b)
 * (b = even number of bits >= log2 n) restricted to [0, n) by cycle walking: distinct by construction, reproducible
 * from (seed, rng_offset); integer work, bit-exact between device and oracle.  n <= 2^31, count <= n.       */
int voxe_random_subset(int64_t n, int64_t count, uint64_t seed, uint64_t rng_offset, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Volumetric render, forward -- replaces the whole chain
 *   render_sh_voxel_grid(_attn)            thre3d_reprs/renderers.py:50-163
 *   -> sample_uniform_points_on_rays       rendering/volumetric/sample.py:15-68 (+ :71-202)
 *   -> process_points_with_sh_voxel_grid   rendering/volumetric/process.py:20-174
 *      -> VoxelGrid.forward(_attn)         thre3d_reprs/voxels.py:287-406
 *      -> evaluate_spherical_harmonics     rendering/volumetric/utils/spherical_harmonics.py:64-132
 *   -> accumulate_radiance_density_on_rays rendering/volumetric/accumulate.py:31-198
 *
 *   rays_o, rays_d [R,3]; jitter [R,S] uniforms in [0,1) or NULL;
 *   outputs colour [R,Cout] (Cout = 3 SH / 1 attn), depth [R], acc [R], disparity [R]
 *   (any of depth/acc/disparity may be NULL).
 * ---------------------------------------------------------------------------------------------- */
/* Workspace: [packed grid | packed gradient | per-ray depth-segment states | segment partials | per-sample gradient
 * sources].  voxe_workspace_bytes() is the size that lets every kernel take its fast route; the forward needs only the
 * packed grid, and the backward needs everything but the last region (16 B per sample of image-ordered renders of SH
 * degree >= 1, capped at 4 GB): without it their gradient-channel groups re-march the rays instead of sharing one march.
 * What the optional regions cost, so that a caller can size its pools:
 *   - view-dependent grids, image-ordered renders: besides the 2 x 16 B per sample above, the GROUP-PLANAR staging gradient of
 *     the lean deposit passes, voxels x 16 B x ceil((F + 1) / 4) (262 MB for SH-1 at 160^3, ~850 MB for SH-3), cleared and
 *     folded into the packed gradient on every such backward whatever the image size;
 *   - unordered / sparse rays (space-binned route): segment tables + per-segment states, and for grids whose region table fits
 *     LDS (up to ~200^3) the per-block rank tables of the segment pass, blocks x (regions + 1) x 24 B (blocks <= 1024: ~48 MB
 *     at 160^3 for a 32 768-ray batch, ~120 MB at 160 000 rays), allocated whether or not VoxeDispatch::region_lds_ranks
 *     takes that pass;
 *   - VoxeDispatch::precise_grad: 5 doubles per (ray, depth segment); cfg->deterministic: 8 B per gradient value.
 * cfg->ray_state_valid = -1 (inference) returns the size without any of these. */
size_t voxe_workspace_bytes(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R);
/* Optional: bytes a caller may ADD to voxe_workspace_bytes() for the per-tile plan of the lean tile kernels (large image-ordered
 * SH-0 launches: 16 B per 8x8-pixel tile and depth segment, 320 KB at 400x400; 0 where no plan is built, and for
 * ray_state_valid = -1).  With a workspace of at least the sum, forward and backward of a render take their per-tile decisions from
 * the plan the forward's schedule pass writes there; with less they derive them per block -- same results, a few percent slower.
 * Forward and backward of one render must be given the same workspace_bytes. */
size_t voxe_tile_plan_bytes(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R);

int voxe_render_fwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                    const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                    float* colour, float* depth, float* acc, float* disparity,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Volumetric render, backward -- replaces autograd through the chain above
 * (loss.backward(): modules/trainers.py:350, modules/sds_trainer.py:332,
 *  modules/attn_grid_trainer.py:372,376).
 *
 *   colour/depth/acc: the forward outputs for the same inputs (same jitter / seed);
 *   d_colour [R,Cout]; d_depth [R] or NULL; d_acc [R] or NULL   (upstream gradients)
 *   d_densities [X,Y,Z,1] or NULL (skip), d_features [X,Y,Z,F] or NULL (skip);
 *   accumulate != 0: += into the outputs, else overwrite.
 * ---------------------------------------------------------------------------------------------- */
int voxe_render_bwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                    const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                    const float* colour, const float* depth, const float* acc,
                    const float* d_colour, const float* d_depth, const float* d_acc,
                    float* d_densities, float* d_features, int32_t accumulate,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Point query -- VoxelGrid.forward / forward_attn  thre3d_reprs/voxels.py:287-406
 *   points [N,3] world coordinates  ->  out [N,F+1] = (trilinear features f_0..f_{F-1}, post(trilinear pre(d*scale)))
 *   NOT masked by the AABB (the reference masks later, process.py:80-84): zero padding outside the grid.
 *   Backward: d_out [N,F+1] -> d_densities / d_features (either may be NULL), accumulate as above.
 *   workspace: >= voxe_workspace_bytes(grid, NULL, 0) (packed grid + gradient region; the forward alone reads and writes only
 *   the packed grid, the first voxe_workspace_grad_offset(grid) bytes, and is refused only below that); cfg-less, so packed-grid
 *   reuse is an explicit flag.
 * ---------------------------------------------------------------------------------------------- */
int voxe_query_fwd(const VoxeGridDesc* grid, const float* points, int64_t N, float* out,
                   int32_t reuse_packed_grid, void* workspace, size_t workspace_bytes, void* stream);
int voxe_query_bwd(const VoxeGridDesc* grid, const float* points, int64_t N, const float* d_out,
                   float* d_densities, float* d_features, int32_t accumulate, int32_t reuse_packed_grid,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-sample probe (test hook for the bit-exact index-math contract): for ray r, sample k writes
 *   idx  [R,S,3] int32  floor() voxel index of the low trilinear corner (may be -1 or N-1.. out of range)
 *   inside [R,S] uint8  strict AABB test (voxels.py:263-285)
 *   zvals [R,S] float   sample depths (sample.py:46-64)
 *   sigma [R,S] float   post-activated, masked density; rad [R,S,Cout] masked raw radiance (process.py:80-84;
 *                       -1e10 outside)
 * any output may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int voxe_sample_probe(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                      const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                      int32_t* idx, uint8_t* inside, float* zvals, float* sigma, float* rad,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-grid passes of the SDS / reconstruction step (HBM-streaming)
 * ---------------------------------------------------------------------------------------------- */
/* _density_correlation_loss  modules/sds_trainer.py:507-524
 *   loss = 1 - mean((a-mean a)(b-mean b)) / (sqrt(var a * var b) + 1e-7)
 *   a = sds densities (differentiated), b = regular densities (constant); n elements
 *   loss_out: 1 float; d_a: n floats (d loss / d a * grad_scale), accumulate as above; d_a may be NULL.
 *   scratch: >= voxe_dcl_scratch_bytes(n) bytes.                                                  */
size_t voxe_dcl_scratch_bytes(int64_t n);
int voxe_dcl_fwd_bwd(const float* a, const float* b, int64_t n, float grad_scale,
                     float* loss_out, float* d_a, int32_t accumulate,
                     void* scratch, size_t scratch_bytes, void* stream);

/* density_correlation_loss_fn's l2_mode / l1_mode  modules/sds_trainer.py:494-503 (+ autograd)
 *   VOXE_DREG_L2: loss = mean((a - b)^2)  (torch mse_loss),  d_a = grad_scale * 2 (a - b) / n
 *   VOXE_DREG_L1: loss = mean(|a - b|)    (torch l1_loss),   d_a = grad_scale * sign(a - b) / n   (sign(0) = 0)
 *   a = sds densities (differentiated), b = regular densities (constant); loss_out: 1 float or NULL; d_a: n floats or NULL
 *   (accumulate as above); scratch: >= voxe_dcl_scratch_bytes(n) bytes (only read when loss_out != NULL).
 *   VOXE_DREG_CORRELATION names the default (_density_correlation_loss, voxe_dcl_fwd_bwd) in VoxeGridRegularisers.      */
enum { VOXE_DREG_CORRELATION = 0, VOXE_DREG_L2 = 1, VOXE_DREG_L1 = 2 };
int voxe_density_diff_fwd_bwd(const float* a, const float* b, int64_t n, int32_t kind, float grad_scale,
                              float* loss_out, float* d_a, int32_t accumulate,
                              void* scratch, size_t scratch_bytes, void* stream);

/* _feature_correlation_loss  modules/sds_trainer.py:526-534 (+ autograd): f = sds features [nvox, F] (differentiated),
 *   r = regular features (constant):  D_v = sum_c (sigmoid(f_vc) - sigmoid(r_vc));  loss = sum_v D_v^2;
 *   d_f[v, c] = grad_scale * 2 D_v sigmoid(f_vc) (1 - sigmoid(f_vc)).  loss_out: 1 float or NULL; d_f: nvox * F floats or NULL
 *   (accumulate as above); scratch: >= voxe_dcl_scratch_bytes(nvox) bytes.  1 <= F <= 64.                                */
int voxe_feature_correlation_fwd_bwd(const float* f, const float* r, int64_t nvox, int32_t F, float grad_scale,
                                     float* loss_out, float* d_f, int32_t accumulate,
                                     void* scratch, size_t scratch_bytes, void* stream);

/* _tv_loss_on_grid  modules/sds_trainer.py:563-567 : grid [X,Y,Z,C]
 *   loss = (mean|diff_x| + mean|diff_y| + mean|diff_z|)/3 ; d_grid accumulates grad_scale * dloss/dgrid */
size_t voxe_tv_scratch_bytes(int32_t X, int32_t Y, int32_t Z, int32_t C);
int voxe_tv_fwd_bwd(const float* grid, int32_t X, int32_t Y, int32_t Z, int32_t C, float grad_scale,
                    float* loss_out, float* d_grid, int32_t accumulate,
                    void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused optimiser step of a voxel grid: gradient un-pack + torch.optim.Adam + re-pack in ONE streaming pass
 *   (modules/sds_trainer.py:200-203,332-333; modules/trainers.py:247-255,350-351).
 *
 * voxe_render_bwd_acc  == voxe_render_bwd that LEAVES the gradient in the workspace (kernel layout) instead of
 *   splitting it into the two API tensors.  zero_first != 0 clears the gradient region first, 0 accumulates on top
 *   (several renders per optimiser step).  *grad_layout (HOST int) receives VOXE_GRAD_LINEAR / VOXE_GRAD_BRICKED
 *   (which backward kernel ran; VOXE_GRAD_ANY for R == 0); every render accumulated into one step must report the
 *   same layout.
 * voxe_grid_adam_step  grid->densities / grid->features are the PARAMETERS and are updated in place (the const
 *   of the descriptor is cast away); gradient = the workspace's packed gradient (chain rule of the density
 *   pre-activation applied like voxe_render_bwd does) + optional extra gradients in API layout (regularisers);
 *   exp_avg / exp_avg_sq: Adam state per tensor, NULL pair = that tensor is frozen.  Afterwards the workspace holds the
 *   NEW grid packed (pass reuse_packed_grid = 1 to the next render) and a ZEROED gradient region (pass zero_first = 0).
 *   [x_begin, x_end) restricts the step to the voxels of those x-planes (0, X = the whole grid; x_begin must be even
 *   for VOXE_GRAD_BRICKED unless it is 0 ... X): an optimiser sharded over GPUs updates only its slab -- a slab is one
 *   contiguous byte range of every tensor involved, the workspace's packed grid and gradient regions included
 *   (voxe_workspace_grad_offset + x_begin * Y * Z * (F + 1) * 4 in the linear layout).
 *   Arithmetic identical to voxe_render_bwd + voxe_adam_step, bit for bit.                                        */
enum { VOXE_GRAD_ANY = -1, VOXE_GRAD_LINEAR = 0, VOXE_GRAD_BRICKED = 1 };
int voxe_render_bwd_acc(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                        const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                        const float* colour, const float* depth, const float* acc,
                        const float* d_colour, const float* d_depth, const float* d_acc,
                        int32_t want_densities, int32_t want_features, int32_t zero_first, int32_t* grad_layout,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The same with the gradient region of ANOTHER workspace of the same grid as the destination (grad_workspace; NULL =
 * `workspace` itself): two renders of one optimiser step that run in different workspaces -- each keeps its own
 * packed grid and per-ray states, e.g. the specular and the diffuse render of a reconstruction iteration
 * (modules/trainers.py:316,333) -- then sum into ONE gradient region that voxe_grid_adam_step consumes.            */
int voxe_render_bwd_acc_into(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                             const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                             const float* colour, const float* depth, const float* acc,
                             const float* d_colour, const float* d_depth, const float* d_acc,
                             int32_t want_densities, int32_t want_features, int32_t zero_first, int32_t* grad_layout,
                             void* workspace, size_t workspace_bytes, void* grad_workspace, size_t grad_workspace_bytes,
                             void* stream);
/* layout the backward of (grid, cfg, R) would write: VOXE_GRAD_LINEAR / VOXE_GRAD_BRICKED (VOXE_GRAD_ANY for R == 0), or
 * a negative VOXE_ERR_* below -1 for invalid arguments -- lets a caller that accumulates several renders into one step
 * check that they agree BEFORE running one                                                                          */
int voxe_render_bwd_layout(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R);
size_t voxe_workspace_grad_offset(const VoxeGridDesc* grid);  /* byte offset / size of the gradient region, e.g. */
size_t voxe_workspace_grad_bytes(const VoxeGridDesc* grid);   /* for the multi-GPU all-reduce between the two calls */
/* Whole-grid regularisers evaluated INSIDE the grid step (modules/sds_trainer.py:305-334): the SDS edit's
 * default regulariser is the density-correlation loss between the edited and the original densities (weight 200,
 * edit_pretrained_relu_field.py:171).  Its gradient is elementwise in the parameters the step streams anyway, so only the
 * moment reduction stays a launch of its own (two small kernels); the separate gradient kernel, the [X,Y,Z,1] gradient
 * buffer and its round trip through HBM are gone.  dcl_reference == NULL: no term.  Requires the whole grid
 * (x_begin = 0, x_end = X: the moments are over all voxels).  Same arithmetic as voxe_dcl_fwd_bwd with
 * grad_scale = dcl_weight (the weight enters the two gradient constants in double instead of multiplying the finished float
 * gradient: results agree to float rounding, not bit for bit).  The total-variation terms (default weight 0) stay
 * separate passes: their stencil reads neighbours the in-place update of this very pass is overwriting. */
typedef struct VoxeGridRegularisers {
  const float* dcl_reference;   /* [X,Y,Z,1] densities of the pretrained field (constant), device; NULL = no DCL term      */
  float dcl_weight;             /* density_correlation_weight (x any schedule / 1 / world factor)                         */
  float* dcl_loss;              /* device float[1] or NULL: receives 1 - corr (unweighted, what the trainer logs)         */
  void* scratch;                /* >= voxe_dcl_scratch_bytes(X * Y * Z) bytes of device memory                            */
  size_t scratch_bytes;
  /* ABI v11: every regulariser the edit's CLI can switch on is a term of the fused step (no torch op, no gradient tensor)   */
  int32_t density_kind;         /* VOXE_DREG_*: what (dcl_reference, dcl_weight, dcl_loss) mean.  L2 / L1 are per-voxel
                                   terms with NO reduction (a reduction runs only when dcl_loss != NULL) and, unlike the
                                   correlation, also work on a slab (x_begin, x_end) -- the loss value then is the slab's
                                   share: sum over the slab / (X Y Z)                                                      */
  const float* feat_reference;  /* [X,Y,Z,F] features of the pretrained field (constant), device; NULL = no term:
                                   _feature_correlation_loss (sds_trainer.py:526-534) evaluated per voxel inside the step
                                   on the parameters the step starts from.  SH-0 / attention grids (F <= 3);
                                   VOXE_ERR_UNSUPPORTED for wider texels (use voxe_feature_correlation_fwd_bwd +
                                   extra_d_features there)                                                                */
  float feat_weight;            /* feature_correlation_weight (x any 1 / world factor)                                    */
  float* feat_loss;             /* device float[1] or NULL: the unweighted loss value (a reduction of its own)            */
} VoxeGridRegularisers;
int voxe_grid_adam_step(const VoxeGridDesc* grid, int32_t grad_layout, int32_t x_begin, int32_t x_end,
                        const float* extra_d_densities, const float* extra_d_features,
                        float* exp_avg_densities, float* exp_avg_sq_densities,
                        float* exp_avg_features, float* exp_avg_sq_features,
                        float lr, float beta1, float beta2, float eps, int64_t step, int64_t step_features,
                        const VoxeGridRegularisers* regularisers /* NULL = none */,
                        void* workspace, size_t workspace_bytes, void* stream);
/*   `step` / `step_features`: the 1-based Adam step counts of the densities and of the features (torch.optim.Adam keeps
 *   one counter per parameter; step_features = 0 means "the same as step").                                          */

/* Which kernels render (grid, cfg, R).  The per-ray states a forward leaves in the workspace belong to ONE route, so a
 * caller that sets cfg->ray_state_valid must know that forward and backward resolve to the same one (the choice also
 * depends on process-level tuning switches); negative VOXE_ERR_* below -1 for invalid arguments.                      */
enum { VOXE_ROUTE_NONE = -1, VOXE_ROUTE_SCATTER = 0, VOXE_ROUTE_TILE = 1, VOXE_ROUTE_PACKED_SCATTER = 2,
       VOXE_ROUTE_REGION = 3, VOXE_ROUTE_DETERMINISTIC = 4 };
int voxe_render_route(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R);

/* disparity = 1 / max(1e-10, depth / acc)   rendering/volumetric/accumulate.py:85-88
 *   chain rule of an upstream d_disparity [R] into d_depth / d_acc (what autograd does through those three tensor ops):
 *   d_depth_out = d_depth_in + dq / acc,  d_acc_out = d_acc_in - dq * depth / acc^2,  dq = -d_disparity / q^2 where
 *   q = depth / acc > 1e-10, 0 elsewhere (and wherever a term is NaN / infinite: rays that miss the volume).
 *   d_*_in may be NULL (= 0); the outputs may alias the inputs.                                                       */
int voxe_disparity_bwd(const float* depth, const float* acc, const float* d_disparity, const float* d_depth_in,
                       const float* d_acc_in, float* d_depth_out, float* d_acc_out, int64_t R, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One iteration of the reconstruction loop in ONE call   modules/trainers.py:288-351
 *   (cast the rays of a random pixel batch over K cached cameras -> render specular [-> render diffuse] -> L1 loss(es)
 *   against the target pixels -> backward -> Adam): the same kernels the separate entry points launch, enqueued back to
 *   back on `stream` with no host work in between -- at 32768 rays the host side of ~45 framework-level launches was
 *   one third of the iteration.
 *   batch   : voxe_random_subset(K*H*W, batch, cfg->seed, cfg->rng_offset) picks flat (camera, y, x) pixels (a uniformly
 *             random set of distinct pixels, like the reference's randperm subset); rays by voxe_cast_rays_indexed; target
 *             pixels gathered from images [N,3,H,W] (row image_rows[camera], or camera itself when image_rows == NULL);
 *   renders : cfg as given with the jitter stream (seed, rng_offset + 1) for the specular render and, when
 *             diffuse_regularisation != 0, a second render with render_diffuse = 1 and the stream (seed, rng_offset + 2)
 *             (trainers.py:316,333); each runs in its own workspace (per-ray states), both gradients sum into the FIRST
 *             workspace's gradient region (voxe_render_bwd_acc_into);
 *   loss    : mean |colour - target| per render (torch.nn.functional.l1_loss), summed; losses[0..3] (DEVICE floats) receive
 *             L1 specular, MSE specular (the trainer logs it as PSNR), L1 diffuse, MSE diffuse (the diffuse pair is written
 *             only when diffuse_regularisation != 0: without that render losses[2..3] keep what they held);
 *   update  : voxe_grid_adam_step over the whole grid with the given Adam state / hyper-parameters; afterwards
 *             `workspace` holds the updated grid packed (pass cfg->reuse_packed_grid = 1 next time) and a cleared gradient.
 *   scratch : voxe_recon_scratch_bytes(batch) bytes of device memory (rays, targets, outputs, upstream gradients).
 *   SH-0 grids with diffuse_regularisation: when `workspace` holds voxe_workspace_bytes(grid, cfg, 2 * batch) bytes, both
 *   renders run as ONE launch of 2 * batch rays (same rays, jitter streams offset + 1 / + 2 as below; one binning pass,
 *   one forward, one backward) and `workspace2` is not touched; a smaller `workspace` takes the two-render path.
 *   Requires an SH grid (3 colour channels).  Arithmetic identical to the composition of the separate calls.        */
typedef struct {
  int32_t H, W;
  float focal;
  const float* poses;           /* [K,3,4] camera-to-world (rotation | translation), device                    */
  const int64_t* image_rows;    /* [K] rows of `images` of the K cameras, device; NULL = 0 .. K-1              */
  const float* images;          /* [N,3,H,W] device                                                            */
  int32_t num_images;           /* N: every entry of image_rows (or K itself when image_rows == NULL) must be below it;
                                   a row outside [0, N) reads nothing and makes that pixel's target NaN (ABI v7)        */
  int32_t K;
  int64_t batch;                /* rays per iteration                                                          */
  int32_t diffuse_regularisation;
  float lr, beta1, beta2, eps;
  int64_t step_densities, step_features;   /* 1-based Adam steps (torch counts per parameter)                  */
  float *exp_avg_densities, *exp_avg_sq_densities, *exp_avg_features, *exp_avg_sq_features;
  float* losses;                /* [4] device                                                                  */
  int32_t zero_gradient_first;  /* != 0: clear the gradient region of `workspace` first (a workspace no fused step has
                                   left cleared yet)                                                           */
} VoxeReconStep;
size_t voxe_recon_scratch_bytes(int64_t batch);
int voxe_recon_step(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const VoxeReconStep* step,
                    void* workspace, size_t workspace_bytes, void* workspace2, size_t workspace2_bytes,
                    void* scratch, size_t scratch_bytes, void* stream);
/* ABI v12.  The NEXT iteration's batch, assembled ahead of its call -- a hint, never a requirement.
 *   Batch assembly (subset, rays, target pixels) and the space-binning passes of the paired SH-0 render read the cameras,
 *   the images and the jitter streams, never the grid: modules/trainers.py:288-312 of iteration i + 1 does not depend on
 *   optimizer.step() of iteration i.  Call this right after voxe_recon_step(i) with the arguments voxe_recon_step(i + 1) WILL
 *   be called with (same pointers and sizes; only cfg->rng_offset, step->poses / image_rows and the Adam step counters
 *   normally differ -- the Adam fields, `losses` and cfg->reuse_packed_grid / ray_state_valid are not looked at): the library
 *   enqueues that work on a stream of its own, ordered behind iteration i's forward, where it overlaps iteration i's
 *   backward and grid step (what that is worth: ~1 % of a device-paced loop, and all the time a slow host would otherwise
 *   leave the device idle -- DESIGN 4.5).  The following voxe_recon_step waits for it and skips its own
 *   batch assembly / binning iff every argument that decides them equals the announced one; otherwise it waits and proceeds
 *   exactly as if no hint had been given.  Results do not depend on whether, or with what, this was called.
 *   The tables of the hint live in the region scratch of `workspace2` (which must hold voxe_workspace_bytes(grid, cfg,
 *   2 * batch) bytes like `workspace`) and alternate with those of `workspace`; `scratch` holds both batches
 *   (voxe_recon_scratch_bytes).  ORDER: the side stream is ordered behind the forward of the voxe_recon_step that was
 *   enqueued last on this workspace -- not behind this call -- so next_step->poses / image_rows / images must be complete on
 *   `stream` BEFORE that step was enqueued (draw the next iteration's cameras first, then call the step, then this), and
 *   stay valid and unchanged until the step that consumes the hint has been enqueued.  Freeing or reusing `workspace2` / `scratch` while a hint is in flight needs a device
 *   synchronisation first (the side stream is the library's own).  Returns VOXE_OK without doing anything when the iteration
 *   would not take the paired route (view-dependent grid, no diffuse regularisation, workspaces too small).            */
int voxe_recon_prefetch(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const VoxeReconStep* next_step,
                        void* workspace, size_t workspace_bytes, void* workspace2, size_t workspace2_bytes,
                        void* scratch, size_t scratch_bytes, void* stream);
/* (test aid) out[3]: hints issued | taken by the step that followed | dropped by it (arguments differed), process-wide */
int voxe_recon_prefetch_stats(int64_t* out);

/* ------------------------------------------------------------------------------------------------
 * One attention grid's share of an iteration of the refinement loop in ONE call (ABI v10)
 *   modules/attn_grid_trainer.py:335-378 -- per grid (edit / object): render_rays_attn -> calc_loss_on_attn_grid
 *   (modules/refinement_functions.py:42-77) + attn_tv_weight * _tv_loss_on_grid (:659-663) -> backward -> Adam step of the
 *   attention tensor.  The cross-attention map of the UNet (`attn_map`, the boundary to the networks) is an INPUT: the
 *   reference computes it before the attention renders, so everything behind it is grid work and runs here back to back on
 *   `stream`: voxe_render_fwd -> masked L1 + its gradient (one block) -> voxe_render_bwd_acc (attention channel only: the
 *   densities are frozen) -> voxe_tv_fwd_bwd -> voxe_grid_adam_step.  Arithmetic identical to the composition of those calls.
 *   grid     : VOXE_FEAT_ATTN; grid->features is the attention tensor [X,Y,Z,1], updated in place;
 *   rays     : [R,3] device, image order when cfg->image_width > 0 (R = H * W); jitter stream (cfg->seed, cfg->rng_offset);
 *   losses   : [2] device floats (or NULL): masked L1, TV (unweighted);
 *   scratch  : voxe_attn_refine_scratch_bytes(grid, R) bytes of device memory (outputs, upstream gradient, TV gradient).
 *   Afterwards `workspace` holds the updated grid packed and a cleared gradient region, like voxe_grid_adam_step.        */
/* calc_loss_on_attn_grid  modules/refinement_functions.py:42-77 (+ autograd), on its own:
 *   mask = render > 0;  *loss_out = sum(|render - map| * mask) / sum(mask);  d_render = ((1 / sum(mask)) * mask) * sign(render - map)
 *   render, map, d_render: [n] device floats; loss_out: device float or NULL; scratch: voxe_attn_masked_l1_scratch_bytes() bytes. */
size_t voxe_attn_masked_l1_scratch_bytes(void);
int voxe_attn_masked_l1(const float* render, const float* attn_map, int64_t n, float* d_render, float* loss_out,
                        void* scratch, size_t scratch_bytes, void* stream);

typedef struct {
  const float* attn_map;        /* [R] device, row-major like the rays                                          */
  float tv_weight;              /* attn_tv_weight; 0: no TV gradient (and no TV pass unless tv_loss_always)      */
  int32_t tv_loss_always;       /* != 0: losses[1] is evaluated even when tv_weight == 0                         */
  float lr, beta1, beta2, eps;
  int64_t step;                 /* 1-based Adam step of the attention tensor                                    */
  float *exp_avg, *exp_avg_sq;  /* [X,Y,Z,1] Adam state of the attention tensor                                 */
  float* losses;                /* [2] device or NULL                                                           */
  float* attn_render;           /* [R] device or NULL: receives the rendered attention image (logging)          */
  int32_t zero_gradient_first;  /* != 0: clear the gradient region of `workspace` first                         */
} VoxeAttnRefineStep;
size_t voxe_attn_refine_scratch_bytes(const VoxeGridDesc* grid, int64_t R);
int voxe_attn_refine_step(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, const VoxeAttnRefineStep* step,
                          const float* rays_o, const float* rays_d, int64_t R, void* workspace, size_t workspace_bytes,
                          void* scratch, size_t scratch_bytes, void* stream);

/* Measurement aids (bench.py, tests): not part of the reference's interface.
 * voxe_clock_probe        sustained shader clock in Hz: a chip-filling VALU + LDS kernel on `stream` reads the shader-clock
 *                         and the constant reference-clock counters around its loop (blocking; `spin` iterations per
 *                         thread, <= 0: default, ~0.3 ms of device time);
 * voxe_region_debug_layout byte offsets (from the start of the workspace) and dimensions of the segment tables of the
 *                         space-binned route: out[0] = offset of the region scratch, out[1..16] = {slot_region, slot_pos,
 *                         slot_seg, sorted, lane_n, count, start} offsets inside it, nslots, nlanes, nreg, slots per
 *                         lane, region edge x / y / z (cells), length classes, longest segment; VOXE_ERR_UNSUPPORTED when
 *                         (grid, cfg, R) does not take that route.                                                    */
int voxe_clock_probe(int32_t spin, double* shader_hz, void* stream);
int voxe_region_debug_layout(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg, int64_t R, int64_t out[17]);

/* torch.optim.Adam(betas, eps, weight_decay=0, amsgrad=False) single-tensor step
 *   modules/sds_trainer.py:200-203, modules/trainers.py:247-255; `step` is the 1-based step count. */
int voxe_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, int64_t step, void* stream);

/* scale_voxel_grid_with_required_output_size  thre3d_reprs/voxels.py:409-447
 *   F.interpolate(mode="trilinear", align_corners=False, recompute_scale_factor=False)
 *   src [X,Y,Z,C] -> dst [X2,Y2,Z2,C]                                                            */
int voxe_upsample_trilinear(const float* src, int32_t X, int32_t Y, int32_t Z, int32_t C,
                            float* dst, int32_t X2, int32_t Y2, int32_t Z2, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Refinement stage: 3-D grid graph cut and connected components.
 * Integer / byte work on whole grids; results are bit-exact between libvoxe_hip.so and the oracle.
 * ---------------------------------------------------------------------------------------------- */

/* capacity quantum: an n-link of affinity exp(-l2/sigma) == 1 gets VOXE_GRAPH_CAP_ONE units per contribution */
#define VOXE_GRAPH_CAP_ONE (1 << 28)
/* direction order of the six n-link capacity planes */
enum { VOXE_DIR_XP = 0, VOXE_DIR_XM = 1, VOXE_DIR_YP = 2, VOXE_DIR_YM = 3, VOXE_DIR_ZP = 4, VOXE_DIR_ZM = 5 };

/* Graph construction of build_graph   modules/refinement_functions.py:182-287
 *   density_grid [X,Y,Z], feature_grid [X,Y,Z,F] (= sigmoid(_features), :378; pooled grids in the
 *   down-sampled branch :189-196).
 *   nodes      : dilate_yz = 1 -> `MaxPool3d(3, 1, 1)(densities[X,Y,Z,1]) > 0` (:186,:200): a 4-D input makes X the
 *                channel axis, so the dilation runs over the Y-Z plane only;  0 -> `density_grid > 0` (:194);
 *   n-links    : node i adds an edge (w, w) to each of its 6 neighbours n with density_grid[n] > 0 (:261-287),
 *                w = K * exp(-l2(feature_i - feature_n) / sigma); a pair of nodes therefore carries
 *                w * ([density_i > 0] + [density_n > 0]) in both directions.  The reference's bounds test (:264-266)
 *                compares every coordinate of n with x, y AND z, i.e. with min(X,Y,Z): on non-cubic grids a voxel
 *                with a coordinate >= min(X,Y,Z) is never visited as a neighbour (reproduced);  K scales every capacity alike
 *                and, with infinite seed t-links only (:252-257), cannot change the cut: capacities are stored as
 *                integers  llrint(exp(-l2/sigma) * VOXE_GRAPH_CAP_ONE) * multiplicity.
 *   node_mask u8 [X,Y,Z];  cap int32 [6,X,Y,Z] (VOXE_DIR_* planes; 0 where there is no edge).            */
int voxe_graph_build(const float* density_grid, const float* feature_grid,
                     int32_t X, int32_t Y, int32_t Z, int32_t F, float sigma, int32_t dilate_yz,
                     uint8_t* node_mask, int32_t* cap, void* stream);

/* g.maxflow() + g.get_segment()   modules/refinement_functions.py:289-294   (PyMaxflow 1.x, Boykov-Kolmogorov)
 *   terminal int8 [X,Y,Z]: +1 = add_tedge(inf, 0) ("edit" seed, source), -1 = add_tedge(0, inf) ("object" seed,
 *   sink), 0 = no t-link.  cap is consumed (holds the residual capacities on return); every capacity must be
 *   <= 2^29 so that a residual (forward + reverse capacity of a pair) stays below 2^31.
 *   segment u8 [X,Y,Z]: 255 = not a node, 1 = the node can still reach a sink seed in the residual graph of a
 *   maximum flow (BK's sink tree, get_segment == 1), 0 = otherwise (get_segment == 0, "edit").  That set is the
 *   same for every maximum flow, so any exact solver yields the same labels.
 *   flow int64[1]: value of the maximum flow in capacity units.
 *   BLOCKING: synchronises `stream` (the iteration count is data dependent).                             */
size_t voxe_graphcut_scratch_bytes(int32_t X, int32_t Y, int32_t Z);
int voxe_graphcut(const uint8_t* node_mask, const int8_t* terminal, int32_t* cap,
                  int32_t X, int32_t Y, int32_t Z, uint8_t* segment, int64_t* flow,
                  void* scratch, size_t scratch_bytes, void* stream);

/* cc3d.largest_k(mask, k, connectivity=26, delta=0)   edit_pretrained_relu_field.py:384-389,411-416
 *   mask u8 [X,Y,Z] (non-zero = foreground).  labels int32 [X,Y,Z]: 0 = background or a component that is not
 *   among the k largest; the M = min(k, N) largest components are numbered 1..M in ascending size (the largest
 *   is M; equal sizes: the component whose first voxel in memory order comes first counts as larger).
 *   num_components int32[1] = N (all 26-connected components).                                            */
size_t voxe_cc_scratch_bytes(int32_t X, int32_t Y, int32_t Z, int32_t k);
int voxe_cc_largest_k(const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t k,
                      int32_t* labels, int32_t* num_components,
                      void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh export (ABI v13): marching cubes over the density iso-surface, DESIGN.md section 4 "Mesh export".
 *   v_i = pre(density_scale * densities[i]) per voxel, 0 where mask[i] == 0 (mask u8 [X,Y,Z], NULL = none); the padded
 *   lattice has nodes at voxel indices -1..N per axis (0 outside the grid).  The surface is trilerp(v) = L with
 *   L = post^-1(level) (Identity / ReLU: level; Softplus: level > 20 ? level : log(expm1(level))), i.e. where the
 *   un-masked density VoxelGrid.forward returns equals `level`; level must exceed post(0) (0, or ln 2 for Softplus), so
 *   that the zero-padded ring is outside and every surface is closed (VOXE_ERR_BAD_SHAPE otherwise).  A node is inside
 *   iff v > L.  Only `densities`, the dims and the density activation fields of the descriptor are read.
 *   voxe_mesh_count: totals (DEVICE int64[2]) = (V, T); the case per node and the scan offsets stay in scratch
 *                    (>= voxe_mesh_scratch_bytes(X, Y, Z) bytes) for voxe_mesh_emit.
 *   voxe_mesh_emit : same grid, level, mask and scratch, on the same stream, after voxe_mesh_count:
 *                    vertices f32 [V,3] in world space: one per crossing lattice edge, numbered by (node, axis), at
 *                    t = (L - v_a) / (v_b - v_a) along the edge; faces int32 [T,3] numbered by (cell, table order),
 *                    counter-clockwise seen from outside (normals toward lower density).  Nothing is written past
 *                    max_vertices / max_faces (a grid changed since the count gives a wrong mesh, never a bad access).
 *   Deterministic: the output is the same bit for bit from run to run.  (X+2)(Y+2)(Z+2) * 5 (the table's most triangles per
 *   cell) must stay below 2^31 (VOXE_ERR_BAD_SHAPE otherwise).  Feature kind SH or attention; the features are not read.         */
size_t voxe_mesh_scratch_bytes(int32_t X, int32_t Y, int32_t Z);
int voxe_mesh_count(const VoxeGridDesc* grid, float level, const uint8_t* mask, int64_t* totals,
                    void* scratch, size_t scratch_bytes, void* stream);
int voxe_mesh_emit(const VoxeGridDesc* grid, float level, const uint8_t* mask,
                   float* vertices, int64_t max_vertices, int32_t* faces, int64_t max_faces,
                   void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Density-gradient normals (additive; still ABI v13), DESIGN.md section 4 "Normals".
 *   The field is the mesh export's: v_i = pre(density_scale * densities[i]), V(p) its trilinear interpolant (grid_sample
 *   semantics, zero padding), u_a = ((p_a * scale_a + bias_a + 1) * N_a - 1) / 2 as in the renderer, the cell floor(u).
 *   G_a(p) = dV/du_a * (N_a * norm_scale_a / 2): the derivative of exactly what VoxelGrid.forward evaluates in that cell
 *   (corners outside the grid count as 0, also for the slope at the faces), in world units.  n(p) = -G / |G| in f32,
 *   (0,0,0) where G == 0: toward lower density, outward on a solid (the side the mesh export's faces wind toward).
 *   voxe_query_normals : points [N,3] (world) -> normals [N,3] = n(p); points outside the grid give (0,0,0).
 *   voxe_render_normals: per ray r, normals [R,3] = sum_k w_k n(p_k) (world space, NOT renormalised: |N_r| <= acc_r, no
 *                        background, white_bkgd does not apply), depth [R,1] = sum_k w_k z_k, acc [R,1] = sum_k w_k (either
 *                        may be NULL), with the points p_k and weights w_k = T_k alpha_k of voxe_render_fwd for the same rays,
 *                        cfg and jitter / (seed, rng_offset).  cfg fields honoured: num_samples, near, far, perturb,
 *                        linear_disparity, aabb_clip, seed, rng_offset; image_width / image_height only choose the ray -> thread
 *                        mapping (pixel tiles when they describe R exactly, linear order otherwise).  Every other field
 *                        (white_bkgd, sh_degree, render_diffuse, term_eps, reuse_packed_grid, deterministic, linear_grad,
 *                        ray_state_valid, dispatch) is ignored.
 *   Only grid->densities ([X,Y,Z,1]) is read: features, F and feature_kind are ignored (features may be NULL), so SH and
 *   attention grid descriptors both work.  No workspace: nothing is packed, no forward record is read or dropped, no
 *   voxe_recon_prefetch hint is touched.  Caller's stream, no host synchronisation, no allocation, no atomics: the same bits
 *   on every run.  Pointers may be NULL when N / R is 0 (VOXE_OK, no launch); R and the voxel count stay below 2^31 and the
 *   grid within validate's 24-bit index limits (VOXE_ERR_BAD_SHAPE otherwise), as does num_samples <= 0.            */
int voxe_query_normals(const VoxeGridDesc* grid, const float* points, int64_t N, float* normals, void* stream);
int voxe_render_normals(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                        const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                        float* normals, float* depth, float* acc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-voxel visibility (additive; still ABI v13), DESIGN.md section 4 "Visibility".
 *   voxe_visibility_accumulate: the samples p_k, depths z_k, inside test and weights w_k = T_k alpha_k (T_k: the transmittance
 *       on arrival at sample k) are those of voxe_render_fwd / voxe_render_normals for the same rays, cfg and jitter / (seed,
 *       rng_offset); the cfg fields honoured and ignored are those of voxe_render_normals.  For every sample that passes the
 *       strict AABB test and each of its 8 footprint corners c inside the grid, with the forward's gather weight
 *       t_c = (wx * wy) * wz:
 *           max_weight[c] = max(max_weight[c], w_k * t_c)
 *           max_trans[c]  = max(max_trans[c],  T_k)            where t_c > 0
 *       (contributions <= 0 or NaN are skipped).  The call ACCUMULATES into max_weight / max_trans (f32 [X,Y,Z], either may be
 *       NULL): the caller zeroes them before the first call, and their contents must be finite and >= 0.  Both NULL or R == 0:
 *       VOXE_OK, no launch.  Two properties are part of the contract:
 *         - order independence, bit for bit: non-negative floats order like their bit patterns, the update is an unsigned
 *           integer atomic max, so the result does not depend on how lanes, waves or launches meet on a voxel;
 *         - what a ray contributes depends on that ray and cfg only -- not on R, the ray's position in the batch or
 *           image_width / image_height (those only choose the ray -> thread mapping): K cameras in one launch, K launches,
 *           linear and shuffled order all give the same bits.
 *       Only grid->densities is read; no workspace, no forward record, no voxe_recon_prefetch hint is touched.  Caller's
 *       stream, no host synchronisation, no allocation.  Validation, the limits on R and the voxel count and the error codes
 *       are those of voxe_render_normals.
 *   voxe_visibility_mask: mask[i] (u8 [X,Y,Z]) = 1 iff some voxel j of the grid within Chebyshev distance `dilate` of i has
 *       vis[j] > threshold, else 0.  The comparison is strict (threshold 0 keeps exactly the voxels that ever contributed) and
 *       NaN is never kept.  dilate in 0..3 and X * Y * Z < 2^31 (VOXE_ERR_BAD_SHAPE otherwise).  One pass, deterministic.     */
int voxe_visibility_accumulate(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                               const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                               float* max_weight /* [X,Y,Z] or NULL */, float* max_trans /* [X,Y,Z] or NULL */,
                               void* stream);
int voxe_visibility_mask(const float* vis, int32_t X, int32_t Y, int32_t Z, float threshold, int32_t dilate,
                         uint8_t* mask /* [X,Y,Z] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Lifting per-ray values into the grid by weighted back-projection (additive; still ABI v13), DESIGN.md section 4.16 "Lifting".
 *   voxe_lift_accumulate: the samples, depths, inside test, T_k and w_k = T_k alpha_k are those of voxe_visibility_accumulate
 *       for the same rays, cfg and jitter / (seed, rng_offset); the cfg fields honoured and ignored, the validation, the limits
 *       and the error codes are those of voxe_visibility_accumulate.  For every sample that passes the strict AABB test and each
 *       of its 8 footprint corners c inside the grid, with a = w_k * t_c -- the float32 value voxe_visibility_accumulate raises
 *       max_weight with, t_c = (wx * wy) * wz:
 *           sum_w[c]      += q(a)
 *           sum_wv[c, ch] += q(a * values[r, ch])      ch = 0 .. C-1, the product rounded to float32
 *           q(x) = (int64) round-to-nearest-even(x * 2^32)
 *       The sums are 64-bit fixed point with 32 fraction bits, added with integer atomics: integer addition is associative, so
 *       the result is the same bit for bit whatever the order of lanes, waves, launches and cameras.  A contribution whose q is 0
 *       is skipped (an exact no-op).  values (f32 [R,C]) must be finite with |v| <= 1: a voxel then has room for 2^31 full-size
 *       contributions.  The call ACCUMULATES into sum_wv (int64 [X,Y,Z,C]) and sum_w (int64 [X,Y,Z]); the caller zeroes them
 *       first.  What a ray contributes depends on that ray and cfg only -- not on R, the ray's position in the batch or
 *       image_width / image_height.
 *         C in 1..8 with values and sum_wv both given: full accumulation (sum_w may still be NULL);
 *         values and sum_wv both NULL: coverage only (C is not read);
 *         exactly one of the two NULL: VOXE_ERR_NULL_POINTER (as for the rays, not when R == 0, where nothing is read);
 *         either given and C outside 1..8: VOXE_ERR_BAD_SHAPE;
 *         both outputs NULL, or R == 0: VOXE_OK, no launch.
 *       Only grid->densities is read; no workspace, no forward record, no voxe_recon_prefetch hint is touched.  Caller's
 *       stream, no host synchronisation, no allocation.
 *   voxe_lift_debug_merge: a test aid.  The kernel has two variants that return identical bits: one atomic per lane, corner and
 *       channel (1), and one that first sums, inside a wave, the contributions of lanes that sit in the same cell at the same
 *       step (2).  0 = the shipped choice (DESIGN.md 4.16 holds the measurement).  Pins the calling thread's later calls; any
 *       other value: VOXE_ERR_BAD_SHAPE.                                                                                      */
int voxe_lift_accumulate(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                         const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                         const float* values /* [R,C] or NULL */, int32_t C,
                         int64_t* sum_wv /* [X,Y,Z,C] or NULL */, int64_t* sum_w /* [X,Y,Z] or NULL */, void* stream);
int voxe_lift_debug_merge(int32_t mode);

/* ------------------------------------------------------------------------------------------------
 * Vector quantisation of feature vectors against a codebook (additive; still ABI v13), DESIGN.md section 4.25 "Compression".
 *   Both calls: N points of F channels, K codewords; F in 1..64, K in 1..65536, 0 <= N < 2^31 (VOXE_ERR_BAD_SHAPE otherwise,
 *   checked first); N == 0: VOXE_OK, no launch, no pointer is looked at; otherwise a NULL pointer other than `dist` gives
 *   VOXE_ERR_NULL_POINTER.  All inputs finite.  Caller's stream, no host synchronisation, no allocation, no workspace.
 *   voxe_vq_assign: index[n] (int32 [N]) is a codeword k that minimises the float32 score
 *           s(n, k) = |c_k|^2 - 2 x_n . c_k
 *       evaluated on the matrix cores as the chain  s = fma(-2 c_kj, x_nj, s)  over ascending channel j, started at
 *       code_norm[k] = sum_j c_kj^2 (plain float32 sum of the rounded squares, ascending j), which a pre-pass of the same call
 *       writes into code_norm (f32 [K], every element).  Among codewords whose float32 scores are bit-equal the lowest k wins;
 *       the scores of duplicated codewords are bit-equal, so the first copy wins.  The arg-min is taken inside the kernel: no
 *       N x K intermediate exists and nothing but code_norm, index and dist is written.  The result does not depend on N, on the
 *       point's position in the batch or on what the outputs held before: two calls return the same bits.
 *       dist[n] (f32 [N], or NULL), is recomputed after the choice for k = index[n] as the plain float32 sum
 *           d = 0;  for j = 0 .. F-1:  u = x_nj - c_kj;  d = d + u * u        each operation rounded, no FMA
 *       so a float32 loop on the host reproduces it bit for bit given the index.  It is exactly 0 for a point equal to its
 *       codeword, which the score s (a difference of large terms) cannot promise.
 *   voxe_vq_accumulate: the weighted centroid sums in the fixed point of voxe_lift_accumulate.  For every point n with
 *       k = index[n] in 0..K-1:
 *           sum_w[k]     += q(w_n)
 *           sum_wx[k, j] += q(w_n * x_nj)       j = 0 .. F-1, the product rounded to float32
 *           q(x) = (int64) round-to-nearest-even(x * 2^32)
 *       with 64-bit integer atomics: integer addition is associative, so the result is the same bit for bit whatever the order
 *       of points, lanes, waves and launches -- shuffled points, the call split in two and both kernel variants agree exactly.
 *       A contribution whose q is 0 is skipped (an exact no-op).  Requirements: |x| <= 1 and 0 <= w <= 1 (a codeword then has
 *       room for 2^31 full-size contributions).  The call ACCUMULATES into sum_wx (int64 [K,F]) and sum_w (int64 [K]); the
 *       caller zeroes them first.  A point whose index lies outside 0..K-1 deposits nothing and no memory outside the sums is
 *       touched; the call has no status word to report it through, so it is the caller who validates the index (the Python
 *       wrapper does, and answers with VOXE_ERR_BAD_SHAPE).
 *   voxe_vq_debug_merge: a test aid.  The accumulate kernel has two variants that return identical bits: one atomic per lane
 *       and channel (1), and one that first sums, inside a wave, each run of consecutive lanes with the same index (2): on
 *       points sorted by index a wave then issues one atomic per run.  0 = the shipped choice (DESIGN.md 4.25 holds the
 *       measurement).  Pins the calling thread's later calls; any other value: VOXE_ERR_BAD_SHAPE.                            */
int voxe_vq_assign(const float* points /* [N,F] */, int64_t N, int32_t F, const float* codebook /* [K,F] */, int32_t K,
                   float* code_norm /* [K], written */, int32_t* index /* [N] */, float* dist /* [N] or NULL */, void* stream);
int voxe_vq_accumulate(const float* points /* [N,F] */, const float* weights /* [N] */, const int32_t* index /* [N] */,
                       int64_t N, int32_t F, int32_t K, int64_t* sum_wx /* [K,F] */, int64_t* sum_w /* [K] */, void* stream);
int voxe_vq_debug_merge(int32_t mode);

/* ------------------------------------------------------------------------------------------------
 * Distortion loss on rays (additive; still ABI v13), DESIGN.md section 4.11 "Distortion".
 *   The samples z_k, the inside test, sigma_k, delta_k and the weights w_k = T_k alpha_k (last dl = 1e10) are those of
 *   voxe_render_fwd / voxe_render_normals / voxe_visibility_accumulate for the same rays, cfg and jitter / (seed, rng_offset);
 *   the cfg fields honoured and ignored are those of voxe_render_normals.  With s_k = (z_k - near) / (far - near) -- ALWAYS
 *   cfg's near and far, also under aabb_clip and linear_disparity (far > near for a finite result):
 *       d_k = s_{k+1} - s_k for k < S-1, d_{S-1} = 0      (the interval the renderer's quadrature gives sample k)
 *       m_k = s_k + d_k / 2
 *       L_r = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
 *       loss = (1/R) sum_r L_r
 *   Samples that fail the AABB test have w = 0 and contribute nothing.  Gradient w.r.t. the raw densities [X,Y,Z,1]:
 *       g_i = dL_r/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i d_i
 *       dL_r/dsigma_k = delta_k [g_k (T_k - w_k) - sum_{i>k} g_i w_i]
 *   and from there through post_activate', the gather weights t_c = (wx * wy) * wz and pre_activate' * density_scale into the
 *   8 footprint corners, with the derivative conventions of voxe_render_bwd.  The samples are constants: no gradient flows
 *   to z.  The kernel evaluates |m_i - m_j| as m_i - m_j for j < i: the renderer's depths never decrease along a ray.
 *   Outputs (each may be NULL): loss_out  device float[1], the UNWEIGHTED mean (grad_scale does not apply to it);
 *                               ray_loss  device [R], L_r;
 *                               d_densities [X,Y,Z,1] = grad_scale * dloss/draw, added to the buffer when accumulate != 0,
 *                               else the buffer is zeroed first (voxels no sample touches keep an exact 0).
 *   The running sums per ray are double, the per-sample work float; the gradient goes through float atomics, so it can differ
 *   in the last bits from run to run (loss and ray_loss do not).  `scratch` (voxe_distortion_scratch_bytes(R), read only when
 *   loss_out != NULL) carries the per-block partials of the loss; too small: VOXE_ERR_WORKSPACE.  R == 0 or all three outputs
 *   NULL: VOXE_OK with no launch (accumulate == 0 with a non-NULL d_densities still zeroes it).  Only grid->densities is read
 *   (SH and attention descriptors both work); no workspace, no forward record, no voxe_recon_prefetch hint is touched.
 *   Caller's stream, no host synchronisation, no allocation.  Validation, the limits on R and the voxel count and the error
 *   codes are those of voxe_render_normals.
 *   voxe_distortion_debug_lanes: test aid.  The kernel splits a ray over 1, 2, 4 or 8 lanes by R; a value of 1 / 2 / 4 / 8 pins
 *   the split for the calling thread's later calls, 0 restores the choice by R (anything else: VOXE_ERR_BAD_SHAPE).        */
size_t voxe_distortion_scratch_bytes(int64_t R);
int voxe_distortion_fwd_bwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                            const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                            float grad_scale,
                            float* loss_out      /* device float[1] or NULL: the UNWEIGHTED mean */,
                            float* ray_loss      /* device [R] or NULL: L_r */,
                            float* d_densities   /* [X,Y,Z,1] or NULL: grad_scale * dloss/draw */,
                            int32_t accumulate   /* as voxe_tv_fwd_bwd / voxe_render_bwd */,
                            void* scratch, size_t scratch_bytes, void* stream);
int voxe_distortion_debug_lanes(int32_t lanes);

/* ------------------------------------------------------------------------------------------------
 * Depth supervision: ray-termination loss towards per-ray depth targets (additive; still ABI v13), DESIGN.md section 4.19.
 * DS-NeRF's term (Deng et al., CVPR 2022) as its published code evaluates it; no voxe_cpu_ twin, the float64 restatement is
 * tests/depth_ref.py.
 *   The samples z_k, the inside test, sigma_k, delta_k = dl_k |d| (last dl = 1e10) and T_k are those of
 *   voxe_distortion_fwd_bwd for the same rays, cfg and jitter / (seed, rng_offset), and so are the cfg fields honoured and
 *   ignored.  The weights w_k = T_k alpha_k are those of the same call in exact arithmetic; this call forms its alpha_k as
 *   -expm1(-sigma_k delta_k) (w sits at or below eps in a nearly empty field, where 1 - exp cancels), the transmittance
 *   product keeps the renderer's 1 - alpha.  With a target depth D_r and a width s_r > 0 per ray, both in the units of z_k:
 *       dz_k = z_{k+1} - z_k for k < S-1, dz_{S-1} = 0
 *       c_k  = exp(-(z_k - D_r)^2 / (2 s_r^2)) dz_k
 *       L_r  = -sum_k c_k log(w_k + eps)
 *       loss = (1/R) sum_r omega_r L_r                      (omega = ray_weight, 1 when NULL)
 *   over ALL S samples: one that fails the AABB test, or lies behind the point where T reaches 0, has w = 0 and contributes
 *   -c_k log(eps) to the value and nothing to the gradient.  eps must be finite and > 0 (VOXE_ERR_BAD_SHAPE otherwise);
 *   DS-NeRF's is 1e-5.  Gradient w.r.t. the raw densities [X,Y,Z,1]:
 *       g_k = dL_r/dw_k = -c_k / (w_k + eps)
 *       dL_r/dsigma_k = delta_k [g_k (T_k - w_k) - sum_{i>k} g_i w_i]
 *   and from there through post_activate', the gather weights and pre_activate' * density_scale into the 8 footprint
 *   corners as in voxe_distortion_fwd_bwd, scaled by grad_scale * omega_r / R.  No gradient flows to z, D, s or omega.
 *   target_depth / target_sigma NULL with R > 0: VOXE_ERR_NULL_POINTER.  The caller guarantees finite D, finite s > 0 and
 *   finite omega >= 0; the three arrays are read for [R] only.
 *   Outputs (each may be NULL): loss_out  device float[1], the weighted mean above (grad_scale does not apply to it);
 *                               ray_loss  device [R], L_r (without omega_r);
 *                               d_densities [X,Y,Z,1], accumulate as in voxe_distortion_fwd_bwd.
 *   loss_out and ray_loss are the same bits from run to run (fixed-order sums); the gradient goes through float atomics.
 *   scratch (voxe_depth_scratch_bytes(R), read only when loss_out != NULL), R == 0, all outputs NULL, validation, limits, error
 *   codes, stream and the "no workspace, no forward record, no voxe_recon_prefetch hint is touched" clause: as
 *   voxe_distortion_fwd_bwd.  voxe_depth_debug_lanes: test aid, as voxe_distortion_debug_lanes.                                */
size_t voxe_depth_scratch_bytes(int64_t R);
int voxe_depth_fwd_bwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                       const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                       const float* target_depth  /* [R] D_r, in the units of the renderer's z_k */,
                       const float* target_sigma  /* [R] s_r > 0, same units */,
                       const float* ray_weight    /* [R] or NULL (= 1) */,
                       float eps, float grad_scale,
                       float* loss_out, float* ray_loss, float* d_densities, int32_t accumulate,
                       void* scratch, size_t scratch_bytes, void* stream);
int voxe_depth_debug_lanes(int32_t lanes);

/* ------------------------------------------------------------------------------------------------
 * Orientation loss on rays (additive; still ABI v13), DESIGN.md section 4.20.  Ref-NeRF's regulariser (Verbin et al., CVPR 2022,
 * eq. 11) against weight on samples whose normal faces away from the viewer; no voxe_cpu_ twin, the float64 restatement is
 * tests/orientation_ref.py.
 *   The samples z_k, the inside test, sigma_k, delta_k = dl_k |d| (last dl = 1e10), T_k and w_k = T_k alpha_k are those of
 *   voxe_distortion_fwd_bwd for the same rays, cfg and jitter / (seed, rng_offset), and so are the cfg fields honoured and
 *   ignored.  The field of the normals is voxe_render_normals's: v_i = pre(density_scale * raw_i), V its trilinear interpolant
 *   with zero padding, G_k the world-space gradient of V in the cell of sample k (a face cell uses the slope with the padded
 *   0).  With u_r = d_r / |d_r| and a guard normal_eps >= 0 in the units of G:
 *       rho_k = sqrt(|G_k|^2 + normal_eps^2)
 *       c_k   = max(0, -(G_k . u_r)) / rho_k                (0 where rho_k == 0)
 *       L_r   = sum_k w_k c_k^2
 *       loss  = (1/R) sum_r omega_r L_r                     (omega = ray_weight, 1 when NULL)
 *   At normal_eps == 0, c_k = max(0, n_k . u_r) with n_k = -G_k / |G_k|, the normal voxe_render_normals composites.  A sample
 *   that fails the AABB test, or lies behind the point where T reaches 0, has w = 0 and contributes nothing.  |G|^2 neither
 *   overflows nor underflows for finite corner values.  normal_eps must be finite and >= 0 (VOXE_ERR_BAD_SHAPE otherwise).
 *   Gradient w.r.t. the raw densities [X,Y,Z,1], two parts on the same 8 footprint corners (one float atomic per corner and
 *   sample):
 *     through the weights:  dL_r/dsigma_k = delta_k [c_k^2 (T_k - w_k) - sum_{i>k} c_i^2 w_i], and from there through
 *       post_activate', the gather weights and pre_activate' * density_scale as in voxe_distortion_fwd_bwd;
 *     through the normals:  dL_r/dG_k = 2 w_k c_k (-u_r / rho_k - c_k G_k / rho_k^2) for c_k > 0, exactly 0 for c_k == 0 or
 *       rho_k == 0;  dG_a/dv_q = (N_a scale_a / 2) * (slope coefficient of corner q on axis a) * (the two other axes' cell
 *       weights), then pre_activate' * density_scale.  post_activate is not on this path.  In a face cell the slope coefficients
 *       are not the gather weights' differences: the padded 0 has a slope but no weight.
 *   Derivative conventions at the kinks of abs / ReLU: voxe_render_bwd's.  The sum is scaled by grad_scale * omega_r / R.  No
 *   gradient flows to the rays, to z or to omega.  The caller guarantees finite omega >= 0; ray_weight is read for [R] only.
 *   Outputs (each may be NULL): loss_out  device float[1], the weighted mean above (grad_scale does not apply to it);
 *                               ray_loss  device [R], L_r (without omega_r);
 *                               d_densities [X,Y,Z,1], accumulate as in voxe_distortion_fwd_bwd (0: the buffer is zeroed
 *                               first, so untouched voxels hold an exact 0).
 *   loss_out and ray_loss are the same bits from run to run (fixed-order sums); the gradient goes through float atomics.
 *   scratch (voxe_orientation_scratch_bytes(R), read only when loss_out != NULL), R == 0, all outputs NULL, validation, limits,
 *   error codes, stream and the "no workspace, no forward record, no voxe_recon_prefetch hint is touched" clause: as
 *   voxe_distortion_fwd_bwd.  voxe_orientation_debug_lanes: test aid, as voxe_distortion_debug_lanes.                         */
size_t voxe_orientation_scratch_bytes(int64_t R);
int voxe_orientation_fwd_bwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                             const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                             const float* ray_weight    /* [R] or NULL (= 1) */,
                             float normal_eps, float grad_scale,
                             float* loss_out, float* ray_loss, float* d_densities, int32_t accumulate,
                             void* scratch, size_t scratch_bytes, void* stream);
int voxe_orientation_debug_lanes(int32_t lanes);

/* ------------------------------------------------------------------------------------------------
 * Per-image exposure compensation (additive; still ABI v13), DESIGN.md section 4.21 "Exposure".  A learned 3x4 affine colour
 * transform per training image (3D Gaussian Splatting's exposure optimisation, URF's exposure term) under the photometric loss,
 * and the sums of the closed-form least-squares affine of the colour-corrected metrics (mip-NeRF 360, RawNeRF).  No grid, no
 * workspace, no voxe_cpu_ twin; the float64 restatement is tests/exposure_ref.py.
 *
 * voxe_exposure_fwd_bwd.  Inputs, device, read only: x [R,3] rendered colours, y [R,3] targets, image_id [R] int32,
 *   delta [N,12] row-major per image: dA (3x3, row-major) then db (3); ray_weight [R] or NULL (= 1).  kind: VOXE_DREG_L1 or
 *   VOXE_DREG_L2 (VOXE_ERR_UNSUPPORTED otherwise).  Per ray r with n = image_id[r]:
 *       A = I + dA_n,  c' = A x_r + db_n,  e = c' - y_r
 *       loss = (1/3R) sum_r omega_r sum_c |e_c|   (L1)   or   (1/3R) sum_r omega_r sum_c e_c^2   (L2)
 *       mse  = (1/3R) sum_r sum_c e_c^2                 (without omega, whichever the kind)
 *       g    = omega_r sign(e)   (L1, sign(0) = 0 as torch's l1_loss)   or   2 omega_r e   (L2)
 *       d_x_r      = (grad_scale / 3R) A^T g
 *       d_delta[n] = (grad_scale / 3R) sum_{r: image_id[r] = n} (g x_r^T row-major, g)
 *   An image_id outside [0, N) is clamped to the nearest end on the device: nothing is read or written out of bounds, and the
 *   ray counts for image 0 or N - 1.  Callers check their ids once per dataset, not per call.
 *   Outputs (each may be NULL = skipped): loss_out, mse_out device float[1] (grad_scale does not apply to them);
 *     corrected [R,3] = c';  d_x [R,3] (always overwritten);  d_delta [N,12]: accumulate == 0 writes every row, rows of images
 *     that no ray names as exact 0.0; accumulate != 0 adds to the rows that rays name and leaves the others untouched.
 *   d_delta is reduced without float atomics: each product is rounded to float, then to 64-bit fixed point with 32 fractional
 *   bits before grad_scale / 3R applies (resolution 2^-33 per product, unscaled sums below 2^31 in magnitude), every add from
 *   there is an integer add, and one conversion ends it (in double, then float: one float rounding; an unscaled sum of 2^21 or
 *   more rounds to a double's 53 bits first).  So d_delta, like loss_out and mse_out (double sums in a fixed
 *   order), holds the same bits from call to call, and d_delta also under any permutation of the rays.
 *   scratch: voxe_exposure_scratch_bytes(R, N) bytes of device memory (0 for shapes the call refuses), read and written when
 *   R > 0 and any of loss_out / mse_out / d_delta is given; missing or short: VOXE_ERR_WORKSPACE.  Limits: 0 <= R < 2^31,
 *   1 <= N < 2^24 (VOXE_ERR_BAD_SHAPE).  NULL delta, or NULL x / y / image_id with R > 0: VOXE_ERR_NULL_POINTER.  All validation
 *   precedes any device work.  R == 0: loss_out and mse_out that exist are set to 0, d_delta to zeros unless accumulate, and
 *   nothing else is touched.  All outputs NULL: VOXE_OK, nothing is launched.  Work is enqueued on `stream`.
 *
 * voxe_exposure_apply_bwd.  The chain rule of c' = A x + db alone, for a loss on the corrected colours formed outside this call
 *   (the trainer's SSIM term): with d_corrected [R,3] = dL/dc', device, read only,
 *       d_x_r = A^T d_corrected_r,   d_delta[n] = sum_{r: image_id[r] = n} (d_corrected_r x_r^T row-major, d_corrected_r)
 *   x, image_id, delta, N, the clamp of image_id, d_x, d_delta, accumulate, scratch (voxe_exposure_scratch_bytes(R, N), used when
 *   d_delta is given), limits, error codes and R == 0 as in voxe_exposure_fwd_bwd.  The fixed point's unit is 2^-33 / R',
 *   R' = R rounded up to a power of two (the gradient of a mean over the batch has entries near 1 / R; sums below 2^31 / R').
 *
 * voxe_exposure_fit_sums.  x, y [N,P,3] float32 (N images of P pixels), device, read only.  sums [N,25] float64, device, per
 *   image with u = (x_0, x_1, x_2, 1):  the 10 entries u_i u_j, i <= j, of sum u u^T in row-major order of the upper triangle
 *   (the last one is P);  the 12 of sum u y^T, row-major [4,3];  the 3 of sum y o y.  Products and sums are formed in double, in
 *   a fixed order: the same bits from call to call.  The host solves (sum u u^T) theta_c = (sum u y_c) per channel.
 *   scratch: voxe_exposure_fit_scratch_bytes(N, P) bytes, always required (VOXE_ERR_WORKSPACE).  Limits: 1 <= N <= 65535,
 *   1 <= P < 2^31 (VOXE_ERR_BAD_SHAPE).                                                                                        */
size_t voxe_exposure_scratch_bytes(int64_t R, int64_t N);
int voxe_exposure_fwd_bwd(const float* x, const float* y, const int32_t* image_id, int64_t R,
                          const float* delta, int64_t N, int32_t kind,
                          const float* ray_weight    /* [R] or NULL (= 1) */,
                          float grad_scale,
                          float* loss_out, float* mse_out, float* corrected, float* d_x, float* d_delta, int32_t accumulate,
                          void* scratch, size_t scratch_bytes, void* stream);
int voxe_exposure_apply_bwd(const float* x, const int32_t* image_id, int64_t R, const float* delta, int64_t N,
                            const float* d_corrected, float* d_x, float* d_delta, int32_t accumulate,
                            void* scratch, size_t scratch_bytes, void* stream);
size_t voxe_exposure_fit_scratch_bytes(int64_t N, int64_t P);
int voxe_exposure_fit_sums(const float* x, const float* y, int64_t N, int64_t P, double* sums,
                           void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Robust photometric loss on pixel patches (additive; still ABI v13), DESIGN.md section 4.22 "Robust loss".  RobustNeRF's
 * (Sabour et al. 2023) trimmed loss for captures with transient objects: a pixel is an outlier when its residual is above an
 * order statistic of the batch's residuals, an outlier is forgiven when its 3x3 neighbourhood or its patch is mostly inliers,
 * and the mask is a constant of the loss.  No grid, no workspace, no voxe_cpu_ twin; the restatement is tests/robust_ref.py.
 *
 * Inputs, device, read only: x, y [N,P,P,C] float32, channel-last (x a render's colour viewed as patches, y the photographs).
 *   Limits: N >= 1, P even, 4 <= P <= 64, C in 1..4, M = N P^2 < 2^31 (VOXE_ERR_BAD_SHAPE).  kind: VOXE_DREG_L1 or VOXE_DREG_L2
 *   (VOXE_ERR_UNSUPPORTED otherwise).  Integer parameters, so that no float comparison of the host decides a mask bit:
 *       rank       0 <= rank < M           the 0-based rank of the threshold among the M residuals
 *                                          (a quantile q: min(M - 1, max(0, ceil(q M) - 1)))
 *       smooth_min 1..9                    inliers needed in a pixel's 3x3 neighbourhood (5: "at least half of 9")
 *       patch_min  1 <= patch_min <= P^2+1 forgiven pixels needed in a patch (a fraction f: ceil(f P^2)); P^2 + 1: never
 *   out of range: VOXE_ERR_BAD_SHAPE.  Per pixel p, every operation rounded to float32:
 *       d_c = x_c - y_c,   e_p = d_0 d_0, then e_p = e_p + d_c d_c for c = 1 .. C-1 in that order (a sum, not a mean)
 *   tau = the element of rank `rank` among all M values e: an exact order statistic, no interpolation, selected over the bit
 *   patterns with integer counters, so the same bits whatever the order of the patches.  Then, all in integers:
 *       a_p = (e_p <= tau)
 *       b_p = (#{q in the 3x3 neighbourhood of p inside p's own patch, p included: a_q} >= smooth_min)
 *       c_p = a_p | b_p,    D_n = (sum_{p in patch n} c_p >= patch_min)
 *       inner(p): row and column both in [P/4, P/4 + P/2) (integer division)
 *       w_p = c_p | (D_n & inner(p))
 *   mask_in [N,P,P] uint8 or NULL: when given, w = (mask_in != 0), no residual statistics are formed, rank / smooth_min /
 *   patch_min are ignored (and not validated), and tau_out and stats are written as zeros.
 *       loss = (1/CM) sum_p w_p sum_c |d_c|  (L1)   or   (1/CM) sum_p w_p sum_c d_c^2  (L2)     (divisor C M, not the inliers)
 *       mse  = (1/CM) sum_p sum_c d_c^2      (without the mask, whichever the kind)
 *       g = (float)((double)grad_scale / (C M))
 *       d_x = (w_p g) sign(d_c)  (L1, sign(0) = 0)   or   (w_p 2g) d_c  (L2, one rounded float product); y gets no gradient
 * Outputs, each may be NULL = skipped: loss_out, mse_out, tau_out device float[1] (grad_scale does not apply to them);
 *   mask_out [N,P,P] uint8, strictly 0 or 1; stats device int64[3] = (sum a, sum c, sum w); d_x [N,P,P,C], every element written.
 *   loss_out and mse_out are double sums in a fixed order with one final float rounding; tau_out, mask_out and stats come from
 *   integer counters: every output holds the same bits from call to call, and tau_out / stats also under any permutation of the
 *   patches (mask_out is permuted with them).  No float atomic is issued.  mask_out may be the same buffer as mask_in (every
 *   byte is read before it is written, by the same thread); no other buffers may overlap.
 * Non-finite inputs: the call returns, nothing is read or written outside the stated extents and mask_out stays 0 / 1; a NaN
 *   residual orders above +inf; values are otherwise unspecified.  A residual e_p that is a float32 denormal is not part of the
 *   contract (its place in the order may differ from a host's).
 * scratch: voxe_robust_scratch_bytes(N, P, C) bytes of device memory (0 for shapes the call refuses), always required: NULL x,
 *   y or scratch is VOXE_ERR_NULL_POINTER, a short one VOXE_ERR_WORKSPACE.  All validation precedes any device work.  All
 *   outputs NULL: VOXE_OK, nothing is launched.  Work is enqueued on `stream`; no allocation, no host synchronisation.          */
size_t voxe_robust_scratch_bytes(int32_t N, int32_t P, int32_t C);
int voxe_robust_fwd_bwd(const float* x, const float* y, int32_t N, int32_t P, int32_t C, int32_t kind,
                        int64_t rank, int32_t smooth_min, int32_t patch_min,
                        const uint8_t* mask_in     /* [N,P,P] or NULL */,
                        float grad_scale,
                        float* loss_out, float* mse_out, float* tau_out, uint8_t* mask_out, int64_t* stats, float* d_x,
                        void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SSIM of two image batches, value and gradient in one call (additive; still ABI v13), DESIGN.md section 4.18 "SSIM".  No
 * voxe_cpu_ twin; the float64 restatement is tests/ssim_ref.py.
 *   x, y: device float, channel-last [N,H,W,C], C in 1..4 (a render's colour viewed as patches or as an image).  Wang et al.
 *   2004: an 11 x 11 Gaussian window of sigma 1.5 -- g1[i] ~ exp(-(i-5)^2 / 4.5), normalised to sum 1 in double, then rounded to
 *   float; the 2-D window is the outer product -- over VALID windows only: an H x W image gives an (H-10) x (W-10) map, there
 *   is no padding of any kind.  With L = data_range, C1 = (0.01 L)^2, C2 = (0.03 L)^2 and, per window, channel and image, the
 *   window sums m_x = sum g x, m_y, m_xx = sum g x^2, m_yy, m_xy:
 *       vx = m_xx - m_x^2,  vy = m_yy - m_y^2,  vxy = m_xy - m_x m_y
 *       A1 = 2 m_x m_y + C1,  A2 = 2 vxy + C2,  B1 = m_x^2 + m_y^2 + C1,  B2 = vx + vy + C2
 *       S = A1 A2 / (B1 B2),   ssim = mean of S over all M = N C (H-10) (W-10) windows
 *   Gradient w.r.t. x only (y is a target and receives none):
 *       Q = dS/dm_xx = -S / B2,   R = dS/dm_xy = 2 A1 / (B1 B2)
 *       P = dS/dm_x  = 2 m_y (A2 - A1) / (B1 B2) + 2 m_x S (1/B2 - 1/B1)
 *       dssim/dx_p = (1/M) sum_{windows q containing p} g(p - q) [P_q + 2 x_p Q_q + y_p R_q]
 *   Outputs (each may be NULL): mean_out  device float[1], the mean over all windows (grad_scale does not apply to it);
 *                               per_image device [N], the mean over the windows of one image;
 *                               ssim_map  device [N,H-10,W-10,C], S;
 *                               d_x       device [N,H,W,C] = grad_scale * dssim/dx, written to every element, or added to the
 *                                         buffer when accumulate != 0.  NULL skips the gradient.
 *   The window sums, S, P, Q, R and the transposed passes of the gradient are double; the images and the three maps the
 *   gradient passes through `scratch` are float.  No atomics: every output has the same bits on every run.  `scratch`
 *   (voxe_ssim_scratch_bytes(N, H, W, C, d_x != NULL); 0 for shapes the call refuses) carries the per-block partial sums and
 *   the maps; its contents mean nothing between calls.  All four outputs NULL: VOXE_OK with no launch.  Caller's stream, no
 *   host synchronisation, no allocation.  Validation, before any device work: x, y or scratch NULL -> VOXE_ERR_NULL_POINTER;
 *   N < 1, H < 11, W < 11, C outside 1..4, data_range <= 0 (or more than 2^31-1 16 x 16 tiles) -> VOXE_ERR_BAD_SHAPE; scratch too
 *   small -> VOXE_ERR_WORKSPACE.                                                                                           */
size_t voxe_ssim_scratch_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t with_grad);
int voxe_ssim_fwd_bwd(const float* x, const float* y, int32_t N, int32_t H, int32_t W, int32_t C,
                      float data_range, float grad_scale,
                      float* mean_out   /* device float[1] or NULL */,
                      float* per_image  /* device [N] or NULL */,
                      float* ssim_map   /* device [N,H-10,W-10,C] or NULL */,
                      float* d_x        /* device [N,H,W,C] or NULL: skip the gradient */,
                      int32_t accumulate,
                      void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ray and camera-pose gradients (additive; still ABI v13), DESIGN.md section 4.13 "Ray gradients".  No voxe_cpu_ twin; the
 * float64 restatement is tests/ray_grad_ref.py.
 *
 * voxe_render_bwd_rays: the gradient of a render with respect to rays_o / rays_d, what the reference chain (sample ->
 *   grid_sample -> SH -> accumulate) delivers to the rays under autograd.  The samples z_k, the inside test, sigma_k, delta_k =
 *   dl_k |d| (last dl = 1e10) and w_k = T_k alpha_k are those of voxe_render_fwd for the same rays, cfg and jitter / (seed,
 *   rng_offset).  Upstream gradients d_colour [R,3], d_depth [R], d_acc [R]; each may be NULL (= 0).  Per ray:
 *       q_k   = d_colour . rad_k + d_depth z_k + d_acc - (white_bkgd ? sum_c d_colour_c : 0)
 *       E_k   = q_k (T_k - w_k) - sum_{i>k} w_i q_i
 *       dL/dsigma_k = delta_k E_k,    dL/ddelta_k = sigma_k E_k
 *       dL/dp_k = dL/dsigma_k post'(v_k) grad v(p_k) + w_k sum_c d_colour_c rad_kc (1 - rad_kc) sum_j B_j(v^) grad f_cj(p_k)
 *       d_rays_o = sum_k dL/dp_k
 *       d_rays_d = sum_k z_k dL/dp_k + (sum_k dL/ddelta_k dl_k) d/|d| + Jn^T (dB/dv^)^T m
 *       m_j = sum_k w_k sum_c d_colour_c rad_kc (1 - rad_kc) f_cj(p_k),   Jn = (I - v^ v^T) / |d|,   v^ = d / |d|
 *   rad_kc = sigmoid(sum_j B_j f_cj); grad of a trilinear interpolant is its slope inside the cell floor(u) the forward used,
 *   corners outside the grid counting as 0 for the slope too, in world units (N_a norm_scale_a / 2 per axis): the conventions
 *   of voxe_render_normals, applied to the pre-activated, scaled density corners and to every feature channel.  With
 *   render_diffuse or sh_degree 0 only B_0 exists and the last term of d_rays_d vanishes.  Samples that fail the strict AABB
 *   test contribute nothing; post' follows voxe_render_bwd.
 *   THE SAMPLE DEPTHS z_k ARE CONSTANTS.  Without aabb_clip that is exactly the reference's autograd (z depends on near / far /
 *   jitter only).  With aabb_clip the per-ray bounds get a stop-gradient: the reference would differentiate the slab test,
 *   this call does not (as voxe_distortion_fwd_bwd: no gradient flows to z).
 *   cfg: term_eps, deterministic, reuse_packed_grid, ray_state_valid and dispatch are ignored; image_width / image_height only
 *   choose the ray -> thread mapping (a ray's gradient depends on that ray and cfg only).  VOXE_FEAT_ATTN grids:
 *   VOXE_ERR_UNSUPPORTED.  Validation, the limits on R and the voxel count and the error codes are those of voxe_render_normals,
 *   plus F == 3 (sh_degree + 1)^2 (VOXE_ERR_BAD_SHAPE) and a non-NULL grid->features.  R == 0 or both outputs NULL: VOXE_OK with
 *   no launch.  accumulate != 0: += into the outputs, else overwrite.
 *   The RAW API tensors (grid->densities, grid->features) are read: no workspace; no forward record or voxe_recon_prefetch hint
 *   is read or dropped.  Caller's stream, no host synchronisation, no allocation.  No atomics: a ray's 6 outputs are written by
 *   one lane, so the result is bit-reproducible for a fixed lanes split.
 *   voxe_render_bwd_rays_debug_lanes: test aid, as voxe_distortion_debug_lanes (0 | 1 | 2 | 4 | 8 lanes per ray for the calling
 *   thread's later calls; anything else: VOXE_ERR_BAD_SHAPE).
 *
 * voxe_cast_rays_bwd: the chain rule of voxe_cast_rays / voxe_cast_rays_indexed into the poses [K,3,4] and the focal length:
 *       d_trans = sum d_rays_o,   d_rot[a][b] = sum d_rays_d[a] dir_cam[b],   d_focal = sum d_rays_d . (R d dir_cam / d focal)
 *   over the rays of each camera (dir_cam = ((x - W/2) / focal, -(y - H/2) / focal, -1)).  flat_index NULL: ray i is pixel i of
 *   K whole images (B must be K * H * W).  Either d_rays_* may be NULL (= 0).  The sums are carried in double, 13 per camera in
 *   `scratch` (voxe_cast_rays_bwd_scratch_bytes(K); too small: VOXE_ERR_WORKSPACE), then cast once into d_poses / d_focal
 *   (device float[1] or NULL), added to them when accumulate != 0.  Cameras with no ray get an exact 0.  The rays of a wave that
 *   share a camera are reduced in the wave before one lane adds; where lanes of different waves meet on a camera the adds are
 *   double atomics, so the result is NOT promised bit-reproducible from run to run.                                          */
int voxe_render_bwd_rays(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                         const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                         const float* d_colour, const float* d_depth, const float* d_acc,
                         float* d_rays_o /* [R,3] or NULL */, float* d_rays_d /* [R,3] or NULL */,
                         int32_t accumulate, void* stream);
int voxe_render_bwd_rays_debug_lanes(int32_t lanes);

size_t voxe_cast_rays_bwd_scratch_bytes(int32_t K);
int voxe_cast_rays_bwd(int32_t H, int32_t W, float focal, const float* poses /* [K,3,4] device */, int32_t K,
                       const int64_t* flat_index /* [B] device or NULL: ray i is pixel i of K whole images */, int64_t B,
                       const float* d_rays_o, const float* d_rays_d /* [B,3], either may be NULL */,
                       float* d_poses /* [K,3,4] */, float* d_focal /* device float[1] or NULL */,
                       int32_t accumulate, void* scratch, size_t scratch_bytes, void* stream);

/* ---- rigid transform, re-gridding and composition of voxel grids (not in the reference) ----------------------
 * An added symbol is backward compatible: VOXE_ABI_VERSION stays 13.  No voxe_cpu_ twin; the float64 restatement is
 * tests/transform_ref.py.
 *
 * voxe_grid_resample: every voxel of a DESTINATION grid [X2,Y2,Z2] samples a SOURCE grid [X,Y,Z] trilinearly at
 *       u = A i + b        i = the destination voxel's integer index, u = continuous source index (voxel centres at integers),
 *   evaluated in float32 without FMA as u_a = ((A_a0 i_x + A_a1 i_y) + A_a2 i_z) + b_a.  For the scene-frame map
 *   p' = s R p + t (R orthogonal, det +-1, s > 0), source low corner lo_s and voxel edges v_s, destination lo_d and v_d:
 *       A = diag(1/v_s) (R^T / s) diag(v_d),     b = diag(1/v_s) ((R^T / s)(lo_d + v_d/2 - t) - lo_s) - 1/2
 *   (computed by the caller in float64, cast to float32).  i0 = floor(u), f = u - i0, per-axis weights (1 - f, f), corner
 *   weights t_c = (wx wy) wz summed corners ascending (x in bit 0) as in the renderer's gather.
 *   Density: each corner is read through density_pre_act (IDENTITY | ABS, no density scale); the interpolated pre-activated
 *   value is stored as the new RAW density (ABS is idempotent on it).  A corner outside the source lattice contributes
 *   density_fill to the density and 0 to every feature channel; a voxel whose 8 corners are all outside gets exactly
 *   (density_fill, 0...) and loads nothing.
 *   Features: sh_degree 0..3 -- C must be 3 (deg+1)^2, laid out [colour channel][coefficient]; per channel and band l the
 *   interpolated coefficients are rotated, c'_l = M_l c_l, M_l the row-major (2l+1)^2 block of sh_rot at offset 0 / 1 / 10 / 35,
 *   defined by b_l(R^T v)^T = b_l(v)^T M_l for every unit v in the renderer's own basis (band 0 is the identity and is not
 *   multiplied).  sh_degree -1 -- C plain channels (1..64), no rotation (the attention grid).
 *   Modes: VOXE_RESAMPLE_REPLACE writes every destination voxel.  VOXE_RESAMPLE_UNION (CSG union of the two pre-activation
 *   fields, in place on the destination): a sample is VALID iff every corner with non-zero weight lies in the source lattice; a
 *   valid sample whose density is strictly greater than pre_act(destination raw density) replaces the destination's density and
 *   all its features; every other destination voxel is not written.  Source and destination must not alias.
 *   taken (uint8 [X2,Y2,Z2] or NULL): UNION -- 1 where the source replaced the destination; REPLACE -- 1 where at least one
 *   corner with non-zero weight lies in the lattice.
 *   Either the density pair or the feature pair may be NULL in REPLACE (both NULL: VOXE_ERR_NULL_POINTER, as is one half of a
 *   pair); UNION needs the density pair.  Shapes: all dims > 0, both voxel counts times (C + 1) < 2^31, X*Y, Y*Z, Z < 2^24 on
 *   either grid, else VOXE_ERR_BAD_SHAPE; an unknown mode / pre-activation / sh_degree: VOXE_ERR_UNSUPPORTED.
 *   Uniform scale is geometric only: raw values are not compensated, so the optical depth through the object scales by s.
 *   No gradient is defined.  No workspace, forward record or voxe_recon_prefetch hint is touched; caller's stream, no host
 *   synchronisation, no allocation.                                                                                         */
typedef enum VoxeResampleMode {
  VOXE_RESAMPLE_REPLACE = 0,
  VOXE_RESAMPLE_UNION = 1
} VoxeResampleMode;

typedef struct VoxeResample {
  float A[9];               /* row-major 3x3                                                       */
  float b[3];
  float sh_rot[84];         /* M_0 (1) | M_1 (9) | M_2 (25) | M_3 (49), each row-major             */
  int32_t sh_degree;        /* -1: plain channels; 0..3: SH, C = 3 (deg+1)^2                       */
  int32_t density_pre_act;  /* VoxeAct: IDENTITY | ABS                                             */
  int32_t mode;             /* VoxeResampleMode                                                    */
  float density_fill;       /* what a corner outside the source lattice adds to the density        */
} VoxeResample;

int voxe_grid_resample(const float* src_densities /* [X,Y,Z,1] or NULL */, const float* src_features /* [X,Y,Z,C] or NULL */,
                       int32_t X, int32_t Y, int32_t Z, int32_t C,
                       float* dst_densities /* [X2,Y2,Z2,1] or NULL */, float* dst_features /* [X2,Y2,Z2,C] or NULL */,
                       int32_t X2, int32_t Y2, int32_t Z2,
                       const VoxeResample* xf, uint8_t* taken /* [X2,Y2,Z2] or NULL */, void* stream);

/* ---- real-capture cameras: intrinsics and lens distortion (not in the reference) ------------------------------
 * An added symbol is backward compatible: VOXE_ABI_VERSION stays 13.  No voxe_cpu_ twin; the float64 restatement and the
 * float32 restatement of the kernel's iteration are tests/camera_ref.py.  voxe_cast_rays, voxe_cast_rays_indexed,
 * voxe_cast_rays_bwd, VoxeReconStep and voxe_recon_step / voxe_recon_prefetch keep the (H, W, focal) camera.
 *
 * VoxeCamera: one pinhole camera with the OpenCV radial / tangential lens model, shared by the K poses of a call.  Pixel
 * (px, py) has its centre at (px + 0.5, py + 0.5); fx, fy, cx, cy are in pixels.
 *
 * voxe_cast_rays_camera: per ray, in float32 without FMA,
 *       x = px + 0.5, y = py + 0.5, xd = (x - cx) / fx, yd = (y - cy) / fy                      (yd is image-down)
 *       (xu, yu) solves D(xu, yu) = (xd, yd),  r2 = xu^2 + yu^2,  rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),
 *         D_x = xu rad + 2 p1 xu yu + p2 (r2 + 2 xu^2),    D_y = yu rad + p1 (r2 + 2 yu^2) + 2 p2 xu yu
 *       dir_cam = (xu, -yu, -1),  rays_d = R dir_cam,  rays_o = t.
 *   The solve starts at (xd, yd) and takes 6 Newton steps with the analytic 2x2 Jacobian on every lane: no early exit, no
 *   data-dependent branch, so a ray's bits depend on that ray only (not on B or its place in the batch).  When all five
 *   coefficients are exactly 0, (xu, yu) = (xd, yd) and no iteration runs; with also fx == fy == focal, cx == W * 0.5f and
 *   cy == H * 0.5f the rays equal those of voxe_cast_rays_indexed bit for bit.  The kernel does not detect a lens model that is
 *   not invertible over the image: that check is the host's (PinholeCamera.validate()).
 *   flat_index (device int64 [B], (camera * H + y) * W + x) picks pixels and is decoded and clamped as voxe_cast_rays_indexed
 *   does; NULL: ray i is pixel i of K whole images and B must be K * H * W.  B == 0: VOXE_OK, no launch.
 *   H, W, K <= 0, B < 0, fx or fy not finite and > 0, cx, cy or a coefficient not finite: VOXE_ERR_BAD_SHAPE.
 *
 * voxe_cast_rays_camera_bwd: the chain rule of voxe_cast_rays_camera by the implicit-function theorem at the forward's
 *   solution (the iterations are not differentiated).  With g = R^T d_rays_d, (g_xu, g_yu) = (g_0, -g_1),
 *   (g_xd, g_yd) = J^-T (g_xu, g_yu), J = dD / d(xu, yu):
 *       d_fx = sum -g_xd xd / fx,  d_cx = sum -g_xd / fx,  d_fy = sum -g_yd yd / fy,  d_cy = sum -g_yd / fy,
 *       d_kj = sum -(g_xd, g_yd) . dD/dkj,   dD/dk1 = r2 (xu, yu), dD/dk2 = r2^2 (xu, yu), dD/dk3 = r2^3 (xu, yu),
 *       dD/dp1 = (2 xu yu, r2 + 2 yu^2), dD/dp2 = (r2 + 2 xu^2, 2 xu yu),
 *   and d_poses as voxe_cast_rays_bwd with this dir_cam.  d_intrinsics: device float[4] (fx fy cx cy); d_distortion: device
 *   float[5] (k1 k2 p1 p2 k3); each of the three outputs may be NULL (not computed).  Either d_rays_* may be NULL (= 0).  The
 *   sums are carried in double, 12 per camera plus 9 global ones in `scratch` (voxe_cast_rays_camera_bwd_scratch_bytes(K); NULL
 *   or too small: VOXE_ERR_WORKSPACE), then cast once into the outputs, added to them when accumulate != 0.  Cameras with no ray
 *   get an exact 0.  B == 0 or all three outputs NULL: VOXE_OK with no launch (B == 0 and accumulate == 0: the outputs are set
 *   to 0).  The 9 global sums are reduced inside the wave before one lane adds, the per-camera sums as voxe_cast_rays_bwd; the
 *   adds are double atomics, so the result is NOT promised bit-reproducible from run to run.  Validation and error codes are
 *   those of voxe_cast_rays_camera and voxe_cast_rays_bwd.  Caller's stream, no host synchronisation, no allocation.        */
typedef struct VoxeCamera {
  int32_t H, W;
  float fx, fy, cx, cy;          /* pixels; pixel (px,py) has centre (px+0.5, py+0.5) */
  float k1, k2, p1, p2, k3;      /* OpenCV radial / tangential coefficients */
} VoxeCamera;

int voxe_cast_rays_camera(const VoxeCamera* cam, const float* poses /* device [K,3,4] */, int32_t K,
                          const int64_t* flat_index /* device [B] or NULL: ray i = pixel i of K whole images */,
                          int64_t B, float* rays_o, float* rays_d, void* stream);
size_t voxe_cast_rays_camera_bwd_scratch_bytes(int32_t K);
int voxe_cast_rays_camera_bwd(const VoxeCamera* cam, const float* poses, int32_t K, const int64_t* flat_index, int64_t B,
                              const float* d_rays_o, const float* d_rays_d /* [B,3], either may be NULL */,
                              float* d_poses /* [K,3,4] or NULL */, float* d_intrinsics /* device float[4] fx fy cx cy, or NULL */,
                              float* d_distortion /* device float[5] k1 k2 p1 p2 k3, or NULL */,
                              int32_t accumulate, void* scratch, size_t scratch_bytes, void* stream);

/* ---- learned environment-map background behind the grid (not in the reference) -----------------------------------
 * An added symbol is backward compatible: VOXE_ABI_VERSION stays 13.  No voxe_cpu_ twin; the float64 restatement is
 * tests/background_ref.py.  No render entry point changes: the background is composited behind a finished render with the
 * ray's leftover transmittance 1 - acc, and its d_acc goes into voxe_render_bwd / voxe_render_bwd_rays as their upstream d_acc.
 *
 * VoxeEnvMap: texels [height, width, 3], float32, contiguous, LOGITS; height >= 2, width >= 2.  For a ray direction
 * d = (dx, dy, dz), which need not be unit length:
 *       r = sqrt(dx^2 + dy^2),  phi = atan2(dy, dx) (0 where r == 0),  theta = atan2(r, dz)
 *       u = (phi / 2 pi + 0.5) width - 0.5,              v = (theta / pi) height - 0.5
 *       x0 = floor(u), fx = u - x0, columns x0 mod width, (x0 + 1) mod width               (the longitude wraps)
 *       y0 = floor(v), fy = v - y0, rows clamp(y0, 0, height - 1), clamp(y0 + 1, 0, height - 1)     (the poles clamp)
 *       t_c = bilinear(E[..., c]),  b_c = sigmoid(t_c),  colour_out_c = colour_in_c + (1 - acc) b_c
 *   A direction with a non-finite component, or of zero length, has b = 0 and no gradient anywhere.  The angles and (u, v) are
 *   evaluated in double, everything else in float.
 *
 * voxe_background_fwd: colour_out [R,3] from colour_in [R,3], acc [R] and rays_d [R,3]; colour_out may be colour_in.
 *
 * voxe_background_bwd: with g = d_colour_out [R,3] (d_colour_in = g needs no call):
 *       d_acc = - sum_c g_c b_c
 *       s_c = (1 - acc) g_c b_c (1 - b_c),   d_texels[tap] += w_tap s_c for the four taps (taps that coincide through the clamp
 *         receive both weights)
 *       d_rays_d = d_u du/dd + d_v dv/dd,  d_u = (width / 2 pi) sum_c s_c ((1 - fy)(E01 - E00) + fy (E11 - E10)),
 *         d_v = (height / pi) sum_c s_c ((1 - fx)(E10 - E00) + fx (E11 - E01)),
 *         dphi/dd = (-dy, dx, 0) / r^2,  dtheta/dd = (dx dz / r, dy dz / r, -r) / |d|^2;  exactly 0 where r == 0
 *   Each of the three outputs may be NULL (not computed).  accumulate == 0 overwrites all of them (d_texels is zeroed first:
 *   texels no ray touches hold an exact 0), accumulate != 0 adds.  A ray whose s is all zero (acc == 1, g == 0) issues no
 *   atomic.  d_texels goes through float atomics, so it can differ in the last bits from run to run; d_acc and d_rays_d are
 *   written by one lane each.  Lanes of a wave that are neighbours and fall into the same cell (x0, y0) are summed in the wave
 *   before the first of them adds (the run merge); voxe_background_debug_merge is a test aid that pins this for the calling
 *   thread's later calls: 0 = the shipped choice, 1 = merge, 2 = one atomic per lane and tap (anything else: VOXE_ERR_BAD_SHAPE).
 *
 * Validation, before any device work: env or env->texels NULL: VOXE_ERR_NULL_POINTER; height < 2, width < 2, R < 0 or
 * R >= 2^31: VOXE_ERR_BAD_SHAPE; R == 0: VOXE_OK and nothing is done (no output is touched); then a NULL rays_d, acc, colour_in,
 * colour_out or d_colour_out: VOXE_ERR_NULL_POINTER.  All three outputs NULL: VOXE_OK with no launch.  Caller's stream, no host
 * synchronisation, no allocation, no workspace.                                                                             */
typedef struct VoxeEnvMap {
  const float* texels;      /* device [height, width, 3], logits */
  int32_t height, width;
} VoxeEnvMap;

int voxe_background_fwd(const VoxeEnvMap* env, const float* rays_d, int64_t R,
                        const float* colour_in, const float* acc, float* colour_out, void* stream);
int voxe_background_bwd(const VoxeEnvMap* env, const float* rays_d, int64_t R, const float* acc,
                        const float* d_colour_out, float* d_acc /* [R] or NULL */,
                        float* d_texels /* [height, width, 3] or NULL */, float* d_rays_d /* [R,3] or NULL */,
                        int32_t accumulate, void* stream);
int voxe_background_debug_merge(int32_t mode);

/* ---- mesh import: a triangle mesh into a signed-distance band on a voxel lattice (not in the reference) -----------
 * An added symbol is backward compatible: VOXE_ABI_VERSION stays 13.  No voxe_cpu_ twin; the numpy restatement (integer parity,
 * float32 distance operation for operation, float64 for bounds) is tests/voxelize_ref.py.
 *
 * Lattice: X x Y x Z voxels, centre i at lo + (i + 0.5) (hi - lo) / N per axis (the mesh export's convention), aabb_lo / aabb_hi
 * HOST float[3].  vertices [V,3] float32 world space, faces [T,3] int32, vertex_colours [V,3] float32 or NULL, all on the device.
 * h > 0 is the band half-width in world units.  Outputs (device, caller-owned; every one but sdf may be NULL):
 *   sdf     [X,Y,Z]   float32  signed distance of the voxel centre to the mesh, negative inside, clamped to +-h
 *   nearest [X,Y,Z]   int32    the triangle that realises it (the lowest id among equal distances), -1 outside the band
 *   colours [X,Y,Z,3] float32  vertex colours interpolated at the closest point of that triangle; 0 outside the band or
 *                              without vertex_colours
 *   inside  [X,Y,Z]   uint8    1 inside
 *   stats   int64[4]           columns (y, z) with an odd number of crossings (an open mesh); triangles skipped as malformed (an
 *                              index outside [0, V), a non-finite vertex, a vertex outside the fixed-point range); voxels in the
 *                              band; work items
 * Distance: exact closest point of every triangle by Voronoi regions on the world-space vertices (taken in ascending vertex id,
 * so the result does not depend on how a face lists them), float32 with every operation rounded on its own; the voxel keeps
 * the minimum of (bits(d^2) << 32 | triangle id) over the triangles with d^2 <= h^2 through one 64-bit integer atomicMin, so the
 * result is the same bits whatever the order of the faces.  Sign: parity of the crossings of the ray through the column's centre
 * along +x, in integers: with u = (p - lo) / step - 0.5 (float32) a vertex is snapped to q = rint(256 u); a vertex is admissible
 * when |u| < 1024 on every axis.  A triangle covers column (y, z) when the centre passes its three edge functions (int64) under a
 * top-left rule -- a centre on an edge belongs to the side the point (y + eps, z + eps^2) falls on, so an edge or vertex shared
 * by several triangles counts exactly as a ray next to it would -- and the crossing is charged to the first voxel whose centre
 * has x >= the plane's x over the centre (an exact ceiling division).  A voxel is inside when the number of crossings charged
 * to voxels 0..i is odd.  Triangles whose snapped vertices are collinear take no part in either pass (they are not malformed).
 *
 * Scratch: voxe_voxelize_scratch_bytes(X, Y, Z, T) = the key grid (8 B per voxel), the counter grid (4 B per voxel and per
 * column, one plane behind the grid for the crossings there), and 12 B per triangle + 8 B for the work list.  The list is
 * bounded by T without a read-back because no work item is stored: the list is the exclusive prefix of the items per triangle
 * (one deterministic one-block scan), and a wave finds its item's triangle by bisection and rebuilds the item's cells from the
 * triangle's vertices.  0 for dims the call refuses.
 *
 * Validation, in this order and before any device work: a NULL sdf, aabb_lo or aabb_hi, NULL vertices with V > 0 or NULL faces
 * with T > 0: VOXE_ERR_NULL_POINTER; X, Y or Z outside 1..VOXE_VOXELIZE_MAX_DIM, V < 0 or >= 2^31, T < 0 or >= 2^31, an empty or
 * non-finite aabb, h <= 0 or not finite: VOXE_ERR_BAD_SHAPE; scratch NULL or short: VOXE_ERR_WORKSPACE.  T == 0: VOXE_OK with
 * sdf = +h, nearest = -1, colours = 0, inside = 0, stats = 0.  Caller's stream, no host synchronisation, no allocation; no
 * render workspace, forward record or prefetch hint is touched.                                                              */
#define VOXE_VOXELIZE_MAX_DIM 1024
size_t voxe_voxelize_scratch_bytes(int32_t X, int32_t Y, int32_t Z, int64_t T);
int voxe_voxelize_mesh(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const float* vertex_colours,
                       int32_t X, int32_t Y, int32_t Z, const float* aabb_lo, const float* aabb_hi, float h,
                       float* sdf, int32_t* nearest, float* colours, uint8_t* inside, int64_t* stats,
                       void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-voxel Fisher information: how well a set of rays pins down each voxel's raw density.
 * An added symbol is backward compatible: VOXE_ABI_VERSION stays 13.  No voxe_cpu_ twin; the float64 restatement is
 * tests/fisher_ref.py.
 *
 * voxe_fisher_rays: the diagonal of J^T J of the rendered colours with respect to the raw densities, and its contraction with
 *   a per-voxel variance.  The samples z_k, the inside test, sigma_k = post(v_k), delta_k = dl_k |d| (last dl = 1e10), T_k,
 *   w_k = T_k alpha_k and rad_{k,ch} are those of voxe_render_fwd for the same rays, cfg and jitter / (seed, rng_offset) AT
 *   term_eps = 0 (the whole ray is marched whatever cfg->term_eps says: a forward that cuts its march short has fewer samples):
 *   SH evaluation on the ray direction, render_diffuse and every sh_degree 0 - 3 included.  With
 *   q_{k,ch} = rad_{k,ch} - (white_bkgd ? 1 : 0), per ray r and colour channel ch:
 *       E_{k,ch}    = q_{k,ch} (T_k - w_k) - sum_{i>k} w_i q_{i,ch}
 *       J_{r,ch}[c] = pre'(scale raw_c) scale * sum_k delta_k E_{k,ch} post'(v_k) t_c(k)
 *       fisher[c]  += sum_ch J_{r,ch}[c]^2                          once per ray
 *       ray_var[r]  = sum_c P[c] sum_ch J_{r,ch}[c]^2               P = voxel_var, 1 when NULL
 *   t_c = (wx * wy) * wz is the gather weight of corner c in sample k's cell, corners inside the grid only.  J_{r,ch} is the
 *   d_densities of voxe_render_bwd for d_colour = e_ch on ray r alone, d_depth = d_acc = 0: the derivative conventions are
 *   voxe_render_bwd's (post', pre' = sign for abs with sign(0) = 0, no suffix at the last sample and where 1 - alpha_k == 0).
 *   The square sits INSIDE the sum over rays: no number of backward passes over several rays yields it.
 *   Only white_bkgd is a background here; a learned environment map is ignored.  The features get no Fisher term.
 *   fisher [X,Y,Z] ACCUMULATES (zero it before the first call) through float atomics: the order of the additions, and so the
 *   last bits, may differ from run to run; a voxel no sample weighs keeps an exact 0.  ray_var [R] is OVERWRITTEN, summed per ray
 *   in double by the ray's one lane without atomics: the same bits on every run, whatever the other rays of the launch, and
 *   exactly 0 for a ray that misses the grid.  voxel_var is read only when ray_var is given.
 *   cfg: term_eps (see above; voxe_render_bwd_rays' rule), deterministic, reuse_packed_grid, ray_state_valid and dispatch are
 *   ignored; image_width / image_height only choose the ray -> thread mapping.  VOXE_FEAT_ATTN grids: VOXE_ERR_UNSUPPORTED.
 *   Validation, the limits on R and the voxel count and the error codes are those of voxe_render_normals, plus
 *   F == 3 (sh_degree + 1)^2 (VOXE_ERR_BAD_SHAPE) and a non-NULL grid->features (VOXE_ERR_NULL_POINTER).  R == 0 or both outputs
 *   NULL: VOXE_OK with no launch.
 *   The RAW API tensors (grid->densities, grid->features) are read: no workspace; no forward record or voxe_recon_prefetch hint
 *   is read or dropped.  Caller's stream, no host synchronisation, no allocation.                                            */
int voxe_fisher_rays(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                     const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                     float*       fisher     /* [X,Y,Z] or NULL: ACCUMULATES H (caller zeroes first) */,
                     const float* voxel_var  /* [X,Y,Z] or NULL: P, read only for ray_var; NULL = 1 */,
                     float*       ray_var    /* [R] or NULL: sum_c P[c] sum_ch J_{r,ch}[c]^2, overwritten */,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * CPU twin == the oracle (oracle/voxe_cpu.c). Same semantics, HOST pointers, no stream/workspace.
 * TEST INFRASTRUCTURE ONLY: never linked into libvoxe_hip.so, never called by the product path.
 * ---------------------------------------------------------------------------------------------- */
int voxe_cpu_cast_rays(int32_t H, int32_t W, float focal, const float* rot, const float* trans,
                       float* rays_o, float* rays_d);
int voxe_cpu_cast_rays_indexed(int32_t H, int32_t W, float focal, const float* poses, int32_t K,
                               const int64_t* flat_index, int64_t B, float* rays_o, float* rays_d);
int voxe_cpu_random_subset(int64_t n, int64_t count, uint64_t seed, uint64_t rng_offset, int64_t* out);
int voxe_cpu_render_fwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                        const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                        float* colour, float* depth, float* acc, float* disparity);
int voxe_cpu_render_bwd(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                        const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                        const float* d_colour, const float* d_depth, const float* d_acc,
                        float* d_densities, float* d_features, int32_t accumulate);
int voxe_cpu_query_fwd(const VoxeGridDesc* grid, const float* points, int64_t N, float* out);
int voxe_cpu_query_bwd(const VoxeGridDesc* grid, const float* points, int64_t N, const float* d_out,
                       float* d_densities, float* d_features, int32_t accumulate);
int voxe_cpu_sample_probe(const VoxeGridDesc* grid, const VoxeRenderCfg* cfg,
                          const float* rays_o, const float* rays_d, int64_t R, const float* jitter,
                          int32_t* idx, uint8_t* inside, float* zvals, float* sigma, float* rad);
int voxe_cpu_dcl_fwd_bwd(const float* a, const float* b, int64_t n, float grad_scale,
                         float* loss_out, float* d_a, int32_t accumulate);
int voxe_cpu_density_diff_fwd_bwd(const float* a, const float* b, int64_t n, int32_t kind, float grad_scale,
                                  float* loss_out, float* d_a, int32_t accumulate);
int voxe_cpu_feature_correlation_fwd_bwd(const float* f, const float* r, int64_t nvox, int32_t F, float grad_scale,
                                         float* loss_out, float* d_f, int32_t accumulate);
int voxe_cpu_tv_fwd_bwd(const float* grid, int32_t X, int32_t Y, int32_t Z, int32_t C,
                        float grad_scale, float* loss_out, float* d_grid, int32_t accumulate);
int voxe_cpu_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                       int64_t n, float lr, float beta1, float beta2, float eps, int64_t step);
int voxe_cpu_upsample_trilinear(const float* src, int32_t X, int32_t Y, int32_t Z, int32_t C,
                                float* dst, int32_t X2, int32_t Y2, int32_t Z2);
int voxe_cpu_graph_build(const float* density_grid, const float* feature_grid,
                         int32_t X, int32_t Y, int32_t Z, int32_t F, float sigma, int32_t dilate_yz,
                         uint8_t* node_mask, int32_t* cap);
int voxe_cpu_graphcut(const uint8_t* node_mask, const int8_t* terminal, int32_t* cap,
                      int32_t X, int32_t Y, int32_t Z, uint8_t* segment, int64_t* flow);
int voxe_cpu_cc_largest_k(const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t k,
                          int32_t* labels, int32_t* num_components);
/* number of OpenMP threads the oracle will use (1 when built without OpenMP) */
int voxe_cpu_num_threads(void);
/* jitter value the HIP kernels draw for (seed, offset, ray, sample): lets tests replay the stream */
float voxe_cpu_jitter_uniform(uint64_t seed, uint64_t rng_offset, int64_t ray, int32_t sample);

#ifdef __cplusplus
}
#endif
#endif /* VOXE_H_ */
