// voxe_ray_march.hpp -- the density-only sample march ("The shared sample march").
//
// These calls walk the forward's exact samples over the RAW densities outside the renderer (their entries share the
// sampling_call_* prologue of voxe_api.hip; this is the one list of them):
//   voxe_render_normals, voxe_visibility_accumulate, voxe_lift_accumulate, voxe_render_bwd_rays, voxe_fisher_rays and the
//   three ray losses voxe_distortion_fwd_bwd, voxe_depth_fwd_bwd, voxe_orientation_fwd_bwd (voxe_ray_loss.hpp)
// What ties them to the renderer lives here, once:
//   depth step : sample k sits at z_k = DepthGen::z(k); its interval is dl_k = z_{k+1} - z_k, kInfinity for the last sample
//   cell       : p = o + d z, footprint(); a sample outside the box has sigma = 0 -> w = 0, T unchanged (the forward's rule)
//   density    : 8 raw loads, v = sum_q pre(raw_q) t_q with t_q = (wx * wy) * wz and the corners ascending (gather()'s
//                weights and FMA order), sigma = post(v)
//   opacity    : delta = dl |d|, e = fast_exp(-(sigma delta)), alpha = 1 - e, 1 - alpha
//   tail       : T *= 1 - alpha; the march ends when T is no longer > 0 (every later weight is 0, or NaN): attenuate()
// plus the split of a ray over G consecutive lanes (pixel rectangle of a block, lane j's block of the S samples, the
// transmittance in front of a block).  Everything is inlined and branch-free on the caller.
#pragma once

#include <climits>
#include <type_traits>

#include "voxe_render_common.hpp"

namespace voxe {

constexpr int kMarchThreads = 256;   // every kernel here: 4 waves per block (map_ray()'s block)

// ---- G lanes per ray ---------------------------------------------------------------------------------------------------
// Pixel rectangle of one block in image order: the 256 / G rays of a block as WX x WY sub-rectangles of WW x WH pixels, ray
// slots row-major inside a sub-rectangle.  The traversal order is part of the measured speed of each caller:
template <int G, int WX, int WY, int WW_>
struct GroupTile {
  static constexpr int kLanes = G;
  static constexpr int kRays = kMarchThreads / G;
  static constexpr int kSub = kRays / (WX * WY);   // ray slots of one sub-rectangle
  static constexpr int NX = WX;
  static constexpr int WW = WW_, WH = kSub / WW_;
  static constexpr int TW = WX * WW, TH = WY * WH;
};
// one rectangle per block, 16x16 / 16x8 / 8x8 / 8x4 pixels (normals)
template <int G>
using BlockRectTile = GroupTile<G, 1, 1, (G <= 2 ? 16 : 8)>;
// one rectangle per wave, the 4 waves as 2 x 2: G == 1 is map_ray()'s 16 x 16 tile of 8 x 8 sub-tiles; more lanes per ray
// shrink the rectangle, not its compactness (distortion, ray gradients)
template <int G>
using WaveRectTile = GroupTile<G, 2, 2, (G <= 2 ? 8 : 4)>;

// ray of this thread's group (false: padding of the launch); uniform over the G lanes of a ray
template <class Tile>
__device__ __forceinline__ bool group_ray(const DevCfg& c, long long& r) {
  const int slot = threadIdx.x / Tile::kLanes;   // ray slot of the block
  if (c.image_width > 0) {
    const int sub = slot / Tile::kSub, q = slot % Tile::kSub;
    const int W = c.image_width, H = c.image_height;
    const long long ntx = (W + Tile::TW - 1) / Tile::TW, per = ntx * ((H + Tile::TH - 1) / Tile::TH);
    const long long b = blockIdx.x, img = b / per, t = b - img * per;
    const int ty = (int)(t / ntx), tx = (int)(t - (long long)ty * ntx);
    const int px = tx * Tile::TW + (sub % Tile::NX) * Tile::WW + q % Tile::WW;
    const int py = ty * Tile::TH + (sub / Tile::NX) * Tile::WH + q / Tile::WW;
    r = (img * H + py) * (long long)W + px;
    return px < W && py < H && r < c.R;
  }
  r = (long long)blockIdx.x * Tile::kRays + slot;
  return r < c.R;
}

template <class Tile>
inline long long group_blocks(const DevCfg& c) {
  if (c.image_width > 0) {
    const long long nimg = c.R / ((long long)c.image_width * c.image_height);
    return nimg * ((c.image_width + Tile::TW - 1) / Tile::TW) * (long long)((c.image_height + Tile::TH - 1) / Tile::TH);
  }
  return (c.R + Tile::kRays - 1) / Tile::kRays;
}

// Lanes per ray of a launch of R rays: enough waves to fill 1024 SIMDs several times over -- R * G >= 2^20
// lane-rays where R allows it, at most 8 lanes per ray; `pinned` != 0 (a *_debug_lanes test aid) wins
inline int lanes_per_ray(long long R, int pinned) {
  if (pinned) return pinned;
  for (int G = 1; G < 8; G <<= 1)
    if (R * G >= (1ll << 20)) return G;
  return 8;
}

// the launch of a lanes-per-ray kernel: f(std::integral_constant<int, G>) for G in {1, 2, 4, 8}
template <class F>
inline void for_lanes(int G, F&& f) {
  switch (G) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

// lane j's contiguous block of the ray's S samples, cut to the samples inside the box (empty: k_lo > k_hi)
template <class RC>
__device__ __forceinline__ void lane_block(const DevCfg& c, const RC& rc, int j, int G, int& k_lo, int& k_hi) {
  const int len = (c.S + G - 1) / G;
  k_lo = max(rc.k_lo, j * len);
  k_hi = min(rc.k_hi, min(c.S, (j + 1) * len) - 1);
}

// transmittance in front of lane j's block: exclusive product of the block transmittances over the lanes before it
template <int G>
__device__ __forceinline__ float group_exclusive_product(float T, int j) {
  float P = T;
#pragma unroll
  for (int off = 1; off < G; off <<= 1) {
    const float t = __shfl_up(P, off, G);
    if (j >= off) P = P * t;
  }
  const float Ts = __shfl_up(P, 1, G);
  return j == 0 ? 1.0f : Ts;
}

// inclusive scan over the G lanes of a ray (sum; distortion, depth)
template <int G>
__device__ __forceinline__ double group_scan(double v, int j) {
#pragma unroll
  for (int off = 1; off < G; off <<= 1) {
    const double t = __shfl_up(v, off, G);
    if (j >= off) v += t;
  }
  return v;
}

// sum over the block, fixed order (thread 0 only holds it)
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double sm[kMarchThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < kMarchThreads / 64; ++i) s += sm[i];
  }
  return s;   // (thread 0 only)
}

// ---- one sample ------------------------------------------------------------------------------------------------------------
// The depth step: z of the current sample, z_next of the one behind it, `last`, and the interval dl.
struct DepthStep {
  float z, z_next;
  bool last;
  __device__ __forceinline__ float dl() const { return last ? kInfinity : (z_next - z); }
  // before sample k_lo; a ray's second march starts here as well (the jitter window restarts at k_lo)
  template <class RC>
  __device__ __forceinline__ void start(RC& rc, int k_lo) {
    rc.dg.kc = INT_MIN;
    z_next = rc.dg.z(k_lo);
  }
  template <class RC>
  __device__ __forceinline__ void advance(RC& rc, const DevCfg& c, int k) {
    z = z_next;
    last = (k == c.S - 1);
    if (!last) z_next = rc.dg.z(k + 1);
  }
};

// The cell of a sample: p = o + d z -> footprint -> inside test -> make_cell_fast.  Two calls, `if (!sc.locate(..)) <skip>;
// sc.make(g);`: make_cell_fast() holds a ballot, and only behind the caller's own branch does the cell stay out of the
// values the loop carries (one call that returns the test costs the callers 9 VGPRs).
struct SampleCell {
  Footprint fp;
  Cell cell;
  // false: outside the box (sigma = 0 -> w = 0, T unchanged; no footprint either)
  template <class RC>
  __device__ __forceinline__ bool locate(const DevGrid& g, const RC& rc, float z) {
    float p[3];
    rc.point(z, p);
    footprint(g, p, fp);
    return fp.inside;
  }
  __device__ __forceinline__ void make(const DevGrid& g) { make_cell_fast(g, fp, cell); }
};

// The tail of a sample: T *= 1 - alpha; false when the march ends here (T no longer > 0: every later w is 0, or NaN)
__device__ __forceinline__ bool attenuate(float& T, float om) {
  T = T * om;
  return T > 0.0f;
}

// The density sample in two halves (load_texels4() / interp_texels4() for the raw densities): a caller can issue loads of
// its own between them.  First the 8 corner indices (corner q = x + 2 y + 4 z) and raw loads, which go out together: one
// memory latency per sample instead of one per corner ...
struct DensityTaps {
  unsigned idx[8];
  float raw[8];
};
__device__ __forceinline__ void load_density(const DevGrid& g, const float* __restrict__ dens, const Cell& cell, DensityTaps& tp) {
  const CellAddr ad = cell_addr(g, cell);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    tp.idx[q] = ad.base + (q & 1) * ad.sx + ((q >> 1) & 1) * ad.sy + (q >> 2) * ad.sz;
    tp.raw[q] = dens[tp.idx[q]];
  }
}
// ... then the arithmetic: gather weights t, pre-activated corners cv, v, sigma (post' as well when DPOST) and the opacity,
// the forward's expressions
struct DensitySample {
  float t[8], cv[8];
  float sigma, dpost;
  float delta, e, alpha, om;   // om = 1 - alpha
};
template <bool DPOST>
__device__ __forceinline__ void eval_density(const DevGrid& g, const Cell& cell, const DensityTaps& tp, float dl, float dnorm,
                                             DensitySample& s) {
  float v = 0.0f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    s.t[q] = (cell.w[0][q & 1] * cell.w[1][(q >> 1) & 1]) * cell.w[2][q >> 2];
    s.cv[q] = pre_activate(g.pre_act, tp.raw[q], g.density_scale);
    v = fmaf(s.cv[q], s.t[q], v);
  }
  if constexpr (DPOST) post_activate_vg(g.post_act, v, s.sigma, s.dpost);
  else s.sigma = post_activate(g.post_act, v);
  s.delta = dl * dnorm;
  s.e = fast_exp(-(s.sigma * s.delta));
  s.alpha = 1.0f - s.e;
  s.om = 1.0f - s.alpha;
}

// ---- the march ---------------------------------------------------------------------------------------------------------------
// Samples k_lo .. k_hi of a ray front to back with the running transmittance T.  body(step, footprint, cell, T) handles one
// sample inside the box and returns its 1 - alpha.
// (Visibility, both distortion marches, the three of the depth loss and both of the orientation loss.  Normals, the ray gradients and lifting write their
// loops out over the same pieces; each says why.)
template <class RC, class Body>
__device__ __forceinline__ void march_block(const DevGrid& g, const DevCfg& c, RC& rc, int k_lo, int k_hi, float& T, Body&& body) {
  if (k_lo > k_hi) return;
  DepthStep st;
  st.start(rc, k_lo);
  for (int k = k_lo; k <= k_hi; ++k) {
    st.advance(rc, c, k);
    SampleCell sc;
    if (!sc.locate(g, rc, st.z)) continue;
    sc.make(g);
    const float om = body(st, sc.fp, sc.cell, T);
    if (!attenuate(T, om)) break;
  }
}

// ---- helpers -----------------------------------------------------------------------------------------------------------------
// Slope coefficients of one axis in terms of the cell's two corners (make_cell): slope = d0 * c0 + d1 * c1.  make_cell moves the
// low corner into the grid and folds the zero padding into the WEIGHTS, which keeps the value but not the derivative:
//   i0 in [0, N-2] : corners (i0, i0+1)          -> v(i0+1) - v(i0)   = c1 - c0
//   i0 == -1       : corners (0, 1), v(-1) = 0    -> v(0) - 0          = c0
//   i0 == N-1      : corners (N-2, N-1), v(N) = 0 -> 0 - v(N-1)        = -c1   (N == 1: stride 0, c0 == c1 == v(0))
//   otherwise      : both footprint corners outside the grid -> 0
__device__ __forceinline__ void slope_coefs(int i0, int N, float& d0, float& d1) {
  const bool lo = i0 < 0, hi = i0 >= N - 1;
  d0 = lo ? (i0 == -1 ? 1.0f : 0.0f) : (hi ? 0.0f : -1.0f);
  d1 = lo ? 0.0f : (hi ? (i0 == N - 1 ? -1.0f : 0.0f) : 1.0f);
}

// index units -> world units of a gradient: N_a * scale_a / 2
__device__ __forceinline__ void index_to_world(const DevGrid& g, float (&gs)[3]) {
  const int N[3] = {g.X, g.Y, g.Z};
#pragma unroll
  for (int a = 0; a < 3; ++a) gs[a] = ((float)N[a] * g.scale[a]) * 0.5f;
}

// World-space gradient G of the density field V in the cell of a sample, from the cell's pre-activated corner values `cv`
// (corner q = x + 2 y + 4 z): per axis the slope along it (slope_coefs) blended bilinearly over the two other axes with the
// cell's weights, times `gs` = N_a * scale_a / 2 (index_to_world).  The normals kernels and the orientation loss share it.
__device__ __forceinline__ void cell_gradient(const DevGrid& g, const Footprint& fp, const Cell& cell, const float (&cv)[8],
                                              const float (&gs)[3], float (&G)[3]) {
  const int N[3] = {g.X, g.Y, g.Z};
  float d[3][2];
#pragma unroll
  for (int a = 0; a < 3; ++a) slope_coefs(fp.i0[a], N[a], d[a][0], d[a][1]);
#pragma unroll
  for (int a = 0; a < 3; ++a) G[a] = 0.0f;
#pragma unroll
  for (int p = 0; p < 4; ++p) {   // p = the corner bits of the two other axes
    // x: corners (0 | 2y | 4z), y: (x | 0 | 4z), z: (x | 2y | 0)
    const int b0 = p & 1, b1 = p >> 1;
    const int kx = 2 * b0 + 4 * b1, ky = b0 + 4 * b1, kz = b0 + 2 * b1;
    const float ex = fmaf(d[0][1], cv[kx + 1], d[0][0] * cv[kx]);
    const float ey = fmaf(d[1][1], cv[ky + 2], d[1][0] * cv[ky]);
    const float ez = fmaf(d[2][1], cv[kz + 4], d[2][0] * cv[kz]);
    G[0] = fmaf(cell.w[1][b0] * cell.w[2][b1], ex, G[0]);
    G[1] = fmaf(cell.w[0][b0] * cell.w[2][b1], ey, G[1]);
    G[2] = fmaf(cell.w[0][b0] * cell.w[1][b1], ez, G[2]);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) G[a] = G[a] * gs[a];
}

// blocks of a launch whose threads find their ray with map_ray(): a 16x16 pixel tile (8x8 per wave) or 256 consecutive rays
inline unsigned map_ray_blocks(const DevCfg& c) {
  const long long ntx = c.image_width > 0 ? (c.image_width + 15) / 16 : 1;
  const long long nty = c.image_width > 0 ? tile_rows_total(c, 16) : (c.R + kMarchThreads - 1) / kMarchThreads;
  return (unsigned)blocks_for_tiles(c.map_mode, ntx, nty);
}

}  // namespace voxe
