// voxe_normals.hip -- density-gradient normals of a voxel grid ("Normals").
//
// The field is the one of the mesh export (section 4.8): v_i = pre(s * raw_i) per voxel, V(p) its trilinear interpolant with
// grid_sample semantics (zero padding).  In the cell floor(u) selects, dV/du_a is a bilinear blend (over the other two axes) of
// the slope along a, and the world gradient is G_a = dV/du_a * (N_a * scale_a / 2).  The point normal is n = -G / |G| (toward
// lower density), (0,0,0) where G == 0.  Only the raw densities are read (4-byte loads, pre_activate per corner: the bits the
// pack kernel stores), so no workspace, no pack pass and no forward record are involved.
//
//   query  : one thread per point (grid-stride).
//   render : G consecutive lanes per ray (G = normals_lanes_for(R) in {1, 2, 4, 8}); lane j marches the j-th contiguous block of the ray's S samples with a local
//            transmittance, exactly the forward's samples (RayCtx / DepthGen / inside_range / footprint / post_activate /
//            fast_exp); the group then folds its blocks front to back with shuffles: exclusive product of the block
//            transmittances, sum of T_start * (normal[3], acc, depth).  No atomics, fixed order: the same bits on every run.
#include <hip/hip_runtime.h>

#include "voxe_launch.hpp"
#include "voxe_render_common.hpp"

namespace voxe {
namespace {

constexpr int kNormThreads = 256;
constexpr int kQueryMaxBlocks = 4096;   // grid-stride beyond this (cdna_hip_programming.md Guideline 11)

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

// The 8 pre-activated corner values of a cell (corner k = x + 2 y + 4 z), read from the raw densities
__device__ __forceinline__ void load_corners(const DevGrid& g, const float* __restrict__ dens, const Cell& cell, float (&cv)[8]) {
  const CellAddr ad = cell_addr(g, cell);
#pragma unroll
  for (int k = 0; k < 8; ++k)
    cv[k] = pre_activate(g.pre_act, dens[ad.base + (k & 1) * ad.sx + ((k >> 1) & 1) * ad.sy + (k >> 2) * ad.sz], g.density_scale);
}

// V(p) with the forward's weights and FMA order (gather(): wxy = wx * wy, w = wxy * wz, corners ascending)
__device__ __forceinline__ float interp_corners(const Cell& cell, const float (&cv)[8]) {
  float v = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float w = (cell.w[0][k & 1] * cell.w[1][(k >> 1) & 1]) * cell.w[2][k >> 2];
    v = fmaf(cv[k], w, v);
  }
  return v;
}

// n(p) = -G / |G| from the cell's corner values; `gs` = N_a * scale_a / 2 (index units -> world units).  G is scaled by its
// largest component first, so no |G|^2 underflows or overflows; exactly (0,0,0) where G == 0.
__device__ __forceinline__ void cell_normal(const DevGrid& g, const Footprint& fp, const Cell& cell, const float (&cv)[8],
                                            const float (&gs)[3], float (&n)[3]) {
  const int N[3] = {g.X, g.Y, g.Z};
  float d[3][2];
#pragma unroll
  for (int a = 0; a < 3; ++a) slope_coefs(fp.i0[a], N[a], d[a][0], d[a][1]);
  float G[3] = {0.0f, 0.0f, 0.0f};
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
  const float m = fmaxf(fmaxf(fabsf(G[0]), fabsf(G[1])), fabsf(G[2]));
  if (m > 0.0f) {
    const float inv = fast_rcp(m);
    const float q[3] = {G[0] * inv, G[1] * inv, G[2] * inv};
    const float r = -__builtin_amdgcn_rsqf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);   // |q| in [1, sqrt 3]
#pragma unroll
    for (int a = 0; a < 3; ++a) n[a] = q[a] * r;
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) n[a] = 0.0f;
  }
}

__device__ __forceinline__ void grad_scale(const DevGrid& g, float (&gs)[3]) {
  const int N[3] = {g.X, g.Y, g.Z};
#pragma unroll
  for (int a = 0; a < 3; ++a) gs[a] = ((float)N[a] * g.scale[a]) * 0.5f;
}

__global__ __launch_bounds__(kNormThreads) void query_normals_kernel(DevGrid g, const float* __restrict__ dens,
                                                                     const float* __restrict__ points, long long N,
                                                                     float* __restrict__ normals) {
  float gs[3];
  grad_scale(g, gs);
  for (long long i = (long long)blockIdx.x * kNormThreads + threadIdx.x; i < N; i += (long long)gridDim.x * kNormThreads) {
    const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    Footprint fp;
    footprint(g, p, fp);
    Cell cell;
    make_cell(g, fp, cell);
    float cv[8];
    load_corners(g, dens, cell, cv);
    float n[3];
    cell_normal(g, fp, cell, cv, gs, n);
#pragma unroll
    for (int a = 0; a < 3; ++a) normals[3 * i + a] = n[a];
  }
}

// Pixel rectangle of one block in image order: kNormThreads / G rays as TW x TH pixels
template <int G>
struct NormTile {
  static constexpr int kRays = kNormThreads / G;
  static constexpr int TW = G == 1 ? 16 : (G == 2 ? 16 : 8);
  static constexpr int TH = kRays / TW;
};

// ray of this thread's group (false: padding of the launch)
template <int G>
__device__ __forceinline__ bool normals_ray(const DevCfg& c, long long& r) {
  const int q = threadIdx.x / G;   // ray slot of the block
  if (c.image_width > 0) {
    using T = NormTile<G>;
    const int W = c.image_width, H = c.image_height;
    const long long ntx = (W + T::TW - 1) / T::TW, per = (long long)ntx * ((H + T::TH - 1) / T::TH);
    const long long b = blockIdx.x, img = b / per, t = b - img * per;
    const int ty = (int)(t / ntx), tx = (int)(t - (long long)ty * ntx);
    const int px = tx * T::TW + q % T::TW, py = ty * T::TH + q / T::TW;
    r = (img * H + py) * (long long)W + px;
    return px < W && py < H && r < c.R;
  }
  r = (long long)blockIdx.x * NormTile<G>::kRays + q;
  return r < c.R;
}

template <int G>
__global__ __launch_bounds__(kNormThreads) void render_normals_kernel(DevGrid g, DevCfg c, const float* __restrict__ dens,
                                                                      const float* __restrict__ rays_o,
                                                                      const float* __restrict__ rays_d,
                                                                      const float* __restrict__ jitter,
                                                                      float* __restrict__ normals, float* __restrict__ depth,
                                                                      float* __restrict__ acc) {
  long long r;
  const bool valid = normals_ray<G>(c, r);   // (uniform over the G lanes of a ray: every lane joins the shuffles below)
  const int j = threadIdx.x % G;
  float T = 1.0f, asum = 0.0f, dsum = 0.0f, nsum[3] = {0.0f, 0.0f, 0.0f};
  if (valid) {
    RayCtx<1, 1, 1> rc;
    rc.init(g, c, r, rays_o, rays_d, jitter);
    float gs[3];
    grad_scale(g, gs);
    const int len = (c.S + G - 1) / G;
    const int k_lo = max(rc.k_lo, j * len), k_hi = min(rc.k_hi, min(c.S, (j + 1) * len) - 1);
    if (k_lo <= k_hi) {
      float z_next = rc.dg.z(k_lo);
      for (int k = k_lo; k <= k_hi; ++k) {
        const float z = z_next;
        const bool last = (k == c.S - 1);
        if (!last) z_next = rc.dg.z(k + 1);
        float p[3];
        rc.point(z, p);
        Footprint fp;
        footprint(g, p, fp);
        if (!fp.inside) continue;   // sigma = 0 -> w = 0, T unchanged (the forward's rule)
        Cell cell;
        make_cell_fast(g, fp, cell);
        float cv[8];
        load_corners(g, dens, cell, cv);
        const float v = interp_corners(cell, cv);
        const float sigma = post_activate(g.post_act, v);
        const float dl = last ? kInfinity : (z_next - z);
        const float delta = dl * rc.dnorm;
        const float e = fast_exp(-(sigma * delta));
        const float alpha = 1.0f - e;
        const float om = 1.0f - alpha;
        const float w = alpha * T;
        T = T * om;
        asum = asum + w;
        dsum = fmaf(z, w, dsum);
        if (w > 0.0f) {
          float n[3];
          cell_normal(g, fp, cell, cv, gs, n);
#pragma unroll
          for (int a = 0; a < 3; ++a) nsum[a] = fmaf(w, n[a], nsum[a]);
        }
      }
    }
  }
  if constexpr (G > 1) {
    // transmittance in front of this lane's block: exclusive product over the lanes before it
    float P = T;
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
      const float t = __shfl_up(P, off, G);
      if (j >= off) P = P * t;
    }
    float Tstart = __shfl_up(P, 1, G);
    if (j == 0) Tstart = 1.0f;
    float s[5] = {Tstart * nsum[0], Tstart * nsum[1], Tstart * nsum[2], Tstart * asum, Tstart * dsum};
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
#pragma unroll
      for (int q = 0; q < 5; ++q) s[q] = s[q] + __shfl_xor(s[q], off, G);
    }
    nsum[0] = s[0]; nsum[1] = s[1]; nsum[2] = s[2]; asum = s[3]; dsum = s[4];
  }
  if (!valid || j != 0) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) normals[3 * r + a] = nsum[a];
  if (depth) depth[r] = dsum;
  if (acc) acc[r] = asum;
}

template <int G>
void launch_render_normals_t(const DevGrid& g, const DevCfg& c, const float* dens, const float* rays_o, const float* rays_d,
                             const float* jitter, float* normals, float* depth, float* acc, hipStream_t st) {
  long long nb;
  if (c.image_width > 0) {
    using T = NormTile<G>;
    const long long nimg = c.R / ((long long)c.image_width * c.image_height);
    nb = nimg * ((c.image_width + T::TW - 1) / T::TW) * (long long)((c.image_height + T::TH - 1) / T::TH);
  } else {
    nb = (c.R + NormTile<G>::kRays - 1) / NormTile<G>::kRays;
  }
  render_normals_kernel<G><<<(unsigned)nb, kNormThreads, 0, st>>>(g, c, dens, rays_o, rays_d, jitter, normals, depth, acc);
}

}  // namespace

int normals_lanes_for(long long R) {
#ifdef VOXE_NORMALS_LANES
  return VOXE_NORMALS_LANES;
#else
  // enough waves to fill 1024 SIMDs several times over: R * G >= 2^20 lane-rays, at most 8 lanes per ray
  for (int G = 1; G < 8; G <<= 1)
    if (R * G >= (1ll << 20)) return G;
  return 8;
#endif
}

void launch_query_normals(const DevGrid& g, const float* dens, const float* points, long long N, float* normals,
                          hipStream_t st) {
  const long long nb = (N + kNormThreads - 1) / kNormThreads;
  query_normals_kernel<<<(unsigned)(nb < kQueryMaxBlocks ? nb : kQueryMaxBlocks), kNormThreads, 0, st>>>(g, dens, points, N, normals);
}

void launch_render_normals(const DevGrid& g, const DevCfg& c, const float* dens, const float* rays_o, const float* rays_d,
                           const float* jitter, float* normals, float* depth, float* acc, hipStream_t st) {
  switch (normals_lanes_for(c.R)) {
    case 1: launch_render_normals_t<1>(g, c, dens, rays_o, rays_d, jitter, normals, depth, acc, st); break;
    case 2: launch_render_normals_t<2>(g, c, dens, rays_o, rays_d, jitter, normals, depth, acc, st); break;
    case 4: launch_render_normals_t<4>(g, c, dens, rays_o, rays_d, jitter, normals, depth, acc, st); break;
    default: launch_render_normals_t<8>(g, c, dens, rays_o, rays_d, jitter, normals, depth, acc, st); break;
  }
}

}  // namespace voxe
