// voxe_normals.hip -- density-gradient normals of a voxel grid ("Normals").
//
// The field is the one of the mesh export (section 4.8): v_i = pre(s * raw_i) per voxel, V(p) its trilinear interpolant with
// grid_sample semantics (zero padding).  In the cell floor(u) selects, dV/du_a is a bilinear blend (over the other two axes) of
// the slope along a, and the world gradient is G_a = dV/du_a * (N_a * scale_a / 2).  The point normal is n = -G / |G| (toward
// lower density), (0,0,0) where G == 0.  Only the raw densities are read (4-byte loads, pre_activate per corner: the bits the
// pack kernel stores), so no workspace, no pack pass and no forward record are involved.
//
//   query  : one thread per point (grid-stride).
//   render : G consecutive lanes per ray (G = lanes_per_ray(R) in {1, 2, 4, 8}); lane j marches the j-th contiguous block of the
//            ray's S samples with a local transmittance, exactly the forward's samples (the depth step, sample cell and
//            density sample of voxe_ray_march.hpp); the group then folds its blocks front to back with shuffles: exclusive
//            product of the block transmittances, sum of T_start * (normal[3], acc, depth).  No atomics, fixed order: the
//            same bits on every run.
#include <hip/hip_runtime.h>

#include "voxe_launch.hpp"
#include "voxe_ray_march.hpp"

namespace voxe {
namespace {

constexpr int kNormThreads = kMarchThreads;
constexpr int kQueryMaxBlocks = 4096;   // grid-stride beyond this (cdna_hip_programming.md Guideline 11)

// n(p) = -G / |G| from the cell's corner values (cell_gradient()); `gs` = N_a * scale_a / 2 (index units -> world units).  G
// is scaled by its largest component first, so no |G|^2 underflows or overflows; exactly (0,0,0) where G == 0.
__device__ __forceinline__ void cell_normal(const DevGrid& g, const Footprint& fp, const Cell& cell, const float (&cv)[8],
                                            const float (&gs)[3], float (&n)[3]) {
  float G[3];
  cell_gradient(g, fp, cell, cv, gs, G);
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

__global__ __launch_bounds__(kNormThreads) void query_normals_kernel(DevGrid g, const float* __restrict__ dens,
                                                                     const float* __restrict__ points, long long N,
                                                                     float* __restrict__ normals) {
  float gs[3];
  index_to_world(g, gs);
  for (long long i = (long long)blockIdx.x * kNormThreads + threadIdx.x; i < N; i += (long long)gridDim.x * kNormThreads) {
    const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    Footprint fp;
    footprint(g, p, fp);
    Cell cell;
    make_cell(g, fp, cell);
    DensityTaps tp;
    load_density(g, dens, cell, tp);
    float cv[8], n[3];
#pragma unroll
    for (int k = 0; k < 8; ++k) cv[k] = pre_activate(g.pre_act, tp.raw[k], g.density_scale);
    cell_normal(g, fp, cell, cv, gs, n);
#pragma unroll
    for (int a = 0; a < 3; ++a) normals[3 * i + a] = n[a];
  }
}

template <int G>
__global__ __launch_bounds__(kNormThreads) void render_normals_kernel(DevGrid g, DevCfg c, const float* __restrict__ dens,
                                                                      const float* __restrict__ rays_o,
                                                                      const float* __restrict__ rays_d,
                                                                      const float* __restrict__ jitter,
                                                                      float* __restrict__ normals, float* __restrict__ depth,
                                                                      float* __restrict__ acc) {
  long long r;
  const bool valid = group_ray<BlockRectTile<G>>(c, r);   // (uniform over the G lanes of a ray: every lane joins the shuffles below)
  const int j = threadIdx.x % G;
  float T = 1.0f, asum = 0.0f, dsum = 0.0f, nsum[3] = {0.0f, 0.0f, 0.0f};
  if (valid) {
    RayCtx<1, 1, 1> rc;
    rc.init(g, c, r, rays_o, rays_d, jitter);
    float gs[3];
    index_to_world(g, gs);
    int k_lo, k_hi;
    lane_block(c, rc, j, G, k_lo, k_hi);
    if (k_lo <= k_hi) {
      // (not march_block: like the forward, this march integrates every sample and has no exit at T == 0)
      DepthStep st;
      st.start(rc, k_lo);
      for (int k = k_lo; k <= k_hi; ++k) {
        st.advance(rc, c, k);
        SampleCell sc;
        if (!sc.locate(g, rc, st.z)) continue;
        sc.make(g);
        DensityTaps tp;
        load_density(g, dens, sc.cell, tp);
        DensitySample s;
        eval_density<false>(g, sc.cell, tp, st.dl(), rc.dnorm, s);
        const float w = s.alpha * T;
        T = T * s.om;
        asum = asum + w;
        dsum = fmaf(st.z, w, dsum);
        if (w > 0.0f) {
          float n[3];
          cell_normal(g, sc.fp, sc.cell, s.cv, gs, n);
#pragma unroll
          for (int a = 0; a < 3; ++a) nsum[a] = fmaf(w, n[a], nsum[a]);
        }
      }
    }
  }
  if constexpr (G > 1) {
    const float Tstart = group_exclusive_product<G>(T, j);   // transmittance in front of this lane's block
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

}  // namespace

void launch_query_normals(const DevGrid& g, const float* dens, const float* points, long long N, float* normals,
                          hipStream_t st) {
  const long long nb = (N + kNormThreads - 1) / kNormThreads;
  query_normals_kernel<<<(unsigned)(nb < kQueryMaxBlocks ? nb : kQueryMaxBlocks), kNormThreads, 0, st>>>(g, dens, points, N, normals);
}

void launch_render_normals(const DevGrid& g, const DevCfg& c, const float* dens, const float* rays_o, const float* rays_d,
                           const float* jitter, float* normals, float* depth, float* acc, hipStream_t st) {
  for_lanes(lanes_per_ray(c.R, 0), [&](auto G) {
    const long long nb = group_blocks<BlockRectTile<G()>>(c);
    render_normals_kernel<G()><<<(unsigned)nb, kNormThreads, 0, st>>>(g, c, dens, rays_o, rays_d, jitter, normals, depth, acc);
  });
}

}  // namespace voxe
