// voxe_visibility.hip -- per-voxel visibility of a voxel grid under a set of rays ("Visibility").
//
//   accumulate : one thread per ray marches the forward's exact samples front to back (voxe_ray_march.hpp: march_block with
//                the two halves of the density sample) and,
//                for every sample inside the box and every corner c of its cell with gather weight t_c = (wx * wy) * wz,
//                raises  max_weight[c] to w_k * t_c  and  max_trans[c] to T_k (where t_c > 0),  w_k = T_k * alpha_k, T_k the
//                transmittance on arrival.  Non-negative floats order like their bit patterns, so the update is an unsigned
//                integer atomic max: the result is the same bit for bit however lanes, waves and launches meet on a voxel.
//                The march is sequential per ray (no lanes-per-ray split): what a ray contributes depends on the ray and cfg
//                only, never on R, the ray's place in the batch or the image fields (those pick the thread mapping).
//                A plain load in front of every atomic (all 16 of a sample issued together with its 8 density loads) skips it
//                when the stored value is already >=: max is monotone, a stale value read there is never above the current
//                one, so a skipped update could not have changed the result.
//   mask       : one thread per voxel (z fastest): 1 iff some voxel within Chebyshev distance `dilate` has vis > threshold.
#include <hip/hip_runtime.h>

#include "voxe_launch.hpp"
#include "voxe_ray_march.hpp"

namespace voxe {
namespace {

constexpr int kVisThreads = kMarchThreads;   // map_ray(): a 16x16 pixel tile (8x8 per wave) or 256 consecutive rays
constexpr int kMaskMaxBlocks = 8192;      // grid-stride beyond this

// buf[i] = max(buf[i], v) for v > 0 on the uint32 view (no-return atomic); `seen` = what a plain load of buf[i] returned before:
// the update is skipped when that is already >=
__device__ __forceinline__ void raise_to(unsigned* buf, unsigned i, float v, unsigned seen) {
  const unsigned bits = __float_as_uint(v);
  if (seen >= bits) return;
  (void)__hip_atomic_fetch_max(buf + i, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kVisThreads) void visibility_accumulate_kernel(DevGrid g, DevCfg c, const float* __restrict__ dens,
                                                                            const float* __restrict__ rays_o,
                                                                            const float* __restrict__ rays_d,
                                                                            const float* __restrict__ jitter, unsigned* max_weight,
                                                                            unsigned* max_trans) {
  long long r;
  if (!map_ray(c, r)) return;
  RayCtx<1, 1, 1> rc;
  rc.init(g, c, r, rays_o, rays_d, jitter);
  float T = 1.0f;
  march_block(g, c, rc, rc.k_lo, rc.k_hi, T, [&](const DepthStep& st, const Footprint&, const Cell& cell, float T) {
    DensityTaps tp;
    unsigned seen_w[8], seen_t[8];
    // the 8 densities and the stored values of the 16 pre-checks do not depend on each other: all loads go out together, one
    // memory latency per sample instead of one per corner
    load_density(g, dens, cell, tp);
#pragma unroll
    for (int q = 0; q < 8; ++q) seen_t[q] = max_trans ? max_trans[tp.idx[q]] : 0u;
#pragma unroll
    for (int q = 0; q < 8; ++q) seen_w[q] = max_weight ? max_weight[tp.idx[q]] : 0u;
    DensitySample s;
    eval_density<false>(g, cell, tp, st.dl(), rc.dnorm, s);
    const float w = s.alpha * T;
    // (corners make_cell moved into the grid carry weight 0: only footprint corners inside the grid are ever raised)
    if (max_trans && T > 0.0f) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (s.t[q] > 0.0f) raise_to(max_trans, tp.idx[q], T, seen_t[q]);
    }
    if (max_weight && w > 0.0f) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float cw = w * s.t[q];
        if (cw > 0.0f) raise_to(max_weight, tp.idx[q], cw, seen_w[q]);
      }
    }
    return s.om;   // (T ends: every later w and T is 0, nothing more to raise)
  });
}

__global__ __launch_bounds__(kVisThreads) void visibility_mask_kernel(const float* __restrict__ vis, int X, int Y, int Z,
                                                                      float threshold, int dilate, uint8_t* __restrict__ mask) {
  const long long n = (long long)X * Y * Z;
  for (long long i = (long long)blockIdx.x * kVisThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kVisThreads) {
    const int z = (int)(i % Z), y = (int)((i / Z) % Y), x = (int)(i / ((long long)Z * Y));
    const int x0 = max(x - dilate, 0), x1 = min(x + dilate, X - 1);
    const int y0 = max(y - dilate, 0), y1 = min(y + dilate, Y - 1);
    const int z0 = max(z - dilate, 0), z1 = min(z + dilate, Z - 1);
    bool keep = false;
    for (int a = x0; a <= x1; ++a)
      for (int b = y0; b <= y1; ++b) {
        const float* row = vis + ((long long)a * Y + b) * Z;
        for (int q = z0; q <= z1; ++q) keep = keep || (row[q] > threshold);   // (NaN > threshold is false: never kept)
      }
    mask[i] = keep ? 1 : 0;
  }
}

}  // namespace

void launch_visibility_accumulate(const DevGrid& g, const DevCfg& c, const float* dens, const float* rays_o, const float* rays_d,
                                  const float* jitter, float* max_weight, float* max_trans, hipStream_t st) {
  visibility_accumulate_kernel<<<map_ray_blocks(c), kVisThreads, 0, st>>>(g, c, dens, rays_o, rays_d, jitter,
                                                                     reinterpret_cast<unsigned*>(max_weight),
                                                                     reinterpret_cast<unsigned*>(max_trans));
}

void launch_visibility_mask(const float* vis, int X, int Y, int Z, float threshold, int dilate, uint8_t* mask, hipStream_t st) {
  const long long nb = ((long long)X * Y * Z + kVisThreads - 1) / kVisThreads;
  visibility_mask_kernel<<<(unsigned)(nb < kMaskMaxBlocks ? nb : kMaskMaxBlocks), kVisThreads, 0, st>>>(vis, X, Y, Z, threshold,
                                                                                                          dilate, mask);
}

}  // namespace voxe
