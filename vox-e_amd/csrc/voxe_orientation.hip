// voxe_orientation.hip -- orientation loss on rays, value and gradient in one call ("Orientation";
// Ref-NeRF, Verbin et al. 2022, eq. 11).
//
// Per ray, with the forward's exact samples (voxe_ray_march.hpp), u = d / |d| and G_k the world-space gradient of the density
// field in the cell of sample k (cell_gradient(): the field of voxe_render_normals, n_k = -G_k / |G_k|):
//   rho_k = sqrt(|G_k|^2 + eps^2),  c_k = max(0, -(G_k . u)) / rho_k  (0 where rho_k == 0),  w_k = T_k alpha_k
//   L_r = sum_k w_k c_k^2
// The densities receive the gradient two ways, on the same 8 corners of the sample's cell:
//   weights : dL_r/dsigma_k = delta_k [c_k^2 (T_k - w_k) - sum_{i>k} c_i^2 w_i], then post'(v), the gather weight t_q and
//             pre'(raw_q)
//   normals : dL_r/dG_k = 2 w_k c_k (-u / rho_k - c_k G_k / rho_k^2) for c_k > 0 (exactly 0 otherwise), then
//             dG_a/dv_q = (N_a scale_a / 2) * (slope coefficient of corner q on axis a) * (the two other axes' cell weights)
//             and pre'(raw_q); post is not on this path.  The slope coefficients differ from the gather weights in the face
//             cells (see slope_coefs()).
// rho and c are formed from G / M and eps / M with M = max(|G_x|, |G_y|, |G_z|, eps): no square overflows or underflows.
//
// G consecutive lanes share a ray (G in {1, 2, 4, 8}); lane j owns the j-th contiguous block of the ray's S samples.  L_r is
// linear in the weights, so a block is summed with a local T = 1 and scaled by the transmittance in front of it:
//   march 1 : the block with a local T = 1: its transmittance product, A = sum w~ c^2 and the last sample that adds to A.  With
//             T_s the exclusive product over the lanes before it the block adds T_s A to L_r; a scan from the back gives the sum
//             over the blocks behind this one.
//   march 2 : (gradient) the block again with the true T; the suffix of a sample is the blocks behind plus the block's total
//             minus its running sum, and nothing of the block behind the block's last contributing sample (the subtraction
//             would leave its rounding there, times delta, on voxels whose gradient is 0).  Both parts are combined per corner
//             before the one float atomic.
// Running sums are double (the suffix is a difference of sums), the per-sample work is float, as in voxe_distortion.hip.
#include <hip/hip_runtime.h>

#include "voxe_ray_loss.hpp"

namespace voxe {
namespace {

constexpr int kOrientThreads = kMarchThreads;

// c_k and, for the normals part, what dL/dG needs: c, the scaled gradient q = G / M, 1 / (rho / M) and 1 / M.  M is brought
// into [2^-64, 2^64] by a power of two first, so v_rcp_f32 sees and returns a normal number.
struct Facing {
  float c, q[3], inv_rho, inv_M;
};
__device__ __forceinline__ void facing(const float (&G)[3], const float (&u)[3], float eps, Facing& f) {
  const float M = fmaxf(fmaxf(fmaxf(fabsf(G[0]), fabsf(G[1])), fabsf(G[2])), eps);
  f.c = 0.0f;
  if (!(M > 0.0f)) return;   // (rho == 0)
  const float sc = M < 0x1p-64f ? 0x1p64f : (M > 0x1p64f ? 0x1p-64f : 1.0f);
  const float inv = fast_rcp(M * sc);
  f.inv_M = inv * sc;
  const float e = (eps * sc) * inv;
#pragma unroll
  for (int a = 0; a < 3; ++a) f.q[a] = (G[a] * sc) * inv;
  // (rho / M)^2 in [1, 4]
  f.inv_rho = __builtin_amdgcn_rsqf(fmaf(f.q[0], f.q[0], fmaf(f.q[1], f.q[1], fmaf(f.q[2], f.q[2], e * e))));
  const float dot = fmaf(f.q[0], u[0], fmaf(f.q[1], u[1], f.q[2] * u[2]));
  f.c = fmaxf(0.0f, -dot) * f.inv_rho;
}

template <int G, bool GRAD>
__global__ __launch_bounds__(kOrientThreads) void orientation_kernel(DevGrid g, DevCfg c, const float* __restrict__ dens,
                                                                     const float* __restrict__ rays_o,
                                                                     const float* __restrict__ rays_d,
                                                                     const float* __restrict__ jitter,
                                                                     const float* __restrict__ rweight, float eps, float gscale,
                                                                     float* __restrict__ ray_loss, double* __restrict__ partial,
                                                                     float* d_dens) {
  long long r;
  const bool valid = group_ray<WaveRectTile<G>>(c, r);   // (uniform over the G lanes of a ray: every lane joins the shuffles below)
  const int j = threadIdx.x % G;
  RayCtx<1, 1, 1> rc;
  int k_lo = 1, k_hi = 0, n_last = -1;   // n_last: the block's last contributing sample, counted over the samples inside the box
  float T = 1.0f, omega = 0.0f;
  float gs[3], u[3] = {0.0f, 0.0f, 0.0f};
  index_to_world(g, gs);
  double A = 0.0;
  if (valid) {
    rc.init(g, c, r, rays_o, rays_d, jitter);
    lane_block(c, rc, j, G, k_lo, k_hi);
    omega = rweight ? rweight[r] : 1.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = rc.d[a] / rc.dnorm;
    int n = 0;
    march_block(g, c, rc, k_lo, k_hi, T, [&](const DepthStep& st, const Footprint& fp, const Cell& cell, float T) {
      DensityTaps tp;
      DensitySample s;
      load_density(g, dens, cell, tp);
      eval_density<false>(g, cell, tp, st.dl(), rc.dnorm, s);
      const float w = s.alpha * T;
      if (w > 0.0f) {
        float Gk[3];
        Facing f;
        cell_gradient(g, fp, cell, s.cv, gs, Gk);
        facing(Gk, u, eps, f);
        const float cw = (f.c * f.c) * w;
        A += (double)cw;
        if (cw != 0.0f) n_last = n;
      }
      ++n;
      return s.om;   // (T ends: every later w of the block is 0)
    });
  }
  // the blocks of a ray folded front to back
  float Ts = 1.0f;
  double Ablk = A, Ltot = A, Abehind = 0.0;
  if constexpr (G > 1) {
    Ts = group_exclusive_product<G>(T, j);
    Ablk = (double)Ts * A;
    Ltot = __shfl(group_scan<G>(Ablk, j), G - 1, G);
    // sum over the blocks behind this one: inclusive scan from the back, read from the next lane
    double v = Ablk;
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
      const double t = __shfl_down(v, off, G);
      if (j + off < G) v += t;
    }
    v = __shfl_down(v, 1, G);
    Abehind = j == G - 1 ? 0.0 : v;
  }
  ray_loss_outputs(valid, j, r, Ltot, omega, ray_loss, partial);
  if constexpr (GRAD) {
    const float gsc = gscale * omega;
    // (no sample of the ray faces away with weight: both parts are exactly 0)
    if (!valid || k_lo > k_hi || !(Ts > 0.0f) || Ltot == 0.0 || gsc == 0.0f) return;
    T = Ts;
    double Arun = 0.0;
    int n = 0;
    march_block(g, c, rc, k_lo, k_hi, T, [&](const DepthStep& st, const Footprint& fp, const Cell& cell, float T) {
      DensityTaps tp;
      DensitySample s;
      load_density(g, dens, cell, tp);
      eval_density<true>(g, cell, tp, st.dl(), rc.dnorm, s);
      const float w = s.alpha * T;
      // (c_k also where w_k == 0: sigma_k == 0 in front of T > 0 still has dL_r/dsigma_k = delta_k c_k^2 T_k)
      float Gk[3];
      Facing f;
      cell_gradient(g, fp, cell, s.cv, gs, Gk);
      facing(Gk, u, eps, f);
      const float c2 = f.c * f.c;
      Arun += (double)(c2 * w);
      // (om == 0: T ends here, every later w is 0 and so is the true suffix; at and behind the block's last contributing
      // sample only the blocks behind are left)
      const bool tail = n >= n_last;
      ++n;
      const double suffix = (st.last || !(s.om > 0.0f)) ? 0.0 : (tail ? Abehind : Abehind + (Ablk - Arun));
      const float dsig = s.delta * (float)((double)(c2 * (T * s.e)) - suffix);   // T e = T - w
      const float dv = (dsig * s.dpost) * gsc;
      const bool turned = f.c > 0.0f && w > 0.0f;
      if (dv != 0.0f || turned) {   // adding exact zeros is skipped
        // normals part: h[a][b] = dL/dG_a * (N_a scale_a / 2) * (slope coefficient of the corners with bit b on axis a)
        float h[3][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
        if (turned) {
          const int N[3] = {g.X, g.Y, g.Z};
          const float k2 = ((2.0f * w) * f.c) * (f.inv_rho * f.inv_M) * gsc;   // 2 w c / rho
          const float cr = f.c * f.inv_rho;                                   // c M / rho
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            float d0, d1;
            slope_coefs(fp.i0[a], N[a], d0, d1);
            const float dG = (k2 * (-u[a] - cr * f.q[a])) * gs[a];
            h[a][0] = dG * d0;
            h[a][1] = dG * d1;
          }
        }
        deposit_corners(g, tp, d_dens, [&](int q) {
          const int bx = q & 1, by = (q >> 1) & 1, bz = q >> 2;
          float gq = dv * s.t[q];
          if (turned) {
            gq = fmaf(h[0][bx], cell.w[1][by] * cell.w[2][bz], gq);
            gq = fmaf(h[1][by], cell.w[0][bx] * cell.w[2][bz], gq);
            gq = fmaf(h[2][bz], cell.w[0][bx] * cell.w[1][by], gq);
          }
          return gq;
        });
      }
      return s.om;   // (T ends: every later term is 0)
    });
  }
}

}  // namespace

void launch_orientation(const DevGrid& g, const DevCfg& c, const float* dens, const float* rays_o, const float* rays_d,
                        const float* jitter, const float* rweight, float eps, float grad_scale, float* loss_out, float* ray_loss,
                        float* d_dens, void* scratch, hipStream_t st) {
  launch_ray_loss(c, tl_lane_pins.orientation, grad_scale, loss_out, d_dens, scratch, st,
                  [&](auto G, auto GRAD, long long nb, float gscale, double* partial) {
                    orientation_kernel<G(), GRAD()><<<(unsigned)nb, kOrientThreads, 0, st>>>(g, c, dens, rays_o, rays_d, jitter, rweight,
                                                                                             eps, gscale, ray_loss, partial, d_dens);
                  });
}

}  // namespace voxe
