// voxe_distortion.hip -- distortion loss on rays, value and gradient in one call ("Distortion").
//
// Per ray, with the forward's exact samples (voxe_ray_march.hpp: both marches are a march_block over the density sample) and
// s_k = (z_k - near) / (far - near) from cfg's bounds:
//   d_k = s_{k+1} - s_k (0 for the last sample),  m_k = s_k + d_k / 2,  w_k = T_k alpha_k
//   L_r = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
// The depths of a ray never decrease, so |m_i - m_j| = m_i - m_j for j < i and, with the exclusive prefixes
// W_i = sum_{j<i} w_j, WM_i = sum_{j<i} w_j m_j:
//   L_r = 2 sum_i w_i (m_i W_i - WM_i) + (1/3) sum_i w_i^2 d_i                                   -- O(S)
//   g_i = dL_r/dw_i = 2 [(m_i W_i - WM_i) + (WM_tot - WM_i - w_i m_i) - m_i (W_tot - W_i - w_i)] + (2/3) w_i d_i
//   dL_r/dsigma_k = delta_k [g_k (T_k - w_k) - sum_{i>k} g_i w_i],   sum_i g_i w_i = 2 L_r  (L_r is homogeneous of degree 2)
//
// G consecutive lanes share a ray (G in {1, 2, 4, 8}, lanes_per_ray(); WaveRectTile, lane_block and group_exclusive_product of
// voxe_ray_march.hpp); lane j owns the j-th contiguous block of the ray's S samples.
//   march 1 : the block with a local T = 1: its transmittance product and A = sum w~, B = sum w~ m, the block's own pair term
//             P = sum_i w~_i (m_i A_i - B_i) and U = sum w~^2 d.  With T_s the transmittance in front of the block (exclusive
//             product over the lanes before it) the true weights are w = T_s w~, so the block adds T_s A to W, T_s B to WM and
//                 T_s^2 (2 P + U / 3) + 2 T_s (B W0 - A WM0)
//             to L_r, W0 / WM0 being the prefixes at the block's first sample (exclusive sums over the lanes before it).
//   march 2 : the block again with the true T, W, WM; the prefix of sum g w at the block's first sample follows from the scans:
//                 sum_{i in Pre} g_i w_i = 2 L(Pre) + 2 [W0 (WM_tot - WM0) - WM0 (W_tot - W0)]
//             (the pairs inside the prefix count twice, the pairs across once); per sample the suffix is 2 L_r - prefix, and the
//             8 corners receive  (grad_scale / R) dL_r/dsigma_k * post'(v) * t_c * pre'(raw_c)  through float atomics.
// Every running sum (W, WM, sum g w, L_r) and the normalised depths are double: the suffix is a difference of sums.  The
// per-sample work (gather, activations, fast_exp, T) is float, as in the renderer.
#include <hip/hip_runtime.h>

#include "voxe_ray_loss.hpp"

namespace voxe {
namespace {

constexpr int kDistThreads = kMarchThreads;

template <int G, bool GRAD>
__global__ __launch_bounds__(kDistThreads) void distortion_kernel(DevGrid g, DevCfg c, const float* __restrict__ dens,
                                                                  const float* __restrict__ rays_o,
                                                                  const float* __restrict__ rays_d,
                                                                  const float* __restrict__ jitter, float gscale,
                                                                  float* __restrict__ ray_loss, double* __restrict__ partial,
                                                                  float* d_dens) {
  long long r;
  const bool valid = group_ray<WaveRectTile<G>>(c, r);   // (uniform over the G lanes of a ray: every lane joins the shuffles below)
  const int j = threadIdx.x % G;
  const double snear = (double)c.near, sinv = 1.0 / ((double)c.far - (double)c.near);
  RayCtx<1, 1, 1> rc;
  int k_lo = 1, k_hi = 0;
  float T = 1.0f;
  double A = 0.0, B = 0.0, P = 0.0, U = 0.0;
  // one sample of either march: the density sample, then w, d and m in double
  const auto sample = [&](const DepthStep& st, const Cell& cell, float T, DensityTaps& tp, DensitySample& s, double& w, double& d,
                          double& m) {
    load_density(g, dens, cell, tp);
    eval_density<true>(g, cell, tp, st.dl(), rc.dnorm, s);
    w = (double)((1.0f - s.e) * T);
    d = st.last ? 0.0 : ((double)st.z_next - (double)st.z) * sinv;
    m = ((double)st.z - snear) * sinv + 0.5 * d;
  };
  if (valid) {
    rc.init(g, c, r, rays_o, rays_d, jitter);
    lane_block(c, rc, j, G, k_lo, k_hi);
    march_block(g, c, rc, k_lo, k_hi, T, [&](const DepthStep& st, const Footprint&, const Cell& cell, float T) {
      DensityTaps tp;
      DensitySample s;
      double w, d, m;
      sample(st, cell, T, tp, s, w, d, m);
      P += w * (m * A - B);
      A += w;
      B += w * m;
      U += (w * w) * d;
      return s.om;   // (T ends: every later w of the block is 0)
    });
  }
  // the blocks of a ray folded front to back
  float Ts = 1.0f;
  double W0 = 0.0, WM0 = 0.0, Lpre = 0.0;
  double Wtot = A, WMtot = B, Ltot = 2.0 * P + U * (1.0 / 3.0);
  if constexpr (G > 1) {
    Ts = group_exclusive_product<G>(T, j);
    const double ts = (double)Ts;
    const double a = ts * A, b = ts * B;
    const double ai = group_scan<G>(a, j), bi = group_scan<G>(b, j);
    W0 = ai - a;
    WM0 = bi - b;
    const double l = (ts * ts) * Ltot + 2.0 * (b * W0 - a * WM0);
    const double li = group_scan<G>(l, j);
    Lpre = li - l;
    Wtot = __shfl(ai, G - 1, G);
    WMtot = __shfl(bi, G - 1, G);
    Ltot = __shfl(li, G - 1, G);
  }
  ray_loss_outputs(valid, j, r, Ltot, 1.0f, ray_loss, partial);
  if constexpr (GRAD) {
    if (!valid || k_lo > k_hi || !(Ts > 0.0f)) return;
    T = Ts;
    double W = W0, WM = WM0;
    double GW = 2.0 * Lpre + 2.0 * (W0 * (WMtot - WM0) - WM0 * (Wtot - W0));   // sum g w over the samples in front of the block
    const double total = 2.0 * Ltot;
    march_block(g, c, rc, k_lo, k_hi, T, [&](const DepthStep& st, const Footprint&, const Cell& cell, float T) {
      DensityTaps tp;
      DensitySample s;
      double w, d, m;
      sample(st, cell, T, tp, s, w, d, m);
      const double gi = 2.0 * ((m * W - WM) + ((WMtot - WM - w * m) - m * (Wtot - W - w))) + (2.0 / 3.0) * (w * d);
      W += w;
      WM += w * m;
      GW += gi * w;
      // (om == 0: T ends here, every later w is 0 and so is the true suffix; what the subtraction leaves is rounding)
      const double suffix = (st.last || !(s.om > 0.0f)) ? 0.0 : (total - GW);
      const float dsig = s.delta * (float)(gi * (double)(T * s.e) - suffix);   // T e = T - w
      const float dv = (dsig * s.dpost) * gscale;
      if (dv != 0.0f) deposit_corners(g, tp, d_dens, [&](int q) { return dv * s.t[q]; });   // adding exact zeros is skipped
      return s.om;   // (T ends: every later term is 0)
    });
  }
}

// loss = (sum of the per-block partials, fixed order) / R; launch_partial_mean() below serves every ray loss (voxe_ray_loss.hpp)
__global__ __launch_bounds__(kDistThreads) void distortion_finalize_kernel(const double* __restrict__ partial, long long nb,
                                                                           double inv_R, float* __restrict__ loss_out) {
  double s = 0.0;
  for (long long i = threadIdx.x; i < nb; i += kDistThreads) s += partial[i];
  const double tot = block_sum(s);
  if (threadIdx.x == 0) *loss_out = (float)(tot * inv_R);
}

}  // namespace

void launch_partial_mean(const double* partial, long long nb, long long R, float* loss_out, hipStream_t st) {
  distortion_finalize_kernel<<<1, kDistThreads, 0, st>>>(partial, nb, 1.0 / (double)R, loss_out);
}

// one partial per block, and a launch never has more blocks than rays (every pixel tile holds at least one pixel)
size_t ray_loss_scratch_bytes(long long R) { return sizeof(double) * (size_t)(R > 0 ? R : 0) + 256; }

void launch_distortion(const DevGrid& g, const DevCfg& c, const float* dens, const float* rays_o, const float* rays_d,
                       const float* jitter, float grad_scale, float* loss_out, float* ray_loss, float* d_dens, void* scratch,
                       hipStream_t st) {
  launch_ray_loss(c, tl_lane_pins.distortion, grad_scale, loss_out, d_dens, scratch, st,
                  [&](auto G, auto GRAD, long long nb, float gscale, double* partial) {
                    distortion_kernel<G(), GRAD()><<<(unsigned)nb, kDistThreads, 0, st>>>(g, c, dens, rays_o, rays_d, jitter, gscale,
                                                                                          ray_loss, partial, d_dens);
                  });
}

}  // namespace voxe
