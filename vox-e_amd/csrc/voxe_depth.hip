// voxe_depth.hip -- ray-termination loss towards per-ray depth targets, value and gradient in one call (DESIGN.md section 4.19,
// "Depth supervision"; DS-NeRF, Deng et al. 2022, as its published code evaluates the term).
//
// Per ray, with the forward's exact samples (voxe_ray_march.hpp), a target depth D and a width s in the units of z:
//   dz_k = z_{k+1} - z_k (0 for the last sample),  c_k = exp(-(z_k - D)^2 / (2 s^2)) dz_k,  w_k = T_k alpha_k
//   L_r = -sum_k c_k log(w_k + eps)  over ALL S samples: one outside the box, or behind the point where T reaches 0, has w = 0
//         and adds the constant -c_k log(eps)
//   g_k = dL_r/dw_k = -c_k / (w_k + eps),   dL_r/dsigma_k = delta_k [g_k (T_k - w_k) - sum_{i>k} g_i w_i]
// The kernel evaluates  L_r = -log(eps) sum_k c_k - sum_k c_k log1p(w_k / eps):  the first sum needs depths only and runs over
// every sample, the second over the samples the march reaches (w = 0 adds exactly 0).
//
// alpha: w_k enters log(w + eps) and 1 / (w + eps) with w at or below eps where the field is nearly empty, so the cancellation
// of 1 - fast_exp(-x) at small x = sigma delta (1e-2 relative to w at x = 1e-6) would reach the result.  alpha here is
// -expm1(-x): a five-term series below x = 1/8 (truncation 4e-8 relative), 1 - e above (1e-6 relative).  The transmittance
// product keeps the renderer's 1 - alpha.
//
// G consecutive lanes share a ray (G in {1, 2, 4, 8}); lane j owns the j-th contiguous block of the ray's S samples.  sum g w is
// not homogeneous in the transmittance in front of a block (eps), so a block cannot be summed with a local T = 1:
//   phase 0 : depths only, the lane's whole block: sum c_k
//   phase 1 : (G > 1) the block's transmittance product; exclusive product over the lanes -> T_s in front of the block
//   phase 2 : the block with the true T: sum c_k log1p(w_k / eps) and the block's B = sum g_k w_k; a scan over the lanes -> L_r,
//             a scan from the back -> A, the sum of B over the blocks behind this one
//   phase 3 : (gradient) the block again; per sample the suffix is A + (B - the block's running sum), and the 8 corners receive
//             (grad_scale omega_r / R) dL_r/dsigma_k * post'(v) * t_c * pre'(raw_c) through float atomics.  The running sum
//             repeats phase 2's additions in phase 2's order, so behind the last sample with c_k != 0 the suffix is exactly 0
//             (a total taken from a scan would leave its rounding there, times delta, on voxels whose gradient is 0)
// Running sums are double (the suffix is a difference of sums), the per-sample work is float, as in voxe_distortion.hip.
#include <hip/hip_runtime.h>

#include "voxe_ray_loss.hpp"

namespace voxe {
namespace {

constexpr int kDepthThreads = kMarchThreads;

// -expm1(-x) for the optical depth x of a sample, e = fast_exp(-x)
__device__ __forceinline__ float opacity_expm1(float x, float e) {
  const float p = fmaf(x, fmaf(x, fmaf(x, fmaf(x, 1.0f / 120.0f, -1.0f / 24.0f), 1.0f / 6.0f), -0.5f), 1.0f);
  return x < 0.125f ? x * p : 1.0f - e;
}

// the target of a ray: c_k of a depth step
struct DepthTarget {
  float D, inv_s;
  __device__ __forceinline__ float coef(const DepthStep& st) const {
    if (st.last) return 0.0f;
    const float t = (st.z - D) * inv_s;
    return fast_exp(-0.5f * (t * t)) * (st.z_next - st.z);
  }
};

template <int G, bool GRAD>
__global__ __launch_bounds__(kDepthThreads) void depth_kernel(DevGrid g, DevCfg c, const float* __restrict__ dens,
                                                              const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                              const float* __restrict__ jitter, const float* __restrict__ tdepth,
                                                              const float* __restrict__ tsigma, const float* __restrict__ rweight,
                                                              float eps, float inv_eps, double neg_log_eps, float gscale,
                                                              float* __restrict__ ray_loss, double* __restrict__ partial,
                                                              float* d_dens) {
  long long r;
  const bool valid = group_ray<WaveRectTile<G>>(c, r);   // (uniform over the G lanes of a ray: every lane joins the shuffles below)
  const int j = threadIdx.x % G;
  RayCtx<1, 1, 1> rc;
  DepthTarget tg{0.0f, 0.0f};
  int k_lo = 1, k_hi = 0;
  float T = 1.0f, omega = 0.0f;
  double Csum = 0.0;
  if (valid) {
    rc.init(g, c, r, rays_o, rays_d, jitter);
    lane_block(c, rc, j, G, k_lo, k_hi);
    tg.D = tdepth[r];
    tg.inv_s = 1.0f / tsigma[r];
    omega = rweight ? rweight[r] : 1.0f;
    // phase 0: every sample of the lane's block, inside the box or not
    const int len = (c.S + G - 1) / G, b_lo = j * len, b_hi = min(c.S, (j + 1) * len) - 1;
    if (b_lo <= b_hi) {
      DepthStep st;
      st.start(rc, b_lo);
      for (int k = b_lo; k <= b_hi; ++k) {
        st.advance(rc, c, k);
        Csum += (double)tg.coef(st);
      }
    }
    // phase 1: the block's transmittance product
    if constexpr (G > 1) {
      march_block(g, c, rc, k_lo, k_hi, T, [&](const DepthStep& st, const Footprint&, const Cell& cell, float) {
        DensityTaps tp;
        DensitySample s;
        load_density(g, dens, cell, tp);
        eval_density<false>(g, cell, tp, st.dl(), rc.dnorm, s);
        return s.om;
      });
    }
  }
  float Ts = 1.0f;
  if constexpr (G > 1) Ts = group_exclusive_product<G>(T, j);
  // phase 2: the block with the true T
  const bool reached = valid && k_lo <= k_hi && Ts > 0.0f;
  double Lw = 0.0, GW = 0.0;
  if (reached) {
    T = Ts;
    march_block(g, c, rc, k_lo, k_hi, T, [&](const DepthStep& st, const Footprint&, const Cell& cell, float T) {
      DensityTaps tp;
      DensitySample s;
      load_density(g, dens, cell, tp);
      eval_density<false>(g, cell, tp, st.dl(), rc.dnorm, s);
      const float ck = tg.coef(st);
      if (ck != 0.0f) {
        const float w = T * opacity_expm1(s.sigma * s.delta, s.e);
        Lw += (double)(ck * log1pf(w * inv_eps));
        GW += (double)((-ck / (w + eps)) * w);
      }
      return s.om;   // (T ends: every later w of the ray is 0, its terms are in Csum)
    });
  }
  double Ctot = Csum, Ltot = neg_log_eps * Csum - Lw, GWbehind = 0.0;
  if constexpr (G > 1) {
    Ctot = __shfl(group_scan<G>(Csum, j), G - 1, G);
    Ltot = __shfl(group_scan<G>(Ltot, j), G - 1, G);
    // sum g w over the blocks behind this one: inclusive scan from the back, read from the next lane
    double v = GW;
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
      const double t = __shfl_down(v, off, G);
      if (j + off < G) v += t;
    }
    v = __shfl_down(v, 1, G);
    GWbehind = j == G - 1 ? 0.0 : v;
  }
  ray_loss_outputs(valid, j, r, Ltot, omega, ray_loss, partial);
  if constexpr (GRAD) {
    const float gs = gscale * omega;
    if (!reached || !(Ctot > 0.0) || gs == 0.0f) return;   // (no c_k, or no weight: the ray's gradient is exactly 0)
    T = Ts;
    double GWrun = 0.0;
    march_block(g, c, rc, k_lo, k_hi, T, [&](const DepthStep& st, const Footprint&, const Cell& cell, float T) {
      DensityTaps tp;
      DensitySample s;
      load_density(g, dens, cell, tp);
      eval_density<true>(g, cell, tp, st.dl(), rc.dnorm, s);
      const float ck = tg.coef(st);
      float gk = 0.0f;
      if (ck != 0.0f) {
        const float w = T * opacity_expm1(s.sigma * s.delta, s.e);
        gk = -ck / (w + eps);
        GWrun += (double)(gk * w);
      }
      // (om == 0: T ends here, every later w is 0 and so is the true suffix; what the subtraction leaves is rounding)
      const double suffix = (st.last || !(s.om > 0.0f)) ? 0.0 : (GWbehind + (GW - GWrun));
      const float dsig = s.delta * (float)((double)(gk * (T * s.e)) - suffix);   // T e = T - w
      const float dv = (dsig * s.dpost) * gs;
      if (dv != 0.0f) deposit_corners(g, tp, d_dens, [&](int q) { return dv * s.t[q]; });   // adding exact zeros is skipped
      return s.om;   // (T ends: every later term is 0)
    });
  }
}

}  // namespace

void launch_depth(const DevGrid& g, const DevCfg& c, const float* dens, const float* rays_o, const float* rays_d,
                  const float* jitter, const float* tdepth, const float* tsigma, const float* rweight, float eps, float grad_scale,
                  float* loss_out, float* ray_loss, float* d_dens, void* scratch, hipStream_t st) {
  const float inv_eps = 1.0f / eps;
  const double neg_log_eps = -log((double)eps);
  launch_ray_loss(c, tl_lane_pins.depth, grad_scale, loss_out, d_dens, scratch, st,
                  [&](auto G, auto GRAD, long long nb, float gscale, double* partial) {
                    depth_kernel<G(), GRAD()><<<(unsigned)nb, kDepthThreads, 0, st>>>(g, c, dens, rays_o, rays_d, jitter, tdepth, tsigma,
                                                                                      rweight, eps, inv_eps, neg_log_eps, gscale,
                                                                                      ray_loss, partial, d_dens);
                  });
}

}  // namespace voxe
