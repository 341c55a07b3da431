// voxe_render.hip -- fused volumetric render kernels for gfx950 (MI355X), forward + backward.
//
// One kernel replaces the reference's sampler -> point processor -> accumulator chain
// (thre3d_atom/rendering/volumetric/render_interface.py:140-171) and never materialises the
// [rays x samples] temporaries; the backward kernel replaces autograd through that chain.
//
// HBM layout: the reference keeps densities [X,Y,Z,1] and features [X,Y,Z,F] as two tensors.  The
// kernels work on a packed array-of-structs copy [X,Y,Z,C], C = F+1, channel order
// (f_0..f_{F-1}, pre(d*scale)) built by the pack kernels of voxe_grid_step.hip (one streaming pass), so a trilinear
// corner is ONE aligned 16-byte load for SH-0 (float4) / 8-byte load for the attention grid, and
// the two z-neighbours of a corner pair are contiguous (32 B).  Gradients are accumulated in the
// same packed layout and split back (with the pre-activation chain rule) by the un-pack kernels there.
#include <stdint.h>
#include <stdlib.h>

#include <math.h>

#include "voxe_device.hpp"
#include "voxe_launch.hpp"
#include "voxe_render_common.hpp"

namespace voxe {

// ------------------------------------------------------------------------------------------------
// Forward
// ------------------------------------------------------------------------------------------------
template <int COUT, int NCM, int NCU>
__global__ __launch_bounds__(256) void render_fwd_kernel(DevGrid g, DevCfg c,
                                                         const float* __restrict__ packed,
                                                         const float* __restrict__ rays_o,
                                                         const float* __restrict__ rays_d,
                                                         const float* __restrict__ jitter,
                                                         float* __restrict__ colour,
                                                         float* __restrict__ depth,
                                                         float* __restrict__ acc,
                                                         float* __restrict__ disparity,
                                                         float* __restrict__ ray_state) {
  long long r;
  if (!map_ray(c, r)) return;
  RayCtx<COUT, NCM, NCU> rc;
  rc.init(g, c, r, rays_o, rays_d, jitter);

  float csum[COUT];
#pragma unroll
  for (int ch = 0; ch < COUT; ++ch) csum[ch] = 0.0f;
  float asum = 0.0f, dsum = 0.0f, T = 1.0f;

  // depth-segment states for the segmented backward: state BEFORE sample b * kSegLen
  const int nbound = ray_state ? num_segments(c.S, c.seg_len) - 1 : 0;
  int nextb = 1;
  auto save_state = [&](int b) {
    constexpr int NC = COUT + 3;
    ray_state[ray_state_index(b, 0, NC, c.R, r)] = T;
#pragma unroll
    for (int ch = 0; ch < COUT; ++ch) ray_state[ray_state_index(b, 1 + ch, NC, c.R, r)] = csum[ch];
    ray_state[ray_state_index(b, 1 + COUT, NC, c.R, r)] = asum;
    ray_state[ray_state_index(b, 2 + COUT, NC, c.R, r)] = dsum;
  };

  if (rc.k_lo <= rc.k_hi) {
    float z_next = rc.dg.z(rc.k_lo);
    for (int k = rc.k_lo; k <= rc.k_hi; ++k) {
      while (nextb <= nbound && nextb * c.seg_len <= k) { save_state(nextb); ++nextb; }
      const float z = z_next;
      const bool last = (k == c.S - 1);
      if (!last) z_next = rc.dg.z(k + 1);
      float p[3];
      rc.point(z, p);
      Footprint fp;
      footprint(g, p, fp);
      if (!fp.inside) continue;  // sigma = 0 -> alpha = 0 -> w = 0, T unchanged (process.py:83)
      Cell cell;
      make_cell_fast(g, fp, cell);
      float v, rad[COUT];
      gather<COUT, NCM, NCU>(g, packed, cell, rc.basis, v, rad);
      const float sigma = post_activate(g.post_act, v);
      // accumulate.py:49-55,63-67
      const float dl = last ? kInfinity : (z_next - z);
      const float delta = dl * rc.dnorm;
      const float e = fast_exp(-(sigma * delta));
      const float alpha = 1.0f - e;
      const float om = 1.0f - alpha;
      const float w = alpha * T;
      T = T * om;
#pragma unroll
      for (int ch = 0; ch < COUT; ++ch) csum[ch] = csum[ch] + sigmoidf(rad[ch]) * w;
      asum = asum + w;
      dsum = dsum + z * w;
    }
  }
  while (nextb <= nbound) { save_state(nextb); ++nextb; }  // boundaries behind the last sample: final state
  // the backward wants SUFFIX sums (what lies at and behind the boundary), see render_fwd_combine_kernel: final - prefix
  // (this single-march forward only runs with early termination or without the segment buffer; the segmented forward
  // sums its suffixes back to front instead)
  for (int b = 1; b <= nbound; ++b) {
    constexpr int NC = COUT + 3;
#pragma unroll
    for (int ch = 0; ch < COUT; ++ch) {
      const long long i = ray_state_index(b, 1 + ch, NC, c.R, r);
      ray_state[i] = csum[ch] - ray_state[i];
    }
    const long long ia = ray_state_index(b, 1 + COUT, NC, c.R, r), id = ray_state_index(b, 2 + COUT, NC, c.R, r);
    ray_state[ia] = asum - ray_state[ia];
    ray_state[id] = dsum - ray_state[id];
  }
  // accumulate.py:77-88
#pragma unroll
  for (int ch = 0; ch < COUT; ++ch) {
    float col = csum[ch];
    if (c.white) {
      float bk = 1.0f - asum;
      if (c.attn) bk = bk * 0.0f;
      col = col + bk;
    }
    if (colour) colour[r * COUT + ch] = col;
  }
  if (depth) depth[r] = dsum;
  if (acc) acc[r] = asum;
  if (disparity) {
    const float q = dsum / asum;
    const float m = (q != q) ? q : (q > kZeroPlus ? q : kZeroPlus);  // torch.maximum keeps NaN
    disparity[r] = 1.0f / m;
  }
}

// ------------------------------------------------------------------------------------------------
// Depth-segmented forward: one 400x400 image is only ~2500 waves, too few to hide the gather latency on
// 1024 SIMDs, and one thread marching all S samples is a long dependent chain.  Compositing is associative:
// segment s (samples [s*kSegLen, (s+1)*kSegLen)) computes, with a LOCAL transmittance starting at 1,
//   Tseg = prod (1 - alpha_k),  csum = sum col_k alpha_k Tloc_k,  asum = sum alpha_k Tloc_k,  dsum = sum z_k alpha_k Tloc_k
// in its own thread (8x more waves), and render_fwd_combine_kernel folds the segments front to back:
//   T_start(s) = prod_{s' < s} Tseg(s'),  colour = sum_s T_start(s) csum(s), ...
// The combine pass also emits the per-ray segment-start states the segmented backward consumes.
// (The forward integrates every sample whatever term_eps says: the switch only truncates gradients, see voxe.h.)
// Tried and measured as nulls (r03, 400x400: 0.246 ms either way): two samples per loop trip with both gathers (16 texel
// loads) in flight before either sample's arithmetic -- the kernel is not short of memory-level parallelism inside a wave;
// fewer registers for more resident waves (launch bounds 6 / 8: 0.284 / 0.438 ms, spills).  PMC: VALU issue 0.47, 3.4 of 5
// possible waves per SIMD resident on average (12 k non-empty one-wave blocks = 2.3 rounds), waves wait 64 % of their time.
// segbuf layout: [segment][component][ray], components (Tseg, csum[COUT], asum, dsum).
// ------------------------------------------------------------------------------------------------
template <int COUT, int NCM, int NCU>
// one-wave blocks (an 8x8 pixel tile each): 2-3 % faster than 256-thread blocks at 400x400, 33 % at 100x100 (finer
// scheduling granularity; the kernel has no block-level cooperation)
#ifndef VOXE_FWD_LB
#define VOXE_FWD_LB 1
#endif
__global__ __launch_bounds__(64, VOXE_FWD_LB) void render_fwd_seg_kernel(DevGrid g, DevCfg c, int fseg,
                                                             const float* __restrict__ packed,
                                                             const float* __restrict__ rays_o,
                                                             const float* __restrict__ rays_d,
                                                             const float* __restrict__ jitter,
                                                             float* __restrict__ segbuf,
                                                             float4* __restrict__ sample_fwd) {
  constexpr int NC = COUT + 3;
  const int nseg = num_segments(c.S, c.seg_len);
  // one thread = `fseg` consecutive depth segments of one ray (fseg = 1: finest split, used for small images)
  const int ncoarse = (nseg + fseg - 1) / fseg;
  // Block order: SEGMENT-MAJOR -- all ray blocks at coarse segment 0, then all at segment 1, ...  The first and last
  // depth segments lie mostly outside the AABB and retire at once; if the segments of one ray block sat on consecutive
  // blocks, "empty" and "full" blocks would alternate with period ncoarse, which aliases with the placement of block b
  // on XCD b % 8 and round-robin on its 32 CUs (see render_bwd_tile_kernel).
  const int nrb = gridDim.x / ncoarse;  // ray blocks (a multiple of 8)
  const int cseg = blockIdx.x / nrb, rb = blockIdx.x - cseg * nrb;
  long long r;
  long long tile_lane = -1;   // (tile * nseg) * seg_len * 64 + lane: base of this lane's slots in sample_fwd (image order only)
  {  // one wave = one 8x8 pixel tile (image order) or 64 consecutive rays
    const int lane = threadIdx.x;
    if (c.image_width > 0) {
      const int W = c.image_width;
      const int ntx = (W + 7) >> 3, nty = (int)tile_rows_total(c, 8);
      const int t = logical_tile_of(c, rb, nrb, ntx, nty);
      if (t < 0) return;
      tile_lane = (long long)t * nseg * c.seg_len * 64 + lane;
      const int ty = t / ntx, tx = t - ty * ntx;
      if (!tile_pixel_ray(c, ty, lane >> 3, (tx << 3) + (lane & 7), 8, r)) return;
    } else {
      const int nt = (int)((c.R + 63) / 64);
      const int t = logical_tile_of(c, rb, nrb, 1, nt);
      if (t < 0) return;
      r = (long long)t * 64 + lane;
      if (r >= c.R) return;
    }
  }
  RayCtx<COUT, NCM, NCU> rc;
  rc.init(g, c, r, rays_o, rays_d, jitter);
  const int s_end = min(nseg, (cseg + 1) * fseg);
  float z_next = 0.0f;
  int z_for = -1;  // sample index z_next belongs to
  for (int seg = cseg * fseg; seg < s_end; ++seg) {
    const int ks = seg * c.seg_len, ke = min(c.S, ks + c.seg_len) - 1;
    const int k_lo = max(rc.k_lo, ks), k_hi = min(rc.k_hi, ke);
    float csum[COUT];
#pragma unroll
    for (int ch = 0; ch < COUT; ++ch) csum[ch] = 0.0f;
    float asum = 0.0f, dsum = 0.0f, T = 1.0f;
    if (k_lo <= k_hi) {
      if (z_for != k_lo) z_next = rc.dg.z(k_lo);
      for (int k = k_lo; k <= k_hi; ++k) {
        const float z = z_next;
        const bool last = (k == c.S - 1);
        if (!last) { z_next = rc.dg.z(k + 1); z_for = k + 1; }
        float p[3];
        rc.point(z, p);
        Footprint fp;
        footprint(g, p, fp);
        if (!fp.inside) continue;
        Cell cell;
        make_cell_fast(g, fp, cell);
        float v, rad[COUT];
        gather<COUT, NCM, NCU>(g, packed, cell, rc.basis, v, rad);
        if constexpr (COUT == 3 && NCU > 1) {
          // slot of (tile, segment, sample k, lane) -- render_bwd_tile_kernel's src_base + k * 64
          if (sample_fwd && tile_lane >= 0)
            sample_fwd[tile_lane + ((long long)seg * c.seg_len + (k - ks)) * 64] = make_float4(rad[0], rad[1], rad[2], v);
        }
        const float sigma = post_activate(g.post_act, v);
        const float dl = last ? kInfinity : (z_next - z);
        const float delta = dl * rc.dnorm;
        const float e = fast_exp(-(sigma * delta));
        const float alpha = 1.0f - e;
        const float om = 1.0f - alpha;
        const float w = alpha * T;
        T = T * om;
#pragma unroll
        for (int ch = 0; ch < COUT; ++ch) csum[ch] = fmaf(sigmoidf(rad[ch]), w, csum[ch]);
        asum = asum + w;
        dsum = fmaf(z, w, dsum);
      }
    }
    const long long base = (long long)seg * NC;
    segbuf[(base + 0) * c.R + r] = T;
#pragma unroll
    for (int ch = 0; ch < COUT; ++ch) segbuf[(base + 1 + ch) * c.R + r] = csum[ch];
    segbuf[(base + 1 + COUT) * c.R + r] = asum;
    segbuf[(base + 2 + COUT) * c.R + r] = dsum;
  }
}

template <int COUT>
__global__ __launch_bounds__(256) void render_fwd_combine_kernel(DevCfg c, const float* __restrict__ segbuf,
                                                                 float* __restrict__ colour,
                                                                 float* __restrict__ depth,
                                                                 float* __restrict__ acc,
                                                                 float* __restrict__ disparity,
                                                                 float* __restrict__ ray_state) {
  constexpr int NC = COUT + 3;
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= c.R) return;
  const int nseg = num_segments(c.S, c.seg_len);
  float csum[COUT];
#pragma unroll
  for (int ch = 0; ch < COUT; ++ch) csum[ch] = 0.0f;
  float asum = 0.0f, dsum = 0.0f, T = 1.0f;
  for (int s = 0; s < nseg; ++s) {
    if (ray_state && s > 0) ray_state[ray_state_index(s, 0, NC, c.R, r)] = T;   // transmittance BEFORE segment s == boundary s
    const long long base = (long long)s * NC;
#pragma unroll
    for (int ch = 0; ch < COUT; ++ch) csum[ch] = fmaf(T, segbuf[(base + 1 + ch) * c.R + r], csum[ch]);
    asum = fmaf(T, segbuf[(base + 1 + COUT) * c.R + r], asum);
    dsum = fmaf(T, segbuf[(base + 2 + COUT) * c.R + r], dsum);
    T = T * segbuf[(base + 0) * c.R + r];
  }
  if (ray_state) {
    // State of boundary s for the backward: transmittance before it and the SUFFIX sums -- what the samples at and
    // behind the boundary contribute to (csum, asum, dsum) -- summed BACK TO FRONT (faint far segments first).  The
    // backward needs sum_{j > k} dL/dw_j w_j; taking it as (whole ray) - (prefix) loses the samples deep inside a dense
    // medium to cancellation (relative error 1e-7 / T_k); suffix sums keep it relative to the suffix itself, like the
    // reference's reverse cumsum (torch's cumprod backward; rendering/volumetric/accumulate.py:63-67).
    float sc[COUT], sa = 0.0f, sd = 0.0f;
#pragma unroll
    for (int ch = 0; ch < COUT; ++ch) sc[ch] = 0.0f;
    for (int s = nseg - 1; s > 0; --s) {
      const float Ts = ray_state[ray_state_index(s, 0, NC, c.R, r)];   // (written by this thread above)
      const long long base = (long long)s * NC;
#pragma unroll
      for (int ch = 0; ch < COUT; ++ch) {
        sc[ch] = fmaf(Ts, segbuf[(base + 1 + ch) * c.R + r], sc[ch]);
        ray_state[ray_state_index(s, 1 + ch, NC, c.R, r)] = sc[ch];
      }
      sa = fmaf(Ts, segbuf[(base + 1 + COUT) * c.R + r], sa);
      sd = fmaf(Ts, segbuf[(base + 2 + COUT) * c.R + r], sd);
      ray_state[ray_state_index(s, 1 + COUT, NC, c.R, r)] = sa;
      ray_state[ray_state_index(s, 2 + COUT, NC, c.R, r)] = sd;
    }
  }
#pragma unroll
  for (int ch = 0; ch < COUT; ++ch) {
    float col = csum[ch];
    if (c.white) {
      float bk = 1.0f - asum;
      if (c.attn) bk = bk * 0.0f;
      col = col + bk;
    }
    if (colour) colour[r * COUT + ch] = col;
  }
  if (depth) depth[r] = dsum;
  if (acc) acc[r] = asum;
  if (disparity) {
    const float q = dsum / asum;
    const float m = (q != q) ? q : (q > kZeroPlus ? q : kZeroPlus);
    disparity[r] = 1.0f / m;
  }
}

// r06: the same pass for at most MAXSEG depth segments with every partial in registers.  The kernel above re-reads, in its
// back-to-front loop, the transmittances it has just stored (a store -> load round trip through memory per boundary, which the
// compiler may not reorder: ~13 us for ANY number of rays, launch-latency scale work turned into seven dependent memory trips --
// kernel timeline, profiles/r06_bench_trace.txt).  Here all loads are issued up front (independent), the boundary transmittances
// stay in registers, and the stores are fire-and-forget: the same products and sums in the same order, bit-identical outputs.
template <int COUT, int MAXSEG>
__global__ __launch_bounds__(256) void render_fwd_combine_reg_kernel(DevCfg c, const float* __restrict__ segbuf,
                                                                     float* __restrict__ colour, float* __restrict__ depth,
                                                                     float* __restrict__ acc, float* __restrict__ disparity,
                                                                     float* __restrict__ ray_state) {
  constexpr int NC = COUT + 3;
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= c.R) return;
  const int nseg = num_segments(c.S, c.seg_len);     // <= MAXSEG (host)
  float part[MAXSEG][NC];
#pragma unroll
  for (int s = 0; s < MAXSEG; ++s)
#pragma unroll
    for (int q = 0; q < NC; ++q) part[s][q] = (s < nseg) ? segbuf[((long long)s * NC + q) * c.R + r] : 0.0f;
  float csum[COUT];
#pragma unroll
  for (int ch = 0; ch < COUT; ++ch) csum[ch] = 0.0f;
  float asum = 0.0f, dsum = 0.0f, T = 1.0f;
  float Tb[MAXSEG];                                   // transmittance BEFORE segment s == boundary s
#pragma unroll
  for (int s = 0; s < MAXSEG; ++s) {
    Tb[s] = T;
    if (s < nseg) {
#pragma unroll
      for (int ch = 0; ch < COUT; ++ch) csum[ch] = fmaf(T, part[s][1 + ch], csum[ch]);
      asum = fmaf(T, part[s][1 + COUT], asum);
      dsum = fmaf(T, part[s][2 + COUT], dsum);
      T = T * part[s][0];
    }
  }
  if (ray_state) {
    float sc[COUT], sa = 0.0f, sd = 0.0f;
#pragma unroll
    for (int ch = 0; ch < COUT; ++ch) sc[ch] = 0.0f;
#pragma unroll
    for (int s = MAXSEG - 1; s > 0; --s) {
      if (s < nseg) {
        const float Ts = Tb[s];
        ray_state[ray_state_index(s, 0, NC, c.R, r)] = Ts;
#pragma unroll
        for (int ch = 0; ch < COUT; ++ch) {
          sc[ch] = fmaf(Ts, part[s][1 + ch], sc[ch]);
          ray_state[ray_state_index(s, 1 + ch, NC, c.R, r)] = sc[ch];
        }
        sa = fmaf(Ts, part[s][1 + COUT], sa);
        sd = fmaf(Ts, part[s][2 + COUT], sd);
        ray_state[ray_state_index(s, 1 + COUT, NC, c.R, r)] = sa;
        ray_state[ray_state_index(s, 2 + COUT, NC, c.R, r)] = sd;
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < COUT; ++ch) {
    float col = csum[ch];
    if (c.white) {
      float bk = 1.0f - asum;
      if (c.attn) bk = bk * 0.0f;
      col = col + bk;
    }
    if (colour) colour[r * COUT + ch] = col;
  }
  if (depth) depth[r] = dsum;
  if (acc) acc[r] = asum;
  if (disparity) {
    const float q = dsum / asum;
    const float m = (q != q) ? q : (q > kZeroPlus ? q : kZeroPlus);
    disparity[r] = 1.0f / m;
  }
}

// ------------------------------------------------------------------------------------------------
// Backward: recompute the march, turn (d_colour, d_depth, d_acc) into per-sample gradients with the
// prefix/total form of the suffix sum, scatter-add to the packed gradient grid.
//   dL/dw_k    = sum_c g_c col_kc - [white & !attn] sum_c g_c + g_depth z_k + g_acc
//   dL/dsig_k  = delta_k e_k (T_k dL/dw_k - (sum_{j>k} dL/dw_j w_j) / om_k)
//   dL/drad_kc = w_k g_c col_kc (1 - col_kc)
// ------------------------------------------------------------------------------------------------
template <int COUT, int NCM, int NCU, bool WANT_D, bool WANT_F>
__global__ __launch_bounds__(256) void render_bwd_kernel(
    DevGrid g, DevCfg c, const float* __restrict__ packed, const float* __restrict__ rays_o,
    const float* __restrict__ rays_d, const float* __restrict__ jitter,
    const float* __restrict__ colour, const float* __restrict__ depth,
    const float* __restrict__ acc, const float* __restrict__ d_colour,
    const float* __restrict__ d_depth, const float* __restrict__ d_acc,
    float* __restrict__ gpacked) {
  constexpr int C = COUT * NCM + 1;
  long long r;
  if (!map_ray(c, r)) return;
  RayCtx<COUT, NCM, NCU> rc;
  rc.init(g, c, r, rays_o, rays_d, jitter);
  if (rc.k_lo > rc.k_hi) return;

  float gc[COUT], gsum = 0.0f;
#pragma unroll
  for (int ch = 0; ch < COUT; ++ch) { gc[ch] = d_colour[r * COUT + ch]; gsum += gc[ch]; }
  const float gdep = d_depth ? d_depth[r] : 0.0f;
  const float gacc = d_acc ? d_acc[r] : 0.0f;
  const bool white = c.white && !c.attn;
  const float asum = acc[r];
  // total = sum_j dL/dw_j w_j from the forward outputs
  float total = gdep * depth[r] + gacc * asum;
#pragma unroll
  for (int ch = 0; ch < COUT; ++ch) {
    const float csum = white ? colour[r * COUT + ch] - (1.0f - asum) : colour[r * COUT + ch];
    total += gc[ch] * csum;
  }
  if (white) total -= gsum * asum;

  float prefix = 0.0f, T = 1.0f;
  int k_sat = -1;      // first saturated interior sample of the ray (om == 0, e != 0), and T in front of it
  float T_sat = 0.0f;
  float z_next = rc.dg.z(rc.k_lo);
  for (int k = rc.k_lo; k <= rc.k_hi; ++k) {
    const float z = z_next;
    const bool last = (k == c.S - 1);
    if (!last) z_next = rc.dg.z(k + 1);
    float p[3];
    rc.point(z, p);
    Footprint fp;
    footprint(g, p, fp);
    if (!fp.inside) continue;
    Cell cell;
    make_cell_fast(g, fp, cell);
    float v, rad[COUT];
    gather<COUT, NCM, NCU>(g, packed, cell, rc.basis, v, rad);
    float sigma, dpost;
    post_activate_vg(g.post_act, v, sigma, dpost);
    const float dl = last ? kInfinity : (z_next - z);
    const float delta = dl * rc.dnorm;
    const float e = fast_exp(-(sigma * delta));
    const float alpha = 1.0f - e;
    const float om = 1.0f - alpha;
    const float w = alpha * T;

    float col[COUT], dldw = gdep * z + gacc;
#pragma unroll
    for (int ch = 0; ch < COUT; ++ch) { col[ch] = sigmoidf(rad[ch]); dldw += gc[ch] * col[ch]; }
    if (white) dldw -= gsum;
    prefix += dldw * w;
    const float suffix = last ? 0.0f : (total - prefix);
    const float tail = (om > 0.0f) ? suffix / om : 0.0f;
    if (WANT_D && om == 0.0f && e != 0.0f && !last && k_sat < 0) { k_sat = k; T_sat = T; }   // (see saturated_correction())
    const float dsig = (delta * e) * (T * dldw - tail);
    const float dv = dsig * dpost;
    float drad[COUT];
    bool any = (dv != 0.0f);
#pragma unroll
    for (int ch = 0; ch < COUT; ++ch) {
      drad[ch] = (w * gc[ch]) * (col[ch] * (1.0f - col[ch]));
      any = any || (drad[ch] != 0.0f);
    }
    T = T * om;

    if (any) {  // adding exact zeros is skipped
      const CellAddr ad = cell_addr(g, cell);
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const float wg = (cell.w[0][kk & 1] * cell.w[1][(kk >> 1) & 1]) * cell.w[2][kk >> 2];
        if (wg != 0.0f) {
          float* __restrict__ dst =
              gpacked + (long long)(ad.base + (kk & 1) * ad.sx + ((kk >> 1) & 1) * ad.sy + (kk >> 2) * ad.sz) * C;
          if constexpr (WANT_F) {
#pragma unroll
            for (int ch = 0; ch < COUT; ++ch)
#pragma unroll
              for (int j = 0; j < NCU; ++j)
                atomicAdd(dst + ch * NCM + j, (drad[ch] * rc.basis[j]) * wg);
          }
          if constexpr (WANT_D) atomicAdd(dst + (C - 1), dv * wg);
        }
      }
    }
    if (c.term_eps > 0.0f && T < c.term_eps) break;
  }
  if constexpr (WANT_D) {
    if (k_sat >= 0) {   // rare: the tail the `suffix / om` form lost at a saturated interior sample, after the march
      UpstreamColour u = {{0.0f, 0.0f, 0.0f}};
#pragma unroll
      for (int ch = 0; ch < COUT; ++ch) u.v[ch] = gc[ch];
      Cell cell;
      const float dv = saturated_correction<COUT, NCM, NCU>(g, c, packed, rc, k_sat, T_sat, u, gsum, gdep, gacc, white, cell);
      if (dv != 0.0f) {
        const CellAddr ad = cell_addr(g, cell);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          const float wg = (cell.w[0][kk & 1] * cell.w[1][(kk >> 1) & 1]) * cell.w[2][kk >> 2];
          if (wg != 0.0f)
            atomicAdd(gpacked + (long long)(ad.base + (kk & 1) * ad.sx + ((kk >> 1) & 1) * ad.sy + (kk >> 2) * ad.sz) * C + (C - 1), dv * wg);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Probe: per-sample index / mask / depth / sigma / radiance (test hook, shares all device code)
// ------------------------------------------------------------------------------------------------
template <int COUT, int NCM, int NCU>
__global__ __launch_bounds__(256) void sample_probe_kernel(
    DevGrid g, DevCfg c, const float* __restrict__ packed, const float* __restrict__ rays_o,
    const float* __restrict__ rays_d, const float* __restrict__ jitter, int32_t* __restrict__ idx,
    uint8_t* __restrict__ inside, float* __restrict__ zvals, float* __restrict__ sigma,
    float* __restrict__ radv) {
  long long r;
  if (!map_ray(c, r)) return;
  RayCtx<COUT, NCM, NCU> rc;
  rc.init(g, c, r, rays_o, rays_d, jitter);
  for (int k = 0; k < c.S; ++k) {
    const float z = rc.dg.z(k);
    float p[3];
    rc.point(z, p);
    Footprint fp;
    footprint(g, p, fp);
    const long long i = r * c.S + k;
    if (idx) { idx[3 * i + 0] = fp.i0[0]; idx[3 * i + 1] = fp.i0[1]; idx[3 * i + 2] = fp.i0[2]; }
    if (inside) inside[i] = fp.inside ? 1 : 0;
    if (zvals) zvals[i] = z;
    float v = 0.0f, rad[COUT];
#pragma unroll
    for (int ch = 0; ch < COUT; ++ch) rad[ch] = -kInfinity;  // process.py:80-82
    float sg = 0.0f;
    // the renderer only evaluates samples of [k_lo, k_hi]; the probe reports the same decision
    if (fp.inside && k >= rc.k_lo && k <= rc.k_hi) {
      Cell cell;
      make_cell(g, fp, cell);
      gather<COUT, NCM, NCU>(g, packed, cell, rc.basis, v, rad);
      sg = post_activate(g.post_act, v);
    }
    if (sigma) sigma[i] = sg;
    if (radv) {
#pragma unroll
      for (int ch = 0; ch < COUT; ++ch) radv[i * COUT + ch] = rad[ch];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Point query: VoxelGrid.forward / forward_attn (voxels.py:287-406), un-masked, + its backward.
// One thread per point; same footprint / cell code as the renderer (indices bit-exact by construction).
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void query_fwd_kernel(DevGrid g, const float* __restrict__ packed,
                                                        const float* __restrict__ points, long long N,
                                                        float* __restrict__ out) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float p[3] = {points[3 * n], points[3 * n + 1], points[3 * n + 2]};
  Footprint fp;
  footprint(g, p, fp);
  Cell cell;
  make_cell(g, fp, cell);
  const CellAddr ad = cell_addr(g, cell);
  float acc[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float w = (cell.w[0][k & 1] * cell.w[1][(k >> 1) & 1]) * cell.w[2][k >> 2];
    const float* __restrict__ src = packed + (long long)(ad.base + (k & 1) * ad.sx + ((k >> 1) & 1) * ad.sy + (k >> 2) * ad.sz) * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = fmaf(src[ch], w, acc[ch]);
  }
  acc[C - 1] = post_activate(g.post_act, acc[C - 1]);
#pragma unroll
  for (int ch = 0; ch < C; ++ch) out[n * C + ch] = acc[ch];
}

template <int C>
__global__ __launch_bounds__(256) void query_bwd_kernel(DevGrid g, const float* __restrict__ packed,
                                                        const float* __restrict__ points, long long N,
                                                        const float* __restrict__ d_out,
                                                        float* __restrict__ gpacked, int want_d, int want_f) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float p[3] = {points[3 * n], points[3 * n + 1], points[3 * n + 2]};
  Footprint fp;
  footprint(g, p, fp);
  Cell cell;
  make_cell(g, fp, cell);
  const CellAddr ad = cell_addr(g, cell);
  float v = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float w = (cell.w[0][k & 1] * cell.w[1][(k >> 1) & 1]) * cell.w[2][k >> 2];
    v = fmaf(packed[(long long)(ad.base + (k & 1) * ad.sx + ((k >> 1) & 1) * ad.sy + (k >> 2) * ad.sz) * C + (C - 1)], w, v);
  }
  float value, dpost;
  post_activate_vg(g.post_act, v, value, dpost);
  const float dv = d_out[n * C + (C - 1)] * dpost;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float w = (cell.w[0][k & 1] * cell.w[1][(k >> 1) & 1]) * cell.w[2][k >> 2];
    if (w != 0.0f) {
      float* __restrict__ dst = gpacked + (long long)(ad.base + (k & 1) * ad.sx + ((k >> 1) & 1) * ad.sy + (k >> 2) * ad.sz) * C;
      if (want_f) {
#pragma unroll
        for (int ch = 0; ch < C - 1; ++ch) atomicAdd(dst + ch, d_out[n * C + ch] * w);
      }
      if (want_d) atomicAdd(dst + (C - 1), dv * w);
    }
  }
}

template <int C>
static void launch_query_t(const DevGrid& g, const float* packed, const float* points, long long N, float* out,
                           const float* d_out, float* gpacked, bool want_d, bool want_f, hipStream_t st) {
  const int nb = (int)((N + 255) / 256);
  if (out) query_fwd_kernel<C><<<nb, 256, 0, st>>>(g, packed, points, N, out);
  else query_bwd_kernel<C><<<nb, 256, 0, st>>>(g, packed, points, N, d_out, gpacked, want_d, want_f);
}

void launch_query(const DevGrid& g, int C, const float* packed, const float* points, long long N, float* out,
                  const float* d_out, float* gpacked, bool want_d, bool want_f, hipStream_t st) {
  switch (C) {
    case 2: launch_query_t<2>(g, packed, points, N, out, d_out, gpacked, want_d, want_f, st); break;
    case 4: launch_query_t<4>(g, packed, points, N, out, d_out, gpacked, want_d, want_f, st); break;
    case 13: launch_query_t<13>(g, packed, points, N, out, d_out, gpacked, want_d, want_f, st); break;
    case 28: launch_query_t<28>(g, packed, points, N, out, d_out, gpacked, want_d, want_f, st); break;
    case 49: launch_query_t<49>(g, packed, points, N, out, d_out, gpacked, want_d, want_f, st); break;
  }
}

// ------------------------------------------------------------------------------------------------
// Host-side launchers (called from voxe_api.hip)
// ------------------------------------------------------------------------------------------------
static inline int blocks_for(const DevCfg& c) {
  if (c.image_width > 0) {
    return blocks_for_tiles(c.map_mode, (c.image_width + 15) / 16, tile_rows_total(c, 16));
  }
  return blocks_for_tiles(c.map_mode, 1, (c.R + 255) / 256);
}

template <int COUT, int NCM, int NCU>
static void launch_fwd_t(const DevGrid& g, const HostCfg& c, const FwdArgs& a, hipStream_t st) {
  const int nseg = num_segments(c.S, c.seg_len);
  // The march of every ray block is split into depth segments handled by different blocks (a 100x100 image alone
  // is 40 blocks; at 400x400 the finer split hides the gather latency better): with the segment-major block order
  // one 32-sample segment per task is fastest at every image size (400x400, mean of three cameras: fseg 1 / 2 / 4 / 8
  // = 0.273 / 0.286 / 0.291 / 0.326 ms).
  // (term_eps never changes a forward -- since r03 it only truncates the BACKWARD: samples behind a transmittance below
  //  it receive no gradient -- so the segmented forward runs whatever its value)
  if (a.segbuf && nseg > 1) {
    const int fseg = c.disp.fwd_segments_per_thread > 0 ? c.disp.fwd_segments_per_thread : 1;
    const int ncoarse = (nseg + fseg - 1) / fseg;
    const int nrb64 = c.image_width > 0
                          ? blocks_for_tiles(c.map_mode, (c.image_width + 7) / 8, tile_rows_total(c, 8))
                          : blocks_for_tiles(c.map_mode, 1, (c.R + 63) / 64);
    if (NCU == 1 && fseg == 1 && fwd_tile4_supported(g, c, a, COUT, NCM))
      launch_fwd_tile4(g, c, a, st);     // r05: the lean tile-ordered forward (voxe_render_tile4.hip)
    else if (NCU == 1 && fseg == 1 && fwd_tile_supported(g, c, COUT, NCM))
      launch_fwd_tile(g, c, a, st);      // texels of a tile staged in LDS (voxe_render_tile.hip)
    else if (NCU > 1 && fseg == 1 && fwd_tilew_supported(g, c, a, COUT, NCM, NCU))
      launch_fwd_tilew(g, c, NCM, a, st);   // r06: whole view-dependent texels of a tile staged in LDS (voxe_render_tilew.hip)
    else
      render_fwd_seg_kernel<COUT, NCM, NCU><<<nrb64 * ncoarse, 64, 0, st>>>(
          g, c, fseg, a.packed, a.rays_o, a.rays_d, a.jitter, a.segbuf, reinterpret_cast<float4*>(a.sample_fwd));
#ifndef VOXE_COMBINE_REG
#define VOXE_COMBINE_REG 1
#endif
    const int cb = (int)((c.R + 255) / 256);
    if (VOXE_COMBINE_REG && nseg <= 8)
      render_fwd_combine_reg_kernel<COUT, 8><<<cb, 256, 0, st>>>(c, a.segbuf, a.colour, a.depth, a.acc, a.disparity, a.ray_state);
    else if (VOXE_COMBINE_REG && nseg <= 16)
      render_fwd_combine_reg_kernel<COUT, 16><<<cb, 256, 0, st>>>(c, a.segbuf, a.colour, a.depth, a.acc, a.disparity, a.ray_state);
    else
      render_fwd_combine_kernel<COUT><<<cb, 256, 0, st>>>(c, a.segbuf, a.colour, a.depth, a.acc, a.disparity, a.ray_state);
    return;
  }
  render_fwd_kernel<COUT, NCM, NCU><<<blocks_for(c), 256, 0, st>>>(
      g, c, a.packed, a.rays_o, a.rays_d, a.jitter, a.colour, a.depth, a.acc, a.disparity, a.ray_state);
}

template <int COUT, int NCM, int NCU>
static void launch_bwd_t(const DevGrid& g, const DevCfg& c, const BwdArgs& a, hipStream_t st) {
  const int nb = blocks_for(c);
#define VOXE_BWD(WD, WF)                                                                         \
  render_bwd_kernel<COUT, NCM, NCU, WD, WF><<<nb, 256, 0, st>>>(                                 \
      g, c, a.packed, a.rays_o, a.rays_d, a.jitter, a.colour, a.depth, a.acc, a.d_colour,        \
      a.d_depth, a.d_acc, a.gpacked)
  if (a.want_d && a.want_f) VOXE_BWD(true, true);
  else if (a.want_d) VOXE_BWD(true, false);
  else VOXE_BWD(false, true);
#undef VOXE_BWD
}

template <int COUT, int NCM, int NCU>
static void launch_probe_t(const DevGrid& g, const DevCfg& c, const ProbeArgs& a, hipStream_t st) {
  sample_probe_kernel<COUT, NCM, NCU><<<blocks_for(c), 256, 0, st>>>(
      g, c, a.packed, a.rays_o, a.rays_d, a.jitter, a.idx, a.inside, a.zvals, a.sigma, a.rad);
}

// variant dispatch on (feature kind, SH degree, diffuse)
#define VOXE_DISPATCH(FN, attn, deg, diffuse, ...)                        \
  do {                                                                    \
    if (attn) { FN<1, 1, 1>(__VA_ARGS__); }                               \
    else if ((deg) == 0) { FN<3, 1, 1>(__VA_ARGS__); }                    \
    else if ((deg) == 1) { if (diffuse) FN<3, 4, 1>(__VA_ARGS__); else FN<3, 4, 4>(__VA_ARGS__); }    \
    else if ((deg) == 2) { if (diffuse) FN<3, 9, 1>(__VA_ARGS__); else FN<3, 9, 9>(__VA_ARGS__); }    \
    else { if (diffuse) FN<3, 16, 1>(__VA_ARGS__); else FN<3, 16, 16>(__VA_ARGS__); }                 \
  } while (0)

void launch_fwd(const DevGrid& g, const HostCfg& c, int deg, int diffuse, const FwdArgs& a,
                hipStream_t st) {
  VOXE_DISPATCH(launch_fwd_t, c.attn, deg, diffuse, g, c, a, st);
}
void launch_bwd(const DevGrid& g, const DevCfg& c, int deg, int diffuse, const BwdArgs& a,
                hipStream_t st) {
  VOXE_DISPATCH(launch_bwd_t, c.attn, deg, diffuse, g, c, a, st);
}
void launch_probe(const DevGrid& g, const DevCfg& c, int deg, int diffuse, const ProbeArgs& a,
                  hipStream_t st) {
  VOXE_DISPATCH(launch_probe_t, c.attn, deg, diffuse, g, c, a, st);
}

}  // namespace voxe
