// voxe_render_rays_bwd.hip -- gradient of a render with respect to its rays ("Ray gradients").
//
// Per ray, with the forward's exact samples (the depth step, sample cell and tail of voxe_ray_march.hpp; the corner loop is this
// file's own interp_cell, which blends the raw feature texels and the slopes along with the density, and the two loops are
// written out: handed to march_block as lambdas, the SH-0 kernels are scheduled differently and lose 5 - 9 %) and the
// upstream gradients g_col [3], g_depth, g_acc of the ray's outputs:
//   q_k = g_col . rad_k + g_depth z_k + g_acc - (white ? sum_c g_col_c : 0)        (dL/dw_k, w_k = T_k alpha_k)
//   E_k = q_k (T_k - w_k) - sum_{i>k} w_i q_i
//   dL/dsigma_k = delta_k E_k,   dL/ddelta_k = sigma_k E_k                           (delta_k = dl_k |d|, last dl = 1e10)
//   dL/dp_k = delta_k E_k post'(v_k) grad v(p_k) + w_k sum_c g_col_c rad_kc (1 - rad_kc) grad x_c(p_k),  rad = sigmoid(x)
//   d_o = sum_k dL/dp_k
//   d_d = sum_k z_k dL/dp_k + (sum_k sigma_k E_k dl_k) d/|d| + Jn^T (dB/dv)^T m,   m_j = sum_k w_k sum_c s_kc F_cj(p_k)
// with s_kc = g_col_c rad_kc (1 - rad_kc), F_cj the interpolated SH coefficients, Jn = (I - v v^T) / |d|, v = d / |d|.  grad of
// an interpolant is its slope inside the cell floor(u) the forward used, zero padding included (slope_coefs of voxe_ray_march.hpp),
// in world units.  The sample depths are constants (no gradient through near / far / the aabb_clip bounds).
//
// The slope is linear in the corner values, so the corner loop keeps, per sample, the value and the three slopes of v and of the
// three x_c (16 accumulators) with every corner contracted with the SH basis first (gather<>()'s re-association): no per-corner
// value stays live, and the loop over the corners can stay rolled for the wide texels.  m_j takes a second pass over the corners
// (L2-resident texels) once s_kc is known.
//
// G consecutive lanes share a ray (G in {1, 2, 4, 8}, lanes_per_ray(); WaveRectTile, lane_block and group_exclusive_product of
// voxe_ray_march.hpp); lane j owns the j-th contiguous block of the ray's S samples.
//   march 1 : the block with a local T = 1: its transmittance product and Q = sum w~ q.
//   scans   : T_s = exclusive product of the block transmittances; prefix of sum w q = exclusive sum of T_s Q; total.
//   march 2 : the block again with the true T; per sample the suffix is total - (inclusive prefix); the 3 + 3 + 1 sums of the
//             ray (double) and m_j (float), then a group reduction and ONE lane writes the ray's 6 outputs: no atomics, the
//             same bits on every run for a fixed G.
#include <hip/hip_runtime.h>

#include "voxe_launch.hpp"
#include "voxe_ray_march.hpp"

namespace voxe {
namespace {

constexpr int kRayThreads = kMarchThreads;

struct RayBwdArgs {
  const float *dens, *feat, *rays_o, *rays_d, *jitter;
  const float *g_col, *g_depth, *g_acc;
  float *d_o, *d_d;
  int accumulate;
  int ncm;   // SH coefficients per colour channel in memory (F / 3)
};

// value (index 0) and slope along x, y, z in index units (1 .. 3) of the interpolated density and pre-sigmoid radiance
struct Interp {
  float v[4];
  float x[3][4];
};

// One pass over the 8 corners of a cell: every corner's texel is contracted with the SH basis, then blended with the value
// weight t = (wx * wy) * wz (the forward's product and corner order) and, when SLOPE, with the three slope weights.
template <int NCU, bool SLOPE>
__device__ __forceinline__ void interp_cell(const DevGrid& g, const RayBwdArgs& a, const Footprint& fp, const Cell& cell,
                                            const float (&basis)[NCU], Interp& out) {
  const CellAddr ad = cell_addr(g, cell);
  const int ncm = NCU > 1 ? NCU : a.ncm;
  const int F = 3 * ncm;
  float sl[3][2];
  if constexpr (SLOPE) {
    const int N[3] = {g.X, g.Y, g.Z};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) slope_coefs(fp.i0[ax], N[ax], sl[ax][0], sl[ax][1]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    out.v[i] = 0.0f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out.x[ch][i] = 0.0f;
  }
  // corners in flight at once (gather<>(): all 8 would be 8 x 48 loaded values at degree 3)
  constexpr int kCornersInFlight = NCU > 9 ? 1 : (NCU > 4 ? 2 : (NCU > 1 ? 4 : 8));
#pragma unroll kCornersInFlight
  for (int k = 0; k < 8; ++k) {
    // (selects, not array indexing: k is a run-time value in the partially unrolled loop)
    const bool bx = k & 1, by = k & 2, bz = k & 4;
    const float wx = bx ? cell.w[0][1] : cell.w[0][0], wy = by ? cell.w[1][1] : cell.w[1][0], wz = bz ? cell.w[2][1] : cell.w[2][0];
    float w[4];
    w[0] = (wx * wy) * wz;
    if constexpr (SLOPE) {
      const float sx = bx ? sl[0][1] : sl[0][0], sy = by ? sl[1][1] : sl[1][0], sz = bz ? sl[2][1] : sl[2][0];
      w[1] = (sx * wy) * wz;
      w[2] = (wx * sy) * wz;
      w[3] = (wx * wy) * sz;
    }
    const unsigned idx = ad.base + (bx ? ad.sx : 0u) + (by ? ad.sy : 0u) + (bz ? ad.sz : 0u);
    const float cv = pre_activate(g.pre_act, a.dens[idx], g.density_scale);
    const float* __restrict__ src = a.feat + (long long)idx * F;
    float r[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      r[ch] = basis[0] * src[ch * ncm];
#pragma unroll
      for (int j = 1; j < NCU; ++j) r[ch] = fmaf(basis[j], src[ch * ncm + j], r[ch]);
    }
#pragma unroll
    for (int i = 0; i < (SLOPE ? 4 : 1); ++i) {
      out.v[i] = fmaf(cv, w[i], out.v[i]);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) out.x[ch][i] = fmaf(r[ch], w[i], out.x[ch][i]);
    }
  }
}

// m_j += sum over the corners of t * sum_c s_c f_cj  (j >= 1; B_0 does not depend on the direction)
template <int NCU>
__device__ __forceinline__ void basis_moments(const DevGrid& g, const RayBwdArgs& a, const Cell& cell, const float (&s)[3],
                                              float (&m)[NCU]) {
  const CellAddr ad = cell_addr(g, cell);
  constexpr int F = 3 * NCU;
  constexpr int kCornersInFlight = NCU > 9 ? 1 : (NCU > 4 ? 2 : (NCU > 1 ? 4 : 8));
#pragma unroll kCornersInFlight
  for (int k = 0; k < 8; ++k) {
    const bool bx = k & 1, by = k & 2, bz = k & 4;
    const float wx = bx ? cell.w[0][1] : cell.w[0][0], wy = by ? cell.w[1][1] : cell.w[1][0], wz = bz ? cell.w[2][1] : cell.w[2][0];
    const float t = (wx * wy) * wz;
    const unsigned idx = ad.base + (bx ? ad.sx : 0u) + (by ? ad.sy : 0u) + (bz ? ad.sz : 0u);
    const float* __restrict__ src = a.feat + (long long)idx * F;
    const float ts[3] = {t * s[0], t * s[1], t * s[2]};
#pragma unroll
    for (int j = 1; j < NCU; ++j) m[j] = fmaf(ts[2], src[2 * NCU + j], fmaf(ts[1], src[NCU + j], fmaf(ts[0], src[j], m[j])));
  }
}

// u = sum_j m_j dB_j/dv at the unit direction v: the derivative of sh_basis()'s polynomials in (x, y, z)
template <int NC>
__device__ __forceinline__ void sh_basis_vjp(const float (&v)[3], const float (&m)[NC], float (&u)[3]) {
  u[0] = u[1] = u[2] = 0.0f;
  if constexpr (NC > 1) {
    const float x = v[0], y = v[1], z = v[2];
    constexpr float C1 = 0.4886025119029199f;
    u[1] -= C1 * m[1];
    u[2] += C1 * m[2];
    u[0] -= C1 * m[3];
    if constexpr (NC > 4) {
      constexpr float C4 = 1.0925484305920792f, C6 = 0.31539156525252005f, C8 = 0.5462742152960396f;
      u[0] += m[4] * (C4 * y) + m[6] * (-2.0f * C6 * x) + m[7] * (-C4 * z) + m[8] * (2.0f * C8 * x);
      u[1] += m[4] * (C4 * x) + m[5] * (-C4 * z) + m[6] * (-2.0f * C6 * y) + m[8] * (-2.0f * C8 * y);
      u[2] += m[5] * (-C4 * y) + m[6] * (4.0f * C6 * z) + m[7] * (-C4 * x);
      if constexpr (NC > 9) {
        constexpr float C9 = 0.5900435899266435f, C10 = 2.890611442640554f, C11 = 0.4570457994644658f,
                        C12 = 0.3731763325901154f, C14 = 1.445305721320277f;
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        u[0] += m[9] * (-6.0f * C9 * xy) + m[10] * (C10 * yz) + m[11] * (2.0f * C11 * xy) + m[12] * (-6.0f * C12 * xz) +
                m[13] * (-C11 * (4.0f * zz - 3.0f * xx - yy)) + m[14] * (2.0f * C14 * xz) + m[15] * (-3.0f * C9 * (xx - yy));
        u[1] += m[9] * (-3.0f * C9 * (xx - yy)) + m[10] * (C10 * xz) + m[11] * (-C11 * (4.0f * zz - xx - 3.0f * yy)) +
                m[12] * (-6.0f * C12 * yz) + m[13] * (2.0f * C11 * xy) + m[14] * (-2.0f * C14 * yz) + m[15] * (6.0f * C9 * xy);
        u[2] += m[10] * (C10 * xy) + m[11] * (-8.0f * C11 * yz) + m[12] * (3.0f * C12 * (2.0f * zz - xx - yy)) +
                m[13] * (-8.0f * C11 * xz) + m[14] * (C14 * (xx - yy));
      }
    }
  }
}

// What a sample contributes besides its gathers: sigma, post', alpha and the radiance
struct Shade {
  float sigma, dpost, delta, e, om, rad[3];
};
__device__ __forceinline__ void shade(const DevGrid& g, const Interp& it, float dl, float dnorm, Shade& s) {
  post_activate_vg(g.post_act, it.v[0], s.sigma, s.dpost);
  s.delta = dl * dnorm;
  s.e = fast_exp(-(s.sigma * s.delta));
  s.om = 1.0f - (1.0f - s.e);   // (the forward's 1 - alpha)
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) s.rad[ch] = sigmoidf(it.x[ch][0]);
}

template <int G, int NCU>
__global__ __launch_bounds__(kRayThreads) void render_rays_bwd_kernel(DevGrid g, DevCfg c, RayBwdArgs a) {
  long long r;
  const bool valid = group_ray<WaveRectTile<G>>(c, r);   // (uniform over the G lanes of a ray: every lane joins the shuffles below)
  const int j = threadIdx.x % G;
  RayCtx<3, NCU, NCU> rc;
  int k_lo = 1, k_hi = 0;
  float T = 1.0f, gc[3] = {0.0f, 0.0f, 0.0f}, gd = 0.0f, q0 = 0.0f;
  double Q = 0.0;
  if (valid) {
    rc.init(g, c, r, a.rays_o, a.rays_d, a.jitter);
    if (a.g_col) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) gc[ch] = a.g_col[3 * r + ch];
    }
    if (a.g_depth) gd = a.g_depth[r];
    q0 = (a.g_acc ? a.g_acc[r] : 0.0f) - (c.white ? (gc[0] + gc[1]) + gc[2] : 0.0f);
    lane_block(c, rc, j, G, k_lo, k_hi);
    if (k_lo <= k_hi) {
      DepthStep st;
      st.start(rc, k_lo);
      for (int k = k_lo; k <= k_hi; ++k) {
        st.advance(rc, c, k);
        SampleCell scl;
        if (!scl.locate(g, rc, st.z)) continue;
        scl.make(g);
        Interp it;
        interp_cell<NCU, false>(g, a, scl.fp, scl.cell, rc.basis, it);
        Shade s;
        shade(g, it, st.dl(), rc.dnorm, s);
        const float w = (1.0f - s.e) * T;
        const float qk = fmaf(gc[0], s.rad[0], fmaf(gc[1], s.rad[1], fmaf(gc[2], s.rad[2], fmaf(gd, st.z, q0))));
        Q += (double)w * (double)qk;
        if (!attenuate(T, s.om)) break;   // every later w of the block is 0
      }
    }
  }
  // the blocks of a ray folded front to back
  float Ts = 1.0f;
  double pre = 0.0, total = Q;
  if constexpr (G > 1) {
    Ts = group_exclusive_product<G>(T, j);
    const double mine = (double)Ts * Q;
    double inc = mine;
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
      const double t = __shfl_up(inc, off, G);
      if (j >= off) inc += t;
    }
    pre = inc - mine;
    total = __shfl(inc, G - 1, G);
  }
  double dO[3] = {0.0, 0.0, 0.0}, dD[3] = {0.0, 0.0, 0.0}, bsum = 0.0;
  float m[NCU];
#pragma unroll
  for (int i = 0; i < NCU; ++i) m[i] = 0.0f;
  if (valid && k_lo <= k_hi && Ts > 0.0f) {
    float gs[3];
    index_to_world(g, gs);
    T = Ts;
    double GW = pre;   // sum w q over the samples up to and including the current one
    DepthStep st;
    st.start(rc, k_lo);
    for (int k = k_lo; k <= k_hi; ++k) {
      st.advance(rc, c, k);
      SampleCell scl;
      if (!scl.locate(g, rc, st.z)) continue;
      scl.make(g);
      const Cell& cell = scl.cell;
      Interp it;
      interp_cell<NCU, true>(g, a, scl.fp, cell, rc.basis, it);
      const float z = st.z, dl = st.dl();
      Shade s;
      shade(g, it, dl, rc.dnorm, s);
      const float w = (1.0f - s.e) * T;
      const float qk = fmaf(gc[0], s.rad[0], fmaf(gc[1], s.rad[1], fmaf(gc[2], s.rad[2], fmaf(gd, z, q0))));
      GW += (double)w * (double)qk;
      // (om == 0: T ends here, every later w is 0 and so is the true suffix; what the subtraction leaves is rounding)
      const double suffix = (st.last || !(s.om > 0.0f)) ? 0.0 : (total - GW);
      const float E = (float)((double)qk * (double)(T * s.e) - suffix);   // T e = T - w
      const float cd = (s.delta * E) * s.dpost;
      float sc[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) sc[ch] = (gc[ch] * s.rad[ch]) * (1.0f - s.rad[ch]);
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        float gi = cd * it.v[1 + ax];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) gi = fmaf(w * sc[ch], it.x[ch][1 + ax], gi);
        const float gw = gi * gs[ax];
        dO[ax] += (double)gw;
        dD[ax] += (double)z * (double)gw;
      }
      bsum += (double)(s.sigma * E) * (double)dl;
      if constexpr (NCU > 1) {
        if (w != 0.0f) {
          const float ws[3] = {w * sc[0], w * sc[1], w * sc[2]};
          basis_moments<NCU>(g, a, cell, ws, m);
        }
      }
      if (!attenuate(T, s.om)) break;   // every later term is 0
    }
  }
  if constexpr (G > 1) {
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        dO[ax] += __shfl_xor(dO[ax], off, G);
        dD[ax] += __shfl_xor(dD[ax], off, G);
      }
      bsum += __shfl_xor(bsum, off, G);
#pragma unroll
      for (int i = 1; i < NCU; ++i) m[i] += __shfl_xor(m[i], off, G);
    }
  }
  if (!valid || j != 0) return;
  const float v[3] = {rc.d[0] / rc.dnorm, rc.d[1] / rc.dnorm, rc.d[2] / rc.dnorm};
  float u[3];
  sh_basis_vjp<NCU>(v, m, u);
  const float uv = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    double dd = dD[ax];
    if (bsum != 0.0) dd += bsum * (double)v[ax];
    if constexpr (NCU > 1) dd += (double)((u[ax] - v[ax] * uv) / rc.dnorm);
    if (a.d_o) a.d_o[3 * r + ax] = (a.accumulate ? a.d_o[3 * r + ax] : 0.0f) + (float)dO[ax];
    if (a.d_d) a.d_d[3 * r + ax] = (a.accumulate ? a.d_d[3 * r + ax] : 0.0f) + (float)dd;
  }
}

template <int NCU>
void launch_g(int G, const DevGrid& g, const DevCfg& c, const RayBwdArgs& a, hipStream_t st) {
  for_lanes(G, [&](auto L) {
    render_rays_bwd_kernel<L(), NCU><<<(unsigned)group_blocks<WaveRectTile<L()>>(c), kRayThreads, 0, st>>>(g, c, a);
  });
}

}  // namespace

void launch_render_rays_bwd(const DevGrid& g, const DevCfg& c, int deg, int diffuse, const float* dens, const float* feat,
                            const float* rays_o, const float* rays_d, const float* jitter, const float* g_col,
                            const float* g_depth, const float* g_acc, float* d_o, float* d_d, int accumulate, hipStream_t st) {
  const int ncm = (deg + 1) * (deg + 1);
  const RayBwdArgs a{dens, feat, rays_o, rays_d, jitter, g_col, g_depth, g_acc, d_o, d_d, accumulate, ncm};
  const int G = lanes_per_ray(c.R, tl_lane_pins.rays_bwd);
  switch (diffuse ? 1 : ncm) {
    case 1: launch_g<1>(G, g, c, a, st); break;
    case 4: launch_g<4>(G, g, c, a, st); break;
    case 9: launch_g<9>(G, g, c, a, st); break;
    default: launch_g<16>(G, g, c, a, st); break;
  }
}

}  // namespace voxe
