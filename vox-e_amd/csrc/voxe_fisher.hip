// voxe_fisher.hip -- per-voxel diagonal Fisher information of the rendered colours ("Fisher information").
//
// Per ray r and colour channel ch, with the forward's exact samples (the depth step, sample cell and tail of voxe_ray_march.hpp,
// SH colour per sample as voxe_render_rays_bwd.hip evaluates it) and q_{k,ch} = rad_{k,ch} - (white ? 1 : 0):
//   E_{k,ch}    = q_{k,ch} (T_k - w_k) - sum_{i>k} w_i q_{i,ch}                       (d C_ch / d sigma_k = delta_k E_{k,ch})
//   J_{r,ch}[c] = pre'(scale raw_c) scale * sum_k delta_k E_{k,ch} post'(v_k) t_c(k)   t_c = (wx * wy) * wz, in-grid corners only
//   fisher[c]  += sum_ch J_{r,ch}[c]^2                                                 once per ray: the square sits INSIDE the sum over rays
//   ray_var[r]  = sum_c P[c] sum_ch J_{r,ch}[c]^2
//
// The samples of one ray that touch a voxel form one contiguous run: along a ray every component of p = o + d z is monotone in z
// (float rounding is monotone), so the cell index floor(u) of each axis is monotone, and a voxel belongs to the cells i - 1 and i
// of its axis only.  A lane therefore carries the 8 corners of its current cell as 8 x 3 PENDING sums sum_k delta_k E post' t_c and
// squares a corner when the ray leaves it:
//   cell change with every |D_axis| <= 1 : axis by axis, the four corners of the side left behind are emitted, the four others
//                                          move over, the side entered starts at 0 (a corner emitted on the x shift is 0 by the
//                                          time the y shift looks at it: nothing is emitted twice)
//   a jump of more than one cell, a sample outside the box, the end of the ray (or of its transmittance): all 8 are emitted
// An emit multiplies with the corner factor pre' scale, squares, sums the channels, and
//   fisher  : one float atomic without return per emit (measured 4.7 - 4.9 per sample on the bench's 160^3 grid at S = 256,
//             about one sample per cell, against the 8 of the scatter backward: DESIGN.md 4.24);
//   ray_var : adds P[c] times it to a per-ray double: no atomics, the same bits on every run.
// Pending sums that are exactly 0 are not emitted: a voxel no sample weighs keeps an exact 0.
//
// One lane per ray.  march 1: the three totals sum_k w_k q_{k,ch} (double).  march 2: the samples again with the running
// inclusive prefix; the suffix is total - prefix (0 at the last sample and where 1 - alpha == 0: voxe_render_bwd's rule).
#include <hip/hip_runtime.h>

#include "voxe_launch.hpp"
#include "voxe_ray_march.hpp"

namespace voxe {
namespace {

struct FisherArgs {
  const float *dens, *feat, *rays_o, *rays_d, *jitter;
  float* fisher;
  const float* voxel_var;
  float* ray_var;
  int ncm;   // SH coefficients per colour channel in memory (F / 3)
};

// interpolated pre-activated density and pre-sigmoid radiance of a cell: every corner's texel contracted with the SH basis first
// (gather<>()'s re-association), value weights t = (wx * wy) * wz in the forward's corner order
template <int NCU>
__device__ __forceinline__ void interp_value(const DevGrid& g, const FisherArgs& a, const Cell& cell, const CellAddr& ad,
                                             const float (&basis)[NCU], float& v, float (&x)[3]) {
  const int ncm = NCU > 1 ? NCU : a.ncm;
  const int F = 3 * ncm;
  v = 0.0f;
  x[0] = x[1] = x[2] = 0.0f;
  constexpr int kCornersInFlight = NCU > 9 ? 1 : (NCU > 4 ? 2 : (NCU > 1 ? 4 : 8));
#pragma unroll kCornersInFlight
  for (int k = 0; k < 8; ++k) {
    // (selects, not array indexing: k is a run-time value in the partially unrolled loop)
    const bool bx = k & 1, by = k & 2, bz = k & 4;
    const float wx = bx ? cell.w[0][1] : cell.w[0][0], wy = by ? cell.w[1][1] : cell.w[1][0], wz = bz ? cell.w[2][1] : cell.w[2][0];
    const float w = (wx * wy) * wz;
    const unsigned idx = ad.base + (bx ? ad.sx : 0u) + (by ? ad.sy : 0u) + (bz ? ad.sz : 0u);
    const float cv = pre_activate(g.pre_act, a.dens[idx], g.density_scale);
    const float* __restrict__ src = a.feat + (long long)idx * F;
    v = fmaf(cv, w, v);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float r = basis[0] * src[ch * ncm];
#pragma unroll
      for (int j = 1; j < NCU; ++j) r = fmaf(basis[j], src[ch * ncm + j], r);
      x[ch] = fmaf(r, w, x[ch]);
    }
  }
}

// The pending sums of a lane: corner q = x + 2 y + 4 z of the cell whose low corner is voxel `base`
struct Pending {
  float s[8][3];
  unsigned base;
  int i[3];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q][0] = s[q][1] = s[q][2] = 0.0f;
  }
};

// One corner leaves the ray: J = (pre' scale) * pending per channel, squared and summed
__device__ __forceinline__ void emit(const DevGrid& g, const FisherArgs& a, unsigned idx, float p0, float p1, float p2, double& rv) {
  if (p0 == 0.0f && p1 == 0.0f && p2 == 0.0f) return;
  float f = g.density_scale;
  if (g.pre_act == VOXE_ACT_ABS) f = pre_activate_grad(g.pre_act, a.dens[idx], g.density_scale);
  const float j0 = f * p0, j1 = f * p1, j2 = f * p2;
  const float h = fmaf(j2, j2, fmaf(j1, j1, j0 * j0));
  if (h == 0.0f) return;
  if (a.fisher) atomicAdd(a.fisher + idx, h);
  if (a.ray_var) rv += (double)(a.voxel_var ? a.voxel_var[idx] : 1.0f) * (double)h;
}

__device__ __forceinline__ void emit_all(const DevGrid& g, const FisherArgs& a, const CellAddr& ad, Pending& p, double& rv) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const unsigned idx = p.base + (q & 1) * ad.sx + ((q >> 1) & 1) * ad.sy + (q >> 2) * ad.sz;
    emit(g, a, idx, p.s[q][0], p.s[q][1], p.s[q][2], rv);
  }
  p.clear();
}

// The cell moves by d in {-1, +1} along AX: the side left behind is emitted, the other side takes its place
template <int AX>
__device__ __forceinline__ void shift_axis(const DevGrid& g, const FisherArgs& a, const CellAddr& ad, int d, Pending& p, double& rv) {
  constexpr int bit = 1 << AX;
  const unsigned stride = AX == 0 ? ad.sx : (AX == 1 ? ad.sy : ad.sz);
  const bool up = d > 0;
#pragma unroll
  for (int lo = 0; lo < 8; ++lo) {
    if (lo & bit) continue;
    const int hi = lo | bit;
    const unsigned idx = p.base + (lo & 1) * ad.sx + ((lo >> 1) & 1) * ad.sy + (lo >> 2) * ad.sz + (up ? 0u : stride);
    emit(g, a, idx, up ? p.s[lo][0] : p.s[hi][0], up ? p.s[lo][1] : p.s[hi][1], up ? p.s[lo][2] : p.s[hi][2], rv);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float keep = up ? p.s[hi][ch] : p.s[lo][ch];
      p.s[lo][ch] = up ? keep : 0.0f;
      p.s[hi][ch] = up ? 0.0f : keep;
    }
  }
  p.base = up ? p.base + stride : p.base - stride;
}

struct Shade {
  float dpost, delta, e, om, q[3];
};
__device__ __forceinline__ void shade(const DevGrid& g, float v, const float (&x)[3], float dl, float dnorm, float bg, Shade& s) {
  float sigma;
  post_activate_vg(g.post_act, v, sigma, s.dpost);
  s.delta = dl * dnorm;
  s.e = fast_exp(-(sigma * s.delta));
  s.om = 1.0f - (1.0f - s.e);   // (the forward's 1 - alpha)
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) s.q[ch] = sigmoidf(x[ch]) - bg;
}

template <int NCU>
__global__ __launch_bounds__(kMarchThreads) void fisher_rays_kernel(DevGrid g, DevCfg c, FisherArgs a) {
  long long r;
  if (!group_ray<WaveRectTile<1>>(c, r)) return;
  RayCtx<3, NCU, NCU> rc;
  rc.init(g, c, r, a.rays_o, a.rays_d, a.jitter);
  const float bg = c.white ? 1.0f : 0.0f;
  const int k_lo = rc.k_lo, k_hi = rc.k_hi;
  double rv = 0.0;
  if (k_lo <= k_hi) {
    // march 1: the totals sum_k w_k q_k
    double total[3] = {0.0, 0.0, 0.0};
    {
      float T = 1.0f;
      DepthStep st;
      st.start(rc, k_lo);
      for (int k = k_lo; k <= k_hi; ++k) {
        st.advance(rc, c, k);
        SampleCell scl;
        if (!scl.locate(g, rc, st.z)) continue;
        scl.make(g);
        float v, x[3];
        interp_value<NCU>(g, a, scl.cell, cell_addr(g, scl.cell), rc.basis, v, x);
        Shade s;
        shade(g, v, x, st.dl(), rc.dnorm, bg, s);
        const float w = (1.0f - s.e) * T;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) total[ch] += (double)w * (double)s.q[ch];
        if (!attenuate(T, s.om)) break;   // every later w is 0
      }
    }
    // march 2: the pending sums
    Pending p;
    p.clear();
    bool live = false;
    CellAddr ad;
    ad.base = 0;
    ad.sx = g.X > 1 ? g.Y * g.Z : 0;
    ad.sy = g.Y > 1 ? g.Z : 0;
    ad.sz = g.Z > 1 ? 1 : 0;
    double GW[3] = {0.0, 0.0, 0.0};   // sum w q over the samples up to and including the current one
    float T = 1.0f;
    DepthStep st;
    st.start(rc, k_lo);
    for (int k = k_lo; k <= k_hi; ++k) {
      st.advance(rc, c, k);
      SampleCell scl;
      if (!scl.locate(g, rc, st.z)) {
        if (live) {
          emit_all(g, a, ad, p, rv);
          live = false;
        }
        continue;
      }
      scl.make(g);
      const Cell& cell = scl.cell;
      const CellAddr cad = cell_addr(g, cell);
      if (live) {
        const int dx = cell.i[0] - p.i[0], dy = cell.i[1] - p.i[1], dz = cell.i[2] - p.i[2];
        if ((dx | dy | dz) != 0) {
          if (abs(dx) > 1 || abs(dy) > 1 || abs(dz) > 1) {
            emit_all(g, a, ad, p, rv);
          } else {
            if (dx != 0) shift_axis<0>(g, a, ad, dx, p, rv);
            if (dy != 0) shift_axis<1>(g, a, ad, dy, p, rv);
            if (dz != 0) shift_axis<2>(g, a, ad, dz, p, rv);
          }
        }
      }
      live = true;
      p.base = cad.base;
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) p.i[ax] = cell.i[ax];
      float v, x[3];
      interp_value<NCU>(g, a, cell, cad, rc.basis, v, x);
      Shade s;
      shade(g, v, x, st.dl(), rc.dnorm, bg, s);
      const float w = (1.0f - s.e) * T;
      const bool cut = st.last || !(s.om > 0.0f);   // (om == 0: T ends here, every later w is 0 and so is the true suffix)
      float cd[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        GW[ch] += (double)w * (double)s.q[ch];
        const double suffix = cut ? 0.0 : (total[ch] - GW[ch]);
        const float E = (float)((double)s.q[ch] * (double)(T * s.e) - suffix);   // T e = T - w
        cd[ch] = (s.delta * E) * s.dpost;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float t = (cell.w[0][q & 1] * cell.w[1][(q >> 1) & 1]) * cell.w[2][q >> 2];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) p.s[q][ch] = fmaf(cd[ch], t, p.s[q][ch]);
      }
      if (!attenuate(T, s.om)) break;   // every later term is 0
    }
    if (live) emit_all(g, a, ad, p, rv);
  }
  if (a.ray_var) a.ray_var[r] = (float)rv;
}

template <int NCU>
void launch_t(const DevGrid& g, const DevCfg& c, const FisherArgs& a, hipStream_t st) {
  fisher_rays_kernel<NCU><<<(unsigned)group_blocks<WaveRectTile<1>>(c), kMarchThreads, 0, st>>>(g, c, a);
}

}  // namespace

void launch_fisher_rays(const DevGrid& g, const DevCfg& c, int deg, int diffuse, const float* dens, const float* feat,
                        const float* rays_o, const float* rays_d, const float* jitter, float* fisher, const float* voxel_var,
                        float* ray_var, hipStream_t st) {
  const int ncm = (deg + 1) * (deg + 1);
  const FisherArgs a{dens, feat, rays_o, rays_d, jitter, fisher, voxel_var, ray_var, ncm};
  switch (diffuse ? 1 : ncm) {
    case 1: launch_t<1>(g, c, a, st); break;
    case 4: launch_t<4>(g, c, a, st); break;
    case 9: launch_t<9>(g, c, a, st); break;
    default: launch_t<16>(g, c, a, st); break;
  }
}

}  // namespace voxe
