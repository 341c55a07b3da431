// voxe_transform.hip -- rigid transform / re-gridding / composition of voxel grids ("Transform").
//
//   resample : one thread per DESTINATION voxel (z fastest, so a wave stores 64 consecutive texels).  The thread maps its integer
//              index i to the continuous source index u = A i + b (A, b wave-uniform kernel arguments, float32, no FMA:
//              u_a = ((A_a0 ix + A_a1 iy) + A_a2 iz) + b_a), takes i0 = floor(u), f = u - i0, per-axis weights (1 - f, f) and
//              corner weights t_c = (wx * wy) * wz, corners ascending with x in bit 0 as in the renderer's gather.  The density is
//              read through the pre-activation (IDENTITY | ABS) per corner; a corner outside the source lattice counts as
//              density_fill for the density and 0 for every feature channel; a voxel whose 8 corners are all outside loads
//              nothing.  SH grids are handled one colour channel at a time: the (deg+1)^2 coefficients of the channel are
//              interpolated from the 8 corners (all loads of the channel issued together, in runs of up to 16 bytes that may
//              start at any float), rotated band by band with the (2l+1)^2 blocks of sh_rot (band 0 is the identity and is not
//              multiplied) and stored; live registers stay near 2 x 16 plus the weights.  The SH-0 texel (one band, the
//              identity) is read and written as one run of 3 floats; plain channels (sh_degree = -1) go one at a time.
//   modes    : REPLACE writes every destination voxel.  UNION replaces a destination voxel (density and all features) iff every
//              corner with non-zero weight lies in the source lattice and the sample's density is strictly greater than the
//              pre-activated destination density; every other destination voxel is not written at all.
// Out-of-range or NaN u: floor(u) is clamped to [-2, N] in float before the conversion, which keeps every corner of that axis
// outside the lattice; loads use indices clamped into the lattice, so no address leaves the source tensors.
#include <hip/hip_runtime.h>

#include "voxe_launch.hpp"

namespace voxe {
namespace {

constexpr int kXfThreads = 256;

struct XfDims {
  int X, Y, Z;      // source
  int X2, Y2, Z2;   // destination
  int C;            // feature channels per texel
};

struct XfSample {
  unsigned vox[8];   // clamped linear voxel index of every corner (always addressable)
  float t[8];        // corner weights
  unsigned in_mask;  // bit q: corner q lies in the source lattice
  bool valid;        // every corner with t != 0 is in the lattice
  bool any;          // some corner with t != 0 is in the lattice
};

__device__ __forceinline__ void xf_sample(const XfDims& d, const VoxeResample& xf, unsigned ix, unsigned iy, unsigned iz,
                                          XfSample& s) {
  const int N[3] = {d.X, d.Y, d.Z};
  const float fi[3] = {(float)ix, (float)iy, (float)iz};
  int c[3][2];
  bool in[3][2];
  float w[3][2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float u = xf.A[3 * a + 0] * fi[0];
    u = u + xf.A[3 * a + 1] * fi[1];
    u = u + xf.A[3 * a + 2] * fi[2];
    u = u + xf.b[a];
    const float fl = floorf(u);
    const float f = u - fl;
    w[a][0] = 1.0f - f;
    w[a][1] = f;
    const int i0 = (int)fminf(fmaxf(fl, -2.0f), (float)N[a]);   // (NaN -> -2: outside)
    in[a][0] = (unsigned)i0 < (unsigned)N[a];
    in[a][1] = (unsigned)(i0 + 1) < (unsigned)N[a];
    c[a][0] = min(max(i0, 0), N[a] - 1);
    c[a][1] = min(max(i0 + 1, 0), N[a] - 1);
  }
  s.in_mask = 0u;
  s.valid = true;
  s.any = false;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int bx = q & 1, by = (q >> 1) & 1, bz = q >> 2;
    // operands of the 24-bit multiplies: X*Y, Y*Z, Z < 2^24 (validated on the host)
    s.vox[q] = __umul24(__umul24((unsigned)c[0][bx], (unsigned)d.Y) + (unsigned)c[1][by], (unsigned)d.Z) + (unsigned)c[2][bz];
    s.t[q] = (w[0][bx] * w[1][by]) * w[2][bz];
    const bool inside = in[0][bx] && in[1][by] && in[2][bz];
    const bool nz = s.t[q] != 0.0f;   // (NaN weights count as non-zero)
    s.in_mask |= inside ? (1u << q) : 0u;
    s.valid = s.valid && (inside || !nz);
    s.any = s.any || (inside && nz);
  }
}

// N consecutive floats as one access.  The type is 4-byte aligned, so a run may start at any float: global memory takes
// unaligned multi-dword accesses, and a texel of 3, 9 or 27 floats is then read in runs of 4 / 3 / 2 / 1 instead of float by float
template <int N>
struct __attribute__((packed, aligned(4))) FloatRun {
  float v[N];
};

template <int K, int AT = 0>
__device__ __forceinline__ void load_run(const float* __restrict__ p, float (&v)[K]) {
  if constexpr (AT < K) {
    constexpr int N = (K - AT >= 4) ? 4 : (K - AT);
    const FloatRun<N> x = *reinterpret_cast<const FloatRun<N>*>(p + AT);
#pragma unroll
    for (int k = 0; k < N; ++k) v[AT + k] = x.v[k];
    load_run<K, AT + N>(p, v);
  }
}

template <int K, int AT = 0>
__device__ __forceinline__ void store_run(float* __restrict__ p, const float (&v)[K]) {
  if constexpr (AT < K) {
    constexpr int N = (K - AT >= 4) ? 4 : (K - AT);
    FloatRun<N> x;
#pragma unroll
    for (int k = 0; k < N; ++k) x.v[k] = v[AT + k];
    *reinterpret_cast<FloatRun<N>*>(p + AT) = x;
    store_run<K, AT + N>(p, v);
  }
}

// K consecutive floats of the texel of every corner, interpolated: out[k] = sum_q t_q * (corner q inside ? src[...] : 0)
template <int K>
__device__ __forceinline__ void xf_gather(const float* __restrict__ src, int C, int off, const XfSample& s, float (&out)[K]) {
  float v[8][K];
#pragma unroll
  for (int q = 0; q < 8; ++q) load_run<K>(src + (size_t)s.vox[q] * (unsigned)C + off, v[q]);
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.0f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const bool inside = (s.in_mask >> q) & 1u;
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = fmaf(inside ? v[q][k] : 0.0f, s.t[q], out[k]);
  }
}

// c'_l = M_l c_l for the bands 1..deg of one colour channel (K = (deg+1)^2 coefficients); band 0 is the identity
template <int K>
__device__ __forceinline__ void xf_rotate(const VoxeResample& xf, const float (&c)[K], float (&r)[K]) {
  r[0] = c[0];
  if constexpr (K > 1) {
    int m = 1;   // offset of the band's block in sh_rot: 1, 10, 35
#pragma unroll
    for (int l = 1; l * l < K; ++l) {
      const int n = 2 * l + 1, first = l * l;
#pragma unroll
      for (int j = 0; j < n; ++j) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < n; ++k) acc = fmaf(xf.sh_rot[m + j * n + k], c[first + k], acc);
        r[first + j] = acc;
      }
      m += n * n;
    }
  }
}

// ROT: an SH grid of K coefficients per colour channel (C = 3 K), rotated channel by channel.  !ROT: C / K groups of K plain
// floats (K = 1: any C; K = 3: the SH-0 texel, whose only band is the identity)
template <int K, bool ROT>
__global__ __launch_bounds__(kXfThreads) void resample_kernel(XfDims d, VoxeResample xf, const float* __restrict__ src_dens,
                                                              const float* __restrict__ src_feat, float* dst_dens,
                                                              float* dst_feat, uint8_t* __restrict__ taken) {
  const unsigned n = (unsigned)d.X2 * (unsigned)d.Y2 * (unsigned)d.Z2;   // < 2^31 (validated on the host)
  const unsigned i = blockIdx.x * (unsigned)kXfThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned iz = i % (unsigned)d.Z2, row = i / (unsigned)d.Z2;
  const unsigned iy = row % (unsigned)d.Y2, ix = row / (unsigned)d.Y2;
  const bool is_union = xf.mode == VOXE_RESAMPLE_UNION;
  const bool use_abs = xf.density_pre_act == VOXE_ACT_ABS;
  XfSample s;
  xf_sample(d, xf, ix, iy, iz, s);
  const int groups = ROT ? 3 : d.C / K;
  float* const out_feat = dst_feat ? dst_feat + (size_t)i * (unsigned)d.C : nullptr;

  if (s.in_mask == 0u) {   // all 8 corners outside the lattice: the fill values, nothing loaded
    if (taken) taken[i] = 0;
    if (is_union) return;
    if (dst_dens) dst_dens[i] = xf.density_fill;
    if (out_feat) {
      float zero[K];
#pragma unroll
      for (int k = 0; k < K; ++k) zero[k] = 0.0f;
      for (int gch = 0; gch < groups; ++gch) store_run<K>(out_feat + gch * K, zero);
    }
    return;
  }

  if (src_dens) {
    float raw[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) raw[q] = src_dens[s.vox[q]];
    float dv = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float pre = use_abs ? fabsf(raw[q]) : raw[q];
      dv = fmaf(((s.in_mask >> q) & 1u) ? pre : xf.density_fill, s.t[q], dv);
    }
    if (is_union) {
      const float old = dst_dens[i];
      const bool take = s.valid && (dv > (use_abs ? fabsf(old) : old));   // (NaN on either side: left alone)
      if (taken) taken[i] = take ? 1 : 0;
      if (!take) return;
    }
    dst_dens[i] = dv;
  }
  if (!is_union && taken) taken[i] = s.any ? 1 : 0;
  if (!out_feat) return;

  for (int gch = 0; gch < groups; ++gch) {
    float c[K], r[K];
    xf_gather<K>(src_feat, d.C, gch * K, s, c);
    if constexpr (ROT) {
      xf_rotate<K>(xf, c, r);
      store_run<K>(out_feat + gch * K, r);
    } else {
      store_run<K>(out_feat + gch * K, c);
    }
  }
}

template <int K, bool ROT>
void launch_one(const XfDims& d, const VoxeResample& xf, const float* src_dens, const float* src_feat, float* dst_dens,
                float* dst_feat, uint8_t* taken, hipStream_t st) {
  const long long n = (long long)d.X2 * d.Y2 * d.Z2;
  const unsigned nb = (unsigned)((n + kXfThreads - 1) / kXfThreads);
  resample_kernel<K, ROT><<<nb, kXfThreads, 0, st>>>(d, xf, src_dens, src_feat, dst_dens, dst_feat, taken);
}

}  // namespace

void launch_grid_resample(const float* src_dens, const float* src_feat, int X, int Y, int Z, int C, float* dst_dens, float* dst_feat,
                          int X2, int Y2, int Z2, const VoxeResample& xf, uint8_t* taken, hipStream_t st) {
  const XfDims d = {X, Y, Z, X2, Y2, Z2, C};
  switch (src_feat ? xf.sh_degree : -1) {
    case 0: launch_one<3, false>(d, xf, src_dens, src_feat, dst_dens, dst_feat, taken, st); break;
    case 1: launch_one<4, true>(d, xf, src_dens, src_feat, dst_dens, dst_feat, taken, st); break;
    case 2: launch_one<9, true>(d, xf, src_dens, src_feat, dst_dens, dst_feat, taken, st); break;
    case 3: launch_one<16, true>(d, xf, src_dens, src_feat, dst_dens, dst_feat, taken, st); break;
    default: launch_one<1, false>(d, xf, src_dens, src_feat, dst_dens, dst_feat, taken, st); break;
  }
}

}  // namespace voxe
