// voxe_grid_elem.hpp -- the per-element arithmetic of the whole-grid passes, written once: the stand-alone passes of
// voxe_grid_ops.hip (Adam, the density regularisers, feature correlation) and the fused grid step of voxe_grid_step.hip call the
// same functions, so "the step computes what the separate passes compute" holds by construction (-ffp-contract=off: the same
// expression gives the same bits wherever it is inlined).  Plus the addressing the pack / unpack / step kernels share.
#pragma once

#include <math.h>
#include <stdint.h>

#include "voxe_device.hpp"
#include "voxe_launch.hpp"

namespace voxe {

// ------------------------------------------------------------------------------------------------
// torch.optim.Adam (single tensor, no weight decay / amsgrad)
// ------------------------------------------------------------------------------------------------
struct AdamHyper {
  float step_size, bc2_sqrt, beta1, beta2, eps;
};
// bias corrections of the 1-based `step` in double, rounded once
inline AdamHyper adam_hyper(float lr, float beta1, float beta2, float eps, long long step) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  return AdamHyper{(float)((double)lr / bc1), (float)sqrt(bc2), beta1, beta2, eps};
}
__device__ __forceinline__ float adam_update(float p, float gi, float& m, float& v, const AdamHyper& h) {
  const float mi = m + (gi - m) * (1.0f - h.beta1);              // exp_avg.lerp_(grad, 1-beta1)
  const float vi = v * h.beta2 + ((1.0f - h.beta2) * gi) * gi;   // mul_(beta2).addcmul_(g, g, 1-beta2)
  const float denom = sqrtf(vi) / h.bc2_sqrt + h.eps;
  m = mi;
  v = vi;
  return p - h.step_size * (mi / denom);                         // addcdiv_(exp_avg, denom, -step_size)
}

// ------------------------------------------------------------------------------------------------
// Regulariser gradients of one voxel (modules/sds_trainer.py:494-534 + autograd).  The stand-alone passes and the terms inside the
// step fold their weight into the constants on the host in two different ways (l2 / l1: w * float(1 / n) against 2 w / n in
// double; correlation: the scale folded by dcl_grad_kernel against by dcl_finalize_kernel) -- the callers' business, left as it
// is: unifying either would change bits.  The functions below take the finished float constants.
// ------------------------------------------------------------------------------------------------
// l2_mode / l1_mode: (a - b) k  /  sign(a - b) k   (sign(0) = 0)
__device__ __forceinline__ float density_diff_grad(int kind, float d, float k) {
  return kind == VOXE_DREG_L2 ? d * k : (d > 0.0f ? k : (d < 0.0f ? -k : 0.0f));
}
// _density_correlation_loss: ma / mb = the two means, k1 / k2 = the two gradient constants of dcl_finalize_kernel
__device__ __forceinline__ float dcl_grad(float a, float b, float ma, float mb, float k1, float k2) {
  const float A = a - ma, B = b - mb;
  return A * k2 - B * k1;
}
// the density term of the fused step: whichever of the two `t.kind` names, against the reference density t.b[i]
__device__ __forceinline__ float dcl_term(const DclTerm& t, float a, long long i) {
  if (t.kind != VOXE_DREG_CORRELATION) return density_diff_grad(t.kind, a - t.b[i], t.k);
  return dcl_grad(a, t.b[i], (float)t.stats[0], (float)t.stats[1], (float)t.stats[2], (float)t.stats[3]);
}

// _feature_correlation_loss: D = sum_c (sigmoid(f_c) - sigmoid(r_c)) in channel order, d f_c = (k D) sigmoid(f_c) (1 - sigmoid(f_c)),
// k = 2 x weight
__device__ __forceinline__ float sigmoid_ref(float x) { return 1.0f / (1.0f + expf(-x)); }   // (torch.sigmoid; not the render's fast path)
__device__ __forceinline__ float featcorr_diff(float f, float r) { return sigmoid_ref(f) - sigmoid_ref(r); }
__device__ __forceinline__ float featcorr_grad(float k, float D, float sg) { return (k * D) * ((1.0f - sg) * sg); }
// ... of a voxel whose F features sit in registers
template <int F>
__device__ __forceinline__ void featcorr_term(const float (&p)[F], const float (&r)[F], float k, float (&out)[F]) {
  float D = 0.0f;
#pragma unroll
  for (int f = 0; f < F; ++f) D += featcorr_diff(p[f], r[f]);
#pragma unroll
  for (int f = 0; f < F; ++f) out[f] = featcorr_grad(k, D, sigmoid_ref(p[f]));
}

// ------------------------------------------------------------------------------------------------
// Addressing of the packed [voxel][C] arrays
// ------------------------------------------------------------------------------------------------
// texel i as one 16-byte (C == 4) / 8-byte (C == 2) access, C scalars otherwise
template <int C>
__device__ __forceinline__ void texel_load(const float* base, long long i, float (&v)[C]) {
  if constexpr (C == 4) {
    const float4 t = reinterpret_cast<const float4*>(base)[i];
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if constexpr (C == 2) {
    const float2 t = reinterpret_cast<const float2*>(base)[i];
    v[0] = t.x; v[1] = t.y;
  } else {
#pragma unroll
    for (int f = 0; f < C; ++f) v[f] = base[i * C + f];
  }
}
template <int C>
__device__ __forceinline__ void texel_store(float* base, long long i, const float (&v)[C]) {
  if constexpr (C == 4) {
    reinterpret_cast<float4*>(base)[i] = make_float4(v[0], v[1], v[2], v[3]);
  } else if constexpr (C == 2) {
    reinterpret_cast<float2*>(base)[i] = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int f = 0; f < C; ++f) base[i * C + f] = v[f];
  }
}
template <int C>
__device__ __forceinline__ void texel_clear(float* base, long long i) {
  float zero[C];
#pragma unroll
  for (int f = 0; f < C; ++f) zero[f] = 0.0f;
  texel_store<C>(base, i, zero);
}

// where voxel i's gradient sits: at i, or in its slot of the 2x2x2-bricked buffer of the scatter backward.  I = long long, or
// unsigned where the launcher bounds the element count below 2^31 (wide texels: 32-bit divisions)
template <class I>
__device__ __forceinline__ long long grad_slot(I i, int bricked, int Y, int Z) {
  if (!bricked) return (long long)i;
  const int z = (int)(i % (I)Z), y = (int)((i / (I)Z) % (I)Y), x = (int)(i / ((I)Y * (I)Z));
  return brick_slot(x, y, z, Y, Z);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }   // (a null pointer counts as aligned)

}  // namespace voxe
