// voxe_grid_step.hip -- the streaming passes between the API tensors (densities [X,Y,Z,1], features [X,Y,Z,F]) and the packed
// grid [X,Y,Z,C = F+1] the render kernels read (layout: voxe_render.hip): pack, un-pack of the gradient with the chain rule of the
// density pre-activation, and the fused optimiser step.  The per-element arithmetic is voxe_grid_elem.hpp's.
#include <type_traits>

#include "voxe_grid_elem.hpp"

namespace voxe {

// ------------------------------------------------------------------------------------------------
// pack / unpack (HBM streaming; voxels.py:303-305 pre-activation is applied per voxel here, exactly
// like the reference applies it to the whole grid before interpolating)
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void pack_grid_kernel(const float* __restrict__ dens,
                                                        const float* __restrict__ feat,
                                                        float* __restrict__ packed, long long nvox,
                                                        float scale, int pre_act) {
  constexpr int F = C - 1;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += stride) {
    float v[C];
#pragma unroll
    for (int f = 0; f < F; ++f) v[f] = feat[i * F + f];
    v[F] = pre_activate(pre_act, dens[i], scale);
    texel_store<C>(packed, i, v);
  }
}

template <int C>
__global__ __launch_bounds__(256) void unpack_grad_kernel(const float* __restrict__ gpacked,
                                                          const float* __restrict__ dens,
                                                          float* __restrict__ d_dens,
                                                          float* __restrict__ d_feat, long long nvox,
                                                          float scale, int pre_act, int accumulate,
                                                          int bricked, int Y, int Z) {
  constexpr int F = C - 1;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += stride) {
    float v[C];
    texel_load<C>(gpacked, grad_slot(i, bricked, Y, Z), v);
    if (d_feat) {
#pragma unroll
      for (int f = 0; f < F; ++f) {
        const long long j = i * F + f;
        d_feat[j] = accumulate ? d_feat[j] + v[f] : v[f];
      }
    }
    if (d_dens) {
      const float gval = v[F] * pre_activate_grad(pre_act, dens[i], scale);
      d_dens[i] = accumulate ? d_dens[i] + gval : gval;
    }
  }
}

// Wide texels (13 / 28 / 49 channels): one thread per ELEMENT of the packed array, so that consecutive lanes touch
// consecutive floats of both layouts (a thread per voxel strides by C floats: 64 cache lines per wave instruction).
template <int C>
__global__ __launch_bounds__(256) void pack_grid_wide_kernel(const float* __restrict__ dens, const float* __restrict__ feat,
                                                             float* __restrict__ packed, long long nvox, float scale,
                                                             int pre_act) {
  constexpr int F = C - 1;
  // (32-bit index math: validate() bounds nvox * C below 2^31)
  const unsigned n = (unsigned)(nvox * C), stride = gridDim.x * blockDim.x;
  for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const unsigned i = e / C, ch = e - i * C;
    packed[e] = ch < F ? feat[i * F + ch] : pre_activate(pre_act, dens[i], scale);
  }
}

template <int C>
__global__ __launch_bounds__(256) void unpack_grad_wide_kernel(const float* __restrict__ gpacked,
                                                               const float* __restrict__ dens, float* __restrict__ d_dens,
                                                               float* __restrict__ d_feat, long long nvox, float scale,
                                                               int pre_act, int accumulate, int bricked, int Y, int Z) {
  constexpr int F = C - 1;
  const unsigned n = (unsigned)(nvox * C), stride = gridDim.x * blockDim.x;
  for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const unsigned i = e / C, ch = e - i * C;
    const float v = gpacked[grad_slot(i, bricked, Y, Z) * C + ch];
    if (ch < F) {
      if (d_feat) d_feat[i * F + ch] = accumulate ? d_feat[i * F + ch] + v : v;
    } else if (d_dens) {
      const float gval = v * pre_activate_grad(pre_act, dens[i], scale);
      d_dens[i] = accumulate ? d_dens[i] + gval : gval;
    }
  }
}

// r04: the same two conversions with 16-byte accesses on BOTH layouts.  A block takes chunks of kWideChunk voxels through LDS:
// the chunk is contiguous in either layout (64 x F floats of `feat`, 64 x C floats of `packed`; both a multiple of 16 bytes),
// only the interleave differs, and that happens on the 4-byte LDS side.  The one-element-per-thread kernels above moved
// 2.3 - 2.8 TB/s at 49 channels (4 bytes per lane and an integer division per element).
// Whole chunks only; the launcher sends the tail (nvox % 64 voxels) and bricked gradient buffers through the kernels above.
constexpr int kWideChunk = 64;
template <int C>
__global__ __launch_bounds__(256) void pack_grid_wide16_kernel(const float* __restrict__ dens, const float* __restrict__ feat,
                                                               float* __restrict__ packed, long long nchunks, float scale,
                                                               int pre_act) {
  constexpr int F = C - 1, V = kWideChunk;
  __shared__ float4 buf4[V * C / 4];
  float* const buf = reinterpret_cast<float*>(buf4);
  const int tid = threadIdx.x;
  for (long long ck = blockIdx.x; ck < nchunks; ck += gridDim.x) {
    const float4* __restrict__ f4 = reinterpret_cast<const float4*>(feat + ck * (V * F));
    for (int q = tid; q < V * F / 4; q += 256) {
      const float4 t = f4[q];
      const float e[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = 4 * q + u, i = idx / F;
        buf[i * C + (idx - i * F)] = e[u];
      }
    }
    if (tid < V) buf[tid * C + F] = pre_activate(pre_act, dens[ck * V + tid], scale);
    __syncthreads();
    float4* __restrict__ p4 = reinterpret_cast<float4*>(packed + ck * (V * C));
    for (int q = tid; q < V * C / 4; q += 256) p4[q] = buf4[q];
    __syncthreads();
  }
}

template <int C>
__global__ __launch_bounds__(256) void unpack_grad_wide16_kernel(const float* __restrict__ gpacked,
                                                                 const float* __restrict__ dens, float* __restrict__ d_dens,
                                                                 float* __restrict__ d_feat, long long nchunks, float scale,
                                                                 int pre_act, int accumulate) {
  constexpr int F = C - 1, V = kWideChunk;
  __shared__ float4 buf4[V * C / 4];
  float* const buf = reinterpret_cast<float*>(buf4);
  const int tid = threadIdx.x;
  for (long long ck = blockIdx.x; ck < nchunks; ck += gridDim.x) {
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(gpacked + ck * (V * C));
    for (int q = tid; q < V * C / 4; q += 256) buf4[q] = g4[q];
    __syncthreads();
    if (d_feat) {
      float4* __restrict__ o4 = reinterpret_cast<float4*>(d_feat + ck * (V * F));
      for (int q = tid; q < V * F / 4; q += 256) {
        float e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int idx = 4 * q + u, i = idx / F;
          e[u] = buf[i * C + (idx - i * F)];
        }
        float4 t = make_float4(e[0], e[1], e[2], e[3]);
        if (accumulate) {
          const float4 old = o4[q];
          t = make_float4(old.x + t.x, old.y + t.y, old.z + t.z, old.w + t.w);
        }
        o4[q] = t;
      }
    }
    if (d_dens && tid < V) {
      const long long i = ck * V + tid;
      const float gval = buf[tid * C + F] * pre_activate_grad(pre_act, dens[i], scale);
      d_dens[i] = accumulate ? d_dens[i] + gval : gval;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// Fused optimiser step: un-pack the gradient (+ chain rule of the density pre-activation), Adam on both parameter
// tensors, re-pack the updated grid, clear the gradient -- one streaming pass instead of four
// (unpack 131 MB + Adam 459 MB + pack 131 MB + memset 65 MB -> 590 MB at 160^3).
// Four kernels, one per data movement (the launcher picks from alignment and layout); the two element functions below are
// what every one of them computes.
// ------------------------------------------------------------------------------------------------
// what all four kernels are handed (m_d / m_f null: that tensor is frozen; extra_*: regulariser gradients in tensor layout, nullable)
struct StepArgs {
  float *gpacked, *dens, *feat, *m_d, *v_d, *m_f, *v_f, *packed;
  const float *extra_d, *extra_f;
  float scale;
  int pre_act;
  AdamHyper h_d, h_f;
  DclTerm dcl;
};
constexpr int kStepBlocks = 16384;   // most blocks of a step launch

// the density of voxel i: chain rule of the pre-activation on its packed gradient g, + the extra gradient, + the regulariser
// term (on the parameter the step starts from, like every gradient), then Adam.  Returns the new raw density.
__device__ __forceinline__ float density_update(const StepArgs& a, long long i, float g, float d, float& m, float& v) {
  const float gd = g * pre_activate_grad(a.pre_act, d, a.scale);
  float gi = a.extra_d ? gd + a.extra_d[i] : gd;
  if (a.dcl.b) gi += dcl_term(a.dcl, d, i);
  return adam_update(d, gi, m, v, a.h_d);
}
// ... the same through memory: returns the density channel of the voxel's new texel
__device__ __forceinline__ float density_element(const StepArgs& a, long long i, float g) {
  float d = a.dens[i];
  if (a.m_d) {
    float m = a.m_d[i], v = a.v_d[i];
    d = density_update(a, i, g, d, m, v);
    a.dens[i] = d; a.m_d[i] = m; a.v_d[i] = v;
  }
  return pre_activate(a.pre_act, d, a.scale);
}
// one feature: its packed gradient g, + the extra gradient `ex` (read only where a.extra_f is set), + the feature-correlation
// term `reg` in the kernels that carry one (REG; texels of up to 4 channels), then Adam.  Returns the new feature.
template <bool REG>
__device__ __forceinline__ float feature_update(const StepArgs& a, float g, float ex, float reg, float p, float& m, float& v) {
  float gi = a.extra_f ? g + ex : g;
  if constexpr (REG) { if (a.dcl.fref) gi += reg; }
  return adam_update(p, gi, m, v, a.h_f);
}
// ... the same through memory, element j of the [voxel][F] tensors
template <bool REG>
__device__ __forceinline__ float feature_element(const StepArgs& a, long long j, float g, float reg) {
  float p = a.feat[j];
  if (a.m_f) {
    float m = a.m_f[j], v = a.v_f[j];
    p = feature_update<REG>(a, g, a.extra_f ? a.extra_f[j] : 0.0f, reg, p, m, v);
    a.feat[j] = p; a.m_f[j] = m; a.v_f[j] = v;
  }
  return p;
}

// one thread per voxel: narrow texels in any layout (bricked buffers, unaligned slabs, the last voxels behind the kernel below)
template <int C>
__global__ __launch_bounds__(256) void grid_adam_kernel(StepArgs a, long long vox_begin, long long vox_end, int bricked, int Y, int Z) {
  constexpr int F = C - 1;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = vox_begin + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < vox_end; i += stride) {
    const long long si = grad_slot(i, bricked, Y, Z);
    float g[C], out[C], fg[F];
    texel_load<C>(a.gpacked, si, g);
    texel_clear<C>(a.gpacked, si);
#pragma unroll
    for (int f = 0; f < F; ++f) fg[f] = 0.0f;
    if (a.dcl.fref && a.m_f) {
      float pf[F], rf[F];
#pragma unroll
      for (int f = 0; f < F; ++f) { pf[f] = a.feat[i * F + f]; rf[f] = a.dcl.fref[i * F + f]; }
      featcorr_term<F>(pf, rf, a.dcl.fk, fg);
    }
#pragma unroll
    for (int f = 0; f < F; ++f) out[f] = feature_element<true>(a, i * F + f, g[f], fg[f]);
    out[F] = density_element(a, i, g[F]);
    texel_store<C>(a.packed, i, out);
  }
}

// C == 4, linear gradient layout, every global access a fully coalesced wave instruction (r03): a wave takes 256 consecutive
// voxels; lane l owns voxels base + l + 64 k (k = 0..3), so the float4 streams (packed gradient, packed grid) and the per-voxel
// scalars (density, its moments) are contiguous across the lanes of every instruction; the [N,3] streams (features, their
// moments) are read as three contiguous float4 instructions per wave and handed to their voxels' lanes through a wave-private
// LDS buffer (stride-3 reads: conflict free), and written back the same way.  Measured against the alternatives (same arithmetic
// per element): one voxel per thread (nine 4-byte accesses of stride 12 for the [N,3] streams) 0.130 ms; four voxels per thread with
// 16-byte chunks at 48 / 64-byte lane strides 0.110 - 0.118 ms and 20 % more bytes written than the streams hold (partial lines,
// PMC WRITE_SIZE 394 MB); this kernel 0.085 ms, 328 MB written.  The sweep direction alternates with the step (the tail of one
// step's sweep is the head of the next in the Infinity Cache: -5 % at 100x100, +-0 at 400x400); non-temporal loads / stores of
// parameters and moments were 25 % slower (the moments live partly in the Infinity Cache from step to step).
__device__ __forceinline__ void wave_lds_order() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// FEATCORR (r06): with the feature-correlation term compiled in, the kernel needs 170 registers -- 2 waves per SIMD instead of the 3
// that 150 leave -- and the plain step ran 103 instead of 86 us (rocprofv3 averages r05 -> r06): the term is its own instantiation.
template <bool FEATCORR>
__global__ __launch_bounds__(256) void grid_adam_v5_kernel(StepArgs a, long long vox_begin, int nchunks, int flip) {
  __shared__ float4 lds4[4][3][192];   // [wave][buffer][256 voxels x 3 floats]
  float4* const gpacked = reinterpret_cast<float4*>(a.gpacked);
  float4* const packed = reinterpret_cast<float4*>(a.packed);
  float4* const feat = reinterpret_cast<float4*>(a.feat);
  float4* const m_f = reinterpret_cast<float4*>(a.m_f);
  float4* const v_f = reinterpret_cast<float4*>(a.v_f);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nwaves = gridDim.x * 4;
  for (int c0 = blockIdx.x * 4 + wave; c0 < nchunks; c0 += nwaves) {
    const int c = flip ? nchunks - 1 - c0 : c0;
    const long long vb = vox_begin + (long long)c * 256;      // first voxel of the chunk (a multiple of 4)
    const long long f4 = vb * 3 / 4;                           // first float4 of the chunk in an [N,3] stream
    float4 g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = gpacked[vb + k * 64 + lane];
    // [N,3] streams -> LDS (three coalesced float4 instructions each)
    float4 (*buf)[192] = lds4[wave];
#pragma unroll
    for (int k = 0; k < 3; ++k) buf[0][k * 64 + lane] = feat[f4 + k * 64 + lane];
    if (m_f) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { buf[1][k * 64 + lane] = m_f[f4 + k * 64 + lane]; buf[2][k * 64 + lane] = v_f[f4 + k * 64 + lane]; }
    }
    float d[4], md[4], vd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[k] = a.dens[vb + k * 64 + lane];
      if (a.m_d) { md[k] = a.m_d[vb + k * 64 + lane]; vd[k] = a.v_d[vb + k * 64 + lane]; }
    }
    wave_lds_order();
    float p[12], m[12], v[12];
    const float* b0 = reinterpret_cast<const float*>(buf[0]);
    const float* b1 = reinterpret_cast<const float*>(buf[1]);
    const float* b2 = reinterpret_cast<const float*>(buf[2]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        const int i = (k * 64 + lane) * 3 + f;
        p[k * 3 + f] = b0[i];
        if (m_f) { m[k * 3 + f] = b1[i]; v[k * 3 + f] = b2[i]; }
      }
    wave_lds_order();
    float fg[12];   // (FEATCORR only)
    if constexpr (FEATCORR) if (m_f && a.dcl.fref) {   // feature-correlation term (r06; weight 0 by default): the reference features through buffer 0
      const float4* __restrict__ fr4 = reinterpret_cast<const float4*>(a.dcl.fref);
#pragma unroll
      for (int k = 0; k < 3; ++k) buf[0][k * 64 + lane] = fr4[f4 + k * 64 + lane];
      wave_lds_order();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float pk[3] = {p[k * 3], p[k * 3 + 1], p[k * 3 + 2]};
        const float rk[3] = {b0[(k * 64 + lane) * 3], b0[(k * 64 + lane) * 3 + 1], b0[(k * 64 + lane) * 3 + 2]};
        float o[3];
        featcorr_term<3>(pk, rk, a.dcl.fk, o);
        fg[k * 3] = o[0]; fg[k * 3 + 1] = o[1]; fg[k * 3 + 2] = o[2];
      }
      wave_lds_order();
    }
    if (m_f) {
      if (a.extra_f) {   // regulariser gradient of the features (rare path): through buffer 0
        const float4* ex4 = reinterpret_cast<const float4*>(a.extra_f);
#pragma unroll
        for (int k = 0; k < 3; ++k) buf[0][k * 64 + lane] = ex4[f4 + k * 64 + lane];
        wave_lds_order();
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int f = 0; f < 3; ++f) {
          const float gj = f == 0 ? g[k].x : (f == 1 ? g[k].y : g[k].z);
          const int j = k * 3 + f;
          p[j] = feature_update<FEATCORR>(a, gj, a.extra_f ? b0[(k * 64 + lane) * 3 + f] : 0.0f, FEATCORR ? fg[j] : 0.0f, p[j], m[j], v[j]);
        }
      wave_lds_order();
      // back through LDS: every lane writes its 12 values of each stream, the wave stores three float4 instructions
      float* w0 = reinterpret_cast<float*>(buf[0]);
      float* w1 = reinterpret_cast<float*>(buf[1]);
      float* w2 = reinterpret_cast<float*>(buf[2]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int f = 0; f < 3; ++f) {
          const int i = (k * 64 + lane) * 3 + f;
          w0[i] = p[k * 3 + f]; w1[i] = m[k * 3 + f]; w2[i] = v[k * 3 + f];
        }
      wave_lds_order();
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        feat[f4 + k * 64 + lane] = buf[0][k * 64 + lane];
        m_f[f4 + k * 64 + lane] = buf[1][k * 64 + lane];
        v_f[f4 + k * 64 + lane] = buf[2][k * 64 + lane];
      }
      wave_lds_order();   // (the buffers are reused by the next chunk)
    }
    if (a.m_d) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long i = vb + k * 64 + lane;
        d[k] = density_update(a, i, g[k].w, d[k], md[k], vd[k]);
        a.dens[i] = d[k];
        a.m_d[i] = md[k];
        a.v_d[i] = vd[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gpacked[vb + k * 64 + lane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      packed[vb + k * 64 + lane] = make_float4(p[k * 3], p[k * 3 + 1], p[k * 3 + 2], pre_activate(a.pre_act, d[k], a.scale));
    }
  }
}

// the same step with one thread per ELEMENT of the packed arrays (wide texels, see pack_grid_wide_kernel)
template <int C>
__global__ __launch_bounds__(256) void grid_adam_wide_kernel(StepArgs a, long long vox_begin, long long vox_end, int bricked, int Y, int Z) {
  constexpr int F = C - 1;
  const unsigned e_end = (unsigned)(vox_end * C), stride = gridDim.x * blockDim.x;
  for (unsigned e = (unsigned)(vox_begin * C) + blockIdx.x * blockDim.x + threadIdx.x; e < e_end; e += stride) {
    const unsigned i = e / C, ch = e - i * C;
    const long long se = grad_slot(i, bricked, Y, Z) * C + ch;
    const float g = a.gpacked[se];
    a.gpacked[se] = 0.0f;
    a.packed[e] = ch < F ? feature_element<false>(a, i * F + ch, g, 0.0f) : density_element(a, i, g);
  }
}

// r04: the wide-texel step with 16-byte accesses (the scheme of pack_grid_wide16_kernel): a block takes chunks of kWideChunk voxels;
// the chunk's packed gradient goes through LDS, the feature-side arrays (feat, exp_avg, exp_avg_sq, extra gradient: [voxel][F], contiguous
// per chunk) move as float4, the updated texels are assembled in the same LDS buffer and leave as float4
// (grid_adam_wide_kernel: 9 four-byte accesses per element, 1.5 ms for a 28-channel 160^3 grid).
template <int C>
__global__ __launch_bounds__(256) void grid_adam_wide16_kernel(StepArgs a, long long vox_begin, long long nchunks) {
  constexpr int F = C - 1, V = kWideChunk;
  __shared__ float4 buf4[V * C / 4];
  float* const buf = reinterpret_cast<float*>(buf4);
  const int tid = threadIdx.x;
  for (long long ck = blockIdx.x; ck < nchunks; ck += gridDim.x) {
    const long long v0 = vox_begin + ck * V;
    float4* __restrict__ g4 = reinterpret_cast<float4*>(a.gpacked + v0 * C);
    for (int q = tid; q < V * C / 4; q += 256) {
      buf4[q] = g4[q];
      g4[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    float4* __restrict__ f4 = reinterpret_cast<float4*>(a.feat + v0 * F);
    for (int q = tid; q < V * F / 4; q += 256) {
      const float4 pf = f4[q];
      float p[4] = {pf.x, pf.y, pf.z, pf.w};
      int slot[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = 4 * q + u, i = idx / F;
        slot[u] = i * C + (idx - i * F);
      }
      if (a.m_f) {
        float4* __restrict__ m4 = reinterpret_cast<float4*>(a.m_f + v0 * F);
        float4* __restrict__ v4 = reinterpret_cast<float4*>(a.v_f + v0 * F);
        const float4 mm = m4[q], vv = v4[q];
        float m[4] = {mm.x, mm.y, mm.z, mm.w}, v[4] = {vv.x, vv.y, vv.z, vv.w};
        float ex[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (a.extra_f) {
          const float4 e4 = reinterpret_cast<const float4*>(a.extra_f + v0 * F)[q];
          ex[0] = e4.x; ex[1] = e4.y; ex[2] = e4.z; ex[3] = e4.w;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = feature_update<false>(a, buf[slot[u]], ex[u], 0.0f, p[u], m[u], v[u]);
        f4[q] = make_float4(p[0], p[1], p[2], p[3]);
        m4[q] = make_float4(m[0], m[1], m[2], m[3]);
        v4[q] = make_float4(v[0], v[1], v[2], v[3]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) buf[slot[u]] = p[u];    // (every slot is read above by the thread that overwrites it)
    }
    if (tid < V) buf[tid * C + F] = density_element(a, v0 + tid, buf[tid * C + F]);
    __syncthreads();
    float4* __restrict__ p4 = reinterpret_cast<float4*>(a.packed + v0 * C);
    for (int q = tid; q < V * C / 4; q += 256) p4[q] = buf4[q];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// Host-side launchers (called from voxe_api.hip)
// ------------------------------------------------------------------------------------------------
static inline int blocks_of(long long threads, int most) { return (int)((threads + 255) / 256 < most ? (threads + 255) / 256 : most); }

template <int C>
static void launch_pack(const VoxeGridDesc* gd, float* packed, hipStream_t st) {
  const long long nvox = (long long)gd->X * gd->Y * gd->Z;
  if constexpr (C > 4) {
    constexpr int F = C - 1;
    long long done = 0;   // voxels converted by the 16-byte kernel (whole chunks; needs 16-byte aligned tensors)
    if (al16(gd->features) && al16(packed) && nvox >= kWideChunk) {
      const long long nchunks = nvox / kWideChunk;
      pack_grid_wide16_kernel<C><<<(int)(nchunks < 4096 ? nchunks : 4096), 256, 0, st>>>(
          gd->densities, gd->features, packed, nchunks, gd->density_scale, gd->density_pre_act);
      done = nchunks * kWideChunk;
    }
    if (done < nvox)
      pack_grid_wide_kernel<C><<<blocks_of((nvox - done) * C, 16384), 256, 0, st>>>(
          gd->densities + done, gd->features + done * F, packed + done * C, nvox - done, gd->density_scale, gd->density_pre_act);
  } else {
    pack_grid_kernel<C><<<blocks_of(nvox, 4096), 256, 0, st>>>(gd->densities, gd->features, packed, nvox, gd->density_scale,
                                                               gd->density_pre_act);
  }
}

template <int C>
static void launch_unpack(const VoxeGridDesc* gd, const float* gpacked, float* d_dens, float* d_feat, int accumulate, int bricked,
                          hipStream_t st) {
  const long long nvox = (long long)gd->X * gd->Y * gd->Z;
  if constexpr (C > 4) {
    constexpr int F = C - 1;
    long long done = 0;
    if (!bricked && al16(gpacked) && (!d_feat || al16(d_feat)) && nvox >= kWideChunk) {
      const long long nchunks = nvox / kWideChunk;
      unpack_grad_wide16_kernel<C><<<(int)(nchunks < 4096 ? nchunks : 4096), 256, 0, st>>>(
          gpacked, gd->densities, d_dens, d_feat, nchunks, gd->density_scale, gd->density_pre_act, accumulate);
      done = nchunks * kWideChunk;
    }
    if (done < nvox)   // (the tail: not bricked here -- a bricked buffer takes the element kernel whole)
      unpack_grad_wide_kernel<C><<<blocks_of((nvox - done) * C, 16384), 256, 0, st>>>(
          gpacked + done * C, gd->densities + done, d_dens ? d_dens + done : nullptr, d_feat ? d_feat + done * F : nullptr,
          nvox - done, gd->density_scale, gd->density_pre_act, accumulate, done ? 0 : bricked, gd->Y, gd->Z);
  } else {
    unpack_grad_kernel<C><<<blocks_of(nvox, 4096), 256, 0, st>>>(gpacked, gd->densities, d_dens, d_feat, nvox, gd->density_scale,
                                                                 gd->density_pre_act, accumulate, bricked, gd->Y, gd->Z);
  }
}

// voxels [vb, ve) of the step; flip: sweep direction of the coalesced kernel
template <int C>
static void launch_grid_adam_t(const VoxeGridDesc* gd, const StepArgs& a, bool bricked, long long vb, long long ve, int flip,
                               hipStream_t st) {
  if constexpr (C > 4) {
    if (!bricked && vb % 4 == 0 && ve - vb >= kWideChunk && al16(a.gpacked) && al16(a.feat) && al16(a.m_f) && al16(a.v_f) &&
        al16(a.extra_f) && al16(a.packed)) {
      const long long nchunks = (ve - vb) / kWideChunk;
      grid_adam_wide16_kernel<C><<<(int)(nchunks < 4096 ? nchunks : 4096), 256, 0, st>>>(a, vb, nchunks);
      vb += nchunks * kWideChunk;
    }
    if (vb < ve)   // bricked gradient buffers, unaligned slabs, the last (ve - vb) % 64 voxels
      grid_adam_wide_kernel<C><<<blocks_of((ve - vb) * C, 4 * kStepBlocks), 256, 0, st>>>(a, vb, ve, bricked ? 1 : 0, gd->Y, gd->Z);
  } else {
    if constexpr (C == 4) {
      if (!bricked && vb % 4 == 0 && ve - vb >= 256 && al16(a.gpacked) && al16(a.dens) && al16(a.feat) && al16(a.extra_d) &&
          al16(a.extra_f) && al16(a.m_d) && al16(a.v_d) && al16(a.m_f) && al16(a.v_f) && al16(a.packed) && al16(a.dcl.fref)) {
        const long long nchunks = (ve - vb) / 256;
        const int nb5 = (int)((nchunks + 3) / 4 < kStepBlocks ? (nchunks + 3) / 4 : kStepBlocks);
        // (two instantiations: see FEATCORR above)
        if (a.dcl.fref && a.m_f) grid_adam_v5_kernel<true><<<nb5, 256, 0, st>>>(a, vb, (int)nchunks, flip);
        else grid_adam_v5_kernel<false><<<nb5, 256, 0, st>>>(a, vb, (int)nchunks, flip);
        vb += nchunks * 256;
        if (vb < ve)   // fewer than 256 voxels left: the per-voxel kernel
          grid_adam_kernel<C><<<1, 256, 0, st>>>(a, vb, ve, 0, gd->Y, gd->Z);
        return;
      }
    }
    grid_adam_kernel<C><<<blocks_of(ve - vb, kStepBlocks), 256, 0, st>>>(a, vb, ve, bricked ? 1 : 0, gd->Y, gd->Z);
  }
}

// the channel counts that have kernels: fn(integral_constant<int, C>) for C = channels, false for any other count
template <class Fn>
static bool for_texel(int channels, Fn&& fn) {
  switch (channels) {
    case 2: fn(std::integral_constant<int, 2>()); return true;
    case 4: fn(std::integral_constant<int, 4>()); return true;
    case 13: fn(std::integral_constant<int, 13>()); return true;
    case 28: fn(std::integral_constant<int, 28>()); return true;
    case 49: fn(std::integral_constant<int, 49>()); return true;
  }
  return false;
}

bool launch_grid_adam(const VoxeGridDesc* gd, bool bricked, int x_begin, int x_end, float* gpacked, const float* extra_d, const float* extra_f,
                      float* m_d, float* v_d, float* m_f, float* v_f, float lr, float beta1, float beta2, float eps,
                      long long step_d, long long step_f, float* packed_out, hipStream_t st, DclTerm dcl) {
  // torch.optim.Adam keeps one step counter PER PARAMETER: the two tensors' bias corrections may differ (a tensor that
  // skipped a step, e.g. a regulariser-only iteration on the densities)
  const StepArgs a{gpacked, const_cast<float*>(gd->densities), const_cast<float*>(gd->features), m_d, v_d, m_f, v_f, packed_out,
                   extra_d, extra_f, gd->density_scale, gd->density_pre_act, adam_hyper(lr, beta1, beta2, eps, step_d),
                   adam_hyper(lr, beta1, beta2, eps, step_f), dcl};
  const long long plane = (long long)gd->Y * gd->Z;
  const int flip = (int)(step_d & 1);   // alternate sweep direction: the tail of one step's sweep is the head of the next (Infinity Cache)
  return for_texel(gd->F + 1, [&](auto c) { launch_grid_adam_t<decltype(c)::value>(gd, a, bricked, x_begin * plane, x_end * plane, flip, st); });
}

void launch_pack_any(const VoxeGridDesc* gd, float* packed, hipStream_t st) {
  for_texel(gd->F + 1, [&](auto c) { launch_pack<decltype(c)::value>(gd, packed, st); });
}
void launch_unpack_any(const VoxeGridDesc* gd, const float* gpacked, float* d_dens, float* d_feat, int accumulate, int bricked,
                       hipStream_t st) {
  for_texel(gd->F + 1, [&](auto c) { launch_unpack<decltype(c)::value>(gd, gpacked, d_dens, d_feat, accumulate, bricked, st); });
}

}  // namespace voxe
