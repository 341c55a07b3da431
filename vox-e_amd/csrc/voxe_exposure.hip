// voxe_exposure.hip -- per-image exposure compensation ("Exposure"): the photometric loss under a
// learned 3x4 affine colour transform per training image, value and gradients in one call, and the sums of the closed-form
// least-squares affine of the colour-corrected metrics.
//
//   fwd_bwd  : per ray r of image n = image_id[r] (clamped into [0, N)), with delta[n] = (dA row-major 3x3, db):
//                A = I + dA,  c' = A x + db,  e = c' - y,  g = omega_r sign(e) (L1) or 2 omega_r e (L2)
//                loss = sum omega_r |e| or omega_r e^2 over the 3R elements / 3R,  mse = sum e^2 / 3R
//                d_x_r      = gs A^T g                      gs = grad_scale / 3R
//                d_delta[n] = gs sum_{r in n} (g x^T, g)
//              d_delta is a segmented reduction of R rays into at most N rows.  Each of a ray's 12 products is rounded to
//              float, then to a 64-bit fixed-point integer q(t) = (int64) rint(t * 2^32) (voxe_lift.hip's), and from there
//              every add is an integer add:
//                wave  : a wave whose rays name one image folds its 12 integers with a butterfly and one lane deposits;
//                block : a block (1024 consecutive rays) keeps a 64-slot table in LDS keyed by image, filled with 64-bit LDS
//                        integer atomics; an image that finds no slot (more than 64 images in one block) goes to the global
//                        sums directly;
//                grid  : one 64-bit integer atomic per block, image the block met and component into acc[N][12] in the scratch;
//                final : d_delta = (float)(acc * 2^-32 * gs) with the product in double: one float rounding (an unscaled sum
//                        of 2^21 or more does not fit a double's 53 bits and rounds there first, by 2^-53 relative); rows no
//                        ray names hold acc == 0 and are written as exact zeros.  Under accumulate a row with acc == 0 is
//                        left alone, whether no ray names it or its rays cancel exactly: adding 0 changes nothing either way.
//              Integer adds are associative, so d_delta is the same bit for bit from call to call and under any permutation
//              of the rays.  No float atomic is issued.  loss and mse are double sums: per thread, per block in a fixed tree,
//              over the blocks in a fixed order.
//   fit_sums : per image the 25 sums of the normal equations of y ~ A x + b, products and sums in double, a fixed tree per
//              block of 2048 pixels and the blocks of an image in order: the same bits from call to call.
#include <hip/hip_runtime.h>

#include "voxe_launch.hpp"

namespace voxe {
namespace {

constexpr int kExpThreads = 256;
constexpr int kExpChunks = 4;                               // chunks of kExpThreads consecutive rays per block
constexpr int kExpRaysPerBlock = kExpThreads * kExpChunks;
constexpr int kExpSlots = 64;                               // images a block keeps in LDS (a power of two)
constexpr float kExpOne = 4294967296.0f;                    // 2^32: the scaling is exact in float
constexpr int kFitPixPerBlock = 2048;
constexpr int kFitSums = 25;

__device__ __forceinline__ long long exp_quantise(float t) { return __float2ll_rn(t * kExpOne); }

__device__ __forceinline__ void exp_add_global(long long* p, long long v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ long long exp_shfl_xor(long long v, int off) {
  const int lo = __shfl_xor((int)(unsigned)(unsigned long long)v, off, 64);
  const int hi = __shfl_xor((int)(unsigned)((unsigned long long)v >> 32), off, 64);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}

// out[i] = sum of v[i] over the block: lanes by a shuffle tree, then the waves in order (threads i < NV write)
template <int NV>
__device__ __forceinline__ void exp_block_sum(double (&v)[NV], double* __restrict__ out) {
  __shared__ double sm[kExpThreads / 64][NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) sm[threadIdx.x >> 6][i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kExpThreads / 64; ++w) s += sm[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// the slot of image `id` in the block's table, claimed on first use; -1: the table is full of other images
__device__ __forceinline__ int exp_find_slot(int* keys, int id) {
  int s = id & (kExpSlots - 1);
  for (int p = 0; p < kExpSlots; ++p) {
    const int prev = atomicCAS(&keys[s], -1, id);
    if (prev == -1 || prev == id) return s;
    s = (s + 1) & (kExpSlots - 1);
  }
  return -1;
}

// MODE: the loss kinds, or kExpUpstream: `y` holds dL/dc' of a loss outside this file in place of the targets, g = y * gs with
// gs a power of two that brings the products near 1 for the fixed point (apply_bwd), and nothing but d_x and acc is produced
constexpr int kExpL2 = 0, kExpL1 = 1, kExpUpstream = 2;

template <int MODE>
__global__ __launch_bounds__(kExpThreads) void exposure_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const int* __restrict__ ids, const float* __restrict__ delta,
                                                               const float* __restrict__ rweight, long long R, int N, float gs,
                                                               float* __restrict__ corrected, float* __restrict__ d_x,
                                                               long long* acc, double* __restrict__ partial) {
  __shared__ int keys[kExpSlots];
  __shared__ long long tab[kExpSlots * 12];
  if (acc) {
    for (int i = threadIdx.x; i < kExpSlots; i += kExpThreads) keys[i] = -1;
    for (int i = threadIdx.x; i < kExpSlots * 12; i += kExpThreads) tab[i] = 0ll;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  double sums[2] = {0.0, 0.0};   // loss, mse
  const long long base = (long long)blockIdx.x * kExpRaysPerBlock;
  for (int ch = 0; ch < kExpChunks; ++ch) {
    const long long r = base + (long long)ch * kExpThreads + threadIdx.x;
    const bool valid = r < R;
    int id = -1;
    long long q[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) q[i] = 0ll;
    if (valid) {
      id = min(max(ids[r], 0), N - 1);   // an id out of range is clamped: nothing is read or written out of bounds
      const float* dl = delta + (long long)id * 12;
      float a[3][3], xv[3], g[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) xv[j] = x[r * 3 + j];
      const float w = rweight ? rweight[r] : 1.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a[c][j] = c == j ? 1.0f + dl[c * 3 + j] : dl[c * 3 + j];
        if constexpr (MODE == kExpUpstream) {
          g[c] = y[r * 3 + c];
        } else {
          const float cc = fmaf(a[c][2], xv[2], fmaf(a[c][1], xv[1], fmaf(a[c][0], xv[0], dl[9 + c])));
          const float e = cc - y[r * 3 + c];
          if (corrected) corrected[r * 3 + c] = cc;
          const double e2 = (double)e * (double)e;
          sums[0] += MODE == kExpL1 ? (double)w * (double)fabsf(e) : (double)w * e2;
          sums[1] += e2;
          // sign(0) = 0
          g[c] = MODE == kExpL1 ? w * (float)((e > 0.0f) - (e < 0.0f)) : (2.0f * w) * e;
        }
      }
      if (d_x) {
        // (upstream: the gradient as it stands, gs only scales the fixed point)
        const float s = MODE == kExpUpstream ? 1.0f : gs;
#pragma unroll
        for (int j = 0; j < 3; ++j) d_x[r * 3 + j] = s * fmaf(a[2][j], g[2], fmaf(a[1][j], g[1], a[0][j] * g[0]));
      }
      if constexpr (MODE == kExpUpstream) {
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] *= gs;   // (a power of two: exact)
      }
      if (acc) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
          for (int j = 0; j < 3; ++j) q[c * 3 + j] = exp_quantise(g[c] * xv[j]);
          q[9 + c] = exp_quantise(g[c]);
        }
      }
    }
    if (acc) {
      // (the chunk loop and this branch are uniform over the wave: every lane joins the shuffles)
      const unsigned long long live = __ballot(valid);
      if (live != 0ull) {
        const int lead = __ffsll((long long)live) - 1;
        const int first = __shfl(id, lead, 64);
        const bool one_image = __all(!valid || id == first);
        if (one_image) {
#pragma unroll
          for (int i = 0; i < 12; ++i) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) q[i] += exp_shfl_xor(q[i], off);
          }
        }
        if (valid && (!one_image || lane == lead)) {
          const int s = exp_find_slot(keys, id);
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            if (q[i] == 0ll) continue;   // (an exact no-op)
            if (s >= 0)
              (void)atomicAdd((unsigned long long*)&tab[s * 12 + i], (unsigned long long)q[i]);
            else
              exp_add_global(acc + (long long)id * 12 + i, q[i]);
          }
        }
      }
    }
  }
  if (acc) {
    __syncthreads();
    for (int i = threadIdx.x; i < kExpSlots * 12; i += kExpThreads) {
      const int k = keys[i / 12];
      const long long v = tab[i];
      if (k >= 0 && v != 0ll) exp_add_global(acc + (long long)k * 12 + (i % 12), v);
    }
  }
  if (partial) exp_block_sum<2>(sums, partial + (long long)blockIdx.x * 2);
}

// block 0: the two scalars from the per-block partials, fixed order; every block: its share of d_delta from the integer sums
__global__ __launch_bounds__(kExpThreads) void exposure_finalize_kernel(const double* __restrict__ partial, long long nb,
                                                                        double inv_n, const long long* __restrict__ acc,
                                                                        long long nd, double gsd, int accumulate,
                                                                        float* __restrict__ loss_out, float* __restrict__ mse_out,
                                                                        float* __restrict__ d_delta) {
  if (d_delta) {
    const long long i = (long long)blockIdx.x * kExpThreads + threadIdx.x;
    if (i < nd) {
      const long long a = acc[i];
      const float v = (float)(((double)a * 0x1p-32) * gsd);
      if (!accumulate)
        d_delta[i] = v;
      else if (a != 0ll)
        d_delta[i] += v;
    }
  }
  if (blockIdx.x == 0 && partial) {
    __shared__ double tot[2];
    double s[2] = {0.0, 0.0};
    for (long long i = threadIdx.x; i < nb; i += kExpThreads) {
      s[0] += partial[i * 2];
      s[1] += partial[i * 2 + 1];
    }
    exp_block_sum<2>(s, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
      if (loss_out) *loss_out = (float)(tot[0] * inv_n);
      if (mse_out) *mse_out = (float)(tot[1] * inv_n);
    }
  }
}

// the 25 sums of one block's pixels of image blockIdx.y
__global__ __launch_bounds__(kExpThreads) void exposure_fit_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                   long long P, double* __restrict__ out) {
  const long long n = blockIdx.y;
  const long long p0 = (long long)blockIdx.x * kFitPixPerBlock;
  const long long p1 = min(p0 + (long long)kFitPixPerBlock, P);
  double s[kFitSums];
#pragma unroll
  for (int i = 0; i < kFitSums; ++i) s[i] = 0.0;
  for (long long p = p0 + threadIdx.x; p < p1; p += kExpThreads) {
    const long long o = (n * P + p) * 3;
    const double u[4] = {(double)x[o], (double)x[o + 1], (double)x[o + 2], 1.0};
    const double v[3] = {(double)y[o], (double)y[o + 1], (double)y[o + 2]};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = i; j < 4; ++j) s[k++] += u[i] * u[j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) s[k++] += u[i] * v[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s[k++] += v[c] * v[c];
  }
  exp_block_sum<kFitSums>(s, out + (n * gridDim.x + blockIdx.x) * kFitSums);
}

// sums[n] = the blocks of image n in order
__global__ __launch_bounds__(64) void exposure_fit_finalize_kernel(const double* __restrict__ partial, int nchunk,
                                                                   double* __restrict__ sums) {
  if (threadIdx.x >= kFitSums) return;
  const long long n = blockIdx.x;
  double s = 0.0;
  for (int c = 0; c < nchunk; ++c) s += partial[(n * nchunk + c) * kFitSums + threadIdx.x];
  sums[n * kFitSums + threadIdx.x] = s;
}

long long exposure_blocks(long long R) { return (R + kExpRaysPerBlock - 1) / kExpRaysPerBlock; }
long long fit_chunks(long long P) { return (P + kFitPixPerBlock - 1) / kFitPixPerBlock; }
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

// acc[N][12] (int64), then two double partials per block
size_t exposure_scratch_bytes(long long R, long long N) {
  return align256(sizeof(long long) * 12 * (size_t)N) + sizeof(double) * 2 * (size_t)exposure_blocks(R) + 256;
}

// one set of 25 partials per block of pixels and image; an image of one block writes its sums directly
size_t exposure_fit_scratch_bytes(long long N, long long P) {
  return sizeof(double) * kFitSums * (size_t)N * (size_t)fit_chunks(P) + 256;
}

bool launch_exposure(const float* x, const float* y, const int* ids, const float* delta, const float* rweight, long long R, int N,
                     bool l1, float grad_scale, float* loss_out, float* mse_out, float* corrected, float* d_x, float* d_delta,
                     int accumulate, void* scratch, hipStream_t st) {
  const long long nb = exposure_blocks(R);
  const size_t acc_bytes = sizeof(long long) * 12 * (size_t)N;
  long long* acc = d_delta ? (long long*)scratch : nullptr;
  double* partial = (loss_out || mse_out) ? (double*)((char*)scratch + align256(acc_bytes)) : nullptr;
  if (acc && hipMemsetAsync(acc, 0, acc_bytes, st) != hipSuccess) return false;
  const double gsd = (double)grad_scale / (3.0 * (double)R);
  if (l1)
    exposure_kernel<kExpL1><<<(unsigned)nb, kExpThreads, 0, st>>>(x, y, ids, delta, rweight, R, N, (float)gsd, corrected, d_x, acc,
                                                                   partial);
  else
    exposure_kernel<kExpL2><<<(unsigned)nb, kExpThreads, 0, st>>>(x, y, ids, delta, rweight, R, N, (float)gsd, corrected, d_x, acc,
                                                                   partial);
  if (acc || partial) {
    const long long nd = 12ll * N;
    const long long fb = acc ? (nd + kExpThreads - 1) / kExpThreads : 1;
    exposure_finalize_kernel<<<(unsigned)fb, kExpThreads, 0, st>>>(partial, nb, 1.0 / (3.0 * (double)R), acc, nd, gsd, accumulate,
                                                                  loss_out, mse_out, d_delta);
  }
  return true;
}

// the chain rule of c' = A x + db alone: d_x = A^T d_corrected, d_delta[n] = sum (d_corrected x^T, d_corrected).  The products
// are quantised in units of 2^-33 / R', R' = R rounded up to a power of two: an upstream gradient of a mean over the batch has
// entries near 1 / R
bool launch_exposure_apply_bwd(const float* x, const int* ids, const float* delta, const float* d_corrected, long long R, int N,
                               float* d_x, float* d_delta, int accumulate, void* scratch, hipStream_t st) {
  const long long nb = exposure_blocks(R);
  long long* acc = d_delta ? (long long*)scratch : nullptr;
  if (acc && hipMemsetAsync(acc, 0, sizeof(long long) * 12 * (size_t)N, st) != hipSuccess) return false;
  float unit = 1.0f;
  while ((long long)unit < R) unit *= 2.0f;
  exposure_kernel<kExpUpstream><<<(unsigned)nb, kExpThreads, 0, st>>>(x, d_corrected, ids, delta, nullptr, R, N, unit, nullptr, d_x,
                                                                       acc, nullptr);
  if (acc) {
    const long long nd = 12ll * N;
    exposure_finalize_kernel<<<(unsigned)((nd + kExpThreads - 1) / kExpThreads), kExpThreads, 0, st>>>(
        nullptr, 0, 0.0, acc, nd, 1.0 / (double)unit, accumulate, nullptr, nullptr, d_delta);
  }
  return true;
}

void launch_exposure_fit(const float* x, const float* y, long long N, long long P, double* sums, void* scratch, hipStream_t st) {
  const long long nc = fit_chunks(P);
  double* out = nc == 1 ? sums : (double*)scratch;
  exposure_fit_kernel<<<dim3((unsigned)nc, (unsigned)N), kExpThreads, 0, st>>>(x, y, P, out);
  if (nc > 1) exposure_fit_finalize_kernel<<<(unsigned)N, 64, 0, st>>>((const double*)scratch, (int)nc, sums);
}

}  // namespace voxe
