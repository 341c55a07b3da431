// voxe_robust.hip -- robust photometric loss for captures with transient objects ("Robust loss"):
// RobustNeRF's trimmed loss on a batch of pixel patches x, y [N,P,P,C].  The inlier mask comes from an exact order statistic of
// the batch's residuals and is smoothed over each pixel's 3x3 neighbourhood and over its patch; the mask is a constant of the
// loss.
//
//   key      : e_p = d_0 d_0 + d_1 d_1 + ... (float, in that order, d = x - y) is non-negative, so its bit pattern with the
//              sign bit cleared orders like the value (+inf above every finite value, a NaN above +inf).  The 32-bit key is cut
//              into digits of 11, 11 and 10 bits.
//   select   : three counting passes, one per digit.  A pass counts the digit of every key that shares the digits found so far
//              (LDS integer atomics per block, then one global integer atomic per block and non-empty bin); every block of the
//              next pass scans that histogram for the bin that holds the rank (a prefix sum over 2048 integers) and block 0
//              records it for the pass after.  tau is the key of 0-based rank `rank`: exact, no interpolation, integer counters
//              only, so the same bits whatever the order of the patches.
//   mask     : one block per patch keeps the patch's inlier bits a = (key <= tau) in LDS, counts each pixel's 3x3 neighbourhood
//              inside the patch (b), c = a | b, counts c over the patch (D), w = c | (D & inner).  Every comparison is an
//              integer one.  The same block forms its pixels' loss terms and d_x.
//   sums     : loss and mse are double sums: per thread, per block in a fixed tree, over the patches in a fixed order.  The
//              three inlier counts are 64-bit integer atomics.  No float atomic is issued.
#include <hip/hip_runtime.h>

#include "voxe_launch.hpp"

namespace voxe {
namespace {

constexpr int kRobThreads = 256;
constexpr int kRobBins = 2048;                       // bins of one digit's histogram (the last digit uses 1024 of them)
constexpr int kRobBinsPerThread = kRobBins / kRobThreads;
constexpr int kRobPixPerBlock = 512;                 // pixels a block of a counting pass reads
constexpr int kRobMaxSide = 64;
constexpr int kRobShift[3] = {21, 10, 0};
constexpr unsigned kRobDigitMask[3] = {0x7ffu, 0x7ffu, 0x3ffu};

// the head of the scratch, cleared before every call that selects
struct RobustHead {
  unsigned hist[3][kRobBins];
  unsigned prefix[3];            // [l]: the digits found by levels 0..l, in place (the bits below them are 0); [2] = tau's key
  unsigned remaining[3];         // [l]: the rank among the keys that share prefix[l]'s digits
  unsigned long long stats[3];   // sum a, sum c, sum w
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
long long count_blocks(long long M) { return (M + kRobPixPerBlock - 1) / kRobPixPerBlock; }

// The bin of `hist` that holds 0-based rank `rank`, and the rank inside that bin: thread t owns bins [8t, 8t + 8), the block
// forms the prefix sums of the threads' totals, and the one thread whose range holds the rank walks its bins.  A rank at or
// above the histogram's total (it cannot happen: every level counts the keys the previous level's bin held) answers bin 0.
__device__ __forceinline__ void rob_find_bin(const unsigned* __restrict__ hist, unsigned rank, unsigned* sm_wave, unsigned* sm_out) {
  unsigned h[kRobBinsPerThread];
  unsigned total = 0;
#pragma unroll
  for (int i = 0; i < kRobBinsPerThread; ++i) {
    h[i] = hist[threadIdx.x * kRobBinsPerThread + i];
    total += h[i];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = total;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  if (threadIdx.x == 0) {
    sm_out[0] = 0u;
    sm_out[1] = 0u;
  }
  if (lane == 63) sm_wave[wave] = incl;
  __syncthreads();
  unsigned before = incl - total;
  for (int w = 0; w < wave; ++w) before += sm_wave[w];
  if (rank >= before && rank - before < total) {
    unsigned r = rank - before;
    int b = 0;
#pragma unroll
    for (int i = 0; i < kRobBinsPerThread - 1; ++i) {
      if (b == i && r >= h[i]) {
        r -= h[i];
        b = i + 1;
      }
    }
    sm_out[0] = (unsigned)(threadIdx.x * kRobBinsPerThread + b);
    sm_out[1] = r;
  }
  __syncthreads();
}

__device__ __forceinline__ unsigned rob_key(const float* __restrict__ x, const float* __restrict__ y, long long p, int C) {
  const float d0 = x[p * C] - y[p * C];
  float e = d0 * d0;
  for (int c = 1; c < C; ++c) {
    const float d = x[p * C + c] - y[p * C + c];
    e = e + d * d;
  }
  return __float_as_uint(e) & 0x7fffffffu;
}

// One counting pass.  LEVEL 0 forms the keys from x and y and stores them; LEVEL 1 and 2 read them back, find the previous
// level's bin (block 0 records it) and count the next digit of the keys inside it.
template <int LEVEL>
__global__ __launch_bounds__(kRobThreads) void robust_count_kernel(const float* __restrict__ x, const float* __restrict__ y, int M,
                                                                   int C, unsigned rank, RobustHead* head,
                                                                   unsigned* __restrict__ keys) {
  __shared__ unsigned sh[kRobBins];
  __shared__ unsigned sm_wave[kRobThreads / 64];
  __shared__ unsigned sm_out[2];
  for (int i = threadIdx.x; i < kRobBins; i += kRobThreads) sh[i] = 0u;
  unsigned prefix = 0u;
  if constexpr (LEVEL > 0) {
    const unsigned before = LEVEL == 1 ? 0u : head->prefix[LEVEL - 2];
    const unsigned r = LEVEL == 1 ? rank : head->remaining[LEVEL - 2];
    rob_find_bin(head->hist[LEVEL - 1], r, sm_wave, sm_out);
    prefix = before | (sm_out[0] << kRobShift[LEVEL - 1]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      head->prefix[LEVEL - 1] = prefix;
      head->remaining[LEVEL - 1] = sm_out[1];
    }
  } else {
    __syncthreads();
  }
  const long long base = (long long)blockIdx.x * kRobPixPerBlock;
  for (int i = threadIdx.x; i < kRobPixPerBlock; i += kRobThreads) {
    const long long p = base + i;
    if (p >= M) break;
    unsigned k;
    if constexpr (LEVEL == 0) {
      k = rob_key(x, y, p, C);
      keys[p] = k;
      (void)atomicAdd(&sh[k >> kRobShift[0]], 1u);
    } else {
      k = keys[p];
      // (the digits above this level's: a shift by kRobShift[LEVEL - 1] drops this digit and those below)
      if ((k >> kRobShift[LEVEL - 1]) == (prefix >> kRobShift[LEVEL - 1]))
        (void)atomicAdd(&sh[(k >> kRobShift[LEVEL]) & kRobDigitMask[LEVEL]], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kRobBins; i += kRobThreads) {
    const unsigned v = sh[i];
    if (v != 0u) (void)atomicAdd(&head->hist[LEVEL][i], v);
  }
}

// out[i] = sum of v[i] over the block: lanes by a shuffle tree, then the waves in order (threads i < 2 write)
__device__ __forceinline__ void rob_block_sum2(double (&v)[2], double* __restrict__ out) {
  __shared__ double sm[kRobThreads / 64][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sm[threadIdx.x >> 6][0] = v[0];
    sm[threadIdx.x >> 6][1] = v[1];
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kRobThreads / 64; ++w) s += sm[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// One block per patch.  SELECT: the mask from the keys and the last histogram; else from mask_in.  mask_in and mask_out are
// read and written by the same thread at the same index, the read first: they may be one buffer.
template <bool SELECT, bool L1>
__global__ __launch_bounds__(kRobThreads) void robust_patch_kernel(const float* __restrict__ x, const float* __restrict__ y, int P,
                                                                   int C, int smooth_min, int patch_min, float g,
                                                                   const unsigned char* mask_in, RobustHead* head,
                                                                   const unsigned* __restrict__ keys, unsigned char* mask_out,
                                                                   float* __restrict__ d_x, double* __restrict__ partial) {
  __shared__ unsigned char sa[kRobMaxSide * kRobMaxSide];
  __shared__ unsigned char sc[kRobMaxSide * kRobMaxSide];
  __shared__ unsigned sm_wave[kRobThreads / 64];
  __shared__ unsigned sm_out[2];
  __shared__ int cnt[3];
  const int PP = P * P;
  const long long base = (long long)blockIdx.x * PP;
  bool whole = false;
  if constexpr (SELECT) {
    rob_find_bin(head->hist[2], head->remaining[1], sm_wave, sm_out);
    const unsigned tau = head->prefix[1] | sm_out[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) head->prefix[2] = tau;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < PP; i += kRobThreads) sa[i] = keys[base + i] <= tau ? 1 : 0;
    __syncthreads();
    int na = 0, nc = 0;
    for (int i = threadIdx.x; i < PP; i += kRobThreads) {
      const int r = i / P, c = i - r * P;
      int n = 0;
      for (int dr = -1; dr <= 1; ++dr) {
        const int rr = r + dr;
        if (rr < 0 || rr >= P) continue;
        for (int dc = -1; dc <= 1; ++dc) {
          const int cc = c + dc;
          if (cc >= 0 && cc < P) n += sa[rr * P + cc];
        }
      }
      const int a = sa[i];
      const int cv = a | (n >= smooth_min ? 1 : 0);
      sc[i] = (unsigned char)cv;
      na += a;
      nc += cv;
    }
    if (na) (void)atomicAdd(&cnt[0], na);
    if (nc) (void)atomicAdd(&cnt[1], nc);
    __syncthreads();
    whole = cnt[1] >= patch_min;
  }
  const int lo = P / 4, hi = P / 4 + P / 2;
  const float wg = L1 ? g : 2.0f * g;
  double sums[2] = {0.0, 0.0};   // loss, mse
  int nw = 0;
  for (int i = threadIdx.x; i < PP; i += kRobThreads) {
    int w;
    if constexpr (SELECT) {
      const int r = i / P, c = i - r * P;
      const bool inner = r >= lo && r < hi && c >= lo && c < hi;
      w = sc[i] | ((whole && inner) ? 1 : 0);
      nw += w;
    } else {
      w = mask_in[base + i] != 0 ? 1 : 0;
    }
    if (mask_out) mask_out[base + i] = (unsigned char)w;
    if (partial || d_x) {
      const float wf = w ? 1.0f : 0.0f;
      const long long o = (base + i) * C;
      for (int c = 0; c < C; ++c) {
        const float d = x[o + c] - y[o + c];
        const double d2 = (double)d * (double)d;
        if (w) sums[0] += L1 ? (double)fabsf(d) : d2;
        sums[1] += d2;
        // sign(0) = 0
        if (d_x) d_x[o + c] = L1 ? (wf * wg) * (float)((d > 0.0f) - (d < 0.0f)) : (wf * wg) * d;
      }
    }
  }
  if constexpr (SELECT) {
    if (nw) (void)atomicAdd(&cnt[2], nw);
    __syncthreads();
    if (threadIdx.x < 3 && cnt[threadIdx.x] != 0)
      (void)__hip_atomic_fetch_add(&head->stats[threadIdx.x], (unsigned long long)cnt[threadIdx.x], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
  }
  if (partial) rob_block_sum2(sums, partial + (long long)blockIdx.x * 2);
}

// one block: the two scalars from the per-patch partials in a fixed order, tau and the counts from the head (zeros without one)
__global__ __launch_bounds__(kRobThreads) void robust_finalize_kernel(const double* __restrict__ partial, long long nb, double inv_n,
                                                                      const RobustHead* __restrict__ head,
                                                                      float* __restrict__ loss_out, float* __restrict__ mse_out,
                                                                      float* __restrict__ tau_out, long long* __restrict__ stats) {
  if (threadIdx.x == 0 && tau_out) *tau_out = head ? __uint_as_float(head->prefix[2]) : 0.0f;
  if (threadIdx.x < 3 && stats) stats[threadIdx.x] = head ? (long long)head->stats[threadIdx.x] : 0ll;
  if (partial) {
    __shared__ double tot[2];
    double s[2] = {0.0, 0.0};
    for (long long i = threadIdx.x; i < nb; i += kRobThreads) {
      s[0] += partial[i * 2];
      s[1] += partial[i * 2 + 1];
    }
    rob_block_sum2(s, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
      if (loss_out) *loss_out = (float)(tot[0] * inv_n);
      if (mse_out) *mse_out = (float)(tot[1] * inv_n);
    }
  }
}

}  // namespace

// the head, the keys [M] (uint32), then two double partials per patch
size_t robust_scratch_bytes(long long N, long long P) {
  const size_t M = (size_t)N * (size_t)P * (size_t)P;
  return align256(sizeof(RobustHead)) + align256(sizeof(unsigned) * M) + sizeof(double) * 2 * (size_t)N + 256;
}

bool launch_robust(const float* x, const float* y, int N, int P, int C, bool l1, long long rank, int smooth_min, int patch_min,
                   const unsigned char* mask_in, float grad_scale, float* loss_out, float* mse_out, float* tau_out,
                   unsigned char* mask_out, long long* stats, float* d_x, void* scratch, hipStream_t st) {
  const int M = N * P * P;
  RobustHead* head = (RobustHead*)scratch;
  unsigned* keys = (unsigned*)((char*)scratch + align256(sizeof(RobustHead)));
  double* partial = (loss_out || mse_out) ? (double*)((char*)keys + align256(sizeof(unsigned) * (size_t)M)) : nullptr;
  const float g = (float)((double)grad_scale / ((double)C * (double)M));
  const bool per_pixel = mask_out || d_x || partial;
  if (!mask_in) {
    if (hipMemsetAsync(head, 0, sizeof(RobustHead), st) != hipSuccess) return false;
    const unsigned cb = (unsigned)count_blocks(M);
    robust_count_kernel<0><<<cb, kRobThreads, 0, st>>>(x, y, M, C, (unsigned)rank, head, keys);
    robust_count_kernel<1><<<cb, kRobThreads, 0, st>>>(x, y, M, C, (unsigned)rank, head, keys);
    robust_count_kernel<2><<<cb, kRobThreads, 0, st>>>(x, y, M, C, (unsigned)rank, head, keys);
    // (tau and the counts come out of the patch pass, so they need it even when no per-pixel output is asked for)
    if (l1)
      robust_patch_kernel<true, true><<<(unsigned)N, kRobThreads, 0, st>>>(x, y, P, C, smooth_min, patch_min, g, nullptr, head, keys,
                                                                           mask_out, d_x, partial);
    else
      robust_patch_kernel<true, false><<<(unsigned)N, kRobThreads, 0, st>>>(x, y, P, C, smooth_min, patch_min, g, nullptr, head, keys,
                                                                            mask_out, d_x, partial);
  } else if (per_pixel) {
    if (l1)
      robust_patch_kernel<false, true><<<(unsigned)N, kRobThreads, 0, st>>>(x, y, P, C, 0, 0, g, mask_in, nullptr, nullptr, mask_out,
                                                                            d_x, partial);
    else
      robust_patch_kernel<false, false><<<(unsigned)N, kRobThreads, 0, st>>>(x, y, P, C, 0, 0, g, mask_in, nullptr, nullptr, mask_out,
                                                                             d_x, partial);
  }
  if (partial || tau_out || stats)
    robust_finalize_kernel<<<1, kRobThreads, 0, st>>>(partial, N, 1.0 / ((double)C * (double)M), mask_in ? nullptr : head, loss_out,
                                                      mse_out, tau_out, stats);
  return true;
}

}  // namespace voxe
