// voxe_vq.hip -- vector quantisation of feature vectors against a codebook ("Compression").
//
//   assign     : index[n] = arg min_k  |c_k|^2 - 2 x_n . c_k   in float32 on the matrix cores (v_mfma_f32_32x32x2_f32), the
//                arg-min folded into the accumulator epilogue: no N x K buffer exists.
//                A block is 4 waves and 256 points; a wave owns 64 points (two 32-column MFMA tiles) and keeps their fragments
//                in registers for the whole call: B[k][j] = x[point j][channel k], lane l holds channel 2s + (l >> 5) of point
//                l & 31 for k-step s -- KS = ceil(F / 2) registers per point tile, zero padded (fma(0, 0, acc) == acc).  The
//                codebook streams through LDS in tiles of 64 codewords (two 32-row MFMA tiles), double buffered: tile t + 1 is
//                fetched into registers before the MFMAs of tile t issue and stored to the other buffer after them, one barrier
//                per tile.  LDS holds -2 c (the scaling is exact) channel-major, [channel][codeword] with a row stride of 65
//                floats: the A operand A[i][k] = -2 c[codeword i][channel k] of lane l is one conflict-free ds_read_b32, and
//                the transposing store of the row-major global tile is conflict-free too.  The four accumulators of a wave
//                (2 codeword tiles x 2 point tiles) start at |c_k|^2 of their row, so that after KS MFMAs register r of lane l
//                is the score of codeword row (r & 3) + 8 (r >> 2) + 4 (l >> 5) for point l & 31 and the epilogue is a bare
//                compare / select over the 16 registers in ascending row order with a strict <: the lowest k wins among
//                bit-equal scores.  The two lane halves meet once, after the last tile (lower score, then lower k).
//                Rows past K carry |c|^2 = +inf and c = 0: never below the running minimum.
//                dist[n] is then recomputed for the chosen codeword alone in plain float32 (sub, mul, add; the tree is built
//                with -ffp-contract=off), ascending channel.
//   norms      : code_norm[k] = sum_j c_kj^2 (plain float32, ascending j), the pre-pass of the same call.
//   accumulate : one lane per point; sum_w[k] += q(w_n), sum_wx[k, j] += q(w_n x_nj), k = index[n], q(x) = (int64) rint(x 2^32),
//                with 64-bit integer atomics at agent scope: the bits do not depend on any order.  MERGE = true first sums,
//                inside a wave, the integers of each run of consecutive lanes with the same k (a segmented scan over the run
//                heads: on index-sorted points a wave then issues one atomic per run and channel); unsorted points have runs of
//                one lane and fall back to the per-lane atomics.  That variant first stages the block's rows -- one contiguous
//                piece of `points` -- in LDS with coalesced loads (row stride F | 1, so a column read is conflict-free).
//                Points whose index is outside 0..K-1 deposit nothing.
#include <hip/hip_runtime.h>

#include <cmath>

#include "voxe_launch.hpp"

namespace voxe {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kVqThreads = 256;                   // 4 waves
constexpr int kVqTileK = 64;                      // codewords per LDS tile
constexpr int kVqWavePts = 64;                    // points per wave
constexpr int kVqBlockPts = kVqWavePts * (kVqThreads / 64);
constexpr int kVqLd = kVqTileK + 1;               // LDS row stride of one channel (floats)

__global__ __launch_bounds__(256) void vq_norm_kernel(const float* __restrict__ codebook, int K, int F,
                                                      float* __restrict__ code_norm) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  float s = 0.0f;
  for (int j = 0; j < F; ++j) {
    const float c = codebook[(size_t)k * F + j];
    s = s + c * c;
  }
  code_norm[k] = s;
}

// the codeword row of accumulator register r in lane half h (programming guide, C/D map of the 32x32 shapes)
__device__ __forceinline__ constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int KS>
__global__ __launch_bounds__(kVqThreads) void vq_assign_kernel(const float* __restrict__ points, int N, int F,
                                                               const float* __restrict__ codebook, int K,
                                                               const float* __restrict__ code_norm, int* __restrict__ index,
                                                               float* __restrict__ dist) {
  constexpr int CH = 2 * KS;                                            // channels after zero padding
  constexpr int NE = (kVqTileK * CH + kVqThreads - 1) / kVqThreads;      // tile elements a thread stages
  constexpr int kBuf = CH * kVqLd + kVqTileK;                           // one buffer: -2 c channel-major, then the 64 norms
  __shared__ float lds[2 * kBuf];
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
  const long long p0 = (long long)blockIdx.x * kVqBlockPts + (tid >> 6) * kVqWavePts;   // the wave's first point
  const bool active = p0 < N;                                                          // (uniform over the wave)

  // the wave's point fragments, held for the whole call
  float xb[2][KS];
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
    const long long n = p0 + pt * 32 + col;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int ch = 2 * s + half;
      xb[pt][s] = (n < N && ch < F) ? points[n * F + ch] : 0.0f;
    }
  }

  // channels F .. CH-1 stay zero in both buffers: the staging below never touches them
  for (int i = tid; i < 2 * kBuf; i += kVqThreads) lds[i] = 0.0f;
  __syncthreads();

  const int tile_elems = kVqTileK * F, total = K * F;
  int loff[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = tid + i * kVqThreads;
    loff[i] = (e % F) * kVqLd + e / F;
  }
  float stage[NE], stage_norm = 0.0f;
  auto fetch = [&](int t) {
    const int base = t * tile_elems;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + i * kVqThreads;
      stage[i] = (e < tile_elems && base + e < total) ? -2.0f * codebook[base + e] : 0.0f;
    }
    if (tid < kVqTileK) {
      const int k = t * kVqTileK + tid;
      stage_norm = k < K ? code_norm[k] : INFINITY;
    }
  };
  auto stash = [&](float* buf) {
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      if (tid + i * kVqThreads < tile_elems) buf[loff[i]] = stage[i];
    }
    if (tid < kVqTileK) buf[CH * kVqLd + tid] = stage_norm;
  };

  float best[2] = {INFINITY, INFINITY};
  int bidx[2] = {0, 0};
  const int T = (K + kVqTileK - 1) / kVqTileK;
  fetch(0);
  stash(lds);
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const float* buf = lds + (t & 1) * kBuf;
    if (t + 1 < T) fetch(t + 1);
    if (active) {
      f32x16 acc[2][2];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float nrm = buf[CH * kVqLd + rt * 32 + acc_row(r, half)];
          acc[rt][0][r] = nrm;
          acc[rt][1][r] = nrm;
        }
      }
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float a0 = buf[(2 * s + half) * kVqLd + col];
        const float a1 = buf[(2 * s + half) * kVqLd + 32 + col];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, xb[0][s], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, xb[1][s], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, xb[0][s], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, xb[1][s], acc[1][1], 0, 0, 0);
      }
      // ascending rows inside the lane, strict <: the first of equal scores stays
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = t * kVqTileK + rt * 32 + acc_row(r, half);
#pragma unroll
          for (int pt = 0; pt < 2; ++pt) {
            const float v = acc[rt][pt][r];
            if (v < best[pt]) {
              best[pt] = v;
              bidx[pt] = row;
            }
          }
        }
      }
    }
    if (t + 1 < T) stash(lds + ((t + 1) & 1) * kBuf);
    __syncthreads();
  }
  if (!active) return;

  // the lane halves hold disjoint rows of every tile: lower score, then lower k
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
    const float ob = __shfl_xor(best[pt], 32, 64);
    const int oi = __shfl_xor(bidx[pt], 32, 64);
    if (ob < best[pt] || (ob == best[pt] && oi < bidx[pt])) {
      best[pt] = ob;
      bidx[pt] = oi;
    }
  }
  // lane l finishes point tile l >> 5, point l & 31
  const long long n = p0 + half * 32 + col;
  if (n >= N) return;
  const int k = half ? bidx[1] : bidx[0];
  index[n] = k;
  if (dist) {
    float d = 0.0f;
    for (int j = 0; j < F; ++j) {
      const float u = points[n * F + j] - codebook[(size_t)k * F + j];
      d = d + u * u;
    }
    dist[n] = d;
  }
}

constexpr float kVqOne = 4294967296.0f;   // 2^32: the scaling is exact in float
__device__ __forceinline__ long long vq_quantise(float x) { return __float2ll_rn(x * kVqOne); }

__device__ __forceinline__ void vq_add_to(long long* p, long long v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ long long vq_shfl_up_ll(long long v, int off) {
  const int lo = __shfl_up((int)(unsigned)(unsigned long long)v, off, 64);
  const int hi = __shfl_up((int)(unsigned)((unsigned long long)v >> 32), off, 64);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}

constexpr int kVqMergeThreads = 128;   // MERGE stages the block's rows in LDS: 128 x 65 floats at F = 64

template <bool MERGE>
__global__ __launch_bounds__(256) void vq_accumulate_kernel(const float* __restrict__ points, const float* __restrict__ weights,
                                                            const int* __restrict__ index, long long N, int F, int K,
                                                            long long* sum_wx, long long* sum_w) {
  extern __shared__ float vq_rows[];   // MERGE only: [point of the block][channel], row stride F | 1 (odd: conflict-free columns)
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int Fp = F | 1;
  if constexpr (MERGE) {
    // the block's rows are one contiguous piece of `points`: read it coalesced, once (a lane walking its own row reads with a
    // stride of F floats)
    const long long first = (long long)blockIdx.x * blockDim.x;
    const long long left = N - first;
    const int count = (int)(left < (long long)blockDim.x ? left : (long long)blockDim.x) * F;
    for (int e = threadIdx.x; e < count; e += blockDim.x) {
      const int r = e / F;
      vq_rows[r * Fp + (e - r * F)] = points[first * F + e];
    }
    __syncthreads();
  }
  const float* row = vq_rows + threadIdx.x * Fp;
  int k = -1;
  float w = 0.0f;
  if (n < N) {
    k = index[n];
    w = weights[n];
  }
  const bool has = k >= 0 && k < K;
  if constexpr (!MERGE) {
    if (!has) return;
    const long long qw = vq_quantise(w);
    if (qw != 0ll) vq_add_to(sum_w + k, qw);
    for (int j = 0; j < F; ++j) {
      const long long qx = vq_quantise(w * points[n * F + j]);
      if (qx != 0ll) vq_add_to(sum_wx + (size_t)k * F + j, qx);
    }
  } else {
    // runs of consecutive lanes with the same k: `start` = the lane of this lane's run head, `last` = this lane ends its run
    const int key = has ? k : -1 - lane;   // (a lane that deposits nothing is a run of its own)
    const int prev = __shfl_up(key, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || prev != key);
    if (heads == ~0ull) {   // (uniform) no two neighbours share a codeword: nothing to merge
      if (!has) return;
      const long long qw = vq_quantise(w);
      if (qw != 0ll) vq_add_to(sum_w + k, qw);
      for (int j = 0; j < F; ++j) {
        const long long qx = vq_quantise(w * row[j]);
        if (qx != 0ll) vq_add_to(sum_wx + (size_t)k * F + j, qx);
      }
      return;
    }
    const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull) != 0ull;
    unsigned take = 0u, levels = 0u;
#pragma unroll
    for (int l = 0; l < 6; ++l) {
      const bool t = lane - (1 << l) >= start;
      if (t) take |= 1u << l;
      if (__ballot(t) != 0ull) levels |= 1u << l;
    }
    auto run_sum = [&](long long v) {
#pragma unroll
      for (int l = 0; l < 6; ++l) {
        if (levels & (1u << l)) {   // (uniform over the wave)
          const long long p = vq_shfl_up_ll(v, 1 << l);
          if (take & (1u << l)) v += p;
        }
      }
      return v;
    };
    const long long qw = run_sum(has ? vq_quantise(w) : 0ll);
    if (has && last && qw != 0ll) vq_add_to(sum_w + k, qw);
    for (int j = 0; j < F; ++j) {
      const long long qx = run_sum(has ? vq_quantise(w * row[j]) : 0ll);
      if (has && last && qx != 0ll) vq_add_to(sum_wx + (size_t)k * F + j, qx);
    }
  }
}

}  // namespace

thread_local int tl_vq_merge = 0;

// the shipped choice of voxe_vq_debug_merge(0): DESIGN.md 4.25 holds the measurement behind it
constexpr bool kVqMergeShipped = true;

void launch_vq_assign(const float* points, long long N, int F, const float* codebook, int K, float* code_norm, int32_t* index,
                      float* dist, hipStream_t st) {
  vq_norm_kernel<<<(K + 255) / 256, 256, 0, st>>>(codebook, K, F, code_norm);
  const unsigned nb = (unsigned)((N + kVqBlockPts - 1) / kVqBlockPts);
#define VOXE_VQ(KSN) vq_assign_kernel<KSN><<<nb, kVqThreads, 0, st>>>(points, (int)N, F, codebook, K, code_norm, index, dist)
  if (F <= 4) VOXE_VQ(2);
  else if (F <= 12) VOXE_VQ(6);
  else if (F <= 16) VOXE_VQ(8);
  else if (F <= 28) VOXE_VQ(14);
  else if (F <= 48) VOXE_VQ(24);
  else VOXE_VQ(32);
#undef VOXE_VQ
}

void launch_vq_accumulate(const float* points, const float* weights, const int32_t* index, long long N, int F, int K,
                          long long* sum_wx, long long* sum_w, hipStream_t st) {
  const bool merge = tl_vq_merge ? tl_vq_merge == 2 : kVqMergeShipped;
  if (merge) {
    const unsigned nb = (unsigned)((N + kVqMergeThreads - 1) / kVqMergeThreads);
    const size_t lds = sizeof(float) * kVqMergeThreads * (size_t)(F | 1);
    vq_accumulate_kernel<true><<<nb, kVqMergeThreads, lds, st>>>(points, weights, index, N, F, K, sum_wx, sum_w);
  } else {
    const unsigned nb = (unsigned)((N + 255) / 256);
    vq_accumulate_kernel<false><<<nb, 256, 0, st>>>(points, weights, index, N, F, K, sum_wx, sum_w);
  }
}

}  // namespace voxe
