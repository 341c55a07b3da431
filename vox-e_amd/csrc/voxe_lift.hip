// voxe_lift.hip -- weighted back-projection of per-ray values into the voxel grid ("Lifting").
//
//   accumulate : one thread per ray marches the forward's exact samples front to back with the pieces of voxe_ray_march.hpp
//                (depth step, sample cell, the two halves of the density sample; the loop is its own, see "Merge" below), and
//                for every sample inside the box and every corner c of its cell takes  a = w_k * t_c  -- the float
//                voxe_visibility_accumulate raises max_weight with, t_c = (wx * wy) * wz, w_k = T_k alpha_k -- and adds
//                    sum_w[c]      += q(a)
//                    sum_wv[c, ch] += q(a * values[r, ch])         q(x) = (int64) rint(x * 2^32), a * v rounded to float first
//                with 64-bit integer atomics at agent scope.  Integer adds are associative: the sums are the same bit for bit
//                however lanes, waves, launches and cameras meet on a voxel.  A contribution with q == 0 is skipped (an exact
//                no-op; empty space, where w == 0, issues no atomic at all).  The march is sequential per ray: what a ray
//                contributes depends on the ray and cfg only.
//
// Merge inside a wave (MERGE = true).  In image order a wave is an 8 x 8 pixel tile whose lanes step through the same cells at
// the same k.  The wave walks k in lock step (from the smallest k_lo to the largest k_hi of its lanes); at every step the lanes
// that deposit are keyed by their cell (its base voxel: equal cells have equal corners) and merged by a butterfly over the lane
// bits in the order 1, 8, 2, 16, 4, 32 (x and y neighbours of the tile alternately): at each level a live lane whose partner
// lane ^ off is live and holds the same key hands its integers to the lower lane of the pair and dies.  Which lanes pair is
// decided from the keys alone, once per step; the 8 (1 + C) integers then follow that plan, and a level at which no pair of
// the wave matches moves nothing.  Only surviving lanes issue atomics.  The sums are integers, so any pairing gives the bits of
// the per-lane variant.
#include <hip/hip_runtime.h>

#include <climits>

#include "voxe_launch.hpp"
#include "voxe_ray_march.hpp"

namespace voxe {
namespace {

constexpr int kLiftThreads = kMarchThreads;   // map_ray(): a 16x16 pixel tile (8x8 per wave) or 256 consecutive rays
constexpr float kLiftOne = 4294967296.0f;   // 2^32: the scaling is exact in float

__device__ __forceinline__ long long quantise(float x) { return __float2ll_rn(x * kLiftOne); }

__device__ __forceinline__ void add_to(long long* p, long long v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ long long shfl_xor_ll(long long v, int off) {
  const int lo = __shfl_xor((int)(unsigned)(unsigned long long)v, off, 64);
  const int hi = __shfl_xor((int)(unsigned)((unsigned long long)v >> 32), off, 64);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}

constexpr int kLevels = 6;
__device__ constexpr int kLevelOff[kLevels] = {1, 8, 2, 16, 4, 32};

// the pairing of one step: bit l of `take` = this lane adds its partner's integers at level l; `levels` = the levels at which
// some pair of the wave merges (uniform over the wave); returns whether this lane survives
struct MergePlan {
  unsigned take, levels;
};
__device__ __forceinline__ bool plan_merge(bool has, unsigned key, MergePlan& mp) {
  const int lane = threadIdx.x & 63;
  bool live = has;
  mp.take = mp.levels = 0u;
#pragma unroll
  for (int l = 0; l < kLevels; ++l) {
    const int off = kLevelOff[l];
    const unsigned pkey = (unsigned)__shfl_xor((int)key, off, 64);
    const int plive = __shfl_xor((int)live, off, 64);
    const bool same = live && plive != 0 && pkey == key;
    if (__ballot(same) != 0ull) mp.levels |= 1u << l;
    if (same) {
      if ((lane & off) == 0) mp.take |= 1u << l; else live = false;
    }
  }
  return live;
}
__device__ __forceinline__ long long merged(long long v, const MergePlan& mp) {
#pragma unroll
  for (int l = 0; l < kLevels; ++l) {
    if (mp.levels & (1u << l)) {   // (uniform over the wave)
      const long long p = shfl_xor_ll(v, kLevelOff[l]);
      if (mp.take & (1u << l)) v += p;
    }
  }
  return v;
}

template <int C, bool MERGE>
__global__ __launch_bounds__(kLiftThreads) void lift_accumulate_kernel(DevGrid g, DevCfg c, const float* __restrict__ dens,
                                                                       const float* __restrict__ rays_o,
                                                                       const float* __restrict__ rays_d,
                                                                       const float* __restrict__ jitter,
                                                                       const float* __restrict__ values, long long* sum_wv,
                                                                       long long* sum_w) {
  long long r = 0;
  bool alive = map_ray(c, r);
  RayCtx<1, 1, 1> rc;
  float val[C > 0 ? C : 1];
  int k_lo = INT_MAX, k_hi = -1;
  if (alive) {
    rc.init(g, c, r, rays_o, rays_d, jitter);
    alive = rc.k_lo <= rc.k_hi;
    if (alive) {
      k_lo = rc.k_lo;
      k_hi = rc.k_hi;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) val[ch] = values[r * C + ch];
    }
  }
  int k = k_lo;
  if constexpr (MERGE) {   // the wave walks k in lock step: every lane stays for the shuffles
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) k = min(k, __shfl_xor(k, off, 64));
  } else {
    if (!alive) return;
  }
  float T = 1.0f;
  DepthStep st;
  st.z_next = 0.0f;
  for (;; ++k) {
    const bool more = alive && k <= k_hi;
    if constexpr (MERGE) {
      if (__ballot(more) == 0ull) break;
    } else {
      if (!more) break;
    }
    bool has = false;          // this lane deposits at this step
    unsigned idx[8];
    float t[8];
    float w = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) { idx[q] = 0u; t[q] = 0.0f; }
    if (more && k >= k_lo) {
      if (k == k_lo) st.start(rc, k);
      st.advance(rc, c, k);
      SampleCell sc;
      if (sc.locate(g, rc, st.z)) {
        sc.make(g);
        DensityTaps tp;
        load_density(g, dens, sc.cell, tp);
        DensitySample s;
        eval_density<false>(g, sc.cell, tp, st.dl(), rc.dnorm, s);
#pragma unroll
        for (int q = 0; q < 8; ++q) { idx[q] = tp.idx[q]; t[q] = s.t[q]; }
        w = s.alpha * T;
        has = w > 0.0f;     // (false for NaN)
        if (!attenuate(T, s.om)) alive = false;   // every later w is 0 (or NaN): nothing more to add
      }
    }
    MergePlan mp;
    bool emit = has;
    if constexpr (MERGE) {
      if (__ballot(has) == 0ull) continue;
      // (the corner strides of cell_addr() are the same for every cell of a launch: equal base voxels mean equal corners)
      emit = plan_merge(has, idx[0], mp);
    } else {
      if (!has) continue;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float a = w * t[q];                 // the value voxe_visibility_accumulate raises max_weight with
      long long qa = has ? quantise(a) : 0ll;
      if constexpr (MERGE) qa = merged(qa, mp);
      if (sum_w && emit && qa != 0ll) add_to(sum_w + idx[q], qa);
      if constexpr (C > 0) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          long long qv = has ? quantise(a * val[ch]) : 0ll;
          if constexpr (MERGE) qv = merged(qv, mp);
          if (emit && qv != 0ll) add_to(sum_wv + (size_t)idx[q] * C + ch, qv);
        }
      }
    }
  }
}

}  // namespace

thread_local int tl_lift_merge = 0;

// the shipped choice of voxe_lift_debug_merge(0): DESIGN.md 4.16 holds the measurement behind it
constexpr bool kLiftMergeShipped = true;

void launch_lift_accumulate(const DevGrid& g, const DevCfg& c, const float* dens, const float* rays_o, const float* rays_d,
                            const float* jitter, const float* values, int C, long long* sum_wv, long long* sum_w,
                            hipStream_t st) {
  const unsigned nb = map_ray_blocks(c);
  const bool merge = tl_lift_merge ? tl_lift_merge == 2 : kLiftMergeShipped;
#define VOXE_LIFT(CN)                                                                                                          \
  case CN:                                                                                                                     \
    if (merge) lift_accumulate_kernel<CN, true><<<nb, kLiftThreads, 0, st>>>(g, c, dens, rays_o, rays_d, jitter, values, sum_wv, sum_w); \
    else lift_accumulate_kernel<CN, false><<<nb, kLiftThreads, 0, st>>>(g, c, dens, rays_o, rays_d, jitter, values, sum_wv, sum_w);      \
    break
  switch (sum_wv ? C : 0) {
    VOXE_LIFT(0); VOXE_LIFT(1); VOXE_LIFT(2); VOXE_LIFT(3); VOXE_LIFT(4); VOXE_LIFT(5); VOXE_LIFT(6); VOXE_LIFT(7); VOXE_LIFT(8);
    default: break;   // (the API admits C in 1..8 only)
  }
#undef VOXE_LIFT
}

}  // namespace voxe
