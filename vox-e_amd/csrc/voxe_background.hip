// voxe_background.hip -- learned environment-map background behind the grid ("Background").
//
// Texels E [He, We, 3] are logits.  Per ray, from the direction d = (dx, dy, dz) alone (any length):
//   r = sqrt(dx^2 + dy^2), phi = atan2(dy, dx) (0 where r == 0), theta = atan2(r, dz)
//   u = (phi / 2 pi + 0.5) We - 0.5,  v = (theta / pi) He - 0.5
//   x0 = floor(u), fx = u - x0: columns x0 mod We, (x0 + 1) mod We;  y0 = floor(v), fy = v - y0: rows clamped to [0, He - 1]
//   b_c = sigmoid(bilinear(E[..., c])),  out_c = colour_c + (1 - acc) b_c
// Backward, g = d_out: d_acc = -sum_c g_c b_c, s_c = (1 - acc) g_c b_c (1 - b_c), d_E[tap] += w_tap s_c, and through (u, v)
// into the direction (include/voxe.h spells the chain rule out).  One thread per ray in both kernels.
//
// The angles and (u, v) are double: u multiplies the angle by We / 2 pi, and the cell a ray falls into must not depend on the
// last bits of a float atan2.  Everything behind (fx, fy) is float, as in the renderer.
//
// Texel gradient: in image order consecutive lanes fall into the same cell for long runs, and lanes on the same dword each
// cost an atomic request (profiles/r01_microbench_atomics.md).  Run merge: a lane whose cell (x0, y0) equals its predecessor's
// in the wave joins that lane's run; the 12 values (4 taps x 3 channels) of a run are summed into its first lane by a segmented
// suffix reduction over the wave (6 shuffle steps), and only run heads issue atomics.  A wave without any run skips the
// reduction.  Rays with s == 0 or an unusable direction belong to no run and issue nothing.
#include <hip/hip_runtime.h>

#include "voxe_launch.hpp"

namespace voxe {
namespace {

constexpr int kBgThreads = 256;
constexpr double kPi = 3.14159265358979323846;

// where a direction falls on the map: the four taps (element offsets of channel 0) and the cell's fractions
struct EnvCell {
  long long o00, o01, o10, o11;   // (row y0, column x0), (y0, x1), (y1, x0), (y1, x1)
  int x0, y0;                     // the cell before wrapping / clamping (the run key)
  float fx, fy;
  double dx, dy, dz, r2;          // the direction, dx^2 + dy^2
};

// false: the direction has a non-finite component or zero length (b = 0, no gradient)
__device__ __forceinline__ bool env_cell(int He, int We, const float* __restrict__ rays_d, long long r, EnvCell& c) {
  const float fx = rays_d[3 * r], fy = rays_d[3 * r + 1], fz = rays_d[3 * r + 2];
  if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) return false;
  c.dx = (double)fx;
  c.dy = (double)fy;
  c.dz = (double)fz;
  c.r2 = c.dx * c.dx + c.dy * c.dy;   // (exact zero only for dx == dy == 0: the squares of floats do not underflow in double)
  if (!(c.r2 + c.dz * c.dz > 0.0)) return false;
  const double phi = c.r2 > 0.0 ? atan2(c.dy, c.dx) : 0.0;
  const double theta = atan2(sqrt(c.r2), c.dz);
  const double u = (phi / (2.0 * kPi) + 0.5) * (double)We - 0.5;   // in [-0.5, We - 0.5]
  const double v = (theta / kPi) * (double)He - 0.5;               // in [-0.5, He - 0.5]
  const double uf = floor(u), vf = floor(v);
  c.fx = (float)(u - uf);
  c.fy = (float)(v - vf);
  c.x0 = (int)uf;
  c.y0 = (int)vf;
  // (any int lands inside the map: the modulo is taken twice, the rows are clamped)
  const int xa = ((c.x0 % We) + We) % We, xb = (xa + 1) % We;
  const int ya = min(max(c.y0, 0), He - 1), yb = min(max(c.y0 + 1, 0), He - 1);
  c.o00 = ((long long)ya * We + xa) * 3;
  c.o01 = ((long long)ya * We + xb) * 3;
  c.o10 = ((long long)yb * We + xa) * 3;
  c.o11 = ((long long)yb * We + xb) * 3;
  return true;
}

__device__ __forceinline__ float sigmoidf(float t) { return 1.0f / (1.0f + expf(-t)); }

// (colour_out may be colour_in: a thread reads its ray's three values before it writes them)
__global__ __launch_bounds__(kBgThreads) void background_fwd_kernel(const float* __restrict__ E, int He, int We,
                                                                    const float* __restrict__ rays_d, long long R,
                                                                    const float* colour_in, const float* __restrict__ acc,
                                                                    float* colour_out) {
  const long long r = (long long)blockIdx.x * kBgThreads + threadIdx.x;
  if (r >= R) return;
  float out[3] = {colour_in[3 * r], colour_in[3 * r + 1], colour_in[3 * r + 2]};
  EnvCell c;
  if (env_cell(He, We, rays_d, r, c)) {
    const float left = 1.0f - acc[r];
    const float w00 = (1.0f - c.fx) * (1.0f - c.fy), w01 = c.fx * (1.0f - c.fy), w10 = (1.0f - c.fx) * c.fy, w11 = c.fx * c.fy;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float t = ((w00 * E[c.o00 + ch] + w01 * E[c.o01 + ch]) + w10 * E[c.o10 + ch]) + w11 * E[c.o11 + ch];
      out[ch] = out[ch] + left * sigmoidf(t);
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) colour_out[3 * r + ch] = out[ch];
}

template <bool ACC>
__device__ __forceinline__ void put(float* p, float v) {
  if constexpr (ACC) *p += v; else *p = v;
}

template <bool MERGE, bool ACC>
__global__ __launch_bounds__(kBgThreads) void background_bwd_kernel(const float* __restrict__ E, int He, int We,
                                                                    const float* __restrict__ rays_d, long long R,
                                                                    const float* __restrict__ acc, const float* __restrict__ g,
                                                                    float* __restrict__ d_acc, float* d_texels,
                                                                    float* __restrict__ d_rays_d) {
  const long long r = (long long)blockIdx.x * kBgThreads + threadIdx.x;
  const bool in_range = r < R;   // (every lane of a wave stays for the shuffles below)
  EnvCell c;
  c.x0 = c.y0 = 0;
  c.o00 = c.o01 = c.o10 = c.o11 = 0;
  float val[12];                 // tap-major: (00, 01, 10, 11) x 3 channels
#pragma unroll
  for (int i = 0; i < 12; ++i) val[i] = 0.0f;
  bool live = false;             // this ray deposits into the texels
  if (in_range) {
    float dacc = 0.0f, dd[3] = {0.0f, 0.0f, 0.0f};
    if (env_cell(He, We, rays_d, r, c)) {
      const float left = 1.0f - acc[r];
      const float w[4] = {(1.0f - c.fx) * (1.0f - c.fy), c.fx * (1.0f - c.fy), (1.0f - c.fx) * c.fy, c.fx * c.fy};
      float du = 0.0f, dv = 0.0f;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float e00 = E[c.o00 + ch], e01 = E[c.o01 + ch], e10 = E[c.o10 + ch], e11 = E[c.o11 + ch];
        const float t = ((w[0] * e00 + w[1] * e01) + w[2] * e10) + w[3] * e11;
        const float b = sigmoidf(t), gc = g[3 * r + ch];
        dacc = dacc - gc * b;
        const float s = (left * gc) * (b * (1.0f - b));
        if (s != 0.0f) live = true;
#pragma unroll
        for (int q = 0; q < 4; ++q) val[q * 3 + ch] = w[q] * s;
        du = du + s * ((1.0f - c.fy) * (e01 - e00) + c.fy * (e11 - e10));
        dv = dv + s * ((1.0f - c.fx) * (e10 - e00) + c.fx * (e11 - e01));
      }
      if (d_rays_d && c.r2 > 0.0) {
        const double dphi = (double)du * ((double)We / (2.0 * kPi)), dtheta = (double)dv * ((double)He / kPi);
        const double rr = sqrt(c.r2), n2 = c.r2 + c.dz * c.dz;
        const double a = dtheta * c.dz / (rr * n2);
        dd[0] = (float)(-dphi * c.dy / c.r2 + a * c.dx);
        dd[1] = (float)(dphi * c.dx / c.r2 + a * c.dy);
        dd[2] = (float)(-dtheta * rr / n2);
      }
    }
    if (d_acc) put<ACC>(d_acc + r, dacc);
    if (d_rays_d) {
#pragma unroll
      for (int a = 0; a < 3; ++a) put<ACC>(d_rays_d + 3 * r + a, dd[a]);
    }
  }
  if (!d_texels) return;         // (uniform over the launch)
  bool head = true;
  if constexpr (MERGE) {
    const int lane = threadIdx.x & 63;
    const int px = __shfl_up(c.x0, 1, 64), py = __shfl_up(c.y0, 1, 64);
    const int plive = __shfl_up((int)live, 1, 64);
    const bool joins = live && lane > 0 && plive != 0 && px == c.x0 && py == c.y0;
    head = !joins;
    if (__ballot(joins) != 0ull) {     // (uniform over the wave)
      // the last lane of this lane's run: in front of the next head above it
      const unsigned long long heads = __ballot(head);      // (every lane votes: lane 63's bit ends the run of lane 62)
      const unsigned long long above = (heads >> lane) >> 1;
      const int last = above ? lane + (__ffsll((long long)above) - 1) : 63;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const bool take = lane + off <= last;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          const float t = __shfl_down(val[i], off, 64);
          if (take) val[i] += t;
        }
      }
    }
  }
  if (live && head) {
    const long long o[4] = {c.o00, c.o01, c.o10, c.o11};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float v = val[q * 3 + ch];
        if (v != 0.0f) atomicAdd(d_texels + o[q] + ch, v);   // adding exact zeros is skipped
      }
    }
  }
}

}  // namespace

thread_local int tl_background_merge = 0;

// the shipped choice of voxe_background_debug_merge(0): DESIGN.md 4.15 holds the measurement behind it
constexpr bool kBackgroundMergeShipped = true;

void launch_background_fwd(const float* texels, int He, int We, const float* rays_d, long long R, const float* colour_in,
                           const float* acc, float* colour_out, hipStream_t st) {
  const unsigned nb = (unsigned)((R + kBgThreads - 1) / kBgThreads);
  background_fwd_kernel<<<nb, kBgThreads, 0, st>>>(texels, He, We, rays_d, R, colour_in, acc, colour_out);
}

void launch_background_bwd(const float* texels, int He, int We, const float* rays_d, long long R, const float* acc,
                           const float* d_colour_out, float* d_acc, float* d_texels, float* d_rays_d, bool accumulate,
                           hipStream_t st) {
  const unsigned nb = (unsigned)((R + kBgThreads - 1) / kBgThreads);
  const bool merge = tl_background_merge ? tl_background_merge == 1 : kBackgroundMergeShipped;
#define VOXE_BG_BWD(M, A) \
  background_bwd_kernel<M, A><<<nb, kBgThreads, 0, st>>>(texels, He, We, rays_d, R, acc, d_colour_out, d_acc, d_texels, d_rays_d)
  if (merge) {
    if (accumulate) VOXE_BG_BWD(true, true); else VOXE_BG_BWD(true, false);
  } else {
    if (accumulate) VOXE_BG_BWD(false, true); else VOXE_BG_BWD(false, false);
  }
#undef VOXE_BG_BWD
}

}  // namespace voxe
