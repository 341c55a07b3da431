// voxe_ssim.hip -- SSIM of two channel-last image batches, value and gradient to x in one call ("SSIM").
//
// Wang et al. 2004 over VALID 11 x 11 Gaussian windows (sigma 1.5): an H x W image gives an (H-10) x (W-10) map.  Per window,
// with the window sums m_x = sum g x, m_y, m_xx = sum g x^2, m_yy, m_xy:
//   vx = m_xx - m_x^2, vy = m_yy - m_y^2, vxy = m_xy - m_x m_y
//   A1 = 2 m_x m_y + C1, A2 = 2 vxy + C2, B1 = m_x^2 + m_y^2 + C1, B2 = vx + vy + C2,  S = A1 A2 / (B1 B2)
//   Q = dS/dm_xx = -S / B2,  R = dS/dm_xy = 2 A1 / (B1 B2),  P = dS/dm_x = 2 m_y (A2 - A1) / (B1 B2) + 2 m_x S (1/B2 - 1/B1)
//   dssim/dx_p = (1/M) sum_{q containing p} g(p - q) [P_q + 2 x_p Q_q + y_p R_q]
//
// Forward : one block = one 16 x 16 tile of windows of one channel of one image.  The 26 x 26 halo of x and y goes to LDS as
//           float, the horizontal pass writes the five row sums of 26 x 16 positions to LDS as double, the vertical pass keeps
//           the five window sums in registers.  S is reduced per block in double into one scratch slot per block.
// Backward: one block = one 16 x 16 tile of pixels of one channel of one image; the 26 x 26 halo of the three maps (zeros
//           outside the map) goes through the same two passes (the Gaussian is symmetric, so the transposed correlation is the
//           same correlation on a halo that starts 10 windows earlier).  No atomics anywhere.
//
// Arithmetic.  On a flat white background (x = y = 1) vx = m_xx - m_x^2 is an exact 0 and Q = -1/C2, R = 2/C2 are about
// -1111 and 2222 while the gradient 2 x Q + y R is an exact 0.  So
//   * every window sum, S, P, Q and R are double (the squares of floats are exact in double, m_xx - m_x^2 keeps ~1e-16);
//   * the maps handed to the backward are P, Q and R2 = R + 2 Q = 2 A1 (B2 - A2) / (B1 B2^2) with B2 - A2 = vx + vy - 2 vxy, so
//         P + 2 x Q + y R = P + 2 (x - y) Q + y R2
//     has no large cancelling pair left: where x = y the middle term is an exact 0 and R2 is as small as the true gradient.
//     That lets the maps be float (12 bytes per window instead of 24) without losing the flat regions;
//   * the backward's two passes accumulate in double and round once, to the float of d_x.
// LDS.  Float halo rows have a pitch of 48 dwords: a 32-lane half of a wave covers two halo rows of 16 outputs in the
// horizontal pass, and ds_read_b32 banks are (dword address) mod 32, so the second row has to start 16 banks after the first
// (pitch = 16 mod 32; 26 columns are needed).  The double row sums have a pitch of 16: the vertical pass reads them with
// ds_read_b64, banks (dword address) mod 64, and a half's two rows of 16 doubles fill the 64 banks exactly.  Both passes are
// free of bank conflicts.
#include <hip/hip_runtime.h>

#include <math.h>

#include "voxe_launch.hpp"

namespace voxe {
namespace {

constexpr int kSsimTile = 16;                        // windows (forward) / pixels (backward) per block side
constexpr int kSsimWin = 11;
constexpr int kSsimHalo = kSsimTile + kSsimWin - 1;  // 26
constexpr int kSsimPitch = 48;                       // dwords per float halo row
constexpr int kSsimThreads = kSsimTile * kSsimTile;  // 256
constexpr int kSsimRows = kSsimHalo * kSsimTile;     // 416 outputs of the horizontal pass

struct SsimWindow {
  float g[kSsimWin];
};

__device__ __forceinline__ double ssim_block_sum(double v) {
  __shared__ double sm[kSsimThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < kSsimThreads / 64; ++i) s += sm[i];
  }
  return s;   // (thread 0 only)
}

// block -> (image n, channel c, tile row ty, tile column tx); the blocks of one image are contiguous
__device__ __forceinline__ void ssim_block(int tiles_x, int tiles_y, int C, long long& n, int& c, int& ty, int& tx) {
  long long b = blockIdx.x;
  tx = (int)(b % tiles_x);
  b /= tiles_x;
  ty = (int)(b % tiles_y);
  b /= tiles_y;
  c = (int)(b % C);
  n = b / C;
}

template <bool GRAD>
__global__ __launch_bounds__(kSsimThreads) void ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                                int W, int C, int tiles_x, int tiles_y, SsimWindow win,
                                                                double C1, double C2, double gscale,
                                                                float* __restrict__ ssim_map, double* __restrict__ partial,
                                                                float* __restrict__ maps, long long map_stride) {
  __shared__ float xs[kSsimHalo * kSsimPitch];
  __shared__ float ys[kSsimHalo * kSsimPitch];
  __shared__ double hs[5][kSsimRows];
  long long n;
  int c, ty, tx;
  ssim_block(tiles_x, tiles_y, C, n, c, ty, tx);
  const int Ho = H - (kSsimWin - 1), Wo = W - (kSsimWin - 1);
  const int i0 = ty * kSsimTile, j0 = tx * kSsimTile;
  const int tid = threadIdx.x;
  for (int e = tid; e < kSsimHalo * kSsimHalo; e += kSsimThreads) {
    const int a = e / kSsimHalo, b = e - a * kSsimHalo;
    const int r = i0 + a, q = j0 + b;
    float xv = 0.0f, yv = 0.0f;
    if (r < H && q < W) {
      const long long at = ((n * H + r) * W + q) * C + c;
      xv = x[at];
      yv = y[at];
    }
    xs[a * kSsimPitch + b] = xv;
    ys[a * kSsimPitch + b] = yv;
  }
  __syncthreads();
  for (int o = tid; o < kSsimRows; o += kSsimThreads) {
    const int a = o >> 4, j = o & 15;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int k = 0; k < kSsimWin; ++k) {
      const double w = (double)win.g[k];
      const double xv = (double)xs[a * kSsimPitch + j + k], yv = (double)ys[a * kSsimPitch + j + k];
      sx = fma(w, xv, sx);
      sy = fma(w, yv, sy);
      sxx = fma(w, xv * xv, sxx);
      syy = fma(w, yv * yv, syy);
      sxy = fma(w, xv * yv, sxy);
    }
    hs[0][o] = sx;
    hs[1][o] = sy;
    hs[2][o] = sxx;
    hs[3][o] = syy;
    hs[4][o] = sxy;
  }
  __syncthreads();
  const int i = tid >> 4, j = tid & 15;
  double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
  for (int k = 0; k < kSsimWin; ++k) {
    const double w = (double)win.g[k];
    const int at = (i + k) * kSsimTile + j;
    mx = fma(w, hs[0][at], mx);
    my = fma(w, hs[1][at], my);
    mxx = fma(w, hs[2][at], mxx);
    myy = fma(w, hs[3][at], myy);
    mxy = fma(w, hs[4][at], mxy);
  }
  const int wi = i0 + i, wj = j0 + j;
  const bool valid = wi < Ho && wj < Wo;
  const double vx = mxx - mx * mx, vy = myy - my * my, vxy = mxy - mx * my;
  const double A1 = 2.0 * mx * my + C1, A2 = 2.0 * vxy + C2;
  const double B1 = mx * mx + my * my + C1, B2 = vx + vy + C2;
  const double inv = 1.0 / (B1 * B2);
  const double S = (A1 * A2) * inv;
  if (valid) {
    if (ssim_map) ssim_map[((n * Ho + wi) * Wo + wj) * C + c] = (float)S;
    if constexpr (GRAD) {
      const double Q = -S / B2;
      const double P = 2.0 * (my * (A2 - A1) + mx * S * (B1 - B2)) * inv;
      const double R2 = 2.0 * A1 * (vx + vy - 2.0 * vxy) * inv / B2;   // R + 2 Q
      const long long at = ((n * C + c) * Ho + wi) * Wo + wj;
      maps[at] = (float)(P * gscale);
      maps[map_stride + at] = (float)(Q * gscale);
      maps[2 * map_stride + at] = (float)(R2 * gscale);
    }
  }
  if (partial) {
    const double s = ssim_block_sum(valid ? S : 0.0);
    if (tid == 0) partial[blockIdx.x] = s;
  }
}

// per_image[n] = (sum of image n's per-block partials, fixed order) / windows of an image; mean = (sum over images) / M
__global__ __launch_bounds__(kSsimThreads) void ssim_finalize_kernel(const double* __restrict__ partial, long long blocks_per_image,
                                                                     int N, double inv_per_image, double inv_M,
                                                                     float* __restrict__ mean_out, float* __restrict__ per_image) {
  double total = 0.0;
  for (int n = 0; n < N; ++n) {
    const double* p = partial + (long long)n * blocks_per_image;
    double s = 0.0;
    for (long long i = threadIdx.x; i < blocks_per_image; i += kSsimThreads) s += p[i];
    const double tot = ssim_block_sum(s);
    if (threadIdx.x == 0) {
      if (per_image) per_image[n] = (float)(tot * inv_per_image);
      total += tot;
    }
    __syncthreads();   // (the next round rewrites the sum's LDS slots)
  }
  if (threadIdx.x == 0 && mean_out) *mean_out = (float)(total * inv_M);
}

template <bool ACCUMULATE>
__global__ __launch_bounds__(kSsimThreads) void ssim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                                int W, int C, int tiles_x, int tiles_y, SsimWindow win,
                                                                const float* __restrict__ maps, long long map_stride,
                                                                float* __restrict__ d_x) {
  __shared__ float ms[3][kSsimHalo * kSsimPitch];
  __shared__ double hs[3][kSsimRows];
  long long n;
  int c, ty, tx;
  ssim_block(tiles_x, tiles_y, C, n, c, ty, tx);
  const int Ho = H - (kSsimWin - 1), Wo = W - (kSsimWin - 1);
  const int i0 = ty * kSsimTile, j0 = tx * kSsimTile;
  const int tid = threadIdx.x;
  const long long plane = (n * C + c) * Ho;
  for (int e = tid; e < kSsimHalo * kSsimHalo; e += kSsimThreads) {
    const int a = e / kSsimHalo, b = e - a * kSsimHalo;
    const int r = i0 - (kSsimWin - 1) + a, q = j0 - (kSsimWin - 1) + b;   // the window whose tap a, b lands on the tile's pixel 0, 0
    float p = 0.0f, qq = 0.0f, r2 = 0.0f;
    if (r >= 0 && r < Ho && q >= 0 && q < Wo) {
      const long long at = (plane + r) * Wo + q;
      p = maps[at];
      qq = maps[map_stride + at];
      r2 = maps[2 * map_stride + at];
    }
    ms[0][a * kSsimPitch + b] = p;
    ms[1][a * kSsimPitch + b] = qq;
    ms[2][a * kSsimPitch + b] = r2;
  }
  __syncthreads();
  for (int o = tid; o < kSsimRows; o += kSsimThreads) {
    const int a = o >> 4, j = o & 15;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < kSsimWin; ++k) {
      const double w = (double)win.g[k];
      s0 = fma(w, (double)ms[0][a * kSsimPitch + j + k], s0);
      s1 = fma(w, (double)ms[1][a * kSsimPitch + j + k], s1);
      s2 = fma(w, (double)ms[2][a * kSsimPitch + j + k], s2);
    }
    hs[0][o] = s0;
    hs[1][o] = s1;
    hs[2][o] = s2;
  }
  __syncthreads();
  const int i = tid >> 4, j = tid & 15;
  double cp = 0.0, cq = 0.0, cr = 0.0;
#pragma unroll
  for (int k = 0; k < kSsimWin; ++k) {
    const double w = (double)win.g[k];
    const int at = (i + k) * kSsimTile + j;
    cp = fma(w, hs[0][at], cp);
    cq = fma(w, hs[1][at], cq);
    cr = fma(w, hs[2][at], cr);
  }
  const int pi = i0 + i, pj = j0 + j;
  if (pi < H && pj < W) {
    const long long at = ((n * H + pi) * W + pj) * C + c;
    const double xv = (double)x[at], yv = (double)y[at];
    const float d = (float)(cp + 2.0 * (xv - yv) * cq + yv * cr);
    if constexpr (ACCUMULATE)
      d_x[at] += d;
    else
      d_x[at] = d;
  }
}

inline long long ssim_tiles(int extent) { return ((long long)extent + kSsimTile - 1) / kSsimTile; }

// blocks of the forward (tiles of windows) and of the backward (tiles of pixels); 0 when either does not fit one launch
inline bool ssim_blocks(int N, int H, int W, int C, long long* fwd, long long* bwd) {
  const long long nc = (long long)N * C;
  *fwd = nc * ssim_tiles(H - (kSsimWin - 1)) * ssim_tiles(W - (kSsimWin - 1));
  *bwd = nc * ssim_tiles(H) * ssim_tiles(W);
  return *bwd <= 0x7fffffffLL;   // (fwd <= bwd)
}

inline size_t ssim_partial_bytes(long long fwd_blocks) { return (sizeof(double) * (size_t)fwd_blocks + 255) / 256 * 256; }

}  // namespace

// [one double per forward block][P, Q, R + 2 Q: three float planes of N C (H-10) (W-10), only with a gradient]
size_t ssim_scratch_bytes(int N, int H, int W, int C, int with_grad) {
  long long fwd, bwd;
  if (!ssim_blocks(N, H, W, C, &fwd, &bwd)) return 0;
  const size_t windows = (size_t)N * C * (size_t)(H - (kSsimWin - 1)) * (size_t)(W - (kSsimWin - 1));
  return ssim_partial_bytes(fwd) + (with_grad ? 3 * sizeof(float) * windows : 0) + 256;
}

void launch_ssim(const float* x, const float* y, int N, int H, int W, int C, float data_range, float grad_scale, float* mean_out,
                 float* per_image, float* ssim_map, float* d_x, int accumulate, void* scratch, hipStream_t st) {
  long long fwd, bwd;
  ssim_blocks(N, H, W, C, &fwd, &bwd);
  const int Ho = H - (kSsimWin - 1), Wo = W - (kSsimWin - 1);
  const long long per_image_windows = (long long)C * Ho * Wo, M = per_image_windows * N;
  SsimWindow win;
  {
    double g[kSsimWin], sum = 0.0;
    for (int i = 0; i < kSsimWin; ++i) sum += g[i] = exp(-(double)((i - 5) * (i - 5)) / 4.5);
    for (int i = 0; i < kSsimWin; ++i) win.g[i] = (float)(g[i] / sum);
  }
  const double L = (double)data_range, C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
  double* partial = (mean_out || per_image) ? (double*)scratch : nullptr;
  float* maps = (float*)((char*)scratch + ssim_partial_bytes(fwd));
  const int ftx = (int)ssim_tiles(Wo), fty = (int)ssim_tiles(Ho);
  if (d_x) {
    ssim_fwd_kernel<true><<<(unsigned)fwd, kSsimThreads, 0, st>>>(x, y, H, W, C, ftx, fty, win, C1, C2,
                                                                  (double)grad_scale / (double)M, ssim_map, partial, maps, M);
  } else if (partial || ssim_map) {
    ssim_fwd_kernel<false><<<(unsigned)fwd, kSsimThreads, 0, st>>>(x, y, H, W, C, ftx, fty, win, C1, C2, 0.0, ssim_map, partial,
                                                                   nullptr, 0);
  }
  if (partial)
    ssim_finalize_kernel<<<1, kSsimThreads, 0, st>>>(partial, fwd / N, N, 1.0 / (double)per_image_windows, 1.0 / (double)M,
                                                     mean_out, per_image);
  if (d_x) {
    const int btx = (int)ssim_tiles(W), bty = (int)ssim_tiles(H);
    if (accumulate)
      ssim_bwd_kernel<true><<<(unsigned)bwd, kSsimThreads, 0, st>>>(x, y, H, W, C, btx, bty, win, maps, M, d_x);
    else
      ssim_bwd_kernel<false><<<(unsigned)bwd, kSsimThreads, 0, st>>>(x, y, H, W, C, btx, bty, win, maps, M, d_x);
  }
}

}  // namespace voxe
