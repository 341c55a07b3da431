// voxe_camera.hip -- ray casting through a real-capture camera: fx, fy, cx, cy and the OpenCV radial / tangential lens model
// (DESIGN.md 4.14), forward and the chain rule into the poses, the intrinsics and the distortion coefficients.
//
// Per ray, float32 without FMA (-ffp-contract=off):
//   x = px + 0.5, y = py + 0.5, xd = (x - cx) / fx, yd = (y - cy) / fy        (yd: image-down)
//   (xu, yu) solves D(xu, yu) = (xd, yd):  r2 = xu^2 + yu^2,  rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),
//     D_x = xu rad + 2 p1 xu yu + p2 (r2 + 2 xu^2),   D_y = yu rad + p1 (r2 + 2 yu^2) + 2 p2 xu yu
//   by kNewtonSteps Newton steps from (xd, yd) with the analytic Jacobian, on every lane, no early exit: a ray's bits depend on
//   that ray only.  All five coefficients exactly 0: (xu, yu) = (xd, yd), no iteration (a launch-uniform branch).
//   dir_cam = (xu, -yu, -1), rays_d = R dir_cam, rays_o = t.
// With fx == fy == focal, cx == W/2, cy == H/2 and no distortion the expressions are those of cast_indexed_ray
// (voxe_grid_ops.hip) operation for operation (the negation of yd is exact), so the rays are equal bit for bit.
#include "voxe_device.hpp"
#include "voxe_launch.hpp"

namespace voxe {

constexpr int kNewtonSteps = 6;

struct LensPoint {
  float xd, yd;   // distorted normalised coordinates (what the pixel says)
  float xu, yu;   // undistorted normalised coordinates (where the ray goes)
};

// D and its Jacobian J = dD / d(xu, yu) at (xu, yu); J is symmetric (j01 == j10)
struct LensJac {
  float dx, dy, j00, j01, j11, r2;
};

__device__ __forceinline__ LensJac lens_eval(const VoxeCamera& c, float xu, float yu) {
  LensJac o;
  const float xx = xu * xu, yy = yu * yu, xy = xu * yu;
  const float r2 = xx + yy;
  const float rad = 1.0f + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
  const float drad = c.k1 + r2 * (2.0f * c.k2 + 3.0f * r2 * c.k3);   // d rad / d r2
  o.r2 = r2;
  o.dx = xu * rad + 2.0f * c.p1 * xy + c.p2 * (r2 + 2.0f * xx);
  o.dy = yu * rad + c.p1 * (r2 + 2.0f * yy) + 2.0f * c.p2 * xy;
  o.j00 = rad + 2.0f * xx * drad + 2.0f * c.p1 * yu + 6.0f * c.p2 * xu;
  o.j01 = 2.0f * xy * drad + 2.0f * c.p1 * xu + 2.0f * c.p2 * yu;
  o.j11 = rad + 2.0f * yy * drad + 6.0f * c.p1 * yu + 2.0f * c.p2 * xu;
  return o;
}

__device__ __forceinline__ LensPoint lens_point(const VoxeCamera& c, int distorted, int px, int py) {
  LensPoint p;
  const float x = (float)px + 0.5f, y = (float)py + 0.5f;
  p.xd = (x - c.cx) / c.fx;
  p.yd = (y - c.cy) / c.fy;
  p.xu = p.xd;
  p.yu = p.yd;
  if (distorted) {
#pragma unroll
    for (int it = 0; it < kNewtonSteps; ++it) {
      const LensJac e = lens_eval(c, p.xu, p.yu);
      const float ex = e.dx - p.xd, ey = e.dy - p.yd;
      const float det = e.j00 * e.j11 - e.j01 * e.j01;
      p.xu = p.xu - (e.j11 * ex - e.j01 * ey) / det;
      p.yu = p.yu - (e.j00 * ey - e.j01 * ex) / det;
    }
  }
  return p;
}

// camera and pixel of flat index f, clamped as cast_indexed_ray does (the API validates the range; never read out of bounds)
__device__ __forceinline__ void decode_pixel(int H, int W, int K, long long f, int& cam, int& px, int& py) {
  const long long per = (long long)H * W;
  long long cm = f / per;
  const long long rem = f - cm * per;
  cm = cm < 0 ? 0 : (cm >= K ? K - 1 : cm);
  cam = (int)cm;
  py = (int)(rem / W);
  px = (int)(rem - (long long)py * W);
}

__global__ __launch_bounds__(256) void cast_rays_camera_kernel(VoxeCamera c, int distorted, int K, const float* __restrict__ poses,
                                                               const long long* __restrict__ flat_index, long long B,
                                                               float* __restrict__ rays_o, float* __restrict__ rays_d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int cam, px, py;
  decode_pixel(c.H, c.W, K, flat_index ? flat_index[i] : i, cam, px, py);
  const LensPoint p = lens_point(c, distorted, px, py);
  const float* pose = poses + (long long)cam * 12;   // [3,4] = rotation | translation
  const float dx = p.xu, dy = -p.yu, dz = -1.0f;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    rays_d[3 * i + r] = pose[4 * r + 0] * dx + pose[4 * r + 1] * dy + pose[4 * r + 2] * dz;
    rays_o[3 * i + r] = pose[4 * r + 3];
  }
}

static int is_distorted(const VoxeCamera& c) {
  return !(c.k1 == 0.0f && c.k2 == 0.0f && c.p1 == 0.0f && c.p2 == 0.0f && c.k3 == 0.0f);
}

void launch_cast_rays_camera(const VoxeCamera& cam, const float* poses, int K, const long long* flat_index, long long B,
                             float* rays_o, float* rays_d, hipStream_t st) {
  cast_rays_camera_kernel<<<(unsigned)((B + 255) / 256), 256, 0, st>>>(cam, is_distorted(cam), K, poses, flat_index, B, rays_o,
                                                                       rays_d);
}

// ------------------------------------------------------------------------------------------------
// backward: implicit-function theorem at the forward's solution (the iterations are not differentiated)
//   g = R^T d_d,  (g_xu, g_yu) = (g_0, -g_1),  (g_xd, g_yd) = J^-T (g_xu, g_yu)
//   d_fx = -g_xd xd / fx,  d_cx = -g_xd / fx,  d_fy = -g_yd yd / fy,  d_cy = -g_yd / fy,  d_kj = -(g_xd, g_yd) . dD/dkj
// The per-ray terms of the intrinsics and the coefficients are float32; every sum is double.  `sums`: kCamPoseSums doubles per
// camera (rot 9 | trans 3), then kCamGlobalSums (fx fy cx cy k1 k2 p1 p2 k3), zeroed by the launcher.  The 9 global sums are
// always reduced in the wave before one lane adds; the per-camera sums as cast_rays_bwd_kernel does.
// ------------------------------------------------------------------------------------------------
constexpr int kCamPoseSums = 12;
constexpr int kCamGlobalSums = 9;

__device__ __forceinline__ double wave_sum(double t) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  return t;
}

__global__ __launch_bounds__(256) void cast_rays_camera_bwd_kernel(VoxeCamera c, int distorted, int K,
                                                                   const float* __restrict__ poses,
                                                                   const long long* __restrict__ flat_index, long long B,
                                                                   const float* __restrict__ d_o, const float* __restrict__ d_d,
                                                                   int want_pose, int want_lens, double* __restrict__ sums) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool on = i < B;   // (no early return: every lane joins the ballots and the shuffles)
  double v[kCamPoseSums];
  float w[kCamGlobalSums];
#pragma unroll
  for (int k = 0; k < kCamPoseSums; ++k) v[k] = 0.0;
#pragma unroll
  for (int k = 0; k < kCamGlobalSums; ++k) w[k] = 0.0f;
  int cam = 0;
  if (on) {
    int px, py;
    decode_pixel(c.H, c.W, K, flat_index ? flat_index[i] : i, cam, px, py);
    const LensPoint p = lens_point(c, distorted, px, py);
    const float* pose = poses + (long long)cam * 12;
    const float dc[3] = {p.xu, -p.yu, -1.0f};
    float gd[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      gd[a] = d_d ? d_d[3 * i + a] : 0.0f;
#pragma unroll
      for (int b = 0; b < 3; ++b) v[3 * a + b] = (double)gd[a] * (double)dc[b];
      v[9 + a] = d_o ? (double)d_o[3 * i + a] : 0.0;
    }
    if (want_lens) {
      const float g_xu = (pose[0] * gd[0] + pose[4] * gd[1]) + pose[8] * gd[2];
      const float g_yu = -((pose[1] * gd[0] + pose[5] * gd[1]) + pose[9] * gd[2]);
      float g_xd = g_xu, g_yd = g_yu;
      if (distorted) {
        const LensJac e = lens_eval(c, p.xu, p.yu);
        const float det = e.j00 * e.j11 - e.j01 * e.j01;
        g_xd = (e.j11 * g_xu - e.j01 * g_yu) / det;   // J^T (g_xd, g_yd) = (g_xu, g_yu), J symmetric
        g_yd = (e.j00 * g_yu - e.j01 * g_xu) / det;
        const float xx = p.xu * p.xu, yy = p.yu * p.yu, xy = p.xu * p.yu, r2 = e.r2;
        const float radial = g_xd * p.xu + g_yd * p.yu;
        w[4] = -(radial * r2);
        w[5] = -(radial * (r2 * r2));
        w[8] = -(radial * ((r2 * r2) * r2));
        w[6] = -(g_xd * (2.0f * xy) + g_yd * (r2 + 2.0f * yy));
        w[7] = -(g_xd * (r2 + 2.0f * xx) + g_yd * (2.0f * xy));
      }
      w[0] = -(g_xd * p.xd) / c.fx;
      w[1] = -(g_yd * p.yd) / c.fy;
      w[2] = -g_xd / c.fx;
      w[3] = -g_yd / c.fy;
    }
  }
  if (__builtin_amdgcn_ballot_w64(on) == 0ull) return;   // (lane 0 of every remaining wave is on: i grows with the lane)
  const bool lead = (threadIdx.x & 63) == 0;
  if (want_lens) {
    double* glob = sums + (long long)K * kCamPoseSums;
#pragma unroll
    for (int k = 0; k < kCamGlobalSums; ++k) {
      if (!distorted && k >= 4) break;
      const double t = wave_sum((double)w[k]);   // (lanes that are off carry 0)
      if (lead) atomicAdd(glob + k, t);
    }
  }
  if (!want_pose) return;
  const int cam0 = __builtin_amdgcn_readfirstlane(cam);
  if (__builtin_amdgcn_ballot_w64(on && cam != cam0) == 0ull) {
#pragma unroll
    for (int k = 0; k < kCamPoseSums; ++k) {
      const double t = wave_sum(v[k]);
      if (lead) atomicAdd(sums + (long long)cam0 * kCamPoseSums + k, t);
    }
  } else if (on) {
#pragma unroll
    for (int k = 0; k < kCamPoseSums; ++k)
      if (v[k] != 0.0) atomicAdd(sums + (long long)cam * kCamPoseSums + k, v[k]);
  }
}

__global__ __launch_bounds__(256) void cast_rays_camera_bwd_finalize_kernel(int K, const double* __restrict__ sums,
                                                                            float* __restrict__ d_poses,
                                                                            float* __restrict__ d_intrinsics,
                                                                            float* __restrict__ d_distortion, int accumulate) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (d_poses && t < K * 12) {
    const int k = t / 12, e = t - k * 12, a = e >> 2, b = e & 3;
    const float val = (float)(b < 3 ? sums[k * kCamPoseSums + 3 * a + b] : sums[k * kCamPoseSums + 9 + a]);
    d_poses[t] = accumulate ? d_poses[t] + val : val;
  }
  if (t < kCamGlobalSums) {
    const float val = (float)sums[(long long)K * kCamPoseSums + t];
    float* out = t < 4 ? (d_intrinsics ? d_intrinsics + t : nullptr) : (d_distortion ? d_distortion + (t - 4) : nullptr);
    if (out) *out = accumulate ? *out + val : val;
  }
}

static size_t camera_sum_count(int K) { return (size_t)kCamPoseSums * (size_t)(K > 0 ? K : 0) + kCamGlobalSums; }

size_t cast_rays_camera_bwd_scratch_bytes(int K) { return sizeof(double) * camera_sum_count(K) + 256; }

hipError_t launch_cast_rays_camera_bwd(const VoxeCamera& cam, const float* poses, int K, const long long* flat_index, long long B,
                                       const float* d_o, const float* d_d, float* d_poses, float* d_intrinsics,
                                       float* d_distortion, int accumulate, void* scratch, hipStream_t st) {
  double* sums = (double*)scratch;
  const hipError_t e = hipMemsetAsync(sums, 0, sizeof(double) * camera_sum_count(K), st);
  if (e != hipSuccess) return e;
  const int want_pose = d_poses != nullptr, want_lens = (d_intrinsics || d_distortion) && d_d;
  if (B > 0 && (d_o || d_d) && (want_pose || want_lens))
    cast_rays_camera_bwd_kernel<<<(unsigned)((B + 255) / 256), 256, 0, st>>>(cam, is_distorted(cam), K, poses, flat_index, B, d_o,
                                                                             d_d, want_pose, want_lens, sums);
  const int n = K * 12 > kCamGlobalSums ? K * 12 : kCamGlobalSums;
  cast_rays_camera_bwd_finalize_kernel<<<(n + 255) / 256, 256, 0, st>>>(K, sums, d_poses, d_intrinsics, d_distortion, accumulate);
  return hipSuccess;
}

}  // namespace voxe
