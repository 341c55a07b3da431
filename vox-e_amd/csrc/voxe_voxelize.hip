// voxe_voxelize.hip -- mesh import: a triangle mesh into a signed-distance band on a voxel lattice.
//
// Index space: u = (p - lo) / step - 0.5 per axis, so voxel centre i sits at u = i.  Every vertex is snapped once to the
// 2^-8-voxel lattice, q = rint(256 u), and everything that DECIDES something (which cells a triangle is tried on, which
// columns it covers, which voxel a crossing is charged to, whether it is degenerate) is integer arithmetic on q.  The distance
// itself is float32 on the world-space vertices, every operation rounded on its own (-ffp-contract=off), restated operation
// for operation by tests/voxelize_ref.py.
//
// Passes (all inside voxe_voxelize_mesh, caller scratch, caller stream, no read-back):
//   init     : key grid = all ones, counter grid = 0, statistics = 0
//   count    : one thread per triangle: validate, work items of the triangle = sign items + distance items (0 when skipped)
//   scan     : one block: exclusive prefix of the item counts (no atomics in the offsets), total, skipped triangles
//   work     : every wave takes a run of consecutive items; it finds the first one's triangle by bisection of the prefix, walks
//              on from there and rebuilds each triangle's boxes from its vertices (nothing per item is stored, so the scratch
//              is bounded by T, not by the number of items).  Sign item: <= 16 x 64 columns (y, z): exact coverage, crossing
//              charged with one int32 atomic add.  Distance item: <= 8 x 8 x 64 cells: closest point, one 64-bit atomicMin of
//              (bits(d^2) << 32 | triangle).
//   columns  : one thread per column walks x: running parity in place of the counters, columns with an odd total
//   finalise : one thread per voxel: decode the key, one sqrt, sign, nearest, colour
// The atomics are integer min / add: the result is the same bits whatever the order the triangles arrive in.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "voxe.h"
#include "voxe_launch.hpp"

namespace voxe {
namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kMaxBlocks = 2048;     // grid-stride beyond this
constexpr int kWorkBlocks = 1024;    // persistent blocks of the work pass (4 waves each)
constexpr int kFrac = 8;             // fraction bits of the snapped lattice
constexpr int kOne = 1 << kFrac;
constexpr int kDX = 8, kDY = 8, kDZ = 64;   // distance item: cells per axis
constexpr int kSY = 16, kSZ = 64;           // sign item: columns per axis
constexpr unsigned long long kNoKey = ~0ull;

struct VoxArgs {
  const float* verts;
  const int32_t* faces;
  const float* vcol;   // nullable
  long long V, T;
  int X, Y, Z;
  float lo[3], step[3];
  int r[3];            // band half-width in cells per axis, ceil(h / step)
  float h, h2;
};

struct Tri {
  float p[3][3];       // world-space vertices, ascending vertex id
  int id[3];
  int q[3][3];         // snapped index-space coordinates
  int d0[3], d1[3];    // distance box (cells, inclusive, clipped); empty when d1 < d0
  int s0[2], s1[2];    // sign box (columns y, z, inclusive, clipped)
  bool degenerate;     // the snapped triangle has zero area: nothing to do
  bool flat;           // zero projected area on (y, z): no sign items
};

__device__ __forceinline__ int floor_cell(int q) { return q >> kFrac; }
__device__ __forceinline__ int ceil_cell(int q) { return -((-q) >> kFrac); }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// false: the triangle is malformed (an index outside [0, V), a non-finite vertex or one outside |u| < 1024) -- no vertex is
// read through a bad index
__device__ __forceinline__ bool load_tri(const VoxArgs& a, long long t, Tri& tr) {
  int i0 = a.faces[3 * t + 0], i1 = a.faces[3 * t + 1], i2 = a.faces[3 * t + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= a.V || i1 >= a.V || i2 >= a.V) return false;
  // ascending ids: the float distance does not depend on how the face lists its vertices
  int s;
  if (i0 > i1) { s = i0; i0 = i1; i1 = s; }
  if (i1 > i2) { s = i1; i1 = i2; i2 = s; }
  if (i0 > i1) { s = i0; i0 = i1; i1 = s; }
  tr.id[0] = i0; tr.id[1] = i1; tr.id[2] = i2;
  bool ok = true;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float p = a.verts[3ll * tr.id[v] + d];
      const float u = (p - a.lo[d]) / a.step[d] - 0.5f;
      ok = ok && (fabsf(u) < 1024.0f);   // (false for NaN)
      tr.p[v][d] = p;
      tr.q[v][d] = ok ? (int)rintf(u * (float)kOne) : 0;
    }
  }
  if (!ok) return false;
  const int N[3] = {a.X, a.Y, a.Z};
  long long e1[3], e2[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int mn = imin(tr.q[0][d], imin(tr.q[1][d], tr.q[2][d]));
    const int mx = imax(tr.q[0][d], imax(tr.q[1][d], tr.q[2][d]));
    tr.d0[d] = imax(0, floor_cell(mn) - a.r[d]);
    tr.d1[d] = imin(N[d] - 1, ceil_cell(mx) + a.r[d]);
    if (d > 0) {
      tr.s0[d - 1] = imax(0, ceil_cell(mn));
      tr.s1[d - 1] = imin(N[d] - 1, floor_cell(mx));
    }
    e1[d] = (long long)tr.q[1][d] - tr.q[0][d];
    e2[d] = (long long)tr.q[2][d] - tr.q[0][d];
  }
  const long long nx = e1[1] * e2[2] - e1[2] * e2[1];
  const long long ny = e1[2] * e2[0] - e1[0] * e2[2];
  const long long nz = e1[0] * e2[1] - e1[1] * e2[0];
  tr.flat = nx == 0;
  tr.degenerate = nx == 0 && ny == 0 && nz == 0;
  return true;
}

__device__ __forceinline__ int chunks(int lo, int hi, int size) { return hi < lo ? 0 : (hi - lo) / size + 1; }

__device__ __forceinline__ int sign_items(const Tri& tr) {
  if (tr.degenerate || tr.flat) return 0;
  return chunks(tr.s0[0], tr.s1[0], kSY) * chunks(tr.s0[1], tr.s1[1], kSZ);
}

__device__ __forceinline__ int dist_items(const Tri& tr) {
  if (tr.degenerate) return 0;
  return chunks(tr.d0[0], tr.d1[0], kDX) * chunks(tr.d0[1], tr.d1[1], kDY) * chunks(tr.d0[2], tr.d1[2], kDZ);
}

__device__ __forceinline__ float dot3(const float* x, const float* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// closest point of triangle (A, B, C) to P by Voronoi regions: the point is A + v AB + w AC; returns |P - point|^2
__device__ __forceinline__ float closest(const Tri& tr, const float* P, float& v, float& w) {
  float ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    ab[d] = tr.p[1][d] - tr.p[0][d];
    ac[d] = tr.p[2][d] - tr.p[0][d];
    ap[d] = P[d] - tr.p[0][d];
    bp[d] = P[d] - tr.p[1][d];
    cp[d] = P[d] - tr.p[2][d];
  }
  const float d1 = dot3(ab, ap), d2 = dot3(ac, ap);
  const float d3 = dot3(ab, bp), d4 = dot3(ac, bp);
  const float d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  if (d1 <= 0.0f && d2 <= 0.0f) { v = 0.0f; w = 0.0f; }
  else if (d3 >= 0.0f && d4 <= d3) { v = 1.0f; w = 0.0f; }
  else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { v = d1 / (d1 - d3); w = 0.0f; }
  else if (d6 >= 0.0f && d5 <= d6) { v = 0.0f; w = 1.0f; }
  else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { v = 0.0f; w = d2 / (d2 - d6); }
  else if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) { w = e43 / (e43 + e56); v = 1.0f - w; }
  else {
    const float denom = 1.0f / ((va + vb) + vc);
    v = vb * denom;
    w = vc * denom;
  }
  float diff[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) diff[d] = P[d] - ((tr.p[0][d] + ab[d] * v) + ac[d] * w);
  return dot3(diff, diff);
}

__device__ __forceinline__ void cell_centre(const VoxArgs& a, int i, int j, int k, float* P) {
  P[0] = a.lo[0] + ((float)i + 0.5f) * a.step[0];
  P[1] = a.lo[1] + ((float)j + 0.5f) * a.step[1];
  P[2] = a.lo[2] + ((float)k + 0.5f) * a.step[2];
}

__global__ __launch_bounds__(kThreads) void vox_init_kernel(unsigned long long* __restrict__ keys, long long nkeys,
                                                            int* __restrict__ counters, long long ncounters,
                                                            long long* __restrict__ stats) {
  const long long stride = (long long)gridDim.x * kThreads;
  const long long first = (long long)blockIdx.x * kThreads + threadIdx.x;
  for (long long n = first; n < nkeys; n += stride) keys[n] = kNoKey;
  for (long long n = first; n < ncounters; n += stride) counters[n] = 0;
  if (first < 4) stats[first] = 0;
}

// items[t] = work items of triangle t, -1 when it is malformed
__global__ __launch_bounds__(kThreads) void vox_count_kernel(VoxArgs a, int* __restrict__ items) {
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < a.T; t += (long long)gridDim.x * kThreads) {
    Tri tr;
    items[t] = load_tri(a, t, tr) ? sign_items(tr) + dist_items(tr) : -1;
  }
}

// one block: offs[t] = exclusive prefix of max(items, 0), offs[T] = total; stats[1] = malformed, stats[3] = total
__global__ __launch_bounds__(kScanThreads) void vox_scan_kernel(const int* __restrict__ items, long long T,
                                                                long long* __restrict__ offs, long long* __restrict__ stats) {
  __shared__ long long wn[kScanThreads / 64], wm[kScanThreads / 64];
  const long long per = (T + kScanThreads - 1) / kScanThreads;
  const long long b = threadIdx.x * per < T ? threadIdx.x * per : T, e = b + per < T ? b + per : T;
  long long sn = 0, sm = 0;
  for (long long t = b; t < e; ++t) {
    const int c = items[t];
    sn += c > 0 ? c : 0;
    sm += c < 0 ? 1 : 0;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long in = sn, im = sm;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long un = __shfl_up(in, off, 64), um = __shfl_up(im, off, 64);
    if (lane >= off) { in += un; im += um; }
  }
  if (lane == 63) { wn[wave] = in; wm[wave] = im; }
  __syncthreads();
  long long on = in - sn, tn = 0, tm = 0;
  for (int w = 0; w < kScanThreads / 64; ++w) {
    if (w < wave) on += wn[w];
    tn += wn[w]; tm += wm[w];
  }
  for (long long t = b; t < e; ++t) {
    offs[t] = on;
    const int c = items[t];
    on += c > 0 ? c : 0;
  }
  if (threadIdx.x == 0) {
    offs[T] = tn;
    stats[1] = tm;
    stats[3] = tn;
  }
}

// sign item `local` of a triangle: columns of one kSY x kSZ chunk of its (y, z) box
__device__ __forceinline__ void sign_item(const VoxArgs& a, const Tri& tr, int local, int lane, int* __restrict__ counters) {
  const int ncz = chunks(tr.s0[1], tr.s1[1], kSZ);
  const int cy = local / ncz, cz = local - cy * ncz;
  const int j0 = tr.s0[0] + cy * kSY, j1 = imin(tr.s1[0], j0 + kSY - 1);
  const int k0 = tr.s0[1] + cz * kSZ, k1 = imin(tr.s1[1], k0 + kSZ - 1);
  const int ez = k1 - k0 + 1, n = (j1 - j0 + 1) * ez;
  // (y, z, x) of the three vertices, counter-clockwise in the projection
  long long A[3] = {tr.q[0][1], tr.q[0][2], tr.q[0][0]};
  long long B[3] = {tr.q[1][1], tr.q[1][2], tr.q[1][0]};
  long long Cc[3] = {tr.q[2][1], tr.q[2][2], tr.q[2][0]};
  long long area = (B[0] - A[0]) * (Cc[1] - A[1]) - (B[1] - A[1]) * (Cc[0] - A[0]);
  if (area < 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { const long long s = B[d]; B[d] = Cc[d]; Cc[d] = s; }
    area = -area;
  }
  const long long den = area * kOne;
  for (int c = lane; c < n; c += 64) {
    const int jj = c / ez;
    const int j = j0 + jj, k = k0 + (c - jj * ez);
    const long long py = (long long)j * kOne, pz = (long long)k * kOne;
    // edge functions of the edges opposite A, B, C; > 0 inside
    long long E[3];
    bool in = true;
    const long long* S[3] = {B, Cc, A};
    const long long* D[3] = {Cc, A, B};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const long long dy = D[q][0] - S[q][0], dz = D[q][1] - S[q][1];
      E[q] = dy * (pz - S[q][1]) - dz * (py - S[q][0]);
      // top-left rule: a centre on the edge belongs to the side the point (y + eps, z + eps^2) falls on
      in = in && (E[q] > 0 || (E[q] == 0 && (dz < 0 || (dz == 0 && dy > 0))));
    }
    if (!in) continue;
    // x of the plane over the centre is num / area (snapped units); first voxel centre at or behind it
    const long long num = E[0] * A[2] + E[1] * B[2] + E[2] * Cc[2];
    long long i = num / den;
    if (num % den > 0) ++i;
    i = i < 0 ? 0 : (i > a.X ? a.X : i);
    atomicAdd(&counters[(i * a.Y + j) * a.Z + k], 1);
  }
}

// distance item `local` of a triangle: cells of one kDX x kDY x kDZ chunk of its dilated box
__device__ __forceinline__ void dist_item(const VoxArgs& a, const Tri& tr, long long t, int local, int lane,
                                          unsigned long long* __restrict__ keys) {
  const int ncy = chunks(tr.d0[1], tr.d1[1], kDY), ncz = chunks(tr.d0[2], tr.d1[2], kDZ);
  const int cx = local / (ncy * ncz), rem = local - cx * (ncy * ncz);
  const int cy = rem / ncz, cz = rem - cy * ncz;
  const int i0 = tr.d0[0] + cx * kDX, i1 = imin(tr.d1[0], i0 + kDX - 1);
  const int j0 = tr.d0[1] + cy * kDY, j1 = imin(tr.d1[1], j0 + kDY - 1);
  const int k0 = tr.d0[2] + cz * kDZ, k1 = imin(tr.d1[2], k0 + kDZ - 1);
  const int ey = j1 - j0 + 1, ez = k1 - k0 + 1, n = (i1 - i0 + 1) * ey * ez;
  for (int c = lane; c < n; c += 64) {
    const int ii = c / (ey * ez), r2 = c - ii * (ey * ez);
    const int jj = r2 / ez;
    const int i = i0 + ii, j = j0 + jj, k = k0 + (r2 - jj * ez);
    float P[3], v, w;
    cell_centre(a, i, j, k, P);
    const float dd = closest(tr, P, v, w);
    if (dd <= a.h2) {   // (false for NaN)
      const unsigned long long key = ((unsigned long long)__float_as_uint(dd) << 32) | (unsigned long long)(uint32_t)t;
      atomicMin(&keys[((long long)i * a.Y + j) * a.Z + k], key);
    }
  }
}

__global__ __launch_bounds__(kThreads) void vox_work_kernel(VoxArgs a, const long long* __restrict__ offs,
                                                            unsigned long long* __restrict__ keys, int* __restrict__ counters) {
  const int lane = threadIdx.x & 63;
  const long long nwaves = (long long)gridDim.x * (kThreads / 64);
  const long long total = offs[a.T];
  // a wave takes a run of consecutive items -- consecutive triangles, which in a mesh are mostly neighbours in space: one
  // bisection per wave, then a walk along the prefix
  const long long per = (total + nwaves - 1) / nwaves;
  long long item = ((long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * per;
  const long long end = item + per < total ? item + per : total;
  if (item >= end) return;
  // the last t with offs[t] <= item (triangles without items share their successor's offset)
  long long t = 0, hi = a.T;   // offs[t] <= item < offs[hi]
  while (hi - t > 1) {
    const long long mid = (t + hi) >> 1;
    if (offs[mid] <= item) t = mid; else hi = mid;
  }
  long long first = offs[t], next = offs[t + 1];
  Tri tr;
  bool loaded = false, ok = false;
  int ns = 0, nd = 0;
  for (; item < end; ++item) {
    while (item >= next) {   // (item < total = offs[T]: stops at some t < T)
      ++t;
      first = next;
      next = offs[t + 1];
      loaded = false;
    }
    if (!loaded) {
      ok = load_tri(a, t, tr);
      ns = ok ? sign_items(tr) : 0;
      nd = ok ? dist_items(tr) : 0;
      loaded = true;
    }
    if (!ok) continue;
    const long long local = item - first;
    if (local < ns) sign_item(a, tr, (int)local, lane, counters);
    else if (local - ns < nd) dist_item(a, tr, t, (int)(local - ns), lane, keys);
  }
}

// one thread per column (y, z): counters -> running parity along x; plane X holds the crossings behind the grid
__global__ __launch_bounds__(kThreads) void vox_columns_kernel(int X, int Y, int Z, int* __restrict__ counters,
                                                               long long* __restrict__ stats) {
  const long long ncol = (long long)Y * Z;
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < ncol; c += (long long)gridDim.x * kThreads) {
    int run = 0;
    // sixteen planes per round, loads before stores: the walk is a chain of memory latencies, not of additions
    for (int i0 = 0; i0 < X; i0 += 16) {
      int cnt[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) cnt[u] = i0 + u < X ? counters[(i0 + u) * ncol + c] : 0;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        run += cnt[u];
        if (i0 + u < X) counters[(i0 + u) * ncol + c] = run & 1;
      }
    }
    run += counters[X * ncol + c];
    if (run & 1) atomicAdd((unsigned long long*)&stats[0], 1ull);
  }
}

__global__ __launch_bounds__(kThreads) void vox_finalise_kernel(VoxArgs a, const unsigned long long* __restrict__ keys,
                                                                const int* __restrict__ parity, float* __restrict__ sdf,
                                                                int32_t* __restrict__ nearest, float* __restrict__ colours,
                                                                uint8_t* __restrict__ inside, long long* __restrict__ stats) {
  const long long N = (long long)a.X * a.Y * a.Z;
  const long long plane = (long long)a.Y * a.Z;
  for (long long base = (long long)blockIdx.x * kThreads; base < N; base += (long long)gridDim.x * kThreads) {
    const long long n = base + threadIdx.x;
    bool band = false;
    if (n < N) {
      const unsigned long long key = keys[n];
      const bool in = parity[n] & 1;
      band = key != kNoKey;
      float d = a.h, col[3] = {0.0f, 0.0f, 0.0f};
      int near = -1;
      if (band) {
        d = fminf(sqrtf(__uint_as_float((uint32_t)(key >> 32))), a.h);
        near = (int)(uint32_t)key;
        Tri tr;
        if (colours && a.vcol && load_tri(a, near, tr)) {
          const int i = (int)(n / plane), r = (int)(n - i * plane);
          const int j = r / a.Z, k = r - j * a.Z;
          float P[3], v, w;
          cell_centre(a, i, j, k, P);
          closest(tr, P, v, w);
          const float u = (1.0f - v) - w;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch)
            col[ch] = (a.vcol[3ll * tr.id[0] + ch] * u + a.vcol[3ll * tr.id[1] + ch] * v) + a.vcol[3ll * tr.id[2] + ch] * w;
        }
      }
      sdf[n] = in ? -d : d;
      if (nearest) nearest[n] = near;
      if (inside) inside[n] = in ? 1 : 0;
      if (colours) {
        colours[3 * n + 0] = col[0];
        colours[3 * n + 1] = col[1];
        colours[3 * n + 2] = col[2];
      }
    }
    const unsigned long long b = __ballot(band);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)&stats[2], (unsigned long long)__popcll(b));
  }
}

__global__ void vox_fill_kernel(float* __restrict__ sdf, int32_t* __restrict__ nearest, float* __restrict__ colours,
                                uint8_t* __restrict__ inside, long long* __restrict__ stats, long long N, float h) {
  for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
    sdf[n] = h;
    if (nearest) nearest[n] = -1;
    if (inside) inside[n] = 0;
    if (colours) {
      colours[3 * n + 0] = 0.0f;
      colours[3 * n + 1] = 0.0f;
      colours[3 * n + 2] = 0.0f;
    }
  }
  if (stats && blockIdx.x == 0 && threadIdx.x < 4) stats[threadIdx.x] = 0;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Scratch {
  unsigned long long* keys;   // [X,Y,Z]
  int* counters;              // [X+1,Y,Z]
  int* items;                 // [T]
  long long* offs;            // [T+1]
  long long* stats;           // [4]
};

Scratch carve(int X, int Y, int Z, long long T, void* base) {
  const size_t N = (size_t)X * Y * Z, plane = (size_t)Y * Z;
  char* p = (char*)base;
  Scratch s;
  s.keys = (unsigned long long*)p;  p += align256(N * 8);
  s.counters = (int*)p;             p += align256((N + plane) * 4);
  s.items = (int*)p;                p += align256((size_t)T * 4);
  s.offs = (long long*)p;           p += align256((size_t)(T + 1) * 8);
  s.stats = (long long*)p;
  return s;
}

int blocks_for(long long n) {
  const long long b = (n + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b < kMaxBlocks ? b : kMaxBlocks));
}

}  // namespace

bool voxelize_dims_ok(int X, int Y, int Z, long long T) {
  return X > 0 && Y > 0 && Z > 0 && X <= VOXE_VOXELIZE_MAX_DIM && Y <= VOXE_VOXELIZE_MAX_DIM && Z <= VOXE_VOXELIZE_MAX_DIM &&
         T >= 0 && T < (1ll << 31);
}

size_t voxelize_scratch_bytes(int X, int Y, int Z, long long T) {
  const size_t N = (size_t)X * Y * Z, plane = (size_t)Y * Z;
  return align256(N * 8) + align256((N + plane) * 4) + align256((size_t)T * 4) + align256((size_t)(T + 1) * 8) + 256;
}

void launch_voxelize(const float* vertices, long long V, const int32_t* faces, long long T, const float* vertex_colours, int X,
                     int Y, int Z, const float* aabb_lo, const float* aabb_hi, float h, float* sdf, int32_t* nearest,
                     float* colours, uint8_t* inside, int64_t* stats, void* scratch, hipStream_t st) {
  const long long N = (long long)X * Y * Z;
  if (T == 0) {
    vox_fill_kernel<<<blocks_for(N), kThreads, 0, st>>>(sdf, nearest, colours, inside, (long long*)stats, N, h);
    return;
  }
  VoxArgs a;
  a.verts = vertices; a.faces = faces; a.vcol = vertex_colours;
  a.V = V; a.T = T;
  a.X = X; a.Y = Y; a.Z = Z;
  const int dims[3] = {X, Y, Z};
  for (int d = 0; d < 3; ++d) {
    a.lo[d] = aabb_lo[d];
    a.step[d] = (aabb_hi[d] - aabb_lo[d]) / (float)dims[d];
    const float cells = ceilf(h / a.step[d]);
    a.r[d] = cells < 2048.0f ? (int)cells : 2048;   // (2048 cells cover any grid from any admissible vertex)
  }
  a.h = h;
  a.h2 = h * h;
  const Scratch s = carve(X, Y, Z, T, scratch);
  vox_init_kernel<<<blocks_for(N + (long long)Y * Z), kThreads, 0, st>>>(s.keys, N, s.counters, N + (long long)Y * Z, s.stats);
  vox_count_kernel<<<blocks_for(T), kThreads, 0, st>>>(a, s.items);
  vox_scan_kernel<<<1, kScanThreads, 0, st>>>(s.items, T, s.offs, s.stats);
  vox_work_kernel<<<kWorkBlocks, kThreads, 0, st>>>(a, s.offs, s.keys, s.counters);
  vox_columns_kernel<<<blocks_for((long long)Y * Z), kThreads, 0, st>>>(X, Y, Z, s.counters, s.stats);
  vox_finalise_kernel<<<blocks_for(N), kThreads, 0, st>>>(a, s.keys, s.counters, sdf, nearest, colours, inside, s.stats);
  if (stats) (void)hipMemcpyAsync(stats, s.stats, 4 * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
}

}  // namespace voxe
