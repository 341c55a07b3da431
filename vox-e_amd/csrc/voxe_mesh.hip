// voxe_mesh.hip -- marching-cubes export of a voxel grid's density iso-surface ("Mesh export").
//
// The padded lattice has nodes at voxel indices -1..N per axis (value 0 outside the grid and outside the mask), node
// n = ((i + 1) * (Y + 2) + (j + 1)) * (Z + 2) + (k + 1).  Node n is the min corner of one cell and the base of its three
// +x/+y/+z lattice edges, so one byte per node -- the case (inside bits of the 8 corners) of its cell -- also gives the
// node's crossing edges (corner 0 vs corners 1, 2, 4).  Three passes, no atomics, so the output is the same bit for bit
// from run to run:
//   count : case per node -> scratch; per tile of 256 nodes the sums of (vertices, triangles)
//   scan  : one block: exclusive scan of the tile sums -> tile offsets, totals (V, T)
//   emit  : vertices: block scan inside each tile + its offset -> per-node vertex / triangle bases, vertex positions;
//           faces: per cell the table's triangles, vertex id of cube edge e = base[owner] + popcount(mask[owner] & lower axes)
// Every store of the emit passes is bounded by the caller's capacities and every scratch read by the lattice size, so a
// grid that changed between count and emit yields a wrong mesh, never an out-of-bounds access.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "voxe.h"
#include "voxe_launch.hpp"
#include "voxe_mc_table.hpp"

namespace voxe {
namespace {

constexpr int kThreads = 256;       // nodes per tile (one per thread)
constexpr int kScanThreads = 1024;
constexpr int kMaxBlocks = 2048;    // grid-stride beyond this (cdna_hip_programming.md Guideline 11)

struct MeshArgs {
  const float* dens;
  const uint8_t* mask;   // nullable
  int X, Y, Z;
  float scale, L;
  int pre;
  float lo[3], step[3];
};

struct Lattice {
  int SY, SZ;           // Y + 2, Z + 2
  long long M;          // nodes
  long long ntiles;
};

__device__ __forceinline__ float node_value(const MeshArgs& a, int i, int j, int k) {
  if (i < 0 || j < 0 || k < 0 || i >= a.X || j >= a.Y || k >= a.Z) return 0.0f;
  const long long vox = ((long long)i * a.Y + j) * a.Z + k;
  if (a.mask && !a.mask[vox]) return 0.0f;
  const float v = a.dens[vox] * a.scale;
  return a.pre == VOXE_ACT_ABS ? fabsf(v) : v;
}

// crossing +x/+y/+z lattice edges of the cell's min node: corner 0 against corners 1, 2, 4
__device__ __forceinline__ unsigned edge_mask(unsigned c) {
  return ((c ^ (c >> 1)) & 1u) | (((c ^ (c >> 2)) & 1u) << 1) | (((c ^ (c >> 4)) & 1u) << 2);
}

__device__ __forceinline__ void node_coords(const Lattice& lt, long long n, int& i, int& j, int& k) {
  const long long plane = (long long)lt.SY * lt.SZ;
  i = (int)(n / plane) - 1;
  const long long r = n - (long long)(i + 1) * plane;
  j = (int)(r / lt.SZ) - 1;
  k = (int)(r - (long long)(j + 1) * lt.SZ) - 1;
}

// exclusive scan of two ints over the 256 threads of a block; totals of both to every thread
__device__ __forceinline__ void block_scan2(int& a, int& b, int& tot_a, int& tot_b) {
  __shared__ int wa[kThreads / 64], wb[kThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int ia = a, ib = b;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int ua = __shfl_up(ia, off, 64), ub = __shfl_up(ib, off, 64);
    if (lane >= off) { ia += ua; ib += ub; }
  }
  if (lane == 63) { wa[wave] = ia; wb[wave] = ib; }
  __syncthreads();
  int ba = 0, bb = 0;
  tot_a = 0; tot_b = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    if (w < wave) { ba += wa[w]; bb += wb[w]; }
    tot_a += wa[w]; tot_b += wb[w];
  }
  __syncthreads();   // (wa / wb are reused by the next tile of a grid-stride loop)
  a = ia - a + ba;
  b = ib - b + bb;
}

__global__ __launch_bounds__(kThreads) void mesh_count_kernel(MeshArgs a, Lattice lt, uint8_t* __restrict__ cases,
                                                              int2* __restrict__ tile_sums) {
  for (long long tile = blockIdx.x; tile < lt.ntiles; tile += gridDim.x) {
    const long long n = tile * kThreads + threadIdx.x;
    unsigned c = 0;
    if (n < lt.M) {
      int i, j, k;
      node_coords(lt, n, i, j, k);
#pragma unroll
      for (int q = 0; q < 8; ++q)
        c |= (node_value(a, i + (q & 1), j + ((q >> 1) & 1), k + ((q >> 2) & 1)) > a.L ? 1u : 0u) << q;
      cases[n] = (uint8_t)c;
    }
    int nv = __popc(edge_mask(c)), nt = kMcTriCount[c];
    int tv, tt;
    block_scan2(nv, nt, tv, tt);
    if (threadIdx.x == 0) tile_sums[tile] = make_int2(tv, tt);
  }
}

// one block: tile_offs[t] = exclusive prefix of tile_sums; totals = (V, T)
__global__ __launch_bounds__(kScanThreads) void mesh_scan_kernel(const int2* __restrict__ tile_sums, long long ntiles,
                                                                 int2* __restrict__ tile_offs, int64_t* __restrict__ totals) {
  __shared__ long long wv[kScanThreads / 64], wt[kScanThreads / 64];
  const long long per = (ntiles + kScanThreads - 1) / kScanThreads;
  const long long b = threadIdx.x * per, e = b + per < ntiles ? b + per : ntiles;
  long long sv = 0, st = 0;
  for (long long t = b; t < e; ++t) {
    const int2 s = tile_sums[t];
    sv += s.x; st += s.y;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long iv = sv, it = st;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long uv = __shfl_up(iv, off, 64), ut = __shfl_up(it, off, 64);
    if (lane >= off) { iv += uv; it += ut; }
  }
  if (lane == 63) { wv[wave] = iv; wt[wave] = it; }
  __syncthreads();
  long long ov = iv - sv, ot = it - st, tv = 0, tt = 0;
  for (int w = 0; w < kScanThreads / 64; ++w) {
    if (w < wave) { ov += wv[w]; ot += wt[w]; }
    tv += wv[w]; tt += wt[w];
  }
  for (long long t = b; t < e; ++t) {
    tile_offs[t] = make_int2((int)ov, (int)ot);   // (the API bounds V, T below 2^31)
    const int2 s = tile_sums[t];
    ov += s.x; ot += s.y;
  }
  if (threadIdx.x == 0) {
    totals[0] = tv;
    totals[1] = tt;
  }
}

// vertex of lattice edge (node (i, j, k), axis ax): t = (L - v_a) / (v_b - v_a) along the edge, then per axis
//   world = f32(lo) + (u + 0.5f) * ((f32(hi) - f32(lo)) / N),  u = index-space coordinate (i + t along ax)
// (-ffp-contract=off: every operation rounds on its own, like the numpy restatement tests/mesh_ref.py)
__device__ __forceinline__ void write_vertex(const MeshArgs& a, int i, int j, int k, int ax, float* __restrict__ out) {
  const float va = node_value(a, i, j, k);
  const float vb = node_value(a, i + (ax == 0), j + (ax == 1), k + (ax == 2));
  const float t = (a.L - va) / (vb - va);
  float u[3] = {(float)i, (float)j, (float)k};
  u[ax] = u[ax] + t;
#pragma unroll
  for (int d = 0; d < 3; ++d) out[d] = a.lo[d] + (u[d] + 0.5f) * a.step[d];
}

__global__ __launch_bounds__(kThreads) void mesh_vertices_kernel(MeshArgs a, Lattice lt, const uint8_t* __restrict__ cases,
                                                                 const int2* __restrict__ tile_offs, int* __restrict__ vbase,
                                                                 int* __restrict__ tbase, float* __restrict__ vertices,
                                                                 long long max_vertices) {
  for (long long tile = blockIdx.x; tile < lt.ntiles; tile += gridDim.x) {
    const long long n = tile * kThreads + threadIdx.x;
    const unsigned c = n < lt.M ? cases[n] : 0u;
    const unsigned em = edge_mask(c);
    int ov = __popc(em), ot = kMcTriCount[c];
    int tv, tt;
    block_scan2(ov, ot, tv, tt);
    if (n >= lt.M) continue;   // (after the block scan: every thread takes part in its barriers)
    const int2 off = tile_offs[tile];
    const int vb = off.x + ov;
    vbase[n] = vb;
    tbase[n] = off.y + ot;
    if (!em) continue;
    int i, j, k;
    node_coords(lt, n, i, j, k);
    int id = vb;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      if (!((em >> ax) & 1u)) continue;
      if (id >= 0 && id < max_vertices) write_vertex(a, i, j, k, ax, vertices + 3ll * id);
      ++id;
    }
  }
}

__global__ __launch_bounds__(kThreads) void mesh_faces_kernel(Lattice lt, const uint8_t* __restrict__ cases,
                                                              const int* __restrict__ vbase, const int* __restrict__ tbase,
                                                              int32_t* __restrict__ faces, long long max_faces) {
  const long long plane = (long long)lt.SY * lt.SZ;
  for (long long n = (long long)blockIdx.x * kThreads + threadIdx.x; n < lt.M; n += (long long)gridDim.x * kThreads) {
    const unsigned c = cases[n];
    const int nt = kMcTriCount[c];
    if (!nt) continue;
    const long long tb = tbase[n];
    for (int s = 0; s < nt; ++s) {
      const long long f = tb + s;
      if (f < 0 || f >= max_faces) break;
      int ids[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const unsigned e = kMcTriEdges[c][3 * s + q];
        const unsigned bc = kMcEdgeBase[e];
        const long long owner = n + (bc & 1u) * plane + ((bc >> 1) & 1u) * lt.SZ + ((bc >> 2) & 1u);
        const unsigned ax = e >> 2;
        ids[q] = owner < lt.M ? vbase[owner] + __popc(edge_mask(cases[owner]) & ((1u << ax) - 1u)) : -1;
      }
      faces[3 * f + 0] = ids[0];
      faces[3 * f + 1] = ids[1];
      faces[3 * f + 2] = ids[2];
    }
  }
}

Lattice lattice_of(int X, int Y, int Z) {
  Lattice lt;
  lt.SY = Y + 2;
  lt.SZ = Z + 2;
  lt.M = (long long)(X + 2) * lt.SY * lt.SZ;
  lt.ntiles = (lt.M + kThreads - 1) / kThreads;
  return lt;
}

struct Scratch {
  uint8_t* cases;
  int* vbase;
  int* tbase;
  int2* tile_sums;
  int2* tile_offs;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

Scratch carve(const Lattice& lt, void* base) {
  char* p = (char*)base;
  Scratch s;
  s.cases = (uint8_t*)p;        p += align256((size_t)lt.M);
  s.vbase = (int*)p;            p += align256((size_t)lt.M * 4);
  s.tbase = (int*)p;            p += align256((size_t)lt.M * 4);
  s.tile_sums = (int2*)p;       p += align256((size_t)lt.ntiles * 8);
  s.tile_offs = (int2*)p;
  return s;
}

MeshArgs mesh_args(const VoxeGridDesc* g, float L, const uint8_t* mask) {
  MeshArgs a;
  a.dens = (const float*)g->densities;
  a.mask = mask;
  a.X = g->X; a.Y = g->Y; a.Z = g->Z;
  a.scale = g->density_scale;
  a.L = L;
  a.pre = g->density_pre_act;
  const int N[3] = {g->X, g->Y, g->Z};
  for (int d = 0; d < 3; ++d) {
    a.lo[d] = g->aabb_lo[d];
    a.step[d] = (g->aabb_hi[d] - g->aabb_lo[d]) / (float)N[d];
  }
  return a;
}

int blocks_for(long long n) { return (int)(n < kMaxBlocks ? n : kMaxBlocks); }

}  // namespace

bool mesh_dims_ok(int X, int Y, int Z) {
  if (X <= 0 || Y <= 0 || Z <= 0) return false;
  if ((long long)X * Y * Z >= (1ll << 31)) return false;
  // int32 vertex / triangle ids and offsets: V <= 3 M, T <= VOXE_MC_MAX_TRIS M
  return lattice_of(X, Y, Z).M * (VOXE_MC_MAX_TRIS > 3 ? VOXE_MC_MAX_TRIS : 3) < (1ll << 31);
}

size_t mesh_scratch_bytes(int X, int Y, int Z) {
  const Lattice lt = lattice_of(X, Y, Z);
  return align256((size_t)lt.M) + 2 * align256((size_t)lt.M * 4) + 2 * align256((size_t)lt.ntiles * 8);
}

void launch_mesh_count(const VoxeGridDesc* g, float L, const uint8_t* mask, int64_t* totals, void* scratch, hipStream_t st) {
  const Lattice lt = lattice_of(g->X, g->Y, g->Z);
  const Scratch s = carve(lt, scratch);
  mesh_count_kernel<<<blocks_for(lt.ntiles), kThreads, 0, st>>>(mesh_args(g, L, mask), lt, s.cases, s.tile_sums);
  mesh_scan_kernel<<<1, kScanThreads, 0, st>>>(s.tile_sums, lt.ntiles, s.tile_offs, totals);
}

void launch_mesh_emit(const VoxeGridDesc* g, float L, const uint8_t* mask, float* vertices, long long max_vertices,
                      int32_t* faces, long long max_faces, void* scratch, hipStream_t st) {
  const Lattice lt = lattice_of(g->X, g->Y, g->Z);
  const Scratch s = carve(lt, scratch);
  mesh_vertices_kernel<<<blocks_for(lt.ntiles), kThreads, 0, st>>>(mesh_args(g, L, mask), lt, s.cases, s.tile_offs, s.vbase,
                                                                    s.tbase, vertices, max_vertices);
  if (max_faces > 0)
    mesh_faces_kernel<<<blocks_for(lt.ntiles), kThreads, 0, st>>>(lt, s.cases, s.vbase, s.tbase, faces, max_faces);
}

}  // namespace voxe
