// Geometry out of a trained scene: the density field sampled on a grid and its iso-surface as an indexed triangle mesh.
//   upnerf_grid_columns  the rays that make the field kernels evaluate grid points: one ray per (x, y) column, o = (x, y, 0),
//                        d = (0, 0, 1), z = the column's z coordinates (o + d z IS the grid point), padded to the field kernels'
//                        minimum of samples by repeating the last depth.
//   upnerf_mtet_count    marching tetrahedra on the Kuhn split of every cell (six tetrahedra round the main diagonal, the same in
//                        every cell, so neighbouring cells agree on their face diagonals and no case is ambiguous).  Every grid
//                        point owns seven edges (+x, +y, +z, three face diagonals, the body diagonal); a mesh vertex is a crossed
//                        edge, so the mesh is welded by construction.  Per point: the 7-bit mask of its crossed edges and the
//                        number of triangles of the cell it is the origin of; then exclusive scans of both (block scan + block
//                        sums, as many levels as the size needs, no atomics: the same bits every run).
//   upnerf_mtet_emit     vertices (position on the edge, normal = -grad sigma interpolated the same way) in (point, edge slot)
//                        order and triangles in (cell, tetrahedron, triangle) order, indexing the vertices through the scan.
// With UPNERF_MTET_SKIP_NONFINITE (a grid with samples nobody observed: tsdf.hip) an edge is crossed only between two finite
// samples and a tetrahedron is triangulated only if its four corners are finite; without it a non-finite sample is "outside".
// The case tables are not here: the caller hands them over (upnerf_mtet_tables; upnerf_amd/geometry.py defines them once) and the
// host derives from them what the kernels look up.  Everything is streaming and memory-bound: 1 + 7 cached reads per point in the
// counting pass, 10 B of scratch per point, one thread per point in every kernel, no LDS beyond the scan and the tables.
#include "common.cuh"
#include "grid.cuh"
#include "scan.cuh"

#include <limits.h>
#include <math.h>

namespace {

// ---- column rays ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NTHREADS) void grid_columns_kernel(upnerf_grid_columns_args a) {
  const int64_t id = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  const int64_t nz = (int64_t)a.count * a.S;
  if (id < nz) {  // z rows first: the bulk of the bytes, consecutive threads write consecutive floats
    const int s = (int)(id % a.S);
    a.z[id] = (float)grid_coord(a.lo[2], a.hi[2], a.Nz, s < a.Nz ? s : a.Nz - 1);
    return;
  }
  const int64_t r = id - nz;
  if (r >= a.count) return;
  const int64_t c = a.col0 + r;
  const int y = (int)(c / a.Nx), x = (int)(c - (int64_t)y * a.Nx);
  float* o = a.o + r * 3;
  float* d = a.d + r * 3;
  o[0] = (float)grid_coord(a.lo[0], a.hi[0], a.Nx, x);
  o[1] = (float)grid_coord(a.lo[1], a.hi[1], a.Ny, y);
  o[2] = 0.f;
  d[0] = 0.f;
  d[1] = 0.f;
  d[2] = 1.f;
}

// ---- what the kernels look up, derived on the host from the caller's tables --------------------------------------------------

struct MtetLut {
  int8_t corner[6][4];  // tetrahedron t, vertex i: corner mask of the cell (bit 0 = +x, bit 1 = +y, bit 2 = +z)
  int8_t owner[6][6];   // tetrahedron t, tet edge e: corner whose grid point owns the edge
  int8_t slot[6][6];    //                            and the edge's slot there
  int8_t off[7][3];     // edge slot s: offset of its far end from the owner
  int8_t tris[16][7];   // case: number of triangles, then three tet edges per triangle
};

bool build_lut(const upnerf_mtet_tables& t, MtetLut* L) {
  for (int s = 0; s < 7; ++s)
    for (int k = 0; k < 3; ++k) {
      if (t.edges[s][k] != 0 && t.edges[s][k] != 1) return false;
      L->off[s][k] = t.edges[s][k];
    }
  for (int i = 0; i < 6; ++i)
    for (int k = 0; k < 4; ++k) {
      if (t.tets[i][k] < 0 || t.tets[i][k] > 7) return false;
      L->corner[i][k] = t.tets[i][k];
    }
  for (int i = 0; i < 6; ++i)
    for (int e = 0; e < 6; ++e) {
      const int va = t.tet_edges[e][0], vb = t.tet_edges[e][1];
      if (va < 0 || va > 3 || vb < 0 || vb > 3 || va == vb) return false;
      const int ca = t.tets[i][va], cb = t.tets[i][vb];
      const int lo = ca & cb, diff = ca ^ cb;
      if ((lo != ca && lo != cb) || diff == 0) return false;  // a Kuhn edge runs from a corner to one that contains it
      int slot = -1;
      for (int s = 0; s < 7; ++s)
        if ((t.edges[s][0] | (t.edges[s][1] << 1) | (t.edges[s][2] << 2)) == diff) slot = s;
      if (slot < 0) return false;
      L->owner[i][e] = (int8_t)lo;
      L->slot[i][e] = (int8_t)slot;
    }
  for (int c = 0; c < 16; ++c) {
    const int n = t.tris[c][0];
    if (n < 0 || n > 2) return false;
    L->tris[c][0] = (int8_t)n;
    for (int k = 1; k < 7; ++k) {
      if (t.tris[c][k] < 0 || t.tris[c][k] > 5) return false;
      L->tris[c][k] = t.tris[c][k];
    }
  }
  return true;
}

__device__ __forceinline__ const MtetLut* stage_lut(const MtetLut& lut, MtetLut* sh) {
  const int8_t* src = (const int8_t*)&lut;
  for (int i = threadIdx.x; i < (int)sizeof(MtetLut); i += NTHREADS) ((int8_t*)sh)[i] = src[i];
  __syncthreads();
  return sh;
}

struct Dims {
  int Nx, Ny, Nz;
  int64_t N;
};

// inside: v >= level; a non-finite sample is outside
__device__ __forceinline__ bool inside(float v, float level) { return isfinite(v) && v >= level; }

// bit c = corner c of the cell at (x, y, z) is inside; corners beyond the grid read as outside (and are never used)
__device__ __forceinline__ int corner_bits(const float* grid, const Dims& d, int x, int y, int z, float level) {
  int bits = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int cx = x + (c & 1), cy = y + ((c >> 1) & 1), cz = z + (c >> 2);
    if (cx < d.Nx && cy < d.Ny && cz < d.Nz && inside(grid[((int64_t)cz * d.Ny + cy) * d.Nx + cx], level)) bits |= 1 << c;
  }
  return bits;
}

// bit c = corner c of the cell at (x, y, z) is a finite sample; corners beyond the grid read as not finite (and are never used)
__device__ __forceinline__ int finite_bits(const float* grid, const Dims& d, int x, int y, int z) {
  int bits = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int cx = x + (c & 1), cy = y + ((c >> 1) & 1), cz = z + (c >> 2);
    if (cx < d.Nx && cy < d.Ny && cz < d.Nz && isfinite(grid[((int64_t)cz * d.Ny + cy) * d.Nx + cx])) bits |= 1 << c;
  }
  return bits;
}

// ---- pass 1: crossed edges per point, triangles per cell -------------------------------------------------------------------

// skip: UPNERF_MTET_SKIP_NONFINITE -- an edge needs both ends finite, a tetrahedron all four corners (fin = every bit set
// otherwise: the conditions below are then the ones without the flag)
__global__ __launch_bounds__(NTHREADS) void mtet_flags_kernel(const float* grid, Dims d, float level, MtetLut lut, uint8_t* emask,
                                                               uint8_t* tcount, int skip) {
  __shared__ MtetLut sh;
  const MtetLut* L = stage_lut(lut, &sh);
  const int64_t g = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (g >= d.N) return;
  const int x = (int)(g % d.Nx), y = (int)((g / d.Nx) % d.Ny), z = (int)(g / ((int64_t)d.Nx * d.Ny));
  const int bits = corner_bits(grid, d, x, y, z, level);
  const int fin = skip ? finite_bits(grid, d, x, y, z) : 0xff;
  const int me = bits & 1;
  int mask = 0;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const int ox = L->off[s][0], oy = L->off[s][1], oz = L->off[s][2];
    const int far = ox | (oy << 1) | (oz << 2);
    if (x + ox < d.Nx && y + oy < d.Ny && z + oz < d.Nz && ((bits >> far) & 1) != me && (fin & 1) && ((fin >> far) & 1)) mask |= 1 << s;
  }
  emask[g] = (uint8_t)mask;
  int nt = 0;
  if (x + 1 < d.Nx && y + 1 < d.Ny && z + 1 < d.Nz) {
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      int cs = 0, ok = 1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cs |= ((bits >> L->corner[t][i]) & 1) << i;
        ok &= fin >> L->corner[t][i];
      }
      nt += ok ? L->tris[cs][0] : 0;
    }
  }
  tcount[g] = (uint8_t)nt;
}

// ---- scratch: [edge masks N B | triangle counts N B | vertex scan N ints | triangle scan N ints | scan levels] ------------

struct Scratch {
  uint8_t* emask;
  uint8_t* tcount;
  int32_t* vscan;
  int32_t* tscan;
  int32_t* levels;
  int64_t bytes;
};

int64_t round16(int64_t x) { return (x + 15) / 16 * 16; }

Scratch carve(void* p, int64_t N) {
  Scratch s;
  uint8_t* b = (uint8_t*)p;
  int64_t o = 0;
  s.emask = b + o, o += round16(N);
  s.tcount = b + o, o += round16(N);
  s.vscan = (int32_t*)(b + o), o += round16(N * 4);
  s.tscan = (int32_t*)(b + o), o += round16(N * 4);
  s.levels = (int32_t*)(b + o), o += round16(scan_level_ints(N) * 4);
  s.bytes = o;
  return s;
}

// sizes a grid must have: two points per axis, and room in int32 for the seven edges of every point and the twelve triangles
// of every cell
bool dims_ok(int Nx, int Ny, int Nz, Dims* d) {
  if (Nx < 2 || Ny < 2 || Nz < 2) return false;
  const int64_t N = (int64_t)Nx * Ny;
  if (N > INT_MAX || N * Nz > INT_MAX / 7) return false;
  const int64_t cells = (int64_t)(Nx - 1) * (Ny - 1) * (Nz - 1);
  if (cells > INT_MAX / 12) return false;
  d->Nx = Nx, d->Ny = Ny, d->Nz = Nz, d->N = N * Nz;
  return true;
}

bool bounds_ok(const upnerf_mtet_args* a) {
  for (int k = 0; k < 3; ++k)
    if (!(a->hi[k] > a->lo[k]) || !isfinite(a->hi[k]) || !isfinite(a->lo[k])) return false;
  return true;
}

// ---- pass 3: vertices ------------------------------------------------------------------------------------------------------

// d sigma / d axis at a grid point: central difference, one-sided at the border (every axis has two points at least)
__device__ __forceinline__ float diff_axis(const float* grid, int64_t g, int i, int n, int64_t stride, float inv_h) {
  if (i == 0) return (grid[g + stride] - grid[g]) * inv_h;
  if (i == n - 1) return (grid[g] - grid[g - stride]) * inv_h;
  return (grid[g + stride] - grid[g - stride]) * (0.5f * inv_h);
}

__global__ __launch_bounds__(NTHREADS) void mtet_vertices_kernel(upnerf_mtet_args a, Dims d, MtetLut lut, const uint8_t* emask,
                                                                  const int32_t* vscan) {
  __shared__ MtetLut sh;
  const MtetLut* L = stage_lut(lut, &sh);
  const int64_t g = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (g >= d.N) return;
  const int mask = emask[g];
  if (!mask) return;
  const int x = (int)(g % d.Nx), y = (int)((g / d.Nx) % d.Ny), z = (int)(g / ((int64_t)d.Nx * d.Ny));
  const int64_t sy = d.Nx, sz = (int64_t)d.Nx * d.Ny;
  const float ih[3] = {(float)((double)(d.Nx - 1) / ((double)a.hi[0] - (double)a.lo[0])),
                       (float)((double)(d.Ny - 1) / ((double)a.hi[1] - (double)a.lo[1])),
                       (float)((double)(d.Nz - 1) / ((double)a.hi[2] - (double)a.lo[2]))};
  const float v0 = a.grid[g];
  const float g0[3] = {diff_axis(a.grid, g, x, d.Nx, 1, ih[0]), diff_axis(a.grid, g, y, d.Ny, sy, ih[1]),
                       diff_axis(a.grid, g, z, d.Nz, sz, ih[2])};
  const double p0[3] = {grid_coord(a.lo[0], a.hi[0], d.Nx, x), grid_coord(a.lo[1], a.hi[1], d.Ny, y),
                        grid_coord(a.lo[2], a.hi[2], d.Nz, z)};
  int64_t idx = vscan[g];
  for (int s = 0; s < 7; ++s) {
    if (!((mask >> s) & 1)) continue;
    const int ox = L->off[s][0], oy = L->off[s][1], oz = L->off[s][2];
    const int64_t g1 = g + ox + oy * sy + oz * sz;
    const float v1 = a.grid[g1];
    // where the level sits on the edge, in fp32; the middle when an end is not a number one can interpolate from
    const float t = (isfinite(v0) && isfinite(v1)) ? (a.level - v0) / (v1 - v0) : 0.5f;
    const double p1[3] = {grid_coord(a.lo[0], a.hi[0], d.Nx, x + ox), grid_coord(a.lo[1], a.hi[1], d.Ny, y + oy),
                          grid_coord(a.lo[2], a.hi[2], d.Nz, z + oz)};
    const float g1v[3] = {diff_axis(a.grid, g1, x + ox, d.Nx, 1, ih[0]), diff_axis(a.grid, g1, y + oy, d.Ny, sy, ih[1]),
                          diff_axis(a.grid, g1, z + oz, d.Nz, sz, ih[2])};
    float n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = -(g0[k] + t * (g1v[k] - g0[k]));
    // scaled by the largest component first: the square of a steep gradient must not overflow
    const float big = fmaxf(fabsf(n[0]), fmaxf(fabsf(n[1]), fabsf(n[2])));
    // (fmaxf drops a NaN operand, so every component is asked on its own)
    if (big > 0.f && isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2])) {
      const float q[3] = {n[0] / big, n[1] / big, n[2] / big};
      const float len = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) n[k] = q[k] / len;
    } else {
      n[0] = n[1] = n[2] = 0.f;  // no gradient, or none that is a number
    }
    if (idx < a.cap_vertices) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a.vertices[idx * 3 + k] = (float)(p0[k] + (double)t * (p1[k] - p0[k]));  // fp64 grid coordinates, rounded once
        a.normals[idx * 3 + k] = n[k];
      }
    }
    ++idx;
  }
}

// ---- pass 4: triangles -----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NTHREADS) void mtet_faces_kernel(upnerf_mtet_args a, Dims d, MtetLut lut, const uint8_t* emask,
                                                               const uint8_t* tcount, const int32_t* vscan, const int32_t* tscan) {
  __shared__ MtetLut sh;
  const MtetLut* L = stage_lut(lut, &sh);
  const int64_t g = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (g >= d.N) return;
  if (!tcount[g]) return;  // (zero as well for a point that is the origin of no cell)
  const int x = (int)(g % d.Nx), y = (int)((g / d.Nx) % d.Ny), z = (int)(g / ((int64_t)d.Nx * d.Ny));
  const int64_t sy = d.Nx, sz = (int64_t)d.Nx * d.Ny;
  const int bits = corner_bits(a.grid, d, x, y, z, a.level);
  const int fin = (a.flags & UPNERF_MTET_SKIP_NONFINITE) ? finite_bits(a.grid, d, x, y, z) : 0xff;
  int64_t f = tscan[g];
  for (int t = 0; t < 6; ++t) {
    int cs = 0, ok = 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      cs |= ((bits >> L->corner[t][i]) & 1) << i;
      ok &= fin >> L->corner[t][i];
    }
    const int nt = ok ? L->tris[cs][0] : 0;  // (the count of pass 1, tetrahedron by tetrahedron)
    for (int k = 0; k < nt; ++k, ++f) {
      if (f >= a.cap_faces) continue;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int e = L->tris[cs][1 + 3 * k + j];
        const int c = L->owner[t][e], s = L->slot[t][e];
        const int64_t p = g + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz;
        a.faces[f * 3 + j] = vscan[p] + __popc((unsigned)emask[p] & ((1u << s) - 1u));
      }
    }
  }
}

}  // namespace

extern "C" int upnerf_grid_columns(const upnerf_grid_columns_args* a, void* stream) {
  if (!a || a->Nx < 1 || a->Ny < 1 || a->Nz < 1 || a->S < a->Nz || a->count < 1 || a->col0 < 0) return UPNERF_EINVAL;
  if (a->col0 + a->count > (int64_t)a->Nx * a->Ny) return UPNERF_EINVAL;
  if (!a->o || !a->d || !a->z) return UPNERF_EINVAL;
  for (int k = 0; k < 3; ++k)
    if (!isfinite(a->lo[k]) || !isfinite(a->hi[k])) return UPNERF_EINVAL;
  const int64_t blocks = ceil_div64((int64_t)a->count * a->S + a->count, NTHREADS);
  if (blocks > INT_MAX) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(grid_columns_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" long long upnerf_mtet_scratch(int Nx, int Ny, int Nz) {
  Dims d;
  if (!dims_ok(Nx, Ny, Nz, &d)) return UPNERF_EINVAL;
  return carve(nullptr, d.N).bytes;
}

extern "C" int upnerf_mtet_count(const upnerf_mtet_args* a, void* scratch, int32_t* totals, void* stream) {
  Dims d;
  MtetLut lut;
  if (!a || !dims_ok(a->Nx, a->Ny, a->Nz, &d) || !a->grid || !scratch || !totals || ((uintptr_t)scratch & 15)) return UPNERF_EINVAL;
  if (a->level != a->level || !build_lut(a->tab, &lut) || (a->flags & ~UPNERF_MTET_SKIP_NONFINITE)) return UPNERF_EINVAL;
  const Scratch s = carve(scratch, d.N);
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)ceil_div64(d.N, NTHREADS);
  hipLaunchKernelGGL(mtet_flags_kernel, dim3(nb), dim3(NTHREADS), 0, st, a->grid, d, a->level, lut, s.emask, s.tcount,
                     a->flags & UPNERF_MTET_SKIP_NONFINITE);
  scan_exclusive<uint8_t, true>(s.emask, d.N, s.vscan, s.levels, totals, st);      // (the levels are free again after each scan:
  scan_exclusive<uint8_t, false>(s.tcount, d.N, s.tscan, s.levels, totals + 1, st);  //  stream order)
  return (int)hipGetLastError();
}

extern "C" int upnerf_mtet_emit(const upnerf_mtet_args* a, const void* scratch, void* stream) {
  Dims d;
  MtetLut lut;
  if (!a || !dims_ok(a->Nx, a->Ny, a->Nz, &d) || !a->grid || !scratch || ((uintptr_t)scratch & 15)) return UPNERF_EINVAL;
  if (a->level != a->level || !build_lut(a->tab, &lut) || !bounds_ok(a) || (a->flags & ~UPNERF_MTET_SKIP_NONFINITE)) return UPNERF_EINVAL;
  if (a->n_vertices < 0 || a->n_faces < 0 || a->n_vertices > 7 * d.N) return UPNERF_EINVAL;
  if (a->cap_vertices < a->n_vertices || a->cap_faces < a->n_faces) return UPNERF_EINVAL;  // nothing is written, not a part
  if (a->n_vertices > 0 && (!a->vertices || !a->normals)) return UPNERF_EINVAL;
  if (a->n_faces > 0 && !a->faces) return UPNERF_EINVAL;
  const Scratch s = carve(const_cast<void*>(scratch), d.N);
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)ceil_div64(d.N, NTHREADS);
  if (a->n_vertices > 0)
    hipLaunchKernelGGL(mtet_vertices_kernel, dim3(nb), dim3(NTHREADS), 0, st, *a, d, lut, (const uint8_t*)s.emask,
                       (const int32_t*)s.vscan);
  if (a->n_faces > 0)
    hipLaunchKernelGGL(mtet_faces_kernel, dim3(nb), dim3(NTHREADS), 0, st, *a, d, lut, (const uint8_t*)s.emask,
                       (const uint8_t*)s.tcount, (const int32_t*)s.vscan, (const int32_t*)s.tscan);
  return (int)hipGetLastError();
}
