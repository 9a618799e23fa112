// Empty-space skipping for whole-frame renders: the density grid as a bit-packed occupancy grid, and the rays of a chunk walked
// through it so that only the rays that touch something are rendered, over only the part of the ray that does.
//   upnerf_occ_build    cells of the density grid (occupied: a corner finite and >= level, the comparison of the mesh) or a
//                       caller's cell array -> `dilate` rounds of 26-neighbour dilation on one byte per cell (two buffers, read
//                       one, write the other) -> fine bits, 32 cells per word, and one bit per 8 x 8 x 8 brick.  One thread per
//                       cell, per word and per brick; every word is written by one thread from the bytes alone: no atomics, the
//                       same words every run.
//   upnerf_occ_spans    one thread per ray: slab test against the box, then Amanatides-Woo -- at brick level while the brick bit
//                       is clear, cell by cell inside a set brick.  All per-ray state is in registers (fp64: the t of a plane is
//                       (plane(i) - o) / d from the plane's INDEX, never a running sum, so the walk cannot drift and a t is one
//                       fp32 rounding from exact); the bit words are read-only and small (256^3 cells = 2 MiB), the rays of a
//                       wave are neighbouring pixels and read the same words.  No LDS.
//   upnerf_occ_compact  stable compaction of the hit rows: exclusive scan of the hit bytes (scan.cuh, shared with the mesh), then
//                       one thread per 16 bytes of a hit row, laid out over the output buffers as upnerf_path_rays lays its
//                       threads out.
//   upnerf_occ_scatter  results of the compacted rows back to full length; a row that is not in the (ascending) index is a miss
//                       and gets the background and its own far.  One thread per row, a binary search of the index.
// All stores are ordinary vector stores from plain C++.
#include "common.cuh"
#include "grid.cuh"
#include "scan.cuh"

#include <limits.h>
#include <math.h>

namespace {

// ---- build -----------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool occ_inside(float v, float level) { return isfinite(v) && v >= level; }

// one byte per cell: any corner of the cell inside (grid), or the caller's byte made 0 / 1 (cells)
__global__ __launch_bounds__(NTHREADS) void occ_flags_kernel(const float* grid, const uint8_t* cells, OccDims d, float level,
                                                              uint8_t* out) {
  const int64_t c = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (c >= d.cells) return;
  if (cells) {
    out[c] = cells[c] ? 1 : 0;
    return;
  }
  const int x = (int)(c % d.Cx), y = (int)((c / d.Cx) % d.Cy), z = (int)(c / ((int64_t)d.Cx * d.Cy));
  const int64_t Nx = d.Cx + 1, Ny = d.Cy + 1;
  int any = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t g = ((int64_t)(z + (k >> 2)) * Ny + (y + ((k >> 1) & 1))) * Nx + (x + (k & 1));
    any |= occ_inside(grid[g], level) ? 1 : 0;
  }
  out[c] = (uint8_t)any;
}

// one round: a cell is set iff any cell of the 3 x 3 x 3 block round it is
__global__ __launch_bounds__(NTHREADS) void occ_dilate_kernel(const uint8_t* in, OccDims d, uint8_t* out) {
  const int64_t c = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (c >= d.cells) return;
  const int x = (int)(c % d.Cx), y = (int)((c / d.Cx) % d.Cy), z = (int)(c / ((int64_t)d.Cx * d.Cy));
  int any = 0;
  for (int dz = -1; dz <= 1; ++dz) {
    const int zz = z + dz;
    if (zz < 0 || zz >= d.Cz) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= d.Cy) continue;
      const int64_t row = ((int64_t)zz * d.Cy + yy) * d.Cx;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = x + dx;
        if (xx >= 0 && xx < d.Cx) any |= in[row + xx];
      }
    }
  }
  out[c] = (uint8_t)(any ? 1 : 0);
}

// one byte per brick: any cell of the 8 x 8 x 8 block (cut at the grid's end) set
__global__ __launch_bounds__(NTHREADS) void occ_brick_flags_kernel(const uint8_t* in, OccDims d, uint8_t* out) {
  const int64_t b = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (b >= d.bricks) return;
  const int bx = (int)(b % d.Bx), by = (int)((b / d.Bx) % d.By), bz = (int)(b / ((int64_t)d.Bx * d.By));
  const int x0 = bx * OCC_BRICK, y0 = by * OCC_BRICK, z0 = bz * OCC_BRICK;
  const int x1 = min(x0 + OCC_BRICK, d.Cx), y1 = min(y0 + OCC_BRICK, d.Cy), z1 = min(z0 + OCC_BRICK, d.Cz);
  int any = 0;
  for (int z = z0; z < z1; ++z)
    for (int y = y0; y < y1; ++y) {
      const int64_t row = ((int64_t)z * d.Cy + y) * d.Cx;
      for (int x = x0; x < x1; ++x) any |= in[row + x];
    }
  out[b] = (uint8_t)(any ? 1 : 0);
}

// bytes -> bits: word w holds bytes [32 w, 32 w + 32), bit i = byte 32 w + i non-zero; bits past n are zero
__global__ __launch_bounds__(NTHREADS) void occ_pack_kernel(const uint8_t* in, int64_t n, int64_t n_words, uint32_t* words) {
  const int64_t w = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (w >= n_words) return;
  const int64_t base = w * 32;
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i)
    if (base + i < n && in[base + i]) v |= 1u << i;
  words[w] = v;
}

// ---- spans -----------------------------------------------------------------------------------------------------------------------

struct OccAxis {
  double lo, step, inv_step;  // plane i = lo + i * step
  double o, d, inv;           // inv = 1 / d (unused when d == 0)
  int C, i, sgn;              // cells, current cell, direction of travel (0: the ray does not move along this axis)
};

__host__ __device__ __forceinline__ double occ_plane(const OccAxis& a, int i) {
#pragma clang fp contract(off)
  const double p = (double)i * a.step;
  return a.lo + p;
}

// t at which the ray crosses plane i of the axis (d != 0)
__host__ __device__ __forceinline__ double occ_t(const OccAxis& a, int i) { return (occ_plane(a, i) - a.o) * a.inv; }

// the cell of coordinate p, held to [c0, c1]: the product with 1 / step proposes, the planes decide (a cell is [plane i, plane i+1))
__host__ __device__ __forceinline__ int occ_cell_of(const OccAxis& a, double p, int c0, int c1) {
  double f = floor((p - a.lo) * a.inv_step);
  int i = f < (double)c0 ? c0 : (f > (double)c1 ? c1 : (int)f);  // (a NaN compares false twice and is cast: held below)
  i = i < c0 ? c0 : (i > c1 ? c1 : i);
  if (i > c0 && p < occ_plane(a, i)) --i;
  else if (i < c1 && p >= occ_plane(a, i + 1)) ++i;
  return i;
}

__host__ __device__ __forceinline__ int occ_imin(int a, int b) { return a < b ? a : b; }

// the walk of one ray row (host and device: the host build is what tests/host/occ_host.hip, run by
// tests/test_walks_host_cpu.py, checks against brute force over every occupied cell)
__host__ __device__ __forceinline__ bool occ_walk(const upnerf_occ_spans_args& a, const OccDims& dm, const float* row, float* t0_out,
                                                  float* t1_out) {
  const float near = row[6], far = row[7];
  const int Cs[3] = {dm.Cx, dm.Cy, dm.Cz};
  OccAxis ax[3];
  double tn = (double)near, tf = (double)far;
  bool miss = !(far > near);  // (a NaN in near or far as well)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    OccAxis& A = ax[k];
    A.C = Cs[k];
    A.lo = (double)a.lo[k];
    A.step = ((double)a.hi[k] - (double)a.lo[k]) / (double)A.C;
    A.inv_step = 1.0 / A.step;
    A.o = (double)row[k];
    A.d = (double)row[3 + k];
    A.i = 0;
    if (A.d == 0.0) {  // no t comes out of this axis: inside its slab or a miss
      A.sgn = 0;
      A.inv = 0.0;
      if (!(A.o >= A.lo && A.o < (double)a.hi[k])) miss = true;
    } else {
      A.sgn = A.d > 0.0 ? 1 : -1;
      A.inv = 1.0 / A.d;
      const double ta = ((double)a.lo[k] - A.o) * A.inv, tb = ((double)a.hi[k] - A.o) * A.inv;
      tn = fmax(tn, fmin(ta, tb));  // (fmin / fmax drop a NaN operand: the test below sees what is left)
      tf = fmin(tf, fmax(ta, tb));
      if (A.d != A.d || A.o != A.o || !isfinite(A.inv)) miss = true;
    }
  }
  if (!(tf > tn)) miss = true;
  float t0 = far, t1 = far;
  bool hit = false;
  if (!miss) {
#pragma unroll
    for (int k = 0; k < 3; ++k) ax[k].i = occ_cell_of(ax[k], ax[k].o + tn * ax[k].d, 0, ax[k].C - 1);
    const uint32_t* fine = a.words;
    const uint32_t* brick = a.words + dm.fine_words;
    double t = tn, t_first = 0.0, t_last = 0.0;
    // every pass moves to another cell or brick along one axis, so the walk ends after at most sum(C) + sum(B) passes; the
    // budget is twice that, and nothing but a ray of numbers that are none could use it up
    int budget = 2 * (dm.Cx + dm.Cy + dm.Cz + dm.Bx + dm.By + dm.Bz) + 8;
    while (budget-- > 0) {
      const int ix = ax[0].i, iy = ax[1].i, iz = ax[2].i;
      if (ix < 0 || ix >= dm.Cx || iy < 0 || iy >= dm.Cy || iz < 0 || iz >= dm.Cz) break;
      const int bx = ix / OCC_BRICK, by = iy / OCC_BRICK, bz = iz / OCC_BRICK;
      const bool in_brick = occ_bit(brick, ((int64_t)bz * dm.By + by) * dm.Bx + bx);
      // the plane through which the ray leaves the cell (set brick) or the brick (clear brick), per axis, and the first of them
      int nxt[3];
      double tx = INFINITY;
      int axis = -1;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const OccAxis& A = ax[k];
        nxt[k] = A.i;
        if (A.sgn == 0) continue;
        int p;
        if (in_brick) p = A.sgn > 0 ? A.i + 1 : A.i;
        else p = A.sgn > 0 ? occ_imin((A.i / OCC_BRICK + 1) * OCC_BRICK, A.C) : (A.i / OCC_BRICK) * OCC_BRICK;
        nxt[k] = A.sgn > 0 ? p : p - 1;  // the cell behind that plane
        const double tk = occ_t(A, p);
        if (tk < tx) tx = tk, axis = k;
      }
      if (in_brick && occ_bit(fine, ((int64_t)iz * dm.Cy + iy) * dm.Cx + ix)) {
        const double te = fmin(tx, tf);
        if (te > t) {
          if (!hit) t_first = t, hit = true;
          t_last = te;
        }
      }
      if (axis < 0 || !(tx < tf)) break;  // the ray ends in this cell (or never leaves it: d == 0 on every axis)
      t = fmax(t, tx);
      if (!in_brick) {  // across a brick: the other axes find their cell again from the point of exit, inside this brick
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (k == axis) continue;
          OccAxis& A = ax[k];
          const int c0 = (A.i / OCC_BRICK) * OCC_BRICK;
          A.i = occ_cell_of(A, A.o + t * A.d, c0, occ_imin(c0 + OCC_BRICK - 1, A.C - 1));
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k == axis) ax[k].i = nxt[k];
    }
    if (hit) {
      t0 = fmaxf((float)t_first, near);
      t1 = fminf((float)t_last, far);
      hit = t1 > t0;
      if (!hit) t0 = t1 = far;
    }
  }
  *t0_out = t0;
  *t1_out = t1;
  return hit;
}

__global__ __launch_bounds__(NTHREADS) void occ_spans_kernel(upnerf_occ_spans_args a, OccDims dm) {
  const int r = blockIdx.x * NTHREADS + threadIdx.x;
  if (r >= a.R) return;
  float t0, t1;
  const bool hit = occ_walk(a, dm, a.rays + (int64_t)r * 8, &t0, &t1);
  a.t0[r] = t0;
  a.t1[r] = t1;
  a.hit[r] = hit ? 1 : 0;
}

// ---- compact ---------------------------------------------------------------------------------------------------------------------

// the grid over the output buffers, as in path.hip: segment 0 = the ray rows (two 16-byte groups each), segment 1 + i = table i
struct OccPlan {
  int blk0[UPNERF_PATH_MAX_TABLES + 2];
  int vec[UPNERF_PATH_MAX_TABLES + 1];
};

__global__ __launch_bounds__(NTHREADS) void occ_compact_kernel(upnerf_occ_compact_args a, OccPlan pl, const int32_t* pos) {
  int seg = 0;  // (uniform over the workgroup)
#pragma unroll
  for (int j = 1; j <= UPNERF_PATH_MAX_TABLES; ++j)
    if (j <= a.n_tables && (int)blockIdx.x >= pl.blk0[j]) seg = j;
  const int64_t id = (int64_t)((int)blockIdx.x - pl.blk0[seg]) * NTHREADS + threadIdx.x;
  if (seg == 0) {
    const int64_t r = id >> 1;
    if (r >= a.R || !a.hit[r]) return;
    const int half = (int)(id & 1);
    const int64_t k = pos[r];
    const float* src = a.rays + r * 8 + half * 4;
    f32x4 v;
    if (pl.vec[0]) v = *(const f32x4*)src;
    else v = f32x4{src[0], src[1], src[2], src[3]};
    if (half) v.z = a.t0[r], v.w = a.t1[r];
    else a.index[k] = (int32_t)r;
    float* dst = a.rays_c + k * 8 + half * 4;
    if (pl.vec[0]) *(f32x4*)dst = v;
    else dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
    return;
  }
  const upnerf_path_table tb = a.tables[seg - 1];
  const int gpr = (tb.dim + 3) >> 2;
  const int64_t r = id / gpr;
  if (r >= a.R || !a.hit[r]) return;
  const int j0 = (int)(id - r * gpr) * 4;
  const float* src = tb.table + r * tb.dim + j0;
  float* dst = tb.out + (int64_t)pos[r] * tb.dim + j0;
  if (pl.vec[seg]) {
    *(f32x4*)dst = *(const f32x4*)src;
  } else {
    const int cnt = tb.dim - j0 < 4 ? tb.dim - j0 : 4;
    for (int j = 0; j < cnt; ++j) dst[j] = src[j];
  }
}

int64_t occ_round16(int64_t x) { return (x + 15) / 16 * 16; }

bool occ_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- scatter ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NTHREADS) void occ_scatter_kernel(upnerf_occ_scatter_args a) {
  const int r = blockIdx.x * NTHREADS + threadIdx.x;
  if (r >= a.R) return;
  int lo = 0, hi = a.n_hit;  // first k with index[k] >= r
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.index[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  const bool found = lo < a.n_hit && a.index[lo] == r;
  float* o = a.rgb + (int64_t)r * 3;
  if (found) {
    const float* s = a.rgb_c + (int64_t)lo * 3;
    o[0] = s[0], o[1] = s[1], o[2] = s[2];
    if (a.depth) a.depth[r] = a.depth_c[lo];
  } else {
    o[0] = o[1] = o[2] = a.background;
    if (a.depth) a.depth[r] = a.rays[(int64_t)r * 8 + 7];
  }
}

}  // namespace

extern "C" long long upnerf_occ_words(int Cx, int Cy, int Cz) {
  OccDims d;
  if (!occ_dims(Cx, Cy, Cz, &d)) return UPNERF_EINVAL;
  return d.fine_words + d.brick_words;
}

extern "C" long long upnerf_occ_build_scratch(int Cx, int Cy, int Cz) {
  OccDims d;
  if (!occ_dims(Cx, Cy, Cz, &d)) return UPNERF_EINVAL;
  return 2 * occ_round16(d.cells);  // two byte-per-cell buffers (the brick bytes reuse the one that is free)
}

extern "C" int upnerf_occ_build(const upnerf_occ_build_args* a, void* stream) {
  OccDims d;
  if (!a || !occ_dims(a->Cx, a->Cy, a->Cz, &d) || a->dilate < 0) return UPNERF_EINVAL;
  if ((a->grid == nullptr) == (a->cells == nullptr) || !a->words || !a->scratch) return UPNERF_EINVAL;
  if (a->grid && a->level != a->level) return UPNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* buf[2] = {(uint8_t*)a->scratch, (uint8_t*)a->scratch + occ_round16(d.cells)};
  const unsigned nb = (unsigned)ceil_div64(d.cells, NTHREADS);
  hipLaunchKernelGGL(occ_flags_kernel, dim3(nb), dim3(NTHREADS), 0, st, a->grid, a->cells, d, a->level, buf[0]);
  int cur = 0;
  const int rounds = a->dilate < d.Cx + d.Cy + d.Cz ? a->dilate : d.Cx + d.Cy + d.Cz;  // (more rounds change nothing)
  for (int i = 0; i < rounds; ++i, cur ^= 1)
    hipLaunchKernelGGL(occ_dilate_kernel, dim3(nb), dim3(NTHREADS), 0, st, (const uint8_t*)buf[cur], d, buf[cur ^ 1]);
  hipLaunchKernelGGL(occ_pack_kernel, dim3((unsigned)ceil_div64(d.fine_words, NTHREADS)), dim3(NTHREADS), 0, st,
                     (const uint8_t*)buf[cur], d.cells, d.fine_words, a->words);
  hipLaunchKernelGGL(occ_brick_flags_kernel, dim3((unsigned)ceil_div64(d.bricks, NTHREADS)), dim3(NTHREADS), 0, st,
                     (const uint8_t*)buf[cur], d, buf[cur ^ 1]);
  hipLaunchKernelGGL(occ_pack_kernel, dim3((unsigned)ceil_div64(d.brick_words, NTHREADS)), dim3(NTHREADS), 0, st,
                     (const uint8_t*)buf[cur ^ 1], d.bricks, d.brick_words, a->words + d.fine_words);
  return (int)hipGetLastError();
}

extern "C" int upnerf_occ_spans(const upnerf_occ_spans_args* a, void* stream) {
  OccDims d;
  if (!a || !occ_dims(a->Cx, a->Cy, a->Cz, &d) || a->R <= 0) return UPNERF_EINVAL;
  if (!a->words || !a->rays || !a->t0 || !a->t1 || !a->hit) return UPNERF_EINVAL;
  for (int k = 0; k < 3; ++k)
    if (!(a->hi[k] > a->lo[k]) || !isfinite(a->hi[k]) || !isfinite(a->lo[k])) return UPNERF_EINVAL;
  hipLaunchKernelGGL(occ_spans_kernel, dim3((a->R + NTHREADS - 1) / NTHREADS), dim3(NTHREADS), 0, (hipStream_t)stream, *a, d);
  return (int)hipGetLastError();
}

extern "C" long long upnerf_occ_compact_scratch(int R) {
  if (R <= 0) return UPNERF_EINVAL;
  return occ_round16((int64_t)R * 4) + occ_round16(scan_level_ints(R) * 4);  // positions, then the levels of the scan
}

extern "C" int upnerf_occ_compact(const upnerf_occ_compact_args* a, void* stream) {
  if (!a || a->R <= 0) return UPNERF_EINVAL;
  if (a->n_tables < 0 || a->n_tables > UPNERF_PATH_MAX_TABLES) return UPNERF_EINVAL;
  if (!a->hit || !a->t0 || !a->t1 || !a->rays || !a->rays_c || !a->index || !a->count) return UPNERF_EINVAL;
  if (!a->scratch || !occ_aligned16(a->scratch)) return UPNERF_EINVAL;
  OccPlan pl = {};
  int64_t blocks = ((int64_t)a->R * 2 + NTHREADS - 1) / NTHREADS;
  pl.vec[0] = occ_aligned16(a->rays) && occ_aligned16(a->rays_c);
  for (int i = 0; i < a->n_tables; ++i) {
    const upnerf_path_table& tb = a->tables[i];
    if (tb.dim < 1 || tb.dim > UPNERF_PATH_MAX_DIM || !tb.table || !tb.out) return UPNERF_EINVAL;
    pl.blk0[i + 1] = (int)blocks;
    pl.vec[i + 1] = tb.dim % 4 == 0 && occ_aligned16(tb.table) && occ_aligned16(tb.out);
    blocks += ((int64_t)a->R * ((tb.dim + 3) / 4) + NTHREADS - 1) / NTHREADS;
  }
  if (blocks > 0x7fffffff) return UPNERF_EUNSUP;
  pl.blk0[a->n_tables + 1] = (int)blocks;
  hipStream_t st = (hipStream_t)stream;
  int32_t* pos = (int32_t*)a->scratch;
  int32_t* levels = (int32_t*)((uint8_t*)a->scratch + occ_round16((int64_t)a->R * 4));
  scan_exclusive<uint8_t, false>(a->hit, a->R, pos, levels, a->count, st);
  hipLaunchKernelGGL(occ_compact_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, st, *a, pl, (const int32_t*)pos);
  return (int)hipGetLastError();
}

extern "C" int upnerf_occ_scatter(const upnerf_occ_scatter_args* a, void* stream) {
  if (!a || a->R <= 0 || a->n_hit < 0 || a->n_hit > a->R || !a->rgb) return UPNERF_EINVAL;
  if (a->n_hit > 0 && (!a->index || !a->rgb_c)) return UPNERF_EINVAL;
  if (a->depth && (!a->rays || (a->n_hit > 0 && !a->depth_c))) return UPNERF_EINVAL;
  hipLaunchKernelGGL(occ_scatter_kernel, dim3((a->R + NTHREADS - 1) / NTHREADS), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}
