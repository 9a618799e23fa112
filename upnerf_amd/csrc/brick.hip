// A sparse baked scene: only the occupied 8 x 8 x 8-cell bricks of the grid are stored, each as 9 x 9 x 9 points (its far faces
// included, so every cell of a brick finds its eight corners inside it).  include/upnerf_hip.h states the layout once; DESIGN.md
// 2.33.  The marcher that reads the pool is in baked.hip.
//   upnerf_brick_table    brick bits -> one byte per brick -> exclusive scan (scan.cuh, as upnerf_occ_compact) -> slots (rank or -1)
//                         and bricks (the inverse), the count on the device.  The ranks are scanned into `slots` itself.
//   upnerf_brick_gather   dense grid -> pool, one thread per 4- or 16-byte word of the pool; a point beyond the grid is zero.
//   upnerf_brick_scatter  pool -> dense grid (zeroed by the caller); a grid point is stored by its owner brick alone.
//   upnerf_brick_occ      cell and brick bits from the pool: one thread per output word, every word written by one thread.
//   upnerf_brick_columns  the rays that make the field kernels evaluate the pool's lines (upnerf_grid_columns for a brick pool).
//   upnerf_brick_face_sum in place on a pool-shaped fp32 array, every copy of a point on a face that bricks share becomes the sum over
//                         the copies, in ascending brick index: one launch collects into the first copy, one spreads it.
//   upnerf_brick_face_max the same kernel with fmaxf for +: what a pool-shaped visibility needs.
// Everything is streaming and memory-bound; no LDS beyond the scan, no atomics.  All stores are ordinary vector stores from plain C++.
#include "common.cuh"
#include "grid.cuh"
#include "scan.cuh"

#include <limits.h>
#include <math.h>

namespace {

#define BRICK_P UPNERF_BRICK_POINTS
#define BRICK_N (BRICK_P * BRICK_P * BRICK_P)  // 729 points of a stored brick
#define BRICK_FACE (BRICK_N - 7 * 7 * 7)       // 386 of them have an l of 0 or 8: the points a neighbouring brick can share

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

int64_t brick_round16(int64_t x) { return (x + 15) / 16 * 16; }

bool brick_size_ok(int E) { return E == 4 || E == 16 || E == 32 || E == 64; }

// a pool point: its slot, where it lies in the brick, and the grid point it stands for
struct BrickPoint {
  int64_t slot;
  int lx, ly, lz, gx, gy, gz;
  bool in_grid;  // the brick is one of the grid's and the point is not beyond the grid's end
};

__device__ __forceinline__ BrickPoint brick_point(int64_t p, const int32_t* bricks, const OccDims& d) {
  BrickPoint q;
  q.slot = p / BRICK_N;
  const int l = (int)(p - q.slot * BRICK_N);
  q.lz = l / (BRICK_P * BRICK_P), q.ly = (l / BRICK_P) % BRICK_P, q.lx = l % BRICK_P;
  const int b = bricks[q.slot];
  const int bx = b % d.Bx, by = (b / d.Bx) % d.By, bz = b / (d.Bx * d.By);
  q.gx = bx * OCC_BRICK + q.lx, q.gy = by * OCC_BRICK + q.ly, q.gz = bz * OCC_BRICK + q.lz;
  q.in_grid = b >= 0 && b < d.bricks && q.gx <= d.Cx && q.gy <= d.Cy && q.gz <= d.Cz;
  return q;
}

__global__ __launch_bounds__(NTHREADS) void brick_flags_kernel(const uint32_t* brick_words, int64_t n, uint8_t* out) {
  const int64_t b = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (b < n) out[b] = occ_bit(brick_words, b) ? 1 : 0;
}

// slots holds the exclusive scan of the flags: an occupied brick keeps its rank and names itself in bricks, an empty one gets -1
__global__ __launch_bounds__(NTHREADS) void brick_emit_kernel(const uint8_t* flags, int64_t n, int32_t* slots, int32_t* bricks) {
  const int64_t b = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (b >= n) return;
  if (flags[b]) bricks[slots[b]] = (int32_t)b;
  else slots[b] = -1;
}

// W: the word a thread moves (uint32_t at E = 4, else 16 bytes); wpp: words per point
template <typename W>
__global__ __launch_bounds__(NTHREADS) void brick_gather_kernel(upnerf_brick_gather_args a, OccDims d, int wpp, int64_t n_words) {
  const int64_t id = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (id >= n_words) return;
  const int64_t p = id / wpp;
  const int q = (int)(id - p * wpp);
  const BrickPoint pt = brick_point(p, a.bricks, d);
  W v = {};
  if (pt.in_grid) {
    const int64_t g = ((int64_t)pt.gz * (d.Cy + 1) + pt.gy) * (d.Cx + 1) + pt.gx;
    v = ((const W*)a.grid)[g * wpp + q];
  }
  ((W*)a.pool)[id] = v;
}

template <typename W>
__global__ __launch_bounds__(NTHREADS) void brick_scatter_kernel(upnerf_brick_scatter_args a, OccDims d, int wpp, int64_t n_words) {
  const int64_t id = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (id >= n_words) return;
  const int64_t p = id / wpp;
  const int q = (int)(id - p * wpp);
  const BrickPoint pt = brick_point(p, a.bricks, d);
  if (!pt.in_grid) return;
  // the owner of a grid point is the brick of cell min(i, C - 1): a far face belongs to the next brick unless it is the grid's end
  if ((pt.lx == OCC_BRICK && pt.gx != d.Cx) || (pt.ly == OCC_BRICK && pt.gy != d.Cy) || (pt.lz == OCC_BRICK && pt.gz != d.Cz)) return;
  const int64_t g = ((int64_t)pt.gz * (d.Cy + 1) + pt.gy) * (d.Cx + 1) + pt.gx;
  ((W*)a.grid)[g * wpp + q] = ((const W*)a.pool)[id];
}

__device__ __forceinline__ bool brick_kept(const uint8_t* pool, int64_t p, int E, int off) {
  const float v = *(const float*)(pool + p * E + off);
  return isfinite(v) && v >= __builtin_bit_cast(float, 1u);  // (upnerf_occ_build's comparison at the smallest positive fp32)
}

// word w < fine_words: cells [32 w, 32 w + 32); after them the brick words, 32 bricks each
__global__ __launch_bounds__(NTHREADS) void brick_occ_kernel(upnerf_brick_occ_args a, OccDims d) {
  const int64_t w = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (w >= d.fine_words + d.brick_words) return;
  uint32_t v = 0;
  if (w < d.fine_words) {
    for (int i = 0; i < 32; ++i) {
      const int64_t c = w * 32 + i;
      if (c >= d.cells) break;
      const int x = (int)(c % d.Cx), y = (int)((c / d.Cx) % d.Cy), z = (int)(c / ((int64_t)d.Cx * d.Cy));
      const int slot = a.slots[((int64_t)(z / OCC_BRICK) * d.By + y / OCC_BRICK) * d.Bx + x / OCC_BRICK];
      if (slot < 0 || slot >= a.n_bricks) continue;
      const int64_t base = (int64_t)slot * BRICK_N + ((z % OCC_BRICK) * BRICK_P + y % OCC_BRICK) * BRICK_P + x % OCC_BRICK;
      bool any = false;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        any = any || brick_kept(a.pool, base + (k >> 2) * BRICK_P * BRICK_P + ((k >> 1) & 1) * BRICK_P + (k & 1), a.E, a.sigma_offset);
      if (any) v |= 1u << i;
    }
  } else {
    // a brick bit is the OR of its cells' bits, and those see exactly the brick's points inside the grid
    for (int i = 0; i < 32; ++i) {
      const int64_t b = (w - d.fine_words) * 32 + i;
      if (b >= d.bricks) break;
      const int slot = a.slots[b];
      if (slot < 0 || slot >= a.n_bricks) continue;
      const int bx = (int)(b % d.Bx), by = (int)((b / d.Bx) % d.By), bz = (int)(b / ((int64_t)d.Bx * d.By));
      const int nx = min(BRICK_P, d.Cx + 1 - bx * OCC_BRICK), ny = min(BRICK_P, d.Cy + 1 - by * OCC_BRICK);
      const int nz = min(BRICK_P, d.Cz + 1 - bz * OCC_BRICK);
      bool any = false;
      for (int lz = 0; lz < nz && !any; ++lz)
        for (int ly = 0; ly < ny && !any; ++ly)
          for (int lx = 0; lx < nx; ++lx)
            any = any || brick_kept(a.pool, (int64_t)slot * BRICK_N + (lz * BRICK_P + ly) * BRICK_P + lx, a.E, a.sigma_offset);
      if (any) v |= 1u << i;
    }
  }
  a.words[w] = v;
}

__global__ __launch_bounds__(NTHREADS) void brick_columns_kernel(upnerf_brick_columns_args a, int Bx, int By) {
  const int64_t id = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  const int64_t nz = (int64_t)a.count * a.S;
  const int64_t r = id < nz ? id / a.S : id - nz;  // z rows first, as upnerf_grid_columns lays its threads out
  if (r >= a.count) return;
  const int64_t line = a.line0 + r;
  const int64_t slot = line / (BRICK_P * BRICK_P);
  const int l = (int)(line - slot * (BRICK_P * BRICK_P));
  const int b = a.bricks[slot];
  const int bx = b % Bx, by = (b / Bx) % By, bz = b / (Bx * By);
  if (id < nz) {
    const int s = (int)(id - r * a.S);
    const int gz = bz * OCC_BRICK + (s < OCC_BRICK ? s : OCC_BRICK);
    a.z[id] = (float)grid_coord(a.lo[2], a.hi[2], a.Nz, gz < a.Nz ? gz : a.Nz - 1);
    return;
  }
  const int gx = bx * OCC_BRICK + l % BRICK_P, gy = by * OCC_BRICK + l / BRICK_P;
  float* o = a.o + r * 3;
  float* dd = a.d + r * 3;
  o[0] = (float)grid_coord(a.lo[0], a.hi[0], a.Nx, gx < a.Nx ? gx : a.Nx - 1);
  o[1] = (float)grid_coord(a.lo[1], a.hi[1], a.Ny, gy < a.Ny ? gy : a.Ny - 1);
  o[2] = 0.f;
  dd[0] = 0.f;
  dd[1] = 0.f;
  dd[2] = 1.f;
}

// face point f < 386 of a brick: the two z faces (81 points each), then the rim of the seven planes between them (32 each)
__device__ __forceinline__ void brick_face_point(int f, int* lx, int* ly, int* lz) {
  if (f < 2 * BRICK_P * BRICK_P) {
    *lz = (f / (BRICK_P * BRICK_P)) * OCC_BRICK, *ly = (f % (BRICK_P * BRICK_P)) / BRICK_P, *lx = f % BRICK_P;
    return;
  }
  f -= 2 * BRICK_P * BRICK_P;
  const int r = f % 32;
  *lz = 1 + f / 32;
  if (r < 2 * BRICK_P) *ly = (r / BRICK_P) * OCC_BRICK, *lx = r % BRICK_P;
  else *ly = 1 + (r - 2 * BRICK_P) / 2, *lx = ((r - 2 * BRICK_P) & 1) * OCC_BRICK;
}

// the bricks that hold grid point 8 b + l of an axis with B bricks, in ascending order, and where: one, or two on a shared plane
struct BrickHolders {
  int n, b0, l0, b1, l1;
  __device__ __forceinline__ int b(int i) const { return i ? b1 : b0; }  // (selects, not an indexed array: the state stays in registers)
  __device__ __forceinline__ int l(int i) const { return i ? l1 : l0; }
};

__device__ __forceinline__ BrickHolders brick_holders(int b, int l, int B) {
  BrickHolders h = {1, b, l, b, l};
  if (l == 0 && b > 0) h.n = 2, h.b0 = b - 1, h.l0 = OCC_BRICK;
  else if (l == OCC_BRICK && b + 1 < B) h.n = 2, h.b1 = b + 1, h.l1 = 0;
  return h;
}

struct BrickAdd {
  __device__ __forceinline__ float operator()(float a, float b) const { return a + b; }
};
struct BrickMax {
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
};

// COLLECT: the copy in the first occupied holder becomes the sum (Op: BrickAdd; the maximum with BrickMax) over the occupied
// holders, in ascending brick index; the other copies are read and not written.  !COLLECT (the launch after it): the other copies
// become the first.  One thread per float of a face point of a slot; a point with one copy, or beyond the grid, is left alone.
template <bool COLLECT, class Op>
__global__ __launch_bounds__(NTHREADS) void brick_face_sum_kernel(upnerf_brick_face_sum_args a, OccDims d, int64_t n_threads) {
  const int64_t id = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (id >= n_threads) return;
  const int64_t fp = id / a.F;
  const int q = (int)(id - fp * a.F);
  const int64_t slot = fp / BRICK_FACE;
  int lx, ly, lz;
  brick_face_point((int)(fp - slot * BRICK_FACE), &lx, &ly, &lz);
  const int b = a.bricks[slot];
  if (b < 0 || b >= d.bricks) return;
  const int bx = b % d.Bx, by = (b / d.Bx) % d.By, bz = b / (d.Bx * d.By);
  if (bx * OCC_BRICK + lx > d.Cx || by * OCC_BRICK + ly > d.Cy || bz * OCC_BRICK + lz > d.Cz) return;
  const BrickHolders hx = brick_holders(bx, lx, d.Bx), hy = brick_holders(by, ly, d.By), hz = brick_holders(bz, lz, d.Bz);
  const int64_t self = (slot * BRICK_N + (lz * BRICK_P + ly) * BRICK_P + lx) * a.F + q;
  int64_t first = -1;
  int m = 0;  // occupied holders met
  float sum = 0.0f;
  for (int iz = 0; iz < hz.n; ++iz)
    for (int iy = 0; iy < hy.n; ++iy)
      for (int ix = 0; ix < hx.n; ++ix) {
        const int s = a.slots[((int64_t)hz.b(iz) * d.By + hy.b(iy)) * d.Bx + hx.b(ix)];
        if (s < 0 || s >= a.n_bricks) continue;
        const int64_t at = ((int64_t)s * BRICK_N + (hz.l(iz) * BRICK_P + hy.l(iy)) * BRICK_P + hx.l(ix)) * a.F + q;
        if (first < 0) {
          if (COLLECT ? at != self : at == self) return;  // (collect: the first copy's thread alone works; spread: all but it)
          first = at;
          if (COLLECT) sum = a.data[at];
          else {
            a.data[self] = a.data[first];
            return;
          }
        } else {
          sum = Op()(sum, a.data[at]);
        }
        ++m;
      }
  if (COLLECT && m > 1) a.data[self] = sum;  // (with one copy nothing is written)
}

// the arguments gather and scatter share, and the words of the pool
template <class Args>
int brick_copy_check(const Args* a, const void* grid, const void* pool, OccDims* d, int* wpp, int64_t* n_words) {
  if (!a || !occ_dims(a->Cx, a->Cy, a->Cz, d) || !brick_size_ok(a->E)) return UPNERF_EINVAL;
  if (a->n_bricks < 1 || a->n_bricks > d->bricks || !a->bricks || !grid || !pool) return UPNERF_EINVAL;
  if (((uintptr_t)pool & (a->E - 1)) != 0 || ((uintptr_t)grid & ((a->E < 16 ? a->E : 16) - 1)) != 0) return UPNERF_EINVAL;
  *wpp = a->E == 4 ? 1 : a->E / 16;
  *n_words = (int64_t)a->n_bricks * BRICK_N * *wpp;
  if (ceil_div64(*n_words, NTHREADS) > INT_MAX) return UPNERF_EUNSUP;
  return 0;
}

}  // namespace

extern "C" long long upnerf_brick_table_scratch(int Cx, int Cy, int Cz) {
  OccDims d;
  if (!occ_dims(Cx, Cy, Cz, &d)) return UPNERF_EINVAL;
  return brick_round16(d.bricks) + brick_round16(scan_level_ints(d.bricks) * 4);  // a byte per brick, then the levels of the scan
}

extern "C" int upnerf_brick_table(const upnerf_brick_table_args* a, void* stream) {
  OccDims d;
  if (!a || !occ_dims(a->Cx, a->Cy, a->Cz, &d)) return UPNERF_EINVAL;
  if (!a->words || !a->slots || !a->bricks || !a->count || !a->scratch || ((uintptr_t)a->scratch & 15)) return UPNERF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* flags = (uint8_t*)a->scratch;
  int32_t* levels = (int32_t*)((uint8_t*)a->scratch + brick_round16(d.bricks));
  const unsigned nb = (unsigned)ceil_div64(d.bricks, NTHREADS);
  hipLaunchKernelGGL(brick_flags_kernel, dim3(nb), dim3(NTHREADS), 0, st, a->words + d.fine_words, d.bricks, flags);
  scan_exclusive<uint8_t, false>(flags, d.bricks, a->slots, levels, a->count, st);
  hipLaunchKernelGGL(brick_emit_kernel, dim3(nb), dim3(NTHREADS), 0, st, (const uint8_t*)flags, d.bricks, a->slots, a->bricks);
  return (int)hipGetLastError();
}

extern "C" int upnerf_brick_gather(const upnerf_brick_gather_args* a, void* stream) {
  OccDims d;
  int wpp;
  int64_t n;
  const int rc = brick_copy_check(a, a ? a->grid : nullptr, a ? a->pool : nullptr, &d, &wpp, &n);
  if (rc) return rc;
  const dim3 grid((unsigned)ceil_div64(n, NTHREADS)), block(NTHREADS);
  if (a->E == 4) hipLaunchKernelGGL(brick_gather_kernel<uint32_t>, grid, block, 0, (hipStream_t)stream, *a, d, wpp, n);
  else hipLaunchKernelGGL(brick_gather_kernel<u32x4>, grid, block, 0, (hipStream_t)stream, *a, d, wpp, n);
  return (int)hipGetLastError();
}

extern "C" int upnerf_brick_scatter(const upnerf_brick_scatter_args* a, void* stream) {
  OccDims d;
  int wpp;
  int64_t n;
  const int rc = brick_copy_check(a, a ? a->grid : nullptr, a ? a->pool : nullptr, &d, &wpp, &n);
  if (rc) return rc;
  const dim3 grid((unsigned)ceil_div64(n, NTHREADS)), block(NTHREADS);
  if (a->E == 4) hipLaunchKernelGGL(brick_scatter_kernel<uint32_t>, grid, block, 0, (hipStream_t)stream, *a, d, wpp, n);
  else hipLaunchKernelGGL(brick_scatter_kernel<u32x4>, grid, block, 0, (hipStream_t)stream, *a, d, wpp, n);
  return (int)hipGetLastError();
}

extern "C" int upnerf_brick_occ(const upnerf_brick_occ_args* a, void* stream) {
  OccDims d;
  if (!a || !occ_dims(a->Cx, a->Cy, a->Cz, &d) || !brick_size_ok(a->E)) return UPNERF_EINVAL;
  if (a->sigma_offset < 0 || (a->sigma_offset & 3) || a->sigma_offset > a->E - 4) return UPNERF_EINVAL;
  if (a->n_bricks < 0 || a->n_bricks > d.bricks || !a->slots || !a->words) return UPNERF_EINVAL;
  if (a->n_bricks > 0 && (!a->pool || ((uintptr_t)a->pool & (a->E - 1)) != 0)) return UPNERF_EINVAL;
  hipLaunchKernelGGL(brick_occ_kernel, dim3((unsigned)ceil_div64(d.fine_words + d.brick_words, NTHREADS)), dim3(NTHREADS), 0,
                     (hipStream_t)stream, *a, d);
  return (int)hipGetLastError();
}

extern "C" int upnerf_brick_columns(const upnerf_brick_columns_args* a, void* stream) {
  OccDims d;
  if (!a || a->Nx < 2 || a->Ny < 2 || a->Nz < 2 || !occ_dims(a->Nx - 1, a->Ny - 1, a->Nz - 1, &d)) return UPNERF_EINVAL;
  if (a->S < 32 || a->count < 1 || a->line0 < 0 || a->n_bricks < 1 || a->n_bricks > d.bricks) return UPNERF_EINVAL;
  if (a->line0 + a->count > (int64_t)a->n_bricks * (BRICK_P * BRICK_P)) return UPNERF_EINVAL;
  if (!a->bricks || !a->o || !a->d || !a->z) return UPNERF_EINVAL;
  for (int k = 0; k < 3; ++k)
    if (!isfinite(a->lo[k]) || !isfinite(a->hi[k])) return UPNERF_EINVAL;
  const int64_t blocks = ceil_div64((int64_t)a->count * a->S + a->count, NTHREADS);
  if (blocks > INT_MAX) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(brick_columns_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a, d.Bx, d.By);
  return (int)hipGetLastError();
}

namespace {

template <class Op>
int brick_face_reduce(const upnerf_brick_face_sum_args* a, void* stream) {
  OccDims d;
  if (!a || !occ_dims(a->Cx, a->Cy, a->Cz, &d) || a->F < 1) return UPNERF_EINVAL;
  if (a->n_bricks < 1 || a->n_bricks > d.bricks || !a->slots || !a->bricks || !a->data || ((uintptr_t)a->data & 3) != 0) return UPNERF_EINVAL;
  const int64_t n = (int64_t)a->n_bricks * BRICK_FACE * a->F;
  if (ceil_div64(n, NTHREADS) > INT_MAX) return UPNERF_EUNSUP;
  const dim3 grid((unsigned)ceil_div64(n, NTHREADS)), block(NTHREADS);
  hipLaunchKernelGGL((brick_face_sum_kernel<true, Op>), grid, block, 0, (hipStream_t)stream, *a, d, n);
  hipLaunchKernelGGL((brick_face_sum_kernel<false, Op>), grid, block, 0, (hipStream_t)stream, *a, d, n);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int upnerf_brick_face_sum(const upnerf_brick_face_sum_args* a, void* stream) { return brick_face_reduce<BrickAdd>(a, stream); }

extern "C" int upnerf_brick_face_max(const upnerf_brick_face_sum_args* a, void* stream) { return brick_face_reduce<BrickMax>(a, stream); }
