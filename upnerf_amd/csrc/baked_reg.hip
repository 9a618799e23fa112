// Coarse-to-fine baked scenes: the total variation of a point array with its gradient, and the doubling of a scene's resolution,
// both for a dense grid and for a brick pool.  include/upnerf_hip.h states every definition once; DESIGN.md 2.37.
//   upnerf_baked_tv            value (per-workgroup partial sums) and gradient (gather form, added) of the TV over the occupied
//                              cells.  One workgroup per 8 x 8 x 8-point tile of a dense grid, staged in LDS with a one-point halo
//                              on either side (10^3 points), or per brick of a pool (9^3 points, no halo: a copy receives what the
//                              cells of its own brick give it).  The floats of a point are staged TV_FS at a time.
//   upnerf_baked_upsample      dense grid -> the grid of twice the cells, one thread per child point, packed at `level`.
//   upnerf_brick_upsample_mark the brick bits of the child grid of a pool: one workgroup per word of 32 child bricks.
//   upnerf_brick_upsample_fill the child pool, one thread per child pool point, read from the 5 x 5 x 5 block of its parent brick.
// No atomics; every output address has one writer; all stores are ordinary vector stores from plain C++.
#include "common.cuh"
#include "grid.cuh"

#include <limits.h>
#include <math.h>

#include <type_traits>

namespace {

#define BRICK_P UPNERF_BRICK_POINTS
#define BRICK_N (BRICK_P * BRICK_P * BRICK_P)
#define TV_FS 8     // floats of a point staged at a time: 10^3 x 8 x 4 bytes = 32 KB of LDS (dense), 9^3 x 8 x 4 = 23 KB (pool)
#define TV_TILE 8   // points per axis of a dense tile
#define TV_MAX_F 28

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

int64_t reg_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- total variation ------------------------------------------------------------------------------------------------------------------

// tv of the cell whose base point is LDS entry `at`: the three forward differences and sqrtf(eps + dx^2 + dy^2 + dz^2)
__device__ __forceinline__ float tv_cell(const float* t, int at, int sy, int sz, float eps, float* dx, float* dy, float* dz) {
  const float a = t[at];
  *dx = t[at + 1] - a, *dy = t[at + sy] - a, *dz = t[at + sz] - a;
  return sqrtf(fmaf(*dz, *dz, fmaf(*dy, *dy, fmaf(*dx, *dx, eps))));
}

template <bool POOL>
__global__ __launch_bounds__(NTHREADS) void baked_tv_kernel(upnerf_baked_tv_args a, OccDims d, int Tx, int Ty) {
  constexpr int TN = POOL ? BRICK_P : TV_TILE + 2, H = POOL ? 0 : 1, PN = POOL ? BRICK_P : TV_TILE;
  constexpr int TN3 = TN * TN * TN, NP = PN * PN * PN, SY = TN, SZ = TN * TN;
  __shared__ float tile[TN3 * TV_FS];
  __shared__ float red[NTHREADS];
  const int tid = threadIdx.x;
  int ox, oy, oz;
  bool valid = true;
  if (POOL) {
    const int b = a.bricks[blockIdx.x];
    valid = b >= 0 && b < d.bricks;  // (uniform over the workgroup)
    ox = (b % d.Bx) * OCC_BRICK, oy = ((b / d.Bx) % d.By) * OCC_BRICK, oz = (b / (d.Bx * d.By)) * OCC_BRICK;
  } else {
    ox = (int)(blockIdx.x % Tx) * TV_TILE, oy = (int)((blockIdx.x / Tx) % Ty) * TV_TILE, oz = (int)(blockIdx.x / ((int64_t)Tx * Ty)) * TV_TILE;
  }
  const int64_t Nx = (int64_t)d.Cx + 1, Ny = (int64_t)d.Cy + 1;
  const int64_t pool_base = (int64_t)blockIdx.x * BRICK_N;
  // local cell (cx, cy, cz) of this tile or brick: inside the grid, inside the brick (pool), and its bit set
  auto cell_on = [&](int cx, int cy, int cz) -> bool {
    if (POOL && (cx < 0 || cy < 0 || cz < 0 || cx >= OCC_BRICK || cy >= OCC_BRICK || cz >= OCC_BRICK)) return false;
    const int gx = ox + cx, gy = oy + cy, gz = oz + cz;
    if (gx < 0 || gy < 0 || gz < 0 || gx >= d.Cx || gy >= d.Cy || gz >= d.Cz) return false;
    return occ_bit(a.words, ((int64_t)gz * d.Cy + gy) * d.Cx + gx);
  };
  float v = 0.0f;
  for (int f0 = 0; valid && f0 < a.F; f0 += TV_FS) {
    const int fs = a.F - f0 < TV_FS ? a.F - f0 : TV_FS;
    __syncthreads();  // the readers of the slice before are done
    for (int idx = tid; idx < TN3 * fs; idx += NTHREADS) {
      const int f = idx % fs, lp = idx / fs;
      float val = 0.0f;
      if (POOL) {
        val = a.data[(pool_base + lp) * a.F + f0 + f];
      } else {
        const int gx = ox + lp % TN - H, gy = oy + (lp / TN) % TN - H, gz = oz + lp / (TN * TN) - H;
        if (gx >= 0 && gy >= 0 && gz >= 0 && gx <= d.Cx && gy <= d.Cy && gz <= d.Cz) val = a.data[(((int64_t)gz * Ny + gy) * Nx + gx) * a.F + f0 + f];
      }
      tile[f * TN3 + lp] = val;
    }
    __syncthreads();
    for (int pt = tid; pt < NP; pt += NTHREADS) {
      const int x = pt % PN, y = (pt / PN) % PN, z = pt / (PN * PN);
      const int gx = ox + x, gy = oy + y, gz = oz + z;
      if (gx > d.Cx || gy > d.Cy || gz > d.Cz) continue;  // beyond the grid: nothing
      const bool own = cell_on(x, y, z), cx = cell_on(x - 1, y, z), cy = cell_on(x, y - 1, z), cz = cell_on(x, y, z - 1);
      if (!own && !cx && !cy && !cz) continue;
      const int64_t gi = POOL ? pool_base + pt : ((int64_t)gz * Ny + gy) * Nx + gx;
      const bool live = a.sigma[gi * a.sigma_stride] != 0.0f;
      const int at = ((z + H) * TN + (y + H)) * TN + (x + H);
      for (int f = 0; f < fs; ++f) {
        const float wf = a.w[f0 + f];
        if (wf == 0.0f) continue;
        const float* t = tile + f * TN3;
        float dx, dy, dz, g = 0.0f;
        if (own) {
          const float tv = tv_cell(t, at, SY, SZ, a.eps, &dx, &dy, &dz);
          v = fmaf(wf, tv, v);
          g = -((dx + dy) + dz) / tv;
        }
        if (!live) continue;
        if (cx) {
          const float tv = tv_cell(t, at - 1, SY, SZ, a.eps, &dx, &dy, &dz);
          g += dx / tv;
        }
        if (cy) {
          const float tv = tv_cell(t, at - SY, SY, SZ, a.eps, &dx, &dy, &dz);
          g += dy / tv;
        }
        if (cz) {
          const float tv = tv_cell(t, at - SZ, SY, SZ, a.eps, &dx, &dy, &dz);
          g += dz / tv;
        }
        float* out = a.grad + gi * a.F + f0 + f;
        *out = fmaf(wf, g, *out);
      }
    }
  }
  if (!a.partial) return;
  red[tid] = v;
  __syncthreads();
  for (int s = NTHREADS / 2; s > 0; s >>= 1) {  // a fixed tree: the same bits every run
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) a.partial[blockIdx.x] = red[0];
}

// the workgroups of a TV launch (= the partial sums it writes), or a refusal
int64_t tv_blocks(int Cx, int Cy, int Cz, int n_bricks, OccDims* d, int* Tx, int* Ty) {
  if (!occ_dims(Cx, Cy, Cz, d) || n_bricks < 0 || n_bricks > d->bricks) return UPNERF_EINVAL;
  if (n_bricks > 0) return n_bricks;
  *Tx = (int)reg_ceil_div((int64_t)Cx + 1, TV_TILE), *Ty = (int)reg_ceil_div((int64_t)Cy + 1, TV_TILE);
  const int64_t n = (int64_t)*Tx * *Ty * reg_ceil_div((int64_t)Cz + 1, TV_TILE);
  return n > INT_MAX ? UPNERF_EUNSUP : n;
}

// ---- doubling the resolution ----------------------------------------------------------------------------------------------------------

template <int DEG>
struct Up {
  static constexpr int NB = (DEG + 1) * (DEG + 1), NV = DEG == 0 ? 4 : 3 * NB + 1, Q = 1 << DEG, E = 16 << DEG;
};

// the numbers of a stored point: r, g, b, sigma, or the 3 nb halves (converted exactly) and then sigma
template <int DEG>
__device__ __forceinline__ void up_load(const uint8_t* p, float* v) {
  constexpr int Q = Up<DEG>::Q;
  uint32_t w[4 * Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const u32x4 r = ((const u32x4*)p)[q];
    w[4 * q] = r.x, w[4 * q + 1] = r.y, w[4 * q + 2] = r.z, w[4 * q + 3] = r.w;
  }
  if constexpr (DEG == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = __builtin_bit_cast(float, w[i]);
  } else {
#pragma unroll
    for (int h = 0; h < 3 * Up<DEG>::NB; ++h) v[h] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[h >> 1] >> ((h & 1) * 16)));
    v[3 * Up<DEG>::NB] = __builtin_bit_cast(float, w[4 * Q - 2]);
  }
}

// the child point between the parents base (+ sx if ox) (+ sy if oy) (+ sz if oz), indices in points: blended per axis -- x pairs,
// then y, then z, each 0.5f * (a + b) -- and packed at `level` by the rule of upnerf_baked_pack / upnerf_baked_sh_pack into rec
template <int DEG>
__device__ __forceinline__ bool up_child(const uint8_t* parent, int64_t base, int64_t sx, int64_t sy, int64_t sz, bool ox, bool oy,
                                         bool oz, float level, uint32_t* rec) {
  constexpr int NV = Up<DEG>::NV, Q = Up<DEG>::Q, E = Up<DEG>::E;
  float vz[NV] = {};
  for (int iz = 0; iz <= (oz ? 1 : 0); ++iz) {
    float vy[NV] = {};
    for (int iy = 0; iy <= (oy ? 1 : 0); ++iy) {
      float vx[NV];
      const int64_t at = base + iz * sz + iy * sy;
      up_load<DEG>(parent + at * E, vx);
      if (ox) {
        float b[NV];
        up_load<DEG>(parent + (at + sx) * E, b);
#pragma unroll
        for (int i = 0; i < NV; ++i) vx[i] = 0.5f * (vx[i] + b[i]);
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) vy[i] = iy == 0 ? vx[i] : 0.5f * (vy[i] + vx[i]);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) vz[i] = iz == 0 ? vy[i] : 0.5f * (vz[i] + vy[i]);
  }
  const float s = vz[NV - 1];
  bool keep = isfinite(s) && s > 0.0f && s >= level;
#pragma unroll
  for (int i = 0; i < 4 * Q; ++i) rec[i] = 0u;
  if constexpr (DEG == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) rec[i] = keep ? __builtin_bit_cast(uint32_t, vz[i]) : 0u;
  } else {
#pragma unroll
    for (int h = 0; h < NV - 1; ++h) {
      keep = keep && isfinite(vz[h]);
      const _Float16 half = (_Float16)fminf(fmaxf(vz[h], -65504.0f), 65504.0f);  // (the conversion rounds to nearest even)
      rec[h >> 1] |= (uint32_t)__builtin_bit_cast(uint16_t, half) << ((h & 1) * 16);
    }
    rec[4 * Q - 2] = __builtin_bit_cast(uint32_t, s);
    if (!keep) {
#pragma unroll
      for (int i = 0; i < 4 * Q; ++i) rec[i] = 0u;
    }
  }
  return keep;
}

template <int DEG>
__device__ __forceinline__ void up_store(uint8_t* out, int64_t id, const uint32_t* rec) {
  constexpr int Q = Up<DEG>::Q;
  u32x4* o = (u32x4*)out + id * Q;
#pragma unroll
  for (int q = 0; q < Q; ++q) o[q] = u32x4{rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]};
}

template <int DEG>
__global__ __launch_bounds__(NTHREADS) void baked_upsample_kernel(upnerf_baked_upsample_args a, int64_t n) {
  const int64_t id = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (id >= n) return;
  const int64_t Mx = 2 * (int64_t)a.Cx + 1, My = 2 * (int64_t)a.Cy + 1, Nx = (int64_t)a.Cx + 1, Ny = (int64_t)a.Cy + 1;
  const int i = (int)(id % Mx), j = (int)((id / Mx) % My), k = (int)(id / (Mx * My));
  uint32_t rec[4 * Up<DEG>::Q];
  up_child<DEG>(a.points, ((int64_t)(k >> 1) * Ny + (j >> 1)) * Nx + (i >> 1), 1, Nx, Nx * Ny, i & 1, j & 1, k & 1, a.level, rec);
  up_store<DEG>(a.out, id, rec);
}

// child brick cb of the child grid dc, and the pool point (lx, ly, lz) in it: where its parents are in the parent pool
struct UpBrick {
  int bx, by, bz;    // the child brick
  int64_t parent;    // the parent brick's slot (< 0: the parent is empty, the child is)
};

__device__ __forceinline__ UpBrick up_brick(int cb, const OccDims& dc, const OccDims& dp, const int32_t* slots, int n_bricks) {
  UpBrick u;
  u.bx = cb % dc.Bx, u.by = (cb / dc.Bx) % dc.By, u.bz = cb / (dc.Bx * dc.By);
  const int s = slots[((int64_t)(u.bz >> 1) * dp.By + (u.by >> 1)) * dp.Bx + (u.bx >> 1)];
  u.parent = s >= 0 && s < n_bricks ? s : -1;
  return u;
}

// point l (0 .. 728) of child brick u: false beyond the child grid; else the record of the child point
template <int DEG>
__device__ __forceinline__ bool up_pool_point(const upnerf_brick_upsample_args& a, const UpBrick& u, const OccDims& dc, int l, uint32_t* rec,
                                              bool* in_grid) {
  const int lx = l % BRICK_P, ly = (l / BRICK_P) % BRICK_P, lz = l / (BRICK_P * BRICK_P);
  *in_grid = u.bx * OCC_BRICK + lx <= dc.Cx && u.by * OCC_BRICK + ly <= dc.Cy && u.bz * OCC_BRICK + lz <= dc.Cz;
  if (!*in_grid) return false;
  const int px = 4 * (u.bx & 1) + (lx >> 1), py = 4 * (u.by & 1) + (ly >> 1), pz = 4 * (u.bz & 1) + (lz >> 1);
  return up_child<DEG>(a.pool, u.parent * BRICK_N + (pz * BRICK_P + py) * BRICK_P + px, 1, BRICK_P, BRICK_P * BRICK_P, lx & 1, ly & 1,
                       lz & 1, a.level, rec);
}

// one workgroup per word of 32 child bricks: a child brick is occupied iff one of its points inside the child grid is kept
template <int DEG>
__global__ __launch_bounds__(NTHREADS) void brick_upsample_mark_kernel(upnerf_brick_upsample_args a, OccDims dp, OccDims dc) {
  uint32_t v = 0;
  for (int i = 0; i < 32; ++i) {
    const int64_t cb = (int64_t)blockIdx.x * 32 + i;
    if (cb >= dc.bricks) break;
    const UpBrick u = up_brick((int)cb, dc, dp, a.slots, a.n_bricks);
    if (u.parent < 0) continue;  // (uniform over the workgroup, as the break above)
    int any = 0;
    for (int l = threadIdx.x; l < BRICK_N; l += NTHREADS) {
      uint32_t rec[4 * Up<DEG>::Q];
      bool in_grid;
      any |= up_pool_point<DEG>(a, u, dc, l, rec, &in_grid) ? 1 : 0;
    }
    if (__syncthreads_or(any)) v |= 1u << i;
  }
  if (threadIdx.x == 0) a.words[dc.fine_words + blockIdx.x] = v;
}

template <int DEG>
__global__ __launch_bounds__(NTHREADS) void brick_upsample_fill_kernel(upnerf_brick_upsample_args a, OccDims dp, OccDims dc, int64_t n) {
  const int64_t id = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (id >= n) return;
  const int64_t slot = id / BRICK_N;
  const int cb = a.child_bricks[slot];
  uint32_t rec[4 * Up<DEG>::Q];
#pragma unroll
  for (int i = 0; i < 4 * Up<DEG>::Q; ++i) rec[i] = 0u;
  if (cb >= 0 && cb < dc.bricks) {
    const UpBrick u = up_brick(cb, dc, dp, a.slots, a.n_bricks);
    bool in_grid;
    if (u.parent >= 0) up_pool_point<DEG>(a, u, dc, (int)(id - slot * BRICK_N), rec, &in_grid);
  }
  up_store<DEG>(a.out, id, rec);
}

template <class F>
void reg_by_degree(int degree, F&& f) {
  if (degree == 0) return f(std::integral_constant<int, 0>());
  if (degree == 1) return f(std::integral_constant<int, 1>());
  return f(std::integral_constant<int, 2>());
}

// what mark and fill share: the parent's and the child's dimensions
int brick_upsample_check(const upnerf_brick_upsample_args* a, OccDims* dp, OccDims* dc) {
  if (!a || !occ_dims(a->Cx, a->Cy, a->Cz, dp) || a->Cx > INT_MAX / 2 || a->Cy > INT_MAX / 2 || a->Cz > INT_MAX / 2) return UPNERF_EINVAL;
  if (!occ_dims(2 * a->Cx, 2 * a->Cy, 2 * a->Cz, dc)) return UPNERF_EINVAL;
  if (a->degree < 0 || a->degree > 2 || a->level != a->level) return UPNERF_EINVAL;
  if (a->n_bricks < 1 || a->n_bricks > dp->bricks || !a->slots || !a->pool) return UPNERF_EINVAL;
  if (((uintptr_t)a->pool & (((size_t)16 << a->degree) - 1)) != 0) return UPNERF_EINVAL;
  return 0;
}

}  // namespace

extern "C" long long upnerf_baked_tv_blocks(int Cx, int Cy, int Cz, int n_bricks) {
  OccDims d;
  int Tx = 0, Ty = 0;
  return tv_blocks(Cx, Cy, Cz, n_bricks, &d, &Tx, &Ty);
}

extern "C" int upnerf_baked_tv(const upnerf_baked_tv_args* a, void* stream) {
  OccDims d;
  int Tx = 0, Ty = 0;
  if (!a) return UPNERF_EINVAL;
  const int64_t blocks = tv_blocks(a->Cx, a->Cy, a->Cz, a->n_bricks, &d, &Tx, &Ty);
  if (blocks < 0) return (int)blocks;
  if (!a->words || !a->data || !a->sigma || !a->grad || a->F < 1 || a->F > TV_MAX_F || a->sigma_stride < 1) return UPNERF_EINVAL;
  if ((a->n_bricks > 0) != (a->slots != nullptr) || (a->n_bricks > 0) != (a->bricks != nullptr)) return UPNERF_EINVAL;
  if (!(a->eps > 0.0f) || !isfinite(a->eps)) return UPNERF_EINVAL;
  for (int f = 0; f < a->F; ++f)
    if (!isfinite(a->w[f])) return UPNERF_EINVAL;
  if (a->n_bricks > 0) hipLaunchKernelGGL(baked_tv_kernel<true>, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a, d, Tx, Ty);
  else hipLaunchKernelGGL(baked_tv_kernel<false>, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a, d, Tx, Ty);
  return (int)hipGetLastError();
}

extern "C" int upnerf_baked_upsample(const upnerf_baked_upsample_args* a, void* stream) {
  OccDims dp, dc;
  if (!a || !occ_dims(a->Cx, a->Cy, a->Cz, &dp) || a->Cx > INT_MAX / 2 || a->Cy > INT_MAX / 2 || a->Cz > INT_MAX / 2) return UPNERF_EINVAL;
  if (!occ_dims(2 * a->Cx, 2 * a->Cy, 2 * a->Cz, &dc)) return UPNERF_EINVAL;
  if (a->degree < 0 || a->degree > 2 || a->level != a->level || !a->points || !a->out) return UPNERF_EINVAL;
  const size_t mask = ((size_t)16 << a->degree) - 1;
  if (((uintptr_t)a->points & mask) != 0 || ((uintptr_t)a->out & mask) != 0) return UPNERF_EINVAL;
  const int64_t n = (2 * (int64_t)a->Cx + 1) * (2 * (int64_t)a->Cy + 1) * (2 * (int64_t)a->Cz + 1);
  if (reg_ceil_div(n, NTHREADS) > INT_MAX) return UPNERF_EUNSUP;
  reg_by_degree(a->degree, [&](auto deg) {
    hipLaunchKernelGGL(baked_upsample_kernel<decltype(deg)::value>, dim3((unsigned)reg_ceil_div(n, NTHREADS)), dim3(NTHREADS), 0, (hipStream_t)stream, *a, n);
  });
  return (int)hipGetLastError();
}

extern "C" int upnerf_brick_upsample_mark(const upnerf_brick_upsample_args* a, void* stream) {
  OccDims dp, dc;
  if (const int rc = brick_upsample_check(a, &dp, &dc)) return rc;
  if (!a->words) return UPNERF_EINVAL;
  reg_by_degree(a->degree, [&](auto deg) {
    hipLaunchKernelGGL(brick_upsample_mark_kernel<decltype(deg)::value>, dim3((unsigned)dc.brick_words), dim3(NTHREADS), 0, (hipStream_t)stream, *a, dp, dc);
  });
  return (int)hipGetLastError();
}

extern "C" int upnerf_brick_upsample_fill(const upnerf_brick_upsample_args* a, void* stream) {
  OccDims dp, dc;
  if (const int rc = brick_upsample_check(a, &dp, &dc)) return rc;
  if (a->n_child < 1 || a->n_child > dc.bricks || !a->child_bricks || !a->out) return UPNERF_EINVAL;
  if (((uintptr_t)a->out & (((size_t)16 << a->degree) - 1)) != 0) return UPNERF_EINVAL;
  const int64_t n = (int64_t)a->n_child * BRICK_N;
  if (reg_ceil_div(n, NTHREADS) > INT_MAX) return UPNERF_EUNSUP;
  reg_by_degree(a->degree, [&](auto deg) {
    hipLaunchKernelGGL(brick_upsample_fill_kernel<decltype(deg)::value>, dim3((unsigned)reg_ceil_div(n, NTHREADS)), dim3(NTHREADS), 0, (hipStream_t)stream, *a, dp, dc, n);
  });
  return (int)hipGetLastError();
}
