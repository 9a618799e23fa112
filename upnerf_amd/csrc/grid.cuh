// The coordinates of a regular grid over fp32 bounds, shared by everything that lives on one (mesh.hip, tsdf.hip), and the packed
// occupancy of its cells (occupancy.hip builds and walks it, baked.hip marches through it).
#pragma once
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>

// coordinate i of n evenly spaced grid coordinates over [lo, hi]: fp64 from the fp32 bounds, every operation rounded on its
// own (no fma), so that numpy's lo + i * ((hi - lo) / (n - 1)) in float64 gives the same bits
__device__ __forceinline__ double grid_coord(float lo, float hi, int n, int i) {
#pragma clang fp contract(off)
  if (n < 2) return (double)lo;
  const double step = ((double)hi - (double)lo) / (double)(n - 1);
  const double p = (double)i * step;
  return (double)lo + p;
}

// ---- packed occupancy (include/upnerf_hip.h: fine bits, 32 cells per word, then one bit per 8 x 8 x 8 brick) ------------------------
#define OCC_BRICK 8

struct OccDims {
  int Cx, Cy, Cz, Bx, By, Bz;
  int64_t cells, bricks, fine_words, brick_words;
};

static inline bool occ_dims(int Cx, int Cy, int Cz, OccDims* d) {
  if (Cx < 1 || Cy < 1 || Cz < 1) return false;
  const int64_t cells = (int64_t)Cx * Cy * Cz;
  if ((int64_t)Cx * Cy > INT_MAX || cells > INT_MAX) return false;
  d->Cx = Cx, d->Cy = Cy, d->Cz = Cz;
  d->Bx = (Cx + OCC_BRICK - 1) / OCC_BRICK, d->By = (Cy + OCC_BRICK - 1) / OCC_BRICK, d->Bz = (Cz + OCC_BRICK - 1) / OCC_BRICK;
  d->cells = cells;
  d->bricks = (int64_t)d->Bx * d->By * d->Bz;
  d->fine_words = (cells + 31) / 32;
  d->brick_words = (d->bricks + 31) / 32;
  return true;
}

__host__ __device__ __forceinline__ bool occ_bit(const uint32_t* words, int64_t b) { return (words[b >> 5] >> (b & 31)) & 1u; }
