// The coordinates of a regular grid over fp32 bounds, shared by everything that lives on one (mesh.hip, tsdf.hip).
#pragma once
#include <hip/hip_runtime.h>

// coordinate i of n evenly spaced grid coordinates over [lo, hi]: fp64 from the fp32 bounds, every operation rounded on its
// own (no fma), so that numpy's lo + i * ((hi - lo) / (n - 1)) in float64 gives the same bits
__device__ __forceinline__ double grid_coord(float lo, float hi, int n, int i) {
#pragma clang fp contract(off)
  if (n < 2) return (double)lo;
  const double step = ((double)hi - (double)lo) / (double)(n - 1);
  const double p = (double)i * step;
  return (double)lo + p;
}
