// Exclusive scan of a device array in workgroup blocks, shared by the kernels that compact (mesh.hip: crossed edges and triangles
// of the grid points; occupancy.hip: the rays that hit something).  No atomics: the same bits every run.
#pragma once
#include "common.cuh"

namespace {

// ---- exclusive scan: SCAN_BLOCK elements per workgroup, block sums scanned by the same kernels one level up ---------------

#define SCAN_ITEMS 4
#define SCAN_BLOCK (NTHREADS * SCAN_ITEMS)

// POP: the elements are the bit counts of the bytes (crossed edges of a point) instead of the bytes themselves
template <typename T, bool POP>
__global__ __launch_bounds__(NTHREADS) void scan_block_kernel(const T* in, int64_t n, int32_t* out, int32_t* sums) {
  __shared__ int32_t sh[2][NTHREADS];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)tid * SCAN_ITEMS;
  int32_t v[SCAN_ITEMS];
  int32_t total = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) {
    int32_t x = 0;
    if (base + i < n) x = POP ? __popc((unsigned)in[base + i]) : (int32_t)in[base + i];
    v[i] = total;  // exclusive within the thread
    total += x;
  }
  int cur = 0;
  sh[0][tid] = total;
  __syncthreads();
  for (int step = 1; step < NTHREADS; step <<= 1) {  // Hillis-Steele over the thread totals (inclusive)
    const int32_t x = sh[cur][tid] + (tid >= step ? sh[cur][tid - step] : 0);
    sh[cur ^ 1][tid] = x;
    cur ^= 1;
    __syncthreads();
  }
  const int32_t before = sh[cur][tid] - total;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i)
    if (base + i < n) out[base + i] = before + v[i];
  if (tid == NTHREADS - 1) sums[blockIdx.x] = sh[cur][tid];
}

__global__ __launch_bounds__(NTHREADS) void scan_add_kernel(int32_t* out, int64_t n, const int32_t* offsets) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i < n) out[i] += offsets[i / SCAN_BLOCK];
}

__global__ void scan_total_kernel(const int32_t* top, int32_t* total) { total[0] = top[0]; }

int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ints of block sums over all levels of a scan of n elements (level k holds the sums of level k - 1's blocks; the last has one)
int64_t scan_level_ints(int64_t n) {
  int64_t total = 0;
  do {
    n = ceil_div64(n, SCAN_BLOCK);
    total += n;
  } while (n > 1);
  return total;
}

// out[i] = sum of the elements before i; *total = the sum of all.  `levels` holds scan_level_ints(n) ints.
template <typename T, bool POP>
void scan_exclusive(const T* in, int64_t n, int32_t* out, int32_t* levels, int32_t* total, hipStream_t st) {
  const int64_t nb = ceil_div64(n, SCAN_BLOCK);
  hipLaunchKernelGGL((scan_block_kernel<T, POP>), dim3((unsigned)nb), dim3(NTHREADS), 0, st, in, n, out, levels);
  if (nb > 1) {  // the block sums become block offsets, in place, and their own total is the total
    scan_exclusive<int32_t, false>(levels, nb, levels, levels + nb, total, st);
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)ceil_div64(n, NTHREADS)), dim3(NTHREADS), 0, st, out, n,
                       (const int32_t*)levels);
  } else {
    hipLaunchKernelGGL(scan_total_kernel, dim3(1), dim3(1), 0, st, (const int32_t*)levels, total);
  }
}

}  // namespace
