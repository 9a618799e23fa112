// Validation images (utils/visualization.py and models/nerf_system.py:276-307 of the reference, which build them on the CPU
// after a copy of every map): depth maps through a colour table, feature maps through their PCA projection, colour and
// single-channel maps quantised, all to uint8 [H][W][3] where the render already is.  Everything here is memory-bound.  The
// depth and colour products move about 1 MB per image and are launch-bound; the PCA projection reads the whole feature map
// once (269 MB at 350 x 500 x 384) with 16-byte loads, the mean and the three components held in registers.
// Reductions are min / max only (exact in any order) and run in a fixed order anyway: per-workgroup partials in scratch,
// one finishing workgroup, no atomics.  Steps that must match numpy bit for bit keep numpy's roundings (contraction switched
// off where a product feeds a sum); the library is built without fast-math, so `/` is the correctly rounded division.
#include "common.cuh"

#include <float.h>
#include <math.h>

namespace {

#define VIZ_REDUCE_BLOCKS 1024  // most workgroups a min / max pass uses (its partials: 2 floats each)
#define VIZ_MAP_BLOCKS 2048     // most workgroups an element-wise or projection pass uses (grid-stride beyond)
#define PCA_MAX_F 512

__device__ __forceinline__ float nan_to_num(float v) {
  if (v != v) return 0.f;
  return v > FLT_MAX ? FLT_MAX : (v < -FLT_MAX ? -FLT_MAX : v);
}

// min of lo and max of hi over the workgroup, valid in every thread; one call per kernel (the LDS slots are not recycled)
__device__ __forceinline__ void block_minmax(float& lo, float& hi) {
  __shared__ float red[2][NTHREADS / 64];
  const int tid = threadIdx.x;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, d));
    hi = fmaxf(hi, __shfl_xor(hi, d));
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = lo;
    red[1][tid >> 6] = hi;
  }
  __syncthreads();
  lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
  hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
}

// (es, shift) of the pred_depths pre-step, computed once per workgroup: exp in fp64, rounded once
__device__ __forceinline__ void depth_pre(const upnerf_viz_depth_args& a, float& es, float& shift) {
  __shared__ float pre[2];
  es = 1.f;
  shift = 0.f;
  if (a.pre != UPNERF_VIZ_PRED_DEPTH) return;  // (uniform over the grid)
  if (threadIdx.x == 0) {
    pre[0] = (float)exp((double)a.depth_scale[0]);
    pre[1] = a.depth_scale[1];
  }
  __syncthreads();
  es = pre[0];
  shift = pre[1];
}

__device__ __forceinline__ float depth_value(const upnerf_viz_depth_args& a, int64_t p, float es, float shift) {
  float v = a.x[p * a.x_stride];
  if (a.pre == UPNERF_VIZ_PRED_DEPTH) {
    {
#pragma clang fp contract(off)  // two roundings, as torch's mul and add: __fmul_rn / __fadd_rn are plain operators here and fuse
      v = v * es;
      v = v + shift;
    }
    v = v < a.inv_far ? a.inv_far : v;
    v = 1.0f / v;
    v = v < a.near ? a.near : v;
  }
  return v;
}

__global__ __launch_bounds__(NTHREADS) void minmax_part_kernel(upnerf_viz_depth_args a, int64_t n, float* __restrict__ part) {
  float es, shift;
  depth_pre(a, es, shift);
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t p = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * NTHREADS) {
    const float v = nan_to_num(depth_value(a, p, es, shift));
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  block_minmax(lo, hi);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = lo;
    part[2 * blockIdx.x + 1] = hi;
  }
}

__global__ __launch_bounds__(NTHREADS) void minmax_finish_kernel(const float* __restrict__ part, int nb, float* __restrict__ out) {
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < nb; i += NTHREADS) {
    lo = fminf(lo, part[2 * i]);
    hi = fmaxf(hi, part[2 * i + 1]);
  }
  block_minmax(lo, hi);
  if (threadIdx.x == 0) {
    out[0] = lo;
    out[1] = hi;
  }
}

// four pixels of three bytes each (col[j] = c0 | c1 << 8 | c2 << 16) as the three little-endian words they occupy
__device__ __forceinline__ void store_pixels4(uint8_t* rgb, int64_t p0, const uint32_t (&col)[4], int cnt, bool packed) {
  if (cnt == 4 && packed) {
    uint32_t* w = reinterpret_cast<uint32_t*>(rgb + 3 * p0);  // p0 % 4 == 0 and the base is 4-byte aligned
    w[0] = col[0] | (col[1] << 24);
    w[1] = (col[1] >> 8) | (col[2] << 16);
    w[2] = (col[2] >> 16) | (col[3] << 8);
    return;
  }
  for (int j = 0; j < cnt; ++j) {
    uint8_t* o = rgb + 3 * (p0 + j);
    o[0] = (uint8_t)(col[j] & 255u);
    o[1] = (uint8_t)((col[j] >> 8) & 255u);
    o[2] = (uint8_t)(col[j] >> 16);
  }
}

// range: device (mi, ma) or NULL for the by-value pair of the arguments
__global__ __launch_bounds__(NTHREADS) void depth_colour_kernel(upnerf_viz_depth_args a, const float* __restrict__ range, int packed) {
  __shared__ uint32_t lut[256];
  static_assert(NTHREADS == 256, "one table entry per thread");
  {
    const uint8_t* e = a.lut + 3 * threadIdx.x;
    lut[threadIdx.x] = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
  }
  float es, shift;
  depth_pre(a, es, shift);
  __syncthreads();
  const float mi = range ? range[0] : a.mi, ma = range ? range[1] : a.ma;
  const float den = (float)((double)ma - (double)mi + 1e-8);
  const int64_t n = (int64_t)a.H * a.W;
  for (int64_t p0 = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) * 4; p0 < n; p0 += (int64_t)gridDim.x * NTHREADS * 4) {
    const int cnt = n - p0 < 4 ? (int)(n - p0) : 4;
    uint32_t col[4] = {0u, 0u, 0u, 0u}, q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) {
        const float v = depth_value(a, p0 + j, es, shift);
        if (a.value) a.value[p0 + j] = v;
        float t = (nan_to_num(v) - mi) / den;
        t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);  // comparisons: a NaN (inf / inf of an infinite range) stays, and maps to entry 0
        q[j] = t == t ? (uint32_t)(255.0f * t) : 0u;
        col[j] = lut[q[j]];
      }
    }
    if (a.index) {
      if (cnt == 4 && packed) *reinterpret_cast<uint32_t*>(a.index + p0) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
      else
        for (int j = 0; j < cnt; ++j) a.index[p0 + j] = (uint8_t)q[j];
    }
    store_pixels4(a.rgb, p0, col, cnt, packed);
  }
}

// .mul(255).clamp(0, 255).byte(): truncation; a NaN gives 0
__device__ __forceinline__ uint32_t quant(float v) {
  v = 255.0f * v;
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  return v == v ? (uint32_t)v : 0u;
}

// fast: [H*W][3] contiguous and 16-byte aligned, four pixels = three float4
__global__ __launch_bounds__(NTHREADS) void rgb_kernel(upnerf_viz_rgb_args a, int fast, int packed) {
  const int64_t n = (int64_t)a.H * a.W;
  for (int64_t p0 = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) * 4; p0 < n; p0 += (int64_t)gridDim.x * NTHREADS * 4) {
    const int cnt = n - p0 < 4 ? (int)(n - p0) : 4;
    uint32_t col[4] = {0u, 0u, 0u, 0u};
    if (fast && cnt == 4) {
      const float4* s = reinterpret_cast<const float4*>(a.x + 3 * p0);
      const float4 u = s[0], v = s[1], w = s[2];
      col[0] = quant(u.x) | (quant(u.y) << 8) | (quant(u.z) << 16);
      col[1] = quant(u.w) | (quant(v.x) << 8) | (quant(v.y) << 16);
      col[2] = quant(v.z) | (quant(v.w) << 8) | (quant(w.x) << 16);
      col[3] = quant(w.y) | (quant(w.z) << 8) | (quant(w.w) << 16);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
          const float* s = a.x + (p0 + j) * a.stride;
          if (a.C == 1) col[j] = quant(s[0]) * 0x010101u;
          else col[j] = quant(s[0]) | (quant(s[a.cstride]) << 8) | (quant(s[2 * a.cstride]) << 16);
        }
      }
    }
    store_pixels4(a.rgb, p0, col, cnt, packed);
  }
}

// normal map: (n + 1) / 2 through quant(); a zero normal is mid-grey.  Four pixels per thread, as rgb_kernel.
__global__ __launch_bounds__(NTHREADS) void normals_kernel(upnerf_viz_normals_args a, int packed) {
  const int64_t n = (int64_t)a.H * a.W;
  float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (a.rot) {
#pragma unroll
    for (int j = 0; j < 9; ++j) r[j] = a.rot[j];
  }
  for (int64_t p0 = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) * 4; p0 < n; p0 += (int64_t)gridDim.x * NTHREADS * 4) {
    const int cnt = n - p0 < 4 ? (int)(n - p0) : 4;
    uint32_t col[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) {
        const float* s = a.n + 3 * (p0 + j);
        const float x = s[0], y = s[1], z = s[2];
        if (x == 0.f && y == 0.f && z == 0.f) {
          col[j] = 0x808080u;
        } else {
          float c[3] = {x, y, z};
          if (a.rot) {
#pragma clang fp contract(off)  // every product and sum rounded on its own, as numpy evaluates the restatement
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = (r[3 * k] * x + r[3 * k + 1] * y) + r[3 * k + 2] * z;
          }
          col[j] = quant((c[0] + 1.0f) * 0.5f) | (quant((c[1] + 1.0f) * 0.5f) << 8) | (quant((c[2] + 1.0f) * 0.5f) << 16);
        }
      }
    }
    store_pixels4(a.rgb, p0, col, cnt, packed);
  }
}

template <int VEC>
__device__ __forceinline__ void load_chunk(const float* p, float (&o)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
  } else {
    o[0] = *p;
  }
}

// pc[r][j] = sum_k (feat[r][k] - m[k]) * c[j][k]: G lanes per row (G a power of two <= 64, NTHREADS / G rows per workgroup
// and iteration), lane l owns the chunks l, l + G, ... of VEC channels and keeps their m and c in registers for all its rows.
// Per lane the chunks are summed in ascending order, then the lanes of a row by a xor tree: one fixed order.
template <int VEC, int PER>
__global__ __launch_bounds__(NTHREADS) void pca_project_kernel(upnerf_viz_pca_args a, int G, float* __restrict__ part) {
  const int tid = threadIdx.x, lane = tid & (G - 1);
  const int nch = a.F / VEC;
  float mr[PER][VEC], cr[3][PER][VEC];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = lane + i * G;
#pragma unroll
    for (int e = 0; e < VEC; ++e) mr[i][e] = cr[0][i][e] = cr[1][i][e] = cr[2][i][e] = 0.f;
    if (k < nch) {
      load_chunk<VEC>(a.m + k * VEC, mr[i]);
#pragma unroll
      for (int j = 0; j < 3; ++j) load_chunk<VEC>(a.c + (int64_t)j * a.F + k * VEC, cr[j][i]);
    }
  }
  const int64_t n = (int64_t)a.H * a.W;
  const int64_t rows = NTHREADS / G, step = (int64_t)gridDim.x * rows;
  float lo = INFINITY, hi = -INFINITY;
  // the trip count is the same for every lane of the grid: the shuffles below always run with whole waves
  for (int64_t r0 = 0; r0 < n; r0 += step) {
    const int64_t r = r0 + (int64_t)blockIdx.x * rows + tid / G;
    const bool valid = r < n;
    float acc[3] = {0.f, 0.f, 0.f};
    if (valid) {
      const float* row = a.feat + r * a.feat_ld;
      float f[PER][VEC];
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int k = lane + i * G;
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[i][e] = 0.f;
        if (k < nch) load_chunk<VEC>(row + k * VEC, f[i]);
      }
#pragma unroll
      for (int i = 0; i < PER; ++i)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float d = f[i][e] - mr[i][e];  // (absent chunks: 0 - 0, times 0)
          acc[0] = fmaf(d, cr[0][i][e], acc[0]);
          acc[1] = fmaf(d, cr[1][i][e], acc[1]);
          acc[2] = fmaf(d, cr[2][i][e], acc[2]);
        }
    }
    for (int d = G >> 1; d >= 1; d >>= 1) {
      acc[0] += __shfl_xor(acc[0], d);
      acc[1] += __shfl_xor(acc[1], d);
      acc[2] += __shfl_xor(acc[2], d);
    }
    if (valid) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (acc[j] == acc[j]) {  // a NaN component takes no part in the range
          lo = fminf(lo, acc[j]);
          hi = fmaxf(hi, acc[j]);
        }
      if (lane == 0) {
        float* o = a.img + 3 * r;
        o[0] = acc[0], o[1] = acc[1], o[2] = acc[2];
      }
    }
  }
  block_minmax(lo, hi);
  if (tid == 0) {
    part[2 * blockIdx.x] = lo;
    part[2 * blockIdx.x + 1] = hi;
  }
}

__device__ __forceinline__ float pca_norm(float pc, float mn, float den) {
  const float v = (pc - mn) / den;
  return v == v ? v : 0.f;
}

// img = (pc - mn) / (mx - mn) in place, and its uint8 form; `total` = H * W * 3 elements, four per thread
__global__ __launch_bounds__(NTHREADS) void pca_normalise_kernel(upnerf_viz_pca_args a, const float* __restrict__ mm, int packed) {
  const float mn = mm[0], den = mm[1] - mm[0];
  const int64_t total = (int64_t)a.H * a.W * 3;
  for (int64_t i0 = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) * 4; i0 < total; i0 += (int64_t)gridDim.x * NTHREADS * 4) {
    if (packed && i0 + 4 <= total) {
      float4 v = *reinterpret_cast<const float4*>(a.img + i0);
      v.x = pca_norm(v.x, mn, den), v.y = pca_norm(v.y, mn, den), v.z = pca_norm(v.z, mn, den), v.w = pca_norm(v.w, mn, den);
      *reinterpret_cast<float4*>(a.img + i0) = v;
      *reinterpret_cast<uint32_t*>(a.rgb + i0) = quant(v.x) | (quant(v.y) << 8) | (quant(v.z) << 16) | (quant(v.w) << 24);
    } else {
      for (int64_t i = i0; i < total && i < i0 + 4; ++i) {
        const float v = pca_norm(a.img[i], mn, den);
        a.img[i] = v;
        a.rgb[i] = (uint8_t)quant(v);
      }
    }
  }
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
int reduce_blocks(int64_t n) { return (int)(ceil_div(n, NTHREADS) < VIZ_REDUCE_BLOCKS ? ceil_div(n, NTHREADS) : VIZ_REDUCE_BLOCKS); }
int map_blocks(int64_t units) { return (int)(units < 1 ? 1 : (units < VIZ_MAP_BLOCKS ? units : VIZ_MAP_BLOCKS)); }
bool aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

int check_depth(const upnerf_viz_depth_args* a) {
  if (!a || a->H < 1 || a->W < 1) return UPNERF_EINVAL;
  if (a->pre != UPNERF_VIZ_PLAIN && a->pre != UPNERF_VIZ_PRED_DEPTH) return UPNERF_EINVAL;
  if (a->range < UPNERF_VIZ_RANGE_OWN || a->range > UPNERF_VIZ_RANGE_DEVICE) return UPNERF_EINVAL;
  return 0;
}

int check_pca(const upnerf_viz_pca_args* a) {
  if (!a || a->H < 1 || a->W < 1 || a->F < 1 || a->F > PCA_MAX_F) return UPNERF_EINVAL;
  return 0;
}

// lanes per row: the power of two that covers the chunks, at most a wave; halved while that leaves no lane idle and a
// lane's chunks still fit its registers (96 chunks at F = 384: 32 lanes x 3)
int pca_group(int nch, int per) {
  int G = 1;
  while (G < nch && G < 64) G <<= 1;
  while (G > 16 && nch % G != 0 && nch % (G >> 1) == 0 && nch / (G >> 1) <= per) G >>= 1;
  return G;
}

int pca_blocks(const upnerf_viz_pca_args* a, bool vec, int* G) {
  *G = pca_group(vec ? a->F / 4 : a->F, vec ? 3 : 8);
  return map_blocks(ceil_div((int64_t)a->H * a->W, NTHREADS / *G));
}

bool pca_vec(const upnerf_viz_pca_args* a) {
  return a->F % 4 == 0 && a->feat_ld % 4 == 0 && aligned(a->feat, 16) && aligned(a->m, 16) && aligned(a->c, 16);
}

}  // namespace

extern "C" int upnerf_viz_minmax_scratch(long long n) {
  if (n < 1) return UPNERF_EINVAL;
  return 2 * reduce_blocks(n);
}

extern "C" int upnerf_viz_minmax(const float* x, long long n, long long stride, float* out, float* scratch, void* stream) {
  if (!x || !out || !scratch || n < 1) return UPNERF_EINVAL;
  upnerf_viz_depth_args a = {};
  a.x = x;
  a.x_stride = stride;
  a.pre = UPNERF_VIZ_PLAIN;
  const int nb = reduce_blocks(n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(minmax_part_kernel, dim3(nb), dim3(NTHREADS), 0, st, a, (int64_t)n, scratch);
  hipLaunchKernelGGL(minmax_finish_kernel, dim3(1), dim3(NTHREADS), 0, st, (const float*)scratch, nb, out);
  return (int)hipGetLastError();
}

// scratch of upnerf_viz_depth: [0..1] the range, then the partials of its reduction
extern "C" int upnerf_viz_depth_scratch(const upnerf_viz_depth_args* a) {
  int rc = check_depth(a);
  if (rc) return rc;
  return 2 + 2 * reduce_blocks((int64_t)a->H * a->W);
}

extern "C" int upnerf_viz_depth(const upnerf_viz_depth_args* a, float* scratch, void* stream) {
  int rc = check_depth(a);
  if (rc) return rc;
  if (!a->x || !a->lut || !a->rgb) return UPNERF_EINVAL;
  if (a->pre == UPNERF_VIZ_PRED_DEPTH && !a->depth_scale) return UPNERF_EINVAL;
  if (a->range == UPNERF_VIZ_RANGE_OWN && !scratch) return UPNERF_EINVAL;
  if (a->range == UPNERF_VIZ_RANGE_DEVICE && !a->range_dev) return UPNERF_EINVAL;
  const int64_t n = (int64_t)a->H * a->W;
  hipStream_t st = (hipStream_t)stream;
  const float* range = a->range == UPNERF_VIZ_RANGE_DEVICE ? a->range_dev : nullptr;
  if (a->range == UPNERF_VIZ_RANGE_OWN) {
    const int nb = reduce_blocks(n);
    hipLaunchKernelGGL(minmax_part_kernel, dim3(nb), dim3(NTHREADS), 0, st, *a, n, scratch + 2);
    hipLaunchKernelGGL(minmax_finish_kernel, dim3(1), dim3(NTHREADS), 0, st, (const float*)(scratch + 2), nb, scratch);
    range = scratch;
  }
  const int packed = aligned(a->rgb, 4) && (!a->index || aligned(a->index, 4));
  hipLaunchKernelGGL(depth_colour_kernel, dim3(map_blocks(ceil_div(n, 4 * NTHREADS))), dim3(NTHREADS), 0, st, *a, range, packed);
  return (int)hipGetLastError();
}

// scratch of upnerf_viz_pca: [0..1] (mn, mx), then the partials of the projection's workgroups
extern "C" int upnerf_viz_pca_scratch(const upnerf_viz_pca_args* a) {
  int rc = check_pca(a);
  if (rc) return rc;
  return 2 + 2 * VIZ_MAP_BLOCKS;  // (the grid depends on the alignment of pointers a size query need not carry)
}

extern "C" int upnerf_viz_pca(const upnerf_viz_pca_args* a, float* scratch, void* stream) {
  int rc = check_pca(a);
  if (rc) return rc;
  if (!a->feat || !a->m || !a->c || !a->img || !a->rgb || !scratch || a->feat_ld < a->F) return UPNERF_EINVAL;
  const bool vec = pca_vec(a);
  int G;
  const int nb = pca_blocks(a, vec, &G);
  const int nch = vec ? a->F / 4 : a->F;
  if ((nch + G - 1) / G > (vec ? 3 : 8)) return UPNERF_EUNSUP;
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL((pca_project_kernel<4, 3>), dim3(nb), dim3(NTHREADS), 0, st, *a, G, scratch + 2);
  else hipLaunchKernelGGL((pca_project_kernel<1, 8>), dim3(nb), dim3(NTHREADS), 0, st, *a, G, scratch + 2);
  hipLaunchKernelGGL(minmax_finish_kernel, dim3(1), dim3(NTHREADS), 0, st, (const float*)(scratch + 2), nb, scratch);
  const int64_t total = (int64_t)a->H * a->W * 3;
  const int packed = aligned(a->img, 16) && aligned(a->rgb, 4);
  hipLaunchKernelGGL(pca_normalise_kernel, dim3(map_blocks(ceil_div(total, 4 * NTHREADS))), dim3(NTHREADS), 0, st, *a,
                     (const float*)scratch, packed);
  return (int)hipGetLastError();
}

extern "C" int upnerf_viz_rgb(const upnerf_viz_rgb_args* a, void* stream) {
  if (!a || a->H < 1 || a->W < 1 || (a->C != 1 && a->C != 3) || !a->x || !a->rgb) return UPNERF_EINVAL;
  const int64_t n = (int64_t)a->H * a->W;
  const int fast = a->C == 3 && a->stride == 3 && a->cstride == 1 && aligned(a->x, 16);
  const int packed = aligned(a->rgb, 4);
  hipLaunchKernelGGL(rgb_kernel, dim3(map_blocks(ceil_div(n, 4 * NTHREADS))), dim3(NTHREADS), 0, (hipStream_t)stream, *a, fast,
                     packed);
  return (int)hipGetLastError();
}

extern "C" int upnerf_viz_normals(const upnerf_viz_normals_args* a, void* stream) {
  if (!a || a->H < 1 || a->W < 1 || !a->n || !a->rgb) return UPNERF_EINVAL;
  const int64_t n = (int64_t)a->H * a->W;
  hipLaunchKernelGGL(normals_kernel, dim3(map_blocks(ceil_div(n, 4 * NTHREADS))), dim3(NTHREADS), 0, (hipStream_t)stream, *a,
                     (int)aligned(a->rgb, 4));
  return (int)hipGetLastError();
}
