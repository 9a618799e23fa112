// Scene loading on the device: the per-pixel buffers the reference builds as CPU tensors for every training image
// (datasets/phototourism.py:242-323: directions, ray infos, pixel coordinates, colours; about 30 M rays per scene) and
// the cv2.resize + normalisation of the DINO / DPT maps (lines 286, 315-321, 371-399).  Both are bandwidth kernels: one
// launch over a table of images / maps, plain coalesced loads and stores, no LDS staging.
//
// Exactness: the ray buffers are the CPU tensors' bits (integer pixel grid, correctly rounded fp32 divisions -- the
// library is built without fast-math); the resize is OpenCV's INTER_LINEAR arithmetic in fp32 (a horizontal then a
// vertical blend), equal to it up to the order of the two products in a blend.
#include "common.cuh"

namespace {

// ---- ray buffers ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NTHREADS) void scene_rays_kernel(upnerf_scene_rays_args a,
                                                             const upnerf_scene_image* __restrict__ tab) {
  const upnerf_scene_image d = tab[blockIdx.y];
  const int ww = d.x1 - d.x0;
  const int64_t n = (int64_t)ww * d.H;
  const int64_t r = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (r >= n) return;
  const int j = (int)(r / ww);
  const int i = d.x0 + (int)(r - (int64_t)j * ww);
  const float fi = (float)i, fj = (float)j;  // exact: the linspace(0, n-1, n) grid is the integers
  const int64_t o = d.row0 + r;
  float* dir = a.directions + o * 3;
  dir[0] = (fi - d.cx) / d.fx;
  dir[1] = -(fj - d.cy) / d.fy;
  dir[2] = -1.f;
  if (a.ray_infos) {
    float* q = a.ray_infos + o * 3;
    q[0] = d.near;
    q[1] = d.far;
    q[2] = d.img_idx;
  }
  if (a.pxl) {
    float* q = a.pxl + o * 2;
    q[0] = fj / (float)(d.H - 1);
    q[1] = fi / (float)(d.W - 1);
  }
  if (a.rgbs) {
    const uint8_t* p = a.pixels + d.pix_off + ((int64_t)j * d.W + i) * 3;
    float* q = a.rgbs + o * 3;
    q[0] = (float)p[0] / 255.f;
    q[1] = (float)p[1] / 255.f;
    q[2] = (float)p[2] / 255.f;
  }
}

// ---- resize ---------------------------------------------------------------------------------------------------------

#define RESIZE_MAX_CHUNKS 8  // chunks of VEC channels per thread (C <= 512)

// OpenCV's INTER_LINEAR source index and weight for destination index d (resize.cpp, the float-coefficient path):
// half-pixel centres, fx rounded to float, clamped to the edge with a zero weight.
__device__ __forceinline__ void lin_coef(int d, int n_src, int n_dst, int& s0, int& s1, float& f) {
  const double scale = 1.0 / ((double)n_dst / (double)n_src);
  float fx = (float)((d + 0.5) * scale - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) {
    sx = 0;
    fx = 0.f;
  }
  if (sx >= n_src - 1) {
    sx = n_src - 1;
    fx = 0.f;
  }
  s0 = sx;
  s1 = sx + 1 < n_src ? sx + 1 : n_src - 1;
  f = fx;
}

template <int VEC>
struct Vec;
template <>
struct Vec<4> {
  typedef f32x4 T;
  static __device__ __forceinline__ T load(const float* p) { return *(const f32x4*)p; }
  static __device__ __forceinline__ void store(float* p, T v) { *(f32x4*)p = v; }
  static __device__ __forceinline__ float sq(T v) { return v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }
  static __device__ __forceinline__ T splat(float s) { return f32x4{s, s, s, s}; }
};
template <>
struct Vec<1> {
  typedef float T;
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
  static __device__ __forceinline__ float sq(T v) { return v * v; }
  static __device__ __forceinline__ T splat(float s) { return s; }
};

__device__ __forceinline__ float group_sum(float v, int G) {
  for (int d = G >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// the depth pre-step of one value: clamp below at 0 (a NaN stays NaN, as the reference's boolean mask leaves it), then
// the affine map with the map's maximum
__device__ __forceinline__ float invdepth(float x, float mx, float scale, float bias) {
  const float v = x < 0.f ? 0.f : x;
  return v / mx * scale + bias;
}

// one destination pixel per group of G lanes; the lanes of a group walk its channels in chunks of VEC floats
// (16-byte loads and stores for VEC = 4), chunk k = lane + t * G.  src and dst may be one buffer (identity maps only).
template <int VEC>
__global__ __launch_bounds__(NTHREADS) void resize_kernel(upnerf_resize_args a, const upnerf_resize_map* __restrict__ tab,
                                                          const float* __restrict__ maxima, int G) {
  typedef typename Vec<VEC>::T V;
  const upnerf_resize_map m = tab[blockIdx.y];
  const int per_block = NTHREADS / G;
  const int64_t p = (int64_t)blockIdx.x * per_block + threadIdx.x / G;
  const int lane = threadIdx.x % G;
  if (p >= (int64_t)m.H * m.W) return;  // whole groups leave together: the shuffles below stay inside a group
  const int dy = (int)(p / m.W), dx = (int)(p - (int64_t)dy * m.W);
  const int C = a.C, nch = C / VEC;
  const float* src = a.src + m.src_off;
  float* dst = a.dst + m.dst_off + p * C;
  const float mx = a.pre == UPNERF_RESIZE_INVDEPTH ? maxima[blockIdx.y] : 1.f;

  if (m.h == m.H && m.w == m.W) {  // same size: cv2.resize copies; only the pre-step applies
    const float* s = src + p * C;
    float n = 1.f;
    if (a.pre == UPNERF_RESIZE_L2) {
      float acc = 0.f;
      for (int k = lane; k < nch; k += G) acc += Vec<VEC>::sq(Vec<VEC>::load(s + k * VEC));
      n = sqrtf(group_sum(acc, G));
    }
    for (int k = lane; k < nch; k += G) {
      V v = Vec<VEC>::load(s + k * VEC);
      if (a.pre == UPNERF_RESIZE_L2) v = v / Vec<VEC>::splat(n);
      else if (a.pre == UPNERF_RESIZE_INVDEPTH) {
        if constexpr (VEC == 1) v = invdepth(v, mx, m.scale, m.bias);
        else {
          v.x = invdepth(v.x, mx, m.scale, m.bias);
          v.y = invdepth(v.y, mx, m.scale, m.bias);
          v.z = invdepth(v.z, mx, m.scale, m.bias);
          v.w = invdepth(v.w, mx, m.scale, m.bias);
        }
      }
      Vec<VEC>::store(dst + k * VEC, v);
    }
    return;
  }

  int x0, x1, y0, y1;
  float fx, fy;
  lin_coef(dx, m.w, m.W, x0, x1, fx);
  lin_coef(dy, m.h, m.H, y0, y1, fy);
  const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
  const float* s00 = src + ((int64_t)y0 * m.w + x0) * C;
  const float* s01 = src + ((int64_t)y0 * m.w + x1) * C;
  const float* s10 = src + ((int64_t)y1 * m.w + x0) * C;
  const float* s11 = src + ((int64_t)y1 * m.w + x1) * C;
  float n00 = 1.f, n01 = 1.f, n10 = 1.f, n11 = 1.f;
  if (a.pre == UPNERF_RESIZE_L2) {  // the norms of the four source pixels (their channels are read again below, from cache)
    float q00 = 0.f, q01 = 0.f, q10 = 0.f, q11 = 0.f;
    for (int k = lane; k < nch; k += G) {
      q00 += Vec<VEC>::sq(Vec<VEC>::load(s00 + k * VEC));
      q01 += Vec<VEC>::sq(Vec<VEC>::load(s01 + k * VEC));
      q10 += Vec<VEC>::sq(Vec<VEC>::load(s10 + k * VEC));
      q11 += Vec<VEC>::sq(Vec<VEC>::load(s11 + k * VEC));
    }
    n00 = sqrtf(group_sum(q00, G));
    n01 = sqrtf(group_sum(q01, G));
    n10 = sqrtf(group_sum(q10, G));
    n11 = sqrtf(group_sum(q11, G));
  }
  for (int k = lane; k < nch; k += G) {
    V v00 = Vec<VEC>::load(s00 + k * VEC), v01 = Vec<VEC>::load(s01 + k * VEC);
    V v10 = Vec<VEC>::load(s10 + k * VEC), v11 = Vec<VEC>::load(s11 + k * VEC);
    if (a.pre == UPNERF_RESIZE_L2) {
      v00 = v00 / Vec<VEC>::splat(n00);
      v01 = v01 / Vec<VEC>::splat(n01);
      v10 = v10 / Vec<VEC>::splat(n10);
      v11 = v11 / Vec<VEC>::splat(n11);
    } else if (a.pre == UPNERF_RESIZE_INVDEPTH) {
      if constexpr (VEC == 1) {
        v00 = invdepth(v00, mx, m.scale, m.bias);
        v01 = invdepth(v01, mx, m.scale, m.bias);
        v10 = invdepth(v10, mx, m.scale, m.bias);
        v11 = invdepth(v11, mx, m.scale, m.bias);
      } else {
#define UPNERF_INVD4(v)                        \
  v.x = invdepth(v.x, mx, m.scale, m.bias);    \
  v.y = invdepth(v.y, mx, m.scale, m.bias);    \
  v.z = invdepth(v.z, mx, m.scale, m.bias);    \
  v.w = invdepth(v.w, mx, m.scale, m.bias);
        UPNERF_INVD4(v00) UPNERF_INVD4(v01) UPNERF_INVD4(v10) UPNERF_INVD4(v11)
#undef UPNERF_INVD4
      }
    }
    const V h0 = v00 * Vec<VEC>::splat(a0) + v01 * Vec<VEC>::splat(a1);
    const V h1 = v10 * Vec<VEC>::splat(a0) + v11 * Vec<VEC>::splat(a1);
    Vec<VEC>::store(dst + k * VEC, h0 * Vec<VEC>::splat(b0) + h1 * Vec<VEC>::splat(b1));
  }
}

// maxima[m] = max over map m of its source values clamped below at 0 (one workgroup per map; fmaxf passes a NaN over)
__global__ __launch_bounds__(NTHREADS) void map_max_kernel(upnerf_resize_args a, const upnerf_resize_map* __restrict__ tab,
                                                           float* __restrict__ maxima) {
  __shared__ float red[NTHREADS / 64];
  const upnerf_resize_map m = tab[blockIdx.x];
  const int64_t n = (int64_t)m.h * m.w * a.C;
  const float* s = a.src + m.src_off;
  float v = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += NTHREADS) v = fmaxf(v, s[i]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) maxima[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

int64_t table_bytes(int n_maps) { return ((int64_t)n_maps * sizeof(upnerf_resize_map) + 15) & ~(int64_t)15; }

int group_size(int nch) {
  int G = 1;
  while (G < nch && G < 64) G <<= 1;
  while (G > 16 && nch % G != 0 && nch % (G >> 1) == 0) G >>= 1;  // 96 chunks (C = 384): 32 lanes x 3, none idle
  return G;
}

}  // namespace

extern "C" int upnerf_scene_rays(const upnerf_scene_rays_args* a, const upnerf_scene_image* images, void* table,
                                 void* stream) {
  if (!a || !images || !table || !a->directions || a->n_images < 1 || a->n_images > 65535 || a->rows < 0)
    return UPNERF_EINVAL;
  if (a->rgbs && (!a->pixels || a->pix_bytes <= 0)) return UPNERF_EINVAL;
  int64_t max_blocks = 0;
  for (int b = 0; b < a->n_images; ++b) {
    const upnerf_scene_image& d = images[b];
    if (d.W < 2 || d.H < 2 || d.x0 < 0 || d.x1 <= d.x0 || d.x1 > d.W || d.row0 < 0) return UPNERF_EINVAL;
    const int64_t n = (int64_t)(d.x1 - d.x0) * d.H;
    if (d.row0 + n > a->rows) return UPNERF_EINVAL;
    if (a->rgbs && (d.pix_off < 0 || d.pix_off + (int64_t)d.W * d.H * 3 > a->pix_bytes)) return UPNERF_EINVAL;
    const int64_t blocks = (n + NTHREADS - 1) / NTHREADS;
    max_blocks = blocks > max_blocks ? blocks : max_blocks;
  }
  if (max_blocks > 0x7fffffffLL) return UPNERF_EUNSUP;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(table, images, sizeof(upnerf_scene_image) * (size_t)a->n_images, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(scene_rays_kernel, dim3((unsigned)max_blocks, (unsigned)a->n_images), dim3(NTHREADS), 0, st, *a,
                     (const upnerf_scene_image*)table);
  return (int)hipGetLastError();
}

extern "C" int upnerf_resize_scratch(const upnerf_resize_args* a) {
  if (!a || a->n_maps < 1 || a->n_maps > 65535) return UPNERF_EINVAL;
  return (int)(table_bytes(a->n_maps) + 4 * (int64_t)a->n_maps);
}

extern "C" int upnerf_resize_linear(const upnerf_resize_args* a, const upnerf_resize_map* maps, void* scratch, void* stream) {
  if (!a || !maps || !scratch || !a->src || !a->dst || a->n_maps < 1 || a->n_maps > 65535) return UPNERF_EINVAL;
  if (a->C < 1 || a->C > 512 || a->pre < UPNERF_RESIZE_PLAIN || a->pre > UPNERF_RESIZE_INVDEPTH) return UPNERF_EINVAL;
  if ((uintptr_t)scratch & 15) return UPNERF_EINVAL;
  const bool inplace = (const void*)a->src == (const void*)a->dst;
  const bool vec = a->C % 4 == 0 && ((uintptr_t)a->src & 15) == 0 && ((uintptr_t)a->dst & 15) == 0;
  int64_t max_pix = 0;
  for (int b = 0; b < a->n_maps; ++b) {
    const upnerf_resize_map& m = maps[b];
    if (m.h < 1 || m.w < 1 || m.H < 1 || m.W < 1 || m.src_off < 0 || m.dst_off < 0) return UPNERF_EINVAL;
    if (m.src_off + (int64_t)m.h * m.w * a->C > a->src_elems) return UPNERF_EINVAL;
    if (m.dst_off + (int64_t)m.H * m.W * a->C > a->dst_elems) return UPNERF_EINVAL;
    if (inplace && (m.h != m.H || m.w != m.W || m.src_off != m.dst_off)) return UPNERF_EINVAL;
    if (vec && ((m.src_off | m.dst_off) & 3)) return UPNERF_EINVAL;  // C % 4 == 0 keeps every pixel 16-byte aligned
    const int64_t pix = (int64_t)m.H * m.W;
    max_pix = pix > max_pix ? pix : max_pix;
  }
  if (!inplace) {  // any overlap of the two buffers other than exact aliasing is refused
    const char *s0 = (const char*)a->src, *s1 = s0 + 4 * a->src_elems, *d0 = (const char*)a->dst, *d1 = d0 + 4 * a->dst_elems;
    if (s0 < d1 && d0 < s1) return UPNERF_EINVAL;
  }
  const int VEC = vec ? 4 : 1;
  const int nch = a->C / VEC;
  const int G = group_size(nch);
  if ((nch + G - 1) / G > RESIZE_MAX_CHUNKS) return UPNERF_EUNSUP;
  const int64_t blocks = (max_pix + NTHREADS / G - 1) / (NTHREADS / G);
  if (blocks > 0x7fffffffLL) return UPNERF_EUNSUP;
  hipStream_t st = (hipStream_t)stream;
  upnerf_resize_map* tab = (upnerf_resize_map*)scratch;
  float* maxima = (float*)((char*)scratch + table_bytes(a->n_maps));
  hipError_t e = hipMemcpyAsync(tab, maps, sizeof(upnerf_resize_map) * (size_t)a->n_maps, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  if (a->pre == UPNERF_RESIZE_INVDEPTH)
    hipLaunchKernelGGL(map_max_kernel, dim3(a->n_maps), dim3(NTHREADS), 0, st, *a, (const upnerf_resize_map*)tab, maxima);
  const dim3 grid((unsigned)blocks, (unsigned)a->n_maps);
  if (vec)
    hipLaunchKernelGGL(resize_kernel<4>, grid, dim3(NTHREADS), 0, st, *a, (const upnerf_resize_map*)tab,
                       (const float*)maxima, G);
  else
    hipLaunchKernelGGL(resize_kernel<1>, grid, dim3(NTHREADS), 0, st, *a, (const upnerf_resize_map*)tab,
                       (const float*)maxima, G);
  return (int)hipGetLastError();
}
