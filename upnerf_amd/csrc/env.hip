// The environment of a baked scene (include/upnerf_hip.h: "what lies outside the box"): a cube map of the colour the
// field shows from the box outwards, composited behind the march with the transmittance that is left.  Four small kernels, one
// thread per item, no LDS, no atomics, plain vector stores, every output address written by one thread: the same bits every run.
//
//   env_lookup           the face, cell, blend and slopes of a direction: ONE __host__ __device__ function, used by the composite
//                        and by its backward, and run without a device by tests/host/env_host.hip
//   upnerf_env_rays      the ray rows that make render_static bake the nodes
//   upnerf_env_seam      the copies of a shared node made byte-identical (the lowest face owns)
//   upnerf_env_composite / _bwd
#include "../../include/upnerf_hip.h"

#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int ENV_THREADS = 256;

__host__ __device__ __forceinline__ float env_lerp(float f, float p, float q) { return fmaf(f, q - p, p); }

// fabsf(x) is finite: false for +-inf and for NaN
__host__ __device__ __forceinline__ bool env_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }

// where a direction falls: face, the axes, the cell and the position in it.  ok = false: a dead direction.
struct EnvCell {
  bool ok;
  int m, a, b, face, iu, iv;
  float dm, am, u, v, fu, fv;
};

__host__ __device__ __forceinline__ void env_axis(float u, int E, float half, int* i, float* f) {
  const float g = (u + 1.0f) * half;
  int c = (int)floorf(g);
  c = c < E - 1 ? c : E - 1;
  *i = c;
  *f = g - (float)c;
}

__host__ __device__ __forceinline__ EnvCell env_cell(const float* d, int E) {
  EnvCell c;
  c.ok = env_finite(d[0]) && env_finite(d[1]) && env_finite(d[2]) && (d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f);
  c.m = 0;
  if (fabsf(d[1]) > fabsf(d[c.m])) c.m = 1;
  if (fabsf(d[2]) > fabsf(d[c.m])) c.m = 2;
  c.a = c.m == 0 ? 1 : 0;
  c.b = c.m == 2 ? 1 : 2;
  c.dm = d[c.m];
  c.am = fabsf(c.dm);
  c.face = 2 * c.m + (c.dm < 0.0f ? 1 : 0);
  c.u = c.v = c.fu = c.fv = 0.0f;
  c.iu = c.iv = 0;
  if (c.ok) {
    c.u = d[c.a] / c.am;
    c.v = d[c.b] / c.am;
    const float half = 0.5f * (float)E;
    env_axis(c.u, E, half, &c.iu, &c.fu);
    env_axis(c.v, E, half, &c.iv, &c.fv);
  }
  return c;
}

struct EnvSample {
  EnvCell c;
  float rgb[3];   // env(d)
  float su[3];    // d env / d g_u, face and cell held fixed
  float sv[3];    // d env / d g_v
};

// the lookup, stated once (include/upnerf_hip.h): host and device
__host__ __device__ __forceinline__ EnvSample env_lookup(const float* env, int E, const float* d) {
  EnvSample s;
  s.c = env_cell(d, E);
  for (int k = 0; k < 3; ++k) s.rgb[k] = s.su[k] = s.sv[k] = 0.0f;
  if (!s.c.ok) return s;
  const int64_t N = (int64_t)E + 1;
  const float4* nodes = reinterpret_cast<const float4*>(env);
  const int64_t at = ((int64_t)s.c.face * N + s.c.iv) * N + s.c.iu;
  const float4 q00 = nodes[at], q10 = nodes[at + 1], q01 = nodes[at + N], q11 = nodes[at + N + 1];
  const float n00[3] = {q00.x, q00.y, q00.z}, n10[3] = {q10.x, q10.y, q10.z};
  const float n01[3] = {q01.x, q01.y, q01.z}, n11[3] = {q11.x, q11.y, q11.z};
  for (int k = 0; k < 3; ++k) {
    const float x0 = env_lerp(s.c.fu, n00[k], n10[k]), x1 = env_lerp(s.c.fu, n01[k], n11[k]);
    s.rgb[k] = env_lerp(s.c.fv, x0, x1);
    s.su[k] = env_lerp(s.c.fv, n10[k] - n00[k], n11[k] - n01[k]);
    s.sv[k] = x1 - x0;
  }
  return s;
}

// rgb_out of one ray
__host__ __device__ __forceinline__ void env_composite_row(const float* env, int E, const float* row, float opacity, const float* in,
                                                           float* out) {
  const EnvSample s = env_lookup(env, E, row + 3);
  const float rest = 1.0f - opacity;
  for (int k = 0; k < 3; ++k) out[k] = fmaf(rest, s.rgb[k], in[k]);
}

// g_opacity and the row of g_rays of one ray
__host__ __device__ __forceinline__ void env_composite_grad(const float* env, int E, const float* row, float opacity, const float* g,
                                                            float* g_opacity, float* g_row) {
  const EnvSample s = env_lookup(env, E, row + 3);
  for (int k = 0; k < 8; ++k) g_row[k] = 0.0f;
  *g_opacity = 0.0f;
  if (!s.c.ok) return;
  *g_opacity = -fmaf(g[2], s.rgb[2], fmaf(g[1], s.rgb[1], g[0] * s.rgb[0]));
  const float rest = 1.0f - opacity;
  float Gu = 0.0f, Gv = 0.0f;
  for (int k = 0; k < 3; ++k) {
    const float a = rest * g[k];
    Gu = fmaf(a, s.su[k], Gu);
    Gv = fmaf(a, s.sv[k], Gv);
  }
  const float half = 0.5f * (float)E;
  const float pu = Gu * half, pv = Gv * half;
  g_row[3 + s.c.a] = pu / s.c.am;
  g_row[3 + s.c.b] = pv / s.c.am;
  g_row[3 + s.c.m] = -fmaf(s.c.u, pu, s.c.v * pv) / s.c.dm;
}

// the direction of node (face, iu, iv): d_m = +-1, the other two one division of exact integers each
__host__ __device__ __forceinline__ void env_node_dir(int E, int face, int iu, int iv, float* x) {
  const int m = face >> 1, a = m == 0 ? 1 : 0, b = m == 2 ? 1 : 2;
  x[m] = (face & 1) ? -1.0f : 1.0f;
  x[a] = (float)(2 * iu - E) / (float)E;
  x[b] = (float)(2 * iv - E) / (float)E;
}

// the ray row of node n
__host__ __device__ __forceinline__ void env_ray_row(int E, int64_t n, const float* lo, const float* hi, float far, float* row) {
  const int64_t N = (int64_t)E + 1;
  const int face = (int)(n / (N * N)), iv = (int)(n / N % N), iu = (int)(n % N);
  float x[3];
  env_node_dir(E, face, iu, iv, x);
  // fp64, the products exact, the sum in the order of the axes: the copies of a shared node get the same bits
  const double len = sqrt(((double)x[0] * (double)x[0] + (double)x[1] * (double)x[1]) + (double)x[2] * (double)x[2]);
  float near = INFINITY;
  for (int k = 0; k < 3; ++k) {
    const float o = (float)(((double)lo[k] + (double)hi[k]) / 2.0);
    const float d = (float)((double)x[k] / len);
    row[k] = o;
    row[3 + k] = d;
    if (d != 0.0f) near = fminf(near, ((d > 0.0f ? hi[k] : lo[k]) - o) / d);
  }
  row[6] = near;
  row[7] = far;
}

// Edge node e of face f (e in [0, 4 E): the border of the (E+1) x (E+1) square, each node once) -> (iu, iv)
__host__ __device__ __forceinline__ void env_edge_node(int E, int e, int* iu, int* iv) {
  const int side = e / E, k = e % E;
  if (side == 0) *iu = k, *iv = 0;           // bottom row, left to right, without its last node
  else if (side == 1) *iu = E, *iv = k;      // right column upwards
  else if (side == 2) *iu = E - k, *iv = E;  // top row, right to left
  else *iu = 0, *iv = E - k;                 // left column downwards
}

// The node of face g with the direction x (a node direction with |x_mg| == 1), or -1 if x is not on face g.  The inverse of
// env_node_dir: x_a = (2 iu - E) / E is rounded from an exact ratio, and (x_a + 1) * (E / 2) rounds back to within 1e-3 of iu
// for E <= UPNERF_ENV_MAX_E, so the nearest integer is iu; the caller checks the node's direction bit for bit.
__host__ __device__ __forceinline__ int64_t env_node_on_face(int E, int g, const float* x) {
  const int m = g >> 1, a = m == 0 ? 1 : 0, b = m == 2 ? 1 : 2;
  if (x[m] != ((g & 1) ? -1.0f : 1.0f)) return -1;
  const float half = 0.5f * (float)E;
  const int iu = (int)floorf((x[a] + 1.0f) * half + 0.5f), iv = (int)floorf((x[b] + 1.0f) * half + 0.5f);
  if (iu < 0 || iu > E || iv < 0 || iv > E) return -1;
  float y[3];
  env_node_dir(E, g, iu, iv, y);
  if (y[0] != x[0] || y[1] != x[1] || y[2] != x[2]) return -1;
  const int64_t N = (int64_t)E + 1;
  return ((int64_t)g * N + iv) * N + iu;
}

// the owner of node (face, iu, iv): the copy on the lowest face (itself, if it has no lower copy)
__host__ __device__ __forceinline__ int64_t env_owner(int E, int face, int iu, int iv) {
  float x[3];
  env_node_dir(E, face, iu, iv, x);
  for (int g = 0; g < face; ++g) {
    const int64_t at = env_node_on_face(E, g, x);
    if (at >= 0) return at;
  }
  const int64_t N = (int64_t)E + 1;
  return ((int64_t)face * N + iv) * N + iu;
}

__global__ __launch_bounds__(ENV_THREADS) void env_rays_kernel(upnerf_env_rays_args a) {
  const int r = blockIdx.x * ENV_THREADS + threadIdx.x;
  if (r >= a.count) return;
  float row[8];
  env_ray_row(a.E, a.n0 + r, a.lo, a.hi, a.far, row);
  float4* out = reinterpret_cast<float4*>(a.rays) + (int64_t)r * 2;
  out[0] = make_float4(row[0], row[1], row[2], row[3]);
  out[1] = make_float4(row[4], row[5], row[6], row[7]);
}

__global__ __launch_bounds__(ENV_THREADS) void env_seam_kernel(upnerf_env_seam_args a) {
  const int t = blockIdx.x * ENV_THREADS + threadIdx.x;
  if (t >= 24 * a.E) return;
  const int face = t / (4 * a.E);
  int iu, iv;
  env_edge_node(a.E, t % (4 * a.E), &iu, &iv);
  const int64_t N = (int64_t)a.E + 1, self = ((int64_t)face * N + iv) * N + iu;
  const int64_t owner = env_owner(a.E, face, iu, iv);
  if (owner == self) return;  // an owner is never written: what the other copies read does not change during the launch
  float4* nodes = reinterpret_cast<float4*>(a.env);
  nodes[self] = nodes[owner];
}

__global__ __launch_bounds__(ENV_THREADS) void env_composite_kernel(upnerf_env_composite_args a) {
  const int r = blockIdx.x * ENV_THREADS + threadIdx.x;
  if (r >= a.R) return;
  const float4* rr = reinterpret_cast<const float4*>(a.rays) + (int64_t)r * 2;
  const float4 r0 = rr[0], r1 = rr[1];
  const float row[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
  const float* src = a.rgb_in + (int64_t)r * 3;
  const float in[3] = {src[0], src[1], src[2]};
  float out[3];
  env_composite_row(a.env, a.E, row, a.opacity[r], in, out);
  float* dst = a.rgb_out + (int64_t)r * 3;
  dst[0] = out[0], dst[1] = out[1], dst[2] = out[2];
}

__global__ __launch_bounds__(ENV_THREADS) void env_composite_bwd_kernel(upnerf_env_composite_bwd_args a) {
  const int r = blockIdx.x * ENV_THREADS + threadIdx.x;
  if (r >= a.R) return;
  const float4* rr = reinterpret_cast<const float4*>(a.rays) + (int64_t)r * 2;
  const float4 r0 = rr[0], r1 = rr[1];
  const float row[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
  const float* src = a.g_out + (int64_t)r * 3;
  const float g[3] = {src[0], src[1], src[2]};
  float go, gr[8];
  env_composite_grad(a.env, a.E, row, a.opacity[r], g, &go, gr);
  a.g_opacity[r] = go;
  float4* out = reinterpret_cast<float4*>(a.g_rays) + (int64_t)r * 2;
  out[0] = make_float4(gr[0], gr[1], gr[2], gr[3]);
  out[1] = make_float4(gr[4], gr[5], gr[6], gr[7]);
}

bool env_aligned(const void* p, size_t to) { return p != nullptr && ((uintptr_t)p & (to - 1)) == 0; }
bool env_size_ok(int E) { return E >= 1 && E <= UPNERF_ENV_MAX_E; }
unsigned env_blocks(int64_t n) { return (unsigned)((n + ENV_THREADS - 1) / ENV_THREADS); }

}  // namespace

extern "C" int upnerf_env_rays(const upnerf_env_rays_args* a, void* stream) {
  if (!a || !env_size_ok(a->E) || !env_aligned(a->rays, 16)) return UPNERF_EINVAL;
  const int64_t nodes = 6 * ((int64_t)a->E + 1) * ((int64_t)a->E + 1);
  if (a->n0 < 0 || a->count < 1 || a->n0 > nodes - a->count) return UPNERF_EINVAL;
  for (int k = 0; k < 3; ++k)
    if (!isfinite(a->lo[k]) || !isfinite(a->hi[k]) || !(a->hi[k] > a->lo[k])) return UPNERF_EINVAL;
  if (!isfinite(a->far) || !(a->far > 0.0f)) return UPNERF_EINVAL;
  hipLaunchKernelGGL(env_rays_kernel, dim3(env_blocks(a->count)), dim3(ENV_THREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_env_seam(const upnerf_env_seam_args* a, void* stream) {
  if (!a || !env_size_ok(a->E) || !env_aligned(a->env, 16)) return UPNERF_EINVAL;
  hipLaunchKernelGGL(env_seam_kernel, dim3(env_blocks(24 * (int64_t)a->E)), dim3(ENV_THREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_env_composite(const upnerf_env_composite_args* a, void* stream) {
  if (!a || !env_size_ok(a->E) || a->R < 0 || !env_aligned(a->env, 16) || !env_aligned(a->rays, 16)) return UPNERF_EINVAL;
  if (!env_aligned(a->opacity, 4) || !env_aligned(a->rgb_in, 4) || !env_aligned(a->rgb_out, 4)) return UPNERF_EINVAL;
  if (a->R == 0) return 0;
  hipLaunchKernelGGL(env_composite_kernel, dim3(env_blocks(a->R)), dim3(ENV_THREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_env_composite_bwd(const upnerf_env_composite_bwd_args* a, void* stream) {
  if (!a || !env_size_ok(a->E) || a->R < 0 || !env_aligned(a->env, 16) || !env_aligned(a->rays, 16)) return UPNERF_EINVAL;
  if (!env_aligned(a->opacity, 4) || !env_aligned(a->g_out, 4) || !env_aligned(a->g_opacity, 4) || !env_aligned(a->g_rays, 16)) return UPNERF_EINVAL;
  if (a->R == 0) return 0;
  hipLaunchKernelGGL(env_composite_bwd_kernel, dim3(env_blocks(a->R)), dim3(ENV_THREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}
