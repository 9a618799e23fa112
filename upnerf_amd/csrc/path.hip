// Novel views along a camera path: the front end of a frame sequence that has no dataset image behind it.
//   upnerf_path_poses  keyframe poses -> one pose and one (near, far) per frame: quaternion slerp of the rotations, linear or
//                      uniform Catmull-Rom translations.  One thread per frame, everything in fp64, rounded to fp32 once
//                      (a few thousand frames at most: the cost is a launch, and the test gate is one fp32 rounding).
//   upnerf_path_rays   rows [row0, row0 + R) of the virtual [F][H][W] pixel list -> the [R][8] rows render_rays takes and, per
//                      embedding table, the [R][dim] rows blended between two table rows of the frame.  A streaming writer:
//                      32 B of rays plus sum(dim) * 4 B of rows per ray, nothing read but a few per-frame values (L2 hits).
//                      One thread per 16 bytes written; the threads of one output buffer are consecutive, so a wave's 64
//                      float4 stores are one contiguous 1 KiB (cdna_hip_programming.md, global memory coalescing).  No LDS,
//                      no atomics, every row a function of its global index alone: any chunking gives the same bits.
#include "common.cuh"

#include <math.h>

namespace {

// ---- poses ----------------------------------------------------------------------------------------------------------

// unit quaternion (w, x, y, z) of a rotation matrix, Shepperd's method: the branch whose divisor is the largest of the trace
// and the three diagonal entries, then normalised (the fp32 keyframes are orthogonal to ~1e-7 only)
__device__ __forceinline__ void quat_of(const double m[3][3], double q[4]) {
  const double tr = m[0][0] + m[1][1] + m[2][2];
  if (tr >= m[0][0] && tr >= m[1][1] && tr >= m[2][2]) {
    q[0] = 1.0 + tr;
    q[1] = m[2][1] - m[1][2];
    q[2] = m[0][2] - m[2][0];
    q[3] = m[1][0] - m[0][1];
  } else if (m[0][0] >= m[1][1] && m[0][0] >= m[2][2]) {
    q[0] = m[2][1] - m[1][2];
    q[1] = 1.0 + m[0][0] - m[1][1] - m[2][2];
    q[2] = m[0][1] + m[1][0];
    q[3] = m[0][2] + m[2][0];
  } else if (m[1][1] >= m[2][2]) {
    q[0] = m[0][2] - m[2][0];
    q[1] = m[0][1] + m[1][0];
    q[2] = 1.0 - m[0][0] + m[1][1] - m[2][2];
    q[3] = m[1][2] + m[2][1];
  } else {
    q[0] = m[1][0] - m[0][1];
    q[1] = m[0][2] + m[2][0];
    q[2] = m[1][2] + m[2][1];
    q[3] = 1.0 - m[0][0] - m[1][1] + m[2][2];
  }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] /= n;
}

__global__ __launch_bounds__(NTHREADS) void path_poses_kernel(upnerf_path_poses_args a) {
  const int f = blockIdx.x * NTHREADS + threadIdx.x;
  if (f >= a.F) return;
  const int K = a.K;
  double u = (double)a.u[f];
  u = fmin(fmax(u, 0.0), (double)(K - 1));  // (a NaN becomes 0)
  int k = (int)floor(u);
  if (k > K - 2) k = K - 2;
  const double s = u - (double)k;
  float* oc = a.c2w + (int64_t)f * 12;
  float* on = a.nf + (int64_t)f * 2;
  if (s == 0.0 || s == 1.0) {  // on a keyframe (s == 1: the last one): its floats, not a round trip through a quaternion
    const int kk = s == 0.0 ? k : k + 1;
#pragma unroll
    for (int i = 0; i < 12; ++i) oc[i] = a.key_c2w[(int64_t)kk * 12 + i];
    on[0] = a.key_nf[kk * 2];
    on[1] = a.key_nf[kk * 2 + 1];
    return;
  }
  const float* c0 = a.key_c2w + (int64_t)k * 12;
  const float* c1 = c0 + 12;
  double m0[3][3], m1[3][3], q0[4], q1[4], q[4];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      m0[i][j] = (double)c0[i * 4 + j];
      m1[i][j] = (double)c1[i * 4 + j];
    }
  quat_of(m0, q0);
  quat_of(m1, q1);
  double dot = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
  if (dot < 0.0) {  // q and -q are one rotation: take the shorter arc
    dot = -dot;
#pragma unroll
    for (int i = 0; i < 4; ++i) q1[i] = -q1[i];
  }
  if (dot > 1.0 - 1e-9) {  // sin(theta) -> 0: normalised lerp (exact for identical keys)
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = (1.0 - s) * q0[i] + s * q1[i];
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] /= n;
  } else {
    const double th = acos(dot), sn = sin(th);
    const double w0 = sin((1.0 - s) * th) / sn, w1 = sin(s * th) / sn;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = w0 * q0[i] + w1 * q1[i];
  }
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double Rm[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                           {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                           {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
  // translation: lerp, or uniform Catmull-Rom through (p0, p1, p2, p3) with the end keys standing in for the missing neighbours
  const float* cm = a.key_c2w + (int64_t)(k > 0 ? k - 1 : 0) * 12;
  const float* cp = a.key_c2w + (int64_t)(k + 2 < K ? k + 2 : K - 1) * 12;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double p1 = (double)c0[i * 4 + 3], p2 = (double)c1[i * 4 + 3];
    double t;
    if (a.mode == UPNERF_PATH_CATMULL) {
      const double p0 = (double)cm[i * 4 + 3], p3 = (double)cp[i * 4 + 3];
      t = 0.5 * (2.0 * p1 + s * ((p2 - p0) + s * ((2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3) + s * (3.0 * (p1 - p2) + p3 - p0))));
    } else {
      t = (1.0 - s) * p1 + s * p2;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) oc[i * 4 + j] = (float)Rm[i][j];
    oc[i * 4 + 3] = (float)t;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
    on[i] = (float)((1.0 - s) * (double)a.key_nf[k * 2 + i] + s * (double)a.key_nf[(k + 1) * 2 + i]);
}

// ---- rays and blended rows ------------------------------------------------------------------------------------------

// how the grid is dealt to the output buffers: segment 0 = the ray rows (two 16-byte groups each), segment 1 + i = table i
// (ceil(dim / 4) groups per row); blk0[j] = first workgroup of segment j, blk0[n_tables + 1] = the grid
struct PathPlan {
  int blk0[UPNERF_PATH_MAX_TABLES + 2];
  int vec[UPNERF_PATH_MAX_TABLES + 1];  // 16-byte accesses allowed (alignment; tables: dim % 4 == 0 as well)
};

// wa * a + wb * b as two products and a sum, each rounded (no fma; the __f*_rn intrinsics are plain operators in HIP and would
// be contracted): with (wa, wb) = (1, 0) or (0, 1) a finite table row comes back bit for bit, and any other weights give what
// torch's `wa * a + wb * b` gives
__device__ __forceinline__ float blend(float wa, float a, float wb, float b) {
#pragma clang fp contract(off)
  const float pa = wa * a;
  const float pb = wb * b;
  return pa + pb;
}

__global__ __launch_bounds__(NTHREADS) void path_rays_kernel(upnerf_path_rays_args a, PathPlan pl) {
  int seg = 0;  // (uniform over the workgroup)
#pragma unroll
  for (int j = 1; j <= UPNERF_PATH_MAX_TABLES; ++j)
    if (j <= a.n_tables && (int)blockIdx.x >= pl.blk0[j]) seg = j;
  const int64_t id = (int64_t)((int)blockIdx.x - pl.blk0[seg]) * NTHREADS + threadIdx.x;
  const int64_t hw = (int64_t)a.H * a.W;
  if (seg == 0) {
    const int64_t r = id >> 1;
    if (r >= a.R) return;
    const int half = (int)(id & 1);
    const int64_t g = a.row0 + r;
    const int64_t f = g / hw, p = g - f * hw;
    const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
    const float* c = a.c2w + f * 12;
    // camera-space direction on the integer pixel grid (no half-pixel shift), rotated and normalised as upnerf_pose_rays_fwd
    const float dx = ((float)x - a.cx) / a.fx, dy = -((float)y - a.cy) / a.fy, dz = -1.f;
    float v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = dx * c[i * 4] + dy * c[i * 4 + 1] + dz * c[i * 4 + 2];
    const float nrm = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    f32x4 o;
    if (half == 0) o = f32x4{c[3], c[7], c[11], v[0] / nrm};
    else o = f32x4{v[1] / nrm, v[2] / nrm, a.nf[f * 2], a.nf[f * 2 + 1]};
    float* dst = a.rays + r * 8 + half * 4;
    if (pl.vec[0]) *(f32x4*)dst = o;
    else dst[0] = o.x, dst[1] = o.y, dst[2] = o.z, dst[3] = o.w;
    return;
  }
  const upnerf_path_table tb = a.tables[seg - 1];
  const int gpr = (tb.dim + 3) >> 2;
  const int64_t r = id / gpr;
  if (r >= a.R) return;
  const int j0 = (int)(id - r * gpr) * 4;
  const int64_t f = (a.row0 + r) / hw;
  int i0 = a.i0[f], i1 = a.i1[f];  // out-of-range rows are clamped (the indices live on the device: no host check)
  i0 = i0 < 0 ? 0 : (i0 >= tb.n_rows ? tb.n_rows - 1 : i0);
  i1 = i1 < 0 ? 0 : (i1 >= tb.n_rows ? tb.n_rows - 1 : i1);
  const float t = a.t[f], w0 = 1.f - t;
  const float* ra = tb.table + (int64_t)i0 * tb.dim + j0;
  const float* rb = tb.table + (int64_t)i1 * tb.dim + j0;
  float* dst = tb.out + r * tb.dim + j0;
  if (pl.vec[seg]) {
    const f32x4 va = *(const f32x4*)ra, vb = *(const f32x4*)rb;
    *(f32x4*)dst = f32x4{blend(w0, va.x, t, vb.x), blend(w0, va.y, t, vb.y), blend(w0, va.z, t, vb.z), blend(w0, va.w, t, vb.w)};
  } else {
    const int cnt = tb.dim - j0 < 4 ? tb.dim - j0 : 4;
    for (int j = 0; j < cnt; ++j) dst[j] = blend(w0, ra[j], t, rb[j]);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int upnerf_path_poses(const upnerf_path_poses_args* a, void* stream) {
  if (!a || a->K < 2 || a->F < 1) return UPNERF_EINVAL;
  if (a->mode != UPNERF_PATH_LINEAR && a->mode != UPNERF_PATH_CATMULL) return UPNERF_EINVAL;
  if (!a->key_c2w || !a->key_nf || !a->u || !a->c2w || !a->nf) return UPNERF_EINVAL;
  hipLaunchKernelGGL(path_poses_kernel, dim3((a->F + NTHREADS - 1) / NTHREADS), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_path_rays(const upnerf_path_rays_args* a, void* stream) {
  if (!a || a->F < 1 || a->H < 1 || a->W < 1 || a->R < 1 || a->row0 < 0) return UPNERF_EINVAL;
  if (a->row0 + a->R > (int64_t)a->F * a->H * a->W) return UPNERF_EINVAL;
  if (a->n_tables < 0 || a->n_tables > UPNERF_PATH_MAX_TABLES) return UPNERF_EINVAL;
  if (!a->c2w || !a->nf || !a->rays) return UPNERF_EINVAL;
  if (!(a->fx != 0.f) || !(a->fy != 0.f) || a->fx != a->fx || a->fy != a->fy) return UPNERF_EINVAL;
  if (a->n_tables > 0 && (!a->i0 || !a->i1 || !a->t)) return UPNERF_EINVAL;
  PathPlan pl = {};
  int64_t blocks = ((int64_t)a->R * 2 + NTHREADS - 1) / NTHREADS;
  pl.vec[0] = aligned16(a->rays);
  for (int i = 0; i < a->n_tables; ++i) {
    const upnerf_path_table& tb = a->tables[i];
    if (tb.dim < 1 || tb.dim > UPNERF_PATH_MAX_DIM || tb.n_rows < 1 || !tb.table || !tb.out) return UPNERF_EINVAL;
    pl.blk0[i + 1] = (int)blocks;
    pl.vec[i + 1] = tb.dim % 4 == 0 && aligned16(tb.table) && aligned16(tb.out);
    blocks += ((int64_t)a->R * ((tb.dim + 3) / 4) + NTHREADS - 1) / NTHREADS;
  }
  if (blocks > 0x7fffffff) return UPNERF_EUNSUP;
  pl.blk0[a->n_tables + 1] = (int)blocks;
  hipLaunchKernelGGL(path_rays_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a, pl);
  return (int)hipGetLastError();
}
