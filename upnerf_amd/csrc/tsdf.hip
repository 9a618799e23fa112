// Depth-map fusion: rendered depth maps folded into a truncated signed distance volume (TSDF) on the grid of the mesher, whose
// zero level upnerf_mtet_* then meshes.  The surface is where the cameras SAW it -- the composited depth the
// model was trained on -- not a threshold of the raw density.
//   upnerf_tsdf_integrate  up to UPNERF_TSDF_MAX_VIEWS views into the volume in one launch.
//   upnerf_tsdf_surface    -tsdf where the voxel was observed often enough, NaN elsewhere: the grid the mesher takes at level 0.
//   upnerf_tsdf_sample     the fused colour at arbitrary points (the mesh's vertices), trilinear over the corners that have one.
//
// The arithmetic of a voxel p (the fp32 grid point: fp64 grid coordinate rounded once, as mesh.hip places its vertices), views
// in index order, all fp32, every operation rounded on its own:
//   1. pc = R^T (p - c), zc = -pc.z (the camera looks down -z); skip unless zc > 0
//   2. u = fx pc.x / zc + cx,  v = cy - fy pc.y / zc            (no half-pixel shift)
//   3. iu = floor(u + 0.5), jv = floor(v + 0.5); skip outside [0, W) x [0, H)
//   4. d = depth[jv W + iu]; skip unless finite and > 0, and unless opacity[jv W + iu] >= min_opacity where there is a map
//   5. r = |p - c|, sdf = d - r; skip if sdf < -trunc            (depths are Euclidean: rays are unit length)
//   6. val = min(1, sdf / trunc); w = 1 or the pixel's opacity; Wn = W + w; T += (val - T) (w / Wn)
//   7. colour, where the view has one and sdf <= trunc: the same running mean with a weight of its own (a fourth volume)
//
// Shape: one thread per voxel, x fastest -- a wave reads and writes 256 contiguous bytes of every volume line -- and the voxel's
// accumulators stay in registers over all views of the launch: the volume is read and written once per LAUNCH, 48 B per voxel
// with colour, whatever the number of views.  The views are part of the kernel's argument block: the view loop is uniform and
// their parameters come through scalar loads.  The depth, opacity and colour maps are gathered (neighbouring voxels project to
// neighbouring pixels: the caches absorb it).  No atomics, no LDS, no cross-thread reduction; fp contraction is off, so a
// register that carries an accumulator from one view to the next holds what a store and a reload would: any split of a list of
// views into launches gives the same bits.  Memory-bound by construction.
#include "common.cuh"
#include "grid.cuh"

#include <limits.h>
#include <math.h>

namespace {

__device__ __forceinline__ void voxel_of(int64_t g, int Nx, int Ny, int& x, int& y, int& z) {
  x = (int)(g % Nx);
  y = (int)((g / Nx) % Ny);
  z = (int)(g / ((int64_t)Nx * Ny));
}

__global__ __launch_bounds__(NTHREADS) void tsdf_integrate_kernel(upnerf_tsdf_integrate_args a, int64_t N) {
#pragma clang fp contract(off)
  const int64_t g = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (g >= N) return;
  int x, y, z;
  voxel_of(g, a.Nx, a.Ny, x, y, z);
  const float px = (float)grid_coord(a.lo[0], a.hi[0], a.Nx, x);
  const float py = (float)grid_coord(a.lo[1], a.hi[1], a.Ny, y);
  const float pz = (float)grid_coord(a.lo[2], a.hi[2], a.Nz, z);
  const bool colour = a.rgb != nullptr;
  float T = a.tsdf[g], Wt = a.weight[g];
  float c0 = 0.f, c1 = 0.f, c2 = 0.f, Cw = 0.f;
  if (colour) {
    c0 = a.rgb[g * 3 + 0], c1 = a.rgb[g * 3 + 1], c2 = a.rgb[g * 3 + 2];
    Cw = a.rgb_weight[g];
  }
  const float trunc = a.trunc;
  for (int k = 0; k < a.n_views; ++k) {
    const upnerf_tsdf_view& vw = a.views[k];
    const float* m = vw.c2w;  // m[4 i + j] = R[i][j], m[4 i + 3] = c[i]
    const float d0 = px - m[3], d1 = py - m[7], d2 = pz - m[11];
    const float pcx = (m[0] * d0 + m[4] * d1) + m[8] * d2;
    const float pcy = (m[1] * d0 + m[5] * d1) + m[9] * d2;
    const float pcz = (m[2] * d0 + m[6] * d1) + m[10] * d2;
    const float zc = -pcz;
    if (!(zc > 0.f)) continue;
    const float u = (vw.fx * pcx) / zc + vw.cx;
    const float v = vw.cy - (vw.fy * pcy) / zc;
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    if (!(fu >= 0.f && fu < (float)vw.W && fv >= 0.f && fv < (float)vw.H)) continue;  // (a NaN fails the comparison)
    const int64_t pix = (int64_t)fv * vw.W + (int64_t)fu;
    const float d = vw.depth[pix];
    if (!(isfinite(d) && d > 0.f)) continue;
    float w = 1.f;
    if (vw.opacity) {
      const float op = vw.opacity[pix];
      if (!(op >= a.min_opacity)) continue;
      if (a.weight_mode == 1) w = op;
    }
    if (!(w > 0.f) || !isfinite(w)) continue;
    const float r = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    const float sdf = d - r;
    if (!(sdf >= -trunc)) continue;
    const float val = fminf(1.f, sdf / trunc);
    const float Wn = Wt + w;
    T += (val - T) * (w / Wn);
    Wt = Wn;
    if (colour && vw.rgb && sdf <= trunc) {
      const float Cn = Cw + w;
      const float q = w / Cn;
      c0 += (vw.rgb[pix * 3 + 0] - c0) * q;
      c1 += (vw.rgb[pix * 3 + 1] - c1) * q;
      c2 += (vw.rgb[pix * 3 + 2] - c2) * q;
      Cw = Cn;
    }
  }
  a.tsdf[g] = T;
  a.weight[g] = Wt;
  if (colour) {
    a.rgb[g * 3 + 0] = c0, a.rgb[g * 3 + 1] = c1, a.rgb[g * 3 + 2] = c2;
    a.rgb_weight[g] = Cw;
  }
}

__global__ __launch_bounds__(NTHREADS) void tsdf_surface_kernel(upnerf_tsdf_surface_args a) {
  const int64_t g = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (g >= a.n) return;
  a.out[g] = a.weight[g] >= a.min_weight ? -a.tsdf[g] : __builtin_nanf("");
}

// continuous index along an axis -> (lower corner, fraction); false for a NaN
__device__ __forceinline__ bool axis_cell(float p, float lo, float hi, int n, int& i, float& f) {
  float gidx = (p - lo) / (hi - lo) * (float)(n - 1);
  if (gidx != gidx) return false;
  gidx = fminf(fmaxf(gidx, 0.f), (float)(n - 1));
  i = min((int)floorf(gidx), n - 2);
  f = gidx - (float)i;
  return true;
}

__global__ __launch_bounds__(NTHREADS) void tsdf_sample_kernel(upnerf_tsdf_sample_args a) {
  const int64_t id = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (id >= a.V) return;
  const float* p = a.points + id * 3;
  int ix, iy, iz;
  float fx, fy, fz;
  float sum = 0.f, c[3] = {0.f, 0.f, 0.f};
  if (axis_cell(p[0], a.lo[0], a.hi[0], a.Nx, ix, fx) && axis_cell(p[1], a.lo[1], a.hi[1], a.Ny, iy, fy) &&
      axis_cell(p[2], a.lo[2], a.hi[2], a.Nz, iz, fz)) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int ox = k & 1, oy = (k >> 1) & 1, oz = k >> 2;
      const int64_t g = ((int64_t)(iz + oz) * a.Ny + (iy + oy)) * a.Nx + (ix + ox);
      const float w = (ox ? fx : 1.f - fx) * (oy ? fy : 1.f - fy) * (oz ? fz : 1.f - fz);
      if (a.rgb_weight[g] > 0.f && w > 0.f) {
        sum += w;
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] += w * a.rgb[g * 3 + j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) a.out[id * 3 + j] = sum > 0.f ? c[j] / sum : 0.5f;
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + NTHREADS - 1) / NTHREADS); }  // n <= INT_MAX everywhere

bool volume_ok(int Nx, int Ny, int Nz, const float* lo, const float* hi, int64_t* N) {
  if (Nx < 2 || Ny < 2 || Nz < 2) return false;
  const int64_t n = (int64_t)Nx * Ny;
  if (n > INT_MAX || n * Nz > INT_MAX) return false;
  for (int k = 0; k < 3; ++k)
    if (!isfinite(lo[k]) || !isfinite(hi[k]) || !(hi[k] > lo[k])) return false;
  *N = n * Nz;
  return true;
}

}  // namespace

extern "C" int upnerf_tsdf_integrate(const upnerf_tsdf_integrate_args* a, void* stream) {
  int64_t N;
  if (!a || !a->tsdf || !a->weight || (a->rgb && !a->rgb_weight)) return UPNERF_EINVAL;
  if (a->n_views < 1 || a->n_views > UPNERF_TSDF_MAX_VIEWS) return UPNERF_EINVAL;
  if (!(a->trunc > 0.f) || !isfinite(a->trunc) || a->min_opacity != a->min_opacity) return UPNERF_EINVAL;
  if (a->weight_mode != 0 && a->weight_mode != 1) return UPNERF_EINVAL;
  if (!volume_ok(a->Nx, a->Ny, a->Nz, a->lo, a->hi, &N)) return UPNERF_EINVAL;
  for (int k = 0; k < a->n_views; ++k) {
    const upnerf_tsdf_view& v = a->views[k];
    if (!v.depth || v.W < 1 || v.H < 1 || (int64_t)v.W * v.H > INT_MAX) return UPNERF_EINVAL;
    if (a->weight_mode == 1 && !v.opacity) return UPNERF_EINVAL;
  }
  const unsigned nb = blocks_for(N);
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(nb), dim3(NTHREADS), 0, (hipStream_t)stream, *a, N);
  return (int)hipGetLastError();
}

extern "C" int upnerf_tsdf_surface(const upnerf_tsdf_surface_args* a, void* stream) {
  if (!a || !a->tsdf || !a->weight || !a->out || a->n < 1 || a->n > INT_MAX) return UPNERF_EINVAL;
  if (a->min_weight != a->min_weight) return UPNERF_EINVAL;
  const unsigned nb = blocks_for(a->n);
  hipLaunchKernelGGL(tsdf_surface_kernel, dim3(nb), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_tsdf_sample(const upnerf_tsdf_sample_args* a, void* stream) {
  int64_t N;
  if (!a || !a->rgb || !a->rgb_weight || !a->points || !a->out || a->V < 1) return UPNERF_EINVAL;
  if (!volume_ok(a->Nx, a->Ny, a->Nz, a->lo, a->hi, &N)) return UPNERF_EINVAL;
  const unsigned nb = blocks_for(a->V);
  hipLaunchKernelGGL(tsdf_sample_kernel, dim3(nb), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}
