// SSIM of rendered images against their targets: utils/metric.py:23-30 of the reference (kornia ssim_loss with a 3x3
// Gaussian window, sigma 1.5, reflect padding; then 1 - 2 * dssim), which runs on the CPU after a copy of every render.
// Memory-bound and small (a 175 k-pixel validation image is 4 MB of reads): one pixel per thread, a 64 x 4 tile per
// workgroup, the 3 x 3 halo read through L1.  The per-image mean is a fixed-order fp64 reduction (tiles -> scratch ->
// one finishing workgroup per image), so the result does not depend on the batch an image comes in.
#include "common.cuh"

namespace {

#define SSIM_TX 64
#define SSIM_TY (NTHREADS / SSIM_TX)

struct SsimWeights {
  float ee, ec, cc;  // outer(g, g) of the normalised 1-D window g = (e, c, e): corner, edge, centre
};

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// one tile of one image: the map (optional) and the tile's sum over (c, y, x) of clamp((1 - s) / 2, 0, 1) in fp64
__global__ __launch_bounds__(NTHREADS) void ssim_tile_kernel(upnerf_ssim_args a, SsimWeights wt, int tiles_x,
                                                            int tiles, double* __restrict__ part) {
  const int tid = threadIdx.x;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int y = (t / tiles_x) * SSIM_TY + tid / SSIM_TX, x = (t % tiles_x) * SSIM_TX + tid % SSIM_TX;
  double acc = 0.0;
  if (y < a.H && x < a.W) {
    const float w[9] = {wt.ee, wt.ec, wt.ee, wt.ec, wt.cc, wt.ec, wt.ee, wt.ec, wt.ee};
    int64_t po[9], go[9];
    {
      const int ys[3] = {reflect(y - 1, a.H), y, reflect(y + 1, a.H)};
      const int xs[3] = {reflect(x - 1, a.W), x, reflect(x + 1, a.W)};
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          po[3 * i + j] = n * a.pred_stride[0] + ys[i] * a.pred_stride[2] + xs[j] * a.pred_stride[3];
          go[3 * i + j] = n * a.gt_stride[0] + ys[i] * a.gt_stride[2] + xs[j] * a.gt_stride[3];
        }
    }
    for (int c = 0; c < a.C; ++c) {
      const float* p = a.pred + c * a.pred_stride[1];
      const float* g = a.gt + c * a.gt_stride[1];
      float u[9], v[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        u[k] = p[po[k]];
        v[k] = g[go[k]];
      }
      float mu1 = 0.f, mu2 = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        mu1 += w[k] * u[k];
        mu2 += w[k] * v[k];
      }
      // centred moments: filter(x^2) - mu^2 in fp32 cancels to ~1e-7 * x^2, which is not small against C2 = 9e-4
      float s11 = 0.f, s22 = 0.f, s12 = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const float du = u[k] - mu1, dv = v[k] - mu2;
        s11 += w[k] * du * du;
        s22 += w[k] * dv * dv;
        s12 += w[k] * du * dv;
      }
      const float C1 = 1e-4f, C2 = 9e-4f;
      const float num = (2.f * mu1 * mu2 + C1) * (2.f * s12 + C2);
      const float den = (mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2);
      const float s = num / (den + 1e-12f);
      if (a.map) a.map[(((int64_t)n * a.C + c) * a.H + y) * a.W + x] = s;
      // torch.clamp: comparisons, not fminf / fmaxf, so that a NaN stays NaN
      float l = (1.f - s) * 0.5f;
      l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
      acc += (double)l;
    }
  }
  const double sum = block_sum_f64(acc);
  if (tid == 0) part[blockIdx.x] = sum;
}

// ssim[n] = 1 - 2 * (sum of the image's tile partials, in tile order per thread, then a fixed tree) / (C * H * W)
__global__ __launch_bounds__(NTHREADS) void ssim_finish_kernel(upnerf_ssim_args a, int tiles,
                                                              const double* __restrict__ part) {
  const int n = blockIdx.x, tid = threadIdx.x;
  const double* q = part + (int64_t)n * tiles;
  double acc = 0.0;
  for (int t = tid; t < tiles; t += NTHREADS) acc += q[t];
  const double sum = block_sum_f64(acc);
  if (tid == 0) a.ssim[n] = (float)(1.0 - 2.0 * (sum / ((double)a.C * a.H * a.W)));
}

int check(const upnerf_ssim_args* a) {
  if (!a || a->N < 1 || a->C < 1 || a->H < 2 || a->W < 2) return UPNERF_EINVAL;
  return 0;
}

long long scratch_doubles(const upnerf_ssim_args* a, int* tiles_x, int* tiles) {
  *tiles_x = (a->W + SSIM_TX - 1) / SSIM_TX;
  *tiles = *tiles_x * ((a->H + SSIM_TY - 1) / SSIM_TY);
  return (long long)a->N * *tiles;
}

}  // namespace

extern "C" int upnerf_ssim_scratch(const upnerf_ssim_args* a) {
  int rc = check(a);
  if (rc) return rc;
  int tx, tiles;
  const long long n = scratch_doubles(a, &tx, &tiles);
  return n > 0x7fffffffLL ? UPNERF_EUNSUP : (int)n;
}

extern "C" int upnerf_ssim(const upnerf_ssim_args* a, double* scratch, void* stream) {
  int rc = check(a);
  if (rc) return rc;
  if (!a->pred || !a->gt || !a->ssim || !scratch) return UPNERF_EINVAL;
  int tiles_x, tiles;
  const long long blocks = scratch_doubles(a, &tiles_x, &tiles);
  if (blocks > 0x7fffffffLL) return UPNERF_EUNSUP;
  // the window in fp64, rounded once: g = exp(-x^2 / (2 * 1.5^2)), x in {-1, 0, 1}, normalised to sum 1
  const double e = exp(-1.0 / 4.5), c = 1.0 / (1.0 + 2.0 * e), ge = e * c;
  const SsimWeights wt = {(float)(ge * ge), (float)(ge * c), (float)(c * c)};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, st, *a, wt, tiles_x, tiles, scratch);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(a->N), dim3(NTHREADS), 0, st, *a, tiles, (const double*)scratch);
  return (int)hipGetLastError();
}
