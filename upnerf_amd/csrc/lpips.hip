// LPIPS (AlexNet) of rendered images against their targets: the third column of the reference's novel-view table
// (models/nerf_system_optmize.py:184, lpips_alex(img_gt, img) with normalize=False), computed where the render already is.
// Three kernels, composed by upnerf_amd/lpips.py:
//   * upnerf_conv2d: convolution + bias + optional ReLU as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products, one
//     rounding per term inside a chunk of 32 terms, the chunks added in fp64, one rounding of the result to fp32).
//     M = C_out, N = images * H_out * W_out, K = C_in * k * k.  A workgroup owns a 64 x 128 tile; per 32-wide K chunk the weights go to LDS as [m][k] and the input
//     patches as [k][n], gathered with stride, zero padding and the optional scaling layer on the way in -- no im2col buffer
//     exists in HBM.  Column n of the product depends on column n of the patch matrix only and the K order is fixed, so an
//     image's bits do not depend on the batch it comes in.
//   * upnerf_maxpool2d: 3 x 3, stride 2, floor mode, one output per thread.
//   * upnerf_lpips_dist: per pixel the two channel norms and the weighted squared difference of the unit vectors, in fp64
//     (memory-bound either way); the spatial mean is the fixed-order reduction of ssim_tile_kernel: tile partials into caller
//     scratch, one finishing workgroup per image pair.
#include "common.cuh"

namespace {

#define CV_BM 64                // C_out rows per workgroup
#define CV_BN 128               // output pixels per workgroup: 32 per wave
#define CV_BK 32                // K chunk
#define CV_LDA (CV_BK + 4)      // [m][k]: 16 rows x 16 bytes of one ds_read_b128 phase cover all 64 banks once
#define CV_LDB (CV_BN + 8)      // [k][n]: rows k and k + 4 (the two lane halves of an MFMA operand) 32 banks apart

// the scaling layer of the lpips package (fp32 buffers there): x = (v - shift) / scale per channel
__device__ __forceinline__ float scale_in_f(float v, int c) {
  const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
  const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
  return (v - shift) / scale;
}

template <int KS, int S, int P>
__global__ __launch_bounds__(NTHREADS) void conv2d_kernel(upnerf_conv2d_args a, int Ho, int Wo, int K, int64_t Ntot) {
  __shared__ __attribute__((aligned(16))) float As[CV_BM * CV_LDA];
  __shared__ __attribute__((aligned(16))) float Bs[CV_BK * CV_LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
  const int m0 = blockIdx.y * CV_BM;
  const int64_t nb = (int64_t)blockIdx.x * CV_BN;
  const int64_t HWo = (int64_t)Ho * Wo;

  // staging roles: weights k = tid & 31 of rows (tid >> 5) + 8 j; patches pixel tid & 127 at k = (tid >> 7) + 2 j
  const int ak = tid & 31, ar = tid >> 5;
  const int bn = tid & 127, bk = tid >> 7;
  const int64_t n = nb + bn;
  const bool nvalid = n < Ntot;
  int64_t xbase = 0;
  int iy0 = 0, ix0 = 0;
  if (nvalid) {
    const int64_t img = n / HWo;
    const int pix = (int)(n - img * HWo);
    const int oy = pix / Wo, ox = pix - oy * Wo;
    iy0 = oy * S - P;
    ix0 = ox * S - P;
    xbase = img * a.x_stride[0];
  }
  float ra[8], rb[16];
  auto gload = [&](int kc) {
    const int ka = kc + ak;
#pragma unroll
    for (int j = 0; j < 8; ++j) ra[j] = ka < K ? a.w[(int64_t)(m0 + ar + 8 * j) * K + ka] : 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int k = kc + bk + 2 * j;
      float v = 0.f;  // the K tail, the N tail and the zero padding (of the SCALED image: 0, not (0 - shift) / scale)
      if (nvalid && k < K) {
        const int c = k / (KS * KS), r = k - c * (KS * KS);
        const int ky = r / KS, kx = r - ky * KS;
        const int iy = iy0 + ky, ix = ix0 + kx;
        if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
          v = a.x[xbase + c * a.x_stride[1] + iy * a.x_stride[2] + ix * a.x_stride[3]];
          if (a.scale_in) v = scale_in_f(v, c);
        }
      }
      rb[j] = v;
    }
  };

  // A chunk's 32 terms are one fp32 MFMA chain; the chunks are added in fp64.  A single fp32 chain over K = 3456 terms leaves
  // ~4e-8 sqrt(K) of relative error on a feature, and LPIPS of a near-identical pair is a sum of squared DIFFERENCES of features
  // that agree to ~1e-3: that error, not the fp32 level of a single feature, decided whether such a pair met 1e-4.
  double sum[2][16];
#pragma unroll
  for (int r = 0; r < 16; ++r) sum[0][r] = sum[1][r] = 0.0;
  gload(0);
  for (int kc = 0; kc < K; kc += CV_BK) {
    __syncthreads();  // the previous chunk has been read
#pragma unroll
    for (int j = 0; j < 8; ++j) As[(ar + 8 * j) * CV_LDA + ak] = ra[j];
#pragma unroll
    for (int j = 0; j < 16; ++j) Bs[(bk + 2 * j) * CV_LDB + bn] = rb[j];
    __syncthreads();
    if (kc + CV_BK < K) gload(kc + CV_BK);  // in flight under the 32 MFMAs below
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
#pragma unroll
    for (int t = 0; t < CV_BK / 8; ++t) {
      // lane half hh takes k = 8 t + 4 hh + q in MFMA q: a permutation of k inside the group of eight, the same for A and B
      const f32x4 a0 = *(const f32x4*)&As[li * CV_LDA + 8 * t + 4 * hh];
      const f32x4 a1 = *(const f32x4*)&As[(32 + li) * CV_LDA + 8 * t + 4 * hh];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float b = Bs[(8 * t + 4 * hh + q) * CV_LDB + wave * 32 + li];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[q], b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[q], b, acc[1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sum[0][r] += (double)acc[0][r];
      sum[1][r] += (double)acc[1][r];
    }
  }

  // D[row = (r & 3) + 8 (r >> 2) + 4 hh][col = li]: the 32 lanes of a half store 32 consecutive pixels of one channel
  const int64_t ncol = nb + wave * 32 + li;
  float bias[2][16];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) bias[mt][r] = a.bias[m0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh];
  if (ncol < Ntot) {
    const int64_t img = ncol / HWo, pix = ncol - img * HWo;
    float* yo = a.y + (img * a.C_out + m0) * HWo + pix;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = (float)(sum[mt][r] + (double)bias[mt][r]);
        if (a.relu) v = v < 0.f ? 0.f : v;  // (a comparison that keeps a NaN, as torch.relu does)
        yo[(int64_t)(mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh) * HWo] = v;
      }
  }
}

__global__ __launch_bounds__(NTHREADS) void maxpool2d_kernel(upnerf_maxpool2d_args a, int Ho, int Wo, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t plane = i / ((int64_t)Ho * Wo);
  const int pix = (int)(i - plane * Ho * Wo);
  const int oy = pix / Wo, ox = pix - oy * Wo;
  const float* x = a.x + (plane * a.H + 2 * oy) * a.W + 2 * ox;
  float m = x[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float v = x[(int64_t)dy * a.W + dx];
      m = (v > m || v != v) ? v : m;  // a NaN in the window wins, as in torch's max_pool2d
    }
  a.y[i] = m;
}

// one tile of 256 pixels of one image pair: sum over the pixels of sum_c w_c (a_c / |a| - b_c / |b|)^2, fp64
__global__ __launch_bounds__(NTHREADS) void lpips_dist_kernel(upnerf_lpips_dist_args a, int64_t HW, int tiles,
                                                             double* __restrict__ part) {
  const int tid = threadIdx.x;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int64_t p = (int64_t)t * NTHREADS + tid;
  double acc = 0.0;
  if (p < HW) {
    const float* fa = a.feat + (int64_t)n * a.C * HW + p;
    const float* fb = a.feat + (int64_t)(a.N + n) * a.C * HW + p;
    double sa = 0.0, sb = 0.0;
    for (int c = 0; c < a.C; ++c) {
      const double u = fa[c * HW], v = fb[c * HW];
      sa += u * u;
      sb += v * v;
    }
    // the epsilon is outside the root: an all-zero pixel (every ReLU dead) gives 0 / 1e-10 = 0, not NaN
    const double ia = 1.0 / (sqrt(sa) + 1e-10), ib = 1.0 / (sqrt(sb) + 1e-10);
    for (int c = 0; c < a.C; ++c) {
      // two rounded products, then the difference: contracted into fma(a, ia, -(b * ib)) a pair of identical images gives the
      // rounding residue of one product (5e-33 measured) instead of exactly 0
#pragma clang fp contract(off)
      const double ua = fa[c * HW] * ia, ub = fb[c * HW] * ib;
      const double d = ua - ub;
      acc += (double)a.w[c] * d * d;
    }
  }
  const double sum = block_sum_f64(acc);
  if (tid == 0) part[blockIdx.x] = sum;
}

// out[n] (+)= (sum of the pair's tile partials, in tile order per thread, then a fixed tree) / (H * W)
__global__ __launch_bounds__(NTHREADS) void lpips_finish_kernel(upnerf_lpips_dist_args a, int64_t HW, int tiles,
                                                               const double* __restrict__ part) {
  const int n = blockIdx.x, tid = threadIdx.x;
  const double* q = part + (int64_t)n * tiles;
  double acc = 0.0;
  for (int t = tid; t < tiles; t += NTHREADS) acc += q[t];
  const double sum = block_sum_f64(acc);
  if (tid == 0) {
    const float d = (float)(sum / (double)HW);
    a.out[n] = a.accumulate ? a.out[n] + d : d;
  }
}

int out_size(int in, int k, int s, int p) { return (in + 2 * p - k) / s + 1; }

const int MAX_DIM = 32768;  // per image side: a pixel index inside one image fits an int

int conv_check(const upnerf_conv2d_args* a, int* Ho, int* Wo) {
  if (!a || a->N < 1 || a->C_in < 1 || a->C_out < 1 || a->H < 1 || a->W < 1 || a->H > MAX_DIM || a->W > MAX_DIM)
    return UPNERF_EINVAL;
  if (!a->x || !a->w || !a->bias || !a->y) return UPNERF_EINVAL;
  const bool known = (a->C_in == 3 && a->k == 11 && a->stride == 4 && a->pad == 2) ||
                     (a->C_in == 64 && a->k == 5 && a->stride == 1 && a->pad == 2) ||
                     ((a->C_in == 192 || a->C_in == 384 || a->C_in == 256) && a->k == 3 && a->stride == 1 && a->pad == 1);
  if (!known || a->C_out % CV_BM) return UPNERF_EUNSUP;
  if (a->scale_in && a->C_in != 3) return UPNERF_EINVAL;
  if (a->H + 2 * a->pad < a->k || a->W + 2 * a->pad < a->k) return UPNERF_EINVAL;
  *Ho = out_size(a->H, a->k, a->stride, a->pad);
  *Wo = out_size(a->W, a->k, a->stride, a->pad);
  return 0;
}

}  // namespace

extern "C" int upnerf_conv2d(const upnerf_conv2d_args* a, void* stream) {
  int Ho, Wo;
  int rc = conv_check(a, &Ho, &Wo);
  if (rc) return rc;
  const int64_t Ntot = (int64_t)a->N * Ho * Wo;
  const int64_t bx = (Ntot + CV_BN - 1) / CV_BN;
  if (bx > 0x7fffffffLL || a->C_out / CV_BM > 65535) return UPNERF_EUNSUP;
  const int K = a->C_in * a->k * a->k;
  const dim3 grid((unsigned)bx, (unsigned)(a->C_out / CV_BM));
  hipStream_t st = (hipStream_t)stream;
  if (a->k == 11)
    hipLaunchKernelGGL((conv2d_kernel<11, 4, 2>), grid, dim3(NTHREADS), 0, st, *a, Ho, Wo, K, Ntot);
  else if (a->k == 5)
    hipLaunchKernelGGL((conv2d_kernel<5, 1, 2>), grid, dim3(NTHREADS), 0, st, *a, Ho, Wo, K, Ntot);
  else
    hipLaunchKernelGGL((conv2d_kernel<3, 1, 1>), grid, dim3(NTHREADS), 0, st, *a, Ho, Wo, K, Ntot);
  return (int)hipGetLastError();
}

extern "C" int upnerf_maxpool2d(const upnerf_maxpool2d_args* a, void* stream) {
  if (!a || a->N < 1 || a->C < 1 || a->H < 3 || a->W < 3 || a->H > MAX_DIM || a->W > MAX_DIM || !a->x || !a->y)
    return UPNERF_EINVAL;
  const int Ho = out_size(a->H, 3, 2, 0), Wo = out_size(a->W, 3, 2, 0);
  const int64_t total = (int64_t)a->N * a->C * Ho * Wo;
  const int64_t blocks = (total + NTHREADS - 1) / NTHREADS;
  if (blocks > 0x7fffffffLL) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(maxpool2d_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a, Ho, Wo, total);
  return (int)hipGetLastError();
}

extern "C" int upnerf_lpips_dist(const upnerf_lpips_dist_args* a, double* scratch, void* stream) {
  if (!a || a->N < 1 || a->C < 1 || a->H < 1 || a->W < 1 || a->H > MAX_DIM || a->W > MAX_DIM) return UPNERF_EINVAL;
  if (!a->feat || !a->w || !a->out || !scratch) return UPNERF_EINVAL;
  const int64_t HW = (int64_t)a->H * a->W;
  const int64_t tiles = (HW + NTHREADS - 1) / NTHREADS;
  if (a->N * tiles > 0x7fffffffLL) return UPNERF_EUNSUP;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lpips_dist_kernel, dim3((unsigned)(a->N * tiles)), dim3(NTHREADS), 0, st, *a, HW, (int)tiles, scratch);
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(a->N), dim3(NTHREADS), 0, st, *a, HW, (int)tiles, (const double*)scratch);
  return (int)hipGetLastError();
}

extern "C" int upnerf_lpips_scratch(upnerf_lpips_scratch_args* a) {
  if (!a || a->N < 1 || a->H < 31 || a->W < 31 || a->H > MAX_DIM || a->W > MAX_DIM) return UPNERF_EINVAL;
  const int h0 = out_size(a->H, 11, 4, 2), w0 = out_size(a->W, 11, 4, 2);  // tap 0
  const int h1 = out_size(h0, 3, 2, 0), w1 = out_size(w0, 3, 2, 0);        // tap 1 (conv1 keeps the size)
  const int h2 = out_size(h1, 3, 2, 0), w2 = out_size(w1, 3, 2, 0);        // taps 2-4
  const int64_t s0 = (int64_t)h0 * w0, s1 = (int64_t)h1 * w1, s2 = (int64_t)h2 * w2;
  auto max3 = [](int64_t x, int64_t y, int64_t z) { return x > y ? (x > z ? x : z) : (y > z ? y : z); };
  // buffer 0: taps 0, 1, 2 and 4; buffer 1: the two pooled maps and tap 3 -- each map is read only while the other is written
  a->act0_elems = 2 * a->N * max3(64 * s0, 192 * s1, 384 * s2);
  a->act1_elems = 2 * a->N * max3(64 * s1, 192 * s2, 256 * s2);
  a->part_elems = a->N * ((s0 + NTHREADS - 1) / NTHREADS);
  return 0;
}
