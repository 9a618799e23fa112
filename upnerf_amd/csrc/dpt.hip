// DPT-Large monocular inverse depth (upnerf_amd/dpt.py): what the convolutional decoder and the two resizes
// around the network need beside upnerf_linear and the ViT kernels of dino.hip.  Maps are NHWC: pixel (y, x) is the row
// (y * W + x) of a [H * W][C] matrix with a row stride, so the token rows of the backbone ARE maps and every 1 x 1 convolution
// is upnerf_linear.  Every kernel: no atomics, a fixed summation order, the same bits every run.
//   * upnerf_conv3x3: 3 x 3, pad 1, stride 1 or 2 as an implicit GEMM on v_mfma_f32_32x32x2_f32 (header comment at the kernel).
//   * upnerf_upsample2x: bilinear x 2, align_corners=True, torch's arithmetic.
//   * upnerf_depth_to_space: the scatter half of a transposed convolution whose kernel equals its stride, plus the bias.
//   * upnerf_resize_cubic: bicubic (A = -0.75, half-pixel centres, clamped taps), optional affine on the way out.
//   * upnerf_vit_patches16: the patch projection's operand rows for a general patch side, from an fp32 image.
#include "common.cuh"

namespace {

// ------------------------------------------------------------------------------------------------ conv3x3
// y[p][co] = [relu]( sum_{ky, kx, ci} f(x[(oy s - 1 + ky, ox s - 1 + kx)][ci]) w[co][ky][kx][ci] + bias[co] + res[p][co] ),
// f = relu or the identity, p = oy * Wo + ox.  As a GEMM: the C_out rows of the weight matrix [C_out][9 C_in] are the MFMA's A
// operand, the output pixels its B operand, K = 9 C_in runs tap by tap along contiguous channels.  C_in % 32 == 0, so a K chunk
// of 32 lies inside ONE tap: the (ky, kx) of a chunk is uniform, a pixel's 32 channels are 128 contiguous bytes, and the halo /
// zero padding is one comparison per pixel and chunk, made as the chunk is loaded for LDS.  No im2col buffer exists.
//
// A workgroup owns C3_BM = 128 output pixels x C3_BN = 64 output channels; wave w owns pixels [32 w, 32 w + 32) and both
// 32-channel tiles (two accumulators).  Per chunk the weights go to LDS as [co][k] and the gathered pixels as [pixel][k], both
// with row stride 36 floats (the 16 rows of a ds_read_b128 lane group start 4 banks apart: conflict-free, as in lpips.hip);
// the next chunk's global loads (6 x 16 bytes per thread) are issued before the 32 MFMAs of the current one.
// D[row = channel (r & 3) + 8 (r >> 2) + 4 hh][col = pixel li]: a lane holds, for ITS pixel, four runs of four consecutive
// channels per accumulator, so bias, residual and store are 16-byte accesses of an NHWC row.
// The K terms are ONE fp32 chain in the order (ky, kx, ci) (exact products, one rounding per term).
// Rows past the last pixel and channels past C_out (C_out % 64 == 32) are staged as zeros without a load and never stored.
// Resources: DESIGN.md 2.30.
#define C3_BM 128
#define C3_BN 64
#define C3_BK 32
#define C3_LD (C3_BK + 4)

__global__ __launch_bounds__(NTHREADS) void conv3x3_kernel(upnerf_conv3x3_args a, int Ho, int Wo, int M) {
  __shared__ __attribute__((aligned(16))) float Ws[C3_BN * C3_LD];
  __shared__ __attribute__((aligned(16))) float Xs[C3_BM * C3_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
  const int p0 = blockIdx.x * C3_BM, n0 = blockIdx.y * C3_BN;
  const int K = 9 * a.C_in, S = a.stride;

  // staging roles: the 16-byte piece g = tid & 7 of rows (tid >> 3) + 32 j: four pixel rows, two weight rows
  const int g4 = 4 * (tid & 7), r0 = tid >> 3;
  int iy0[4], ix0[4];  // top-left tap of each pixel this thread stages; a row past M gets iy0 = -4: every tap fails the test
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = p0 + r0 + 32 * j;
    const int oy = p / Wo, ox = p - oy * Wo;
    iy0[j] = p < M ? oy * S - 1 : -4;
    ix0[j] = ox * S - 1;
  }
  const float* wrow[2];
  bool wok[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = n0 + r0 + 32 * j;
    wok[j] = co < a.C_out;
    wrow[j] = a.w + (int64_t)(wok[j] ? co : 0) * K + g4;
  }

  f32x4 rx[4], rw[2];
  auto gload = [&](int kc) {
    const int tap = kc / a.C_in, c0 = kc - tap * a.C_in;
    const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      rw[j] = *(const f32x4*)&wrow[j][kc];  // (row 0 for a channel past C_out: in bounds, masked)
      if (!wok[j]) rw[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int iy = iy0[j] + ky, ix = ix0[j] + kx;
      const bool in = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      const int64_t row = in ? (int64_t)iy * a.W + ix : 0;  // an unconditional load of pixel 0, masked afterwards
      f32x4 v = *(const f32x4*)&a.x[row * a.ldx + c0 + g4];
      if (a.pre_relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];  // (a comparison that keeps a NaN, as torch.relu does)
      }
      rx[j] = in ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
  gload(0);
  for (int kc = 0; kc < K; kc += C3_BK) {
    __syncthreads();  // the previous chunk has been read
#pragma unroll
    for (int j = 0; j < 2; ++j) *(f32x4*)&Ws[(r0 + 32 * j) * C3_LD + g4] = rw[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) *(f32x4*)&Xs[(r0 + 32 * j) * C3_LD + g4] = rx[j];
    __syncthreads();
    if (kc + C3_BK < K) gload(kc + C3_BK);  // in flight under the 32 MFMAs below
#pragma unroll
    for (int t = 0; t < C3_BK / 8; ++t) {
      // lane half hh takes k = 8 t + 4 hh + q in MFMA q: a permutation of k inside the group of eight, the same for A and B
      const f32x4 w0 = *(const f32x4*)&Ws[li * C3_LD + 8 * t + 4 * hh];
      const f32x4 w1 = *(const f32x4*)&Ws[(32 + li) * C3_LD + 8 * t + 4 * hh];
      const f32x4 xv = *(const f32x4*)&Xs[(32 * wave + li) * C3_LD + 8 * t + 4 * hh];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[q], xv[q], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[q], xv[q], acc[1], 0, 0, 0);
      }
    }
  }

  const int p = p0 + 32 * wave + li;
  if (p >= M) return;  // (no barrier below)
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    if (n0 + 32 * mt >= a.C_out) break;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int co = n0 + 32 * mt + 8 * g + 4 * hh;
      f32x4 v = {acc[mt][4 * g], acc[mt][4 * g + 1], acc[mt][4 * g + 2], acc[mt][4 * g + 3]};
      if (a.bias) v += *(const f32x4*)&a.bias[co];
      if (a.res) v += *(const f32x4*)&a.res[(int64_t)p * a.ldr + co];
      if (a.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];
      }
      *(f32x4*)&a.y[(int64_t)p * a.ldy + co] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ upsample2x
// torch's upsample_bilinear2d with align_corners=True at scale 2: scale = (in - 1) / (out - 1) in fp32 (0 for in = 1),
// src = scale * dst, i0 = (int)src, i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1;
// out = l0y (l0x x00 + l1x x01) + l1y (l0x x10 + l1x x11).  V = 4: 16-byte accesses (C % 4 == 0), else element-wise.
template <int V>
__global__ __launch_bounds__(NTHREADS) void upsample2x_kernel(upnerf_upsample2x_args a, int Cv, float sy, float sx, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t pix = i / Cv;
  const int c = (int)(i - pix * Cv) * V;
  const int Wo = 2 * a.W;
  const int oy = (int)(pix / Wo), ox = (int)(pix - (int64_t)oy * Wo);
  const float fy = sy * (float)oy, fx = sx * (float)ox;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + 1 < a.H ? y0 + 1 : a.H - 1, x1 = x0 + 1 < a.W ? x0 + 1 : a.W - 1;
  const float ly1 = fy - (float)y0, lx1 = fx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  const float* p00 = a.x + ((int64_t)y0 * a.W + x0) * a.ldx + c;
  const float* p01 = a.x + ((int64_t)y0 * a.W + x1) * a.ldx + c;
  const float* p10 = a.x + ((int64_t)y1 * a.W + x0) * a.ldx + c;
  const float* p11 = a.x + ((int64_t)y1 * a.W + x1) * a.ldx + c;
  float* o = a.y + pix * a.ldy + c;
  if constexpr (V == 4) {
    const f32x4 v00 = *(const f32x4*)p00, v01 = *(const f32x4*)p01, v10 = *(const f32x4*)p10, v11 = *(const f32x4*)p11;
    *(f32x4*)o = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
  } else {
    *o = ly0 * (lx0 * *p00 + lx1 * *p01) + ly1 * (lx0 * *p10 + lx1 * *p11);
  }
}

// ------------------------------------------------------------------------------------------------ depth to space
// y[(py s + dy, px s + dx)][c] = x[(py, px)][(dy s + dx) C + c] + bias[c]: data movement and one add
template <int V>
__global__ __launch_bounds__(NTHREADS) void depth_to_space_kernel(upnerf_depth_to_space_args a, int Cv, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t pix = i / Cv;
  const int c = (int)(i - pix * Cv) * V;
  const int s = a.s, Wo = a.W * s;
  const int oy = (int)(pix / Wo), ox = (int)(pix - (int64_t)oy * Wo);
  const int py = oy / s, dy = oy - py * s, px = ox / s, dx = ox - px * s;
  const float* src = a.x + ((int64_t)py * a.W + px) * a.ldx + (dy * s + dx) * a.C + c;
  float* o = a.y + pix * a.ldy + c;
  if constexpr (V == 4) {
    f32x4 v = *(const f32x4*)src;
    if (a.bias) v += *(const f32x4*)&a.bias[c];
    *(f32x4*)o = v;
  } else {
    *o = a.bias ? *src + a.bias[c] : *src;
  }
}

// ------------------------------------------------------------------------------------------------ bicubic resize
// cubic convolution coefficients, A = -0.75 (cv2 INTER_CUBIC and torch's bicubic): taps at floor(src) - 1 .. floor(src) + 2
__device__ __forceinline__ void cubic_coeffs(float t, float (&w)[4]) {
  const float A = -0.75f;
  const float u = 1.f - t;
  w[0] = ((A * (t + 1.f) - 5.f * A) * (t + 1.f) + 8.f * A) * (t + 1.f) - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w[3] = ((A * (u + 1.f) - 5.f * A) * (u + 1.f) + 8.f * A) * (u + 1.f) - 4.f * A;
}

__global__ __launch_bounds__(NTHREADS) void resize_cubic_kernel(upnerf_resize_cubic_args a, float sy, float sx, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t pix = i / a.C;
  const int c = (int)(i - pix * a.C);
  const int oy = (int)(pix / a.W), ox = (int)(pix - (int64_t)oy * a.W);
  // half-pixel centres: src = (dst + 0.5) in / out - 0.5, not clamped; the TAPS are clamped (the border is replicated)
  const float fy = sy * ((float)oy + 0.5f) - 0.5f, fx = sx * ((float)ox + 0.5f) - 0.5f;
  const float yf = floorf(fy), xf = floorf(fx);
  const int y0 = (int)yf, x0 = (int)xf;
  float wy[4], wx[4];
  cubic_coeffs(fy - yf, wy);
  cubic_coeffs(fx - xf, wx);
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int yy = y0 - 1 + j;
    yy = yy < 0 ? 0 : (yy > a.h - 1 ? a.h - 1 : yy);
    float row = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int xx = x0 - 1 + k;
      xx = xx < 0 ? 0 : (xx > a.w - 1 ? a.w - 1 : xx);
      const int64_t e = ((int64_t)yy * a.w + xx) * a.C + c;
      const float v = a.u8 ? (float)((const uint8_t*)a.x)[e] / 255.0f : ((const float*)a.x)[e];
      row += wx[k] * v;
    }
    acc += wy[j] * row;
  }
  a.y[i] = a.affine ? (acc - a.mean[c]) / a.std[c] : acc;
}

// ------------------------------------------------------------------------------------------------ patches
// rows[t][(c P + ky) P + kx] = image[(ty P + ky, tx P + kx)][c]: the operand of a P x P, stride P patch convolution as a GEMM
__global__ __launch_bounds__(NTHREADS) void vit_patches16_kernel(upnerf_vit_patches16_args a, int w0, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= total) return;
  const int P = a.patch, PP = P * P;
  const int64_t t = i / (3 * PP);
  const int k = (int)(i - t * (3 * PP));
  const int c = k / PP, r = k - c * PP, ky = r / P, kx = r - ky * P;
  const int ty = (int)(t / w0), tx = (int)(t - (int64_t)ty * w0);
  a.rows[i] = a.image[((int64_t)(ty * P + ky) * a.W + (tx * P + kx)) * 3 + c];
}

const int DPT_MAX_SIDE = 32768;
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int64_t nblocks(int64_t n) { return (n + NTHREADS - 1) / NTHREADS; }
// do the byte ranges of two row-strided fp32 maps ([rows][cols], row stride ld) overlap?
bool overlap(const float* p, int64_t rows, int64_t ld, int64_t cols, const float* q, int64_t rows2, int64_t ld2, int64_t cols2) {
  const uintptr_t p0 = (uintptr_t)p, p1 = p0 + 4 * ((rows - 1) * ld + cols);
  const uintptr_t q0 = (uintptr_t)q, q1 = q0 + 4 * ((rows2 - 1) * ld2 + cols2);
  return p0 < q1 && q0 < p1;
}

}  // namespace

extern "C" int upnerf_conv3x3(const upnerf_conv3x3_args* a, void* stream) {
  if (!a || a->H < 1 || a->W < 1 || a->H > DPT_MAX_SIDE || a->W > DPT_MAX_SIDE || a->C_in < 1 || a->C_out < 1) return UPNERF_EINVAL;
  if (!a->x || !a->w || !a->y) return UPNERF_EINVAL;
  if (a->stride != 1 && a->stride != 2) return UPNERF_EUNSUP;
  if ((a->C_in & 31) || (a->C_out & 31) || a->C_in > 1024 || a->C_out > 1024) return UPNERF_EUNSUP;
  if (a->ldx < a->C_in || a->ldy < a->C_out || (a->ldx & 3) || (a->ldy & 3) || !aligned16(a->x) || !aligned16(a->y) ||
      !aligned16(a->w))
    return UPNERF_EINVAL;
  if (a->bias && !aligned16(a->bias)) return UPNERF_EINVAL;
  const int Ho = (a->H - 1) / a->stride + 1, Wo = (a->W - 1) / a->stride + 1;
  const int64_t M = (int64_t)Ho * Wo, Min = (int64_t)a->H * a->W;
  if (M > 0x7fffffffLL - C3_BM) return UPNERF_EUNSUP;
  if (overlap(a->x, Min, a->ldx, a->C_in, a->y, M, a->ldy, a->C_out)) return UPNERF_EINVAL;
  if (a->res) {
    if (a->ldr < a->C_out || (a->ldr & 3) || !aligned16(a->res)) return UPNERF_EINVAL;
    if (overlap(a->res, M, a->ldr, a->C_out, a->y, M, a->ldy, a->C_out) ||
        overlap(a->res, M, a->ldr, a->C_out, a->x, Min, a->ldx, a->C_in))
      return UPNERF_EINVAL;
  }
  const dim3 grid((unsigned)((M + C3_BM - 1) / C3_BM), (unsigned)((a->C_out + C3_BN - 1) / C3_BN));
  hipLaunchKernelGGL(conv3x3_kernel, grid, dim3(NTHREADS), 0, (hipStream_t)stream, *a, Ho, Wo, (int)M);
  return (int)hipGetLastError();
}

extern "C" int upnerf_upsample2x(const upnerf_upsample2x_args* a, void* stream) {
  if (!a || a->H < 1 || a->W < 1 || a->H > DPT_MAX_SIDE / 2 || a->W > DPT_MAX_SIDE / 2 || a->C < 1 || !a->x || !a->y ||
      a->ldx < a->C || a->ldy < a->C)
    return UPNERF_EINVAL;
  const int64_t Min = (int64_t)a->H * a->W, M = 4 * Min;
  if (overlap(a->x, Min, a->ldx, a->C, a->y, M, a->ldy, a->C)) return UPNERF_EINVAL;
  const bool vec = !(a->C & 3) && !(a->ldx & 3) && !(a->ldy & 3) && aligned16(a->x) && aligned16(a->y);
  const int Cv = vec ? a->C / 4 : a->C;
  const int64_t total = M * Cv;
  if (nblocks(total) > 0x7fffffffLL) return UPNERF_EUNSUP;
  // torch's area_pixel_compute_scale for align_corners=True: (in - 1) / (out - 1), out = 2 in >= 2
  const float sy = (float)(a->H - 1) / (float)(2 * a->H - 1), sx = (float)(a->W - 1) / (float)(2 * a->W - 1);
  const dim3 grid((unsigned)nblocks(total));
  if (vec)
    hipLaunchKernelGGL(upsample2x_kernel<4>, grid, dim3(NTHREADS), 0, (hipStream_t)stream, *a, Cv, sy, sx, total);
  else
    hipLaunchKernelGGL(upsample2x_kernel<1>, grid, dim3(NTHREADS), 0, (hipStream_t)stream, *a, Cv, sy, sx, total);
  return (int)hipGetLastError();
}

extern "C" int upnerf_depth_to_space(const upnerf_depth_to_space_args* a, void* stream) {
  if (!a || a->H < 1 || a->W < 1 || a->H > DPT_MAX_SIDE / 4 || a->W > DPT_MAX_SIDE / 4 || a->C < 1 || !a->x || !a->y)
    return UPNERF_EINVAL;
  if (a->s != 2 && a->s != 4) return UPNERF_EUNSUP;
  const int64_t cin = (int64_t)a->s * a->s * a->C;
  if (cin > 0x7fffffffLL || a->ldx < cin || a->ldy < a->C) return UPNERF_EINVAL;
  const int64_t Min = (int64_t)a->H * a->W, M = Min * a->s * a->s;
  if (overlap(a->x, Min, a->ldx, cin, a->y, M, a->ldy, a->C)) return UPNERF_EINVAL;
  const bool vec = !(a->C & 3) && !(a->ldx & 3) && !(a->ldy & 3) && aligned16(a->x) && aligned16(a->y) &&
                   (!a->bias || aligned16(a->bias));
  const int Cv = vec ? a->C / 4 : a->C;
  const int64_t total = M * Cv;
  if (nblocks(total) > 0x7fffffffLL) return UPNERF_EUNSUP;
  const dim3 grid((unsigned)nblocks(total));
  if (vec)
    hipLaunchKernelGGL(depth_to_space_kernel<4>, grid, dim3(NTHREADS), 0, (hipStream_t)stream, *a, Cv, total);
  else
    hipLaunchKernelGGL(depth_to_space_kernel<1>, grid, dim3(NTHREADS), 0, (hipStream_t)stream, *a, Cv, total);
  return (int)hipGetLastError();
}

extern "C" int upnerf_resize_cubic(const upnerf_resize_cubic_args* a, void* stream) {
  if (!a || a->h < 1 || a->w < 1 || a->H < 1 || a->W < 1 || a->h > DPT_MAX_SIDE || a->w > DPT_MAX_SIDE || a->H > DPT_MAX_SIDE ||
      a->W > DPT_MAX_SIDE || !a->x || !a->y)
    return UPNERF_EINVAL;
  if (a->C != 1 && a->C != 3) return UPNERF_EUNSUP;
  if (a->affine)
    for (int c = 0; c < a->C; ++c)
      if (!(a->std[c] > 0.f)) return UPNERF_EINVAL;
  const int64_t total = (int64_t)a->H * a->W * a->C;
  // torch's area_pixel_compute_scale for align_corners=False without a given scale factor: in / out in fp32
  const float sy = (float)a->h / (float)a->H, sx = (float)a->w / (float)a->W;
  hipLaunchKernelGGL(resize_cubic_kernel, dim3((unsigned)nblocks(total)), dim3(NTHREADS), 0, (hipStream_t)stream, *a, sy, sx, total);
  return (int)hipGetLastError();
}

extern "C" int upnerf_vit_patches16(const upnerf_vit_patches16_args* a, void* stream) {
  if (!a || !a->image || !a->rows || a->patch < 1 || a->patch > 64 || a->H < a->patch || a->W < a->patch || a->H > DPT_MAX_SIDE ||
      a->W > DPT_MAX_SIDE)
    return UPNERF_EINVAL;
  const int h0 = a->H / a->patch, w0 = a->W / a->patch;
  const int64_t total = (int64_t)h0 * w0 * 3 * a->patch * a->patch;
  if (nblocks(total) > 0x7fffffffLL) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(vit_patches16_kernel, dim3((unsigned)nblocks(total)), dim3(NTHREADS), 0, (hipStream_t)stream, *a, w0, total);
  return (int)hipGetLastError();
}
