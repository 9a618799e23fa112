// Surface normals from the analytic density gradient.
//
// upnerf_density_grad: sigma(x) and d sigma / d x of one field at arbitrary points, in ONE launch with no activation traffic.
// A workgroup owns a tile of 64 points.  Forward: BARF-masked encoding -> D trunk layers on the fp32 MFMA -> share_sigma ->
// softplus, the formulas and the summation order of csrc/field.hip (the skip layer contracts its encoding block first, then
// its activation block).  The tile's activations move layer to layer through LDS and are never stored; what the backward
// half needs of them is one bit per unit and layer (was the ReLU open?), kept in REGISTERS in the accumulator layout: the
// gradient of an activation is produced under the same wave tiling as the activation was, so every lane re-reads its own
// bits.  Backward: w_sig * softplus'(pre) through the transposed weight fragments (packing.frag_t_hip), masked layer by
// layer, the skip layer's encoding block added to layer 0's, then through the derivative of the encoding.
//
// LDS: the activation tile [64][W] (64 KiB at W = 256) + the encoding [64][64] (16 KiB, read three times: layer 0, the skip
// layer, the encoding's derivative; its pad column 63 carries softplus'(pre) once the trunk is done) = 80 KiB exactly: two
// workgroups per CU, as the field kernels run.
// Registers: accumulators 64 (W = 256: two 32 x 64 blocks per wave), the encoding gradient's 16, the masks 2 x D <= 16.
//
// upnerf_normal_composite: per-ray normal from per-sample gradients and compositing weights, one ray per wave.
#include "common.cuh"

#define NORMALS_TILE 64

namespace {

// dot of LDS row segment [0, K) with w, split over the TPR adjacent threads that share a row (as csrc/field.hip: the same order)
template <int TPR>
__device__ __forceinline__ float rowdot(const float* Hs, int ldw, int row, int part, int K, const float* __restrict__ w) {
  float s = 0.0f;
  const int kb = part * (K / TPR);
  for (int k = 0; k < K / TPR; k += 4) {
    const f32x4 a = *(const f32x4*)&Hs[swz4(row, kb + k, ldw)];
    const f32x4 ww = *(const f32x4*)&w[kb + k];
    s += a.x * ww.x + a.y * ww.y + a.z * ww.z + a.w * ww.w;
  }
#pragma unroll
  for (int d = 1; d < TPR; d <<= 1) s += __shfl_xor(s, d);
  return s;
}

template <int W>
__global__ __launch_bounds__(NTHREADS, (W == 256) ? 2 : 4) void density_grad_kernel(upnerf_layout L, upnerf_density_grad_args a) {
  constexpr int TILE = NORMALS_TILE;
  __shared__ __attribute__((aligned(16))) float Hs[TILE * W];          // activations, then their gradients
  __shared__ __attribute__((aligned(16))) float Xs[TILE * UPNERF_X0];  // the encoding x0 (swizzled, row stride 64)
  constexpr int TPR = NTHREADS / TILE;
  using TW = WaveTile<W, TILE>;
  using TX = WaveTile<UPNERF_X0, TILE>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.M, m0 = blockIdx.x * TILE, D = L.D;
  const float* __restrict__ P = a.P;
  const float* __restrict__ PT = a.PT;
  const int n0 = TW::n0(wave), row0 = TW::row0(wave);
  const int xn0 = TX::n0(wave), xrow0 = TX::row0(wave);

  // ---- the points; rows past M are evaluated at the origin and never stored
  if (tid < TILE) {
    const int m = m0 + tid;
    float x = 0.f, y = 0.f, zc = 0.f;
    if (m < M) {
      x = a.points[(size_t)m * 3 + 0];
      y = a.points[(size_t)m * 3 + 1];
      zc = a.points[(size_t)m * 3 + 2];
    }
    Xs[swz(tid, 0, UPNERF_X0)] = x;
    Xs[swz(tid, 1, UPNERF_X0)] = y;
    Xs[swz(tid, 2, UPNERF_X0)] = zc;
    Xs[swz(tid, 63, UPNERF_X0)] = 0.0f;
  }
  __syncthreads();
  // ---- BARF-masked encoding [x, sin(2^k pi x_n) w_k, cos(2^k pi x_n) w_k], band-major so that a wave's band is uniform
  static_assert((TILE * 3) % 64 == 0, "a wave's items share one band");
#pragma unroll 1
  for (int i0 = 64 * __builtin_amdgcn_readfirstlane(tid >> 6); i0 < TILE * 3 * 10; i0 += NTHREADS) {
    const int k = i0 / (TILE * 3);
    const int it = i0 + lane - k * (TILE * 3), row = it / 3, n = it - row * 3;
    const float wk = a.wk_xyz[k];
    float sv = 0.0f, cv = 0.0f;
    if (__builtin_amdgcn_readfirstlane(__float_as_uint(wk)) != 0u) {
      sincos_f32_via_f64(Xs[swz(row, n, UPNERF_X0)] * ldexpf(PI_F, k), sv, cv);
      sv *= wk;
      cv *= wk;
    }
    Xs[swz(row, 3 + 20 * n + k, UPNERF_X0)] = sv;
    Xs[swz(row, 3 + 20 * n + 10 + k, UPNERF_X0)] = cv;
  }
  __syncthreads();

  // ---- trunk, forward.  bits[] is indexed by compile-time constants only (select chains over the uniform l), so it stays in
  // registers while the layer loops stay rolled.
  unsigned long long bits[UPNERF_MAX_D];
#pragma unroll
  for (int j = 0; j < UPNERF_MAX_D; ++j) bits[j] = 0ull;
#pragma unroll 1
  for (int l = 0; l < D; ++l) {
    f32x16 acc[TW::MT][TW::NT];
    acc_zero(acc);
    if (l == 0) {
      mma_lds(acc, Xs, UPNERF_X0, row0, 0, P + L.w[0], UPNERF_X0, n0, 0, UPNERF_X0, lane);
    } else if (l == L.skip) {
      mma_lds(acc, Xs, UPNERF_X0, row0, 0, P + L.w[l], UPNERF_X0 + W, n0, 0, UPNERF_X0, lane);
      mma_lds(acc, Hs, W, row0, 0, P + L.w[l], UPNERF_X0 + W, n0, UPNERF_X0, W, lane);
    } else {
      mma_lds(acc, Hs, W, row0, 0, P + L.w[l], W, n0, 0, W, lane);
    }
    const unsigned long long nb = acc_bias_relu_pack(acc, P + L.b[l], n0, lane);
#pragma unroll
    for (int j = 0; j < UPNERF_MAX_D; ++j) bits[j] = (j == l) ? nb : bits[j];
    __syncthreads();
    acc_to_lds(acc, Hs, W, row0, n0, 0, lane);
    __syncthreads();
  }
  auto mask_of = [&](int l) {
    unsigned long long m = 0ull;
#pragma unroll
    for (int j = 0; j < UPNERF_MAX_D; ++j) m = (j == l) ? bits[j] : m;
    return m;
  };

  // ---- share_sigma + softplus; softplus'(x) = sigmoid(x), and 1 on the branch where softplus_f returns x itself
  {
    const int prow = tid / TPR, part = tid % TPR, pm = m0 + prow;
    const float pre = rowdot<TPR>(Hs, W, prow, part, W, P + L.wsig) + P[L.bsig];
    if (part == 0) {
      Xs[swz(prow, 63, UPNERF_X0)] = pre > 20.0f ? 1.0f : sigmoid_f(pre);  // (the pad column: no contraction reads Xs any more)
      if (pm < M) a.sigma[pm] = softplus_f(pre);
    }
  }
  __syncthreads();
  // ---- d h_{D-1} = w_sig * dpre, masked
  {
    f32x16 acc[TW::MT][TW::NT];
    acc_zero(acc);
    const float* __restrict__ ws = P + L.wsig;
    acc_map(acc, row0, n0, lane, [&](float, int row, int col) { return ws[col] * Xs[swz(row, 63, UPNERF_X0)]; });
    acc_apply_mask(acc, mask_of(D - 1));
    acc_to_lds(acc, Hs, W, row0, n0, 0, lane);
    __syncthreads();
  }
  // ---- trunk, last layer to first, through the transposed weights
  f32x16 accx[TX::MT][TX::NT];
  acc_zero(accx);
#pragma unroll 1
  for (int l = D - 1; l >= 1; --l) {
    if (l == L.skip) mma_lds(accx, Hs, W, xrow0, 0, PT + L.t_skipx, W, xn0, 0, W, lane);
    f32x16 acc[TW::MT][TW::NT];
    acc_zero(acc);
    mma_lds(acc, Hs, W, row0, 0, PT + L.t_w[l], W, n0, 0, W, lane);
    acc_apply_mask(acc, mask_of(l - 1));
    __syncthreads();
    acc_to_lds(acc, Hs, W, row0, n0, 0, lane);
    __syncthreads();
  }
  // ---- d x0 (first layer + skip) -> d x through the encoding:
  //      d/dx [w_k sin(2^k pi x)] = 2^k pi (w_k cos),  d/dx [w_k cos(2^k pi x)] = -2^k pi (w_k sin),  plus the identity block
  mma_lds(accx, Hs, W, xrow0, 0, PT + L.t_w[0], W, xn0, 0, W, lane);
  __syncthreads();
  acc_to_lds(accx, Hs, W, xrow0, xn0, 0, lane);
  __syncthreads();
  for (int it = tid; it < TILE * 3; it += NTHREADS) {
    const int row = it / 3, n = it - row * 3, m = m0 + row;
    if (m >= M) continue;
    float g = Hs[swz(row, n, W)];
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      const float f = ldexpf(PI_F, k);
      const float xs = Xs[swz(row, 3 + 20 * n + k, UPNERF_X0)], xc = Xs[swz(row, 3 + 20 * n + 10 + k, UPNERF_X0)];
      g += f * (xc * Hs[swz(row, 3 + 20 * n + k, W)] - xs * Hs[swz(row, 3 + 20 * n + 10 + k, W)]);
    }
    a.grad[(size_t)m * 3 + n] = g;
  }
}

// normal[r] = normalise(sum_i w_i * (-g_i / |g_i|)); a term is zero where |g_i| (fp32) is 0 or not finite or w_i is not finite;
// (0, 0, 0) where the sum's length is 0 or not finite.  One ray per wave: lane j sums samples j, j + 64, ... in ascending order,
// the lanes meet in a xor tree -- one fixed order.
__global__ __launch_bounds__(NTHREADS) void normal_composite_kernel(upnerf_normal_composite_args a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (NTHREADS / 64) + (threadIdx.x >> 6);
  if (r >= a.R) return;  // (wave-uniform)
  const int S = a.S;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int i = lane; i < S; i += 64) {
    const size_t m = (size_t)r * S + i;
    const float w = a.w[m];
    const float gx = a.grad[3 * m + 0], gy = a.grad[3 * m + 1], gz = a.grad[3 * m + 2];
    const float len = sqrtf(gx * gx + gy * gy + gz * gz);
    if (len > 0.f && len <= 3.402823466e38f && fabsf(w) <= 3.402823466e38f) {  // (comparisons are false for a NaN)
      const float s = -w / len;
      sx += s * gx;
      sy += s * gy;
      sz += s * gz;
    }
  }
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  sz = wave_sum(sz);
  if (lane == 0) {
    const float len = sqrtf(sx * sx + sy * sy + sz * sz);
    const bool ok = len > 0.f && len <= 3.402823466e38f;
    a.normal[(size_t)r * 3 + 0] = ok ? sx / len : 0.f;
    a.normal[(size_t)r * 3 + 1] = ok ? sy / len : 0.f;
    a.normal[(size_t)r * 3 + 2] = ok ? sz / len : 0.f;
  }
}

}  // namespace

extern "C" int upnerf_density_grad(const upnerf_layout* L, const upnerf_density_grad_args* a, void* stream) {
  if (!L) return UPNERF_EINVAL;
  if (L->W != 64 && L->W != 256) return UPNERF_EUNSUP;
  if (L->D < 1 || L->D > UPNERF_MAX_D) return UPNERF_EUNSUP;
  if (L->skip >= L->D) return UPNERF_EINVAL;
  if (!a || a->M <= 0 || !a->points || !a->P || !a->PT || !a->sigma || !a->grad) return UPNERF_EINVAL;
  const int grid = (int)(((long long)a->M + NORMALS_TILE - 1) / NORMALS_TILE);
  hipStream_t st = (hipStream_t)stream;
  if (L->W == 256) hipLaunchKernelGGL((density_grad_kernel<256>), dim3(grid), dim3(NTHREADS), 0, st, *L, *a);
  else hipLaunchKernelGGL((density_grad_kernel<64>), dim3(grid), dim3(NTHREADS), 0, st, *L, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_normal_composite(const upnerf_normal_composite_args* a, void* stream) {
  if (!a || a->R <= 0 || a->S <= 0 || !a->grad || !a->w || !a->normal) return UPNERF_EINVAL;
  if ((long long)a->R * a->S > 0x7fffffffLL) return UPNERF_EINVAL;
  const int wpb = NTHREADS / 64;
  hipLaunchKernelGGL(normal_composite_kernel, dim3((a->R + wpb - 1) / wpb), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}
