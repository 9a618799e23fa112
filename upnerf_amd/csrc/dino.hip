// DINO ViT descriptors (upnerf_amd/dino.py): what a pre-norm vision transformer needs beside upnerf_linear, and
// the moments of the descriptor PCA.  Every kernel: no atomics, a fixed summation order, the same bits every run.
//   * upnerf_vit_patches: the patch convolution's operand rows gathered from the image, normalised on the way.
//   * upnerf_vit_embed: the class row and the position rows.
//   * upnerf_layernorm: one wave per row, the row in registers, mean and centred variance in fp64.
//   * upnerf_vit_attention: streaming-softmax attention on v_mfma_f32_32x32x2_f32 (header comment at the kernel).
//   * upnerf_vit_gelu, upnerf_vit_residual: elementwise.
//   * upnerf_pca_fit: L2-normalised rows -> column mean and centred Gram matrix, fp64 partials per chunk, fixed-order finish.
#include "common.cuh"

namespace {

// ------------------------------------------------------------------------------------------------ patches, embed
#define VP_K (3 * UPNERF_VIT_PATCH * UPNERF_VIT_PATCH)  // 192

__global__ __launch_bounds__(NTHREADS) void vit_patches_kernel(upnerf_vit_patches_args a, int w0, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= total) return;
  const int64_t t = i / VP_K;
  const int k = (int)(i - t * VP_K);
  const int c = k >> 6, ky = (k >> 3) & 7, kx = k & 7;
  const int ty = (int)(t / w0), tx = (int)(t - (int64_t)ty * w0);
  const int64_t pix = ((int64_t)(ty * a.stride + ky) * a.W + (tx * a.stride + kx)) * 3 + c;
  // ToTensor then Normalize: fp32 steps, each rounded on its own (a division and a subtraction: nothing to contract)
  const float v = a.u8 ? (float)((const uint8_t*)a.image)[pix] / 255.0f : ((const float*)a.image)[pix];
  a.rows[i] = (v - a.mean[c]) / a.std[c];
}

__global__ __launch_bounds__(NTHREADS) void vit_embed_kernel(int64_t total, int D, const float* __restrict__ cls,
                                                             const float* __restrict__ pos, float* __restrict__ tok) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= total) return;
  tok[i] = (i < D ? cls[i] : tok[i]) + pos[i];
}

// ------------------------------------------------------------------------------------------------ layer norm
// One wave per row: lane l holds the 16-byte pieces l, l + 64, l + 128, l + 192 of the row (D <= 1024).  The sum and the sum of
// squared centred values are fp64: a row of mean 1e4 and spread 1 loses its mean to ~1e-3 in an fp32 sum, which is the whole
// output.  A constant row gives centred values of exactly 0 and so exactly beta.
__global__ __launch_bounds__(NTHREADS) void layernorm_kernel(int M, int D, const float* x, int64_t ldx,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float eps, float* y, int64_t ldy) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * (NTHREADS / 64) + (threadIdx.x >> 6);
  if (m >= M) return;  // (whole waves leave; no barrier below)
  const int G = D >> 2;
  const float* xr = x + m * ldx;
  f32x4 v[4];
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int g = lane + 64 * j;
    v[j] = g < G ? *(const f32x4*)&xr[4 * g] : f32x4{0.f, 0.f, 0.f, 0.f};
    s += ((double)v[j][0] + (double)v[j][1]) + ((double)v[j][2] + (double)v[j][3]);
  }
  const double mean = wave_sum_f64(s) / (double)D;
  double q = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool in = lane + 64 * j < G;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = in ? (double)v[j][e] - mean : 0.0;
      v[j][e] = (float)d;
      q += d * d;
    }
  }
  const float rstd = (float)(1.0 / sqrt(wave_sum_f64(q) / (double)D + (double)eps));
  float* yr = y + m * ldy;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int g = lane + 64 * j;
    if (g < G) {
      const f32x4 ga = *(const f32x4*)&gamma[4 * g], be = *(const f32x4*)&beta[4 * g];
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = v[j][e] * rstd * ga[e] + be[e];
      *(f32x4*)&yr[4 * g] = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------ attention
// out[n][h] = softmax_j(scale q_n . k_j) v_j for one head of width 64, streaming (FlashAttention-style online softmax): a
// workgroup owns AT_BQ = 128 query rows of one head, a wave 32 of them; key / value tiles of AT_BK = 64 rows go through LDS
// once per workgroup and are shared by its four waves.  Nothing of size N x N exists.
//
// Both products are fp32-input MFMAs (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate), the route of gemm.hip
// and lpips.hip.  The scores are computed TRANSPOSED, S^T[key][query] = K . Q^T, so that a lane's 16 accumulator registers are
// 16 keys of ONE query (query = lane & 31, keys (r & 3) + 8 (r >> 2) + 4 (lane >> 5)): the row maximum and the row sum are a
// loop over registers and one exchange between the two lane halves, the running maximum, sum and rescale factor are one
// value per lane, and the probabilities are already where the second product wants them: O^T[d][query] = V^T . P^T takes
// B[k = lane >> 5][j = lane & 31] from the very register the first product left there, if MFMA step s contracts the keys
// (s & 3) + 8 (s >> 2) + 4 (lane >> 5) -- a permutation of the key order inside the subtile, the same for A (the V row read)
// and B.  P never goes through LDS or a shuffle.  The queries (pre-multiplied by scale) stay in 32 registers for the whole
// kernel, O^T in 32 accumulators.
//
// LDS: Ks, Vs [64][68] fp32 = 2 x 17 408 = 34 816 bytes per workgroup (row stride 68: the 16 rows of a ds_read_b128 lane
// group start 4 banks apart, conflict-free; the V reads are ds_read_b32 of 32 consecutive floats).  The next tile's global
// loads are issued before the products of the current one and held in 8 x 16 bytes of registers.
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): 197 VGPRs, 0 AGPRs, no spills, 34 816 bytes of LDS:
// 2 waves per SIMD by registers (176-256 allocated), i.e. 2 workgroups per CU; LDS alone would allow 4.  The fp16 3-term
// split of DESIGN.md 2.4 was not built for this kernel (DESIGN.md 2.29 says why and what was measured).
//
// Masking: key rows >= N are staged as zeros (V too: 0 x garbage could be NaN) and their scores set to -inf before the
// maximum; key 0 is always valid, so the running maximum is finite from the first subtile on.  Query rows >= N are computed
// on a clamped row (each query is one lane's column: it enters nobody else's sums) and not stored.
#define AT_BQ 128
#define AT_BK 64
#define AT_LD 68

__global__ __launch_bounds__(NTHREADS, 2) void vit_attention_kernel(upnerf_vit_attention_args a) {
  __shared__ __attribute__((aligned(16))) float Ks[AT_BK * AT_LD];
  __shared__ __attribute__((aligned(16))) float Vs[AT_BK * AT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
  const int N = a.N, head = blockIdx.y;
  const int qrow = blockIdx.x * AT_BQ + wave * 32 + li;
  const float* __restrict__ kp = a.k + head * 64;
  const float* __restrict__ vp = a.v + head * 64;

  // this lane's query: d = 8 t + 4 hh + e in qv[t][e], the k order of the first product's MFMAs (as in lpips.hip)
  f32x4 qv[8];
  {
    const float* qp = a.q + (int64_t)(qrow < N ? qrow : N - 1) * a.ldq + head * 64 + 4 * hh;
#pragma unroll
    for (int t = 0; t < 8; ++t) qv[t] = *(const f32x4*)&qp[8 * t] * a.scale;
  }

  // staging: 16-byte piece g = idx & 15 of key row idx >> 4, idx = tid + 256 j
  f32x4 rk[4], rv[4];
  auto gload = [&](int key0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = tid + NTHREADS * j;
      const int row = key0 + (idx >> 4), g = idx & 15;
      const int64_t rc = row < N ? row : N - 1;  // unconditional loads of a clamped row, masked afterwards
      rk[j] = *(const f32x4*)&kp[rc * a.ldk + 4 * g];
      rv[j] = *(const f32x4*)&vp[rc * a.ldv + 4 * g];
      if (row >= N) rk[j] = rv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  f32x16 o[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) o[0][r] = o[1][r] = 0.f;
  float mrun = -INFINITY, lrun = 0.f;

  gload(0);
  for (int key0 = 0; key0 < N; key0 += AT_BK) {
    __syncthreads();  // the previous tile has been read
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = tid + NTHREADS * j;
      *(f32x4*)&Ks[(idx >> 4) * AT_LD + 4 * (idx & 15)] = rk[j];
      *(f32x4*)&Vs[(idx >> 4) * AT_LD + 4 * (idx & 15)] = rv[j];
    }
    __syncthreads();
    if (key0 + AT_BK < N) gload(key0 + AT_BK);  // in flight under the products below

#pragma unroll 1
    for (int sub = 0; sub < AT_BK; sub += 32) {
      if (key0 + sub >= N) break;  // (uniform) a subtile without a valid key
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const f32x4 kv = *(const f32x4*)&Ks[(sub + li) * AT_LD + 8 * t + 4 * hh];
#pragma unroll
        for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[e], qv[t][e], s, 0, 0, 0);
      }
      // s[r] = score of key key0 + sub + (r & 3) + 8 (r >> 2) + 4 hh against this lane's query
      const int kbase = key0 + sub + 4 * hh;
      float mloc = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (kbase + (r & 3) + 8 * (r >> 2) >= N) s[r] = -INFINITY;
        mloc = fmaxf(mloc, s[r]);
      }
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
      const float mnew = fmaxf(mrun, mloc);
      const float alpha = expf(mrun - mnew);  // 0 on the first subtile (mrun = -inf, mnew finite)
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = expf(s[r] - mnew);
        ps += s[r];
      }
      ps += __shfl_xor(ps, 32);  // (a + b in both halves: the same bits)
      lrun = lrun * alpha + ps;
      mrun = mnew;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o[0][r] *= alpha;
        o[1][r] *= alpha;
      }
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const float* vr = &Vs[(sub + (st & 3) + 8 * (st >> 2) + 4 * hh) * AT_LD + li];
        o[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], s[st], o[0], 0, 0, 0);
        o[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], s[st], o[1], 0, 0, 0);
      }
    }
  }

  // o[dt][r] = O[query][d = 32 dt + (r & 3) + 8 (r >> 2) + 4 hh]: four consecutive d per group of registers
  if (qrow < N) {
    const float inv = 1.0f / lrun;
    float* op = a.out + (int64_t)qrow * a.ldo + head * 64 + 4 * hh;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 w = {o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv, o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv};
        *(f32x4*)&op[32 * dt + 8 * g] = w;
      }
  }
}

// ------------------------------------------------------------------------------------------------ elementwise
__global__ __launch_bounds__(NTHREADS) void vit_gelu_kernel(float* __restrict__ x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i >= n) return;
  // x Phi(x) with Phi(x) = erfc(-x / sqrt 2) / 2: the same function as x (1 + erf(x / sqrt 2)) / 2 without the cancellation
  // in 1 + erf at negative x
  const float v = x[i];
  x[i] = 0.5f * v * erfcf(-v * 0.70710678118654752440f);
}

__global__ __launch_bounds__(NTHREADS) void vit_residual_kernel(float* __restrict__ x, const float* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (i < n) x[i] += y[i];
}

// ------------------------------------------------------------------------------------------------ PCA moments
#define PCA_CH 1024  // rows per chunk (one fp64 partial per chunk)
#define PCA_TB 16    // Gram tile side per workgroup: one element per thread

// one wave per row: inv[t] = 1 / |x_t| in fp64
__global__ __launch_bounds__(NTHREADS) void pca_norm_kernel(upnerf_pca_fit_args a, double* __restrict__ inv) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (NTHREADS / 64) + (threadIdx.x >> 6);
  if (t >= a.T) return;
  const float* xr = a.x + t * a.ldx;
  double s = 0.0;
  for (int c = lane; c < a.D; c += 64) s += (double)xr[c] * (double)xr[c];
  s = wave_sum_f64(s);
  if (lane == 0) inv[t] = 1.0 / sqrt(s);
}

// pm[chunk][c] = sum over the chunk's rows, in row order, of x[t][c] inv[t]
__global__ __launch_bounds__(NTHREADS) void pca_colsum_kernel(upnerf_pca_fit_args a, const double* __restrict__ inv,
                                                              double* __restrict__ pm) {
  const int c = blockIdx.y * NTHREADS + threadIdx.x;
  if (c >= a.D) return;
  const int t0 = blockIdx.x * PCA_CH, t1 = t0 + PCA_CH < a.T ? t0 + PCA_CH : a.T;
  double s = 0.0;
  for (int t = t0; t < t1; ++t) s += (double)a.x[(int64_t)t * a.ldx + c] * inv[t];
  pm[(int64_t)blockIdx.x * a.D + c] = s;
}

__global__ __launch_bounds__(NTHREADS) void pca_mean_kernel(upnerf_pca_fit_args a, int nch, const double* __restrict__ pm,
                                                            double* __restrict__ mean64) {
  const int c = blockIdx.x * NTHREADS + threadIdx.x;
  if (c >= a.D) return;
  double s = 0.0;
  for (int j = 0; j < nch; ++j) s += pm[(int64_t)j * a.D + c];
  s /= (double)a.T;
  mean64[c] = s;
  a.mean[c] = (float)s;
}

// pg[chunk][i][j] = sum over the chunk's rows, in row order, of (u_t[i] - mean[i]) (u_t[j] - mean[j]), a 16 x 16 tile per workgroup
__global__ __launch_bounds__(NTHREADS) void pca_gram_kernel(upnerf_pca_fit_args a, const double* __restrict__ inv,
                                                            const double* __restrict__ mean64, double* __restrict__ pg) {
  __shared__ double xi[64][PCA_TB + 1], xj[64][PCA_TB + 1];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int i0 = blockIdx.y * PCA_TB, j0 = blockIdx.z * PCA_TB;
  const int t0 = blockIdx.x * PCA_CH, t1 = t0 + PCA_CH < a.T ? t0 + PCA_CH : a.T;
  double acc = 0.0;
  for (int tb = t0; tb < t1; tb += 64) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = (tid >> 4) + 16 * q, c = tid & 15, t = tb + r;
      double vi = 0.0, vj = 0.0;  // rows past the chunk and columns past D add 0
      if (t < t1) {
        const double w = inv[t];
        if (i0 + c < a.D) vi = (double)a.x[(int64_t)t * a.ldx + i0 + c] * w - mean64[i0 + c];
        if (j0 + c < a.D) vj = (double)a.x[(int64_t)t * a.ldx + j0 + c] * w - mean64[j0 + c];
      }
      xi[r][c] = vi;
      xj[r][c] = vj;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < 64; ++r) acc += xi[r][ti] * xj[r][tj];
  }
  if (i0 + ti < a.D && j0 + tj < a.D) pg[((int64_t)blockIdx.x * a.D + i0 + ti) * a.D + j0 + tj] = acc;
}

__global__ __launch_bounds__(NTHREADS) void pca_gram_finish_kernel(upnerf_pca_fit_args a, int nch, const double* __restrict__ pg) {
  const int64_t e = (int64_t)blockIdx.x * NTHREADS + threadIdx.x, DD = (int64_t)a.D * a.D;
  if (e >= DD) return;
  double s = 0.0;
  for (int j = 0; j < nch; ++j) s += pg[(int64_t)j * DD + e];
  a.gram[e] = s;
}

const int VIT_MAX_SIDE = 32768;
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int64_t nblocks(int64_t n) { return (n + NTHREADS - 1) / NTHREADS; }

}  // namespace

extern "C" int upnerf_vit_patches(const upnerf_vit_patches_args* a, void* stream) {
  if (!a || !a->image || !a->rows || a->stride < 1 || a->H < UPNERF_VIT_PATCH || a->W < UPNERF_VIT_PATCH ||
      a->H > VIT_MAX_SIDE || a->W > VIT_MAX_SIDE)
    return UPNERF_EINVAL;
  for (int c = 0; c < 3; ++c)
    if (!(a->std[c] > 0.f)) return UPNERF_EINVAL;
  const int h0 = 1 + (a->H - UPNERF_VIT_PATCH) / a->stride, w0 = 1 + (a->W - UPNERF_VIT_PATCH) / a->stride;
  const int64_t total = (int64_t)h0 * w0 * VP_K;
  if (nblocks(total) > 0x7fffffffLL) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(vit_patches_kernel, dim3((unsigned)nblocks(total)), dim3(NTHREADS), 0, (hipStream_t)stream, *a, w0, total);
  return (int)hipGetLastError();
}

extern "C" int upnerf_vit_embed(int N, int D, const float* cls, const float* pos, float* tok, void* stream) {
  if (N < 1 || D < 1 || !cls || !pos || !tok) return UPNERF_EINVAL;
  const int64_t total = (int64_t)N * D;
  if (nblocks(total) > 0x7fffffffLL) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(vit_embed_kernel, dim3((unsigned)nblocks(total)), dim3(NTHREADS), 0, (hipStream_t)stream, total, D, cls, pos,
                     tok);
  return (int)hipGetLastError();
}

extern "C" int upnerf_layernorm(int M, int D, const float* x, int ldx, const float* gamma, const float* beta, float eps, float* y,
                                int ldy, void* stream) {
  if (M < 1 || D < 1 || !x || !gamma || !beta || !y || ldx < D || ldy < D || !(eps >= 0.f)) return UPNERF_EINVAL;
  if (D > 1024 || (D & 3)) return UPNERF_EUNSUP;
  if ((ldx & 3) || (ldy & 3) || !aligned16(x) || !aligned16(y) || !aligned16(gamma) || !aligned16(beta)) return UPNERF_EINVAL;
  hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)((M + 3) / 4)), dim3(NTHREADS), 0, (hipStream_t)stream, M, D, x,
                     (int64_t)ldx, gamma, beta, eps, y, (int64_t)ldy);
  return (int)hipGetLastError();
}

extern "C" int upnerf_vit_attention(const upnerf_vit_attention_args* a, void* stream) {
  if (!a || a->N < 1 || a->heads < 1 || a->heads > 65535 || !a->q || !a->k || !a->v || !a->out) return UPNERF_EINVAL;
  if (a->head_dim != UPNERF_VIT_HEAD_DIM) return UPNERF_EUNSUP;
  const int64_t w = (int64_t)a->heads * UPNERF_VIT_HEAD_DIM;
  if (a->ldq < w || a->ldk < w || a->ldv < w || a->ldo < w || ((a->ldq | a->ldk | a->ldv | a->ldo) & 3)) return UPNERF_EINVAL;
  if (!aligned16(a->q) || !aligned16(a->k) || !aligned16(a->v) || !aligned16(a->out)) return UPNERF_EINVAL;
  const dim3 grid((unsigned)((a->N + AT_BQ - 1) / AT_BQ), (unsigned)a->heads);
  hipLaunchKernelGGL(vit_attention_kernel, grid, dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_vit_gelu(float* x, long long n, void* stream) {
  if (!x || n < 1) return UPNERF_EINVAL;
  if (nblocks(n) > 0x7fffffffLL) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(vit_gelu_kernel, dim3((unsigned)nblocks(n)), dim3(NTHREADS), 0, (hipStream_t)stream, x, (int64_t)n);
  return (int)hipGetLastError();
}

extern "C" int upnerf_vit_residual(float* x, const float* y, long long n, void* stream) {
  if (!x || !y || n < 1) return UPNERF_EINVAL;
  if (nblocks(n) > 0x7fffffffLL) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(vit_residual_kernel, dim3((unsigned)nblocks(n)), dim3(NTHREADS), 0, (hipStream_t)stream, x, y, (int64_t)n);
  return (int)hipGetLastError();
}

// scratch (doubles): inv [T] | mean64 [D] | pm [nch][D] | pg [nch][D][D]
extern "C" long long upnerf_pca_fit_scratch(int T, int D) {
  if (T < 1 || D < 1 || D > 1024) return UPNERF_EINVAL;
  const long long nch = ((long long)T + PCA_CH - 1) / PCA_CH;
  return (long long)T + D + nch * D + nch * D * D;
}

extern "C" int upnerf_pca_fit(const upnerf_pca_fit_args* a, double* scratch, void* stream) {
  if (!a || a->T < 1 || a->D < 1 || !a->x || !a->mean || !a->gram || !scratch || a->ldx < a->D) return UPNERF_EINVAL;
  if (a->D > 1024) return UPNERF_EUNSUP;
  const int nch = (a->T + PCA_CH - 1) / PCA_CH, D = a->D, tiles = (D + PCA_TB - 1) / PCA_TB;
  double* inv = scratch;
  double* mean64 = inv + a->T;
  double* pm = mean64 + D;
  double* pg = pm + (int64_t)nch * D;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pca_norm_kernel, dim3((unsigned)((a->T + 3) / 4)), dim3(NTHREADS), 0, st, *a, inv);
  hipLaunchKernelGGL(pca_colsum_kernel, dim3(nch, (D + NTHREADS - 1) / NTHREADS), dim3(NTHREADS), 0, st, *a, (const double*)inv, pm);
  hipLaunchKernelGGL(pca_mean_kernel, dim3((D + NTHREADS - 1) / NTHREADS), dim3(NTHREADS), 0, st, *a, nch, (const double*)pm, mean64);
  hipLaunchKernelGGL(pca_gram_kernel, dim3(nch, tiles, tiles), dim3(NTHREADS), 0, st, *a, (const double*)inv, (const double*)mean64,
                     pg);
  hipLaunchKernelGGL(pca_gram_finish_kernel, dim3((unsigned)nblocks((int64_t)D * D)), dim3(NTHREADS), 0, st, *a, nch,
                     (const double*)pg);
  return (int)hipGetLastError();
}
