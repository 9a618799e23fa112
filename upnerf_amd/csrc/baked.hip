// A baked scene: the static field sampled once into a colour-density grid (r, g, b, sigma per grid point, 16 bytes), and rays
// marched through that grid without touching the field (include/upnerf_hip.h states the arithmetic).
//   upnerf_baked_pack    sigma [n] and rgb [n][3] -> rgbs [n][4]; a point whose sigma is below the level, not positive or not
//                        finite becomes (0, 0, 0, 0), so a cell none of whose corners kept a sigma holds eight exact zeros.
//   upnerf_baked_render  one thread per ray, one wave per workgroup (a chunk of 16 384 rays is 256 workgroups: one per CU).  The
//                        samples sit on a lattice the ray alone fixes, t_k = fmaf(k + 0.5, step, near): every sample is computed
//                        from its index.  Every fp32 operation between k and the grid coordinate g is monotone (a rounding never
//                        reverses an order), so g is monotone in k on every axis -- and with it the cell, the brick and the side
//                        of the box a sample falls on.  Skipping rests on that alone: where sample k lies in an empty region (outside
//                        the box on one axis; a brick with a clear bit; a cell with a clear bit), a later sample k' is PROPOSED
//                        from the plane through which the ray leaves the region, and the jump is taken only if sample k', located
//                        by the same arithmetic as any sample, lies in the SAME region: then so does every sample between them.  A
//                        refused proposal costs one step.  No span, no epsilon, nothing a rounding could move across an edge: the
//                        picture is, bit for bit, the one that visits every sample (tests/test_hip_baked.py runs both).
//                        A visited sample reads its eight corners as eight 16-byte loads; the rays of a wave are 64 neighbouring
//                        pixels of an image row and read neighbouring corners.  All per-ray state is in registers; no LDS.
//   upnerf_baked_sh_render  the same march (ONE template, baked_march<DEG, SPARSE>) through records that hold, per grid point, the fp16
//                        coefficients of a spherical-harmonic expansion of the colour over direction and a fp32 sigma (32 bytes at
//                        degree 1, 64 at degree 2).  The basis of the ray's direction is formed once per ray and
//                        kept in registers; a corner is reduced to (r, g, b, sigma) as it is read -- nb fmas per channel -- so the
//                        blend sees the four floats per corner it sees at degree 0.  Degree 0 is the instantiation that reads rgbs.
//   upnerf_baked_sparse_render  the same march again through a brick pool (brick.hip): the template's second
//                        parameter is the layout, and all three entry points fill one BakedArgs.  Where the dense march tests a sample's brick bit, the sparse one reads the
//                        brick's slot (< 0: the empty brick), and the eight corners are base, + 1, + 9, + 81 inside that slot.
//   upnerf_sh_accumulate, upnerf_baked_sh_pack  the projection's running sum over directions, and the records from it.
//   upnerf_baked_render_bwd  the gradient of a dense scene's render with respect to its points: one thread per
//                        ray again, two marches with the forward's own walk, ray and blend (baked_walk, BakedRay, baked_blend:
//                        each stated once) -- the first forms Q = sum w q, the second hands every sample's four gradients to
//                        the eight corners of its cell, summed in registers while the ray stays in the cell and added to memory
//                        with atomicAdd(float*) when it leaves it.  The one entry point here whose bits depend on the run.
//   upnerf_baked_sparse_render_bwd  the same kernel's other layout (the template's second parameter again): the
//                        gradient is pool-shaped, and a copy of a point on a face that bricks share receives the part that the
//                        samples inside its own brick give it -- upnerf_brick_face_sum (brick.hip) makes the copies whole.
//   upnerf_baked_ray_bwd  the gradient of a render with respect to each ray's own row o | d | near | far, both
//                        layouts: two marches again, the second one meets every sample's four gradients with the slopes of
//                        the blend in its cell; all sums in the ray's registers, the row written once: the same bits every run.
//   upnerf_baked_project the tuned points back into the marcher's domain (sigma >= 0 and finite; degree 0: colours in [0, 1]).
//   upnerf_baked_visibility  what a set of rays sees of a scene, both layouts and every degree in one instantiation
//                        per layout: one more march with the forward's walk, ray and blend, the corners read through a reader that
//                        returns (0, 0, 0, sigma) from a point of E bytes -- w depends on sigma alone.  The largest w of the ray's
//                        samples in a cell is kept in a register and, when the ray leaves the cell, maxed into the cell's live
//                        corners with atomicMax on the bits of a positive float: exact and commutative, the same bits every run.
//   upnerf_baked_prune   a point whose visibility is below a weight becomes the all-zero record upnerf_baked_pack leaves.
// All stores are ordinary vector stores and vector float atomics from plain C++.
#include "common.cuh"
#include "grid.cuh"

#include <math.h>

#include <type_traits>

namespace {

#define BAKED_THREADS 64

struct BakedGrid {
  int C[3];        // cells per axis
  float lo[3], inv[3], Cf[3];
  int64_t sy, sz;  // strides of the point grid, in points
};

// sample k of a ray: its t, its grid coordinates, and where it falls
struct BakedSample {
  float t, g[3];
  int i[3];     // cell per axis (inside only)
  int side[3];  // 0: inside the slab of the axis, -1: g < 0, +1: g > C, 2: not a number
  bool inside;
};

__host__ __device__ __forceinline__ BakedSample baked_locate(const BakedGrid& G, const float* o, const float* d, float near,
                                                             float step, int k) {
  BakedSample s;
  s.t = fmaf((float)k + 0.5f, step, near);
  s.inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p = fmaf(s.t, d[a], o[a]);
    const float g = (p - G.lo[a]) * G.inv[a];
    s.g[a] = g;
    s.side[a] = g < 0.0f ? -1 : (g > G.Cf[a] ? 1 : (g >= 0.0f ? 0 : 2));
    if (s.side[a] != 0) s.inside = false;
    const int i = (int)floorf(s.side[a] == 0 ? g : 0.0f);
    s.i[a] = i < G.C[a] - 1 ? i : G.C[a] - 1;
  }
  return s;
}

// the sample index proposed for a t at which the ray leaves a region: the last sample before it, less one; < 0: none
__host__ __device__ __forceinline__ int baked_propose(float t_exit, float near, float step, int K) {
  const float x = floorf((t_exit - near) / step - 0.5f) - 1.0f;
  if (!(x > 0.0f)) return -1;
  return x < (float)(K - 1) ? (int)x : K - 1;
}

struct BakedOut {
  float rgb[3], depth, opacity;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// where the four channels of a corner come from: BakedCorner<0> reads rgbs, BakedCorner<1 | 2> evaluates a record's expansion
// for the direction of the ray it was made for (include/upnerf_hip.h states the basis and the order of the sum)
template <int DEG>
struct BakedCorner {
  static constexpr int NB = (DEG + 1) * (DEG + 1), Q = DEG == 1 ? 2 : 4;  // basis functions; 16-byte loads per record
  const u32x4* rec;
  float Y[NB];
  __host__ __device__ __forceinline__ BakedCorner(const void* points, const float* d, float len) : rec((const u32x4*)points) {
    const float x = d[0] / len, y = d[1] / len, z = d[2] / len;
    Y[0] = 0.28209479177387814f;
    Y[1] = -0.4886025119029199f * y, Y[2] = 0.4886025119029199f * z, Y[3] = -0.4886025119029199f * x;
    if constexpr (DEG > 1) {
      Y[4] = 1.0925484305920792f * (x * y), Y[5] = -1.0925484305920792f * (y * z);
      Y[6] = 0.31539156525252005f * fmaf(2.0f * z, z, -fmaf(x, x, y * y));
      Y[7] = -1.0925484305920792f * (x * z), Y[8] = 0.5462742152960396f * fmaf(x, x, -(y * y));
    }
  }
  __host__ __device__ __forceinline__ f32x4 operator()(int64_t p) const {
    uint32_t w[4 * Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const u32x4 v = rec[p * Q + q];
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
    f32x4 out;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int h = c * NB + j;
        const float k = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[h >> 1] >> ((h & 1) * 16)));
        acc = fmaf(Y[j], k, acc);
      }
      out[c] = acc;
    }
    out[3] = __builtin_bit_cast(float, w[4 * Q - 2]);  // sigma: byte 24 of 32, byte 56 of 64
    return out;
  }
};

template <>
struct BakedCorner<0> {
  const f32x4* pts;
  __host__ __device__ __forceinline__ BakedCorner(const void* points, const float*, float) : pts((const f32x4*)points) {}
  __host__ __device__ __forceinline__ f32x4 operator()(int64_t p) const { return pts[p]; }
};

// the sigma of a point of any degree, colours zero: BAKED_SIGMA is no degree, and baked_blend<BAKED_SIGMA> clamps nothing, so its
// colour blends are dead code and its sigma, e, alpha, w and T are the forward's of the scene's own degree
#define BAKED_SIGMA (-1)
template <>
struct BakedCorner<BAKED_SIGMA> {
  const uint8_t* bytes;
  int64_t E;
  __host__ __device__ __forceinline__ BakedCorner(const void* points, int E_, int sigma_offset)
      : bytes((const uint8_t*)points + sigma_offset), E(E_) {}
  __host__ __device__ __forceinline__ f32x4 operator()(int64_t p) const { return f32x4{0.0f, 0.0f, 0.0f, *(const float*)(bytes + p * E)}; }
};

// a ray as both marches read it: the 32-byte row o | d | near | far (16-byte aligned), whether it can hit at all (eight finite
// numbers, far > near), its sample count K, |d| and the optical length of one step
struct BakedRay {
  float o[3], d[3], near, far;
  bool ok;
  int K;
  float len, delta;
  __host__ __device__ __forceinline__ BakedRay(const float* row, float step) {
    const f32x4 r0 = ((const f32x4*)row)[0], r1 = ((const f32x4*)row)[1];
    o[0] = r0.x, o[1] = r0.y, o[2] = r0.z, d[0] = r0.w, d[1] = r1.x, d[2] = r1.y, near = r1.z, far = r1.w;
    ok = far > near;
#pragma unroll
    for (int j = 0; j < 4; ++j) ok = ok && isfinite(r0[j]) && isfinite(r1[j]);
    K = 0;
    len = delta = 0.0f;
    if (ok) {
      const float nk = ceilf((far - near) / step);
      K = nk < (float)UPNERF_BAKED_MAX_SAMPLES ? (int)nk : UPNERF_BAKED_MAX_SAMPLES;
      len = sqrtf(fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0])));
      delta = step * len;
    }
  }
};

// The walk of a ray, the ONLY statement of the skipping logic: the samples that count -- inside the box, in a cell with a set bit
// (use_bits == false: every sample inside the box; a sparse march still passes over the empty bricks, which hold nothing) -- are
// handed in sample order to visit(s, base, sy, sz): `base` the point index of the cell's corner (0, 0, 0), sy and sz the strides
// to its y and z neighbours; visit returns true to end the ray (`stop`).  The forward and both passes of the backward march with
// it, so the backward's visited set is the forward's by construction.  The dense layouts index the whole grid
// [Cz+1][Cy+1][Cx+1]; the sparse one (brick.hip; include/upnerf_hip.h states it) finds a sample's brick in `slots` (< 0: the empty
// brick) and its corners among the 9 x 9 x 9 points of that slot.
template <bool SPARSE, class Visit>
__host__ __device__ __forceinline__ void baked_walk(const uint32_t* words, const int32_t* slots, float step, const BakedGrid& G,
                                                    const OccDims& dm, const BakedRay& ray, bool use_bits, Visit&& visit) {
  constexpr int P = UPNERF_BRICK_POINTS;
  const float *o = ray.o, *d = ray.d;
  const float near = ray.near;
  const int K = ray.K;
  const uint32_t* fine = words;
  const uint32_t* brick = words + dm.fine_words;
  int k = 0;
  while (k < K) {
    const BakedSample s = baked_locate(G, o, d, near, step, k);
    int next = k + 1;
    if (!s.inside) {
      // outside on an axis along which the ray does not come back: every later sample is outside too
      bool gone = false;
      float t_in = -INFINITY;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (s.side[a] == 1 || s.side[a] == -1) {
          const bool away = s.side[a] > 0 ? d[a] >= 0.0f : d[a] <= 0.0f;
          if (away) gone = true;
          else t_in = fmaxf(t_in, ((s.side[a] > 0 ? G.lo[a] + G.Cf[a] / G.inv[a] : G.lo[a]) - o[a]) / d[a]);
        }
      }
      if (gone) break;
      if (use_bits) {
        const int kp = baked_propose(t_in, near, step, K);
        if (kp > k) {
          const BakedSample q = baked_locate(G, o, d, near, step, kp);
          bool same = false;
#pragma unroll
          for (int a = 0; a < 3; ++a) same = same || ((s.side[a] == 1 || s.side[a] == -1) && q.side[a] == s.side[a]);
          if (same) next = kp + 1;
        }
      }
      k = next;
      continue;
    }
    int64_t slot = 0;  // (sparse: the sample's brick in the pool; it is read with or without the bits, the points hang on it)
    if (use_bits || SPARSE) {
      const int bx = s.i[0] / OCC_BRICK, by = s.i[1] / OCC_BRICK, bz = s.i[2] / OCC_BRICK;
      const int64_t b = ((int64_t)bz * dm.By + by) * dm.Bx + bx;
      int shift = -1;  // the empty region the sample lies in: 3 = its brick, 0 = its cell, -1 = none
      bool empty_brick;
      if constexpr (SPARSE) empty_brick = (slot = slots[b]) < 0;
      else empty_brick = !occ_bit(brick, b);
      if (empty_brick) shift = 3;
      else if (use_bits && !occ_bit(fine, ((int64_t)s.i[2] * dm.Cy + s.i[1]) * dm.Cx + s.i[0])) shift = 0;
      if (shift >= 0 && !use_bits) {  // (sparse, every sample visited: an empty brick holds nothing)
        k = next;
        continue;
      }
      if (shift >= 0) {
        float t_out = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          if (d[a] == 0.0f) continue;
          const int r = s.i[a] >> shift;
          int plane = d[a] > 0.0f ? (r + 1) << shift : r << shift;
          plane = plane < G.C[a] ? plane : G.C[a];
          t_out = fminf(t_out, ((G.lo[a] + (float)plane / G.inv[a]) - o[a]) / d[a]);
        }
        const int kp = baked_propose(t_out, near, step, K);
        if (kp > k) {
          const BakedSample q = baked_locate(G, o, d, near, step, kp);
          if (q.inside && (q.i[0] >> shift) == (s.i[0] >> shift) && (q.i[1] >> shift) == (s.i[1] >> shift) &&
              (q.i[2] >> shift) == (s.i[2] >> shift))
            next = kp + 1;
        }
        k = next;
        continue;
      }
    }
    const int64_t sy = SPARSE ? P : G.sy, sz = SPARSE ? P * P : G.sz;
    const int64_t base = SPARSE ? slot * (P * P * P) + (((s.i[2] % OCC_BRICK) * P + s.i[1] % OCC_BRICK) * P + s.i[0] % OCC_BRICK)
                                : ((int64_t)s.i[2] * G.sz + (int64_t)s.i[1] * G.sy) + s.i[0];
    if (visit(s, base, sy, sz)) break;
    k = next;
  }
}

// one counted sample as every march sees it: the trilinear blend of the eight corners (x first, then y, then z), the clamp of an
// expansion's colours, and the compositing step from the transmittance T before the sample
struct BakedBlend {
  float f[3];     // the sample's position in its cell
  float v[4];     // r, g, b (clamped at DEG > 0), sigma
  float w, Tn;    // w_k and T_{k+1}
  unsigned live;  // bit j: corner j (x = j & 1, y = j >> 1 & 1, z = j >> 2) stores a sigma that is not zero
  unsigned open;  // bit c: colour channel c was not clamped
};

template <int DEG>
__host__ __device__ __forceinline__ BakedBlend baked_blend(const BakedCorner<DEG>& pts, const BakedSample& s, int64_t base, int64_t sy,
                                                           int64_t sz, float delta, float T) {
  BakedBlend b;
  b.f[0] = s.g[0] - (float)s.i[0], b.f[1] = s.g[1] - (float)s.i[1], b.f[2] = s.g[2] - (float)s.i[2];
  // (written out, not a loop over j: with the loop the dense degree-1 forward holds 129 registers instead of 104, a wave less)
  const f32x4 c[8] = {pts(base),      pts(base + 1),      pts(base + sy),      pts(base + sy + 1),
                      pts(base + sz), pts(base + sz + 1), pts(base + sz + sy), pts(base + sz + sy + 1)};
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    const float x00 = fmaf(b.f[0], c[1][ch] - c[0][ch], c[0][ch]), x10 = fmaf(b.f[0], c[3][ch] - c[2][ch], c[2][ch]);
    const float x01 = fmaf(b.f[0], c[5][ch] - c[4][ch], c[4][ch]), x11 = fmaf(b.f[0], c[7][ch] - c[6][ch], c[6][ch]);
    const float y0 = fmaf(b.f[1], x10 - x00, x00), y1 = fmaf(b.f[1], x11 - x01, x01);
    b.v[ch] = fmaf(b.f[2], y1 - y0, y0);
  }
  b.live = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) b.live |= (c[j][3] != 0.0f ? 1u : 0u) << j;
  b.open = 7u;
  // (DEG > 0, not DEG != 0: BAKED_SIGMA is -1 and, like degree 0, clamps nothing -- upnerf_baked_visibility rests on that)
  static_assert(DEG >= BAKED_SIGMA && DEG <= 2, "a degree, or the sigma-only reader");
  if (DEG > 0) {  // an expansion is not held to [0, 1] as the colour head's sigmoid is
    b.open = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      b.open |= (b.v[ch] >= 0.0f && b.v[ch] <= 1.0f ? 1u : 0u) << ch;
      b.v[ch] = fminf(fmaxf(b.v[ch], 0.0f), 1.0f);
    }
  }
  const float e = expf(-delta * b.v[3]);
  const float alpha = 1.0f - e;
  b.w = T * alpha;
  b.Tn = T * (1.0f - alpha);
  return b;
}

// what a forward launch reads: the scene's points (rgbs, records or a pool) with, for a pool, its slot table; the bits; the rays.
// (The scalars come first as they do in the public structs: with the pointers first the dense degree-1 kernel compiles to 138
// registers instead of 104 and loses a wave per SIMD)
struct BakedArgs {
  int R;
  float step, background, stop;
  const void* points;
  const int32_t* slots;  // NULL: a dense layout
  const uint32_t* words;
  const float* rays;
  float *rgb, *depth, *opacity;
};

// the march of one ray row (host and device: the host build is what tests/host/baked_host.hip, run by
// tests/test_walks_host_cpu.py, checks against brute force over every sample and against the fp64 restatement)
template <int DEG, bool SPARSE>
__host__ __device__ __forceinline__ BakedOut baked_march(const BakedArgs& A, const BakedGrid& G, const OccDims& dm, const float* row,
                                                         bool use_bits) {
  const BakedRay ray(row, A.step);
  BakedOut out;
  out.rgb[0] = out.rgb[1] = out.rgb[2] = 0.0f;
  out.depth = 0.0f;
  out.opacity = 0.0f;
  if (ray.ok) {
    const BakedCorner<DEG> pts(A.points, ray.d, ray.len);
    float T = 1.0f;
    auto composite = [&](const BakedSample& s, int64_t base, int64_t sy, int64_t sz) __attribute__((always_inline)) {
      const BakedBlend b = baked_blend<DEG>(pts, s, base, sy, sz, ray.delta, T);
#pragma unroll
      for (int c = 0; c < 3; ++c) out.rgb[c] = fmaf(b.w, b.v[c], out.rgb[c]);
      out.depth = fmaf(b.w, s.t, out.depth);
      out.opacity += b.w;
      T = b.Tn;
      return A.stop > 0.0f && T < A.stop;
    };
    baked_walk<SPARSE>(A.words, A.slots, A.step, G, dm, ray, use_bits, composite);
  }
  const float rest = 1.0f - out.opacity;
#pragma unroll
  for (int c = 0; c < 3; ++c) out.rgb[c] = fmaf(rest, A.background, out.rgb[c]);
  out.depth = fmaf(rest, ray.far, out.depth);
  return out;
}

template <int DEG, bool SPARSE>
__global__ __launch_bounds__(BAKED_THREADS) void baked_render_kernel(BakedArgs a, BakedGrid G, OccDims dm) {
  const int r = blockIdx.x * BAKED_THREADS + threadIdx.x;
  if (r >= a.R) return;
  const BakedOut out = baked_march<DEG, SPARSE>(a, G, dm, a.rays + (int64_t)r * 8, true);
  float* c = a.rgb + (int64_t)r * 3;
  c[0] = out.rgb[0], c[1] = out.rgb[1], c[2] = out.rgb[2];
  a.depth[r] = out.depth;
  a.opacity[r] = out.opacity;
}

// ---- the backward march: upnerf_baked_render_bwd and, through a brick pool, upnerf_baked_sparse_render_bwd (include/upnerf_hip.h
// states the gradient).  The kernel takes the public struct of its layout by value, scalars first (BakedArgs
// says why); the two structs name the scene's points differently.
template <bool SPARSE>
using BakedBwdArgs = std::conditional_t<SPARSE, upnerf_baked_sparse_render_bwd_args, upnerf_baked_render_bwd_args>;
__device__ __forceinline__ const void* baked_bwd_points(const upnerf_baked_render_bwd_args& a) { return a.points; }
__device__ __forceinline__ const void* baked_bwd_points(const upnerf_baked_sparse_render_bwd_args& a) { return a.pool; }

template <int DEG, bool SPARSE>
__global__ __launch_bounds__(BAKED_THREADS) void baked_render_bwd_kernel(BakedBwdArgs<SPARSE> a, BakedGrid G, OccDims dm) {
  constexpr int NB = (DEG + 1) * (DEG + 1);
  const int32_t* slots = nullptr;
  if constexpr (SPARSE) slots = a.slots;
  const int r = blockIdx.x * BAKED_THREADS + threadIdx.x;
  if (r >= a.R) return;
  // upstream: g_rgb | g_depth | g_opacity; a ray none of whose gradients is set adds nothing
  const float g[5] = {a.g_rgb[(int64_t)r * 3], a.g_rgb[(int64_t)r * 3 + 1], a.g_rgb[(int64_t)r * 3 + 2], a.g_depth ? a.g_depth[r] : 0.0f,
                      a.g_opacity ? a.g_opacity[r] : 0.0f};
  if (g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f && g[3] == 0.0f && g[4] == 0.0f) return;
  const BakedRay ray(a.rays + (int64_t)r * 8, a.step);
  if (!ray.ok) return;  // a miss
  const BakedCorner<DEG> pts(baked_bwd_points(a), ray.d, ray.len);
  // q of a counted sample, from the forward's numbers for it
  auto q_of = [&](const BakedBlend& b, float t) __attribute__((always_inline)) {
    return fmaf(g[0], b.v[0] - a.background, fmaf(g[1], b.v[1] - a.background, fmaf(g[2], b.v[2] - a.background, fmaf(g[3], t - ray.far, g[4]))));
  };

  // first pass: the forward's recurrence, and Q = sum_k w_k q_k
  float Q = 0.0f, T = 1.0f;
  auto first = [&](const BakedSample& s, int64_t base, int64_t sy, int64_t sz) __attribute__((always_inline)) {
    const BakedBlend b = baked_blend<DEG>(pts, s, base, sy, sz, ray.delta, T);
    Q = fmaf(b.w, q_of(b, s.t), Q);
    T = b.Tn;
    return a.stop > 0.0f && T < a.stop;
  };
  baked_walk<SPARSE>(a.words, slots, a.step, G, dm, ray, true, first);

  // second pass: the same samples with the same numbers; the suffix of sample k is Q less the prefix up to and including k.  The
  // four gradients of a sample go to the eight corners of its cell with their trilinear weights: summed in registers while the
  // ray stays in one cell, added to memory when it leaves it
  // (`cell` is the visit's `base`, which names a cell uniquely in both layouts; the strides to its corners are the visit's too:
  // the grid's in a dense scene, 9 and 81 inside a slot of a pool -- so a pool's copy of a shared point receives what the samples
  // in its own brick's cells give it and nothing else)
  float acc[8][4];
  int64_t cell = -1;
  unsigned live = 0u;
  auto flush = [&]() __attribute__((always_inline)) {
    const int64_t sy = SPARSE ? UPNERF_BRICK_POINTS : G.sy, sz = SPARSE ? UPNERF_BRICK_POINTS * UPNERF_BRICK_POINTS : G.sz;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!(live >> j & 1u)) continue;  // a corner whose stored sigma is zero is no parameter
      const int64_t p = cell + (j & 1) + (j >> 1 & 1) * sy + (j >> 2) * sz;
      if constexpr (DEG == 0) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) atomicAdd(a.grad + p * 4 + ch, acc[j][ch]);
      } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
          for (int jb = 0; jb < NB; ++jb) atomicAdd(a.grad_coef + (p * 3 + ch) * NB + jb, pts.Y[jb] * acc[j][ch]);
        atomicAdd(a.grad_sigma + p, acc[j][3]);
      }
    }
  };
  float P = 0.0f;
  T = 1.0f;
  auto second = [&](const BakedSample& s, int64_t base, int64_t sy, int64_t sz) __attribute__((always_inline)) {
    const BakedBlend b = baked_blend<DEG>(pts, s, base, sy, sz, ray.delta, T);
    const float q = q_of(b, s.t);
    P = fmaf(b.w, q, P);
    const float gs = ray.delta * fmaf(b.Tn, q, -(Q - P));
    if (base != cell) {
      if (cell >= 0) flush();
      cell = base;
      live = b.live;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0f;
    }
    float gc[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) gc[ch] = (b.open >> ch & 1u) ? b.w * g[ch] : 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float wt = ((j & 4 ? b.f[2] : 1.0f - b.f[2]) * (j & 2 ? b.f[1] : 1.0f - b.f[1])) * (j & 1 ? b.f[0] : 1.0f - b.f[0]);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[j][ch] = fmaf(wt, gc[ch], acc[j][ch]);
      acc[j][3] = fmaf(wt, gs, acc[j][3]);
    }
    T = b.Tn;
    return a.stop > 0.0f && T < a.stop;
  };
  baked_walk<SPARSE>(a.words, slots, a.step, G, dm, ray, true, second);
  if (cell >= 0) flush();
}

// ---- the gradient of a ray's own row: upnerf_baked_ray_bwd (include/upnerf_hip.h states the gradient and the order of every sum;
// DESIGN.md 2.36).  What a launch reads and writes, scalars first (BakedArgs says why); both layouts and the three degrees.
struct BakedRayArgs {
  int R;
  float step, background, stop;
  const void* points;
  const int32_t* slots;  // NULL: a dense layout
  const uint32_t* words;
  const float* rays;
  const float *g_rgb, *g_depth, *g_opacity;
  float* g_rays;
};

struct BakedRayGrad {
  float v[8];  // the gradient of o | d | near | far
};

__host__ __device__ __forceinline__ float baked_lerp(float f, float a, float b) { return fmaf(f, b - a, a); }

// Z_j += sum_c s[c] k[c][j] over the stored halves of record p, channel by channel and j ascending (s: a corner's trilinear
// weight times the colour gradients of the sample): the blend of the coefficients is never formed
template <int DEG>
__host__ __device__ __forceinline__ void baked_coef_sum(const BakedCorner<DEG>& pts, int64_t p, const float* s, float* Z) {
  if constexpr (DEG > 0) {
    constexpr int NB = BakedCorner<DEG>::NB, Q = BakedCorner<DEG>::Q;
    uint32_t w[4 * Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const u32x4 v = pts.rec[p * Q + q];
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int h = c * NB + j;
        const float k = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[h >> 1] >> ((h & 1) * 16)));
        Z[j] = fmaf(k, s[c], Z[j]);
      }
  }
}

// the gradient of one ray row for the upstream gradients g = g_rgb | g_depth | g_opacity (host and device: the host build is
// what tests/host/baked_ray_host.hip holds to the fp64 restatement).  Two marches with the forward's walk, ray and blend: the
// first forms Q, the second the sums; the visited samples and their cells are the forward's and are held fixed.
template <int DEG, bool SPARSE>
__host__ __device__ __forceinline__ BakedRayGrad baked_ray_grad(const BakedRayArgs& A, const BakedGrid& G, const OccDims& dm,
                                                                const float* row, const float* g, bool use_bits) {
  constexpr int NB = (DEG + 1) * (DEG + 1);
  BakedRayGrad out;
#pragma unroll
  for (int i = 0; i < 8; ++i) out.v[i] = 0.0f;
  if (g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f && g[3] == 0.0f && g[4] == 0.0f) return out;
  const BakedRay ray(row, A.step);
  if (!ray.ok || ray.len == 0.0f) return out;  // a miss; a direction of length zero
  const BakedCorner<DEG> pts(A.points, ray.d, ray.len);
  auto q_of = [&](const BakedBlend& b, float t) __attribute__((always_inline)) {
    return fmaf(g[0], b.v[0] - A.background, fmaf(g[1], b.v[1] - A.background, fmaf(g[2], b.v[2] - A.background, fmaf(g[3], t - ray.far, g[4]))));
  };

  float Q = 0.0f, T = 1.0f;
  auto first = [&](const BakedSample& s, int64_t base, int64_t sy, int64_t sz) __attribute__((always_inline)) {
    const BakedBlend b = baked_blend<DEG>(pts, s, base, sy, sz, ray.delta, T);
    Q = fmaf(b.w, q_of(b, s.t), Q);
    T = b.Tn;
    return A.stop > 0.0f && T < A.stop;
  };
  baked_walk<SPARSE>(A.words, A.slots, A.step, G, dm, ray, use_bits, first);

  // So[a] = sum_k S_k[a] and St[a] = sum_k t_k S_k[a], S_k[a] = sum_ch a_k[ch] s_a[ch]: the grid's 1 / cell is applied once, after
  float P = 0.0f, O = 0.0f, E = 0.0f, So[3] = {0.0f, 0.0f, 0.0f}, St[3] = {0.0f, 0.0f, 0.0f}, Z[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) Z[j] = 0.0f;
  T = 1.0f;
  auto second = [&](const BakedSample& s, int64_t base, int64_t sy, int64_t sz) __attribute__((always_inline)) {
    const BakedBlend b = baked_blend<DEG>(pts, s, base, sy, sz, ray.delta, T);
    const float q = q_of(b, s.t);
    P = fmaf(b.w, q, P);
    const float I = fmaf(b.Tn, q, -(Q - P));
    float a[4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) a[ch] = (b.open >> ch & 1u) ? b.w * g[ch] : 0.0f;
    a[3] = ray.delta * I;
    E = fmaf(b.v[3], I, E);
    O += b.w;
    // the slopes of the blend in its cell, from the corners as the blend read them
    const f32x4 c[8] = {pts(base),      pts(base + 1),      pts(base + sy),      pts(base + sy + 1),
                        pts(base + sz), pts(base + sz + 1), pts(base + sz + sy), pts(base + sz + sy + 1)};
    float S[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const float sx = baked_lerp(b.f[2], baked_lerp(b.f[1], c[1][ch] - c[0][ch], c[3][ch] - c[2][ch]),
                                  baked_lerp(b.f[1], c[5][ch] - c[4][ch], c[7][ch] - c[6][ch]));
      const float sy_ = baked_lerp(b.f[2], baked_lerp(b.f[0], c[2][ch] - c[0][ch], c[3][ch] - c[1][ch]),
                                   baked_lerp(b.f[0], c[6][ch] - c[4][ch], c[7][ch] - c[5][ch]));
      const float sz_ = baked_lerp(b.f[1], baked_lerp(b.f[0], c[4][ch] - c[0][ch], c[5][ch] - c[1][ch]),
                                   baked_lerp(b.f[0], c[6][ch] - c[2][ch], c[7][ch] - c[3][ch]));
      S[0] = fmaf(a[ch], sx, S[0]), S[1] = fmaf(a[ch], sy_, S[1]), S[2] = fmaf(a[ch], sz_, S[2]);
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) So[ax] += S[ax], St[ax] = fmaf(s.t, S[ax], St[ax]);
    if constexpr (DEG > 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float wt = ((j & 4 ? b.f[2] : 1.0f - b.f[2]) * (j & 2 ? b.f[1] : 1.0f - b.f[1])) * (j & 1 ? b.f[0] : 1.0f - b.f[0]);
        const float sc[3] = {wt * a[0], wt * a[1], wt * a[2]};
        baked_coef_sum<DEG>(pts, base + (j & 1) + (j >> 1 & 1) * sy + (j >> 2) * sz, sc, Z);
      }
    }
    T = b.Tn;
    return A.stop > 0.0f && T < A.stop;
  };
  baked_walk<SPARSE>(A.words, A.slots, A.step, G, dm, ray, use_bits, second);

  const float u[3] = {ray.d[0] / ray.len, ray.d[1] / ray.len, ray.d[2] / ray.len};
  const float Es = E * A.step;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    out.v[ax] = G.inv[ax] * So[ax];
    out.v[3 + ax] = fmaf(Es, u[ax], G.inv[ax] * St[ax]);
  }
  if constexpr (DEG > 0) {  // sum_j Z_j dY_j/du, then through du/dd = (I - u u^T) / len
    const float c1 = 0.4886025119029199f, c2 = 1.0925484305920792f, c3 = 0.31539156525252005f, c4 = 0.5462742152960396f;
    float gu[3] = {-c1 * Z[3], -c1 * Z[1], c1 * Z[2]};
    if constexpr (DEG > 1) {
      gu[0] = fmaf(2.0f * c4 * u[0], Z[8], fmaf(-c2 * u[2], Z[7], fmaf(-2.0f * c3 * u[0], Z[6], fmaf(c2 * u[1], Z[4], gu[0]))));
      gu[1] = fmaf(-2.0f * c4 * u[1], Z[8], fmaf(-2.0f * c3 * u[1], Z[6], fmaf(-c2 * u[2], Z[5], fmaf(c2 * u[0], Z[4], gu[1]))));
      gu[2] = fmaf(-c2 * u[0], Z[7], fmaf(4.0f * c3 * u[2], Z[6], fmaf(-c2 * u[1], Z[5], gu[2])));
    }
    const float along = fmaf(u[2], gu[2], fmaf(u[1], gu[1], u[0] * gu[0]));
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) out.v[3 + ax] += fmaf(-u[ax], along, gu[ax]) / ray.len;
  }
  out.v[6] = fmaf(g[3], O, fmaf(ray.d[2], out.v[2], fmaf(ray.d[1], out.v[1], ray.d[0] * out.v[0])));
  out.v[7] = g[3] * (1.0f - O);
  return out;
}

template <int DEG, bool SPARSE>
__global__ __launch_bounds__(BAKED_THREADS) void baked_ray_bwd_kernel(BakedRayArgs a, BakedGrid G, OccDims dm) {
  const int r = blockIdx.x * BAKED_THREADS + threadIdx.x;
  if (r >= a.R) return;
  const float g[5] = {a.g_rgb[(int64_t)r * 3], a.g_rgb[(int64_t)r * 3 + 1], a.g_rgb[(int64_t)r * 3 + 2], a.g_depth ? a.g_depth[r] : 0.0f,
                      a.g_opacity ? a.g_opacity[r] : 0.0f};
  const BakedRayGrad out = baked_ray_grad<DEG, SPARSE>(a, G, dm, a.rays + (int64_t)r * 8, g, true);
  f32x4* dst = (f32x4*)(a.g_rays + (int64_t)r * 8);
  dst[0] = f32x4{out.v[0], out.v[1], out.v[2], out.v[3]};
  dst[1] = f32x4{out.v[4], out.v[5], out.v[6], out.v[7]};
}

// ---- what a set of rays sees: upnerf_baked_visibility (include/upnerf_hip.h states the definition).  What a launch
// reads and writes, scalars first (BakedArgs says why); both layouts, the degree only through E and the sigma's byte offset.
struct BakedVisArgs {
  int R;
  float step, stop;
  int E, sigma_offset;
  const void* points;
  const int32_t* slots;  // NULL: a dense layout
  const uint32_t* words;
  const float* rays;
  float* vis;
};

// the march of one ray row for its visibility (host and device: the host build is what tests/host/baked_vis_host.hip runs).  A
// sample met with T > 0 gives m = fmaxf(w, 2^-126); the largest m of the consecutive samples in one cell (`cell` is the visit's
// `base`, as in the backward) goes to record(p, m) for each live corner p of the cell when the ray leaves it.  Once T is exactly
// zero nothing later can record and the ray ends.
template <bool SPARSE, class Record>
__host__ __device__ __forceinline__ void baked_visibility_ray(const BakedVisArgs& A, const BakedGrid& G, const OccDims& dm, const float* row,
                                                              bool use_bits, Record&& record) {
  const BakedRay ray(row, A.step);
  if (!ray.ok) return;  // a miss
  const BakedCorner<BAKED_SIGMA> pts(A.points, A.E, A.sigma_offset);
  float T = 1.0f, m = 0.0f;
  int64_t cell = -1;
  unsigned live = 0u;
  auto flush = [&]() __attribute__((always_inline)) {
    const int64_t sy = SPARSE ? UPNERF_BRICK_POINTS : G.sy, sz = SPARSE ? UPNERF_BRICK_POINTS * UPNERF_BRICK_POINTS : G.sz;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (live >> j & 1u) record(cell + (j & 1) + (j >> 1 & 1) * sy + (j >> 2) * sz, m);
  };
  auto see = [&](const BakedSample& s, int64_t base, int64_t sy, int64_t sz) __attribute__((always_inline)) {
    if (!(T > 0.0f)) return true;
    const BakedBlend b = baked_blend<BAKED_SIGMA>(pts, s, base, sy, sz, ray.delta, T);
    if (base != cell) {
      if (cell >= 0) flush();
      cell = base;
      live = b.live;
      m = 0.0f;
    }
    m = fmaxf(m, fmaxf(b.w, 1.17549435e-38f));  // (2^-126: a sample met with light left is seen, however small its weight)
    T = b.Tn;
    return A.stop > 0.0f && T < A.stop;
  };
  baked_walk<SPARSE>(A.words, A.slots, A.step, G, dm, ray, use_bits, see);
  if (cell >= 0) flush();
}

template <bool SPARSE>
__global__ __launch_bounds__(BAKED_THREADS) void baked_visibility_kernel(BakedVisArgs a, BakedGrid G, OccDims dm) {
  const int r = blockIdx.x * BAKED_THREADS + threadIdx.x;
  if (r >= a.R) return;
  // every recorded value is a positive, finite float: its bits order as it does.  (The load first is a monotone race: a stale
  // value is a smaller one and only lets an atomic through that changes nothing.)
  auto record = [&](int64_t p, float m) __attribute__((always_inline)) {
    if (!(a.vis[p] >= m)) atomicMax((unsigned*)(a.vis + p), __builtin_bit_cast(unsigned, m));
  };
  baked_visibility_ray<SPARSE>(a, G, dm, a.rays + (int64_t)r * 8, true, record);
}

// upnerf_baked_prune: one thread per point of E bytes
__global__ __launch_bounds__(NTHREADS) void baked_prune_kernel(upnerf_baked_prune_args a) {
  const int64_t n = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (n >= a.n) return;
  const bool keep = a.vis[n] >= a.min_weight;
  if (!keep) {
    u32x4* rec = (u32x4*)(a.points + n * a.E);
    for (int q = 0; q < a.E / 16; ++q) rec[q] = u32x4{0u, 0u, 0u, 0u};
  }
  if (a.kept) a.kept[n] = keep ? 1 : 0;
}

// upnerf_baked_project: the point of a tuned scene back into the set the marcher is defined on
__global__ __launch_bounds__(NTHREADS) void baked_project_kernel(upnerf_baked_project_args a) {
  const int64_t n = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (n >= a.n) return;
  if (a.degree == 0) {
    f32x4 v = ((f32x4*)a.rgbs)[n];
    const bool keep = isfinite(v.w) && v.w > 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = keep && v[c] > 0.0f ? (v[c] < 1.0f ? v[c] : 1.0f) : 0.0f;
    v.w = keep ? v.w : 0.0f;
    ((f32x4*)a.rgbs)[n] = v;
  } else {
    const float s = a.sigma[n];
    a.sigma[n] = isfinite(s) && s > 0.0f ? s : 0.0f;
  }
}

__global__ __launch_bounds__(NTHREADS) void baked_pack_kernel(upnerf_baked_pack_args a) {
  const int64_t n = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (n >= a.n) return;
  const float s = a.sigma[n];
  const bool keep = isfinite(s) && s > 0.0f && s >= a.level;
  f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (keep) {
    if (a.rgb) v.x = a.rgb[n * 3], v.y = a.rgb[n * 3 + 1], v.z = a.rgb[n * 3 + 2];
    v.w = s;
  }
  ((f32x4*)a.rgbs)[n] = v;
  if (a.kept) a.kept[n] = keep ? 1 : 0;
}

__global__ __launch_bounds__(NTHREADS) void sh_accumulate_kernel(upnerf_sh_accumulate_args a) {
  const int64_t n = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (n >= a.n) return;
  const float* rgb = a.rgb + n * 3;
  float* acc = a.acc + n * 3 * a.nb;
  for (int c = 0; c < 3; ++c) {
    const float v = rgb[c];
    for (int j = 0; j < a.nb; ++j) acc[c * a.nb + j] = fmaf(a.w[j], v, a.first ? 0.0f : acc[c * a.nb + j]);
  }
}

template <int DEG>
__global__ __launch_bounds__(NTHREADS) void baked_sh_pack_kernel(upnerf_baked_sh_pack_args a) {
  constexpr int NB = (DEG + 1) * (DEG + 1), Q = DEG == 1 ? 2 : 4;
  const int64_t n = (int64_t)blockIdx.x * NTHREADS + threadIdx.x;
  if (n >= a.n) return;
  const float s = a.sigma[n];
  bool keep = isfinite(s) && s > 0.0f && s >= a.level;
  uint32_t w[4 * Q];
#pragma unroll
  for (int i = 0; i < 4 * Q; ++i) w[i] = 0u;
  const float* acc = a.acc + n * 3 * NB;
#pragma unroll
  for (int h = 0; h < 3 * NB; ++h) {
    const float k = acc[h];
    keep = keep && isfinite(k);
    const _Float16 half = (_Float16)fminf(fmaxf(k, -65504.0f), 65504.0f);  // (the conversion rounds to nearest even)
    w[h >> 1] |= (uint32_t)__builtin_bit_cast(uint16_t, half) << ((h & 1) * 16);
  }
  w[4 * Q - 2] = __builtin_bit_cast(uint32_t, s);
  u32x4* rec = (u32x4*)a.records + n * Q;
#pragma unroll
  for (int q = 0; q < Q; ++q) rec[q] = keep ? u32x4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]} : u32x4{0u, 0u, 0u, 0u};
  if (a.kept) a.kept[n] = keep ? 1 : 0;
}

bool baked_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the arguments a launch may be given, and the grid as the kernel reads it
// (`points`: the rgbs or the records of `a`, aligned to `size`, the bytes of one point)
template <class Args>
bool baked_lattice(const Args* a, const void* points, size_t size, BakedGrid* G, OccDims* dm) {
  if (!a || !occ_dims(a->Cx, a->Cy, a->Cz, dm) || a->R <= 0) return false;
  if (!points || !a->words || !a->rays) return false;
  if (((uintptr_t)points & (size - 1)) != 0 || !baked_aligned16(a->rays)) return false;
  if (!(a->step > 0.0f) || !isfinite(a->step) || !isfinite(a->background) || !(a->stop >= 0.0f && a->stop < 1.0f)) return false;
  const int C[3] = {a->Cx, a->Cy, a->Cz};
  for (int k = 0; k < 3; ++k) {
    if (!(a->hi[k] > a->lo[k]) || !isfinite(a->hi[k]) || !isfinite(a->lo[k])) return false;
    G->C[k] = C[k];
    G->Cf[k] = (float)C[k];
    G->lo[k] = a->lo[k];
    G->inv[k] = (float)((double)C[k] / ((double)a->hi[k] - (double)a->lo[k]));
    if (!(G->inv[k] > 0.0f) || !isfinite(G->inv[k])) return false;
  }
  G->sy = (int64_t)a->Cx + 1;
  G->sz = G->sy * ((int64_t)a->Cy + 1);
  return true;
}

// a run-time degree in MIN .. 2, checked by the caller, to the code of that degree: f(std::integral_constant<int, DEG>())
template <int MIN, class F>
void baked_by_degree(int degree, F&& f) {
  if constexpr (MIN == 0)
    if (degree == 0) return f(std::integral_constant<int, 0>());
  if (degree == 1) return f(std::integral_constant<int, 1>());
  return f(std::integral_constant<int, 2>());
}

dim3 baked_blocks(int R) { return dim3((R + BAKED_THREADS - 1) / BAKED_THREADS); }

// a forward entry point after its own refusals: the outputs, the lattice, the kernel's arguments, the launch
template <bool SPARSE, class Args>
int baked_forward(const Args* a, int degree, const void* points, const int32_t* slots, void* stream) {
  BakedGrid G;
  OccDims dm;
  if (!a || !a->rgb || !a->depth || !a->opacity || !baked_lattice(a, points, (size_t)16 << degree, &G, &dm)) return UPNERF_EINVAL;
  const BakedArgs A = {a->R, a->step, a->background, a->stop, points, slots, a->words, a->rays, a->rgb, a->depth, a->opacity};
  baked_by_degree<0>(degree, [&](auto deg) {
    hipLaunchKernelGGL((baked_render_kernel<decltype(deg)::value, SPARSE>), baked_blocks(a->R), dim3(BAKED_THREADS), 0, (hipStream_t)stream, A, G, dm);
  });
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int upnerf_baked_render(const upnerf_baked_render_args* a, void* stream) {
  return baked_forward<false>(a, 0, a ? a->rgbs : nullptr, nullptr, stream);
}

extern "C" int upnerf_baked_pack(const upnerf_baked_pack_args* a, void* stream) {
  if (!a || a->n <= 0 || !a->sigma || !a->rgbs || !baked_aligned16(a->rgbs) || a->level != a->level) return UPNERF_EINVAL;
  const int64_t blocks = (a->n + NTHREADS - 1) / NTHREADS;
  if (blocks > 0x7fffffff) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(baked_pack_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_baked_sh_render(const upnerf_baked_sh_render_args* a, void* stream) {
  if (!a || (a->degree != 1 && a->degree != 2)) return UPNERF_EINVAL;
  return baked_forward<false>(a, a->degree, a->records, nullptr, stream);
}

extern "C" int upnerf_baked_sparse_render(const upnerf_baked_sparse_render_args* a, void* stream) {
  if (!a || a->degree < 0 || a->degree > 2 || !a->slots) return UPNERF_EINVAL;
  return baked_forward<true>(a, a->degree, a->pool, a->slots, stream);
}

// a backward entry point after its own refusals: the upstream gradient and the outputs of the degree, the lattice, the launch
template <class Args>
int baked_backward(const Args* a, const void* points, BakedGrid* G, OccDims* dm) {
  if (!a || a->degree < 0 || a->degree > 2 || !a->g_rgb) return UPNERF_EINVAL;
  if (a->degree == 0 ? !a->grad : (!a->grad_coef || !a->grad_sigma)) return UPNERF_EINVAL;
  return baked_lattice(a, points, (size_t)16 << a->degree, G, dm) ? 0 : UPNERF_EINVAL;
}

template <bool SPARSE, class Args>
int baked_backward_launch(const Args* a, const BakedGrid& G, const OccDims& dm, void* stream) {
  baked_by_degree<0>(a->degree, [&](auto deg) {
    hipLaunchKernelGGL((baked_render_bwd_kernel<decltype(deg)::value, SPARSE>), baked_blocks(a->R), dim3(BAKED_THREADS), 0, (hipStream_t)stream, *a, G, dm);
  });
  return (int)hipGetLastError();
}

extern "C" int upnerf_baked_render_bwd(const upnerf_baked_render_bwd_args* a, void* stream) {
  BakedGrid G;
  OccDims dm;
  if (const int rc = baked_backward(a, a ? a->points : nullptr, &G, &dm)) return rc;
  if (a->slots) return UPNERF_EUNSUP;  // a brick pool is upnerf_baked_sparse_render_bwd's: its output is pool-shaped
  return baked_backward_launch<false>(a, G, dm, stream);
}

extern "C" int upnerf_baked_sparse_render_bwd(const upnerf_baked_sparse_render_bwd_args* a, void* stream) {
  BakedGrid G;
  OccDims dm;
  if (!a || !a->slots) return UPNERF_EINVAL;
  if (const int rc = baked_backward(a, a->pool, &G, &dm)) return rc;
  return baked_backward_launch<true>(a, G, dm, stream);
}

extern "C" int upnerf_baked_ray_bwd(const upnerf_baked_ray_bwd_args* a, void* stream) {
  BakedGrid G;
  OccDims dm;
  if (!a || a->degree < 0 || a->degree > 2 || !a->g_rgb || !a->g_rays || !baked_aligned16(a->g_rays)) return UPNERF_EINVAL;
  if (!baked_lattice(a, a->points, (size_t)16 << a->degree, &G, &dm)) return UPNERF_EINVAL;
  const BakedRayArgs A = {a->R,    a->step,  a->background, a->stop,      a->points, a->slots,
                          a->words, a->rays, a->g_rgb,      a->g_depth,   a->g_opacity, a->g_rays};
  baked_by_degree<0>(a->degree, [&](auto deg) {
    if (a->slots)
      hipLaunchKernelGGL((baked_ray_bwd_kernel<decltype(deg)::value, true>), baked_blocks(a->R), dim3(BAKED_THREADS), 0, (hipStream_t)stream, A, G, dm);
    else
      hipLaunchKernelGGL((baked_ray_bwd_kernel<decltype(deg)::value, false>), baked_blocks(a->R), dim3(BAKED_THREADS), 0, (hipStream_t)stream, A, G, dm);
  });
  return (int)hipGetLastError();
}

extern "C" int upnerf_baked_visibility(const upnerf_baked_visibility_args* a, void* stream) {
  BakedGrid G;
  OccDims dm;
  if (!a || !a->vis || (a->E != 16 && a->E != 32 && a->E != 64)) return UPNERF_EINVAL;
  if (a->sigma_offset < 0 || (a->sigma_offset & 3) || a->sigma_offset > a->E - 4) return UPNERF_EINVAL;
  // the forward's refusals, on the forward's own struct (its background is not this entry point's: zero)
  upnerf_baked_sparse_render_args f = {};
  f.Cx = a->Cx, f.Cy = a->Cy, f.Cz = a->Cz, f.R = a->R;
  for (int k = 0; k < 3; ++k) f.lo[k] = a->lo[k], f.hi[k] = a->hi[k];
  f.step = a->step, f.stop = a->stop, f.words = a->words, f.rays = a->rays;
  if (!baked_lattice(&f, a->points, (size_t)a->E, &G, &dm)) return UPNERF_EINVAL;
  const BakedVisArgs A = {a->R, a->step, a->stop, a->E, a->sigma_offset, a->points, a->slots, a->words, a->rays, a->vis};
  if (a->slots)
    hipLaunchKernelGGL(baked_visibility_kernel<true>, baked_blocks(a->R), dim3(BAKED_THREADS), 0, (hipStream_t)stream, A, G, dm);
  else
    hipLaunchKernelGGL(baked_visibility_kernel<false>, baked_blocks(a->R), dim3(BAKED_THREADS), 0, (hipStream_t)stream, A, G, dm);
  return (int)hipGetLastError();
}

extern "C" int upnerf_baked_prune(const upnerf_baked_prune_args* a, void* stream) {
  if (!a || a->n <= 0 || (a->E != 16 && a->E != 32 && a->E != 64) || !a->vis || !a->points || !baked_aligned16(a->points)) return UPNERF_EINVAL;
  if (a->min_weight != a->min_weight) return UPNERF_EINVAL;
  const int64_t blocks = (a->n + NTHREADS - 1) / NTHREADS;
  if (blocks > 0x7fffffff) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(baked_prune_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_baked_project(const upnerf_baked_project_args* a, void* stream) {
  if (!a || a->n <= 0 || a->degree < 0 || a->degree > 2) return UPNERF_EINVAL;
  if (a->degree == 0 ? (!a->rgbs || !baked_aligned16(a->rgbs)) : !a->sigma) return UPNERF_EINVAL;
  const int64_t blocks = (a->n + NTHREADS - 1) / NTHREADS;
  if (blocks > 0x7fffffff) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(baked_project_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_sh_accumulate(const upnerf_sh_accumulate_args* a, void* stream) {
  if (!a || a->n <= 0 || (a->nb != 4 && a->nb != 9) || !a->rgb || !a->acc) return UPNERF_EINVAL;
  for (int j = 0; j < a->nb; ++j)
    if (!isfinite(a->w[j])) return UPNERF_EINVAL;
  const int64_t blocks = (a->n + NTHREADS - 1) / NTHREADS;
  if (blocks > 0x7fffffff) return UPNERF_EUNSUP;
  hipLaunchKernelGGL(sh_accumulate_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  return (int)hipGetLastError();
}

extern "C" int upnerf_baked_sh_pack(const upnerf_baked_sh_pack_args* a, void* stream) {
  if (!a || a->n <= 0 || (a->degree != 1 && a->degree != 2) || !a->sigma || !a->acc || !a->records || a->level != a->level)
    return UPNERF_EINVAL;
  if (((uintptr_t)a->records & (a->degree == 1 ? 31 : 63)) != 0) return UPNERF_EINVAL;
  const int64_t blocks = (a->n + NTHREADS - 1) / NTHREADS;
  if (blocks > 0x7fffffff) return UPNERF_EUNSUP;
  baked_by_degree<1>(a->degree, [&](auto deg) {
    hipLaunchKernelGGL(baked_sh_pack_kernel<decltype(deg)::value>, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream, *a);
  });
  return (int)hipGetLastError();
}
