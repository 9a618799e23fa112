/*
 * upnerf_hip.h -- C ABI of libupnerf_hip.so, the MI355X (gfx950) implementation of the UP-NeRF
 * render_rays training hot path.
 *
 * The reference (mlvlab/UP-NeRF) is pure Python on PyTorch: it has no native boundary of its own
 * (SURVEY.md 2.2).  The entry points below are therefore the leaf operations its Python hot path
 * performs, one per group of ATen launches, and each cites the reference lines it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding a maintainer
 * of the reference would add to call them from models/rendering.py.
 *
 * Conventions
 *  - every function returns 0 on success, a hipError_t (>0) on a HIP failure, or a negative
 *    UPNERF_E* code on an argument error; nothing is printed, nothing throws.
 *  - all pointers are DEVICE pointers to fp32 (or int64 where said), row-major, contiguous; they
 *    are borrowed for the duration of the call (stream-ordered) -- the library allocates nothing
 *    and keeps no global state.  `stream` is a hipStream_t passed as void*.
 *  - "rows" M = R * S (rays x samples per ray), sample i of ray r is row r*S + i.
 */
#ifndef UPNERF_HIP_H
#define UPNERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UPNERF_ABI_VERSION 11
#define UPNERF_EINVAL (-1)   /* bad size / null pointer */
#define UPNERF_EUNSUP (-2)   /* unsupported width/depth combination */

#ifndef UPNERF_TILE_ROWS
#define UPNERF_TILE_ROWS 64  /* rows of samples per workgroup in the fused field kernels */
#endif
#define UPNERF_X0 64         /* positional encoding 3+6*10 = 63 padded to 64 floats per row */
#define UPNERF_AUXK 80       /* per-ray rgb-head side input [dirPE(27) | appearance(48) | 0 x5] */
#define UPNERF_CK 16         /* candidate embedding width */
#define UPNERF_MAX_D 8

int upnerf_abi_version(void);

/* ---- a2-a4: pose refinement + ray generation (utils/camera.py:87-98,113-152 se3_to_SE3;
 *      camera.py:51-58 compose_pair; utils/ray.py:44-56 get_rays batched branch) -------------------
 * se3 [R][6] (already gathered rows of se3_refine, or NULL = identity refinement), c2w [R][3][4],
 * dirs [R][3] camera-space directions -> rays_o [R][3], rays_d [R][3] (unit norm).
 * bwd: g_o, g_d [R][3] -> g_se3 [R][6] (per ray; the caller scatter-adds rows by img_idx). */
int upnerf_pose_rays_fwd(int R, const float* se3, const float* c2w, const float* dirs,
                         float* rays_o, float* rays_d, void* stream);
int upnerf_pose_rays_bwd(int R, const float* se3, const float* c2w, const float* dirs,
                         const float* g_o, const float* g_d, float* g_se3, void* stream);

/* ---- a5: stratified coarse depths (models/rendering.py:232-249) ---------------------------------
 * near_far [R][2]; steps [S] = linspace(0,1,S); u [R][S] uniform draws or NULL (perturb == 0);
 * z_out [R][S]. */
int upnerf_sample_coarse(int R, int S, const float* near_far, const float* steps, const float* u,
                         float perturb, int use_disp, float* z_out, void* stream);

/* ---- uniform draws for a5 / a11 (the reference calls torch.rand / rand_like, models/rendering.py:248, 29) --------------
 * out[r][c] = u(seed, step, row0 + r * row_stride, draw, c) in [0, 1), c < n: Philox4x32-10 with counter (global row, c / 4,
 * step, draw) and key seed, 24 bits per value.  row0 + r * row_stride = GLOBAL row of local ray r in the data-parallel batch, so
 * the numbers do not depend on how the batch is split over ranks: contiguous shards pass (rank * R, 1), shards
 * dealt like DistributedSampler (local ray r = global ray r * world + rank) pass (rank, world).  draw = 0 coarse jitter, 1, 2 =
 * the sample_pdf sets in call order.  step_dev (DEVICE [1] float or NULL) overrides `step` at execution time (graph replay). */
int upnerf_uniform_keyed(int R, int n, uint64_t seed, int step, const float* step_dev, int row0, int row_stride, int draw,
                         float* out, void* stream);

/* Key of the uniform draws, for kernels that GENERATE their draws instead of reading a buffer upnerf_uniform_keyed wrote (round
 * 6: one launch less per consumer).  Same fields, same numbers: u(seed, step, row0 + r * row_stride, draw, column). */
typedef struct upnerf_rng {
  uint64_t seed;
  int32_t step;           /* optimisation step; overridden by step_dev[0] when step_dev != NULL (graph replay) */
  int32_t row0, row_stride;
  const float* step_dev;  /* DEVICE [1] float or NULL */
} upnerf_rng;

/* a5 with the jitter draws generated in the kernel (draw 0 of upnerf_uniform_keyed): z_out as upnerf_sample_coarse would compute
 * it from u = upnerf_uniform_keyed(R, S, ..., draw 0), bit for bit.  perturb > 0. */
int upnerf_sample_coarse_keyed(int R, int S, const float* near_far, const float* steps, const upnerf_rng* rng, float perturb,
                               int use_disp, float* z_out, void* stream);

/* ---- a11: inverse-CDF resampling (models/rendering.py:7-50 sample_pdf) ---------------------------
 * z [R][S] coarse depths (bins = midpoints, computed inside), weights [R][S] (only [1:S-1] used),
 * u [u_rows][n] with u_rows == R, or u_rows == 1 for the deterministic linspace; writes n values per
 * ray to out + r*out_stride. */
int upnerf_sample_pdf(int R, int S, const float* z, const float* weights, const float* u, int u_rows,
                      int n, float* out, int out_stride, void* stream);

/* ---- a12: ascending sort of each row (models/rendering.py:275,290,298,307 torch.sort values) ----- */
int upnerf_sort_rows(int R, int S, float* z, void* stream);

/* ---- a11 + a12 in one launch (models/rendering.py:262-308): zf[r] = sort(z[r] | set A | set B), S = Nc + n_a + n_b columns.
 * z [R][Nc] coarse depths; set X = n_x inverse-CDF samples of the weights w_x [R][Nc] (entries 1..Nc-2 used, as upnerf_sample_pdf)
 * that upnerf_sample_pdf would write to columns [col_x, col_x + n_x) of zf before upnerf_sort_rows sorts the row -- the same
 * arithmetic call for call, so zf equals the three-launch sequence bit for bit.  n_b may be 0 (one set).  Uniforms: u_x
 * [u_rows][n_x] (u_rows = R, or 1 for the deterministic linspace) or, where u_x is NULL, generated from `rng` as draw number
 * draw_x of upnerf_uniform_keyed (the caller numbers its draws in call order; draw 0 is the coarse jitter). */
int upnerf_resample_sort(int R, int Nc, const float* z, const float* w_a, int n_a, int col_a, const float* u_a, int draw_a,
                         const float* w_b, int n_b, int col_b, const float* u_b, int draw_b, int u_rows, const upnerf_rng* rng,
                         float* zf, void* stream);

/* ---- per-ray rgb-head side input: [PE(rays_d, L=4, masked) | appearance row | 0]  (nerf.py:102-107;
 *      the reference repeats it per sample, rendering.py:104-109) ---------------------------------- */
int upnerf_ray_aux(int R, const float* rays_d, const float* a_rows /*[R][48] or NULL*/,
                   const float* wk_dir /*[4] HOST*/, const float* wk_dir_dev /*[4] DEVICE or NULL: overrides wk_dir (graph
                   replay: per-step scalars live in device memory, see upnerf_set_scalars)*/,
                   float* aux /*[R][UPNERF_AUXK]*/, void* stream);

/* ---- a6-a9: fused NeRF field, forward (models/nerf.py:80-124 + 126-147) --------------------------
 * Layout of the packed parameter buffers (floats): offsets below; a matrix is [N][Kp] with Kp a multiple
 * of 8 (zero padded), N a multiple of 32.  Two orderings of the SAME offsets are used:
 *   row-major      W[n][k] at off + n*Kp + k           -- gradients (upnerf_wgrad output) and host code
 *   fragment order W[n][k] at off + ((n/32)*(Kp/8) + k/8)*256 + (((k/4)%2)*32 + n%32)*4 + k%4
 *                                                        -- what upnerf_field_fwd/bwd READ (one 1 KiB block =
 *                                                           one wave-wide MFMA B-operand load)
 * Vectors (biases, the 1- and 3-wide heads wsig/wcsig/wr2) are stored plainly in both.
 * See upnerf_amd/packing.py (pack / frag / pack_t / frag_t) for the packing from the reference's
 * state_dict names. */
typedef struct {
  int32_t W, D, skip;            /* width (64 or 256), depth (<= 8), index of the skip layer or -1 */
  int32_t w[UPNERF_MAX_D];       /* trunk layer l: [W][Kp_l], Kp_0 = 64, Kp_skip = 64 + W, else W */
  int32_t b[UPNERF_MAX_D];       /* trunk biases [W] */
  int32_t we, be;                /* xyz_encoding_final [W][W], [W] */
  int32_t wsig, bsig;            /* share_sigma.0 [W], [1] */
  int32_t wc1, bc1;              /* candidate_encoding.0 [W/2][W + 16], [W/2] */
  int32_t wc2, bc2;              /* candidate_encoding.2 [W/2][W/2], [W/2] */
  int32_t wcsig, bcsig;          /* candidate_sigma.0 [W/2], [1] */
  int32_t wr1, br1;              /* folded rgb_share_layer.0 [W/2][W + 80], [W/2] */
  int32_t wr2, br2;              /* rgb_share_layer.2 [3][W/2], [3] (padded to 4) */
  int32_t total;                 /* floats in P */
  /* transposed copies for the backward data-gradient chain, in buffer PT */
  int32_t t_w[UPNERF_MAX_D];     /* layer l: [Kin_l][W] with Kin_0 = 64; skip: h part [W][W] */
  int32_t t_skipx;               /* skip layer, encoding part [64][W] */
  int32_t t_we;                  /* [W][W] */
  int32_t t_head;                /* [W][W]: cols [0,W/2) = wr1[:, :W]^T, cols [W/2,W) = wc1[:, :W]^T */
  int32_t t_wc2;                 /* [W/2][W/2] */
  int32_t t_total;
} upnerf_layout;

typedef struct {
  int32_t R, S;                  /* rays, samples per ray */
  int32_t use_cand, use_rgb;     /* sched_mult < 1 && encode_candidate ; sched_mult > 0 */
  const float* rays_o;           /* [R][3] */
  const float* rays_d;           /* [R][3] */
  const float* z;                /* [R][S] */
  const float* c_rows;           /* [R][16] candidate embedding rows (use_cand) */
  const float* aux;              /* [R][80] from upnerf_ray_aux (use_rgb) */
  float wk_xyz[10];              /* BARF band weights for the xyz encoding */
  const float* P;                /* packed parameters, matrices in fragment order */
  /* per-sample outputs */
  float* sigma_s;                /* [M] softplus output */
  float* sigma_c;                /* [M] (use_cand) */
  float* rgb;                    /* [M][3] sigmoid output (use_rgb) */
  /* activations kept for compositing and for the backward pass.  Inference (no gradient wanted): h, hmask, g1, r1 may be
   * NULL = not stored; e and g2 may be NULL when the compositing mode does not build a feature map (mode 2).  x0 is
   * always required (the skip layer re-reads it). */
  float* x0;                     /* [M][64] */
  float* h;                      /* [D][M][W] post-ReLU trunk activations */
  uint64_t* hmask;               /* ReLU sign bits of h in the kernels' accumulator layout, private to a forward / backward kernel
                                    pair: [D + 1][tiles][threads per workgroup] words.  (D + 1) * ceil(M/128) * 512 words cover
                                    either tiling */
  float* amax;                   /* [16] or NULL: running max|.| (atomicMax; zero it first) of h_0..h_{D-1} (slots 0..D-1),
                                    e (D), g1 (D+1), r1 (D+3), x0 (D+4) -- scale exponents of upnerf_wgrad16 */
  float* e;                      /* [M][W]   xyz_encoding_final output */
  float* g1;                     /* [M][W/2] (use_cand) */
  float* g2;                     /* [M][W/2] (use_cand) */
  float* r1;                     /* [M][W/2] (use_rgb) */
  /* f16x3 variant only (upnerf_field_fwd_f16x3): */
  const void* P16;               /* matrices of P as scaled fp16 (hi, lo) fragments, from upnerf_frag16 (forward set) */
  const int32_t* wexp;           /* [16] per-matrix exponents from upnerf_frag16 */
  const float* wk_xyz_dev;       /* [10] DEVICE or NULL: overrides wk_xyz (read at execution time, so a captured HIP graph
                                    follows the schedule from one replay to the next) */
  int32_t planes;                /* upnerf_field_fwd_f16x3 only: 0 or 2 = f16x3 (fp32-accurate hi/lo split, three MFMAs per
                                    product); 1 = f16 (fp16 weights and activations, one MFMA per product, fp32 accumulate:
                                    BASELINE.json configs[3]); the lo halves of P16 are then never read */
  int32_t tile_rows;             /* upnerf_field_fwd_f16x3 only: samples per workgroup.  0 or 64: four waves, two workgroups per CU.
                                    (128, round 3's software-pipelined trunk, left the library in round 4: UPNERF_EINVAL.)  The
                                    backward pass of the same evaluation must be given the same value (the hmask layout follows
                                    the tile).
                                    256 (planes = 1 only, S >= 32): the REGISTER-RESIDENT kernels of csrc/field16rr.hip -- eight waves
                                    of 32 samples whose activations stay in registers, every weight slab staged once per workgroup
                                    in an LDS ring by LDS-DMA.  Contract of that variant: P16 / PT16 from upnerf_frag16 with
                                    perm_fwd = perm_bwd = 1 and `wnorm` from the same call; EVERY per-sample tensor with more than
                                    4 floats per sample (x0, e, g1, g2, r1, h, h16, hmask and the backward pass's gz_*, gz16) has room
                                    for Mp = ceil(M / 256) * 256 rows (rows >= M are written with padding values); h16 / gz16 are in
                                    FRAGMENT order -- [layer][Mp / 32][k-block 0..15][lane 0..63][8] fp16, feature of element j of
                                    lane l in k-block s = 16 s + 8 (j / 4) + 4 (l / 32) + j % 4, row = 32 tile + l % 32 -- with one
                                    exponent per 32 rows (hexp / gzexp [D][Mp / 32]); hmask holds (D + 3) * Mp * 4 words in the
                                    kernel pair's own layout; `h` is [Mp][W] (last layer, h_last_only = 1) */
  const float* wnorm;            /* [64] row 1-norms from upnerf_frag16 (forward set at 0.., transposed set at 32..): required by the
                                    register-resident kernels (tile_rows = 256), must be NULL otherwise */
  /* fp16 STORAGE of the trunk activations (always in the f16 mode; an option in the f16x3 mode, where it rounds only the
   * operands of the weight gradients): halves what the pass writes and what the weight-gradient kernels read back
   * (UPNERF_WG_F16_TILE).  h16[l][m][k] = fp16(h_l[m][k] * 2^hexp[l][m / 64]): the content of the
   * LDS plane of the 64-sample tile, copied out as it stands, with the tile's power-of-two exponent beside it. */
  uint16_t* h16;                 /* [D][M][W] fp16 bits, or NULL (fp32 `h` as above) */
  int32_t* hexp;                 /* [D][ceil(M/64)] */
  int32_t h_last_only;           /* with h16: `h` (if non-NULL) receives layer D-1 only, as [M][W] fp32 (density-head and
                                    final-layer weight gradients read it) */
  void* x0f;                     /* reserved (was the 128-sample tiling's encoding scratch): ignored */
  uint16_t* e16;                 /* tile_rows = 256 only, or NULL: e as fp16 operand fragments [ceil(M/256) * 8][16][64][8] like one
                                    layer of h16 (then `e` may be NULL); upnerf_composite_fwd / _bwd and upnerf_wgrad16 read it */
  int32_t* eexp;                 /* [ceil(M/256) * 8] */
  uint16_t* g2_16;               /* the same for g2 (128 wide: [..][8][64][8]; then `g2` may be NULL) and for r1: compositing / */
  int32_t* g2exp;                /* upnerf_vec_wgrad_frag16 read them; the backward kernel works from the sign bits in hmask */
  uint16_t* r1_16;
  int32_t* r1exp;
  uint16_t* g1_16;               /* and for g1 (candidate_encoding.2's weight gradient reads it: upnerf_wgrad16, 128-wide fragments) */
  int32_t* g1exp;
  uint8_t* h_lo8;                /* f16x3 mode with h16, or NULL: [D][M][W] bytes, the rounding residual of every h16 element in 1/32 of
                                    its tile's scaled unit (byte = round(32 lo) + 128): h16 + h_lo8 = the trunk activation to 2^-20
                                    of its tile's maximum in 3 bytes ("24-bit" weight-gradient operands, UPNERF_WG_F24) */
  int64_t rows_capacity;         /* (ABI 9) tile_rows = 256: the number of rows every per-sample tensor passed here was allocated with.
                                    The register-resident kernels write whole 256-sample tiles: tensors need ceil(M / 256) * 256 rows.
                                    A caller that says so here gets UPNERF_EINVAL instead of a write past the end when it is less;
                                    0 = not stated (unchecked, as before) */
} upnerf_field_fwd_args;

int upnerf_field_fwd(const upnerf_layout* L, const upnerf_field_fwd_args* a, void* stream);
/* Same contract, contractions on the f16 matrix cores with the 3-term hi/lo split (fp32-level accuracy, see
 * csrc/common16.cuh).  W = 256 only; `P` is read for the vectors only (biases, wsig, wcsig, wr2: any ordering of P has
 * them in place); hmask needs D+1 slots (slot D = sign bits of g1). */
int upnerf_field_fwd_f16x3(const upnerf_layout* L, const upnerf_field_fwd_args* a, void* stream);

/* ---- a10: alpha compositing, forward (models/rendering.py:125-218) -------------------------------
 * Features are composited in the W-wide space of xyz_encoding_final / candidate_encoding and projected
 * once per ray by the caller (exact algebra: feat = W_f (sum w e) + b_f sum w). */
typedef struct {
  int32_t R, S, W;
  int32_t mode;                  /* 0: candidate+shared (sched==0), 1: both + rgb (0<sched<1),
                                    2: shared only (sched==1), 3: shared only, feature map (no candidate, sched<1) */
  const float* z;                /* [R][S] */
  const float* sigma_s;          /* [M] */
  const float* sigma_c;          /* [M] modes 0,1 */
  const float* rgb;              /* [M][3] modes 1,2,3 when sched>0 */
  int32_t has_rgb;
  const float* e;                /* [M][W] */
  const float* g2;               /* [M][W/2] modes 0,1 */
  /* per-sample outputs (also the saved state of the backward) */
  float* w_all;                  /* [M] alpha*T       -> c_weights      (modes 0,1) */
  float* w_sj;                   /* [M] alpha_s*T     (joint transmittance, modes 0,1) */
  float* w_cj;                   /* [M] alpha_c*T     (modes 0,1) */
  float* w_s;                    /* [M] alpha_s*T_s   -> s_weights */
  /* per-ray outputs */
  float* E_s;                    /* [R][W]   sum_i ws_feat_i e_i   (ws_feat = w_sj in modes 0,1; w_s in mode 3) */
  float* G_c;                    /* [R][W/2] sum_i w_cj g2_i       (modes 0,1) */
  float* sum_sfeat;              /* [R] sum_i ws_feat_i */
  float* t_weight;               /* [R] sum_i w_cj */
  float* c_depth;                /* [R] sum_i w_all z */
  float* s_depth;                /* [R] sum_i w_s z */
  float* rgb_map;                /* [R][3] sum_i w_s rgb_i */
  /* W = 256: e as the fp16 operand fragments of the register-resident field kernels instead of fp32 rows (then `e` is
   * ignored): upnerf_field_fwd_args.e16 / eexp */
  const uint16_t* e16;
  const int32_t* eexp;
  const uint16_t* g2_16;         /* with e16 (modes 0, 1): g2 the same way, 128 wide = 8 k-blocks per 32 samples (then `g2` is ignored) */
  const int32_t* g2exp;
  /* encode_feat = False (models/rendering.py:177-190): the shared colour composited with the JOINT-transmittance weights,
   * sum_i w_sj rgb_i -- the shared half of `c_rgb`.  NULL = not wanted; modes 0, 1 with has_rgb only.  (ABI 9) */
  float* rgb_joint_map;          /* [R][3] */
} upnerf_composite_fwd_args;

int upnerf_composite_fwd(const upnerf_composite_fwd_args* a, void* stream);

/* ---- a10 backward (division-free reverse scan) ------------------------------ */
typedef struct {
  int32_t R, S, W, mode, has_rgb;
  const float* z; const float* sigma_s; const float* sigma_c; const float* rgb;
  const float* e; const float* g2;
  const float* w_all; const float* w_sj; const float* w_cj; const float* w_s;
  /* upstream gradients (any may be NULL = zero) */
  const float* g_E_s;            /* [R][W] */
  const float* g_G_c;            /* [R][W/2] */
  const float* g_sum_sfeat;      /* [R] */
  const float* g_t_weight;       /* [R] */
  const float* g_c_depth;        /* [R] */
  const float* g_s_depth;        /* [R] */
  const float* g_rgb_map;        /* [R][3] */
  const float* g_w_all;          /* [M] */
  const float* g_w_s;            /* [M] */
  /* outputs */
  float* d_sigma_s;              /* [M] */
  float* d_sigma_c;              /* [M] modes 0,1 */
  float* d_rgb;                  /* [M][3] has_rgb */
  const uint16_t* e16;           /* as in upnerf_composite_fwd_args */
  const int32_t* eexp;
  const uint16_t* g2_16;
  const int32_t* g2exp;
  const float* g_rgb_joint_map;  /* [R][3] upstream gradient of upnerf_composite_fwd_args.rgb_joint_map, or NULL (ABI 9) */
} upnerf_composite_bwd_args;

int upnerf_composite_bwd(const upnerf_composite_bwd_args* a, void* stream);

/* ---- a7-a9 backward: data-gradient chain through the fused field (autograd of nerf.py:80-124) ----
 * Consumes the per-sample gradients from upnerf_composite_bwd plus the rank-1 feature terms
 * (w_feat_s[m] * g_E_s[ray], w_cj[m] * g_G_c[ray]) and writes the pre-activation gradient of every layer
 * (inputs of upnerf_wgrad) and d(xyz). */
typedef struct {
  int32_t R, S, use_cand, use_rgb, need_dxyz;
  const float* PT;               /* transposed parameter copies (layout t_*), fragment order */
  const float* P;                /* forward parameters (vectors wsig, wcsig, wr2) */
  const float* d_sigma_s; const float* d_sigma_c; const float* d_rgb;
  const float* sigma_s; const float* sigma_c; const float* rgb;
  const float* w_feat_s;         /* [M] weight multiplying e_i in the feature map (w_sj or w_s), or NULL */
  const float* w_cj;             /* [M] */
  const float* g_E_s;            /* [R][W] or NULL */
  const float* g_G_c;            /* [R][W/2] or NULL */
  const float* x0; const float* h; const float* g1; const float* g2; const float* r1;
  const uint64_t* hmask;         /* from upnerf_field_fwd */
  float* gmax;                   /* [16] or NULL: running max|.| of gz_h[0..D-1] (slots 0..D-1), gz_e (D), gz_g1 (D+1),
                                    gz_g2 (D+2), gz_r1 (D+3) */
  /* outputs */
  float* gz_h;                   /* [D][M][W] */
  float* gz_e;                   /* [M][W] */
  float* gz_g1; float* gz_g2;    /* [M][W/2] */
  float* gz_r1;                  /* [M][W/2] */
  float* dpre_sig_s;             /* [M] */
  float* dpre_sig_c;             /* [M] */
  float* dpre_rgb;               /* [M][4] (3 used) */
  float* dxyz;                   /* [M][3] (need_dxyz) */
  /* f16x3 variant only (upnerf_field_bwd_f16x3): */
  const void* PT16;              /* transposed set of upnerf_frag16 */
  const int32_t* wexp;           /* [16] */
  int32_t planes;                /* as in upnerf_field_fwd_args: 0 / 2 = f16x3, 1 = f16 */
  int32_t tile_rows;             /* as in upnerf_field_fwd_args; must equal the forward pass's */
  uint16_t* gz16;                /* [D][M][W] fp16 bits of gz_h, tile-scaled like h16 (then gz_h may be NULL).  tile_rows = 256
                                    with gz_e == NULL: [D + 1] layers, the last one d e in the same form (and gzexp [D + 1] rows) */
  int32_t* gzexp;                /* [D][ceil(M/64)] */
  void* xs;                      /* reserved (was the 128-sample tiling's scratch): ignored */
  float* tile_part;              /* NULL, or [ceil(M/64)][UPNERF_TILE_PART_STRIDE] (f16x3 variant, tile_rows 0 / 64 only): per-tile
                                    partial sums of what upnerf_vec_wgrad (dpre_sig_c x g2, dpre_rgb x r1) and upnerf_ray_sum
                                    (gz_g1, gz_r1) would re-read M x W/2 tensors for; finished by upnerf_tile_part_finish.
                                    tile_rows = 256: NULL, or [ceil(M/256) * 8][UPNERF_RR_PART_STRIDE]: the per-ray sums only, per
                                    32 samples, finished by upnerf_ray_part_finish */
  int32_t gz_rg_ld;              /* f16x3 variant: row stride (floats) of gz_r1 and gz_g1; 0 = W/2 (two dense tensors).  With
                                    gz_g1 = gz_r1 + W/2 and a stride of W the two form ONE [M][W] tensor [gz_r1 | gz_g1], whose
                                    weight gradient against e is one launch (upnerf_wgrad_desc.n2); its running maximum is
                                    tracked in gmax slot D+4 */
  int32_t reserved_;
  const float* wnorm;            /* as in upnerf_field_fwd_args (tile_rows = 256: required; else NULL) */
  uint16_t* gz_rg16;             /* tile_rows = 256 with both heads, or NULL: [gz_r1 | gz_g1] as ONE 256-wide tensor of fp16 operand
                                    fragments (then gz_r1 / gz_g1 may be NULL: with tile_part their per-ray sums still leave) */
  int32_t* gzrgexp;              /* [ceil(M/256) * 8] */
  uint16_t* gz_g2_16;            /* tile_rows = 256, or NULL: gz_g2 as 128-wide fp16 operand fragments (then gz_g2 may be NULL) */
  int32_t* gzg2exp;
  uint8_t* gz_lo8;               /* f16x3 mode with gz16, or NULL: [D][M][W] residual bytes of gz16 (as upnerf_field_fwd_args.h_lo8) */
  int64_t rows_capacity;         /* (ABI 9) as in upnerf_field_fwd_args */
} upnerf_field_bwd_args;

/* Layout of one row of tile_part (floats): d w_csig [W/2] | d w_r2 [3][W/2] | sum dpre_sig_c, sum dpre_rgb[0..2] | 4 pad |
 * sums of gz_g1 over the tile's rows of ray slot 0, 1, 2 [3][W/2] | the same for gz_r1 [3][W/2]; ray slot of row i of tile t =
 * (64 t + i) / S - (64 t) / S.  W/2 = 128. */
#define UPNERF_TILE_PART_STRIDE 1288
/* Finishes the per-tile partial sums: rs_g1 / rs_r1 [R][128] = per-ray sums of gz_g1 / gz_r1 (upnerf_ray_sum's result),
 * d_wcsig [128], d_bcsig [1], d_wr2 [3][128], d_br2 [3] = upnerf_vec_wgrad's results; any output may be NULL.  Fixed summation
 * order (bitwise reproducible).  scratch: 128 * 520 floats. */
int upnerf_tile_part_finish(int R, int S, const float* tile_part, float* rs_g1, float* rs_r1, float* d_wcsig, float* d_bcsig,
                            float* d_wr2, float* d_br2, float* scratch, void* stream);

/* tile_rows = 256: one row of tile_part per 32 samples: sums of gz_r1 over the rows of the first / second ray of those 32 samples
 * [2][128], then the same for gz_g1 (S >= 32: at most two rays; the second block is only written when there is a second ray). */
#define UPNERF_RR_PART_STRIDE 512
/* rs_g1 / rs_r1 [R][128] from those rows, in a fixed order (either may be NULL). */
int upnerf_ray_part_finish(int R, int S, const float* tile_part, float* rs_g1, float* rs_r1, void* stream);

int upnerf_field_bwd(const upnerf_layout* L, const upnerf_field_bwd_args* a, void* stream);
/* f16x3 variant: W = 256 and S >= 32 (at most 3 rays per 64-sample tile); hmask from upnerf_field_fwd_f16x3. */
int upnerf_field_bwd_f16x3(const upnerf_layout* L, const upnerf_field_bwd_args* a, void* stream);

/* ---- weight gradients: dW[N][ldo] (+)= sum_m A[m][n] * B[m][k], db[n] = sum_m A[m][n] ------------
 * A [M][lda] (N columns used), B [M][ldb] (K columns used); K, N multiples of 32 (N <= 256, K <= 256).
 * `slabs` is scratch for nsplit partial results (nsplit * N * K floats); reduced in fixed order, so the
 * result is bitwise reproducible.  db may be NULL. */
int upnerf_wgrad(int M, const float* A, int lda, int N, const float* B, int ldb, int K,
                 float* dW, int ldo, float* db, float* slabs, int nsplit, void* stream);

/* Many small weight gradients in one launch + one fixed-order reduction (the per-ray layers of TransientNet and the
 * feature projections, M = rays: separately each is a 25 us launch that fills a quarter of the GPU).  Same arithmetic
 * as upnerf_wgrad (fp32 MFMA); N, K, lda, ldb, ldo multiples of 4, any N and K (cut into 128 x 128 blocks).
 * scratch: upnerf_wgrad_grouped_scratch(...) floats (a negative return is an error code). */
#define UPNERF_MAX_WGRAD_GROUPS 32
typedef struct {
  const float* A;                /* [M][lda], N columns used */
  const float* B;                /* [M][ldb], K columns used */
  float* dW;                     /* [N][ldo] */
  float* db;                     /* [N] or NULL */
  int32_t M, N, K, lda, ldb, ldo;
} upnerf_wgrad_group;
int upnerf_wgrad_grouped_scratch(const upnerf_wgrad_group* groups, int ngroups, int nsplit);
int upnerf_wgrad_grouped(const upnerf_wgrad_group* groups, int ngroups, float* scratch, int nsplit, void* stream);

/* ---- TransientNet (models/transient_net.py:5-38) as one forward and one backward launch: feat_dim 384, hidden width 256,
 * transient embedding width 128 (the reference's defaults), one row per ray.  Weights in the nn.Linear layout ([out][in],
 * row-major); fp32 MFMA, fp32 accumulate.  The forward pass stores what the backward pass and the weight gradients read. */
typedef struct {
  int32_t R; float beta_min;
  const float* feat;             /* [R][384] */
  const float* t_emb;            /* [R][128] rows of embedding_t */
  const float* w0; const float* b0;   /* feat_encoder.0  [256][384], [256] */
  const float* w1; const float* b1;   /* feat_encoder.2  [256][256] */
  const float* w2; const float* b2;   /* feat_encoder.4 */
  const float* w3; const float* b3;   /* feat_encoder.6 */
  const float* wf; const float* bf;   /* final_encoder   [256][256] */
  const float* wt; const float* bt;   /* t_encoder.0     [128][384] over [final_encoding | t_emb] */
  const float* wa; const float* ba;   /* alpha_layer.0   [1][256] */
  const float* wb; const float* bb;   /* beta_layer.0    [1][128] */
  const float* wr; const float* br;   /* rgb_layer.0     [3][128] */
  float* h;                      /* [4][R][256] post-ReLU outputs of the four feat_encoder layers */
  float* e;                      /* [R][256] final_encoding */
  float* t;                      /* [R][128] post-ReLU output of t_encoder */
  float* alpha; float* rgb; float* beta;   /* [R], [R][3], [R]: the module's outputs */
  float* spre;                   /* [R] pre-activation of the beta head */
} upnerf_transient_args;
typedef struct {
  const float* d_alpha; const float* d_rgb; const float* d_beta;   /* [R], [R][3], [R]; NULL = zero */
  float* dz_heads;               /* [R][8]: pre-activation gradients of alpha, beta, rgb[3] (3 unused) */
  float* gz_t;                   /* [R][128] */
  float* gz_e;                   /* [R][256] */
  float* gz_h;                   /* [4][R][256] */
  float* g_temb;                 /* [R][128] or NULL */
  float* g_feat;                 /* [R][384] or NULL */
} upnerf_transient_grads;
int upnerf_transient_fwd(const upnerf_transient_args* a, void* stream);
/* data gradients only; the weight gradients are upnerf_wgrad_grouped over (gz_*, stored inputs) */
int upnerf_transient_bwd(const upnerf_transient_args* a, const upnerf_transient_grads* g, void* stream);

/* ---- weight gradients on the f16 matrix cores: ONE entry point, the problem in a descriptor ------------------------------
 * Same contract as upnerf_wgrad (dW[n][k] = sum_m A[m][n] B[m][k], db[n] = sum_m A[m][n], nsplit slabs summed in a fixed
 * order: bitwise reproducible).  Both operands are brought to tensor-wide power-of-two scales 2^*expo_a / 2^*expo_b (DEVICE
 * ints, chosen so that the scaled maxima are ~2^14; upnerf_scale_exponents) and contracted in fp16 with fp32 accumulation.
 * How an operand is STORED is its `kind`; A and B are of the same kind, or B is fp32 rows beside a fp16-stored A (the
 * encoding x0). */
enum {
  /* fp32 rows [M][ld]; ld, N, K multiples of 4.  desc.planes picks the arithmetic: 0 / 2 (f16x3) = split on load into fp16
   * hi + lo parts, Ah Bh + Ah Bl + Al Bh accumulated in fp32 -- fp32-level accuracy at 5.3x fewer matrix cycles than the fp32
   * MFMA (HBM-bound); 1 (f16) = rounded to fp16, one MFMA per block (the "f16" field mode).  Any N and K. */
  UPNERF_WG_F32 = 0,
  /* fp16 bits [M][ld], value * 2^exp[m / 64]: the f16 field mode's fp16-STORED operands (upnerf_field_bwd_f16x3's gz16 /
   * gzexp, h16 / hexp).  Brought to the tensor-wide exponent on load: value * 2^(e_tensor - e_tile) rounded ONCE to fp16 -- exact
   * while the result is a normal fp16 number, to 2^-25 (half a subnormal step) below 2^-14, for any exponent difference (a tile
   * more than 2^24 below the tensor's maximum is rounded from the exact fp32 product; nothing is clamped).  This holds for every
   * stored kind and plane below.  One MFMA per block, fp32 accumulate.  Reads 1 KB per sample and layer instead of 2.  ld, N, K multiples of 8; 256 x 256 blocks (B stored the
   * same way) and 256 x 64 (fp32 B). */
  UPNERF_WG_F16_TILE,
  /* the operand FRAGMENTS of the register-resident field kernels (upnerf_field_fwd_args.tile_rows = 256: [32-row tile]
   * [k-block][lane][8], one exponent per 32 rows); ld is ignored.  N = 256 or 128 with a B of the same kind and K = N, or
   * N = 256 with fp32 B (K = 64). */
  UPNERF_WG_F16_FRAG,
  /* "24-bit" operands (f16x3 mode): p = fp16 hi, lo = uint8 residual, both [M][ld], exponents per 64 rows, as the f16x3 field
   * kernels write them (h16 + h_lo8, gz16 + gz_lo8); a fp32 B beside them is split into hi + lo on load.  Three MFMAs per
   * block as for UPNERF_WG_F32 rows: the operands are exact to 2^-20 of their tile's maximum in 3 bytes per element instead
   * of 4.  Row-major only (no fragment order); 256 x 256 and 256 x 64 blocks. */
  UPNERF_WG_F24,
  /* PRODUCER-SPLIT operands (round 6): p / lo are the (hi, lo) fp16 planes of the f16x3 field kernels' tiles, row-major
   * [M][256], value = (hi + lo) * 2^-exp[m / 64] (upnerf_field_fwd_args.h16 / h_lo16 / hexp, upnerf_field_bwd_args.gz16 /
   * gz_lo16 / gzexp) -- the 4 bytes per element of the fp32 rows, which ARE hi + lo, already split.  The kernel stages them by
   * LDS-DMA (no conversion pass, no staging registers, three 16-row chunks in flight) and contracts as for UPNERF_WG_F32 rows
   * (three MFMAs per block).  N = K = ld = 256 and M % 64 == 0 (UPNERF_EUNSUP otherwise: the caller keeps the fp32 rows for
   * such shapes).  Measured, not wired into the training step. */
  UPNERF_WG_PLANES
};
typedef struct {
  const void* p;                 /* fp32 rows, fp16 bits or fragments, as `kind` says */
  const void* lo;                /* UPNERF_WG_F24: uint8 residuals; UPNERF_WG_PLANES: fp16 lo plane; else unused */
  const int32_t* exp;            /* per-tile exponents of the fp16-stored kinds; unused for UPNERF_WG_F32 */
  int32_t ld, kind;
} upnerf_wgrad_operand;

/* A problem whose slabs are written but not summed (nsplit == 0: none).  Handed to upnerf_wgrad16, the slabs of one weight
 * gradient are summed by the first workgroups of the NEXT weight-gradient launch (a prologue that costs it a few microseconds)
 * instead of a reduction launch of their own (20+ us each, 40 per step): the call sums what is pending -- in its kernel's
 * prologue when the grid is large enough, by a reduction launch otherwise -- and replaces it by the description of ITS
 * problem.  upnerf_wgrad_finish sums what is pending and clears it.  The caller alternates between two slab buffers: desc.slabs
 * must differ from pending->slabs.  One run may mix every kind of operand; same arithmetic and summation order as without. */
typedef struct {
  const float* slabs; const float* bslabs;
  float* dW; float* db;
  int32_t N, K, TN, TK, nsplit, ldo, rblocks;
  int32_t n2;                    /* > 0: rows n >= n2 of the result go to dW2[(n - n2) * ldo2 + k], db2[n - n2] */
  float* dW2; float* db2;
  int32_t ldo2, pad;
  /* a vector head that shares B with the problem (upnerf_wgrad_desc.v): per-split partial sums [nsplit][K + 4]
   * (vslabs: K sums of v[m] B[m][k], then the sum of v) -> dv [K], dbv [1]; NULL: none */
  const float* vslabs; float* dv; float* dbv;
} upnerf_wgrad_pending;

typedef struct {
  int32_t M, N, K;
  int32_t planes;                /* arithmetic for UPNERF_WG_F32 operands: 0 / 2 = 3-term split, 1 = one MFMA; else ignored */
  upnerf_wgrad_operand A, B;     /* A [M] x N columns, B [M] x K columns */
  const int32_t* expo_a; const int32_t* expo_b;   /* DEVICE: the tensor-wide exponents */
  float* dW; float* db;          /* [N][ldo], [N] or NULL; ldo a multiple of 4 */
  int32_t ldo;
  /* n2 > 0: a result split by rows between two destinations, rows [n2, N) -> dW2 [N - n2][ldo2] / db2 (two layers that share
   * B and whose A operands sit side by side in one tensor: the colour and candidate heads' first layers, both fed by e) */
  int32_t n2;
  float* dW2; float* db2;
  int32_t ldo2, nsplit;
  /* a 1-wide head fed by the same B rows rides on the launch, in the same pass over B:  dv[k] = sum_m v[m] B[m][k],
   * dbv[0] = sum_m v[m]  (the shared density head: share_sigma reads the last trunk activation, which is also the B operand of
   * xyz_encoding_final's weight gradient -- models/nerf.py:89, 93 -- so the separate upnerf_vec_wgrad / upnerf_vec_wgrad_frag16
   * launch and its second read of that tensor, 1 KB per sample, go away).  fp32 arithmetic for the vector (as upnerf_vec_wgrad),
   * fixed summation order.  N = K = 256 only, on UPNERF_WG_F32 rows with planes = 2 or on UPNERF_WG_F16_FRAG operands on both
   * sides (UPNERF_EUNSUP otherwise); NULL: none. */
  const float* v; float* dv; float* dbv;
  float* slabs;                  /* scratch: upnerf_wgrad16_scratch(desc) floats */
} upnerf_wgrad_desc;
/* floats `slabs` must hold: nsplit * (slabs + bias slabs [+ the riding head's K + 4]) at the block shape the call picks for
 * (N, K); reads N, K, nsplit and v only.  A negative return is an error code. */
long long upnerf_wgrad16_scratch(const upnerf_wgrad_desc* d);
/* pending == NULL: the slabs are summed at once by a reduction launch; else a link of a chained run (upnerf_wgrad_pending) */
int upnerf_wgrad16(const upnerf_wgrad_desc* d, upnerf_wgrad_pending* pending, void* stream);
int upnerf_wgrad_finish(upnerf_wgrad_pending* pending, void* stream);

/* dw[c][k] = sum_m v[m*ldv + c] * X[m][k], c < nvec <= 3; dbv[c] = sum_m v[m*ldv + c]   (N=1/3 heads);
 * K in {32, 64, 128, 256}; scratch: nsplit * 4 * (K+1) floats */
int upnerf_vec_wgrad(int M, const float* v, int ldv, int nvec, const float* X, int ldx, int K,
                     float* dw /*[nvec][K]*/, float* dbv /*[nvec]*/, float* scratch, int nsplit, void* stream);

/* upnerf_vec_wgrad (same v / ldv / nvec / dw / dbv) against a 256- or 128-wide fp16 tensor in the operand-fragment order of the
 * register-resident field kernels (upnerf_field_fwd_args.tile_rows = 256: h16 / hexp of one layer, g2_16, r1_16; padded to whole
 * 32-sample tiles); scratch: nsplit * 4 * (K + 1) floats.  Fixed summation order. */
int upnerf_vec_wgrad_frag16(int M, const float* v, int ldv, int nvec, const uint16_t* X16, const int32_t* xexp, int K, float* dw,
                            float* dbv, float* scratch, int nsplit, void* stream);  /* nvec <= 3, K = 256 or 128 */

/* out[r][c] = sum_{i<S} X[(r*S+i)][c]  (per-ray sums of a per-sample tensor; embedding-row gradients) */
int upnerf_ray_sum(int R, int S, const float* X, int C, float* out, void* stream);
/* (d_o, d_d)[r] = (sum_i dxyz_i, sum_i z_i dxyz_i)    */
int upnerf_ray_geom_bwd(int R, int S, const float* dxyz, const float* z, float* d_o, float* d_d, void* stream);

/* ---- f1: train-split ray sampler (datasets/phototourism.py:420-454, PhototourismDataset.__getitem__ + default
 * collate): gathers a batch of rays from the flat per-ray buffers, resident in HBM, and interpolates each ray's
 * feature bilinearly from its image's [h][h][C] map with the reference's weights (incl. its vanishing weights on the
 * last row / column).  Bit-exact with the reference.  inv_depths / feats may be NULL (depth / feature supervision off). */
typedef struct {
  int32_t R, h, C;                 /* rays in the batch, feature-map side, channels */
  const int64_t* idx;              /* [R] indices into the flat ray buffers */
  const float* all_ray_infos;      /* [N][3] near, far, image index */
  const float* all_directions;     /* [N][3] */
  const float* all_rgbs;           /* [N][3] */
  const float* all_pxl_coords;     /* [N][2] (row, column) in [0, 1] */
  const float* all_inv_depths;     /* [N] or NULL */
  const float* feat_maps;          /* [I][h][h][C] or NULL */
  const float* poses;              /* [I][3][4] camera-to-world per image index */
  float* ray_infos;                /* [R][2] */
  float* directions;               /* [R][3] */
  int64_t* img_idx;                /* [R] */
  float* c2w;                      /* [R][3][4] */
  float* rgbs;                     /* [R][3] */
  float* feats;                    /* [R][C] or NULL */
  float* inv_depths;               /* [R] or NULL */
} upnerf_gather_rays_args;
int upnerf_gather_rays(const upnerf_gather_rays_args* a, void* stream);

/* ---- dense gradient of an embedding table (autograd of nn.Embedding(img_idx): the per-image appearance / candidate /
 * transient rows, se3_refine and depth_scale of models/nerf_system.py:79-91): out[n][:] = sum_{r: idx[r]==n} g[r][:],
 * rows without a hit are written as zeros; summation in increasing r (bitwise reproducible).  dim <= 256. */
int upnerf_embed_bwd(int R, int N, int dim, const int64_t* idx, const float* g, float* out, void* stream);
/* The same for up to UPNERF_MAX_EMBED_GROUPS tables of N rows gathered with the SAME idx (every per-image table of a
 * training step): one scan of idx serves all of them. */
#define UPNERF_MAX_EMBED_GROUPS 8
typedef struct {
  const float* g;                /* [R][dim] gradient of the gathered rows */
  float* out;                    /* [N][dim] dense table gradient */
  int32_t dim;                   /* <= 256 */
} upnerf_embed_group;
int upnerf_embed_bwd_grouped(int R, int N, const int64_t* idx, const upnerf_embed_group* groups, int ngroups, void* stream);
/* The forward side of the same tables (nn.Embedding.forward, models/nerf_system.py:79-91 called at :160, :170 and in
 * rendering.py:177-181 / transient_net.py:31): rows[r][:] = table[idx[r]][:] for up to UPNERF_MAX_EMBED_GROUPS tables of N
 * rows in one launch instead of an index_select launch per table.  An index outside [0, N) is UPNERF_EINVAL-free on the host
 * (it lives in device memory): its row is written as NaN, which no test or loss survives unnoticed. */
typedef struct {
  const float* table;            /* [N][dim] */
  float* rows;                   /* [R][dim] gathered rows */
  int32_t dim;                   /* <= 256 */
} upnerf_embed_rows_group;
int upnerf_embed_fwd_grouped(int R, int N, const int64_t* idx, const upnerf_embed_rows_group* groups, int ngroups, void* stream);


/* ---- generic fp32 MFMA linear layer: C[M][N] = act(A[M][K] . B[N][K]^T + bias) --------------------
 * (TransientNet, models/transient_net.py:27-38, and the per-ray feature projection.)  K multiple of 8,
 * act bit 0: ReLU; act bit 1: B is given as [K][N] (row stride ldb), i.e. C = act(A . B + bias) -- the data-gradient
 * form, no transposed copy needed.  N arbitrary (ldb/ldc are row strides). */
int upnerf_linear(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                  const float* bias, float* C, int ldc, int act, void* stream);
/* Matrix-vector products in a fixed summation order (the bias fold of the colour layer, both directions):
 * trans = 0: y[m] = add[m] + sum_k A[m][k] x[k], m < M;  trans = 1: y[k] = add[k] + sum_m A[m][k] x[m], k < K.  add may be NULL. */
int upnerf_matvec(int M, int K, const float* A, int lda, const float* x, const float* add, float* y, int trans, void* stream);
/* p[0 .. n) = 0 (p 16-byte aligned): the one fill of a training step's zero arena (upnerf_amd/zero_pool.py). */
int upnerf_zero(float* p, long long n, void* stream);
/* out_j[i] = a_j[i] + b_j[i], i < n_j, for up to UPNERF_MAX_ADD_PAIRS tensors in one launch (the gradient sum of a tensor with two
 * consumers: ops._Fanout; fp32 addition is commutative, so the result is autograd's own a + b bit for bit). */
#define UPNERF_MAX_ADD_PAIRS 8
typedef struct upnerf_add_pair {
  const float* a;
  const float* b;
  float* out;   /* may alias a or b */
  int32_t n;
} upnerf_add_pair;
int upnerf_add_pairs(const upnerf_add_pair* pairs, int npairs, void* stream);
/* The backward of the bias fold in one launch: y[k] = sum_m A[m][k] x[m] (upnerf_matvec, trans = 1, add = NULL, bit for bit) AND the
 * rank-1 update R[m][k] += x[m] v[k] (m < M, k < K; row stride ldr) that the caller used to issue as a separate addr_ launch
 * (d W_r1[:, :F] += g_br1 (x) b_feat, the second term of the folded colour layer's gradient). */
int upnerf_matvec_rank1(int M, int K, const float* A, int lda, const float* x, float* y, float* R, int ldr, const float* v,
                        void* stream);

/* ---- a15 + a17: depth-prior affine (models/nerf_system.py:169-177) fused with UPNeRFLoss (losses.py:21-64) --------
 * Per-ray inputs only ([R], [R,3], [R,F]); any absent tensor is NULL.  `terms` receives the 8 loss terms in the order
 * l_depth_c, l_feat_c, l_rgb_c, l_depth_f, l_feat_f, l_rgb_f, l_beta, l_alpha (zero where a term does not exist in
 * the phase).  bwd: g_terms[8] are the upstream gradients of the terms (device memory); every non-NULL d_* receives
 * the gradient of sum_k g_terms[k] * terms[k]. */
typedef struct {
  int32_t R, F, fine, has_tw;            /* rays, feature width, fine network present, t_weight_* present */
  float sched, depth_mult, alpha_reg, near, far;
  const float* depth_direct;             /* [R] depth targets given directly (losses.py calling convention), or NULL: */
  const float* inv_depth;                /* [R] mono-depth prior, and */
  const float* depth_scale_rows;         /* [R][2] per-image (scale, shift) rows -> target computed here (a15) */
  const float* s_depth_c; const float* s_depth_f;     /* [R] */
  const float* t_weight_c; const float* t_weight_f;   /* [R] (treated as constants, losses.py:27,48) */
  const float* feat_c; const float* feat_f; const float* feat_gt;   /* [R][F] */
  const float* rgb_c; const float* rgb_f; const float* rgb_gt;      /* [R][3] */
  const float* beta; const float* alpha;                             /* [R] */
  const float* sched_dev;                /* [1] DEVICE or NULL: the multiplier m of the terms is read from here at execution
                                            time (graph replay); `sched` then only selects the phase (== 0, in (0,1), == 1) */
  /* (ABI 9) the sum of the terms a phase uses, as part of the same two launches instead of a select + reduce + product on the
   * caller's side: bit k of term_mask = term k counts (`sum(loss_d.values())`, models/nerf_system.py:183).  upnerf_loss_fwd
   * writes total[0] = sum of the masked terms in term order when `total` is given; upnerf_loss_bwd adds g_total[0] to the
   * upstream gradient of every masked term when `g_total` is given (g_terms may then be NULL). */
  int32_t term_mask, reserved_;
  float* total;                          /* [1] or NULL */
  const float* g_total;                  /* [1] DEVICE or NULL (backward only) */
} upnerf_loss_args;
int upnerf_loss_fwd(const upnerf_loss_args* a, float* depth_out /*[R]*/, float* terms /*[8]*/,
                    float* scratch /*[64*8]*/, void* stream);
typedef struct {
  float* d_depth_scale_rows;             /* [R][2] */
  float* d_depth;                        /* [R] gradient w.r.t. the depth target (depth_direct mode) */
  float* d_s_depth_c; float* d_s_depth_f;
  float* d_feat_c; float* d_feat_f;
  float* d_rgb_c; float* d_rgb_f;
  float* d_beta; float* d_alpha;
} upnerf_loss_grads;
int upnerf_loss_bwd(const upnerf_loss_args* a, const float* g_terms /*[8] device*/, const upnerf_loss_grads* g,
                    void* stream);

/* ---- parameter re-layout: row-major matrices of `src` -> MFMA fragment order in `dst` (optionally transposed) ------
 * One launch re-packs every matrix of a field (forward copies and the transposed copies the backward chain reads).
 * Logical matrix X[r][c], r < rows (multiple of 32), c < cols:
 *     X[r][c] = transpose ? src[src_off + c*src_ld + r] : src[src_off + r*src_ld + c]
 * is written as columns [dst_k0, dst_k0+cols) of a fragment-ordered [rows][dst_kp] matrix at dst + dst_off. */
typedef struct {
  int32_t src_off, src_ld, transpose, rows, cols, dst_off, dst_kp, dst_k0;
} upnerf_frag_desc;
#define UPNERF_MAX_FRAG_DESC 32
int upnerf_frag_copy(const float* src, float* dst, const upnerf_frag_desc* descs /*host*/, int ndesc, void* stream);

/* ---- packed parameter buffer P <-> the network's named parameters (one launch instead of ~40 cat / pad / copy launches) ----
 * pack   (unpack = 0): P[dst_off + r*dst_ld + c] = ptr[r*src_ld + c] for c < cols (padding columns are left alone: start
 *                      from a zeroed P); with `accumulate` the value is added to what P holds (bias of the folded layer).
 * unpack (unpack = 1): ((float*)ptr)[r*src_ld + c] = P[dst_off + r*dst_ld + c]   -- the backward of pack on dP.
 * Descriptors are host memory, `ptr` are device pointers; at most UPNERF_MAX_PACK_DESC per call.
 * The destinations of one call must be disjoint (pack: the P elements of all descriptors, unpack: the parameters): one thread
 * moves one element, so two descriptors that write -- or accumulate into -- the same element in one call race.
 * The elements of one call (sum of rows * cols) are indexed in int: more than 2^31 - 2048 of them are refused (UPNERF_EINVAL). */
#define UPNERF_MAX_PACK_DESC 48
typedef struct {
  const float* ptr;              /* device pointer of the parameter (pack: source, unpack: destination) */
  int32_t rows, cols, src_ld;    /* logical shape and row stride of the parameter */
  int32_t dst_off, dst_ld;       /* float offset and row stride inside P (dst_ld >= cols) */
  int32_t accumulate;            /* pack only */
} upnerf_pack_desc;
int upnerf_pack(float* P, const upnerf_pack_desc* descs, int ndesc, int unpack, void* stream);

/* ---- f16x3 weight re-layout: every matrix of `src` -> scaled fp16 (hi, lo) pairs in MFMA fragment order ------------
 * Same descriptors as upnerf_frag_copy plus `exp_id`: matrices sharing an id share one power-of-two exponent
 * (2^14 / max|.| over all their elements), written to wexp[exp_id].  Destination element (r, k) of a [rows][dst_kp]
 * matrix at float offset dst_off:  byte dst_off*4 + (((r/32)*(dst_kp/16) + k/16)*2 + plane)*1024
 *                                       + (((k/8)%2)*32 + r%32)*16 + (k%8)*2,   plane 0 = hi, 1 = lo.
 * `amax_scratch` [16] floats is zeroed and used inside.
 * perm_fwd / perm_bwd = 1 write the k index inside every 16-deep block in the order in which a converted 32x32 MFMA result
 * presents its rows as the next product's operand -- element j of lane half h holds k = 8(j/4) + 4h + j%4 instead of
 * 8h + j: (k%8) above becomes ((k%16)/8)*4 + k%4 and ((k/8)%2) becomes ((k%16)/4)%2 -- what the register-resident field
 * kernels (upnerf_field_fwd_f16x3 with activations chained through registers) read.
 * wnorm (DEVICE [64] or NULL): receives max_r sum_c |X[r][c]| per descriptor, forward set at [0..), transposed set at [32..). */
typedef struct {
  int32_t src_off, src_ld, transpose, rows, cols, dst_off, dst_kp, dst_k0, exp_id;
} upnerf_frag16_desc;
int upnerf_frag16(const float* src, void* dst_fwd, void* dst_bwd, const upnerf_frag16_desc* fwd, int nfwd,
                  const upnerf_frag16_desc* bwd, int nbwd, float* amax_scratch /*[16]*/, int32_t* wexp /*[16]*/,
                  int perm_fwd, int perm_bwd, float* wnorm, void* stream);

/* ---- a18: fused Adam on a flat fp32 buffer (torch.optim.Adam semantics, utils/optim.py:20-33) ----
 * step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), both formed by the host in double precision and rounded
 * to fp32 (as torch forms them).  dyn2 (DEVICE [step_size, bc2_sqrt], or NULL) overrides the by-value pair at execution
 * time: a captured graph follows the step count and the learning-rate schedule from one replay to the next. */
int upnerf_adam(int64_t n, float* p, const float* g, float* m, float* v, float beta1, float beta2, float eps,
                float step_size, float bc2_sqrt, const float* dyn2, void* stream);
/* The same update over ndesc pieces of the flat buffers, each with its gradient wherever autograd left it: piece j covers
 * elements [off, off + n) of p / m / v and reads the n floats at g.  Bitwise the result of gathering the gradients first. */
#define UPNERF_MAX_ADAM_DESC 96
typedef struct { const float* g; int32_t off, n; } upnerf_adam_desc;
int upnerf_adam_gather(float* p, float* m, float* v, const upnerf_adam_desc* descs /*host*/, int ndesc, float beta1, float beta2,
                       float eps, float step_size, float bc2_sqrt, const float* dyn2, void* stream);

/* ---- per-step scalars for captured HIP graphs: dst[i] = vals[i], i < n <= UPNERF_MAX_SCALARS --------------------------
 * `vals` is HOST memory, copied into the kernel arguments at call time (no staging buffer whose lifetime the caller would
 * have to manage, no host-device synchronisation): one small launch in front of every graph replay carries the learning
 * rates, Adam bias corrections, BARF band weights and the schedule multiplier of that step. */
#define UPNERF_MAX_SCALARS 96
int upnerf_set_scalars(float* dst, int n, const float* vals, void* stream);

/* out[i] = 14 - ceil(log2(max(maxima[i], 1e-30))), i < n <= 64: the power-of-two exponents that upnerf_wgrad16
 * takes (expo_a / expo_b) from the maxima the field kernels track in `amax` / `gmax`; device to device, no
 * host synchronisation (replaces rendering.py's five ATen launches per table). */
int upnerf_scale_exponents(const float* maxima, int n, int32_t* out, void* stream);

/* ---- SSIM of rendered images against their targets (utils/metric.py:23-30: kornia ssim_loss, 3x3 Gaussian window,
 * sigma 1.5, reflect padding, C1 = 1e-4, C2 = 9e-4, eps 1e-12; the reference then takes 1 - 2 * dssim) --------------
 * Pixel (n, c, y, x) of pred / gt is read at element offset n*s[0] + c*s[1] + y*s[2] + x*s[3] of its own strides, so
 * NCHW images and the ray layout [N][H*W][3] are both read in place.  The window's moments are centred
 * (sum w (x - mu)^2, not sum w x^2 - mu^2: fp32 keeps C2 = 9e-4 against the flat patches that way).
 *   ssim[n] = 1 - 2 * mean over (c, y, x) of clamp((1 - s) / 2, 0, 1)      (NaN stays NaN)
 *   map[n][c][y][x] = s, before the clamp (map may be NULL).
 * Two launches: per-tile fp64 partial sums into `scratch`, then a fixed-order finish per image; the order depends on
 * (C, H, W) only, so an image gets the same bits alone or in a batch.  H, W >= 2 (reflect padding).
 * scratch: upnerf_ssim_scratch(a) doubles (a negative return is an error code). */
typedef struct {
  int32_t N, C, H, W;
  const float* pred; const float* gt;
  int64_t pred_stride[4];                /* (n, c, y, x), in elements */
  int64_t gt_stride[4];
  float* ssim;                           /* [N] */
  float* map;                            /* [N][C][H][W] or NULL */
} upnerf_ssim_args;
int upnerf_ssim_scratch(const upnerf_ssim_args* a);
int upnerf_ssim(const upnerf_ssim_args* a, double* scratch, void* stream);

/* ---- LPIPS (AlexNet) of rendered images against their targets (models/nerf_system_optmize.py:184: lpips_alex(gt, img),
 * normalize=False) from weights the caller supplies.  Written from the published lpips 0.1.x definition:
 *   x = (image - shift) / scale per channel, shift = (-.030, -.088, -.188), scale = (.458, .448, .450)
 *   five taps, each after its ReLU: conv 3->64 k11 s4 p2 | maxpool k3 s2, conv 64->192 k5 p2 | maxpool k3 s2,
 *   conv 192->384 k3 p1 | conv 384->256 k3 p1 | conv 256->256 k3 p1          (sizes floor((H + 2p - k) / s) + 1)
 *   d_l = mean over pixels of sum_c w_l[c] * (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2,   LPIPS = sum_l d_l
 * The library allocates nothing: upnerf_lpips_scratch reports the buffers, the caller (upnerf_amd/lpips.py) runs the twelve
 * calls on its stream, so the sequence can sit inside a captured graph.  The render and its target go through the network
 * as ONE batch of 2N images (renders first); no kernel's result for an image depends on the batch around it.
 *
 * upnerf_conv2d: y = [relu](conv(x, w) + bias) as an implicit GEMM on the fp32-input MFMA (exact fp32 products; the
 * patch gather with stride and padding happens on the load into LDS).  Pixel (n, c, y, x) of the input is read at element
 * offset n*s[0] + c*s[1] + y*s[2] + x*s[3], so NCHW images and the ray layout [N][H*W][3] are both read in place; w is
 * [C_out][C_in][k][k], y is dense [N][C_out][H_out][W_out].  scale_in != 0 (C_in == 3 only) applies the scaling layer as a
 * pixel is loaded; the zero padding is then padding of the SCALED image (a padded position contributes 0).
 * Shapes: C_out % 64 == 0 and (C_in, k, stride, pad) one of (3, 11, 4, 2), (64, 5, 1, 2), (192 | 384 | 256, 3, 1, 1);
 * anything else is UPNERF_EUNSUP. */
typedef struct {
  int32_t N, C_in, H, W;
  int32_t C_out, k, stride, pad;
  int32_t relu, scale_in;
  const float* x;
  int64_t x_stride[4];                   /* (n, c, y, x), in elements */
  const float* w; const float* bias;
  float* y;
} upnerf_conv2d_args;
int upnerf_conv2d(const upnerf_conv2d_args* a, void* stream);

/* upnerf_maxpool2d: 3 x 3 window, stride 2, no padding, floor mode, dense NCHW in and out; a NaN in the window gives NaN.
 * H, W >= 3. */
typedef struct {
  int32_t N, C, H, W;
  const float* x;                        /* [N][C][H][W] */
  float* y;                              /* [N][C][(H - 3) / 2 + 1][(W - 3) / 2 + 1] */
} upnerf_maxpool2d_args;
int upnerf_maxpool2d(const upnerf_maxpool2d_args* a, void* stream);

/* upnerf_lpips_dist: d_l of one tap for N image pairs; feat holds the 2N feature maps, the N renders followed by their N
 * targets.  out[n] = d (accumulate == 0) or out[n] + d (accumulate != 0): the caller adds the taps in order, tap 0 first.
 * Norms and differences in fp64; per-tile fp64 partials into `scratch` (N * ceil(H * W / 256) doubles; the part_elems of
 * upnerf_lpips_scratch covers every tap), then a fixed-order finish per pair -- no atomics.  w is not clamped. */
typedef struct {
  int32_t N, C, H, W;
  int32_t accumulate, reserved_;
  const float* feat;                     /* [2N][C][H][W] */
  const float* w;                        /* [C] */
  float* out;                            /* [N] */
} upnerf_lpips_dist_args;
int upnerf_lpips_dist(const upnerf_lpips_dist_args* a, double* scratch, void* stream);

/* upnerf_lpips_scratch: for N pairs of H x W images (H, W >= 31: below that the last taps have no pixel, UPNERF_EINVAL),
 * the element counts of the two fp32 activation buffers the layers alternate between (buffer 0: taps 0, 1, 2, 4; buffer 1:
 * the pooled maps and tap 3; both for 2N images) and of the fp64 partials. */
typedef struct {
  int32_t N, H, W, reserved_;
  int64_t act0_elems, act1_elems, part_elems;   /* out */
} upnerf_lpips_scratch_args;
int upnerf_lpips_scratch(upnerf_lpips_scratch_args* a);

/* ---- scene loading: the per-pixel buffers of datasets/phototourism.py:242-323 (and custom.py, the optimize splits) ----
 * upnerf_scene_rays writes, for every image descriptor, the rows of its column window [x0, x1) in row-major order
 * (row = row0 + (j * (x1 - x0) + i - x0) for pixel (i, j) of the full W x H image):
 *   directions = ((i - cx) / fx, -(j - cy) / fy, -1)            utils/ray.py:5-27 on the integer pixel grid
 *   ray_infos  = (near, far, img_idx)                           (NULL: not written)
 *   pxl        = (j / (H - 1), i / (W - 1))                     torch.linspace(0, n-1, n) / (n-1); (NULL: not written)
 *   rgbs       = pixels[pix_off + (j * W + i) * 3 + c] / 255    ToTensor of uint8 RGB [H][W][3]; (NULL: not written)
 * Every division is a correctly rounded fp32 division, so the values are the CPU tensors' bits.  H, W >= 2.
 * `images` is host memory; it is validated against the capacities in `a` and copied into `table` (device memory of
 * n_images * sizeof(upnerf_scene_image) bytes, stream-ordered) for the one launch. */
typedef struct {
  int32_t W, H;             /* full image size */
  int32_t x0, x1;           /* column window, 0 <= x0 < x1 <= W */
  float fx, fy, cx, cy;
  float near, far, img_idx;
  int32_t reserved_;
  int64_t row0;             /* first output row of the window */
  int64_t pix_off;          /* byte offset of the image's [H][W][3] uint8 pixels in `pixels` */
} upnerf_scene_image;
typedef struct {
  int32_t n_images, reserved_;
  int64_t rows;             /* capacity of every output, in rows */
  int64_t pix_bytes;        /* size of `pixels` */
  const uint8_t* pixels;    /* NULL only when rgbs is NULL */
  float* directions;        /* [rows][3] */
  float* ray_infos;         /* [rows][3] or NULL */
  float* pxl;               /* [rows][2] or NULL */
  float* rgbs;              /* [rows][3] or NULL */
} upnerf_scene_rays_args;
int upnerf_scene_rays(const upnerf_scene_rays_args* a, const upnerf_scene_image* images, void* table, void* stream);

/* upnerf_resize_linear: cv2.resize(src, (W, H)) with INTER_LINEAR on fp32 [h][w][C] maps, C in [1, 512], every map of
 * the table in one launch: half-pixel source coordinates, edge clamping, a horizontal then a vertical blend in fp32
 * (a map whose size does not change is copied, as cv2.resize does).  Optional pre-step on every source pixel:
 *   UPNERF_RESIZE_L2       x / ||x||_2 over C, no epsilon          (phototourism.py:287, 371)
 *   UPNERF_RESIZE_INVDEPTH v = (x < 0 ? 0 : x); v / max_map(v) * scale + bias; max over the map, on the device
 *                          (lines 318-320: scale = 1/near - 1/far, bias = 1/far, rounded to fp32 by the caller)
 * src == dst (in place) is allowed when every map keeps its size and offset.  `maps` is host memory, validated against
 * the capacities and copied into `scratch` (upnerf_resize_scratch(a) bytes of device memory, 16-byte aligned). */
#define UPNERF_RESIZE_PLAIN 0
#define UPNERF_RESIZE_L2 1
#define UPNERF_RESIZE_INVDEPTH 2
typedef struct {
  int32_t h, w;             /* source size */
  int32_t H, W;             /* destination size */
  int64_t src_off;          /* float offset of the source map in src */
  int64_t dst_off;          /* float offset of the destination map in dst */
  float scale, bias;        /* UPNERF_RESIZE_INVDEPTH only */
  int32_t reserved_[2];
} upnerf_resize_map;
typedef struct {
  int32_t n_maps, C, pre, reserved_;
  int64_t src_elems, dst_elems;  /* capacities, in floats */
  const float* src;
  float* dst;
} upnerf_resize_args;
int upnerf_resize_scratch(const upnerf_resize_args* a);
int upnerf_resize_linear(const upnerf_resize_args* a, const upnerf_resize_map* maps, void* scratch, void* stream);

/* ---- validation images (utils/visualization.py; models/nerf_system.py:276-307): uint8 [H][W][3] pictures of the maps of a
 * full-image render, built where the maps are.  Every entry point: nothing allocated, no host read-back, no atomics,
 * fixed-order reductions, all launches on `stream` (capturable).  Pixel p = y * W + x of a map is read at element offset
 * p * stride, so a column of the ray layout [H*W][C] is read in place.  Scratch sizes are in floats (a negative return is
 * an error code); scratch holds only what a call writes before it reads it.
 *
 * upnerf_viz_minmax: out[0] = min, out[1] = max over n values of nan_to_num(x) (NaN -> 0, +inf -> FLT_MAX,
 * -inf -> -FLT_MAX, as np.nan_to_num); two launches (partials per workgroup, one finishing workgroup). */
int upnerf_viz_minmax_scratch(long long n);
int upnerf_viz_minmax(const float* x, long long n, long long stride, float* out, float* scratch, void* stream);

/* upnerf_viz_depth: visualize_depth (visualization.py:7-23), every step in the precision numpy gives it:
 *   x = nan_to_num(value);  (mi, ma) by `range`;  den = (float)((double)ma - (double)mi + 1e-8);
 *   t = (x - mi) / den in fp32, the division correctly rounded;  t = clip(t, 0, 1) by comparisons;
 *   q = (uint8)(255.0f * t), truncating (a NaN t, from an infinite range, gives 0);  rgb[p][c] = lut[q][c].
 * The table is device memory, 256 x 3 bytes, and is copied column for column: a table in cv2's BGR order gives a picture
 * whose first channel is cv2's blue, which is what the reference logs (it hands applyColorMap's BGR output to PIL as is).
 * pre = UPNERF_VIZ_PRED_DEPTH: `x` holds inverse depths and value = the reference's pred_depths (nerf_system.py:249-256),
 *   es = (float)exp((double)depth_scale[0]);  v = inv * es, then + depth_scale[1] (two roundings, no fma);
 *   v < inv_far ? inv_far : v;  d = 1 / v, correctly rounded;  d < near ? near : d   (a NaN stays NaN until nan_to_num)
 * range: UPNERF_VIZ_RANGE_OWN (min / max of x itself, reduced on the device), _HOST (the fields mi, ma), _DEVICE
 * (range_dev[0], range_dev[1], e.g. what upnerf_viz_minmax wrote for another map earlier on the stream). */
#define UPNERF_VIZ_RANGE_OWN 0
#define UPNERF_VIZ_RANGE_HOST 1
#define UPNERF_VIZ_RANGE_DEVICE 2
#define UPNERF_VIZ_PLAIN 0
#define UPNERF_VIZ_PRED_DEPTH 1
typedef struct {
  int32_t H, W, pre, range;
  const float* x; int64_t x_stride;
  const float* depth_scale;  /* [2] (scale, shift) of the image, device memory; UPNERF_VIZ_PRED_DEPTH only */
  float inv_far, near;       /* UPNERF_VIZ_PRED_DEPTH only; inv_far = 1 / far rounded to fp32 by the caller */
  float mi, ma;              /* UPNERF_VIZ_RANGE_HOST */
  const float* range_dev;    /* UPNERF_VIZ_RANGE_DEVICE */
  const uint8_t* lut;        /* [256][3] */
  uint8_t* rgb;              /* [H][W][3] */
  uint8_t* index;            /* [H][W], q itself, or NULL */
  float* value;              /* [H*W], the value before nan_to_num (pred_depths under the pre-step), or NULL */
} upnerf_viz_depth_args;
int upnerf_viz_depth_scratch(const upnerf_viz_depth_args* a);
int upnerf_viz_depth(const upnerf_viz_depth_args* a, float* scratch, void* stream);

/* upnerf_viz_pca: get_pca_img (visualization.py:26-30) of [H*W][F] rows (row r at feat + r * feat_ld, channels contiguous),
 * 1 <= F <= 512:  pc[r][j] = sum_k (feat[r][k] - m[k]) * c[j][k], fp32 accumulation in a fixed order (16-byte loads when
 * F % 4 == 0 and the rows are 16-byte aligned, a scalar path otherwise);  mn / mx = ONE min and ONE max over all rows and
 * the three components;  img[r][j] = (pc - mn) / (mx - mn);  rgb[r][j] = (uint8)min(max(255.0f * img, 0), 255), truncating.
 * Deviation from the reference: a NaN component is left out of mn / mx and written as 0 in both outputs (the reference's
 * whole image turns NaN); so is every component of a map with mx == mn (0 / 0).
 * Three launches: projection + per-workgroup min / max, a one-workgroup finish, normalise + quantise. */
typedef struct {
  int32_t H, W, F, reserved_;
  const float* feat; int64_t feat_ld;
  const float* m;            /* [F] */
  const float* c;            /* [3][F] */
  float* img;                /* [H][W][3], the float image the reference returns */
  uint8_t* rgb;              /* [H][W][3] */
} upnerf_viz_pca_args;
int upnerf_viz_pca_scratch(const upnerf_viz_pca_args* a);
int upnerf_viz_pca(const upnerf_viz_pca_args* a, float* scratch, void* stream);

/* upnerf_viz_rgb: a float map with C = 3 or C = 1 channels to uint8, pixel p channel k read at x[p * stride + k * cstride];
 * q = (uint8)min(max(255.0f * v, 0), 255), truncating (what .mul(255).clamp(0, 255).byte() gives; NaN -> 0); a
 * single-channel map is replicated to three channels. */
typedef struct {
  int32_t H, W, C, reserved_;
  const float* x; int64_t stride, cstride;
  uint8_t* rgb;              /* [H][W][3] */
} upnerf_viz_rgb_args;
int upnerf_viz_rgb(const upnerf_viz_rgb_args* a, void* stream);

/* ---- novel views along a camera path (csrc/path.hip): poses between keyframes, and the rays and blended
 * embedding rows of whole frames without a per-pixel directions buffer.  Added under ABI 11: new symbols only.  Every entry
 * point: arguments refused on the host (-1) before anything is launched, nothing allocated, no host read-back, no atomics,
 * one launch on `stream`.
 *
 * upnerf_path_poses: frame f sits at path parameter u[f] in [0, K-1] (clamped in the kernel; NaN -> 0); k = floor(u) held to
 * k + 1 <= K - 1, s = u - k.  Everything is evaluated in fp64 from the fp32 keys and rounded to fp32 once.
 *   s == 0 (or s == 1 at the last key): the keyframe's twelve floats and its (near, far) are COPIED, bit for bit.
 *   rotation: unit quaternions of keys k, k + 1 (Shepperd's branch on the largest of trace and diagonal, normalised);
 *     q1 negated when q0 . q1 < 0 (shorter arc); slerp with sin((1-s) th) / sin th and sin(s th) / sin th, th = acos(q0 . q1);
 *     normalised lerp when q0 . q1 > 1 - 1e-9; back to a matrix.
 *   translation: UPNERF_PATH_LINEAR (1-s) p1 + s p2; UPNERF_PATH_CATMULL the uniform Catmull-Rom spline through
 *     p(k-1), p(k), p(k+1), p(k+2), the first / last key standing in for a neighbour that does not exist.
 *   near, far: always (1-s) a + s b. */
#define UPNERF_PATH_LINEAR 0
#define UPNERF_PATH_CATMULL 1
typedef struct {
  int32_t K, F, mode, reserved_;
  const float* key_c2w;      /* [K][3][4] */
  const float* key_nf;       /* [K][2] near, far */
  const float* u;            /* [F] */
  float* c2w;                /* [F][3][4] */
  float* nf;                 /* [F][2] */
} upnerf_path_poses_args;
int upnerf_path_poses(const upnerf_path_poses_args* a, void* stream);

/* upnerf_path_rays: rows [row0, row0 + R) of the virtual pixel list [F][H][W]; global row g is frame f = g / (H W), pixel
 * y = (g % (H W)) / W, x = g % W.  Per row:
 *   rays[r] = o | d | near_f | far_f   (the [R][8] rows render_rays slices) with
 *     dir = ((x - cx) / fx, -(y - cy) / fy, -1)      utils/ray.py:22-25 on the integer pixel grid, no half-pixel shift
 *     d = R_f dir / |R_f dir|                        fp32, correctly rounded sqrt and division (as upnerf_pose_rays_fwd)
 *     o = c2w[f][:, 3], (near_f, far_f) = nf[f]      copied
 *   tables[i].out[r][j] = (1 - t[f]) * T[i0[f]][j] + t[f] * T[i1[f]][j], two rounded products and a rounded sum (no fma):
 *     t = 0 and t = 1 return a finite table row bit for bit (up to the sign of a zero entry).
 * i0, i1, t are device arrays, so the host cannot see an index: one outside [0, n_rows) is clamped into it by the kernel.
 * A row's values depend on its global index only: any split of the rows into calls gives the same bits.
 * One thread per 16 bytes written; 16-byte stores for the rays when `rays` is 16-byte aligned and for a table when
 * dim % 4 == 0 and `table` and `out` are 16-byte aligned, scalar accesses otherwise. */
#define UPNERF_PATH_MAX_TABLES 4
#define UPNERF_PATH_MAX_DIM 64
typedef struct {
  const float* table;        /* [n_rows][dim] */
  int32_t dim, n_rows;       /* 1 <= dim <= UPNERF_PATH_MAX_DIM */
  float* out;                /* [R][dim] */
} upnerf_path_table;
typedef struct {
  int32_t F, H, W, n_tables;
  int64_t row0;
  int32_t R, reserved_;
  float fx, fy, cx, cy;
  const float* c2w;          /* [F][3][4] */
  const float* nf;           /* [F][2] */
  const int32_t* i0;         /* [F]; NULL allowed when n_tables == 0, like i1 and t */
  const int32_t* i1;         /* [F] */
  const float* t;            /* [F] */
  float* rays;               /* [R][8] */
  upnerf_path_table tables[UPNERF_PATH_MAX_TABLES];
} upnerf_path_rays_args;
int upnerf_path_rays(const upnerf_path_rays_args* a, void* stream);

/* ---- geometry: the density field on a grid and its iso-surface as a triangle mesh (csrc/mesh.hip).  Added under
 * ABI 11: new symbols only.  Every entry point: arguments refused on the host before anything is launched, nothing allocated,
 * no host read-back, no atomics (the same bits every run), all launches on `stream`.
 *
 * Grid coordinate i of n along an axis = lo + i * ((hi - lo) / (n - 1)), evaluated in fp64 from the fp32 bounds with every
 * operation rounded on its own (lo when n == 1); grid point (x, y, z) has linear index (z * Ny + y) * Nx + x.
 *
 * upnerf_grid_columns: rays that make the field kernels evaluate grid points.  Column c = y * Nx + x; row r of the outputs is
 * column col0 + r:  o[r] = (coord_x, coord_y, 0), d[r] = (0, 0, 1), z[r][s] = coord_z(min(s, Nz - 1)) for s < S -- o + d z is the
 * grid point exactly, and S >= Nz pads a short column with its last depth (the field kernels want S >= 32).  Coordinates are
 * rounded to fp32 once.  A row depends on its column only: any split into calls gives the same bits. */
typedef struct {
  int32_t Nx, Ny, Nz, S;
  float lo[3], hi[3];
  int64_t col0;
  int32_t count, reserved_;
  float* o;                  /* [count][3] */
  float* d;                  /* [count][3] */
  float* z;                  /* [count][S] */
} upnerf_grid_columns_args;
int upnerf_grid_columns(const upnerf_grid_columns_args* a, void* stream);

/* Marching tetrahedra on the Kuhn split of every cell: six tetrahedra round the main diagonal, the same in every cell, so
 * neighbouring cells agree on their face diagonals and no case is ambiguous.  A sample is inside when it is finite and
 * >= level.  Corner c of a cell is its origin + (c & 1, (c >> 1) & 1, c >> 2).  The tables come from the caller
 * (upnerf_amd/geometry.py defines them once); a table that does not describe such a split is UPNERF_EINVAL:
 *   tets[t][i]      corner of vertex i of tetrahedron t; every pair of a tetrahedron's corners must be nested (a & b in {a, b})
 *   edges[s]        offset (dx, dy, dz) in {0, 1}^3 of the far end of edge slot s from the grid point that owns it
 *   tet_edges[e]    the two tetrahedron vertices that tet edge e joins
 *   tris[case]      case = sum of (vertex i inside) << i: number of triangles (0..2), then three tet edges per triangle
 * Vertices are the crossed edges in (owner point, slot) order:  t = (level - v0) / (v1 - v0) in fp32 (0.5 when an end is not
 * finite), position = p0 + t (p1 - p0) on fp64 grid coordinates rounded once, normal = -(g0 + t (g1 - g0)) normalised, g = the
 * grid's central differences (one-sided at the border) over the spacing; a gradient that is zero or not finite gives (0, 0, 0).
 * Triangles come in (cell origin, tetrahedron, triangle) order and index the vertices.
 *
 * upnerf_mtet_scratch(Nx, Ny, Nz): bytes of scratch (16-byte aligned device memory); UPNERF_EINVAL for an axis with fewer than
 *   two points, or when 7 Nx Ny Nz or 12 x cells does not fit int32 (the counts are int32).
 * upnerf_mtet_count: fills the scratch (edge masks, triangle counts, their exclusive scans) and writes totals[0] = vertices,
 *   totals[1] = triangles (device memory).  Reads Nx..grid and tab of the arguments.
 * upnerf_mtet_emit: writes the mesh from the scratch of a count of the SAME grid, level and tables.  n_vertices / n_faces are
 *   what that count reported; a capacity below them is UPNERF_EINVAL and nothing is written; the kernels hold every store to
 *   the capacities besides. */
typedef struct {
  int8_t tets[6][4];
  int8_t edges[7][3];
  int8_t tet_edges[6][2];
  int8_t tris[16][7];
  int8_t reserved_[7];
} upnerf_mtet_tables;
typedef struct {
  int32_t Nx, Ny, Nz;
  float level;
  float lo[3], hi[3];        /* bounds: grid point (0, 0, 0) and (Nx - 1, Ny - 1, Nz - 1); hi > lo (emit only) */
  const float* grid;         /* [Nz][Ny][Nx] */
  upnerf_mtet_tables tab;
  int32_t n_vertices, n_faces, cap_vertices, cap_faces;   /* emit only, like the outputs */
  float* vertices;           /* [cap_vertices][3] */
  float* normals;            /* [cap_vertices][3] */
  int32_t* faces;            /* [cap_faces][3] */
  int32_t flags, reserved2_; /* UPNERF_MTET_* bits (count and emit must agree); 0: everything above, bit for bit */
} upnerf_mtet_args;
/* UPNERF_MTET_SKIP_NONFINITE: cells that touch a sample nobody observed emit nothing.  An edge is crossed only if BOTH its ends
 * are finite (and one is inside, the other not), and a tetrahedron is triangulated only if all FOUR of its corners are finite --
 * so every emitted triangle indexes emitted vertices, and no wall is built where finite samples meet non-finite ones (the
 * back of a truncation shell, the edge of a frustum: csrc/tsdf.hip).  A vertex may remain that no triangle uses.  Any other
 * bit in `flags` is UPNERF_EINVAL. */
#define UPNERF_MTET_SKIP_NONFINITE 1
long long upnerf_mtet_scratch(int Nx, int Ny, int Nz);
int upnerf_mtet_count(const upnerf_mtet_args* a, void* scratch, int32_t* totals /*[2] device*/, void* stream);
int upnerf_mtet_emit(const upnerf_mtet_args* a, const void* scratch, void* stream);

/* ---- empty-space skipping: a bit-packed occupancy grid and the rays of a frame walked through it (csrc/occupancy.hip;
 * DESIGN.md 2.25).  Added under ABI 11: new symbols only.  Every entry point: arguments refused on the host before anything is
 * launched, nothing allocated, no host read-back, no atomics (the same bits every run), all launches on `stream`.
 *
 * Geometry: that of the density grid.  A grid of Nx x Ny x Nz points spans `lo`..`hi` inclusively; its CELLS are the
 * Cx x Cy x Cz = (Nx-1) x (Ny-1) x (Nz-1) boxes between the points (the cells marching tetrahedra walks), half-open [i, i+1)
 * per axis.  Plane i of an axis = lo + i * ((hi - lo) / C), in fp64 from the fp32 bounds.
 *
 * The packed grid is upnerf_occ_words(Cx, Cy, Cz) uint32 words (UPNERF_EINVAL for an axis without a cell or more than 2^31 - 1
 * cells):  first ceil(Cx Cy Cz / 32) words of FINE bits -- cell (x, y, z) is bit (z * Cy + y) * Cx + x, bit b of word b / 32
 * at position b % 32 -- then ceil(Bx By Bz / 32) words of BRICK bits, B = ceil(C / 8): brick (bx, by, bz) is bit
 * (bz * By + by) * Bx + bx of that part and is set iff any cell of the 8 x 8 x 8 block is.  Unused high bits are zero.
 *
 * upnerf_occ_build: from `grid` [Cz+1][Cy+1][Cx+1] (a cell is occupied iff any of its 8 corners is finite and >= level, the
 *   comparison of upnerf_mtet_count: every triangle of the mesh at that level lies in an occupied cell) or from `cells`
 *   [Cz][Cy][Cx] (non-zero = occupied); exactly one of the two is given.  Then `dilate` rounds of 26-neighbour dilation, then
 *   the packing.  `scratch`: upnerf_occ_build_scratch(Cx, Cy, Cz) bytes. */
typedef struct {
  int32_t Cx, Cy, Cz, dilate;
  float level;               /* with `grid`; a NaN is refused */
  int32_t reserved_;
  const float* grid;         /* [Cz+1][Cy+1][Cx+1] or NULL */
  const uint8_t* cells;      /* [Cz][Cy][Cx] or NULL */
  uint32_t* words;           /* [upnerf_occ_words] */
  void* scratch;
} upnerf_occ_build_args;
long long upnerf_occ_words(int Cx, int Cy, int Cz);
long long upnerf_occ_build_scratch(int Cx, int Cy, int Cz);
int upnerf_occ_build(const upnerf_occ_build_args* a, void* stream);

/* upnerf_occ_spans: one thread per ray row o | d | near | far (d need not be unit length: t is in units of d).  The ray is clipped
 * to the box by the slab test and to [near, far], then walked cell by cell (Amanatides-Woo) -- brick by brick where the brick
 * bit is clear.  Every t is (plane - o) / d evaluated in fp64 from the plane's index (no running sum) and rounded to fp32 once.
 *   t0[r] = entry into the first occupied cell (>= near), t1[r] = exit from the last one (<= far), hit[r] = 1 iff t1 > t0 in
 *   fp32; a miss has hit = 0, t0 = t1 = far.
 * An axis with d == 0 never produces a t: the ray is a miss when o lies outside [lo, hi) of that axis, and keeps its cell
 * otherwise.  A ray with a NaN in it is a miss. */
typedef struct {
  int32_t Cx, Cy, Cz, R;
  float lo[3], hi[3];        /* hi > lo, finite */
  const uint32_t* words;
  const float* rays;         /* [R][8] */
  float* t0;                 /* [R] */
  float* t1;                 /* [R] */
  uint8_t* hit;              /* [R] */
} upnerf_occ_spans_args;
int upnerf_occ_spans(const upnerf_occ_spans_args* a, void* stream);

/* upnerf_occ_compact: the rows with hit != 0, in ascending order (block scan, scan of the block sums, emit):
 *   index[k] = source row of the k-th hit, rays_c[k] = rays[index[k]] with near, far replaced by t0, t1,
 *   tables[i].out[k] = tables[i].table[index[k]] (here `table` holds one row per RAY, [R][dim]; n_rows is ignored),
 *   count[0] = number of hits (device memory).  Rows k >= count[0] of the outputs are not written.
 * `scratch`: upnerf_occ_compact_scratch(R) bytes, 16-byte aligned. */
typedef struct {
  int32_t R, n_tables;
  const uint8_t* hit;        /* [R], every byte 0 or 1 (what upnerf_occ_spans writes) */
  const float* t0;           /* [R] */
  const float* t1;           /* [R] */
  const float* rays;         /* [R][8] */
  float* rays_c;             /* [R][8] */
  int32_t* index;            /* [R] */
  int32_t* count;            /* [1] */
  void* scratch;
  upnerf_path_table tables[UPNERF_PATH_MAX_TABLES];
} upnerf_occ_compact_args;
long long upnerf_occ_compact_scratch(int R);
int upnerf_occ_compact(const upnerf_occ_compact_args* a, void* stream);

/* upnerf_occ_scatter: the results of the n_hit compacted rows back to the R full-length rows.  Row r finds itself in the
 * ascending `index` (binary search): rgb[r] = rgb_c[k], depth[r] = depth_c[k] when index[k] == r; any other row is a miss:
 * rgb[r] = (background, background, background), depth[r] = rays[r][7], the far of that ray.  n_hit is a host value (the
 * caller read count[0] to size the render); n_hit == 0 makes every row a miss. */
typedef struct {
  int32_t R, n_hit;
  float background;
  int32_t reserved_;
  const int32_t* index;      /* [n_hit] ascending; NULL allowed when n_hit == 0, like rgb_c */
  const float* rays;         /* [R][8]; NULL allowed when depth is NULL */
  const float* rgb_c;        /* [n_hit][3] */
  const float* depth_c;      /* [n_hit]; NULL allowed when depth is NULL or n_hit == 0 */
  float* rgb;                /* [R][3] */
  float* depth;              /* [R] or NULL */
} upnerf_occ_scatter_args;
int upnerf_occ_scatter(const upnerf_occ_scatter_args* a, void* stream);

/* ---- surface normals from the analytic density gradient (csrc/normals.hip, csrc/viz.hip).  Added under
 * ABI 11: new symbols only.  Every entry point: arguments refused on the host before anything is launched, nothing allocated,
 * no host read-back, no atomics (the same bits every run), one launch on `stream`.
 *
 * upnerf_density_grad: sigma[m] = the shared density (after the softplus) of the field (L, P) at points[m], and
 * grad[m] = d sigma / d x there, in world space.  One fused launch: encoding, trunk, share_sigma and the walk back through
 * the transposed weights happen per 64-point tile in LDS and registers; nothing of size M x W is read or written.  fp32 MFMA
 * whatever the field mode of the training step.  P: the parameters with the matrices in fragment order (what
 * upnerf_field_fwd reads), PT: the transposed fragments (what upnerf_field_bwd reads).  Any M >= 1; a point's outputs do not
 * depend on M or on its position in the batch, bit for bit.  softplus'(x) is the sigmoid, and 1 where x > 20 (the branch on
 * which the softplus returns x). */
typedef struct {
  int32_t M, reserved_;
  const float* points;       /* [M][3] */
  const float* P;
  const float* PT;
  float wk_xyz[10];          /* BARF band weights of the xyz encoding */
  float* sigma;              /* [M] */
  float* grad;               /* [M][3] */
} upnerf_density_grad_args;
int upnerf_density_grad(const upnerf_layout* L, const upnerf_density_grad_args* a, void* stream);

/* upnerf_normal_composite: normal[r] = normalise(sum_i w[r][i] * (-grad[r*S+i] / |grad[r*S+i]|)).  A term is zero where the
 * fp32 length of the gradient is 0 or not finite (a NaN or infinite component, or an overflow of the squares) or the weight
 * is not finite; the result is (0, 0, 0) where the length of the sum is 0 or not finite.  Never NaN.  One ray per wave, fixed
 * summation order.  R * S < 2^31. */
typedef struct {
  int32_t R, S;
  const float* grad;         /* [R*S][3] */
  const float* w;            /* [R][S], upnerf_composite_fwd's w_s */
  float* normal;             /* [R][3], unit length or (0, 0, 0) */
} upnerf_normal_composite_args;
int upnerf_normal_composite(const upnerf_normal_composite_args* a, void* stream);

/* upnerf_viz_normals: normals [H*W][3] to packed RGB8.  n' = rot . n when `rot` is given (row-major 3 x 3 in device memory,
 * e.g. a world-to-camera rotation; every product and sum rounded on its own, (r0 nx + r1 ny) + r2 nz), else n;
 * channel = q((n' + 1) / 2) with q = upnerf_viz_rgb's rule ((uint8)min(max(255.0f * v, 0), 255), truncating; NaN -> 0).
 * A normal whose three components are exactly zero is drawn as (128, 128, 128). */
typedef struct {
  int32_t H, W;
  const float* n;            /* [H*W][3] */
  const float* rot;          /* [3][3] DEVICE, or NULL */
  uint8_t* rgb;              /* [H][W][3] */
} upnerf_viz_normals_args;
int upnerf_viz_normals(const upnerf_viz_normals_args* a, void* stream);

/* ---- depth-map fusion: a truncated signed distance volume (TSDF) from rendered depth maps (csrc/tsdf.hip).
 * Added under ABI 11: new symbols only.  Every entry point: arguments refused on the host before anything is launched, nothing
 * allocated, no host read-back, no atomics and no cross-thread reduction (the same bits every run), one launch on `stream`.
 *
 * The volume lives on the grid of the mesher: Nx x Ny x Nz points over lo..hi, point (x, y, z) at linear index
 * (z * Ny + y) * Nx + x and at the grid coordinates defined above (fp64 from the fp32 bounds, rounded to fp32 ONCE: that fp32
 * point p is what everything below sees).  Four fp32 volumes: `tsdf` (the running mean of the truncated distance in units of
 * `trunc`, in [-1, 1]; the caller initialises it, 1 by convention), `weight` (the sum of the view weights, 0 = never observed),
 * and optionally `rgb` [..][3] with `rgb_weight`, a volume of its OWN for the colour's weight (not packed into anything): colour
 * is fused in a narrower set of views than distance (rule 7), so its mean needs its own denominator.
 *
 * upnerf_tsdf_integrate folds views[0 .. n_views) into the volume, one thread per voxel, views in index order, all in fp32,
 * every operation rounded on its own (no fma).  A view is a pinhole camera looking down its -z axis with +y up
 * (c2w = [R | c] row-major 3 x 4, utils/ray.py) and a map of EUCLIDEAN distances along unit-length rays (`s_depth_*`):
 *   1. pc = R^T (p - c), zc = -pc.z; the view is skipped unless zc > 0.
 *   2. u = fx * pc.x / zc + cx, v = cy - fy * pc.y / zc (pixel centres at integers: no half-pixel shift).
 *   3. iu = floor(u + 0.5), jv = floor(v + 0.5); skipped outside [0, W) x [0, H).
 *   4. d = depth[jv * W + iu]; skipped if d is not finite or d <= 0, or if the view has an opacity map and its pixel is not
 *      >= min_opacity (a NaN opacity is skipped).
 *   5. r = |p - c|, sdf = d - r; skipped if sdf < -trunc (behind the band; a NaN is skipped too).
 *   6. val = min(1, sdf / trunc); w = 1 (weight_mode 0) or the pixel's opacity (weight_mode 1, which needs the map of every
 *      view; skipped unless w > 0);  Wn = W + w;  tsdf += (val - tsdf) * (w / Wn);  W = Wn.
 *   7. if the volume and the view both have colour and sdf <= trunc:  Cn = C + w;  rgb += (pixel - rgb) * (w / Cn);  C = Cn.
 * A voxel's accumulators stay in registers over the views of a launch and each step rounds to fp32 exactly as a store would,
 * so folding a list of views in one launch or in any split into consecutive launches gives the same bits.
 * UPNERF_EINVAL: null `tsdf` / `weight` / `depth`, `rgb` without `rgb_weight`, n_views outside [1, UPNERF_TSDF_MAX_VIEWS],
 * trunc not > 0 or not finite, a NaN min_opacity, weight_mode outside {0, 1} or 1 with a view that has no opacity map, an axis
 * < 2, Nx Ny Nz beyond int32, bounds that are not finite with hi > lo, a view with W or H < 1 or W H beyond int32. */
#define UPNERF_TSDF_MAX_VIEWS 8
typedef struct {
  float c2w[12];             /* row-major 3 x 4 camera-to-world */
  float fx, fy, cx, cy;
  int32_t W, H;
  const float* depth;        /* [H*W] */
  const float* opacity;      /* [H*W] or NULL */
  const float* rgb;          /* [H*W][3] or NULL */
} upnerf_tsdf_view;
typedef struct {
  int32_t Nx, Ny, Nz, n_views;
  float lo[3], hi[3];
  float trunc, min_opacity;
  int32_t weight_mode, reserved_;
  float* tsdf;               /* [Nz][Ny][Nx] */
  float* weight;             /* [Nz][Ny][Nx] */
  float* rgb;                /* [Nz][Ny][Nx][3] or NULL */
  float* rgb_weight;         /* [Nz][Ny][Nx], with rgb */
  upnerf_tsdf_view views[UPNERF_TSDF_MAX_VIEWS];
} upnerf_tsdf_integrate_args;
int upnerf_tsdf_integrate(const upnerf_tsdf_integrate_args* a, void* stream);

/* upnerf_tsdf_surface: the grid upnerf_mtet_* meshes at level 0 with UPNERF_MTET_SKIP_NONFINITE:  out[i] = -tsdf[i] where
 * weight[i] >= min_weight -- positive behind the surface, so the mesher's normals (towards lower values) point at the cameras --
 * and NaN elsewhere (a NaN weight included).  n in [1, 2^31). */
typedef struct {
  int64_t n;
  float min_weight;
  int32_t reserved_;
  const float* tsdf;         /* [n] */
  const float* weight;       /* [n] */
  float* out;                /* [n] */
} upnerf_tsdf_surface_args;
int upnerf_tsdf_surface(const upnerf_tsdf_surface_args* a, void* stream);

/* upnerf_tsdf_sample: the colour volume at V points, trilinear and weight-aware.  Per axis g = (p - lo) / (hi - lo) * (N - 1)
 * clamped to [0, N - 1], i = min(floor(g), N - 2), f = g - i (fp32); a corner counts with its trilinear weight if its
 * rgb_weight is > 0 and with 0 otherwise, and the result is the weighted sum over the sum of the weights that count: corners
 * without colour are left out and the rest renormalised.  (0.5, 0.5, 0.5) where that sum is not > 0; a point with a NaN in it
 * gives that grey as well.  V >= 1, sizes as for upnerf_tsdf_integrate. */
typedef struct {
  int32_t Nx, Ny, Nz, V;
  float lo[3], hi[3];
  const float* rgb;          /* [Nz][Ny][Nx][3] */
  const float* rgb_weight;   /* [Nz][Ny][Nx] */
  const float* points;       /* [V][3] */
  float* out;                /* [V][3] */
} upnerf_tsdf_sample_args;
int upnerf_tsdf_sample(const upnerf_tsdf_sample_args* a, void* stream);

/* ---- DINO ViT descriptors and their PCA (csrc/dino.hip, upnerf_amd/dino.py): the pieces of a pre-norm vision
 * transformer that upnerf_linear does not cover, and the moments of the descriptor PCA.  Added under ABI 11: new symbols only.
 * Every entry point: arguments refused on the host before anything is launched, nothing allocated, no host read-back, no atomics
 * and a fixed summation order (the same bits every run), all launches on `stream`.
 *
 * upnerf_vit_patches: rows[t][(c * 8 + ky) * 8 + kx] = ((v / 255 or v) - mean[c]) / std[c] with v = pixel (ty * stride + ky,
 * tx * stride + kx) of channel c, t = ty * w0 + tx, h0 = 1 + (H - 8) / stride, w0 likewise: the operand of the patch projection
 * as a GEMM against the flattened [D][3 * 8 * 8] convolution weight.  u8 != 0: the image is uint8 and divided by 255 first;
 * else fp32, taken as already in [0, 1].  Pixels right of or below the last full patch are never read. */
#define UPNERF_VIT_PATCH 8
#define UPNERF_VIT_HEAD_DIM 64
typedef struct {
  int32_t H, W, stride, u8;
  const void* image;         /* [H][W][3] uint8 or fp32 */
  float mean[3], std[3];
  float* rows;               /* [h0 * w0][192] */
} upnerf_vit_patches_args;
int upnerf_vit_patches(const upnerf_vit_patches_args* a, void* stream);

/* upnerf_vit_embed: tok[0][:] = cls[:] + pos[0][:]; tok[n][:] += pos[n][:] for 1 <= n < N (rows 1.. hold the patch projection). */
int upnerf_vit_embed(int N, int D, const float* cls, const float* pos, float* tok, void* stream);

/* upnerf_layernorm: y[m][:] = (x[m][:] - mean) / sqrt(var + eps) * gamma + beta, var the mean of the squared CENTRED values.
 * D <= 1024, D % 4 == 0 (else UPNERF_EUNSUP); one wave per row, the row in registers, the two sums in fp64.  y may be x. */
int upnerf_layernorm(int M, int D, const float* x, int ldx, const float* gamma, const float* beta, float eps, float* y, int ldy,
                     void* stream);

/* upnerf_vit_attention: out[n][h * 64 + :] = softmax_j(scale * q[n][h] . k[j][h]) v[j][h], n, j < N, for each head h < heads.
 * q, k, v: row n of head h starts at p + n * ld + h * 64 (for a fused [N][3 D] qkv buffer: q = qkv, k = qkv + D, v = qkv + 2 D,
 * ld = 3 D); pointers 16-byte aligned, strides multiples of 4.  head_dim must be 64 (UPNERF_EUNSUP).  Streaming softmax: no
 * N x N buffer exists; N is arbitrary.  out must not overlap q, k or v. */
typedef struct {
  int32_t N, heads, head_dim, reserved_;
  const float* q; const float* k; const float* v;
  int64_t ldq, ldk, ldv;
  float scale, reserved2_;
  float* out;                /* [N][ldo], columns [0, heads * 64) written */
  int64_t ldo;
} upnerf_vit_attention_args;
int upnerf_vit_attention(const upnerf_vit_attention_args* a, void* stream);

/* upnerf_vit_gelu: x = x / 2 * erfc(-x / sqrt(2)) in place (the exact erf form of GELU), n elements.
 * upnerf_vit_residual: x += y, n elements. */
int upnerf_vit_gelu(float* x, long long n, void* stream);
int upnerf_vit_residual(float* x, const float* y, long long n, void* stream);

/* upnerf_pca_fit: the moments of the PCA of T descriptor rows of width D (D <= 1024), each row divided by its L2 norm as it is
 * read (no epsilon: a zero row gives NaN, as the division it restates).  mean[D] (fp32) = the column mean; gram[D][D] (fp64) =
 * sum_t (u_t - mean)(u_t - mean)^T with the fp64 mean: fp64 partials per chunk of 1024 rows into `scratch`
 * (upnerf_pca_fit_scratch(T, D) doubles), summed in chunk order by a second pass.  The eigenproblem is the caller's. */
typedef struct {
  int32_t T, D;
  const float* x; int64_t ldx;
  float* mean;               /* [D] */
  double* gram;              /* [D][D] */
} upnerf_pca_fit_args;
long long upnerf_pca_fit_scratch(int T, int D);
int upnerf_pca_fit(const upnerf_pca_fit_args* a, double* scratch, void* stream);

/* ---- DPT-Large inverse depth (csrc/dpt.hip, upnerf_amd/dpt.py): the convolutional decoder and the resizes
 * around the network; the backbone is the ViT entry points above.  Added under ABI 11: new symbols only.  Every entry point:
 * arguments refused on the host before anything is launched, nothing allocated, no host read-back, no atomics and a fixed
 * summation order (the same bits every run), all launches on `stream`.
 *
 * Maps are NHWC: pixel (y, x) of an H x W map with C channels is the C floats at p + (y * W + x) * ld (ld >= C: a row stride), so
 * the token rows of the backbone are maps and every 1 x 1 convolution is upnerf_linear.
 *
 * upnerf_conv3x3: y = [relu]( conv(pre_relu ? relu(x) : x, w) + bias + res ), kernel 3 x 3, padding 1 (zeros, of the map AFTER the
 * pre-ReLU), stride 1 or 2 (else UPNERF_EUNSUP); output (H - 1) / stride + 1 by (W - 1) / stride + 1.  w is [C_out][3][3][C_in]
 * (ky, kx, ci; the checkpoint's [C_out][C_in][3][3] relaid once by the caller).  C_in, C_out: multiples of 32 up to 1024 (else
 * UPNERF_EUNSUP).  bias [C_out] and res (an output-sized map, row stride ldr) may be NULL.  Pointers 16-byte aligned, strides
 * multiples of 4.  y must not overlap x; res may overlap neither (UPNERF_EINVAL).  An implicit GEMM on the fp32-input MFMA: exact
 * fp32 products summed as one fp32 chain in the order (ky, kx, ci). */
typedef struct {
  int32_t H, W, C_in, C_out, stride, pre_relu, relu, reserved_;
  const float* x; int64_t ldx;
  const float* w;
  const float* bias;
  const float* res; int64_t ldr;
  float* y; int64_t ldy;
} upnerf_conv3x3_args;
int upnerf_conv3x3(const upnerf_conv3x3_args* a, void* stream);

/* upnerf_upsample2x: bilinear, H x W -> 2 H x 2 W, align_corners=True, in torch's arithmetic: fp32 scale = (in - 1) / (out - 1)
 * (0 for in = 1), src = scale * dst, i0 = (int)src, i1 = min(i0 + 1, in - 1).  16-byte accesses when C, the strides and the
 * pointers allow it, element-wise otherwise.  y must not overlap x. */
typedef struct {
  int32_t H, W, C, reserved_;
  const float* x; int64_t ldx;
  float* y; int64_t ldy;
} upnerf_upsample2x_args;
int upnerf_upsample2x(const upnerf_upsample2x_args* a, void* stream);

/* upnerf_depth_to_space: the scatter half of a transposed convolution whose kernel equals its stride s (2 or 4, else
 * UPNERF_EUNSUP): y[(py * s + dy, px * s + dx)][c] = x[(py, px)][(dy * s + dx) * C + c] + bias[c], x the H x W map with s * s * C
 * columns that upnerf_linear makes against the weight relaid to [(dy, dx, c_out)][c_in].  bias may be NULL.  y must not overlap x. */
typedef struct {
  int32_t H, W, C, s;
  const float* x; int64_t ldx;
  const float* bias;
  float* y; int64_t ldy;
} upnerf_depth_to_space_args;
int upnerf_depth_to_space(const upnerf_depth_to_space_args* a, void* stream);

/* upnerf_resize_cubic: [h][w][C] -> [H][W][C] (contiguous, C = 1 or 3, else UPNERF_EUNSUP), cubic convolution with A = -0.75,
 * half-pixel centres (src = (dst + 0.5) * in / out - 0.5 in fp32), the four taps per axis clamped to the image, no antialiasing:
 * cv2's INTER_CUBIC on a float image and torch's bicubic with align_corners=False.  u8 != 0: x is uint8 and divided by 255 as it
 * is read.  affine != 0: (v - mean[c]) / std[c] on the way out (std > 0, else UPNERF_EINVAL). */
typedef struct {
  int32_t h, w, H, W, C, u8, affine, reserved_;
  const void* x;
  float mean[3], std[3];
  float* y;
} upnerf_resize_cubic_args;
int upnerf_resize_cubic(const upnerf_resize_cubic_args* a, void* stream);

/* upnerf_vit_patches16: rows[t][(c * P + ky) * P + kx] = image[(ty * P + ky, tx * P + kx)][c], t = ty * (W / P) + tx, P = patch
 * (1..64): the operand rows of a P x P patch convolution at stride P from an fp32 [H][W][3] image, taken as it is (the general-
 * patch sibling of upnerf_vit_patches).  Pixels right of or below the last full patch are never read. */
typedef struct {
  int32_t H, W, patch, reserved_;
  const float* image;        /* [H][W][3] */
  float* rows;               /* [(H / P) * (W / P)][3 * P * P] */
} upnerf_vit_patches16_args;
int upnerf_vit_patches16(const upnerf_vit_patches16_args* a, void* stream);

/* ---- a baked scene: rays marched through a colour-density grid, the field never touched (csrc/baked.hip).
 * Added under ABI 11: new symbols only.  Arguments refused on the host before anything is launched, nothing allocated, no host
 * read-back, no atomics, one launch on `stream`; the same bits every run and however the rays are cut into launches.
 *
 * Geometry: that of the occupancy grid above.  `rgbs` [Cz+1][Cy+1][Cx+1][4] holds r, g, b, sigma at the grid points (16-byte
 * aligned); `words` are the upnerf_occ_words(Cx, Cy, Cz) words of a grid in which every cell with a clear bit has eight
 * corners that are (0, 0, 0, 0): the bits say where the integrand is zero and never change the picture.
 *
 * One thread per ray row o | d | near | far (d need not be unit length).  All fp32:
 *   K = ceilf((far - near) / step), held to UPNERF_BAKED_MAX_SAMPLES; t_k = fmaf(k + 0.5, step, near), k = 0 .. K-1;
 *   p = fmaf(t_k, d, o) per axis; g = (p - lo) * inv per axis, inv = (float)(C / ((double)hi - (double)lo));
 *   a sample with an axis on which NOT (0 <= g <= C) contributes nothing; i = min((int)floorf(g), C - 1), f = g - i;
 *   v = the trilinear blend of the eight corners of cell i, four channels: along x first, then y, then z, each blend
 *   fmaf(f, b - a, a);
 *   delta = step * sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))); e = expf(-delta * v.sigma); alpha = 1 - e; w = T * alpha;
 *   rgb += w * v.rgb (fmaf), depth = fmaf(w, t_k, depth), opacity += w; T *= 1 - alpha; in sample order, T starts at 1;
 *   stop > 0: the ray ends after the sample that brought T below `stop`;
 *   at the end rgb = fmaf(1 - opacity, background, rgb), depth = fmaf(1 - opacity, far, depth).
 * A ray with a NaN or an infinity among its eight numbers, or with NOT (far > near), is a miss: rgb = background, depth = far, opacity = 0.
 * Samples are skipped only where their OWN cell, computed as above, has a clear bit (or lies in a brick with a clear bit, or
 * outside the box): the result is, bit for bit, that of visiting every sample. */
#define UPNERF_BAKED_MAX_SAMPLES 4194304
typedef struct {
  int32_t Cx, Cy, Cz, R;
  float lo[3], hi[3];        /* hi > lo, finite */
  float step;                /* > 0, finite */
  float background;          /* finite */
  float stop;                /* >= 0, < 1; 0 = never */
  int32_t reserved_;
  const float* rgbs;         /* [Cz+1][Cy+1][Cx+1][4], 16-byte aligned */
  const uint32_t* words;     /* [upnerf_occ_words(Cx, Cy, Cz)] */
  const float* rays;         /* [R][8], 16-byte aligned */
  float* rgb;                /* [R][3] */
  float* depth;              /* [R] */
  float* opacity;            /* [R] */
} upnerf_baked_render_args;
int upnerf_baked_render(const upnerf_baked_render_args* a, void* stream);

/* upnerf_baked_pack: the grid of a baked scene from its parts.  rgbs[n] = (rgb[n], sigma[n]) where sigma[n] is finite, > 0 and
 * >= level, else (0, 0, 0, 0); `rgb` NULL: colour (0, 0, 0).  kept[n] (optional) = 1 / 0 accordingly.  One thread per point. */
typedef struct {
  int64_t n;
  float level;               /* not NaN */
  int32_t reserved_;
  const float* sigma;        /* [n] */
  const float* rgb;          /* [n][3] or NULL */
  float* rgbs;               /* [n][4], 16-byte aligned */
  uint8_t* kept;             /* [n] or NULL */
} upnerf_baked_pack_args;
int upnerf_baked_pack(const upnerf_baked_pack_args* a, void* stream);

/* ---- a baked scene with view dependence: per grid point the coefficients of a real spherical-harmonic expansion of the colour
 * over the viewing direction, evaluated for each ray's own direction (csrc/baked.hip).  Added under ABI 11: new
 * symbols only.  Degree 1 or 2, nb = (degree + 1)^2 = 4 or 9 basis functions; degree 0 is upnerf_baked_render on `rgbs`.
 *
 * The record of a grid point, aligned to its own size -- the stored record is the definition:
 *   degree 1: 32 bytes: 12 fp16 coefficients in bytes 0..23, fp32 sigma at byte 24;
 *   degree 2: 64 bytes: 27 fp16 coefficients in bytes 0..53, fp32 sigma at byte 56;
 * coefficients channel-major, k[c][j] is half c * nb + j (c = r, g, b; j = 0 .. nb-1); every other byte is zero; a dropped
 * point is an all-zero record, so a cell with a clear bit has eight exact zeros of sigma as it has in `rgbs`.
 *
 * The basis of a unit direction (x, y, z), the constants rounded to fp32, every operation fp32:
 *   Y0 = 0.28209479177387814;  Y1 = -0.4886025119029199 * y;  Y2 = 0.4886025119029199 * z;  Y3 = -0.4886025119029199 * x;
 *   Y4 = 1.0925484305920792 * (x * y);  Y5 = -1.0925484305920792 * (y * z);
 *   Y6 = 0.31539156525252005 * fmaf(2 z, z, -fmaf(x, x, y * y));  Y7 = -1.0925484305920792 * (x * z);
 *   Y8 = 0.5462742152960396 * fmaf(x, x, -(y * y)).
 *
 * upnerf_baked_sh_render: upnerf_baked_render in everything (lattice, skipping, blend, compositing, misses) but the four
 * channels of a corner.  Once per ray: len = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) (delta = step * len, as above),
 * (x, y, z) = d / len per component, Y_0 .. Y_{nb-1} as above.  Per corner of a visited sample: the halves converted exactly to
 * fp32; col[c] = acc after acc = 0, acc = fmaf(Y_j, k[c][j], acc) for j = 0 .. nb-1 in that order; the corner is
 * (col[0], col[1], col[2], sigma).  The trilinear blend is that of upnerf_baked_render; then the three blended colours are
 * clamped, v = fminf(fmaxf(v, 0), 1), and composited as above.  (A ray with d = 0 has no direction: its colours clamp to 0 and
 * its alpha is 0.) */
typedef struct {
  int32_t Cx, Cy, Cz, R;
  float lo[3], hi[3];        /* hi > lo, finite */
  float step;                /* > 0, finite */
  float background;          /* finite */
  float stop;                /* >= 0, < 1; 0 = never */
  int32_t degree;            /* 1 or 2 */
  const uint8_t* records;    /* [Cz+1][Cy+1][Cx+1][32 | 64], aligned to the record size */
  const uint32_t* words;     /* [upnerf_occ_words(Cx, Cy, Cz)] */
  const float* rays;         /* [R][8], 16-byte aligned */
  float* rgb;                /* [R][3] */
  float* depth;              /* [R] */
  float* opacity;            /* [R] */
} upnerf_baked_sh_render_args;
int upnerf_baked_sh_render(const upnerf_baked_sh_render_args* a, void* stream);

/* upnerf_sh_accumulate: one direction's share of a least-squares projection onto the basis.  With w[j] = W[j][k], column k of
 * the fp32 pseudo-inverse of the [K][nb] basis matrix of the K directions (formed by the caller in fp64),
 *   acc[p][c][j] = fmaf(w[j], rgb[p][c], first ? 0 : acc[p][c][j]),   j = 0 .. nb-1, c = 0 .. 2.
 * Called for k = 0 .. K-1 in order (first != 0 for k = 0), the sum has one fixed order.  One thread per point. */
typedef struct {
  int64_t n;
  int32_t nb;                /* 4 or 9 */
  int32_t first;             /* != 0: write, do not accumulate */
  float w[9];                /* w[0 .. nb-1], finite */
  int32_t reserved_;
  const float* rgb;          /* [n][3]: the colours for this direction */
  float* acc;                /* [n][3][nb] */
} upnerf_sh_accumulate_args;
int upnerf_sh_accumulate(const upnerf_sh_accumulate_args* a, void* stream);

/* upnerf_baked_sh_pack: the records of a baked scene from sigma and the accumulated coefficients.  A point is kept iff its sigma
 * is finite, > 0 and >= level (the rule of upnerf_baked_pack) and all its 3 nb coefficients are finite.  Kept: each coefficient
 * held to [-65504, 65504] (fminf(fmaxf(.))) and rounded to fp16, to nearest even; sigma copied; the other bytes zero.  Dropped:
 * a zero record.  kept[n] (optional) = 1 / 0 accordingly.  One thread per point. */
typedef struct {
  int64_t n;
  float level;               /* not NaN */
  int32_t degree;            /* 1 or 2 */
  const float* sigma;        /* [n] */
  const float* acc;          /* [n][3][nb] */
  uint8_t* records;          /* [n][32 | 64], aligned to the record size */
  uint8_t* kept;             /* [n] or NULL */
} upnerf_baked_sh_pack_args;
int upnerf_baked_sh_pack(const upnerf_baked_sh_pack_args* a, void* stream);

/* ---- a sparse baked scene: only the occupied 8 x 8 x 8-cell bricks of the grid are stored (csrc/brick.hip, the marcher in
 * csrc/baked.hip).  Added under ABI 11: new symbols only.  Every entry point: arguments refused on the host
 * before anything is launched, nothing allocated, no host read-back, no atomics, all launches on `stream`; the same bits every
 * run and however the work is cut into launches.
 *
 * Geometry and occupancy words are those of the occupancy grid above: cells C = N - 1 per axis, bricks B = ceil(C / 8), linear
 * brick index (bz * By + by) * Bx + bx.  The layout, stated once:
 *   slots  [Bz][By][Bx] int32: an occupied brick holds its rank among the occupied bricks in ascending linear brick index, an
 *          empty brick holds -1;
 *   bricks [n_bricks] int32: the inverse of slots, the linear brick index of each slot (ascending);
 *   pool   [n_bricks][9][9][9][E] bytes, E = 16 (degree 0: r, g, b, sigma fp32), 32 (degree 1) or 64 (degree 2): the records
 *          of the dense scene, unchanged, aligned to E.  (E = 4 is a plain fp32 grid, e.g. sigma alone: gather / scatter / occ.)
 * Pool point (slot, lz, ly, lx) is grid point (8 bx + lx, 8 by + ly, 8 bz + lz); a pool point beyond the grid (a ragged last
 * brick) is all zero bytes.  A brick stores its far faces as well -- UPNERF_BRICK_POINTS = 9 points per axis, not 8 -- so the
 * eight corners of any of its cells are inside it; points on faces that bricks share are stored once per brick with identical
 * bytes.  A kept point makes every cell that touches it occupied and every brick that contains such a cell occupied: no kept
 * point is lost, and an empty brick holds only zero records.
 *
 * upnerf_brick_table: slots, bricks and count[0] = n_bricks (device) from the brick bits of `words` (block scan, scan of the block
 *   sums, emit).  `bricks` has room for every brick, Bx By Bz entries; the entries from n_bricks on are not written.  `scratch`:
 *   upnerf_brick_table_scratch(Cx, Cy, Cz) bytes, 16-byte aligned.
 * upnerf_brick_gather: pool from a dense grid [Cz+1][Cy+1][Cx+1][E]; one thread per 4-byte (E = 4) or 16-byte word of the pool;
 *   out-of-grid points become zero.
 * upnerf_brick_scatter: the inverse, into a dense grid the caller has zeroed.  A grid point is written only by its owner brick,
 *   the brick of cell min(i, C - 1) per axis: no two threads store to one address.
 * upnerf_brick_occ: the upnerf_occ_words(Cx, Cy, Cz) words from the pool and its table; one thread per output word.  A cell bit
 *   is set iff its brick has a slot and any of the cell's eight pool corners has a finite sigma >= the smallest positive fp32
 *   (upnerf_occ_build at that level, no dilation); a brick bit is set iff any of its cells' bits is.  sigma is the fp32 at byte
 *   sigma_offset of a record.  n_bricks = 0 (pool and bricks may be NULL then) gives all-zero words. */
#define UPNERF_BRICK_POINTS 9
typedef struct {
  int32_t Cx, Cy, Cz, reserved_;
  const uint32_t* words;     /* [upnerf_occ_words(Cx, Cy, Cz)] */
  int32_t* slots;            /* [Bz][By][Bx] */
  int32_t* bricks;           /* [Bx By Bz] capacity; [count] written */
  int32_t* count;            /* [1] */
  void* scratch;             /* [upnerf_brick_table_scratch] bytes, 16-byte aligned */
} upnerf_brick_table_args;
long long upnerf_brick_table_scratch(int Cx, int Cy, int Cz);
int upnerf_brick_table(const upnerf_brick_table_args* a, void* stream);

typedef struct {
  int32_t Cx, Cy, Cz;
  int32_t n_bricks;          /* >= 1, <= Bx By Bz */
  int32_t E;                 /* bytes per point: 4, 16, 32 or 64 */
  int32_t reserved_;
  const int32_t* bricks;     /* [n_bricks] */
  const uint8_t* grid;       /* [Cz+1][Cy+1][Cx+1][E], aligned to min(E, 16) */
  uint8_t* pool;             /* [n_bricks][9][9][9][E], aligned to E */
} upnerf_brick_gather_args;
int upnerf_brick_gather(const upnerf_brick_gather_args* a, void* stream);

typedef struct {
  int32_t Cx, Cy, Cz;
  int32_t n_bricks;          /* >= 1, <= Bx By Bz */
  int32_t E;                 /* bytes per point: 4, 16, 32 or 64 */
  int32_t reserved_;
  const int32_t* bricks;     /* [n_bricks] */
  const uint8_t* pool;       /* [n_bricks][9][9][9][E], aligned to E */
  uint8_t* grid;             /* [Cz+1][Cy+1][Cx+1][E], aligned to min(E, 16), zeroed by the caller */
} upnerf_brick_scatter_args;
int upnerf_brick_scatter(const upnerf_brick_scatter_args* a, void* stream);

typedef struct {
  int32_t Cx, Cy, Cz;
  int32_t n_bricks;          /* >= 0, <= Bx By Bz */
  int32_t E;                 /* bytes per point: 4, 16, 32 or 64 */
  int32_t sigma_offset;      /* byte of the fp32 sigma in a record: a multiple of 4, <= E - 4 */
  const int32_t* slots;      /* [Bz][By][Bx] */
  const uint8_t* pool;       /* [n_bricks][9][9][9][E], aligned to E */
  uint32_t* words;           /* [upnerf_occ_words(Cx, Cy, Cz)] */
} upnerf_brick_occ_args;
int upnerf_brick_occ(const upnerf_brick_occ_args* a, void* stream);

/* upnerf_brick_columns: rays that make the field kernels evaluate pool points, the sibling of upnerf_grid_columns.  Line
 * l = (slot * 9 + ly) * 9 + lx of the pool; row r of the outputs is line line0 + r.  With (bx, by, bz) the brick of the slot:
 *   o[r] = (coord_x(min(8 bx + lx, Nx - 1)), coord_y(min(8 by + ly, Ny - 1)), 0), d[r] = (0, 0, 1),
 *   z[r][s] = coord_z(min(8 bz + min(s, 8), Nz - 1)) for s < S, S >= 32 (the field kernels' minimum),
 * coordinates by the rule of upnerf_grid_columns (fp64, every operation rounded on its own, rounded to fp32 once): for a pool
 * point inside the grid o + d z is the grid point the dense bake evaluates, in the same bits.  (A line beyond the grid in x or
 * y, or a sample beyond it in z, repeats the last grid point: its pool point is zero whatever the field says there.)  A row
 * depends on its line only: any split into calls gives the same bits. */
typedef struct {
  int32_t Nx, Ny, Nz, S;
  float lo[3], hi[3];
  int64_t line0;             /* >= 0 */
  int32_t count;             /* rows R of this call, >= 1; line0 + count <= 81 n_bricks */
  int32_t n_bricks;
  const int32_t* bricks;     /* [n_bricks] */
  float* o;                  /* [count][3] */
  float* d;                  /* [count][3] */
  float* z;                  /* [count][S] */
} upnerf_brick_columns_args;
int upnerf_brick_columns(const upnerf_brick_columns_args* a, void* stream);

/* upnerf_baked_sparse_render: upnerf_baked_render (degree 0) / upnerf_baked_sh_render (degree 1, 2) through a brick pool: the
 * same template with another layout -- lattice, skipping proposals, blend, clamp and compositing are one source.  Where the
 * dense march tests the brick bit of a sample's brick, this one reads slot = slots[brick]: slot < 0 is the empty brick; else the
 * eight corners of cell (ix, iy, iz) are pool points base, base + 1, + 9, + 81 with
 * base = slot * 729 + ((iz & 7) * 9 + (iy & 7)) * 9 + (ix & 7).  `words` are read for their cell bits only.  On a pool gathered
 * from a dense scene, with that scene's words, the result is bit for bit the dense marcher's. */
typedef struct {
  int32_t Cx, Cy, Cz, R;
  float lo[3], hi[3];        /* hi > lo, finite */
  float step;                /* > 0, finite */
  float background;          /* finite */
  float stop;                /* >= 0, < 1; 0 = never */
  int32_t degree;            /* 0, 1 or 2 */
  const uint8_t* pool;       /* [n_bricks][9][9][9][16 | 32 | 64], aligned to the record size */
  const int32_t* slots;      /* [Bz][By][Bx]; every entry < n_bricks */
  const uint32_t* words;     /* [upnerf_occ_words(Cx, Cy, Cz)] */
  const float* rays;         /* [R][8], 16-byte aligned */
  float* rgb;                /* [R][3] */
  float* depth;              /* [R] */
  float* opacity;            /* [R] */
} upnerf_baked_sparse_render_args;
int upnerf_baked_sparse_render(const upnerf_baked_sparse_render_args* a, void* stream);

/* ---- tuning a baked scene: the marcher's backward pass (csrc/baked.hip).  Added under ABI 11: new symbols only.
 * upnerf_baked_render_bwd: the gradient of a loss over the outputs of upnerf_baked_render (degree 0, `points` = rgbs) or
 * upnerf_baked_sh_render (degree 1, 2, `points` = records) with respect to the points of a DENSE scene, ADDED into outputs the
 * caller has zeroed.  Lattice, skipping, step, background, stop, words, rays, misses and the refusals are the forward's; one
 * thread per ray, one launch, nothing allocated, no host read-back.  The sums over rays are float atomic adds: their order is the
 * order of arrival, so this entry point -- alone among the baked ones -- does NOT give the same bits every run.
 *
 * The definition.  The visited samples of a ray are exactly those the forward composites, in its order; the sample after which
 * `stop` ends the ray is the last.  For visited sample k, with v the blended and (degree > 0) clamped channels and e, alpha,
 * w_k = T_k alpha_k, T_{k+1} = T_k (1 - alpha_k) formed as the forward forms them (all fp32):
 *   q_k = fmaf(g_rgb[0], v.r - background, fmaf(g_rgb[1], v.g - background, fmaf(g_rgb[2], v.b - background,
 *         fmaf(g_depth, t_k - far, g_opacity))))            (a NULL g_depth or g_opacity is zero);
 *   dL/dc_k[c] = w_k g_rgb[c] where the unclamped blend was in [0, 1] (always, at degree 0), else 0;
 *   dL/dsigma_k = delta fmaf(T_{k+1}, q_k, -(Q - P_k)),  P_k = fmaf(w_k, q_k, P_{k-1}),  Q = P of the last visited sample
 *   (a first march forms Q, a second the gradients: Q - P_k is the sum over the later samples, sum_{j > k} w_j q_j).
 * These are the derivatives of rgb = sum w (c - background) + background, depth = sum w (t - far) + far, opacity = sum w.
 * Corner j of the sample's cell (x = j & 1, y = j >> 1 & 1, z = j >> 2) receives its trilinear weight
 *   ((z ? fz : 1 - fz) * (y ? fy : 1 - fy)) * (x ? fx : 1 - fx)
 * times these four numbers; the shares of consecutive samples in one cell are summed first (fmaf, in sample order) and added to
 * memory once.  Degree 0: grad[p] += (r, g, b, sigma shares).  Degree 1, 2: grad_coef[p][c][j] += Y_j * (the colour share of c),
 * Y the basis of the ray's direction exactly as upnerf_baked_sh_render forms it, and grad_sigma[p] += the sigma share: the
 * gradient with respect to the fp32 value of each stored half, in the layout upnerf_baked_sh_pack reads its `acc` in.
 * A corner whose stored sigma is exactly zero is not a parameter and receives nothing (a cell with a clear bit keeps eight zero
 * corners).  Nothing is added for a miss, nor for a ray whose g_rgb, g_depth and g_opacity are all zero.
 * Refused: what the forward refuses (UPNERF_EINVAL), a NULL g_rgb or output, a degree outside {0, 1, 2}; `slots` not NULL, a
 * brick pool, is UPNERF_EUNSUP: faces that bricks share are stored once per brick, so a gradient would have to be summed over the
 * copies -- densify the scene, tune it, sparsify it again, or use upnerf_baked_sparse_render_bwd and upnerf_brick_face_sum
 * below, whose outputs are pool-shaped. */
typedef struct {
  int32_t Cx, Cy, Cz, R;
  float lo[3], hi[3];        /* hi > lo, finite */
  float step;                /* > 0, finite */
  float background;          /* finite */
  float stop;                /* >= 0, < 1; 0 = never */
  int32_t degree;            /* 0, 1 or 2 */
  const uint8_t* points;     /* rgbs [..][16] (degree 0) or records [..][32 | 64], aligned to the size of a point */
  const uint32_t* words;     /* [upnerf_occ_words(Cx, Cy, Cz)] */
  const float* rays;         /* [R][8], 16-byte aligned */
  const int32_t* slots;      /* NULL (a sparse scene's slots: UPNERF_EUNSUP) */
  const float* g_rgb;        /* [R][3] */
  const float* g_depth;      /* [R] or NULL */
  const float* g_opacity;    /* [R] or NULL */
  float* grad;               /* [n][4], n = (Cx+1)(Cy+1)(Cz+1): degree 0 */
  float* grad_coef;          /* [n][3][nb]: degree 1, 2 */
  float* grad_sigma;         /* [n]: degree 1, 2 */
} upnerf_baked_render_bwd_args;
int upnerf_baked_render_bwd(const upnerf_baked_render_bwd_args* a, void* stream);

/* upnerf_baked_project: after an optimiser step, the points back into the set the marcher is defined on.  One thread per point.
 * A sigma that is finite and > 0 stays; every other sigma (negative, zero, NaN, an infinity) becomes +0.  Degree 0, `rgbs` [n][4]
 * in place: where sigma stays, each colour c becomes c > 0 ? (c < 1 ? c : 1) : 0 (the degree-0 forward does not clamp; NaN -> 0);
 * where it does not, the point becomes (0, 0, 0, 0), as upnerf_baked_pack leaves a dropped point.  Degree 1, 2: `sigma` [n] in
 * place (upnerf_baked_sh_pack drops the point).  A sigma projected to zero is dead from then on: upnerf_baked_render_bwd gives a
 * corner whose sigma is zero no gradient. */
typedef struct {
  int64_t n;
  int32_t degree;            /* 0, 1 or 2 */
  int32_t reserved_;
  float* rgbs;               /* [n][4], 16-byte aligned: degree 0 */
  float* sigma;              /* [n]: degree 1, 2 */
} upnerf_baked_project_args;
int upnerf_baked_project(const upnerf_baked_project_args* a, void* stream);

/* ---- tuning a sparse baked scene in place: the backward pass on the brick pool (csrc/baked.hip, csrc/brick.hip).
 * Added under ABI 11: new symbols only.
 *
 * upnerf_baked_sparse_render_bwd: the gradient of a loss over the outputs of upnerf_baked_sparse_render with respect to the
 * points of its pool.  The definition is upnerf_baked_render_bwd's, word for word -- q, P, Q, the suffix, the live corners (a
 * stored sigma that is not zero), the open channels, the trilinear weights, the Y_j share at degree 1, 2, the sums over the
 * consecutive samples of one cell -- on the samples the sparse forward composites, through the same walk.  The outputs are
 * POOL-shaped, n = 729 n_bricks points: corner (x, y, z) of cell (ix, iy, iz) is pool point base + x + 9 y + 81 z with the
 * forward's base = slot * 729 + ((iz & 7) * 9 + (iy & 7)) * 9 + (ix & 7).  Contributions are ADDED with float atomics into
 * buffers the caller has zeroed: not the same bits every run.
 * A grid point on a face that bricks share is stored once per brick, and EACH COPY RECEIVES ONLY WHAT THE SAMPLES INSIDE ITS OWN
 * BRICK'S CELLS GIVE IT: the gradient of the point is the sum over its copies, which upnerf_brick_face_sum forms and writes to
 * every copy.  (A copy in a brick no ray enters stays exactly zero.)  Pool points beyond the grid receive nothing.
 * Refused (UPNERF_EINVAL): what upnerf_baked_sparse_render refuses (a NULL `slots` among it), a NULL g_rgb, a NULL output of the
 * degree (grad at degree 0; grad_coef or grad_sigma at degree 1, 2).  The fields keep the order of the other baked structs,
 * scalars first. */
typedef struct {
  int32_t Cx, Cy, Cz, R;
  float lo[3], hi[3];        /* hi > lo, finite */
  float step;                /* > 0, finite */
  float background;          /* finite */
  float stop;                /* >= 0, < 1; 0 = never */
  int32_t degree;            /* 0, 1 or 2 */
  const uint8_t* pool;       /* [n_bricks][9][9][9][16 | 32 | 64], aligned to the record size */
  const int32_t* slots;      /* [Bz][By][Bx]; every entry < n_bricks */
  const uint32_t* words;     /* [upnerf_occ_words(Cx, Cy, Cz)] */
  const float* rays;         /* [R][8], 16-byte aligned */
  const float* g_rgb;        /* [R][3] */
  const float* g_depth;      /* [R] or NULL */
  const float* g_opacity;    /* [R] or NULL */
  float* grad;               /* [n_bricks][9][9][9][4]: degree 0 */
  float* grad_coef;          /* [n_bricks][9][9][9][3][nb]: degree 1, 2 */
  float* grad_sigma;         /* [n_bricks][9][9][9]: degree 1, 2 */
} upnerf_baked_sparse_render_bwd_args;
int upnerf_baked_sparse_render_bwd(const upnerf_baked_sparse_render_bwd_args* a, void* stream);

/* upnerf_brick_face_sum: in place on a pool-shaped fp32 array `data` [n_bricks][729][F] (F floats per point: 4, 3 nb, 1, ...),
 * every copy of a grid point becomes the sum over its copies.  Grid point i of an axis (0 <= i <= C) lies in brick i / 8 at
 * l = i % 8 where that brick exists (i / 8 < B), and, if i % 8 == 0 and i > 0, in brick i / 8 - 1 at l = 8 as well: a point has
 * up to 2 x 2 x 2 = 8 copies.  With b_1 < ... < b_m the OCCUPIED bricks (slot >= 0) that hold a copy, in ascending linear
 * brick index, and x_b the copy of brick b, every copy becomes
 *   ((x_b1 + x_b2) + ...) + x_bm,   fp32, in that order,
 * per float.  Where m = 1 nothing is written; pool points beyond the grid are not touched.  Two launches: in the first the
 * thread of the copy in b_1 reads the others and stores the sum to its own copy, in the second the others read it -- no two
 * threads store to one address, no atomics, nothing allocated, the same bits every run.  One thread per (face point, float): the
 * 386 points of a brick with an l of 0 or 8; its 343 interior points are never read.  After it the copies of a point hold
 * identical bytes again, which is the layout's invariant: an optimiser that is given identical gradients, parameters and
 * moments on every copy keeps them identical.
 * Refused (UPNERF_EINVAL): NULL arguments, cells outside upnerf_occ_words' range, n_bricks < 1 or > Bx By Bz, F < 1, `data`
 * not 4-byte aligned; UPNERF_EUNSUP: more threads than a launch has. */
typedef struct {
  int32_t Cx, Cy, Cz;
  int32_t n_bricks;          /* >= 1, <= Bx By Bz */
  int32_t F;                 /* floats per point, >= 1 */
  int32_t reserved_;
  const int32_t* slots;      /* [Bz][By][Bx]; every entry < n_bricks */
  const int32_t* bricks;     /* [n_bricks] */
  float* data;               /* [n_bricks][9][9][9][F] */
} upnerf_brick_face_sum_args;
int upnerf_brick_face_sum(const upnerf_brick_face_sum_args* a, void* stream);

/* ---- posing a photograph against a baked scene: the marcher's ray gradients (csrc/baked.hip).  Added under
 * ABI 11: new symbols only.
 *
 * upnerf_baked_ray_bwd: the gradient of a loss over (rgb, depth, opacity) of the baked forward with respect to each ray's own
 * row o | d | near | far, WRITTEN (not added) to g_rays [R][8].  One entry point for both layouts: `slots` NULL is a dense grid
 * (`points` = rgbs at degree 0, records at degree 1, 2), else `points` is the pool of upnerf_baked_sparse_render.  One thread per
 * ray, one wave per workgroup, one launch, nothing allocated, no host read-back; a ray's sums stay in its thread's registers: no
 * LDS, no atomics, the same bits every run and however the rays are cut into launches.  upnerf_pose_rays_bwd maps the rows' o and
 * d parts on to se(3).
 *
 * The definition.  The visited samples of a ray, their cells i, positions f in the cell, corners c_0..7 (x = j & 1, y = j >> 1 & 1,
 * z = j >> 2; at degree > 0 each colour already reduced with the ray's Y, as the forward reads it), blended channels v, the clamp
 * with its `open` mask, w_k, T_{k+1} and the `stop` sample are the forward's, formed by the same code; q_k, P_k and Q are
 * upnerf_baked_render_bwd's.  The set of visited samples and the cell of each are HELD FIXED: this is the derivative of the
 * piecewise-smooth function the forward computes (K's dependence on near and far is a step function and contributes nothing).
 * All fp32; lerp(f, a, b) = fmaf(f, b - a, a).  Per visited sample k, in sample order:
 *   I_k = fmaf(T_{k+1}, q_k, -(Q - P_k));   a_k[c] = open_c ? w_k * g_rgb[c] : 0 (c = r, g, b);   a_k[sigma] = delta * I_k
 *   per channel ch = r, g, b, sigma, the slopes of the blend
 *     s_x = lerp(fz, lerp(fy, c1 - c0, c3 - c2), lerp(fy, c5 - c4, c7 - c6))
 *     s_y = lerp(fz, lerp(fx, c2 - c0, c3 - c1), lerp(fx, c6 - c4, c7 - c5))
 *     s_z = lerp(fy, lerp(fx, c4 - c0, c5 - c1), lerp(fx, c6 - c2, c7 - c3))
 *   S_k[a] = the fmaf chain over ch in that order, from zero: S = fmaf(a_k[ch], s_a[ch], S)
 *   So[a] += S_k[a];  St[a] = fmaf(t_k, S_k[a], St[a]);  E = fmaf(v_k.sigma, I_k, E);  O += w_k
 *   degree > 0: for corner j = 0..7, with wt_j = ((z ? fz : 1 - fz) * (y ? fy : 1 - fy)) * (x ? fx : 1 - fx), for c = r, g, b and
 *   basis function i ascending:  Z_i = fmaf(k_j[c][i], wt_j * a_k[c], Z_i),  k_j the corner's stored halves, converted exactly.
 * The gradient with respect to the sample's position is G_k[a] = inv[a] S_k[a], inv[a] = C[a] / (hi[a] - lo[a]) as the forward
 * holds it; the factor is applied once to the sums.  Per ray, with u = d / len as the forward forms it:
 *   d_o[a]  = inv[a] * So[a]
 *   d_d[a]  = fmaf(E * step, u[a], inv[a] * St[a])     (sum_k t_k G_k, and E, the gradient of delta = step len, through len)
 *             + fmaf(-u[a], u . gu, gu[a]) / len  at degree > 0:  gu[a] = sum_i Z_i dY_i/du[a] for the basis as stated at
 *             upnerf_baked_sh_render (a fmaf chain over i ascending, the constants folded into the factor of Z_i), u . gu =
 *             fmaf(u_z, gu_z, fmaf(u_y, gu_y, u_x * gu_x)): dY/dd = (dY/du)(I - u u^T) / len
 *   d_near  = fmaf(g_depth, O, fmaf(d_z, d_o[z], fmaf(d_y, d_o[y], d_x * d_o[x])))     (= sum_k (d . G_k + g_depth w_k))
 *   d_far   = g_depth * (1 - O)
 * A row of eight zeros is written for a miss (a number that is not finite, far <= near), for a ray with len == 0, and for a ray
 * whose g_rgb, g_depth and g_opacity are all zero.
 * Refused (UPNERF_EINVAL): what the forward of the same layout refuses, a NULL g_rgb or g_rays, g_rays not 16-byte aligned, a
 * degree outside {0, 1, 2}. */
typedef struct {
  int32_t Cx, Cy, Cz, R;
  float lo[3], hi[3];        /* hi > lo, finite */
  float step;                /* > 0, finite */
  float background;          /* finite */
  float stop;                /* >= 0, < 1; 0 = never */
  int32_t degree;            /* 0, 1 or 2 */
  const uint8_t* points;     /* rgbs, records, or a pool [n_bricks][9][9][9][16 | 32 | 64]; aligned to the size of a point */
  const int32_t* slots;      /* NULL: a dense grid; else [Bz][By][Bx], every entry < n_bricks */
  const uint32_t* words;     /* [upnerf_occ_words(Cx, Cy, Cz)] */
  const float* rays;         /* [R][8], 16-byte aligned */
  const float* g_rgb;        /* [R][3] */
  const float* g_depth;      /* [R] or NULL */
  const float* g_opacity;    /* [R] or NULL */
  float* g_rays;             /* [R][8], 16-byte aligned */
} upnerf_baked_ray_bwd_args;
int upnerf_baked_ray_bwd(const upnerf_baked_ray_bwd_args* a, void* stream);

/* ---- coarse-to-fine baked scenes: total variation and the doubling of the resolution (csrc/baked_reg.hip).  Added
 * under ABI 11: new symbols only.  Arguments refused on the host before anything is launched, nothing allocated, no host read-back,
 * no atomics, every output address has one writer: the same bits every run.
 *
 * upnerf_baked_tv: the total variation of a fp32 point array `data` [n][F] (F floats per point: rgbs with F = 4; coef with
 * F = 3 nb; sigma with F = 1) over the OCCUPIED cells, and its gradient.  Geometry and `words` are the occupancy grid's.  Cell
 * (i, j, k) has base point p = (i, j, k) and forward neighbours px = p + ex, py = p + ey, pz = p + ez (corners of the cell: they
 * exist).  All fp32.  For every cell c whose cell bit is set and every float f with w[f] != 0:
 *   dx = data[px][f] - data[p][f], dy and dz likewise;   tv_f(c) = sqrtf(fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, eps)))).
 * The value is sum_f w[f] sum_c tv_f(c).  It is written as one partial sum per workgroup to partial[0 .. upnerf_baked_tv_blocks)
 * (a thread adds its terms by fmaf(w[f], tv, .) in the order it meets them, the workgroup sums its 256 threads by a fixed tree);
 * the caller adds the partials.  `partial` NULL: no value.
 * The gradient, in gather form: point p receives up to four terms in this order -- the sum g IS the own term where that is
 * present and 0.0f where it is not, and each later term present is added to it (g += term):
 *   -((dx + dy) + dz) / tv_f(c)   of its own cell c = p, if that cell exists and is occupied,
 *   + dx' / tv_f(c')              of cell c' = p - ex, if it exists and is occupied (dx' = data[p][f] - data[p - ex][f]: p is its px),
 *   + dy' / tv_f(c')              of cell p - ey likewise,   + dz' / tv_f(c') of cell p - ez likewise,
 * and grad[p][f] = fmaf(w[f], that sum, grad[p][f]): ADDED, as every baked gradient is.  A point none of whose four cells is
 * occupied, and a float with w[f] == 0, are not touched.  A point whose sigma -- sigma[p * sigma_stride], an element stride so
 * that rgbs' fourth float serves -- is exactly zero is not a parameter and receives nothing (upnerf_baked_render_bwd's rule); its
 * own cell still counts in the value and in its neighbours' gradients: the field is zero there.
 * Dense (n_bricks = 0, slots = bricks = NULL): n = (Cx+1)(Cy+1)(Cz+1).  One workgroup per tile of 8 x 8 x 8 points, staged in LDS
 * with a one-point halo on either side, 8 floats of a point at a time.
 * Pool (n_bricks >= 1, slots and bricks given): n = 729 n_bricks, the layout of the sparse scene above.  One workgroup per brick;
 * only the 8 x 8 x 8 cells of the brick itself count for its points: EACH COPY of a point on a face that bricks share RECEIVES
 * ONLY WHAT THE CELLS INSIDE ITS OWN BRICK GIVE IT (the contract of upnerf_baked_sparse_render_bwd), and upnerf_brick_face_sum
 * forms the point's gradient on every copy.  Pool points beyond the grid receive nothing.  Every occupied cell lies in one brick:
 * the value is the dense one's up to the order of the sum.
 * Refused (UPNERF_EINVAL): NULL words, data, sigma or grad; cells outside upnerf_occ_words' range; n_bricks < 0 or > Bx By Bz;
 * slots or bricks given without the other or without n_bricks >= 1; F < 1 or > 28; sigma_stride < 1; eps <= 0 or not finite; a
 * weight among w[0 .. F-1] that is not finite.  UPNERF_EUNSUP: more workgroups than a launch has. */
typedef struct {
  int32_t Cx, Cy, Cz;
  int32_t n_bricks;          /* 0: a dense grid; else the bricks of the pool */
  int32_t F;                 /* floats per point, 1 .. 28 */
  int32_t sigma_stride;      /* floats from one point's sigma to the next's, >= 1 */
  float eps;                 /* > 0, finite */
  float w[28];               /* w[0 .. F-1], finite */
  int32_t reserved_;
  const uint32_t* words;     /* [upnerf_occ_words(Cx, Cy, Cz)] */
  const int32_t* slots;      /* NULL, or [Bz][By][Bx] */
  const int32_t* bricks;     /* NULL, or [n_bricks] */
  const float* data;         /* [n][F] */
  const float* sigma;        /* sigma of point p at sigma[p * sigma_stride] */
  float* grad;               /* [n][F], added into */
  float* partial;            /* [upnerf_baked_tv_blocks(Cx, Cy, Cz, n_bricks)] or NULL */
} upnerf_baked_tv_args;
long long upnerf_baked_tv_blocks(int Cx, int Cy, int Cz, int n_bricks);
int upnerf_baked_tv(const upnerf_baked_tv_args* a, void* stream);

/* upnerf_baked_upsample: the dense scene of twice the cells per axis, 2 C cells and 2 N - 1 points, from the points of a dense
 * scene (`points`: rgbs at degree 0, records at degree 1, 2).  One thread per child point.  Child point (i', j', k') is the
 * trilinear value of the parent grid at (i' / 2, j' / 2, k' / 2), formed per stored number -- r, g, b, sigma at degree 0; the
 * 3 nb halves, converted exactly to fp32, and the fp32 sigma at degree 1, 2 -- per axis in a fixed order: along x an even i'
 * copies parent i' / 2 and an odd one is 0.5f * (a + b) of parents (i' - 1) / 2 and (i' + 1) / 2, for each of the up to 2 x 2
 * (y, z) parents; then the same along y on those results, then along z.  The halving is exact (but for a subnormal), only the
 * additions round; a dropped parent is the zero record it is stored as.  The child is then packed at `level` by the rule of
 * upnerf_baked_pack (degree 0) or upnerf_baked_sh_pack (degree 1, 2: kept iff sigma is finite, > 0 and >= level and every
 * coefficient is finite; the coefficients held to +-65504 and rounded to nearest even to fp16).
 * Refused (UPNERF_EINVAL): NULL or misaligned points / out, a degree outside {0, 1, 2}, a NaN level, parent or child cells outside
 * upnerf_occ_words' range.  UPNERF_EUNSUP: more threads than a launch has. */
typedef struct {
  int32_t Cx, Cy, Cz;        /* the PARENT's cells */
  int32_t degree;            /* 0, 1 or 2 */
  float level;               /* not NaN */
  int32_t reserved_;
  const uint8_t* points;     /* [Cz+1][Cy+1][Cx+1][16 | 32 | 64], aligned to the size of a point */
  uint8_t* out;              /* [2Cz+1][2Cy+1][2Cx+1][16 | 32 | 64], aligned to the size of a point */
} upnerf_baked_upsample_args;
int upnerf_baked_upsample(const upnerf_baked_upsample_args* a, void* stream);

/* The same from pool to pool, nothing the size of either grid.  The child grid has B' = ceil(2 C / 8) bricks per axis (2 B or
 * 2 B - 1); child brick (bx', by', bz') holds child points 8 bx' .. 8 bx' + 8, whose parents are points 4 (bx' & 1) ..
 * 4 (bx' & 1) + 4 of parent brick (bx' >> 1, by' >> 1, bz' >> 1): a 5 x 5 x 5 block of ONE parent brick.  PRECONDITION: the
 * parent pool keeps the layout's invariant (a kept point makes every brick that contains a cell touching it occupied); then every
 * child brick with a kept point is the child of an occupied parent, and children of empty parents are empty.
 * upnerf_brick_upsample_mark: the brick bits of the CHILD grid into words[fine_words' ..] (words: the child's
 *   upnerf_occ_words(2 Cx, 2 Cy, 2 Cz) words; only the brick words are written, all of them).  A child brick's bit is set iff its
 *   parent has a slot and one of its child points inside the child grid is kept by upnerf_baked_upsample's rule at `level`: iff
 *   one of its cells touches a kept child point.  One workgroup per word.  upnerf_brick_table then makes the child's table.
 * upnerf_brick_upsample_fill: the child pool `out` [n_child][9][9][9][E] for the child bricks `child_bricks`: the records of
 *   upnerf_baked_upsample, far faces included; zero records beyond the child grid (and for a child of an empty parent).  One
 *   thread per child pool point.  upnerf_brick_occ then makes the child's cell bits.
 * Refused (UPNERF_EINVAL): what upnerf_baked_upsample refuses, n_bricks < 1 or > Bx By Bz, NULL slots or pool; mark: NULL words;
 * fill: n_child < 1 or > B'x B'y B'z, NULL or misaligned out, NULL child_bricks.  UPNERF_EUNSUP: more threads than a launch has. */
typedef struct {
  int32_t Cx, Cy, Cz;        /* the PARENT's cells */
  int32_t degree;            /* 0, 1 or 2 */
  float level;               /* not NaN */
  int32_t n_bricks;          /* the parent's, >= 1 */
  int32_t n_child;           /* fill: the child's bricks */
  int32_t reserved_;
  const int32_t* slots;      /* the parent's [Bz][By][Bx] */
  const uint8_t* pool;       /* the parent's [n_bricks][9][9][9][16 | 32 | 64] */
  const int32_t* child_bricks; /* fill: [n_child] */
  uint32_t* words;           /* mark: the child's [upnerf_occ_words(2 Cx, 2 Cy, 2 Cz)] */
  uint8_t* out;              /* fill: the child's pool */
} upnerf_brick_upsample_args;
int upnerf_brick_upsample_mark(const upnerf_brick_upsample_args* a, void* stream);
int upnerf_brick_upsample_fill(const upnerf_brick_upsample_args* a, void* stream);

/* ---- what lies outside the box of a baked scene: a cube-map environment behind the march (csrc/env.hip).  Added
 * under ABI 11: new symbols only.  Arguments refused on the host before anything is launched, nothing allocated, no host read-back,
 * one thread per item, no LDS, no atomics, every output address has one writer: the same bits every run and however the items are
 * cut into launches.
 *
 * The map.  env is fp32 [6][E+1][E+1][4], E >= 1 cells per face side (E <= UPNERF_ENV_MAX_E: 2 iu - E and g stay exact fp32
 * integers): node (face, iu, iv) is at env[((face (E+1) + iv) (E+1) + iu) 4 ..], its floats r, g, b and one padding float that is
 * stored as 0 and never read (a node is one 16-byte load).  The nodes sit on the CORNERS of the cells, the edges of the faces
 * included: a node on a face edge is stored once per face that contains it (2 copies; 3 at a cube corner), and with the copies
 * equal the bilinear lookup is continuous over the whole sphere with no seam handling in it.
 *
 * The lookup env(d) of a direction d = (d_0, d_1, d_2), all fp32 (env_lookup, a __host__ __device__ function of csrc/env.hip):
 *   m = the axis of the largest |d_a|, ties to the lowest axis;  face = 2 m + (d_m < 0);  (a, b) = the two other axes ascending;
 *   u = d_a / |d_m|, v = d_b / |d_m| (one division each, in [-1, 1]);  g_u = (u + 1) * (E / 2) (an addition and a product; E / 2 is
 *   exact), i_u = min((int)floorf(g_u), E - 1), f_u = g_u - i_u (exact, in [0, 1]);  v likewise.
 *   With n00 = node (face, i_u, i_v), n10 = (face, i_u + 1, i_v), n01 = (face, i_u, i_v + 1), n11 = (face, i_u + 1, i_v + 1) and
 *   lerp(f, p, q) = fmaf(f, q - p, p), per channel:  env(d) = lerp(f_v, lerp(f_u, n00, n10), lerp(f_u, n01, n11)).
 * d is never normalised: env(s d) = env(d) for s > 0 up to the rounding of the divisions.  A direction with a component that is
 * not finite, or with three zero components, is DEAD: colour (0, 0, 0), every gradient 0.
 * Node (face, iu, iv) has the direction d_m = +-1, d_a = (2 iu - E) / E, d_b = (2 iv - E) / E: one fp32 division of exact integers
 * each, so the copies of a shared node have bit-identical directions.
 *
 * upnerf_env_rays: the ray rows o | d | near | far [count][8] of nodes n0 .. n0 + count (n = (face (E+1) + iv) (E+1) + iu) that make
 * render_static bake the map -- the sibling of upnerf_grid_columns and upnerf_brick_columns.  In fp64, every operation rounded
 * on its own, rounded to fp32 once: o = (lo + hi) / 2, the box centre; d = the node direction x / sqrt(x_0^2 + x_1^2 + x_2^2) (the
 * sum in the order of the AXES, not of the face: a shared node's copies get the same bits).  In fp32, from the o and d just
 * written: near = fminf over the axes with d_a != 0 of ((d_a > 0 ? hi_a : lo_a) - o_a) / d_a, the t at which the ray leaves the
 * box (the slab test from the inside);  far as given.  A row depends on its node only.
 * Refused (UPNERF_EINVAL): NULL rays, rays not 16-byte aligned, E < 1 or > UPNERF_ENV_MAX_E, n0 < 0, count < 1,
 * n0 + count > 6 (E+1)^2, a box that is not finite or has hi <= lo on an axis, far not finite or <= 0. */
#define UPNERF_ENV_MAX_E 8192
typedef struct {
  int32_t E;
  int32_t count;             /* rows of this call, >= 1 */
  int64_t n0;                /* first node, >= 0; n0 + count <= 6 (E+1)^2 */
  float lo[3], hi[3];        /* hi > lo, finite */
  float far;                 /* > 0, finite */
  int32_t reserved_;
  float* rays;               /* [count][8], 16-byte aligned */
} upnerf_env_rays_args;
int upnerf_env_rays(const upnerf_env_rays_args* a, void* stream);

/* upnerf_env_seam: makes the copies of every shared node byte-identical, in place: every copy takes the 16 bytes of the copy on
 * the LOWEST face index (the owner).  The field kernels' last bit depends on which samples share a tile (upnerf_brick_columns),
 * so a bake gives the copies of a node colours one ulp apart; after this pass the lookup is continuous to the bit.  One thread
 * per edge node of every face (24 E per map).  A node's copies are the nodes of other faces with the SAME direction; the owner
 * of a set of copies is never written (it has no lower copy) and every other copy is written by its own thread alone: no two
 * threads store to one address, no thread reads what another writes.  Interior nodes are not touched.
 * Refused (UPNERF_EINVAL): NULL env, env not 16-byte aligned, E < 1 or > UPNERF_ENV_MAX_E. */
typedef struct {
  int32_t E;
  int32_t reserved_;
  float* env;                /* [6][E+1][E+1][4], 16-byte aligned */
} upnerf_env_seam_args;
int upnerf_env_seam(const upnerf_env_seam_args* a, void* stream);

/* upnerf_env_composite: the environment behind a march that was made with background 0.  For ray r with direction d_r =
 * rays[r][3..5], per channel:  rgb_out[r] = fmaf(1 - opacity[r], env(d_r), rgb_in[r]).  rgb_out may be rgb_in.  With a map that
 * holds the constant c this is the marcher's own fmaf(rest, background, rgb) at background = c, in the same bits (a dead
 * direction shows 0 where the marcher shows c).
 * upnerf_env_composite_bwd, from g_out [R][3] (the gradient of rgb_out; the gradient of rgb_in is g_out itself and is not written):
 *   g_opacity[r] = -fmaf(g_out[2], e[2], fmaf(g_out[1], e[1], g_out[0] * e[0])),  e = env(d_r)
 *   g_rays[r] = the gradient of the row o | d | near | far: zero but for d.  Face and cell are HELD FIXED (upnerf_baked_ray_bwd's
 *   convention).  With x0 = lerp(f_u, n00, n10), x1 = lerp(f_u, n01, n11) per channel, the slopes of the blend are
 *     s_u = lerp(f_v, n10 - n00, n11 - n01),  s_v = x1 - x0;   a[c] = (1 - opacity[r]) * g_out[c];
 *     G_u = the fmaf chain over c = r, g, b from zero, G = fmaf(a[c], s_u[c], G);  G_v likewise;
 *     p_u = G_u * (E / 2), p_v = G_v * (E / 2);   g_d[a] = p_u / |d_m|,  g_d[b] = p_v / |d_m|,  g_d[m] = -fmaf(u, p_u, v * p_v) / d_m.
 *   A dead direction writes g_opacity = 0 and eight zeros.  There is no gradient with respect to the map: it is baked from the
 *   field and stays frozen.
 * Refused (UPNERF_EINVAL): R < 0, E < 1 or > UPNERF_ENV_MAX_E, a NULL pointer, env, rays or g_rays not 16-byte aligned, any other
 * pointer not 4-byte aligned.  R == 0 launches nothing. */
typedef struct {
  int32_t E;
  int32_t R;                 /* >= 0 */
  const float* env;          /* [6][E+1][E+1][4], 16-byte aligned */
  const float* rays;         /* [R][8], 16-byte aligned */
  const float* opacity;      /* [R] */
  const float* rgb_in;       /* [R][3] */
  float* rgb_out;            /* [R][3]; may be rgb_in */
} upnerf_env_composite_args;
int upnerf_env_composite(const upnerf_env_composite_args* a, void* stream);

typedef struct {
  int32_t E;
  int32_t R;                 /* >= 0 */
  const float* env;          /* [6][E+1][E+1][4], 16-byte aligned */
  const float* rays;         /* [R][8], 16-byte aligned */
  const float* opacity;      /* [R] */
  const float* g_out;        /* [R][3] */
  float* g_opacity;          /* [R], written */
  float* g_rays;             /* [R][8], 16-byte aligned, written */
} upnerf_env_composite_bwd_args;
int upnerf_env_composite_bwd(const upnerf_env_composite_bwd_args* a, void* stream);

/* ---- pruning a baked scene by what a set of rays sees (csrc/baked.hip, csrc/brick.hip).  Added under ABI 11: new
 * symbols only.
 *
 * upnerf_baked_visibility: per point of a scene, the largest compositing weight that any ray of `rays` gives a sample in a cell
 * touching the point, MAXED into `vis`, which the caller has zeroed.  One entry point for both layouts (`slots` NULL: a dense
 * grid, else the pool of upnerf_baked_sparse_render) and every degree: a point is E bytes (16 | 32 | 64) with its fp32 sigma at
 * byte `sigma_offset` (12, 24, 56 in the three layouts of this header), and nothing else of it is read.  One thread per ray row
 * o | d | near | far, one wave per workgroup, one launch, nothing allocated, no host read-back.
 *
 * The definition.  The visited samples of a ray, their order, cells, f, blended sigma, delta, e, alpha, w_k = T_k alpha_k,
 * T_{k+1} and the `stop` sample are the forward's, formed by the same code (the sigma channel of its blend); there is no
 * background.  A visited sample with T_k > 0 records m_k = fmaxf(w_k, 2^-126), 2^-126 the smallest positive normal fp32; a
 * sample with T_k == 0 records nothing (and the ray ends there: no later sample can record).  Then
 *   vis[p] = max(vis[p], max over the rays and over their recorded samples in the (up to 8) cells that have p as a LIVE corner
 *            -- a stored sigma that is not zero, upnerf_baked_render_bwd's rule -- of m_k).
 * So vis[p] > 0 exactly when some ray reaches a cell of p with light left, and the value is the largest weight there.  The eight
 * corners of a cell receive ONE value, no trilinear share: a cell that holds a significant sample keeps its whole integrand.
 * The maxima of consecutive samples in one cell are taken in a register and go to memory once, with an atomic max on the bits
 * of the value as an unsigned integer (every recorded value is a positive, finite float, so its bits order as it does).  A
 * maximum is exact and commutative: THE SAME BITS EVERY RUN AND HOWEVER THE RAYS ARE CUT INTO LAUNCHES.
 * A pool: `vis` is pool-shaped, [n_bricks][729], corner (x, y, z) of a cell at base + x + 9 y + 81 z as in
 * upnerf_baked_sparse_render_bwd, and each copy of a shared point receives what its own brick's cells give it --
 * upnerf_brick_face_max makes the copies whole.  A miss records nothing.
 * Refused (UPNERF_EINVAL): what the forward of the layout refuses, a NULL vis, an E outside {16, 32, 64}, a sigma_offset that
 * is negative, no multiple of 4 or > E - 4.  The fields keep the order of the other baked structs, scalars first. */
typedef struct {
  int32_t Cx, Cy, Cz, R;
  float lo[3], hi[3];        /* hi > lo, finite */
  float step;                /* > 0, finite */
  float stop;                /* >= 0, < 1; 0 = never */
  int32_t E;                 /* bytes of a point: 16, 32 or 64 */
  int32_t sigma_offset;      /* the byte of the point's fp32 sigma: a multiple of 4, <= E - 4 */
  const uint8_t* points;     /* rgbs, records, or a pool [n_bricks][9][9][9][E]; aligned to E */
  const int32_t* slots;      /* NULL: a dense grid; else [Bz][By][Bx], every entry < n_bricks */
  const uint32_t* words;     /* [upnerf_occ_words(Cx, Cy, Cz)] */
  const float* rays;         /* [R][8], 16-byte aligned */
  float* vis;                /* [(Cz+1)(Cy+1)(Cx+1)] or [n_bricks][9][9][9]; zeroed by the caller, maxed into */
} upnerf_baked_visibility_args;
int upnerf_baked_visibility(const upnerf_baked_visibility_args* a, void* stream);

/* upnerf_brick_face_max: upnerf_brick_face_sum with fmaxf in place of +: every copy of a grid point becomes
 * fmaxf(fmaxf(x_b1, x_b2), ...) over its copies in the occupied bricks -- the same struct, the same two launches, one writer
 * per address, the same refusals, the same bits every run.  After it a pool-shaped visibility holds the point's value on every
 * copy. */
int upnerf_brick_face_max(const upnerf_brick_face_sum_args* a, void* stream);

/* upnerf_baked_prune: in place on `points` [n][E] (a grid or a pool, any degree), a point with NOT (vis[p] >= min_weight) becomes
 * an all-zero record, as upnerf_baked_pack leaves a dropped point; every other point keeps its bytes.  kept[p] (optional) =
 * 1 / 0 accordingly.  One thread per point.  Refused (UPNERF_EINVAL): n <= 0, an E outside {16, 32, 64}, a NULL vis or points,
 * points not 16-byte aligned, a min_weight that is NaN. */
typedef struct {
  int64_t n;
  float min_weight;          /* not NaN */
  int32_t E;                 /* bytes of a point: 16, 32 or 64 */
  const float* vis;          /* [n] */
  uint8_t* points;           /* [n][E], 16-byte aligned */
  uint8_t* kept;             /* [n] or NULL */
} upnerf_baked_prune_args;
int upnerf_baked_prune(const upnerf_baked_prune_args* a, void* stream);

#ifdef UPNERF_STAMPS
/* Diagnostic build only (make -C upnerf_amd/csrc stamps -> libupnerf_hip_stamps.so, never the shipped library): per-phase
 * shader-clock sums accumulated by the f16x3 field kernels; out16[0..7] forward trunk phases, [8..15] backward stages. */
int upnerf_stamps_read(unsigned long long* out16, int reset);
/* same for the register-resident forward kernel (field16r.hip): 8 phase sums of its slab loop */
int upnerf_stamps_read_r(unsigned long long* out8, int reset);
#endif

#ifdef __cplusplus
}
#endif
#endif /* UPNERF_HIP_H */
