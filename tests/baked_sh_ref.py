"""fp64 numpy restatement of a baked scene with spherical-harmonic colour (include/upnerf_hip.h: upnerf_baked_sh_render,
upnerf_sh_accumulate, upnerf_baked_sh_pack; upnerf_amd/baked.py).  Grids, rays and the whole march are those of
tests/baked_ref.py (render_ray with dcol and the clamp), whose definition and derivation this docstring extends and does not
repeat; ray_grid is what a direction adds.
Shared by tests/test_baked_sh_cpu.py and tests/test_hip_baked_sh.py.

    basis(dirs, degree) -> [K, nb]                project(rgb_dirs, dirs, degree) -> (coefficients, condition sums)
    pack(coef, sigma, level, degree) -> (records uint8, kept)              unpack(records, degree) -> (k fp64, sigma fp64)
    render(records, degree, bounds, rays, step, background, stop) -> the dict of baked_ref.render, plus "clamp" [R, 3]

The definition.  The stored record is the input: its halves and its fp32 sigma, converted exactly.  Per ray u = d / |d| and
Y_j(u) in fp64; the four channels of a corner are (sum_j Y_j k[c][j], sigma); they are blended as baked_ref blends rgbs; the three
blended colours are clamped to [0, 1]; everything else is baked_ref's.

The gates: baked_ref's, with the new roundings only (u = 2^-24; no constant that is not a count).
  u_a    |d| is sqrtf of fma, fma, product: 3 roundings (taken whole, not halved through the root) and the root's own, then the
         division: 5 u relative in every component of the unit vector.
  Y_j    Y0 is a rounded constant: 1 u |Y0|.  Y1..3 = c u_a: the component (5), the constant (1), the product (1): 7 u |Y_j|.
         Y4, Y5, Y7 = c (a b): two components (10), their product (1), the constant (1), the product (1): 13 u |Y_j|.
         Y8 = c fma(x, x, -(y y)): each square carries 10 u of itself, y y rounds (1) and the fma (1), each of the last two on no
         more than xx + yy; the constant and the product (2): 14 u c (xx + yy).
         Y6 = c fma(2 z, z, -fma(x, x, y y)): the squares 10 u of themselves, y y (1), the inner fma (1), the outer fma (1), none
         on more than 2 zz + xx + yy; the constant and the product (2): 15 u c (2 zz + xx + yy).
         Written dY_j = n_j u m_j with the counts N_BASIS and m_j = |Y_j|, or the sum of the terms' magnitudes for Y6 and Y8.
  corner col[c] is nb fmas, each rounding once on a partial sum <= sum_j |Y_j k_cj|, of a basis that is off by dY:
         dcol_c = u sum_j (nb + n_j) m_j |k_cj|.  The conversion of a half is exact; sigma is read as it is stored.
  v      baked_ref's dv (the moves of g, evaluated on the unclamped blend, and 9 u max |corner| over the corners' four channels)
         plus, for the colours, the largest dcol_c among the eight corners (a blend is a convex combination).
  clamp  is 1-Lipschitz: it adds nothing.
Alpha, T, w and the sums follow baked_ref's recurrence unchanged, with the clamped colours as c.

project's condition sums: acc_j = sum_k W_jk rgb_k is K fmas in fp32 with weights rounded once from fp64:
(K + 1) u sum_k |W_jk| |rgb_k| per coefficient."""
import numpy as np

import baked_ref as br

U = br.U
Y0, Y1, Y2, Y3, Y4 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
NB = {1: 4, 2: 9}
RECORD = {1: 32, 2: 64}
SIGMA_BYTE = {1: 24, 2: 56}
N_BASIS = np.array([1, 7, 7, 7, 13, 13, 15, 13, 14], np.float64)  # roundings behind each basis value (docstring)
HALF_MAX = 65504.0


def basis(dirs, degree):
    """[K, nb] fp64 of directions [K, 3] (normalised here)."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    x, y, z = (d / np.linalg.norm(d, axis=1, keepdims=True)).T
    B = [np.full_like(x, Y0), -Y1 * y, Y1 * z, -Y1 * x, Y2 * x * y, -Y2 * y * z, Y3 * (2 * z * z - x * x - y * y), -Y2 * x * z,
         Y4 * (x * x - y * y)]
    return np.stack(B[:NB[degree]], 1)


def basis_magnitude(u, degree):
    """[nb] m_j of a unit vector u: |Y_j|, and for Y6, Y8 the sum of the magnitudes of their terms."""
    x, y, z = np.asarray(u, np.float64)
    m = np.abs(basis(u, 2)[0])
    m[6], m[8] = Y3 * (2 * z * z + x * x + y * y), Y4 * (x * x + y * y)
    return m[:NB[degree]]


def sphere_directions(K=48):
    """The Fibonacci lattice of upnerf_amd.baked.sphere_directions, restated."""
    i = np.arange(K, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / K
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def project(rgb_dirs, dirs, degree):
    """(coef [..., 3, nb], cond [..., 3, nb]) fp64 of colours rgb_dirs [K, ..., 3] at directions dirs [K, 3]: the least-squares
    coefficients pinv(B) rgb and the condition sums sum_k |W_jk| |rgb_k| its fp32 evaluation is judged by."""
    W = np.linalg.pinv(basis(dirs, degree))  # [nb, K]
    rgb = np.asarray(rgb_dirs).astype(np.float64)
    return np.einsum("jk,k...c->...cj", W, rgb), np.einsum("jk,k...c->...cj", np.abs(W), np.abs(rgb))


def pack(coef, sigma, level, degree):
    """(records uint8 [..., 32 | 64], kept bool [...]) of fp32 coefficients [..., 3, nb] and sigma [...]: baked_ref.prune's rule,
    and in addition a point with a coefficient that is not finite is dropped.  numpy's float16 cast is the rounding (to nearest
    even), after the coefficients are held to +-65504."""
    nb = NB[degree]
    coef = np.asarray(coef, np.float32).reshape(np.shape(sigma) + (3 * nb,))
    sigma = np.asarray(sigma, np.float32)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(sigma) & (sigma > 0) & (sigma >= np.float32(level)) & np.isfinite(coef).all(-1)
    rec = np.zeros(sigma.shape + (RECORD[degree],), np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        halves = np.clip(np.where(keep[..., None], coef, 0), -HALF_MAX, HALF_MAX).astype(np.float16)
    rec[..., :6 * nb] = np.ascontiguousarray(halves).view(np.uint8).reshape(sigma.shape + (6 * nb,))
    s = np.ascontiguousarray(np.where(keep, sigma, 0).astype(np.float32))
    rec[..., SIGMA_BYTE[degree]:SIGMA_BYTE[degree] + 4] = s.view(np.uint8).reshape(sigma.shape + (4,))
    return rec, keep


def unpack(records, degree):
    """(k fp64 [..., 3, nb], sigma fp64 [...]) of records: the stored numbers, converted exactly."""
    nb = NB[degree]
    rec = np.ascontiguousarray(records)
    k = np.ascontiguousarray(rec[..., :6 * nb]).view(np.float16).astype(np.float64).reshape(rec.shape[:-1] + (3, nb))
    s = np.ascontiguousarray(rec[..., SIGMA_BYTE[degree]:SIGMA_BYTE[degree] + 4]).view(np.float32).astype(np.float64)
    return k, s.reshape(rec.shape[:-1])


def ray_grid(k, sigma, d, degree, gates=True, view_sign=1.0):
    """(grid [Nz, Ny, Nx, 4], dcol [Nz, Ny, Nx, 4] or None, Y [nb], m [nb]) of a ray with direction d: the corners' four channels
    (sum_j Y_j k[c][j], sigma) and the colours' own errors (docstring: corner).  view_sign = -1: the colours of the opposite
    direction."""
    nb = NB[degree]
    unit = view_sign * d / np.sqrt((d * d).sum())
    Y, m = basis(unit, degree)[0], basis_magnitude(unit, degree)
    dcol = np.concatenate([U * (np.abs(k) * ((nb + N_BASIS[:nb]) * m)).sum(-1), np.zeros(sigma.shape + (1,))], -1) if gates else None
    return np.concatenate([k @ Y, sigma[..., None]], -1), dcol, Y, m


def render(records, degree, bounds, rays, step, background=0.0, stop=0.0, view_sign=1.0):
    """The restatement over rays [R, 8] fp32 and records uint8 [Nz, Ny, Nx, 32 | 64]: baked_ref.render_ray on the ray's own grid,
    clamped, and "clamp": the counts (below 0, above 1, neither) of the blended colour values of its contributing samples."""
    k, sigma = unpack(records, degree)
    lo, hi, C, rays, step, background, stop = br.args64(bounds, rays, sigma.shape, step, background, stop)

    def one(row):
        grid, dcol = ray_grid(k, sigma, row[3:6], degree, True, view_sign)[:2]
        return br.render_ray(grid, lo, hi, C, row, step, background, stop, dcol, clamp=True)
    return br.render_rows(rays, one, clamp=True)


# ---- the test scenes ----------------------------------------------------------------------------------------------------------------

GRIDS = {"blob": br.blob_grid, "corners": br.corner_grid}
# mean and standard deviation of a kept corner's colour over direction and point: the blends of eight corners leave [0, 1] on
# either side often enough (the mean above 0.5 because a blend with dropped corners is pulled towards 0; test_baked_sh_cpu.py counts)
MEAN, SPREAD = 0.65, 0.9


def coefficients(shape, degree, seed, mean=MEAN, spread=SPREAD):
    """fp32 [shape, 3, nb]: the constant term about mean / Y0, every term normal with the deviation that gives the colour the
    deviation `spread` (the basis is orthonormal: the mean of sum_j Y_j^2 over the sphere is nb / 4 pi)."""
    nb = NB[degree]
    amp = spread / np.sqrt(nb / (4 * np.pi))
    k = np.random.RandomState(seed).randn(*shape, 3, nb) * amp
    k[..., 0] += mean / Y0
    return k.astype(np.float32)


def sh_grid(name, degree, seed=11):
    """(records, level) of a test grid of baked_ref with random coefficients at its kept points."""
    rgbs, level = GRIDS[name]()
    sigma = rgbs[..., 3]
    return pack(coefficients(sigma.shape, degree, seed + degree), sigma, level, degree)[0], level


def steps(records):
    """About a cell, and a tenth of a cell, in units of t."""
    cell = br.cell_size(records)
    return {"cell": float(np.float32(cell)), "tenth": float(np.float32(cell / 10))}
