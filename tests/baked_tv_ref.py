"""fp64 numpy restatement of the total variation of a baked scene's point array and of its gradient (include/upnerf_hip.h:
upnerf_baked_tv; upnerf_amd/baked_reg.py), with a per-element gate.  Shared by tests/test_baked_tv_cpu.py and
tests/test_hip_baked_tv.py, which also take their five grids from here (GRIDS).

    tv(data [Nz, Ny, Nx, F], sigma [Nz, Ny, Nx], cells bool [Cz, Cy, Cx], w [F], eps, roundings=4, grad0=None)
        -> {"value", "value_gate", "grad" [Nz, Ny, Nx, F], "gate" [Nz, Ny, Nx, F], "touched" bool [Nz, Ny, Nx, F]}
    tv_pool(pool_data [n, 9, 9, 9, F], pool_sigma [n, 9, 9, 9], bricks, cells, w, eps) -> the same per COPY: every brick on its own
        cells alone (what upnerf_baked_tv gives a pool before the face sum)

The definition.  Cell c = (i, j, k) has base point p and forward neighbours px, py, pz.  For every cell whose bit is set and every
float f with w[f] != 0: dx = data[px][f] - data[p][f], dy, dz likewise; tv_f(c) = sqrt(eps + dx^2 + dy^2 + dz^2).  The value is
sum_f w[f] sum_c tv_f(c).  Point p receives -(dx + dy + dz) / tv from its own cell and + dx' / tv' from cell p - ex (dy', dz' from
p - ey, p - ez), each where the cell exists and is occupied, times w[f]; a point whose sigma is exactly zero receives nothing.

The gate (u = 2^-24, the unit roundoff of fp32; the inputs are fp32 numbers, exact in fp64), first order, every constant a count of
roundings in the stated operation order:
  d        each difference of two fp32 values rounds once: u |d|.
  q        q = eps + dx^2 + dy^2 + dz^2: the differences' errors give 2 u d^2 each, no more than 2 u q together; the three squares
           and the sum are counted as four roundings, none on more than q (the kernel's three fmas are three of them): 6 u q.
  tv       half of that through the root, and the root's own rounding: 4 u tv.
  own      the numerator (dx + dy) + dz: the three differences u m together, m = |dx| + |dy| + |dz|, and two additions, neither on
           more than m: 3 u m.  The quotient t = n / tv: 3 u m / tv from the numerator, 4 u |t| from tv, the division u |t|:
           (3 m / tv + 5 |t|) u.
  other    t = d' / tv': the difference (1), tv' (4), the division (1): 6 u |t|.
  sum      the four terms are summed and multiplied by w[f] into the gradient with one fma.  Dense: three additions and the fma,
           none on more than |w| S + |grad0|, S = sum |t_i|: roundings = 4.  On a pool the terms are split over the m <= 4 copies
           whose bricks hold their cells: 4 - m additions inside the copies, m fmas, m - 1 merges in the face sum: 3 + m <= 7, the
           n - 1 of any bracketing and a product per copy.  `roundings` is that count; grad0 is what the buffer held before.
  element  gate = |w| (sum of the terms' errors) + roundings u (|w| S + |grad0|).
  value    each term w tv is off by 4 u |w| tv; n terms are added by n fmas and no more than n merges (the threads' chains, the
           workgroup's tree, the caller's sum of the partials), none on more than V = sum |w| tv: value_gate = 4 u V + 2 n u V."""
import numpy as np

import baked_ref as br
import baked_sparse_ref as sr

U = br.U


def tv(data, sigma, cells, w, eps, roundings=4, grad0=None):
    data = np.asarray(data, np.float32).astype(np.float64)
    if data.ndim == 3:
        data = data[..., None]
    w = np.asarray(w, np.float32).astype(np.float64)
    eps = float(np.float32(eps))
    live = (np.asarray(sigma) != 0)[..., None]
    on = np.asarray(cells, bool)[..., None] & (w != 0)
    a = data[:-1, :-1, :-1]
    dx, dy, dz = data[:-1, :-1, 1:] - a, data[:-1, 1:, :-1] - a, data[1:, :-1, :-1] - a
    t = np.sqrt(eps + dx * dx + dy * dy + dz * dz)
    m = np.abs(dx) + np.abs(dy) + np.abs(dz)
    V = float((np.abs(w) * t * on).sum())
    out = {"value": float((w * t * on).sum()), "value_gate": (4 + 2 * int(on.sum())) * U * V}
    grad, err, mag = (np.zeros_like(data) for _ in range(3))
    touched = np.zeros(data.shape, bool)
    own = np.where(on, -(dx + dy + dz) / t, 0.0)
    terms = [((slice(None, -1), slice(None, -1), slice(None, -1)), own, np.where(on, U * (3 * m / t + 5 * np.abs(own)), 0.0))]
    for at, d in (((slice(None, -1), slice(None, -1), slice(1, None)), dx), ((slice(None, -1), slice(1, None), slice(None, -1)), dy),
                  ((slice(1, None), slice(None, -1), slice(None, -1)), dz)):
        q = np.where(on, d / t, 0.0)
        terms.append((at, q, 6 * U * np.abs(q)))
    for at, q, dq in terms:
        grad[at] += q
        err[at] += dq
        mag[at] += np.abs(q)
        touched[at] |= on
    grad, err, mag, touched = (np.where(live, z, 0) for z in (grad, err, mag, touched))
    g0 = np.zeros_like(data) if grad0 is None else np.abs(np.asarray(grad0, np.float64)).reshape(data.shape)
    out["grad"] = w * grad
    out["gate"] = np.where(touched, np.abs(w) * err + roundings * U * (np.abs(w) * mag + g0), 0.0)
    out["touched"] = touched.astype(bool)
    return out


def brick_cells(cells, b):
    """bool [8, 8, 8]: the cells of brick b (linear index) of the grid's cell bits, False beyond the grid."""
    Cz, Cy, Cx = cells.shape
    Bx, By, Bz = sr.brick_dims((Cx, Cy, Cz))
    bx, by, bz = b % Bx, (b // Bx) % By, b // (Bx * By)
    pad = np.zeros((Bz * 8, By * 8, Bx * 8), bool)
    pad[:Cz, :Cy, :Cx] = cells
    return pad[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8]


def tv_pool(pool_data, pool_sigma, bricks, cells, w, eps, grad0=None):
    """tv on every brick of a pool with the brick's own cells alone: the per-copy gradient, its gate, and the value."""
    pool_data = np.asarray(pool_data)
    if pool_data.ndim == 4:
        pool_data = pool_data[..., None]
    res = [tv(pool_data[s], pool_sigma[s], brick_cells(cells, int(b)), w, eps, grad0=None if grad0 is None else grad0[s])
           for s, b in enumerate(bricks)]
    out = {k: np.stack([r[k] for r in res]) for k in ("grad", "gate", "touched")}
    out["value"], out["value_gate"] = sum(r["value"] for r in res), sum(r["value_gate"] for r in res)
    return out


# ---- the five grids of the total variation and upsampling tests --------------------------------------------------------------------

def single_cell(seed=2):
    """(rgbs [2, 2, 2, 4], level): one cell; seven kept corners and one dropped."""
    rng = np.random.RandomState(seed)
    sigma = rng.uniform(1.0, 6.0, (2, 2, 2))
    sigma[1, 0, 1] = 0.2
    return br.prune(sigma.astype(np.float32), rng.uniform(0, 1, (2, 2, 2, 3)).astype(np.float32), 0.5), 0.5


def far_face(seed=3):
    """(rgbs [5, 6, 12, 4], level): 11 x 5 x 4 cells, two bricks in x; the only kept points lie on the plane x = 8, the far face of
    brick 0 (and the near face of brick 1)."""
    rng = np.random.RandomState(seed)
    sigma = np.zeros((5, 6, 12))
    sigma[1:4, 1:5, 8] = rng.uniform(1.0, 6.0, (3, 4))
    return br.prune(sigma.astype(np.float32), rng.uniform(0, 1, (5, 6, 12, 3)).astype(np.float32), 0.5), 0.5


GRIDS = {"blob": br.blob_grid,                                   # 8 x 9 x 10 cells: 1 x 2 x 2 bricks
         "big": lambda: br.blob_grid(shape=(12, 17, 10)),       # 9 x 16 x 11 cells: 2 x 2 x 2 bricks, point (8, 8, 8) in all eight
         "cell": single_cell,                                    # one cell
         "exact": lambda: br.blob_grid(shape=(9, 6, 7), seed=5),  # 6 x 5 x 8 cells: C = 8 exactly in z
         "face": far_face}


def point_data(name, F, seed=7):
    """fp32 [Nz, Ny, Nx, F]: smooth-ish random numbers of very different sizes at every point of grid `name`, dead ones included."""
    rgbs = GRIDS[name]()[0]
    rng = np.random.RandomState(seed + F)
    d = rng.randn(*rgbs.shape[:3], F) * np.exp(rng.randn(F))
    d[..., ::3] *= 1e-3  # every third float varies by little: tv near sqrt(eps) at eps = 1
    return d.astype(np.float32)


def weights(F, seed=1):
    return np.random.RandomState(seed + F).uniform(0.2, 2.0, F).astype(np.float32)
