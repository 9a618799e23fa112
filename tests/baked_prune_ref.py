"""fp64 restatement of a baked scene's visibility (include/upnerf_hip.h: upnerf_baked_visibility), built on
tests/baked_ref.py's per-sample numbers (w, dw, dT, dg and their gates, taken sample by sample from its lattice, blended, alphas
and transmit), and of upnerf_baked_prune.  Shared by tests/test_baked_prune_cpu.py and tests/test_hip_baked_prune.py.

    visibility(sigma [Nz, Ny, Nx] fp32, bounds, rays, step, stop) -> (lo, hi), fp64 [Nz, Ny, Nx]

The kernel's value is a maximum over samples, and which samples take part is a matter of fp32 roundings (the cell of a sample
on a face, whether any light is left, where `stop` ends the ray), so the restatement gives an INTERVAL per point and nobody is
left out: the check is lo <= vis <= hi everywhere.  With TINY_NORMAL = 2^-126:

  A sample is CERTAIN when its cell is the same at g - dg and g + dg on every axis (so it is inside the box either way), the
  transmittance before it has T - dT > 0, and it does not lie after a `stop` decision that fell within dT of `stop`.  A certain
  sample gives max(w - dw, TINY_NORMAL) to lo and max(w + dw, TINY_NORMAL) to hi of the live corners (stored sigma != 0) of its cell.
  Any other sample that may be inside the box gives max(w + dw, TINY_NORMAL) to hi only, at the live corners of every cell it
  may lie in.

One rule beyond those, from the number format alone (it only narrows hi): fp32 forms alpha = 1 - e, and 1 - e IS 1 when
e <= 2^-25; then T (1 - alpha) is exactly zero and the kernel's ray records nothing more.  A sample that is surely inside the
box and whose e is below 2^-25 even at the low end of its exponent's gate (x - dx, times expf's 1 + 2u) ends the ray here too.
Without it a wall that fp32 cannot see through would leave everything behind it undecided (hi > 0 from a fp64 T of 1e-18).
The rule takes for granted that the kernel VISITS such a sample, that is, that its cell's occupancy bit is set.  That is the
invariant of a BakedScene -- its bits are built from its own stored sigmas, and a blended sigma above zero has a corner above
zero -- and so holds for every scene of these tests; it is not a fact about upnerf_baked_visibility called with words of the
caller's own that clear a cell with density in it (such a march skips the sample, and the rule would end the ray too early).

uncertain(lo, hi) is the share of points with lo == 0 < hi among those with hi > 0: a condition on the test's rays (at most one
in ten per scene), asserted on the restatement alone."""
import itertools

import numpy as np

import baked_ref as br

U = br.U
TINY_NORMAL = float(np.float32(2.0 ** -126))
OPAQUE = 2.0 ** -25  # 1 - e rounds to 1 in fp32 at and below this e


def _cell(x, C):
    return np.minimum(np.floor(np.clip(x, 0.0, C)), C - 1).astype(np.int64)


def visibility_ray(grid, live, lo_b, hi_b, C, row, step, stop, lo, hi):
    """One ray into lo and hi (in place).  grid: sigma fp64 [Nz, Ny, Nx, 1]; live: bool [Nz, Ny, Nx]."""
    lat = br.lattice(lo_b, hi_b, C, row, step)
    if lat is None:
        return
    _, g, dg, _ = lat
    maybe = ((g + dg >= 0) & (g - dg <= C)).all(1)
    if not maybe.any():
        return
    surely = ((g - dg >= 0) & (g + dg <= C)).all(1)[maybe]
    g, dg = g[maybe], dg[maybe]
    v, _, dv = br.blended(grid, g, dg, C)
    _, x, dx, alpha, dalpha = br.alphas(v[:, 0], dv[:, 0], row[3:6], step)
    c_lo, c_hi = _cell(g - dg, C), _cell(g + dg, C)
    after = False
    for n, T, dT, w, dw, Tn, dTn in br.transmit(alpha, dalpha, range(len(g))):
        certain = bool(surely[n] and (c_lo[n] == c_hi[n]).all() and T - dT > 0 and not after)
        top, low = max(w + dw, TINY_NORMAL), max(w - dw, TINY_NORMAL)
        for cx, cy, cz in itertools.product(*(range(c_lo[n, a], c_hi[n, a] + 1) for a in range(3))):
            sl = (slice(cz, cz + 2), slice(cy, cy + 2), slice(cx, cx + 2))
            m = live[sl]
            hi[sl] = np.where(m, np.maximum(hi[sl], top), hi[sl])
            if certain:
                lo[sl] = np.where(m, np.maximum(lo[sl], low), lo[sl])
        if surely[n] and np.exp(-(x[n] - dx[n])) * (1 + 2 * U) < OPAQUE:
            return  # fp32's alpha is 1: its T is exactly zero from here on
        if stop > 0:
            if Tn + dTn < stop:
                return
            if Tn - dTn < stop:
                after = True


def visibility(sigma, bounds, rays, step, stop=0.0):
    """(lo, hi) fp64 [Nz, Ny, Nx] of the fp32 sigmas `sigma` [Nz, Ny, Nx] and rays [R, 8] fp32."""
    s32 = np.asarray(sigma, np.float32)
    lo_b, hi_b, C, rays, step, _, stop = br.args64(bounds, rays, s32.shape, step, 0.0, stop)
    grid, live, lo, hi = s32.astype(np.float64)[..., None], s32 != 0, np.zeros(s32.shape), np.zeros(s32.shape)
    for row in rays:
        visibility_ray(grid, live, lo_b, hi_b, C, row, step, stop, lo, hi)
    return lo, hi


def within(vis, lo, hi):
    """bool, the shape of vis: lo <= vis <= hi (vis fp32, compared in fp64)."""
    v = np.asarray(vis, np.float32).astype(np.float64)
    return (lo <= v) & (v <= hi)


def uncertain(lo, hi):
    """The share of points with lo == 0 < hi among those with hi > 0 (0 with no such point)."""
    seen = hi > 0
    return float(((lo == 0) & seen).sum()) / max(1, int(seen.sum()))


def prune(points, vis, min_weight):
    """upnerf_baked_prune in numpy: (points [..., E] with the points of NOT (vis >= min_weight) zeroed, kept uint8 [...])."""
    with np.errstate(invalid="ignore"):
        keep = np.asarray(vis, np.float32) >= np.float32(min_weight)
    return np.where(keep[..., None], points, np.zeros((), points.dtype)), keep.astype(np.uint8)


def face_max(pool_vis, bricks, resolution):
    """[n, 9, 9, 9] with every copy of a grid point set to the maximum over its copies (numpy: scatter with max, gather)."""
    import baked_sparse_ref as sr
    Nx, Ny, Nz = resolution
    Bx, By, Bz = sr.brick_dims((Nx - 1, Ny - 1, Nz - 1))
    pad = np.full((Bz * 8 + 1, By * 8 + 1, Bx * 8 + 1), -np.inf, pool_vis.dtype)
    where = []
    for s, b in enumerate(np.asarray(bricks, np.int64)):
        bx, by, bz = b % Bx, (b // Bx) % By, b // (Bx * By)
        sl = (slice(8 * bz, 8 * bz + 9), slice(8 * by, 8 * by + 9), slice(8 * bx, 8 * bx + 9))
        pad[sl] = np.maximum(pad[sl], pool_vis[s])
        where.append(sl)
    out = np.stack([pad[sl] for sl in where]) if where else pool_vis.copy()
    inside = np.zeros(pad.shape, bool)
    inside[:Nz, :Ny, :Nx] = True
    keep = np.stack([inside[sl] for sl in where]) if where else np.zeros(pool_vis.shape, bool)
    return np.where(keep, out, pool_vis)  # (pool points beyond the grid are not touched)


# ---- the test scenes beyond baked_ref's ----------------------------------------------------------------------------------------

def ragged_grid(seed=41):
    """(rgbs, level) of [Nz, Ny, Nx] = 11 x 10 x 18 points: 17 cells on x, so three bricks there and two shared faces.  Smooth
    density over the whole x range, zero on the outermost layer."""
    rng = np.random.RandomState(seed)
    shape = (11, 10, 18)
    z, y, x = np.meshgrid(np.linspace(-1, 1, shape[0]), np.linspace(-1, 1, shape[1]), np.linspace(-1, 1, shape[2]), indexing="ij")
    sigma = np.zeros(shape)
    for cx in (-0.6, 0.0, 0.6):
        sigma += rng.uniform(4, 12) * np.exp(-((x - cx) ** 2 / (2 * 0.3 ** 2) + (y * y + z * z) / (2 * 0.5 ** 2)))
    sigma[[0, -1]] = sigma[:, [0, -1]] = sigma[:, :, [0, -1]] = 0
    rgb = rng.uniform(0, 1, shape + (3,))
    return br.prune(sigma.astype(np.float32), rgb.astype(np.float32), 0.4), 0.4


WALL_X = (6, 7, 8)  # the wall's three layers of points
BLOB_X = (12, 15)   # the hidden blob: points 12 .. 14 on x, three empty cells (9, 10, 11) behind the wall's last layer


def wall_grid(seed=42):
    """(rgbs, level) of [Nz, Ny, Nx] = 12 x 12 x 20 points: a slab three points thick with sigma 1000 across the whole interior
    of the box's y-z section, and a blob behind it.  Zero on the outermost layer."""
    rng = np.random.RandomState(seed)
    shape = (12, 12, 20)
    sigma = np.zeros(shape)
    sigma[1:-1, 1:-1, WALL_X[0]:WALL_X[-1] + 1] = 1000.0
    sigma[3:9, 3:9, BLOB_X[0]:BLOB_X[1]] = rng.uniform(2.0, 9.0, (6, 6, 3))
    rgb = rng.uniform(0, 1, shape + (3,))
    return br.prune(sigma.astype(np.float32), rgb.astype(np.float32), 1.0), 1.0


def wall_rays(bounds=br.BOUNDS, n=8):
    """(rays [n * n, 8], step): rays along +x from in front of the box over the interior of its y-z section, `step` half a cell
    of x, the samples a quarter and three quarters of the way through each cell: in the wall's first cell (sigma 250 and 750 there)
    the second sample's alpha rounds to 1 in fp32 and T becomes exactly 0."""
    lo, hi = br.bounds64(bounds)
    cell = (hi - lo) / np.array([19.0, 11.0, 11.0])
    step = float(np.float32(cell[0] / 2))
    ys = lo[1] + cell[1] * np.linspace(1.3, 9.7, n)
    zs = lo[2] + cell[2] * np.linspace(1.4, 9.6, n)
    rows = [[lo[0] - 2 * cell[0], y, z, 1.0, 0.0, 0.0, 0.0, float(hi[0] - lo[0]) + 3 * cell[0]] for z in zs for y in ys]
    return np.asarray(rows, np.float32), step
