"""numpy restatement of the sum over the copies of a brick pool's shared points (include/upnerf_hip.h: upnerf_brick_face_sum;
upnerf_amd/baked_sparse_tune.py), built on tests/baked_sparse_ref.py, whose layout it uses and does not repeat.
Shared by tests/test_baked_sparse_tune_cpu.py and tests/test_hip_baked_sparse_tune.py.

    holders(i, C) -> [(brick, l)] of grid point i of an axis with C cells, ascending: brick i // 8 at l = i % 8 where that brick
        exists, and before it brick i // 8 - 1 at l = 8 if i % 8 == 0 and i > 0
    copies(x, y, z, slots, cells) -> [(slot, lz, ly, lx)] over the OCCUPIED bricks that hold the point, in ascending linear brick
        index (z slowest, then y, then x: the order of (bz By + by) Bx + bx)
    face_sum(pool fp32 [n, 9, 9, 9, F], slots, cells) -> a new pool: every copy of a point with m >= 2 copies becomes
        ((x_b1 + x_b2) + ...) + x_bm in fp32, in that order; every other pool point (m = 1, beyond the grid) keeps its bits
    copy_groups(slots, cells) -> the lists `copies` returns that have two entries at least (the shared points)
    scatter_add(pool, slots, cells) -> fp64 grid [Nz, Ny, Nx, F]: the sum over all copies of every grid point
    holes_bits(cells) -> a cell pattern with whole bricks missing between occupied neighbours; geometric_copies(x, y, z, cells)

The gradient the backward kernel gives the copies is compared with tests/baked_tune_ref.py's dense gradient gathered to the pool
(baked_sparse_ref.gather); the gate is gathered with it and NOT widened.  Why: a sum of n fp32 contributions costs n - 1 roundings
however it is bracketed.  Each of a point's m copies starts from an exact zero and sums its own n_i contributions (n_i - 1
roundings each, sum n - m); the face sum merges the m copies with m - 1 more: n - 1 again, every one of them on a partial sum
bounded by the sum of the contributions' magnitudes.  baked_tune_ref's element term already allows n roundings in any order."""
import numpy as np

import baked_sparse_ref as sr

P = sr.P


def holders(i, C):
    B = (C + sr.BRICK - 1) // sr.BRICK
    out = []
    if i % sr.BRICK == 0 and i > 0:
        out.append((i // sr.BRICK - 1, sr.BRICK))
    if i // sr.BRICK < B:
        out.append((i // sr.BRICK, i % sr.BRICK))
    return out


def copies(x, y, z, slots, cells):
    Cx, Cy, Cz = cells
    out = []
    for bz, lz in holders(z, Cz):
        for by, ly in holders(y, Cy):
            for bx, lx in holders(x, Cx):
                s = int(slots[bz, by, bx])
                if s >= 0:
                    out.append((s, lz, ly, lx))
    return out


def copy_groups(slots, cells):
    Cx, Cy, Cz = cells
    plane = lambda C: [i for i in range(C + 1) if i % sr.BRICK == 0 and 0 < i]  # (only these coordinates have two holders)
    seen, groups = set(), []
    for axis, C in enumerate((Cx, Cy, Cz)):
        for i in plane(C):
            ranges = [range(Cx + 1), range(Cy + 1), range(Cz + 1)]
            ranges[axis] = [i]
            for z in ranges[2]:
                for y in ranges[1]:
                    for x in ranges[0]:
                        if (x, y, z) in seen:
                            continue
                        seen.add((x, y, z))
                        c = copies(x, y, z, slots, cells)
                        if len(c) >= 2:
                            groups.append(((x, y, z), c))
    return groups


def face_sum(pool, slots, cells):
    assert pool.dtype == np.float32 and pool.ndim == 5 and pool.shape[1:4] == (P, P, P)
    out = pool.copy()
    for _, c in copy_groups(slots, cells):
        total = pool[c[0]].copy()
        for at in c[1:]:
            total = (total + pool[at]).astype(np.float32)  # fp32, in ascending brick order
        for at in c:
            out[at] = total
    return out


def scatter_add(pool, slots, cells):
    Cx, Cy, Cz = cells
    grid = np.zeros((Cz + 1, Cy + 1, Cx + 1, pool.shape[4]), np.float64)
    for z in range(Cz + 1):
        for y in range(Cy + 1):
            for x in range(Cx + 1):
                for at in copies(x, y, z, slots, cells):
                    grid[z, y, x] += pool[at]
    return grid


def holes_bits(cells):
    """bool cells [Cz, Cy, Cx], all set but for every third brick (linear index k % 3 == 1), which is left whole and empty: shared
    points then have fewer copies than the geometry allows, and the first occupied holder is not always the first geometric one."""
    Cx, Cy, Cz = cells
    bits = np.ones((Cz, Cy, Cx), bool)
    Bx, By, Bz = sr.brick_dims(cells)
    for k, (bz, by, bx) in enumerate(np.ndindex(Bz, By, Bx)):
        if k % 3 == 1:
            bits[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = False
    return bits


def geometric_copies(x, y, z, cells):
    """The number of bricks that hold grid point (x, y, z), occupied or not."""
    return len(holders(x, cells[0])) * len(holders(y, cells[1])) * len(holders(z, cells[2]))


def in_grid(bricks, cells):
    """bool [n, 9, 9, 9]: the pool points that stand for a grid point."""
    return sr.gather(np.ones((cells[2] + 1, cells[1] + 1, cells[0] + 1, 1), np.uint8), bricks)[..., 0] != 0
