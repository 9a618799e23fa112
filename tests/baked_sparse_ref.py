"""numpy restatement of a sparse baked scene's layout (include/upnerf_hip.h: upnerf_brick_table, upnerf_brick_gather,
upnerf_brick_scatter, upnerf_brick_occ; upnerf_amd/baked.py).  All of it is integer and byte work: the results
are exact, and the tests compare with them byte for byte.  Shared by tests/test_baked_sparse_cpu.py and
tests/test_hip_baked_sparse.py.

    cells C = N - 1 per axis, bricks B = ceil(C / 8), linear brick index (bz By + by) Bx + bx
    table(brick_bits [Bz, By, Bx]) -> (slots int32 [Bz, By, Bx], bricks int32 [n])
    gather(grid [Nz, Ny, Nx, E], bricks) -> pool [n, 9, 9, 9, E]          scatter(pool, bricks, (Nx, Ny, Nz)) -> grid
    cell_bits(pool_sigma [n, 9, 9, 9], slots, (Cx, Cy, Cz)) -> bool [Cz, Cy, Cx]
    words(cell_bits) -> uint32 [upnerf_occ_words]: the cell bits, 32 per word, then one bit per brick (the OR of its cells)"""
import numpy as np

BRICK, P = 8, 9
TINY = np.float32(2.0 ** -149)


def brick_dims(cells):
    """(Bx, By, Bz) of (Cx, Cy, Cz) cells."""
    return tuple((int(c) + BRICK - 1) // BRICK for c in cells)


def brick_bits(cell_bits):
    """bool [Bz, By, Bx]: a brick is occupied iff one of its cells is."""
    Cz, Cy, Cx = cell_bits.shape
    Bx, By, Bz = brick_dims((Cx, Cy, Cz))
    pad = np.zeros((Bz * BRICK, By * BRICK, Bx * BRICK), bool)
    pad[:Cz, :Cy, :Cx] = cell_bits
    return pad.reshape(Bz, BRICK, By, BRICK, Bx, BRICK).any(axis=(1, 3, 5))


def words(cell_bits):
    """uint32 words of bool cells [Cz, Cy, Cx]: cell (x, y, z) is bit (z Cy + y) Cx + x, 32 per word; then the brick bits."""
    def pack(bits):
        b = np.zeros((bits.size + 31) // 32 * 32, np.uint64)
        b[:bits.size] = bits.reshape(-1)
        return (b.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
    return np.concatenate([pack(cell_bits), pack(brick_bits(cell_bits))])


def table(bits):
    """(slots, bricks) of bool brick bits [Bz, By, Bx]: the rank of each occupied brick in ascending linear index, -1 elsewhere."""
    flat = bits.reshape(-1)
    bricks = np.nonzero(flat)[0].astype(np.int32)
    slots = np.full(flat.size, -1, np.int32)
    slots[bricks] = np.arange(bricks.size, dtype=np.int32)
    return slots.reshape(bits.shape), bricks


def gather(grid, bricks):
    """pool [n, 9, 9, 9, E] of grid [Nz, Ny, Nx, E]: pool point (slot, lz, ly, lx) is grid point (8 bx + lx, 8 by + ly, 8 bz + lz),
    zero beyond the grid."""
    Nz, Ny, Nx, E = grid.shape
    Bx, By, Bz = brick_dims((Nx - 1, Ny - 1, Nz - 1))
    pad = np.zeros((Bz * BRICK + 1, By * BRICK + 1, Bx * BRICK + 1, E), grid.dtype)
    pad[:Nz, :Ny, :Nx] = grid
    pool = np.zeros((len(bricks), P, P, P, E), grid.dtype)
    for s, b in enumerate(np.asarray(bricks, np.int64)):
        bx, by, bz = b % Bx, (b // Bx) % By, b // (Bx * By)
        pool[s] = pad[8 * bz:8 * bz + P, 8 * by:8 * by + P, 8 * bx:8 * bx + P]
    return pool


def scatter(pool, bricks, resolution):
    """grid [Nz, Ny, Nx, E] of a pool: zero outside the bricks.  A grid point is written by its owner, the brick of cell
    min(i, C - 1) per axis: a far face (l = 8) belongs to the next brick unless it is the grid's last point."""
    Nx, Ny, Nz = resolution
    Bx, By, Bz = brick_dims((Nx - 1, Ny - 1, Nz - 1))
    grid = np.zeros((Nz, Ny, Nx, pool.shape[4]), pool.dtype)
    for s, b in enumerate(np.asarray(bricks, np.int64)):
        bx, by, bz = b % Bx, (b // Bx) % By, b // (Bx * By)
        for lz in range(P):
            for ly in range(P):
                for lx in range(P):
                    x, y, z = 8 * bx + lx, 8 * by + ly, 8 * bz + lz
                    if x >= Nx or y >= Ny or z >= Nz:
                        continue
                    if (lx == 8 and x != Nx - 1) or (ly == 8 and y != Ny - 1) or (lz == 8 and z != Nz - 1):
                        continue
                    grid[z, y, x] = pool[s, lz, ly, lx]
    return grid


def cell_bits(pool_sigma, slots, cells):
    """bool [Cz, Cy, Cx] from the pool alone: a cell is occupied iff its brick has a slot and one of its eight pool corners has a
    finite sigma >= the smallest positive fp32."""
    Cx, Cy, Cz = cells
    with np.errstate(invalid="ignore"):
        kept = np.isfinite(pool_sigma) & (pool_sigma >= TINY)
    out = np.zeros((Cz, Cy, Cx), bool)
    for z in range(Cz):
        for y in range(Cy):
            for x in range(Cx):
                s = slots[z // 8, y // 8, x // 8]
                if s >= 0:
                    out[z, y, x] = kept[s, z % 8:z % 8 + 2, y % 8:y % 8 + 2, x % 8:x % 8 + 2].any()
    return out


def dense_cell_bits(sigma):
    """bool [Cz, Cy, Cx] of a dense sigma [Nz, Ny, Nx]: OccupancyGrid.from_density at the smallest positive fp32, no dilation."""
    with np.errstate(invalid="ignore"):
        k = np.isfinite(sigma) & (sigma >= TINY)
    c = np.zeros(tuple(n - 1 for n in k.shape), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                c |= k[dz:dz + c.shape[0], dy:dy + c.shape[1], dx:dx + c.shape[2]]
    return c


def zero_outside(grid, bits):
    """`grid` [Nz, Ny, Nx, E] with every point whose OWNER brick (that of cell min(i, C - 1) per axis) is empty set to zero
    (bits: bool [Bz, By, Bx]).  A scene's grid is like that: a kept point makes every cell that touches it occupied, its owner's
    among them."""
    Nz, Ny, Nx, _ = grid.shape
    owner = lambda n: np.minimum(np.arange(n), n - 2) // BRICK
    keep = bits[owner(Nz)[:, None, None], owner(Ny)[None, :, None], owner(Nx)[None, None, :]]
    return np.where(keep[..., None], grid, np.zeros((), grid.dtype))
