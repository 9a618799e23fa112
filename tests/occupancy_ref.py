"""fp64 numpy reference of the occupancy grid (upnerf_amd/occupancy.py, csrc/occupancy.hip) and the inputs of its tests.

Brute force, nothing of the kernel's traversal: a ray is intersected with the box of EVERY occupied cell by the slab test; a
cell counts when its chord, clipped to [near, far], is positive; t0 is the smallest entry and t1 the largest exit over the
cells that count.  Planes are lo + i * ((hi - lo) / C) in fp64 from the fp32 bounds."""
import numpy as np

BOUNDS = ((-1.0, -0.75, -0.5), (1.0, 0.875, 0.75))  # fp32-exact
SPAN_CASES = [  # (cells (Cx, Cy, Cz), occupied share, seed) of the random span test
    ((12, 10, 9), 0.15, 0),
    ((12, 10, 9), 0.03, 1),
    ((5, 4, 3), 0.3, 2),
]
N_RAYS = 4096
GRAZE = 1e-3  # a ray is grazing if a cell's status differs between the cell shrunk and grown by this share of its edge


def bounds64(bounds):
    lo, hi = (np.asarray(b, dtype=np.float32).astype(np.float64) for b in bounds)
    return lo, hi


def cell_status(cells, bounds, rays, eps=0.0):
    """(ok bool [R, N], te [R, N], tx [R, N], xyz [N, 3]) over the N occupied cells of `cells` (bool [Cz, Cy, Cx]): clipped entry
    and exit of every ray in every cell's box grown by eps of its edge on every side, ok = the chord is positive."""
    cells = np.asarray(cells).astype(bool)
    Cz, Cy, Cx = cells.shape
    lo, hi = bounds64(bounds)
    step = (hi - lo) / np.array([Cx, Cy, Cz], dtype=np.float64)
    xyz = np.argwhere(cells)[:, ::-1].astype(np.float64)  # [N, 3] as (x, y, z)
    p0 = lo + xyz * step - eps * step
    p1 = lo + (xyz + 1) * step + eps * step
    r = np.asarray(rays, dtype=np.float64)
    o, d = r[:, None, 0:3], r[:, None, 3:6]
    near, far = r[:, None, 6], r[:, None, 7]
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (p0 - o) / d, (p1 - o) / d
    zero = np.broadcast_to(d == 0, ta.shape)
    inside = (o >= p0) & (o < p1)  # an axis the ray does not move along: in the cell's slab or never
    ta = np.where(zero, np.where(inside, -np.inf, np.inf), ta)
    tb = np.where(zero, np.inf, tb)  # (outside: entry = exit = +inf, no chord)
    te = np.maximum(near, np.minimum(ta, tb).max(-1))
    tx = np.minimum(far, np.maximum(ta, tb).min(-1))
    return tx > te, te, tx, xyz


def spans_ref(cells, bounds, rays):
    """(t0 fp64 [R], t1 fp64 [R], hit bool [R]); t0 = t1 = far on a miss."""
    r = np.asarray(rays, dtype=np.float64)
    ok, te, tx, _ = cell_status(cells, bounds, rays)
    hit = ok.any(1) if ok.shape[1] else np.zeros(r.shape[0], bool)
    t0 = np.where(ok, te, np.inf).min(1, initial=np.inf)
    t1 = np.where(ok, tx, -np.inf).max(1, initial=-np.inf)
    return np.where(hit, t0, r[:, 7]), np.where(hit, t1, r[:, 7]), hit


def grazing(cells, bounds, rays):
    """bool [R]: the status of some occupied cell differs between the cell shrunk and grown by GRAZE of its edge."""
    small = cell_status(cells, bounds, rays, -GRAZE)[0]
    big = cell_status(cells, bounds, rays, GRAZE)[0]
    return (small != big).any(1)


def span_tolerance(dims, bounds, rays):
    """3 x (5 x 2^-24 x M / min_k |d_k|) per ray: five fp32 roundings (the plane's coordinate, the subtraction, the division) of
    numbers of size M = the largest |plane| + |o_k| of the case, with a margin of 3."""
    lo, hi = bounds64(bounds)
    r = np.asarray(rays, dtype=np.float64)
    M = (np.maximum(np.abs(lo), np.abs(hi)) + np.abs(r[:, 0:3]).max(0)).max()
    return 3.0 * 5.0 * 2.0 ** -24 * M / np.abs(r[:, 3:6]).min(1)


def random_cells(dims, share, seed):
    Cx, Cy, Cz = dims
    n = Cx * Cy * Cz  # exactly round(share * n) occupied cells, wherever the seed puts them
    flat = np.zeros(n, bool)
    flat[np.random.RandomState(1000 + seed).permutation(n)[:int(round(share * n))]] = True
    return flat.reshape(Cz, Cy, Cx)


def random_rays(bounds, seed, n=N_RAYS):
    """fp32 [n, 8]: origins half on a shell outside the box (looking at a point of a ball round the box: some miss it), half
    inside the box; unit directions with every |d_k| >= 0.05; near in [0, 0.3], far = near + [0.5, 4]."""
    rng = np.random.RandomState(seed)
    lo, hi = bounds64(bounds)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    rad = 1.25 * np.linalg.norm(h)
    rays = np.zeros((n, 8), np.float32)
    k = 0
    while k < n:
        if k < n // 2:
            v = rng.randn(3)
            o = c + rad * v / np.linalg.norm(v)
            w = rng.randn(3)
            d = c + 0.75 * np.linalg.norm(h) * rng.rand() ** (1 / 3) * w / np.linalg.norm(w) - o
        else:
            o = lo + rng.rand(3) * (hi - lo)
            d = rng.randn(3)
        d = (d / np.linalg.norm(d)).astype(np.float32)
        d = d / np.float32(np.linalg.norm(d.astype(np.float64)))
        if np.abs(d).min() < 0.05:
            continue
        near = rng.uniform(0.0, 0.3)
        rays[k] = np.concatenate([o, d, [near, near + rng.uniform(0.5, 4.0)]]).astype(np.float32)
        k += 1
    return rays
