"""Adversarial grids and rays for the two walks -- baked_walk (csrc/baked.hip) and occ_walk (csrc/occupancy.hip) -- shared by
tests/test_walks_host_cpu.py (the host programs of tests/host/) and tests/test_hip_walk_edges.py (the entry points on the GPU).

Grids (all in baked_ref.BOUNDS; (rgbs [Nz, Ny, Nx, 4] fp32, level, edge)): `blob` and `corners` are baked_ref's, zero on their
outermost layer of points.  `faces` has density and colour on all six faces and a mostly empty interior; `ragged` is 17 x 9 x 1
cells (3 x 2 x 1 bricks, one of them empty, a single cell in z); `one-cell` is 16^3 cells with the grid's last point kept alone:
one occupied cell in the far corner brick, seven empty bricks.  edge = the grid has density on its outermost layer, where the
blend is not continuous across the face and fp32 and fp64 may take different sides: baked_ref's gate does not cover a sample
there, and `borderline` names the rays that have one.

Ray families (fp32 [n, 8], seeded): see each generator.  `ref=True` is the parametrisation for the comparison with fp64 on the
edge grids, chosen so that few rays have a sample within its dg of a face (borderline); it gives up what the family is named
for (no lo or hi face in `in-plane`, a twentieth to half a step instead of ulps in `faces-start`, 10 and 100 diagonals in
`far-origin`, interior lattice points in `vertices`), so that comparison does not see those cases.  The exact checks use
ref=False on every grid."""
import numpy as np

import baked_ref as br
import baked_sh_ref as sh
import baked_sparse_ref as sr

BOUNDS = br.BOUNDS
FAMILIES = ("vertices", "in-plane", "shallow", "faces-start", "far-origin", "caps", "random-wide")
F32 = np.float32


def faces_grid(seed=21):
    rng = np.random.RandomState(seed)
    shape = (9, 10, 17)  # 16 x 9 x 8 cells
    sigma = rng.uniform(0.5, 6.0, shape)
    inner = rng.uniform(size=(7, 8, 15)) < 0.2
    sigma[1:-1, 1:-1, 1:-1] *= inner
    rgb = rng.uniform(0, 1, shape + (3,))
    return br.prune(sigma.astype(F32), rgb.astype(F32), 0.4), 0.4


def ragged_grid(seed=22):
    rng = np.random.RandomState(seed)
    shape = (2, 10, 18)  # 17 x 9 x 1 cells
    sigma = rng.uniform(0.5, 8.0, shape) * (rng.uniform(size=shape) < 0.4)
    sigma[:, :, 8:17] = 0  # cells 8 .. 15 in x: an empty brick between two occupied ones (the last holds one cell per row)
    sigma[:, :, 17] = rng.uniform(0.5, 8.0, (2, 10))
    rgb = rng.uniform(0, 1, shape + (3,))
    return br.prune(sigma.astype(F32), rgb.astype(F32), 0.4), 0.4


def one_cell_grid(seed=23):
    rng = np.random.RandomState(seed)
    sigma = np.zeros((17, 17, 17))
    sigma[16, 16, 16] = 30.0
    rgb = rng.uniform(0, 1, (17, 17, 17, 3))
    return br.prune(sigma.astype(F32), rgb.astype(F32), 1.0), 1.0


GRIDS = {"blob": (br.blob_grid, False), "corners": (br.corner_grid, False), "faces": (faces_grid, True), "ragged": (ragged_grid, True),
         "one-cell": (one_cell_grid, True)}
_SCENES = {}


def scene(name):
    """Everything a march of the grid reads, as numpy arrays, built once: rgbs, level, edge, cells (Cx, Cy, Cz), bits
    [Cz, Cy, Cx], words, slots, bricks, points[degree] (rgbs | records) and pool[degree]."""
    if name not in _SCENES:
        make, edge = GRIDS[name]
        rgbs, level = make()
        sigma = rgbs[..., 3]
        bits = sr.dense_cell_bits(sigma)
        slots, bricks = sr.table(sr.brick_bits(bits))
        points = {0: rgbs}
        for degree in (1, 2):
            points[degree] = sh.pack(sh.coefficients(sigma.shape, degree, 31 + degree), sigma, level, degree)[0]
        pool = {0: sr.gather(rgbs, bricks)}
        for degree in (1, 2):
            pool[degree] = sr.gather(points[degree], bricks)
        _SCENES[name] = dict(name=name, rgbs=rgbs, level=level, edge=edge, cells=tuple(int(n) - 1 for n in sigma.shape[::-1]), bits=bits,
                             words=sr.words(bits), slots=slots, bricks=bricks, points=points, pool=pool)
    return _SCENES[name]


def steps(name):
    """t per step: about a cell, a tenth of a cell, and more than the box's diagonal."""
    lo, hi = br.bounds64(BOUNDS)
    cell = br.cell_size(scene(name)["rgbs"])
    return {"cell": float(F32(cell)), "tenth": float(F32(cell / 10)), "over": float(F32(1.5 * np.linalg.norm(hi - lo)))}


def _ulps(x, j):
    """fp32 x moved by j units in its last place."""
    x = np.asarray(x, F32)
    for _ in range(abs(int(j))):
        x = np.nextafter(x, F32(np.inf if j > 0 else -np.inf))
    return x


def _slab(o, d, lo, hi):
    """(t_in, t_out) of the line o + t d through the box, fp64; d without a zero component."""
    ta, tb = (lo - o) / d, (hi - o) / d
    return np.minimum(ta, tb).max(), np.maximum(ta, tb).min()


def _through(rng, lo, hi, speed=1.0):
    """A ray through a random point of the box from outside it: (o, d, t_in, t_out) in fp64, |d| = speed."""
    mid, ext = (lo + hi) / 2, hi - lo
    a = mid + rng.uniform(-0.45, 0.45, 3) * ext
    u = rng.randn(3)
    u /= np.linalg.norm(u)
    o = (a - rng.uniform(2.0, 3.0) * u).astype(F32).astype(np.float64)
    d = (speed * u).astype(F32).astype(np.float64)
    return (o, d) + _slab(o, d, lo, hi)


def family(name, n, seed, cells, step, ref=False, big=True):
    """fp32 [n, 8] rays of a family for a grid of `cells` in BOUNDS marched at `step`."""
    lo, hi = br.bounds64(BOUNDS)
    mid, ext = (lo + hi) / 2, hi - lo
    C = np.asarray(cells, np.float64)
    cell = ext / C
    diag = float(np.linalg.norm(ext))
    rng = np.random.RandomState(seed * 101 + FAMILIES.index(name))
    rows = []

    def ray(o, d, near, far):
        rows.append(np.concatenate([np.asarray(o, np.float64), np.asarray(d, np.float64), [near, far]]).astype(F32))

    while len(rows) < n:
        i = len(rows)
        if name == "vertices":
            # from a lattice point (inside the box or up to three cells outside) along small integer ratios of the cells: the
            # ray goes through cell corners and edges, so the exit planes tie on two and three axes
            k = np.array([rng.randint(-3, int(c) + 4) for c in C], np.float64)
            if ref:  # from a lattice point strictly inside the box (half a cell in on an axis of one cell)
                k = np.array([rng.randint(1, int(c)) if c > 1 else 0.5 for c in C])
            m = rng.randint(-3, 4, 3)
            if not m.any():
                continue
            s = rng.choice([0.5, 1.0, 2.0])
            near = rng.choice([0.0, -1.0, 0.5]) if not ref else rng.uniform(0.0, 0.3)
            ray(lo + k * cell, s * m * cell, near, near + rng.uniform(2.0, 20.0) / s)
        elif name == "in-plane":
            # the origin exactly on a grid plane with d == 0 on that axis: the lo face, the hi face (outside: o < hi is the
            # rule) and planes between; every third ray does so on two axes (along an edge of the box or of a cell)
            o = mid + rng.uniform(-0.7, 0.7, 3) * ext
            d = rng.randn(3)
            axes = rng.permutation(3)[:2 if i % 3 == 2 else 1]
            for a in axes:
                pick = rng.randint(3) if not ref else 2
                o[a] = (lo[a], hi[a], lo[a] + rng.randint(1, max(int(C[a]), 2)) * cell[a])[pick]
                if C[a] == 1 and pick == 2:
                    o[a] = lo[a] + 0.5 * cell[a]
                d[a] = 0.0
            d /= np.linalg.norm(d)
            back = rng.uniform(0.0, 2.0)
            ray(o - back * d, d, rng.choice([0.0, 0.1]), back + rng.uniform(0.5, 3.0))
        elif name == "shallow":
            # one component of 1 next to one or two tiny ones, down to denormals whose reciprocal is inf in fp32
            a = rng.randint(3)
            d = np.zeros(3)
            d[a] = rng.choice([-1.0, 1.0])
            tiny = [1e-3, 1e-7, 1e-20, 1e-38, 1e-39, 1.4e-45]
            for b in rng.permutation([x for x in range(3) if x != a])[:1 + i % 2]:
                d[b] = rng.choice([-1.0, 1.0]) * tiny[rng.randint(len(tiny))]
            o = mid + rng.uniform(-0.55, 0.55, 3) * ext
            if i % 4 == 0 and not ref:  # the slow coordinate on a face or a grid plane
                b = (a + 1) % 3
                o[b] = (lo[b], hi[b], lo[b] + rng.randint(0, int(C[b]) + 1) * cell[b])[rng.randint(3)]
            o[a] = mid[a] - d[a] * rng.uniform(0.2, 1.5) * ext[a]
            ray(o, d, 0.0, rng.uniform(0.5, 3.0) * ext[a])
        elif name == "faces-start":
            # sample 0 (even rays), the last sample (i % 4 == 1) or the span's entry / exit (i % 4 == 3) within a few fp32 ulps of
            # where the ray enters or leaves the box, inside and outside; ref: a twentieth to half a step away instead
            o, d, t_in, t_out = _through(rng, lo, hi, rng.uniform(0.7, 1.4))
            if not t_out > t_in:
                continue
            j = int(rng.randint(-2, 3))
            off = rng.choice([-1.0, 1.0]) * rng.uniform(0.05, 0.45) * step if ref else 0.0
            if i % 4 == 0 or i % 4 == 2:
                ray(o, d, _ulps(F32(t_in - 0.5 * step + off), j), t_out + rng.uniform(0.1, 0.5))
            elif i % 4 == 1:
                near = F32(rng.uniform(0.0, 0.2))
                k = np.floor((t_out - near) / step)
                ray(o, d, near, _ulps(F32(near + k * step + off), j) if i % 8 == 1 else _ulps(F32(t_out + off), j))
            else:
                ray(o, d, _ulps(F32(t_in + off), j), _ulps(F32(t_out + off), int(rng.randint(-2, 3))))
        elif name == "far-origin":
            # origins 1e3 and 1e6 box sizes away, aimed at the box: p - lo cancels, and at the larger distance a step is less
            # than an ulp of t, so consecutive t_k are equal
            D = ((1e3, 1e6) if not ref else (1e1, 1e2))[i % 2] * diag  # (ref: at 1e6 diagonals dg is larger than the grid)
            a = mid + rng.uniform(-0.45, 0.45, 3) * ext
            u = rng.randn(3)
            u /= np.linalg.norm(u)
            ray(a - D * u, u, D - diag, D + diag)
        elif name == "caps":
            o, d, t_in, t_out = _through(rng, lo, hi, 1.0)
            near = max(t_in - 0.3, 0.0)
            kind = i % 9
            if kind == 0 and i < 18 and big:  # more samples than UPNERF_BAKED_MAX_SAMPLES: two rays (4 M samples each)
                ray(o, d, near, near + 5.0e6 * step)
            elif kind == 1:
                ray(o, d, near, float(F32(near)) + step / 2)  # K = 1
            elif kind == 2:
                ray(o, d, near, np.inf)
            elif kind == 3:
                ray(o, d, -np.inf, t_out)
            elif kind == 4:
                ray(o, d, (np.nan, near)[i % 2], (t_out, np.nan)[i % 2])
            elif kind == 5:
                ray(o, d, -rng.uniform(0.5, 3.0), t_out + 0.2)  # a negative near: samples behind the origin
            elif kind == 6:
                ray(o, d, t_out + 0.2, near)  # far < near
            elif kind == 7:
                ray(o, d, near, float(F32(near)))  # far == near
            else:
                ray(o, d, near, near + rng.uniform(0.2, 1.0) * step)  # one sample, short of a step
        elif name == "random-wide":
            # baked_ref.make_rays' random rays with |d| in [0.1, 10] and no component held away from zero
            a = mid + rng.uniform(-0.45, 0.45, 3) * ext
            u = rng.randn(3)
            u /= np.linalg.norm(u)
            s = 10.0 ** rng.uniform(-1.0, 1.0)
            back = rng.uniform(0.8, 1.6)
            ray(a - back * u, s * u, rng.uniform(0.0, 0.2) / s, (back + rng.uniform(0.6, 1.8)) / s)
        else:
            raise KeyError(name)
    return np.stack(rows)


def rays_of(n_per_family, seed, cells, step, ref=False, big=True):
    """(rays fp32 [7 n, 8], fam int [7 n]: the index into FAMILIES of each ray)."""
    parts = [family(f, n_per_family, seed, cells, step, ref, big) for f in FAMILIES]
    return np.concatenate(parts), np.repeat(np.arange(len(FAMILIES)), n_per_family)


def borderline(cells, rays, step):
    """bool [R]: some sample of the ray has a grid coordinate within its own dg (baked_ref's, the bound of what fp32 moves it by)
    of 0 or C on an axis."""
    lo, hi = br.bounds64(BOUNDS)
    C = np.asarray(cells, np.float64)
    inv = C / (hi - lo)
    rays = np.asarray(rays, F32).astype(np.float64)
    step = float(F32(step))
    out = np.zeros(len(rays), bool)
    for r, row in enumerate(rays):
        if not np.isfinite(row).all() or not row[7] > row[6]:
            continue
        K = br.n_samples(row[6], row[7], step)
        t = row[6] + (np.arange(K, dtype=np.float64) + 0.5) * step
        p = row[:3] + t[:, None] * row[3:6]
        g = (p - lo) * inv
        dg = br.U * (inv * (np.abs(t[:, None] * row[3:6]) + np.abs(p) + np.abs(p - lo)) + 2 * np.abs(g))
        out[r] = bool(((np.abs(g) <= dg) | (np.abs(g - C) <= dg)).any())
    return out
