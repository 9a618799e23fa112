"""fp64 numpy restatement of a baked scene's render (include/upnerf_hip.h: upnerf_baked_render; upnerf_amd/baked.py), brute force
over every lattice sample: the occupancy bits are never consulted.  Shared by tests/test_baked_cpu.py (closed forms) and
tests/test_hip_baked.py (the kernel), which also take their grids and rays from here.

    render(rgbs, bounds, rays, step, background, stop) -> {"rgb" [R, 3], "depth" [R], "opacity" [R], "n" [R], "gate_*"}

A ray's samples are stated here once, for every march of a baked scene (baked_sh_ref, baked_tune_ref, baked_pose_ref,
baked_prune_ref and baked_upsample_ref call these and keep only what is their own): args64 (the arguments as fp32 numbers),
lattice (t, g and the gate `g`), moved and blended (v and the gate `v`), alphas (the gate `alpha`), transmit (the gates `T` and `w`,
sample by sample) and visited (the same as arrays up to `stop`).  A new march extends these; it does not copy them.

The definition.  Inputs are fp32 numbers, all arithmetic fp64 except K, which IS a fp32 number: K = ceilf((far - near) / step).
t_k = near + (k + 0.5) step; p = o + t_k d; g = (p - lo) C / (hi - lo) per axis; a sample with g < 0 or g > C on an axis
contributes nothing; i = min(floor(g), C - 1), f = g - i; v = trilinear blend of the eight corners (r, g, b, sigma);
alpha = 1 - exp(-sigma step |d|); w = T alpha; rgb += w c, depth += w t_k, opacity += w; T *= 1 - alpha; with stop > 0 the ray
ends after the sample that brought T below stop; rgb += (1 - opacity) background, depth += (1 - opacity) far.  A ray with a
number that is not finite, or with far <= near, is a miss.

The gates (u = 2^-24, the unit roundoff of fp32), a first-order bound of what the fp32 kernel may differ by, ray by ray, from the
reference's own numbers -- no constant that is not a count of roundings:
  g      t_k is one fma (u |t|, times |d| in p), p one fma (u |p|), p - lo one rounding (u |p - lo|), the product with inv one
         more and inv itself another (2 u |g|):  dg = u (inv (|t d| + |p| + |p - lo|) + 2 |g|).
  v      moves by at most max |v(g +- dg e_a) - v(g)| per axis (evaluated, not estimated: it covers a sample that changes its
         cell, and one that enters or leaves the box -- the test grids are zero on their outermost layer, so v is continuous
         there), and each of its three blends fma(f, b - a, a) rounds twice on values <= 3 max |corner|: 9 u max |corner|.
  alpha  delta = step sqrt(fma, fma, product): three roundings and half of them through the root, the product with step, the
         product with sigma: 6 u relative in x = delta sigma; expf to one ulp, 2 u e; the difference 1 - e, u alpha:
         d alpha = e (6 u x + delta dv_sigma + 2 u) + u alpha.
  T      dT' = dT (1 - alpha) + T (d alpha + u (1 - alpha)) + u T'   (1 - alpha is formed from alpha, then the product).
  w      dw = dT alpha + T d alpha + u w.
  sums   rgb: sum (dw |c| + w dv_c) + (n + 2) u (sum w |c| + |background|) + d opacity |background|;
         depth: sum (dw t + w u t) + (n + 2) u (sum w t + |far|) + d opacity |far|;  opacity: sum dw + n u sum w."""
import numpy as np

U = 2.0 ** -24
BOUNDS = ((-0.7, -0.5, -0.6), (0.8, 0.6, 0.9))


def bounds64(bounds):
    return tuple(np.asarray(b, np.float32).astype(np.float64) for b in bounds)


def prune(sigma, rgb, level):
    """rgbs [Nz, Ny, Nx, 4] fp32 of sigma [Nz, Ny, Nx] and rgb [Nz, Ny, Nx, 3] (or None): a point is kept iff its sigma is finite,
    positive and >= level; every other point is (0, 0, 0, 0)."""
    sigma = np.asarray(sigma, np.float32)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(sigma) & (sigma > 0) & (sigma >= np.float32(level))
    out = np.zeros(sigma.shape + (4,), np.float32)
    if rgb is not None:
        out[..., :3] = np.where(keep[..., None], np.asarray(rgb, np.float32), 0)
    out[..., 3] = np.where(keep, sigma, 0)
    return out


def occupied_cells(rgbs):
    """bool [Cz, Cy, Cx]: a cell is occupied iff one of its corners kept a positive sigma."""
    s = rgbs[..., 3] > 0
    c = np.zeros(tuple(n - 1 for n in s.shape), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                c |= s[dz:dz + c.shape[0], dy:dy + c.shape[1], dx:dx + c.shape[2]]
    return c


def n_samples(near, far, step):
    """K of a ray: a fp32 number."""
    with np.errstate(over="ignore"):
        k = np.ceil((np.float32(far) - np.float32(near)) / np.float32(step))
    return int(min(k, 4194304))


def trilinear(grid, g, C):
    """[n, 4] values of grid [Nz, Ny, Nx, 4] (fp64) at grid coordinates g [n, 3]; a row with a coordinate outside [0, C] is 0."""
    inside = ((g >= 0) & (g <= C)).all(1)
    gi = np.where(inside[:, None], g, 0.0)
    i = np.minimum(np.floor(gi), C - 1).astype(np.int64)
    f = gi - i
    x, y, z = i[:, 0], i[:, 1], i[:, 2]
    fx, fy, fz = f[:, 0:1], f[:, 1:2], f[:, 2:3]
    c = lambda dz, dy, dx: grid[z + dz, y + dy, x + dx]
    x00, x10 = c(0, 0, 0) + fx * (c(0, 0, 1) - c(0, 0, 0)), c(0, 1, 0) + fx * (c(0, 1, 1) - c(0, 1, 0))
    x01, x11 = c(1, 0, 0) + fx * (c(1, 0, 1) - c(1, 0, 0)), c(1, 1, 0) + fx * (c(1, 1, 1) - c(1, 1, 0))
    y0, y1 = x00 + fy * (x10 - x00), x01 + fy * (x11 - x01)
    v = y0 + fz * (y1 - y0)
    cmax = np.zeros_like(v)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cmax = np.maximum(cmax, np.abs(c(dz, dy, dx)))
    return np.where(inside[:, None], v, 0.0), inside, np.where(inside[:, None], cmax, 0.0)


def args64(bounds, rays, shape, step, background=0.0, stop=0.0):
    """(lo, hi, C, rays, step, background, stop) as a march takes them: the fp32 numbers of the arguments in fp64, and the cells
    per axis C (x, y, z) of points [Nz, Ny, Nx, ...] of `shape`."""
    lo, hi = bounds64(bounds)
    C = np.array(shape[2::-1], np.float64) - 1
    return (lo, hi, C, np.asarray(rays, np.float32).astype(np.float64)) + tuple(float(np.float32(x)) for x in (step, background, stop))


def lattice(lo, hi, C, row, step):
    """(t [K], g [K, 3], dg [K, 3], inv [3]) of a ray's samples, or None for a miss (a number that is not finite, far <= near)."""
    o, d, near, far = row[:3], row[3:6], row[6], row[7]
    if not np.isfinite(row).all() or not far > near:
        return None
    t = near + (np.arange(n_samples(near, far, step), dtype=np.float64) + 0.5) * step
    inv = C / (hi - lo)
    p = o + t[:, None] * d
    g = (p - lo) * inv
    return t, g, U * (inv * (np.abs(t[:, None] * d) + np.abs(p) + np.abs(p - lo)) + 2 * np.abs(g)), inv


def moved(fn, g, dg, C, onto=0.0):
    """`onto` plus, axis after axis, the largest |fn(g +- dg e_a) - fn(g)|.  (A sample just outside the box is judged at its face:
    v = 0 there.)  Additions are not associative: a caller that adds the three axes' sum to its other terms passes nothing."""
    base, total = fn(g), onto
    for a in range(3):
        e = np.zeros(3)
        e[a] = 1.0
        worst = 0.0
        for s in (-1.0, 1.0):
            worst = np.maximum(worst, np.abs(fn(np.clip(g + s * dg[:, a:a + 1] * e, 0.0, C)) - base))
        total = total + worst
    return total


def blended(grid, g, dg, C, dcol=None, gates=True, apart=False):
    """(v [K, ch], inside [K], dv [K, ch]) of the samples: the gate `v` of the docstring, with the largest dcol among a sample's
    eight corners (baked_sh_ref) where the corners carry an error of their own; zeros with gates=False.  apart: the moves of the
    three axes are summed on their own and added last (baked_pose_ref's order of the same terms)."""
    v, inside, cmax = trilinear(grid, g, C)
    if not gates:
        return v, inside, np.zeros_like(v)
    own = 9 * U * cmax + (trilinear(dcol, g, C)[2] if dcol is not None else 0.0)
    move = moved(lambda x: trilinear(grid, x, C)[0], g, dg, C, 0.0 if apart else own)
    return v, inside, own + move if apart else move


def alphas(sigma, dsigma, d, step):
    """(delta, x, dx, alpha, dalpha) of blended densities sigma [K] with gates dsigma: the gate `alpha`, dx the part of it on x."""
    delta = step * np.sqrt((d * d).sum())
    x = delta * sigma
    dx = 6 * U * np.abs(x) + delta * dsigma
    alpha = -np.expm1(-x)
    return delta, x, dx, alpha, np.exp(-x) * (dx + 2 * U) + U * np.abs(alpha)


def transmit(alpha, dalpha, ks):
    """The gates `T` and `w` along the samples ks: yields (k, T, dT, w, dw, T', dT') -- the transmittance before sample k and
    after it.  Where the ray ends is the consumer's decision: it breaks."""
    T, dT = 1.0, 0.0
    for k in ks:
        a = alpha[k]
        w = T * a
        Tn = T * (1.0 - a)
        dTn = dT * (1.0 - a) + T * (dalpha[k] + U * (1.0 - a)) + U * Tn
        yield k, T, dT, w, dT * a + T * dalpha[k] + U * w, Tn, dTn
        T, dT = Tn, dTn


def visited(alpha, dalpha, inside, stop):
    """(ks, w, dw, T', dT', stop margin) of the visited samples as arrays: those inside the box up to the one that brings T below
    `stop`; the margin is the least |T' - stop| - dT' (only a positive one lets fp32 and fp64 end the ray alike)."""
    rows, margin = [], np.inf
    for k, _, _, w, dw, Tn, dTn in transmit(alpha, dalpha, np.nonzero(inside)[0]):
        rows.append((k, w, dw, Tn, dTn))
        if stop > 0:
            margin = min(margin, abs(Tn - stop) - dTn)
            if Tn < stop:
                break
    ks, w, dw, Tn, dTn = (np.asarray(z, np.float64) for z in zip(*rows)) if rows else (np.zeros(0),) * 5
    return ks.astype(np.int64), w, dw, Tn, dTn, margin


def render_ray(grid, lo, hi, C, row, step, background, stop, dcol=None, clamp=False):
    """One ray; returns (rgb [3], depth, opacity, n contributing samples, gates (rgb [3], depth, opacity), n inside).  dcol: the
    corners' own errors (baked_sh_ref).  clamp: the blended colours are held to [0, 1], and a seventh value counts the colour
    values (below 0, above 1, neither) of the contributing samples."""
    far, counts = row[7], np.zeros(3, np.int64)
    lat = lattice(lo, hi, C, row, step)
    if lat is None:
        return (np.full(3, background), far, 0.0, 0, (np.zeros(3), 0.0, 0.0), 0) + ((counts,) if clamp else ())
    t, g, dg, _ = lat
    v, inside, dv = blended(grid, g, dg, C, dcol)
    raw = v[:, :3].copy()
    if clamp:
        v[:, :3] = np.clip(raw, 0.0, 1.0)
    alpha, dalpha = alphas(v[:, 3], dv[:, 3], row[3:6], step)[3:]
    rgb, depth, op = np.zeros(3), 0.0, 0.0
    g_rgb, g_depth, g_op = np.zeros(3), 0.0, 0.0
    s_rgb, s_depth = np.zeros(3), 0.0
    n = 0
    for k, _, _, w, dw, Tn, _ in transmit(alpha, dalpha, np.nonzero(inside)[0]):
        rgb += w * v[k, :3]
        depth += w * t[k]
        op += w
        g_rgb += dw * np.abs(v[k, :3]) + w * dv[k, :3]
        g_depth += dw * abs(t[k]) + w * U * abs(t[k])
        g_op += dw
        s_rgb += w * np.abs(v[k, :3])
        s_depth += w * abs(t[k])
        if w != 0.0:
            n += 1
            counts += [int((raw[k] < 0).sum()), int((raw[k] > 1).sum()), int(((raw[k] >= 0) & (raw[k] <= 1)).sum())]
        if stop > 0 and Tn < stop:
            break
    g_op += n * U * op
    g_rgb += (n + 2) * U * (s_rgb + abs(background)) + g_op * abs(background)
    g_depth += (n + 2) * U * (s_depth + abs(far)) + g_op * abs(far)
    rgb = rgb + (1.0 - op) * background
    depth = depth + (1.0 - op) * far
    return (rgb, depth, op, n, (g_rgb, g_depth, g_op), int(inside.sum())) + ((counts,) if clamp else ())


def render_rows(rays, one, clamp=False):
    """The dict of `render` from one(row) -> render_ray's tuple, ray by ray."""
    R = rays.shape[0]
    out = {"rgb": np.zeros((R, 3)), "depth": np.zeros(R), "opacity": np.zeros(R), "n": np.zeros(R, np.int64),
           "gate_rgb": np.zeros((R, 3)), "gate_depth": np.zeros(R), "gate_opacity": np.zeros(R), "inside": np.zeros(R, np.int64)}
    if clamp:
        out["clamp"] = np.zeros((R, 3), np.int64)
    for r in range(R):
        res = one(rays[r])
        out["rgb"][r], out["depth"][r], out["opacity"][r], out["n"][r], out["inside"][r] = res[:4] + res[5:6]
        out["gate_rgb"][r], out["gate_depth"][r], out["gate_opacity"][r] = res[4]
        if clamp:
            out["clamp"][r] = res[6]
    return out


def render(rgbs, bounds, rays, step, background=0.0, stop=0.0):
    """The restatement over rays [R, 8] fp32 and rgbs [Nz, Ny, Nx, 4] fp32."""
    grid = np.asarray(rgbs, np.float32).astype(np.float64)
    lo, hi, C, rays, step, background, stop = args64(bounds, rays, grid.shape, step, background, stop)
    return render_rows(rays, lambda row: render_ray(grid, lo, hi, C, row, step, background, stop))


# ---- the test scenes ----------------------------------------------------------------------------------------------------------------

def blob_grid(shape=(11, 10, 9), seed=4, level=0.4):
    """(rgbs, level) of a [Nz, Ny, Nx] = 11 x 10 x 9 point grid -- 8 x 9 x 10 cells: the bricks are cut at another place on every
    axis and 720 cell bits are no multiple of 32 -- with smooth random density up to ~40 in its interior (some rays end inside it), pruned at `level`, and
    zero on its outermost layer of points."""
    rng = np.random.RandomState(seed)
    Nz, Ny, Nx = shape
    z, y, x = np.meshgrid(np.linspace(-1, 1, Nz), np.linspace(-1, 1, Ny), np.linspace(-1, 1, Nx), indexing="ij")
    sigma = np.zeros(shape)
    for _ in range(3):
        c = rng.uniform(-0.5, 0.5, 3)
        sigma += rng.uniform(5, 25) * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * rng.uniform(0.2, 0.35) ** 2))
    sigma[[0, -1]] = sigma[:, [0, -1]] = sigma[:, :, [0, -1]] = 0
    rgb = rng.uniform(0, 1, shape + (3,))
    return prune(sigma.astype(np.float32), rgb.astype(np.float32), level), level


def corner_grid(seed=6):
    """(rgbs, level) of 17 x 17 x 17 points (two bricks per axis) with density in two opposite corner bricks only: six whole
    empty bricks, and between the two the plane of bricks each shares with none.  Zero on the outermost layer."""
    rng = np.random.RandomState(seed)
    sigma = np.zeros((17, 17, 17))
    sigma[1:7, 1:7, 1:7] = rng.uniform(0.5, 5.0, (6, 6, 6))
    sigma[10:16, 10:16, 10:16] = rng.uniform(0.5, 5.0, (6, 6, 6))
    rgb = rng.uniform(0, 1, (17, 17, 17, 3))
    return prune(sigma.astype(np.float32), rgb.astype(np.float32), 1.0), 1.0


def make_rays(bounds=BOUNDS, seed=9, R=67):
    """[67, 8] fp32 rays round the box: the named special cases first, random rays through the box after them."""
    lo, hi = bounds64(bounds)
    mid, ext = (lo + hi) / 2, hi - lo
    rng = np.random.RandomState(seed)
    rows = []

    def ray(o, d, near, far):
        rows.append(list(o) + list(d) + [near, far])

    ray([lo[0] - 0.5, mid[1] + 0.013, mid[2] - 0.021], [1, 0, 0], 0.0, ext[0] + 1.0)     # 0: axis-parallel, two zero components
    ray(mid + [0.05, -0.03, 0.02], [0.3, -0.5, 0.8], 0.0, 3.0)                             # 1: starts inside the box
    ray([lo[0] - 0.5, hi[1] + 0.4, mid[2]], [1, 0.05, 0.02], 0.0, 3.0)                     # 2: misses the box
    dn = (hi - lo) / np.linalg.norm(hi - lo)
    ray(lo - 0.3 * dn, dn, 0.3 + 0.35 * np.linalg.norm(ext), 0.3 + 0.7 * np.linalg.norm(ext))  # 3: near / far cut inside the box
    d4 = np.array([0.6, 0.5, -0.62])
    ray(mid - 1.2 * d4, 2.5 * d4 / np.linalg.norm(d4), 0.0, 1.2)                           # 4: |d| = 2.5
    ray([np.nan, 0, 0], [0, 0, 1], 0.0, 2.0)                                               # 5: a NaN
    ray(lo - 0.2, [1, 1, 1], 1.5, 1.5)                                                     # 6: far <= near
    ray([mid[0], mid[1], hi[2] + 0.4], [0, 0, -1], 0.1, ext[2] + 0.8)                      # 7: axis-parallel, against the axis
    while len(rows) < R:
        a = mid + rng.uniform(-0.45, 0.45, 3) * ext  # a point in the box the ray goes through
        d = rng.randn(3)
        d /= np.linalg.norm(d)
        back = rng.uniform(0.8, 1.6)
        ray(a - back * d, d * rng.uniform(0.7, 1.4), rng.uniform(0.0, 0.2), back + rng.uniform(0.6, 1.8))
    return np.asarray(rows, np.float32)


def cell_size(rgbs, bounds=BOUNDS):
    lo, hi = bounds64(bounds)
    return float(((hi - lo) / (np.array(rgbs.shape[2::-1]) - 1)).min())
