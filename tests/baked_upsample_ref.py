"""numpy float32 / float16 restatement of the doubling of a baked scene's resolution (include/upnerf_hip.h: upnerf_baked_upsample,
upnerf_brick_upsample_mark / _fill; upnerf_amd/baked_reg.py).  The operation order is fixed and halving is exact,
so the kernels are held to it bit for bit.  Shared by tests/test_baked_upsample_cpu.py and tests/test_hip_baked_upsample.py; the
grids are those of tests/baked_tv_ref.py.

    blend(values [Nz, Ny, Nx, K]) -> [2 Nz - 1, 2 Ny - 1, 2 Nx - 1, K], the dtype kept: along x an even index copies, an odd one is
        0.5 * (a + b) of its two parents; then the same along y, then along z
    upsample(points, degree, level) -> the child's rgbs (degree 0) or records (degree 1 | 2): blend in fp32 of the stored numbers
        (the halves converted exactly), then baked_ref.prune / baked_sh_ref.pack at `level`
    numbers(points, degree) -> what the fp64 renderers take: rgbs as fp64, or (k, sigma)
    render_gate(child points, parent points, degree, bounds, rays, step, background) -> (gate_rgb [R, 3], gate_depth, gate_opacity)

The refined scene is the same continuous field as its parent: a trilinear interpolant reproduces a trilinear function, and the
child's points are the parent's interpolant at the half-integer lattice.  In exact arithmetic the two renders are equal; what
separates them is the rounding of the child's stored values alone, and render_gate is the first-order bound of that:
  value    a child value is formed by at most three fp32 additions (one per axis; the halvings are exact), each rounding on no more
           than the blend of its parents' magnitudes: delta <= 3 u A, A = blend(|parent|) (in fp64), u = 2^-24.
  half     at degree 1 | 2 a coefficient is then rounded once to fp16: 2^-11 of its magnitude (<= A + delta), or 2^-25 where it is
           subnormal.  sigma stays fp32.
  colour   at degree 1 | 2 a corner's colour is sum_j Y_j k_j: sum_j |Y_j| delta_j.  The clamp is 1-Lipschitz.
  sample   the blend of the eight corners is a convex combination: dv <= the trilinear blend of the corners' deltas.
  alpha    d alpha = exp(-delta_t sigma) delta_t dv_sigma;   dw = dT alpha + T d alpha;   dT' = dT (1 - alpha) + T d alpha.
  sums     rgb: sum dw |c| + w dv_c + d opacity |background|;  depth: sum dw |t| + d opacity |far|;  opacity: sum dw."""
import numpy as np

import baked_ref as br
import baked_sh_ref as sh

U = br.U
TINY = np.float32(2.0 ** -149)


def blend(v):
    v = np.asarray(v)
    half = v.dtype.type(0.5)
    for axis in (2, 1, 0):  # x, then y, then z
        n = v.shape[axis]
        out = np.zeros(v.shape[:axis] + (2 * n - 1,) + v.shape[axis + 1:], v.dtype)
        even, odd, lo, hi = ([slice(None)] * v.ndim for _ in range(4))
        even[axis], odd[axis], lo[axis], hi[axis] = slice(0, None, 2), slice(1, None, 2), slice(None, -1), slice(1, None)
        out[tuple(even)] = v
        with np.errstate(invalid="ignore", over="ignore"):
            out[tuple(odd)] = half * (v[tuple(lo)] + v[tuple(hi)])
        v = out
    return v


def stored(points, degree, dtype=np.float32):
    """[Nz, Ny, Nx, 4 | 3 nb + 1]: the numbers of the stored points (the halves converted exactly), sigma last."""
    if degree == 0:
        return np.asarray(points, np.float32).astype(dtype)
    nb = sh.NB[degree]
    rec = np.ascontiguousarray(points)
    k = np.ascontiguousarray(rec[..., :6 * nb]).view(np.float16).astype(dtype)
    s = np.ascontiguousarray(rec[..., sh.SIGMA_BYTE[degree]:sh.SIGMA_BYTE[degree] + 4]).view(np.float32).astype(dtype)
    return np.concatenate([k, s], -1)


def upsample(points, degree, level):
    v = blend(stored(points, degree))
    if degree == 0:
        return br.prune(v[..., 3], v[..., :3], level)
    nb = sh.NB[degree]
    return sh.pack(v[..., :3 * nb].reshape(v.shape[:3] + (3, nb)), v[..., 3 * nb], level, degree)[0]


def numbers(points, degree):
    if degree == 0:
        return np.asarray(points, np.float32).astype(np.float64)
    return sh.unpack(points, degree)


def deltas(parent, degree):
    """The bound of |stored child value - exact trilinear value| per child point and number, [2 Nz - 1, .., 4 | 3 nb + 1]."""
    A = blend(np.abs(stored(parent, degree, np.float64)))
    d = 3 * U * A
    if degree:
        d[..., :-1] += np.maximum(2.0 ** -11 * (A[..., :-1] + d[..., :-1]), 2.0 ** -25)
    return d


def render_gate(child, parent, degree, bounds, rays, step, background=0.0):
    d_all = deltas(parent, degree)
    lo, hi, C, rays, step, background, _ = br.args64(bounds, rays, d_all.shape, step, background)
    if degree == 0:
        grid = numbers(child, 0)
        dgrid = d_all
    else:
        k, sigma = numbers(child, degree)
        dk = d_all[..., :-1].reshape(sigma.shape + (3, sh.NB[degree]))
    R = rays.shape[0]
    g_rgb, g_depth, g_op = np.zeros((R, 3)), np.zeros(R), np.zeros(R)
    for r in range(R):
        d, far = rays[r, 3:6], rays[r, 7]
        lat = br.lattice(lo, hi, C, rays[r], step)
        if lat is None or (degree and not (d * d).sum() > 0):
            continue
        if degree:
            grid, _, Y, _ = sh.ray_grid(k, sigma, d, degree, gates=False)
            dgrid = np.concatenate([dk @ np.abs(Y), d_all[..., -1:]], -1)
        t, g = lat[:2]
        v, inside, _ = br.trilinear(grid, g, C)
        dv = br.trilinear(dgrid, g, C)[0]
        if degree:
            v[:, :3] = np.clip(v[:, :3], 0.0, 1.0)
        dl = step * np.sqrt((d * d).sum())
        alpha = -np.expm1(-dl * v[:, 3])
        dalpha = np.exp(-dl * v[:, 3]) * dl * dv[:, 3]
        T, dT = 1.0, 0.0
        for i in np.nonzero(inside)[0]:  # (no rounding terms: the shared recurrence does not state this one)
            a = alpha[i]
            w, dw = T * a, dT * a + T * dalpha[i]
            g_rgb[r] += dw * np.abs(v[i, :3]) + w * dv[i, :3]
            g_depth[r] += dw * abs(t[i])
            g_op[r] += dw
            dT = dT * (1.0 - a) + T * dalpha[i]
            T *= 1.0 - a
        g_rgb[r] += g_op[r] * abs(background)
        g_depth[r] += g_op[r] * abs(far)
    return g_rgb, g_depth, g_op


def parents(name, degree):
    """(points, level) of grid `name` of baked_tv_ref.GRIDS: rgbs at degree 0, else records with seeded coefficients."""
    import baked_tv_ref as tvr
    rgbs, level = tvr.GRIDS[name]()
    if degree == 0:
        return rgbs, level
    return sh.pack(sh.coefficients(rgbs[..., 3].shape, degree, 11 + degree), rgbs[..., 3], level, degree)[0], level
