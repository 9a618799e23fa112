"""fp64 numpy restatement of the baked marcher's gradient (include/upnerf_hip.h: upnerf_baked_render_bwd, upnerf_baked_project;
upnerf_amd/baked_tune.py): brute force over every lattice sample, the occupancy bits never consulted.  It extends
tests/baked_ref.py and tests/baked_sh_ref.py, whose definitions, grids, rays and sample statements it calls and does not repeat;
`march` adds what the upstream gradients make of a ray's visited samples, for this file's scatter and for baked_pose_ref.
Shared by tests/test_baked_tune_cpu.py and tests/test_hip_baked_tune.py.

    grad(points, degree, bounds, rays, step, background, stop, g_rgb, g_depth, g_opacity, gates=True) -> dict
        degree 0: points = rgbs [Nz, Ny, Nx, 4]; "grad" and "gate" [Nz, Ny, Nx, 4]
        degree 1 | 2: points = (k [Nz, Ny, Nx, 3, nb], sigma [Nz, Ny, Nx]) as numbers (fp64 or the stored fp32 / fp16 values);
        "grad_coef", "gate_coef" [Nz, Ny, Nx, 3, nb] and "grad_sigma", "gate_sigma" [Nz, Ny, Nx]
        "stop_margin": the least |T - stop| - dT over the samples (only a positive one lets fp32 and fp64 end a ray alike)
    functional(points, degree, ...) -> sum_r g_rgb . rgb + g_depth depth + g_opacity opacity, the fp64 render the gradient is of

The definition.  L is any function of the forward's outputs with upstream gradients g_rgb, g_depth, g_opacity.  The visited samples
of a ray are those inside the box, in order, the one that brings T below `stop` the last.  For sample k with blended (degree > 0:
clamped) channels v, alpha, w = T alpha, T' = T (1 - alpha):
    q = g_rgb . (c - background) + g_depth (t - far) + g_opacity
    dL/dc = w g_rgb, zero in a channel whose unclamped blend is outside [0, 1];   dL/dsigma = delta (T' q - sum_{j > k} w_j q_j).
Grid point p receives hat(gx - px) hat(gy - py) hat(gz - pz) times these four (hat(x) = max(0, 1 - |x|): the trilinear weight of
a corner of the sample's cell, zero elsewhere); at degree > 0 coefficient (c, j) receives Y_j times the share of channel c.  A
point whose stored sigma is exactly zero receives nothing.  Nothing for a miss or a ray whose upstream gradients are all zero.

The gates (u = 2^-24), first order, every constant a count of roundings; baked_ref's dg, dv, dalpha, dT, dw are taken as they are.
  weight   f = g - i is exact; each 1 - f rounds once and the two products once each: 5 u wt.  The MOVED-SAMPLE term applies to the
           weights: a sample that fp32 places dg away gives point p the weight hat(g +- dg e_a - p): the change is evaluated per
           axis on the 4 x 4 x 4 points round the sample's cell, so a sample that changes its cell is covered -- the points of the
           other cell receive what they would receive, no more than dg of the rest.
  q        one subtraction per term and a chain of four fmas, five roundings on no more than mq = |g_rgb| . |c - bg| + |g_depth|
           |t - far| + |g_opacity|; c is off by dv_c, t by u |t|:  dq = |g_rgb| . dv + |g_depth| u |t| + 5 u mq.
  w q      d(wq) = dw |q| + w dq + u |w q|  (the fma that sums it rounds on the sum: next line).
  suffix   S_k = Q - P_k with P the running fma sum and Q its last value: the terms up to k are the same bits in both, the later
           ones carry their own errors, every fma rounds on a partial sum and the subtraction once:
           dS_k = sum_{j > k} d(wq_j) + (n + 2) u sum_j |w_j q_j|.
  sigma    inner = fma(T', q, -S): dT' |q| + T' dq + dS + u |inner|; delta carries 5 u (three roundings under the root, the root,
           the product with step) and the product with it one: d = delta d(inner) + 6 u |delta inner|.
  colour   w g: dw |g| + u |w g|.  The clamp's mask is a step: a channel whose unclamped blend is within dv of 0 or of 1 may be
           masked on one side only, so its whole |w g| is added.
  element  a contribution wt X is off by dwt |X| + wt dX + 5 u |wt X|; the sum of an element's n contributions, in registers and in
           memory in whatever order they arrive, by n u sum |contribution|.
  Y_j      (degree > 0) baked_sh_ref's dY_j = N_j u m_j, and the product one rounding: |share| (N_j m_j + |Y_j|) u."""
from types import SimpleNamespace

import numpy as np

import baked_ref as br
import baked_sh_ref as sh

U = br.U


def _hat(x):
    return np.maximum(0.0, 1.0 - np.abs(x))


def march(grid, dcol, clamp, lo, hi, C, row, step, background, stop, gr, gd, go, gates, apart=False, omit_open=False):
    """The visited samples of one ray and what the upstream gradients make of them, or None for a miss or a ray whose upstream
    gradients are all zero.  Per visited sample: t, g, dg, v (clamped), dv, w, dw; n of them, delta, inv and the stop margin; and
    with n > 0 the docstring's q, suffix and sigma gates as inner, dinner, and a, da [n, 4]: a[c] = w g_rgb[c] on the open
    channels (else 0) with the gate `colour`, a[sigma] = delta inner with the gate `sigma`.  apart: baked_ref.blended's;
    omit_open: the mask is left out (baked_pose_ref plants it)."""
    lat = br.lattice(lo, hi, C, row, step)
    if lat is None or (not gr.any() and gd == 0 and go == 0):
        return None
    t, g, dg, inv = lat
    v, inside, dv = br.blended(grid, g, dg, C, dcol, gates, apart)
    raw = v[:, :3].copy()
    if clamp:
        v[:, :3] = np.clip(raw, 0.0, 1.0)
    delta, _, _, alpha, dalpha = br.alphas(v[:, 3], dv[:, 3], row[3:6], step)
    ks, w, dw, Tn, dTn, margin = br.visited(alpha, dalpha, inside, stop)
    n = ks.size
    m = SimpleNamespace(t=t[ks], g=g[ks], dg=dg[ks], v=v[ks], dv=dv[ks], w=w, dw=dw, n=n, delta=delta, inv=inv, margin=margin)
    if n == 0:
        return m
    c, rawk, far = m.v[:, :3], raw[ks], row[7]
    q = (c - background) @ gr + gd * (m.t - far) + go
    mq = np.abs(c - background) @ np.abs(gr) + abs(gd) * np.abs(m.t - far) + abs(go)
    dq = m.dv[:, :3] @ np.abs(gr) + abs(gd) * U * np.abs(m.t) + 5 * U * mq
    wq = w * q
    dwq = dw * np.abs(q) + w * dq + U * np.abs(wq)
    after = lambda z: np.concatenate([np.cumsum(z[::-1])[::-1][1:], [0.0]])  # sum over the later samples
    S, dS = after(wq), after(dwq) + (n + 2) * U * np.abs(wq).sum()
    m.inner = Tn * q - S
    m.dinner = dTn * np.abs(q) + Tn * dq + dS + U * np.abs(m.inner)
    m.a, m.da = np.zeros((n, 4)), np.zeros((n, 4))
    m.a[:, 3] = delta * m.inner
    m.da[:, 3] = delta * m.dinner + 6 * U * np.abs(m.a[:, 3])
    is_open = (rawk >= 0) & (rawk <= 1) if clamp and not omit_open else np.ones_like(rawk, bool)
    full = w[:, None] * gr
    m.a[:, :3] = np.where(is_open, full, 0.0)
    m.da[:, :3] = dw[:, None] * np.abs(gr) + U * np.abs(full)
    if clamp:
        edge = (np.abs(rawk) <= m.dv[:, :3]) | (np.abs(rawk - 1) <= m.dv[:, :3])
        m.da[:, :3] += np.where(edge, np.abs(full), 0.0)
    return m


def _ray(grid, dcol, clamp, lo, hi, C, row, step, background, stop, gr, gd, go, gates):
    """The contributions of one ray: (point index [m, 3] as (z, y, x), value [m, 4], error [m, 4], stop margin) or None."""
    m = march(grid, dcol, clamp, lo, hi, C, row, step, background, stop, gr, gd, go, gates)
    if m is None or m.n == 0:
        return None
    n, gk, dgk, X, dX, margin = m.n, m.g, m.dg, m.a, m.da, m.margin
    # the weights of the 4 x 4 x 4 points round each sample's cell, and what a moved sample changes of them
    i = np.minimum(np.floor(gk), C - 1)
    cand = i[:, :, None] + np.arange(-1, 3)  # [n, axis, 4]
    valid = (cand >= 0) & (cand <= C[None, :, None])
    h = _hat(gk[:, :, None] - cand)
    dh = np.zeros_like(h)
    if gates:
        for s in (-1.0, 1.0):
            moved = np.clip(gk + s * dgk, 0.0, C)
            dh = np.maximum(dh, np.abs(_hat(moved[:, :, None] - cand) - h))
    hx, hy, hz = h[:, 0], h[:, 1], h[:, 2]
    wt = hz[:, :, None, None] * hy[:, None, :, None] * hx[:, None, None, :]  # [n, z, y, x]
    dwt = dh[:, 2][:, :, None, None] * hy[:, None, :, None] * hx[:, None, None, :] + \
        hz[:, :, None, None] * dh[:, 1][:, None, :, None] * hx[:, None, None, :] + \
        hz[:, :, None, None] * hy[:, None, :, None] * dh[:, 0][:, None, None, :]
    ok = valid[:, 2][:, :, None, None] & valid[:, 1][:, None, :, None] & valid[:, 0][:, None, None, :] & ((wt > 0) | (dwt > 0))
    cz = np.broadcast_to(cand[:, 2][:, :, None, None], wt.shape)[ok].astype(np.int64)
    cy = np.broadcast_to(cand[:, 1][:, None, :, None], wt.shape)[ok].astype(np.int64)
    cx = np.broadcast_to(cand[:, 0][:, None, None, :], wt.shape)[ok].astype(np.int64)
    sample = np.broadcast_to(np.arange(n)[:, None, None, None], wt.shape)[ok]
    wt, dwt = wt[ok][:, None], dwt[ok][:, None]
    val = wt * X[sample]
    err = dwt * np.abs(X[sample]) + wt * dX[sample] + 5 * U * np.abs(val)
    return np.stack([cz, cy, cx], 1), val, err, margin


def points64(points, degree):
    """(k or None, sigma, rgbs or None) in fp64 of points as `grad` takes them, not rounded to fp32."""
    if degree == 0:
        grid = np.asarray(points, np.float64)
        return None, grid[..., 3], grid
    k, sigma = (np.asarray(z, np.float64) for z in points)
    return k, sigma, None


def upstream64(R, g_rgb, g_depth, g_opacity):
    return np.asarray(g_rgb, np.float64), *(np.zeros(R) if z is None else np.asarray(z, np.float64) for z in (g_depth, g_opacity))


def grad(points, degree, bounds, rays, step, background=0.0, stop=0.0, g_rgb=None, g_depth=None, g_opacity=None, gates=True):
    k, sigma, grid = points64(points, degree)
    lo, hi, C, rays, step, background, stop = br.args64(bounds, rays, sigma.shape, step, background, stop)
    R, shape, nb = rays.shape[0], sigma.shape, sh.NB.get(degree, 0)
    g_rgb, g_depth, g_opacity = upstream64(R, g_rgb, g_depth, g_opacity)
    live = sigma != 0
    out4, gate4, abs4 = (np.zeros(shape + (4,)) for _ in range(3))
    count = np.zeros(shape)
    if degree:
        outk, gatek, absk = (np.zeros(shape + (3, nb)) for _ in range(3))
    margin = np.inf
    for r in range(R):
        dcol = None
        if degree:
            d = rays[r, 3:6]
            if not np.isfinite(rays[r]).all() or not (d * d).sum() > 0:
                continue
            grid, dcol, Y, m = sh.ray_grid(k, sigma, d, degree, gates)
        res = _ray(grid, dcol, degree > 0, lo, hi, C, rays[r], step, background, stop, g_rgb[r], g_depth[r], g_opacity[r], gates)
        if res is None:
            continue
        idx, val, err, mg = res
        margin = min(margin, mg)
        keep = live[idx[:, 0], idx[:, 1], idx[:, 2]]
        idx, val, err = idx[keep], val[keep], err[keep]
        at = (idx[:, 0], idx[:, 1], idx[:, 2])
        np.add.at(out4, at, val)
        np.add.at(gate4, at, err)
        np.add.at(abs4, at, np.abs(val))
        np.add.at(count, at, 1.0)
        if degree:
            np.add.at(outk, at, val[:, :3, None] * Y)
            np.add.at(gatek, at, err[:, :3, None] * np.abs(Y) + np.abs(val[:, :3, None]) * ((sh.N_BASIS[:nb] * m + np.abs(Y)) * U))
            np.add.at(absk, at, np.abs(val[:, :3, None] * Y))
    gate4 += count[..., None] * U * abs4
    if degree == 0:
        return {"grad": out4, "gate": gate4, "count": count, "stop_margin": margin}
    gatek += count[..., None, None] * U * absk
    return {"grad_coef": outk, "gate_coef": gatek, "grad_sigma": out4[..., 3], "gate_sigma": gate4[..., 3], "count": count,
            "stop_margin": margin}


def render64(points, degree, bounds, rays, step, background=0.0, stop=0.0):
    """(rgb [R, 3], depth [R], opacity [R]) of fp64 parameters: baked_ref.render_ray on numbers that are NOT rounded to fp32
    first (a central difference needs the parameters as they are given)."""
    k, sigma, grid = points64(points, degree)
    lo, hi, C, rays, step, background, stop = br.args64(bounds, rays, sigma.shape, step, background, stop)
    R = rays.shape[0]
    rgb, depth, op = np.zeros((R, 3)), np.zeros(R), np.zeros(R)
    for r in range(R):
        dcol = None
        if degree:
            grid, dcol = sh.ray_grid(k, sigma, rays[r, 3:6], degree)[:2]
        rgb[r], depth[r], op[r] = br.render_ray(grid, lo, hi, C, rays[r], step, background, stop, dcol, clamp=degree > 0)[:3]
    return rgb, depth, op


def functional(points, degree, bounds, rays, step, background, stop, g_rgb, g_depth=None, g_opacity=None):
    rgb, depth, op = render64(points, degree, bounds, rays, step, background, stop)
    L = (np.asarray(g_rgb, np.float64) * rgb).sum()
    if g_depth is not None:
        L += (np.asarray(g_depth, np.float64) * depth).sum()
    if g_opacity is not None:
        L += (np.asarray(g_opacity, np.float64) * op).sum()
    return float(L)


def project(degree, rgbs=None, sigma=None):
    """upnerf_baked_project in numpy, dtype kept: a sigma that is finite and > 0 stays, every other becomes +0; degree 0: where
    sigma stays each colour becomes c > 0 ? (c < 1 ? c : 1) : 0, where it does not the point becomes (0, 0, 0, 0)."""
    with np.errstate(invalid="ignore"):
        if degree == 0:
            s = rgbs[..., 3]
            keep = np.isfinite(s) & (s > 0)
            c = rgbs[..., :3]
            c = np.where(c > 0, np.where(c < 1, c, 1), 0)
            out = np.zeros_like(rgbs)
            out[..., :3] = np.where(keep[..., None], c, 0)
            out[..., 3] = np.where(keep, s, 0)
            return out
        return np.where(np.isfinite(sigma) & (sigma > 0), sigma, 0).astype(sigma.dtype)


# ---- the upstream gradients and rays of the kernel tests ------------------------------------------------------------------------------

def upstream(R, seed=21, zero_rows=(9, 20, 40)):
    """(g_rgb [R, 3], g_depth [R], g_opacity [R]) fp32, seeded; the rows `zero_rows` are zero in all three."""
    rng = np.random.RandomState(seed)
    g = [rng.randn(R, 3).astype(np.float32), rng.randn(R).astype(np.float32), rng.randn(R).astype(np.float32)]
    for z in g:
        z[[r for r in zero_rows if r < R]] = 0
    return g


def extra_rays(rgbs, bounds=br.BOUNDS):
    """[65, 8]: 64 copies of one ray through the middle of the box (every lane of a wave adds to the same addresses), and one
    ray that runs inside a face of the cells (its y is a grid plane: f = 0 there, or 1 on the other side of a rounding)."""
    lo, hi = br.bounds64(bounds)
    mid, ext = (lo + hi) / 2, hi - lo
    d = np.array([0.55, 0.48, 0.68])
    one = list(mid - 1.1 * d) + list(d) + [0.05, 2.4]
    Ny = rgbs.shape[1]
    y = lo[1] + ext[1] * (Ny // 2) / (Ny - 1)
    face = [lo[0] - 0.2, y, mid[2] + 0.037 * ext[2], 1.0, 0.0, 0.0, 0.0, ext[0] + 0.4]
    return np.asarray([one] * 64 + [face], np.float32)


# ---- the tuning problem of the test that cannot pass without the feature ---------------------------------------------------------------

TUNE_LR, TUNE_ITERS, TUNE_BETAS, TUNE_EPS = 0.05, 15, (0.9, 0.999), 1e-8


def tuning_problem(degree, seed=31):
    """(A, B, level, rays, step): scene A is the blob grid (at degree 2 with gentle random coefficients), B is A with seeded
    perturbations of the kept colours (or coefficients) and sigmas; the rays are those of make_rays() that are valid; one cell a
    step.  A and B are fp32 arrays (degree 0: rgbs; degree 2: (coef, sigma))."""
    rgbs, level = br.blob_grid()
    rng = np.random.RandomState(seed + degree)
    kept = rgbs[..., 3] > 0
    rays = br.make_rays()
    rays = rays[np.isfinite(rays).all(1) & (rays[:, 7] > rays[:, 6])]
    step = float(np.float32(br.cell_size(rgbs)))
    sigma_b = np.where(kept, rgbs[..., 3] * np.exp(0.5 * rng.randn(*kept.shape)) + 1.0, 0).astype(np.float32)
    if degree == 0:
        B = rgbs.copy()
        B[..., :3] = np.where(kept[..., None], np.clip(rgbs[..., :3] + 0.3 * rng.randn(*rgbs[..., :3].shape), 0, 1), 0)
        B[..., 3] = sigma_b
        return rgbs, B.astype(np.float32), level, rays, step
    coef = sh.coefficients(kept.shape, degree, seed, mean=0.5, spread=0.15) * kept[..., None, None]
    coef = coef.astype(np.float16).astype(np.float32)  # (what a record stores)
    coef_b = ((coef + 0.5 * rng.randn(*coef.shape)) * kept[..., None, None]).astype(np.float16).astype(np.float32)
    return (coef, rgbs[..., 3].copy()), (coef_b, sigma_b), level, rays, step


def tune_loop(degree, iters=TUNE_ITERS, lr=TUNE_LR):
    """The loss curve L(0) .. L(iters) of the fp64 loop on the tuning problem: mean squared error of the colours against A's
    render, the restatement's gradient, torch.optim.Adam's update, the projection.  L(i) is the loss before update i."""
    A, B, level, rays, step = tuning_problem(degree)
    target = render64(A, degree, br.BOUNDS, rays, step)[0]
    P = [np.asarray(z, np.float64).copy() for z in ((B,) if degree == 0 else B)]
    m, v = [np.zeros_like(z) for z in P], [np.zeros_like(z) for z in P]
    b1, b2 = TUNE_BETAS
    curve = []
    for it in range(iters + 1):
        pts = P[0] if degree == 0 else tuple(P)
        diff = render64(pts, degree, br.BOUNDS, rays, step)[0] - target
        curve.append(float((diff * diff).mean()))
        if it == iters:
            break
        res = grad(pts, degree, br.BOUNDS, rays, step, g_rgb=diff * (2.0 / diff.size), gates=False)
        G = [res["grad"]] if degree == 0 else [res["grad_coef"], res["grad_sigma"]]
        t = it + 1
        for z, gz, mz, vz in zip(P, G, m, v):
            mz *= b1
            mz += (1 - b1) * gz
            vz *= b2
            vz += (1 - b2) * gz * gz
            z -= lr / (1 - b1 ** t) * mz / (np.sqrt(vz) / np.sqrt(1 - b2 ** t) + TUNE_EPS)
        if degree == 0:
            P[0] = project(0, rgbs=P[0])
        else:
            P[1] = project(degree, sigma=P[1])
            P[0] = P[0] * (P[1] != 0)[..., None, None]  # (a dropped point is a zero record)
    return curve
