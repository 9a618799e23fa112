"""fp64 numpy restatement of the baked marcher's gradient with respect to its rays (include/upnerf_hip.h: upnerf_baked_ray_bwd;
upnerf_amd/baked_pose.py): brute force over every lattice sample, the occupancy bits never consulted.  It builds
on tests/baked_ref.py, tests/baked_sh_ref.py and tests/baked_tune_ref.py, whose definitions, grids, rays and gates (dg, dv,
dalpha, dT, dw, dq, the suffix, `inner` and a, all through baked_tune_ref.march) it calls and does not state again.
Shared by tests/test_baked_pose_cpu.py and tests/test_hip_baked_pose.py.

    ray_grad(points, degree, bounds, rays, step, background, stop, g_rgb, g_depth, g_opacity, gates=True, omit=()) -> dict
        points as baked_tune_ref.grad takes them; "grad", "gate" [R, 8] (o | d | near | far), "stop_margin"
        omit: names among OMISSIONS, each a term of the definition left out on purpose (the tests plant them)
    pose_rays(se3, c2w, dirs) -> (rays o | d [n, 6], their Jacobian [n, 6, 6]) in fp64 (oracle/upnerf_oracle.py, autograd)
    pose_loop(...) -> the fp64 localisation loop

The definition.  The visited samples, w, T', q, the suffix S and inner = T' q - S are baked_tune_ref's.  With a[c] = w g_rgb[c] on
the open channels (else 0), a[sigma] = delta inner, the corners c_0..7 of the sample's cell (colours reduced with the ray's Y at
degree > 0) and lerp_y(a, b) = a + fy (b - a):
    s_x = lerp_z(lerp_y(c1 - c0, c3 - c2), lerp_y(c5 - c4, c7 - c6)), s_y and s_z alike;  G_k[a] = inv[a] sum_ch a[ch] s_a[ch]
    d_o = sum_k G_k;  d_near = sum_k (d . G_k + g_depth w_k);  d_far = g_depth (1 - opacity)
    d_d = sum_k t_k G_k + E step d / len + sum_j Z_j dY_j/dd,   E = sum_k sigma_k inner_k,   Z_j = sum_k sum_c a[c] m_k[c][j],
    m_k the trilinear blend of the stored coefficients, dY/dd = (dY/du)(I - u u^T) / len.
The visited set and every sample's cell are held fixed.  Eight zeros for a miss, len == 0, or upstream gradients that are all zero.

The gates (u = 2^-24), first order, every constant a count of roundings.
  a        baked_tune_ref's dX: the colours dw |g| + u |w g| (+ the whole |w g| where the unclamped blend is within dv of 0 or 1:
           the mask is a step), sigma delta d(inner) + 6 u |delta inner|.
  slope    a difference of corners (1) and two lerps, each a difference and a fma (4): 5 u on no more than 2 max |corner|, and at
           degree > 0 twice the corners' own dcol.  The MOVED-SAMPLE term: a slope along x is bilinear in (fy, fz) inside a cell
           and JUMPS at a cell face, so it is evaluated, not bounded: the slopes at g +- dg e_a per axis, each located by its own
           floor (the 4 x 4 x 4 points round the cell cover every cell such a sample can fall in), the largest change per axis,
           the three added.
  S_k      sum over four channels of da |s| + |a| ds, and four fmas: 4 u sum |a s|.
  sums     So: sum dS_k + n u M, M = sum_k sum_ch |a s|.  St: t carries u |t|: sum (|t| dS_k + u |t| M_k) + n u sum |t| M_k.
           inv carries one rounding and the product one: 2 u.
  E        sum (dv_sigma |inner| + |sigma| d(inner)) + (n + 1) u sum |sigma inner|; the product with step (1), u_a = d_a / len
           (baked_sh_ref: 5), the fma (1).
  Z_j      per sample and channel |m| da + |a| dm, dm the moved-sample change of the blended coefficient, evaluated as above;
           wt carries baked_tune_ref's 5 u, its product with a one, and each of the 24 n fmas rounds on a partial sum:
           (6 + 24 n) u sum |a| blend(|k|).
  dY/du    a component of u (5) times constants and at most one more component: 8 u |dY_j/du_a| (with the magnitudes of the terms).
  gu, u.gu nb and 3 fmas; the projection's fma, the division, len's 5.
  near     |g_depth| dO + sum_a |d_a| d(d_o[a]) + 4 u (|g_depth O| + sum |d_a d_o[a]|), dO baked_ref's sum dw + n u O.
  far      |g_depth| (dO + 2 u (1 + O))."""
import numpy as np

import baked_ref as br
import baked_sh_ref as sh
import baked_tune_ref as tr

U = br.U
OMISSIONS = ("delta", "near", "dY", "open")


def _cell(g, C):
    i = np.minimum(np.floor(g), C - 1).astype(np.int64)
    return i, g - i


def slopes(grid, g, C):
    """[n, 3, ch]: d blend / d g_a of grid [Nz, Ny, Nx, ch] at grid coordinates g [n, 3] (inside the box), in the cell of each."""
    i, f = _cell(g, C)
    x, y, z = i[:, 0], i[:, 1], i[:, 2]
    fx, fy, fz = f[:, 0:1], f[:, 1:2], f[:, 2:3]
    c = [grid[z + (j >> 2), y + (j >> 1 & 1), x + (j & 1)] for j in range(8)]
    lerp = lambda f_, a, b: a + f_ * (b - a)
    sx = lerp(fz, lerp(fy, c[1] - c[0], c[3] - c[2]), lerp(fy, c[5] - c[4], c[7] - c[6]))
    sy = lerp(fz, lerp(fx, c[2] - c[0], c[3] - c[1]), lerp(fx, c[6] - c[4], c[7] - c[5]))
    sz = lerp(fy, lerp(fx, c[4] - c[0], c[5] - c[1]), lerp(fx, c[6] - c[2], c[7] - c[3]))
    return np.stack([sx, sy, sz], 1)


def dbasis(unit, degree):
    """(dY/du [nb, 3], the magnitudes of its terms [nb, 3]) of sh.basis at a unit vector, the basis taken as the polynomial it
    is written as."""
    x, y, z = unit
    c1, c2, c3, c4 = sh.Y1, sh.Y2, sh.Y3, sh.Y4
    D = np.array([[0, 0, 0], [0, -c1, 0], [0, 0, c1], [-c1, 0, 0], [c2 * y, c2 * x, 0], [0, -c2 * z, -c2 * y],
                  [-2 * c3 * x, -2 * c3 * y, 4 * c3 * z], [-c2 * z, 0, -c2 * x], [2 * c4 * x, -2 * c4 * y, 0]], np.float64)
    return D[:sh.NB[degree]], np.abs(D[:sh.NB[degree]])


def _ray(grid, dcol, coef, clamp, lo, hi, C, row, step, background, stop, gr, gd, go, gates, omit, degree=0):
    """(grad [8], gate [8], stop margin) of one ray, or None for a row of zeros."""
    d = row[3:6]
    m = tr.march(grid, dcol, clamp, lo, hi, C, row, step, background, stop, gr, gd, go, gates, apart=True, omit_open="open" in omit)
    if m is None or not (d * d).sum() > 0:
        return None
    grad, gate = np.zeros(8), np.zeros(8)
    n, w, dw, tk, gk, dgk, dvk, inv, margin = m.n, m.w, m.dw, m.t, m.g, m.dg, m.dv, m.inv, m.margin
    O, dO = w.sum(), dw.sum() + n * U * w.sum()
    grad[7] = gd * (1.0 - O)
    gate[7] = abs(gd) * (dO + 2 * U * (1.0 + O))
    if n == 0:
        return grad, gate, margin
    a, da, inner, dinner, length = m.a, m.da, m.inner, m.dinner, np.sqrt((d * d).sum())
    # the slopes and S_k
    s = slopes(grid, gk, C)  # [n, 3, 4]
    ds = np.zeros_like(s)
    if gates:
        ck = br.trilinear(grid, gk, C)[2]
        ds = 5 * U * 2 * ck[:, None, :] + br.moved(lambda x: slopes(grid, x, C), gk, dgk, C)
        if dcol is not None:
            ds = ds + 2 * br.trilinear(dcol, gk, C)[2][:, None, :]
    Sk = (a[:, None, :] * s).sum(2)  # [n, 3]
    Mk = (np.abs(a)[:, None, :] * np.abs(s)).sum(2)
    dSk = (da[:, None, :] * np.abs(s) + np.abs(a)[:, None, :] * ds).sum(2) + 4 * U * Mk
    So, dSo = Sk.sum(0), dSk.sum(0) + n * U * Mk.sum(0)
    tabs = np.abs(tk)[:, None]
    St, dSt = (tk[:, None] * Sk).sum(0), (tabs * dSk + U * tabs * Mk).sum(0) + n * U * (tabs * Mk).sum(0)
    d_o, dd_o = inv * So, inv * dSo + 2 * U * inv * Mk.sum(0)
    grad[:3], gate[:3] = d_o, dd_o
    unit = d / length
    part = [inv * St]
    err = inv * dSt + 2 * U * inv * (tabs * Mk).sum(0)
    if "delta" not in omit:
        sig = m.v[:, 3]
        E = (sig * inner).sum()
        dE = (dvk[:, 3] * np.abs(inner) + np.abs(sig) * dinner).sum() + (n + 1) * U * np.abs(sig * inner).sum()
        part.append(E * step * unit)
        err = err + step * np.abs(unit) * dE + 7 * U * np.abs(E * step * unit)
    if degree > 0 and "dY" not in omit:
        nb = sh.NB[degree]
        flat = coef.reshape(coef.shape[:3] + (3 * nb,))
        blend = lambda x: br.trilinear(flat, x, C)[0]
        m = blend(gk).reshape(n, 3, nb)
        mabs = br.trilinear(np.abs(flat), gk, C)[0].reshape(n, 3, nb)
        dm = br.moved(blend, gk, dgk, C).reshape(n, 3, nb) if gates else np.zeros_like(m)
        Z = (a[:, :3, None] * m).sum((0, 1))
        dZ = (da[:, :3, None] * np.abs(m) + np.abs(a[:, :3, None]) * dm).sum((0, 1)) + (6 + 24 * n) * U * (np.abs(a[:, :3, None]) * mabs).sum((0, 1))
        D, Dabs = dbasis(unit, degree)
        gu = Z @ D
        dgu = dZ @ Dabs + np.abs(Z) @ (8 * U * Dabs) + nb * U * (np.abs(Z) @ Dabs)
        along = unit @ gu
        dalong = np.abs(unit) @ dgu + 8 * U * (np.abs(unit) @ np.abs(gu))
        mag = (np.abs(gu) + np.abs(unit * along)) / length
        part.append((gu - unit * along) / length)
        err = err + (dgu + np.abs(unit) * dalong + 6 * U * np.abs(unit * along) + U * np.abs(gu)) / length + 6 * U * mag
    grad[3:6] = sum(part)
    gate[3:6] = err + len(part) * U * sum(np.abs(z) for z in part)
    if "near" not in omit:
        grad[6] = gd * O + d @ d_o
        gate[6] = abs(gd) * dO + np.abs(d) @ dd_o + 4 * U * (abs(gd * O) + np.abs(d) @ np.abs(d_o))
    return grad, gate, margin


def ray_grad(points, degree, bounds, rays, step, background=0.0, stop=0.0, g_rgb=None, g_depth=None, g_opacity=None, gates=True, omit=()):
    assert all(x in OMISSIONS for x in omit)
    coef, sigma, grid = tr.points64(points, degree)
    lo, hi, C, rays, step, background, stop = br.args64(bounds, rays, sigma.shape, step, background, stop)
    R = rays.shape[0]
    g_rgb, g_depth, g_opacity = tr.upstream64(R, g_rgb, g_depth, g_opacity)
    out = {"grad": np.zeros((R, 8)), "gate": np.zeros((R, 8)), "stop_margin": np.inf}
    for r in range(R):
        dcol = None
        if degree:
            d = rays[r, 3:6]
            if not np.isfinite(rays[r]).all() or not (d * d).sum() > 0:
                continue
            grid, dcol = sh.ray_grid(coef, sigma, d, degree, gates)[:2]
        res = _ray(grid, dcol, coef, degree > 0, lo, hi, C, rays[r], step, background, stop, g_rgb[r], g_depth[r], g_opacity[r], gates,
                   omit, degree)
        if res is not None:
            out["grad"][r], out["gate"][r] = res[0], res[1]
            out["stop_margin"] = min(out["stop_margin"], res[2])
    return out


# ---- the chain to se(3) and the localisation loop ----------------------------------------------------------------------------------

def pose_rays(se3, c2w, dirs):
    """(o | d [n, 6], J [n, 6 (o | d), 6 (se3)]) in fp64: get_rays(dirs, compose(se3_exp(se3), c2w)) of oracle/upnerf_oracle.py and
    its Jacobian by autograd, per row."""
    import torch
    import upnerf_oracle as orc
    se3 = torch.tensor(np.asarray(se3, np.float64), requires_grad=True)
    c2w, dirs = torch.tensor(np.asarray(c2w, np.float64)), torch.tensor(np.asarray(dirs, np.float64))
    o, d = orc.get_rays(dirs, orc.compose_pair(orc.se3_exp(se3), c2w))
    od = torch.cat([o, d], 1)
    J = torch.stack([torch.autograd.grad(od[:, i].sum(), se3, retain_graph=True)[0] for i in range(6)], 1)
    return od.detach().numpy(), J.numpy()


def pixel_dirs(x, y, K):
    fx, fy, cx, cy = K
    return np.stack([(x - cx) / fx, -(y - cy) / fy, -np.ones_like(x, dtype=np.float64)], 1)


def image_rays(c2w, K, wh, near_far):
    """fp32-representable rays [H W, 8] of a camera: the pose kernel's convention (unit d, integer pixel grid, row-major)."""
    W, H = wh
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = pixel_dirs(x.ravel(), y.ravel(), K)
    od, _ = pose_rays(np.zeros((H * W, 6)), np.broadcast_to(c2w, (H * W, 3, 4)), dirs)
    return np.concatenate([od, np.broadcast_to(np.asarray(near_far, np.float64), (H * W, 2))], 1)


def pose_error(poses, truth):
    """(largest rotation angle in radians, largest translation distance) between [N, 3, 4] poses."""
    rot, tra = 0.0, 0.0
    for P, Q in zip(np.asarray(poses, np.float64), np.asarray(truth, np.float64)):
        cosang = (np.trace(P[:, :3] @ Q[:, :3].T) - 1) / 2
        rot = max(rot, float(np.arccos(np.clip(cosang, -1, 1))))
        tra = max(tra, float(np.linalg.norm(P[:, 3] - Q[:, 3])))
    return rot, tra


def refined(se3, c2w):
    """[N, 3, 4] fp64: compose(se3_exp(se3), c2w)."""
    import torch
    import upnerf_oracle as orc
    return orc.compose_pair(orc.se3_exp(torch.tensor(np.asarray(se3, np.float64))), torch.tensor(np.asarray(c2w, np.float64))).numpy()


# the localisation problem of the test that cannot pass without the feature: two cameras 1.6 above and beside the blob grid, 24 x 16
# pixels each; every pose starts with a roll of LOC_ROT radians about its optical axis and LOC_TRA along it (opposite signs on the
# two cameras) -- the two motions so small a picture determines well; a pan is told from a sideways step only by parallax
LOC_K, LOC_WH, LOC_NEAR_FAR = (24.0, 24.0, 11.5, 7.5), (24, 16), (0.3, 3.0)
LOC_ROT, LOC_TRA, LOC_LR, LOC_ITERS, LOC_BATCH, LOC_SEED = 0.05, 0.05, 0.004, 40, 64, 0


def localisation_problem(degree):
    """(A, truth [2, 3, 4], init [2, 3, 4], step): scene A of baked_tune_ref.tuning_problem, the true poses and the perturbed
    ones, as fp32 numbers; one cell a step."""
    A = tr.tuning_problem(degree)[0]
    lo, hi = br.bounds64(br.BOUNDS)
    mid = (lo + hi) / 2
    down = np.concatenate([np.eye(3), (mid + [0.0, 0.0, 1.6])[:, None]], 1)
    side = np.concatenate([np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]]), (mid + [0.0, 1.6, 0.0])[:, None]], 1)
    truth = np.stack([down, side]).astype(np.float32).astype(np.float64)
    off = np.zeros((2, 6))
    off[:, 2], off[:, 5] = [LOC_ROT, -LOC_ROT], [-LOC_TRA, LOC_TRA]
    init = refined(off, truth).astype(np.float32).astype(np.float64)
    return A, truth, init, float(np.float32(br.cell_size(br.blob_grid()[0])))


def pose_loop(points, degree, bounds, targets, K, c2w_init, near_far, step, iters, lr, batches, betas=(0.9, 0.999), eps=1e-8):
    """The fp64 localisation loop: targets [N, H, W, 3], batches a list of `iters` index arrays into [N][H][W].  Per iteration the
    rays of the batch under the poses as they are, baked_tune_ref.render64, the mean squared error, this file's ray gradient,
    the pose-ray Jacobian, torch.optim.Adam's update on se3 [N, 6].  Returns (se3, the loss curve L(0) .. L(iters - 1), each
    before its update)."""
    targets = np.asarray(targets, np.float64)
    N, H, W = targets.shape[:3]
    flat = targets.reshape(-1, 3)
    nf = np.broadcast_to(np.asarray(near_far, np.float64), (N, 2))
    se3, m, v = np.zeros((N, 6)), np.zeros((N, 6)), np.zeros((N, 6))
    b1, b2 = betas
    curve = []
    for it in range(iters):
        idx = np.asarray(batches[it])
        img, pix = idx // (H * W), idx % (H * W)
        dirs = pixel_dirs((pix % W).astype(np.float64), (pix // W).astype(np.float64), K)
        od, J = pose_rays(se3[img], np.asarray(c2w_init, np.float64)[img], dirs)
        rays = np.concatenate([od, nf[img]], 1)
        diff = tr.render64(points, degree, bounds, rays, step)[0] - flat[idx]
        curve.append(float((diff * diff).mean()))
        g_rays = ray_grad(points, degree, bounds, rays, step, g_rgb=diff * (2.0 / diff.size), gates=False)["grad"]
        G = np.zeros((N, 6))
        np.add.at(G, img, np.einsum("ni,nij->nj", g_rays[:, :6], J))
        t = it + 1
        m = b1 * m + (1 - b1) * G
        v = b2 * v + (1 - b2) * G * G
        se3 = se3 - lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    return se3, curve
