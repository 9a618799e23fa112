"""fp64 numpy restatement of the environment of a baked scene (include/upnerf_hip.h: "what lies outside the box"; csrc/env.hip;
upnerf_amd/baked_env.py): the cube-map lookup, the composite behind a march, its backward and the node rays, with
derived first-order gates.  Shared by tests/test_env_cpu.py and tests/test_hip_env.py.

    node_dirs(E) -> [6, E+1, E+1, 3]          the node directions, the fp32 numbers of the definition
    owners(E) -> [6 (E+1)^2]                  the flat index of each node's copy on the lowest face (itself for an unshared node)
    cell(d, E) -> dict                        face, axes, u, v, g, cell and position of directions [n, 3] (dead rows flagged)
    lookup(env, d) -> dict                    "rgb", "su", "sv" [n, 3] and the cell's entries
    composite(env, rays, opacity, rgb_in) -> {"rgb", "gate"}
    composite_bwd(env, rays, opacity, g_out) -> {"g_opacity", "gate_opacity", "g_rays", "gate_rays", "near_line"}
    node_rays(E, bounds, far) -> {"rays" [n, 8], "gate_near" [n]}
    families(E, seed) -> {name: directions [n, 3] fp32}, each also scaled by 1e-6 and 1e6 by `scaled`
    sky_problem(), sky_loop(...)              the localisation against the sky alone, in fp64

The definition is the header's.  Face selection compares the fp32 inputs themselves, so the restatement and the kernel always
choose the same face; within the face g = (u + 1) E / 2 carries roundings and may fall into the neighbouring cell.

The gates (u = 2^-24), first order, every constant a count of roundings.
  u, v     one division: u |u|, and half a denormal step where the quotient is denormal.
  g        the addition (1) and the product (1): dg = (E / 2) (du + u |u + 1|) + u g.  f = g - i is exact.
  value    x0 = fma(fu, n10 - n00, n00): the difference (1) and the fma (1): dx0 = u (fu |n10 - n00| + |x0|); x1 alike;
           V = fma(fv, x1 - x0, x0): dV = fv (dx0 + dx1 + u |x1 - x0|) + dx0 + u |V|.
           The MOVED term: V is continuous and piecewise bilinear in g, and a rounding can carry g over a node line, so the change is
           evaluated, not bounded: |V(g +- dg e_a) - V(g)| per axis, each located by its own floor, the larger sign, the two added.
  composite rest = 1 - opacity (1), the fma (1): |rest| (dV + moved) + u |rest V| + u |out|.
  g_opacity three products and two fma roundings on partial sums: sum |g| dV' + 3 u sum |g e|, dV' = dV + moved.
  slopes   su = fma(fv, B - A, A), A = n10 - n00, B = n11 - n01: dsu = fv u (|A| + |B| + |B - A|) + u |A| + u |su|;
           sv = x1 - x0: dsv = dx0 + dx1 + u |sv|; both with their own moved term (they JUMP at a node line: see near_line).
  a        rest (1) and the product (1): 2 u |a|.   G = three fmas: sum (da |s| + |a| ds) + 3 u sum |a s|.
  p        the product with E / 2 (1).   g_d[a] = p_u / |d_m| (1).   g_d[m] = -fma(u, p_u, v p_v) / d_m: the product (1), the fma (1),
           the division (1), and du, dv on p.
  near     hi - o (1) and the division (1): 2 u near.
near_line flags the directions whose g lies within its own dg of a node line, or that have a tie |d_a| = |d_b| for the largest
magnitude: face and cell are held fixed there and the slopes jump; tests may leave them out of the g_rays comparison."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149


# ---- the map's geometry -------------------------------------------------------------------------------------------------------------

def axes(face):
    m = face >> 1
    return m, (1 if m == 0 else 0), (1 if m == 2 else 2)


def node_dirs(E):
    """[6, E+1, E+1, 3] float32, indexed [face][iv][iu]."""
    out = np.zeros((6, E + 1, E + 1, 3), np.float32)
    line = (2 * np.arange(E + 1, dtype=np.float32) - np.float32(E)) / np.float32(E)
    for face in range(6):
        m, a, b = axes(face)
        out[face, :, :, m] = -1.0 if face & 1 else 1.0
        out[face, :, :, a] = line[None, :]
        out[face, :, :, b] = line[:, None]
    return out


def owners(E):
    """The flat index of the lowest-face copy of every node, by the nodes' directions themselves (bit for bit)."""
    d = node_dirs(E).reshape(-1, 3)
    first = {}
    out = np.empty(len(d), np.int64)
    for i, row in enumerate(d):
        key = (row + np.float32(0.0)).tobytes()  # (-0.0 does not occur: 2 iu - E is an integer, 0 gives +0)
        out[i] = first.setdefault(key, i)
    return out


def edge_mask(E):
    """[6, E+1, E+1] bool: the nodes on the border of their face."""
    m = np.zeros((E + 1, E + 1), bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return np.broadcast_to(m, (6, E + 1, E + 1)).copy()


# ---- lookup -------------------------------------------------------------------------------------------------------------------------

def cell(d, E):
    d = np.asarray(d, np.float64)
    n = len(d)
    dead = ~np.isfinite(d).all(1) | ~d.any(1)
    safe = np.where(dead[:, None], np.array([1.0, 0.0, 0.0]), d)
    mag = np.abs(safe)
    m = np.zeros(n, np.int64)
    m = np.where(mag[:, 1] > mag[np.arange(n), m], 1, m)
    m = np.where(mag[:, 2] > mag[np.arange(n), m], 2, m)
    a, b = np.where(m == 0, 1, 0), np.where(m == 2, 1, 2)
    rows = np.arange(n)
    dm = safe[rows, m]
    am = np.abs(dm)
    u, v = safe[rows, a] / am, safe[rows, b] / am
    half = E / 2
    gu, gv = (u + 1) * half, (v + 1) * half
    srt = np.sort(mag, 1)
    out = dict(dead=dead, m=m, a=a, b=b, dm=dm, am=am, face=2 * m + (dm < 0), u=u, v=v, gu=gu, gv=gv, tie=srt[:, 2] == srt[:, 1])
    # u carries one rounding (half a denormal step where it is denormal), g the addition and the product
    du, dv = U * np.abs(u) + TINY, U * np.abs(v) + TINY
    out.update(du=du, dv=dv, dgu=half * (du + U * np.abs(u + 1)) + U * gu, dgv=half * (dv + U * np.abs(v + 1)) + U * gv)
    return out


def _blend(env, face, gu, gv):
    """(V, su, sv, parts) of the bilinear blend at g in its own cell; env [6, E+1, E+1, >= 3] fp64."""
    E = env.shape[1] - 1
    iu = np.minimum(np.floor(gu), E - 1).astype(np.int64)
    iv = np.minimum(np.floor(gv), E - 1).astype(np.int64)
    fu, fv = (gu - iu)[:, None], (gv - iv)[:, None]
    n00, n10 = env[face, iv, iu, :3], env[face, iv, iu + 1, :3]
    n01, n11 = env[face, iv + 1, iu, :3], env[face, iv + 1, iu + 1, :3]
    x0, x1 = n00 + fu * (n10 - n00), n01 + fu * (n11 - n01)
    V = x0 + fv * (x1 - x0)
    A, B = n10 - n00, n11 - n01
    su = A + fv * (B - A)
    sv = x1 - x0
    dx0, dx1 = U * (fu * np.abs(A) + np.abs(x0)), U * (fu * np.abs(B) + np.abs(x1))
    dV = fv * (dx0 + dx1 + U * np.abs(sv)) + dx0 + U * np.abs(V)
    dsu = fv * U * (np.abs(A) + np.abs(B) + np.abs(B - A)) + U * np.abs(A) + U * np.abs(su)
    dsv = dx0 + dx1 + U * np.abs(sv)
    return V, su, sv, dV, dsu, dsv, iu, iv


def _moved(fn, gu, gv, dgu, dgv, E):
    """The sum over the two axes of the largest |fn(g +- dg e_a) - fn(g)|."""
    base, total = fn(gu, gv), 0.0
    for du_, dv_ in ((dgu, 0.0), (0.0, dgv)):
        worst = 0.0
        for s in (-1.0, 1.0):
            worst = np.maximum(worst, np.abs(fn(np.clip(gu + s * du_, 0.0, E), np.clip(gv + s * dv_, 0.0, E)) - base))
        total = total + worst
    return total


def lookup(env, d):
    env = np.asarray(env, np.float64)
    E = env.shape[1] - 1
    c = cell(d, E)
    live = ~c["dead"][:, None]
    V, su, sv, dV, dsu, dsv, iu, iv = _blend(env, c["face"], c["gu"], c["gv"])
    pick = lambda k: (lambda gu, gv: _blend(env, c["face"], gu, gv)[k])
    mV, msu, msv = (_moved(pick(k), c["gu"], c["gv"], c["dgu"], c["dgv"], E) for k in range(3))
    line = lambda g, dg: (np.abs(g - np.round(g)) <= dg) & (np.round(g) > 0) & (np.round(g) < E)
    c.update(rgb=V * live, su=su * live, sv=sv * live, d_rgb=(dV + mV) * live, d_su=(dsu + msu) * live, d_sv=(dsv + msv) * live,
             iu=iu, iv=iv, near_line=c["tie"] | line(c["gu"], c["dgu"]) | line(c["gv"], c["dgv"]), E=E)
    return c


def composite(env, rays, opacity, rgb_in):
    rays, opacity, rgb_in = (np.asarray(x, np.float64) for x in (rays, opacity, rgb_in))
    L = lookup(env, rays[:, 3:6])
    rest = (1.0 - opacity)[:, None]
    out = rgb_in + rest * L["rgb"]
    gate = np.abs(rest) * L["d_rgb"] + U * np.abs(rest * L["rgb"]) + U * np.abs(out)
    return dict(rgb=out, gate=gate, env=L["rgb"], look=L)


def composite_bwd(env, rays, opacity, g_out):
    rays, opacity, g = (np.asarray(x, np.float64) for x in (rays, opacity, g_out))
    L = lookup(env, rays[:, 3:6])
    n, E = len(rays), L["E"]
    live = ~L["dead"]
    e = L["rgb"]
    g_opacity = -(g * e).sum(1) * live
    gate_opacity = ((np.abs(g) * L["d_rgb"]).sum(1) + 3 * U * np.abs(g * e).sum(1)) * live
    rest = (1.0 - opacity)[:, None]
    a = rest * g
    da = 2 * U * np.abs(a)
    half = E / 2
    G, dG = {}, {}
    for k, dk in (("su", "d_su"), ("sv", "d_sv")):
        G[k] = (a * L[k]).sum(1)
        dG[k] = (da * np.abs(L[k]) + np.abs(a) * L[dk]).sum(1) + 3 * U * np.abs(a * L[k]).sum(1)
    pu, pv = G["su"] * half, G["sv"] * half
    dpu, dpv = half * dG["su"] + U * np.abs(pu), half * dG["sv"] + U * np.abs(pv)
    am, dm, u, v = L["am"], L["dm"], L["u"], L["v"]
    ga, gb = pu / am, pv / am
    inner = u * pu + v * pv
    gm = -inner / dm
    d_inner = np.abs(u) * dpu + L["du"] * np.abs(pu) + np.abs(v) * dpv + L["dv"] * np.abs(pv) + 2 * U * (np.abs(u * pu) + np.abs(v * pv))
    grad, gate = np.zeros((n, 8)), np.zeros((n, 8))
    rows = np.arange(n)
    grad[rows, 3 + L["a"]], gate[rows, 3 + L["a"]] = ga, dpu / am + U * np.abs(ga)
    grad[rows, 3 + L["b"]], gate[rows, 3 + L["b"]] = gb, dpv / am + U * np.abs(gb)
    grad[rows, 3 + L["m"]], gate[rows, 3 + L["m"]] = gm, d_inner / am + U * np.abs(gm)
    grad, gate = grad * live[:, None], gate * live[:, None]
    return dict(g_opacity=g_opacity, gate_opacity=gate_opacity, g_rays=grad, gate_rays=gate, near_line=L["near_line"], dead=L["dead"])


# ---- node rays ------------------------------------------------------------------------------------------------------------------------

def node_rays(E, bounds, far):
    """The rows of every node, n = (face (E+1) + iv) (E+1) + iu: o and d the fp32 numbers of the definition (fp64 operations, each
    rounded on its own, rounded to fp32 once), near the exact slab exit of those in fp64 with its gate."""
    lo, hi = (np.asarray(b, np.float32).astype(np.float64) for b in bounds)
    x = node_dirs(E).reshape(-1, 3).astype(np.float64)
    length = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
    d = (x / length[:, None]).astype(np.float32).astype(np.float64)
    o = np.broadcast_to(((lo + hi) / 2.0).astype(np.float32).astype(np.float64), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d != 0, (np.where(d > 0, hi, lo) - o) / d, np.inf)
    near = t.min(1)
    rays = np.concatenate([o, d, near[:, None], np.full((len(d), 1), float(np.float32(far)))], 1)
    return dict(rays=rays, gate_near=2 * U * np.abs(near))


# ---- maps and direction families -------------------------------------------------------------------------------------------------------

def smooth_map(E, seed=0):
    """A map [6, E+1, E+1, 4] fp32 that is a smooth function of the node direction (so its shared copies agree by construction)."""
    rng = np.random.default_rng(seed)
    M, c = rng.normal(size=(3, 3)), rng.uniform(0.3, 0.7, 3)
    x = node_dirs(E).astype(np.float64)
    x = x / np.linalg.norm(x, axis=-1, keepdims=True)
    rgb = c + 0.25 * np.sin(2.0 * (x @ M.T)) + 0.1 * x[..., ::-1]
    return np.concatenate([rgb, np.zeros_like(rgb[..., :1])], -1).astype(np.float32)


def random_map(E, seed=0):
    """Random node colours in [-1, 2], the copies of shared nodes made equal (the owner's)."""
    rng = np.random.default_rng(seed)
    env = np.concatenate([rng.uniform(-1, 2, (6, E + 1, E + 1, 3)), np.zeros((6, E + 1, E + 1, 1))], -1).astype(np.float32)
    return env.reshape(-1, 4)[owners(E)].reshape(env.shape).copy()


def _ulp_steps(x, k):
    return (x.view(np.int32) + (np.where(x >= 0, 1, -1) * k).astype(np.int32)).view(np.float32)


def families(E, seed=0, n=256):
    """{name: [k, 3] fp32} -- the direction families of the tests.  "edge" families sit on ties or node lines (value-only for the
    slopes), the others are generic."""
    rng = np.random.default_rng(seed)
    out = {}
    out["random"] = rng.normal(size=(n, 3)).astype(np.float32)
    out["axes"] = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    s = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float32)
    ties = []
    for i, j in ((0, 1), (0, 2), (1, 2)):
        k = 3 - i - j
        for t in (0.0, 0.37, -0.81, 0.999):
            e = np.ones((8, 3), np.float32)
            e[:, k] = t
            ties.append(e * s)
    out["ties"] = np.concatenate(ties + [s * np.float32(0.731)])
    z = []
    for i in range(3):
        e = rng.normal(size=(4, 3)).astype(np.float32)
        e[:, i] = 0
        z.append(e)
        e2 = np.zeros((2, 3), np.float32)
        e2[:, (i + 1) % 3] = [0.5, -2.0]
        z.append(e2)
    out["zeros"] = np.concatenate(z)
    den = rng.normal(size=(12, 3)).astype(np.float32)
    den[np.arange(12), np.arange(12) % 3] = np.array([1e-40, -3e-42, 1.4e-45, -1e-39] * 3, np.float32)
    out["denormal"] = den
    # one ulp either side of every node line of every face, in u and in v
    line = (2 * np.arange(E + 1, dtype=np.float32) - np.float32(E)) / np.float32(E)
    rows = []
    for face in range(6):
        m, a, b = axes(face)
        for val in line:
            for k in (-1, 0, 1):
                w = np.float32(val) if k == 0 else _ulp_steps(np.array([val], np.float32), k)[0]
                if abs(w) > 1 or (val == 0 and k != 0):
                    w = np.float32(val) if val != 0 else np.float32(k * 1.4e-45)
                for other in (np.float32(0.3141), np.float32(-0.77)):
                    for ax, ot in ((a, b), (b, a)):
                        e = np.zeros(3, np.float32)
                        e[m] = -1.0 if face & 1 else 1.0
                        e[ax], e[ot] = w, other
                        rows.append(e * np.float32(2.0))
    out["lines"] = np.asarray(rows, np.float32)
    out["dead"] = np.array([[np.nan, 1, 0], [1, np.inf, 0], [0, 0, -np.inf], [0, 0, 0], [-0.0, 0.0, -0.0], [np.nan] * 3], np.float32)
    return out


EDGE_FAMILIES = ("axes", "ties", "lines", "dead")  # on ties or node lines by construction


def value_only(name, E):
    """Whether family `name` sits on node lines or ties at size E, so that only values (and g_opacity) are compared, not g_rays:
    the edge families, and at an even E the directions with a zero or denormal component (u = 0 is the node line g = E / 2
    then, and a denormal u rounds on to it)."""
    return name in EDGE_FAMILIES or (name in ("zeros", "denormal") and E % 2 == 0)
SCALES = (1.0, 1e-6, 1e6)
LEFT_OUT_CAP = 0.02


def scaled(dirs):
    """Each direction as it is, scaled by 1e-6 and by 1e6 (fp32)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.concatenate([(dirs * np.float32(s)).astype(np.float32) for s in SCALES])


def problem(E, name, dirs, seed=0):
    """(rays [n, 8], opacity [n], rgb_in [n, 3], g_out [n, 3]) fp32 of a family's scaled directions."""
    d = scaled(dirs)
    rng = np.random.default_rng(seed + 7)
    n = len(d)
    rays = np.concatenate([rng.normal(size=(n, 3)), d, np.full((n, 1), 0.5), np.full((n, 1), 4.0)], 1).astype(np.float32)
    opacity = rng.uniform(0, 1, n).astype(np.float32)
    opacity[::5] = 0.0
    opacity[1::7] = 1.0
    return rays, opacity, rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)


# ---- localising against the sky alone ---------------------------------------------------------------------------------------------------
# An empty box shows only the environment: rgb = env(d).  One 16 x 12 camera at the box centre looking down -z; its pose starts with
# a rotation of SKY_ROT radians about each of two axes.  Only rotation can be recovered (the map has no parallax): the translation
# columns of se3 receive no gradient and stay zero.
SKY_E, SKY_WH, SKY_K, SKY_NEAR_FAR = 8, (16, 12), (10.0, 10.0, 7.5, 5.5), (0.1, 2.0)
SKY_ROT, SKY_LR, SKY_ITERS, SKY_BATCH, SKY_SEED = 0.04, 0.004, 30, 96, 0


def sky_problem():
    """(env fp32, truth [1, 3, 4], init [1, 3, 4]) as fp32 numbers."""
    import baked_pose_ref as pr
    truth = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None].astype(np.float32).astype(np.float64)
    off = np.zeros((1, 6))
    off[0, :3] = [SKY_ROT, -SKY_ROT, 0.0]
    return smooth_map(SKY_E, seed=3), truth, pr.refined(off, truth).astype(np.float32).astype(np.float64)


def sky_loop(env, targets, c2w_init, iters, lr, batches, betas=(0.9, 0.999), eps=1e-8):
    """The fp64 localisation loop of baked_pose_ref.pose_loop with the empty box's render, rgb = env(d): (se3 [1, 6], the loss
    curve, each loss before its update)."""
    import baked_pose_ref as pr
    targets = np.asarray(targets, np.float64)
    N, H, W = targets.shape[:3]
    flat = targets.reshape(-1, 3)
    se3, m, v = np.zeros((N, 6)), np.zeros((N, 6)), np.zeros((N, 6))
    b1, b2 = betas
    curve = []
    for it in range(iters):
        idx = np.asarray(batches[it])
        img, pix = idx // (H * W), idx % (H * W)
        dirs = pr.pixel_dirs((pix % W).astype(np.float64), (pix // W).astype(np.float64), SKY_K)
        od, J = pr.pose_rays(se3[img], np.asarray(c2w_init, np.float64)[img], dirs)
        rays = np.concatenate([od, np.broadcast_to(np.asarray(SKY_NEAR_FAR, np.float64), (len(idx), 2))], 1)
        zero = np.zeros(len(idx))
        diff = composite(env, rays, zero, np.zeros((len(idx), 3)))["rgb"] - flat[idx]
        curve.append(float((diff * diff).mean()))
        g_rays = composite_bwd(env, rays, zero, diff * (2.0 / diff.size))["g_rays"]
        G = np.zeros((N, 6))
        np.add.at(G, img, np.einsum("ni,nij->nj", g_rays[:, :6], J))
        t = it + 1
        m = b1 * m + (1 - b1) * G
        v = b2 * v + (1 - b2) * G * G
        se3 = se3 - lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    return se3, curve
