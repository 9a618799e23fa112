"""fp64 numpy restatement of depth-map fusion (upnerf_tsdf_integrate, include/upnerf_hip.h), with a projection of its own, and
the small synthetic scene the tests of it share.  Nothing is imported from the module under test.

The rule, per point p (the fp32 grid point: the fp64 grid coordinate rounded once) and per view, in view order:
  1. pc = R^T (p - c), zc = -pc.z (the camera looks down -z); skip unless zc > 0
  2. u = fx pc.x / zc + cx, v = cy - fy pc.y / zc (pixel centres at integers)
  3. iu = floor(u + 0.5), jv = floor(v + 0.5); skip outside [0, W) x [0, H)
  4. d = depth[jv W + iu]; skip unless finite and > 0, and unless opacity >= min_opacity where the view has a map
  5. r = |p - c|, sdf = d - r; skip if sdf < -trunc
  6. val = min(1, sdf / trunc); w = 1 or the pixel's opacity; Wn = W + w; T += (val - T) w / Wn
  7. colour, where volume and view have one and sdf <= trunc: the same running mean with a weight C of its own
Everything is float64 except the two weights, which are accumulated in float32 in view order as the kernel does (sums of a few
fp32 values: both sides then hold the same bits and compare exactly); the ratio w / Wn is formed in float64 from them.

Worked by hand (test_tsdf_cpu.test_reference_reproduces_the_hand_worked_example).  One camera at c = (0, 0, 2) with R = I,
looking down -z at the origin; fx = fy = 2, cx = cy = 1, 3 x 3 pixels; trunc = 0.5; volume initialised to T = 1, W = 0,
colour 0.  Three points on the optical axis (every one projects to u = v = 1, pixel (1, 1)), r = 2 - z:
  view 1: depth 1.5 everywhere, colour (1, 0, 0.5);   view 2: depth 1.75 everywhere, colour (0, 1, 0.5).
  A = (0, 0, 0.5):   r = 1.5.   view 1: sdf = 0, val = 0, W = 1, T = 1 + (0 - 1) 1/1 = 0, colour (1, 0, 0.5), C = 1.
                                view 2: sdf = 0.25, val = 0.5, W = 2, T = 0 + 0.5 / 2 = 0.25, colour (0.5, 0.5, 0.5), C = 2.
  B = (0, 0, 1.25):  r = 0.75.  view 1: sdf = 0.75, val = min(1, 1.5) = 1, W = 1, T = 1; sdf > trunc: no colour.
                                view 2: sdf = 1, val = 1, W = 2, T = 1; no colour: C = 0, colour stays (0, 0, 0).
  C = (0, 0, -0.25): r = 2.25.  view 1: sdf = -0.75 < -trunc: skipped.
                                view 2: sdf = -0.5, not below -trunc: val = -1, W = 1, T = 1 + (-1 - 1) 1/1 = -1,
                                        colour (0, 1, 0.5), C = 1."""
import numpy as np

# what became of a point in a view
BEHIND, OUTSIDE, NO_DEPTH, LOW_OPACITY, BEHIND_BAND, UPDATED = range(6)


def axis_coords(lo, hi, n):
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return lo + np.arange(n, dtype=np.float64) * ((hi - lo) / (n - 1))


def grid_points(bounds, res):
    """[Nz * Ny * Nx, 3] float64 values of the fp32 grid points, x fastest."""
    cx, cy, cz = (axis_coords(bounds[0][k], bounds[1][k], n).astype(np.float32).astype(np.float64) for k, n in enumerate(res))
    Z, Y, X = np.meshgrid(cz, cy, cx, indexing="ij")
    return np.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], 1)


def make_view(c2w, fx, fy, cx, cy, W, H, depth, opacity=None, rgb=None):
    f32 = lambda a, shape: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))
    return dict(c2w=np.asarray(c2w, np.float32).reshape(3, 4), fx=float(np.float32(fx)), fy=float(np.float32(fy)),
                cx=float(np.float32(cx)), cy=float(np.float32(cy)), W=int(W), H=int(H), depth=f32(depth, H * W),
                opacity=f32(opacity, H * W), rgb=f32(rgb, (H * W, 3)))


def new_state(n, colour=True, tsdf0=1.0, rgb0=0.0):
    return dict(tsdf=np.full(n, tsdf0, np.float64), weight=np.zeros(n, np.float32),
                rgb=np.full((n, 3), rgb0, np.float64) if colour else None, rgb_weight=np.zeros(n, np.float32) if colour else None)


def integrate_points(P, state, views, trunc, min_opacity=0.5, weight_mode="count"):
    """Folds `views` into `state` (new_state) at the points P [n, 3] float64, in place.  Returns per view a dict of what
    happened: `branch` [n] (the constants above), `sdf` [n] (NaN where step 5 was not reached), `near_pixel_edge` [n] (u + 0.5
    or v + 0.5 within 1e-4 of an integer), `near_band_edge` [n] (sdf within 1e-5 of -trunc), `coloured` [n]."""
    trunc = float(np.float32(trunc))
    min_opacity = float(np.float32(min_opacity))
    n = P.shape[0]
    report = []
    for vw in views:
        M = vw["c2w"].astype(np.float64)
        R, c = M[:, :3], M[:, 3]
        dlt = P - c
        pc = dlt @ R  # row i: R^T (p_i - c)
        zc = -pc[:, 2]
        branch = np.full(n, BEHIND)
        front = zc > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            u = vw["fx"] * pc[:, 0] / zc + vw["cx"]
            v = vw["cy"] - vw["fy"] * pc[:, 1] / zc
        fu, fv = np.floor(u + 0.5), np.floor(v + 0.5)
        with np.errstate(invalid="ignore"):
            inside = front & (fu >= 0) & (fu < vw["W"]) & (fv >= 0) & (fv < vw["H"])
            edge = front & ((np.abs(u + 0.5 - np.round(u + 0.5)) < 1e-4) | (np.abs(v + 0.5 - np.round(v + 0.5)) < 1e-4))
        branch[front] = OUTSIDE
        pix = np.where(inside, fv * vw["W"] + fu, 0).astype(np.int64)
        d = vw["depth"][pix].astype(np.float64)
        with np.errstate(invalid="ignore"):
            has_d = inside & np.isfinite(d) & (d > 0)
        branch[inside] = NO_DEPTH
        ok = has_d
        w = np.ones(n, np.float32)
        if vw["opacity"] is not None:
            op = vw["opacity"][pix]
            with np.errstate(invalid="ignore"):
                ok = has_d & (op.astype(np.float64) >= min_opacity)
            branch[has_d] = LOW_OPACITY
            if weight_mode == "opacity":
                w = op.copy()
        elif weight_mode == "opacity":
            raise ValueError("weight_mode 'opacity' needs the opacity map of every view")
        with np.errstate(invalid="ignore"):
            ok = ok & (w > 0) & np.isfinite(w)
        r = np.sqrt((dlt ** 2).sum(1))
        sdf = np.where(ok, d - r, np.nan)
        with np.errstate(invalid="ignore"):
            upd = ok & (sdf >= -trunc)
            band_edge = ok & (np.abs(sdf + trunc) < 1e-5)
        branch[ok] = BEHIND_BAND
        branch[upd] = UPDATED
        val = np.minimum(1.0, sdf / trunc)
        w = np.where(upd, w, np.float32(0)).astype(np.float32)
        Wn = (state["weight"] + w).astype(np.float32)
        i = np.nonzero(upd)[0]
        state["tsdf"][i] += (val[i] - state["tsdf"][i]) * (w[i].astype(np.float64) / Wn[i].astype(np.float64))
        state["weight"] = Wn
        coloured = np.zeros(n, bool)
        if state["rgb"] is not None and vw["rgb"] is not None:
            with np.errstate(invalid="ignore"):
                coloured = upd & (sdf <= trunc)
            wc = np.where(coloured, w, np.float32(0)).astype(np.float32)
            Cn = (state["rgb_weight"] + wc).astype(np.float32)
            j = np.nonzero(coloured)[0]
            q = (wc[j].astype(np.float64) / Cn[j].astype(np.float64))[:, None]
            state["rgb"][j] += (vw["rgb"][pix[j]].astype(np.float64) - state["rgb"][j]) * q
            state["rgb_weight"] = Cn
        report.append(dict(branch=branch, sdf=sdf, near_pixel_edge=edge, near_band_edge=band_edge, coloured=coloured))
    return report


# ---- the scene the GPU tests share: a sphere seen by three cameras ---------------------------------------------------------------

RES = (24, 20, 17)                               # Nx, Ny, Nz: 8160 voxels, no multiple of the 256-thread block, all axes differ
BOUNDS = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
TRUNC = 0.25
IMG_WH = (40, 30)
FX = FY = 26.0
CX, CY = 19.5, 14.5
RADIUS, DISTANCE = 0.8, 2.5


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


ROTATIONS = [_rot("y", 10) @ _rot("x", -7) @ _rot("z", 3), _rot("y", 70) @ _rot("x", -20) @ _rot("z", -5),
             _rot("x", -55) @ _rot("y", -30) @ _rot("z", 8)]


def camera(R):
    """[3, 4] fp32 pose at DISTANCE from the origin, looking at it: the camera looks down -z, so c = DISTANCE * R[:, 2]."""
    return np.concatenate([R, DISTANCE * R[:, 2:3]], 1).astype(np.float32)


def sphere_depth(c2w, wh=IMG_WH, intr=(FX, FY, CX, CY), radius=RADIUS):
    """[H * W] fp32: the fp64 distance along the unit ray through every pixel centre (no half-pixel shift) to the sphere round
    the origin, from the fp32 pose; NaN where the ray misses."""
    W, H = wh
    fx, fy, cx, cy = intr
    M = np.asarray(c2w, np.float32).astype(np.float64)
    R, o = M[:, :3], M[:, 3]
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([(i - cx) / fx, -(j - cy) / fy, -np.ones_like(i)], -1).reshape(-1, 3)
    dirs = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    d = dirs @ R.T
    b = d @ o
    disc = b * b - (o @ o - radius * radius)
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    return np.where(disc > 0, t, np.nan).astype(np.float32)


_SCENE = {}


def scene():
    """The three views (depth, a random colour and a random opacity in [0.3, 1) per pixel), built once and never changed."""
    if not _SCENE:
        rng = np.random.default_rng(7)
        views = []
        for R in ROTATIONS:
            c2w = camera(R)
            n = IMG_WH[0] * IMG_WH[1]
            views.append(make_view(c2w, FX, FY, CX, CY, IMG_WH[0], IMG_WH[1], sphere_depth(c2w),
                                   opacity=0.3 + 0.7 * rng.random(n, dtype=np.float32), rgb=rng.random((n, 3), dtype=np.float32)))
        _SCENE["views"] = views
        _SCENE["points"] = grid_points(BOUNDS, RES)
    return _SCENE["views"], _SCENE["points"]


def without(view, *names):
    """The view with the named maps (opacity, rgb) removed."""
    return {k: (None if k in names else v) for k, v in view.items()}
