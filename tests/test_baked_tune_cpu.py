"""The gradient of a baked scene's render, without a GPU: the fp64 restatement (tests/baked_tune_ref.py) against central differences
of its own render and against closed forms, the fp64 tuning loop the GPU test is measured by, and the refusals of the two new
entry points, which are decided on the host (include/upnerf_hip.h)."""
import ctypes

import numpy as np
import pytest

import baked_ref as br
import baked_sh_ref as sh
import baked_tune_ref as tr

EINVAL, EUNSUP = -1, -2


def _subset():
    """20 of make_rays()'s rays that hit the blob, and an upstream gradient for them."""
    rgbs, _ = br.blob_grid()
    rays = br.make_rays()
    step = float(np.float32(br.cell_size(rgbs) / 2))
    ref = br.render(rgbs, br.BOUNDS, rays, step)
    rays = rays[np.nonzero(ref["n"] > 0)[0][:20]]
    assert rays.shape[0] == 20
    return rgbs, rays, step, tr.upstream(20, zero_rows=(3,))


@pytest.mark.parametrize("degree", [0, 2])
def test_the_gradient_is_the_central_difference_of_the_render(degree):
    """Along seeded random directions in parameter space (over the points that are parameters: sigma != 0), with stop = 0.  The
    render is smooth there except at the colour clamp: at degree 2 the corners' colours are held a margin inside [0, 1] -- a
    blend is a convex combination of them and of the zeros of dropped corners, so it cannot cross 0 or 1 either.

    The tolerance is stated, not picked: a central difference with step h is off by h^2 / 6 times the third derivative along the
    direction, and by the rounding of the two fp64 renders, 2^-53 / h times the magnitude of what they sum.  Along a direction with
    entries in [-1, 1] a ray's optical depth moves by no more than D = delta n (n samples) and its colours by no more than 1 (by
    sum_j |Y_j| at degree 2) per unit, so the third derivative of a ray's term is bounded by (D^3 + 3 D^2 + 3 D) G with G the
    magnitude of the ray's upstream gradient against its outputs; the rounding term takes n + 8 operations per sample."""
    rgbs, rays, step, (g_rgb, g_depth, g_op) = _subset()
    kept = rgbs[..., 3] > 0
    if degree == 0:
        P = [rgbs.astype(np.float64)]
        masks = [np.broadcast_to(kept[..., None], rgbs.shape)]
        pts = lambda Q: Q[0]
        amp = 1.0
    else:
        coef = sh.coefficients(kept.shape, degree, 5, mean=0.5, spread=0.04).astype(np.float64) * kept[..., None, None]
        P = [coef, rgbs[..., 3].astype(np.float64)]
        masks = [np.broadcast_to(kept[..., None, None], coef.shape), kept]
        pts = lambda Q: (Q[0], Q[1])
        dirs = rays[:, 3:6] / np.linalg.norm(rays[:, 3:6], axis=1, keepdims=True)
        Y = sh.basis(dirs, degree)
        col = np.einsum("...cj,rj->r...c", coef, Y)[:, kept]
        amp = float(np.abs(Y).sum(1).max())
        assert col.min() > 0.1 and col.max() < 0.9, (col.min(), col.max())  # the margin: h amp is far below it
    res = tr.grad(pts(P), degree, br.BOUNDS, rays, step, 0.3, 0.0, g_rgb, g_depth, g_op, gates=False)
    G = [res["grad"]] if degree == 0 else [res["grad_coef"], res["grad_sigma"]]
    for g, mk in zip(G, masks):
        assert float(np.abs(g[~mk]).max(initial=0.0)) == 0.0 and float(np.abs(g[mk]).max()) > 0
    # the scales of the tolerance
    n = np.array([br.n_samples(r[6], r[7], step) for r in rays], np.float64)
    D = step * np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1) * n
    far = np.abs(rays[:, 7].astype(np.float64))
    Gmag = np.abs(g_rgb).sum(1) * (1 + 0.3) * amp + np.abs(g_depth) * far + np.abs(g_op)
    third = float(((D ** 3 + 3 * D ** 2 + 3 * D) * Gmag).sum())
    summed = float(((n + 8) * n * Gmag).sum())
    h = 1e-4
    tol = h * h / 6 * third + 2.0 ** -53 / h * summed
    rng = np.random.RandomState(8)
    worst = 0.0
    for _ in range(4):
        dirn = [rng.uniform(-1, 1, z.shape) * mk for z, mk in zip(P, masks)]
        plus = tr.functional(pts([z + h * dz for z, dz in zip(P, dirn)]), degree, br.BOUNDS, rays, step, 0.3, 0.0, g_rgb, g_depth, g_op)
        minus = tr.functional(pts([z - h * dz for z, dz in zip(P, dirn)]), degree, br.BOUNDS, rays, step, 0.3, 0.0, g_rgb, g_depth, g_op)
        fd = (plus - minus) / (2 * h)
        an = sum(float((g * dz).sum()) for g, dz in zip(G, dirn))
        worst = max(worst, abs(fd - an) / tol)
        assert abs(an) > 1e-2  # a derivative of some size: the comparison looks at something
        assert abs(fd - an) <= tol, (degree, fd, an, tol)
    print(f"degree {degree}: h = {h}, tolerance {tol:.3e} (truncation {h * h / 6 * third:.3e}, rounding {2.0 ** -53 / h * summed:.3e}), "
          f"worst |fd - analytic| / tolerance {worst:.3f}")


UNIFORM = ((0.0, 0.0, 0.0), (2.0, 2.0, 2.0))


def _uniform(sigma=1.5, colour=(0.2, 0.5, 0.7)):
    g = np.zeros((3, 3, 3, 4))
    g[..., :3] = colour
    g[..., 3] = sigma
    return g


def test_one_sample_in_a_uniform_cell_has_its_closed_form():
    """One ray along x through cell (0, 0, 0) of a 2 x 2 x 2-cell grid of constant (c, sigma), one sample at x = 0.25 of the cell:
    alpha = 1 - exp(-delta sigma), w = alpha; dL/dc = w g_rgb, dL/dsigma = delta (1 - alpha) q with
    q = g_rgb . (c - bg) + g_depth (t - far) + g_opacity; corner (x, y, z) gets (x ? 0.25 : 0.75)(y ? 0.5 : 0.5)(z ? 0.75 : 0.25)."""
    grid = _uniform()
    step, bg = 0.5, 0.25
    rays = np.array([[0.0, 0.5, 0.75, 1.0, 0.0, 0.0, 0.0, 0.5]], np.float32)  # one sample, t = 0.25
    g_rgb, g_depth, g_op = np.array([[0.3, -1.1, 0.6]]), np.array([0.8]), np.array([-0.4])
    res = tr.grad(grid, 0, UNIFORM, rays, step, bg, 0.0, g_rgb, g_depth, g_op)
    alpha = 1 - np.exp(-0.5 * 1.5)
    q = g_rgb[0] @ (np.array([0.2, 0.5, 0.7]) - bg) + 0.8 * (0.25 - 0.5) - 0.4
    four = np.concatenate([alpha * g_rgb[0], [0.5 * (1 - alpha) * q]])
    want = np.zeros((3, 3, 3, 4))
    for z in (0, 1):
        for y in (0, 1):
            for x in (0, 1):
                want[z, y, x] = (0.25 if x else 0.75) * 0.5 * (0.75 if z else 0.25) * four
    assert np.abs(res["grad"] - want).max() <= 1e-15
    assert (res["gate"] >= 0).all() and res["gate"][want != 0].min() > 0 and res["gate"].max() < 1e-5
    assert res["count"].sum() == 8


def test_zero_upstream_dead_corners_and_the_clamp():
    rgbs, rays, step, (g_rgb, g_depth, g_op) = _subset()
    # a ray whose upstream gradient is zero adds nothing: alone it gives a zero gradient, among others it changes nothing
    z3, z1 = np.zeros((1, 3)), np.zeros(1)
    alone = tr.grad(rgbs, 0, br.BOUNDS, rays[:1], step, 0.0, 0.0, z3, z1, z1)
    assert float(np.abs(alone["grad"]).max()) == 0.0 and alone["count"].sum() == 0
    assert not g_rgb[3].any() and g_depth[3] == 0 and g_op[3] == 0
    full = tr.grad(rgbs, 0, br.BOUNDS, rays, step, 0.0, 0.0, g_rgb, g_depth, g_op, gates=False)["grad"]
    less = tr.grad(rgbs, 0, br.BOUNDS, np.delete(rays, 3, 0), step, 0.0, 0.0, *(np.delete(g, 3, 0) for g in (g_rgb, g_depth, g_op)), gates=False)["grad"]
    assert np.array_equal(full, less)
    # a corner with sigma 0 receives nothing, though its weight is not zero and its neighbours receive something
    dead = rgbs[..., 3] == 0
    assert dead.any() and float(np.abs(full[dead]).max()) == 0.0 and float(np.abs(full[~dead]).max()) > 0
    grid = _uniform()
    grid[0, 0, 0] = 0
    one = np.array([[0.0, 0.5, 0.75, 1.0, 0.0, 0.0, 0.0, 0.5]], np.float32)
    g = tr.grad(grid, 0, UNIFORM, one, 0.5, 0.0, 0.0, np.ones((1, 3)), None, None)["grad"]
    assert float(np.abs(g[0, 0, 0]).max()) == 0.0 and float(np.abs(g[0, 0, 1]).min()) > 0
    # the clamp masks the colour gradient: a constant expansion of 1.5 / Y0 in red, 0.5 / Y0 in green, -0.2 / Y0 in blue
    k = np.zeros((3, 3, 3, 3, 4))
    k[..., 0, 0], k[..., 1, 0], k[..., 2, 0] = 1.5 / sh.Y0, 0.5 / sh.Y0, -0.2 / sh.Y0
    sigma = np.full((3, 3, 3), 1.5)
    res = tr.grad((k, sigma), 1, UNIFORM, one, 0.5, 0.0, 0.0, np.ones((1, 3)), None, None)
    gc = res["grad_coef"][0, 0, 1]
    assert float(np.abs(gc[0]).max()) == 0.0 and float(np.abs(gc[2]).max()) == 0.0 and gc[1, 0] > 0
    alpha = 1 - np.exp(-0.75)
    assert abs(gc[1, 0] - 0.25 * 0.5 * 0.25 * alpha * sh.Y0) <= 1e-15
    # sigma still sees the CLAMPED colours: q = 1 + 0.5 + 0
    assert abs(res["grad_sigma"][0, 0, 1] - 0.25 * 0.5 * 0.25 * 0.5 * (1 - alpha) * 1.5) <= 1e-15


@pytest.mark.parametrize("degree", [0, 2])
def test_the_fp64_tuning_loop_halves_the_loss(degree):
    """rho_ref = L(k) / L(0) <= 0.5 for the fp64 loop: the condition tests/test_hip_baked_tune.py measures the GPU's loop by."""
    curve = tr.tune_loop(degree)
    rho = curve[-1] / curve[0]
    print(f"degree {degree}: L(0) = {curve[0]:.4e}, L({tr.TUNE_ITERS}) = {curve[-1]:.4e}, rho_ref = {rho:.3f}")
    assert curve[0] > 1e-4 and np.isfinite(curve).all()
    assert rho <= 0.5


def test_project_in_numpy_is_what_the_header_says():
    p = np.array([[0.5, -0.1, 1.5, 2.0], [0.5, 0.5, 0.5, -1.0], [np.nan, np.inf, -np.inf, 1.0], [0.3, 0.3, 0.3, np.nan],
                  [0.3, 0.3, 0.3, np.inf], [0.3, 0.3, 0.3, -0.0]], np.float32)
    out = tr.project(0, rgbs=p)
    want = np.array([[0.5, 0, 1, 2.0], [0, 0, 0, 0], [0, 1, 0, 1.0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.float32)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), want.view(np.uint32))  # (-0 becomes +0)
    s = tr.project(2, sigma=p[:, 3].copy())
    assert np.array_equal(s.view(np.uint32), np.array([2, 0, 1, 0, 0, 0], np.float32).view(np.uint32))


# ---- host refusals (the pattern of test_abi_cpu.py: every pointer non-null and never dereferenced) -------------------------------------

def _bwd_args(**kw):
    from upnerf_amd import _lib
    one = ctypes.c_void_p(64)
    a = _lib.BakedRenderBwdArgs(Cx=8, Cy=9, Cz=10, R=67, lo=(ctypes.c_float * 3)(-0.7, -0.5, -0.6), hi=(ctypes.c_float * 3)(0.8, 0.6, 0.9),
                                step=0.1, background=0.0, stop=0.0, degree=0, points=one, words=one, rays=one, slots=None, g_rgb=one,
                                g_depth=None, g_opacity=None, grad=one, grad_coef=one, grad_sigma=one)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BWD_REFUSALS = [
    (dict(g_rgb=None), EINVAL), (dict(degree=3), EINVAL), (dict(degree=-1), EINVAL), (dict(step=0.0), EINVAL), (dict(step=-0.1), EINVAL),
    (dict(step=float("nan")), EINVAL), (dict(step=float("inf")), EINVAL), (dict(points=None), EINVAL), (dict(words=None), EINVAL),
    (dict(rays=None), EINVAL), (dict(rays=ctypes.c_void_p(72)), EINVAL), (dict(R=0), EINVAL), (dict(Cx=0), EINVAL),
    (dict(background=float("nan")), EINVAL), (dict(stop=1.0), EINVAL), (dict(stop=-0.5), EINVAL),
    (dict(hi=(ctypes.c_float * 3)(0.8, -0.5, 0.9)), EINVAL),
    (dict(points=ctypes.c_void_p(72)), EINVAL),                               # degree 0: a point is 16 bytes
    (dict(degree=1, points=ctypes.c_void_p(80)), EINVAL),                     # a record is aligned to its 32 bytes
    (dict(degree=2, points=ctypes.c_void_p(96)), EINVAL),                     # ... or to its 64
    (dict(grad=None), EINVAL), (dict(degree=1, grad_coef=None), EINVAL), (dict(degree=2, grad_sigma=None), EINVAL),
    (dict(slots=ctypes.c_void_p(64)), EUNSUP), (dict(degree=2, slots=ctypes.c_void_p(64)), EUNSUP),  # a brick pool
]


@pytest.mark.parametrize("case,want", BWD_REFUSALS)
def test_render_bwd_refuses_before_launch(case, want):
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_baked_render_bwd(ctypes.byref(_bwd_args(**case)), None) == want


def test_render_bwd_and_project_refuse_null_and_the_rest():
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_baked_render_bwd(None, None) == EINVAL
    assert _lib.lib.upnerf_baked_project(None, None) == EINVAL
    one = ctypes.c_void_p(64)
    P = _lib.BakedProjectArgs
    for a in (P(n=0, degree=0, rgbs=one), P(n=4, degree=3, rgbs=one, sigma=one), P(n=4, degree=0, rgbs=None, sigma=one),
              P(n=4, degree=0, rgbs=ctypes.c_void_p(68)), P(n=4, degree=1, rgbs=one, sigma=None), P(n=4, degree=-1, rgbs=one, sigma=one)):
        assert _lib.lib.upnerf_baked_project(ctypes.byref(a), None) == EINVAL


def test_the_sparse_refusal_says_what_to_do_instead():
    """The Python layer refuses a sparse scene before anything is built, with the route in the text."""
    from upnerf_amd import baked_tune
    from upnerf_amd.baked import BakedScene
    scene = BakedScene.__new__(BakedScene)
    scene.pool = object()  # (what makes a scene sparse; nothing else of it is looked at)
    for make in (lambda: baked_tune.BakedTuner(scene, 1e-2), lambda: baked_tune.SceneParams.of(scene), lambda: scene.tune(1e-2),
                 lambda: baked_tune.distill(None, scene, [0, 1], 1, 1, 0.1)):
        with pytest.raises(ValueError) as e:
            make()
        assert "densify()" in str(e.value) and "sparsify()" in str(e.value) and "once per brick" in str(e.value)
    assert "densify()" in baked_tune.SPARSE_REFUSAL and "sparsify()" in baked_tune.SPARSE_REFUSAL
