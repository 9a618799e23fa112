"""Tuning a sparse baked scene on its pool, on the GPU (csrc/baked.hip: upnerf_baked_sparse_render_bwd; csrc/brick.hip:
upnerf_brick_face_sum; upnerf_amd/baked_sparse_tune.py).

The face sum is held to the numpy restatement tests/baked_sparse_tune_ref.py bit for bit.  The gradient is held to
tests/baked_tune_ref.py -- fp64, brute force over every lattice sample of the DENSE grid, no bits, no bricks -- with its gradient
and its gate gathered to the pool (baked_sparse_ref.gather).  The gate is not widened: baked_sparse_tune_ref's docstring counts
the roundings (n - m inside the m copies, m - 1 merges: the n - 1 of any bracketing).  The sums over rays are float atomics, so two
runs are held to the gate and not to each other.

The grid with shared points: blob_grid(shape=(12, 17, 10)), 9 x 16 x 11 cells, 2 x 2 x 2 bricks, all eight occupied, ragged in x
and z and exact in y; grid point (8, 8, 8) is held by all eight.  The blob grid of the dense tests (1 x 2 x 2 bricks) is the
second.  Rays, upstream gradients, steps and settings are those of tests/test_hip_baked_tune.py.  Worst measured error / gate on an
MI355X: 0.293 at the cell step, 0.202 at the tenth."""
import numpy as np
import pytest
import torch

import baked_cases as cases
import baked_ref as br
import baked_sh_ref as sh
import baked_sparse_ref as sr
import baked_sparse_tune_ref as ft
import baked_tune_ref as tr
from test_hip_baked_sparse import CELLS, pattern
from baked_cases import dev
from test_hip_baked_tune import SETTINGS, within

pytestmark = pytest.mark.gpu

_CACHE = {}
GRIDS = {"big": lambda: br.blob_grid(shape=(12, 17, 10)), "blob": br.blob_grid}


def cells_of(rgbs):
    return tuple(n - 1 for n in rgbs.shape[2::-1])


def numbers(name, degree):
    """The numbers the reference differentiates: rgbs, or (k, sigma) as the records store them; and the level."""
    key = ("numbers", name, degree)
    if key not in _CACHE:
        rgbs, level = GRIDS[name]()
        if degree == 0:
            _CACHE[key] = (rgbs, None, level)
        else:
            records = sh.pack(sh.coefficients(rgbs[..., 3].shape, degree, 11 + degree), rgbs[..., 3], level, degree)[0]
            _CACHE[key] = (sh.unpack(records, degree), records, level)
    return _CACHE[key]


def scene_of(name, degree):
    """The sparse scene of a grid (the dense scene's sparsify())."""
    pts, records, level = numbers(name, degree)
    return cases.scene_of((__name__, name, degree), lambda: cases.build(pts if degree == 0 else records, level, degree), sparse=True)


def rays_of(name):
    return cases.rays_all(GRIDS[name]()[0])


def to_pool(ref, degree, bricks):
    """A reference of baked_tune_ref with every grid array gathered to the pool: the expectation and its gate per COPY."""
    g = lambda a: sr.gather(a.reshape(a.shape[:3] + (-1,)), bricks)
    if degree == 0:
        return {"grad": g(ref["grad"]), "gate": g(ref["gate"]), "count": g(ref["count"])[..., 0]}
    nb = sh.NB[degree]
    five = lambda a: g(a).reshape(len(bricks), 9, 9, 9, 3, nb)
    return {"grad_coef": five(ref["grad_coef"]), "gate_coef": five(ref["gate_coef"]), "grad_sigma": g(ref["grad_sigma"])[..., 0],
            "gate_sigma": g(ref["gate_sigma"])[..., 0], "count": g(ref["count"])[..., 0]}


def reference(name, step, degree, setting, rows=None, seed=21):
    """(the fp64 restatement on the dense grid, the same gathered to the pool): computed once per case and never changed."""
    key = ("ref", name, step, degree, setting, rows, seed)
    if key not in _CACHE:
        bg, stop, rest = SETTINGS[setting]
        rays = rays_of(name) if rows is None else special_rays(name)
        g_rgb, g_depth, g_op = tr.upstream(rays.shape[0], seed=seed, zero_rows=(9, 20, 40) if rows is None else ())
        dt = sh.steps(GRIDS[name]()[0])[step]
        pts = numbers(name, degree)[0]
        ref = tr.grad(pts, degree, br.BOUNDS, rays, dt, bg, stop, g_rgb, g_depth if rest else None, g_op if rest else None)
        _CACHE[key] = (ref, to_pool(ref, degree, scene_of(name, degree).bricks.cpu().numpy()))
    return _CACHE[key]


def launch(name, step, degree, setting, rows=slice(None), out=None, params=None, face_sum=True, special=False):
    """upnerf_baked_sparse_render_bwd (and the face sum) on the rays `rows`: the pool-shaped gradient."""
    from upnerf_amd import baked_sparse_tune as st
    bg, stop, rest = SETTINGS[setting]
    scene = scene_of(name, degree)
    params = params or st.PoolParams.of(scene, requires_grad=False)
    rays = special_rays(name) if special else rays_of(name)
    g_rgb, g_depth, g_op = (dev(g[rows]) for g in tr.upstream(rays.shape[0], zero_rows=() if special else (9, 20, 40)))
    dt = sh.steps(GRIDS[name]()[0])[step]
    got = st.backward(scene.pool, params, dev(rays[rows]), dt, bg, stop, g_rgb, g_depth if rest else None, g_op if rest else None,
                      out=out, face_sum=face_sum)
    torch.cuda.synchronize()
    return got


def groups_of(name, degree=0):
    key = ("groups", name)
    if key not in _CACHE:
        _CACHE[key] = ft.copy_groups(scene_of(name, degree).slots.cpu().numpy(), cells_of(GRIDS[name]()[0]))
    return _CACHE[key]


# ---- 1. the face sum ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 4, 27])
# fully occupied; one brick; a seeded third of the cells (which occupies every brick); whole bricks missing between occupied ones
@pytest.mark.parametrize("kind", ["set", "last", "seeded", "holes"])
@pytest.mark.parametrize("cells", CELLS)
def test_face_sum_is_the_restatement_bit_for_bit(cells, kind, F):
    from upnerf_amd import baked
    from upnerf_amd import baked_sparse_tune as st
    from upnerf_amd.occupancy import OccupancyGrid
    key = ("layout", cells, kind)
    if key not in _CACHE:
        occ = OccupancyGrid.from_cells(dev(ft.holes_bits(cells) if kind == "holes" else pattern(cells, kind)), br.BOUNDS)
        slots, bricks, n = baked.brick_table(occ.words, cells)
        _CACHE[key] = (occ, slots, bricks, ft.copy_groups(slots.cpu().numpy(), cells))
    occ, slots, bricks, groups = _CACHE[key]
    n = bricks.numel()
    layout = st.PoolParams(slots, bricks, occ, br.BOUNDS, 0, rgbs=torch.zeros(n, 9, 9, 9, 4, device="cuda"))
    rng = np.random.RandomState(n + F)
    data = (rng.randn(n, 9, 9, 9, F) * np.exp(3 * rng.randn(n, 9, 9, 9, F))).astype(np.float32)  # magnitudes apart: the order shows
    want = ft.face_sum(data, slots.cpu().numpy(), cells)
    t = dev(data)
    assert st.face_sum(t, layout) is t
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    again = st.face_sum(dev(data), layout).cpu().numpy()  # a second run: the same bits
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    host = t.cpu()
    for _, c in groups:  # every copy of a shared point holds the same bits
        assert all(torch.equal(host[at], host[c[0]]) for at in c[1:])
    if kind == "set" and cells != (8, 8, 8):
        assert groups and (want != data).any()
    if kind == "holes" and cells != (8, 8, 8):
        # points with fewer copies than the geometry allows, yet two at least: the kernel passes over an empty holder; and points whose
        # first geometric holder is the empty one, so that the copy that collects is not the first the geometry names
        short = [(p, c) for p, c in groups if 2 <= len(c) < ft.geometric_copies(*p, cells)]
        empty = slots.cpu().numpy()
        first_missing = [p for p, c in short if empty[ft.holders(p[2], cells[2])[0][0], ft.holders(p[1], cells[1])[0][0], ft.holders(p[0], cells[0])[0][0]] < 0]
        assert short and n < empty.size and (first_missing or cells != (20, 12, 33))  # (the 3 x 2 x 5 layout has 82 such points)
        assert any((want[c[0]] != data[c[0]]).any() for _, c in short)
    if cells == (8, 8, 8) or kind == "last":
        assert not groups and np.array_equal(got.view(np.uint32), data.view(np.uint32))  # one brick: nothing is shared, nothing written


# ---- 2. the gradient against fp64 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("step", ["cell", "tenth"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_gradient_is_within_the_gathered_gate_of_the_fp64_restatement(name, step, degree, setting):
    dense, ref = reference(name, step, degree, setting)
    if SETTINGS[setting][1] > 0:
        assert dense["stop_margin"] > 0
    got = launch(name, step, degree, setting)
    worst = within(got, ref, degree, what=(name, step, degree, setting))
    # the test sees shared points: live points on faces that bricks share, and on the big grid the point all eight bricks hold
    live = dense["count"] > 0
    shared = [(x, y, z) for (x, y, z), _ in groups_of(name)]
    on_faces = sum(bool(live[z, y, x]) for x, y, z in shared)
    print(f"{name} {step} degree {degree} {setting}: {int(live.sum())} points receive a gradient, {on_faces} of them on shared faces "
          f"({len(shared)} shared points), up to {int(dense['count'].max())} contributions each; worst err / gate {worst:.3f}")
    assert on_faces >= 50
    if name == "big":
        assert scene_of(name, degree).n_bricks == 8 and live[8, 8, 8] and len(dict(groups_of(name))[(8, 8, 8)]) == 8
    copies = (got if degree == 0 else got[1]).cpu()
    for _, c in groups_of(name):  # after the face sum every copy holds the same bits
        assert all(torch.equal(copies[at], copies[c[0]]) for at in c[1:])


# ---- 3. the raw copies ----------------------------------------------------------------------------------------------------------------

def special_rays(name):
    """Rays along x through the cells below the planes y = 8 and z = 8 of the grid: they enter the bricks with by = bz = 0 only, and
    give the points of those planes a gradient there."""
    rgbs = GRIDS[name]()[0]
    Cx, Cy, Cz = cells_of(rgbs)
    lo, hi = br.bounds64(br.BOUNDS)
    ext = hi - lo
    rows = []
    for gy, gz in ((7.5, 7.4), (7.25, 6.6), (6.5, 7.8), (5.4, 5.3)):
        rows.append([lo[0] - 0.2, lo[1] + ext[1] * gy / Cy, lo[2] + ext[2] * gz / Cz, 1.0, 0.0, 0.0, 0.0, ext[0] + 0.4])
    return np.asarray(rows, np.float32)


@pytest.mark.parametrize("degree", [0, 2])
@pytest.mark.parametrize("name", list(GRIDS))
def test_raw_copies_hold_their_own_bricks_share_and_sum_to_the_gradient(name, degree):
    from upnerf_amd import baked_sparse_tune as st
    scene = scene_of(name, degree)
    bricks = scene.bricks.cpu().numpy()
    Bx, By, Bz = sr.brick_dims(cells_of(GRIDS[name]()[0]))
    for special, step, setting in ((True, "cell", "bg0-all"), (False, "tenth", "bg0-all")):
        dense, ref = reference(name, step, degree, setting, rows="special" if special else None)
        raw = launch(name, step, degree, setting, face_sum=False, special=special)
        raws = [raw] if degree == 0 else list(raw)
        if special:  # no ray enters a brick with by > 0 or bz > 0: every copy there is exactly zero
            away = [s for s, b in enumerate(bricks) if (b // Bx) % By > 0 or b // (Bx * By) > 0]
            assert away and len(away) < len(bricks)
            assert all(float(t[away].abs().max()) == 0.0 for t in raws)
            plane = dense["count"][8, 8, :] if Bz > 1 else dense["count"][:, 8, :]
            assert plane.sum() > 0  # ... though points they hold copies of did receive a gradient, in the bricks the rays entered
        # the fp64 sum over the copies is the point's gradient, within the gate gathered to the pool
        slots = scene.slots.cpu().numpy()
        summed = []
        for t in raws:
            a = t.cpu().numpy().astype(np.float64)
            a = a.reshape(a.shape[:4] + (-1,))
            total = sr.gather(ft.scatter_add(a, slots, cells_of(GRIDS[name]()[0])), bricks)
            summed.append(torch.from_numpy(total.reshape(t.shape)))
        within(summed[0] if degree == 0 else tuple(summed), ref, degree, what=(name, degree, special))
        # and the face sum of the raw copies is the launch with face_sum = True, within the gate
        for t in raws:
            st.face_sum(t, scene)
        within(raw, ref, degree, what=(name, degree, special, "summed on the GPU"))


# ---- 4. two runs, a cut launch, every cell bit set ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [0, 1, 2])
def test_two_runs_a_cut_launch_and_all_bits_set_agree_within_the_gate(degree):
    from upnerf_amd import baked_sparse_tune as st
    from upnerf_amd.occupancy import OccupancyGrid
    name, step, setting = "big", "tenth", "bg0-all"
    _, ref = reference(name, step, degree, setting)
    within(launch(name, step, degree, setting), ref, degree, what="first run")
    within(launch(name, step, degree, setting), ref, degree, what="second run")
    # cut at ray 33 (inside the first wave): both parts added raw into the same buffers, the faces summed once
    part = launch(name, step, degree, setting, rows=slice(0, 33), face_sum=False)
    both = launch(name, step, degree, setting, rows=slice(33, None), out=part, face_sum=False)
    scene = scene_of(name, degree)
    for t in ((both,) if degree == 0 else both):
        st.face_sum(t, scene)
    within(both, ref, degree, what="cut at 33")
    # every cell bit set: the march visits every sample inside an occupied brick (all eight are)
    params = st.PoolParams.of(scene, requires_grad=False)
    params.occupancy = OccupancyGrid.from_cells(torch.ones_like(scene.occupancy.cells()), br.BOUNDS)
    assert params.occupancy.fraction == 1.0 and scene.occupancy.fraction < 1.0
    within(launch(name, step, degree, setting, params=params), ref, degree, what="all bits set")


# ---- 5. autograd ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [0, 2])
def test_autograd_render_is_the_sparse_marcher_and_its_backward_the_kernel(degree):
    from upnerf_amd import baked_sparse_tune as st
    name, dt = "big", sh.steps(GRIDS["big"]()[0])["tenth"]
    scene = scene_of(name, degree)
    rays = dev(rays_of(name))
    params = st.PoolParams.of(scene)
    out = st.render(params, rays, dt, background=0.5, stop=1e-3)
    direct = scene.render(rays, dt, background=0.5, stop=1e-3)
    for k in ("rgb", "depth", "opacity"):
        assert torch.equal(out[k], direct[k]), k
    g_rgb, g_depth, g_op = (dev(g) for g in tr.upstream(rays.shape[0]))
    ((out["rgb"] * g_rgb).sum() + (out["depth"] * g_depth).sum() + (out["opacity"] * g_op).sum()).backward()
    # the direct call's gate: the reference for these arguments (background 0.5, stop 1e-3, all three upstream gradients)
    key = ("ref-autograd", degree)
    if key not in _CACHE:
        ref = tr.grad(numbers(name, degree)[0], degree, br.BOUNDS, rays_of(name), dt, 0.5, 1e-3, *tr.upstream(rays.shape[0]))
        assert ref["stop_margin"] > 0
        _CACHE[key] = to_pool(ref, degree, scene.bricks.cpu().numpy())
    ref = _CACHE[key]
    want = st.backward(scene.pool, params, rays, dt, 0.5, 1e-3, g_rgb, g_depth, g_op)
    within(want, ref, degree, what="direct")
    grads = tuple(t.grad for t in params.tensors)
    assert all(g is not None and g.shape == t.shape and g.dtype == torch.float32 for g, t in zip(grads, params.tensors))
    within(grads[0] if degree == 0 else grads, ref, degree, what="autograd")
    params2 = st.PoolParams.of(scene)  # a loss that uses the colour alone: depth and opacity arrive as None
    (st.render(params2, rays, dt)["rgb"] ** 2).mean().backward()
    assert all(t.grad is not None and float(t.grad.abs().max()) > 0 for t in params2.tensors)
    with pytest.raises(ValueError):
        st.PoolParams.of(scene.densify())
    with pytest.raises(ValueError):
        scene.densify().tune_pool(1e-2)


# ---- 6. the tuner ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [0, 2])
def test_the_pool_tuner_brings_a_perturbed_scene_back_and_keeps_the_copies_identical(degree):
    """The dense test's problem and criterion (rho_ref from the fp64 loop of the restatement, not from here), scene B sparsified
    and tuned on its pool."""
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.baked_sparse_tune import PoolTuner
    A, B, level, rays, step = tr.tuning_problem(degree)
    key = ("tune", degree)
    if key not in _CACHE:
        _CACHE[key] = tr.tune_loop(degree)
    curve = _CACHE[key]
    rho_ref = curve[-1] / curve[0]
    assert rho_ref <= 0.5

    def scene(P):
        if degree == 0:
            return BakedScene.from_grids(dev(P[..., 3]), dev(P[..., :3]), br.BOUNDS, level)
        return BakedScene.from_records(dev(sh.pack(P[0], P[1], level, degree)[0]), br.BOUNDS, level, degree)

    rays_d = dev(rays)
    target = scene(A).render(rays_d, step)["rgb"].clone()
    b = scene(B).sparsify()
    assert b.sparse and b.n_bricks == 4
    tuner = b.tune_pool(tr.TUNE_LR, betas=tr.TUNE_BETAS, eps=tr.TUNE_EPS)
    assert isinstance(tuner, PoolTuner) and tuner.p.numel() == 4 * 729 * (4 if degree == 0 else 28)
    losses = [tuner.step(rays_d, target, step) for _ in range(tr.TUNE_ITERS)]
    tuned = tuner.scene()
    last = float(((tuned.render(rays_d, step)["rgb"] - target) ** 2).mean())
    first = float(losses[0])
    print(f"degree {degree}: fp64 loop L(0) = {curve[0]:.4e} -> L(k) = {curve[-1]:.4e} (rho_ref {rho_ref:.3f}); pool tuner L(0) = {first:.4e} -> "
          f"L(k) = {last:.4e} (rho {last / first:.3f}; the gate is {rho_ref + (1 - rho_ref) / 2:.3f})")
    assert abs(first - curve[0]) <= 1e-3 * curve[0]  # the same problem
    assert last <= first * (rho_ref + (1 - rho_ref) / 2)
    # the layout's invariant: every copy of every shared point holds the same bytes, in the masters and in the tuned pool
    groups = ft.copy_groups(b.slots.cpu().numpy(), tuple(n - 1 for n in b.resolution))
    assert len(groups) >= 100
    for t in list(tuner.masters) + [tuned.pool]:
        flat = t.contiguous().view(torch.uint8).reshape(4, 9, 9, 9, -1).cpu()
        for _, c in groups:
            assert all(torch.equal(flat[at], flat[c[0]]) for at in c[1:])
    assert tuned.sparse and torch.equal(tuned.bricks, b.bricks) and torch.equal(tuned.slots, b.slots)
    dense = tuned.densify()
    for bg in (0.0, 1.0):
        out, want = tuned.render(rays_d, step, background=bg), dense.render(rays_d, step, background=bg)
        assert all(torch.equal(out[k], want[k]) for k in out)
        assert all(bool(torch.isfinite(v).all()) for v in out.values())
    assert not tuned.occupancy.cells()[~b.occupancy.cells()].any()  # frozen: nothing grew where B was empty


# ---- 7. distill on a sparse bake --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def system():
    return cases.make_system()


def test_distill_on_a_sparse_bake_lowers_the_loss_and_keeps_the_bricks(system):
    from upnerf_amd import baked_sparse_tune as st
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.geometry import density_grid
    box, res, img = ((-0.7, -0.5, -0.6), (0.8, 0.6, 0.9)), (9, 9, 17), 4  # 8 x 8 x 16 cells: two bricks along z
    sigma = density_grid(system, box, res)
    scene = BakedScene.build(system, box, res, float(sigma.median()), img_id=img, sparse=True)
    assert scene.sparse and scene.n_bricks >= 1 and scene.slots.numel() == 2
    ids = [0, 2, 5]
    tuned, curve = st.distill(system, scene, ids, iters=8, batch=256, baked_step=0.05, seed=3, lr=0.05, img_id=img)
    print(f"distill on the pool ({scene.n_bricks} bricks): loss {curve[0]:.4e} -> {curve[-1]:.4e} over {len(curve)} iterations")
    assert len(curve) == 8 and np.isfinite(curve).all() and curve[-1] < curve[0]
    assert isinstance(tuned, BakedScene) and tuned.sparse and tuned.resolution == scene.resolution
    assert torch.equal(tuned.bricks, scene.bricks) and torch.equal(tuned.slots, scene.slots)
    with pytest.raises(ValueError):
        st.distill(system, scene.densify(), ids, iters=2, batch=64, baked_step=0.05, img_id=img)  # a dense scene is baked_tune's
