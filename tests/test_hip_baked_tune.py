"""The baked marcher's backward pass on the GPU (csrc/baked.hip: upnerf_baked_render_bwd, upnerf_baked_project;
upnerf_amd/baked_tune.py).

Reference: tests/baked_tune_ref.py -- fp64 numpy, brute force over every lattice sample, never a look at the occupancy bits; its
docstring derives the per-element gates from counts of roundings.  The gradient's sums are float atomic adds, so nothing here is
held to equality between two launches: two runs, a launch cut in two and a launch into filled buffers are held to the same gates.

Grids and rays: those of tests/test_hip_baked.py (67 rays: a full wave and a ragged one, misses and non-finite rows among them),
then 64 identical rays (every lane adds to the same addresses) and one ray inside a cell face; a step of one cell (the register
accumulator is flushed at every sample) and of a tenth of a cell (it is flushed rarely).  Worst measured error / gate on an MI355X:
0.260 at the cell step, 0.139 at the tenth."""
import numpy as np
import pytest
import torch

import baked_cases as cases
import baked_ref as br
import baked_sh_ref as sh
import baked_tune_ref as tr
from baked_cases import dev

pytestmark = pytest.mark.gpu

_CACHE = {}
# the two settings every (grid, step, degree) is run under: background, stop, and whether g_depth / g_opacity are given
SETTINGS = {"bg0-all": (0.0, 0.0, True), "bg1-stop-rgb": (1.0, 1e-3, False)}


def rays_all(name):
    return cases.rays_all(sh.GRIDS[name]()[0])


def scene_of(name, degree):
    """(BakedScene, the numbers the reference differentiates: rgbs, or (k, sigma) of the stored records)."""
    points, level = sh.GRIDS[name]() if degree == 0 else sh.sh_grid(name, degree)
    scene = cases.scene_of((__name__, name, degree), lambda: cases.build(points, level, degree))
    return scene, points if degree == 0 else sh.unpack(points, degree)


def reference(name, step, degree, setting):
    """The fp64 restatement, computed once per case and never changed."""
    key = ("ref", name, step, degree, setting)
    if key not in _CACHE:
        bg, stop, rest = SETTINGS[setting]
        rays = rays_all(name)
        g_rgb, g_depth, g_op = tr.upstream(rays.shape[0])
        dt = sh.steps(sh.GRIDS[name]()[0])[step]
        _CACHE[key] = tr.grad(scene_of(name, degree)[1], degree, br.BOUNDS, rays, dt, bg, stop, g_rgb, g_depth if rest else None,
                              g_op if rest else None)
    return _CACHE[key]


def launch(name, step, degree, setting, rows=slice(None), out=None, scene=None):
    """upnerf_baked_render_bwd on the rays `rows`: the gradient (a device tensor at degree 0, else the pair)."""
    from upnerf_amd import baked_tune
    bg, stop, rest = SETTINGS[setting]
    scene = scene or scene_of(name, degree)[0]
    rays = rays_all(name)
    g_rgb, g_depth, g_op = (dev(g[rows]) for g in tr.upstream(rays.shape[0]))
    dt = sh.steps(sh.GRIDS[name]()[0])[step]
    got = baked_tune.backward(scene.grid, degree, scene.occupancy, br.BOUNDS, dev(rays[rows]), dt, bg, stop, g_rgb,
                              g_depth if rest else None, g_op if rest else None, out=out)
    torch.cuda.synchronize()
    return got


def pairs(got, ref, degree):
    """[(name, kernel value fp64, reference, gate)] of a gradient."""
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)
    if degree == 0:
        return [("grad", f(got), ref["grad"], ref["gate"])]
    return [("grad_coef", f(got[0]), ref["grad_coef"], ref["gate_coef"]), ("grad_sigma", f(got[1]), ref["grad_sigma"], ref["gate_sigma"])]


def within(got, ref, degree, slack=1.0, what=""):
    worst = 0.0
    for name, g, want, gate in pairs(got, ref, degree):
        assert np.isfinite(g).all()
        err = np.abs(g - want)
        worst = max(worst, float((err / np.maximum(slack * gate, 1e-300))[gate > 0].max(initial=0.0)))
        assert float(np.abs(g[gate == 0]).max(initial=0.0)) == 0.0, (what, name)  # no contribution: exactly nothing
        assert (err <= slack * gate).all(), (what, name, np.argwhere(err > slack * gate)[:5], float(err.max()))
    return worst


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("step", ["cell", "tenth"])
@pytest.mark.parametrize("name", list(sh.GRIDS))
def test_gradient_is_within_its_gate_of_the_fp64_restatement(name, step, degree, setting):
    ref = reference(name, step, degree, setting)
    if SETTINGS[setting][1] > 0:
        assert ref["stop_margin"] > 0  # no ray ends on a sample that fp32 could place on the other side of `stop`
    got = launch(name, step, degree, setting)
    worst = within(got, ref, degree, what=(name, step, degree, setting))
    live = ref["count"] > 0
    big = np.abs(ref["grad"] if degree == 0 else ref["grad_sigma"]).max()
    print(f"{name} {step} degree {degree} {setting}: {int(live.sum())} points receive a gradient, up to {int(ref['count'].max())} "
          f"contributions each, largest sigma gradient {big:.3e}; worst err / gate {worst:.3f}")
    assert live.sum() >= 50 and big > 1e-3
    sigma = scene_of(name, degree)[1][..., 3] if degree == 0 else scene_of(name, degree)[1][1]
    assert not live[sigma == 0].any()  # a corner whose sigma is zero is no parameter


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_two_runs_a_cut_launch_filled_buffers_and_all_bits_set_agree_within_the_gate(degree):
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.occupancy import OccupancyGrid
    name, step, setting = "blob", "tenth", "bg0-all"
    ref = reference(name, step, degree, setting)
    first = launch(name, step, degree, setting)
    within(launch(name, step, degree, setting), ref, degree, what="second run")
    # cut at ray 33 (inside the first wave), both parts summed into the same buffers
    part = launch(name, step, degree, setting, rows=slice(0, 33))
    both = launch(name, step, degree, setting, rows=slice(33, None), out=part)
    within(both, ref, degree, what="cut at 33")
    # pre-filled buffers: pre-fill plus gradient; the sum into a filled element rounds on the fill as well, once per contribution
    fill = 0.75
    zeros = [torch.zeros_like(t) for t in ((first,) if degree == 0 else first)]
    filled = [z + fill for z in zeros]
    got = launch(name, step, degree, setting, out=filled[0] if degree == 0 else tuple(filled))
    got = [got] if degree == 0 else list(got)
    for (nm, g, want, gate), t in zip(pairs(first, ref, degree), got):
        g = t.detach().cpu().numpy().astype(np.float64)
        count = ref["count"][..., None] if g.ndim == 4 else (ref["count"][..., None, None] if g.ndim == 5 else ref["count"])
        assert (np.abs(g - fill - want) <= gate + (count + 1) * tr.U * fill).all(), nm
        assert (g[np.broadcast_to(count, g.shape) == 0] == fill).all()
    # the visited set: every occupancy bit set, the marcher visits every sample inside the box
    scene = scene_of(name, degree)[0]
    full = BakedScene(scene.rgbs, br.BOUNDS, scene.level) if degree == 0 else BakedScene.from_records(scene.records, br.BOUNDS, scene.level, degree)
    full.occupancy = OccupancyGrid.from_cells(torch.ones_like(scene.occupancy.cells()), br.BOUNDS)
    assert full.occupancy.fraction == 1.0 and scene.occupancy.fraction < 1.0
    within(launch(name, step, degree, setting, scene=full), ref, degree, what="all bits set")


@pytest.mark.parametrize("degree", [0, 2])
def test_autograd_render_is_the_marcher_and_its_backward_the_kernel(degree):
    from upnerf_amd import baked_tune
    name, dt = "blob", sh.steps(sh.GRIDS["blob"]()[0])["tenth"]
    scene = scene_of(name, degree)[0]
    rays = dev(br.make_rays())
    params = baked_tune.SceneParams.of(scene)
    out = baked_tune.render(params, rays, dt, background=0.5, stop=1e-3)
    direct = scene.render(rays, dt, background=0.5, stop=1e-3)
    for k in ("rgb", "depth", "opacity"):  # (degree 2: the records packed from the unpacked parameters are the records)
        assert torch.equal(out[k], direct[k]), k
    g_rgb, g_depth, g_op = (dev(g) for g in tr.upstream(67))
    loss = (out["rgb"] * g_rgb).sum() + (out["depth"] * g_depth).sum() + (out["opacity"] * g_op).sum()
    loss.backward()
    want = baked_tune.backward(scene.grid, degree, scene.occupancy, br.BOUNDS, rays, dt, 0.5, 1e-3, g_rgb, g_depth, g_op)
    want = (want,) if degree == 0 else want
    for t, w in zip(params.tensors, want):
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == torch.float32
        scale = float(w.abs().max())
        assert scale > 0 and float((t.grad - w).abs().max()) <= 1e-4 * scale  # two launches of an atomic sum: rounding apart
    # a loss that uses the colour alone: depth and opacity arrive as None, not as zeros
    params2 = baked_tune.SceneParams.of(scene)
    (baked_tune.render(params2, rays, dt)["rgb"] ** 2).mean().backward()
    assert all(t.grad is not None and float(t.grad.abs().max()) > 0 for t in params2.tensors)
    with pytest.raises(ValueError):
        baked_tune.SceneParams.of(scene.sparsify())
    with pytest.raises(ValueError):
        baked_tune.BakedTuner(scene.sparsify(), 1e-2)


@pytest.mark.parametrize("n", [1, 63, 65])
def test_project_is_numpy_bit_for_bit(n):
    from upnerf_amd import baked_tune
    rng = np.random.RandomState(n)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1.5, 1.0, 1.5, 2.0 ** -149, -2.0 ** -149], np.float32)
    rgbs = rng.uniform(-0.5, 1.5, (n, 4)).astype(np.float32)
    rgbs.reshape(-1)[rng.permutation(n * 4)[:min(n * 4, 3 * special.size)]] = np.resize(special, min(n * 4, 3 * special.size))
    if n == 1:
        rgbs[0] = [np.nan, 1.5, -0.25, 2.0]
    t = dev(rgbs.reshape(1, 1, n, 4))
    baked_tune.project(0, rgbs=t)
    assert np.array_equal(t.cpu().numpy().reshape(n, 4).view(np.uint32), tr.project(0, rgbs=rgbs).view(np.uint32))
    for degree in (1, 2):
        s = dev(rgbs[:, 3].copy())
        baked_tune.project(degree, sigma=s)
        assert np.array_equal(s.cpu().numpy().view(np.uint32), tr.project(degree, sigma=rgbs[:, 3].copy()).view(np.uint32))


@pytest.mark.parametrize("degree", [0, 2])
def test_the_tuner_brings_a_perturbed_scene_back_towards_its_targets(degree):
    """The test that cannot pass without the backward pass.  Scene A, scene B = A perturbed, targets A's own render; the GPU's
    loop must achieve at least half the reduction the fp64 loop of the restatement achieves (rho_ref from there, not from here)."""
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.baked_tune import BakedTuner
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
    b = scene(B)
    tuner = b.tune(tr.TUNE_LR, betas=tr.TUNE_BETAS, eps=tr.TUNE_EPS)
    assert isinstance(tuner, BakedTuner)
    losses = [tuner.step(rays_d, target, step) for _ in range(tr.TUNE_ITERS)]
    tuned = tuner.scene()
    last = float(((tuned.render(rays_d, step)["rgb"] - target) ** 2).mean())
    first = float(losses[0])
    print(f"degree {degree}: fp64 loop L(0) = {curve[0]:.4e} -> L(k) = {curve[-1]:.4e} (rho_ref {rho_ref:.3f}); GPU L(0) = {first:.4e} -> "
          f"L(k) = {last:.4e} (rho {last / first:.3f}; the gate is {rho_ref + (1 - rho_ref) / 2:.3f})")
    assert abs(first - curve[0]) <= 1e-3 * curve[0]  # the same problem
    assert last <= first * (rho_ref + (1 - rho_ref) / 2)
    # the occupancy invariant: every clear cell has eight zero corners
    sigma = tuned.rgbs[..., 3] if degree == 0 else tuned.records[..., 56:60].contiguous().view(torch.float32).squeeze(-1)
    occupied = dev(br.occupied_cells(np.stack([sigma.cpu().numpy()] * 4, -1)))
    assert torch.equal(tuned.occupancy.cells(), occupied)
    assert not tuned.occupancy.cells()[~b.occupancy.cells()].any()  # frozen: nothing grew where B was empty
    out = tuned.render(rays_d, step, background=1.0)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())


@pytest.fixture(scope="module")
def system():
    return cases.make_system()


def test_distill_lowers_the_loss_against_the_fields_own_renders(system):
    from upnerf_amd import baked_tune
    from upnerf_amd import novel_view as nv
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.geometry import density_grid
    box, res, img = ((-0.7, -0.5, -0.6), (0.8, 0.6, 0.9)), (9, 9, 9), 4  # round the origin, where the fields' density is
    sigma = density_grid(system, box, res)
    scene = BakedScene.build(system, box, res, float(sigma.median()), img_id=img)
    ids = [0, 2, 5]  # three of the six training cameras, 16 x 12 pixels each: 576 rays
    tuned, curve = baked_tune.distill(system, scene, ids, iters=8, batch=256, baked_step=0.05, seed=3, lr=0.05, img_id=img)
    path = nv.CameraPath.through_images(system, ids, n_frames=7)
    again = baked_tune.distill(system, scene, path, iters=2, batch=256, baked_step=0.05, seed=3, lr=0.05, img_id=img)[1]
    print(f"distill: loss {curve[0]:.4e} -> {curve[-1]:.4e} over {len(curve)} iterations")
    assert len(curve) == 8 and np.isfinite(curve).all() and curve[-1] < curve[0]
    assert abs(again[0] - curve[0]) <= 1e-5 * curve[0]  # a path's keyframes are its cameras; seeded batches: the same first loss
    assert isinstance(tuned, BakedScene) and tuned.resolution == scene.resolution and not tuned.sparse
    with pytest.raises(ValueError):
        baked_tune.distill(system, scene, ids, iters=2, batch=64, baked_step=0.05)  # no appearance named
