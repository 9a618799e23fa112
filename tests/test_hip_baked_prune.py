"""Pruning a baked scene by what a set of rays sees, on the GPU (csrc/baked.hip: upnerf_baked_visibility, upnerf_baked_prune;
csrc/brick.hip: upnerf_brick_face_max; upnerf_amd/baked_prune.py).

The visibility is held to the fp64 restatement tests/baked_prune_ref.py, which gives an interval per point (its docstring says
why, and tests/test_baked_prune_cpu.py asserts that few points of these scenes are undecided); to itself bit for bit across runs,
cuts of the launch, degrees and layouts -- a maximum is exact and commutative --; and the pruned scene to the claim that makes the
default weight safe: the rays it was pruned for render to the same bits.

Scenes: baked_ref's blob (11 x 10 x 9 points) and corner grids with its 67 rays; a ragged 18 x 10 x 11-point grid (17 cells on x:
three bricks, two shared faces); a wall 20 x 12 x 12 points with a slab of sigma 1000 three points thick and a blob three empty
cells behind it, 64 rays from the front at half a cell a step -- alpha rounds to 1 and T is exactly 0 inside the wall."""
import ctypes as C

import numpy as np
import pytest
import torch

import baked_cases as cases
import baked_prune_ref as pr
import baked_ref as br
import baked_sh_ref as sh
import baked_sparse_ref as sr
import baked_sparse_tune_ref as ft
import baked_tune_ref as tr
from baked_cases import dev

pytestmark = pytest.mark.gpu

_CACHE = {}
F32 = np.float32
GRIDS = {"blob": br.blob_grid, "corners": br.corner_grid, "ragged": pr.ragged_grid, "wall": pr.wall_grid}
STOPS = (0.0, 1e-3)


def grid_of(name):
    if ("grid", name) not in _CACHE:
        _CACHE[("grid", name)] = GRIDS[name]()
    return _CACHE[("grid", name)]


def rays_of(name):
    return pr.wall_rays()[0] if name == "wall" else br.make_rays()


def steps_of(name):
    if name == "wall":
        return {"half": pr.wall_rays()[1]}
    cell = br.cell_size(grid_of(name)[0])
    return {"cell": float(F32(cell)), "tenth": float(F32(cell / 10))}


def scene_of(name, degree=0, sparse=False):
    rgbs, level = grid_of(name)
    records = lambda: sh.pack(sh.coefficients(rgbs[..., 3].shape, degree, 31 + degree), rgbs[..., 3], level, degree)[0]
    return cases.scene_of((__name__, name, degree), lambda: cases.build(rgbs if degree == 0 else records(), level, degree), sparse)


def reference(name, step_name, stop):
    """(lo, hi) of the restatement: computed once per case and never changed."""
    key = ("ref", name, step_name, stop)
    if key not in _CACHE:
        _CACHE[key] = pr.visibility(grid_of(name)[0][..., 3], br.BOUNDS, rays_of(name), steps_of(name)[step_name], stop)
    return _CACHE[key]


CASES = [(n, s) for n in GRIDS for s in (("half",) if n == "wall" else ("cell", "tenth"))]


# ---- (a) the intervals ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("name,step_name", CASES)
def test_visibility_lies_inside_the_restatements_intervals(name, step_name, stop):
    lo, hi = reference(name, step_name, stop)
    rays, step = dev(rays_of(name)), steps_of(name)[step_name]
    dense = scene_of(name).visibility(rays, step, stop)
    sparse_scene = scene_of(name, sparse=True)
    pool = sparse_scene.visibility(rays, step, stop)
    torch.cuda.synchronize()
    d = dense.cpu().numpy()
    ok = pr.within(d, lo, hi)
    print(f"{name} {step_name} stop {stop}: {int((d > 0).sum())} of {d.size} points seen, undecided share {pr.uncertain(lo, hi):.4f}, "
          f"outside {int((~ok).sum())}")
    assert d.shape == grid_of(name)[0].shape[:3] and ok.all(), (np.argwhere(~ok)[:5], d[~ok][:5], lo[~ok][:5], hi[~ok][:5])
    bricks = sparse_scene.bricks.cpu().numpy()
    lo_p, hi_p = (sr.gather(x[..., None], bricks)[..., 0] for x in (lo, hi))
    assert tuple(pool.shape) == (len(bricks), 9, 9, 9) and pr.within(pool.cpu().numpy(), lo_p, hi_p).all()
    assert (d > 0).sum() > 50 and ((d == 0) | (d >= F32(pr.TINY_NORMAL))).all()


# ---- (b) the same bits every run and however the rays are cut ------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
def test_two_runs_cut_launches_and_single_rays_give_the_same_bits(sparse):
    from upnerf_amd import baked_prune as bp
    scene = scene_of("blob", sparse=sparse)
    rays, step, stop = dev(br.make_rays()), steps_of("blob")["tenth"], 1e-3
    shape = (scene.n_bricks, 9, 9, 9) if sparse else scene.resolution[::-1]

    def launch(rows, out=None):
        out = torch.zeros(shape, device="cuda") if out is None else out
        bp.march_visibility(scene, rays[rows], step, stop, out)
        return out

    whole, again = launch(slice(None)), launch(slice(None))
    assert torch.equal(whole, again) and float(whole.max()) > 0
    cut = torch.zeros(shape, device="cuda")
    for a, b in ((0, 1), (1, 8), (8, 35), (35, 67)):
        launch(slice(a, b), cut)
    assert torch.equal(cut, whole)
    singles = torch.zeros(shape, device="cuda")
    for r in range(67):
        singles = torch.maximum(singles, launch(slice(r, r + 1)))
    assert torch.equal(singles, whole)
    assert torch.equal(scene.visibility(rays, step, stop, chunk=5), scene.visibility(rays, step, stop))
    if not sparse:
        assert torch.equal(scene.visibility(rays, step, stop), whole)  # (a pool's is taken after the face max)


# ---- (c) the degree is not seen ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("name", ["blob", "corners"])
def test_visibility_is_the_same_at_every_degree(name, sparse):
    rays = dev(rays_of(name))
    for step_name, stop in (("cell", 0.0), ("tenth", 1e-3)):
        step = steps_of(name)[step_name]
        v0 = scene_of(name, 0, sparse).visibility(rays, step, stop)
        for degree in (1, 2):
            assert torch.equal(scene_of(name, degree, sparse).visibility(rays, step, stop), v0), (name, degree, step_name)


# ---- (d) the pool against the grid; the face max; the face sum as it was -------------------------------------------------------------

@pytest.mark.parametrize("name", list(GRIDS))
def test_sparse_visibility_is_the_dense_one_gathered(name):
    from upnerf_amd.baked import brick_gather
    rays = dev(rays_of(name))
    for step_name, step in steps_of(name).items():
        for stop in STOPS:
            sparse = scene_of(name, sparse=True)
            dense = scene_of(name).visibility(rays, step, stop)
            want = brick_gather(dense.unsqueeze(-1).contiguous(), sparse.bricks).squeeze(-1)
            assert torch.equal(sparse.visibility(rays, step, stop), want), (name, step_name, stop)


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("name", ["ragged", "corners"])
def test_face_max_is_numpys_and_face_sum_keeps_its_bits(name, F):
    from upnerf_amd import baked_prune as bp
    from upnerf_amd import baked_sparse_tune as st
    scene = scene_of(name, sparse=True)
    n, cells = scene.n_bricks, tuple(c - 1 for c in scene.resolution)
    rng = np.random.RandomState(n + F)
    data = (rng.randn(n, 9, 9, 9, F) * np.exp(3 * rng.randn(n, 9, 9, 9, F))).astype(F32)
    t = dev(data)
    assert bp.face_max(t, scene) is t
    want = np.stack([pr.face_max(data[..., f], scene.bricks.cpu().numpy(), scene.resolution) for f in range(F)], -1)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(bp.face_max(dev(data), scene), t)  # a second run
    if name == "ragged":
        assert (want != data).any()
    s = st.face_sum(dev(data), scene).cpu().numpy()
    assert np.array_equal(s.view(np.uint32), ft.face_sum(data, scene.slots.cpu().numpy(), cells).view(np.uint32))


# ---- (e) upnerf_baked_prune ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [16, 32, 64])
def test_prune_kernel_zeroes_what_is_below_the_weight_and_keeps_the_rest(E):
    from upnerf_amd import _lib
    from upnerf_amd import baked_prune as bp
    from upnerf_amd.baked import _aligned
    n = 1031  # more than one block, no multiple of anything
    rng = np.random.RandomState(E)
    pts = rng.randint(1, 256, (n, E)).astype(np.uint8)
    vis = rng.uniform(0, 1, n).astype(F32)
    vis[::7], vis[3], vis[5], vis[11] = 0.0, np.nan, F32(pr.TINY_NORMAL), 0.25
    for w in (None, 0.25):
        store = _aligned(n * E, E, "cuda")[:n * E].view(n, E).copy_(dev(pts))
        kept = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        assert bp.prune_points(store, dev(vis), E, w, kept) is store
        want, keep = pr.prune(pts, vis, pr.TINY_NORMAL if w is None else w)
        assert np.array_equal(store.cpu().numpy(), want) and np.array_equal(kept.cpu().numpy(), keep)
        assert keep[11] == 1 and keep[3] == 0 and keep[0] == 0 and keep[5] == (1 if w is None else 0)
    store = _aligned(n * E, E, "cuda")[:n * E].view(n, E).copy_(dev(pts))
    bp.prune_points(store, dev(vis), E, 0.5)  # without kept
    assert np.array_equal(store.cpu().numpy(), pr.prune(pts, vis, 0.5)[0])
    v = dev(vis)
    ok = dict(n=n, min_weight=0.5, E=E, vis=_lib.ptr(v), points=_lib.ptr(store), kept=None)
    for bad in (dict(n=0), dict(E=8), dict(E=48), dict(vis=None), dict(points=None), dict(min_weight=float("nan")),
                dict(points=store.data_ptr() + 4)):
        a = _lib.BakedPruneArgs(**{**ok, **bad})
        assert _lib.lib.upnerf_baked_prune(C.byref(a), _lib.stream()) == -1, bad
    with pytest.raises(ValueError):
        bp.prune_points(store, v[:-1], E, 0.5)


def test_visibility_refuses_what_the_forward_refuses_and_its_own():
    from upnerf_amd import _lib
    from upnerf_amd.baked import _common
    scene, sparse = scene_of("blob"), scene_of("blob", sparse=True)
    rays = dev(br.make_rays())
    vis = torch.zeros(scene.resolution[::-1], device="cuda")
    common = _common(scene.occupancy, scene.bounds, rays, 0.1, 0.0, 0.0)
    del common["background"]
    ok = dict(common, E=16, sigma_offset=12, points=_lib.ptr(scene.grid), slots=None, vis=_lib.ptr(vis))
    call = lambda **kw: _lib.lib.upnerf_baked_visibility(C.byref(_lib.BakedVisibilityArgs(**{**ok, **kw})), _lib.stream())
    assert call() == 0
    for bad in (dict(vis=None), dict(E=8), dict(E=24), dict(E=128), dict(sigma_offset=14), dict(sigma_offset=16), dict(sigma_offset=-4),
                dict(points=None), dict(words=None), dict(rays=None), dict(R=0), dict(step=0.0), dict(step=float("inf")), dict(stop=1.0),
                dict(stop=-0.1), dict(Cx=0), dict(rays=rays.data_ptr() + 4), dict(points=scene.grid.data_ptr() + 4),
                dict(hi=(C.c_float * 3)(*scene.bounds[0]))):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        scene.visibility(rays, 0.1, stop=1.0)
    with pytest.raises(ValueError):
        scene.visibility(rays, 0.1, chunk=0)
    with pytest.raises(ValueError):
        sparse.prune(rays, 0.1, min_weight=float("nan"))


# ---- (f) invariance: the rays a scene was pruned for render to the same bits ----------------------------------------------------------

@pytest.mark.parametrize("degree", [0, 2])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("name", list(GRIDS))
def test_the_pruned_scene_renders_its_rays_to_the_same_bits(name, sparse, degree):
    scene = scene_of(name, degree, sparse)
    rays = dev(rays_of(name))
    dropped = 0
    for step_name, step in steps_of(name).items():
        for stop in STOPS:
            before = scene.render(rays, step, background=0.25, stop=stop)
            small = scene.prune(rays, step, stop=stop)
            after = small.render(rays, step, background=0.25, stop=stop)
            for k in ("rgb", "depth", "opacity"):
                same = before[k] == after[k]
                assert torch.equal(before[k], after[k]), (name, sparse, degree, step_name, stop, k, torch.nonzero(~same)[:5].tolist())
            assert small.sparse == sparse and small.sh_degree == degree and small.resolution == scene.resolution
            assert small.nbytes <= scene.nbytes and small.fraction <= scene.fraction
            dropped += int(small.fraction < scene.fraction)
    assert dropped > 0  # the rays do not see everything


# ---- (g) the wall -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [0, 2])
def test_what_the_wall_hides_is_gone_and_sparse_prune_is_dense_prune_sparsified(degree):
    from upnerf_amd.baked import SIGMA_AT
    from upnerf_amd.baked_env import Environment
    rays, step = dev(pr.wall_rays()[0]), pr.wall_rays()[1]
    dense, sparse = scene_of("wall", degree), scene_of("wall", degree, sparse=True)
    env = Environment.from_array(np.random.RandomState(5).uniform(0, 1, (6, 5, 5, 4)).astype(F32), "cuda")
    sparse_env = sparse.with_environment(env)
    held = [t.clone() for t in (sparse.pool, sparse.slots, sparse.bricks, sparse.occupancy.words, dense.grid, dense.occupancy.words)]
    pd, ps = dense.prune(rays, step), sparse_env.prune(rays, step)
    sigma = pd.grid.view(torch.uint8)[..., SIGMA_AT[degree]:SIGMA_AT[degree] + 4].contiguous().view(torch.float32).squeeze(-1).cpu().numpy()
    before = grid_of("wall")[0][..., 3]
    assert (before[:, :, pr.BLOB_X[0]:pr.BLOB_X[1]] > 0).any() and (sigma[:, :, pr.BLOB_X[0]:pr.BLOB_X[1]] == 0).all()  # the hidden blob
    assert (sigma[:, :, pr.WALL_X[1]:] == 0).all()  # the layers of the wall behind the one T ends in, the back layer among them
    assert (sigma[2:-2, 2:-2, pr.WALL_X[0]] == 1000.0).all()  # the front layer stays where the rays arrive
    kept = sigma != 0
    assert np.array_equal(pd.grid.view(torch.uint8).cpu().numpy()[kept], dense.grid.view(torch.uint8).cpu().numpy()[kept])  # bytes kept
    assert ps.n_bricks < sparse.n_bricks and ps.nbytes < sparse.nbytes and pd.n_bricks == ps.n_bricks
    want = pd.sparsify()
    assert torch.equal(ps.pool.view(torch.uint8), want.pool.view(torch.uint8)) and torch.equal(ps.slots, want.slots) and torch.equal(ps.bricks, want.bricks)
    assert torch.equal(ps.occupancy.words, want.occupancy.words)
    now = (sparse.pool, sparse.slots, sparse.bricks, sparse.occupancy.words, dense.grid, dense.occupancy.words)
    assert all(torch.equal(a, b) for a, b in zip(held, now))  # the input scenes are untouched
    assert ps.env is env and pd.env is None and ps.level == sparse.level and ps.bounds == sparse.bounds and ps.sh_degree == degree
    # a weight between the two samples of the wall's first cell (w ~ 1 and ~ 5e-5) keeps it; one above every weight empties the scene
    assert dense.prune(rays, step, min_weight=0.5).fraction == pd.fraction
    assert sparse.prune(rays, step, min_weight=2.0).n_bricks == 0


# ---- (h) the tuners -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
def test_tuner_pruned_keeps_kind_and_settings_resets_adam_and_still_learns(sparse):
    from upnerf_amd.baked import BakedScene
    A, B, level, rays, step = tr.tuning_problem(0)
    make = lambda P: BakedScene.from_grids(dev(P[..., 3]), dev(P[..., :3]), br.BOUNDS, level)
    rays_d = dev(rays)
    target = make(A).render(rays_d, step)["rgb"].clone()
    b = make(B).sparsify() if sparse else make(B)
    tuner = (b.tune_pool if sparse else b.tune)(tr.TUNE_LR, betas=tr.TUNE_BETAS, eps=tr.TUNE_EPS, tv_sigma=1e-4)
    tuner.step(rays_d, target, step)
    small = tuner.pruned(rays_d, step)
    assert type(small) is type(tuner) and small.t == 0 and small.lr == tuner.lr and small.betas == tuner.betas and small.eps == tuner.eps
    assert small.tv_sigma == 1e-4 and small.tv_colour == tuner.tv_colour and small.tv_eps == tuner.tv_eps
    assert float(small.m.abs().max()) == 0.0 and float(small.v.abs().max()) == 0.0
    assert small.occupancy.n_occupied() < tuner.occupancy.n_occupied()
    if sparse:
        assert small.scene().n_bricks <= tuner.scene().n_bricks
    losses = [float(small.step(rays_d, target, step)) for _ in range(2)]
    print(f"{'pool' if sparse else 'dense'} tuner after pruned(): loss {losses[0]:.4e} -> {losses[1]:.4e}")
    assert small.t == 2 and np.isfinite(losses).all() and losses[1] < losses[0]
    heavy = tuner.pruned(rays_d, step, min_weight=0.05, stop=1e-3)
    assert heavy.occupancy.n_occupied() < small.occupancy.n_occupied()


# ---- (i), (j) distill -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def system():
    return cases.make_system()


@pytest.mark.parametrize("sparse", [False, True])
def test_distill_prunes_then_upsamples_and_is_unchanged_without_prune_at(system, sparse):
    from upnerf_amd import baked_sparse_tune, baked_tune
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.geometry import density_grid
    box, res, img = ((-0.7, -0.5, -0.6), (0.8, 0.6, 0.9)), (9, 9, 9), 4
    sigma = density_grid(system, box, res)
    scene = BakedScene.build(system, box, res, float(sigma.median()), img_id=img, sparse=sparse)
    mod = baked_sparse_tune if sparse else baked_tune
    common = dict(iters=4, batch=256, baked_step=0.05, seed=3, lr=0.05, img_id=img)
    tuned, curve = mod.distill(system, scene, [0, 2, 5], prune_at=(2,), upsample_at=(2,), **common)
    print(f"distill {'pool' if sparse else 'dense'} with a prune and an upsampling before iteration 2: {['%.3e' % c for c in curve]}")
    assert len(curve) == 4 and np.isfinite(curve).all()
    assert tuned.resolution == (17, 17, 17) and tuned.sparse == sparse
    plain, plain_curve = mod.distill(system, scene, [0, 2, 5], upsample_at=(2,), **common)
    assert curve[0] == plain_curve[0] and plain.resolution == tuned.resolution  # (the first loss is formed before any gradient)
    # (j) with prune_at empty nothing changes and nothing is launched.  Bit for bit where a call is the same bits every run: with
    # ONE ray a batch the backward's float atomics are issued by one thread in program order, so the whole loop is deterministic, and
    # the loss curve and every tensor of the returned scene are torch.equal to those of a call without the argument
    tensors = lambda s: [s.grid, s.occupancy.words] + ([s.slots, s.bricks] if s.sparse else [])
    one = dict(common, batch=1)
    p, cp = mod.distill(system, scene, [0, 2, 5], **one)
    q, cq = mod.distill(system, scene, [0, 2, 5], prune_at=(), prune_weight=None, **one)
    assert cp == cq and len(cp) == 4 and all(torch.equal(x, y) for x, y in zip(tensors(p), tensors(q)))
    assert not torch.equal(p.grid, scene.grid)  # (the four steps did move the scene)
    # At 256 rays a batch the sums over rays are float atomics in the order of arrival (the one baked entry point whose bits depend
    # on the run: DESIGN.md 2.34), so two runs of the SAME call differ in the last bits after the first loss.  Exact there: the first
    # loss (formed before any gradient) and the number of calls into the library (upnerf_amd._lib.CALLS counts every checked one);
    # the rest of the curve and the scene's points to the bound tests/test_hip_baked_tune.py holds two launches of that atomic sum
    # to, 1e-4 of the largest magnitude; the table and the bits exactly
    from upnerf_amd import _lib
    n0 = _lib.CALLS[0]
    a, ca = mod.distill(system, scene, [0, 2, 5], **common)
    n1 = _lib.CALLS[0]
    b, cb = mod.distill(system, scene, [0, 2, 5], prune_at=(), prune_weight=None, **common)
    n2 = _lib.CALLS[0]
    ga, gb = a.grid.float(), b.grid.float()
    apart, scale = float((ga - gb).abs().max()), float(ga.abs().max())
    print(f"without prune_at: {n1 - n0} library calls either way; curves equal to the bit: {ca == cb}, apart by {max(abs(x - y) for x, y in zip(ca, cb)):.2e}; "
          f"scenes equal to the bit: {torch.equal(a.grid, b.grid)}, apart by {apart:.2e} of {scale:.2e}")
    assert n2 - n1 == n1 - n0 and ca[0] == cb[0] and a.resolution == b.resolution == scene.resolution
    assert max(abs(x - y) for x, y in zip(ca, cb)) <= 1e-4 * max(ca)
    assert scale > 0 and apart <= 1e-4 * scale
    assert all(torch.equal(x, y) for x, y in zip(tensors(a)[1:], tensors(b)[1:]))
    with pytest.raises(ValueError):
        mod.distill(system, scene, [0, 2, 5], prune_at=(4,), **common)
    with pytest.raises(ValueError):
        mod.distill(system, scene, [0, 2, 5], prune_at=(1, 1), **common)
