"""The baked scenes' Python layer, dense grid or brick pool, held to ITSELF across a rewrite (upnerf_amd/baked*.py; DESIGN.md
2.40): the launches every public call makes, in order and with their units; the dense marcher against the pool marcher; and what
each kind of scene exposes.  Public names only.  The launch sequences below were recorded on the commit before the layout object
existed (2026-10-21, MI355X) and are literal: a call that gains, loses or reorders a launch fails here.

The scene: CELLS[1] of tests/test_hip_baked_sparse.py (9 x 17 x 5 cells, 2 x 3 x 1 bricks, ragged on every axis) with its "seeded"
pattern -- none of that file's patterns has an empty brick AND two occupied bricks sharing a face (each occupies all of its bricks,
one, or none), so the pattern's points of y > 14 are left empty here: the bricks by = 0 and by = 1 are occupied (four, sharing
faces in x and y) and by = 2 is empty (two).  64 rays of baked_ref.make_rays: a miss, a NaN row and far <= near among them."""
import numpy as np
import pytest
import torch

import baked_cases as cases
import baked_ref as br
from baked_cases import dev
from test_hip_baked_sparse import CELLS, pattern

pytestmark = pytest.mark.gpu

CELL = CELLS[1]
STEP = 0.05
_CACHE = {}


def rays():
    if "rays" not in _CACHE:
        _CACHE["rays"] = dev(br.make_rays(R=64))
    return _CACHE["rays"]


def environment():
    from upnerf_amd.baked_env import Environment
    return Environment.from_array(np.random.RandomState(3).uniform(0, 1, (6, 3, 3, 3)).astype(np.float32))  # size 2


def scene_of(degree, sparse=False):
    """The test scene at a degree, dense or its sparsify(); built once and never changed."""
    def make():
        from upnerf_amd.baked import BakedScene, sphere_directions
        Cx, Cy, Cz = CELL
        rng = np.random.RandomState(7)
        sigma = np.zeros((Cz + 1, Cy + 1, Cx + 1), np.float32)
        sigma[:Cz, :Cy, :Cx] = np.where(pattern(CELL, "seeded"), rng.uniform(2, 30, (Cz, Cy, Cx)), 0)
        sigma[:, 15:] = 0
        if degree == 0:
            rgb = rng.uniform(0, 1, sigma.shape + (3,)).astype(np.float32)
            return BakedScene.from_grids(dev(sigma), dev(rgb), br.BOUNDS, 0.0)
        dirs = sphere_directions(12)
        rgb = rng.uniform(0, 1, (12,) + sigma.shape + (3,)).astype(np.float32)
        return BakedScene.from_direction_grids(dev(sigma), dev(rgb), dirs, br.BOUNDS, 0.0, sh_degree=degree)
    return cases.scene_of((__name__, degree), make, sparse)


# ---- 1. the launches -----------------------------------------------------------------------------------------------------------------

def record(monkeypatch, calls):
    """{label: [(TIMER name, units), ...]} of the launches each of `calls` makes through TIMER.run."""
    from upnerf_amd import ops
    log = []
    run = ops.TIMER.run

    def spy(name, fn, units=0):
        log.append((name, int(units)))
        return run(name, fn, units=units)

    monkeypatch.setattr(ops.TIMER, "run", spy)
    out = {}
    for label, call in calls:
        del log[:]
        call()
        out[label] = list(log)
    torch.cuda.synchronize()
    return out


def step_calls():
    target = dev(np.random.RandomState(5).uniform(0, 1, (64, 3)).astype(np.float32))
    calls = []
    for sparse in (False, True):
        for degree in (0, 2):
            for tv in (False, True):
                for env in (False, True):
                    scene = scene_of(degree, sparse).with_environment(environment() if env else None)
                    kw = dict(tv_sigma=1e-3, tv_colour=1e-3) if tv else {}
                    tuner = scene.tune_pool(1e-2, **kw) if sparse else scene.tune(1e-2, **kw)
                    label = f"step {'pool' if sparse else 'dense'} degree {degree}{' tv' if tv else ''}{' env' if env else ''}"
                    calls.append((label, lambda tuner=tuner: tuner.step(rays(), target, STEP)))
    return calls


def scene_calls():
    calls = []
    for sparse in (False, True):
        for degree in (0, 2):
            scene = scene_of(degree, sparse)
            for what, call in (("render", lambda s=scene: s.render(rays(), STEP)), ("visibility", lambda s=scene: s.visibility(rays(), STEP)),
                               ("prune", lambda s=scene: s.prune(rays(), STEP)), ("upsample", lambda s=scene: s.upsample()),
                               ("sparsify", lambda s=scene: s.sparsify()), ("densify", lambda s=scene: s.densify())):
                calls.append((f"{what} {'pool' if sparse else 'dense'} degree {degree}", call))
    return calls


SEQUENCES = {
    'step dense degree 0': [('baked_render', 64), ('baked_render_bwd', 64), ('adam', 4320), ('baked_project', 1080)],
    'step dense degree 0 env': [
        ('baked_render', 64), ('env_composite', 64), ('env_composite_bwd', 64), ('baked_render_bwd', 64), ('adam', 4320),
        ('baked_project', 1080)],
    'step dense degree 0 tv': [('baked_render', 64), ('baked_render_bwd', 64), ('baked_tv', 4320), ('adam', 4320), ('baked_project', 1080)],
    'step dense degree 0 tv env': [
        ('baked_render', 64), ('env_composite', 64), ('env_composite_bwd', 64), ('baked_render_bwd', 64), ('baked_tv', 4320), ('adam', 4320),
        ('baked_project', 1080)],
    'step dense degree 2': [('baked_sh_render', 64), ('baked_render_bwd', 64), ('adam', 30240), ('baked_project', 1080), ('baked_sh_pack', 1080)],
    'step dense degree 2 env': [
        ('baked_sh_render', 64), ('env_composite', 64), ('env_composite_bwd', 64), ('baked_render_bwd', 64), ('adam', 30240),
        ('baked_project', 1080), ('baked_sh_pack', 1080)],
    'step dense degree 2 tv': [
        ('baked_sh_render', 64), ('baked_render_bwd', 64), ('baked_tv', 29160), ('baked_tv', 1080), ('adam', 30240), ('baked_project', 1080),
        ('baked_sh_pack', 1080)],
    'step dense degree 2 tv env': [
        ('baked_sh_render', 64), ('env_composite', 64), ('env_composite_bwd', 64), ('baked_render_bwd', 64), ('baked_tv', 29160),
        ('baked_tv', 1080), ('adam', 30240), ('baked_project', 1080), ('baked_sh_pack', 1080)],
    'step pool degree 0': [
        ('baked_sparse_render', 64), ('baked_sparse_render_bwd', 64), ('brick_face_sum', 6176), ('adam', 11664), ('baked_project', 2916)],
    'step pool degree 0 env': [
        ('baked_sparse_render', 64), ('env_composite', 64), ('env_composite_bwd', 64), ('baked_sparse_render_bwd', 64), ('brick_face_sum', 6176),
        ('adam', 11664), ('baked_project', 2916)],
    'step pool degree 0 tv': [
        ('baked_sparse_render', 64), ('baked_sparse_render_bwd', 64), ('baked_tv', 11664), ('brick_face_sum', 6176), ('adam', 11664),
        ('baked_project', 2916)],
    'step pool degree 0 tv env': [
        ('baked_sparse_render', 64), ('env_composite', 64), ('env_composite_bwd', 64), ('baked_sparse_render_bwd', 64), ('baked_tv', 11664),
        ('brick_face_sum', 6176), ('adam', 11664), ('baked_project', 2916)],
    'step pool degree 2': [
        ('baked_sparse_render', 64), ('baked_sparse_render_bwd', 64), ('brick_face_sum', 41688), ('brick_face_sum', 1544), ('adam', 81648),
        ('baked_project', 2916), ('baked_sh_pack', 2916)],
    'step pool degree 2 env': [
        ('baked_sparse_render', 64), ('env_composite', 64), ('env_composite_bwd', 64), ('baked_sparse_render_bwd', 64),
        ('brick_face_sum', 41688), ('brick_face_sum', 1544), ('adam', 81648), ('baked_project', 2916), ('baked_sh_pack', 2916)],
    'step pool degree 2 tv': [
        ('baked_sparse_render', 64), ('baked_sparse_render_bwd', 64), ('baked_tv', 78732), ('baked_tv', 2916), ('brick_face_sum', 41688),
        ('brick_face_sum', 1544), ('adam', 81648), ('baked_project', 2916), ('baked_sh_pack', 2916)],
    'step pool degree 2 tv env': [
        ('baked_sparse_render', 64), ('env_composite', 64), ('env_composite_bwd', 64), ('baked_sparse_render_bwd', 64), ('baked_tv', 78732),
        ('baked_tv', 2916), ('brick_face_sum', 41688), ('brick_face_sum', 1544), ('adam', 81648), ('baked_project', 2916),
        ('baked_sh_pack', 2916)],
    'render dense degree 0': [('baked_render', 64)],
    'visibility dense degree 0': [('baked_visibility', 64)],
    'prune dense degree 0': [('baked_visibility', 64), ('baked_prune', 1080), ('occ_build', 765)],
    'upsample dense degree 0': [('baked_upsample', 7315), ('occ_build', 6120)],
    'sparsify dense degree 0': [('brick_table', 6), ('brick_gather', 2916), ('brick_occ', 25)],
    'densify dense degree 0': [],
    'render dense degree 2': [('baked_sh_render', 64)],
    'visibility dense degree 2': [('baked_visibility', 64)],
    'prune dense degree 2': [('baked_visibility', 64), ('baked_prune', 1080), ('occ_build', 765)],
    'upsample dense degree 2': [('baked_upsample', 7315), ('occ_build', 6120)],
    'sparsify dense degree 2': [('brick_table', 6), ('brick_gather', 2916), ('brick_occ', 25)],
    'densify dense degree 2': [],
    'render pool degree 0': [('baked_sparse_render', 64)],
    'visibility pool degree 0': [('baked_visibility', 64), ('brick_face_max', 1544)],
    'prune pool degree 0': [
        ('baked_visibility', 64), ('brick_face_max', 1544), ('baked_prune', 2916), ('brick_occ', 25), ('brick_table', 6), ('brick_occ', 25)],
    'upsample pool degree 0': [('brick_upsample_mark', 30), ('brick_table', 30), ('brick_upsample_fill', 16767), ('brick_occ', 193)],
    'sparsify pool degree 0': [],
    'densify pool degree 0': [('brick_scatter', 2916), ('occ_build', 765)],
    'render pool degree 2': [('baked_sparse_render', 64)],
    'visibility pool degree 2': [('baked_visibility', 64), ('brick_face_max', 1544)],
    'prune pool degree 2': [
        ('baked_visibility', 64), ('brick_face_max', 1544), ('baked_prune', 2916), ('brick_occ', 25), ('brick_table', 6), ('brick_occ', 25)],
    'upsample pool degree 2': [('brick_upsample_mark', 30), ('brick_table', 30), ('brick_upsample_fill', 16767), ('brick_occ', 193)],
    'sparsify pool degree 2': [],
    'densify pool degree 2': [('brick_scatter', 2916), ('occ_build', 765)],
}


def test_every_public_call_makes_the_launches_it_made(monkeypatch):
    got = record(monkeypatch, step_calls() + scene_calls())
    assert sorted(got) == sorted(SEQUENCES)
    for label in SEQUENCES:
        assert got[label] == SEQUENCES[label], label


# ---- 2. dense against pool -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [0, 2])
def test_dense_and_pool_march_to_the_same_bits_and_one_ray_differentiates_to_the_same_bits(degree):
    from upnerf_amd import baked_sparse_tune, baked_tune
    dense, sparse = scene_of(degree), scene_of(degree, True)
    sides = ((baked_tune, baked_tune.SceneParams.of(dense), dense), (baked_sparse_tune, baked_sparse_tune.PoolParams.of(sparse), sparse))
    outs = [mod.render(params, rays(), STEP) for mod, params, _ in sides]
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in ("rgb", "depth", "opacity"))
    assert 0 < int((outs[0]["opacity"] > 0).sum()) < 64
    hit = int(outs[0]["opacity"].argmax())
    one = rays()[hit:hit + 1].contiguous()  # ONE ray: one thread orders every atomic add, so a run is deterministic
    g_rgb = torch.ones(1, 3, device="cuda")
    for mod, params, scene in sides:
        if mod is baked_tune:
            direct = lambda: mod.backward(scene.grid, degree, scene.occupancy, scene.bounds, one, STEP, 0.0, 0.0, g_rgb)
        else:
            direct = lambda: mod.backward(scene.pool, params, one, STEP, 0.0, 0.0, g_rgb)
        first, second = direct(), direct()
        first, second = ((first,), (second,)) if degree == 0 else (first, second)
        assert all(torch.equal(a, b) for a, b in zip(first, second))
        assert float(first[-1].abs().max()) > 0
        mod.render(params, one, STEP)["rgb"].sum().backward()
        assert all(torch.equal(t.grad, g) for t, g in zip(params.tensors, first))


# ---- 3. what a scene exposes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_attributes_of_the_six_kinds_of_scene_and_their_files(degree, sparse, tmp_path):
    from upnerf_amd.baked import BakedScene
    scene = scene_of(degree, sparse)
    Cx, Cy, Cz = CELL
    E = {0: 16, 1: 32, 2: 64}[degree]
    dtype, last = (torch.float32, 4) if degree == 0 else (torch.uint8, E)
    words = scene.occupancy.words.numel()
    assert scene.sparse is sparse and scene.sh_degree == degree and scene.resolution == (Cx + 1, Cy + 1, Cz + 1)
    assert scene.n_bricks == 4
    if sparse:
        assert scene.rgbs is None and scene.records is None and scene.grid is scene.pool
        assert scene.pool.dtype == dtype and tuple(scene.pool.shape) == (4, 9, 9, 9, last) and scene.pool.data_ptr() % E == 0
        assert scene.slots.dtype == torch.int32 and tuple(scene.slots.shape) == (1, 3, 2)
        slots = scene.slots.cpu().numpy()  # by = 0 and 1 occupied and sharing faces, by = 2 empty
        assert (slots[0, :2] >= 0).all() and (slots[0, 2] == -1).all()
        assert scene.bricks.dtype == torch.int32 and scene.bricks.tolist() == [0, 1, 2, 3]
        assert scene.nbytes == 4 * 729 * E + (6 + 4 + words) * 4
    else:
        assert scene.pool is None and scene.slots is None and scene.bricks is None
        assert (scene.rgbs is None) == (degree != 0) and (scene.records is None) == (degree == 0)
        assert scene.grid is (scene.records if degree else scene.rgbs)
        assert scene.grid.dtype == dtype and tuple(scene.grid.shape) == (Cz + 1, Cy + 1, Cx + 1, last) and scene.grid.data_ptr() % E == 0
        assert scene.nbytes == (Cz + 1) * (Cy + 1) * (Cx + 1) * E + words * 4
    if hasattr(BakedScene, "layout"):  # (the one name here that the commit the sequences were recorded on does not have)
        assert tuple(scene.layout.shape) == ((4, 9, 9, 9) if sparse else (Cz + 1, Cy + 1, Cx + 1))
    path = str(tmp_path / "scene.npz")
    scene.save(path)
    back = BakedScene.load(path)
    assert back.sparse is sparse and back.sh_degree == degree and back.resolution == scene.resolution and back.level == scene.level
    assert back.bounds == scene.bounds and back.nbytes == scene.nbytes
    assert back.grid.dtype == scene.grid.dtype and torch.equal(back.grid.view(torch.uint8), scene.grid.view(torch.uint8))
    assert torch.equal(back.occupancy.words, scene.occupancy.words)
    if sparse:
        assert torch.equal(back.slots, scene.slots) and torch.equal(back.bricks, scene.bricks)
