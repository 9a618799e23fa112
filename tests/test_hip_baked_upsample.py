"""Doubling a baked scene's resolution on the GPU (csrc/baked_reg.hip: upnerf_baked_upsample, upnerf_brick_upsample_mark / _fill;
upnerf_amd/baked_reg.py).

The kernels are held bit for bit to the numpy float32 / float16 restatement tests/baked_upsample_ref.py (points and occupancy
words), the sparse route bit for bit to the dense route's sparsify().  The render of the refined scene is held to the PARENT's fp64
restatement: within render_gate -- the bound of what the rounding of the child's stored values can change, checked on the CPU in
tests/test_baked_upsample_cpu.py -- plus the fp32 marcher's own gate on the child scene (baked_ref / baked_sh_ref: the marcher
against its restatement), since the picture comes out of the fp32 marcher.  How large each part is, per ray on the colours of
the hit rays (median, largest; the colours are of order 1):
    degree 0      child roundings 2.0e-7 .. 2.4e-7, 3.4e-7      the marcher's own 5.7e-6 .. 6.6e-6, 9.5e-6
    degree 1, 2   child roundings 8.7e-4 .. 1.3e-3, 1.4e-3      the marcher's own 1.0e-5 .. 1.6e-5, 1.9e-5
At degree 0 the marcher's part is about 25 times the other: the test there holds the refined picture to the parent's fp64 picture
to about 1e-5, which a misplaced, unhalved or wrongly pruned child (errors of 1e-2 and more) cannot meet, but which does not
resolve the children's last-bit roundings -- those are held bit for bit by the first test.  At degree 1, 2 the child part, the
fp16 rounding of the coefficients, is the larger by 70.  The five grids are baked_tv_ref.GRIDS."""
import numpy as np
import pytest
import torch

import baked_cases as cases
import baked_ref as br
import baked_sh_ref as sh
import baked_sparse_ref as sr
import baked_tune_ref as tr
import baked_tv_ref as tvr
import baked_upsample_ref as ur
from baked_cases import dev

pytestmark = pytest.mark.gpu

TINY = float(ur.TINY)


def scene_of(name, degree):
    return cases.scene_of((__name__, name, degree), lambda: cases.build(*ur.parents(name, degree), degree))


def host(t):
    return t.detach().cpu().numpy()


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("name", list(tvr.GRIDS))
def test_dense_and_sparse_upsample_are_the_restatement_bit_for_bit(name, degree):
    parent, level = ur.parents(name, degree)
    scene = scene_of(name, degree)
    up = scene.upsample()
    want = ur.upsample(parent, degree, level)
    Nx, Ny, Nz = scene.resolution
    assert up.resolution == (2 * Nx - 1, 2 * Ny - 1, 2 * Nz - 1) and not up.sparse and up.sh_degree == degree
    assert up.level == scene.level and np.array_equal(np.asarray(up.bounds), np.asarray(scene.bounds))
    got = host(up.grid)
    assert same_bytes(got, want), int((got.view(np.uint8) != want.view(np.uint8)).sum())
    sigma = ur.stored(want, degree)[..., -1]
    assert np.array_equal(host(up.occupancy.words).view(np.uint32), sr.words(sr.dense_cell_bits(sigma)))
    assert ((sigma == 0) | (sigma >= np.float32(level))).all() and (sigma > 0).any()  # no kept child below the scene's level
    # pool to pool: the sparse route gives the dense route's sparsify(), byte for byte
    a, b = scene.sparsify().upsample(), up.sparsify()
    assert a.sparse and a.n_bricks == b.n_bricks >= 1 and a.resolution == b.resolution and a.sh_degree == degree
    for what in ("pool", "slots", "bricks"):
        assert same_bytes(host(getattr(a, what)), host(getattr(b, what))), (name, degree, what)
    assert same_bytes(host(a.occupancy.words), host(b.occupancy.words))
    again = scene.sparsify().upsample()
    assert same_bytes(host(again.pool), host(a.pool))
    # another level prunes the children there
    loose = scene.upsample(level=TINY)
    assert same_bytes(host(loose.grid), ur.upsample(parent, degree, TINY)) and loose.level == TINY
    assert same_bytes(host(scene.sparsify().upsample(level=TINY).pool), host(loose.sparsify().pool))


@pytest.mark.parametrize("degree", [0, 2])
def test_upsample_twice_on_the_single_cell(degree):
    parent, level = ur.parents("cell", degree)
    scene = scene_of("cell", degree)
    twice = scene.upsample().upsample()
    want = ur.upsample(ur.upsample(parent, degree, level), degree, level)
    assert twice.resolution == (5, 5, 5) and same_bytes(host(twice.grid), want)
    sparse = scene.sparsify().upsample().upsample()
    assert same_bytes(host(sparse.pool), host(twice.sparsify().pool)) and sparse.resolution == (5, 5, 5)


@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("name", ["blob", "big"])
def test_render_of_the_upsampled_scene_is_the_parents_within_the_gate(name, degree):
    parent, _ = ur.parents(name, degree)
    scene = scene_of(name, degree)
    rays = np.concatenate([br.make_rays(), tr.extra_rays(tvr.GRIDS[name]()[0])])
    dt = sh.steps(tvr.GRIDS[name]()[0])["cell"]
    child = ur.upsample(parent, degree, ur.TINY)
    rgb_p, depth_p, op_p = tr.render64(ur.numbers(parent, degree), degree, br.BOUNDS, rays, dt)  # stop = 0
    g_rgb, g_depth, g_op = ur.render_gate(child, parent, degree, br.BOUNDS, rays, dt)
    own = br.render(child, br.BOUNDS, rays, dt) if degree == 0 else sh.render(child, degree, br.BOUNDS, rays, dt)  # the marcher's own gates
    up = scene.upsample(level=TINY)
    for what, s in (("dense", up), ("sparse", scene.sparsify().upsample(level=TINY))):
        out = s.render(dev(rays), dt)
        torch.cuda.synchronize()
        worst = 0.0
        for k, want, gate in (("rgb", rgb_p, g_rgb + own["gate_rgb"]), ("depth", depth_p, g_depth + own["gate_depth"]),
                              ("opacity", op_p, g_op + own["gate_opacity"])):
            got = host(out[k]).astype(np.float64)
            err = np.abs(got - want)
            assert (err <= gate).all(), (name, degree, what, k, np.argwhere(err > gate)[:5], float(err.max()))
            worst = max(worst, float((err / np.maximum(gate, 1e-300))[gate > 0].max(initial=0.0)))
        print(f"{name} degree {degree} {what}: worst err / gate {worst:.3f}; the child's roundings alone allow up to {float(g_rgb.max()):.3e}")
    assert (op_p > 1e-3).sum() >= 30


@pytest.mark.parametrize("sparse", [False, True])
def test_tuner_upsampled_doubles_the_cells_and_resets_adam(sparse):
    scene = scene_of("blob", 0)
    scene = scene.sparsify() if sparse else scene
    tuner = (scene.tune_pool if sparse else scene.tune)(0.02, tv_sigma=0.1)
    rays = dev(br.make_rays())
    rays = rays[torch.isfinite(rays).all(1) & (rays[:, 7] > rays[:, 6])]
    target = torch.full((rays.shape[0], 3), 0.5, device="cuda")
    tuner.step(rays, target, 0.1)
    assert tuner.t == 1
    finer = tuner.upsampled()
    assert type(finer) is type(tuner) and finer.t == 0 and finer.lr == tuner.lr and finer.tv_sigma == 0.1 and finer.betas == tuner.betas
    assert finer.occupancy.dims == tuple(2 * c for c in tuner.occupancy.dims)
    assert float(finer.m.abs().max()) == 0.0 and float(finer.v.abs().max()) == 0.0
    loss = finer.step(rays, target, 0.1)
    assert bool(torch.isfinite(loss)) and finer.t == 1 and finer.scene().sparse == sparse


@pytest.fixture(scope="module")
def system():
    return cases.make_system()


@pytest.mark.parametrize("sparse", [False, True])
def test_distill_with_one_upsampling_returns_the_finer_scene(system, sparse):
    from upnerf_amd import baked_sparse_tune, baked_tune
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.geometry import density_grid
    box, res, img = ((-0.7, -0.5, -0.6), (0.8, 0.6, 0.9)), (9, 9, 9), 4
    sigma = density_grid(system, box, res)
    scene = BakedScene.build(system, box, res, float(sigma.median()), img_id=img, sparse=sparse)
    mod = baked_sparse_tune if sparse else baked_tune
    tuned, curve = mod.distill(system, scene, [0, 2, 5], iters=6, batch=256, baked_step=0.05, seed=3, lr=0.05, img_id=img,
                               tv=(1e-3, 1e-3), upsample_at=(3,))
    print(f"distill {'pool' if sparse else 'dense'} with tv and one upsampling: {['%.3e' % c for c in curve]}")
    assert len(curve) == 6 and np.isfinite(curve).all()
    assert tuned.resolution == (17, 17, 17) and tuned.sparse == sparse
    plain = mod.distill(system, scene, [0, 2, 5], iters=2, batch=256, baked_step=0.05, seed=3, lr=0.05, img_id=img)
    assert plain[0].resolution == scene.resolution and abs(plain[1][0] - curve[0]) <= 1e-5 * curve[0]  # the defaults are as before
    with pytest.raises(ValueError):
        mod.distill(system, scene, [0, 2, 5], iters=2, batch=64, baked_step=0.05, img_id=img, upsample_at=(2,))
