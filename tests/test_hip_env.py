"""The environment map on the GPU (csrc/env.hip; upnerf_amd/baked_env.py).

upnerf_env_composite and upnerf_env_composite_bwd are held to the fp64 restatement tests/env_ref.py within its derived gates on
every direction family at E = 1, 2 and 5 (the comparisons are tests/test_env_cpu.py's, which holds the kernels' host bodies to the
same gates); a constant map is held bit for bit to the marcher's own flat background; upnerf_env_rays to the node formula exactly
and to the fp64 slab exit; upnerf_env_seam to the lowest face's bytes; and the plumbing -- build, save / load, sparsify, upsample,
the tuners, render_path, the localiser -- to the pieces it is made of.  The system is the synthetic one of the baked family's
tests (tests/test_hip_tsdf.py: make_system)."""
import numpy as np
import pytest
import torch

import baked_pose_ref as pr
import baked_ref as br
import env_ref as er
from test_env_cpu import BOXES, SIZES, check_against_gates

pytestmark = pytest.mark.gpu

_CACHE = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def environment(env):
    from upnerf_amd.baked_env import Environment
    return Environment.from_array(dev(env))


# ---- the composite and its backward against fp64 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", SIZES)
def test_composite_and_backward_are_within_the_gates_on_every_family(E):
    from upnerf_amd import baked_env
    env = er.random_map(E, seed=E)
    envd = environment(env)
    for name, dirs in er.families(E).items():
        rays, opacity, rgb_in, g_out = er.problem(E, name, dirs)
        R = len(rays)
        r, o, c, g = dev(rays).requires_grad_(True), dev(opacity).requires_grad_(True), dev(rgb_in).requires_grad_(True), dev(g_out)
        out = envd.composite(r, c, o)
        g_op, g_rays = baked_env.composite_backward(envd.env, r.detach(), o.detach(), g)
        worst = check_against_gates(E, name, rays, opacity, rgb_in, g_out, out.detach().cpu().numpy(), g_op.cpu().numpy(), g_rays.cpu().numpy(),
                                    env, "gpu")
        print(f"E {E} {name}: {R} directions, worst err / gate " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        # autograd through Environment.composite gives the kernel's outputs (g_rgb is g_out itself)
        out.backward(g)
        assert torch.equal(r.grad.view(torch.int32), g_rays.view(torch.int32)) and torch.equal(o.grad.view(torch.int32), g_op.view(torch.int32))
        assert torch.equal(c.grad, g)
        # two runs, and launches cut at odd row counts, give the same bits; in place is allowed
        again = envd.composite(r.detach(), c.detach(), o.detach())
        assert torch.equal(again.view(torch.int32), out.detach().view(torch.int32))
        cuts = [0, 1, min(R, 8), min(R, 35), R]
        parts = [envd.composite(r.detach()[a:b].clone(), c.detach()[a:b].clone(), o.detach()[a:b].clone()) for a, b in zip(cuts, cuts[1:]) if b > a]
        assert torch.equal(torch.cat(parts).view(torch.int32), out.detach().view(torch.int32))
        gparts = [baked_env.composite_backward(envd.env, r.detach()[a:b].clone(), o.detach()[a:b].clone(), g[a:b].clone())[1] for a, b in zip(cuts, cuts[1:]) if b > a]
        assert torch.equal(torch.cat(gparts).view(torch.int32), g_rays.view(torch.int32))
        inplace = c.detach().clone()
        envd.composite_(r.detach().contiguous(), inplace, o.detach())
        assert torch.equal(inplace.view(torch.int32), out.detach().view(torch.int32))
        # lookup is the composite at opacity 0 on black
        look = envd.lookup(dev(rays[:, 3:6]))
        ref = er.lookup(env, rays[:, 3:6])
        assert (np.abs(look.cpu().numpy() - ref["rgb"]) <= ref["d_rgb"] + er.U * np.abs(ref["rgb"])).all()


# ---- a constant map is the marcher's flat background, bit for bit -----------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("degree", [0, 2])
@pytest.mark.parametrize("name", ["blob", "corners"])
def test_a_constant_map_is_the_flat_background_bit_for_bit(name, degree, sparse):
    """(Rays whose direction is not finite or all zero are left out: there the marcher shows `background` and the map shows 0.)"""
    from test_hip_baked_sparse import dense_scene
    scene = dense_scene(name, degree)
    scene = scene.sparsify() if sparse else scene
    rays = br.make_rays()
    d = rays[:, 3:6]
    rays = dev(rays[np.isfinite(rays).all(1) & d.any(1)])
    assert len(rays) >= 50
    step = 0.05
    for c in (0.0, 1.0, 0.3):
        for E in (1, 3):
            env = np.zeros((6, E + 1, E + 1, 4), np.float32)
            env[..., :3] = np.float32(c)
            with_env = scene.with_environment(environment(env))
            assert scene.env is None and with_env.env is not None
            got, want = with_env.render(rays, step, background=0.77), scene.render(rays, step, background=c)
            for k in ("rgb", "depth", "opacity"):
                assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (c, E, k)
    assert int((want["opacity"] > 0.05).sum()) > 10 and int((want["opacity"] < 0.5).sum()) > 10


# ---- node rays and the seam ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", SIZES)
def test_node_rays_are_the_node_formula_and_the_slab_exit(E):
    from upnerf_amd import baked_env
    n = 6 * (E + 1) ** 2
    for bname, box in BOXES.items():
        ref = er.node_rays(E, box, 9.0)
        rows = baked_env.node_rays(box, E, 9.0, 0, n, "cuda").cpu().numpy()
        assert np.array_equal(rows[:, :6].astype(np.float64), ref["rays"][:, :6]) and (rows[:, 7] == 9.0).all()
        err = np.abs(rows[:, 6].astype(np.float64) - ref["rays"][:, 6])
        assert (err <= ref["gate_near"]).all() and (rows[:, 6] > 0).all()
        assert np.array_equal(rows[er.owners(E)], rows)  # copies of shared nodes carry identical rows
        cuts = sorted({0, 1, min(n, 7), n // 2, n})
        parts = [baked_env.node_rays(box, E, 9.0, a, b - a, "cuda").cpu().numpy() for a, b in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts).view(np.uint32), rows.view(np.uint32))
        print(f"E {E} box {bname}: near worst err / gate {float((err / ref['gate_near']).max()):.3f}")


@pytest.mark.parametrize("E", SIZES + (8,))
def test_the_seam_gives_every_copy_the_lowest_faces_bytes(E):
    from upnerf_amd import baked_env
    rng = np.random.default_rng(E)
    raw = rng.integers(0, 256, (6, E + 1, E + 1, 16), dtype=np.uint8)
    env = dev(raw).view(torch.float32)
    baked_env.seam(env)
    got = env.view(torch.uint8).cpu().numpy().reshape(-1, 16)
    want = raw.reshape(-1, 16)[er.owners(E)]
    assert np.array_equal(got, want)
    inner = ~er.edge_mask(E).reshape(-1)
    assert np.array_equal(got[inner], raw.reshape(-1, 16)[inner])  # interior nodes are untouched


# ---- the plumbing, on the synthetic system ---------------------------------------------------------------------------------------------------

BOX = ((-0.6, -0.5, -0.6), (0.6, 0.5, 0.6))
IMG = 4


@pytest.fixture(scope="module")
def system():
    from test_hip_tsdf import make_system
    return make_system()


def test_build_is_render_static_of_the_node_rays_and_everything_carries_the_map(system, tmp_path):
    from upnerf_amd import baked_env, novel_view as nv
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.static_scene import appearance_rows, near_far, render_static, static_keys
    E = 2
    n = 6 * (E + 1) ** 2
    hp = system.hparams
    old = hp["val.chunk_size"]
    hp["val.chunk_size"] = 20  # 54 node rays in chunks of 20, 20 and 14
    try:
        env = baked_env.Environment.build(system, BOX, E, img_id=IMG)
        far = max(near_far(system, i)[1] for i in range(6))
        keys = static_keys(system, 1)
        want = torch.zeros(n, 4, device="cuda")
        for n0 in range(0, n, 20):
            cnt = min(20, n - n0)
            rays = baked_env.node_rays(BOX, E, far, n0, cnt, "cuda")
            res = render_static(system, rays, appearance_rows(system, keys, IMG, cnt), 1)
            want[n0:n0 + cnt, :3] = res["s_rgb_fine"]
        own = torch.from_numpy(er.owners(E)).cuda()
        assert torch.equal(env.env.view(-1, 4).view(torch.int32), want[own].view(torch.int32))  # render_static, then the seam
        assert float(env.env[..., :3].abs().max()) > 0 and not bool(env.env[..., 3].any())
        assert torch.equal(env.env.view(-1, 4)[own], env.env.view(-1, 4))  # every seam copy is identical
        assert env.E == E and env.nbytes == n * 16 and env.device.type == "cuda"
        scene = BakedScene.build(system, BOX, (9, 9, 9), 0.5, img_id=IMG, env_size=E)
    finally:
        hp["val.chunk_size"] = old
    same = lambda s: s.env is not None and torch.equal(s.env.env.view(torch.int32), env.env.view(torch.int32))
    assert same(scene)
    path = str(tmp_path / "scene.npz")
    scene.save(path)
    assert same(BakedScene.load(path, "cuda"))
    sp = scene.sparsify()
    assert same(sp) and same(sp.densify()) and same(scene.upsample()) and same(sp.upsample())
    sp.save(path)
    loaded = BakedScene.load(path, "cuda")
    assert loaded.sparse and same(loaded)
    assert same(scene.tune(lr=1e-2).scene()) and same(scene.tune(lr=1e-2).upsampled().scene())
    if sp.n_bricks:
        assert same(sp.tune_pool(lr=1e-2).scene())
    assert scene.with_environment(None).env is None and same(scene)
    # a file as the parent commit's save wrote it: no `env` array, and it loads with env None
    bare = scene.with_environment(None)
    bare.save(path)
    with np.load(path) as f:
        assert set(f.files) == {"rgbs", "bounds", "level"}
    back = BakedScene.load(path, "cuda")
    assert back.env is None and torch.equal(back.rgbs, scene.rgbs)
    # render_path shows the environment with no new argument: frame by frame scene.render on the path's rays
    c = np.cos(0.3), np.sin(0.3)
    c2w = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 1.6]], [[c[0], 0, c[1], 0.4], [0, 1, 0, 0.1], [-c[1], 0, c[0], 1.5]]])
    K = torch.tensor([[22.0, 0, 11.6], [0, 21.0, 7.8], [0, 0, 1]])
    cam = nv.CameraPath.from_poses(c2w, [(0.1, 5.0), (0.2, 4.5)], 2, appearance=(1, 4), img_wh=(24, 16), K=K)
    out = nv.render_path(system, cam, chunk=100, outputs=("rgb_float",), baked=scene, baked_step=0.04)
    poses, nf = nv.path_poses(cam.key_c2w.cuda(), cam.key_near_far.cuda(), cam.u.cuda(), cam.mode)
    for f in range(2):
        rays, _ = nv.path_rays(poses, nf, cam.img_wh, cam.K, f * 384, 384)
        direct = scene.render(rays, 0.04)
        assert torch.equal(out["rgb_float"][f], direct["rgb"])
        flat = bare.render(rays, 0.04, background=0.0)
        assert torch.equal(direct["opacity"], flat["opacity"]) and torch.equal(direct["depth"], flat["depth"])
        assert torch.equal(direct["rgb"], scene.env.composite(rays, flat["rgb"], flat["opacity"]))
        assert not torch.equal(direct["rgb"], flat["rgb"])


# ---- tuning ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
def test_the_points_gradient_is_the_marchers_with_the_environments_opacity_term(sparse):
    """baked_tune.render / baked_sparse_tune.render with an environment send the points what upnerf_baked_render_bwd gives when
    called with g_opacity - g_rgb . env(d).  The inputs of the two launches are the same bits, so they differ by the order of the
    float atomic adds alone (two runs agree to rounding, not to the bit): the allowance is twice what two direct calls differ by,
    measured here, plus R u max |gradient| for a reordering of the at most R rays' sums into one point."""
    from upnerf_amd import baked_env, baked_sparse_tune, baked_tune
    from test_hip_baked_sparse import dense_scene
    E = 3
    env = environment(er.smooth_map(E, seed=2))
    scene = dense_scene("blob", 0).with_environment(env)
    rays = br.make_rays()
    rays = dev(rays[np.isfinite(rays).all(1) & rays[:, 3:6].any(1)])
    R = len(rays)
    rng = np.random.default_rng(3)
    g_rgb, g_op = dev(rng.normal(size=(R, 3)).astype(np.float32)), dev(rng.normal(size=R).astype(np.float32))
    step = 0.05
    if sparse:
        scene = scene.sparsify()
        params = baked_sparse_tune.PoolParams.of(scene)
        out = baked_sparse_tune.render(params, rays, step, background=0.9)
    else:
        params = baked_tune.SceneParams.of(scene)
        out = baked_tune.render(params, rays, step, background=0.9)
    assert params.env is env
    assert torch.equal(out["rgb"].detach(), scene.render(rays, step)["rgb"])
    ((out["rgb"] * g_rgb).sum() + (out["opacity"] * g_op).sum()).backward()
    got = params.rgbs.grad
    op = out["opacity"].detach()
    total = g_op + baked_env.composite_backward(env.env, rays, op, g_rgb)[0]  # g_opacity - g_rgb . env(d)
    ref64 = er.composite_bwd(env.env.cpu().numpy(), rays.cpu().numpy(), op.cpu().numpy(), g_rgb.cpu().numpy())
    assert (np.abs((total - g_op).cpu().numpy() - ref64["g_opacity"]) <= ref64["gate_opacity"] + er.U * np.abs(total.cpu().numpy())).all()
    if sparse:
        direct = lambda: baked_sparse_tune.backward(params.rgbs.detach(), params, rays, step, 0.0, 0.0, g_rgb, g_opacity=total)
    else:
        direct = lambda: baked_tune.backward(params.rgbs.detach(), 0, scene.occupancy, scene.bounds, rays, step, 0.0, 0.0, g_rgb, g_opacity=total)
    a, b = direct(), direct()
    room = 2 * float((a - b).abs().max()) + R * er.U * float(a.abs().max())
    assert float(a.abs().max()) > 1e-2 and float((got - a).abs().max()) <= room, (float((got - a).abs().max()), room)
    total = g_op  # the same call without the environment's term: far outside the allowance, so the comparison sees the term
    assert float((direct() - a).abs().max()) > 1e-2 * float(a.abs().max()) > 10 * room


def test_a_tuner_step_with_an_environment_lowers_the_loss():
    """A 4^3-point scene in front of a smooth environment; the targets are its own render with the sigmas scaled by 0.5.  Ten
    steps of BakedTuner at lr = 0.05 lower the loss, and the first loss is that of scene.render (the environment included)."""
    from upnerf_amd.baked import BakedScene
    rng = np.random.default_rng(0)
    sigma = rng.uniform(2.0, 6.0, (4, 4, 4)).astype(np.float32)
    rgb = rng.uniform(0, 1, (4, 4, 4, 3)).astype(np.float32)
    env = environment(er.smooth_map(4, seed=5))
    truth = BakedScene.from_grids(dev(sigma * 0.5), dev(rgb), br.BOUNDS, 0.0).with_environment(env)
    scene = BakedScene.from_grids(dev(sigma), dev(rgb), br.BOUNDS, 0.0).with_environment(env)
    rays = br.make_rays(R=267)
    rays = dev(rays[np.isfinite(rays).all(1) & rays[:, 3:6].any(1)])
    target = truth.render(rays, 0.05)["rgb"]
    tuner = scene.tune(lr=0.05)
    losses = torch.stack([tuner.step(rays, target, 0.05) for _ in range(10)]).cpu().numpy()
    diff = scene.render(rays, 0.05)["rgb"] - target
    first = float((diff * diff).mean())  # (the tuner's own expression on the same bits)
    print(f"loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert float(losses[0]) == first and first > 0 and losses[-1] < losses[0] and tuner.scene().env is env


# ---- localising against the sky alone ----------------------------------------------------------------------------------------------------------

def test_the_localiser_recovers_a_rotation_from_the_sky_alone():
    """The test that cannot pass without the environment's ray gradient: an EMPTY box (the marcher gives every ray opacity 0 and
    no gradient), a smooth E = 8 map, one 16 x 12 photograph from the box centre, the pose SKY_ROT = 0.04 rad off about two axes.
    The fp64 loop of the restatement (env_ref.sky_loop, the same index draws, SKY_ITERS = 30 iterations of 96 pixels at lr = 0.004)
    must bring the rotation error to a quarter or less -- it brings it to 0.034 of its initial value (loss 3.7e-4 -> 1.7e-6) -- and
    the GPU's loop to a half or less: the factor of two is the room for the fp32 and fp64 Adam trajectories to part (the rule of
    tests/test_hip_baked_pose.py)."""
    from upnerf_amd import baked_pose
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.camera import get_rays
    env, truth, init = er.sky_problem()
    W, H = er.SKY_WH
    gen = torch.Generator(device="cpu").manual_seed(er.SKY_SEED)
    batches = [torch.randint(0, H * W, (er.SKY_BATCH,), generator=gen).numpy() for _ in range(er.SKY_ITERS)]
    rays64 = pr.image_rays(truth[0], er.SKY_K, er.SKY_WH, er.SKY_NEAR_FAR)
    zero = np.zeros(len(rays64))
    targets64 = er.composite(env, rays64, zero, np.zeros((len(rays64), 3)))["rgb"].reshape(1, H, W, 3)
    se3_ref, curve = er.sky_loop(env, targets64, init, er.SKY_ITERS, er.SKY_LR, batches)
    rot0 = pr.pose_error(init, truth)[0]
    rot_ref = pr.pose_error(pr.refined(se3_ref, init), truth)[0]
    assert rot_ref <= rot0 / 4, rot_ref / rot0

    box = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    scene = BakedScene.from_grids(torch.zeros(2, 2, 2, device="cuda"), None, box, 0.0).with_environment(environment(env))
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    dirs = baked_pose.pixel_directions(xx.reshape(-1), yy.reshape(-1), er.SKY_K)
    nf = torch.tensor(er.SKY_NEAR_FAR, device="cuda").expand(H * W, 2)
    target_rays = torch.cat(get_rays(dirs, dev(truth[0].astype(np.float32))) + (nf,), 1).contiguous()
    shown = scene.render(target_rays, 0.1)
    assert not bool(shown["opacity"].any())
    targets = shown["rgb"].view(1, H, W, 3).contiguous()
    loc = baked_pose.BakedLocaliser(scene, targets, er.SKY_K, dev(init.astype(np.float32)), er.SKY_NEAR_FAR, lr=er.SKY_LR)
    gen = torch.Generator(device="cpu").manual_seed(er.SKY_SEED)
    losses = torch.stack([loc.step(er.SKY_BATCH, 0.1, gen) for _ in range(er.SKY_ITERS)]).cpu().numpy()
    rot = pr.pose_error(loc.poses().cpu().numpy(), truth)[0]
    print(f"fp64 loop rotation {rot0:.4f} -> {rot_ref:.4f}, loss {curve[0]:.3e} -> {curve[-1]:.3e}; GPU rotation -> {rot:.4f}, "
          f"loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert rot <= rot0 / 2
    # without the environment the same photograph gives the localiser nothing
    bare = baked_pose.BakedLocaliser(scene.with_environment(None), targets, er.SKY_K, dev(init.astype(np.float32)), er.SKY_NEAR_FAR, lr=er.SKY_LR)
    gen = torch.Generator(device="cpu").manual_seed(er.SKY_SEED)
    bare.step(er.SKY_BATCH, 0.1, gen)
    assert not bool(bare.se3.detach().any())
