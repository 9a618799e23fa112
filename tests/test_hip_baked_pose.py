"""The baked marcher's ray gradient on the GPU (csrc/baked.hip: upnerf_baked_ray_bwd; upnerf_amd/baked_pose.py).

Reference: tests/baked_pose_ref.py -- fp64 numpy, brute force over every lattice sample, never a look at the occupancy bits; its
docstring derives the per-element gates from counts of roundings.  Every ray's row is written by its own thread from its own
registers, so two launches, and a launch cut into pieces, are held to equality of bits, and so is the sparse layout against the
dense one.

Grids, rays, upstream gradients and settings: those of tests/test_hip_baked_tune.py (67 rays: a full wave and a ragged one, misses
and non-finite rows among them, rows without an upstream gradient, then 64 identical rays and one ray inside a cell face)."""
import numpy as np
import pytest
import torch

import baked_cases as cases
import baked_pose_ref as pr
import baked_ref as br
import baked_sh_ref as sh
import baked_tune_ref as tr
from baked_cases import dev

pytestmark = pytest.mark.gpu

_CACHE = {}
SETTINGS = {"bg0-all": (0.0, 0.0, True), "bg1-stop-rgb": (1.0, 1e-3, False)}  # (those of tests/test_hip_baked_tune.py)


def rays_all(name):
    return cases.rays_all(sh.GRIDS[name]()[0])


def scene_of(name, degree, sparse=False):
    """(BakedScene, the numbers the reference differentiates: rgbs, or (k, sigma) of the stored records)."""
    points, level = sh.GRIDS[name]() if degree == 0 else sh.sh_grid(name, degree)
    scene = cases.scene_of((__name__, name, degree), lambda: cases.build(points, level, degree), sparse)
    return scene, points if degree == 0 else sh.unpack(points, degree)


def reference(name, degree, setting):
    """The fp64 restatement, computed once per case and never changed."""
    key = ("ref", name, degree, setting)
    if key not in _CACHE:
        bg, stop, rest = SETTINGS[setting]
        rays = rays_all(name)
        g_rgb, g_depth, g_op = tr.upstream(rays.shape[0])
        dt = sh.steps(sh.GRIDS[name]()[0])["cell"]
        _CACHE[key] = pr.ray_grad(scene_of(name, degree)[1], degree, br.BOUNDS, rays, dt, bg, stop, g_rgb, g_depth if rest else None,
                                  g_op if rest else None)
    return _CACHE[key]


def launch(name, degree, setting, sparse=False, rows=slice(None)):
    """upnerf_baked_ray_bwd on the rays `rows`, into a buffer filled with NaN (it is written, not added to): [R, 8] as numpy."""
    from upnerf_amd import baked_pose
    bg, stop, rest = SETTINGS[setting]
    rays = rays_all(name)
    g_rgb, g_depth, g_op = (dev(g[rows]) for g in tr.upstream(rays.shape[0]))
    dt = sh.steps(sh.GRIDS[name]()[0])["cell"]
    out = torch.full((len(rays[rows]), 8), float("nan"), device="cuda")
    got = baked_pose.ray_backward(scene_of(name, degree, sparse)[0], dev(rays[rows]), dt, bg, stop, g_rgb, g_depth if rest else None,
                                  g_op if rest else None, out=out)
    torch.cuda.synchronize()
    assert got is out
    return out.cpu().numpy()


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("name", list(sh.GRIDS))
def test_the_ray_gradient_is_within_its_gate_of_the_fp64_restatement(name, degree, sparse, setting):
    ref = reference(name, degree, setting)
    if SETTINGS[setting][1] > 0:
        assert ref["stop_margin"] > 0  # no ray ends on a sample that fp32 could place on the other side of `stop`
    got = launch(name, degree, setting, sparse)
    assert np.isfinite(got).all()
    val = got.astype(np.float64)
    err, gate = np.abs(val - ref["grad"]), ref["gate"]
    worst = float((err / np.maximum(gate, 1e-300))[gate > 0].max(initial=0.0))
    print(f"{name} degree {degree} {'sparse' if sparse else 'dense'} {setting}: {int((gate > 0).any(1).sum())} rays with a gradient, "
          f"largest entry {np.abs(ref['grad']).max():.3e}; worst err / gate {worst:.3f}")
    assert (val[gate == 0] == 0).all()
    assert (err <= gate).all(), (np.argwhere(err > gate)[:5], worst)
    rays, up = rays_all(name), tr.upstream(len(rays_all(name)))
    rest = SETTINGS[setting][2]
    zero = ~np.isfinite(rays).all(1) | ~(rays[:, 7] > rays[:, 6]) | ~(up[0].any(1) | (rest & (up[1] != 0)) | (rest & (up[2] != 0)))
    assert zero.sum() >= 5 and not got[zero].view(np.uint32).any()  # misses, rows without an upstream gradient: eight zeros
    assert (gate > 0).any(1).sum() >= 60 and np.abs(ref["grad"]).max() > 1e-2


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_two_runs_cut_launches_and_both_layouts_give_the_same_bits(degree):
    name, setting = "blob", "bg0-all"
    first = launch(name, degree, setting).view(np.uint32)
    assert np.array_equal(launch(name, degree, setting).view(np.uint32), first)
    R = len(first)
    for cuts in ((0, 1, 64, R), (0, 63, R), (0, 65, R)):  # launches of 1, 63 and the rest; of 63; of 65
        parts = [launch(name, degree, setting, rows=slice(a, b)).view(np.uint32) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts), first), cuts
    assert np.array_equal(launch(name, degree, setting, sparse=True).view(np.uint32), first)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("degree", [0, 2])
def test_autograd_render_is_the_marcher_and_its_backward_the_kernel(degree, sparse):
    """Fails without the feature: there is no module and no ray gradient."""
    from upnerf_amd import baked_pose
    dt = sh.steps(sh.GRIDS["blob"]()[0])["tenth"]
    scene = scene_of("blob", degree, sparse)[0]
    rays = dev(br.make_rays()).requires_grad_(True)
    out = baked_pose.render(scene, rays, dt, background=0.5, stop=1e-3)
    direct = scene.render(rays.detach(), dt, background=0.5, stop=1e-3)
    for k in ("rgb", "depth", "opacity"):
        assert torch.equal(out[k], direct[k]), k
    out["rgb"].sum().backward()
    want = baked_pose.ray_backward(scene, rays.detach(), dt, 0.5, 1e-3, torch.ones(67, 3, device="cuda"))
    assert rays.grad is not None and rays.grad.shape == (67, 8) and torch.equal(rays.grad, want)
    assert float(want.abs().max()) > 0
    # all three outputs in the loss
    rays2 = dev(br.make_rays()).requires_grad_(True)
    out2 = baked_pose.render(scene, rays2, dt, background=0.5, stop=1e-3)
    g_rgb, g_depth, g_op = (dev(g) for g in tr.upstream(67))
    ((out2["rgb"] * g_rgb).sum() + (out2["depth"] * g_depth).sum() + (out2["opacity"] * g_op).sum()).backward()
    assert torch.equal(rays2.grad, baked_pose.ray_backward(scene, rays2.detach(), dt, 0.5, 1e-3, g_rgb, g_depth, g_op))
    with pytest.raises(ValueError):
        baked_pose.render(None, rays, dt)
    with pytest.raises(ValueError):
        baked_pose.ray_backward(scene, rays.detach(), dt, 0.0, 0.0, torch.ones(66, 3, device="cuda"))


@pytest.mark.parametrize("degree", [0, 2])
def test_the_chain_to_se3_is_the_fp64_chain(degree):
    """se3.grad of sum g . outputs through refine_and_get_rays and baked_pose.render against the restated ray gradient times the
    fp64 pose-ray Jacobian.  The gate is the ray gradient's, propagated through |J| (the restated rays are the kernel's rays
    rounded to fp32, so the two gradients are of the same rows), plus the pose kernel's own backward: 6 products summed per
    entry and a Jacobian formed in fp32 from a dozen operations -- 32 u sum_i |g_i| |J_ij|."""
    from upnerf_amd import baked_pose
    from upnerf_amd.camera import refine_and_get_rays
    name = "blob"
    scene, numbers = scene_of(name, degree)
    dt = sh.steps(sh.GRIDS[name]()[0])["cell"]
    rng = np.random.RandomState(5)
    R = 65
    lo, hi = br.bounds64(br.BOUNDS)
    eye = np.concatenate([np.eye(3), ((lo + hi) / 2 + [0.0, 0.0, 1.6])[:, None]], 1)  # a camera above the box looking down -z
    c2w = np.broadcast_to(eye, (R, 3, 4)).astype(np.float32)
    se3 = (0.05 * rng.randn(R, 6)).astype(np.float32)
    dirs = np.stack([rng.uniform(-0.3, 0.3, R), rng.uniform(-0.3, 0.3, R), -np.ones(R)], 1).astype(np.float32)
    nf = np.broadcast_to(np.float32([0.2, 2.6]), (R, 2))
    g_rgb, g_depth, g_op = tr.upstream(R)
    s = dev(se3).requires_grad_(True)
    o, d = refine_and_get_rays(s, dev(c2w), dev(dirs))
    rays = torch.cat([o, d, dev(nf)], 1)
    out = baked_pose.render(scene, rays, dt)
    ((out["rgb"] * dev(g_rgb)).sum() + (out["depth"] * dev(g_depth)).sum() + (out["opacity"] * dev(g_op)).sum()).backward()
    got = s.grad.cpu().numpy().astype(np.float64)
    ref = pr.ray_grad(numbers, degree, br.BOUNDS, rays.detach().cpu().numpy(), dt, 0.0, 0.0, g_rgb, g_depth, g_op)
    J = pr.pose_rays(se3, c2w, dirs)[1]
    want = np.einsum("ni,nij->nj", ref["grad"][:, :6], J)
    gate = np.einsum("ni,nij->nj", ref["gate"][:, :6], np.abs(J)) + 32 * pr.U * np.einsum("ni,nij->nj", np.abs(ref["grad"][:, :6]), np.abs(J))
    err = np.abs(got - want)
    print(f"degree {degree}: largest se3 gradient {np.abs(want).max():.3e}, worst err / gate {float((err / np.maximum(gate, 1e-300))[gate > 0].max()):.3f}")
    assert np.abs(want).max() > 1e-2 and (err <= gate).all(), np.argwhere(err > gate)[:5]


def loc_batches(n):
    """The index draws of BakedLocaliser.step under localise's generator, restated: `LOC_ITERS` draws of `LOC_BATCH` from [0, n)."""
    gen = torch.Generator(device="cpu").manual_seed(pr.LOC_SEED)
    return [torch.randint(0, n, (pr.LOC_BATCH,), generator=gen).numpy() for _ in range(pr.LOC_ITERS)]


@pytest.mark.parametrize("degree", [0, 2])
def test_the_localiser_brings_perturbed_poses_back_towards_the_truth(degree):
    """The test that cannot pass without the ray gradient.  Two 24 x 16 photographs of the blob scene rendered by the marcher
    itself from the true poses; the poses start LOC_ROT = 0.05 rad and LOC_TRA = 0.05 off; 40 iterations of 64 pixels at
    lr = 0.004.  The fp64 loop of the restatement (pose_loop, the same index draws) must bring the rotation and the translation
    error to a quarter or less -- it brings them to 0.162 and 0.236 of their initial values at degree 0, to 0.175 and 0.166 at degree
    2 (loss 1.28e-3 -> 1.4e-5 and 9.0e-4 -> 7.0e-6) -- and the GPU's loop to a half or less: the factor of two is the room for the fp32 and
    fp64 Adam trajectories to part.  The first loss equals the reference's on the GPU's own fp32 rays within the forward's gates
    (baked_ref / baked_sh_ref) of the rendered and the target pixels, propagated through the squared error."""
    from upnerf_amd import baked_pose
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.camera import get_rays
    A, truth, init, step = pr.localisation_problem(degree)
    W, H = pr.LOC_WH
    n = 2 * H * W
    batches = loc_batches(n)
    key = ("loop", degree)
    if key not in _CACHE:
        targets64 = np.stack([tr.render64(A, degree, br.BOUNDS, pr.image_rays(c, pr.LOC_K, pr.LOC_WH, pr.LOC_NEAR_FAR), step)[0].reshape(H, W, 3)
                              for c in truth])
        _CACHE[key] = pr.pose_loop(A, degree, br.BOUNDS, targets64, pr.LOC_K, init, pr.LOC_NEAR_FAR, step, pr.LOC_ITERS, pr.LOC_LR, batches)
    se3_ref, curve = _CACHE[key]
    rot0, tra0 = pr.pose_error(init, truth)
    rot_ref, tra_ref = pr.pose_error(pr.refined(se3_ref, init), truth)
    assert rot_ref <= rot0 / 4 and tra_ref <= tra0 / 4, (rot_ref / rot0, tra_ref / tra0)

    level = tr.tuning_problem(degree)[2]
    if degree == 0:
        scene = BakedScene.from_grids(dev(A[..., 3]), dev(A[..., :3]), br.BOUNDS, level)
        records = None
    else:
        records = sh.pack(A[0], A[1], level, degree)[0]
        scene = BakedScene.from_records(dev(records), br.BOUNDS, level, degree)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    dirs = baked_pose.pixel_directions(xx.reshape(-1), yy.reshape(-1), pr.LOC_K)
    nf = torch.tensor(pr.LOC_NEAR_FAR, device="cuda").expand(H * W, 2)
    target_rays = torch.cat([torch.cat(get_rays(dirs, dev(c.astype(np.float32))) + (nf,), 1) for c in truth]).contiguous()
    targets = scene.render(target_rays, step)["rgb"].view(2, H, W, 3).contiguous()
    loc = baked_pose.BakedLocaliser(scene, targets, pr.LOC_K, dev(init.astype(np.float32)), pr.LOC_NEAR_FAR, lr=pr.LOC_LR)
    first_rays = loc.rays_of(dev(batches[0])).detach().cpu().numpy()
    gen = torch.Generator(device="cpu").manual_seed(pr.LOC_SEED)
    losses = torch.stack([loc.step(pr.LOC_BATCH, step, gen) for _ in range(pr.LOC_ITERS)]).cpu().numpy()
    rot, tra = pr.pose_error(loc.poses().cpu().numpy(), truth)
    # the first loss on the GPU's own rays, in fp64, and the forward's gates of both pictures
    render = (lambda r: br.render(A, br.BOUNDS, r, step)) if degree == 0 else (lambda r: sh.render(records, degree, br.BOUNDS, r, step))
    mine, theirs = render(first_rays), render(target_rays.cpu().numpy()[batches[0]])
    diff, e = mine["rgb"] - theirs["rgb"], mine["gate_rgb"] + theirs["gate_rgb"]
    L0 = float((diff * diff).mean())
    gate0 = float((2 * np.abs(diff) * e + e * e).mean()) + (diff.size + 3) * pr.U * L0
    print(f"degree {degree}: fp64 loop rotation {rot0:.4f} -> {rot_ref:.4f}, translation {tra0:.4f} -> {tra_ref:.4f}, loss {curve[0]:.3e} -> {curve[-1]:.3e}; "
          f"GPU rotation -> {rot:.4f}, translation -> {tra:.4f}, loss {losses[0]:.3e} -> {losses[-1]:.3e}; first loss off by {abs(losses[0] - L0):.2e}, gate {gate0:.2e}")
    assert abs(float(losses[0]) - L0) <= gate0
    assert rot <= rot0 / 2 and tra <= tra0 / 2
