"""The baked scene on the GPU (csrc/baked.hip, upnerf_amd/baked.py, the `baked` keyword of render_path).

Reference: tests/baked_ref.py -- fp64 numpy, brute force over every lattice sample, never a look at the occupancy bits.  Its
docstring derives the per-ray gates from the reference's own condition sums; nothing here is a hand-picked constant.  Worst
measured error / gate on an MI355X: see DESIGN.md 2.31.  Everything else is bit for bit (`torch.equal`).

Grids: 9 x 10 x 11 points (8 x 9 x 10 cells: bricks cut elsewhere on every axis, 720 bits) and 17^3 points with density in two
opposite corner bricks, both zero on their outermost layer (a density on the boundary is a hard edge on whose side fp32 and
fp64 may disagree).  67 rays (baked_ref.make_rays), at a step of three cells and at one of a thirtieth of a cell."""
import os
import sys

import numpy as np
import pytest
import torch

import baked_cases as cases
import baked_ref as br
from baked_cases import dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))

GRIDS = {"blob": br.blob_grid, "corners": br.corner_grid}
_CACHE = {}


def steps(rgbs):
    cell = br.cell_size(rgbs)
    return {"coarse": float(np.float32(3 * cell)), "fine": float(np.float32(cell / 30))}


def scene_of(name):
    """(BakedScene, rgbs) of a test grid, built once (from_grids prunes again what the reference pruned: the same grid)."""
    rgbs, level = GRIDS[name]()
    return cases.scene_of((__name__, name), lambda: cases.build(rgbs, level)), rgbs


def reference(name, step, background):
    """The fp64 restatement, computed once per case and never changed."""
    key = (name, step, background)
    if key not in _CACHE:
        _CACHE[key] = br.render(GRIDS[name]()[0], br.BOUNDS, br.make_rays(), step, background)
    return _CACHE[key]


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("rgb", "depth", "opacity"))


def test_from_grids_prunes_as_the_reference_and_packs_the_kept_sigmas():
    from upnerf_amd.baked import BakedScene
    rng = np.random.RandomState(1)
    sigma = rng.uniform(-0.5, 3.0, (6, 7, 9)).astype(np.float32)
    sigma.reshape(-1)[[3, 50, 200]] = [np.nan, np.inf, -np.inf]
    sigma.reshape(-1)[7] = 1.25  # a sample AT the level is kept
    rgb = rng.uniform(0, 1, (6, 7, 9, 3)).astype(np.float32)
    scene = BakedScene.from_grids(dev(sigma), dev(rgb), br.BOUNDS, 1.25)
    want = br.prune(sigma, rgb, 1.25)
    assert want[..., 3].reshape(-1)[7] == 1.25 and 0.2 < (want[..., 3] > 0).mean() < 0.8
    assert torch.equal(scene.rgbs, dev(want))
    assert torch.equal(scene.occupancy.cells(), dev(br.occupied_cells(want)))
    assert scene.resolution == (9, 7, 6) and scene.nbytes == want.size * 4 + scene.occupancy.words.numel() * 4
    assert abs(scene.fraction - br.occupied_cells(want).mean()) < 1e-6
    black = BakedScene.from_grids(dev(sigma), None, br.BOUNDS, 1.25)
    assert torch.equal(black.rgbs[..., 3], scene.rgbs[..., 3]) and float(black.rgbs[..., :3].abs().max()) == 0
    kept_all = BakedScene.from_grids(dev(np.abs(np.nan_to_num(sigma, posinf=1.0, neginf=1.0)) + 0.1), dev(rgb), br.BOUNDS)  # level 0
    assert kept_all.fraction == 1.0
    with pytest.raises(ValueError):
        BakedScene.from_grids(dev(sigma), dev(rgb[..., :2]), br.BOUNDS, 1.0)
    with pytest.raises(ValueError):
        BakedScene.from_grids(dev(sigma), dev(rgb), br.BOUNDS, float("nan"))
    with pytest.raises(ValueError):
        BakedScene.from_grids(dev(sigma[:1]), None, br.BOUNDS, 1.0)  # an axis without a cell


@pytest.mark.parametrize("background", [0.0, 1.0])
@pytest.mark.parametrize("step", ["coarse", "fine"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_render_matches_the_fp64_restatement_ray_by_ray(name, step, background):
    scene, rgbs = scene_of(name)
    dt = steps(rgbs)[step]
    rays = br.make_rays()
    out = {k: v.cpu().numpy().astype(np.float64) for k, v in scene.render(dev(rays), dt, background=background).items()}
    ref = reference(name, dt, background)
    ratio = {}
    for k in ("rgb", "depth", "opacity"):
        err, gate = np.abs(out[k] - ref[k]), ref[f"gate_{k}"]
        ok = np.isfinite(ref[k]).all(-1) if k == "rgb" else np.isfinite(ref[k])  # (the ray with a NaN has far = a number: all finite)
        assert ok.all()
        ratio[k] = float((err / np.maximum(gate, 1e-300)).max())
        assert (err <= gate).all(), (k, np.argwhere(err > gate)[:5], err.max())
    hit = ref["n"] > 0
    print(f"{name} {step} (dt {dt:.5f}) background {background}: samples per ray up to {ref['inside'].max()}, contributing up to "
          f"{ref['n'].max()}, hit {hit.sum()} of 67, opacity up to {ref['opacity'].max():.4f}; worst err / gate rgb {ratio['rgb']:.3f} "
          f"depth {ratio['depth']:.3f} opacity {ratio['opacity']:.3f}; median rgb gate of the hits {np.median(ref['gate_rgb'][hit]):.2e}")
    assert hit.sum() >= 20 and ref["opacity"].max() > 0.8
    if step == "fine":
        assert ref["inside"].max() >= 300
    for r in (2, 5, 6):  # misses the box, a NaN, far <= near: the background at far, bit for bit
        assert (out["rgb"][r] == background).all() and out["opacity"][r] == 0
        assert out["depth"][r] == rays[r, 7]


@pytest.mark.parametrize("step", ["coarse", "fine"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_skipping_is_exact_and_the_bits_do_not_depend_on_run_or_launch(name, step):
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.occupancy import OccupancyGrid
    scene, rgbs = scene_of(name)
    dt = steps(rgbs)[step]
    rays = dev(br.make_rays())
    out = scene.render(rays, dt, background=0.5)
    # every occupancy bit set: the marcher visits every sample inside the box
    full = BakedScene(scene.rgbs, br.BOUNDS, scene.level)
    cells = scene.occupancy.cells()
    assert 0 < float(cells.float().mean()) < 1  # empty cells in both grids; whole empty bricks in the second
    assert int(scene.occupancy.bricks().sum()) == (2 if name == "corners" else 4)
    full.occupancy = OccupancyGrid.from_cells(torch.ones_like(cells), br.BOUNDS)
    assert full.occupancy.fraction == 1.0
    assert same(full.render(rays, dt, background=0.5), out)
    assert same(scene.render(rays, dt, background=0.5), out)  # a second run
    a, b = scene.render(rays[:64], dt, background=0.5), scene.render(rays[64:], dt, background=0.5)  # 64 + 3
    assert same({k: torch.cat([a[k], b[k]]) for k in a}, out)
    # preallocated outputs with rows to spare, and a buffer of rays that is not 16-byte aligned
    ws = {"rgb": torch.full((80, 3), -1.0).cuda(), "depth": torch.full((80,), -1.0).cuda(), "opacity": torch.full((80,), -1.0).cuda()}
    assert same(scene.render(rays, dt, background=0.5, out=ws), out) and float(ws["rgb"][67:].max()) == -1.0
    odd = torch.zeros(67 * 8 + 1, device="cuda")
    odd[1:] = rays.reshape(-1)
    assert same(scene.render(odd[1:].view(67, 8), dt, background=0.5), out)


@pytest.mark.parametrize("step", ["coarse", "fine"])
def test_stop_ends_a_ray_within_its_bound(step):
    scene, rgbs = scene_of("blob")
    dt = steps(rgbs)[step]
    rays = br.make_rays()
    bg = 0.5
    full = {k: v.cpu().numpy() for k, v in scene.render(dev(rays), dt, background=bg).items()}
    cut = {k: v.cpu().numpy() for k, v in scene.render(dev(rays), dt, background=bg, stop=1e-3).items()}
    cmax = float(rgbs[..., :3].max())
    ok = np.isfinite(rays).all(1)
    d_rgb = np.abs(cut["rgb"] - full["rgb"])[ok].max()
    d_depth = (np.abs(cut["depth"] - full["depth"]) / np.abs(rays[:, 7]))[ok].max()
    ended = int((full["opacity"] > 1 - 1e-3).sum())
    print(f"stop = 1e-3 at the {step} step: {ended} rays end early; rgb moves by {d_rgb:.2e} (bound {1e-3 * (cmax + bg):.2e}), "
          f"depth by {d_depth:.2e} of far (bound 1e-3)")
    assert ended >= 3 and d_rgb > 0  # some rays do end inside the volume
    assert d_rgb <= 1e-3 * (cmax + bg) and d_depth <= 1e-3


# ---- the bake of a field ------------------------------------------------------------------------------------------------------------

BOX = ((-0.7, -0.5, -0.6), (0.8, 0.6, 0.9))
RES = (7, 6, 9)  # (Nx, Ny, Nz): 42 columns of 9 points, padded to the field kernels' 32 samples
IMG = 4


@pytest.fixture(scope="module")
def system():
    return cases.make_system()


def oracle_rgb(system, view_dir, img_id):
    """[Nz, Ny, Nx, 3] fp64 static colour of the oracle's fine field at the fp32 grid points, for one direction and one row."""
    import upnerf_oracle as orc
    Nx, Ny, Nz = RES
    model = system.models["nerf_fine"]
    p = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    hp = system.hparams
    cfg = orc.NerfCfg(typ="fine", D=8, W=256, xyz_L=hp["nerf.N_emb_xyz"], dir_L=hp["nerf.N_emb_dir"], c2f=hp["pose.c2f"])
    axis = lambda lo, hi, n: (float(np.float32(lo)) + np.arange(n, dtype=np.float64) * ((float(np.float32(hi)) - float(np.float32(lo))) / (n - 1))).astype(np.float32)
    x, y, z = (axis(BOX[0][k], BOX[1][k], n) for k, n in enumerate(RES))
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    xyz = torch.from_numpy(np.stack([X, Y, Z], -1).reshape(-1, 3)).double()
    M = xyz.shape[0]
    v = torch.as_tensor(view_dir).detach().cpu().float().double().expand(M, 3)
    a = system.embeddings["fine_a"].weight.detach().cpu()[img_id].double().expand(M, -1)
    with torch.no_grad():
        out = orc.nerf_field(p, cfg, xyz, v, a, None, 1.0, float(np.float32(0.8)))
    return out["s_rgb"].reshape(Nz, Ny, Nx, 3).numpy()


def test_build_bakes_the_density_grid_and_the_oracles_colour(system):
    from upnerf_amd.baked import BakedScene, mean_optical_axis
    from upnerf_amd.geometry import density_grid
    sigma = density_grid(system, BOX, RES)
    level = float(sigma.median())
    scene = BakedScene.build(system, BOX, RES, level, img_id=IMG, chunk=5)  # 42 columns in chunks of 5: the last one is shorter
    keep = sigma >= level
    assert 0.3 < float(keep.float().mean()) < 0.7
    assert torch.equal(scene.rgbs[..., 3], torch.where(keep, sigma, torch.zeros_like(sigma)))  # bit for bit
    assert float(scene.rgbs[~keep].abs().max()) == 0.0  # pruned points are exact zeros
    view = mean_optical_axis(system)
    assert abs(float(view.norm()) - 1) < 1e-6
    ref = oracle_rgb(system, view, IMG)
    got = scene.rgbs[..., :3].cpu().numpy().astype(np.float64)
    k = keep.cpu().numpy()
    err = np.abs(got - ref)[k]
    worst = float((err / np.maximum(1e-4 * np.abs(ref[k]), 1e-6)).max())
    print(f"bake {RES}: {int(k.sum())} of {k.size} points kept at level {level:.4f}; colour in [{ref[k].min():.3f}, {ref[k].max():.3f}], "
          f"max abs err {err.max():.2e}, worst err / gate {worst:.3f}")
    assert ref[k].max() - ref[k].min() > 0.05  # a colour field with some range
    assert worst <= 1.0
    for chunk in (1, 42, None):
        assert torch.equal(BakedScene.build(system, BOX, RES, level, img_id=IMG, chunk=chunk).rgbs, scene.rgbs), chunk
    # another photograph's appearance, another direction, an explicit row
    assert not torch.equal(BakedScene.build(system, BOX, RES, level, img_id=1).rgbs, scene.rgbs)
    other = BakedScene.build(system, BOX, RES, level, img_id=IMG, view_dir=(0.0, 1.0, 0.0))
    assert not torch.equal(other.rgbs[..., :3], scene.rgbs[..., :3]) and torch.equal(other.rgbs[..., 3], scene.rgbs[..., 3])
    row = system.embeddings["fine_a"].weight.detach()[IMG]
    assert torch.equal(BakedScene.build(system, BOX, RES, level, rows=row, view_dir=view * 2.0).rgbs, scene.rgbs)  # (normalised)
    with pytest.raises(ValueError):
        BakedScene.build(system, BOX, RES, level)  # neither img_id nor rows
    with pytest.raises(ValueError):
        BakedScene.build(system, BOX, RES, level, img_id=6)
    with pytest.raises(ValueError):
        BakedScene.build(system, BOX, (7, 1, 9), level, img_id=IMG)


def test_save_and_load_give_the_same_scene(tmp_path):
    from upnerf_amd.baked import BakedScene
    scene, rgbs = scene_of("blob")
    path = str(tmp_path / "scene.npz")
    scene.save(path)
    back = BakedScene.load(path, "cuda")
    assert torch.equal(back.rgbs, scene.rgbs) and torch.equal(back.occupancy.words, scene.occupancy.words)
    assert back.bounds == scene.bounds and back.level == scene.level
    rays = dev(br.make_rays())
    assert same(back.render(rays, 0.05), scene.render(rays, 0.05))


SCENE = ((-0.9, -0.8, -4.0), (0.7, 0.9, -1.5))  # a box in front of the cameras of the path below (they look down -z), smaller than their view


def test_render_path_with_a_baked_scene_is_scene_render_on_the_path_rays(system):
    from upnerf_amd import novel_view as nv
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.occupancy import OccupancyGrid
    from upnerf_amd.visualization import depth_image, rgb_image
    rgbs, level = br.blob_grid()
    scene = BakedScene.from_grids(dev(rgbs[..., 3] * 0.1), dev(rgbs[..., :3]), SCENE, level * 0.1)
    c = np.cos(0.3), np.sin(0.3)
    c2w = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 0.2]], [[c[0], 0, c[1], -0.2], [0, 1, 0, 0.1], [-c[1], 0, c[0], 0.0]]])
    K = torch.tensor([[22.0, 0, 11.6], [0, 21.0, 7.8], [0, 0, 1]])
    path = nv.CameraPath.from_poses(c2w, [(0.1, 5.0), (0.2, 4.5)], 2, appearance=(1, 4), img_wh=(24, 16), K=K)
    dt = 0.04
    out = nv.render_path(system, path, chunk=100, outputs=("rgb_float", "rgb", "depth"), depth_range=(0.1, 5.0), baked=scene,
                         baked_step=dt)  # 768 rays in chunks of 100: they straddle the frames
    assert tuple(out["rgb"].shape) == (2, 16, 24, 3) and tuple(out["depth"].shape) == (2, 16, 24, 3)
    poses, nf = nv.path_poses(path.key_c2w.cuda(), path.key_near_far.cuda(), path.u.cuda(), path.mode)
    for f in range(2):
        rays, _ = nv.path_rays(poses, nf, path.img_wh, path.K, f * 384, 384)
        direct = scene.render(rays, dt, background=0.0)
        assert int((direct["opacity"] > 0.05).sum()) > 20 and int((direct["opacity"] == 0).sum()) > 20  # the volume and the background
        assert torch.equal(out["rgb_float"][f], direct["rgb"]), f
        assert torch.equal(out["rgb"][f], rgb_image(direct["rgb"], (24, 16)))
        assert torch.equal(out["depth"][f], depth_image(direct["depth"], (24, 16), min_max=(0.1, 5.0)))
    whole = nv.render_path(system, path, outputs=("rgb_float",), baked=scene, baked_step=dt)  # one chunk
    assert torch.equal(whole["rgb_float"], out["rgb_float"])
    occ = OccupancyGrid.from_cells(torch.ones(4, 4, 4, dtype=torch.bool).cuda(), SCENE)
    with pytest.raises(ValueError):
        nv.render_path(system, path, baked=scene, baked_step=dt, occupancy=occ)
    with pytest.raises(ValueError):
        nv.render_path(system, path, outputs=("normal",), baked=scene, baked_step=dt)
    with pytest.raises(ValueError):
        nv.render_path(system, path, baked=scene)  # no step
    with pytest.raises(ValueError):
        nv.render_path(system, path, baked_step=dt)  # a step without a scene
