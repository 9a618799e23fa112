"""The baked scene with spherical-harmonic colour on the GPU (csrc/baked.hip: upnerf_baked_sh_render, upnerf_sh_accumulate,
upnerf_baked_sh_pack; upnerf_amd/baked.py; the `baked` keyword of render_path).

Reference: tests/baked_sh_ref.py -- fp64 numpy over the STORED records (their halves converted exactly), brute force over every
lattice sample, never a look at the occupancy bits.  Its docstring derives the per-ray gates; nothing here is a hand-picked
constant.  Worst measured error / gate on an MI355X: see DESIGN.md 2.32.  Everything else is bit for bit (`torch.equal`).

Grids and rays are baked_ref's (11 x 10 x 9 points with 720 cell bits and unevenly cut bricks; 17^3 points with six empty bricks;
67 = 64 + 3 rays with the axis-parallel, inside-start, miss, |d| = 2.5, NaN and far <= near cases), with random coefficients at
the kept points (baked_sh_ref.sh_grid; tests/test_baked_sh_cpu.py holds them to clamping on both sides)."""
import numpy as np
import pytest
import torch

import baked_cases as cases
import baked_ref as br
import baked_sh_ref as sh
from baked_cases import dev

pytestmark = pytest.mark.gpu

_CACHE = {}
U = sh.U


def scene_of(name, degree):
    """(BakedScene, records) of a test grid, built once."""
    records, level = sh.sh_grid(name, degree)
    return cases.scene_of((__name__, name, degree), lambda: cases.build(records, level, degree)), records


def reference(name, degree, step, background):
    """The fp64 restatement, computed once per case and never changed."""
    key = (name, degree, step, background)
    if key not in _CACHE:
        _CACHE[key] = sh.render(sh.sh_grid(name, degree)[0], degree, br.BOUNDS, br.make_rays(), step, background)
    return _CACHE[key]


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("rgb", "depth", "opacity"))


def within_gates(out, ref, rows=slice(None)):
    """{name: worst error / gate} of a render against the restatement; asserts every ray within its gate."""
    ratio = {}
    for k in ("rgb", "depth", "opacity"):
        got = out[k].cpu().numpy().astype(np.float64)
        err, gate = np.abs(got - ref[k][rows]), ref[f"gate_{k}"][rows]
        assert np.isfinite(got).all()
        ratio[k] = float((err / np.maximum(gate, 1e-300)).max())
        assert (err <= gate).all(), (k, np.argwhere(err > gate)[:5], err.max())
    return ratio


# ---- projection and packing ----------------------------------------------------------------------------------------------------------

def accumulate(rgb_dirs, dirs, degree):
    """[..., 3, nb] fp32: upnerf_sh_accumulate over the K directions in order, as BakedScene._project calls it."""
    import ctypes as C
    from upnerf_amd import _lib, baked
    W = baked.sh_weights(dirs, degree)
    nb, K = W.shape
    n = rgb_dirs[0].numel() // 3
    acc = torch.full(tuple(rgb_dirs.shape[1:-1]) + (3, nb), float("nan"), device="cuda")  # (the first call writes: nothing of this is read)
    for k in range(K):
        a = _lib.ShAccumulateArgs(n=n, nb=nb, first=int(k == 0), w=(C.c_float * 9)(*W[:, k].tolist()), rgb=_lib.ptr(rgb_dirs[k]), acc=_lib.ptr(acc))
        _lib.check(_lib.lib.upnerf_sh_accumulate(C.byref(a), _lib.stream()), "upnerf_sh_accumulate")
    return acc


@pytest.mark.parametrize("degree", [1, 2])
def test_accumulate_projects_and_pack_rounds_and_prunes_as_the_reference(degree):
    import ctypes as C
    from upnerf_amd import _lib
    from upnerf_amd.baked import BakedScene
    nb, size = sh.NB[degree], sh.RECORD[degree]
    rng = np.random.RandomState(5)
    shape = (6, 7, 9)  # 378 points: one block of 256 and a ragged one
    dirs = sh.sphere_directions(48)
    coef = rng.randn(*shape, 3, nb)
    coef[..., 0] += 0.5 / sh.Y0
    rgb_dirs = (np.einsum("kj,...cj->k...c", sh.basis(dirs, degree), coef) + rng.randn(48, *shape, 3) * 0.05).astype(np.float32)
    acc = accumulate(dev(rgb_dirs), dirs, degree)
    want, cond = sh.project(rgb_dirs, dirs, degree)
    err = np.abs(acc.cpu().numpy().astype(np.float64) - want)
    gate = (48 + 1) * U * cond
    print(f"degree {degree}: accumulate over 48 directions, worst err / gate {(err / gate).max():.3f}, |coefficient| up to {np.abs(want).max():.2f}")
    assert (err <= gate).all() and np.abs(want - coef).max() < 0.2
    # packing, bit for bit, of the kernel's own sums with planted cases: NaN, negative and infinite sigma, a sigma AT the level,
    # an infinite and a NaN coefficient, coefficients beyond the range of fp16
    sums = acc.clone()
    sigma = rng.uniform(-0.5, 3.0, shape).astype(np.float32)
    sigma.reshape(-1)[[3, 50, 200, 7]] = [np.nan, np.inf, -np.inf, 1.25]
    sigma.reshape(-1)[[100, 101, 102, 103]] = 2.0
    flat = sums.view(-1, 3 * nb)
    flat[100, 1], flat[101, 3 * nb - 1], flat[102, 0], flat[103, 2] = float("inf"), float("nan"), 1e6, -65519.9
    records = torch.full((378 * size + size,), 255, dtype=torch.uint8, device="cuda")
    off = -records.data_ptr() % size
    rec = records[off:off + 378 * size].view(*shape, size)
    kept = torch.full(shape, 7, dtype=torch.uint8, device="cuda")
    a = _lib.BakedShPackArgs(n=378, level=1.25, degree=degree, sigma=_lib.ptr(dev(sigma)), acc=_lib.ptr(sums), records=_lib.ptr(rec), kept=_lib.ptr(kept))
    _lib.check(_lib.lib.upnerf_baked_sh_pack(C.byref(a), _lib.stream()), "upnerf_baked_sh_pack")
    want_rec, want_kept = sh.pack(sums.cpu().numpy(), sigma, 1.25, degree)
    rule = br.prune(sigma, None, 1.25)[..., 3] > 0
    rule.reshape(-1)[[100, 101]] = False
    assert np.array_equal(want_kept, rule) and want_kept.reshape(-1)[7] and want_kept.reshape(-1)[[102, 103]].all() and 0.2 < rule.mean() < 0.8
    assert torch.equal(rec, dev(want_rec)) and torch.equal(kept, dev(want_kept.astype(np.uint8)))
    k, _ = sh.unpack(want_rec, degree)
    assert k.reshape(-1, 3 * nb)[102, 0] == 65504.0 and k.reshape(-1, 3 * nb)[103, 2] == -65504.0
    assert int(records[off + 378 * size:].min()) == 255 and int(records[:off].min() if off else 255) == 255  # nothing beyond the records
    # the same through the Python surface: from_direction_grids is accumulate, pack and the bits of the kept sigmas
    scene = BakedScene.from_direction_grids(dev(sigma), dev(rgb_dirs), dirs, br.BOUNDS, 1.25, degree)
    plain, plain_kept = sh.pack(acc.cpu().numpy(), sigma, 1.25, degree)
    assert scene.sh_degree == degree and scene.rgbs is None and torch.equal(scene.records, dev(plain))
    assert scene.records.data_ptr() % size == 0
    cells = br.occupied_cells(np.where(plain_kept, sigma, 0)[..., None].repeat(4, -1))
    assert torch.equal(scene.occupancy.cells(), dev(cells))
    assert scene.resolution == (9, 7, 6) and scene.nbytes == 378 * size + scene.occupancy.words.numel() * 4
    assert abs(scene.fraction - cells.mean()) < 1e-6
    with pytest.raises(ValueError):
        BakedScene.from_direction_grids(dev(sigma), dev(rgb_dirs[:40]), dirs, br.BOUNDS, 1.25, degree)
    with pytest.raises(ValueError):
        BakedScene.from_direction_grids(dev(sigma), dev(rgb_dirs), dirs, br.BOUNDS, float("nan"), degree)
    with pytest.raises(ValueError):
        BakedScene.from_direction_grids(dev(sigma), dev(rgb_dirs[:3]), dirs[:3], br.BOUNDS, 1.25, degree)


# ---- the render ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("background", [0.0, 1.0])
@pytest.mark.parametrize("step", ["cell", "tenth"])
@pytest.mark.parametrize("name", list(sh.GRIDS))
@pytest.mark.parametrize("degree", [1, 2])
def test_render_matches_the_fp64_restatement_ray_by_ray(degree, name, step, background):
    scene, records = scene_of(name, degree)
    dt = sh.steps(records)[step]
    rays = br.make_rays()
    out = scene.render(dev(rays), dt, background=background)
    ref = reference(name, degree, dt, background)
    ratio = within_gates(out, ref)
    hit = ref["n"] > 0
    print(f"degree {degree} {name} {step} (dt {dt:.5f}) background {background}: samples per ray up to {ref['inside'].max()}, contributing up "
          f"to {ref['n'].max()}, hit {hit.sum()} of 67, opacity up to {ref['opacity'].max():.4f}; worst err / gate rgb {ratio['rgb']:.3f} "
          f"depth {ratio['depth']:.3f} opacity {ratio['opacity']:.3f}; median rgb gate of the hits {np.median(ref['gate_rgb'][hit]):.2e}")
    assert hit.sum() >= 20 and ref["opacity"].max() > 0.8
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for r in (2, 5, 6):  # misses the box, a NaN, far <= near: the background at far, bit for bit
        assert (got["rgb"][r] == background).all() and got["opacity"][r] == 0 and got["depth"][r] == rays[r, 7]


@pytest.mark.parametrize("step", ["cell", "tenth"])
@pytest.mark.parametrize("name", list(sh.GRIDS))
@pytest.mark.parametrize("degree", [1, 2])
def test_skipping_is_exact_and_the_bits_do_not_depend_on_run_or_launch(degree, name, step):
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.occupancy import OccupancyGrid
    scene, records = scene_of(name, degree)
    dt = sh.steps(records)[step]
    rays = dev(br.make_rays())
    out = scene.render(rays, dt, background=0.5)
    full = BakedScene.from_records(scene.records, br.BOUNDS, scene.level, degree)
    cells = scene.occupancy.cells()
    assert 0 < float(cells.float().mean()) < 1
    assert int(scene.occupancy.bricks().sum()) == (2 if name == "corners" else 4)
    full.occupancy = OccupancyGrid.from_cells(torch.ones_like(cells), br.BOUNDS)  # every bit set: every sample in the box is visited
    assert full.occupancy.fraction == 1.0
    assert same(full.render(rays, dt, background=0.5), out)
    assert same(scene.render(rays, dt, background=0.5), out)  # a second run
    a, b = scene.render(rays[:33], dt, background=0.5), scene.render(rays[33:], dt, background=0.5)  # a launch cut at ray 33
    assert same({k: torch.cat([a[k], b[k]]) for k in a}, out)
    ws = {"rgb": torch.full((80, 3), -1.0).cuda(), "depth": torch.full((80,), -1.0).cuda(), "opacity": torch.full((80,), -1.0).cuda()}
    assert same(scene.render(rays, dt, background=0.5, out=ws), out) and float(ws["rgb"][67:].max()) == -1.0


# ---- what a scene without view dependence cannot show -----------------------------------------------------------------------------------

def test_a_ray_against_the_baked_direction_needs_the_expansion():
    """A volume whose colour over direction IS a degree-2 expansion, baked with sh_degree = 2 and, for view_dir = +x, without;
    one ray along +x and one along -x through the same samples.  The SH scene follows the direction-dependent definition on both
    rays; the degree-0 scene shows the -x ray the colours of +x."""
    from upnerf_amd.baked import BakedScene
    rgbs, level = br.blob_grid()
    sigma = rgbs[..., 3]
    rng = np.random.RandomState(21)
    coef = rng.randn(*sigma.shape, 3, 9) * 0.1  # colour 0.5 +- 0.1 or so over direction: inside [0, 1], nothing clamps
    coef[..., 0] += 0.5 / sh.Y0
    dirs = sh.sphere_directions(48)
    rgb_dirs = np.einsum("kj,...cj->k...c", sh.basis(dirs, 2), coef).astype(np.float32)
    assert 0 < rgb_dirs.min() and rgb_dirs.max() < 1
    plus_x = np.einsum("j,...cj->...c", sh.basis([[1.0, 0, 0]], 2)[0], coef).astype(np.float32)
    scene2 = BakedScene.from_direction_grids(dev(sigma), dev(rgb_dirs), dirs, br.BOUNDS, level, 2)
    scene0 = BakedScene.from_grids(dev(sigma), dev(plus_x), br.BOUNDS, level)
    assert torch.equal(scene2.occupancy.words, scene0.occupancy.words)
    lo, hi = br.bounds64(br.BOUNDS)
    mid = (lo + hi) / 2
    dt = float(np.float32(0.0625))
    far = 2.5  # 40 steps exactly: the two rays share their 40 sample points
    o = np.array([lo[0] - 0.5, mid[1] + 0.013, mid[2] - 0.021])
    rays = np.array([list(o) + [1, 0, 0, 0, far], list(o + [far, 0, 0]) + [-1, 0, 0, 0, far]], np.float32)
    ref = sh.render(scene2.records.cpu().numpy(), 2, br.BOUNDS, rays, dt)
    assert (ref["n"] >= 8).all() and (ref["opacity"] > 0.5).all() and ref["clamp"][:, :2].sum() == 0
    ratio = within_gates(scene2.render(dev(rays), dt), ref)
    flat = scene0.render(dev(rays), dt)["rgb"].cpu().numpy().astype(np.float64)
    off = np.abs(flat - ref["rgb"]) / ref["gate_rgb"]
    print(f"+x and -x through the same samples: SH err / gate rgb {ratio['rgb']:.3f}; the scene baked for +x is off by {off[0].max():.0f} gates "
          f"on +x (fp16 coefficients, the fit) and by {off[1].max():.0f} on -x (rgb {flat[1]} against {ref['rgb'][1]})")
    assert off[1].max() > 100
    # on the direction it was baked for it agrees to what the fp16 coefficients (2^-11 relative each), the fp32 fit (49 u) and
    # the rounding of the +x colours to fp32 (u) leave of sum_j |Y_j k_j|, beside the two renders' own gates
    size = float((np.abs(coef) * np.abs(sh.basis([[1.0, 0, 0]], 2)[0])).sum(-1).max())
    assert (np.abs(flat[0] - ref["rgb"][0]) <= size * (2.0 ** -11 + 50 * U) + 2 * ref["gate_rgb"][0]).all()


# ---- the bake of a field, render_path, save and load -------------------------------------------------------------------------------------

BOX = ((-0.7, -0.5, -0.6), (0.8, 0.6, 0.9))
RES = (7, 6, 9)  # (Nx, Ny, Nz): 42 columns; the field kernels are not under test here
IMG = 4


@pytest.fixture(scope="module")
def system():
    return cases.make_system()


def test_build_is_from_direction_grids_on_the_fields_own_grids(system):
    from upnerf_amd.baked import BakedScene, field_colour, sphere_directions
    from upnerf_amd.geometry import density_grid
    dirs = sphere_directions(8)
    sigma = density_grid(system, BOX, RES)
    level = float(sigma.median())
    scene = BakedScene.build(system, BOX, RES, level, img_id=IMG, sh_degree=1, dirs=dirs)
    rgb_dirs = torch.stack([field_colour(system, BOX, RES, d, img_id=IMG) for d in dirs])
    want = BakedScene.from_direction_grids(sigma, rgb_dirs, dirs, BOX, level, 1)
    assert scene.sh_degree == 1 and tuple(scene.records.shape) == (9, 6, 7, 32) and scene.resolution == RES
    assert torch.equal(scene.records, want.records) and torch.equal(scene.occupancy.words, want.occupancy.words)
    k, s = sh.unpack(scene.records.cpu().numpy(), 1)
    keep = (sigma >= level).cpu().numpy()
    assert 0.3 < keep.mean() < 0.7 and np.array_equal(s, np.where(keep, sigma.cpu().numpy(), 0).astype(np.float64))
    assert np.abs(k[keep][:, :, 1:]).max() > 1e-3  # the colour head does depend on the direction
    with pytest.raises(ValueError):
        BakedScene.build(system, BOX, RES, level, img_id=IMG, sh_degree=1, view_dir=(0, 0, 1))
    with pytest.raises(ValueError):
        BakedScene.build(system, BOX, RES, level, img_id=IMG, dirs=dirs)
    with pytest.raises(ValueError):
        BakedScene.build(system, BOX, RES, level, img_id=IMG, sh_degree=2, dirs=dirs)  # 8 directions, 9 coefficients


SCENE = ((-0.9, -0.8, -4.0), (0.7, 0.9, -1.5))  # the box of test_hip_baked.py's path test, in front of its cameras


def test_render_path_save_and_load_give_scene_render_on_the_path_rays(system, tmp_path):
    from upnerf_amd import novel_view as nv
    from upnerf_amd.baked import BakedScene
    records, level = sh.sh_grid("blob", 2)
    k, sigma = sh.unpack(records, 2)
    scaled, _ = sh.pack(k.astype(np.float32), (sigma * 0.1).astype(np.float32), level * 0.1, 2)  # (the box is deeper: a thinner density)
    scene = BakedScene.from_records(dev(scaled), SCENE, level * 0.1, 2)
    c = np.cos(0.3), np.sin(0.3)
    c2w = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 0.2]], [[c[0], 0, c[1], -0.2], [0, 1, 0, 0.1], [-c[1], 0, c[0], 0.0]]])
    K = torch.tensor([[22.0, 0, 11.6], [0, 21.0, 7.8], [0, 0, 1]])
    path = nv.CameraPath.from_poses(c2w, [(0.1, 5.0), (0.2, 4.5)], 2, appearance=(1, 4), img_wh=(24, 16), K=K)
    dt = 0.04
    out = nv.render_path(system, path, chunk=100, outputs=("rgb_float", "depth"), depth_range=(0.1, 5.0), baked=scene, baked_step=dt)
    file = str(tmp_path / "scene.npz")
    scene.save(file)
    back = BakedScene.load(file, "cuda")
    assert back.sh_degree == 2 and back.rgbs is None and torch.equal(back.records, scene.records)
    assert torch.equal(back.occupancy.words, scene.occupancy.words) and back.bounds == scene.bounds and back.level == scene.level
    again = nv.render_path(system, path, outputs=("rgb_float", "depth"), depth_range=(0.1, 5.0), baked=back, baked_step=dt)
    poses, nf = nv.path_poses(path.key_c2w.cuda(), path.key_near_far.cuda(), path.u.cuda(), path.mode)
    for f in range(2):
        rays, _ = nv.path_rays(poses, nf, path.img_wh, path.K, f * 384, 384)
        direct = scene.render(rays, dt, background=0.0)
        assert int((direct["opacity"] > 0.05).sum()) > 20 and int((direct["opacity"] == 0).sum()) > 20
        assert torch.equal(out["rgb_float"][f], direct["rgb"]), f
    assert torch.equal(again["rgb_float"], out["rgb_float"]) and torch.equal(again["depth"], out["depth"])
